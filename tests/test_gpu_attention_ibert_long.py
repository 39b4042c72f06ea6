"""Fused I-BERT attention on long rows (ivit_attention_fused_i8_ibert_long, 208 .. 1025 tokens) against its specification in numpy
(tests/ibert_long_ref.py), crafted rows on which the order of the float32 row sum decides output bytes, its argument errors, and
I-BERT / I-ViT models of 577 and 785 tokens through the module path: one fused attention launch per block, logits bit for bit
those of the literal path."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402
import ibert_long_ref as R  # noqa: E402
import attention_ref as A  # noqa: E402
from attention_ref import DEV, release, st  # noqa: E402,F401  (release: the autouse fixture)

NAME = "ivit_attention_fused_i8_ibert_long"


def _run(qkv, ms, es, mo, eo, tab, band, blocks):
    return A.run_ibert(NAME, qkv, ms, es, mo, eo, tab, band, blocks)


# (B, H, T, score multiplier, band form, block-layout output).  s_mult 1: Ms a power of two (float32 requantisation of the scores),
# otherwise float64.  T >> 4 <= 40: the 1024-thread form, above: the 768-thread one.  T < 512, < 1024, >= 1024: no / one / two full
# groups in the cascade of the row sum; 209, 577, 785, 1025: T % 8 != 0 (a scalar tail); 208, 256, 656, 1024: T % 16 == 0; 208, 209,
# 577, 655, 656, 785, 1000: (T >> 3) % 4 != 0 (vectors behind the interleaved part).  25 x 12 heads at 209, 17 x 12 at 577 and 11 x 12
# at 785 tokens: one workgroup per head; the small launches: several.
CASES = [(2, 2, 208, 1.0, False, 0), (25, 12, 209, 1.3, True, 1), (1, 3, 256, 1.3, False, 1), (2, 2, 256, 1.0, True, 0),
         (2, 2, 577, 1.0, True, 0), (17, 12, 577, 1.7, False, 1), (1, 2, 655, 1.0, False, 1), (1, 2, 656, 1.3, True, 0),
         (1, 2, 785, 1.0, True, 1), (11, 12, 785, 1.3, False, 0), (1, 2, 1000, 1.3, True, 0), (1, 1, 1024, 1.0, False, 1),
         (1, 2, 1025, 1.0, True, 1), (1, 2, 1025, 1.1, False, 0)]


@pytest.mark.parametrize("B,H,T,s_mult,band,blocks", CASES)
def test_attention_ibert_long_equals_specification(B, H, T, s_mult, band, blocks):
    rng = np.random.default_rng(500 + B * H + T)
    hd = 64
    qkv = np.clip(np.rint(rng.normal(0, 30, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)
    # a one-hot row: query 5 of (0, 0) has one dominant key (17) among small ones; its score saturates at 127, and the table holds
    # the power of two 16384 at distance 0 of that row maximum (255 % 3 == 0): p = 128
    qkv[0, 0, 0, 5] = 0
    qkv[0, 0, 0, 5, :8] = 127
    qkv[1, 0, 0] = np.clip(qkv[1, 0, 0], -10, 10)
    qkv[1, 0, 0, 17, :8] = 127
    ms, es = dyadic(np.float32(np.float32(2.0 ** -11) * np.float32(s_mult)), np.float32(2.0 ** -2))
    mo, eo = dyadic(np.float32(2.0 ** -10), np.float32(2.0 ** -3))
    assert ((int(ms[0]) & (int(ms[0]) - 1)) == 0) == (s_mult == 1.0)
    tab = R.synthetic_table(T)
    exp, n128, omax = R.expected(qkv, ms, es, mo, eo, tab)
    assert n128 > 0 and np.abs(exp).max() > 20
    got = _run(qkv, ms, es, mo, eo, tab, band, blocks)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"
    assert np.array_equal(got[0, 5, :hd], exp[0, 5, :hd])


@pytest.mark.parametrize("T,seed,bits", R.CRAFTED)
def test_crafted_rows_pin_the_order_of_the_row_sum(T, seed, bits):
    """a score row t reaches the kernel exactly through q = 64 e_0, K[:, 0] = t and the score multiplier 2^-6; output multiplier 1
    and V in {-1, 0, 1}, so that a probability that moves by one moves an output byte by one and nothing saturates.  The
    expectation with torch's order differs from the one with the left-to-right sum in the crafted queries' bytes, and the kernel
    gives the former"""
    row = R.crafted_row(T, seed, bits)
    t, e = row["t"], R.crafted_exponents(row)
    pt = R.probabilities(e, orc.torch_rowsum(e))
    pa = R.probabilities(e, R.sum_left_to_right(e))
    moved = pt != pa
    assert moved.any()
    rng = np.random.default_rng(seed + T)
    hd = 64
    queries = (0, 16 * 7 + 3, T - 1)                       # the same row in three query tiles, the last (partial) one included
    qkv = np.zeros((3, 1, 1, T, hd), np.int8)
    for i in queries:
        qkv[0, 0, 0, i, 0] = 64
    qkv[1, 0, 0, :, 0] = t
    V = rng.integers(-1, 2, size=(T, hd)).astype(np.int8)
    V[moved, 0] = 1
    V[moved, 1] = -1
    qkv[2, 0, 0] = V
    tab = R.synthetic_table(T)
    tab[row["qm"] + 128] = row["tabrow"]
    ms, es = dyadic(np.float32(2.0 ** -6), np.float32(1.0))
    mo, eo = dyadic(np.float32(1.0), np.float32(1.0))
    S = orc.gemm_i8(qkv[0, 0, 0], qkv[1, 0, 0])
    ka = orc.requant(S, ms.astype(np.float64), es, 8)
    for i in queries:
        assert np.array_equal(ka[i], t.astype(np.int32))   # the wanted scores, exactly
    exp, _, omax = R.expected(qkv, ms, es, mo, eo, tab)
    exp_a, _, omax_a = R.expected(qkv, ms, es, mo, eo, tab, rowsum=R.sum_left_to_right)
    assert omax <= 127 and omax_a <= 127                   # |O| <= sum p <= 128: nothing saturates
    for i in queries:
        assert exp[0, i, 0] - exp_a[0, i, 0] == int((pt - pa)[moved].sum()) != 0
        assert exp[0, i, 1] - exp_a[0, i, 1] == -int((pt - pa)[moved].sum())
    if (T, seed, bits) in R.CRAFTED_B:
        exp_b, _, _ = R.expected(qkv, ms, es, mo, eo, tab, rowsum=R.sum_lane_tree)
        assert not np.array_equal(exp[0, list(queries)], exp_b[0, list(queries)])
    got = _run(qkv, ms, es, mo, eo, tab, False, 0)
    for i in queries:
        assert np.array_equal(got[0, i], exp[0, i]), (i, got[0, i, :4], exp[0, i, :4], exp_a[0, i, :4])
        assert not np.array_equal(got[0, i], exp_a[0, i])
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"


@pytest.mark.parametrize("T,hd,null,match", [(1026, 64, None, "unsupported geometry"), (207, 64, None, "unsupported geometry"),
                                             (577, 32, None, "unsupported geometry"), (577, 64, "qkv", "NULL|bad operand"),
                                             (577, 64, "table", "NULL|bad operand")])
def test_attention_ibert_long_argument_errors(T, hd, null, match):
    a = torch.zeros(3 * T * 64 + 64, dtype=torch.int8, device=DEV)
    tab = torch.zeros(65536, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_attention_fused_i8_ibert_long", None if null == "qkv" else _lib.ptr(a), _lib.ptr(a), 1, 1, T, hd, 1 << 30, 40,
                  1 << 30, 40, None if null == "table" else _lib.ptr(tab), None, 0, 0, st())


# ----------------------------------------------------------------------------------- models through the module path
def _images(n, img, g):
    """smooth random patterns plus noise: image content at the scale of patches"""
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def _calibrated(img, patch, embed_dim, depth, heads, pow2, seed, family, peak=4.0):
    """tests/test_gpu_attention_long.py::_calibrated with the operator family and the factor on the qkv weights as arguments"""
    torch.manual_seed(img + patch + embed_dim)
    model = ivit.VisionTransformer(img_size=img, patch_size=patch, embed_dim=embed_dim, depth=depth, num_heads=heads, mlp_ratio=4,
                                   qkv_bias=True, num_classes=40, gelu_type=family, softmax_type=family,
                                   layernorm_type=family).to(DEV).eval()
    with torch.no_grad():
        for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
        for blk in model.blocks:              # peaked attention: a near-uniform row of hundreds of keys rounds every probability to 0
            blk.attn.qkv.weight.mul_(peak)
        g = torch.Generator(device="cpu").manual_seed(seed)
        calib = _images(4, img, g)
        model(calib)
        model(calib.flip(0) * 0.7)
    if pow2:
        for mod in model.modules():
            if isinstance(mod, q.QuantAct):
                qmax = 2 ** (mod.activation_bit - 1) - 1
                a = max(-float(mod.x_min), float(mod.x_max)) / qmax
                p = 2.0 ** np.ceil(np.log2(a))
                mod.x_max.fill_(qmax * p)
                mod.x_min.fill_(-qmax * p)
    ivit.freeze_model(model)
    return model, g


class _Trace:
    """records the names _lib.call is asked for, and calls through"""

    def __enter__(self):
        self.names, self.orig = [], _lib.call

        def call(name, *args):
            self.names.append(name)
            return self.orig(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig
        return False


def _literal(model, x):
    from ivit_amd.quantization_utils import lazy
    old = lazy.ENABLED
    try:
        lazy.ENABLED = False
        return model(x)
    finally:
        lazy.ENABLED = old


@pytest.mark.parametrize("img,patch,embed_dim,heads,batch,pow2", [(384, 16, 128, 2, 3, False), (384, 16, 128, 2, 3, True),
                                                                  (224, 8, 128, 2, 3, False), (224, 8, 128, 2, 3, True),
                                                                  (384, 16, 768, 12, 4, False)])
def test_ibert_model_module_path_uses_the_long_kernel(img, patch, embed_dim, heads, batch, pow2):
    """a frozen I-BERT model of 577 / 785 tokens, called as the reference calls it: the model itself declines the fused engine, the
    int8-carrying module path launches one fused attention per block (no q . k^T GEMM, no score tensor) and its logits are bit for
    bit those of the literal module-by-module path.  C = 768 at batch 4: 2308 token rows, the GEMMs' block layout"""
    from ivit_amd.quantization_utils import lazy
    depth = 2
    # C = 768: the factor 4 on the qkv weights that makes the 128-wide models' attention peaked drives these scores to +-230 at a
    # scale of 1.8, where I-BERT's integer exponential is 0 for every key but the maximum's neighbours and the attention output's
    # calibrated range collapses to 0; factor 1 gives scores of +-15
    model, g = _calibrated(img, patch, embed_dim, depth, heads, pow2, 5, "ibert", 4.0 if embed_dim == 128 else 1.0)
    for blk in model.blocks:                  # a live attention: the calibrated output range is not empty
        assert float(blk.attn.qact2.x_max) > 0 and float(blk.attn.qact2.x_min) < 0
    reason = model.engine_unsupported_reason()
    assert reason is not None and "tokens" in reason
    x = _images(batch, img, g)
    with torch.no_grad():
        model(x)                              # warm-up: tables and (m, e) pairs are cached
        lazy.STATS.update(fused=0, materialised=0)
        with _Trace() as tr:
            y = model(x)
        stats = dict(lazy.STATS)
        yl = _literal(model, x)
    assert tr.names.count(NAME) == depth, [n for n in tr.names if "attention" in n or "bgemm" in n]
    assert "ivit_bgemm_qk_i8" not in tr.names and "ivit_attention_fused_i8_ibert" not in tr.names
    assert stats["materialised"] == 1, stats          # the logits, at the model's boundary
    assert torch.equal(y, yl)
    assert not torch.equal(y[0], y[1]) and y.abs().max() > 0


def test_ibert_model_with_a_collapsed_attention_range_keeps_the_literal_attention():
    """C = 768 with the factor 4 on the qkv weights: every probability of the calibration images is 0, the attention output's range
    is empty and the output multiplier (s_pv / s_out) is beyond the kernel's 512.  Such a model ran the literal attention before
    the long-row kernel was routed in, and still does: no launch, no error, the literal path's logits"""
    model, g = _calibrated(384, 16, 768, 2, 12, False, 5, "ibert", 4.0)
    assert all(float(blk.attn.qact2.x_max) == 0 == float(blk.attn.qact2.x_min) for blk in model.blocks)
    x = _images(2, 384, g)
    with torch.no_grad():
        with _Trace() as tr:
            y = model(x)
        yl = _literal(model, x)
    assert not [n for n in tr.names if n.startswith("ivit_attention_fused")]
    assert torch.equal(y, yl)


@pytest.mark.parametrize("pow2", [False, True])
def test_ivit_model_module_path_uses_the_long_kernel(pow2):
    """the I-ViT family at 384 / 16 with the engine switched off: the module path launches ivit_attention_fused_i8_long once per
    block; logits equal the literal path's and the engine's"""
    depth = 2
    model, g = _calibrated(384, 16, 128, depth, 2, pow2, 5, "ivit")
    assert model.engine_unsupported_reason() is None
    x = _images(3, 384, g)
    with torch.no_grad():
        ye = model(x)
        assert model._engine is not None and model._engine[2].T == 577
        model.use_engine = False
        try:
            model(x)
            with _Trace() as tr:
                y = model(x)
            yl = _literal(model, x)
        finally:
            model.use_engine = True
    assert tr.names.count("ivit_attention_fused_i8_long") == depth, [n for n in tr.names if "attention" in n or "bgemm" in n]
    assert "ivit_bgemm_qk_i8" not in tr.names
    assert torch.equal(y, yl) and torch.equal(y, ye)
    assert not torch.equal(y[0], y[1]) and y.abs().max() > 0
