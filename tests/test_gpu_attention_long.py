"""Fused attention on long rows (ivit_attention_fused_i8_long, 208 .. 1025 tokens) against the oracle, and the engine at 384 / 16
(577 tokens) and 224 / 8 (785 tokens) against the module-by-module path."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402
import attention_ref as A  # noqa: E402
from attention_ref import DEV, release, st  # noqa: E402,F401  (release: the autouse fixture)


def _expected(qkv, ms, es, s_at, mo, eo, compat):
    return A.expected(qkv, s_at, ms, es, mo, eo, compat, 8, pmax=127)[0]


def _run(qkv, ms, es, s_at, mo, eo, form, blocks):
    return A.run("ivit_attention_fused_i8_long", qkv, s_at, ms, es, mo, eo, form, 8, blocks)


# (B, H, T, score multiplier, Shiftmax regime, block-layout output).  s_mult 1: Ms a power of two (float32 requantisation of the
# scores), otherwise float64.  Small B * H: several workgroups per head; 25 x 12 heads at 209 tokens: one.
CASES = [(2, 2, 209, 1.0, "pow2", 0), (25, 12, 209, 1.3, "pow2", 1), (1, 3, 256, 1.3, "pow2", 1), (2, 2, 256, 1.0, "band", 0),
         (2, 2, 577, 1.0, "pow2", 0), (1, 2, 577, 1.7, "band", 1), (1, 2, 785, 1.0, "pow2", 1), (1, 2, 785, 1.3, "exp2d", 0),
         (1, 2, 1025, 1.0, "pow2", 1), (1, 2, 1025, 1.1, "band", 0), (1, 1, 1025, 1.3, "exp2d", 1)]


@pytest.mark.parametrize("B,H,T,s_mult,form,blocks", CASES)
def test_attention_long_equals_oracle(B, H, T, s_mult, form, blocks):
    rng = np.random.default_rng(300 + B * H + T)
    hd = 64
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)
    # a one-hot row: query 5 of (0, 0) has one dominant key (17) among small ones
    qkv[0, 0, 0, 5] = 0
    qkv[0, 0, 0, 5, :8] = 127
    qkv[1, 0, 0] = np.clip(qkv[1, 0, 0], -20, 20)
    qkv[1, 0, 0, 17, :8] = 127
    natural = form != "pow2"
    s_at, ms, es, mo, eo = A.scales(natural, s_mult, 8)
    exp = _expected(qkv, ms, es, s_at, mo, eo, natural)
    got = _run(qkv, ms, es, s_at, mo, eo, form, blocks)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"
    assert np.abs(exp).max() > 5
    assert np.array_equal(got[0, 5, :hd], exp[0, 5, :hd])


def _probability(e, S):
    """Shiftmax's p of an exponent e in a row whose exponent sum is S (ivit_modules.py:171-175): S rounded to float32, clamped at
    2^31, factor = floor(2^31 / S), p = floor(fl32(e * factor) / 2^24)"""
    S = min(np.float32(S), np.float32(2.0 ** 31))
    factor = np.floor(np.float32(np.float32(1.0) / S) * np.float32(2.0 ** 31))
    return int(np.floor(np.float32(np.float32(e) * factor) / np.float32(2.0 ** 24)))


def test_attention_long_row_sum_beyond_32_bits():
    """x0 = -520 and flat scores at 1025 tokens: every exponent is e0 = 520 * 2^15, the exact row sum 1025 * e0 = 1.75e10 exceeds
    2^32 and clamps to 2^31 (factor 1, p = 1).  The sum wrapped to 32 bits is 2.85e8 < 2^31 (factor 7, p = 7): a 32-bit accumulator,
    or a lost high half in the lane reduction, changes every output of that head"""
    B, H, T, hd = 1, 2, 1025, 64
    rng = np.random.default_rng(7)
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)
    qkv[1, 0, 0] = 0                                   # head 0: every score 0
    s_a1 = np.float32(2.0 ** -4)
    s_S = np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125))
    s_at = np.float32(1.0 / 519.5)                     # floor(-1 / s) = -520
    assert np.floor(np.float32(np.float32(1.0) / s_at) * np.float32(-1.0)) == -520
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(np.float32(np.float32(1 / 128.0) * s_a1), np.float32(2.0 ** -6))
    e0 = 520 * 2 ** 15
    exact, wrapped = T * e0, (T * e0) % 2 ** 32
    assert exact > 2 ** 32 and wrapped < 2 ** 31
    assert _probability(e0, exact) == 1 and _probability(e0, wrapped) == 7
    S = orc.gemm_i8(qkv[0, 0, 0], qkv[1, 0, 0])
    P = orc.shiftmax(orc.requant(S, ms.astype(np.float64), es, 8), s_at)
    assert (P == 1).all()                              # the oracle agrees: the clamped exact sum
    exp = _expected(qkv, ms, es, s_at, mo, eo, False)
    got = _run(qkv, ms, es, s_at, mo, eo, "pow2", 0)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"
    # the two sums give different outputs for this head: p = 1 against p = 7 on every key
    O1 = qkv[2, 0, 0].astype(np.int64).sum(axis=0)
    r1 = orc.requant(O1.reshape(1, -1).astype(np.int32), mo.astype(np.float64), eo, 8)
    r7 = orc.requant((7 * O1).reshape(1, -1).astype(np.int32), mo.astype(np.float64), eo, 8)
    assert np.array_equal(exp[0, :, :64], np.broadcast_to(r1, (T, 64))) and not np.array_equal(r1, r7)


@pytest.mark.parametrize("T,hd,null,match", [(1026, 64, False, "unsupported geometry"), (207, 64, False, "unsupported geometry"),
                                             (577, 32, False, "unsupported geometry"), (577, 64, True, "NULL")])
def test_attention_long_argument_errors(T, hd, null, match):
    a = torch.zeros(3 * T * 64 + 64, dtype=torch.int8, device=DEV)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_attention_fused_i8_long", None if null else _lib.ptr(a), _lib.ptr(a), 1, 1, T, hd, 1 << 30, 40, 0.25,
                  1 << 30, 40, None, None, 0, 0, st())


# ----------------------------------------------------------------------------------- engine against the module path
def _images(n, img, g):
    """smooth random patterns plus noise: image content at the scale of patches (the class token's attention over hundreds of
    patches averages white noise out)"""
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def _calibrated(img, patch, embed_dim, depth, heads, pow2, seed):
    torch.manual_seed(img + patch + embed_dim)
    model = ivit.VisionTransformer(img_size=img, patch_size=patch, embed_dim=embed_dim, depth=depth, num_heads=heads, mlp_ratio=4,
                                   qkv_bias=True, num_classes=40).to(DEV).eval()
    with torch.no_grad():
        for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
        # peaked attention: with 8-bit probabilities a near-uniform row of hundreds of keys rounds every probability to 0, and the
        # class token would no longer see the image
        for blk in model.blocks:
            blk.attn.qkv.weight.mul_(4.0)
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


def _module_paths(model, x):
    from ivit_amd.quantization_utils import lazy
    model.use_engine = False
    try:
        yl = model(x)
        old = lazy.ENABLED
        try:
            lazy.ENABLED = False
            ym = model(x)
        finally:
            lazy.ENABLED = old
    finally:
        model.use_engine = True
    return yl, ym


@pytest.mark.parametrize("img,patch,pow2", [(384, 16, False), (384, 16, True), (224, 8, False), (224, 8, True)])
def test_engine_long_rows_equal_the_module_path(img, patch, pow2):
    """the engine takes 577 / 785 tokens (ivit_attention_fused_i8_long) and equals the literal module-by-module path and the
    int8-carrying one bit for bit; forward_topk and graph replay equal the eager forward"""
    T = (img // patch) ** 2 + 1
    model, g = _calibrated(img, patch, 128, 2, 2, pow2, 5)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    x = _images(3, img, g)
    with torch.no_grad():
        ye = model(x)
        assert model._engine is not None and model._engine[2].T == T
        yl, ym = _module_paths(model, x)
    assert torch.equal(ye, ym) and torch.equal(yl, ym)
    assert not torch.equal(ye[0], ye[1]) and ye.abs().max() > 0
    eng = model._engine[2]
    xi = x.contiguous().float()
    li, lf, t1 = (t.clone() for t in eng.forward(xi))
    assert torch.equal(lf, ye)
    ki, kf, tk = (t.clone() for t in eng.forward_topk(xi, k=5))
    assert torch.equal(ki, li) and torch.equal(kf, lf) and torch.equal(tk[:, 0], t1)
    gi, gf, gt = (t.clone() for t in eng.forward_graph(xi))
    assert torch.equal(gi, li) and torch.equal(gf, lf) and torch.equal(gt, t1)
    hi, hf, hk = (t.clone() for t in eng.forward_topk_graph(xi, k=5))
    assert torch.equal(hi, li) and torch.equal(hk, tk)
    torch.cuda.synchronize()


def test_engine_deit_base_width_at_384():
    """C = 768 (12 heads), depth 2, 384 px, batch 4: 2308 token rows, so the GEMMs take the block layout and attention writes it"""
    model, g = _calibrated(384, 16, 768, 2, 12, False, 11)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    x = _images(4, 384, g)
    with torch.no_grad():
        ye = model(x)
        assert model._engine[2].T == 577
        yl, ym = _module_paths(model, x)
    assert torch.equal(ye, ym) and torch.equal(yl, ym)
