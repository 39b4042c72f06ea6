"""ViT's 16-bit configurations (vit_quant.py:180-187, what `--bitwidth 16` sets) on the integer-carrying module path
(quantization_utils/lazy.py): the reference's goldens at 224 px, long rows (577 / 785 tokens) through
ivit_attention_fused_i8_wide_long, DeiT-B width through the fused 16-bit residual GEMM, and the configurations that keep a literal
step -- each against the literal module-by-module path (lazy.ENABLED = False), bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.prepare import sym_scale  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

DEV = "cuda:0"
W16 = dict(patch_embed_bw=16, pos_encoding_bw=8, block_input_bw=16, attention_out_bw=16, softmax_bw=8, mlp_out_bw=16, norm2_in_bw=16,
           att_block_out_bw=16)                                       # the 16-bit residual stream
W16ALL = dict(W16, pos_encoding_bw=16, softmax_bw=16)                  # every knob at 16
W8 = {k: 8 for k in W16}
LITERAL = ("ivit_bgemm_", "ivit_shiftmax_", "ivit_f32_to_i32")         # launches of the float module path


def bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def _images(n, img, g):
    """smooth random patterns plus noise: image content at the scale of patches"""
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def _calibrated(img, patch, embed_dim, depth, heads, pow2, seed, family, widths, peak=4.0, freeze=True):
    """tests/test_gpu_attention_ibert_long.py::_calibrated with the width knobs as an argument"""
    torch.manual_seed(img + patch + embed_dim)
    model = ivit.VisionTransformer(img_size=img, patch_size=patch, embed_dim=embed_dim, depth=depth, num_heads=heads, mlp_ratio=4,
                                   qkv_bias=True, num_classes=40, gelu_type=family, softmax_type=family, layernorm_type=family,
                                   **widths).to(DEV).eval()
    with torch.no_grad():
        for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
        for blk in model.blocks:              # peaked attention
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
    if freeze:
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
    old = lazy.ENABLED
    try:
        lazy.ENABLED = False
        return model(x)
    finally:
        lazy.ENABLED = old


def _carried(model, x):
    """module path with the engine off: warm-up forward, then a traced one -> (logits, launch names, lazy.STATS of that forward)"""
    model.use_engine = False
    with torch.no_grad():
        model(x)                              # warm-up: tables, (m, e) pairs and the embedding constants are cached
        lazy.STATS.update(fused=0, materialised=0)
        with _Trace() as tr:
            y = model(x)
        stats = dict(lazy.STATS)
    return y, tr.names, stats


def _assert_carried(names, stats):
    """integers from the input QuantAct to the logits: nothing of the float module path runs, and the one float conversion is the
    classifier's output at the model's boundary (lazy.linear_to_float: the one materialisation)"""
    assert stats["materialised"] == 1, stats
    assert not [n for n in names if n.startswith(LITERAL)], sorted({n for n in names if n.startswith(LITERAL)})
    assert names.count("ivit_i32_to_f32") == 1 and names[-1] == "ivit_i32_to_f32"


# ----------------------------------------------------------------------------------- the reference's goldens at 224 px
@pytest.mark.parametrize("tag,attn", [("deit_tiny_w16", "ivit_attention_fused_i8_compat_band"),
                                      ("deit_tiny_w16all", "ivit_attention_fused_i8_wide"),
                                      ("deit_tiny_ibert_w16all", "ivit_attention_fused_i8_ibert_wide")])
def test_golden_16bit_models_are_carried_as_integers(tag, attn):
    """the reference's fixtures with the 16-bit stream (w16), with every knob at 16 (w16all) and the latter with the I-BERT operators:
    the reference's logits, from a forward that carries integers from the input QuantAct to the classifier and launches one fused
    attention per block"""
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    fam = meta.get("family", "ivit")
    kw = dict(gelu_type=fam, softmax_type=fam, layernorm_type=fam) if fam != "ivit" else {}
    model = ivit.deit_tiny_patch16_224(**kw, **meta["widths"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    mods = dict(model.named_modules())
    for name, mod in mods.items():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    for name, sh in meta.get("ln_shifts", {}).items():
        mods[name].shift.fill_(float(sh))
    model.to(DEV)
    ivit.freeze_model(model)
    imgs = torch.from_numpy(synth.make_images(2, meta["image_seed"])).to(DEV)
    y, names, stats = _carried(model, imgs)
    with torch.no_grad():
        assert torch.equal(y, _literal(model, imgs))
    if fam == "ivit":
        assert np.array_equal(bits(y), z["logits_f32_bits"][:2])
    else:
        # ranges as calibrated: the reference's head multiplies fl(fl(q s) / s) in a float32 GEMM and its float logits carry that
        # noise in their last bits; the fixture's contract is the INT32 logits (test_ibert_int16_matches_the_reference)
        li = np.rint(y.cpu().numpy().astype(np.float64) / z["head_scale"].astype(np.float64)).astype(np.int32)
        assert np.array_equal(li, z["logits_int32"][:2])
    assert np.array_equal(y.argmax(dim=1).cpu().numpy(), z["top1"][:2])
    _assert_carried(names, stats)
    assert [n for n in names if n.startswith("ivit_attention_fused")] == [attn] * cfg["depth"]
    # nothing is read back from the device once the constants are cached
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            y2 = model(imgs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(y2, y)


# ----------------------------------------------------------------------------------- long rows, I-ViT family
@pytest.mark.parametrize("img,patch,pow2,widths,attn", [
    (384, 16, False, W16ALL, "ivit_attention_fused_i8_wide_long"), (384, 16, True, W16ALL, "ivit_attention_fused_i8_wide_long"),
    (224, 8, False, W16ALL, "ivit_attention_fused_i8_wide_long"), (224, 8, True, W16ALL, "ivit_attention_fused_i8_wide_long"),
    (384, 16, False, W16, "ivit_attention_fused_i8_long"), (224, 8, True, W16, "ivit_attention_fused_i8_long")])
def test_long_rows_on_the_16bit_stream(img, patch, pow2, widths, attn):
    """577 / 785 tokens with the 16-bit stream: the engine declines, the module path carries int16 between the blocks and launches
    one fused long-row attention per block -- the 16-bit-probability kernel with every knob at 16, the 8-bit one with softmax and
    position embedding at 8 bits"""
    depth = 2
    model, g = _calibrated(img, patch, 128, depth, 2, pow2, 5, "ivit", widths)
    for blk in model.blocks:
        assert float(blk.attn.qact2.x_max) > 0 and float(blk.attn.qact2.x_min) < 0
    reason = model.engine_unsupported_reason()
    assert reason is not None and "tokens" in reason
    x = _images(3, img, g)
    y, names, stats = _carried(model, x)
    with torch.no_grad():
        yl = _literal(model, x)
    assert torch.equal(y, yl)
    assert [n for n in names if n.startswith("ivit_attention_fused")] == [attn] * depth
    _assert_carried(names, stats)
    assert names.count("ivit_residual_requant_i16") == 2 * depth and names.count("ivit_embed_assemble_i16") == 1
    assert sum(n.startswith("ivit_layernorm_i16_i8") for n in names) == 2 * depth + 1
    assert not torch.equal(y[0], y[1]) and y.abs().max() > 0


def test_deit_base_width_at_384_fuses_the_residual_gemm():
    """C = 768 (12 heads), depth 2, 384 px, batch 4: 2308 token rows -- the head-major qkv GEMM with the fragment weights, and
    projection / fc2 + their 16-bit QuantAct + the residual QuantAct as one kernel each"""
    depth = 2
    model, g = _calibrated(384, 16, 768, depth, 12, False, 11, "ivit", W16ALL)
    for blk in model.blocks:
        assert float(blk.attn.qact2.x_max) > 0 and float(blk.attn.qact2.x_min) < 0
    x = _images(4, 384, g)
    y, names, stats = _carried(model, x)
    with torch.no_grad():
        yl = _literal(model, x)
    assert torch.equal(y, yl)
    _assert_carried(names, stats)
    assert names.count("ivit_gemm_i8_requant_i16_residual_i16_ex") == 2 * depth and "ivit_residual_requant_i16" not in names
    assert names.count("ivit_attention_fused_i8_wide_long") == depth and names.count("ivit_gemm_i8_requant_qkv_ex") == depth


# ----------------------------------------------------------------------------------- what keeps a literal step
def test_ibert_all16_at_577_tokens_keeps_the_literal_attention():
    """IBERTIntSoftmax with output_bit = 16 has a fused kernel for 193 .. 207 tokens only: at 577 the attention core runs literally,
    nothing fused is launched for it, and the logits are the literal path's.  The qkv weights keep their factor 1: the literal
    P . V (ivit_bgemm_pv_i32_i8) refuses a probability of 2^15 -- a one-hot row -- over 577 keys, whose int32 sum it cannot bound"""
    model, g = _calibrated(384, 16, 128, 2, 2, False, 5, "ibert", W16ALL, peak=1.0)
    x = _images(3, 384, g)
    y, names, stats = _carried(model, x)
    with torch.no_grad():
        yl = _literal(model, x)
    assert not [n for n in names if n.startswith("ivit_attention_fused")]
    assert torch.equal(y, yl)
    assert not torch.equal(y[0], y[1])
    # everything else is still carried: the int16 stream and its LayerNorm
    assert names.count("ivit_residual_requant_i16") == 4 and names.count("ivit_ibert_layernorm_i16_i8_ex") == 5


@pytest.mark.parametrize("widths", [dict(W8, att_block_out_bw=16), dict(W8, patch_embed_bw=16), dict(W8, softmax_bw=16, pos_encoding_bw=16)],
                         ids=["att_block_out", "patch_embed", "softmax_pos"])
def test_other_width_patterns_equal_the_literal_path(widths):
    """a width pattern that is neither all 8 nor the 16-bit stream: whatever mixture of fused and materialised steps it takes, the
    literal path's logits"""
    model, g = _calibrated(224, 16, 128, 2, 2, False, 5, "ivit", widths)
    x = _images(2, 224, g)
    y, names, stats = _carried(model, x)
    with torch.no_grad():
        yl = _literal(model, x)
    assert torch.equal(y, yl)
    assert not torch.equal(y[0], y[1])


@pytest.mark.parametrize("widths", [W16, W16ALL], ids=["softmax8", "softmax16"])
def test_collapsed_attention_range_keeps_the_literal_attention(widths):
    """an attention output range of 0 (every probability of the calibration images 0): the output multiplier s_pv / s_out is beyond
    the long-row kernels' 512 (engine_common.long_multipliers_ok), so no fused attention is launched, without an error, and the logits
    are the literal path's.  With 16-bit probabilities s_pv is 2^-15 * s_v and stays inside the bound at a calibrated value scale:
    the range of attn.qact1 is widened to 512 (s_v = 4) so that the multiplier is beyond it there, too"""
    model, g = _calibrated(384, 16, 128, 2, 2, False, 5, "ivit", widths, freeze=False)
    for blk in model.blocks:
        blk.attn.qact2.x_min.fill_(0.0)
        blk.attn.qact2.x_max.fill_(0.0)
        if widths["softmax_bw"] == 16:
            blk.attn.qact1.x_min.fill_(-512.0)
            blk.attn.qact1.x_max.fill_(512.0)
    ivit.freeze_model(model)
    for blk in model.blocks:
        s_v, s_out = sym_scale(float(blk.attn.qact1.x_min), float(blk.attn.qact1.x_max), 8), sym_scale(0.0, 0.0, 8)
        assert 2.0 ** -(widths["softmax_bw"] - 1) * float(s_v) / float(s_out) >= 512.0
    x = _images(2, 384, g)
    y, names, stats = _carried(model, x)
    with torch.no_grad():
        yl = _literal(model, x)
    assert not [n for n in names if n.startswith("ivit_attention_fused")]
    assert torch.equal(y, yl)
