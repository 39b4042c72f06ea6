"""ViT's width knobs at 4 (vit_quant.py:180-187, what `--bitwidth 4` sets) on the integer-carrying module path
(quantization_utils/lazy.py): small calibrated models at 17, 197 and 577 tokens with both operator families, and subsets of the eight
knobs, each against the literal module-by-module path (lazy.ENABLED = False), bit for bit; a width the reference does not clamp
at (6) behaves as it did."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402

import ivit_amd.quantization_utils as q  # noqa: E402
from test_gpu_vit16_lazy import DEV, LITERAL, W8, _assert_carried, _carried, _images, _literal, bits  # noqa: E402

W4 = {k: 4 for k in W8}                                                # every knob at 4
STREAM = ("patch_embed_bw", "block_input_bw", "attention_out_bw", "mlp_out_bw", "norm2_in_bw", "att_block_out_bw")
NARROW = ("ivit_gemm_i8_requant_bits_ex", "ivit_gemm_i8_requant_residual_bits_ex", "ivit_residual_requant_i8_bits")


PEAK = 16.0     # factor on the qkv weights: at 4 bits a row of hundreds of keys needs a sharp peak to hold a probability of 1/8 at all


def _calibrated(img, patch, embed_dim, depth, heads, pow2, seed, family, widths, peak=PEAK):
    """tests/test_gpu_vit16_lazy.py::_calibrated for a 4-bit stream, whose step is a seventh of the largest activation: the class
    token and the position embedding are drawn at the size of the patch embedding (at the init's 0.02 the class row is all zeros
    at 4 bits, and with it every logit)"""
    torch.manual_seed(img + patch + embed_dim)
    model = ivit.VisionTransformer(img_size=img, patch_size=patch, embed_dim=embed_dim, depth=depth, num_heads=heads, mlp_ratio=4,
                                   qkv_bias=True, num_classes=40, gelu_type=family, softmax_type=family, layernorm_type=family,
                                   **widths).to(DEV).eval()
    with torch.no_grad():
        for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
        model.cls_token.normal_(0.0, 2.0)
        model.pos_embed.normal_(0.0, 0.7)
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
                assert a > 0, "a QuantAct of the test model saw nothing but zeros"
                p2 = 2.0 ** np.ceil(np.log2(a))
                mod.x_max.fill_(qmax * p2)
                mod.x_min.fill_(-qmax * p2)
    ivit.freeze_model(model)
    return model, g


# ----------------------------------------------------------------------------------- the reference's fixtures
@pytest.mark.parametrize("tag,attn", [("deit_tiny_w4", "ivit_attention_fused_i8_wide"), ("deit_tiny_w4_natural", "ivit_attention_fused_i8_wide"),
                                      ("deit_tiny_ibert_w4", "ivit_attention_fused_i8_ibert_wide"),
                                      ("deit_tiny_ibert_w4_natural", "ivit_attention_fused_i8_ibert_wide")])
def test_golden_4bit_models_are_carried_as_integers(tag, attn):
    """scripts/gen_w4_golden.py's fixtures (the reference's own forward with every knob at 4): its INT32 logits, top-1 and the CRC32
    of every QuantAct tap, from a forward that carries integers from the input QuantAct to the classifier and launches one fused
    attention per block"""
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    fam = meta["family"]
    model = ivit.deit_tiny_patch16_224(gelu_type=fam, softmax_type=fam, layernorm_type=fam, **meta["widths"])
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
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    y, names, stats = _carried(model, imgs)
    li = np.rint(y.cpu().numpy().astype(np.float64) / z["head_scale"].astype(np.float64)).astype(np.int32)
    assert np.array_equal(li, z["logits_int32"]), f"{(li != z['logits_int32']).sum()} INT32 logits differ from the reference's"
    assert np.array_equal(y.argmax(dim=1).cpu().numpy(), z["top1"])
    _assert_carried(names, stats)
    assert not [n for n in names if n.startswith(LITERAL)]
    assert [n for n in names if n.startswith("ivit_attention_fused")] == [attn] * cfg["depth"]
    # the taps, on the literal path (a hook's float view would materialise the carried integers): the reference's, by CRC32
    import zlib
    taps = {}
    hooks = [mod.register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, torch.round(o[0] / o[1]).to(torch.int32).cpu().numpy()))
             for name, mod in mods.items() if isinstance(mod, q.QuantAct) and not name.endswith("int_softmax.act")]
    with torch.no_grad():
        y_lit = _literal(model, imgs)         # (_carried switched the engine off)
    for h in hooks:
        h.remove()
    assert torch.equal(y_lit, y)
    gold = dict(zip([str(x) for x in z["tap_names"]], z["tap_crc32"]))
    bad = [n for n, t in taps.items() if n in gold and (zlib.crc32(np.ascontiguousarray(t).tobytes()) & 0xFFFFFFFF) != int(gold[n])]
    assert not bad and len([n for n in taps if n in gold]) == len(gold), (bad[:5], len(taps), len(gold))


def _small(img, family, widths, pow2=True, seed=3):
    return _calibrated(img, 16, 128, 2, 2, pow2, seed, family, widths)


def _both(model, g, img, n=3):
    x = _images(n, img, g)
    model.use_engine = False                  # both sides module by module (the engine: tests/test_gpu_w4_engine.py)
    with torch.no_grad():
        y_lit = _literal(model, x)
    y, names, stats = _carried(model, x)
    assert torch.isfinite(y_lit).all() and int((y_lit != 0).sum()) > y_lit.numel() // 2, "the literal logits are (mostly) zero"
    assert (bits(y) == bits(y_lit)).all(), f"{(bits(y) != bits(y_lit)).sum()} of {y.numel()} logits differ"
    return names, stats


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "natural"])
@pytest.mark.parametrize("img,family,attn", [(224, "ivit", "ivit_attention_fused_i8_wide"), (224, "ibert", "ivit_attention_fused_i8_ibert_wide"),
                                             (64, "ivit", "ivit_attention_fused_i8_wide"), (384, "ivit", "ivit_attention_fused_i8_wide_long")])
def test_every_knob_at_4_is_carried_and_equals_the_literal_path(img, family, attn, pow2):
    """197, 17 and 577 tokens: integers from the input QuantAct to the classifier, one fused attention per block through the wide
    entries with softmax_bits = 4, the narrow GEMM / residual entries at the stream sites"""
    model, g = _small(img, family, W4, pow2)
    names, stats = _both(model, g, img)
    _assert_carried(names, stats)
    assert names.count(attn) == 2 and [n for n in names if "attention" in n] == [attn] * 2
    assert any(n in NARROW for n in names), sorted(set(names))
    assert "ivit_gemm_i8_requant_residual_ex" not in names and "ivit_residual_requant_i8" not in names


def test_ibert_softmax_at_4_bits_on_long_rows_keeps_the_literal_core():
    """I-BERT's softmax has no wide long-row kernel: at 577 tokens the attention core runs literally (as its 16-bit form does), its
    result re-enters the integer stream, and the logits are the literal path's"""
    model, g = _small(384, "ibert", W4)
    names, stats = _both(model, g, 384, n=2)
    assert not [n for n in names if "attention_fused" in n]
    assert any(n in NARROW for n in names)


@pytest.mark.parametrize("family", ["ivit", "ibert"])
@pytest.mark.parametrize("widths", [dict(W8, block_input_bw=4), dict(W8, softmax_bw=4), dict(W8, **{k: 4 for k in STREAM}),
                                    dict(W8, pos_encoding_bw=4), dict(W4, norm2_in_bw=8, mlp_out_bw=8)],
                         ids=["block_input", "softmax", "stream", "position", "mixed_residual"])
def test_knob_subsets_are_carried(widths, family):
    """each site is resolved by its own module: any subset of the knobs at 4 with the others at 8"""
    model, g = _small(224, family, widths)
    names, stats = _both(model, g, 224)
    _assert_carried(names, stats)
    wide = "ivit_attention_fused_i8_ibert_wide" if family == "ibert" else "ivit_attention_fused_i8_wide"
    assert (names.count(wide) == 2) == (widths["softmax_bw"] == 4)


def test_attention_calibrated_on_all_zero_probabilities_keeps_the_literal_core():
    """without the sharp peak the 4-bit Shiftmax of 197 keys is zero everywhere, attn.qact2 is calibrated on zeros and its
    requantiser leaves the fused kernels' bound (multiplier < 512): the attention core runs literally, at any token count, the
    rest of the forward stays carried and the logits are the literal path's"""
    model, g = _calibrated(224, 16, 128, 2, 2, False, 3, "ivit", W4, peak=1.0)
    assert all(float(b.attn.qact2.x_max) == 0.0 and float(b.attn.qact2.x_min) == 0.0 for b in model.blocks), "the precondition of this case"
    names, stats = _both(model, g, 224)
    assert not [n for n in names if "attention_fused" in n] and any(n.startswith("ivit_shiftmax") for n in names)
    assert any(n in NARROW for n in names)


def test_position_parameter_at_4_bits_is_quantised_once():
    """qact_pos on the position parameter (pos_encoding_bw = 4): quantised at the warm-up forward, cached per parameter version"""
    model, g = _small(224, "ivit", W4)
    names, _ = _both(model, g, 224)
    assert "ivit_quantize_input_f32_i32" not in names      # the traced forward is the second carried one: it finds the cache


@pytest.mark.parametrize("widths,entry", [(W4, "ivit_gemm_i8_requant_residual_bits_ex"), (dict(W4, norm2_in_bw=8), "ivit_gemm_i8_requant_residual_bits_ex"),
                                          (dict(W8, att_block_out_bw=4), "ivit_gemm_i8_requant_residual_bits_ex"),
                                          (W8, "ivit_gemm_i8_requant_residual_ex")], ids=["all4", "mid4_out8", "mid8_out4", "all8"])
def test_fused_residual_gemm_takes_both_widths(widths, entry):
    """DeiT-Tiny width at 11 images (2167 rows, from 2048 the weights-in-registers GEMM): attn.proj / mlp.fc2, their QuantAct and
    the residual QuantAct behind it are one kernel, with the widths of both QuantActs; at 8 / 8 the launch is the one it was"""
    model, g = _calibrated(224, 16, 192, 1, 3, True, 5, "ivit", widths)
    names, stats = _both(model, g, 224, n=11)
    _assert_carried(names, stats)
    # depth 1: attn.proj + qact2 and mlp.fc2 + qact4, each one fused launch.  A pair with a 4-bit QuantAct takes the _bits entry, a
    # pair at 8 / 8 the entry it always took
    pairs = [(widths["attention_out_bw"], widths["norm2_in_bw"]), (widths["mlp_out_bw"], widths["att_block_out_bw"])]
    narrow = sum(1 for p in pairs if 4 in p)
    assert names.count("ivit_gemm_i8_requant_residual_bits_ex") == narrow and names.count("ivit_gemm_i8_requant_residual_ex") == 2 - narrow
    assert entry in names and "ivit_residual_requant_i8" not in names and "ivit_residual_requant_i8_bits" not in names


def test_a_width_the_reference_does_not_clamp_at_is_refused_as_before():
    """block_input_bw = 6: the reference returns unclamped integers there (quant_utils.py: bit_num in [4, 8, 16, 32]); this
    package's QuantAct has never taken such a width -- ivit_requant_i32 refuses it -- with the integer-carrying path on or off"""
    torch.manual_seed(1)
    model = ivit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                   num_classes=10, **dict(W8, block_input_bw=6)).to(DEV).eval()
    x = _images(2, 64, torch.Generator(device="cpu").manual_seed(1))
    with torch.no_grad(), pytest.raises(_lib.IvitError, match="ivit_requant_i32: bits=6"):
        model(x)
