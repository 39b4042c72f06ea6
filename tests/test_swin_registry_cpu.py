"""Swin and the operator registry, on the host: the default model is what it was, the fork's default ('ibert') names build a Swin with
the I-BERT operators, the new window-attention entry is declared, bound and exported, and the host proof that lets it take a shift
mask agrees with a float32 brute force over a sweep of scales."""
import ctypes
import os
import re
from functools import partial

import numpy as np
import pytest

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib, inference  # noqa: E402
from ivit_amd.prepare import ibert_saturated_exp, ibert_window_mask_ok  # noqa: E402
from ivit_amd.quantization_utils.ibert_modules import softmax_constants  # noqa: E402

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(img_size=56, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2), num_heads=(3, 6), num_classes=10)
# the I-ViT module tree of one block, a merging and the stem / tail: what a Swin built before the registry reached it consists of
IVIT_CLASSES = {"patch_embed.norm": "IVITIntLayerNorm", "layers.0.blocks.1.norm1": "IVITIntLayerNorm", "layers.0.blocks.1.norm2": "IVITIntLayerNorm",
                "layers.0.blocks.1.attn.log_int_softmax": "IVITIntSoftmax", "layers.0.blocks.1.mlp.act": "IVITIntGELU",
                "layers.0.downsample.norm": "IVITIntLayerNorm", "norm": "IVITIntLayerNorm"}


def classes(model):
    return {n: type(m).__name__ for n, m in model.named_modules()}


def test_default_swin_is_unchanged():
    """the defaults, the factory and an explicit norm_layer= all give the I-ViT tree with the state_dict keys of the I-ViT modules;
    an explicit norm_layer wins over layernorm_type"""
    explicit = ivit.SwinTransformer(norm_layer=partial(qu.IntLayerNorm, eps=1e-6), **SMALL)
    default = ivit.SwinTransformer(**SMALL)
    assert list(default.state_dict()) == list(explicit.state_dict()) and classes(default) == classes(explicit)
    got = classes(default)
    assert all(got[n] == c for n, c in IVIT_CLASSES.items()), {n: got[n] for n in IVIT_CLASSES}
    assert default.op_types == ("ivit",) * 3 and default.op_params == ({}, {}, {}) and default.engine_unsupported_reason() is None
    assert default._reference_widths == explicit._reference_widths
    keys = list(default.state_dict())
    assert "layers.0.blocks.0.attn.log_int_softmax.act_scaling_factor" in keys and "patch_embed.norm.norm_scaling_factor" in keys
    assert not [k for k in keys if ".log_int_softmax.act." in k or k.endswith(".shift")]
    wins = ivit.SwinTransformer(norm_layer=partial(qu.IntLayerNorm, eps=1e-6), layernorm_type="ibert", **SMALL)
    assert classes(wins)["norm"] == "IVITIntLayerNorm" and classes(wins) == classes(explicit)
    tiny = ivit.swin_tiny_patch4_window7_224()
    assert tiny.op_types == ("ivit",) * 3 and all(classes(tiny)[n] == c for n, c in IVIT_CLASSES.items())


def test_swin_takes_the_registry_names():
    m = ivit.SwinTransformer(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert", **SMALL)
    got = classes(m)
    assert all(got[n] == c.replace("IVIT", "IBERT") for n, c in IVIT_CLASSES.items())
    assert m.layers[0].blocks[0].attn.log_int_softmax.output_bit == 8
    assert "operator family" in m.engine_unsupported_reason()
    mixed = ivit.SwinTransformer(gelu_type="ibert", **SMALL)
    assert mixed.op_types == ("ibert", "ivit", "ivit") and "operator family" in mixed.engine_unsupported_reason()
    assert classes(mixed)["layers.1.blocks.0.mlp.act"] == "IBERTIntGELU" and classes(mixed)["norm"] == "IVITIntLayerNorm"
    isq = ivit.SwinTransformer(layernorm_type="ibert_use-int-sqrt_true", **SMALL)
    assert isq.op_params[2] == {"use_int_sqrt": True} and isq.norm.use_int_sqrt and "operator family" in isq.engine_unsupported_reason()
    with pytest.raises(KeyError):
        ivit.SwinTransformer(softmax_type="ppoly", **SMALL)


def test_build_model_gives_swin_the_forks_default_operators():
    m = inference.build_model({"model_name": "swin_tiny_patch4_window7_224"})
    assert type(m).__name__ == "SwinTransformer" and m.op_types == ("ibert",) * 3
    assert type(m.layers[2].blocks[5].attn.log_int_softmax).__name__ == "IBERTIntSoftmax"
    m = inference.build_model({"model_name": "swin_tiny_patch4_window7_224", "gelu_type": "ivit"}, softmax_type="ivit", layernorm_type="ivit")
    assert m.op_types == ("ivit",) * 3 and m.engine_unsupported_reason() is None


def test_new_entry_is_declared_bound_and_exported():
    name = "ivit_window_attention_i8_ibert"
    sig = _lib.SIGNATURES[name]
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
    assert decl, "not declared in include/ivit_hip.h"
    params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(sig) == 25
    for p, c in zip(params, sig):
        want = (ctypes.c_void_p if "*" in p or p.startswith("ivit_stream_t") else ctypes.c_float if p.startswith("float") else
                ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_uint32 if p.startswith("uint32_t") else ctypes.c_int)
        assert c is want or (want is ctypes.c_int and c is ctypes.c_int32), (p, c)
    assert "PRECONDITION" in header[header.index("Window attention with IBERTIntSoftmax"):decl.start()]
    if os.path.exists(_lib.LIB_PATH):          # built trees: the product and the lab library export it
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert getattr(_lib.lib(), name).argtypes == sig


def brute_force(s, x0_int, n=30):
    """every (masked q, row maximum qm) pair, one at a time, in float32: no masked value reaches an unmasked one, and every masked
    distance lands on int_exp's clamp"""
    s = f32(s)
    clamp = f32(f32(n) * f32(x0_int))
    lo_unmasked = min(f32(f32(f32(q) * s) / s) for q in range(-128, 128))
    for q in range(-128, 128):
        xm = f32(f32(f32(f32(q) * s) + f32(-100.0)) / s)
        if not xm < lo_unmasked:
            return False
        for qm in range(-128, 128):
            if not f32(xm - f32(f32(f32(qm) * s) / s)) <= clamp:
                return False
    return True


def test_mask_proof_against_a_brute_force():
    rng = np.random.default_rng(17)
    scales = [2.0 ** -k for k in range(1, 9)] + [0.2887, 0.2889, 0.29, 0.3, 0.31, 0.3465, 0.3466, 0.2310, 0.2311] + list(rng.uniform(0.02, 0.6, 24))
    verdicts = []
    for s in scales:
        x0 = softmax_constants(s, 0.0, 1.0)[0]
        verdicts.append(ibert_window_mask_ok(s, x0))
        assert verdicts[-1] == brute_force(s, x0), s
        if s <= 0.25:
            assert verdicts[-1], s               # 100 / s - 255 >= 30 * ceil(0.6931 / s)
        if s >= 0.35:
            assert not verdicts[-1], s
    assert any(verdicts) and not all(verdicts)


def test_saturated_value_is_the_tables_clamped_entry():
    """the value a masked score contributes = exp_int at distance >= 30 |x0_int| of the softmax restated in oracle/ibert.py"""
    from oracle import ibert as ib
    for s, rng in ((0.125, (0.0, 5.0e6)), (0.1173, (0.0, 1.9e11)), (0.25, (0.0, 3.0e4))):
        c = softmax_constants(s, *rng)
        k = np.array([[127, -128]], np.int32)               # distance 255 >= 30 |x0_int| for s >= 0.0816
        assert 30 * -c[0] <= 255
        _, _, _, ex = ib.softmax(k, s, *rng, return_exp=True)
        x0_int, b_int, c_int, exp_sf, act_sf, m, e = ib.softmax_constants(f32(s), *rng)
        z_int = np.rint(f32(ex[0, 1] / exp_sf))
        q16 = np.clip(np.rint(np.float64(z_int) * m / 2.0 ** e), -32768, 32767)
        want = f32(f32(f32(q16) * act_sf) / act_sf)
        assert ibert_saturated_exp(*c) == want and ex[0, 1] == c[2], (s, ibert_saturated_exp(*c), want)
