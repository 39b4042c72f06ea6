"""Token features without a GPU: the prototypes of the four float-emitting LayerNorm entries against the ctypes table, the ABI
ratchets' view of them, the refusals of forward_tokens on CPU-resident models before any library call, and -- with the native library
stubbed as tests/test_feature_maps_cpu.py stubs it -- the launches IntViTEngine.forward_tokens adds behind the second residual GEMM
of each selected block.  (The tensors themselves: tests/test_gpu_layernorm_f32.py, tests/test_gpu_forward_tokens.py.)"""
import os
import re

import pytest
import torch

import ivit_amd as ivit
from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine

from test_abi_coverage_cpu import declared_names
from test_feature_maps_cpu import _trace, calls, no_library      # noqa: F401  (fixtures)
from test_strides_coverage_cpu import ld_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = ["x", "ldx", "B", "T_all", "t0", "T", "C"]
ENTRIES = {
    "ivit_layernorm_i8_f32": SELECT + ["bias_int", "s_ln", "remap", "phi", "out", "ldo", "flags", "stream"],
    "ivit_layernorm_i16_f32": SELECT + ["s_in", "bias_int", "s_ln", "out", "ldo", "flags", "stream"],
    "ivit_ibert_layernorm_i8_f32": SELECT + ["s_in", "bias_int", "s_out", "shift_pow2", "out", "ldo", "flags", "stream"],
    "ivit_ibert_layernorm_i16_f32": SELECT + ["s_in", "bias_int", "s_out", "shift_pow2", "out", "ldo", "flags", "stream"],
}


def _prototype(name):
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ivit_hip.h")).read(), flags=re.S)
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "const int16_t*": _lib.vp, "const float*": _lib.vp, "float*": _lib.vp, "int": _lib.ci,
             "int64_t": _lib.i64, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [kinds[re.sub(r"\s+\w+$", "", p)] for p in params], [re.findall(r"\w+", p)[-1] for p in params]


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_prototypes_match_ctypes_table(name):
    kinds, names = _prototype(name)
    assert _lib.SIGNATURES[name] == kinds
    assert names == ENTRIES[name]


def test_the_abi_ratchets_see_the_new_entries():
    assert set(ENTRIES) <= set(declared_names())
    ex = ld_exports()
    for name in ENTRIES:
        assert [n for n in ex[name] if n.startswith("ld")] == ["ldx", "ldo"]
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    assert "#define IVIT_LN_F32_CHANNEL_MAJOR 1" in hdr and "#define IVIT_LN_F32_FAST_DIV 2" in hdr
    from ivit_amd import engine_common
    assert (engine_common.LN_F32_CHANNEL_MAJOR, engine_common.LN_F32_FAST_DIV) == (1, 2)


# ---------------------------------------------------------------------------- refusals, before any library call
def _vit():
    return ivit.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=5).eval()


def _swin():
    return ivit.SwinTransformer(img_size=56, patch_size=4, embed_dim=96, depths=(2, 2), num_heads=(3, 6), window_size=7, num_classes=5).eval()


@pytest.mark.parametrize("bad", [(3,), (-1,), (1, 1)])
def test_vit_model_refuses_bad_indices(no_library, bad):
    with pytest.raises(ValueError, match="indices"):
        _vit().forward_tokens(torch.zeros(1, 3, 32, 32), bad)


@pytest.mark.parametrize("idx", [(1,), (1, 2), (0, 1, 2)])
def test_vit_model_refuses_integers_off_the_last_block(no_library, idx):
    with pytest.raises(ValueError, match="integers=True"):
        _vit().forward_tokens(torch.zeros(1, 3, 32, 32), idx, integers=True)


def test_models_refuse_an_unknown_format(no_library):
    with pytest.raises(ValueError, match="fmt="):
        _vit().forward_tokens(torch.zeros(1, 3, 32, 32), fmt="NHWC")
    with pytest.raises(ValueError, match="fmt="):
        _swin().forward_tokens(torch.zeros(1, 3, 56, 56), fmt="NLHC")


def test_swin_has_no_prefix(no_library):
    with pytest.raises(ValueError, match="prefix"):
        _swin().forward_tokens(torch.zeros(1, 3, 56, 56), prefix=True)


# ---------------------------------------------------------------------------- the engine's launches, library stubbed
F32 = tuple(sorted(ENTRIES))


@pytest.mark.parametrize("tag,kw,entry", [
    ("deit_tiny", {}, "ivit_layernorm_i8_f32"), ("deit_tiny_natural", {}, "ivit_layernorm_i8_f32"),
    ("deit_tiny_ibert", dict(family="ibert"), "ivit_ibert_layernorm_i8_f32"),
    ("deit_tiny_w16", dict(stream_bits=16, softmax_bits=16, pos_bits=16), "ivit_layernorm_i16_f32")])
@pytest.mark.parametrize("fmt", ["NLC", "NCHW"])
def test_forward_tokens_adds_one_float_layernorm_per_selected_block(calls, tag, kw, entry, fmt):
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4, **kw)
    B, C, T, D = 2, cfg["embed_dim"], eng.T, cfg["depth"]
    x = torch.zeros(B, 3, 224, 224)
    full, _ = _trace(calls, lambda: eng.forward(x))
    got, (tokens, prefixes, scale) = _trace(calls, lambda: eng.forward_tokens(x, (2, 0), fmt, prefix=False))
    assert list(tokens) == [2, 0] and prefixes == {}
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (C,)
    for t in tokens.values():
        assert t.dtype == torch.float32 and tuple(t.shape) == ((B, T - 1, C) if fmt == "NLC" else (B, C, 14, 14))
    where = [i for i, (n, _) in enumerate(got) if n in F32]
    assert len(where) == 2 and all(got[i][0] == entry for i in where), "one float LayerNorm launch per selected index"
    assert [c for i, c in enumerate(got) if i not in where] == full, "the forward's own launches must not change"
    for block, i in zip((0, 2), where):
        a = got[i][1]
        assert len(a) == len(_lib.SIGNATURES[entry])
        prev = got[i - 1]                     # the second residual GEMM of the block: its output is the stream the launch reads
        assert "residual" in prev[0] and a[0] in prev[1]
        assert a[1:7] == (C, B, T, 1, T - 1, C)
        assert a[-4] == tokens[block].data_ptr() and a[-3] == (C if fmt == "NLC" else T - 1) and a[-2] & 1 == int(fmt == "NCHW")
    # with the prefix: NLC takes the class row in the same launch, NCHW in one small launch of its own
    got, (tokens, prefixes, _) = _trace(calls, lambda: eng.forward_tokens(x, (1,), fmt))
    sel = [a for n, a in got if n in F32]
    assert list(prefixes) == [1] and tuple(prefixes[1].shape) == (B, 1, C)
    if fmt == "NLC":
        assert [a[3:6] for a in sel] == [(T, 0, T)]
        assert prefixes[1].data_ptr() + 4 * C == tokens[1].data_ptr()
    else:
        assert [a[3:6] for a in sel] == [(T, 1, T - 1), (T, 0, 1)]
    # the last block by default; never in the plain forward, the pruned tail or what the graphs capture
    last, (tokens, _, _) = _trace(calls, lambda: eng.forward_tokens(x, fmt=fmt))
    assert list(tokens) == [D - 1] and [c for c in last if c[0] not in F32] == full
    for run in (lambda: eng.forward(x), lambda: eng._graph_forward(x), lambda: eng.forward_features(x)):
        assert not [n for n, _ in _trace(calls, run)[0] if n in F32]


def test_a_headless_engine_launches_nothing_behind_the_last_selected_block(calls):
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4)
    x = torch.zeros(2, 3, 224, 224)
    whole, _ = _trace(calls, lambda: eng.forward_tokens(x, (0, 2)))
    eng.head = None                                       # (what a source without head.weight leaves)
    early, _ = _trace(calls, lambda: eng.forward_tokens(x, (0, 2)))
    names = [n for n, _ in early]
    assert names[-1] == "ivit_layernorm_i8_f32" and names == [n for n, _ in whole][:len(names)]
    assert names.count("ivit_gemm_i8_requant_qkv_ex") == 3 and "ivit_gemm_i8_i32" not in names and "ivit_head_argmax" not in names


def test_integers_run_the_int8_layernorm_over_all_rows(calls):
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4)
    B, C, T, D = 2, cfg["embed_dim"], eng.T, cfg["depth"]
    x = torch.zeros(B, 3, 224, 224)
    full, _ = _trace(calls, lambda: eng.forward(x))
    got, (tokens, prefixes, scale) = _trace(calls, lambda: eng.forward_tokens(x, fmt="NCHW", integers=True))
    extra = [c for c in got if c not in full]
    assert [n for n, _ in extra] == ["ivit_layernorm_i8_ex", "ivit_tokens_to_nchw_i8"] and extra[0][1][2] == B * T
    assert scale == eng.s_feat and tokens[D - 1].dtype == torch.int8 and tuple(tokens[D - 1].shape) == (B, C, 14, 14)
    assert prefixes[D - 1].dtype == torch.int8 and tuple(prefixes[D - 1].shape) == (B, 1, C)
    del calls[:]
    for idx in ((0,), (D - 2, D - 1)):
        with pytest.raises(ValueError, match="integers=True"):
            eng.forward_tokens(x, idx, integers=True)
    for bad in ((D,), (-1,), (1, 1)):
        with pytest.raises(ValueError, match="indices"):
            eng.forward_tokens(x, bad)
    with pytest.raises(ValueError, match="fmt="):
        eng.forward_tokens(x, fmt="NHWC")
    assert not calls
