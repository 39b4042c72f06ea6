"""Feature maps without a GPU: the prototypes of the four ivit_tokens_to_nchw_* entries against the ctypes table (the helper pattern
of tests/test_attention_long_cpu.py), the forward_intermediates methods of both model and both engine classes, index validation on a
CPU-resident model before any library call, and -- with the native library stubbed as tests/test_attention_probs_cpu.py stubs it --
the one launch IntViTEngine.forward_intermediates adds behind the second residual GEMM of each selected block.  (The maps
themselves: tests/test_gpu_feature_maps.py.)"""
import ctypes
import inspect
import os
import re

import pytest
import torch

import ivit_amd as ivit
from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine
from ivit_amd.swin_engine import IntSwinEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ivit_tokens_to_nchw_i8_f32", "ivit_tokens_to_nchw_i16_f32", "ivit_tokens_to_nchw_i8", "ivit_tokens_to_nchw_i16")


def _prototype(name):
    """(ctypes kinds, parameter names) `name` is declared with in include/ivit_hip.h"""
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "int8_t*": _lib.vp, "const int16_t*": _lib.vp, "int16_t*": _lib.vp, "float*": _lib.vp,
             "int": _lib.ci, "int64_t": _lib.i64, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    params = [p.strip() for p in m.group(1).split(",")]
    return [kinds[re.sub(r"\s+\w+$", "", p)] for p in params], [re.findall(r"\w+", p)[-1] for p in params]


@pytest.mark.parametrize("name", ENTRIES)
def test_prototypes_match_ctypes_table(name):
    kinds, names = _prototype(name)
    assert _lib.SIGNATURES[name] == kinds
    scale = ["s"] if name.endswith("_f32") else []
    assert names == ["x", "ldx", "B", "T_all", "t0", "T", "C"] + scale + ["out", "stream"]


@pytest.mark.parametrize("cls", [ivit.VisionTransformer, ivit.SwinTransformer, IntViTEngine, IntSwinEngine])
def test_forward_intermediates_signature(cls):
    sig = inspect.signature(cls.forward_intermediates)
    p = list(sig.parameters.values())
    assert [q.name for q in p][2:] == ["indices", "integers"] and len(p) == 4
    assert p[2].default is None and p[3].default is False


@pytest.fixture
def no_library(monkeypatch):
    """any call into the native library fails the test"""
    def refuse(*a, **k):
        raise AssertionError("a library call before the indices were validated")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("bad", [(3,), (-1,), (1, 1)])
def test_vit_model_refuses_bad_indices_before_any_library_call(no_library, bad):
    m = ivit.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=3, num_heads=2, num_classes=5).eval()
    with pytest.raises(ValueError, match="indices"):
        m.forward_intermediates(torch.zeros(1, 3, 32, 32), bad)


@pytest.mark.parametrize("bad", [(2,), (-1,), (1, 1)])
def test_swin_model_refuses_bad_indices_before_any_library_call(no_library, bad):
    m = ivit.SwinTransformer(img_size=56, patch_size=4, embed_dim=96, depths=(2, 2), num_heads=(3, 6), window_size=7, num_classes=5).eval()
    with pytest.raises(ValueError, match="indices"):
        m.forward_intermediates(torch.zeros(1, 3, 56, 56), bad)


# ---------------------------------------------------------------------------- the engine's launches, library stubbed
@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(name, *args):
        if name == "ivit_ibert_softmax_build_table":      # engine_common reads the table back to choose the band form
            ctypes.memset(args[-2], 0, 65536 * 4)
        rec.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "lib", lambda: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return rec


def _trace(calls, run):
    del calls[:]
    out = run()
    return list(calls), out


@pytest.mark.parametrize("tag,kw,integers,entry", [
    ("deit_tiny", {}, False, ENTRIES[0]), ("deit_tiny_natural", {}, True, ENTRIES[2]), ("deit_tiny_ibert", dict(family="ibert"), False, ENTRIES[0]),
    ("deit_tiny_w16", dict(stream_bits=16, softmax_bits=16, pos_bits=16), False, ENTRIES[1]),
    ("deit_tiny_w16", dict(stream_bits=16, softmax_bits=16, pos_bits=16), True, ENTRIES[3])])
def test_forward_intermediates_adds_one_launch_behind_the_second_residual_gemm(calls, tag, kw, integers, entry):
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4, **kw)
    B, C, T = 2, cfg["embed_dim"], eng.T
    x = torch.zeros(B, 3, 224, 224)
    full, _ = _trace(calls, lambda: eng.forward(x))
    got, (maps, scales) = _trace(calls, lambda: eng.forward_intermediates(x, (2, 0), integers))
    assert list(maps) == [2, 0] and list(scales) == [2, 0]
    want = torch.float32 if not integers else torch.int16 if kw.get("stream_bits") == 16 else torch.int8
    for i, m in maps.items():
        assert m.dtype == want and tuple(m.shape) == (B, C, 14, 14) and m.is_contiguous()
        assert isinstance(scales[i], float) and scales[i] == float(torch.tensor(scales[i], dtype=torch.float32)) > 0
    where = [i for i, (n, _) in enumerate(got) if n in ENTRIES]
    assert len(where) == 2 and all(got[i][0] == entry for i in where)
    assert [c for i, c in enumerate(got) if i not in where] == full, "the forward's own launches must not change"
    for block, i in zip((0, 2), where):
        a = got[i][1]
        assert len(a) == len(_lib.SIGNATURES[entry])
        prev = got[i - 1]                     # the second residual GEMM of the block: its output is the stream the launch reads
        assert "residual" in prev[0] and a[0] in prev[1]
        assert a[1:7] == (C, B, T, 1, T - 1, C) and a[-2] == maps[block].data_ptr()
        if not integers:
            assert a[7] == scales[block]
    assert sum(n.startswith("ivit_layernorm") or n.startswith("ivit_ibert_layernorm") for n, _ in got[:where[0]]) == 2, "behind block 0"
    # every block by default; never in the plain forward, the taps, the pruned tail or what the graphs capture
    every, (maps, _) = _trace(calls, lambda: eng.forward_intermediates(x, None, integers))
    assert list(maps) == list(range(cfg["depth"])) and [n for n, _ in every].count(entry) == cfg["depth"]
    runs = [lambda: eng.forward(x), lambda: eng._graph_forward(x)]
    if eng.stream_bits != 16:
        runs.append(lambda: eng.forward(x, taps={}))
    for run in runs:
        assert not [n for n, _ in _trace(calls, run)[0] if n in ENTRIES]


def test_engine_refuses_bad_indices_before_any_launch(calls):
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4)
    x = torch.zeros(2, 3, 224, 224)
    del calls[:]
    for bad in ((cfg["depth"],), (-1,), (1, 1)):
        with pytest.raises(ValueError, match="indices"):
            eng.forward_intermediates(x, bad)
    assert not calls
