"""Attention maps without a GPU: the prototypes of the two probability entries against the ctypes table, and -- with the native library
stubbed as tests/test_cls_tail_cpu.py stubs it -- the launches IntViTEngine.attention_maps adds to the eager forward: exactly one
behind the qkv GEMM of each selected block, nothing else moved.  (The probabilities themselves: tests/test_gpu_attention_probs.py.)"""
import ctypes
import os
import re

import pytest
import torch

from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = ("ivit_attention_probs_u8", "ivit_attention_probs_u8_ibert")


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


def _engine(tag="deit_tiny", **kw):
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    return IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4, **kw), cfg


def _trace(calls, run):
    del calls[:]
    out = run()
    return list(calls), out


@pytest.mark.parametrize("name", PROBS)
def test_probs_prototypes_match_ctypes_table(name):
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "uint8_t*": _lib.vp, "const uint32_t*": _lib.vp, "const float*": _lib.vp, "int": _lib.ci,
             "int64_t": _lib.i64, "uint32_t": _lib.u32, "int32_t": _lib.i32, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    params = [p.strip() for p in m.group(1).split(",")]
    assert _lib.SIGNATURES[name] == [kinds[re.sub(r"\s+\w+$", "", p)] for p in params]
    names = [re.findall(r"\w+", p)[-1] for p in params]
    assert names[:8] == ["qkv", "probs", "ldp", "batch", "heads", "tokens", "head_dim", "q_rows"] and names[-1] == "stream"
    # the I-BERT entry: the Shiftmax one without s_attn, the float table in place of exp2d
    assert ("s_attn" in names) == (name == PROBS[0]) and names[-4:-1] == (["exp2d", "band", "band_w"] if name == PROBS[0] else ["table", "band", "band_w"])


@pytest.mark.parametrize("tag,kw,entry", [("deit_tiny", {}, PROBS[0]), ("deit_tiny_natural", {}, PROBS[0]),
                                          ("deit_tiny_ibert", dict(family="ibert"), PROBS[1])])
@pytest.mark.parametrize("rows", ["cls", "all"])
def test_attention_maps_adds_one_launch_behind_the_qkv_gemm(calls, tag, kw, entry, rows):
    eng, cfg = _engine(tag, **kw)
    B, H, T = 2, cfg["num_heads"], eng.T
    x = torch.zeros(B, 3, 224, 224)
    full, _ = _trace(calls, lambda: eng.forward(x))
    got, (maps, scale) = _trace(calls, lambda: eng.attention_maps(x, layers=[0, 1], rows=rows))
    R = 1 if rows == "cls" else T
    assert scale == 2.0 ** -7 and sorted(maps) == [0, 1]
    for m in maps.values():
        assert m.dtype == torch.uint8 and tuple(m.shape) == (B, H, R, T) and m.is_contiguous()
    where = [i for i, (n, _) in enumerate(got) if n in PROBS]
    assert len(where) == 2 and all(got[i][0] == entry for i in where)
    assert [c for i, c in enumerate(got) if i not in where] == full, "the forward's own launches must not change"
    qkv = [i for i, (n, _) in enumerate(got) if n == "ivit_gemm_i8_requant_qkv_ex"]
    assert where == [qkv[0] + 1, qkv[1] + 1]
    for layer, i in zip((0, 1), where):
        a = got[i][1]
        assert len(a) == len(_lib.SIGNATURES[entry])
        assert a[0] == got[i - 1][1][7], "the probabilities read the buffer the qkv GEMM wrote"
        assert a[1] == maps[layer].data_ptr() and a[2:8] == (T, B, H, T, 64, R)
        attn = got[i + 1][1]                  # the fused attention behind it: the same score requantiser and tables
        assert got[i + 1][0].startswith("ivit_attention_fused_i8") and a[8:10] == attn[6:8]
        assert a[-4:-1] == attn[-5:-2]
    # every block by default
    every, (maps, _) = _trace(calls, lambda: eng.attention_maps(x, rows=rows))
    assert sorted(maps) == list(range(cfg["depth"])) and [n for n, _ in every].count(entry) == cfg["depth"]


def test_no_layers_is_the_plain_forward(calls):
    eng, _ = _engine()
    x = torch.zeros(2, 3, 224, 224)
    full, _ = _trace(calls, lambda: eng.forward(x))
    got, (maps, scale) = _trace(calls, lambda: eng.attention_maps(x, layers=[]))
    assert maps == {} and scale == 2.0 ** -7 and got == full
    # and the forward, the taps and the pruned tail never launch the entry
    for run in (lambda: eng.forward(x), lambda: eng.forward(x, taps={}), lambda: eng.forward(x, cls_tail=True), lambda: eng._graph_forward(x)):
        assert not [n for n, _ in _trace(calls, run)[0] if n in PROBS]


def test_other_softmax_widths_and_bad_arguments_are_refused(calls):
    eng, _ = _engine("deit_tiny_w16", stream_bits=16, softmax_bits=16, pos_bits=16)
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(ValueError, match="16 bits"):
        eng.attention_maps(x)
    assert not calls or all(n not in PROBS for n, _ in calls)
    eng, cfg = _engine()
    with pytest.raises(ValueError, match="rows"):
        eng.attention_maps(x, rows="first")
    with pytest.raises(ValueError, match="layers"):
        eng.attention_maps(x, layers=[cfg["depth"]])
