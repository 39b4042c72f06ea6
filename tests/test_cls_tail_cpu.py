"""The pruned last block of IntViTEngine (cls_tail) on the CPU, with the native library stubbed: which launches the eager forward, the
pruned forward and the graph hooks issue, and with which shapes.  (tests/test_engine_launch_trace.py pins every argument of the
eager forward; the results are compared on the GPU in tests/test_gpu_cls_tail.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine


@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(name, *args):
        if name == "ivit_ibert_softmax_build_table":      # engine.py reads the table back to choose the band form
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
    return IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=16, **kw), cfg


def _trace(calls, run):
    del calls[:]
    run()
    return list(calls)


# name -> index of the row count M in its argument list (include/ivit_hip.h)
ROWS = {"ivit_gemm_i8_requant_ex": 9, "ivit_gemm_i8_requant_residual_ex": 15, "ivit_shiftgelu_lut_i8_ex": 2, "ivit_layernorm_i8_ex": 2,
        "ivit_layernorm_i8_compat": 2}


@pytest.mark.parametrize("tag", ["deit_tiny", "deit_tiny_natural"])
@pytest.mark.parametrize("B", [2, 16])
def test_pruned_forward_replaces_the_last_block_only(calls, tag, B):
    eng, cfg = _engine(tag)
    assert eng.cls_tail_ok
    x = torch.zeros(B, 3, 224, 224)
    C, D, T = cfg["embed_dim"], cfg["depth"], eng.T
    M = B * T
    full = _trace(calls, lambda: eng.forward(x))
    cut = _trace(calls, lambda: eng.forward(x, cls_tail=True))
    per_block = 8                         # LN1, qkv, attention, proj, LN2, fc1, GELU, fc2
    head = len(full) - 3 - per_block      # stem + blocks 0 .. D-2: everything before the last block's first launch
    assert [n for n, _ in full[head:]][1:3] == ["ivit_gemm_i8_requant_qkv_ex", "ivit_attention_fused_i8_compat_band"]
    assert cut[:head] == full[:head], "the launches in front of the last block must not change"
    assert cut[head] == full[head]        # LN1 on every row
    tail = cut[head + 1:]
    ln1, ln2, ln_f = full[head][0], full[head + 4][0], full[-3][0]      # each site's form follows its input scale
    assert {ln1, ln2, ln_f} <= {"ivit_layernorm_i8_ex", "ivit_layernorm_i8_compat"}
    assert [n for n, _ in tail] == ["ivit_gemm_i8_requant_qkv_planes_ex", ln1, "ivit_gemm_i8_requant_ex", "ivit_attention_cls_i8",
                                    "ivit_gemm_i8_requant_residual_ex", ln2, "ivit_gemm_i8_requant_ex", "ivit_shiftgelu_lut_i8_ex",
                                    "ivit_gemm_i8_requant_residual_ex", ln_f, "ivit_gemm_i8_i32", "ivit_head_argmax"]
    # K and V for every token: planes 1 and 2, N = 2C, the weight / bias / requantisers from channel C on
    kv, qkv_full = tail[0][1], full[head + 1][1]
    assert kv[8:17] == (T, cfg["num_heads"], 64, 1, 2, M, 2 * C, C, qkv_full[14])
    assert kv[7] == qkv_full[7] and kv[0] == qkv_full[0]
    assert kv[2] - qkv_full[2] == C * C and [kv[i] - qkv_full[i] for i in (4, 5, 6)] == [4 * C] * 3
    # no full-size launch after it: every row-wise operator runs on the B class rows
    for name, args in tail[1:]:
        if name in ROWS:
            assert args[ROWS[name]] == B, (name, args[ROWS[name]])
    a = tail[3][1]
    assert a[4:9] == (C, B, cfg["num_heads"], T, 64) and a[1] - a[0] == M * C     # the K and V planes of the same buffer
    assert tail[1][1][1] == T * C and tail[4][1][8] == T * C                     # class rows read in place: ldx, ldr = T * C
    assert tail[2][1][10] == C and tail[6][1][10] == 4 * C and tail[8][1][16:18] == (C, 4 * C)
    # the eager forward, forward_topk and a taps request keep today's launches
    assert _trace(calls, lambda: eng.forward(x)) == full
    assert [n for n, _ in _trace(calls, lambda: eng.forward(x, taps={}))].count("ivit_attention_fused_i8_compat_band") == D
    assert [n for n, _ in _trace(calls, lambda: eng.forward_topk(x, k=5))][:-1] == [n for n, _ in full][:-1]
    # what the graph replays capture
    assert _trace(calls, lambda: eng._graph_forward(x)) == cut
    topk = _trace(calls, lambda: eng._graph_forward_topk(x, 5, None, None))
    assert topk[:-1] == cut[:-1] and topk[-1][0] == "ivit_head_topk"


@pytest.mark.parametrize("tag,kw", [("deit_tiny_ibert", dict(family="ibert")), ("deit_tiny_w16", dict(stream_bits=16))])
def test_other_engines_capture_the_full_forward(calls, tag, kw):
    eng, cfg = _engine(tag, **kw)
    assert not eng.cls_tail_ok
    x = torch.zeros(2, 3, 224, 224)
    full = _trace(calls, lambda: eng.forward(x))
    assert _trace(calls, lambda: eng._graph_forward(x)) == full
    assert "ivit_attention_cls_i8" not in [n for n, _ in full]
    with pytest.raises(ValueError, match="cls_tail"):
        eng.forward(x, cls_tail=True)


def test_long_rows_keep_the_full_tail(calls):
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    fs = dict(fs)
    fs["pos_embed"] = np.random.default_rng(577).normal(0, 0.02, size=(1, 577, cfg["embed_dim"])).astype(np.float32)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=2, img_size=384, patch_size=16)
    assert not eng.cls_tail_ok
    names = [n for n, _ in _trace(calls, lambda: eng._graph_forward(torch.zeros(2, 3, 384, 384)))]
    assert names.count("ivit_attention_fused_i8_long") == cfg["depth"] and "ivit_attention_cls_i8" not in names


def test_taps_and_pruned_tail_exclude_each_other(calls):
    eng, _ = _engine()
    with pytest.raises(ValueError, match="cls_tail"):
        eng.forward(torch.zeros(2, 3, 224, 224), taps={}, cls_tail=True)
