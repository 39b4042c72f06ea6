"""Swin attention maps without a GPU.
  * The numpy specification of the window probabilities (tests/window_probs_ref.py) against the CPU restatements the window-attention
    kernels are already pinned to: its P, multiplied with V and requantised, is their output (test_gpu_swin.window_attention_ref for
    Shiftmax, test_gpu_window_attention_ibert.reference for I-BERT), and its three Shiftmax routes agree where more than one applies.
  * The prototypes of the two entries against the ctypes table, as tests/test_attention_probs_cpu.py does.
  * With the native library stubbed as in that file, the launches IntSwinEngine.attention_maps adds to the eager forward: exactly one
    behind the qkv GEMM of each selected block, nothing else moved; bad `blocks` raise before any launch.
(The probabilities themselves, and the hooks route of the model: tests/test_gpu_window_probs.py -- every operator needs the library.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc

import ivit_amd as ivit
from ivit_amd import _lib
from ivit_amd.swin_engine import IntSwinEngine, shift_mask_regions

import window_probs_ref as wp
from test_gpu_swin import window_attention_ref
from test_gpu_window_attention_ibert import SCALES as IBERT_SCALES, act_range, reference as ibert_reference
from test_swin_ibert_engine_cpu import fixture_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = ("ivit_window_attention_probs_u8", "ivit_window_attention_probs_u8_ibert")
f32 = np.float32


# ---------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("N,nH,nW,imgs,shifted", [(49, 3, 4, 2, True), (16, 1, 1, 3, False), (144, 3, 4, 1, True), (65, 1, 1, 2, False)])
def test_spec_times_v_is_the_shiftmax_window_attention(N, nH, nW, imgs, shifted):
    nwin = nW * imgs
    qkv, bias = wp.problem(N, nH, nwin, 31 * N + nH)
    s_S, s_at, s_A = f32(2.0 ** -12), f32(2.0 ** -2), f32(2.0 ** -3)
    region = None
    if shifted:
        ws = int(round(N ** 0.5))
        region = shift_mask_regions(2 * ws, 2 * ws, ws, ws // 2).astype(np.uint8)
    P = wp.probs("ivit", qkv, bias, region, nW, s_S, s_at, s_A, s_A)      # s_tab = s_A: the bias operand is the table itself
    mask_add = None
    if shifted:
        mval = int(f32(-100.0) / s_A)
        mask_add = np.where(region[:, :, None] != region[:, None, :], mval, 0).astype(np.int16)
    omO = orc.dyadic(f32(2.0 ** -7 * 0.05), f32(0.043))
    ref, kA, Pm = window_attention_ref(qkv[0], qkv[1], qkv[2], bias.astype(np.int16), mask_add, nW, orc.dyadic(s_S, s_at),
                                       orc.dyadic(s_at, s_A), s_A, omO)
    assert np.array_equal(P, Pm)
    O = np.einsum("bhqk,bhkd->bqhd", P.astype(np.int64), qkv[2].astype(np.int64)).astype(np.int32)
    assert np.array_equal(orc.requant(O.reshape(-1, wp.HD), omO[0], omO[1], 8).reshape(nwin, N, nH * wp.HD), ref)
    assert wp.one_hot_rows(P).any() and wp.near_flat_rows(P).any() and 0 <= P.min() and P.max() <= 127
    if shifted:
        assert (P[np.broadcast_to(wp.masked_pairs(region, nwin, nW), P.shape)] == 0).all()


@pytest.mark.parametrize("regime", ["pow2", "natural"])
@pytest.mark.parametrize("N,nH,nW,imgs,shifted", [(49, 3, 4, 1, True), (144, 1, 1, 2, False)])
def test_spec_times_v_is_the_ibert_window_attention(N, nH, nW, imgs, shifted, regime):
    sc = IBERT_SCALES[regime]
    s_S, s_at, s_A, s_tab, s_qkv, s_a3 = sc
    rng_act = act_range(s_A, regime)
    nwin = nW * imgs
    qkv, bias = wp.problem(N, nH, nwin, 17 * N + nH)
    region = None
    if shifted:
        ws = int(round(N ** 0.5))
        region = shift_mask_regions(2 * ws, 2 * ws, ws, ws // 2).astype(np.uint8)
    P = wp.probs("ibert", qkv, bias, region, nW, s_S, s_at, s_A, s_tab, rng_act)
    want, p = ibert_reference(qkv, bias, region, nW, sc, rng_act)
    assert np.array_equal(P, p) and 0 <= P.min() and P.max() <= 128
    O = np.einsum("whij,whjd->whid", P, qkv[2].astype(np.int64)).astype(np.int32)
    o = orc.requant(O, *orc.dyadic(f32(f32(2.0 ** -7) * f32(s_qkv)), s_a3), 8)
    assert np.array_equal(o.transpose(0, 2, 1, 3).reshape(nwin, N, nH * wp.HD).astype(np.int8), want)


@pytest.mark.parametrize("s_A", [2.0 ** -3, 0.271, 0.1173, 0.031])
def test_the_shiftmax_routes_of_the_spec_agree(s_A):
    """without a mask the float view is the integer route: oracle.shiftmax_xint on fl(fl(q * s) / s) equals oracle.shiftmax (power-of-two
    scale) / oracle.shiftmax_compat (natural scale) -- at 144 tokens with rows whose sum reaches 2^24"""
    qkv, bias = wp.problem(144, 1, 2, 5)
    ka = wp.scores(qkv, bias, f32(2.0 ** -12), f32(2.0 ** -2), f32(s_A), f32(2.0 ** -5))
    a = wp.shiftmax_probs(ka, s_A, None)
    b = orc.shiftmax_xint((wp.float_view(ka, s_A, None) / f32(s_A)).astype(f32), f32(s_A))
    assert np.array_equal(a, b) and a.max() > 8


# ---------------------------------------------------------------------------- prototypes
@pytest.mark.parametrize("name", PROBS)
def test_window_probs_prototypes_match_ctypes_table(name):
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "uint8_t*": _lib.vp, "const int16_t*": _lib.vp, "const uint8_t*": _lib.vp, "const uint32_t*": _lib.vp,
             "const float*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64, "uint32_t": _lib.u32, "int32_t": _lib.i32, "float": _lib.f32,
             "ivit_stream_t": _lib.vp}
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert _lib.SIGNATURES[name] == [kinds[re.sub(r"\s+\w+$", "", p)] for p in params]
    names = [re.findall(r"\w+", p)[-1] for p in params]
    shared = ["nwin", "windows_per_image", "heads", "tokens", "head_dim", "m_s", "e_s", "m_b", "e_b"]
    if name == PROBS[0]:
        assert names == ["qkv", "probs", "ldp", "bias", "region", "mask_value"] + shared + ["s_attn", "phi", "phim", "band", "band_w",
                                                                                            "band_rows", "stream"]
    else:
        assert names == ["qkv", "probs", "ldp", "bias", "region", "masked_exp"] + shared + ["table", "band_w", "stream"]
    if os.path.exists(_lib.LIB_PATH):          # built trees: the product and the lab library export it
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and hasattr(ctypes.CDLL(_lib.LAB_PATH), name)


# ---------------------------------------------------------------------------- the engine's launches, library stubbed
@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(name, *args):
        if name == "ivit_ibert_softmax_build_table":      # the spec reads the table back to choose the band form
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


def _engine(family):
    fs, ranges, shifts, args, kw = fixture_state()
    if family == "ibert":
        return IntSwinEngine({**fs, **shifts}, ranges, *args, family="ibert", **kw)
    return IntSwinEngine(fs, ranges, *args, **kw)


@pytest.mark.parametrize("family,entry", [("ivit", PROBS[0]), ("ibert", PROBS[1])])
def test_attention_maps_adds_one_launch_behind_the_qkv_gemm(calls, family, entry):
    eng = _engine(family)
    assert eng.depths == (2, 2) and eng.heads == (3, 6)
    B = 2
    x = torch.zeros(B, 3, eng.img_size, eng.img_size)
    full, _ = _trace(calls, lambda: eng.forward(x))
    sel = [(1, 0), (0, 1)]
    got, (maps, scale) = _trace(calls, lambda: eng.attention_maps(x, blocks=sel))
    assert scale == 2.0 ** -7 and list(maps) == sel
    shapes = {(0, 0): (B, 4, 3, 49, 49), (0, 1): (B, 4, 3, 49, 49), (1, 0): (B, 1, 6, 49, 49), (1, 1): (B, 1, 6, 49, 49)}
    for key, m in maps.items():
        assert m.dtype == torch.uint8 and tuple(m.shape) == shapes[key] and m.is_contiguous()
    where = [i for i, (n, _) in enumerate(got) if n in PROBS]
    assert len(where) == 2 and all(got[i][0] == entry for i in where)
    assert [c for i, c in enumerate(got) if i not in where] == full, "the forward's own launches must not change"
    qkv = [i for i, (n, _) in enumerate(got) if n == "ivit_gemm_i8_requant_qkv_ex"]
    assert len(qkv) == 4 and where == [qkv[1] + 1, qkv[2] + 1]           # blocks (0, 1) and (1, 0), in forward order
    for key, i in zip(((0, 1), (1, 0)), where):
        a = got[i][1]
        nW, nH = shapes[key][1], shapes[key][2]
        assert len(a) == len(_lib.SIGNATURES[entry])
        assert a[0] == got[i - 1][1][7], "the probabilities read the buffer the qkv GEMM wrote"
        assert a[1] == maps[key].data_ptr() and a[2] == 49 and a[6:11] == (B * nW, nW, nH, 49, 32)
        attn = got[i + 1]                      # the fused window attention behind it: the same operands, requantisers and tables
        assert attn[0].startswith("ivit_window_attention_i8") and a[0] == attn[1][0] and a[3:5] == attn[1][3:5]
        assert (a[4] is not None) == (key == (0, 1)), "only the shifted block has a region table"
        ms = attn[1].index(a[11], 6)
        assert a[11:15] == attn[1][ms:ms + 4]
    # every block by default; never in the plain forward, the taps, the feature maps or what the graphs capture
    every, (maps, _) = _trace(calls, lambda: eng.attention_maps(x))
    assert list(maps) == sorted(shapes) and [n for n, _ in every].count(entry) == 4
    none, (maps, _) = _trace(calls, lambda: eng.attention_maps(x, blocks=[]))
    assert maps == {} and none == full
    for run in (lambda: eng.forward(x), lambda: eng.forward(x, taps={}), lambda: eng.forward_intermediates(x)):
        assert not [n for n, _ in _trace(calls, run)[0] if n in PROBS]


def test_engine_refuses_bad_blocks_before_any_launch(calls):
    eng = _engine("ivit")
    x = torch.zeros(2, 3, eng.img_size, eng.img_size)
    del calls[:]
    for bad in ([(2, 0)], [(0, 2)], [(-1, 0)], [(0, 1), (0, 1)], [3], [(0, 0, 0)]):
        with pytest.raises(ValueError, match="blocks"):
            eng.attention_maps(x, blocks=bad)
    assert not calls


@pytest.fixture
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a library call before the arguments were validated")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(_lib, "lib", refuse)


def test_model_refuses_bad_blocks_and_other_softmax_widths_before_any_library_call(no_library):
    m = ivit.SwinTransformer(img_size=56, patch_size=4, embed_dim=96, depths=(2, 2), num_heads=(3, 6), window_size=7, num_classes=5).eval()
    x = torch.zeros(1, 3, 56, 56)
    for bad in ([(2, 0)], [(1, 2)], [(0, 0), (0, 0)]):
        with pytest.raises(ValueError, match="blocks"):
            m.attention_maps(x, blocks=bad)
    m.layers[1].blocks[0].attn.log_int_softmax.output_bit = 16
    with pytest.raises(ValueError, match="16 bits"):
        m.attention_maps(x)
