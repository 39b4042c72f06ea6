"""Label propagation on the GPU: ivit_local_topk_i8, ivit_propagate_labels_f32 and propagate.TokenMemory against numpy
(tests/propagate_ref.py), exactly: indices as integers, floats by bit pattern."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.knn import knn_weights  # noqa: E402
from ivit_amd.propagate import TokenMemory  # noqa: E402

import knn_ref  # noqa: E402
import propagate_ref  # noqa: E402

DEV = "cuda:0"
TARGET, ZERO_TARGET = (1, 1), (3, 2)      # the target with a planted best row three columns away; the all-zero target


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached problems are read-only)


@functools.lru_cache(maxsize=None)
def problem(Gh, Gw, F, Cc):
    """(q, bank, rnorm): twin frames, a zero context row, a zero target, and the best row of TARGET just outside its window at radius 2"""
    rng = np.random.default_rng(1000 * Gh + 10 * F + Cc)
    hw = Gh * Gw
    q = rng.integers(-20, 21, size=(hw, Cc)).astype(np.int8)                # |dot| <= 1024 * 400 < 2^24
    bank = rng.integers(-20, 21, size=(F * hw, Cc)).astype(np.int8)
    if F > 1:
        bank[hw:2 * hw] = bank[:hw]                                         # equal scores in every window: order by row
    bank[2 * Gw + 3] = 0                                                    # rnorm 0, score +0 whatever the target
    q[ZERO_TARGET[0] * Gw + ZERO_TARGET[1]] = 0                             # ties with everything in its window
    bank[(F - 1) * hw + TARGET[0] * Gw + TARGET[1] + 3] = q[TARGET[0] * Gw + TARGET[1]]      # cosine 1, |dx| = 3
    for a in (q, bank):
        a.setflags(write=False)
    return q, bank, knn_ref.rnorm(bank)


@functools.lru_cache(maxsize=None)
def reference(Gh, Gw, F, Cc, radius, k):
    q, bank, rn = problem(Gh, Gw, F, Cc)
    return propagate_ref.local_topk(q, bank, rn, Gh, Gw, F, radius, k)


def corner(Gh, Gw, F, radius):
    return F * (min(radius, Gh - 1) + 1) * (min(radius, Gw - 1) + 1)


def raw_topk(qd, bd, rn, Gh, Gw, F, Cc, radius, k, splits):      # the entry itself on dense device operands -> (idx, score) as numpy
    need = C.c_int64(-1)
    _lib.call("ivit_local_topk_workspace_bytes", Gh, Gw, F, k, splits, C.byref(need))
    assert (need.value == 0) == (splits == 1)
    ws = torch.empty(max(need.value // 8, 1), dtype=torch.int64, device=DEV)
    idx = torch.full((Gh * Gw, max(k, 1)), -7, dtype=torch.int32, device=DEV)
    score = torch.full((Gh * Gw, max(k, 1)), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("ivit_local_topk_i8", _lib.ptr(qd), qd.stride(0), Gh, Gw, _lib.ptr(bd), bd.stride(0), F, Cc, _lib.ptr(rn), radius, k, splits,
              _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy()


CASES = [(g, F, r, Cc, s, min(5, corner(*g, F, r))) for g in ((5, 11), (9, 13)) for F in (1, 3) for r in (0, 2, 12) for Cc in (64, 1024)
         for s in (1, 2, 3) if s <= F] + [((9, 13), 3, 12, 64, s, 32) for s in (1, 3)]


@pytest.mark.parametrize("grid,F,radius,Cc,splits,k", CASES)
def test_local_topk_matches_the_masked_sort(grid, F, radius, Cc, splits, k):
    Gh, Gw = grid
    q, bank, rn = problem(Gh, Gw, F, Cc)
    ridx, rsc = reference(Gh, Gw, F, Cc, radius, k)
    planted = (F - 1) * Gh * Gw + TARGET[0] * Gw + TARGET[1] + 3
    assert (ridx[TARGET[0] * Gw + TARGET[1], 0] == planted) == (radius >= 3)      # what a missing mask gets wrong
    idx, score = raw_topk(dev(q), dev(bank), dev(rn), Gh, Gw, F, Cc, radius, k, splits)
    assert np.array_equal(idx, ridx), np.argwhere(idx != ridx)[:8]
    assert np.array_equal(knn_ref.bits(score), knn_ref.bits(rsc))


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 65])
def test_label_mix_matches_sequential_float32(K, k):
    Gh, Gw, F, Cc = 9, 13, 3, 64
    q, _, _ = problem(Gh, Gw, F, Cc)
    idx5, sc5 = reference(Gh, Gw, F, Cc, 2, 5)
    idx = np.ascontiguousarray(idx5[:, :k])
    w = np.exp(knn_ref.cosine(sc5, q)[:, :k] / np.float32(0.1)).astype(np.float32)
    w[7] = w[7, 0]                                                          # all-equal weights
    seg = np.random.default_rng(K).random((F * Gh * Gw, K), dtype=np.float32)
    out = torch.full((Gh * Gw, K), float("nan"), dtype=torch.float32, device=DEV)
    di, dw, ds = dev(idx), dev(w), dev(seg)                                 # named: a temporary's memory would be the next upload's
    _lib.call("ivit_propagate_labels_f32", _lib.ptr(di), _lib.ptr(dw), Gh * Gw, k, _lib.ptr(ds), F * Gh * Gw, K, _lib.ptr(out), _lib.stream_ptr())
    assert np.array_equal(knn_ref.bits(out.cpu().numpy()), knn_ref.bits(propagate_ref.mix(idx, w, seg)))


def test_token_memory_propagates_end_to_end():
    Gh, Gw, F, Cc, K, radius, k, T = 5, 11, 3, 64, 3, 2, 5, 0.1
    hw = Gh * Gw
    q, bank, rn = problem(Gh, Gw, F, Cc)
    seg = np.random.default_rng(5).random((F * hw, K), dtype=np.float32)
    mem = TokenMemory(Gh, Gw, Cc, K, F, DEV)
    wide = torch.zeros(hw, 2 * Cc, dtype=torch.int8, device=DEV)
    for f in range(F):
        wide[:, :Cc] = dev(bank[f * hw:(f + 1) * hw])
        mem.put(f, wide[:, :Cc], dev(seg[f * hw:(f + 1) * hw]))             # a strided view
    assert np.array_equal(knn_ref.bits(mem.rnorm.cpu().numpy()), knn_ref.bits(rn))
    qd = torch.zeros(hw, Cc + 8, dtype=torch.int8, device=DEV)             # rows off the 16-byte grid: the wrapper copies them
    qd[:, :Cc] = dev(q)
    ridx, rsc = reference(Gh, Gw, F, Cc, radius, k)
    idx, cos = mem.neighbours(qd[:, :Cc], radius, k)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.array_equal(knn_ref.bits(cos.cpu().numpy()), knn_ref.bits(knn_ref.cosine(rsc, q)))
    w = knn_weights(cos, T).cpu().numpy()                                   # torch's exp, read back: the mix is then exact
    out = mem.propagate(qd[:, :Cc], radius, k, T)
    assert np.array_equal(knn_ref.bits(out.cpu().numpy()), knn_ref.bits(propagate_ref.mix(ridx, w, seg)))


def test_refusals():
    Gh, Gw, F = 5, 11, 2
    bd, qd = dev(np.ones((F * Gh * Gw, 1088), np.int8)), dev(np.ones((Gh * Gw, 1088), np.int8))
    rn = torch.ones(F * Gh * Gw, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.IvitError, match="1024"):
        raw_topk(qd, bd, rn, Gh, Gw, F, 1088, 2, 5, 1)
    with pytest.raises(_lib.IvitError, match="above 32"):
        raw_topk(qd, bd, rn, Gh, Gw, F, 64, 12, 33, 1)
    with pytest.raises(_lib.IvitError, match="corner"):
        raw_topk(qd, bd, rn, Gh, Gw, F, 64, 1, 9, 1)                        # F * 2 * 2 = 8 candidates
    with pytest.raises(_lib.IvitError, match="radius=-1"):
        raw_topk(qd, bd, rn, Gh, Gw, F, 64, -1, 1, 1)
    with pytest.raises(_lib.IvitError, match="splits=3"):
        raw_topk(qd, bd, rn, Gh, Gw, F, 64, 2, 5, 3)
    mem = TokenMemory(Gh, Gw, 64, 2, F, DEV)
    with pytest.raises(TypeError, match="int8"):
        mem.neighbours(torch.zeros(Gh * Gw, 64, device=DEV), 2, 5)
