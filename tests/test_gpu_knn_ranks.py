"""Retrieval ranks on the GPU: ivit_knn_ranks_i8 and FeatureBank.ranks against numpy (knn_ref.scores, per query
np.lexsort((index, -(s + 0))), a target's rank its position in that order), exactly: ranks as integers, scores by bit pattern."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.knn import FeatureBank  # noqa: E402

import knn_ref  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ref_ranks(q, bank, lists):      # -> (ranks, scores) in list order
    s, n = knn_ref.scores(q, bank), bank.shape[0]
    place = np.stack([np.argsort(np.lexsort((np.arange(n), -(s[i] + np.float32(0))))) for i in range(len(lists))])
    pairs = (np.repeat(np.arange(len(lists)), [len(t) for t in lists]), np.concatenate(lists).astype(np.int64))
    return place[pairs].astype(np.int32), s[pairs]


def raw_ranks(qd, bd, rn, tptr, tidx, splits, C_=None):      # the entry itself on dense device operands -> (rank, score) as numpy
    Q, N, nnz = qd.shape[0], bd.shape[0], len(tidx)
    need = C.c_int64(-1)
    _lib.call("ivit_knn_ranks_workspace_bytes", Q, N, nnz, splits, C.byref(need))
    ws = torch.empty(max(need.value // 8, 1), dtype=torch.int64, device=DEV)
    rank = torch.full((max(nnz, 1),), -7, dtype=torch.int32, device=DEV)
    score = torch.full((max(nnz, 1),), float("nan"), dtype=torch.float32, device=DEV)
    tp, ti = dev(np.asarray(tptr, np.int32)), dev(np.asarray(tidx, np.int32))
    _lib.call("ivit_knn_ranks_i8", _lib.ptr(qd), qd.stride(0), Q, _lib.ptr(bd), bd.stride(0), N, C_ or bd.shape[1], _lib.ptr(rn), _lib.ptr(tp), _lib.ptr(ti), nnz, splits, _lib.ptr(rank), _lib.ptr(score), _lib.ptr(ws), need.value, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rank.cpu().numpy()[:nnz], score.cpu().numpy()[:nnz]


def problem(Cc, N):
    """33 queries (two query tiles, the second with one live query), twin rows, a zero row, a zero query, and every kind of list"""
    rng = np.random.default_rng(100 * Cc + N)
    bank = rng.integers(-20, 21, size=(N, Cc)).astype(np.int8)      # |dot| <= 1024 * 400 < 2^24
    bank[40] = bank[7]                                              # equal scores: order by index
    bank[50] = 0                                                    # rnorm 0, score +0 whatever the query
    q = rng.integers(-20, 21, size=(33, Cc)).astype(np.int8)
    q[5] = 0                                                        # ties with every row
    order = np.argsort(-knn_ref.scores(q, bank), axis=1, kind="stable")
    lists = [rng.choice(N, size=int(rng.integers(1, 9)), replace=False) for _ in range(33)]
    lists[0] = np.zeros(0, np.int64)                                # an empty list
    lists[1] = np.array([order[1, N // 2]])                         # one target
    lists[2] = np.resize(np.arange(N), 256)                         # 256 targets (every row, most of them more than once)
    lists[3] = np.array([7, 40, 7, 50])                             # a duplicate, the twins, the zero row
    lists[4] = np.array([order[4, -1], 3])                          # the worst row: every score of the query takes the slow path
    lists[6] = np.array([order[6, 0]])                              # the best row: nothing passes the threshold
    lists[32] = np.array([order[32, 1], order[32, -2], 50])         # the live query of the second tile
    return q, bank, lists


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("N", [63, 193])
@pytest.mark.parametrize("Cc", [64, 1024])
def test_ranks_match_the_full_sort(Cc, N, splits):
    q, bank, lists = problem(Cc, N)
    rr, rs = ref_ranks(q, bank, lists)
    tptr = np.concatenate([[0], np.cumsum([len(t) for t in lists])])
    bd = dev(bank)
    rn = torch.empty(N, dtype=torch.float32, device=DEV)
    _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(bd), Cc, N, Cc, _lib.ptr(rn), _lib.stream_ptr())
    rank, score = raw_ranks(dev(q), bd, rn, tptr, np.concatenate(lists), splits)
    assert np.array_equal(rank, rr), np.flatnonzero(rank != rr)[:8]
    assert np.array_equal(knn_ref.bits(score), knn_ref.bits(rs))


def test_search_and_ranks_agree():
    rng = np.random.default_rng(7)
    bank, q = rng.integers(-128, 128, size=(1000, 128)).astype(np.int8), rng.integers(-128, 128, size=(5, 128)).astype(np.int8)
    fb = FeatureBank(dev(bank), torch.zeros(1000, dtype=torch.int32), 1.0)
    qd = dev(q)
    idx, cos = fb.search(qd, 256)
    ranks, scores, tptr = fb.ranks(qd, list(idx))
    assert np.array_equal(ranks.cpu().numpy().reshape(5, 256), np.tile(np.arange(256, dtype=np.int32), (5, 1)))
    qn = torch.from_numpy(knn_ref.rnorm(q)).to(DEV)
    assert torch.equal((scores.reshape(5, 256) * qn[:, None]).view(torch.int32), cos.view(torch.int32))


def test_wrapper_serves_a_list_of_300_in_pieces():
    rng = np.random.default_rng(8)
    bank, q = rng.integers(-128, 128, size=(400, 64)).astype(np.int8), rng.integers(-128, 128, size=(2, 64)).astype(np.int8)
    lists = [rng.permutation(400)[:300], np.array([399, 0])]
    fb = FeatureBank(dev(bank), torch.zeros(400, dtype=torch.int32), 1.0)
    ranks, scores, tptr = fb.ranks(dev(q), (np.array([0, 300, 302]), np.concatenate(lists)))      # the CSR form
    rr, rs = ref_ranks(q, bank, lists)
    assert np.array_equal(ranks.cpu().numpy(), rr) and np.array_equal(knn_ref.bits(scores.cpu().numpy()), knn_ref.bits(rs))


def test_refusals():
    bd, qd = dev(np.ones((300, 1088), np.int8)), dev(np.ones((1, 1088), np.int8))
    rn = torch.ones(300, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.IvitError, match="1024"):
        raw_ranks(qd, bd, rn, [0, 1], [0], 1)
    with pytest.raises(_lib.IvitError, match="at most 256 per query"):
        raw_ranks(qd, bd, rn, [0, 257], np.arange(257), 1, C_=64)
    fb = FeatureBank(bd[:, :64].contiguous(), torch.zeros(300, dtype=torch.int32), 1.0)
    with pytest.raises(ValueError, match="outside"):
        fb.ranks(qd[:, :64].contiguous(), [[299, 300]])
