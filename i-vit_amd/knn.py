"""k-NN evaluation on the int8 feature bank (include/ivit_hip.h, "k-NN evaluation on an int8 feature bank").

    bank, labels, scale = inference.extract_features(model, loader, device, integers=True)
    fb = FeatureBank(bank, labels, scale)
    idx, cos = fb.search(q_int8, k=20)                  # exact cosine neighbours, unique order
    classes, votes = knn_classify(fb, q_int8, k=20)     # weighted vote, w = exp(cos / T)
    ranks, scores, tptr = fb.ranks(q_int8, targets)     # where listed rows stand in the full ranking (retrieval)
    ap, prec = retrieval_ap(ranks, tptr, is_positive)   # average precision per query, junk rows removed

The bank stays int8 and is never copied; the similarity runs on the int8 MFMA and the selection in the kernel's epilogue, so no
[Q, N] score matrix exists.  The per-tensor scale of the rows cancels in a cosine: it is kept only so that queries under another
scale can be told apart by the caller (inference.evaluate_knn refuses them).  There is no fallback: a bank the kernels do not take
(float rows, C not a multiple of 64, rows not on 16-byte boundaries) raises.  Rows of up to 1024 channels take the kernel that
splits the bank rows over a workgroup's waves, wider ones (to 4096: the pooled features of inference.extract_features(wide=True))
the one that splits the channels (ivit_knn_topk_i8_wide).
Retrieval: FeatureBank.ranks counts, in one more pass over the int8 bank (ivit_knn_ranks_i8, rows of up to 1024 channels), how many
rows precede each listed row in the search's order; retrieval_ap scores those ranks on the host ("Retrieval
ranks")."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

K_MAX = 256          # IVIT_KNN_K_MAX
SPLITS_MAX = 64      # IVIT_KNN_SPLITS_MAX
C_NARROW_MAX = 1024  # the widest rows of ivit_knn_topk_i8, ivit_gram_i8_i64 and ivit_group_sums_i8_i64
C_WIDE_MAX = 4096    # IVIT_KNN_C_WIDE_MAX: the widest rows of their _wide namesakes
RANK_TARGETS_MAX = 256  # IVIT_KNN_RANK_TARGETS_MAX: the longest list of one query row of ivit_knn_ranks_i8


def _rows_ok(t, what):
    if t.dtype != torch.int8:
        raise TypeError(f"{what}: int8 integers wanted, got {t.dtype} -- extract the features with integers=True "
                        "(inference.extract_features(..., integers=True) returns the int8 rows and their scale)")
    if t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"{what}: a [rows, C] tensor on the device wanted, got shape {tuple(t.shape)} on {t.device}")
    c = int(t.shape[1])
    if c % 64 != 0 or not 64 <= c <= C_WIDE_MAX:
        raise ValueError(f"{what}: C={c} is not a multiple of 64 between 64 and {C_WIDE_MAX}")


def _aligned(t):
    return t.stride(1) == 1 and t.stride(0) % 16 == 0 and t.data_ptr() % 16 == 0


def _target_lists(targets, Q, N, who):
    """targets -> (tptr int64 [Q + 1], tidx int64 [nnz]) as numpy, checked on the host: a (tptr, tidx) tuple, or Q index sequences"""
    def host(t):
        return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.int64).reshape(-1)
    if isinstance(targets, tuple) and len(targets) == 2:
        tptr, tidx = host(targets[0]), host(targets[1])
    else:
        lists = [host(t) for t in targets]
        tptr = np.concatenate([[0], np.cumsum([t.size for t in lists])]).astype(np.int64)
        tidx = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if tptr.size != Q + 1 or tptr[0] != 0 or (np.diff(tptr) < 0).any() or tptr[-1] != tidx.size:
        raise ValueError(f"{who}: target lists for {Q} queries wanted (tptr of {Q + 1} ascending offsets from 0 to len(tidx)={tidx.size})")
    if tidx.size and (tidx.min() < 0 or tidx.max() >= N):
        raise ValueError(f"{who}: a target index outside [0, N={N}) ({int(tidx.min())} .. {int(tidx.max())})")
    return tptr, tidx


def _chunked(tptr):
    """lists of more than RANK_TARGETS_MAX targets cut into pieces -> (qrow [Q'], tptr' [Q' + 1]): piece p is a list of query qrow[p]"""
    pieces = np.maximum(-(-np.diff(tptr) // RANK_TARGETS_MAX), 1)
    qrow = np.repeat(np.arange(tptr.size - 1), pieces)
    within = np.arange(qrow.size) - np.repeat(np.cumsum(pieces) - pieces, pieces)
    return qrow, np.concatenate([tptr[qrow] + RANK_TARGETS_MAX * within, tptr[-1:]])


class FeatureBank:
    """int8 rows [N, C] (a view, never a copy), their labels [N] and the rows' per-tensor scale.  rnorm = 1 / |row| is computed once."""

    def __init__(self, rows_int8, labels, scale):
        _rows_ok(rows_int8, "FeatureBank")
        if int(rows_int8.shape[0]) < 1:
            raise ValueError("FeatureBank: an empty bank")
        if not _aligned(rows_int8):
            raise ValueError("FeatureBank: rows must be contiguous in C and start on 16-byte boundaries (the bank is used in place)")
        if labels.shape != (rows_int8.shape[0],):
            raise ValueError(f"FeatureBank: {tuple(labels.shape)} labels for {int(rows_int8.shape[0])} rows")
        self.rows = rows_int8
        self.N, self.C = int(rows_int8.shape[0]), int(rows_int8.shape[1])
        self.labels = labels.to(device=rows_int8.device, dtype=torch.int32).contiguous()
        self.scale = None if scale is None else float(torch.as_tensor(scale).reshape(-1)[0])
        self.rnorm = torch.empty(self.N, dtype=torch.float32, device=rows_int8.device)
        self.workspace = None
        _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(self.rows), self.rows.stride(0), self.N, self.C, _lib.ptr(self.rnorm), _lib.stream_ptr())

    def _workspace(self, Q, k, splits):
        need = C.c_int64(0)
        _lib.call("ivit_knn_workspace_bytes", Q, self.N, k, splits, C.byref(need))
        if need.value and (self.workspace is None or self.workspace.numel() * 8 < need.value):
            self.workspace = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=self.rows.device)
        return need.value

    def search(self, q_int8, k, splits=0):
        """-> (idx int32 [Q, k], cos float32 [Q, k]): per query the k bank rows of largest cosine, descending, equal scores by
        ascending index.  splits: bank segments (0: chosen by the launcher); the result does not depend on it."""
        _rows_ok(q_int8, "FeatureBank.search")
        if int(q_int8.shape[1]) != self.C:
            raise ValueError(f"FeatureBank.search: queries of {int(q_int8.shape[1])} channels against a bank of {self.C}")
        k = int(k)
        if not 1 <= k <= self.N:
            raise ValueError(f"FeatureBank.search: k={k} outside [1, N={self.N}]")
        if k > K_MAX:
            raise ValueError(f"FeatureBank.search: k={k} above {K_MAX}")
        if not 0 <= splits <= SPLITS_MAX:
            raise ValueError(f"FeatureBank.search: splits={splits} outside [0, {SPLITS_MAX}]")
        q = q_int8 if _aligned(q_int8) else q_int8.contiguous()
        Q, dev = int(q.shape[0]), self.rows.device
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        score = torch.empty(Q, k, dtype=torch.float32, device=dev)
        qnorm = torch.empty(Q, dtype=torch.float32, device=dev)
        if Q == 0:
            return idx, score
        need = self._workspace(Q, k, splits)
        st = _lib.stream_ptr()
        _lib.call("ivit_knn_topk_i8" if self.C <= C_NARROW_MAX else "ivit_knn_topk_i8_wide", _lib.ptr(q), q.stride(0), Q, _lib.ptr(self.rows), self.rows.stride(0), self.N, self.C, _lib.ptr(self.rnorm),
                  k, splits, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(self.workspace) if need else None, need, st)
        _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(q), q.stride(0), Q, self.C, _lib.ptr(qnorm), st)
        return idx, score * qnorm[:, None]          # one more float32 product: the cosine

    def ranks(self, q_int8, targets, splits=0):
        """-> (ranks int32 [nnz], scores float32 [nnz], tptr int64 [Q + 1] on the host): for every listed bank row of every query its
        position in the query's full ranking of the bank, in search's order (0: the nearest row), and its score (search's, before
        the query norm).  targets: a list of Q index tensors / sequences (bank rows; any length, a row may repeat), or a tuple
        (tptr, tidx) of the same lists in CSR form; results are in list order.  Exact integers from one counting pass over the
        int8 bank (ivit_knn_ranks_i8): no sort, no [Q, N] matrix, no float copy.  A list longer than RANK_TARGETS_MAX is served in
        pieces against the same query row.  Rows wider than 1024 channels are refused."""
        who = "FeatureBank.ranks"
        if self.C > C_NARROW_MAX:
            raise ValueError(f"{who}: a bank of C={self.C} channels: the rank kernel takes rows of at most {C_NARROW_MAX} (there is no float path)")
        if not 0 <= splits <= SPLITS_MAX:
            raise ValueError(f"{who}: splits={splits} outside [0, {SPLITS_MAX}]")
        if q_int8.dim() != 2 or int(q_int8.shape[1]) != self.C:
            raise ValueError(f"{who}: queries of shape {tuple(q_int8.shape)} against a bank of {self.C} channels")
        tptr, tidx = _target_lists(targets, int(q_int8.shape[0]), self.N, who)
        _rows_ok(q_int8, who)
        dev, nnz = self.rows.device, int(tidx.size)
        rank = torch.empty(nnz, dtype=torch.int32, device=dev)
        score = torch.empty(nnz, dtype=torch.float32, device=dev)
        if nnz == 0:
            return rank, score, torch.from_numpy(tptr)
        qrow, tp = _chunked(tptr)
        q = q_int8 if qrow.size == tptr.size - 1 else q_int8[torch.from_numpy(qrow).to(dev)]
        q = q if _aligned(q) else q.contiguous()
        Q = int(q.shape[0])
        tp_d, ti_d = torch.from_numpy(tp.astype(np.int32)).to(dev), torch.from_numpy(tidx.astype(np.int32)).to(dev)
        need = C.c_int64(0)
        _lib.call("ivit_knn_ranks_workspace_bytes", Q, self.N, nnz, splits, C.byref(need))
        if self.workspace is None or self.workspace.numel() * 8 < need.value:
            self.workspace = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
        _lib.call("ivit_knn_ranks_i8", _lib.ptr(q), q.stride(0), Q, _lib.ptr(self.rows), self.rows.stride(0), self.N, self.C, _lib.ptr(self.rnorm),
                  _lib.ptr(tp_d), _lib.ptr(ti_d), nnz, splits, _lib.ptr(rank), _lib.ptr(score), _lib.ptr(self.workspace), need.value, _lib.stream_ptr())
        return rank, score, torch.from_numpy(tptr)

    def vote(self, idx, w, r):
        """-> (classes int32 [Q, r], votes float32 [Q, r]): the r labels of largest summed weight among each query's neighbours
        (sum in rank order), vote descending, equal votes by ascending label; (-1, 0.0) behind the distinct labels."""
        if idx.shape != w.shape or idx.dim() != 2:
            raise ValueError(f"FeatureBank.vote: idx {tuple(idx.shape)} and w {tuple(w.shape)}")
        Q, k = int(idx.shape[0]), int(idx.shape[1])
        if not 1 <= r <= k or k > K_MAX:
            raise ValueError(f"FeatureBank.vote: r={r} outside [1, k={k}] or k above {K_MAX}")
        idx = idx.to(torch.int32).contiguous()
        w = w.to(torch.float32).contiguous()
        classes = torch.empty(Q, r, dtype=torch.int32, device=idx.device)
        votes = torch.empty(Q, r, dtype=torch.float32, device=idx.device)
        if Q:
            _lib.call("ivit_knn_vote_f32", _lib.ptr(idx), _lib.ptr(self.labels), _lib.ptr(w), Q, self.N, k, r, _lib.ptr(classes), _lib.ptr(votes),
                      _lib.stream_ptr())
        return classes, votes


def knn_weights(cos, T):
    """the standard weights of a weighted k-NN vote: exp(cos / T), torch's float32 on the device (Q x k values, no hot path)"""
    return torch.exp(cos / T)


def knn_classify(bank, q_int8, k=20, T=0.07, r=5):
    """-> (classes [Q, r], votes [Q, r]): weighted k-NN vote of the queries against `bank` (a FeatureBank)"""
    idx, cos = bank.search(q_int8, k)
    return bank.vote(idx, knn_weights(cos, T), r)


def retrieval_ap(ranks, tptr, is_positive, junk=None, ks=(1, 5, 10)):
    """-> (ap float64 [Q], prec float64 [Q, len(ks)]): average precision and precision at ks per query from FeatureBank.ranks'
    output, float64 on the host.  is_positive / junk: bool [nnz] over the listed rows; junk=None: every listed row that is not a
    positive.  The revisited-Oxford rule: a junk row is taken out of the ranking, so a positive's adjusted rank is its rank minus the
    number of its query's junk rows ranked above it; a row that is neither stays where it is.  AP is the trapezoidal average
    precision of the original Oxford compute_ap: the n-th positive (from 0, by adjusted rank r) adds
    ((n / r if r else 1) + (n + 1) / (r + 1)) / 2 / n_pos.  Precision at k counts the positives of adjusted rank below
    kq = min(k, the last positive's adjusted rank + 1) and divides by kq.  A query without a positive gets nan (leave it out of a mean)."""
    r = np.asarray(ranks.cpu() if isinstance(ranks, torch.Tensor) else ranks, dtype=np.int64).reshape(-1)
    tp = np.asarray(tptr.cpu() if isinstance(tptr, torch.Tensor) else tptr, dtype=np.int64).reshape(-1)
    pos = np.asarray(is_positive.cpu() if isinstance(is_positive, torch.Tensor) else is_positive, dtype=bool).reshape(-1)
    jk = ~pos if junk is None else np.asarray(junk.cpu() if isinstance(junk, torch.Tensor) else junk, dtype=bool).reshape(-1)
    if not (r.size == pos.size == jk.size == tp[-1]) or (pos & jk).any():
        raise ValueError(f"retrieval_ap: {r.size} ranks, {pos.size} / {jk.size} flags for {int(tp[-1])} listed rows, or a row both positive and junk")
    Q = tp.size - 1
    ap, prec = np.full(Q, np.nan), np.full((Q, len(ks)), np.nan)
    for i in range(Q):
        sl = slice(tp[i], tp[i + 1])
        rp, rj = np.sort(r[sl][pos[sl]]), np.sort(r[sl][jk[sl]])
        if rp.size == 0:
            continue
        adj = (rp - np.searchsorted(rj, rp)).astype(np.float64)
        n = np.arange(rp.size, dtype=np.float64)
        before = np.where(adj > 0, n / np.maximum(adj, 1.0), 1.0)
        ap[i] = ((before + (n + 1.0) / (adj + 1.0)) / 2.0).sum() / rp.size
        for c, k in enumerate(ks):
            kq = min(float(k), adj[-1] + 1.0)
            prec[i, c] = (adj < kq).sum() / kq
    return ap, prec
