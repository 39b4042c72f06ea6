"""k-NN evaluation on the int8 feature bank (include/ivit_hip.h, "k-NN evaluation on an int8 feature bank").

    bank, labels, scale = inference.extract_features(model, loader, device, integers=True)
    fb = FeatureBank(bank, labels, scale)
    idx, cos = fb.search(q_int8, k=20)                  # exact cosine neighbours, unique order
    classes, votes = knn_classify(fb, q_int8, k=20)     # weighted vote, w = exp(cos / T)

The bank stays int8 and is never copied; the similarity runs on the int8 MFMA and the selection in the kernel's epilogue, so no
[Q, N] score matrix exists.  The per-tensor scale of the rows cancels in a cosine: it is kept only so that queries under another
scale can be told apart by the caller (inference.evaluate_knn refuses them).  There is no fallback: a bank the kernels do not take
(float rows, C not a multiple of 64, rows not on 16-byte boundaries) raises."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

K_MAX = 256          # IVIT_KNN_K_MAX
SPLITS_MAX = 64      # IVIT_KNN_SPLITS_MAX


def _rows_ok(t, what):
    if t.dtype != torch.int8:
        raise TypeError(f"{what}: int8 integers wanted, got {t.dtype} -- extract the features with integers=True "
                        "(inference.extract_features(..., integers=True) returns the int8 rows and their scale)")
    if t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"{what}: a [rows, C] tensor on the device wanted, got shape {tuple(t.shape)} on {t.device}")
    c = int(t.shape[1])
    if c % 64 != 0 or not 64 <= c <= 1024:
        raise ValueError(f"{what}: C={c} is not a multiple of 64 between 64 and 1024")


def _aligned(t):
    return t.stride(1) == 1 and t.stride(0) % 16 == 0 and t.data_ptr() % 16 == 0


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
        _lib.call("ivit_knn_topk_i8", _lib.ptr(q), q.stride(0), Q, _lib.ptr(self.rows), self.rows.stride(0), self.N, self.C, _lib.ptr(self.rnorm),
                  k, splits, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(self.workspace) if need else None, need, st)
        _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(q), q.stride(0), Q, self.C, _lib.ptr(qnorm), st)
        return idx, score * qnorm[:, None]          # one more float32 product: the cosine

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
