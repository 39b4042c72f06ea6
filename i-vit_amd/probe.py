"""Linear probe on the int8 feature bank (include/ivit_hip.h, "linear probe on an int8 feature bank").

    bank, labels, scale = inference.extract_features(model, loader, device, integers=True)
    stats = BankStats(C, num_classes, device)
    stats.update(bank, labels, scale)                   # or per batch; BankStats.from_bank(FeatureBank, num_classes)
    probe = stats.ridge(1e-2)                           # least squares onto one-hot targets, solved in float64 on the host
    acc, logits = probe.logits(q_int8)                  # the int8 head GEMM
    probe.load_into(model)                              # ... or inside model(x), at engine speed

Everything a closed-form linear classifier needs from the bank is a sum of integers: the Gram matrix, the per-class row sums and the
class counts.  The kernels compute them exactly on the int8 rows in place -- no float copy of the bank exists -- so they are unique
for any tiling and additive over batches and ranks.  The solve is a C x C problem on the host; its result becomes the integer
parameters of a QuantLinear head (prepare.LinearParams), so the probed classifier runs through the existing head GEMM and top-k
selection.  There is no fallback: rows the kernels do not take raise, as knn.FeatureBank's do."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .knn import FeatureBank, _aligned, _rows_ok
from .prepare import LinearParams, pad_head
from .topk import TOPK_MAX

GROUPS_MAX = 1 << 20      # IVIT_GROUPS_MAX


def _scale_of(scale):
    return None if scale is None else float(torch.as_tensor(scale).reshape(-1)[0])


class BankStats:
    """gram int64 [C, C] = X^T X, sums int64 [K, C] = the per-class row sums, counts int64 [K], on the device, and the rows' scale."""

    def __init__(self, C, num_classes, device):
        C, K = int(C), int(num_classes)
        if C % 64 != 0 or not 64 <= C <= 1024:
            raise ValueError(f"BankStats: C={C} is not a multiple of 64 between 64 and 1024")
        if not 1 <= K <= GROUPS_MAX:
            raise ValueError(f"BankStats: num_classes={K} outside [1, {GROUPS_MAX}]")
        self.C, self.K, self.device = C, K, torch.device(device)
        self.gram = torch.zeros(C, C, dtype=torch.int64, device=device)
        self.sums = torch.zeros(K, C, dtype=torch.int64, device=device)
        self.counts = torch.zeros(K, dtype=torch.int64, device=device)
        self.scale = None
        self.workspace = None

    def _check_scale(self, scale, who):
        s = _scale_of(scale)
        if s is not None and self.scale is not None and s != self.scale:
            raise ValueError(f"{who}: rows under scale {s!r} after rows under scale {self.scale!r}: not the same frozen model")
        return self.scale if s is None else s

    def update(self, rows_int8, labels, scale=None):
        """add a batch (or a whole bank) of int8 rows [n, C] with labels [n]; the rows are used in place.  scale: the rows' per-tensor
        scale (extract_features' third result); one that differs from the first raises."""
        who = "BankStats.update"
        _rows_ok(rows_int8, who)
        n = int(rows_int8.shape[0])
        if int(rows_int8.shape[1]) != self.C:
            raise ValueError(f"{who}: rows of {int(rows_int8.shape[1])} channels into statistics of {self.C}")
        if not _aligned(rows_int8):
            raise ValueError(f"{who}: rows must be contiguous in C and start on 16-byte boundaries (the rows are used in place)")
        if labels.shape != (n,):
            raise ValueError(f"{who}: {tuple(labels.shape)} labels for {n} rows")
        s = self._check_scale(scale, who)
        if n == 0:
            self.scale = s
            return self
        labels = labels.to(device=rows_int8.device, dtype=torch.int64)
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= self.K:
            raise ValueError(f"{who}: label {lo if lo < 0 else hi} outside [0, {self.K})")
        self.scale = s
        # the CSR form of the labels: row indices grouped by class (stable), and where each class starts
        perm = torch.sort(labels, stable=True).indices.to(torch.int32)
        counts = torch.bincount(labels, minlength=self.K)
        group_ptr = torch.zeros(self.K + 1, dtype=torch.int64, device=rows_int8.device)
        group_ptr[1:] = torch.cumsum(counts, 0)
        need = C.c_int64(0)
        _lib.call("ivit_gram_workspace_bytes", n, self.C, 0, C.byref(need))
        if self.workspace is None or self.workspace.numel() * 4 < need.value:
            self.workspace = torch.empty((need.value + 3) // 4, dtype=torch.int32, device=rows_int8.device)
        st = _lib.stream_ptr()
        _lib.call("ivit_gram_i8_i64", _lib.ptr(rows_int8), rows_int8.stride(0), n, self.C, 0, 1, _lib.ptr(self.gram), _lib.ptr(self.workspace),
                  need.value, st)
        _lib.call("ivit_group_sums_i8_i64", _lib.ptr(rows_int8), rows_int8.stride(0), n, self.C, _lib.ptr(perm), _lib.ptr(group_ptr), self.K, 1,
                  _lib.ptr(self.sums), st)
        self.counts += counts
        return self

    @classmethod
    def from_bank(cls, fb: FeatureBank, num_classes):
        """the statistics of a knn.FeatureBank (its rows in place, its labels, its scale)"""
        return cls(fb.C, num_classes, fb.rows.device).update(fb.rows, fb.labels, fb.scale)

    def merge(self, other):
        """add another BankStats (another shard of the same bank): int64 sums, exact"""
        if (other.C, other.K) != (self.C, self.K):
            raise ValueError(f"BankStats.merge: statistics of C={other.C}, K={other.K} into C={self.C}, K={self.K}")
        self.scale = self._check_scale(other.scale, "BankStats.merge")
        self.gram += other.gram.to(self.gram.device)
        self.sums += other.sums.to(self.sums.device)
        self.counts += other.counts.to(self.counts.device)
        return self

    def all_reduce(self):
        """sum the statistics over the ranks of the default process group (nothing without one): int64 sums, exact"""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            for t in (self.gram, self.sums, self.counts):
                dist.all_reduce(t)
        return self

    def _host(self, who):
        if self.scale is None:
            raise ValueError(f"{who}: the rows' scale is unknown (pass it to update)")
        G = self.gram.cpu().numpy().astype(np.float64)      # every integer here is below 2^53: exact
        S = self.sums.cpu().numpy().astype(np.float64)
        n = self.counts.cpu().numpy().astype(np.float64)
        if n.sum() == 0:
            raise ValueError(f"{who}: no rows")
        return G, S, n

    def ridge(self, lam):
        """-> LinearProbe: least squares onto one-hot targets with an intercept and the ridge lam * trace(Sigma) / C, in float64 on
        the host from the exact integers (integer units; W = V^T / scale for features f = scale * x)"""
        G, S, n = self._host("BankStats.ridge")
        W, b = ridge_solve(G, S, n, float(lam), self.scale)
        return LinearProbe(W, b, self.scale, self.device)

    def ncm(self):
        """-> LinearProbe: the class-mean (prototype) classifier, W_k = (S_k / n_k) / |S_k / n_k| / scale, b = 0"""
        G, S, n = self._host("BankStats.ncm")
        W, b = ncm_solve(S, n, self.scale)
        return LinearProbe(W, b, self.scale, self.device)


def ridge_solve(G, S, n, lam, scale):
    """float64 G [C, C], S [K, C], n [K] (exact integers) -> (W float32 [K, C], b float32 [K])"""
    Cc = G.shape[0]
    N = n.sum()
    mu = S.sum(axis=0) / N
    sigma = G / N - np.outer(mu, mu)
    sigma = (sigma + sigma.T) / 2.0
    t = np.trace(sigma) / Cc
    if not t > 0.0:
        raise ValueError("BankStats.ridge: all rows are equal (trace of the covariance is 0)")
    A = sigma + lam * t * np.eye(Cc)
    R = ((S - n[:, None] * mu[None, :]) / N).T              # [C, K]
    V = np.linalg.solve(A, R)
    a = n / N - V.T @ mu
    empty = n == 0
    V[:, empty] = 0.0
    a[empty] = 0.0
    return (V.T / np.float64(scale)).astype(np.float32), a.astype(np.float32)


def ncm_solve(S, n, scale):
    """float64 S [K, C], n [K] -> (W float32 [K, C], b float32 [K]); a class without rows or with a zero mean gets a zero row"""
    m = S / np.maximum(n, 1.0)[:, None]
    norm = np.sqrt((m * m).sum(axis=1))
    W = np.where(norm[:, None] > 0, m / np.where(norm > 0, norm, 1.0)[:, None], 0.0) / np.float64(scale)
    return W.astype(np.float32), np.zeros(S.shape[0], np.float32)


class LinearProbe:
    """float32 W [K, C], b [K] for features under `scale`, and their integer form -- prepare.LinearParams(W, b, scale), the rule
    QuantLinear applies: W8, b32, s_acc -- on the device, padded for the head GEMM (prepare.pad_head)."""

    def __init__(self, W, b, scale, device):
        self.W, self.b, self.scale = np.asarray(W, np.float32), np.asarray(b, np.float32), float(scale)
        self.K, self.C = self.W.shape
        self.params = LinearParams(self.W, self.b, self.scale)
        W8, b32, s_acc, _ = pad_head(self.params.W8, self.params.b32, self.params.s_acc)
        self.Np = W8.shape[0]
        self.device = torch.device(device)
        self.W8 = torch.from_numpy(np.ascontiguousarray(W8)).to(device)
        self.b32 = torch.from_numpy(np.ascontiguousarray(b32)).to(device)
        self.s_acc = torch.from_numpy(np.ascontiguousarray(s_acc)).to(device)

    def _acc(self, q_int8, who):
        _rows_ok(q_int8, who)
        if int(q_int8.shape[1]) != self.C:
            raise ValueError(f"{who}: queries of {int(q_int8.shape[1])} channels against a probe of {self.C}")
        q = q_int8 if _aligned(q_int8) else q_int8.contiguous()
        Q = int(q.shape[0])
        acc = torch.empty(Q, self.Np, dtype=torch.int32, device=q.device)
        if Q:
            _lib.call("ivit_gemm_i8_i32", _lib.ptr(q), q.stride(0), _lib.ptr(self.W8), self.C, _lib.ptr(self.b32), _lib.ptr(acc), self.Np, Q,
                      self.Np, self.C, _lib.stream_ptr())
        return acc

    def logits(self, q_int8):
        """-> (acc int32 [Q, K], logits float32 [Q, K]): the head's accumulators and fl32(float(acc) * s_acc)"""
        acc = self._acc(q_int8, "LinearProbe.logits")
        Q = int(acc.shape[0])
        out = torch.empty(Q, self.Np, dtype=torch.float32, device=acc.device)
        top1 = torch.empty(Q, dtype=torch.int32, device=acc.device)
        if Q:
            _lib.call("ivit_head_argmax", _lib.ptr(acc), _lib.ptr(self.s_acc), Q, self.Np, _lib.ptr(out), _lib.ptr(top1), _lib.stream_ptr())
        return acc[:, :self.K], out[:, :self.K]

    def topk(self, q_int8, k=5, targets=None, hits=None):
        """-> int32 [Q, k]: the k classes of largest logit, descending, equal logits by ascending class (ivit_head_topk).  targets
        int32 [Q] with hits int64 [k] (both or neither): hits[r] += the rows whose target is their rank-r class."""
        k = int(k)
        if not 1 <= k <= min(self.K, TOPK_MAX):
            raise ValueError(f"LinearProbe.topk: k={k} outside [1, min(classes={self.K}, {TOPK_MAX})]")
        if (targets is None) != (hits is None):
            raise ValueError("LinearProbe.topk: targets and hits go together")
        acc = self._acc(q_int8, "LinearProbe.topk")
        Q = int(acc.shape[0])
        if targets is not None:
            if targets.dtype != torch.int32 or targets.shape != (Q,) or not targets.is_contiguous():
                raise TypeError(f"LinearProbe.topk: targets must be a contiguous int32 tensor [{Q}]")
            if hits.dtype != torch.int64 or hits.shape != (k,) or not hits.is_contiguous():
                raise TypeError(f"LinearProbe.topk: hits must be a contiguous int64 tensor [{k}]")
        out = torch.empty(Q, k, dtype=torch.int32, device=acc.device)
        if Q:
            _lib.call("ivit_head_topk", _lib.ptr(acc), _lib.ptr(self.s_acc), Q, self.Np, self.K, k, None, _lib.ptr(out), _lib.ptr(targets),
                      _lib.ptr(hits), _lib.stream_ptr())
        return out

    def load_into(self, model):
        """copy W and b into model.head (a QuantLinear of [K, C]) in place: a frozen model then classifies with the probe in
        model(x) and evaluate_dataset -- the head's integer parameters and the engine are rebuilt from the new weights"""
        head = getattr(model, "head", None)
        w = getattr(head, "weight", None)
        if w is None or tuple(w.shape) != (self.K, self.C) or getattr(head, "bias", None) is None:
            raise ValueError(f"LinearProbe.load_into: model.head is not a linear layer of [{self.K}, {self.C}] with a bias")
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(self.W))
            head.bias.copy_(torch.from_numpy(self.b))
        return model
