"""k-means on the int8 feature bank (include/ivit_hip.h, "k-means on the int8 feature bank").

    rows, targets, scale = inference.extract_features(model, loader, device, integers=True)
    km = KMeans(C, K, device)
    labels = km.fit(rows, iters=20, seed=0)            # int32 [N]; km.centroids, km.inertia, km.history
    partition_scores(labels, targets)                  # {"NMI", "ARI", "purity"}, float64 on the host

Lloyd's iteration with the centroids kept as int16 fixed point (7 fractional bits, c16 = 128 * centroid) in two int8 planes
hi = c16 >> 7 and lo = c16 & 127: the assignment is an exact integer argmin on the int8 MFMA (csrc/kmeans.hip), the sums are
ivit_group_sums_i8_i64 on the CSR form of the labels, the update is an integer division rounded half up.  No float copy of the bank
exists and a whole trajectory depends on the initial rows alone -- not on the tiling, not on the launch plan.  Equal distances go to
the lower centroid; an empty cluster keeps its centroid.  Patch tokens of forward_tokens(..., integers=True) [B, hw, C] go into
KMeans.fit directly after tokens.reshape(-1, C) (a codebook over patch tokens).  There is no fallback: anything the kernels do not
take raises IvitError with the offending value named, before anything is allocated."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import IvitError

K_MAX = 65536           # IVIT_KMEANS_K_MAX
C_MAX = 1024
FIT_ROWS_MAX = 1 << 22  # dist <= 2^40 per row: the inertia of more rows could pass 2^62


def _geometry(who, C, K):
    C, K = int(C), int(K)
    if C % 64 != 0 or not 64 <= C <= C_MAX:
        raise IvitError(f"{who}: C={C} is not a multiple of 64 between 64 and {C_MAX}")
    if not 1 <= K <= K_MAX:
        raise IvitError(f"{who}: K={K} outside [1, {K_MAX}]")
    return C, K


def _operands(who, rows, C, K=None):
    """-> N after the checks the entry would make (and K <= N for a fit), before anything is allocated"""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int8:
        raise IvitError(f"{who}: int8 integers wanted, got {getattr(rows, 'dtype', type(rows).__name__)} -- take the rows from "
                        "extract_features(..., integers=True)")
    if rows.dim() != 2 or int(rows.shape[1]) != C:
        raise IvitError(f"{who}: rows of shape [N, {C}] wanted, got {tuple(rows.shape)}")
    N = int(rows.shape[0])
    if N >= 2 ** 31:
        raise IvitError(f"{who}: N={N} rows outside [0, 2^31)")
    if K is not None and K > N:
        raise IvitError(f"{who}: K={K} above the N={N} rows")
    if N and (rows.stride(1) != 1 or rows.stride(0) % 16 or rows.stride(0) < C or rows.data_ptr() % 16):
        raise IvitError(f"{who}: misaligned rows: strides {tuple(rows.stride())} and address {rows.data_ptr():#x} (unit channel stride, row "
                        "stride and address multiples of 16 bytes)")
    if not rows.is_cuda:
        raise IvitError(f"{who}: rows on the device wanted, got {rows.device}")
    return N


class KMeans:
    """K centroids of C channels on `device`: the planes hi, lo int8 [K, C], cnorm int64 [K]; after fit() labels of the final
    assignment are returned, .inertia is their summed distance (a Python int, in units of 1 / 128^2 of the rows' integers squared),
    .history the inertia of every iteration's assignment."""

    def __init__(self, C, K, device):
        self.C, self.K = _geometry("KMeans", C, K)
        self.device = torch.device(device)
        self.hi = torch.zeros(self.K, self.C, dtype=torch.int8, device=self.device)
        self.lo = torch.zeros(self.K, self.C, dtype=torch.int8, device=self.device)
        self.cnorm = torch.zeros(self.K, dtype=torch.int64, device=self.device)
        self.inertia, self.history = None, []

    @property
    def c16(self):
        """int32 [K, C]: 128 * hi + lo"""
        return self.hi.to(torch.int32) * 128 + self.lo.to(torch.int32)

    @property
    def centroids(self):
        """float32 [K, C]: c16 / 128, in the rows' integer units"""
        return self.c16.to(torch.float32) / 128.0

    def init_from_rows(self, rows_int8, idx):
        """centroid k = bank row idx[k]: c16 = 128 * x, i.e. hi = x, lo = 0"""
        who = "KMeans.init_from_rows"
        N = _operands(who, rows_int8, self.C)
        idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
        if idx.numel() != self.K or (self.K and (int(idx.min()) < 0 or int(idx.max()) >= N)):
            raise IvitError(f"{who}: {idx.numel()} row indices for K={self.K} centroids, or one outside [0, {N})")
        x = rows_int8[idx.to(rows_int8.device)]
        self.hi.copy_(x)
        self.lo.zero_()
        self.cnorm.copy_((x.to(torch.int64) * 128).square().sum(dim=1))
        return self

    def fit(self, rows_int8, iters=20, init=None, seed=0):
        """Lloyd's iteration from the rows `init` (K row indices; default: the first K of torch.randperm(N) drawn on the CPU from a
        generator seeded with `seed`) until no centroid moves or `iters` iterations are done -> labels int32 [N] of the final
        assignment (after iters iterations without convergence: one more assignment against the last centroids)."""
        who = "KMeans.fit"
        iters = int(iters)
        if iters < 1:
            raise IvitError(f"{who}: iters={iters} below 1")
        N = _operands(who, rows_int8, self.C, self.K)
        if rows_int8.device != self.hi.device:
            raise IvitError(f"{who}: rows on {rows_int8.device}, centroids on {self.hi.device}")
        if N > FIT_ROWS_MAX:
            raise IvitError(f"{who}: N={N} rows above 2^22 (the inertia, up to 2^40 per row, could pass 2^62)")
        if init is None:
            init = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:self.K]
        self.init_from_rows(rows_int8, init)
        self.history = []
        moved = True
        for _ in range(iters):
            label, dist, changed = self._iterate(rows_int8, N)
            self.history.append(int(dist.sum()))
            moved = int(changed.sum()) != 0
            if not moved:
                break
        if moved:
            label, dist = _assign(rows_int8, N, self)
        self.inertia = int(dist.sum())
        return label

    def _iterate(self, rows, N):
        """one iteration on checked rows: assign, sums, update -> (label, dist, changed int32 [K]), nothing read back"""
        dev, st = rows.device, _lib.stream_ptr()
        label, dist = _assign(rows, N, self)
        # the CSR form of the labels, as BankStats.update builds it: row indices grouped by cluster (stable), the counts from its offsets
        long = label.to(torch.int64)
        perm = torch.sort(long, stable=True).indices.to(torch.int32)
        counts = torch.bincount(long, minlength=self.K)
        group_ptr = torch.zeros(self.K + 1, dtype=torch.int64, device=dev)
        group_ptr[1:] = torch.cumsum(counts, 0)
        sums = torch.empty(self.K, self.C, dtype=torch.int64, device=dev)
        changed = torch.empty(self.K, dtype=torch.int32, device=dev)
        _lib.call("ivit_group_sums_i8_i64", _lib.ptr(rows), rows.stride(0), N, self.C, _lib.ptr(perm), _lib.ptr(group_ptr), self.K, 0, _lib.ptr(sums), st)
        _lib.call("ivit_kmeans_update_i16", _lib.ptr(sums), _lib.ptr(counts), self.K, self.C, _lib.ptr(self.hi), _lib.ptr(self.lo),
                  _lib.ptr(self.cnorm), _lib.ptr(changed), st)
        return label, dist, changed


def _assign(rows, N, km):
    label = torch.empty(N, dtype=torch.int32, device=rows.device)
    dist = torch.empty(N, dtype=torch.int64, device=rows.device)
    _lib.call("ivit_kmeans_assign_i8", _lib.ptr(rows), rows.stride(0) if N else km.C, N, km.C, _lib.ptr(km.hi), _lib.ptr(km.lo), _lib.ptr(km.cnorm),
              km.K, _lib.ptr(label), _lib.ptr(dist), _lib.stream_ptr())
    return label, dist


def assign(rows_int8, km):
    """-> (label int32 [N], dist int64 [N]): per row the nearest centroid of km (equal distances: the lower index) and
    |128 * x - c16_label|^2 (ivit_kmeans_assign_i8)"""
    if not isinstance(km, KMeans):
        raise IvitError(f"assign: a KMeans wanted, got {type(km).__name__}")
    N = _operands("assign", rows_int8, km.C)
    if rows_int8.device != km.hi.device:
        raise IvitError(f"assign: rows on {rows_int8.device}, centroids on {km.hi.device}")
    return _assign(rows_int8, N, km)


def partition_scores(labels, targets):
    """-> {"NMI", "ARI", "purity"}: two partitions of the same items compared in float64 on the host from their int64 contingency
    table.  NMI = I(L; T) / ((H(L) + H(T)) / 2), natural logarithms (1.0 where both entropies are 0); ARI = the adjusted Rand index
    (1.0 where its denominator is 0: both partitions trivial); purity = the share of items in the majority target of their cluster."""
    l = np.asarray(torch.as_tensor(labels).detach().cpu()).astype(np.int64).reshape(-1)
    t = np.asarray(torch.as_tensor(targets).detach().cpu()).astype(np.int64).reshape(-1)
    if l.shape != t.shape or l.size == 0:
        raise ValueError(f"partition_scores: {l.size} labels for {t.size} targets")
    if l.min() < 0 or t.min() < 0:
        raise ValueError("partition_scores: a negative label")
    nt = int(t.max()) + 1
    table = np.bincount(l * nt + t, minlength=(int(l.max()) + 1) * nt).reshape(-1, nt)      # int64 [clusters, targets]
    n = int(table.sum())
    a, b = table.sum(axis=1), table.sum(axis=0)

    def entropy(m):
        p = m[m > 0].astype(np.float64) / n
        return float(-(p * np.log(p)).sum())

    i, j = np.nonzero(table)
    nij = table[i, j].astype(np.float64)
    mi = float((nij / n * (np.log(nij * n) - np.log(a[i].astype(np.float64) * b[j].astype(np.float64)))).sum())
    ha, hb = entropy(a), entropy(b)
    nmi = 1.0 if ha == 0.0 and hb == 0.0 else mi / ((ha + hb) / 2.0)
    pairs = lambda m: float((m.astype(np.float64) * (m.astype(np.float64) - 1.0) / 2.0).sum())      # noqa: E731
    sij, sa, sb, tot = pairs(table), pairs(a), pairs(b), n * (n - 1) / 2.0
    expected = sa * sb / tot if tot > 0 else 0.0
    denom = (sa + sb) / 2.0 - expected
    ari = 1.0 if denom == 0.0 else (sij - expected) / denom
    return {"NMI": nmi, "ARI": ari, "purity": float(table.max(axis=1).sum()) / n}
