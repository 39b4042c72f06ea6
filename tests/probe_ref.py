"""The numpy reference of the linear probe on the int8 feature bank (include/ivit_hip.h, "linear probe on an int8 feature bank";
ivit_amd/probe.py): Gram matrix, group sums, ridge, ncm, the integer logits of the head and its top-k rule.

gram() is a float64 dgemm on the converted rows.  That is EXACT here: every product is an integer of at most 2^14 in magnitude and
every partial sum of at most 2^31 of them an integer below 2^45 < 2^53, so no addition, in whatever order the BLAS makes them,
rounds.  gram_direct() is the same sum in int64, for the small cases tests/test_probe_cpu.py compares the two on."""
import numpy as np

from ivit_amd.prepare import LinearParams

f32 = np.float32


def gram(x):
    """int8 [rows, C] -> int64 [C, C], exact"""
    xf = np.asarray(x, np.int8).astype(np.float64)
    return (xf.T @ xf).astype(np.int64)


def gram_direct(x):
    xi = np.asarray(x, np.int8).astype(np.int64)
    return np.einsum("ri,rj->ij", xi, xi)


def csr(labels, groups):
    """labels [rows] -> (perm int32 [rows], group_ptr int64 [groups + 1]): the row indices grouped by class, stable"""
    labels = np.asarray(labels, np.int64)
    perm = np.argsort(labels, kind="stable").astype(np.int32)
    ptr = np.zeros(groups + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(labels, minlength=groups))
    return perm, ptr


def group_sums(x, perm, group_ptr):
    """-> int64 [groups, C]: sums[g] = the sum of the rows perm[group_ptr[g] : group_ptr[g + 1]]"""
    xi = np.asarray(x, np.int8).astype(np.int64)
    out = np.zeros((len(group_ptr) - 1, xi.shape[1]), np.int64)
    for g in range(len(group_ptr) - 1):
        out[g] = xi[np.asarray(perm[group_ptr[g]:group_ptr[g + 1]], np.int64)].sum(axis=0)
    return out


def stats(x, labels, K):
    """-> (G int64 [C, C], S int64 [K, C], n int64 [K])"""
    perm, ptr = csr(labels, K)
    return gram(x), group_sums(x, perm, ptr), np.diff(ptr)


def ridge_system(G, S, n, lam):
    """the system ridge solves, in float64 from the exact integers -> (A [C, C], R [C, K], mu [C], N)"""
    G, S, n = (np.asarray(v).astype(np.float64) for v in (G, S, n))
    C = G.shape[0]
    N = n.sum()
    if N == 0:
        raise ValueError("no rows")
    mu = S.sum(axis=0) / N
    sigma = G / N - np.outer(mu, mu)
    sigma = (sigma + sigma.T) / 2.0
    t = np.trace(sigma) / C
    if not t > 0.0:
        raise ValueError("all rows are equal")
    A = sigma + lam * t * np.eye(C)
    R = ((S - n[:, None] * mu[None, :]) / N).T
    return A, R, mu, N


def ridge(G, S, n, lam, scale):
    """-> (W float32 [K, C], b float32 [K], V float64 [C, K]): least squares onto one-hot targets with an intercept, in integer
    units; W = V^T / scale for features f = scale * x.  A class without rows gets a zero row."""
    A, R, mu, N = ridge_system(G, S, n, lam)
    nf = np.asarray(n).astype(np.float64)
    V = np.linalg.solve(A, R)
    a = nf / N - V.T @ mu
    V[:, nf == 0] = 0.0
    a[nf == 0] = 0.0
    return (V.T / np.float64(scale)).astype(f32), a.astype(f32), V


def ncm(S, n, scale):
    """-> (W float32 [K, C], b float32 [K]): W_k = (S_k / n_k) / |S_k / n_k| / scale, zero rows for empty or zero-mean classes"""
    S, n = np.asarray(S).astype(np.float64), np.asarray(n).astype(np.float64)
    m = S / np.maximum(n, 1.0)[:, None]
    norm = np.sqrt((m * m).sum(axis=1))
    W = np.where(norm[:, None] > 0, m / np.where(norm > 0, norm, 1.0)[:, None], 0.0) / np.float64(scale)
    return W.astype(f32), np.zeros(S.shape[0], f32)


def int_logits(q, W, b, scale):
    """the head as QuantLinear runs it: (acc int32 [Q, K], logits float32 [Q, K]) = (q W8^T + b32, fl32(float(acc) * s_acc))"""
    lp = LinearParams(np.asarray(W, f32), np.asarray(b, f32), scale)
    acc = np.asarray(q, np.int8).astype(np.int64) @ lp.W8.astype(np.int64).T + lp.b32.astype(np.int64)[None, :]
    assert np.abs(acc).max() < 2 ** 31
    acc = acc.astype(np.int32)
    return acc, (acc.astype(f32) * lp.s_acc[None, :].astype(f32)).astype(f32)


def topk(logits, k):
    """ivit_head_topk's rule -> int32 [Q, k]: value descending, equal values by ascending class (-0 == +0)"""
    return np.argsort(-(np.asarray(logits, f32) + f32(0.0)), axis=1, kind="stable")[:, :k].astype(np.int32)


def hits(top, targets):
    """-> int64 [k]: hits[r] = the rows whose target is their rank-r class"""
    return (np.asarray(top) == np.asarray(targets).reshape(-1, 1)).sum(axis=0).astype(np.int64)


def percentages(top, targets):
    h = hits(top, targets)
    n = max(len(targets), 1)
    return 100.0 * int(h[0]) / n, 100.0 * int(h.sum()) / n


def generator(seed=0, K=10, C=192, n_bank=4000, n_query=500, scale=0.0371):
    """the seeded clusters of the tests: K centres N(0, 12^2) in C dimensions, rows clip(rint(centre + N(0, 25^2)), -128, 127)
    -> (bank int8, labels, queries int8, targets, scale)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 12.0, size=(K, C))

    def draw(n):
        lab = rng.integers(0, K, size=n)
        return np.clip(np.rint(centres[lab] + rng.normal(0.0, 25.0, size=(n, C))), -128, 127).astype(np.int8), lab.astype(np.int64)
    bank, labels = draw(n_bank)
    q, targets = draw(n_query)
    return bank, labels, q, targets, scale
