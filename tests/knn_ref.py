"""numpy reference of the k-NN contract (include/ivit_hip.h, "k-NN evaluation on an int8 feature bank"): integer dots in int64,
rnorm = float32(1) / sqrt(float32(n2)) (0 where n2 == 0), score = float32(dot) * rnorm in ONE float32 product, neighbours by
np.lexsort((index, -score)) -- score descending, equal scores (-0 == +0) by ascending index -- and a sequential float32 vote.
Comparisons are by bit pattern (`bits`), every element."""
import numpy as np


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def rnorm(rows):
    n2 = (rows.astype(np.int64) ** 2).sum(axis=1)
    f = n2.astype(np.float32)
    with np.errstate(divide="ignore"):
        r = np.float32(1) / np.sqrt(f)
    return np.where(n2 == 0, np.float32(0), r).astype(np.float32)


def scores(q, bank, rn=None):
    """float32 [Q, N]"""
    rn = rnorm(bank) if rn is None else rn
    dot = q.astype(np.int64) @ bank.astype(np.int64).T
    assert np.abs(dot).max(initial=0) <= 2 ** 24
    return (dot.astype(np.float32) * rn[None, :].astype(np.float32)).astype(np.float32)


def topk(q, bank, k, rn=None):
    """-> (idx int32 [Q, k], score float32 [Q, k])"""
    s = scores(q, bank, rn)
    Q, N = s.shape
    idx = np.empty((Q, k), np.int32)
    for i in range(Q):
        neg = -(s[i] + np.float32(0))                # -0 -> +0 first: equal under the float comparison, equal as sort keys
        idx[i] = np.lexsort((np.arange(N), neg))[:k]
    sc = np.take_along_axis(s, idx.astype(np.int64), axis=1)
    return idx, sc


def cosine(score, q):
    return (score * rnorm(q)[:, None]).astype(np.float32)


def topk_brute(q, bank, k):
    """the same by explicit loops and comparisons (tests/test_knn_cpu.py checks topk against it)"""
    rn = rnorm(bank)
    Q, N = q.shape[0], bank.shape[0]
    idx = np.empty((Q, k), np.int32)
    sc = np.empty((Q, k), np.float32)
    for i in range(Q):
        cand = []
        for j in range(N):
            d = sum(int(a) * int(b) for a, b in zip(q[i], bank[j]))
            cand.append((np.float32(np.float32(d) * rn[j]), j))
        chosen = []
        left = list(cand)
        for _ in range(k):
            best = left[0]
            for c in left[1:]:
                if c[0] > best[0] or (c[0] == best[0] and c[1] < best[1]):
                    best = c
            left.remove(best)
            chosen.append(best)
        idx[i] = [c[1] for c in chosen]
        sc[i] = [c[0] for c in chosen]
    return idx, sc


def vote(idx, labels, w, r):
    """-> (classes int32 [Q, r], votes float32 [Q, r]): per label the float32 sum of w in rank order from 0; the r largest, vote
    descending, equal votes by ascending label; (-1, 0) behind the distinct labels"""
    Q, k = idx.shape
    classes = np.full((Q, r), -1, np.int32)
    votes = np.zeros((Q, r), np.float32)
    for i in range(Q):
        acc = {}
        for n in range(k):
            l = int(labels[idx[i, n]])
            acc[l] = np.float32(acc.get(l, np.float32(0)) + np.float32(w[i, n]))
        order = sorted(acc.items(), key=lambda kv: (-float(kv[1]), kv[0]))[:r]
        for p, (l, v) in enumerate(order):
            classes[i, p], votes[i, p] = l, v
    return classes, votes
