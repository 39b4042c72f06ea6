"""numpy reference of the label propagation contract (include/ivit_hip.h, "label propagation on int8 patch tokens"): knn_ref.scores,
the window as a boolean mask, per target np.lexsort((row, -(score + 0))) over the allowed rows; the label mix by sequential float32
loops."""
import numpy as np

import knn_ref


def window_mask(Gh, Gw, F, radius):
    """bool [Gh * Gw, F * Gh * Gw]: context token (f, y, x) is a candidate of target (ty, tx)"""
    y, x = np.divmod(np.arange(Gh * Gw), Gw)
    near = (np.abs(y[:, None] - y[None, :]) <= radius) & (np.abs(x[:, None] - x[None, :]) <= radius)
    return np.tile(near, (1, F))


def local_topk(q, bank, rn, Gh, Gw, F, radius, k):
    """-> (idx int32 [Gh * Gw, k], score float32 [Gh * Gw, k])"""
    s = knn_ref.scores(q, bank, rn)
    allowed = window_mask(Gh, Gw, F, radius)
    idx = np.empty((Gh * Gw, k), np.int32)
    for t in range(Gh * Gw):
        rows = np.flatnonzero(allowed[t])
        idx[t] = rows[np.lexsort((rows, -(s[t, rows] + np.float32(0))))[:k]]
    return idx, np.take_along_axis(s, idx.astype(np.int64), axis=1)


def mix(idx, w, seg):
    """-> float32 [T, K]: (sum_j w[t, j] * seg[idx[t, j]]) / sum_j w[t, j], both sums in rank order from 0, every step rounded"""
    T, k = idx.shape
    out = np.empty((T, seg.shape[1]), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            acc, sw = np.zeros(seg.shape[1], np.float32), np.float32(0)
            for j in range(k):
                acc = (acc + (np.float32(w[t, j]) * seg[idx[t, j]]).astype(np.float32)).astype(np.float32)
                sw = np.float32(sw + np.float32(w[t, j]))
            out[t] = acc / sw
    return out
