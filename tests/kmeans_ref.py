"""The integer statement of k-means on int8 rows (include/ivit_hip.h, "k-means on the int8 feature bank") in numpy int64."""
import numpy as np


def planes(c16):
    c16 = np.asarray(c16, np.int64)
    return (c16 >> 7).astype(np.int8), (c16 & 127).astype(np.int8)


def assign(x, c16):
    """-> (label int32 [N], dist int64 [N]): the k of smallest D = cnorm[k] - 256 dot(x, c16_k), equal D to the lower k"""
    x, c16 = np.asarray(x, np.int64), np.asarray(c16, np.int64)
    D = (c16 * c16).sum(axis=1)[None, :] - 256 * (x @ c16.T)
    label = D.argmin(axis=1)      # the first of equal minima
    return label.astype(np.int32), D[np.arange(len(x)), label] + 16384 * (x * x).sum(axis=1)


def update(S, n, c16):
    """-> (c16 int64 [K, C], changed int32 [K]): floor((256 S + n) / (2 n)) where n > 0 (numpy's // floors), the old row otherwise"""
    S, n, c16 = np.asarray(S, np.int64), np.asarray(n, np.int64), np.asarray(c16, np.int64)
    new = np.where(n[:, None] > 0, (256 * S + n[:, None]) // np.maximum(2 * n[:, None], 1), c16)
    return new, (new != c16).any(axis=1).astype(np.int32)


def fit(x, init, iters):
    """-> (label, c16, history, inertia) of the trajectory from the rows `init`"""
    x = np.asarray(x, np.int64)
    c16 = 128 * x[np.asarray(init)]
    history, changed = [], np.ones(1)
    for _ in range(iters):
        label, dist = assign(x, c16)
        history.append(int(dist.sum()))
        S = np.zeros_like(c16)
        np.add.at(S, label, x)
        c16, changed = update(S, np.bincount(label, minlength=len(c16)), c16)
        if not changed.any():
            break
    if changed.any():
        label, dist = assign(x, c16)
    return label, c16, history, int(dist.sum())
