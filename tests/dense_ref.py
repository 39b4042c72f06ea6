"""The numpy reference of the dense linear probe (include/ivit_hip.h, "dense linear probe"; ivit_amd/dense.py): the exact bilinear
combination of the head's int32 accumulators, the float64 scores, the argmax with its tie rule, the confusion matrix and the patch
mode.  Plain and dense: a [K, H, W] int64 tensor per image."""
import numpy as np

# (batch, gh, gw, r, classes, np): every grid, factor, class count and batch of the specification at least once; 3 x 17 at r = 7 has
# rows of 119 bytes (byte stores), 2 x 33 a third chunk of one column whose halo is the clamped edge
CASES = [(1, 1, 1, 1, 1, 64), (1, 1, 1, 16, 2, 64), (3, 2, 3, 7, 19, 64), (1, 3, 17, 2, 150, 192), (1, 2, 33, 16, 19, 64),
         (3, 3, 17, 1, 255, 256), (1, 2, 3, 32, 255, 256), (1, 2, 33, 32, 2, 64), (3, 1, 1, 32, 150, 192), (1, 3, 17, 7, 150, 160),
         (1, 2, 33, 2, 1, 64)]


def taps(g, r):
    """one axis of g patches upsampled by r -> (i0 [g * r], i1 [g * r], f [g * r]): integer weights (2r - f, f) on (i0, i1)"""
    n = 2 * np.arange(g * r, dtype=np.int64) + 1 - r
    i0 = np.where(n < 0, 0, n // (2 * r))
    f = np.where(n < 0, 0, n % (2 * r))
    return i0, np.minimum(i0 + 1, g - 1), f


def interpolate(acc, r):
    """int [B, gh, gw, K] -> int64 [B, K, gh * r, gw * r]: I_k, exact"""
    a = np.asarray(acc).astype(np.int64).transpose(0, 3, 1, 2)
    _, _, gh, gw = a.shape
    y0, y1, fy = taps(gh, r)
    x0, x1, fx = taps(gw, r)
    rows = (2 * r - fy)[:, None] * a[:, :, y0, :] + fy[:, None] * a[:, :, y1, :]
    return (2 * r - fx) * rows[..., x0] + fx * rows[..., x1]


def scores(acc, s_acc, classes, r):
    """-> float64 [B, classes, H, W]: fl64(fl64(I_k) * fl64(s_acc[k]))"""
    I = interpolate(np.asarray(acc)[..., :classes], r)
    assert np.abs(I).max() < 2 ** 53
    return I.astype(np.float64) * np.asarray(s_acc, np.float32)[:classes].astype(np.float64)[None, :, None, None]


def argmax(acc, s_acc, classes, r):
    """-> uint8 [B, H, W]: the smallest class of maximal score"""
    return np.argmax(scores(acc, s_acc, classes, r), axis=1).astype(np.uint8)


def confusion(labels, target, classes, ignore_index=255):
    """-> int64 [classes, classes]: conf[t, p] over the pixels whose target is below classes and not ignore_index"""
    t, p = np.asarray(target).reshape(-1).astype(np.int64), np.asarray(labels).reshape(-1).astype(np.int64)
    keep = (t < classes) & (t != ignore_index)
    conf = np.zeros((classes, classes), np.int64)
    np.add.at(conf, (t[keep], p[keep]), 1)
    return conf


def patch_mode(target, r, classes, ignore_index=255):
    """uint8 [B, gh * r, gw * r] -> uint8 [B, gh, gw]: the most frequent valid class of a patch (ties to the lower class);
    ignore_index where fewer than half of its pixels are valid"""
    t = np.asarray(target)
    B, H, W = t.shape
    cells = t.reshape(B, H // r, r, W // r, r).transpose(0, 1, 3, 2, 4).reshape(B, H // r, W // r, r * r).astype(np.int64)
    valid = (cells < classes) & (cells != ignore_index)
    counts = np.stack([(valid & (cells == k)).sum(axis=-1) for k in range(classes)], axis=-1)
    return np.where(2 * valid.sum(axis=-1) < r * r, ignore_index, counts.argmax(axis=-1)).astype(np.uint8)


def margin(acc, s_acc, classes, r):
    """the smallest relative gap between the two largest scores of a pixel (inf with one class)"""
    if classes < 2:
        return np.inf
    s = np.sort(scores(acc, s_acc, classes, r), axis=1)
    return float(((s[:, -1] - s[:, -2]) / np.maximum(np.abs(s[:, -1]), np.abs(s[:, -2]))).min())


def random_case(seed, batch, gh, gw, classes, np_, lo=-2 ** 20, hi=2 ** 20):
    """seeded accumulators int32 [batch, gh, gw, np_] and scales float32 [np_]; the padding columns classes .. np_ - 1 hold 2^31 - 1
    under the largest scale: they would win every pixel if they were read"""
    rng = np.random.default_rng(seed)
    acc = rng.integers(lo, hi, size=(batch, gh, gw, np_)).astype(np.int32)
    s = rng.uniform(0.5, 2.0, size=np_).astype(np.float32) * np.float32(1e-4)
    acc[..., classes:] = 2 ** 31 - 1
    s[classes:] = 1.0
    return acc, s
