"""numpy references of the video segmentation scoring, written from the specifications of include/ivit_hip.h ("video segmentation
scoring"): the exact float64 bilinear upsample + argmax, and the J / F counts of davis2017-evaluation without void pixels."""
import numpy as np


def _taps(G, r):
    n = np.maximum(2 * np.arange(G * r) + 1 - r, 0)
    y0, a1 = n // (2 * r), n % (2 * r)
    return y0, np.minimum(y0 + 1, G - 1), (2 * r - a1).astype(np.float64), a1.astype(np.float64)


def upsample_argmax(seg, Gh, Gw, r):
    """seg float32 [Gh * Gw, K] -> uint8 [Gh * r, Gw * r]: four exact products, three float64 additions in the header's order"""
    s = seg.reshape(Gh, Gw, -1).astype(np.float64)
    (y0, y1, ay0, ay1), (x0, x1, ax0, ax1) = _taps(Gh, r), _taps(Gw, r)

    def term(yy, ay, xx, ax):
        return (ay[:, None] * ax[None, :])[:, :, None] * s[yy][:, xx]

    v = (term(y0, ay0, x0, ax0) + term(y0, ay0, x1, ax1)) + (term(y1, ay1, x0, ax0) + term(y1, ay1, x1, ax1))
    return np.argmax(v, axis=2).astype(np.uint8)          # the first of equal maxima


def boundary(m):
    e, s, se = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    e[:, :-1], s[:-1, :], se[:-1, :-1] = m[:, 1:], m[1:, :], m[1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[-1, :], b[:, -1] = m[-1, :] ^ e[-1, :], m[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def dilate(b, R):
    H, W = b.shape
    out = np.zeros_like(b)
    for dy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
            if dx * dx + dy * dy <= R * R:      # out[y][x] |= b[y + dy][x + dx]
                out[max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)] |= b[max(dy, 0):H - max(-dy, 0), max(dx, 0):W - max(-dx, 0)]
    return out


def mask_scores(pred, truth, O, R):
    """uint8 [n, H, W] twice -> int64 [n, O, 6]: inter, union, n_fg, n_gt, fg_match, gt_match"""
    out = np.zeros((pred.shape[0], O, 6), np.int64)
    for f in range(pred.shape[0]):
        for o in np.intersect1d(np.union1d(pred[f], truth[f]), np.arange(1, O + 1)):
            mp, mt = pred[f] == o, truth[f] == o
            bp, bt = boundary(mp), boundary(mt)
            out[f, o - 1] = [(mp & mt).sum(), (mp | mt).sum(), bp.sum(), bt.sum(), (bp & dilate(bt, R)).sum(), (bt & dilate(bp, R)).sum()]
    return out


def blobs(rng, n, H, W, O):
    """label maps of a few random rectangles and disks per object; object 1 fills the top left corner, object O the bottom right"""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((n, H, W), np.uint8)
    for f in range(n):
        for o in range(1, O + 1):
            cy, cx, rad = rng.integers(-1, H + 1), rng.integers(-1, W + 1), rng.integers(1, max(2, min(H, W) // 3) + 1)
            out[f][(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = o
            y0, x0 = rng.integers(-2, H), rng.integers(-2, W)
            out[f, max(y0, 0):max(y0 + rng.integers(1, H // 2 + 2), 0), max(x0, 0):max(x0 + rng.integers(1, W // 3 + 2), 0)] = o
        out[f, :H // 4 + 1, :W // 5 + 1], out[f, H - H // 4 - 1:, W - W // 5 - 1:] = 1, O
    return out
