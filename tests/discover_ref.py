"""Object discovery in plain numpy (include/ivit_hip.h, "object discovery on int8 patch tokens", steps 1 - 6), one image."""
import numpy as np


def affinity(tokens):
    """int8 [hw, C] -> d int64 [hw, hw].  The product runs in float64, where it is exact (|d| <= 1024 * 127^2 < 2^24 << 2^53)."""
    t = tokens.astype(np.float64)
    return (t @ t.T).astype(np.int64)


def discover(d, Gh, Gw, k):
    """d = affinity(tokens) -> (box (x0, y0, x1, y1), seed, deg int64 [hw], component bool [Gh, Gw])"""
    hw = Gh * Gw
    pos = d > 0
    np.fill_diagonal(pos, False)
    deg = pos.sum(axis=1)
    order = np.lexsort((np.arange(hw), deg))              # deg ascending, index ascending
    seed, potentials = int(order[0]), order[:min(k, hw)]
    similars = [p for p in potentials if p == seed or d[seed, p] > 0]
    M = d[similars].sum(axis=0)
    assert np.abs(M).max() < 2 ** 31
    mask = (M > 0).reshape(Gh, Gw)
    sy, sx = divmod(seed, Gw)
    comp = np.zeros((Gh, Gw), dtype=bool)
    comp[sy, sx] = True
    todo = [(sy, sx)] if mask[sy, sx] else []
    while todo:                                           # 4-connected
        y, x = todo.pop()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < Gh and 0 <= xx < Gw and mask[yy, xx] and not comp[yy, xx]:
                comp[yy, xx] = True
                todo.append((yy, xx))
    ys, xs = np.nonzero(comp)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())), seed, deg, comp


def row_words(comp):
    """bool [Gh, Gw] -> the component as row words, bit x of word y for the cell (y, x), as int64 bit patterns"""
    w = (comp.astype(np.uint64) << np.arange(comp.shape[1], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return w.view(np.int64)
