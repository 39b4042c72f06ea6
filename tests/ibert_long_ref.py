"""The specification of ivit_attention_fused_i8_ibert_long in numpy (shared by tests/test_attention_ibert_long_cpu.py,
tests/test_gpu_attention_ibert_long.py and scripts/find_rowsum_rows.py), and the crafted score rows for which the ORDER of the
float32 row sum decides the probabilities.

A crafted row (construction: `crafted_row`): one dominant key whose table entry x is free, a dozen near keys, the rest far away;
the table row is scaled so that the row sum sits at 2^30, where factor = floor(2^32 / S) is 4 for S <= 2^30 and 3 above.  x is then
searched (scripts/find_rowsum_rows.py) so that torch's sum and another order's sum fall on different sides: a quarter of every
probability hangs on the last bit of S."""
import numpy as np

from oracle import oracle as orc

TWO32 = np.float32(4294967296.0)


def synthetic_table(seed=0):
    """[256][256] float32, entry (row max + 128, q + 128): exp-like in the distance row max - q with a full-mantissa perturbation
    (the order of a sum matters), 0 beyond ~90 steps as the real table's saturated tail is constant; entry 16384 at distance 0
    for every third row maximum, so that a one-hot row gives p = 128.  Entries above the diagonal (q > row max) are never read."""
    rng = np.random.default_rng(1000 + seed)
    dist = np.arange(256)
    prof = np.floor(16384.0 * np.exp(-dist / 9.0))
    tab = np.zeros((256, 256), np.float32)
    for qm in range(256):
        d = qm - np.arange(qm + 1)
        v = prof[d] * (1.0 + rng.uniform(-1, 1, size=qm + 1) * 2.0 ** -12)
        tab[qm, :qm + 1] = v.astype(np.float32)
        if qm % 3 == 0:
            tab[qm, qm] = np.float32(16384.0)
    return tab


def sum_left_to_right(e):
    """(a) the plain float32 loop"""
    return np.cumsum(np.asarray(e, np.float32), dtype=np.float32)[-1]


def sum_lane_tree(e):
    """(b) what a kernel would do without care: key 16 kt + 4 g + r belongs to lane g of the query's four lanes; each lane adds its
    keys in register order (kt, then r), then a tree over the lanes: (s0 + s1) + (s2 + s3)"""
    e = np.asarray(e, np.float32)
    pad = np.zeros((-e.size) % 16, np.float32)
    x = np.concatenate([e, pad]).reshape(-1, 4, 4)
    s = [np.cumsum(x[:, g, :].reshape(-1), dtype=np.float32)[-1] for g in range(4)]
    return np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3]))


def probabilities(e, S):
    """ibert_modules.py:313-314 at output_bit 8: factor = floor(2^32 / S), p = floor(fl32(e * factor) / 2^25)"""
    e = np.asarray(e, np.float32)
    factor = np.floor(TWO32 / np.float32(S)).astype(np.float32)
    return np.floor((e * factor).astype(np.float32) / np.float32(2.0 ** 25)).astype(np.int32)


def row_probabilities(ka_row, tab, rowsum=orc.torch_rowsum):
    e = tab[int(ka_row.max()) + 128, ka_row.astype(np.int64) + 128].astype(np.float32)
    return probabilities(e, rowsum(e))


def expected(qkv, ms, es, mo, eo, tab, rowsum=orc.torch_rowsum):
    """-> (out int32 [B, T, H * 64], number of p == 128, largest |O|) of the whole attention: scores by the oracle's GEMM and
    requantisation, table lookup over (row max, q), row sum, factor, floor, P . V in int64, output requantisation"""
    _, B, H, T, hd = qkv.shape
    out = np.empty((B, T, H * hd), np.int32)
    n128, omax = 0, 0
    for b in range(B):
        for h in range(H):
            S = orc.gemm_i8(qkv[0, b, h], qkv[1, b, h])
            ka = orc.requant(S, ms.astype(np.float64), es, 8)
            E = tab[ka.max(axis=1)[:, None] + 128, ka + 128].astype(np.float32)
            P = np.empty((T, T), np.int32)
            for i in range(T):
                P[i] = probabilities(E[i], rowsum(E[i]))
            assert P.max() <= 128 and P.min() >= 0
            n128 += int((P == 128).sum())
            O = P.astype(np.int64) @ qkv[2, b, h].astype(np.int64)
            omax = max(omax, int(np.abs(O).max()))
            out[b, :, h * hd:(h + 1) * hd] = orc.requant(O.astype(np.int32), mo.astype(np.float64), eo, 8)
    return out, n128, omax


def cascade_class(T):
    """torch's row sum at 208 .. 1025 elements: T >> 5 interleaved steps in groups of 16 -> no full group, one, two"""
    return 0 if T < 512 else 1 if T < 1024 else 2


def crafted_row(T, seed, x_bits=None):
    """-> dict(t: int8 score row [T], qm: its maximum, pos: the dominant key, tabrow: float32 [256] = the table row of qm with the
    dominant key's entry (index qm + 128) set from x_bits, 0.0 when None).  Deterministic in (T, seed)."""
    rng = np.random.default_rng(seed * 100003 + T)
    qm = int(rng.integers(40, 100))
    dist = np.clip(30 + np.abs(rng.normal(0, 15, size=T)), 30, 255).astype(np.int64)
    near = rng.choice(T, size=13, replace=False)
    dist[near[1:]] = rng.integers(1, 7, size=12)
    pos = int(near[0])
    dist[pos] = 0
    dist = np.minimum(dist, qm + 128)                  # q >= -128
    t = (qm - dist).astype(np.int8)
    prof = np.exp(-np.arange(256) / 9.0) * (1.0 + rng.uniform(-1, 1, size=256) * 2.0 ** -3)
    rest = prof[dist].sum() - prof[0]
    scale = 0.6 * 2.0 ** 30 / rest                     # the other keys' exponents add up to about 0.6 * 2^30
    tabrow = np.zeros(256, np.float32)
    tabrow[qm + 128 - np.arange(qm + 129)] = (prof[:qm + 129] * scale).astype(np.float32)
    tabrow[qm + 128] = np.float32(0.0) if x_bits is None else np.array([x_bits], np.uint32).view(np.float32)[0]
    return dict(t=t, qm=qm, pos=pos, tabrow=tabrow)


def crafted_exponents(row):
    return row["tabrow"][row["t"].astype(np.int64) + 128].astype(np.float32)


# (T, seed, bits of the dominant key's table entry): found by scripts/find_rowsum_rows.py, one or two per cascade class; for every
# row the probabilities under torch's order differ from those under (a); CRAFTED_B lists the rows that also differ under (b)
CRAFTED = [(301, 1, 0x4dcccccc), (577, 0, 0x4dcccccf), (785, 0, 0x4dccccce), (1000, 1, 0x4dccccc8), (1024, 1, 0x4dccccc4),
           (1025, 2, 0x4dccccc9)]
CRAFTED_B = CRAFTED
