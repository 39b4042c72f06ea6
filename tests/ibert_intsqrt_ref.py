"""numpy restatement of IBERTIntLayerNorm.integer_sqrt (the reference's ibert_modules.py:85-109) and of the LayerNorm around it, op for
op in float32 -- the reference of tests/test_ibert_intsqrt_cpu.py and tests/test_gpu_ibert_intsqrt.py, itself pinned against the
reference's own outputs in tests/golden/ibert_intsqrt_kat.npz.

`bits` = floor(log2(max(n, 1))) + 1 with the reference's FLOAT32 log2, restated without calling a log2: for n = m 2^e the correctly
rounded float32 log2 reaches E = e + 1 when n lies within floor(ln 2 * 2^P) float32 steps below 2^E, P = ceil(log2 E) - 1 (half the gap
between E and the float32 in front of it, in units of the derivative of log2 at 2^E; csrc/isqrt.h has the derivation)."""
import functools

import numpy as np

f32 = np.float32
LN2_Q32 = 0xB17217F7          # floor(ln 2 * 2^32)


def log2_bits(n):
    """floor(float32 log2(max(n, 1))) + 1 for a float32 array n"""
    u = np.maximum(np.asarray(n, f32), f32(1)).view(np.uint32).astype(np.int64)
    E = (u >> 23) - 126
    d = 0x800000 - (u & 0x7FFFFF)
    P = np.where(E <= 1, -1, np.ceil(np.log2(np.maximum(E, 1).astype(np.float64))).astype(np.int64) - 1)
    dmax = LN2_Q32 >> (32 - P)
    return E + (d <= dmax)


def integer_sqrt(n):
    """float32 array -> int32 array, :85-109"""
    n = np.asarray(n, f32)
    mask = n > 0                                                               # :90
    n = np.maximum(n, f32(0))                                                  # :93
    x = np.exp2(((log2_bits(n) + 1) // 2).astype(f32)).astype(f32)             # :96-99  2^ceil(bits / 2), exact
    for _ in range(4):
        inv = np.floor((n / np.maximum(x, f32(1))).astype(f32))                # :103
        x = np.floor(((x + inv).astype(f32) / f32(2)).astype(f32))             # :104
    return np.where(mask, x.astype(np.int64), 0).astype(np.int32)              # :106-109


def layernorm(x_int, bias_int, s_out, shift_pow2, mean_int=None, var_int=None, int_sqrt=True):
    """IBERTIntLayerNorm.forward (:129-156) on x_int = x / scaling_factor (float32 [rows, C]) -> the module's float32 output.
    The two row sums are taken in float64 and rounded: exact wherever they stay below 2^24; mean_int / var_int [rows, 1] override them
    (rows whose float32 sums depend on the order of the additions: the fixture holds torch's)."""
    x_int = np.asarray(x_int, f32)
    C = x_int.shape[-1]
    if mean_int is None:
        mean_int = np.rint((x_int.astype(np.float64).sum(-1, keepdims=True).astype(f32) / f32(C)).astype(f32))
    y = (x_int - mean_int).astype(f32)
    ys = np.floor((y / f32(shift_pow2)).astype(f32))
    if var_int is None:
        var_int = (ys * ys).astype(f32).astype(np.float64).sum(-1, keepdims=True).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = integer_sqrt(var_int).astype(f32) if int_sqrt else np.floor(np.sqrt(var_int).astype(f32))
        std_int = (root * f32(shift_pow2)).astype(f32)                         # :143 / :145
        factor = np.floor((f32(2.0 ** 31) / std_int).astype(f32))              # :146
        v = np.floor(((y * factor).astype(f32) / f32(2)).astype(f32))          # :147
        return ((v + np.asarray(bias_int, f32)).astype(f32) * np.asarray(s_out, f32)).astype(f32)


# ---------------------------------------------------------------------------------------------------------------- operator vectors
# Inputs by seed for tests/golden/ibert_intsqrt_ops.npz (scripts/make_ibert_intsqrt_golden.py stores what the reference's
# IBERTIntLayerNorm(use_int_sqrt=True) returns for them).  96 rows per case:
#   row 0        constant (var = 0 -> std = 0 -> factor = inf, 0 * inf = NaN, as the reference)
#   rows 1 ..    a few +-k entries on a constant row whose sum of squares is a chosen value of var_int: values where four Newton steps
#                end above isqrt (3, 15, 80, 255, ...), values just below a power of two where the float32 log2 rounds up (2^21 - 1,
#                2^22 - 1: the one where the result changes, 2^23 - 5, 2^24 - 11 ...), as far as the width and the element range allow;
#                below 2^24 var_int is that value exactly (power-of-two s_in), above it the float32 sum lands on or next to it
#   the rest     random rows of the set's magnitude
ROWS = 96
SETS = {            # name: (element bits, sigma of the random rows or None for +-full-scale rows, (power-of-two s_in, calibrated s_in))
    "q8": (8, 30.0, (2.0 ** -4, 0.0371)),          # var_int < 2^24
    "q8max": (8, None, (2.0 ** -4, 0.0371)),       # int8 at full scale: the largest var_int 8-bit rows reach (still below 2^24 for C <= 1024)
    "q16": (16, 1500.0, (2.0 ** -9, 1.37e-4)),     # var_int >= 2^24: the float32 sum depends on the order of the additions
}
CASES = [(C, name, shift_pow2, si) for C in (192, 384, 768, 1024) for name in SETS for shift_pow2 in (1, 4) for si in (0, 1)]


@functools.lru_cache(maxsize=None)
def hazard_targets():
    """values of var_int the special rows aim at, ascending"""
    import math
    t = [3, 15, 80, 255]
    for k in (64, 181, 1024, 2048, 2896, 4096, 5793, 8192, 11585, 16384, 23170):          # k^2 - 1 that do end above isqrt
        for kk in range(k, k + 40):
            v = kk * kk - 1
            if v < 2 ** 24 or v % 2 == 0:      # (odd values from 2^24 on are not float32 numbers)
                if int(integer_sqrt(np.array([v], f32))[0]) != math.isqrt(int(f32(v))):
                    t.append(v)
                    break
    t += [2 ** 21 - 1, 2 ** 22 - 1, 2 ** 23 - 5, 2 ** 24 - 11, 2 ** 24 - 1, 2 ** 26 - 12, 2 ** 28 - 11 * 16, 2 ** 30 - 5 * 64]
    return tuple(sorted(set(t)))


def _entries(T, kmax):
    """integers (+a, -a pairs, at most one 1) whose squares add up to T, |a| <= kmax"""
    import math
    out, rest = [], int(T)
    while rest >= 2:
        a = min(kmax, math.isqrt(rest // 2))
        out += [a, -a]
        rest -= 2 * a * a
    return out + [1] * rest


def make_case(case):
    """-> dict(q int32 [ROWS, C], s_in, gamma, beta, shift_pow2, targets {row: var_int aimed at})"""
    C, name, shift_pow2, si = case
    bits, sigma, scales = SETS[name]
    rng = np.random.default_rng([C, bits, int(sigma or 0), shift_pow2, si])
    lim = 2 ** (bits - 1) - 1
    if sigma is None:
        q = rng.choice(np.array([-lim - 1, lim]), size=(ROWS, C))
        q[ROWS // 2:] = np.clip(np.rint(rng.normal(0, 90, size=(ROWS - ROWS // 2, C))), -lim - 1, lim)
    else:
        q = np.clip(np.rint(rng.normal(0, sigma, size=(ROWS, C))), -lim - 1, lim)
    q = q.astype(np.int64)
    q[0] = 5
    targets, row = {}, 1
    base = 5
    for T in hazard_targets():
        g = 2 if T >= 2 ** 24 else 1             # even entries from 2^24 on: every partial sum of the squares is a float32 number
        if T % (g * g):
            continue
        e = _entries(T // (g * g), (lim - base) // (shift_pow2 * g))
        if len(e) > C - 8 or row >= ROWS // 3:
            continue
        r = np.full(C, base, np.int64)
        r[rng.permutation(C)[:len(e)]] += np.array(e, np.int64) * shift_pow2 * g
        q[row], targets[row] = r, T
        row += 1
    return dict(C=C, q=q.astype(np.int32), s_in=f32(scales[si]), shift_pow2=float(shift_pow2), targets=targets,
                gamma=rng.uniform(0.5, 1.5, size=C).astype(f32), beta=rng.uniform(-1, 1, size=C).astype(f32))


def case_key(case):
    return "c{}_{}_s{}_{}".format(*case)


def x_int_of(q, s_in):
    """what the module divides out: fl(fl(q * s) / s), :129"""
    s = f32(s_in)
    return ((np.asarray(q).astype(f32) * s).astype(f32) / s).astype(f32)


def layernorm_constants(gamma, beta):
    """bias_int[C], s_out[C] (:148-155)"""
    C = len(gamma)
    sf = f32(np.sqrt(f32(C)).astype(f32) / f32(2 ** 30))
    return np.floor(((beta / gamma).astype(f32) / sf).astype(f32)).astype(f32), (sf * gamma).astype(f32)


def row_crcs(y):
    import zlib
    return np.array([zlib.crc32(np.ascontiguousarray(r, f32).tobytes()) for r in y], np.uint32)
