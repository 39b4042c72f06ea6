"""numpy restatement of torch.quantile(x, q) for a 1-D float32 x with the default linear interpolation -- the formula the launcher of
ivit_quantile_pair_f32 and its last kernel implement (include/ivit_hip.h).  test_quantile_cpu.py pins it against torch.quantile bit
for bit; above torch's limit of 2^24 elements it is the only reference there is.  Every operation is one float32 rounding; the interpolation's product and sum are one (torch's lerp kernels fuse them)."""
import numpy as np

f32 = np.float32


def percentile_qs(p):
    """the reference's two q (quant_modules.py:325-329) as torch.quantile receives them, rounded to float32"""
    percentile_min = (100 - p) / 2
    percentile_max = 100 - percentile_min
    return f32(percentile_min / 100.0), f32(percentile_max / 100.0)


def ranks(n, q):
    """-> (lo, hi, w): indices of the two order statistics and the interpolation weight"""
    q = f32(q)
    nm1 = f32(n - 1)                                   # round to nearest; exact up to 2^24
    rank = f32(q * nm1)
    lo, hi = np.floor(rank), np.ceil(rank)
    w = f32(rank - lo)
    return min(int(lo), n - 1), min(int(hi), n - 1), w          # fl32(n - 1) can exceed n - 1 above 2^24


def fma32(x, y, z):
    """float32 fused multiply-add: x * y is exact in float64; the sum is rounded to odd there, which makes the final rounding to
    float32 the single rounding of the exact x * y + z (53 bits are more than 2 * 24 + 2)"""
    p, z = float(f32(x)) * float(f32(y)), float(f32(z))
    s = p + z
    if not np.isfinite(s):
        return f32(s)
    bb = s - p
    err = (p - (s - bb)) + (z - bb)                    # TwoSum: p + z == s + err exactly
    if err != 0.0 and (np.float64(s).view(np.int64) & 1) == 0:
        s = float(np.nextafter(s, np.inf if err > 0 else -np.inf))
    return f32(s)


def lerp(a, b, w):
    """torch's lerp: the product and the sum of either branch are one fused multiply-add in its kernels"""
    a, b, w = f32(a), f32(b), f32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f32(b - a)
        if w < f32(0.5):
            return fma32(w, d, a)
        return fma32(-d, f32(f32(1.0) - w), b)


def quantile(x, q):
    """torch.quantile(x, q) of a 1-D float32 array; np.partition selects, nothing is sorted"""
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1)
    if np.isnan(x).any():
        return f32(np.nan)
    lo, hi, w = ranks(x.size, q)
    part = np.partition(x, sorted({lo, hi}))
    return lerp(part[lo], part[hi], w)


def quantile_pair(x, q_lo, q_hi):
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1)
    if np.isnan(x).any():
        return f32(np.nan), f32(np.nan)
    (l0, h0, w0), (l1, h1, w1) = ranks(x.size, q_lo), ranks(x.size, q_hi)
    part = np.partition(x, sorted({l0, h0, l1, h1}))
    return lerp(part[l0], part[h0], w0), lerp(part[l1], part[h1], w1)


def same_bits(a, b):
    """bitwise equal float32 values, except that a zero may carry either sign and any NaN equals any NaN"""
    a, b = np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1)
    eq = a.view(np.int32) == b.view(np.int32)
    return bool(np.all(eq | ((a == 0) & (b == 0)) | (np.isnan(a) & np.isnan(b))))
