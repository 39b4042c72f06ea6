// isqrt.h -- IBERTIntLayerNorm.integer_sqrt (ibert_modules.py:85-109), the use_int_sqrt = True form of std_int (:143).
//
// The reference runs, on a float32 tensor n:
//   mask = n > 0; n = clamp(n, min=0)                                          :90-93
//   bits = floor(log2(clamp(n, min=1))) + 1              (float32 log2)         :96
//   x = 2^ceil(bits / 2)                                 (int64)                :99
//   four times:  inv = floor(n / clamp(x, min=1));  x = floor((x + inv) / 2)   (float32 division and addition)   :102-104
//   result = int32(x) where mask, else 0                                        :106-109
// It is NOT floor(sqrt(n)): four steps can end on the upper value of a two-cycle (3 -> 2, 15 -> 4, 255 -> 16, 16777215 -> 4096), so the
// four literal float32 steps run here.  And `bits` is not the bit length: the float32 log2 of a value just below 2^E rounds up to E.
//
// bits without a device log2 (which need not be correctly rounded).  n = m 2^e, 1 <= m < 2, E = e + 1, m = 2 (1 - t) with
// t = d 2^-24, d = 2^23 - mantissa.  log2(n) = E - delta, delta = -log2(1 - t) = (t + t^2 / 2 + ...) / ln 2.  The correctly rounded
// float32 of it is E exactly when delta is below half the gap between E and the float32 in front of it, h = 2^(P - 24) with
// P = ceil(log2(E)) - 1 (E in (2^P, 2^(P+1)]: the gap in front of a power of two is half the one behind it).  That is
// d (1 + t / 2 + ...) < ln 2 * 2^P.  For every finite float32 P <= 6, so d <= 44, t < 3e-6 and the bracket moves the left side by less
// than 2e-4, while ln 2 * 2^P (0.35, 0.69, 1.39, 2.77, 5.55, 11.09, 22.18, 44.36) stays 0.09 or more away from an integer:
// the log2 rounds up  <=>  d <= floor(ln 2 * 2^P)  (no value of d for E <= 2; d <= 11 for E = 17 .. 32).
#pragma once

IVIT_DEV int ib_integer_sqrt(float n)
{
    if (!(n > 0.0f)) return 0;                                                   // :90, 109
    const unsigned u = (unsigned)__float_as_int(fmaxf(n, 1.0f));                // :96 clamp(min=1)
    const int E = (int)(u >> 23) - 126;                                          // floor(log2) + 1 of the exact value
    const int d = 0x800000 - (int)(u & 0x7fffffu);
    const int P = E <= 1 ? -1 : 31 - __builtin_clz((unsigned)(E - 1));
    const int dmax = (int)(0xB17217F7ull >> (32 - P));                           // floor(ln 2 * 2^P); 0xB17217F7 = floor(ln 2 * 2^32)
    const int bits = E + (d <= dmax ? 1 : 0);                                    // :96
    float x = __builtin_ldexpf(1.0f, (bits + 1) >> 1);                           // :99  2^ceil(bits / 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float inv = floorf(n / fmaxf(x, 1.0f));                            // :103
        x = floorf((x + inv) / 2.0f);                                            // :104
    }
    return (int)x;                                                               // :106
}

// std_int of ibert_modules.py:142-145 from the float32 row sum var_int
template <bool ISQ>
IVIT_DEV float ib_std_int(float var_int, float shift_pow2)
{
    if constexpr (ISQ) return (float)ib_integer_sqrt(var_int) * shift_pow2;      // :143
    else return floorf(sqrtf(var_int)) * shift_pow2;                             // :145
}
