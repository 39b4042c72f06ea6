"""Shiftmax (IVITIntSoftmax.forward, ivit_modules.py:164-176) with the row sum taken two ways, in numpy.

The exponents of a row are integers held in float32.  Their float32 sum is exact and order-free below 2^24; from 2^24 on the
reference's `exp_int.sum(dim=-1)` depends on the order in which torch's CPU kernel adds.  This module restates the operator
with both candidates for that sum

    "torch":  the partial sums of ATen's vectorised inner sum (8-float vectors x 4 accumulator rows, 4-level cascade),
              every addition rounded to float32;
    "exact":  the exact integer sum, rounded to float32 once (RN24),

so that a test can say which of the two a kernel took.  tests/golden/shiftmax_bigsum_kat.npz holds rows on which they differ,
together with the outputs of the reference module itself; nothing here reads the reference.

Row classes of the fixture:
    CLASS_A  sum >= 2^24 but order-free: every term a multiple of 2^g and the sum below 2^(24 + g)
    CLASS_B  torch's sum != RN24(exact sum), the outputs agree
    CLASS_C  the two sums give different outputs
"""
import numpy as np

CLASS_A, CLASS_B, CLASS_C = 0, 1, 2
CLASS_NAMES = {CLASS_A: "a", CLASS_B: "b", CLASS_C: "c"}
F32 = np.float32
TWO31 = F32(2147483648.0)


def phi_table(s):
    """phi_s(q) = fl(fl(q * s) / s), q = -128 .. 127: what Shiftmax's `x / scaling_factor` (:165) makes of an 8-bit score"""
    q = np.arange(-128, 128, dtype=F32)
    s = F32(s)
    return ((q * s).astype(F32) / s).astype(F32)


def x0_of(s):
    return F32(np.floor(F32(-1.0) / F32(s)))                         # :154


def shiftexp(d, x0, n=15):
    """int_exp_shift (:150-162) on d = x_int - max, float32 step by step"""
    d = np.asarray(d, F32)
    x0 = F32(x0)
    x = (d + np.floor(d / F32(2.0))) - np.floor(d / F32(16.0))         # :151
    x = np.maximum(x, F32(n) * x0)                                     # :155
    q = np.floor(x / x0)                                               # :157
    r = x - x0 * q                                                     # :158
    ex = r / F32(2.0) - x0                                             # :159
    ex = np.floor(ex * np.ldexp(F32(1.0), (n - q).astype(np.int32)).astype(F32))   # :160
    return np.maximum(ex, F32(0.0)).astype(F32)


def exponents(q, s):
    """q [..., T] int8 scores at scale s -> float32 exponents (:165-170)"""
    xi = phi_table(s)[np.asarray(q, np.int64) + 128]
    return shiftexp(xi - xi.max(axis=-1, keepdims=True), x0_of(s))


def torch_rowsum_batch(ef):
    """float32 sum over the last axis of ef [N, T] in the order of torch's CPU sum kernel, all N rows at once
    (the order of oracle/ivit_oracle.c ivo_torch_rowsum_f32, which tests check this against)"""
    ef = np.ascontiguousarray(ef, F32)
    N, n = ef.shape
    if n < 8:
        ps = np.zeros((N, 4), F32)
        m = n // 4
        for i in range(m):
            ps += ef[:, 4 * i:4 * i + 4]
        for i in range(4 * m, n):
            ps[:, 0] += ef[:, i]
        for k in range(1, 4):
            ps[:, 0] += ps[:, k]
        return ps[:, 0].copy()
    vec, = (n // 8,)
    ilp = vec // 4
    lp = max(4, int(np.ceil(np.log2(ilp))) // 4 if ilp > 1 else 4)
    step = 1 << lp
    acc = np.zeros((4, N, 32), F32)
    i = 0
    while i + step <= ilp:
        for _ in range(step):
            acc[0] += ef[:, 32 * i:32 * i + 32]
            i += 1
        for j in range(1, 4):
            acc[j] += acc[j - 1]
            acc[j - 1] = 0
            if i & ((step - 1) << (j * lp)):
                break
    while i < ilp:
        acc[0] += ef[:, 32 * i:32 * i + 32]
        i += 1
    for j in range(1, 4):
        acc[0] += acc[j]
    ps = acc[0]
    for i in range(4 * ilp, vec):
        ps[:, :8] += ef[:, 8 * i:8 * i + 8]
    for k in range(1, 4):
        ps[:, :8] += ps[:, 8 * k:8 * k + 8]
    fin = np.zeros(N, F32)
    for i in range(8 * vec, n):
        fin += ef[:, i]
    for l in range(8):
        fin += ps[:, l]
    return fin


def factor_of(S):
    S = np.minimum(np.asarray(S, F32), TWO31)                          # :173
    return np.floor((F32(1.0) / S).astype(F32) * TWO31).astype(F32)    # :174


def outputs(ef, S, output_bit):
    """:174-175 from the exponents ef [N, T] and the row sums S [N] -> int32 [N, T]"""
    f = factor_of(S)[:, None]
    return np.floor((ef * f).astype(F32) / F32(2.0 ** (31 - output_bit + 1))).astype(np.int32)


def both_sums(ef):
    """-> (torch's float32 sum, RN24(exact sum), exact sum as int64), each [N]"""
    isum = ef.astype(np.int64).sum(axis=-1)
    assert np.array_equal(ef.astype(np.int64).astype(F32), ef)
    return torch_rowsum_batch(ef), isum.astype(F32), isum            # int64 -> float32 rounds to nearest even: RN24


def order_free(ef, isum):
    """class (a)'s certificate: every term a multiple of 2^g and the sum below 2^(24 + g), so every partial sum of every order
    is a multiple of 2^g below 2^(24 + g), i.e. representable"""
    e = ef.astype(np.int64)
    g = np.zeros(len(e), np.int64)
    for k in range(1, 16):
        g[np.all(e % (1 << k) == 0, axis=-1)] = k
    return (isum >= 1 << 24) & (isum < (np.int64(1) << (24 + g)))


def classify(q, s, output_bit):
    """q [N, T] int8 -> (class [N] (-1: none of the three), out_torch, out_exact)"""
    ef = exponents(q, s)
    St, Se, isum = both_sums(ef)
    ot, oe = outputs(ef, St, output_bit), outputs(ef, Se, output_bit)
    cls = np.full(len(ef), -1, np.int64)
    diff_out = np.any(ot != oe, axis=-1)
    cls[order_free(ef, isum)] = CLASS_A
    cls[(St != Se) & ~diff_out] = CLASS_B
    cls[diff_out] = CLASS_C
    return cls, ot, oe
