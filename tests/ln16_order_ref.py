"""I-LayerNorm on 16-bit rows (IVITIntLayerNorm.forward, ivit_modules.py:30-65) with the two steps taken two ways, in numpy.

A row of 16-bit integers q carried at the scale s reaches the module as x = q * s; `x / scaling_factor` (:36) gives the float32
values phi(q) = fl(fl(q * s) / s) (the integers themselves at a power-of-two scale).  Two steps of the module depend on how they
are computed once the row is large:

  the mean (:37)      `x_int.mean(axis=2)` is a float32 sum.  Below 2^24 it is exact in any order; from there on it is
        "torch":  the value ATen's CPU kernel reaches in its order of additions (shiftmax_order_ref.torch_rowsum_batch);
        "exact":  the exact sum rounded to float32 once (RN24).
  the squares (:41)   `y_int ** 2` stays int32, so from |x - mean| = 46 341 on the square wraps:
        wrap=True:   the low 32 bits of the product, read as int32 (what torch computes);
        wrap=False:  the 64-bit square.
  The sum of the squares (:42) is int64 either way.

The reference is ("torch", wrap=True).  tests/golden/ln16_bigrows_kat.npz holds rows on which the candidates differ together with
the outputs of the reference module + its 8-bit QuantAct; nothing here reads the reference.  The QuantAct behind the LayerNorm is
taken from the CPU oracle (oracle.roundtrip / dyadic / requant): it is elementwise and not what these rows are about.

Row classes of the fixture (one per row, in this order of precedence):
    CLASS_W  max |x - mean| >= 46 341: a square wraps; both sums give the same mean
    CLASS_C  |sum| >= 2^24, the two sums give another mean_int and another int8 row
    CLASS_B  |sum| >= 2^24, the same mean_int from both sums
    CLASS_V  |sum| < 2^24, no wrap, built so that RN24(var) lies in or next to the band in which swin.hip's ln16_std10 runs the
             literal Newton loop (V_KIND says which)
    CLASS_A  control: |sum| < 2^24, no wrap
"""
import numpy as np

from oracle import oracle as orc
import shiftmax_order_ref as smo

CLASS_A, CLASS_B, CLASS_C, CLASS_W, CLASS_V = 0, 1, 2, 3, 4
CLASS_NAMES = {CLASS_A: "a", CLASS_B: "b", CLASS_C: "c", CLASS_W: "w", CLASS_V: "v"}
V_NONE, V_INSIDE, V_OUTSIDE, V_BOUNDARY = 0, 1, 2, 3      # class (v): inside the band, just outside it, on the 2^37 boundary
F32 = np.float32
WRAP_FROM = 46341                                          # 46 341^2 = 2 147 488 281 > 2^31 - 1 = 46 340^2 + 92 047
TILED_C = (768, 776, 1024, 1536)                           # swin.hip ln16_tiling takes these
OTHER_C = (772, 2048)                                      # ... and refuses these (C % 8, C > 1536)
V_BINADES_OTHER_C = (24, 30, 36, 39)                       # class (v) at the widths of OTHER_C (no shortcut in their kernels)
S_POW2 = F32(2.0 ** -10)
S_NATURAL = F32(0.000913)
SCALES = (S_POW2, S_NATURAL)


def xint_of(q, s):
    """:36 on the float view q * s (quant_modules.py:387)"""
    s = F32(s)
    return ((np.asarray(q).astype(F32) * s).astype(F32) / s).astype(F32)


def both_sums(xf):
    """-> (torch's float32 sum, RN24(exact sum)), each [N].  The exact sum in float64: every phi value is a float32 of magnitude
    below 2^16 and, unless zero, at least 0.5, so a multiple of 2^-24, and the sum stays below 2^27: 51 bits"""
    return smo.torch_rowsum_batch(xf), xf.astype(np.float64).sum(axis=-1).astype(F32)


def mean_int_of(S, C):
    return np.rint((np.asarray(S, F32) / F32(C)).astype(F32)).astype(np.int64)      # :37, round_ste: ties to even


def squares(d, wrap):
    """:41 on int64 differences |d| < 2^16"""
    sq = d * d
    return ((sq + (1 << 31)) % (1 << 32)) - (1 << 31) if wrap else sq


def newton10(varf):
    """:45-49, the ten float32 steps from k = 2^16"""
    varf = np.asarray(varf, F32)
    t = np.full(varf.shape, 65536.0, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(10):
            t = np.floor((t + np.floor(varf / t)) / F32(2.0)).astype(F32)
    return t


def std10_rule(varf):
    """swin.hip ln16_std10 restated: -> (slow, s).  Where `slow` is False the kernel returns s = floor(sqrt(varf)) for the ten
    Newton steps; where it is True the wave runs the literal loop.  varf: positive integers held in float32."""
    varf = np.asarray(varf, F32)
    v = varf.astype(np.float64)
    s = np.floor(np.sqrt(v))
    s = np.where(s * s > v, s - 1.0, s)
    s = np.where((s + 1.0) * (s + 1.0) <= v, s + 1.0, s)
    gap = (s + 1.0) * (s + 1.0) - v
    small = varf < F32(16777216.0)
    slow = np.where(small, (varf < F32(142883.0)) | (gap == 1.0), gap <= (varf * F32(2.0 ** -22)).astype(F32).astype(np.float64))
    return slow, s.astype(F32)


def ln_constants(C, gamma, beta):
    sf = F32(np.sqrt(F32(C))) / F32(2.0 ** 30)                                      # :32-33, :53
    gamma, beta = np.asarray(gamma, F32), np.asarray(beta, F32)
    bias_int = np.floor(((beta / gamma).astype(F32) / sf).astype(F32)).astype(F32)  # :56-57
    return bias_int, (sf * gamma).astype(F32)                                       # :62


def layernorm(q, s, gamma, beta, order="torch", wrap=True):
    """q [N, C] integers at scale s -> dict(y [N, C] float32 (:61), s_ln [C], mean_int, var (int64), maxd, S)"""
    xf = xint_of(q, s)
    C = xf.shape[1]
    St, Se = both_sums(xf)
    S = St if order == "torch" else Se
    mean_int = mean_int_of(S, C)
    d = np.trunc(xf).astype(np.int64) - mean_int[:, None]                           # :38-40
    var = squares(d, wrap).sum(axis=1)                                              # :41-42
    t = newton10(var.astype(F32))
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = np.floor(((F32(1.0) / t).astype(F32) * F32(2147483648.0)).astype(F32))      # :51  scalar / tensor = reciprocal * scalar
        v = np.floor(((d.astype(F32) * factor[:, None]).astype(F32) / F32(2.0)).astype(F32))  # :52
    bias_int, s_ln = ln_constants(C, gamma, beta)
    return dict(y=(v + bias_int).astype(F32), s_ln=s_ln, mean_int=mean_int, var=var, maxd=np.abs(d).max(axis=1), S=S)


def quantact8(y, s_ln, lo, hi):
    """the 8-bit QuantAct behind the LayerNorm with the fixed range (lo, hi): y * s_ln (:63) -> int8"""
    s_out = orc.sym_scale(lo, hi, 8)
    m, e = orc.dyadic(s_ln, s_out)
    return orc.requant(orc.roundtrip(y, s_ln), m, e, 8).astype(np.int8)


def candidates(q, s, gamma, beta, lo, hi):
    """-> {(order, wrap): int8 [N, C]} for the four combinations, and the reference-form intermediate dict"""
    out = {}
    ref = None
    for order in ("torch", "exact"):
        for wrap in (True, False):
            r = layernorm(q, s, gamma, beta, order, wrap)
            if order == "torch" and wrap:
                ref = r
            ok = r["var"] > 0
            o = np.zeros(r["y"].shape, np.int8)
            if ok.any():
                o[ok] = quantact8(r["y"][ok], r["s_ln"], lo, hi)
            out[(order, wrap)] = o
    return out, ref


def classify(q, s, gamma, beta, lo, hi):
    """-> (class [N] without the (v) tag: a, b, c or w; -1 outside the pinned domain (wrapped var_int <= 0, or a row on which both
    steps differ at once), candidates, the reference-form intermediates)"""
    cand, ref = candidates(q, s, gamma, beta, lo, hi)
    xf = xint_of(q, s)
    C = xf.shape[1]
    St, Se = both_sums(xf)
    isum = np.abs(xf.astype(np.float64).sum(axis=-1))
    mt, me = mean_int_of(St, C), mean_int_of(Se, C)
    big = isum >= 2.0 ** 24
    if np.array_equal(xf, np.rint(xf)):                     # integers (a power-of-two scale): exact in any order below 2^24
        assert np.array_equal(St[~big], Se[~big])
    cls = np.full(len(xf), CLASS_A, np.int64)
    cls[~big & (mt != me)] = -1                             # (a natural scale's phi values are no integers: any row can round)
    cls[big] = CLASS_B
    diff_out = np.any(cand[("torch", True)] != cand[("exact", True)], axis=1)
    cls[big & (mt != me) & diff_out] = CLASS_C
    cls[big & (mt != me) & ~diff_out] = -1                  # another mean that the 8-bit output does not show: not stored
    wraps = ref["maxd"] >= WRAP_FROM
    cls[wraps] = np.where(mt[wraps] == me[wraps], CLASS_W, -1)
    cls[ref["var"] <= 0] = -1
    return cls, cand, ref
