"""The float32 bracket certificate of the int8-output LayerNorm kernels (csrc/ln_chain.h, the bracket of csrc/common.h
ln_build_table) restated in numpy, so that a test can tell on the CPU which rows a kernel certifies and which it must redo
literally -- and feed the GPU rows of both kinds by construction (tests/test_gpu_ops.py test_layernorm_literal_tail_rows,
tests/test_gpu_swin.py test_layernorm_i16_literal_tail_rows)."""
import math

import numpy as np

from oracle import oracle as orc

EPS = 1.25 / 4194304.0      # 1.25 * 2^-22
KEEP_FAIL, KEEP_PASS, FLOOR = 18, 19, 16      # 37 rows: ragged for every group size of 2, 4, 8 and 16 rows


def bracket(m, e):
    """M = m * 2^-e -> (largest float32 <= M (1 - EPS), smallest float32 >= M (1 + EPS))"""
    M = np.ldexp(np.asarray(m, np.float64), -np.asarray(e, np.int64))
    lod, hid = M * (1.0 - EPS), M * (1.0 + EPS)
    lo, hi = lod.astype(np.float32), hid.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > lod, np.nextafter(lo, np.float32(-np.inf)), lo)
    hi = np.where(hi.astype(np.float64) < hid, np.nextafter(hi, np.float32(np.inf)), hi)
    return lo, hi


def failing_rows(y, m, e):
    """y [rows, C] float32 (the LayerNorm output before * s_ln) -> bool [rows]: some element's certificate fails.  The products
    of two float32 are exact in float64."""
    lo, hi = bracket(m, e)
    y = y.astype(np.float64)
    return (np.rint(y * lo.astype(np.float64)) != np.rint(y * hi.astype(np.float64))).any(axis=1)


def n_draw(C):
    """a plain draw fails about once per 1e5 elements: rows for ~48 failing ones"""
    return math.ceil(48 / (1e-5 * C))


def pick_rows(fail):
    """indices of the first KEEP_FAIL failing and KEEP_PASS passing rows, shuffled; at least FLOOR failing rows must exist"""
    f, p = np.nonzero(fail)[0], np.nonzero(~fail)[0]
    assert len(f) >= FLOOR and len(p) >= KEEP_PASS, (len(f), len(p))
    idx = np.concatenate([f[:KEEP_FAIL], p[:KEEP_PASS]])
    return idx[np.random.default_rng(len(idx)).permutation(len(idx))]


def s_out_pow2(y, s_ln, scale_out=0.8):
    return np.float32(2.0 ** np.ceil(np.log2(np.abs(y * s_ln).max() / 127 * scale_out)))


def draw_i8(Cn):
    """the rows of test_layernorm_certificate_regimes (mean per row ~ N(0, 20), sigma uniform in 0.5 .. 60), default_rng(Cn)
    -> k int8 [n_draw, Cn], gamma, beta"""
    rng = np.random.default_rng(Cn)
    rows = n_draw(Cn)
    k = np.clip(np.rint(rng.normal(rng.normal(0, 20, size=(rows, 1)), rng.uniform(0.5, 60, size=(rows, 1)), size=(rows, Cn))),
                -128, 127).astype(np.int8)
    return k, rng.uniform(0.5, 1.5, size=Cn).astype(np.float32), rng.normal(0, 0.1, size=Cn).astype(np.float32)


def draw_i16(C):
    """the draw of test_layernorm_i16_certificate_regimes (sigma per row uniform in 5 .. 6000), default_rng(C)"""
    rng = np.random.default_rng(C)
    rows = n_draw(C)
    x = np.clip(np.rint(rng.normal(0, rng.uniform(5, 6000, size=(rows, 1)), size=(rows, C))), -32768, 32767).astype(np.int16)
    return x, rng.uniform(0.5, 1.5, size=C).astype(np.float32), (rng.standard_normal(C) * 0.1).astype(np.float32)


def case(x, gamma, beta, layernorm=orc.layernorm):
    """-> (rows of x picked by pick_rows, s_out, expected int8 output of those rows, number of failing rows in the draw)"""
    y, s_ln, _ = layernorm(x.astype(np.int32), gamma, beta)
    s_out = s_out_pow2(y, s_ln)
    m, e = orc.dyadic(s_ln, s_out)
    fail = failing_rows(y, m, e)
    idx = pick_rows(fail)
    return x[idx], s_out, orc.requant(orc.roundtrip(y[idx], s_ln), m, e, 8), int(fail.sum())
