"""Shiftmax rows whose exponent sum reaches 2^24 (tests/golden/shiftmax_bigsum_kat.npz: the reference module's own outputs on
crafted rows, oracle/gen_golden.py gen_shiftmax_bigsum), on the host: the fixture holds what it must hold, the numpy restatement
of tests/shiftmax_order_ref.py reproduces both stored candidates and the class of every row, and the two CPU oracles give the
reference's column.  No GPU; the reference tree is not read."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as orc
import shiftmax_order_ref as smo

LENGTHS = (49, 144, 197, 208, 577, 1025)
POW2 = (0.25, 0.125)
NATURAL = (0.2113, 0.11873, 0.0571)


@pytest.fixture(scope="module")
def kat(golden_dir):
    return np.load(os.path.join(golden_dir, "shiftmax_bigsum_kat.npz"))


def rows_of(kat, T):
    """-> q int8 [n, T], s [n], bits [n], class [n], the reference's output [n, T], the exact-sum candidate [n, T]"""
    ref = kat[f"ref_{T}"].astype(np.int32)
    return (kat[f"q_{T}"], kat[f"s_{T}"], kat[f"bits_{T}"].astype(np.int32), kat[f"cls_{T}"].astype(np.int32), ref,
            ref + kat[f"exact_minus_ref_{T}"].astype(np.int32))


def groups(kat, T):
    q, s, bits, cls, ref, exact = rows_of(kat, T)
    for sv in np.unique(s):
        for b in (8, 16):
            m = np.flatnonzero((s == sv) & (bits == b))
            if len(m):
                yield np.float32(sv), b, q[m], cls[m], ref[m], exact[m]


def test_fixture_holds_the_required_rows(kat, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "shiftmax_bigsum_kat.npz")) < 300 * 1024
    assert tuple(kat["lengths"]) == LENGTHS
    meta = json.loads(str(kat["meta"]))
    assert [tuple(v) for v in meta["scales"]] == [(float(np.float32(s)), x0) for s, x0 in
                                                  ((0.25, -4), (0.125, -8), (0.2113, -5), (0.11873, -9), (0.0571, -18))]
    c8 = 0
    for T in LENGTHS:
        q, s, bits, cls, ref, exact = rows_of(kat, T)
        assert q.dtype == np.int8 and q.shape[1] == T and set(np.unique(bits)) <= {8, 16}
        pow2 = np.isin(s, np.array(POW2 + (0.0625,), np.float32))
        for sv in np.unique(s):
            x0 = int(smo.x0_of(sv))
            assert T > 208 or T * abs(x0) * 2 ** 15 < 2 ** 32          # the short entries' bound on the exact sum
        c16 = (cls == smo.CLASS_C) & (bits == 16)
        if T >= 144:
            assert (c16 & pow2).sum() >= 4 and (c16 & ~pow2).sum() >= 4, T
            assert (cls == smo.CLASS_A).sum() >= 4 and (cls == smo.CLASS_B).sum() >= 4, T
        else:
            assert (cls == smo.CLASS_A).sum() >= 4, T
            assert (cls != smo.CLASS_A).any() or f"T{T}" in meta["notes"]      # class (a) only: the file says so
        c8 += int(((cls == smo.CLASS_C) & (bits == 8)).sum())
        # class (c) is "the two candidates differ", nothing else is
        assert np.array_equal(np.any(ref != exact, axis=1), cls == smo.CLASS_C)
    assert c8 >= 4


@pytest.mark.parametrize("T", LENGTHS)
def test_restatement_reproduces_candidates_and_classes(kat, T):
    for s, bits, q, cls, ref, exact in groups(kat, T):
        got_cls, ot, oe = smo.classify(q, s, bits)
        assert np.array_equal(ot, ref), (T, s, bits, "torch's order is not the reference's output")
        assert np.array_equal(oe, exact), (T, s, bits)
        assert np.array_equal(got_cls, cls), (T, s, bits)
        ef = smo.exponents(q, s)
        St, Se, isum = smo.both_sums(ef)
        assert np.all(isum >= 1 << 24)
        # the vectorised order is the oracle's restatement of torch's kernel, row by row
        assert np.array_equal(St, np.array([orc.torch_rowsum(e) for e in ef], np.float32))
        a = cls == smo.CLASS_A
        assert np.all(smo.order_free(ef, isum)[a]) and np.array_equal(St[a], Se[a])
        assert np.all(St[cls == smo.CLASS_B] != Se[cls == smo.CLASS_B])
        # class (c): the sums lie on either side of a boundary of floor(2^31 / S)
        c = cls == smo.CLASS_C
        assert np.all(smo.factor_of(St[c]) != smo.factor_of(Se[c]))
        # at a power-of-two scale the exponents are what the integer form gives
        if np.array_equal(smo.phi_table(s), np.arange(-128, 128, dtype=np.float32)):
            d = q.astype(np.int64) - q.max(axis=1, keepdims=True)
            assert np.array_equal(ef, integer_shiftexp(d, int(smo.x0_of(s))).astype(np.float32))


def integer_shiftexp(d, x0, n=15):
    """int_exp_shift (ivit_modules.py:150-162) in integers, d <= 0"""
    x = d + (d >> 1) - (d >> 4)                   # floor division by 2 and 16
    x = np.maximum(x, n * x0)
    q = x // x0                                   # floor: x and x0 are both <= 0
    r = x - x0 * q
    num = r - 2 * x0                              # 2 * (r / 2 - x0)
    sh = n - q
    return np.where(sh >= 1, num << np.maximum(sh - 1, 0), num >> 1)      # floor((r / 2 - x0) * 2^(n - q))


@pytest.mark.parametrize("T", LENGTHS)
def test_oracles_give_the_reference_column(kat, T):
    """oracle.shiftmax (power-of-two scales) and oracle.shiftmax_compat (any scale) against the reference's outputs; both count
    the rows whose exact sum is 2^24 or more"""
    seen = 0
    for s, bits, q, cls, ref, exact in groups(kat, T):
        k = q.astype(np.int32)
        got, ninx = orc.shiftmax_compat(k, s, output_bit=bits, return_inexact=True)
        assert np.array_equal(got, ref), (T, s, bits, "shiftmax_compat")
        assert ninx == len(q)
        if orc.phi_is_identity(s) and float(s) in POW2 + (0.0625,):
            got, ninx = orc.shiftmax(k, s, output_bit=bits, return_inexact=True)
            bad = np.flatnonzero(np.any(got != ref, axis=1))
            assert not len(bad), (T, s, bits, f"shiftmax differs on {len(bad)} rows, classes {cls[bad].tolist()}")
            assert ninx == len(q)
        seen += len(q)
    assert seen == len(kat[f"q_{T}"])


def test_rows_below_the_threshold_do_not_depend_on_the_order():
    """the other side of 2^24: any order of a row whose sum stays below it gives the exact sum, so both candidates agree"""
    rng = np.random.default_rng(5)
    for s in POW2 + NATURAL:
        q = np.clip(np.rint(rng.normal(0, 30, size=(64, 197))), -128, 127).astype(np.int8)
        ef = smo.exponents(q, np.float32(s))
        St, Se, isum = smo.both_sums(ef)
        small = isum < 1 << 24
        assert small.sum() > 32 and np.array_equal(St[small], Se[small])
        assert np.array_equal(orc.shiftmax_compat(q.astype(np.int32), np.float32(s)), smo.outputs(ef, St, 8))
