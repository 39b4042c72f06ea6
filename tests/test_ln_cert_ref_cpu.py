"""tests/ln_cert_ref.py on the CPU: the numpy restatement of the LayerNorm kernels' float32 bracket certificate finds enough
failing rows in the draws the GPU tests use (their precondition), and the draws are the ones the counts were recorded for."""
import numpy as np
import pytest

from oracle import oracle as orc

import ln_cert_ref as R


def test_bracket_is_the_tightest_float32_pair():
    rng = np.random.default_rng(0)
    m = rng.integers(1 << 30, 1 << 31, size=1000).astype(np.float64)
    e = rng.integers(20, 45, size=1000).astype(np.int32)
    M = np.ldexp(m, -e.astype(np.int64))
    lo, hi = R.bracket(m, e)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert (lo.astype(np.float64) <= M * (1 - R.EPS)).all() and (np.nextafter(lo, np.float32(np.inf)).astype(np.float64) > M * (1 - R.EPS)).all()
    assert (hi.astype(np.float64) >= M * (1 + R.EPS)).all() and (np.nextafter(hi, np.float32(-np.inf)).astype(np.float64) < M * (1 + R.EPS)).all()


@pytest.mark.parametrize("draw,C,failing", [(R.draw_i8, 1100, 44), (R.draw_i16, 200, 42), (R.draw_i16, 96, 40)])
def test_failing_row_counts(draw, C, failing):
    x, gamma, beta = draw(C)
    assert len(x) == R.n_draw(C)
    xs, s_out, exp, n = R.case(x, gamma, beta)
    assert n == failing and n >= R.FLOOR
    assert len(xs) == R.KEEP_FAIL + R.KEEP_PASS == 37
    # the picked rows are 18 failing and 19 passing ones
    y, s_ln, _ = orc.layernorm(xs.astype(np.int32), gamma, beta)
    assert int(R.failing_rows(y, *orc.dyadic(s_ln, s_out)).sum()) == R.KEEP_FAIL
