"""tests/far.py can fail, in the spirit of test_fenced_cpu.py: device="cpu", the guard, the zones and the chunk scaled down by 2^16
(offsets of 16 bits stand for offsets of 32), and numpy stand-ins for a kernel that truncates a row offset, skips a row, writes a
pad byte or modifies its input.  Each is reported by kind and position; the correct stand-in passes.  No kernel is broken on
purpose anywhere."""
import numpy as np
import pytest

import far
import fenced

ROWS, W = 6, 40
BITS = 16                        # the stand-in for 32: offsets wrap at 2^16, the sign bit is 2^15


@pytest.fixture(autouse=True)
def _small(monkeypatch):
    monkeypatch.setattr(far, "LEAD_GUARD", 2 ** (BITS - 1))
    monkeypatch.setattr(far, "ZONES", (2 ** (BITS - 1), 2 ** BITS))
    monkeypatch.setattr(far, "CHUNK", 2 ** 12)       # several chunks per buffer, rows and guards split across them
    yield
    far.release()


def _op(x):
    x = x.astype(np.int32)
    return np.clip(x - x.max(axis=1, keepdims=True) // 2, -128, 127).astype(np.int8)


def _case():
    k = np.random.default_rng(5).integers(-100, 100, size=(ROWS, W)).astype(np.int8)
    return k, _op(k)


def _buffers(lead=0, multiple=16):
    k, exp = _case()
    ld = far.ld_for(ROWS, 1, multiple, least=W)
    x = far.input(k, ld, 127, lead_bytes=lead, oracle=_op, expected=exp, device="cpu")
    o = far.output(ROWS, W, ld, np.int8, expected=exp, lead_bytes=lead, device="cpu")
    return k, exp, x, o


def _kernel(x, o, offset=lambda off: off, rows=range(ROWS)):
    """a row operator that addresses its output as base + offset(row * ldo + column)"""
    src, dst = x.t.numpy(), o.t.numpy()
    for r in rows:
        row = src[x.start + r * x.ld:x.start + r * x.ld + W]
        res = _op(row[None])[0]
        for c in range(W):
            dst[o.start + offset(r * o.ld + c)] = res[c]


def _wrap(off):
    return off % 2 ** BITS


def _sign_extend(off):
    off %= 2 ** BITS
    return off - 2 ** BITS if off >= 2 ** (BITS - 1) else off


def test_ld_for_puts_a_row_in_each_zone():
    for rows in (3, 4, 6, 37, 258):
        for item, mult in ((1, 16), (2, 8), (4, 1), (1, 4)):
            ld = far.ld_for(rows, item, mult)
            assert ld % mult == 0 and (rows == 3 or (rows - 2) * ld * item >= far.SPREAD * far.ZONES[1] > (rows - 2) * (ld - mult) * item - 1)
            starts = np.arange(rows) * ld * item
            assert (starts < far.ZONES[0]).any() and ((starts >= far.ZONES[0]) & (starts < far.ZONES[1])).any() and (starts >= far.ZONES[1]).any()
    with pytest.raises(AssertionError, match="three rows"):
        far.ld_for(2)
    with pytest.raises(AssertionError, match="all three zones"):
        far.output(ROWS, W, W + 16, np.int8, sentinel=85, device="cpu")
    o = far.output(3, W, far.ld_for(3, 1, 16), np.int8, sentinel=85, lead_bytes=12, device="cpu")      # three rows: 0, 0.75, 1.5 x 2^k
    assert far.need_bytes(3, o.ld) >= o.total


def test_every_truncation_of_an_offset_stays_inside_the_allocation():
    """the reason for the layout: for every byte offset of the body, the wrapped and the sign-extended offset, and either plus a
    whole row (a wrapped row product + column), address the allocation"""
    k, exp, x, o = _buffers(lead=4, multiple=4)
    off = np.arange(o.body, dtype=np.int64)
    lo = off % 2 ** BITS
    se = np.where(lo >= 2 ** (BITS - 1), lo - 2 ** BITS, lo)
    for t in (lo, se, lo + o.ld, se + o.ld):
        assert (o.start + t).min() >= 0 and (o.start + t).max() < o.total
    assert far.need_bytes(ROWS, o.ld) >= o.total


@pytest.mark.parametrize("lead,multiple", [(0, 16), (4, 4)])
def test_a_correct_kernel_passes(lead, multiple):
    k, exp, x, o = _buffers(lead, multiple)
    assert x.start % 16 == lead and o.ptr.value % 16 == lead
    _kernel(x, o)
    far.check(o, exp)
    far.check(x)
    far.check(x)                                      # an input is restored by its check
    assert np.array_equal(x.rows2d().numpy(), k)


def test_store_at_the_offset_modulo_2_k_is_reported():
    k, exp, x, o = _buffers()
    _kernel(x, o, _wrap)
    r = -(-2 ** BITS // o.ld)                          # the first row that starts beyond 2^k: its bytes went into row 0's pad
    c = r * o.ld - 2 ** BITS
    assert W <= c < o.ld
    with pytest.raises(AssertionError, match=rf"data differs at row {r}, column 0: .*never stored.*the first: pad written at row 0, column {c} "):
        far.check(o, exp)


def test_store_at_the_sign_extended_offset_is_reported():
    k, exp, x, o = _buffers()
    _kernel(x, o, _sign_extend)
    r = -(-2 ** (BITS - 1) // o.ld)                    # the first row in [2^(k-1), 2^k): stored 2^k bytes early, in the lead guard
    with pytest.raises(AssertionError, match=rf"data differs at row {r}, column 0: .*never stored.*the first: guard written {2 ** BITS - r * o.ld} elements before row 0"):
        far.check(o, exp)


def test_row_never_stored_is_reported():
    k, exp, x, o = _buffers()
    _kernel(x, o, rows=[r for r in range(ROWS) if r != ROWS - 1])
    with pytest.raises(AssertionError, match=rf"data differs at row {ROWS - 1}, column 0: .*never stored\); {W} of {ROWS * W} elements differ$"):
        far.check(o, exp)


def test_wrong_value_is_reported():
    k, exp, x, o = _buffers()
    _kernel(x, o)
    o.rows2d()[4, 7] += 1
    with pytest.raises(AssertionError, match=rf"data differs at row 4, column 7: got {int(exp[4, 7]) + 1}, expected {int(exp[4, 7])}; 1 of"):
        far.check(o, exp)


@pytest.mark.parametrize("row", [0, 3, ROWS - 1])
def test_pad_byte_written_is_reported(row):
    k, exp, x, o = _buffers()
    _kernel(x, o)
    o.t[o.start + row * o.ld + o.ld - 1] = 0          # the last row's is the slack
    with pytest.raises(AssertionError, match=rf"^far: pad written at row {row}, column {o.ld - 1} \(ld {o.ld}\): 0 over the fill"):
        far.check(o, exp)


@pytest.mark.parametrize("where", ["before", "behind"])
def test_guard_byte_written_is_reported(where):
    k, exp, x, o = _buffers()
    _kernel(x, o)
    if where == "before":
        o.t[o.start - 2 ** (BITS - 1) - 3] = 0
        msg = f"guard written {2 ** (BITS - 1) + 3} elements before row 0"
    else:
        o.t[o.start + o.body + 2] = 0
        msg = "guard written 2 elements behind the last row's slack"
    with pytest.raises(AssertionError, match=msg):
        far.check(o, exp)


def test_modified_input_is_reported():
    k, exp, x, o = _buffers()
    x.rows2d()[5, 1] = 3
    with pytest.raises(AssertionError, match=r"input changed: data differs at row 5, column 1: got 3"):
        far.check(x)
    k, exp, x, o = _buffers()
    x.t[x.start + 2 * x.ld + W + 9] = 0
    with pytest.raises(AssertionError, match=rf"input changed: pad written at row 2, column {W + 9}"):
        far.check(x)


def test_wider_elements_compare_bit_patterns():
    exp = np.random.default_rng(2).standard_normal((ROWS, 5)).astype(np.float32)
    exp[1, 1] = np.nan
    ld = far.ld_for(ROWS, 4, 1)
    o = far.output(ROWS, 5, ld, np.float32, expected=exp, lead_bytes=4, device="cpu")
    assert o.fill_bits == fenced.SENTINELS[4][0]
    o.rows2d().copy_(far._upload(exp, np.float32, "cpu"))
    far.check(o, exp)
    e16 = np.random.default_rng(3).integers(-30000, 30000, size=(ROWS, 6)).astype(np.int16)
    x = far.input(e16, far.ld_for(ROWS, 2, 8), 32767, device="cpu")
    far.check(x)
    x.t[x.start // 2 - 1] = 0
    with pytest.raises(AssertionError, match="input changed: guard written 1 elements before row 0"):
        far.check(x)


def test_release_drops_the_buffers():
    k, exp, x, o = _buffers()
    far.release()
    assert x.t is None and o.t is None and not far._LIVE
