"""tests/fenced.py can fail: numpy stand-ins for a kernel that ignores `ld`, writes a pad column, writes a guard row or skips a dword
are each reported, by kind and position; the two CPU conditions (poison effective, sentinel visible) reject the inputs they should.
Host buffers only (device=None): no kernel is broken on purpose anywhere."""
import numpy as np
import pytest

import fenced

ROWS, W, LDX, LDO = 5, 12, 20, 16


def _case():
    rng = np.random.default_rng(3)
    k = rng.integers(-100, 100, size=(ROWS, W)).astype(np.int8)
    return k, _op(k)


def _op(x):
    """a row operator with a row maximum in it, as ShiftGELU has"""
    x = x.astype(np.int32)
    return np.clip(x - x.max(axis=1, keepdims=True) // 2, -128, 127).astype(np.int8)


def _buffers(lead=0):
    k, exp = _case()
    x = fenced.input(k, LDX, 127, lead_bytes=lead, oracle=_op, expected=exp, device=None)
    o = fenced.output(ROWS, W, LDO, np.int8, expected=exp, lead_bytes=lead, device=None)
    return k, exp, x, o


def _good_kernel(x, o):
    o.rows2d()[:, :W] = _op(x.rows2d()[:, :W])


@pytest.mark.parametrize("lead", [0, 4])
def test_a_correct_kernel_passes(lead):
    k, exp, x, o = _buffers(lead)
    assert x.start % 16 == lead and o.start % 16 == lead
    _good_kernel(x, o)
    fenced.check(o, exp)
    fenced.check(x)
    assert (x.rows2d()[:, W:] == 127).all() and (x.host[:x.start].view(np.int8) == 127).all()


def test_kernel_that_ignores_ldx_reads_poison():
    k, exp, x, o = _buffers()
    dense = x.body_view()[:ROWS * W].reshape(ROWS, W)          # rows addressed with W where ldx was meant
    o.rows2d()[:, :W] = _op(dense)
    with pytest.raises(AssertionError, match=r"data differs at row 1, column 0"):  # row 0 is the same either way; row 1 takes in row 0's pad
        fenced.check(o, exp)


def test_kernel_that_ignores_ldo_is_reported():
    k, exp, x, o = _buffers()
    o.body_view()[:ROWS * W] = exp.reshape(-1)                 # stores with stride W into a buffer of stride LDO
    with pytest.raises(AssertionError, match=r"data differs at row 1, column 0"):
        fenced.check(o, exp)


def test_store_into_a_pad_column_is_reported():
    k, exp, x, o = _buffers()
    _good_kernel(x, o)
    o.rows2d()[3, W + 1] = exp[3, 0]
    with pytest.raises(AssertionError, match=rf"pad written at row 3, column {W + 1} \(ld {LDO}\)"):
        fenced.check(o, exp)
    # the slack behind the last row is pad of the last row
    k, exp, x, o = _buffers()
    _good_kernel(x, o)
    o.rows2d()[ROWS - 1, LDO - 1] = 0
    with pytest.raises(AssertionError, match=rf"pad written at row {ROWS - 1}, column {LDO - 1}"):
        fenced.check(o, exp)


@pytest.mark.parametrize("where", ["before", "behind"])
def test_store_into_a_guard_row_is_reported(where):
    k, exp, x, o = _buffers()
    _good_kernel(x, o)
    if where == "before":
        o.host[o.start - 3] = 0
        msg = "guard written 3 elements before row 0"
    else:
        o.host[o.start + o.body + 2] = 0
        msg = "guard written 2 elements behind the last row's slack"
    with pytest.raises(AssertionError, match=msg):
        fenced.check(o, exp)


def test_skipped_dword_is_reported_as_never_stored():
    k, exp, x, o = _buffers()
    _good_kernel(x, o)
    o.rows2d()[2, 4:8] = o.fill
    with pytest.raises(AssertionError, match=r"data differs at row 2, column 4: .*never stored"):
        fenced.check(o, exp)


def test_write_to_an_input_is_reported():
    k, exp, x, o = _buffers()
    x.rows2d()[1, W + 2] = 0
    with pytest.raises(AssertionError, match="input changed"):
        fenced.check(x)


def test_sentinel_is_chosen_visible_or_the_case_fails():
    exp = np.zeros((3, 8), np.int8)
    exp[1, 4:8] = fenced.SENTINELS[1][0]                       # a whole aligned dword of the first sentinel
    assert not fenced.sentinel_visible(exp, fenced.SENTINELS[1][0])
    exp[1, 3] = fenced.SENTINELS[1][0]                         # unaligned runs do not matter
    o = fenced.output(3, 8, 12, np.int8, expected=exp, device=None)
    assert o.fill == fenced.SENTINELS[1][1]
    with pytest.raises(AssertionError, match="sentinel occurs"):
        fenced.output(3, 8, 12, np.int8, sentinel=fenced.SENTINELS[1][0], expected=exp, device=None)
    for i, s in enumerate(fenced.SENTINELS[1]):
        exp[2 if i % 2 else 0, 4 * (i // 2):4 * (i // 2) + 4] = s
    with pytest.raises(AssertionError, match="every sentinel"):
        fenced.output(3, 8, 12, np.int8, expected=exp, device=None)
    # 16- and 32-bit elements: a dword is two elements, one element; floats by bit pattern
    e16 = np.zeros((2, 6), np.int16)
    e16[0, 2:4] = fenced.SENTINELS[2][0]
    assert fenced.pick_sentinel(e16) == fenced.SENTINELS[2][1]
    e16[0, 2] = 0
    assert fenced.pick_sentinel(e16) == fenced.SENTINELS[2][0]
    f = np.zeros((2, 3), np.float32)
    f.view(np.int32)[1, 1] = fenced.SENTINELS[4][0]
    assert fenced.pick_sentinel(f) == fenced.SENTINELS[4][1]
    o = fenced.output(2, 3, 5, np.float32, expected=f, device=None)
    assert o.fill.dtype == np.float32 and o.fill.view(np.int32) == fenced.SENTINELS[4][1]
    o.rows2d()[:, :3] = f
    fenced.check(o, f)


def test_poison_must_change_every_row():
    k, exp = _case()
    k[2, 5] = 127                                              # this row's maximum is the poison already
    with pytest.raises(AssertionError, match="leaves row 2"):
        fenced.input(k, LDX, 127, oracle=_op, expected=_op(k), device=None)
    with pytest.raises(AssertionError, match="leaves row 0"):  # -128 never moves a maximum
        fenced.input(_case()[0], LDX, -128, oracle=_op, expected=exp, device=None)


def test_block_layout_output_is_fenced_behind_the_padded_size():
    rows, width = 21, 64
    exp = np.random.default_rng(1).integers(-100, 100, size=(rows, width)).astype(np.int8)
    o = fenced.output(rows, width, width, np.int8, expected=exp, blocks=True, device=None)
    assert o.body == 32 * width
    o.body_view()[fenced.block_offsets(rows, width)] = exp
    fenced.check(o, exp)
    o.host[o.start + o.body] = 0
    with pytest.raises(AssertionError, match="guard written 0 elements behind"):
        fenced.check(o, exp)
    o = fenced.output(rows, width, width, np.int8, expected=exp, blocks=True, device=None)
    o.body_view()[fenced.block_offsets(rows, width)] = exp
    o.body_view()[fenced.block_offsets(rows, width)[20, 16:20]] = o.fill
    with pytest.raises(AssertionError, match="data differs at row 20, column 16.*never stored"):
        fenced.check(o, exp)
