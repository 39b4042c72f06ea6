"""Strided, fenced operands for the tests of the C ABI's leading dimensions (tests/test_gpu_strides.py).

A buffer made here holds a [rows, width] matrix with row stride `ld` >= width inside a larger allocation:

    | guard (>= one row) | row 0: width data, ld - width pad | row 1 ... | row rows-1: data, pad (the slack) | guard (>= one row) |

Every byte that is not data holds one fill value: the POISON of an input (a value that changes the operator's result if it is read)
or the SENTINEL of an output (a value the operator does not produce, so that a store that went astray -- or never happened -- shows).
`lead_bytes` shifts the first row off the allocation's 16-byte alignment, down to the smallest alignment an entry admits.

    x = fenced.input(k, ldx, 127, oracle=f, expected=exp)      # f(k widened by one poisoned dword) must differ from exp in every row
    o = fenced.output(rows, C, ldo, np.int8, expected=exp)     # the sentinel is chosen so that no dword of exp could pass for it
    _lib.call("ivit_...", x.ptr, x.ld, ..., o.ptr, o.ld, ...)
    fenced.check(o, exp)                                       # data bit for bit; pad, guards and slack untouched
    fenced.check(x)                                            # (an input is still what it was)

The two conditions -- poison effective in every row, sentinel visible in every dword -- are asserted here, on the CPU, from the
expected values alone and before anything is launched; they are the only statements of these tests that are not comparisons.
With device=None the buffer lives in host memory (`.host`, `.rows2d()`): tests/test_fenced_cpu.py drives the checks with numpy
stand-ins for a faulty kernel."""
import numpy as np

SENTINELS = {        # per element size: the short fixed list the sentinel of an output is taken from
    1: (-86, 85, -51, 102),                                  # 0xAA, 0x55, 0xCD, 0x66
    2: (-21846, 21845, -12851, 26214),
    4: (-1431655766, 1431655765, -842150451, 1717986918),    # as int32; float outputs take the same bit patterns
}
POISON = {np.dtype(np.int8): 127, np.dtype(np.int16): 32767, np.dtype(np.int32): 2 ** 30, np.dtype(np.float32): 1e30}


def _bits(a):
    """an array as integers of its element size: floats (NaNs included) compare by bit pattern"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.int8, 2: np.int16, 4: np.int32}[a.dtype.itemsize])


def sentinel_visible(expected, sentinel):
    """no aligned group of one dword (4 / 2 / 1 consecutive elements) within a row of `expected` equals the sentinel throughout"""
    e = _bits(expected)
    e = e.reshape(e.shape[0], -1)
    g = 4 // e.dtype.itemsize
    n = e.shape[1] // g * g
    hit = (e[:, :n].reshape(e.shape[0], -1, g) == sentinel).all(axis=2)
    tail = (e[:, n:] == sentinel).all(axis=1) if n < e.shape[1] else np.zeros(e.shape[0], bool)
    return not (hit.any() or tail.any())


def pick_sentinel(expected):
    e = _bits(expected)
    for s in SENTINELS[e.dtype.itemsize]:
        if sentinel_visible(e, s):
            return s
    raise AssertionError("fenced: every sentinel of the list occurs as a whole dword of the expected output")


class Buffer:
    def __init__(self, rows, width, ld, dtype, fill, lead_bytes=0, device="cuda:0", block_bytes=0, guard_bytes=0):
        dtype = np.dtype(dtype)
        item = dtype.itemsize
        assert ld >= width > 0 and rows > 0 and lead_bytes % item == 0 and 0 <= lead_bytes < 16
        self.rows, self.width, self.ld, self.dtype, self.lead_bytes, self.device = rows, width, ld, dtype, lead_bytes, device
        self.fill = np.array(fill).astype(dtype)[()]
        # a block-layout matrix (include/ivit_hip.h IVIT_LAYOUT_BLOCKS) is `block_bytes` dense bytes: no rows to tell apart
        self.body = block_bytes if block_bytes else rows * ld * item
        self.guard = (max(64, ld * item, guard_bytes) + 15) // 16 * 16
        self.start = self.guard + lead_bytes
        total = (self.start + self.body + self.guard + 15) // 16 * 16
        self.host = np.empty(total, np.uint8)
        self.host.view(dtype)[:] = self.fill                     # total and start are multiples of the element size
        self.blocks = bool(block_bytes)
        self.t = None

    # ---- host side
    def body_view(self, raw=None):
        raw = self.host if raw is None else raw
        return raw[self.start:self.start + self.body].view(self.dtype)

    def rows2d(self, raw=None):
        """[rows, ld] view of the body (row-major buffers)"""
        assert not self.blocks
        return self.body_view(raw).reshape(self.rows, self.ld)

    def upload(self):
        if self.device is None:
            return self
        import torch
        self.t = torch.from_numpy(self.host).to(self.device)
        assert self.t.data_ptr() % 16 == 0
        return self

    def fetch(self):
        if self.t is None:
            return self.host
        return self.t.cpu().numpy()

    # ---- what the C ABI gets
    @property
    def tensor(self):
        """a torch view that starts at element (0, 0) (for _lib.ptr)"""
        return self.t[self.start:]

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.t.data_ptr() + self.start)


def _widen(a, poison):
    n = max(1, 4 // a.dtype.itemsize)
    return np.concatenate([a, np.full((a.shape[0], n), poison, a.dtype)], axis=1)


def poison_effective(array2d, poison, oracle, expected):
    """`oracle` on the rows widened by one poisoned dword -- what a kernel that reads one dword too many would see -- differs from
    `expected` in at least one element of every row"""
    got = np.asarray(oracle(_widen(np.ascontiguousarray(array2d), poison)))
    exp = np.asarray(expected)
    assert got.shape[0] == exp.shape[0], "fenced: the oracle changed the number of rows"
    got = got.reshape(got.shape[0], -1)[:, :exp.reshape(exp.shape[0], -1).shape[1]]
    same = (_bits(got.astype(exp.dtype)) == _bits(exp).reshape(exp.shape[0], -1)).all(axis=1)
    assert not same.any(), f"fenced: poison {poison} leaves row {int(np.argmax(same))} ({int(same.sum())} rows) of the result unchanged"


def input(array2d, ld, poison, lead_bytes=0, oracle=None, expected=None, device="cuda:0"):      # noqa: A001 (the name the tests read best with)
    """device buffer holding `array2d` with row stride ld; pad columns, guard rows and slack hold `poison`.  With `oracle` (a
    function of the input matrix) and `expected` (its value on `array2d`) the poison is shown to be effective first."""
    a = np.ascontiguousarray(array2d)
    assert a.ndim == 2
    if oracle is not None:
        poison_effective(a, poison, oracle, expected)
    b = Buffer(a.shape[0], a.shape[1], ld, a.dtype, poison, lead_bytes, device)
    b.rows2d()[:, :a.shape[1]] = a
    b.initial = b.host.copy()
    return b.upload()


def input_blocks(flat, rows, width, poison, device="cuda:0"):
    """a block-layout operand (dense bytes, as tiled by the caller) between two poisoned guards"""
    flat = np.ascontiguousarray(flat).reshape(-1)
    b = Buffer(rows, width, width, flat.dtype, poison, 0, device, block_bytes=flat.nbytes)
    b.body_view()[:] = flat
    b.initial = b.host.copy()
    return b.upload()


def output(rows, width, ld, dtype, sentinel=None, expected=None, lead_bytes=0, blocks=False, guard_bytes=0, device="cuda:0"):
    """device buffer for a [rows, width] result with row stride ld, every byte `sentinel`.  sentinel=None: the first of SENTINELS
    that is visible against `expected`; a given one is checked against `expected` when that is passed.  blocks=True: the
    ceil(rows / 16) * 16 * width bytes of a block-layout output (ld == width, int8) instead of rows.  guard_bytes: guards of at least
    that size (an entry that is handed a larger buffer of which it may write this part only)."""
    dtype = np.dtype(dtype)
    if expected is not None:
        expected = np.asarray(expected).astype(dtype)
    if sentinel is None:
        assert expected is not None, "fenced.output: a sentinel or the expected values to pick one"
        sentinel = pick_sentinel(expected)
    elif expected is not None:
        assert sentinel_visible(expected, _bits(np.array([sentinel]).astype(dtype))[0]), "fenced: the sentinel occurs as a whole dword of the expected output"
    if dtype.kind == "f":
        sentinel = np.array([sentinel], np.int32).view(np.float32)[0] if isinstance(sentinel, (int, np.integer)) else sentinel
    block_bytes = 0
    if blocks:
        assert ld == width and dtype.itemsize == 1 and width % 64 == 0
        block_bytes = (rows + 15) // 16 * 16 * width
    b = Buffer(rows, width, ld, dtype, sentinel, lead_bytes, device, block_bytes=block_bytes, guard_bytes=guard_bytes)
    b.initial = None
    return b.upload()


def block_offsets(rows, width):
    """IVIT_LAYOUT_BLOCKS of include/ivit_hip.h: byte offset of element (r, c) of a [rows, width] int8 matrix"""
    r, c = np.meshgrid(np.arange(rows), np.arange(width), indexing="ij")
    rl = r & 15
    return ((r >> 4) * (width >> 6) + (c >> 6)) * 1024 + (((rl << 2) + (((c >> 4) & 3) ^ ((rl >> 2) & 3))) << 4) + (c & 15)


def _first(mask):
    i = np.argwhere(mask)
    return tuple(int(v) for v in i[0])


def check(out, expected=None):
    """`out[:, :width]` == expected element for element (bit patterns); every pad column, both guards and the slack behind the last
    row still hold the fill.  expected=None: an input -- the whole allocation is what was uploaded.  A block-layout buffer compares
    the defined rows at their documented offsets and the guards.  Raises AssertionError naming the first bad element."""
    raw = out.fetch()
    if expected is None:
        assert out.initial is not None, "fenced.check: an output needs its expected values"
        bad = raw != out.initial
        assert not bad.any(), f"fenced: input changed at byte {_first(bad)[0] - out.start} of its rows ({int(bad.sum())} bytes)"
        return
    exp = np.asarray(expected)
    assert exp.shape == (out.rows, out.width), (exp.shape, out.rows, out.width)
    exp = _bits(exp.astype(out.dtype))
    fill = _bits(np.array([out.fill]))[0]
    if out.initial is None:      # an output that was filled with a sentinel (in place, the poison of the input is the fill)
        assert sentinel_visible(exp, fill), "fenced: the sentinel occurs as a whole dword of the expected output"
    item = out.dtype.itemsize
    before = _bits(raw[:out.start // item * item].view(out.dtype)) != fill
    after = _bits(raw[out.start + out.body:].view(out.dtype)) != fill
    if out.blocks:
        got = _bits(out.body_view(raw))[block_offsets(out.rows, out.width)]
        pad = np.zeros((out.rows, 0), bool)
    else:
        body = _bits(out.rows2d(raw))
        got, pad = body[:, :out.width], body[:, out.width:] != fill
    data = got != exp
    if data.any():
        r, c = _first(data)
        never = " (still the sentinel: never stored)" if got[r, c] == fill else ""
        raise AssertionError(f"fenced: data differs at row {r}, column {c}: got {got[r, c]}, expected {exp[r, c]}{never}; "
                             f"{int(data.sum())} of {data.size} elements differ")
    if pad.any():
        r, c = _first(pad)
        raise AssertionError(f"fenced: pad written at row {r}, column {out.width + c} (ld {out.ld}): {_bits(out.rows2d(raw))[r, out.width + c]} "
                             f"over the fill {fill}; {int(pad.sum())} pad elements changed")
    if before.any() or after.any():
        where = f"{out.start // item - _first(before)[0]} elements before row 0" if before.any() else f"{_first(after)[0]} elements behind the last row's slack"
        raise AssertionError(f"fenced: guard written {where}; {int(before.sum()) + int(after.sum())} guard elements changed")
