"""Fenced operands of more than 4 GiB, on the device: tests/fenced.py's contract (`input`, `output`, `check`, `.ptr`, `.ld`) for the
tests that put the rows of ONE operand on both sides of 2^31 and of 2^32 bytes (tests/test_gpu_far_*.py).

    | lead guard: 2^31 bytes + one row | row 0: width data, ld - width pad | row 1 ... | last row, slack | tail guard: one row, >= 64 bytes |

Every byte that is not data holds the fill -- the POISON of an input, a sentinel of fenced.SENTINELS for an output -- chosen and
asserted by fenced.pick_sentinel / fenced.poison_effective on the CPU, from the expected values, before anything is launched.  The
leading dimension is `ld_for(rows, ...)`: ceil(1.02 * 2^32 / (rows - 2)) bytes, rounded up to the granularity of the entry, so that
one row starts in each of [0, 2^31), [2^31, 2^32) and [2^32, ...) (asserted in Buffer; with exactly three rows the leading dimension is 0.75 * 2^32 bytes instead).

Why this layout: no faults by construction.  The body is longer than 2^32 bytes and 2^31 bytes plus a row lie in front of it, so
every plausible truncation of a CORRECT byte offset x, 0 <= x < body, lands inside the allocation:
    low 32 bits, zero-extended             -> [0, 2^32): in the body
    low 32 bits, sign-extended             -> [-2^31, 2^31): lead guard or body
    a 32-bit product row * ld wrapped before it was widened, then + column: either of the two, at most one row further
A forgotten cast therefore shows as a damaged fill or as a wrong / never-stored value -- a failed comparison -- and never as an
access out of bounds.  This holds for offsets derived from a correct 64-bit one only; an offset that is wrong for another reason
is what reading the kernel is for.

Allocation, fill, gather and compare all happen on the device (a host copy of 7 GB is no option): rows are gathered through
torch.as_strided and compared as bit patterns with the expected values uploaded once; then the data columns are overwritten with
the fill and the whole allocation must equal the fill, in chunks of at most CHUNK bytes, so that no temporary is as large as the
buffer.  One far operand per call -- the others are ordinary `fenced` buffers -- keeps the peak near 7 GB; `release()` (from an
autouse fixture of the test module) synchronises and drops every buffer made here after each test, and `release(all=True)` at
the end of the module empties torch's cache (see there why not after every test).

device="cpu" and smaller LEAD_GUARD / ZONES / CHUNK: tests/test_far_cpu.py drives `check` with stand-ins for a faulty kernel."""
import ctypes

import numpy as np

import fenced

LEAD_GUARD = 2 ** 31             # bytes in front of row 0, plus one row
ZONES = (2 ** 31, 2 ** 32)       # a row must start below the first, between the two, and from the second on
CHUNK = 2 ** 28                  # bytes per compare
SPREAD = 1.02                    # rows - 2 leading dimensions reach 2 % beyond ZONES[1]

_LIVE = []


def ld_for(rows, itemsize=1, multiple=1, least=0):
    """leading dimension in ELEMENTS: ceil(SPREAD * ZONES[1] / (rows - 2)) bytes, rounded up to `multiple` elements, at least `least`"""
    assert rows >= 3, "far: three rows at least (one per zone)"
    if rows == 3:          # rows - 2 == 1 would skip the middle zone: rows at 0, 0.75 and 1.5 times ZONES[1]
        nbytes = -(-3 * ZONES[1] // 4)
    else:
        nbytes = -(-int(SPREAD * ZONES[1]) // (rows - 2))
    ld = max(-(-nbytes // itemsize), least)
    return -(-ld // multiple) * multiple


def need_bytes(rows, ld, itemsize=1):
    """device memory of one far buffer"""
    row = ld * itemsize
    return LEAD_GUARD + row + 16 + 16 + rows * row + max(64, row) + 32          # (16: the largest lead_bytes)


def _torch_int(itemsize):
    import torch
    return {1: torch.int8, 2: torch.int16, 4: torch.int32}[itemsize]


class Buffer:
    """`.t`: the whole allocation as integers of the element size (bit patterns); `.rows2d()`: the [rows, width] data as a strided view"""

    def __init__(self, rows, width, ld, dtype, fill, lead_bytes=0, device="cuda:0", zones=True):
        import torch
        dtype = np.dtype(dtype)
        item = dtype.itemsize
        assert rows >= 3 and ld >= width > 0 and lead_bytes % item == 0 and 0 <= lead_bytes < 16
        self.rows, self.width, self.ld, self.dtype, self.lead_bytes, self.device = rows, width, ld, dtype, lead_bytes, device
        self.fill = np.array(fill).astype(dtype)[()]
        self.fill_bits = int(fenced._bits(np.array([self.fill]))[0])
        row = ld * item
        self.guard = (LEAD_GUARD + row + 15) // 16 * 16
        self.start = self.guard + lead_bytes
        self.body = rows * row
        self.tail = (max(64, row) + 15) // 16 * 16
        self.total = (self.start + self.body + self.tail + 15) // 16 * 16
        starts = np.arange(rows, dtype=np.int64) * row
        assert not zones or (starts < ZONES[0]).any() and ((starts >= ZONES[0]) & (starts < ZONES[1])).any() and (starts >= ZONES[1]).any(), \
            f"far: {rows} rows of {row} bytes do not start in all three zones"
        self.t = torch.empty(self.total // item, dtype=_torch_int(item), device=device)
        self.t.fill_(self.fill_bits)
        assert self.t.data_ptr() % 16 == 0
        self.data = None          # an input: the device copy of what was written (bit patterns)
        _LIVE.append(self)

    def rows2d(self):
        import torch
        return torch.as_strided(self.t, (self.rows, self.width), (self.ld, 1), self.start // self.dtype.itemsize)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.start)


def _upload(a, dtype, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(fenced._bits(np.asarray(a).astype(dtype)))).to(device)


def input(array2d, ld, poison, lead_bytes=0, oracle=None, expected=None, device="cuda:0", zones=True):      # noqa: A001 (as fenced.input)
    """device buffer holding `array2d` with row stride ld; pad columns, guards and slack hold `poison` (shown effective first, as
    fenced.input does, when `oracle` and `expected` are given).  zones=False: an operand at a launcher's bound, which need not
    reach all three zones; the layout and the check are the same."""
    a = np.ascontiguousarray(array2d)
    assert a.ndim == 2
    if oracle is not None:
        fenced.poison_effective(a, poison, oracle, expected)
    b = Buffer(a.shape[0], a.shape[1], ld, a.dtype, poison, lead_bytes, device, zones)
    b.data = _upload(a, a.dtype, device)
    b.rows2d().copy_(b.data)
    return b


def output(rows, width, ld, dtype, sentinel=None, expected=None, lead_bytes=0, device="cuda:0", zones=True):
    """device buffer for a [rows, width] result with row stride ld, every byte the sentinel (fenced.pick_sentinel on `expected`, or
    the given one, checked against `expected`)"""
    dtype = np.dtype(dtype)
    if expected is not None:
        expected = np.asarray(expected).astype(dtype)
    if sentinel is None:
        assert expected is not None, "far.output: a sentinel or the expected values to pick one"
        sentinel = fenced.pick_sentinel(expected)
    elif expected is not None:
        assert fenced.sentinel_visible(expected, fenced._bits(np.array([sentinel]).astype(dtype))[0]), "far: the sentinel occurs as a whole dword of the expected output"
    if dtype.kind == "f" and isinstance(sentinel, (int, np.integer)):
        sentinel = np.array([sentinel], np.int32).view(np.float32)[0]
    return Buffer(rows, width, ld, dtype, sentinel, lead_bytes, device, zones)


def _where(out, elem):
    """an element index of the allocation, in words"""
    item = out.dtype.itemsize
    first = out.start // item
    if elem < first:
        return f"guard written {first - elem} elements before row 0"
    if elem >= first + out.body // item:
        return f"guard written {elem - first - out.body // item} elements behind the last row's slack"
    r, c = divmod(elem - first, out.ld)
    return f"{'pad' if c >= out.width else 'data column'} written at row {r}, column {c} (ld {out.ld})"


def _stray(out):
    """with the data columns holding the fill: (number of elements that are not the fill, index of the first) over the whole allocation"""
    import torch
    step = max(1, CHUNK // out.dtype.itemsize)
    n = out.t.numel()
    counts = torch.stack([(out.t[a:a + step] != out.fill_bits).sum() for a in range(0, n, step)]).cpu().numpy()
    if not counts.any():
        return 0, None
    a = int(np.argmax(counts > 0)) * step
    return int(counts.sum()), a + int((out.t[a:a + step] != out.fill_bits).nonzero()[0, 0])


def check(out, expected=None):
    """`out[:, :width]` == expected, bit for bit; every pad column, both guards and the slack still hold the fill.  expected=None:
    an input -- the data columns are what was written.  Raises AssertionError naming the first bad element as (row, column) or as
    an offset into a guard.  A buffer checked against `expected` is spent afterwards (its data columns hold the fill), an input
    checked against itself is restored."""
    import torch
    if out.device != "cpu":
        torch.cuda.synchronize()
    what = "input changed: " if expected is None else ""
    if expected is None:
        assert out.data is not None, "far.check: an output needs its expected values"
        exp = out.data
    else:
        e = np.asarray(expected)
        assert e.shape == (out.rows, out.width), (e.shape, out.rows, out.width)
        e = fenced._bits(e.astype(out.dtype))
        if out.data is None:          # (an input that was overwritten in place keeps its poison as the fill: no such condition)
            assert fenced.sentinel_visible(e, out.fill_bits), "far: the sentinel occurs as a whole dword of the expected output"
        exp = torch.from_numpy(np.ascontiguousarray(e)).to(out.device)
    view = out.rows2d()
    step = max(1, CHUNK // (out.width * out.dtype.itemsize))
    bad, first = 0, None
    for r0 in range(0, out.rows, step):
        ne = view[r0:r0 + step] != exp[r0:r0 + step]
        n = int(ne.sum())
        if n and first is None:
            i = ne.nonzero()[0]
            first = (r0 + int(i[0]), int(i[1]))
        bad += n
    got = int(view[first]) if first else None
    want = int(exp[first]) if first else None
    view.fill_(out.fill_bits)
    strays, at = _stray(out)
    if expected is None:
        view.copy_(out.data)
    if first:
        never = " (still the sentinel: never stored)" if got == out.fill_bits and out.data is None else ""
        astray = f"; {strays} elements outside the data changed, the first: {_where(out, at)}" if strays else ""
        raise AssertionError(f"far: {what}data differs at row {first[0]}, column {first[1]}: got {got}, expected {want}{never}; "
                             f"{bad} of {out.rows * out.width} elements differ{astray}")
    if strays:
        raise AssertionError(f"far: {what}{_where(out, at)}: {int(out.t[at])} over the fill {out.fill_bits}; {strays} elements changed")


def untouched(out):
    """an output that a refused call was handed: every byte still holds the sentinel"""
    import torch
    if out.device != "cpu":
        torch.cuda.synchronize()
    assert out.data is None
    strays, at = _stray(out)
    assert not strays, f"far: a refused call wrote: {_where(out, at)}; {strays} elements changed"


def free(*bufs):
    """give the buffers' memory back to torch's allocator: the next far buffer of a test reuses it"""
    for b in bufs:
        b.t = b.data = None


KEEP_CACHED = 64 << 30          # bytes torch's allocator may keep between the tests of one module (the flat entries' operands: 17 GB each)


def release(all=False):      # noqa: A002
    """synchronise and drop every buffer made here (after each test); hand the memory back to the driver when more than
    KEEP_CACHED bytes are reserved, or all of it (`all`: at the end of a test module, so that nothing of this size stays cached
    for the rest of the suite).  Why not after every test: returning a 7 GB block to the driver and asking for it again stalls
    the process for 4 - 5 s about once in twenty round trips (measured: 40 rounds of output / check / release, two stalls, one
    inside the allocation and one at the next synchronisation; none in 40 rounds that kept the block cached), which made single
    cases of these files take 5 - 6 s.  Tests of one shape follow each other, so the cached block is the next test's buffer."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    for b in _LIVE:
        b.t = b.data = None
    _LIVE.clear()
    if torch.cuda.is_available() and (all or torch.cuda.memory_reserved() > KEEP_CACHED):
        torch.cuda.empty_cache()
