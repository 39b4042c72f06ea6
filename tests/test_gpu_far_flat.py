"""The flat entries with `int64_t n` beyond 2^31 (and, where 20 GB allow, 2^32) elements.

Periodic expectations: the input is one block of P = 1 000 003 elements repeated on the device -- P is odd and prime, so it has no
common factor with a grid stride or a power of two -- and the expected output is the oracle's for that one block, compared on the
device period by period, in chunks.  An index that wrapped at 2^31 or 2^32 reads or writes another phase of the block and
differs: asserted on the CPU beforehand (the expected block differs from itself shifted by 2^31 mod P and by 2^32 mod P).

Every operand has 2^31 ELEMENTS of guard in front (a sign-extended 32-bit index stays inside the allocation, as in tests/far.py)
and 4099 behind; output guards hold a sentinel and are compared whole.

The second size, 2^32 + 4099 elements, where it fits 20 GB in total: ivit_residual_requant_i8 / _bits (three int8 operands of
6.4 GB with their guards: 19.3 GB) and ivit_requant_i8_i16 (int8 in, int16 out: 12.9 GB of data; at this size the guards in front
are 2^30 elements, 19.3 GB in all -- a sign-extended index would leave them, which the first size has already ruled out for this
kernel).  Every other entry has a 4-byte operand, 17.2 GB at the second size without any guard and 34 GB with its partner: they run
at the first size only.  Tile / untile: 2^31 + 4160 bytes (rows * K); the row loop is the one far dimension they have."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402

import far  # noqa: E402
from test_gpu_far_rows import room  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
P = 1_000_003
LEAD, TAIL = 2 ** 31, 4099
CHUNK = 2 ** 28
SIZES = {"2^31": 2 ** 31 + 4099, "2^32": 2 ** 32 + 4099}
_TD = {np.dtype(np.int8): torch.int8, np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}


@pytest.fixture(autouse=True)
def _release():
    yield
    far.release()          # keeps up to far.KEEP_CACHED bytes for the next test (see there), everything goes at the module's end


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


def st():
    return _lib.stream_ptr()


def has_period_P_only(block):
    """the block differs from itself shifted by 2^31 mod P and by 2^32 mod P (in a good share of its elements)"""
    b = np.asarray(block).reshape(-1)
    return len(b) % 2 == 1 and all((b != np.roll(b, -(s % len(b)))).mean() > 0.2 for s in (2 ** 31, 2 ** 32))


class Flat:
    """| LEAD elements | n elements | TAIL elements |, every guard element `fill`"""

    def __init__(self, n, dtype, fill, lead=LEAD):
        dtype = np.dtype(dtype)
        room((lead + n + TAIL) * dtype.itemsize)
        self.n, self.fill, self.lead = n, fill, lead
        self.t = torch.full((lead + n + TAIL,), fill, dtype=_TD[dtype], device=DEV)
        self.body = self.t[lead:lead + n]

    @property
    def ptr(self):
        return _lib.ptr(self.body)

    def tile(self, block):
        """body[i] = block[i mod len(block)] (P elements, or 3 P where three channels alternate)"""
        b = torch.from_numpy(np.ascontiguousarray(block)).to(DEV)
        P = b.numel()
        full = self.n // P
        per = max(1, CHUNK // (P * b.element_size()))
        for k in range(0, full, per):
            m = min(per, full - k)
            self.body[k * P:(k + m) * P].view(m, P).copy_(b.expand(m, P))
        self.body[full * P:].copy_(b[:self.n - full * P])
        self.block = b
        return self

    def mismatches(self, block):
        """number of body elements that differ (bit patterns) from block[i mod P], and the first such index"""
        b = torch.from_numpy(np.ascontiguousarray(block)).to(DEV)
        if b.dtype == torch.float32:
            b, body = b.view(torch.int32), self.body.view(torch.int32)
        else:
            body = self.body
        P = b.numel()
        full = self.n // P
        per = max(1, CHUNK // (P * b.element_size()))
        counts, spans = [], []
        for k in range(0, full, per):
            m = min(per, full - k)
            counts.append((body[k * P:(k + m) * P].view(m, P) != b).sum())
            spans.append((k * P, (k + m) * P))
        counts.append((body[full * P:] != b[:self.n - full * P]).sum())
        spans.append((full * P, self.n))
        counts = torch.stack(counts).cpu().numpy()
        if not counts.any():
            return 0, None
        a, e = spans[int(np.argmax(counts > 0))]
        idx = torch.arange(a, e, device=DEV) % P
        return int(counts.sum()), a + int((body[a:e] != b[idx]).nonzero()[0, 0])

    def guards_hold(self):
        bad = 0
        for part in (self.t[:self.lead], self.t[self.lead + self.n:]):
            for a in range(0, part.numel(), CHUNK):
                bad += int((part[a:a + CHUNK] != self.fill).sum())
        return bad == 0


def block_chunk_offsets():
    """IVIT_LAYOUT_BLOCKS inside one 1 KB block: byte offset of (row % 16, column % 64), on the device"""
    rl, c = np.meshgrid(np.arange(16), np.arange(64), indexing="ij")
    return torch.from_numpy(((((rl << 2) + (((c >> 4) & 3) ^ ((rl >> 2) & 3))) << 4) + (c & 15)).reshape(-1)).to(DEV)


def blocks_mismatch(dst, src, rows, K):
    """number of bytes of the block-layout matrix `dst` (flat, ceil(rows / 16) * 16 * K bytes) that differ from the documented place
    of their byte of the row-major `src` (flat, rows * K): block (row / 16, k / 64) at ((row / 16) * (K / 64) + k / 64) * 1024"""
    off, kb, full = block_chunk_offsets(), K // 64, rows // 16
    per = max(1, CHUNK // (16 * K))
    bad = []
    for b0 in range(0, full, per):
        b1 = min(full, b0 + per)
        s = src[b0 * 16 * K:b1 * 16 * K].view(-1, 16, kb, 64).permute(0, 2, 1, 3).reshape(-1, kb, 1024)
        want = torch.empty_like(s)
        want[:, :, off] = s
        bad.append((dst[b0 * 16 * K:b1 * 16 * K].view(-1, kb, 1024) != want).sum())
    r = rows - full * 16
    if r:
        last = dst[full * 16 * K:(full + 1) * 16 * K].view(kb, 1024)[:, off].view(kb, 16, 64).permute(1, 0, 2).reshape(16, K)[:r]
        bad.append((last != src[full * 16 * K:].view(r, K)).sum())
    return int(torch.stack(bad).sum())


def check(out, exp_block):
    torch.cuda.synchronize()
    bad, first = out.mismatches(exp_block)
    assert bad == 0, f"{bad} of {out.n} elements differ, the first at index {first} = 2^31 + {first - 2 ** 31} (phase {first % len(exp_block)})"
    assert out.guards_hold(), "a guard element in front of or behind the output changed"


def unchanged(x):
    assert x.mismatches(x.block.cpu().numpy())[0] == 0 and x.guards_hold(), "an input changed"


# ------------------------------------------------------------------------------------------- the entries
@pytest.mark.parametrize("size", ["2^31", "2^32"])
def test_residual_requant_i8_beyond_2_31_elements(size):
    """ivit_residual_requant_i8 and ivit_residual_requant_i8_bits (8): 3 int8 arrays of 2^31 + n + 4099 bytes each: 19.3 GB at
    2^32 + 4099 (the module docstring says which entries have the second size)"""
    n = SIZES[size]
    rng = np.random.default_rng(31)
    a, b = rng.integers(-128, 128, size=(2, P)).astype(np.int8)
    m1, e1 = dyadic(f32(0.0421), f32(0.0517))
    m2, e2 = dyadic(f32(0.0333), f32(0.0517))
    exp = orc.requant(a.astype(np.int32)[None], m1.astype(np.float64), e1, 8, z2=b.astype(np.int32)[None], m2=m2.astype(np.float64), e2=e2)[0].astype(np.int8)
    assert has_period_P_only(exp) and (exp != 85).mean() > 0.9
    xa, xb = Flat(n, np.int8, 127).tile(a), Flat(n, np.int8, 127).tile(b)
    o = Flat(n, np.int8, 85)
    _lib.call("ivit_residual_requant_i8", xa.ptr, int(m1[0]), int(e1[0]), xb.ptr, int(m2[0]), int(e2[0]), o.ptr, n, st())
    check(o, exp)
    o.body.fill_(85)
    _lib.call("ivit_residual_requant_i8_bits", xa.ptr, int(m1[0]), int(e1[0]), xb.ptr, int(m2[0]), int(e2[0]), o.ptr, n, 8, st())
    check(o, exp)
    unchanged(xa)
    unchanged(xb)


@pytest.mark.parametrize("size", ["2^31", "2^32"])
def test_requant_i8_i16_beyond_2_31_elements(size):
    """ivit_requant_i8_i16: int8 in, int16 out; 2^31-element guards at the first size, 2^30-element ones at the second (19.3 GB)"""
    n = SIZES[size]
    lead = LEAD if size == "2^31" else 2 ** 30
    x = np.random.default_rng(32).integers(-128, 128, size=P).astype(np.int8)
    m, e = dyadic(f32(0.0421), f32(0.000517))
    exp = orc.requant(x.astype(np.int32)[None], m.astype(np.float64), e, 16)[0].astype(np.int16)
    assert has_period_P_only(exp) and np.abs(exp).max() > 1000
    xi = Flat(n, np.int8, 127, lead).tile(x)
    o = Flat(n, np.int16, -21846, lead)
    assert size == "2^31" or xi.t.numel() + 2 * o.t.numel() < 20e9
    _lib.call("ivit_requant_i8_i16", xi.ptr, int(m[0]), int(e[0]), o.ptr, n, st())
    check(o, exp)
    unchanged(xi)


def test_narrow_i32_i8_beyond_2_31_elements():
    """ivit_narrow_i32_i8: values inside int8 (flag stays 0), then ONE value outside at index 2^31 + 5 (flag raised, value clamped)"""
    n = SIZES["2^31"]
    z = np.random.default_rng(33).integers(-128, 128, size=P).astype(np.int32)
    exp = z.astype(np.int8)
    assert has_period_P_only(exp)
    zi = Flat(n, np.int32, 2 ** 30).tile(z)
    o = Flat(n, np.int8, 85)
    flag = torch.zeros(3, dtype=torch.int32, device=DEV)
    _lib.call("ivit_narrow_i32_i8", zi.ptr, o.ptr, n, _lib.ptr(flag), st())
    check(o, exp)
    assert flag.cpu().tolist() == [0, 0, 0]
    at = 2 ** 31 + 5
    zi.body[at] = 300
    _lib.call("ivit_narrow_i32_i8", zi.ptr, o.ptr, n, _lib.ptr(flag), st())
    torch.cuda.synchronize()
    assert flag.cpu().tolist() == [1, 0, 0] and int(o.body[at]) == 127
    o.body[at] = int(exp[at % P])
    check(o, exp)


def test_quantize_input_f32_i8_beyond_2_31_elements():
    """ivit_quantize_input_f32_i8: float32 in (4 elements per thread, scalar tail: n % 4 == 3), int8 out"""
    n = SIZES["2^31"]
    assert n % 4 == 3
    x = (np.random.default_rng(34).standard_normal(P) * 2).astype(f32)
    inv = f32(127 / 6.0)
    exp = np.clip(np.rint((inv * x).astype(f32)), -128, 127).astype(np.int8)
    assert has_period_P_only(exp)
    xi = Flat(n, np.float32, 1e30).tile(x)
    o = Flat(n, np.int8, 85)
    _lib.call("ivit_quantize_input_f32_i8", xi.ptr, o.ptr, n, float(inv), st())
    check(o, exp)
    unchanged(xi)


def test_minmax_f32_beyond_2_31_elements():
    """ivit_minmax_f32 on a constant array with the minimum at index 2^31 + 5 and the maximum at the last index"""
    n = SIZES["2^31"]
    x = Flat(n, np.float32, 1e30)
    x.body.fill_(0.5)
    x.body[2 ** 31 + 5] = -3.25
    x.body[n - 1] = 7.75
    mm = torch.empty(2, dtype=torch.float32, device=DEV)
    _lib.call("ivit_minmax_f32", x.ptr, n, _lib.ptr(mm), st())
    assert mm.cpu().tolist() == [-3.25, 7.75]
    assert x.guards_hold() and int((x.body != 0.5).sum()) == 2, "the input changed"


def test_quantile_pair_refuses_2_31_elements_with_a_real_buffer():
    """ivit_quantile_pair_f32 documents 1 <= n < 2^31: n = 2^31 and 2^31 + 4099 are IVIT_ERR_INVALID, nothing is launched"""
    import test_gpu_quantile as tq
    x = Flat(SIZES["2^31"], np.float32, 1e30)
    x.body.fill_(0.5)
    ws = torch.full((tq.WS,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((6,), 12345.0, dtype=torch.float32, device=DEV)
    for n in (2 ** 31, SIZES["2^31"]):
        with pytest.raises(_lib.IvitError, match="outside 1 .. 2\\^31 - 1"):
            _lib.call("ivit_quantile_pair_f32", x.ptr, n, 0.25, 0.75, _lib.ptr(out[2:4]), _lib.ptr(ws), tq.WS, st())
        torch.cuda.synchronize()
        assert bool((ws == 0xA5).all()) and bool((out == 12345.0).all()), "a refused call launched something"
    assert x.guards_hold() and bool((x.body == 0.5).all()), "the input changed"


def test_quantile_pair_at_its_largest_n():
    """n = 2^31 - 1, the largest the entry admits (tests/test_gpu_quantile.py stops far below): x[i] = (-1, 0.5, 2)[i mod 3], so
    the ranks of q = 0.25 and 0.75 fall inside the runs of -1 and of 2 of the sorted array and both neighbours of each rank are
    equal: the results are -1 and 2 exactly, whatever the interpolation weight"""
    import test_gpu_quantile as tq
    n = 2 ** 31 - 1
    assert 0.25 * (n - 1) + 2 < n // 3 and 0.75 * (n - 1) - 2 > 2 * (n // 3 + 1)
    x = Flat(n, np.float32, 1e30).tile(np.tile(np.array([-1.0, 0.5, 2.0], f32), 333_333))      # a period of 999 999 elements
    ws = torch.full((tq.WS,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((6,), 12345.0, dtype=torch.float32, device=DEV)
    _lib.call("ivit_quantile_pair_f32", x.ptr, n, 0.25, 0.75, _lib.ptr(out[2:4]), _lib.ptr(ws), tq.WS, st())
    assert out.cpu().tolist() == [12345.0, 12345.0, -1.0, 2.0, 12345.0, 12345.0]
    unchanged(x)


# ------------------------------------------------------------------------------------------- 4-byte entries
N3 = SIZES["2^31"]
assert N3 % 3 == 0          # rows x 3 channels with the same product


def _three_channel_block(draw):
    """3 P elements: element i belongs to channel i mod 3 in every period (3 P is odd)"""
    return draw(3 * P)


def test_requant_i32_beyond_2_31_elements():
    """ivit_requant_i32 on rows x 3 int32 with per-channel (m, e), 8 bits: 2 x 17.2 GB with the guards"""
    n, C = N3, 3
    rng = np.random.default_rng(41)
    z = _three_channel_block(lambda k: rng.integers(-20000, 20000, size=k).astype(np.int32))
    pre = np.array([0.0031, 0.0057, 0.0043], f32)
    m, e = dyadic(pre, f32(1.0))
    exp = orc.requant(z.reshape(-1, C), m.astype(np.float64), e, 8).reshape(-1).astype(np.int32)
    assert has_period_P_only(exp) and len(np.unique(exp)) > 100
    zi = Flat(n, np.int32, 2 ** 30).tile(z)
    o = Flat(n, np.int32, -1431655766)
    md, ed = torch.from_numpy(m.view(np.int32)).to(DEV), torch.from_numpy(e).to(DEV)
    _lib.call("ivit_requant_i32", zi.ptr, n // C, C, _lib.ptr(md), _lib.ptr(ed), C, None, None, None, 0, 8, o.ptr, st())
    check(o, exp)
    unchanged(zi)


def test_f32_to_i32_and_back_beyond_2_31_elements():
    """ivit_f32_to_i32 (round) and ivit_i32_to_f32 on rows x 3 with per-channel scales"""
    n, C = N3, 3
    rng = np.random.default_rng(42)
    x = _three_channel_block(lambda k: rng.normal(0, 50, size=k).astype(f32))
    s_vec = np.array([2.0 ** -3, 2.0 ** -5, 0.0437], f32)
    z = np.rint((x.reshape(-1, C) / s_vec).astype(f32)).astype(np.int32)
    y = (z.astype(f32) * s_vec).astype(f32)
    assert has_period_P_only(z) and has_period_P_only(y.view(np.int32))
    sd = torch.from_numpy(s_vec).to(DEV)
    xi = Flat(n, np.float32, 1e30).tile(x)
    o = Flat(n, np.int32, -1431655766)
    _lib.call("ivit_f32_to_i32", xi.ptr, n // C, C, _lib.ptr(sd), C, 0, o.ptr, st())
    check(o, z.reshape(-1))
    unchanged(xi)
    del xi
    yo = Flat(n, np.float32, 1e30)
    _lib.call("ivit_i32_to_f32", o.ptr, n // C, C, _lib.ptr(sd), C, yo.ptr, st())
    check(yo, y.reshape(-1))
    check(o, z.reshape(-1))


def test_quantize_input_f32_i32_beyond_2_31_elements():
    """ivit_quantize_input_f32_i32 at 16 bits"""
    n = SIZES["2^31"]
    x = (np.random.default_rng(43).standard_normal(P) * 4).astype(f32)
    inv = f32(1.0) / f32(0.000317)
    exp = np.clip(np.rint((inv * x).astype(f32)), f32(-32768), f32(32767)).astype(np.int32)
    assert has_period_P_only(exp) and exp.max() == 32767
    xi = Flat(n, np.float32, 1e30).tile(x)
    o = Flat(n, np.int32, -1431655766)
    _lib.call("ivit_quantize_input_f32_i32", xi.ptr, o.ptr, n, float(inv), 16, st())
    check(o, exp)
    unchanged(xi)


def test_ibert_gelu_beyond_2_31_elements():
    """ivit_ibert_gelu_i32 on integers and ivit_ibert_gelu_f32_f32 on their float view (s = 2^-4: x / s is the integer)"""
    from oracle import ibert as ib
    n = SIZES["2^31"]
    s = f32(2.0 ** -4)
    k = np.random.default_rng(44).integers(-128, 128, size=P).astype(np.int32)
    b_int, c_int, shift_int, s_out = ib.gelu_constants(s)
    want_int, so = ib.gelu(k, s)
    want_int = want_int.astype(np.int32)
    want_f = ((want_int + f32(0.0)).astype(f32) * s_out).astype(f32)
    assert so == s_out and has_period_P_only(want_int)
    ki = Flat(n, np.int32, 2 ** 30).tile(k)
    o = Flat(n, np.int32, -1431655766)
    _lib.call("ivit_ibert_gelu_i32", ki.ptr, n, float(b_int), float(c_int), float(shift_int), o.ptr, st())
    check(o, want_int)
    unchanged(ki)
    del ki, o
    xi = Flat(n, np.float32, 1e30).tile((k.astype(f32) * s).astype(f32))
    of = Flat(n, np.float32, 1e30)
    _lib.call("ivit_ibert_gelu_f32_f32", xi.ptr, n, float(s), float(b_int), float(c_int), float(shift_int), float(s_out), of.ptr, st())
    check(of, want_f)
    unchanged(xi)


def test_residual_requant_i16_beyond_2_31_elements():
    """ivit_residual_requant_i16 (a_bits = 8, no window map) wants C % 4 == 0, which no factor of 2^31 + 4099 is: rows x 4 with
    2^31 + 4100 elements"""
    C = 4
    n = (SIZES["2^31"] + C - 1) // C * C
    rng = np.random.default_rng(45)
    a = rng.integers(-128, 128, size=P).astype(np.int8)
    r = rng.integers(-20000, 20000, size=P).astype(np.int16)
    ma, ea = dyadic(f32(0.0421), f32(0.000517))
    mr, er = dyadic(f32(0.000333), f32(0.000517))
    exp = orc.requant(a.astype(np.int32)[None], ma.astype(np.float64), ea, 16, z2=r.astype(np.int32)[None], m2=mr.astype(np.float64), e2=er)[0].astype(np.int16)
    assert has_period_P_only(exp)
    ai, ri = Flat(n, np.int8, 127).tile(a), Flat(n, np.int16, 32767).tile(r)
    o = Flat(n, np.int16, -21846)
    _lib.call("ivit_residual_requant_i16", ai.ptr, 8, None, None, int(ma[0]), int(ea[0]), ri.ptr, int(mr[0]), int(er[0]), o.ptr, n // C, C,
              0, 0, 0, 0, st())
    check(o, exp)
    unchanged(ai)
    unchanged(ri)


def test_tile_and_untile_beyond_2_31_bytes():
    """ivit_tile_operand_i8 / ivit_untile_operand_i8 by rows: K = 64, 2^25 + 65 rows (2^31 + 4160 bytes), the source one block of
    1021 rows (odd) repeated.  The expected block layout is computed on the device from the source rows by the documented formula
    (16 rows x 64 bytes are one 1 KB block), chunk by chunk; the way back must give the source"""
    K, rows = 64, 2 ** 25 + 65
    n = rows * K
    R16 = (rows + 15) // 16 * 16
    blk = np.random.default_rng(46).integers(-128, 127, size=(1021, K)).astype(np.int8)
    assert all((blk.reshape(-1) != np.roll(blk.reshape(-1), -(w % blk.size))).mean() > 0.2 for w in (2 ** 31, 2 ** 32))
    src = Flat(n, np.int8, 127).tile(blk.reshape(-1))
    dst = Flat(R16 * K, np.int8, 85)
    _lib.call("ivit_tile_operand_i8", src.ptr, K, rows, K, dst.ptr, st())
    torch.cuda.synchronize()
    bad = blocks_mismatch(dst.body, src.body, rows, K)
    assert bad == 0, f"{bad} bytes of the block layout differ from the documented place of their source byte"
    assert dst.guards_hold()
    unchanged(src)
    back = Flat(n, np.int8, 85)
    _lib.call("ivit_untile_operand_i8", dst.ptr, rows, K, back.ptr, K, st())
    check(back, blk.reshape(-1))


# ------------------------------------------------------------------------------------------- dense row passes
def _rows_pattern(rows, row_elems, dtype):
    """row r is a 1021-element random block read from phase 37 r on (no two rows alike)"""
    blk = torch.from_numpy(np.random.default_rng(rows).integers(-100, 100, size=1021).astype(dtype)).to(DEV)
    return blk, lambda r, a, e: blk[(torch.arange(a, e, device=DEV) + 37 * r) % 1021]


def test_window_rows_beyond_2_32_bytes():
    """ivit_window_rows has no leading dimension and bounds row_bytes at 2^20 (refused beyond, as the header says), so its far
    dimension is the rows: 2 x 48 x 48 tokens (4 x 4 windows, shift 2) of 2^20 bytes are 4.5 GiB per buffer.  Forward: dst row j is
    src row order[j]; inverse: back to the source"""
    import test_gpu_strides as S
    Bn, H, W, ws, shift = 2, 48, 48, 4, 2
    rows, RB = Bn * H * W, 2 ** 20
    assert rows * RB > 2 ** 32
    order = torch.from_numpy(S._win_order(np.arange(rows, dtype=np.int64)[:, None], Bn, H, ws, shift)[:, 0]).to(DEV)
    src, dst = Flat(rows * RB, np.int8, 127), Flat(rows * RB, np.int8, 85)
    blk = torch.from_numpy(np.random.default_rng(rows).integers(-100, 100, size=1021).astype(np.int8)).to(DEV)
    col = torch.arange(RB, device=DEV, dtype=torch.int32)
    sv, dv = src.body.view(rows, RB), dst.body.view(rows, RB)
    for r0 in range(0, rows, 64):          # row r: the block read from phase 37 r on (1021 is prime: no two rows alike)
        r = torch.arange(r0, min(rows, r0 + 64), device=DEV, dtype=torch.int32)
        sv[r0:r0 + 64] = blk[((col[None, :] + 37 * r[:, None]) % 1021).long()]
    with pytest.raises(_lib.IvitError, match="row_bytes must be a positive multiple of 16"):
        _lib.call("ivit_window_rows", src.ptr, dst.ptr, 1, 8, 8, RB + 16, ws, shift, 0, st())
    _lib.call("ivit_window_rows", src.ptr, dst.ptr, Bn, H, W, RB, ws, shift, 0, st())
    torch.cuda.synchronize()
    bad = sum(int((dv[j0:j0 + 64] != sv[order[j0:j0 + 64]]).any(dim=1).sum()) for j0 in range(0, rows, 64))
    assert bad == 0, f"{bad} window-order rows are not their source rows"
    assert dst.guards_hold() and src.guards_hold()
    back = Flat(rows * RB, np.int8, 85)
    _lib.call("ivit_window_rows", dst.ptr, back.ptr, Bn, H, W, RB, ws, shift, 1, st())
    torch.cuda.synchronize()
    assert torch.equal(back.body, src.body) and back.guards_hold()


def test_patch_merge_i16_beyond_2_31_elements():
    """ivit_patch_merge_i16 has no leading dimension; its far dimension is H * W * C: 4 x 4 tokens of C = 2^27 + 8 channels are
    2^31 + 128 int16 elements (4 GiB).  out [4, 4 C]: channel block (dy, dx) of token (i, j) is token (2 i + dy, 2 j + dx), blocks in
    the order (0, 0), (1, 0), (0, 1), (1, 1)"""
    Bn, H, W, C = 1, 4, 4, 2 ** 27 + 8
    assert H * W * C > 2 ** 31
    x, o = Flat(H * W * C, np.int16, 32767), Flat(H * W * C, np.int16, -21846)
    blk, gen = _rows_pattern(H * W, C, np.int16)
    for r in range(H * W):
        x.body[r * C:(r + 1) * C] = gen(r, 0, C)
    _lib.call("ivit_patch_merge_i16", x.ptr, o.ptr, Bn, H, W, C, st())
    torch.cuda.synchronize()
    xv, ov = x.body.view(H, W, C), o.body.view(H // 2, W // 2, 4, C)
    bad = [(i, j, b) for i in range(H // 2) for j in range(W // 2) for b, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1)))
           if not torch.equal(ov[i, j, b], xv[2 * i + dy, 2 * j + dx])]
    assert not bad, f"(token row, token column, channel block) {bad[:8]} are not their source token"
    assert o.guards_hold() and x.guards_hold()
