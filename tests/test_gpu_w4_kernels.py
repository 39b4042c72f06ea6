"""The 4-bit width of the C ABI (the width knobs of vit_quant.py:180-187 at 4): ivit_gemm_i8_requant_bits_ex,
ivit_gemm_i8_requant_residual_bits_ex, ivit_residual_requant_i8_bits, ivit_embed_assemble_i8_bits and softmax_bits = 4 of the three
wide attention entries, against the oracle (oracle.requant with bits = 4, oracle.shiftmax / shiftmax_compat and oracle/ibert.py
softmax with output_bit = 4), bit for bit, through tests/fenced.py: strided rows between poisoned pads, sentinel-filled outputs.

Shapes: the smallest that reach each kernel (docstring of tests/test_gpu_strides.py): M = 258 and 8 the small kernel; M = 8197, N = 96,
K = 64 / 128 the skinny-K forms; M = 2125, N = K = 192 the persistent kernel (layouts 0, row-major W with ldw = K + 64) and the
weights-in-registers kernel with IVIT_W_FRAGS / IVIT_W_FRAGS16, each also with block-layout A (and block-layout output where the entry
has one).  Attention at B = 1, H = 2: tokens 193 .. 208 the tuned form, fewer the general one, 209 .. 655 / 656 .. 1025 the two long forms.

Before anything is launched every case asserts, on the oracle's values alone, that a 4-bit clamp is what it tests (narrow_ok): at
least 1 % of the expected elements at -8 and 1 % at 7, at least half strictly between, and at least 1 % of the values in front of the
clamp in (7, 127] or [-128, -9] -- values an 8-bit clamp passes, so the 8-bit entry's result on the same operands is another one."""
import functools

import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic, shiftexp2d, shiftexp_band  # noqa: E402

import fenced  # noqa: E402

DEV = "cuda:0"
HD = 64
f32 = np.float32
_KEEP = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


def p(t):
    return _lib.ptr(t)


def fin(a, ld, poison=None, **kw):
    a = np.ascontiguousarray(a)
    b = fenced.input(a, ld, fenced.POISON[a.dtype] if poison is None else poison, device=DEV, **kw)
    _KEEP.append(b)
    return b


def fin_blocks(a):
    """[rows, K] int8 -> the block-layout operand (include/ivit_hip.h IVIT_LAYOUT_BLOCKS); the padding rows of the last block are poison"""
    rows, K = a.shape
    flat = np.full((rows + 15) // 16 * 16 * K, 127, np.int8)
    flat[fenced.block_offsets(rows, K)] = a
    b = fenced.input_blocks(flat, rows, K, 127, device=DEV)
    _KEEP.append(b)
    return b


def fout(rows, width, ld, dtype, expected, **kw):
    b = fenced.output(rows, width, ld, dtype, expected=expected, device=DEV, **kw)
    _KEEP.append(b)
    return b


def got_rows(o):
    """what an entry left in a fenced row-major output: [rows, width]"""
    return o.rows2d(o.fetch())[:, :o.width].copy()


def refused(name, *args):
    """IVIT_ERR_INVALID naming the width"""
    with pytest.raises(_lib.IvitError, match="bits") as ei:
        _lib.call(name, *args)
    assert "(-1)" in str(ei.value), f"{name}: expected IVIT_ERR_INVALID, got {ei.value}"


def narrow_ok(exp4, pre, what):
    """the conditions of the module docstring on a 4-bit expectation `exp4` and the values `pre` in front of its clamp"""
    n = exp4.size
    assert exp4.min() == -8 and exp4.max() == 7, what
    assert (exp4 == -8).sum() >= 0.01 * n and (exp4 == 7).sum() >= 0.01 * n, (what, (exp4 == -8).mean(), (exp4 == 7).mean())
    assert ((exp4 > -8) & (exp4 < 7)).sum() >= 0.5 * n, (what, ((exp4 > -8) & (exp4 < 7)).mean())
    passes8 = ((pre > 7) & (pre <= 127)) | ((pre >= -128) & (pre <= -9))
    assert passes8.sum() >= 0.01 * n, (what, passes8.mean())


# =========================================================================================== GEMM
BOUNDS = {4: (-8, 7), 8: (-128, 127)}


class Gemm:
    """one problem: A [M, K], W [N, K], bias, a per-channel requantiser that spreads the accumulators over about +-12 (the 4-bit
    clamp takes a seventh of them on either side), and a residual QuantAct whose two terms are each a few units wide"""

    def __init__(self, M, N, K, seed):
        rng = self.rng = np.random.default_rng(seed)
        self.M, self.N, self.K = M, N, K
        self.A = rng.integers(-128, 127, size=(M, K)).astype(np.int8)       # below the poison 127
        self.W = rng.integers(-128, 127, size=(N, K)).astype(np.int8)
        self.b = rng.integers(-50000, 50000, size=N).astype(np.int32)
        self.acc = orc.gemm_i8(self.A, self.W, self.b)
        sigma = 74.0 * 74.0 * np.sqrt(K)                                     # of a sum of K products of two uniform int8 values
        self.m, self.e = dyadic((rng.uniform(5.0, 8.0, size=N) / sigma).astype(f32), f32(1.0))
        self.md = self.m.astype(np.float64)
        self.pre = orc.requant(self.acc, self.md, self.e, 32)
        self.k = {b: orc.requant(self.acc, self.md, self.e, b) for b in (4, 8)}
        assert np.array_equal(self.k[4], np.clip(self.pre, -8, 7)) and np.array_equal(self.k[8], np.clip(self.pre, -128, 127))
        narrow_ok(self.k[4], self.pre, "requant")
        self.res = rng.integers(-128, 127, size=(M, N)).astype(np.int8)
        m1, e1 = dyadic(f32(0.61), f32(1.0))
        m2, e2 = dyadic(f32(0.047), f32(1.0))
        self.sc = (int(m1[0]), int(e1[0]), int(m2[0]), int(e2[0]))
        self.out = {}
        for bm in (4, 8):
            pre_o = orc.requant(self.k[bm], m1.astype(np.float64), e1, 32, z2=self.res.astype(np.int32), m2=m2.astype(np.float64), e2=e2)
            for bo in (4, 8):
                self.out[bm, bo] = orc.requant(self.k[bm], m1.astype(np.float64), e1, bo, z2=self.res.astype(np.int32),
                                               m2=m2.astype(np.float64), e2=e2)
                assert np.array_equal(self.out[bm, bo], np.clip(pre_o, *BOUNDS[bo]))
                if bo == 4:
                    narrow_ok(self.out[bm, 4], pre_o, f"residual ({bm}, 4)")
        # the middle clamp shows behind the residual QuantAct as well
        assert (self.out[4, 8] != self.out[8, 8]).mean() >= 0.01 and (self.out[4, 4] != self.out[8, 4]).mean() >= 0.01

    def operands(self, lda, ldw):
        """on the device: A and W in strided rows (the poison condition of A: a K loop one dword too long takes in the pads of A and
        W), bias and requantiser tables"""
        self.db = dev(self.b)
        self.me = (p(dev(self.m.view(np.int32))), p(dev(self.e)))
        Ww = np.concatenate([self.W, np.full((self.N, 4), 127, np.int8)], axis=1)
        self.a = fin(self.A, lda, 127, oracle=lambda Aw: orc.requant(orc.gemm_i8(Aw, Ww, self.b), self.md, self.e, 4), expected=self.k[4])
        self.w = fin(self.W, ldw, 127)
        return self

    def check_inputs(self):
        fenced.check(self.a)
        fenced.check(self.w)


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, seed):
    return Gemm(M, N, K, seed)


@pytest.mark.parametrize("M,N,K", [(258, 208, 128), (8, 192, 192)])
def test_gemm_bits_small_kernel(M, N, K):
    """gemm_i8_kernel (M < 2048): two tiles + 2 rows and one tile + 80 channels, and 8 class rows; lda = K + 16, ldw = K + 32,
    ldo = N + 16, ldr = N + 32; the residual entry at the four width pairs, out of place and in place"""
    g = gemm_case(M, N, K, 1).operands(K + 16, K + 32)
    head = (g.a.ptr, g.a.ld, g.w.ptr, g.w.ld, p(g.db), *g.me)
    o4 = fout(M, N, N + 16, np.int8, g.k[4])
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o4.ptr, o4.ld, M, N, K, 0, 4, st())
    fenced.check(o4, g.k[4])
    o8 = fout(M, N, N + 16, np.int8, g.k[8])
    _lib.call("ivit_gemm_i8_requant_ex", *head, o8.ptr, o8.ld, M, N, K, 0, st())
    fenced.check(o8, g.k[8])
    assert (got_rows(o8) != g.k[4]).mean() >= 0.01                       # the 8-bit entry gives another result
    o = fout(M, N, N + 16, np.int8, g.k[8])
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o.ptr, o.ld, M, N, K, 0, 8, st())
    fenced.check(o, got_rows(o8))                                        # bits = 8: the bytes of the entry it extends
    for bm, bo in ((4, 4), (4, 8), (8, 4), (8, 8)):
        exp = g.out[bm, bo]
        r = fin(g.res, N + 32)
        o = fout(M, N, N + 16, np.int8, exp)
        _lib.call("ivit_gemm_i8_requant_residual_bits_ex", *head, r.ptr, r.ld, *g.sc, o.ptr, o.ld, M, N, K, 0, bm, bo, st())
        fenced.check(o, exp)
        fenced.check(r)
        if (bm, bo) == (8, 8):
            o8 = fout(M, N, N + 16, np.int8, exp)
            _lib.call("ivit_gemm_i8_requant_residual_ex", *head, r.ptr, r.ld, *g.sc, o8.ptr, o8.ld, M, N, K, 0, st())
            fenced.check(o, got_rows(o8))
        _lib.call("ivit_gemm_i8_requant_residual_bits_ex", *head, r.ptr, r.ld, *g.sc, r.ptr, r.ld, M, N, K, 0, bm, bo, st())     # in place
        fenced.check(r, exp)
    g.check_inputs()


@pytest.mark.parametrize("K", [64, 128])
def test_gemm_bits_skinny_k(K):
    """gemm_i8_skinny_kernel (M >= 8192, plain requant only): M = 8192 + 5, N = 96, lda = ldw = K + 16, ldo = N + 16, the compile-time
    K = 64 and K = 128 forms"""
    M, N = 8197, 96
    g = gemm_case(M, N, K, 10 + K).operands(K + 16, K + 16)
    head = (g.a.ptr, g.a.ld, g.w.ptr, g.w.ld, p(g.db), *g.me)
    o4 = fout(M, N, N + 16, np.int8, g.k[4])
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o4.ptr, o4.ld, M, N, K, 0, 4, st())
    fenced.check(o4, g.k[4])
    o8 = fout(M, N, N + 16, np.int8, g.k[8])
    _lib.call("ivit_gemm_i8_requant_ex", *head, o8.ptr, o8.ld, M, N, K, 0, st())
    o = fout(M, N, N + 16, np.int8, g.k[8])
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o.ptr, o.ld, M, N, K, 0, 8, st())
    fenced.check(o, got_rows(o8))
    fenced.check(o, g.k[8])
    g.check_inputs()


def _packed(g, lay):
    """the fragment-packed copy of g.W made from its strided rows (lay 8: IVIT_W_FRAGS, 16: IVIT_W_FRAGS16)"""
    Wf = torch.zeros((g.N + 63) // 64 * 64 * g.K, dtype=torch.int8, device=DEV)
    _KEEP.append(Wf)
    if lay == 8:
        _lib.call("ivit_pack_weight_frags_i8", g.w.ptr, g.w.ld, g.N, g.K, p(Wf), st())
    else:
        _lib.call("ivit_pack_weight_frags16_i8", g.w.ptr, g.w.ld, g.N, g.K, p(Wf), st())
    return Wf


@pytest.mark.parametrize("a_blocks", [0, 1], ids=["A_rows", "A_blocks"])
@pytest.mark.parametrize("lay", [0, 8, 16], ids=["persistent", "w_frags", "w_frags16"])
def test_gemm_bits_large_kernels(lay, a_blocks):
    """M = 2048 + 77, N = K = 192: gemm_i8_pers_kernel (row-major W with ldw = K + 64) and gemm_i8_wreg_kernel in both fragment orders;
    A in strided rows (lda = K + 16) or in the block layout, and then the plain entry's output in the block layout too"""
    M, N, K = 2125, 192, 192
    g = gemm_case(M, N, K, 20).operands(K + 16, K + 64)
    w = (g.w.ptr, g.w.ld) if lay == 0 else (p(_packed(g, lay)), K)
    ab = fin_blocks(g.A) if a_blocks else None
    a = (ab.ptr, K) if a_blocks else (g.a.ptr, g.a.ld)
    head = (*a, *w, p(g.db), *g.me)
    lay_rq = lay | (5 if a_blocks else 0)                               # IVIT_A_BLOCKS | IVIT_OUT_BLOCKS
    ldo = N if a_blocks else N + 16
    o4 = fout(M, N, ldo, np.int8, g.k[4], blocks=bool(a_blocks))
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o4.ptr, o4.ld, M, N, K, lay_rq, 4, st())
    fenced.check(o4, g.k[4])
    o8 = fout(M, N, ldo, np.int8, g.k[8], blocks=bool(a_blocks))
    _lib.call("ivit_gemm_i8_requant_ex", *head, o8.ptr, o8.ld, M, N, K, lay_rq, st())
    fenced.check(o8, g.k[8])
    o = fout(M, N, ldo, np.int8, g.k[8], blocks=bool(a_blocks))
    _lib.call("ivit_gemm_i8_requant_bits_ex", *head, o.ptr, o.ld, M, N, K, lay_rq, 8, st())
    assert np.array_equal(o.fetch(), o8.fetch())                        # bits = 8: the whole allocation, byte for byte
    lay_res = lay | a_blocks
    for bm, bo in ((4, 4), (4, 8), (8, 4), (8, 8)):
        exp = g.out[bm, bo]
        r = fin(g.res, N + 32)
        o = fout(M, N, N + 16, np.int8, exp)
        _lib.call("ivit_gemm_i8_requant_residual_bits_ex", *head, r.ptr, r.ld, *g.sc, o.ptr, o.ld, M, N, K, lay_res, bm, bo, st())
        fenced.check(o, exp)
        fenced.check(r)
        if (bm, bo) == (8, 8):
            o8 = fout(M, N, N + 16, np.int8, exp)
            _lib.call("ivit_gemm_i8_requant_residual_ex", *head, r.ptr, r.ld, *g.sc, o8.ptr, o8.ld, M, N, K, lay_res, st())
            fenced.check(o, got_rows(o8))
        _lib.call("ivit_gemm_i8_requant_residual_bits_ex", *head, r.ptr, r.ld, *g.sc, r.ptr, r.ld, M, N, K, lay_res, bm, bo, st())   # in place
        fenced.check(r, exp)
    if ab is not None:
        fenced.check(ab)
    g.check_inputs()


# =========================================================================================== row operators
def test_residual_requant_bits():
    """ivit_residual_requant_i8_bits at n = 1000 (four blocks of 256 threads, the last one partial)"""
    n = 1000
    rng = np.random.default_rng(n)
    a = rng.integers(-8, 8, size=(1, n)).astype(np.int8)
    b = rng.integers(-128, 127, size=(1, n)).astype(np.int8)
    m1, e1 = dyadic(f32(0.93), f32(1.0))
    m2, e2 = dyadic(f32(0.055), f32(1.0))
    sc = lambda bits: orc.requant(a.astype(np.int32), m1.astype(np.float64), e1, bits, z2=b.astype(np.int32), m2=m2.astype(np.float64), e2=e2)  # noqa: E731
    exp4, exp8, pre = sc(4), sc(8), sc(32)
    narrow_ok(exp4, pre, "residual_requant")
    xa, xb = fin(a, n), fin(b, n)
    args = (xa.ptr, int(m1[0]), int(e1[0]), xb.ptr, int(m2[0]), int(e2[0]))
    o4 = fout(1, n, n, np.int8, exp4)
    _lib.call("ivit_residual_requant_i8_bits", *args, o4.ptr, n, 4, st())
    fenced.check(o4, exp4)
    o8 = fout(1, n, n, np.int8, exp8)
    _lib.call("ivit_residual_requant_i8", *args, o8.ptr, n, st())
    fenced.check(o8, exp8)
    assert (got_rows(o8) != exp4).mean() >= 0.01
    o = fout(1, n, n, np.int8, exp8)
    _lib.call("ivit_residual_requant_i8_bits", *args, o.ptr, n, 8, st())
    fenced.check(o, got_rows(o8))
    fenced.check(xa)
    fenced.check(xb)


@pytest.mark.parametrize("B,T,C", [(2, 5, 64), (2, 197, 192)])
def test_embed_assemble_bits(B, T, C):
    """ivit_embed_assemble_i8_bits: out[b][0] = cls_row, out[b][1 + i] = clamp4(RNE(patch * M) + pos_add[1 + i]) (vit_quant.py:290-296);
    the class row and pos_add are the caller's, at the widths of their own QuantActs"""
    rng = np.random.default_rng(B * T + C)
    patch = rng.integers(-128, 127, size=(B * (T - 1), C)).astype(np.int8)
    pos = rng.integers(-3, 4, size=(T, C)).astype(np.int16)
    cls = rng.integers(-8, 8, size=(1, C)).astype(np.int8)
    m, e = dyadic(f32(0.066), f32(1.0))
    pre = orc.requant(patch.astype(np.int32), m.astype(np.float64), e, 32).reshape(B, T - 1, C) + pos[None, 1:].astype(np.int32)
    exp = {}
    for bits in (4, 8):
        full = np.empty((B, T, C), np.int32)
        full[:, 0] = cls[0]
        full[:, 1:] = np.clip(pre, *BOUNDS[bits])
        exp[bits] = full.reshape(B * T, C)
    narrow_ok(exp[4].reshape(B, T, C)[:, 1:], pre, "embed")
    xp, xo, xc = fin(patch, C), fin(pos, C), fin(cls, C)
    args = (xp.ptr, xo.ptr, xc.ptr, int(m[0]), int(e[0]))
    o4 = fout(B * T, C, C, np.int8, exp[4])
    _lib.call("ivit_embed_assemble_i8_bits", *args, o4.ptr, B, T, C, 4, st())
    fenced.check(o4, exp[4])
    o8 = fout(B * T, C, C, np.int8, exp[8])
    _lib.call("ivit_embed_assemble_i8", *args, o8.ptr, B, T, C, st())
    fenced.check(o8, exp[8])
    assert (got_rows(o8) != exp[4]).mean() >= 0.01
    o = fout(B * T, C, C, np.int8, exp[8])
    _lib.call("ivit_embed_assemble_i8_bits", *args, o.ptr, B, T, C, 8, st())
    fenced.check(o, got_rows(o8))
    for x in (xp, xo, xc):
        fenced.check(x)


@pytest.mark.parametrize("bits", [0, 2, 6, 16])
def test_other_widths_are_refused(bits):
    """IVIT_ERR_INVALID before any launch: the sentinel-filled outputs are untouched (operands of the smallest GEMM case)"""
    M, N, K = 8, 192, 192
    g = gemm_case(M, N, K, 1).operands(K + 16, K + 32)
    head = (g.a.ptr, g.a.ld, g.w.ptr, g.w.ld, p(g.db), *g.me)
    r = fin(g.res, N + 32)
    o = fout(M, N, N + 16, np.int8, g.k[4])
    untouched = o.fetch().copy()
    refused("ivit_gemm_i8_requant_bits_ex", *head, o.ptr, o.ld, M, N, K, 0, bits, st())
    for bm, bo in ((bits, 4), (8, bits), (bits, bits)):
        refused("ivit_gemm_i8_requant_residual_bits_ex", *head, r.ptr, r.ld, *g.sc, o.ptr, o.ld, M, N, K, 0, bm, bo, st())
    refused("ivit_residual_requant_i8_bits", r.ptr, g.sc[0], g.sc[1], r.ptr, g.sc[2], g.sc[3], o.ptr, 64, bits, st())
    pos = fin(np.zeros((2, 64), np.int16), 64)
    refused("ivit_embed_assemble_i8_bits", r.ptr, pos.ptr, r.ptr, g.sc[0], g.sc[1], o.ptr, 1, 2, 64, bits, st())
    torch.cuda.synchronize()
    assert np.array_equal(o.fetch(), untouched)
    fenced.check(r)


# =========================================================================================== attention, softmax_bits = 4
def attn_scales(natural, s_mult):
    """as tests/attention_ref.py scales() at 4 bits, with a natural Shiftmax scale wide enough for peaked rows (a row whose
    probabilities are all below 1/8 is all zero at 4 bits): the Shiftmax output scale is 2^-3"""
    s_a1 = f32(0.0571 if natural else 2.0 ** -4)
    s_S = f32(f32(f32(s_a1 * s_a1) * f32(0.125)) * f32(s_mult))
    s_at = f32(0.1437 if natural else 2.0 ** -3)
    s_pv = f32(f32(2.0 ** -3) * s_a1)
    s_a2 = f32(0.0273 if natural else 2.0 ** -5)
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(s_pv, s_a2)
    if not natural:
        assert ((int(ms[0]) & (int(ms[0]) - 1)) == 0) == (s_mult == 1.0)
    return s_at, ms, es, mo, eo


def attn_inputs(T, seed):
    """q, k, v for B = 1, H = 2 with a peak in every score row (at 4 bits a row whose probabilities are all below 1/8 is all zero, and
    of random scores most rows are): query i points along dimension i % 64, key j along j % 64 with a length that falls with j // 64,
    so that query i prefers key i % 64, then i % 64 + 64, ...; noise on top, v random.  In head 0 query 2 sees key 3 at +127 and every
    other key at -128 after the requantisation: a one-hot row"""
    rng = np.random.default_rng(seed)
    qkv = rng.normal(0, 5, size=(3, 1, 2, T, HD))
    qkv[2] = rng.normal(0, 40, size=(1, 2, T, HD))
    t = np.arange(T)
    qkv[0, :, :, t, t % HD] += 119.0
    qkv[1, :, :, t, t % HD] += (119.0 - 9.0 * (t // HD))[:, None, None]
    qkv = np.clip(np.rint(qkv), -128, 127).astype(np.int8)
    qkv[0, 0, 0, 2] = 0
    qkv[0, 0, 0, 2, :8] = 127
    qkv[1, 0, 0, :, :8] = -127
    qkv[1, 0, 0, 3, :8] = 127
    return qkv


def attn_expected(qkv, ms, es, mo, eo, softmax, one_hot):
    """per (image, head): matmul -> requant -> softmax (the probabilities as integers) -> int64 P.V -> requant.  The conditions on the
    probabilities: none negative, at least one non-zero in every row, some row with one of 4 or more, the one-hot row at `one_hot`"""
    _, B, H, T, _ = qkv.shape
    exp = np.empty((B * T, H * HD), np.int32)
    pmax = 0
    for h in range(H):
        S = orc.gemm_i8(qkv[0, 0, h], qkv[1, 0, h])
        ka = orc.requant(S, ms.astype(np.float64), es, 8)
        P = softmax(ka).astype(np.int64)
        assert P.min() >= 0 and P.max() <= one_hot and (P.max(axis=1) >= 1).all(), (h, P.max(), int((P.max(axis=1) < 1).sum()))
        pmax = max(pmax, int(P.max()))
        if h == 0:
            assert P[2, 3] == one_hot and P[2].sum() == one_hot, P[2]
        O = P @ qkv[2, 0, h].astype(np.int64)
        exp[:, h * HD:(h + 1) * HD] = orc.requant(O.astype(np.int32), mo.astype(np.float64), eo, 8)
    assert pmax >= 4 and np.abs(exp).max() > 20
    return exp


@functools.lru_cache(maxsize=None)
def shiftmax_case(T, natural, s_mult):
    s_at, ms, es, mo, eo = attn_scales(natural, s_mult)
    qkv = attn_inputs(T, 900 + T)
    sm = orc.shiftmax_compat if natural else orc.shiftmax
    exp = attn_expected(qkv, ms, es, mo, eo, lambda ka: sm(ka, s_at, output_bit=4), 7)
    return qkv, (int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0])), exp


@functools.lru_cache(maxsize=None)
def shiftmax_tables(s_at):
    tab = shiftexp2d(f32(s_at))
    bt, bw = shiftexp_band(tab)
    assert 16 <= bw <= 256
    return tab, bt, bw


def table_args(s_at, form):
    if form == "pow2":
        return None, None, 0
    tab, bt, bw = shiftmax_tables(s_at)
    if form == "band":
        return None, p(dev(bt.view(np.int32))), bw
    return p(dev(tab.view(np.int32))), None, 0


SHIFTMAX_FORMS = [("pow2", 1.0), ("pow2", 1.37), ("exp2d", 1.37), ("band", 1.37)]


@pytest.mark.parametrize("blocks", [0, 1], ids=["rows", "blocks"])
@pytest.mark.parametrize("form,s_mult", SHIFTMAX_FORMS)
@pytest.mark.parametrize("T", [197, 193, 208, 50, 5])
def test_attention_wide_4_bit_probabilities(T, form, s_mult, blocks):
    """ivit_attention_fused_i8_wide, softmax_bits = 4: the tuned form (193 .. 208 tokens) and the general one; the float32 and the
    float64 requantisation of the scores, the three Shiftmax regimes, both output layouts"""
    qkv, sc, exp = shiftmax_case(T, form != "pow2", s_mult)
    x = fin(qkv.reshape(-1, HD), HD)
    o = fout(T, 2 * HD, 2 * HD, np.int8, exp, blocks=bool(blocks))
    _lib.call("ivit_attention_fused_i8_wide", x.ptr, o.ptr, 1, 2, T, HD, *sc, *table_args(sc[2], form), 4, blocks, st())
    fenced.check(o, exp)
    fenced.check(x)


@pytest.mark.parametrize("blocks", [0, 1], ids=["rows", "blocks"])
@pytest.mark.parametrize("form,s_mult", SHIFTMAX_FORMS)
@pytest.mark.parametrize("T", [209, 577, 785])
def test_attention_wide_long_4_bit_probabilities(T, form, s_mult, blocks):
    """ivit_attention_fused_i8_wide_long, softmax_bits = 4: 209 and 577 tokens the 1024-thread form, 785 the 768-thread one"""
    qkv, sc, exp = shiftmax_case(T, form != "pow2", s_mult)
    x = fin(qkv.reshape(-1, HD), HD)
    o = fout(T, 2 * HD, 2 * HD, np.int8, exp, blocks=bool(blocks))
    _lib.call("ivit_attention_fused_i8_wide_long", x.ptr, o.ptr, 1, 2, T, HD, *sc, *table_args(sc[2], form), 4, blocks, st())
    fenced.check(o, exp)
    fenced.check(x)


@functools.lru_cache(maxsize=None)
def ibert_case(T, natural):
    """IBERTIntSoftmax(output_bit = 4) behind the requantised scores: oracle/ibert.py softmax with the range of its internal
    16-bit QuantAct as calibrated (the largest exponent maps to 32767), so that a one-hot row gives p = 8"""
    s_at, ms, es, mo, eo = attn_scales(natural, 1.37)
    qkv = attn_inputs(T, 700 + T)
    ex = ib.softmax(np.arange(-128, 128, dtype=np.int32)[None, :], s_at, -1.0, 1.0, return_exp=True)[3]
    act = (float(ex.min()), float(ex.max()))

    def softmax(ka):
        out, s_out, ninexact = ib.softmax(ka, s_at, *act, output_bit=4)
        assert s_out == f32(0.125) and ninexact == 0            # row sums below 2^24: exact in any order
        return out
    exp = attn_expected(qkv, ms, es, mo, eo, softmax, 8)
    return qkv, s_at, act, (int(ms[0]), int(es[0]), int(mo[0]), int(eo[0])), exp


@pytest.mark.parametrize("blocks", [0, 1], ids=["rows", "blocks"])
@pytest.mark.parametrize("natural,band", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["pow2-table", "pow2-band", "natural-table", "natural-band"])
@pytest.mark.parametrize("T", [193, 197, 207])
def test_attention_ibert_wide_4_bit_probabilities(T, natural, band, blocks):
    """ivit_attention_fused_i8_ibert_wide, softmax_bits = 4: p = floor(fl32(e * factor) / 2^29) in [0, 8], the full table and its band form"""
    qkv, s_at, act, sc, exp = ibert_case(T, natural)
    x0i, bi, ci, exp_sf, act_sf, ma, ea = ib.softmax_constants(s_at, *act)
    tab = torch.zeros(65536, dtype=torch.float32, device=DEV)
    _KEEP.append(tab)
    _lib.call("ivit_ibert_softmax_build_table", float(s_at), float(x0i), float(bi), float(ci), float(exp_sf), float(act_sf), int(ma), int(ea),
              p(tab), st())
    bandt, bw = None, 0
    if band:
        bt, bw = shiftexp_band(tab.cpu().numpy().view(np.uint32).reshape(256, 256))
        assert bw and 16 <= bw <= 256
        bandt = dev(bt.view(np.float32).reshape(-1))
    x = fin(qkv.reshape(-1, HD), HD)
    o = fout(T, 2 * HD, 2 * HD, np.int8, exp, blocks=bool(blocks))
    _lib.call("ivit_attention_fused_i8_ibert_wide", x.ptr, o.ptr, 1, 2, T, HD, *sc, p(tab), p(bandt), bw, 4, blocks, st())
    fenced.check(o, exp)
    fenced.check(x)
