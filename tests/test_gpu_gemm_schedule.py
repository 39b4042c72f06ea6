"""GPU parity of the int8 GEMM's tile scheduling: the WHOLE output of launches with more tiles than workgroup slots against an
exact reference, for gemm_i8_wreg_kernel (both fragment forms) and gemm_i8_pers_kernel, all epilogues.

What a workgroup does from its second tile on -- the prefetch under the epilogue, the double-buffered per-channel tables, the
waits across the tile boundary, the change from a full tile to a half tile -- and how a sparse last round is split shows only
in launches of more than 512 tiles.  The shapes (tests/gemm_sched_ref.py) hold every regime of the launcher's arithmetic at
K = 192, where an exact product of 30 M outputs is one float32 BLAS call.  Every output starts from a sentinel, so a tile that
no workgroup computes fails, and a failure names the first differing tile."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_sched_ref as gs  # noqa: E402
import test_gpu_ops as ops  # noqa: E402
from test_gpu_ops import DEV, _block_layout_host, _head_major, dev, dyadic, me_dev, rand_me, st  # noqa: E402

K = gs.K_SCHED
SENT = 77               # every output buffer starts as this; no 16 x 64 block of a reference consists of it (checked)
HD = 64
FORMS = {"frags": ("wreg", 8), "frags16": ("wreg", 16), "pers": ("pers", 0)}      # form -> (shape table, fragment layout bit)
NO_SPLIT, WIDE_SPLIT = 1 << 27, 1 << 11      # ivit_debug_set_gemm_flags: no tail split; split up to 2R <= 512


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    ops._KEEP.clear()


def _i8(x):
    return np.ascontiguousarray(x.astype(np.int8))


class Reference:
    """operands and expected outputs of one table entry; each expected output is computed on first use and kept"""

    def __init__(self, table, sid):
        (self.tt, self.tc), shapes = gs.TABLES[table]
        self.M, self.N = M, N = shapes[sid]
        rng, self.A, self.W, self.b = gs.tie_operands(M, N, K, M + N)
        self.m, self.e = rand_me(rng, N, -16, -9)
        self.m[::5] = 1 << 30                    # power-of-two multipliers: exact .5 ties -> the float64 path of a batch
        self.res = rng.integers(-128, 128, size=(M, N), dtype=np.int8)
        self.m16, self.e16 = rand_me(rng, N, -8, 1)      # the 16-bit intermediate spans and exceeds the int16 range
        self.lut = rng.integers(-128, 128, size=256, dtype=np.int8)
        # residual QuantAct multipliers of test_gemm_weight_fragment_layout: (m1, e1) runs on float32 fmas; m3 = 2^30 - 1, e3 = 31
        # is one step below 1/2, the launcher's exhaustive check rejects its float32 image and the float64 form runs
        self.m1, self.e1 = dyadic(np.float32(0.7 * 2 ** -4), np.float32(2 ** -4))
        self.m2, self.e2 = dyadic(np.float32(2 ** -5), np.float32(2 ** -4))
        self.m3, self.e3 = np.array([(1 << 30) - 1], np.uint32), np.array([31], np.int32)
        # 16-bit residual QuantActs: EPI_RESID16 with sums on both sides of the int16 range; EPI_RQ16_RES16 with a scale pair of
        # test_gemm_requant_i16_residual_i16
        self.m4, self.e4 = dyadic(np.float32(0.02), np.float32(0.002))        # k8 * 10 + res16 * 1.5: a third of the sums saturate
        self.m5, self.e5 = dyadic(np.float32(0.003), np.float32(0.002))
        self.m6, self.e6 = dyadic(np.float32(0.3337), np.float32(0.0517))
        self.m7, self.e7 = dyadic(np.float32(0.0421), np.float32(0.0517))
        self.T = max(d for d in range(1, 1025) if M % d == 0)     # tokens per image of the q/k/v epilogue: any divisor of M

    @functools.cached_property
    def res16(self):
        rng = np.random.default_rng(self.M + self.N + 1)
        return rng.integers(-32768, 32768, size=(self.M, self.N), dtype=np.int16)

    @functools.cached_property
    def acc(self):
        return gs.gemm_ref(self.A, self.W, self.b)

    @functools.cached_property
    def k8_32(self):
        return orc.requant(self.acc, self.m.astype(np.float64), self.e, 8)

    @functools.cached_property
    def k8(self):
        return _i8(self.k8_32)

    def _resid(self, ma, ea):
        return _i8(orc.requant(self.k8_32, ma.astype(np.float64), ea, 8, z2=self.res.astype(np.int32), m2=self.m2.astype(np.float64),
                               e2=self.e2))

    @functools.cached_property
    def resid_f32(self):
        return self._resid(self.m1, self.e1)

    @functools.cached_property
    def resid_f64(self):
        return self._resid(self.m3, self.e3)

    @functools.cached_property
    def blocks(self):
        """the block-layout output; the pad rows of the last 16-row group are never written"""
        exp = _block_layout_host(self.k8)
        M16 = self.M // 16 * 16
        if M16 < self.M:
            written = _block_layout_host(np.ones((self.M - M16, self.N), np.int8))
            exp[M16 * self.N:][written == 0] = SENT
        return exp

    @functools.cached_property
    def qkv(self):
        return np.ascontiguousarray(_head_major(self.k8, self.M // self.T, self.T, self.N // (3 * HD), HD)).reshape(-1)

    @functools.cached_property
    def resid16(self):
        """EPI_RESID16: the int8 requant, then the two-operand QuantAct with a 16-bit residual and output"""
        return orc.requant(self.k8_32, self.m4.astype(np.float64), self.e4, 16, z2=self.res16.astype(np.int32),
                           m2=self.m5.astype(np.float64), e2=self.e5).astype(np.int16)

    @functools.cached_property
    def rq16_resid16(self):
        """EPI_RQ16_RES16: a 16-bit per-channel QuantAct of the accumulators, then the 16-bit residual QuantAct"""
        k16 = orc.requant(self.acc, self.m16.astype(np.float64), self.e16, 16)
        return orc.requant(k16, self.m6.astype(np.float64), self.e6, 16, z2=self.res16.astype(np.int32),
                           m2=self.m7.astype(np.float64), e2=self.e7).astype(np.int16)

    @functools.cached_property
    def mapped(self):
        return np.ascontiguousarray(self.lut[self.k8_32 + 128])


@functools.lru_cache(maxsize=2)     # the cases are ordered by table entry: both fragment forms and their lab runs share one
def reference(table, sid):
    return Reference(table, sid)


def first_bad_tile(out, exp, ref, layout="rows"):
    """None if equal; else (token tile, channel tile) of the first differing element, and how many tiles differ"""
    if torch.equal(out, exp):
        return None
    idx = (out != exp).reshape(-1).nonzero().reshape(-1)
    N, tt, tc = ref.N, ref.tt, ref.tc
    if layout == "rows":
        ld = out.shape[1]
        row, col = idx // ld, idx % ld
    elif layout == "blocks":          # include/ivit_hip.h IVIT_LAYOUT_BLOCKS: 1 KB blocks of 16 rows x 64 bytes
        blk = idx // 1024
        row, col = (blk // (N >> 6)) * 16 + ((idx % 1024) >> 6), (blk % (N >> 6)) * 64
    else:                             # [3, B, H, T, hd]
        H = N // (3 * HD)
        d, tok, h, b, which = idx % HD, (idx // HD) % ref.T, (idx // (HD * ref.T)) % H, (idx // (HD * ref.T * H)) % (ref.M // ref.T), idx // (ref.M * H * HD)
        row, col = b * ref.T + tok, (which * H + h) * HD + d
    tiles = torch.unique((row // tt) * 4096 + col // tc)
    return (int(row[0]) // tt, int(col[0]) // tc), f"{idx.numel()} elements in {tiles.numel()} tiles differ"


def assert_sentinel_free(exp2d):
    """no 16 x 64 block of an expected output (a quarter of a wave's share of a half tile) is all sentinel: a work item that is
    never run, or a wave of it that stores nothing, leaves a difference"""
    M, N = exp2d.shape
    ne = exp2d != SENT
    M16 = M // 16 * 16
    assert bool(ne[:M16].reshape(M16 // 16, 16, N // 64, 64).any(dim=3).any(dim=1).all())
    if M16 < M:
        assert bool(ne[M16:].reshape(M - M16, N // 64, 64).any(dim=2).any(dim=0).all())


class Launch:
    """device operands of one (form, table entry) and the entry points on them"""

    def __init__(self, form, ref):
        self.ref, (_, self.FR) = ref, FORMS[form]
        M, N = ref.M, ref.N
        self.dA, self.db = dev(ref.A), dev(ref.b)
        self.md, self.ed = me_dev(ref.m, ref.e)
        dW = dev(ref.W)
        self.At = torch.zeros((M + 15) // 16 * 16 * K, dtype=torch.int8, device=DEV)
        _lib.call("ivit_tile_operand_i8", _lib.ptr(self.dA), K, M, K, _lib.ptr(self.At), st())
        if self.FR:
            self.Wrow = torch.zeros(N * K, dtype=torch.int8, device=DEV)
            _lib.call("ivit_pack_weight_frags_i8" if self.FR == 8 else "ivit_pack_weight_frags16_i8", _lib.ptr(dW), K, N, K, _lib.ptr(self.Wrow), st())
            self.Wblk = self.Wrow
            self.lay_row, self.lay_blk = self.FR, self.FR | 1
        else:
            self.Wrow = dW
            self.Wblk = torch.zeros(N * K, dtype=torch.int8, device=DEV)
            _lib.call("ivit_tile_operand_i8", _lib.ptr(dW), K, N, K, _lib.ptr(self.Wblk), st())
            self.lay_row, self.lay_blk = 0, 3        # IVIT_A_BLOCKS | IVIT_W_BLOCKS

    def _ops(self, lay):
        blk = lay & 1
        return (self.At if blk else self.dA), (self.Wblk if blk else self.Wrow)

    def out(self, shape, dtype=torch.int8):
        return torch.full(shape, SENT, dtype=dtype, device=DEV)

    def plain(self, lay, out_blocks=False, lut=None, A=None, lda=K, ldo=None):
        r = self.ref
        a, w = self._ops(lay)
        a = a if A is None else A
        ldo = r.N if ldo is None else ldo
        out = self.out(((r.M + 15) // 16 * 16 * r.N,)) if out_blocks else self.out((r.M, ldo))
        if lut is None:
            _lib.call("ivit_gemm_i8_requant_ex", _lib.ptr(a), lda, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(self.md), _lib.ptr(self.ed),
                      _lib.ptr(out), ldo, r.M, r.N, K, lay | (4 if out_blocks else 0), st())
        else:
            _lib.call("ivit_gemm_i8_requant_lut_ex", _lib.ptr(a), lda, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(self.md), _lib.ptr(self.ed),
                      _lib.ptr(lut), _lib.ptr(out), ldo, r.M, r.N, K, lay, st())
        return out

    def residual(self, lay, dres, ma, ea, A=None, lda=K, ldo=None, ldr=None):
        r = self.ref
        a, w = self._ops(lay)
        a = a if A is None else A
        ldo, ldr = (r.N if ldo is None else ldo), (r.N if ldr is None else ldr)
        out = self.out((r.M, ldo))
        _lib.call("ivit_gemm_i8_requant_residual_ex", _lib.ptr(a), lda, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(self.md), _lib.ptr(self.ed),
                  _lib.ptr(dres), ldr, int(ma[0]), int(ea[0]), int(r.m2[0]), int(r.e2[0]), _lib.ptr(out), ldo, r.M, r.N, K, lay, st())
        return out

    def qkv(self, lay):
        r = self.ref
        a, w = self._ops(lay)
        out = self.out((r.M * r.N,))
        _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(self.md), _lib.ptr(self.ed),
                  _lib.ptr(out), r.T, r.N // (3 * HD), HD, r.M, r.N, K, lay, st())
        return out

    def residual16(self, lay, dres16, rq16):
        """rq16 False: ivit_gemm_i8_requant_residual_i16_ex (EPI_RESID16); True: ivit_gemm_i8_requant_i16_residual_i16_ex"""
        r = self.ref
        a, w = self._ops(lay)
        out = self.out((r.M, r.N), torch.int16)
        if rq16:
            md, ed = me_dev(r.m16, r.e16)
            _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", _lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(md), _lib.ptr(ed),
                      _lib.ptr(dres16), r.N, int(r.m6[0]), int(r.e6[0]), int(r.m7[0]), int(r.e7[0]), _lib.ptr(out), r.N, r.M, r.N, K, lay, st())
        else:
            _lib.call("ivit_gemm_i8_requant_residual_i16_ex", _lib.ptr(a), K, _lib.ptr(w), K, _lib.ptr(self.db), _lib.ptr(self.md), _lib.ptr(self.ed),
                      _lib.ptr(dres16), r.N, int(r.m4[0]), int(r.e4[0]), int(r.m5[0]), int(r.e5[0]), _lib.ptr(out), r.N, r.M, r.N, K, lay, st())
        return out


def _cases(sids):
    return [pytest.param(form, sid, id=f"{sid}-{form}") for sid in sids for form in FORMS]


def _collect(bad, what, got):
    if got is not None:
        bad.append((what,) + got)


@pytest.mark.parametrize("form,sid", _cases("ABCDEFG"))
def test_gemm_schedule_whole_output(form, sid):
    """every epilogue of the kernel form, byte for byte over the whole output, against the exact reference: plain (row-major A,
    block-layout A, block-layout output), both residual forms, head-major q/k/v where N % 192 == 0, the 16-bit residual entries,
    the output map on entries A and F.  Failures are reported as (epilogue, first differing (token tile, channel tile), extent)."""
    table, FR = FORMS[form]
    ref = reference(table, sid)
    L = Launch(form, ref)
    k8 = dev(ref.k8)
    assert_sentinel_free(k8)
    bad = []
    _collect(bad, "plain, row-major A", first_bad_tile(L.plain(L.lay_row), k8, ref))
    _collect(bad, "plain, block-layout A", first_bad_tile(L.plain(L.lay_blk), k8, ref))
    _collect(bad, "block-layout output", first_bad_tile(L.plain(L.lay_blk, out_blocks=True), dev(ref.blocks), ref, "blocks"))
    dres = dev(ref.res)
    for what, lay, (ma, ea), exp in (("residual, float32 form", L.lay_row, (ref.m1, ref.e1), ref.resid_f32),
                                     ("residual, float64 form", L.lay_blk, (ref.m3, ref.e3), ref.resid_f64)):
        dexp = dev(exp)
        assert_sentinel_free(dexp)
        _collect(bad, what, first_bad_tile(L.residual(lay, dres, ma, ea), dexp, ref))
    if ref.N % (3 * HD) == 0:
        _collect(bad, f"q/k/v, {ref.T} tokens", first_bad_tile(L.qkv(L.lay_blk), dev(ref.qkv), ref, "qkv"))
    dres16 = dev(ref.res16)
    d16 = dev(ref.resid16)
    assert_sentinel_free(d16)
    _collect(bad, "16-bit residual", first_bad_tile(L.residual16(L.lay_row, dres16, False), d16, ref))
    if FR == 8:          # csrc/gemm.hip: among the tile-looping kernels only the 32x32x32 fragment form has EPI_RQ16_RES16
        d1616 = dev(ref.rq16_resid16)
        assert_sentinel_free(d1616)
        _collect(bad, "16-bit QuantAct + 16-bit residual", first_bad_tile(L.residual16(L.lay_row, dres16, True), d1616, ref))
    if FR and sid in "AF":
        dmap = dev(ref.mapped)
        assert_sentinel_free(dmap)
        _collect(bad, "output map", first_bad_tile(L.plain(L.lay_row, lut=dev(ref.lut)), dmap, ref))
    assert not bad, (form, sid, gs.regime(ref.M, ref.N, ref.tt, ref.tc), bad)


@pytest.mark.parametrize("flag", [NO_SPLIT, WIDE_SPLIT], ids=["no_split", "split_to_512"])
@pytest.mark.parametrize("form,sid", _cases("ABCDEF"))
def test_gemm_schedule_split_threshold(form, sid, flag):
    """the lab build with the tail split off (bit 27) and extended to 2R <= 512 (bit 11): every entry runs under the schedule
    the product's threshold does not give it, plain and residual epilogues, whole output"""
    table, FR = FORMS[form]
    ref = reference(table, sid)
    k8, dres = dev(ref.k8), dev(ref.res)
    bad = []
    with _lib.lab_session():
        _lib.call("ivit_debug_set_gemm_flags", flag)
        L = Launch(form, ref)
        _collect(bad, "plain, row-major A", first_bad_tile(L.plain(L.lay_row), k8, ref))
        _collect(bad, "plain, block-layout A", first_bad_tile(L.plain(L.lay_blk), k8, ref))
        _collect(bad, "residual, float32 form", first_bad_tile(L.residual(L.lay_blk, dres, ref.m1, ref.e1), dev(ref.resid_f32), ref))
        _collect(bad, "residual, float64 form", first_bad_tile(L.residual(L.lay_row, dres, ref.m3, ref.e3), dev(ref.resid_f64), ref))
    assert not bad, (form, sid, flag, bad)


@pytest.mark.parametrize("form,sid", _cases("AF"))
def test_gemm_schedule_strides(form, sid):
    """lda = K + 64, ldo = N + 16, ldr = N + 32 on multi-round launches (row-major operands): plain and residual epilogues equal the
    reference and the pad columns of the output keep their sentinel"""
    table, FR = FORMS[form]
    ref = reference(table, sid)
    M, N = ref.M, ref.N
    L = Launch(form, ref)
    A2 = torch.full((M, K + 64), 99, dtype=torch.int8, device=DEV)
    A2[:, :K] = L.dA
    res2 = torch.full((M, N + 32), 55, dtype=torch.int8, device=DEV)
    res2[:, :N] = dev(ref.res)
    bad = []
    for what, out, exp in (("plain", L.plain(L.lay_row, A=A2, lda=K + 64, ldo=N + 16), ref.k8),
                           ("residual", L.residual(L.lay_row, res2, ref.m1, ref.e1, A=A2, lda=K + 64, ldo=N + 16, ldr=N + 32), ref.resid_f32)):
        _collect(bad, what, first_bad_tile(out[:, :N].contiguous(), dev(exp), ref))
        assert bool((out[:, N:] == SENT).all()), (form, sid, what, "pad columns written")
    assert not bad, (form, sid, bad)
