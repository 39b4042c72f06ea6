"""Operands of more than 4 GiB: every strided entry once more with ONE operand as a tests/far.py buffer, whose rows start below 2^31,
between 2^31 and 2^32 and beyond 2^32 bytes; the other operands are the near `fenced` buffers of tests/test_gpu_strides.py, whose
problem builders (and shapes, and oracle expectations, bit for bit) these cases reuse.  A row offset that lost its upper bits on
the way to the load or the store shows as a wrong or never-stored value or as a damaged fill (far.py: never as a fault).
tests/test_far_coverage_cpu.py keeps the list complete; the launcher bounds themselves are in tests/test_gpu_far_bounds.py.

Which kernel each case reaches: the one of its near twin (the far leading dimension keeps the twin's granularity -- ld % 16, % 8,
% 4 or none, and the twin's base-pointer alignment), except where a launcher condition looks at rows * ld:
  int8 LayerNorm: ln_stream_takes wants rows * ldx and (rows + 15) * ldo below 2^31, so a far operand never streams, and lab form
    4 falls through to v2 (C = 768) / half a wave per row (C = 192).
  GEMM, M = 258: gemm_i8_kernel, which has no such condition.  M = 2125: the persistent kernel and the IVIT_W_FRAGS form, neither
    with a condition on M * ld; IVIT_W_FRAGS16 is bounded (test_gpu_far_bounds.py).  M = 8197: a far ldo leaves the skinny-K
    admission (M * ldo >= 2^32) for gemm_i8_kernel (N = 96 < 128); a far lda stays in it (no condition on M * lda: 64-bit A addressing)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as ISQ  # noqa: E402
from ivit_amd.prepare import LayerNormParams, markstein_division_ok, phi_tables  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import test_gpu_strides as S  # noqa: E402

DEV = S.DEV
f32 = np.float32
st, p, dev = S.st, S.p, S.dev


@pytest.fixture(autouse=True)
def _release():
    yield
    far.release()
    S._KEEP.clear()


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


def room(nbytes):
    """the only skip of these tests: less free device memory than the case needs"""
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < nbytes + (1 << 30):
        pytest.skip(f"{nbytes >> 20} MiB of device memory needed, {free >> 20} MiB free")


def far_in(a, multiple=1, lead=0, poison=None, **kw):
    a = np.ascontiguousarray(a)
    ld = far.ld_for(a.shape[0], a.itemsize, multiple, least=a.shape[1] + multiple)
    room(far.need_bytes(a.shape[0], ld, a.itemsize))
    return far.input(a, ld, fenced.POISON[a.dtype] if poison is None else poison, lead_bytes=lead, device=DEV, **kw)


def far_out(rows, width, dtype, expected, multiple=1, lead=0):
    item = np.dtype(dtype).itemsize
    ld = far.ld_for(rows, item, multiple, least=width + multiple)
    room(far.need_bytes(rows, ld, item))
    return far.output(rows, width, ld, dtype, expected=expected, lead_bytes=lead, device=DEV)


def done(o, expected):
    far.check(o, expected) if isinstance(o, far.Buffer) else fenced.check(o, expected)
    if isinstance(o, far.Buffer):
        far.free(o)


def same(x):
    far.check(x) if isinstance(x, far.Buffer) else fenced.check(x)


# =========================================================================================== int8 LayerNorm
LN_MULT = {"min": 4, "al16": 16}


@pytest.fixture(params=[0, 4], ids=["product", "lab_streaming"])
def ln_form(request):
    if request.param == 0:
        yield 0
        return
    with _lib.lab_session():
        _lib.call("ivit_debug_ln_wave_per_row", request.param)
        yield request.param


@pytest.mark.parametrize("operand", ["x", "out"])
@pytest.mark.parametrize("strides", list(S.LN_STRIDES))
@pytest.mark.parametrize("C", [192, 768])
def test_layernorm_i8_far_rows(C, strides, operand, ln_form):
    """ivit_layernorm_i8 / _ex, 37 rows (18 with a failing certificate: the literal tail addresses far rows too)"""
    dx, do, lead = S.LN_STRIDES[strides]
    k, gamma, beta, s_out, exp = S.ln8_case(C)
    rows = len(k)
    t = S.Tables(gamma, beta, s_out)
    orac = S.ln_oracle(gamma, beta, s_out)
    if operand == "x":
        x = far_in(k, LN_MULT[strides], lead, 127, oracle=orac, expected=exp)
    else:
        x = S.fin(k, C + dx, 127, lead_bytes=lead, oracle=orac, expected=exp)

    def out():
        return far_out(rows, C, np.int8, exp, LN_MULT[strides], lead) if operand == "out" else S.fout(rows, C, C + do, np.int8, exp, lead_bytes=lead)
    o = out()
    _lib.call("ivit_layernorm_i8", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, st())
    done(o, exp)
    o = out()
    _lib.call("ivit_layernorm_i8_ex", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, 0, st())
    done(o, exp)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
@pytest.mark.parametrize("strides", list(S.LN_STRIDES))
@pytest.mark.parametrize("C", [192, 768, 1096])
def test_layernorm_i8_compat_far_rows(C, strides, operand, ln_form):
    """ivit_layernorm_i8_compat: v2 up to C = 1024, a wave per row at 1096"""
    dx, do, lead = S.LN_STRIDES[strides]
    q, s, gamma, beta, s_out, exp, lay = S.ln8_compat_case(C)
    rows = len(q)
    t = S.Tables(gamma, beta, s_out)
    remap, phi = phi_tables(s)
    orac = S.ln_oracle(gamma, beta, s_out, lay)
    if operand == "x":
        x = far_in(q, LN_MULT[strides], lead, 127, oracle=orac, expected=exp)
        o = S.fout(rows, C, C + do, np.int8, exp, lead_bytes=lead)
    else:
        x = S.fin(q, C + dx, 127, lead_bytes=lead, oracle=orac, expected=exp)
        o = far_out(rows, C, np.int8, exp, LN_MULT[strides], lead)
    _lib.call("ivit_layernorm_i8_compat", x.ptr, x.ld, rows, C, *t.args, p(dev(remap)), p(dev(phi)), o.ptr, o.ld, 0, st())
    done(o, exp)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_layernorm_i32_f32_far_rows(operand):
    """the module-level form: C = 100, 4-byte elements, no alignment rule (odd leading dimensions, base + 4 bytes)"""
    C, rows = 100, 37
    rng = np.random.default_rng(C)
    k = rng.integers(-30000, 30001, size=(rows, C)).astype(np.int32)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    lp = LayerNormParams(gamma, beta, f32(0.03))

    def orac(x):
        y, s_ln, _ = orc.layernorm(x, S._wide(gamma, x.shape[1]), S._wide(beta, x.shape[1]))
        return (y * s_ln).astype(f32)
    exp = orac(k)
    if operand == "x":
        x = far_in(k, 1, 4, 2 ** 30, oracle=orac, expected=exp)
        o = S.fout(rows, C, C + 5, np.float32, exp, lead_bytes=4)
    else:
        x = S.fin(k, C + 3, 2 ** 30, lead_bytes=4, oracle=orac, expected=exp)
        o = far_out(rows, C, np.float32, exp, 1, 4)
    _lib.call("ivit_layernorm_i32_f32", x.ptr, x.ld, rows, C, p(dev(lp.bias_int)), p(dev(lp.s_ln)), o.ptr, o.ld, st())
    done(o, exp)
    same(x)


# =========================================================================================== Swin / 16-bit LayerNorm
@pytest.mark.parametrize("multiple", [1, 16], ids=["ldo_odd", "ldo_%16"])
@pytest.mark.parametrize("C", [96, 768])
def test_layernorm_i16_i8_far_output(C, multiple):
    """ivit_layernorm_i16_i8 and _compat (fast_division 0 / 1): ldo far, odd (the wave-per-row / literal kernels: ln16_tiling wants
    ldo % 8 == 0) or a multiple of 16 (the tiled kernels); 37 rows in row order and 64 rows through a window map (H = W = 8,
    ws = 4, shift = 2), where the permuted row index is what ldo multiplies"""
    s_in = f32(0.000913)
    assert markstein_division_ok(s_in, 16)
    rng = np.random.default_rng(C)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = (rng.standard_normal(C) * 0.1).astype(f32)
    s_out = f32(4.0 / 127.0)
    t = S.Tables(gamma, beta, s_out)
    for rows, geo in ((37, (0, 0, 0, 0)), (64, (8, 8, 4, 2))):
        xh = rng.integers(-20000, 20001, size=(rows, C)).astype(np.int16)
        xh[0] = 0
        x = S.fin(xh, C)
        for name, extra, lay in (("plain", (), orc.layernorm),
                                 ("compat", (float(s_in), 0), lambda q, g, b: orc.layernorm_scaled(q, s_in, g, b)),
                                 ("compat", (float(s_in), 1), lambda q, g, b: orc.layernorm_scaled(q, s_in, g, b))):
            exp = S.ln_oracle(gamma, beta, s_out, lay)(xh)
            if geo[2]:
                exp = S._win_order(exp, 1, geo[0], geo[2], geo[3])
            o = far_out(rows, C, np.int8, exp, multiple)
            assert multiple != 1 or o.ld % 8 != 0
            if name == "plain":
                _lib.call("ivit_layernorm_i16_i8", x.ptr, rows, C, *t.args, o.ptr, o.ld, *geo, st())
            else:
                _lib.call("ivit_layernorm_i16_i8_compat", x.ptr, rows, C, *extra, *t.args, o.ptr, o.ld, *geo, st())
            done(o, exp)
        fenced.check(x)


# =========================================================================================== I-BERT LayerNorm, engine forms
@pytest.mark.parametrize("operand", ["x", "out"])
@pytest.mark.parametrize("strides", ["min", "al16"])
@pytest.mark.parametrize("C", [96, 768])
@pytest.mark.parametrize("bits", [8, 16])
def test_ibert_layernorm_engine_forms_far_rows(bits, C, strides, operand):
    """ivit_ibert_layernorm_i8, ivit_ibert_layernorm_i16_i8 and _ex as in test_ibert_layernorm_engine_forms_strided_rows: an odd
    leading dimension from an element-aligned base (the literal kernel of the int8 entry) and a multiple of 16 (its fast kernel)"""
    dx, do = {"min": (3, 5), "al16": (16, 32)}[strides]
    mult = 1 if strides == "min" else 16
    rows = 37
    rng = np.random.default_rng(C + bits)
    s_in, sigma, dt = (f32(2.0 ** -4), 30.0, np.int8) if bits == 8 else (f32(2.0 ** -9), 80.0, np.int16)
    lim = 127 if bits == 8 else 32767
    q = np.clip(np.rint(rng.normal(rng.normal(0, 5, size=(rows, 1)), sigma, size=(rows, C))), -lim - 1, lim).astype(dt)
    q[1] = q[1, 0]
    q[1, 3] += 9
    assert (q.astype(np.int64) ** 2).sum(1).max() < 2 ** 24 and markstein_division_ok(s_in, 16)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    for isq in (False, True):
        lp, orac = S.ibert_ln_oracle(gamma, beta, s_in, 1.0, isq)
        exp = orac(q)
        lead = q.itemsize if strides == "min" else 0
        if operand == "x":
            x = far_in(q, mult, lead, oracle=orac, expected=exp)
        else:
            x = S.fin(q, C + dx, lead_bytes=lead, oracle=orac, expected=exp)

        def out(lead_o=0):
            return far_out(rows, C, np.int8, exp, mult, lead_o) if operand == "out" else S.fout(rows, C, C + do, np.int8, exp, lead_bytes=lead_o)
        tabs = (p(dev(lp.bias_int)), p(dev(lp.s_ln)), 1.0, p(dev(lp.m.view(np.int32))), p(dev(lp.e)))
        flag = ISQ if isq else 0
        if bits == 8:
            o = out(1 if strides == "min" else 0)
            _lib.call("ivit_ibert_layernorm_i8", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, flag, st())
            done(o, exp)
        else:
            if not isq:
                o = out()
                _lib.call("ivit_ibert_layernorm_i16_i8", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, st())
                done(o, exp)
            for fd in (0, 1):
                o = out()
                _lib.call("ivit_ibert_layernorm_i16_i8_ex", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, fd | flag, st())
                done(o, exp)
        same(x)
        if operand == "x":
            far.free(x)


# =========================================================================================== ShiftGELU
@pytest.mark.parametrize("operand", ["x", "out"])
@pytest.mark.parametrize("L", [50, 257])
def test_shiftgelu_direct_far_rows(L, operand):
    """ivit_shiftgelu_i8 and ivit_shiftgelu_i8_i32: 7 rows, no alignment rule (odd leading dimension, odd base address)"""
    rows = 7
    k, y, me, orac, exp = S.gelu_case(rows, L)
    fenced.poison_effective(k, 127, lambda a: orc.shiftgelu(a.astype(np.int32), S.GELU_S)[0], y)
    if operand == "x":
        x = far_in(k, 1, 1, 127, oracle=orac, expected=exp)
        o, o32 = S.fout(rows, L, L + 5, np.int8, exp, lead_bytes=1), S.fout(rows, L, L + 5, np.int32, y)
    else:
        x = S.fin(k, L + 3, 127, lead_bytes=1, oracle=orac, expected=exp)
        o = far_out(rows, L, np.int8, exp, 1, 1)
    _lib.call("ivit_shiftgelu_i8", x.ptr, x.ld, rows, L, float(S.GELU_S), me[0], me[1], o.ptr, o.ld, st())
    done(o, exp)
    if operand == "out":
        o32 = far_out(rows, L, np.int32, y, 1, 0)
    _lib.call("ivit_shiftgelu_i8_i32", x.ptr, x.ld, rows, L, float(S.GELU_S), o32.ptr, o32.ld, st())
    done(o32, y)
    same(x)


# in place runs on 16-byte-aligned strides only, as its near twin does
@pytest.mark.parametrize("strides,operand", [("min", "x"), ("min", "out"), ("al16", "x"), ("al16", "out"), ("al16", "in_place")])
@pytest.mark.parametrize("rows,L", [(7, 388), (7, 3100), (4099, 96), (4099, 380)])
def test_shiftgelu_lut_far_rows(rows, L, strides, operand):
    """ivit_shiftgelu_lut_i8 / _ex row-major: a wave per row (NJ = 3), the generic form, half a wave per row (NJ = 1, 3); in place
    (out == x, ldx == ldo) on a far buffer"""
    dx, do, lead = {"min": (4, 12, 4), "al16": (16, 32, 0)}[strides]
    mult = LN_MULT[strides]
    k, _, me, orac, exp = S.gelu_case(rows, L)
    lut = S.gelu_lut(me)
    if operand == "in_place":
        xi = far_in(k, 16, 0, 127, oracle=orac, expected=exp)
        _lib.call("ivit_shiftgelu_lut_i8_ex", xi.ptr, xi.ld, rows, L, p(lut), xi.ptr, xi.ld, 0, st())
        far.check(xi, exp)                                   # an input checked against values: the pads keep their poison
        return
    if operand == "x":
        x = far_in(k, mult, lead, 127, oracle=orac, expected=exp)
    else:
        x = S.fin(k, L + dx, 127, lead_bytes=lead, oracle=orac, expected=exp)

    def out():
        return far_out(rows, L, np.int8, exp, mult, lead) if operand == "out" else S.fout(rows, L, L + do, np.int8, exp, lead_bytes=lead)
    o = out()
    _lib.call("ivit_shiftgelu_lut_i8", x.ptr, x.ld, rows, L, p(lut), o.ptr, o.ld, st())
    done(o, exp)
    o = out()
    _lib.call("ivit_shiftgelu_lut_i8_ex", x.ptr, x.ld, rows, L, p(lut), o.ptr, o.ld, 0, st())
    done(o, exp)
    same(x)


# =========================================================================================== GEMM
def far_gemm(M, N, K, lda, ldw, seed, operand):
    """S.Gemm with A (operand 'a') or W ('w') replaced by a far buffer of the same values"""
    g = S.Gemm(M, N, K, lda, ldw, seed)
    if operand == "a":
        g.a = far_in(g.A, 16, 0, 127)
    if operand == "w":
        g.w = far_in(g.W, 16, 0, 127)
    return g


def _gemm_check_inputs(g):
    same(g.a)
    same(g.w)


@pytest.mark.parametrize("operand", ["a", "w", "out", "res"])
def test_gemm_small_kernel_int8_epilogues_far_rows(operand):
    """gemm_i8_kernel, M = 258, N = 208, K = 128: requant and residual entries with A, W, the output or the residual far; in place
    (out == res) on a far buffer"""
    M, N, K = 258, 208, 128
    g = far_gemm(M, N, K, K + 16, K + 32, 1, operand)

    def out(exp):
        return far_out(M, N, np.int8, exp, 16) if operand == "out" else S.fout(M, N, N + 16, np.int8, exp)
    if operand != "res":
        o = out(g.k8)
        _lib.call("ivit_gemm_i8_requant", *g.head, *g.me, o.ptr, o.ld, M, N, K, st())
        done(o, g.k8)
        o = out(g.k8)
        _lib.call("ivit_gemm_i8_requant_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, st())
        done(o, g.k8)
    res, sc, exp = g.residual(8)
    r = far_in(res, 16) if operand == "res" else S.fin(res, N + 32)
    o = out(exp)
    _lib.call("ivit_gemm_i8_requant_residual", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, st())
    done(o, exp)
    o = out(exp)
    _lib.call("ivit_gemm_i8_requant_residual_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    done(o, exp)
    # the width knobs: (8, 8) is the same kernel byte for byte, 4 bits clamps to [-8, 7]
    k4 = orc.requant(g.acc, g.m.astype(np.float64), g.e, 4)
    _, _, exp4 = g.residual(4, k=k4, res=res)
    assert np.abs(k4).max() <= 8 and np.abs(exp4).max() <= 8 and len(np.unique(exp4)) > 8
    if operand != "res":
        o = out(k4)
        _lib.call("ivit_gemm_i8_requant_bits_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, 4, st())
        done(o, k4)
    o = out(exp4)
    _lib.call("ivit_gemm_i8_requant_residual_bits_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, 4, 4, st())
    done(o, exp4)
    same(r)
    if operand == "res":
        _lib.call("ivit_gemm_i8_requant_residual", *g.head, *g.me, r.ptr, r.ld, *sc, r.ptr, r.ld, M, N, K, st())     # in place
        far.check(r, exp)
    _gemm_check_inputs(g)


@pytest.mark.parametrize("operand", ["a", "out", "res"])
def test_gemm_small_kernel_16_bit_epilogues_far_rows(operand):
    """residual_i16 (both entries) and i16_residual_i16 on gemm_i8_kernel: 16-bit residual / output rows, ld multiples of 8 elements"""
    M, N, K = 258, 208, 128
    g = far_gemm(M, N, K, K + 16, K + 32, 2, operand)
    res, sc, exp = g.residual(16)
    r = far_in(res, 8) if operand == "res" else S.fin(res, N + 8)

    def out(e):
        return far_out(M, N, np.int16, e, 8) if operand == "out" else S.fout(M, N, N + 24, np.int16, e)
    o = out(exp)
    _lib.call("ivit_gemm_i8_requant_residual_i16", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, st())
    done(o, exp)
    o = out(exp)
    _lib.call("ivit_gemm_i8_requant_residual_i16_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    done(o, exp)
    _, _, exp16 = g.residual(16, k=g.k16, res=res)
    o = out(exp16)
    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", *g.head, *g.me16, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    done(o, exp16)
    same(r)
    _gemm_check_inputs(g)


@pytest.mark.parametrize("operand", ["a", "out"])
def test_gemm_small_kernel_wide_outputs_far_rows(operand):
    """requant_i16 and the raw int32 accumulators: N = 204, ldo a multiple of 4 elements"""
    M, N, K = 258, 204, 128
    g = far_gemm(M, N, K, K + 16, K + 32, 3, operand)
    o = far_out(M, N, np.int16, g.k16, 4) if operand == "out" else S.fout(M, N, N + 4, np.int16, g.k16)
    _lib.call("ivit_gemm_i8_requant_i16", *g.head, *g.me16, o.ptr, o.ld, M, N, K, st())
    done(o, g.k16)
    o = far_out(M, N, np.int32, g.acc, 4) if operand == "out" else S.fout(M, N, N + 4, np.int32, g.acc)
    _lib.call("ivit_gemm_i8_i32", *g.head, o.ptr, o.ld, M, N, K, st())
    done(o, g.acc)
    _gemm_check_inputs(g)


@pytest.mark.parametrize("operand", ["a", "w"])
def test_gemm_small_kernel_head_major_outputs_far_operands(operand):
    """qkv, qkv_ex and qkv_planes_ex: the output is dense (bounded: test_gpu_far_bounds.py); A or W far"""
    import ctypes
    B, T, H, hd, K = 6, 43, 5, 16, 128
    M, N = B * T, 3 * H * hd
    g = far_gemm(M, N, K, K + 16, K + 32, 4, operand)
    exp = S.head_major(g.k8, B, T, H, hd).reshape(-1, hd)
    o = S.fout(len(exp), hd, hd, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_qkv", *g.head, *g.me, o.ptr, T, H, hd, M, N, K, st())
    fenced.check(o, exp)
    o = S.fout(len(exp), hd, hd, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_qkv_ex", *g.head, *g.me, o.ptr, T, H, hd, M, N, K, 0, st())
    fenced.check(o, exp)
    plane, Cn = M * H * hd, H * hd
    exp2 = exp[len(exp) // 3:]
    o = S.fout(len(exp2), hd, hd, np.int8, exp2, guard_bytes=plane)
    w1 = ctypes.c_void_p(g.w.ptr.value + Cn * g.w.ld)
    _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", g.a.ptr, g.a.ld, w1, g.w.ld, p(g.db[Cn:]), p(dev(g.m.view(np.int32)[Cn:])), p(dev(g.e[Cn:])),
              ctypes.c_void_p(o.ptr.value - plane), T, H, hd, 1, 2, M, 2 * Cn, K, 0, st())
    fenced.check(o, exp2)
    _gemm_check_inputs(g)


@pytest.mark.parametrize("operand", ["a", "w", "out", "res"])
def test_gemm_large_kernels_int8_far_rows(operand):
    """M = 2125, N = K = 192: the persistent kernel (row-major W, ldw far or K + 64) and gemm_i8_wreg_kernel with IVIT_W_FRAGS,
    whose launcher has no bound on M * ld: requant, residual and the output map"""
    M, N, K = 2125, 192, 192
    g = far_gemm(M, N, K, K + 16, K + 64, 21, operand)
    Wf = S._pack(g, 8)

    def out(e):
        return far_out(M, N, np.int8, e, 16) if operand == "out" else S.fout(M, N, N + 16, np.int8, e)
    res, sc, exp = g.residual(8)
    r = far_in(res, 16) if operand == "res" else S.fin(res, N + 32)
    for lay in (0, 8):
        w = (g.w.ptr, g.w.ld) if lay == 0 else (p(Wf), K)
        if operand != "res":
            o = out(g.k8)
            _lib.call("ivit_gemm_i8_requant_ex", g.a.ptr, g.a.ld, *w, p(g.db), *g.me, o.ptr, o.ld, M, N, K, lay, st())
            done(o, g.k8)
        o = out(exp)
        _lib.call("ivit_gemm_i8_requant_residual_ex", g.a.ptr, g.a.ld, *w, p(g.db), *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, lay, st())
        done(o, exp)
    if operand in ("a", "out"):
        lut = g.rng.integers(-128, 128, size=256).astype(np.int8)
        expl = lut[g.k8 + 128]
        o = out(expl)
        _lib.call("ivit_gemm_i8_requant_lut_ex", g.a.ptr, g.a.ld, p(Wf), K, p(g.db), *g.me, p(dev(lut)), o.ptr, o.ld, M, N, K, 8, st())
        done(o, expl)
    same(r)
    _gemm_check_inputs(g)


@pytest.mark.parametrize("operand", ["a", "out", "res"])
def test_gemm_large_kernels_16_bit_epilogues_far_rows(operand):
    """M = 2125: ivit_gemm_i8_requant_residual_i16_ex on the persistent kernel and IVIT_W_FRAGS, i16_residual_i16 with IVIT_W_FRAGS"""
    M, N, K = 2125, 192, 192
    g = far_gemm(M, N, K, K + 16, K + 64, 20, operand)
    res, sc, exp = g.residual(16)
    r = far_in(res, 8) if operand == "res" else S.fin(res, N + 8)
    Wf = S._pack(g, 8)

    def out(e):
        return far_out(M, N, np.int16, e, 8) if operand == "out" else S.fout(M, N, N + 24, np.int16, e)
    for lay in (0, 8):
        w = (g.w.ptr, g.w.ld) if lay == 0 else (p(Wf), K)
        o = out(exp)
        _lib.call("ivit_gemm_i8_requant_residual_i16_ex", g.a.ptr, g.a.ld, *w, p(g.db), *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, lay, st())
        done(o, exp)
    _, _, exp16 = g.residual(16, k=g.k16, res=res)
    o = out(exp16)
    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", g.a.ptr, g.a.ld, p(Wf), K, p(g.db), *g.me16, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 8, st())
    done(o, exp16)
    same(r)
    _gemm_check_inputs(g)


# =========================================================================================== layout passes
def test_pack_weight_frags_from_far_rows():
    """ivit_pack_weight_frags_i8 / _frags16_i8 from a far W (N = 200 rows)"""
    N, K = 200, 192
    W = np.random.default_rng(8).integers(-128, 127, size=(N, K)).astype(np.int8)
    w = far_in(W, 16, 0, 127)
    exp = S._frag_layout_host(W).reshape(256, K)
    o = S.fout(256, K, K, np.int8, exp)
    _lib.call("ivit_pack_weight_frags_i8", w.ptr, w.ld, N, K, o.ptr, st())
    fenced.check(o, exp)
    exp = S._frag16_layout_host(W).reshape(256, K)
    o = S.fout(256, K, K, np.int8, exp)
    _lib.call("ivit_pack_weight_frags16_i8", w.ptr, w.ld, N, K, o.ptr, st())
    fenced.check(o, exp)
    far.check(w)


def test_tile_and_untile_far_rows():
    """ivit_tile_operand_i8 from far rows and ivit_untile_operand_i8 into far rows (37 rows: the last block is partly padding)"""
    rows, K = 37, 192
    X = np.random.default_rng(9).integers(-128, 127, size=(rows, K)).astype(np.int8)
    x = far_in(X, 16, 0, 127)
    t = S.fout(rows, K, K, np.int8, X, blocks=True)
    _lib.call("ivit_tile_operand_i8", x.ptr, x.ld, rows, K, t.ptr, st())
    fenced.check(t, X)
    far.check(x)
    far.free(x)
    u = far_out(rows, K, np.int8, X, 16)
    _lib.call("ivit_untile_operand_i8", t.ptr, rows, K, u.ptr, u.ld, st())
    far.check(u, X)


# =========================================================================================== window attention (ldo over (window, token))
def test_window_attention_natural_scale_forms_far_output():
    """ivit_window_attention_i8_compat and _band at the smallest window (2 x 2 tokens, 1 head, 2 windows: 8 output rows), ldo far
    (a multiple of 8, as the entry wants); the problem of test_window_attention_natural_scale_forms_strided_output"""
    import test_gpu_swin as ts
    from ivit_amd.prepare import window_shiftexp_band
    B_, nW, nH, N, hd = 2, 1, 1, 4, 32
    rng = np.random.default_rng(44)
    qkv = rng.integers(-128, 128, size=(3, B_, nH, N, hd)).astype(np.int8)
    s_S, s_at = f32(2.0 ** -9 * 0.9), f32(0.1173)
    ms, omS = ts.sme(s_S, s_at), ts.ome(s_S, s_at)
    mb, omB = ts.sme(s_at * f32(0.75), s_at), ts.ome(s_at * f32(0.75), s_at)
    mo, omO = ts.sme(f32(2.0 ** -7 * 0.05), 0.043), ts.ome(f32(2.0 ** -7 * 0.05), 0.043)
    bias_add = rng.integers(-60, 61, size=(nH, N, N)).astype(np.int16)
    bias_pad = np.full((nH, N, 64), 99, np.int16)
    bias_pad[:, :, :N] = bias_add
    Sc = np.einsum("bhqd,bhkd->bhqk", qkv[0].astype(np.int64), qkv[1].astype(np.int64)).astype(np.int32)
    kS = orc.requant(Sc.reshape(-1, N), omS[0], omS[1], 8).reshape(B_, nH, N, N)
    lin = orc.requant(kS.reshape(-1, N), omB[0], omB[1], 32).reshape(B_, nH, N, N)
    kA = np.clip(lin + bias_add[None].astype(np.int32), -128, 127).astype(f32)
    Pm = orc.shiftmax_xint((((kA * s_at).astype(f32)) / s_at).astype(f32), s_at)
    O = np.einsum("bhqk,bhkd->bqhd", Pm.astype(np.int64), qkv[2].astype(np.int64)).astype(np.int32)
    exp = orc.requant(O.reshape(-1, hd), omO[0], omO[1], 8).reshape(B_ * N, nH * hd)
    assert Pm.max() > 0 and np.abs(exp).max() > 0
    qv = np.arange(-128, 128, dtype=f32)
    phi = ((qv * s_at).astype(f32) / s_at).astype(f32)
    phim = ((((qv * s_at).astype(f32) + f32(-100.0)).astype(f32)) / s_at).astype(f32)
    dq, db = dev(qkv), dev(bias_pad)
    o = far_out(B_ * N, nH * hd, np.int8, exp, 8)
    _lib.call("ivit_window_attention_i8_compat", p(dq), o.ptr, o.ld, p(db), None, -1, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1],
              float(s_at), mo[0], mo[1], p(dev(phi)), p(dev(phim)), st())
    done(o, exp)
    band, bw = window_shiftexp_band(s_at, False)
    assert band is not None
    o = far_out(B_ * N, nH * hd, np.int8, exp, 8)
    _lib.call("ivit_window_attention_i8_band", p(dq), o.ptr, o.ld, p(db), None, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1], float(s_at),
              mo[0], mo[1], p(dev(band)), bw, band.shape[0], 0, 0, 0, 0, st())
    done(o, exp)


def test_window_attention_long_far_output():
    """ivit_window_attention_i8_long at its smallest square window (9 x 9 tokens, 1 head, 1 window: 81 output rows)"""
    import test_gpu_swin_384 as w
    ws, B_, nW, nH = 9, 1, 1, 1
    qkv, s_at, me, bias_add, bias_pad, region = w._setup(ws, B_, nW, nH, 0.25, False, False, 9001)
    N, hd = ws * ws, 32
    exp = w._pv(qkv, orc.shiftmax(w._scores(qkv, me, bias_add), s_at), me).reshape(B_ * N, nH * hd)
    o = far_out(B_ * N, nH * hd, np.int8, exp, 8)
    _lib.call("ivit_window_attention_i8_long", p(dev(qkv)), o.ptr, o.ld, p(dev(bias_pad)), None, 0, B_, nW, nH, N, hd, me["ms"][0], me["ms"][1],
              me["mb"][0], me["mb"][1], float(s_at), me["mo"][0], me["mo"][1], None, None, None, 0, 0, ws, ws, ws, 0, 0, st())
    done(o, exp)


def test_window_attention_ibert_far_output():
    """ivit_window_attention_i8_ibert at 2 x 2 tokens, 1 head, 2 windows: 8 output rows"""
    import test_gpu_window_attention_ibert as wi
    from ivit_amd.swin_engine import HEAD_DIM, window_attention_ibert_spec
    N, nH, nwin, nW = 4, 1, 2, 1
    sc = wi.SCALES["natural"]
    s_S, s_at, s_A, s_tab, s_qkv, s_a3 = sc
    rng_act = wi.act_range(s_A, "natural")
    qkv, bias = wi.make_inputs(N, nH, nwin, 77)
    want, _ = wi.reference(qkv, bias, None, nW, sc, rng_act)
    exp = want.reshape(nwin * N, nH * HEAD_DIM)
    a = window_attention_ibert_spec(wi.upload, DEV, st(), bias, f32(s_tab), f32(s_S), f32(s_at), f32(s_A), f32(f32(2.0 ** -7) * f32(s_qkv)),
                                    f32(s_a3), None, N, rng_act, form="table")
    o = far_out(nwin * N, nH * HEAD_DIM, np.int8, exp, 8)
    _lib.call("ivit_window_attention_i8_ibert", p(dev(qkv)), o.ptr, o.ld, p(a["bias"]), p(a["region"]), a["masked_exp"], nwin, nW, nH, N,
              HEAD_DIM, *a["ms"], *a["mb"], *a["mo"], p(a["table"]), a["band_w"], 2, 2, 2, 0, 0, st())
    done(o, exp)


# =========================================================================================== attention maps and the class-token row
@pytest.mark.parametrize("T,full", [(197, False), (197, True), (199, True), (1025, True)], ids=["197-cls", "197-all", "199-all", "1025-all"])
def test_attention_probabilities_into_far_rows(T, full):
    """ivit_attention_probs_u8 and ivit_attention_probs_u8_ibert: ldp such that (bh * q_rows + row) * ldp passes 2^31 and 2^32 --
    between the four (image, head) pairs of the class rows, and inside a pair's map for q_rows = tokens; 197 tokens from an odd
    address (byte stores), 199 and 1025 (attention_maps(x, rows="all") at 1025 tokens: the long form) with ldp % 4 == 0 (packed
    dwords).  The problems and oracle maps of tests/test_gpu_attention_probs.py"""
    import test_gpu_attention_probs as tp
    B, H = tp._bh(T) if T <= 209 else (2, 2)
    q_rows = T if full else 1
    lead, mult = (3, 1) if T == 197 else (0, 4)
    s_at, ms, es, _, _ = tp._shiftmax_scales("pow2")
    if T <= 209:
        qkv, P = tp._shiftmax_case(T, "pow2")
    else:          # two images (four rows of pairs): the module's case has one
        qkv1, P1 = tp._shiftmax_case(T, "pow2")
        qkv, P = np.concatenate([qkv1, qkv1[:, :, ::-1]], axis=1), np.concatenate([P1, P1[:, ::-1]], axis=0)
    exp = P[:, :, :q_rows].reshape(B * H * q_rows, T)
    o = far_out(B * H * q_rows, T, np.uint8, exp, mult, lead)
    assert (o.ld % 4 == 0 and lead == 0) == (T != 197)
    _lib.call("ivit_attention_probs_u8", p(dev(qkv)), o.ptr, o.ld, B, H, T, 64, q_rows, int(ms[0]), int(es[0]), float(s_at), None, None, 0, st())
    done(o, exp)
    qkv, tab, P, _ = tp._ibert_case(T, False)
    Bi, Hi = tp._bh(T)
    if Bi * Hi * q_rows < 4:
        qkv, P = np.concatenate([qkv, qkv[:, :, ::-1]], axis=1), np.concatenate([P, P[:, ::-1]], axis=0)
        Bi *= 2
    exp = P[:, :, :q_rows].reshape(Bi * Hi * q_rows, T)
    o = far_out(Bi * Hi * q_rows, T, np.uint8, exp, mult, lead)
    ms, es = tp.IBERT_MS
    _lib.call("ivit_attention_probs_u8_ibert", p(dev(qkv)), o.ptr, o.ld, Bi, Hi, T, 64, q_rows, int(ms[0]), int(es[0]),
              p(dev(tab.reshape(-1))), None, 0, st())
    done(o, exp)


@pytest.mark.parametrize("N,mult", [(49, 1), (49, 4), (64, 1)], ids=["bytes", "dwords", "odd_ld"])
def test_window_probabilities_into_far_rows(N, mult):
    """ivit_window_attention_probs_u8 and _ibert (8 windows x 3 heads x N rows): the problem of
    test_gpu_window_probs.py::test_fenced_outputs_of_both_entries with ldp far"""
    import test_gpu_window_probs as tw
    nH, nW, imgs = 3, 4, 2
    nwin = nW * imgs
    qkv, bias = tw.wp.problem(N, nH, nwin, 3 * N + mult)
    ws = int(round(N ** 0.5))
    region = tw.shift_mask_regions(2 * ws, 2 * ws, ws, ws // 2).astype(np.uint8)
    up = dev
    s_S, s_at, s_A, s_tab = (f32(v) for v in tw.SHIFTMAX_SCALES["pow2"][0])
    a, form = tw.window_attention_spec(up, bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N)
    assert form is None
    exp = tw.wp.probs("ivit", qkv, bias, region, nW, s_S, s_at, s_A, s_tab).reshape(nwin * nH * N, N)
    o = far_out(nwin * nH * N, N, np.uint8, exp, mult)
    assert (o.ld % 4 == 0) == (mult == 4)
    _lib.call("ivit_window_attention_probs_u8", p(up(qkv)), o.ptr, o.ld, p(a["bias"]), p(a["region"]), a["mask_value"], nwin, nW, nH,
              N, tw.HD, *a["ms"], *a["mb"], a["s_attn"], None, None, None, 0, 0, st())
    done(o, exp)
    s_S, s_at, s_A, s_tab, _, _ = (f32(v) for v in tw.IBERT_SCALES["natural"])
    rng_act = tw.act_range(s_A, "natural")
    b = tw.window_attention_ibert_spec(up, DEV, st(), bias, s_tab, s_S, s_at, s_A, f32(2.0 ** -11), f32(2.0 ** -5), region, N, rng_act,
                                       form="band")
    exp = tw.wp.probs("ibert", qkv, bias, region, nW, s_S, s_at, s_A, s_tab, rng_act).reshape(nwin * nH * N, N)
    o = far_out(nwin * nH * N, N, np.uint8, exp, mult)
    _lib.call("ivit_window_attention_probs_u8_ibert", p(up(qkv)), o.ptr, o.ld, p(b["bias"]), p(b["region"]), b["masked_exp"], nwin,
              nW, nH, N, tw.HD, *b["ms"], *b["mb"], p(b["table"]), b["band_w"], st())
    done(o, exp)


def test_attention_cls_far_rows():
    """ivit_attention_cls_i8: one output row per image, ldo (a multiple of 16) far: 4 images x 3 heads, 50 tokens"""
    import test_gpu_cls_tail as tc
    T, H, B = 50, 3, 4
    qkv = tc._crafted("random", np.random.default_rng(300 + T + H), B, H, T)
    exp, _ = tc._expected_row0(qkv, "pow2")
    assert np.abs(exp).max() > 5
    s_at, (ms, es), (mo, eo) = tc._scales("pow2")
    d = dev(qkv)
    q_cls = dev(np.ascontiguousarray(qkv[0, :, :, 0, :]).reshape(B, H * tc.HD))
    o = far_out(B, H * tc.HD, np.int8, exp, 16)
    _lib.call("ivit_attention_cls_i8", p(d[1]), p(d[2]), p(q_cls), o.ptr, o.ld, B, H, T, tc.HD, int(ms[0]), int(es[0]), float(s_at),
              int(mo[0]), int(eo[0]), None, None, 0, st())
    done(o, exp)


# =========================================================================================== feature maps
@pytest.mark.parametrize("aligned", [False, True], ids=["element_loads", "vector_loads"])
@pytest.mark.parametrize("bits", [8, 16])
def test_tokens_to_nchw_from_far_rows(bits, aligned):
    """the four ivit_tokens_to_nchw entries from token rows with ldx far: 2 x 130 rows of 200 channels, tokens 2 .. 128 selected;
    an odd ldx from an element-aligned base (element loads) and rows of a multiple of 16 bytes (vector loads); the dense
    channel-major output is a near fenced buffer"""
    import test_gpu_feature_maps as tf
    shape = B, T_all, t0, T, C = (2, 130, 2, 127, 200)
    di = np.int8 if bits == 8 else np.int16
    item = np.dtype(di).itemsize
    q = tf._source(shape, di, seed=sum(shape) + item)
    x = far_in(q.reshape(B * T_all, C), 16 // item if aligned else 1, 0 if aligned else item)
    assert aligned or (x.ld * item) % 4 != 0 or x.lead_bytes % 4 != 0
    s = tf.SCALES[1]
    exp = tf._expected(q, shape, np.float32, s).reshape(B * C, T)
    o = S.fout(B * C, T, T, np.float32, exp)
    if bits == 8:
        _lib.call("ivit_tokens_to_nchw_i8_f32", x.ptr, x.ld, B, T_all, t0, T, C, float(s), o.ptr, st())
    else:
        _lib.call("ivit_tokens_to_nchw_i16_f32", x.ptr, x.ld, B, T_all, t0, T, C, float(s), o.ptr, st())
    fenced.check(o, exp)
    exp = tf._expected(q, shape, di, None).reshape(B * C, T)
    o = S.fout(B * C, T, T, di, exp)
    if bits == 8:
        _lib.call("ivit_tokens_to_nchw_i8", x.ptr, x.ld, B, T_all, t0, T, C, o.ptr, st())
    else:
        _lib.call("ivit_tokens_to_nchw_i16", x.ptr, x.ld, B, T_all, t0, T, C, o.ptr, st())
    fenced.check(o, exp)
    far.check(x)


@pytest.mark.parametrize("B_,nW,nH,N,s_attn,masked", [(8, 4, 3, 49, 0.25, True), (2, 2, 2, 9, 0.0625, True)])
def test_window_attention_far_output(B_, nW, nH, N, s_attn, masked):
    """ivit_window_attention_i8 (rows in window order) and ivit_window_attention_i8_unwindow (the same rows at their image
    positions, shift 0 and ws / 2: the permuted row index is what ldo multiplies), ldo far; the problem and oracle of
    test_gpu_swin.py::test_window_attention"""
    import test_gpu_swin as ts
    from ivit_amd.swin_engine import window_row_map
    rng = np.random.default_rng(B_ * 1000 + N)
    hd = 32
    qkv = rng.integers(-128, 128, size=(3, B_, nH, N, hd)).astype(np.int8)
    qkv[0, 0, 0, 0] = 127
    qkv[1, 0, 0] = 127
    s_S, s_at = f32(2.0 ** -9 * 0.9), f32(s_attn)
    ms, omS = ts.sme(s_S, s_at), ts.ome(s_S, s_at)
    ratio = f32(0.75 if N == 49 else 1.0)
    mb, omB = ts.sme(s_at * ratio, s_at), ts.ome(s_at * ratio, s_at)
    mo, omO = ts.sme(f32(2.0 ** -7 * 0.05), 0.043), ts.ome(f32(2.0 ** -7 * 0.05), 0.043)
    bias_add = rng.integers(-60, 61, size=(nH, N, N)).astype(np.int16)
    bias_pad = np.full((nH, N, 64), 99, np.int16)
    bias_pad[:, :, :N] = bias_add
    mval = int(f32(-100.0) / s_at)
    region = np.full((nW, 64), 200, np.uint8)
    region[:, :N] = rng.integers(0, 4, size=(nW, N))
    mask_add = np.where(region[:, :N, None] != region[:, None, :N], mval, 0).astype(np.int16)
    ref, kA, Pm = ts.window_attention_ref(qkv[0], qkv[1], qkv[2], bias_add, mask_add, nW, omS, omB, s_at, omO)
    exp = np.asarray(ref).reshape(B_ * N, nH * hd)
    assert Pm.max() > 0
    dq, db, dr = dev(qkv), dev(bias_pad), dev(region)
    o = far_out(B_ * N, nH * hd, np.int8, exp, 8)
    _lib.call("ivit_window_attention_i8", p(dq), o.ptr, o.ld, p(db), p(dr), mval, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1],
              float(s_at), mo[0], mo[1], st())
    done(o, exp)
    ws_ = int(round(np.sqrt(N)))
    gh, gw = {2: (1, 2), 4: (2, 2)}[nW]
    H, W = gh * ws_, gw * ws_
    for shift in sorted({0, ws_ // 2}):
        dst = window_row_map(B_ // nW, H, W, ws_, shift)        # image row r -> its row in window order
        o = far_out(B_ * N, nH * hd, np.int8, exp[dst], 8)
        _lib.call("ivit_window_attention_i8_unwindow", p(dq), o.ptr, o.ld, p(db), p(dr), mval, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1],
                  float(s_at), mo[0], mo[1], None, None, H, W, ws_, shift, st())
        done(o, exp[dst])


# =========================================================================================== I-BERT LayerNorm, module forms
@pytest.mark.parametrize("operand", ["x", "out"])
@pytest.mark.parametrize("isq", [False, True], ids=["float_sqrt", "int_sqrt"])
def test_ibert_layernorm_module_forms_ex_far_rows(isq, operand):
    """ivit_ibert_layernorm_i32_f32_ex and ivit_ibert_layernorm_f32_f32_ex: C = 100, 37 rows of 4-byte elements, the input or the
    output far; the problem of test_ibert_layernorm_module_forms_ex_strided_rows"""
    import ibert_intsqrt_ref as R
    C, rows = 100, 37
    rng = np.random.default_rng(C + isq)
    s_in = f32(2.0 ** -6)
    k = np.clip(np.rint(rng.normal(rng.normal(0, 20, size=(rows, 1)), 300.0, size=(rows, C))), -32768, 32767).astype(np.int32)
    assert (k.astype(np.int64) ** 2).sum(1).max() < 2 ** 24
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    bias_int, s_out = R.layernorm_constants(gamma, beta)

    def lay(x_int):
        n = x_int.shape[1]
        b, so = R.layernorm_constants(S._wide(gamma, n), S._wide(beta, n))
        with np.errstate(over="ignore", invalid="ignore"):
            return R.layernorm(x_int, b, so, 1.0, int_sqrt=isq)

    def orac(q):
        return lay(R.x_int_of(q, s_in))
    exp = orac(k)
    assert np.isfinite(exp).all()
    flag = ISQ if isq else 0
    tabs = (p(dev(bias_int)), p(dev(s_out)), 1.0)
    xfh = (k.astype(f32) * s_in).astype(f32)
    oracf = lambda v: lay((v / s_in).astype(f32))      # noqa: E731
    if operand == "x":
        x = far_in(k, 1, 0, oracle=orac, expected=exp)
        o = S.fout(rows, C, C + 5, np.float32, exp)
    else:
        x = S.fin(k, C + 3, oracle=orac, expected=exp)
        o = far_out(rows, C, np.float32, exp, 1)
    _lib.call("ivit_ibert_layernorm_i32_f32_ex", x.ptr, x.ld, rows, C, *tabs, o.ptr, o.ld, flag, st())
    done(o, exp)
    same(x)
    if operand == "x":
        far.free(x)
        xf = far_in(xfh, 1, 0, oracle=oracf, expected=exp)
        o = S.fout(rows, C, C + 5, np.float32, exp)
    else:
        xf = S.fin(xfh, C + 3, oracle=oracf, expected=exp)
        o = far_out(rows, C, np.float32, exp, 1)
    _lib.call("ivit_ibert_layernorm_f32_f32_ex", xf.ptr, xf.ld, rows, C, p(dev(np.array([s_in], f32))), 1, *tabs, o.ptr, o.ld, flag, st())
    done(o, exp)
    same(xf)


# =========================================================================================== patchify: lda of the patch matrix
def test_patchify_into_far_rows():
    """the four patchify entries (square and h x w, float and uint8 pixels) into a patch matrix whose lda is far: 2 images of
    3 x 16 x 16, patch 4 -> 32 rows of 48 bytes.  Expected: q = clamp(round(inv_scale * x)) resp. lut[c][v], in im2col order"""
    B, C, hw, patch = 2, 3, 16, 4
    g = hw // patch
    rows, K = B * g * g, C * patch * patch
    rng = np.random.default_rng(hw + patch)
    inv = f32(1.0 / 0.0317)
    imgf = (rng.standard_normal((B, C, hw, hw)) * 40.0 / float(inv)).astype(f32)
    imgu = rng.integers(0, 256, size=(B, C, hw, hw), dtype=np.uint8)
    lut = rng.integers(-128, 128, size=(C, 256)).astype(np.int8)
    im2col = lambda q: np.ascontiguousarray(q.reshape(B, C, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5)).reshape(rows, K)      # noqa: E731
    expf = im2col(np.clip(np.rint((inv * imgf).astype(f32)), -128, 127).astype(np.int8))
    expu = im2col(lut[np.arange(C)[None, :, None, None], imgu])
    assert len(np.unique(expf)) > 50 and len(np.unique(expu)) > 50
    df, du, dl = dev(imgf), dev(imgu), dev(lut)
    o = far_out(rows, K, np.int8, expf, 16)
    _lib.call("ivit_quantize_patchify_ld_f32_i8", p(df), o.ptr, o.ld, B, C, hw, patch, float(inv), st())
    done(o, expf)
    o = far_out(rows, K, np.int8, expf, 16)
    _lib.call("ivit_quantize_patchify_hw_f32_i8", p(df), o.ptr, o.ld, B, C, hw, hw, patch, float(inv), st())
    done(o, expf)
    o = far_out(rows, K, np.int8, expu, 16)
    _lib.call("ivit_quantize_patchify_u8_i8", p(du), o.ptr, o.ld, B, C, hw, patch, p(dl), st())
    done(o, expu)
    o = far_out(rows, K, np.int8, expu, 16)
    _lib.call("ivit_quantize_patchify_hw_u8_i8", p(du), o.ptr, o.ld, B, C, hw, hw, patch, p(dl), st())
    done(o, expu)


# =========================================================================================== module-level forms
def far_pair(operand, xdata, ldx_near, rows, width, out_dtype, exp, ldo_near):
    """(x, out): the input far and the output near (operand 'x'), or the other way round ('out'); no alignment rule: odd strides"""
    if operand == "x":
        return far_in(xdata, 1, 0), S.fout(rows, width, ldo_near, out_dtype, exp)
    return S.fin(xdata, ldx_near), far_out(rows, width, out_dtype, exp, 1)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_shiftmax_module_forms_far_rows(operand):
    """ivit_shiftmax_i8, _i32_i8, _f32_i8 and _f32_i16 (16 bits): 37 rows of 50 scores (flat, one-hot, repeated-maximum rows among
    them: test_gpu_module_kernels.sm_rows), the input or the output far"""
    import test_gpu_module_kernels as mk
    L, rows, s = 50, 37, f32(2.0 ** -3)
    k = mk.sm_rows(L, rows, 9)
    want = orc.shiftmax(k, s)
    assert want.max() > 0
    x, o = far_pair(operand, k.astype(np.int8), L + 3, rows, L, np.int8, want, L + 5)
    _lib.call("ivit_shiftmax_i8", x.ptr, x.ld, rows, L, float(s), o.ptr, o.ld, st())
    done(o, want)
    same(x)
    far.free(x) if operand == "x" else None
    x, o = far_pair(operand, k.astype(np.int32), L + 3, rows, L, np.int8, want, L + 5)
    _lib.call("ivit_shiftmax_i32_i8", x.ptr, x.ld, rows, L, float(s), o.ptr, o.ld, st())
    done(o, want)
    same(x)
    far.free(x) if operand == "x" else None
    xf = (k.astype(f32) * s).astype(f32)
    want8, want16 = orc.shiftmax_compat(k, s, output_bit=8), orc.shiftmax_compat(k, s, output_bit=16)
    x, o = far_pair(operand, xf, L + 3, rows, L, np.int8, want8, L + 5)
    _lib.call("ivit_shiftmax_f32_i8", x.ptr, x.ld, rows, L, float(s), o.ptr, o.ld, st())
    done(o, want8)
    if operand == "out":
        o = far_out(rows, L, np.int16, want16, 1)
    else:
        o = S.fout(rows, L, L + 5, np.int16, want16)
    _lib.call("ivit_shiftmax_f32_i16", x.ptr, x.ld, rows, L, float(s), 16, o.ptr, o.ld, st())
    done(o, want16)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_layernorm_literal_forms_far_rows(operand):
    """ivit_layernorm_f32_f32 and _ex (outer_mean 0): C = 100, 61 rows at a natural 8-bit scale, every third an exact tie of the mean"""
    import test_gpu_module_kernels as mk
    C, rows, s = 100, 61, 0.0371
    gamma, beta = mk._affine(C, C)
    q = mk.ln_rows(rows, C, C + 8, 8)
    y, s_ln, bias_int, _ = orc.layernorm_compat(q, s, gamma, beta)
    want = (y * s_ln).astype(f32)
    xf = (q.astype(f32) * f32(s)).astype(f32)
    tabs = (p(dev(np.array([s], f32))), 1, p(dev(bias_int)), p(dev(s_ln)))
    x, o = far_pair(operand, xf, C + 3, rows, C, np.float32, want, C + 5)
    _lib.call("ivit_layernorm_f32_f32", x.ptr, x.ld, rows, C, *tabs, o.ptr, o.ld, st())
    done(o, want)
    o = far_out(rows, C, np.float32, want, 1) if operand == "out" else S.fout(rows, C, C + 5, np.float32, want)
    _lib.call("ivit_layernorm_f32_f32_ex", x.ptr, x.ld, rows, C, *tabs, o.ptr, o.ld, 0, st())
    done(o, want)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_ibert_softmax_module_forms_far_rows(operand):
    """ivit_ibert_softmax_i32 and ivit_ibert_softmax_f32_f32: 37 rows of 49 scores at s = 2^-4 (x / s is the integer), 8 bits"""
    import test_gpu_ibert_ops as io
    from oracle import ibert as ib
    L, rows, s, bit = 49, 37, f32(2.0 ** -4), 8
    k = io.sm_set_a(L, s, 127)
    act = io.sm_act(s, "pow2")
    want, _, ninx = ib.softmax(k, s, *act, output_bit=bit)
    assert ninx == 0 and io._roundtrip_is_identity(k, s)
    want_f = (want.astype(f32) * f32(2 / 2 ** bit)).astype(f32)
    x0_int, b_int, c_int, exp_sf, act_sf, m, e = ib.softmax_constants(s, *act)
    consts = (float(x0_int), float(b_int), float(c_int), float(exp_sf), float(act_sf), int(m), int(e), bit)
    x, o = far_pair(operand, k.astype(np.int32), L + 3, rows, L, np.int32, want.astype(np.int32), L + 5)
    _lib.call("ivit_ibert_softmax_i32", x.ptr, x.ld, rows, L, *consts, o.ptr, o.ld, None, st())
    done(o, want.astype(np.int32))
    same(x)
    far.free(x) if operand == "x" else None
    x, o = far_pair(operand, (k.astype(f32) * s).astype(f32), L + 3, rows, L, np.float32, want_f, L + 5)
    _lib.call("ivit_ibert_softmax_f32_f32", x.ptr, x.ld, rows, L, float(s), *consts, o.ptr, o.ld, None, st())
    done(o, want_f)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_ibert_layernorm_module_forms_far_rows(operand):
    """ivit_ibert_layernorm_i32_f32 and ivit_ibert_layernorm_f32_f32: C = 100, 50 rows, per-channel power-of-two input scales"""
    import test_gpu_ibert_ops as io
    from oracle import ibert as ib
    C, rows = 100, 50
    gamma, beta = io._affine(C, C)
    s_vec = (2.0 ** -np.random.default_rng(C).integers(3, 7, size=C)).astype(f32)
    k = np.rint(np.random.default_rng(C).normal(0, 40, size=(rows, C))).astype(np.int32)
    y, s_out, ninx = ib.layernorm(k, s_vec, gamma, beta)
    want = (y * s_out).astype(f32)
    assert ninx == 0 and np.isfinite(want).all() and io._roundtrip_is_identity(k, s_vec)
    bias_int, s_o = ib.layernorm_constants(gamma, beta)
    x, o = far_pair(operand, k, C + 3, rows, C, np.float32, want, C + 5)
    _lib.call("ivit_ibert_layernorm_i32_f32", x.ptr, x.ld, rows, C, p(dev(bias_int)), p(dev(s_o)), 1.0, o.ptr, o.ld, st())
    done(o, want)
    same(x)
    far.free(x) if operand == "x" else None
    x, o = far_pair(operand, (k.astype(f32) * s_vec).astype(f32), C + 3, rows, C, np.float32, want, C + 5)
    _lib.call("ivit_ibert_layernorm_f32_f32", x.ptr, x.ld, rows, C, p(dev(s_vec)), s_vec.size, p(dev(bias_int)), p(dev(s_o)), 1.0, o.ptr, o.ld, st())
    done(o, want)
    same(x)


@pytest.mark.parametrize("operand", ["x", "out"])
def test_ibert_layernorm_window_order_far_rows(operand):
    """ivit_ibert_layernorm_i16_i8_win: 14 x 14 tokens, 7 x 7 windows, shift 3, C = 96: the window-order row index is what ldo
    multiplies, the image-order one what ldx multiplies; fast_division 0 / 1, with and without the integer square root"""
    from ivit_amd.swin_engine import window_row_map
    C, B, H, W, ws, shift = 96, 1, 14, 14, 7, 3
    rows = B * H * W
    rng = np.random.default_rng(C + 16)
    s_in = f32(2.0 ** -9)
    q = np.clip(np.rint(rng.normal(rng.normal(0, 5, size=(rows, 1)), 80.0, size=(rows, C))), -32768, 32767).astype(np.int16)
    q[1] = q[1, 0]
    q[1, 3] += 9
    assert (q.astype(np.int64) ** 2).sum(1).max() < 2 ** 24 and markstein_division_ok(s_in, 16)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    perm = window_row_map(B, H, W, ws, shift)
    x = None
    for isq in (False, True):
        lp, orac = S.ibert_ln_oracle(gamma, beta, s_in, 1.0, isq)
        exp = orac(q)
        want = np.empty_like(exp)
        want[perm] = exp
        if x is None:
            x = far_in(q, 8, 0, oracle=orac, expected=exp) if operand == "x" else S.fin(q, C + 8, oracle=orac, expected=exp)
        tabs = (p(dev(lp.bias_int)), p(dev(lp.s_ln)), 1.0, p(dev(lp.m.view(np.int32))), p(dev(lp.e)))
        for fd in (0, 1):
            o = far_out(rows, C, np.int8, want, 64) if operand == "out" else S.fout(rows, C, 128, np.int8, want)
            _lib.call("ivit_ibert_layernorm_i16_i8_win", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, fd | (ISQ if isq else 0),
                      H, W, ws, shift, st())
            done(o, want)
    same(x)


@pytest.mark.parametrize("operand", ["w", "w8"])
def test_weight_quant_rows_far_rows(operand):
    """ivit_weight_quant_rows_f32_i8: the float weight rows (ldw) or the int8 rows (ldo) far; 37 rows of 200 columns, scale and
    w_int dense"""
    from ivit_amd.prepare import LinearParams
    rows, cols = 37, 200
    rng = np.random.default_rng(rows + cols)
    Wt = (rng.standard_normal((rows, cols)) * rng.uniform(0.01, 2.0, size=(rows, 1))).astype(f32)
    lp = LinearParams(Wt, None, f32(0.03))
    w = far_in(Wt, 1, 0) if operand == "w" else S.fin(Wt, cols + 1)
    w8 = far_out(rows, cols, np.int8, lp.W8, 1) if operand == "w8" else S.fout(rows, cols, cols + 1, np.int8, lp.W8)
    scale = S.fout(1, rows, rows, np.float32, lp.sw[None])
    w_int = S.fout(rows, cols, cols, np.float32, lp.W8.astype(f32))
    _lib.call("ivit_weight_quant_rows_f32_i8", w.ptr, w.ld, rows, cols, scale.ptr, w8.ptr, w8.ld, w_int.ptr, st())
    done(w8, lp.W8)
    fenced.check(scale, lp.sw[None])
    fenced.check(w_int, lp.W8.astype(f32))
    same(w)


def test_logits_topk_far_rows():
    """ivit_logits_topk_f32: 7 rows of 10 classes (ties included), ld far: batch * ld passes 2^31 elements"""
    import test_gpu_topk as tt
    B, N, k = 7, 10, 5
    rng = np.random.default_rng(B * 7 + N + k)
    lf = rng.integers(-5, 6, size=(B, N)).astype(f32)          # few distinct values: ties across rank k
    ld = 2 * far.ld_for(B, 4, 1)          # twice the byte spread: the ELEMENT offset of the last rows passes 2^31 as well
    assert (B - 2) * ld >= 2 ** 31 > ld
    room(far.need_bytes(B, ld, 4))
    x = far.input(lf, ld, 1e30, device=DEV)
    tk = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    _lib.call("ivit_logits_topk_f32", x.ptr, B, x.ld, N, k, p(tk), None, None, st())
    torch.cuda.synchronize()
    assert np.array_equal(tk.cpu().numpy(), tt.stable_topk(lf, N, k))
    far.check(x)


def test_head_topk_far_rows():
    """ivit_head_topk: `ld` (an int) is the stride of the accumulators AND of the float logits it writes for every column up to
    ld, so both are far and dense here: 7 rows of ld = 438 M elements (batch * ld passes 2^31 elements, the byte offsets 2^32),
    periodic accumulators and scales; logits compared on the device row by row, the selection over the first 1000 columns by the
    stable sort of tests/test_gpu_topk.py (columns beyond N hold larger logits that must not be selected)"""
    import test_gpu_topk as tt
    from test_gpu_far_flat import Flat, P
    B, N, k = 7, 1000, 5
    ld = 2 * far.ld_for(B, 4, 1)
    assert (B - 2) * ld >= 2 ** 31 > ld
    rng = np.random.default_rng(B * 7 + N + k)
    accb = rng.integers(-300000, 300000, size=P).astype(np.int32)
    sb = rng.uniform(1e-6, 2e-6, size=P).astype(f32)
    acc = Flat(B * ld, np.int32, 2 ** 30).tile(accb)
    acc.body.view(B, ld)[:, N:N + 64] = 2 ** 30          # padded classes that would win if the selection read them
    sd = Flat(ld, np.float32, 1e30).tile(sb)
    sd.body[N:N + 64] = 1.0
    lf = Flat(B * ld, np.float32, 1e30)
    tk = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    _lib.call("ivit_head_topk", acc.ptr, sd.ptr, B, ld, N, k, lf.ptr, p(tk), None, None, st())
    torch.cuda.synchronize()
    step = 2 ** 26
    bad = 0
    for r in range(B):
        for c in range(0, ld, step):
            want = acc.body[r * ld + c:r * ld + min(ld, c + step)].float() * sd.body[c:min(ld, c + step)]
            bad += int((lf.body[r * ld + c:r * ld + min(ld, c + step)].view(torch.int32) != want.view(torch.int32)).sum())
    assert bad == 0, f"{bad} logits differ from float(acc) * s"
    assert lf.guards_hold() and acc.guards_hold()
    exp = lf.body.view(B, ld)[:, :N].cpu().numpy()
    got = tk.cpu().numpy()
    assert np.array_equal(got, tt.stable_topk(exp, N, k)) and got.max() < N
