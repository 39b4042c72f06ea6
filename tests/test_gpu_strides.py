"""Leading dimensions of the C ABI on the fused engines' path: every operator with strided rows (ld > width) between poisoned pads
and guard rows, every output into a sentinel-filled strided buffer (tests/fenced.py).  Each operator runs with the smallest strides
its own argument check admits and with 16-byte-aligned ones -- the two sides of the launchers' alignment branches -- and, where the
entry admits a base pointer aligned to less than 16 bytes, from such a pointer.  Expectations are the oracle's (oracle/oracle.py,
oracle/ibert.py, tests/*_ref.py), bit for bit; nothing here has a tolerance.  tests/test_strides_coverage_cpu.py keeps the list of
entries complete.

Which kernel each case reaches, from the launchers' own conditions:
  int8 LayerNorm (csrc/rowops.hip ivit_layernorm_i8_ex / _compat, csrc/ln_stream.h ln_stream_takes / ln_stream_pays)
    "min" strides (C + 4 / C + 12, base + 4 bytes): ln_stream_takes is false for every form (ld % 16, pointer % 16), so lab form 4
      falls through: product and forms 4, 3 -> v2 at C = 768, half wave at C <= 384, wave per row (NJ = 2 at 388, 8 at 1100);
      form 2 -> half wave up to C = 1536; form 1 -> wave per row.  _compat: v2 up to C = 1024, wave per row beyond or under form 1.
    "al16" strides (C + 16 / C + 32): the same ladder, and under lab form 4 the streaming kernel at C = 192 and 768.
    streaming threshold: 15 627 x 768 >= 12 000 000, ldx 784, ldo 800, all 16-byte aligned: the product itself streams.
    class rows: rows = 8, ldx = 197 C: below the threshold (v2 / half wave); lab form 4 streams with (rows - 1) ldx + C buffer sizes.
  16-bit LayerNorm (csrc/swin.hip ln16_tiling): ldo = C + 5 -> the wave-per-row / literal kernels (ldo % 8 != 0), ldo = C + 16 -> the
    tiled kernels (LPR 4, NJ 3 at C = 96; LPR 32, NJ 3 at C = 768), plain and compat with fast_division 1; fast_division 0 literal.
  I-BERT LayerNorm (csrc/ibert.hip): int8 C + 3 / C + 5 -> `fast` false, the literal kernel; C + 16 / C + 32 -> the fast kernel (NJ 1, 3);
    int16: C = 768 the register kernel NK = 12 on both stride pairs (element accesses), C = 96 the literal one.
  ShiftGELU table (csrc/rowops.hip ivit_shiftgelu_lut_i8_ex): L = 388, 1100, 2052, 3100 at 7 rows -> a wave per row NJ = 3, 6, 12 and
    the generic form; 4099 rows of L = 96, 200, 380 -> half a wave per row NJ = 1, 2, 3 (rows >= 4096 and L <= 384), lab bit 24 -> NJ 3
    whole wave; block-layout input: the INB instantiations of the same kernels.
  GEMM (csrc/gemm.hip launch_gemm): M = 258 or 8 -> gemm_i8_kernel (below M = 2048); M = 8197, N = 96, K = 64 / 128 -> the skinny-K
    admission (lda % 16, ldw % 8, ldo % 16 hold at K + 16 / N + 16) with its compile-time K = 64 / 128 forms, lab flags2 bit 21 the
    run-time-K form; M = 2125, N = K = 192 -> the persistent kernel (layouts 0, row-major W with ldw = K + 64), gemm_i8_wreg_kernel
    with IVIT_W_FRAGS and, for IVIT_W_FRAGS16, its 16x16x64 form, whose epilogue addresses output and residual with 32-bit
    row * ld offsets."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as ISQ  # noqa: E402
from ivit_amd.prepare import LayerNormParams, dyadic, markstein_division_ok, phi_tables, window_shiftexp_band  # noqa: E402

import fenced  # noqa: E402
import ibert_intsqrt_ref as R  # noqa: E402
import ln_cert_ref  # noqa: E402

DEV = "cuda:0"
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


def fout(rows, width, ld, dtype, expected, **kw):
    b = fenced.output(rows, width, ld, dtype, expected=expected, device=DEV, **kw)
    _KEEP.append(b)
    return b


def refused(match, name, *args):
    with pytest.raises(_lib.IvitError, match=match) as ei:
        _lib.call(name, *args)
    assert "(-1)" in str(ei.value), f"{name}: expected IVIT_ERR_INVALID, got {ei.value}"


@pytest.fixture(params=[0, 4, 3, 2, 1], ids=["product", "lab_streaming", "lab_grouped", "lab_half_wave_per_row", "lab_wave_per_row"])
def ln_form(request):
    """as in test_gpu_ops.py: the product's own choice of int8 LayerNorm kernel, and every form forced through the lab build (a form
    that cannot take a width falls through to the next one of the launcher's ladder)"""
    if request.param == 0:
        yield 0
        return
    with _lib.lab_session():
        _lib.call("ivit_debug_ln_wave_per_row", request.param)
        yield request.param


class Tables:
    """per-channel LayerNorm constants on the device"""

    def __init__(self, gamma, beta, s_out):
        self.lp = lp = LayerNormParams(gamma, beta, s_out)
        self.args = (p(dev(lp.bias_int)), p(dev(lp.s_ln)), p(dev(lp.m.view(np.int32))), p(dev(lp.e)))


def _wide(v, n):
    return np.concatenate([v, v[:n - len(v)]])


def ln_oracle(gamma, beta, s_out, layernorm=orc.layernorm):
    """LayerNorm + QuantAct as a function of the input matrix (of C or, for the poison condition, a few more columns)"""
    def f(x):
        n = x.shape[1]
        y, s_ln = layernorm(x.astype(np.int32), _wide(gamma, n), _wide(beta, n))[:2]
        m, e = orc.dyadic(s_ln, s_out)
        return orc.requant(orc.roundtrip(y, s_ln), m, e, 8)
    return f


# =========================================================================================== I-ViT LayerNorm, int8
LN_STRIDES = {"min": (4, 12, 4), "al16": (16, 32, 0)}      # ldx - C, ldo - C, lead_bytes: ln8_check admits ld % 4 == 0 and 4-byte pointers


@functools.lru_cache(maxsize=None)
def ln8_case(C):
    """37 rows, 18 of them with a failing certificate (tests/ln_cert_ref.py): the literal tail runs on strided rows too"""
    k, gamma, beta = ln_cert_ref.draw_i8(C)
    ks, s_out, exp, _ = ln_cert_ref.case(k, gamma, beta)
    return ks, gamma, beta, s_out, exp


@functools.lru_cache(maxsize=None)
def ln8_compat_case(C, rows=37, s=0.0371):
    rng = np.random.default_rng(C + rows)
    s = f32(s)
    q = np.clip(np.rint(rng.normal(rng.normal(0, 10, size=(rows, 1)), rng.uniform(1, 50, size=(rows, 1)), size=(rows, C))), -128, 127).astype(np.int32)
    for r in range(0, rows, 3):        # exact ties of the mean, as test_layernorm_compat_random_vs_oracle makes them
        d = C // 2 + C * int(rng.integers(-10, 10)) - int(q[r].sum())
        for c in rng.permutation(C):
            if d == 0:
                break
            nv = int(np.clip(q[r, c] + d, -128, 127))
            d -= nv - q[r, c]
            q[r, c] = nv
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    y, s_ln = orc.layernorm_compat(q, s, gamma, beta)[:2]
    s_out = f32(np.abs(y * s_ln).max() / 127 * 0.83)
    lay = lambda x, g, b: orc.layernorm_compat(x, s, g, b)      # noqa: E731
    exp = ln_oracle(gamma, beta, s_out, lay)(q)
    return q.astype(np.int8), s, gamma, beta, s_out, exp, lay


@pytest.mark.parametrize("strides", list(LN_STRIDES))
@pytest.mark.parametrize("C", [96, 192, 388, 768, 1100])
def test_layernorm_i8_strided_rows(C, strides, ln_form):
    """ivit_layernorm_i8 / _ex: ldx = C + 4, ldo = C + 12 from a 4-byte-aligned base (no streaming kernel: ln_stream_takes wants 16
    bytes everywhere) and ldx = C + 16, ldo = C + 32 (the streaming kernel under lab form 4 at C = 192, 768)"""
    dx, do, lead = LN_STRIDES[strides]
    k, gamma, beta, s_out, exp = ln8_case(C)
    rows = len(k)
    t = Tables(gamma, beta, s_out)
    x = fin(k, C + dx, 127, lead_bytes=lead, oracle=ln_oracle(gamma, beta, s_out), expected=exp)
    o = fout(rows, C, C + do, np.int8, exp, lead_bytes=lead)
    _lib.call("ivit_layernorm_i8", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, st())
    fenced.check(o, exp)
    o = fout(rows, C, C + do, np.int8, exp, lead_bytes=lead)
    _lib.call("ivit_layernorm_i8_ex", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, 0, st())
    fenced.check(o, exp)
    fenced.check(x)


@pytest.mark.parametrize("strides", list(LN_STRIDES))
@pytest.mark.parametrize("C", [96, 192, 768, 1096])
def test_layernorm_i8_compat_strided_rows(C, strides, ln_form):
    """ivit_layernorm_i8_compat (natural input scale, every third row an exact tie of the mean) on the same two stride pairs"""
    dx, do, lead = LN_STRIDES[strides]
    q, s, gamma, beta, s_out, exp, lay = ln8_compat_case(C)
    rows = len(q)
    t = Tables(gamma, beta, s_out)
    remap, phi = phi_tables(s)
    x = fin(q, C + dx, 127, lead_bytes=lead, oracle=ln_oracle(gamma, beta, s_out, lay), expected=exp)
    o = fout(rows, C, C + do, np.int8, exp, lead_bytes=lead)
    _lib.call("ivit_layernorm_i8_compat", x.ptr, x.ld, rows, C, *t.args, p(dev(remap)), p(dev(phi)), o.ptr, o.ld, 0, st())
    fenced.check(o, exp)
    fenced.check(x)


@pytest.mark.parametrize("entry", ["ivit_layernorm_i8", "ivit_layernorm_i8_compat"])
@pytest.mark.parametrize("C", [192, 768])
def test_layernorm_i8_class_rows(C, entry, ln_form):
    """the geometry of the pruned last block (engine.py _cls_block): 8 class rows, ldx = 197 * C, ldo = C; the 196 tokens between
    two class rows are poison here"""
    T, B = 197, 8
    if entry == "ivit_layernorm_i8":
        k, gamma, beta, s_out, exp = ln8_case(C)
        extra, orac = (), ln_oracle(gamma, beta, s_out)
    else:
        k, s, gamma, beta, s_out, exp, lay = ln8_compat_case(C)
        remap, phi = phi_tables(s)
        extra, orac = (p(dev(remap)), p(dev(phi))), ln_oracle(gamma, beta, s_out, lay)
    k, exp = k[5:5 + B], exp[5:5 + B]                      # rows of the dense case: the same rows of its reference
    t = Tables(gamma, beta, s_out)
    x = fin(k, T * C, 127, oracle=orac, expected=exp)
    o = fout(B, C, C, np.int8, exp)
    if entry == "ivit_layernorm_i8":
        _lib.call("ivit_layernorm_i8", x.ptr, x.ld, B, C, *t.args, o.ptr, o.ld, st())
    else:
        _lib.call("ivit_layernorm_i8_compat", x.ptr, x.ld, B, C, *t.args, *extra, o.ptr, o.ld, 0, st())
    fenced.check(o, exp)


def test_layernorm_i8_streaming_threshold():
    """rows x C >= 12 000 000 (ln_stream_pays) at C = 768 with ldx = 784, ldo = 800: the product's own dispatch takes the streaming
    kernel with strided buffer resources"""
    C, rows = 768, 15627
    assert rows * C >= 12_000_000
    rng = np.random.default_rng(rows)
    k = np.clip(np.rint(rng.normal(rng.normal(0, 10, size=(rows, 1)), rng.uniform(1, 50, size=(rows, 1)), size=(rows, C))), -128, 127).astype(np.int8)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    y, s_ln, _ = orc.layernorm(k.astype(np.int32), gamma, beta)
    s_out = f32(2.0 ** np.ceil(np.log2(np.abs(y * s_ln).max() / 127 * 0.8)))
    orac = ln_oracle(gamma, beta, s_out)
    exp = orac(k)
    t = Tables(gamma, beta, s_out)
    x = fin(k, 784, 127, oracle=orac, expected=exp)
    o = fout(rows, C, 800, np.int8, exp)
    _lib.call("ivit_layernorm_i8", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, st())
    fenced.check(o, exp)


@pytest.mark.parametrize("C", [192, 768])
def test_layernorm_i8_block_layout_from_strided_rows(C, ln_form):
    """out_blocks = 1 (ldo == C) from ldx = C + 16: fenced behind the padded size, the defined rows at their documented offsets and
    once more through ivit_untile_operand_i8 into strided rows"""
    k, gamma, beta, s_out, exp = ln8_case(C)
    rows = len(k)
    t = Tables(gamma, beta, s_out)
    x = fin(k, C + 16, 127, oracle=ln_oracle(gamma, beta, s_out), expected=exp)
    o = fout(rows, C, C, np.int8, exp, blocks=True)
    _lib.call("ivit_layernorm_i8_ex", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, 1, st())
    fenced.check(o, exp)
    u = fout(rows, C, C + 48, np.int8, exp)
    _lib.call("ivit_untile_operand_i8", o.ptr, rows, C, u.ptr, u.ld, st())
    fenced.check(u, exp)


def test_layernorm_i32_f32_strided_rows():
    """the module-level form, no alignment rule: C = 100, ldx = C + 3, ldo = C + 5, 16-bit values, float output y * s_ln"""
    C, rows = 100, 37
    rng = np.random.default_rng(C)
    k = rng.integers(-30000, 30001, size=(rows, C)).astype(np.int32)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    lp = LayerNormParams(gamma, beta, f32(0.03))

    def orac(x):
        y, s_ln, _ = orc.layernorm(x, _wide(gamma, x.shape[1]), _wide(beta, x.shape[1]))
        return (y * s_ln).astype(f32)
    exp = orac(k)
    x = fin(k, C + 3, 2 ** 30, lead_bytes=4, oracle=orac, expected=exp)
    o = fout(rows, C, C + 5, np.float32, exp, lead_bytes=4)
    _lib.call("ivit_layernorm_i32_f32", x.ptr, x.ld, rows, C, p(dev(lp.bias_int)), p(dev(lp.s_ln)), o.ptr, o.ld, st())
    fenced.check(o, exp)
    fenced.check(x)


# =========================================================================================== Swin / 16-bit LayerNorm
def _win_order(a, B, H, ws, shift):
    """row r of `a` (image order) -> row win_row(r): roll by -shift, window partition (as test_layernorm_i16_i8_window_order)"""
    C = a.shape[1]
    return orc._win_partition(np.roll(a.reshape(B, H, H, C), (-shift, -shift), axis=(1, 2)), ws).reshape(-1, C)


@pytest.mark.parametrize("do", [5, 16], ids=["ldo_C+5", "ldo_C+16"])
@pytest.mark.parametrize("C", [96, 768])
def test_layernorm_i16_i8_strided_output(C, do):
    """ivit_layernorm_i16_i8 and ivit_layernorm_i16_i8_compat (fast_division 0 / 1): ldo = C + 5 (no alignment rule: the wave-per-row
    kernel, ln16_tiling wants ldo % 8 == 0) and ldo = C + 16 (the tiled kernels); 37 rows in row order and 64 rows through a window
    map (H = W = 8, ws = 4, shift = 2), where the permuted row index is what ldo multiplies"""
    s_in = f32(0.000913)
    assert markstein_division_ok(s_in, 16)
    rng = np.random.default_rng(C)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = (rng.standard_normal(C) * 0.1).astype(f32)
    s_out = f32(4.0 / 127.0)
    t = Tables(gamma, beta, s_out)
    for rows, geo in ((37, (0, 0, 0, 0)), (64, (8, 8, 4, 2))):
        xh = rng.integers(-20000, 20001, size=(rows, C)).astype(np.int16)
        xh[0] = 0
        x = fin(xh, C)                                       # the entry takes dense rows: guards only
        for name, extra, lay in (("plain", (), orc.layernorm),
                                 ("compat", (float(s_in), 0), lambda q, g, b: orc.layernorm_scaled(q, s_in, g, b)),
                                 ("compat", (float(s_in), 1), lambda q, g, b: orc.layernorm_scaled(q, s_in, g, b))):
            exp = ln_oracle(gamma, beta, s_out, lay)(xh)
            if geo[2]:
                exp = _win_order(exp, 1, geo[0], geo[2], geo[3])
            o = fout(rows, C, C + do, np.int8, exp)
            if name == "plain":
                _lib.call("ivit_layernorm_i16_i8", x.ptr, rows, C, *t.args, o.ptr, o.ld, *geo, st())
            else:
                _lib.call("ivit_layernorm_i16_i8_compat", x.ptr, rows, C, *extra, *t.args, o.ptr, o.ld, *geo, st())
            fenced.check(o, exp)
        fenced.check(x)


# =========================================================================================== engine forms of the I-BERT LayerNorm
def ibert_ln_oracle(gamma, beta, s_in, shift_pow2, isq):
    """IBERTIntLayerNorm (tests/ibert_intsqrt_ref.py, op for op) + the QuantAct behind it, as test_gpu_ibert_intsqrt.expected does;
    row sums below 2^24 (asserted by the caller): exact in any order"""
    lp = LayerNormParams(gamma, beta, float(f32(3.1 / 127)))

    def f(q):
        n = q.shape[1]
        bias_int, s_out = R.layernorm_constants(_wide(gamma, n), _wide(beta, n))
        M = _wide(lp.m.astype(np.float64) * np.exp2(-lp.e.astype(np.float64)), n)
        y = R.layernorm(R.x_int_of(q.astype(np.int32), s_in), bias_int, s_out, shift_pow2, int_sqrt=isq)
        with np.errstate(invalid="ignore"):
            zq = np.rint((y / s_out).astype(f32))
            return np.fmin(np.fmax(np.rint(zq.astype(np.float64) * M), -128.0), 127.0).astype(np.int8)
    return lp, f


@pytest.mark.parametrize("strides", ["min", "al16"])
@pytest.mark.parametrize("C", [96, 768])
@pytest.mark.parametrize("bits", [8, 16])
def test_ibert_layernorm_engine_forms_strided_rows(bits, C, strides):
    """ivit_ibert_layernorm_i8 (flags 0 / IVIT_IBERT_LN_INT_SQRT), ivit_ibert_layernorm_i16_i8 and _ex (fast_division 0 / 1, with and
    without the flag): ldx = C + 3, ldo = C + 5 from element-aligned base pointers (nothing is required: the int8 entry then runs its literal kernel) and ldx = C + 16,
    ldo = C + 32 (its fast kernel)"""
    dx, do = {"min": (3, 5), "al16": (16, 32)}[strides]
    rows = 37
    rng = np.random.default_rng(C + bits)
    s_in, sigma, dt = (f32(2.0 ** -4), 30.0, np.int8) if bits == 8 else (f32(2.0 ** -9), 80.0, np.int16)
    lim = 127 if bits == 8 else 32767
    q = np.clip(np.rint(rng.normal(rng.normal(0, 5, size=(rows, 1)), sigma, size=(rows, C))), -lim - 1, lim).astype(dt)
    q[1] = q[1, 0]
    q[1, 3] += 9                                           # tiny variance
    assert (q.astype(np.int64) ** 2).sum(1).max() < 2 ** 24 and markstein_division_ok(s_in, 16)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.uniform(-1, 1, size=C).astype(f32)
    for isq in (False, True):
        lp, orac = ibert_ln_oracle(gamma, beta, s_in, 1.0, isq)
        exp = orac(q)
        assert np.abs(exp.astype(np.int32)).max() > 50
        lead = q.itemsize if strides == "min" else 0      # no alignment rule: a base pointer aligned to the element only
        x = fin(q, C + dx, lead_bytes=lead, oracle=orac, expected=exp)
        tabs = (p(dev(lp.bias_int)), p(dev(lp.s_ln)), 1.0, p(dev(lp.m.view(np.int32))), p(dev(lp.e)))
        flag = ISQ if isq else 0
        if bits == 8:
            o = fout(rows, C, C + do, np.int8, exp, lead_bytes=1 if strides == "min" else 0)
            _lib.call("ivit_ibert_layernorm_i8", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, flag, st())
            fenced.check(o, exp)
        else:
            if not isq:
                o = fout(rows, C, C + do, np.int8, exp)
                _lib.call("ivit_ibert_layernorm_i16_i8", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, st())
                fenced.check(o, exp)
            for fd in (0, 1):
                o = fout(rows, C, C + do, np.int8, exp)
                _lib.call("ivit_ibert_layernorm_i16_i8_ex", x.ptr, x.ld, rows, C, float(s_in), *tabs, o.ptr, o.ld, fd | flag, st())
                fenced.check(o, exp)
        fenced.check(x)


@pytest.mark.parametrize("isq", [False, True], ids=["float_sqrt", "int_sqrt"])
def test_ibert_layernorm_module_forms_ex_strided_rows(isq):
    """ivit_ibert_layernorm_i32_f32_ex and ivit_ibert_layernorm_f32_f32_ex (flags 0 / IVIT_IBERT_LN_INT_SQRT): C = 100, ldx = C + 3,
    ldo = C + 5; the entries without `flags` have this in test_gpu_ibert_ops.py, these two ran with ld == C only"""
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
        b, so = R.layernorm_constants(_wide(gamma, n), _wide(beta, n))
        with np.errstate(over="ignore", invalid="ignore"):      # the poisoned dword of the effectiveness check overflows float32
            return R.layernorm(x_int, b, so, 1.0, int_sqrt=isq)

    def orac(q):
        return lay(R.x_int_of(q, s_in))
    exp = orac(k)
    assert np.isfinite(exp).all()
    flag = ISQ if isq else 0
    tabs = (p(dev(bias_int)), p(dev(s_out)), 1.0)
    x = fin(k, C + 3, oracle=orac, expected=exp)
    o = fout(rows, C, C + 5, np.float32, exp)
    _lib.call("ivit_ibert_layernorm_i32_f32_ex", x.ptr, x.ld, rows, C, *tabs, o.ptr, o.ld, flag, st())
    fenced.check(o, exp)
    fenced.check(x)
    xf = fin((k.astype(f32) * s_in).astype(f32), C + 3, oracle=lambda v: lay((v / s_in).astype(f32)), expected=exp)
    o = fout(rows, C, C + 5, np.float32, exp)
    _lib.call("ivit_ibert_layernorm_f32_f32_ex", xf.ptr, xf.ld, rows, C, p(dev(np.array([s_in], f32))), 1, *tabs, o.ptr, o.ld, flag, st())
    fenced.check(o, exp)
    fenced.check(xf)


# =========================================================================================== ShiftGELU
GELU_S = f32(2.0 ** -4)


@functools.lru_cache(maxsize=None)
def gelu_case(rows, L):
    rng = np.random.default_rng(rows * 7 + L)
    k = np.clip(np.rint(rng.normal(0, 35, size=(rows, L))), -128, 120).astype(np.int8)      # row maxima below the poison 127
    k[::3] = np.minimum(k[::3], -3)                                                          # rows with a negative maximum
    y, s_go = orc.shiftgelu(k.astype(np.int32), GELU_S)
    m, e = dyadic(s_go, f32(2.0 ** -4))

    def orac(x):
        return orc.requant(orc.shiftgelu(x.astype(np.int32), GELU_S)[0], m.astype(np.float64), e, 8)
    return k, y, (int(m[0]), int(e[0])), orac, orac(k)


@functools.lru_cache(maxsize=None)
def _gelu_lut_host(me):
    lut = torch.empty(65536, dtype=torch.int8, device=DEV)
    _lib.call("ivit_shiftgelu_build_lut", float(GELU_S), me[0], me[1], p(lut), st())
    torch.cuda.synchronize()
    return lut.cpu().numpy()


def gelu_lut(me):
    return dev(_gelu_lut_host(me))


@pytest.mark.parametrize("dx,do", [(3, 5), (16, 32)])
@pytest.mark.parametrize("L", [50, 257])
def test_shiftgelu_direct_strided_rows(L, dx, do):
    """ivit_shiftgelu_i8 and ivit_shiftgelu_i8_i32: no alignment rule at all (L + 3 / L + 5 from an odd base address)"""
    rows = 7
    k, y, me, orac, exp = gelu_case(rows, L)
    lead = 1 if dx == 3 else 0
    x = fin(k, L + dx, 127, lead_bytes=lead, oracle=orac, expected=exp)
    o = fout(rows, L, L + do, np.int8, exp, lead_bytes=lead)
    _lib.call("ivit_shiftgelu_i8", x.ptr, x.ld, rows, L, float(GELU_S), me[0], me[1], o.ptr, o.ld, st())
    fenced.check(o, exp)
    x32 = fin(k, L + dx, 127, lead_bytes=lead, oracle=lambda a: orc.shiftgelu(a.astype(np.int32), GELU_S)[0], expected=y)
    o32 = fout(rows, L, L + do, np.int32, y)
    _lib.call("ivit_shiftgelu_i8_i32", x32.ptr, x32.ld, rows, L, float(GELU_S), o32.ptr, o32.ld, st())
    fenced.check(o32, y)
    fenced.check(x)
    fenced.check(x32)


# (rows, L, lab bit 24): one L for every instantiation ivit_shiftgelu_lut_i8_ex selects -- a wave per row NJ = 3 (L <= 768), 6 (<= 1536),
# 12 (<= 3072), the generic form beyond; half a wave per row NJ = 1 (L <= 128), 2 (<= 256), 3 (<= 384) from 4096 rows; and the
# whole-wave form where the half-wave one would run (lab bit 24)
GELU_LUT_CASES = [(7, 388, 0), (7, 1100, 0), (7, 2052, 0), (7, 3100, 0), (4099, 96, 0), (4099, 200, 0), (4099, 380, 0), (4099, 380, 1)]


@pytest.mark.parametrize("strides", ["min", "al16"])
@pytest.mark.parametrize("rows,L,whole_wave", GELU_LUT_CASES)
def test_shiftgelu_lut_strided_rows(rows, L, whole_wave, strides):
    """ivit_shiftgelu_lut_i8 / _ex row-major: L + 4 / L + 12 from a 4-byte-aligned base, L + 16 / L + 32; then in place with equal
    strides (out == x, ldx == ldo == L + 16): the pad keeps its poison"""
    dx, do, lead = {"min": (4, 12, 4), "al16": (16, 32, 0)}[strides]
    k, _, me, orac, exp = gelu_case(rows, L)
    lut = gelu_lut(me)

    def run():
        x = fin(k, L + dx, 127, lead_bytes=lead, oracle=orac, expected=exp)
        o = fout(rows, L, L + do, np.int8, exp, lead_bytes=lead)
        _lib.call("ivit_shiftgelu_lut_i8", x.ptr, x.ld, rows, L, p(lut), o.ptr, o.ld, st())
        fenced.check(o, exp)
        fenced.check(x)
        o = fout(rows, L, L + do, np.int8, exp, lead_bytes=lead)
        _lib.call("ivit_shiftgelu_lut_i8_ex", x.ptr, x.ld, rows, L, p(lut), o.ptr, o.ld, 0, st())
        fenced.check(o, exp)
        if strides == "al16":
            xi = fin(k, L + 16, 127, oracle=orac, expected=exp)
            _lib.call("ivit_shiftgelu_lut_i8_ex", xi.ptr, xi.ld, rows, L, p(lut), xi.ptr, xi.ld, 0, st())
            fenced.check(xi, exp)
    if whole_wave:
        with _lib.lab_session():
            _lib.call("ivit_debug_ln_ablate", 1 << 24)
            run()
    else:
        run()


@pytest.mark.parametrize("rows,L", [(7, 384), (7, 3136), (4099, 384)])
def test_shiftgelu_lut_between_block_layout_and_strided_rows(rows, L):
    """block-layout input -> strided row-major output and strided row-major input -> block-layout output (wave-per-row NJ = 3, the
    generic form, half a wave per row)"""
    k, _, me, orac, exp = gelu_case(rows, L)
    lut = gelu_lut(me)
    R16 = (rows + 15) // 16 * 16
    tiled = np.full(R16 * L, 127, np.int8)                 # the pad rows of the last block: poison as well
    tiled[fenced.block_offsets(rows, L)] = k
    xb = fenced.input_blocks(tiled, rows, L, 127, device=DEV)
    _KEEP.append(xb)
    o = fout(rows, L, L + 16, np.int8, exp)
    _lib.call("ivit_shiftgelu_lut_i8_ex", xb.ptr, L, rows, L, p(lut), o.ptr, o.ld, 2, st())
    fenced.check(o, exp)
    fenced.check(xb)
    x = fin(k, L + 32, 127, oracle=orac, expected=exp)
    ob = fout(rows, L, L, np.int8, exp, blocks=True)
    _lib.call("ivit_shiftgelu_lut_i8_ex", x.ptr, x.ld, rows, L, p(lut), ob.ptr, ob.ld, 1, st())
    fenced.check(ob, exp)
    fenced.check(x)


# =========================================================================================== GEMM
def rand_me(rng, n, lo_exp, hi_exp):
    pre = (rng.uniform(0.5, 1.0, size=n) * 2.0 ** rng.integers(lo_exp, hi_exp, size=n)).astype(f32)
    return dyadic(pre, f32(1.0))


class Gemm:
    """one problem: A [M, K] (lda), W [N, K] (ldw), bias, per-channel requantiser; the oracle's accumulators and 8 / 16-bit QuantAct"""

    def __init__(self, M, N, K, lda, ldw, seed, wide16=False):
        rng = self.rng = np.random.default_rng(seed)
        self.M, self.N, self.K = M, N, K
        self.A = rng.integers(-128, 127, size=(M, K)).astype(np.int8)       # below the poison 127
        self.W = rng.integers(-128, 127, size=(N, K)).astype(np.int8)
        self.b = rng.integers(-50000, 50000, size=N).astype(np.int32)
        self.m, self.e = rand_me(rng, N, -16, -9)
        self.m16, self.e16 = rand_me(rng, N, -8, 1)
        self.acc = orc.gemm_i8(self.A, self.W, self.b)
        self.k8 = orc.requant(self.acc, self.m.astype(np.float64), self.e, 8)
        self.k16 = orc.requant(self.acc, self.m16.astype(np.float64), self.e16, 16)
        # the poison condition of A: a kernel that runs its K loop one dword too far takes in the pads of A and W (127 * 127 each)
        Ww = np.concatenate([self.W, np.full((N, 4), 127, np.int8)], axis=1)
        self.a = fin(self.A, lda, 127, oracle=lambda Aw: orc.requant(orc.gemm_i8(Aw, Ww, self.b), self.m.astype(np.float64), self.e, 8),
                     expected=self.k8)
        self.w = fin(self.W, ldw, 127)
        self.db = dev(self.b)
        self.me = (p(dev(self.m.view(np.int32))), p(dev(self.e)))
        self.me16 = (p(dev(self.m16.view(np.int32))), p(dev(self.e16)))

    @property
    def head(self):
        return (self.a.ptr, self.a.ld, self.w.ptr, self.w.ld, p(self.db))

    def residual(self, bits, s_main=0.3337, s_res=0.0421, s_out=0.0517, k=None, res=None):
        """-> res [M, N] (drawn unless given), the four scalars of the residual QuantAct, expected output on k (default: the 8-bit
        QuantAct of the accumulators)"""
        if res is not None:
            pass
        elif bits == 8:
            res = self.rng.integers(-128, 128, size=(self.M, self.N)).astype(np.int8)
        else:
            res = np.clip(np.rint(self.rng.normal(0, 9000, size=(self.M, self.N))), -32768, 32767).astype(np.int16)
        m1, e1 = dyadic(f32(s_main), f32(s_out))
        m2, e2 = dyadic(f32(s_res), f32(s_out))
        exp = orc.requant(self.k8 if k is None else k, m1.astype(np.float64), e1, bits, z2=res.astype(np.int32), m2=m2.astype(np.float64), e2=e2)
        return res, (int(m1[0]), int(e1[0]), int(m2[0]), int(e2[0])), exp

    def check_inputs(self):
        fenced.check(self.a)
        fenced.check(self.w)


def head_major(X, B, T, H, hd, planes=3):
    return np.ascontiguousarray(X.reshape(B, T, planes, H, hd).transpose(2, 0, 3, 1, 4))


def test_gemm_small_kernel_int8_epilogues_strided():
    """gemm_i8_kernel (M < 2048): M = 2 tiles + 2, N = 208 = 1 tile + 80, K = 128, lda = K + 16, ldw = K + 32; requant (ldo = N + 16),
    residual (ldr = N + 32, and in place with ldo == ldr)"""
    M, N, K = 258, 208, 128
    g = Gemm(M, N, K, K + 16, K + 32, 1)
    for entry, extra in (("plain", ()), ("ex", (0,))):
        o = fout(M, N, N + 16, np.int8, g.k8)
        if entry == "plain":
            _lib.call("ivit_gemm_i8_requant", *g.head, *g.me, o.ptr, o.ld, M, N, K, st())
        else:
            _lib.call("ivit_gemm_i8_requant_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, st())
        fenced.check(o, g.k8)
    res, sc, exp = g.residual(8)
    r = fin(res, N + 32)
    o = fout(M, N, N + 16, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_residual", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, st())
    fenced.check(o, exp)
    o = fout(M, N, N + 16, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_residual_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, exp)
    fenced.check(r)
    _lib.call("ivit_gemm_i8_requant_residual", *g.head, *g.me, r.ptr, r.ld, *sc, r.ptr, r.ld, M, N, K, st())     # in place
    fenced.check(r, exp)
    g.check_inputs()


def test_gemm_small_kernel_16_bit_epilogues_strided():
    """residual_i16 (both entries) and i16_residual_i16 with layouts = 0: ldr = N + 8, ldo = N + 24 (multiples of 8 elements), and
    in place"""
    M, N, K = 258, 208, 128
    g = Gemm(M, N, K, K + 16, K + 32, 2)
    res, sc, exp = g.residual(16)
    r = fin(res, N + 8)
    o = fout(M, N, N + 24, np.int16, exp)
    _lib.call("ivit_gemm_i8_requant_residual_i16", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, st())
    fenced.check(o, exp)
    o = fout(M, N, N + 24, np.int16, exp)
    _lib.call("ivit_gemm_i8_requant_residual_i16_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, exp)
    _, _, exp16 = g.residual(16, k=g.k16, res=res)
    o = fout(M, N, N + 24, np.int16, exp16)
    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", *g.head, *g.me16, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, exp16)
    fenced.check(r)
    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", *g.head, *g.me16, r.ptr, r.ld, *sc, r.ptr, r.ld, M, N, K, 0, st())
    fenced.check(r, exp16)
    g.check_inputs()


def test_gemm_small_kernel_wide_outputs_strided():
    """requant_i16 and the raw int32 accumulators: N = 204 (N % 4 == 0), ldo = N + 4"""
    M, N, K = 258, 204, 128
    g = Gemm(M, N, K, K + 16, K + 32, 3)
    o = fout(M, N, N + 4, np.int16, g.k16)
    _lib.call("ivit_gemm_i8_requant_i16", *g.head, *g.me16, o.ptr, o.ld, M, N, K, st())
    fenced.check(o, g.k16)
    o = fout(M, N, N + 4, np.int32, g.acc)
    _lib.call("ivit_gemm_i8_i32", *g.head, o.ptr, o.ld, M, N, K, st())
    fenced.check(o, g.acc)
    g.check_inputs()


def test_gemm_small_kernel_head_major_outputs():
    """qkv, qkv_ex and qkv_planes_ex from strided A and W: the dense head-major output fenced before and behind; with planes 1 .. 2
    selected, plane 0 of the buffer is the guard in front"""
    B, T, H, hd, K = 6, 43, 5, 16, 128
    M, N = B * T, 3 * H * hd                               # 258 x 240: two tiles + 2, one tile + 112
    g = Gemm(M, N, K, K + 16, K + 32, 4)
    exp = head_major(g.k8, B, T, H, hd).reshape(-1, hd)
    for entry in ("plain", "ex"):
        o = fout(len(exp), hd, hd, np.int8, exp)
        if entry == "plain":
            _lib.call("ivit_gemm_i8_requant_qkv", *g.head, *g.me, o.ptr, T, H, hd, M, N, K, st())
        else:
            _lib.call("ivit_gemm_i8_requant_qkv_ex", *g.head, *g.me, o.ptr, T, H, hd, M, N, K, 0, st())
        fenced.check(o, exp)
    plane = M * H * hd
    Cn = H * hd
    exp2 = exp[len(exp) // 3:]
    o = fout(len(exp2), hd, hd, np.int8, exp2, guard_bytes=plane)
    w1 = ctypes.c_void_p(g.w.ptr.value + Cn * g.w.ld)      # the first selected channel
    _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", g.a.ptr, g.a.ld, w1, g.w.ld, p(g.db[Cn:]), p(dev(g.m.view(np.int32)[Cn:])), p(dev(g.e[Cn:])),
              ctypes.c_void_p(o.ptr.value - plane), T, H, hd, 1, 2, M, 2 * Cn, K, 0, st())
    fenced.check(o, exp2)
    g.check_inputs()


def test_gemm_small_kernel_class_row_residual():
    """the residual GEMM of engine.py _cls_block: M = 8 class rows, ldr = 197 * N, N = 192"""
    M, N, K = 8, 192, 192
    g = Gemm(M, N, K, K + 16, K + 32, 5)
    res, sc, exp = g.residual(8)
    r = fin(res, 197 * N)
    o = fout(M, N, N, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_residual_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, exp)
    fenced.check(r)
    g.check_inputs()


@pytest.mark.parametrize("K,any_k", [(64, 0), (128, 0), (64, 1)])
def test_gemm_skinny_k_strided(K, any_k):
    """gemm_i8_skinny_kernel (M >= 8192): M = 8192 + 5, N = 96, lda = ldw = K + 16, ldo = N + 16; the compile-time K = 64 and 128
    forms the product selects and the run-time-K form (lab flags2 bit 21; the entry's K % 64 == 0 leaves it no K of its own);
    requant and head-major epilogues"""
    M, N, hd = 8197, 96, 32
    T, H = 1171, 1                                          # 8197 = 7 x 1171
    g = Gemm(M, N, K, K + 16, K + 16, 10 + K + any_k)
    exp_q = head_major(g.k8, M // T, T, H, hd).reshape(-1, hd)

    def run():
        o = fout(M, N, N + 16, np.int8, g.k8)
        _lib.call("ivit_gemm_i8_requant_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, st())
        fenced.check(o, g.k8)
        o = fout(len(exp_q), hd, hd, np.int8, exp_q)
        _lib.call("ivit_gemm_i8_requant_qkv_ex", *g.head, *g.me, o.ptr, T, H, hd, M, N, K, 0, st())
        fenced.check(o, exp_q)
    if any_k:
        with _lib.lab_session():
            _lib.call("ivit_debug_set_gemm_flags2", 1 << 21)
            run()
    else:
        run()
    g.check_inputs()


def _pack(g, entry):
    """the fragment-packed copy of g.W made from its STRIDED rows"""
    Wf = torch.zeros((g.N + 63) // 64 * 64 * g.K, dtype=torch.int8, device=DEV)
    _KEEP.append(Wf)
    if entry == 8:
        _lib.call("ivit_pack_weight_frags_i8", g.w.ptr, g.w.ld, g.N, g.K, p(Wf), st())
    else:
        _lib.call("ivit_pack_weight_frags16_i8", g.w.ptr, g.w.ld, g.N, g.K, p(Wf), st())
    return Wf


def test_gemm_large_kernels_16_bit_epilogues_strided():
    """M = 2048 + 77, N = 192, K = 192: ivit_gemm_i8_requant_residual_i16_ex on the persistent kernel (layouts 0, row-major W with
    ldw = K + 64) and on both fragment forms, ivit_gemm_i8_requant_i16_residual_i16_ex with IVIT_W_FRAGS; ldr = N + 8, ldo = N + 24,
    32-bit row * ld offsets with ld > width"""
    M, N, K = 2125, 192, 192
    g = Gemm(M, N, K, K + 16, K + 64, 20)
    res, sc, exp = g.residual(16)
    r = fin(res, N + 8)
    for lay in (0, 8, 16):
        w = (g.w.ptr, g.w.ld) if lay == 0 else (p(_pack(g, lay)), K)
        o = fout(M, N, N + 24, np.int16, exp)
        _lib.call("ivit_gemm_i8_requant_residual_i16_ex", g.a.ptr, g.a.ld, *w, p(g.db), *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, lay, st())
        fenced.check(o, exp)
    _, _, exp16 = g.residual(16, k=g.k16, res=res)
    o = fout(M, N, N + 24, np.int16, exp16)
    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", g.a.ptr, g.a.ld, p(_pack(g, 8)), K, p(g.db), *g.me16, r.ptr, r.ld, *sc, o.ptr, o.ld,
              M, N, K, 8, st())
    fenced.check(o, exp16)
    fenced.check(r)
    g.check_inputs()


def test_gemm_large_kernels_int8_strided_weight_and_output_map():
    """the persistent kernel's row-major weight with ldw = K + 64 (requant and residual, ldo = N + 16), and the output map of
    ivit_gemm_i8_requant_lut_ex with ldo = N + 16"""
    M, N, K = 2125, 192, 192
    g = Gemm(M, N, K, K + 16, K + 64, 21)
    o = fout(M, N, N + 16, np.int8, g.k8)
    _lib.call("ivit_gemm_i8_requant_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, g.k8)
    res, sc, exp = g.residual(8)
    r = fin(res, N + 32)
    o = fout(M, N, N + 16, np.int8, exp)
    _lib.call("ivit_gemm_i8_requant_residual_ex", *g.head, *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 0, st())
    fenced.check(o, exp)
    lut = g.rng.integers(-128, 128, size=256).astype(np.int8)
    expl = lut[g.k8 + 128]
    o = fout(M, N, N + 16, np.int8, expl)
    _lib.call("ivit_gemm_i8_requant_lut_ex", g.a.ptr, g.a.ld, p(_pack(g, 8)), K, p(g.db), *g.me, p(dev(lut)), o.ptr, o.ld, M, N, K, 8, st())
    fenced.check(o, expl)
    fenced.check(r)
    g.check_inputs()


# =========================================================================================== layout passes
def _frag_layout_host(W):
    """include/ivit_hip.h IVIT_W_FRAGS, by its documented formula; channels padded with zero rows to a multiple of 64"""
    N, K = W.shape
    out = np.zeros((N + 63) // 64 * 64 * K, np.int8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    off = ((n // 64) * (K // 64) + k // 64) * 4096 + (((n // 32) % 2 * 2 + (k // 32) % 2) * 2 + (k // 16) % 2) * 512 + (n % 32) * 16 + k % 16
    out[off.reshape(-1)] = W.reshape(-1)
    return out


def _frag16_layout_host(W):
    N, K = W.shape
    out = np.zeros((N + 63) // 64 * 64 * K, np.int8)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    off = ((n // 64) * (K // 64) + k // 64) * 4096 + ((n // 16) % 4) * 1024 + ((k // 16) % 4) * 256 + (n % 16) * 16 + k % 16
    out[off.reshape(-1)] = W.reshape(-1)
    return out


def test_pack_weight_frags_from_strided_rows():
    """ivit_pack_weight_frags_i8 / _frags16_i8 from ldw = K + 32, N = 200: the documented layout of the dense matrix byte for byte,
    channels 200 .. 255 zero, nothing behind 256 * K"""
    N, K = 200, 192
    W = np.random.default_rng(8).integers(-128, 127, size=(N, K)).astype(np.int8)
    w = fin(W, K + 32, 127)
    for fr, host in ((8, _frag_layout_host), (16, _frag16_layout_host)):
        exp = host(W).reshape(256, K)
        assert not exp.reshape(-1)[host(np.ones((N, K), np.int8)) == 0].any()
        o = fout(256, K, K, np.int8, exp)
        if fr == 8:
            _lib.call("ivit_pack_weight_frags_i8", w.ptr, w.ld, N, K, o.ptr, st())
        else:
            _lib.call("ivit_pack_weight_frags16_i8", w.ptr, w.ld, N, K, o.ptr, st())
        fenced.check(o, exp)
    fenced.check(w)


def test_tile_and_untile_strided_rows():
    """ivit_tile_operand_i8 from ld = K + 16 (37 rows: the last block is partly padding) and ivit_untile_operand_i8 into ld = K + 48:
    the pad columns stay untouched and the round trip is the source"""
    rows, K = 37, 192
    X = np.random.default_rng(9).integers(-128, 127, size=(rows, K)).astype(np.int8)
    x = fin(X, K + 16, 127)
    t = fout(rows, K, K, np.int8, X, blocks=True)
    _lib.call("ivit_tile_operand_i8", x.ptr, x.ld, rows, K, t.ptr, st())
    fenced.check(t, X)
    u = fout(rows, K, K + 48, np.int8, X)
    _lib.call("ivit_untile_operand_i8", t.ptr, rows, K, u.ptr, u.ld, st())
    fenced.check(u, X)
    fenced.check(x)


# =========================================================================================== window attention (smallest window)
def test_window_attention_natural_scale_forms_strided_output():
    """ivit_window_attention_i8_compat and _band at the smallest window (2 x 2 tokens, 1 head), ldo = 32 + 8 (the entry wants
    ldo % 8 == 0); the existing tests of the two pass the bare width"""
    import test_gpu_swin as ts
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
    S = np.einsum("bhqd,bhkd->bhqk", qkv[0].astype(np.int64), qkv[1].astype(np.int64)).astype(np.int32)
    kS = orc.requant(S.reshape(-1, N), omS[0], omS[1], 8).reshape(B_, nH, N, N)
    lin = orc.requant(kS.reshape(-1, N), omB[0], omB[1], 32).reshape(B_, nH, N, N)
    kA = np.clip(lin + bias_add[None].astype(np.int32), -128, 127).astype(f32)
    Pm = orc.shiftmax_xint((((kA * s_at).astype(f32)) / s_at).astype(f32), s_at)
    O = np.einsum("bhqk,bhkd->bqhd", Pm.astype(np.int64), qkv[2].astype(np.int64)).astype(np.int32)
    exp = orc.requant(O.reshape(-1, hd), omO[0], omO[1], 8).reshape(B_ * N, nH * hd)
    assert Pm.max() > 0 and np.abs(exp).max() > 0
    qv = np.arange(-128, 128, dtype=f32)
    phi = ((qv * s_at).astype(f32) / s_at).astype(f32)
    phim = ((((qv * s_at).astype(f32) + f32(-100.0)).astype(f32)) / s_at).astype(f32)
    ld = nH * hd + 8
    dq, db = dev(qkv), dev(bias_pad)
    o = fout(B_ * N, nH * hd, ld, np.int8, exp)
    _lib.call("ivit_window_attention_i8_compat", p(dq), o.ptr, o.ld, p(db), None, -1, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1],
              float(s_at), mo[0], mo[1], p(dev(phi)), p(dev(phim)), st())
    fenced.check(o, exp)
    band, bw = window_shiftexp_band(s_at, False)
    assert band is not None
    o = fout(B_ * N, nH * hd, ld, np.int8, exp)
    _lib.call("ivit_window_attention_i8_band", p(dq), o.ptr, o.ld, p(db), None, B_, nW, nH, N, hd, ms[0], ms[1], mb[0], mb[1], float(s_at),
              mo[0], mo[1], p(dev(band)), bw, band.shape[0], 0, 0, 0, 0, st())
    fenced.check(o, exp)


def test_window_attention_long_strided_output():
    """ivit_window_attention_i8_long (65 .. 144 tokens: its smallest square window, 9 x 9, 1 head, 1 window), ldo = 32 + 8"""
    import test_gpu_swin_384 as w
    ws, B_, nW, nH = 9, 1, 1, 1
    qkv, s_at, me, bias_add, bias_pad, region = w._setup(ws, B_, nW, nH, 0.25, False, False, 9001)
    N, hd = ws * ws, 32
    exp = w._pv(qkv, orc.shiftmax(w._scores(qkv, me, bias_add), s_at), me).reshape(B_ * N, nH * hd)
    o = fout(B_ * N, nH * hd, nH * hd + 8, np.int8, exp)
    _lib.call("ivit_window_attention_i8_long", p(dev(qkv)), o.ptr, o.ld, p(dev(bias_pad)), None, 0, B_, nW, nH, N, hd, me["ms"][0], me["ms"][1],
              me["mb"][0], me["mb"][1], float(s_at), me["mo"][0], me["mo"][1], None, None, None, 0, 0, ws, ws, ws, 0, 0, st())
    fenced.check(o, exp)


def test_window_attention_ibert_strided_output():
    """ivit_window_attention_i8_ibert at 2 x 2 tokens, 1 head, ldo = 32 + 8"""
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
    o = fout(nwin * N, nH * HEAD_DIM, nH * HEAD_DIM + 8, np.int8, exp)
    _lib.call("ivit_window_attention_i8_ibert", p(dev(qkv)), o.ptr, o.ld, p(a["bias"]), p(a["region"]), a["masked_exp"], nwin, nW, nH, N,
              HEAD_DIM, *a["ms"], *a["mb"], *a["mo"], p(a["table"]), a["band_w"], 2, 2, 2, 0, 0, st())
    fenced.check(o, exp)


# =========================================================================================== refusals
def _refusal_cases():
    """(id, entry, match, args(builder)) -- every strided entry above, and the six window-attention entries, with ld < width, ld off
    its alignment, and a block layout with ld != width; `b` hands out small device buffers, b.s the sentinel buffer every output pointer points into"""
    C, K, N, M = 64, 64, 64, 16
    c = []

    def add(cid, name, match, f):
        c.append(pytest.param(name, match, f, id=f"{name}-{cid}"))
    ln8 = lambda b, ldx, ldo, blocks=0: (b.x, ldx, M, C, b.f, b.f, b.i, b.i, b.s, ldo)      # noqa: E731
    for name, tail in (("ivit_layernorm_i8", ()), ("ivit_layernorm_i8_ex", (0,))):
        add("ldx<C", name, "rows must be 4-byte aligned", lambda b, tail=tail: (*ln8(b, C - 4, C), *tail, b.st))
        add("ldo<C", name, "rows must be 4-byte aligned", lambda b, tail=tail: (*ln8(b, C, C - 4), *tail, b.st))
        add("ldx%4", name, "rows must be 4-byte aligned", lambda b, tail=tail: (*ln8(b, C + 2, C), *tail, b.st))
        add("ldo%4", name, "rows must be 4-byte aligned", lambda b, tail=tail: (*ln8(b, C, C + 2), *tail, b.st))
    add("blocks-ldo!=C", "ivit_layernorm_i8_ex", "block-layout output needs", lambda b: (*ln8(b, C, C + 16), 1, b.st))
    lnc = lambda b, ldx, ldo, flags: (b.x, ldx, M, C, b.f, b.f, b.i, b.i, b.x, b.f, b.s, ldo, flags, b.st)      # noqa: E731
    add("ldx<C", "ivit_layernorm_i8_compat", "rows must be 4-byte aligned", lambda b: lnc(b, C - 4, C, 0))
    add("ldo%4", "ivit_layernorm_i8_compat", "rows must be 4-byte aligned", lambda b: lnc(b, C, C + 2, 0))
    add("blocks-ldo!=C", "ivit_layernorm_i8_compat", "block-layout output needs", lambda b: lnc(b, C, C + 16, 1))
    add("ldx<C", "ivit_layernorm_i32_f32", "bad shape", lambda b: (b.x, C - 1, M, C, b.f, b.f, b.s, C, b.st))
    add("ldo<C", "ivit_layernorm_i32_f32", "bad shape", lambda b: (b.x, C, M, C, b.f, b.f, b.s, C - 1, b.st))
    add("ldo<C", "ivit_layernorm_i16_i8", "bad operand", lambda b: (b.x, M, C, b.f, b.f, b.i, b.i, b.s, C - 1, 0, 0, 0, 0, b.st))
    add("ldo<C", "ivit_layernorm_i16_i8_compat", "bad operand", lambda b: (b.x, M, C, 0.001, 0, b.f, b.f, b.i, b.i, b.s, C - 1, 0, 0, 0, 0, b.st))
    ib = lambda b, ldx, ldo: (b.x, ldx, M, C, 0.0625, b.f, b.f, 1.0, b.i, b.i, b.s, ldo)      # noqa: E731
    for name, tail in (("ivit_ibert_layernorm_i8", (0,)), ("ivit_ibert_layernorm_i16_i8", ()), ("ivit_ibert_layernorm_i16_i8_ex", (0,))):
        add("ldx<C", name, "bad operand", lambda b, tail=tail: (*ib(b, C - 1, C), *tail, b.st))
        add("ldo<C", name, "bad operand", lambda b, tail=tail: (*ib(b, C, C - 1), *tail, b.st))
    add("blocks-ldo!=C", "ivit_ibert_layernorm_i8", "block-layout output needs", lambda b: (*ib(b, C, C + 16), 1, b.st))
    add("ldx<L", "ivit_shiftgelu_i8", "bad operand", lambda b: (b.x, C - 1, M, C, 0.0625, 1 << 30, 40, b.s, C, b.st))
    add("ldo<L", "ivit_shiftgelu_i8", "bad operand", lambda b: (b.x, C, M, C, 0.0625, 1 << 30, 40, b.s, C - 1, b.st))
    add("ldx<L", "ivit_shiftgelu_i8_i32", "bad operand", lambda b: (b.x, C - 1, M, C, 0.0625, b.s, C, b.st))
    add("ldo<L", "ivit_shiftgelu_i8_i32", "bad operand", lambda b: (b.x, C, M, C, 0.0625, b.s, C - 1, b.st))
    gl = lambda b, ldx, ldo: (b.x, ldx, M, C, b.x, b.s, ldo)      # noqa: E731
    for name, tail in (("ivit_shiftgelu_lut_i8", ()), ("ivit_shiftgelu_lut_i8_ex", (0,))):
        add("ldx<L", name, "4-byte aligned rows", lambda b, tail=tail: (*gl(b, C - 4, C), *tail, b.st))
        add("ldo<L", name, "4-byte aligned rows", lambda b, tail=tail: (*gl(b, C, C - 4), *tail, b.st))
        add("ldx%4", name, "4-byte aligned rows", lambda b, tail=tail: (*gl(b, C + 2, C), *tail, b.st))
        add("ldo%4", name, "4-byte aligned rows", lambda b, tail=tail: (*gl(b, C, C + 2), *tail, b.st))
    add("blocks-ldo!=L", "ivit_shiftgelu_lut_i8_ex", "block-layout output needs", lambda b: (*gl(b, C, C + 16), 1, b.st))
    add("blocks-ldx!=L", "ivit_shiftgelu_lut_i8_ex", "bad layouts", lambda b: (*gl(b, C + 16, C), 2, b.st))
    add("in-place-ldx!=ldo", "ivit_shiftgelu_lut_i8_ex", "in place .* needs ldx == ldo", lambda b: (b.s, C + 16, M, C, b.x, b.s, C + 32, 0, b.st))
    # GEMMs: (A, lda, W, ldw, bias, m, e | ... | out, ldo, M, N, K)
    gh = lambda b, lda=K, ldw=K: (b.x, lda, b.x, ldw, b.i)      # noqa: E731
    rq = lambda b, lda=K, ldw=K, ldo=N: (*gh(b, lda, ldw), b.i, b.i, b.s, ldo, M, N, K)      # noqa: E731
    for name, tail in (("ivit_gemm_i8_requant", ()), ("ivit_gemm_i8_requant_ex", (0,))):
        add("lda<K", name, "must be >= K and multiples of 16", lambda b, tail=tail: (*rq(b, lda=K - 16), *tail, b.st))
        add("ldw%16", name, "must be >= K and multiples of 16", lambda b, tail=tail: (*rq(b, ldw=K + 8), *tail, b.st))
        add("ldo<N", name, "must be >= N and a multiple of 16", lambda b, tail=tail: (*rq(b, ldo=N - 16), *tail, b.st))
        add("ldo%16", name, "must be >= N and a multiple of 16", lambda b, tail=tail: (*rq(b, ldo=N + 8), *tail, b.st))
    big = lambda b, lda=K, ldw=K, ldo=128: (*gh(b, lda, ldw), b.i, b.i, b.s, ldo, 2048, 128, K)      # noqa: E731
    add("blocks-lda!=K", "ivit_gemm_i8_requant_ex", "block-layout A operand is dense", lambda b: (*big(b, lda=K + 16), 1, b.st))
    add("blocks-ldw!=K", "ivit_gemm_i8_requant_ex", "block-layout W operand is dense", lambda b: (*big(b, ldw=K + 16), 2, b.st))
    add("blocks-ldo!=N", "ivit_gemm_i8_requant_ex", "ldo == N", lambda b: (*big(b, ldo=128 + 16), 4, b.st))
    add("ldo%16", "ivit_gemm_i8_requant_lut_ex", "must be >= N and a multiple of 16",
        lambda b: (*gh(b, 192, 192), b.i, b.i, b.x, b.s, 128 + 8, 2048, 128, 192, 8, b.st))
    rs = lambda b, ldr=N, ldo=N: (*gh(b), b.i, b.i, b.x, ldr, 1 << 30, 31, 1 << 30, 31, b.s, ldo, M, N, K)      # noqa: E731
    for name, tail in (("ivit_gemm_i8_requant_residual", ()), ("ivit_gemm_i8_requant_residual_ex", (0,))):
        add("ldr<N", name, "residual operand missing or misaligned", lambda b, tail=tail: (*rs(b, ldr=N - 16), *tail, b.st))
        add("ldr%16", name, "residual operand missing or misaligned", lambda b, tail=tail: (*rs(b, ldr=N + 8), *tail, b.st))
        add("ldo%16", name, "must be >= N and a multiple of 16", lambda b, tail=tail: (*rs(b, ldo=N + 8), *tail, b.st))
    for name, tail in (("ivit_gemm_i8_requant_residual_i16", ()), ("ivit_gemm_i8_requant_residual_i16_ex", (0,)),
                       ("ivit_gemm_i8_requant_i16_residual_i16_ex", (0,))):
        add("ldr<N", name, "16-bit .*rows must be 16-byte aligned", lambda b, tail=tail: (*rs(b, ldr=N - 8), *tail, b.st))
        add("ldr%8", name, "16-bit .*rows must be 16-byte aligned", lambda b, tail=tail: (*rs(b, ldr=N + 4), *tail, b.st))
        add("ldo%8", name, "16-bit .*rows must be 16-byte aligned", lambda b, tail=tail: (*rs(b, ldo=N + 4), *tail, b.st))
    add("ldo<N", "ivit_gemm_i8_requant_i16", "must be multiples of 4", lambda b: (*rq(b, ldo=N - 4), b.st))
    add("ldo%4", "ivit_gemm_i8_requant_i16", "must be multiples of 4", lambda b: (*rq(b, ldo=N + 2), b.st))
    add("ldo<N", "ivit_gemm_i8_i32", "must be multiples of 4", lambda b: (*gh(b), b.s, N - 4, M, N, K, b.st))
    add("ldo%4", "ivit_gemm_i8_i32", "must be multiples of 4", lambda b: (*gh(b), b.s, N + 2, M, N, K, b.st))
    qk = lambda b, lda=K, ldw=K: (*gh(b, lda, ldw), b.i, b.i, b.s, 4, 1, 16)      # noqa: E731   tokens 4, 1 head of 16
    add("lda<K", "ivit_gemm_i8_requant_qkv", "must be >= K and multiples of 16", lambda b: (*qk(b, lda=K - 16), M, 48, K, b.st))
    add("ldw%16", "ivit_gemm_i8_requant_qkv_ex", "must be >= K and multiples of 16", lambda b: (*qk(b, ldw=K + 8), M, 48, K, 0, b.st))
    add("lda%16", "ivit_gemm_i8_requant_qkv_planes_ex", "must be >= K and multiples of 16", lambda b: (*qk(b, lda=K + 8), 1, 2, M, 32, K, 0, b.st))
    for name in ("ivit_pack_weight_frags_i8", "ivit_pack_weight_frags16_i8"):
        add("ldw<K", name, "bad operand", lambda b: (b.x, K - 16, N, K, b.s, b.st))
        add("ldw%16", name, "bad operand", lambda b: (b.x, K + 8, N, K, b.s, b.st))
    add("ldo<C", "ivit_layernorm_i8_compat", "rows must be 4-byte aligned", lambda b: lnc(b, C, C - 4, 0))
    add("ldx%4", "ivit_layernorm_i8_compat", "rows must be 4-byte aligned", lambda b: lnc(b, C + 2, C, 0))
    lt = lambda b, lda=192, ldo=128: (*gh(b, lda, 192), b.i, b.i, b.x, b.s, ldo, 2048, 128, 192, 8, b.st)      # noqa: E731
    add("lda<K", "ivit_gemm_i8_requant_lut_ex", "must be >= K and multiples of 16", lambda b: lt(b, lda=176))
    add("ldo<N", "ivit_gemm_i8_requant_lut_ex", "must be >= N and a multiple of 16", lambda b: lt(b, ldo=112))
    add("blocks-lda!=K", "ivit_gemm_i8_requant_residual_ex", "block-layout A operand is dense",
        lambda b: (*gh(b, K + 16, K), b.i, b.i, b.x, 128, 1 << 30, 31, 1 << 30, 31, b.s, 128, 2048, 128, K, 1, b.st))
    add("ldw%16", "ivit_gemm_i8_requant_qkv", "must be >= K and multiples of 16", lambda b: (*qk(b, ldw=K + 8), M, 48, K, b.st))
    add("lda<K", "ivit_gemm_i8_requant_qkv_ex", "must be >= K and multiples of 16", lambda b: (*qk(b, lda=K - 16), M, 48, K, 0, b.st))
    add("ldw<K", "ivit_gemm_i8_requant_qkv_planes_ex", "must be >= K and multiples of 16", lambda b: (*qk(b, ldw=K - 16), 1, 2, M, 32, K, 0, b.st))
    # window attention: one window of 2 x 2 (9 x 9 for the long entry) tokens, one head of 32; ldo >= 32 and a multiple of 8
    rq3 = (1 << 30, 40, 1 << 30, 31)
    wa = {"ivit_window_attention_i8": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 0, 1, 1, 1, 4, 32, *rq3, 0.25, 1 << 30, 40, b.st),
          "ivit_window_attention_i8_compat": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 0, 1, 1, 1, 4, 32, *rq3, 0.25, 1 << 30, 40, b.f, b.f, b.st),
          "ivit_window_attention_i8_band": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 1, 1, 1, 4, 32, *rq3, 0.25, 1 << 30, 40, b.i, 16, 256,
                                                           0, 0, 0, 0, b.st),
          "ivit_window_attention_i8_unwindow": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 0, 1, 1, 1, 4, 32, *rq3, 0.25, 1 << 30, 40, None, None,
                                                               2, 2, 2, 0, b.st),
          "ivit_window_attention_i8_long": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 0, 1, 1, 1, 81, 32, *rq3, 0.25, 1 << 30, 40, None, None,
                                                           None, 0, 0, 9, 9, 9, 0, 0, b.st),
          "ivit_window_attention_i8_ibert": lambda b, ldo: (b.x, b.s, ldo, b.x, None, 0.0, 1, 1, 1, 4, 32, *rq3, 1 << 30, 40, b.f, 0,
                                                            2, 2, 2, 0, 0, b.st)}
    for name, f in wa.items():
        add("ldo<width", name, "misaligned operand or ldo too small", lambda b, f=f: f(b, 24))
        add("ldo%8", name, "misaligned operand or ldo too small", lambda b, f=f: f(b, 36))
    add("ld<K", "ivit_tile_operand_i8", "bad operand", lambda b: (b.x, K - 16, M, K, b.s, b.st))
    add("ld%16", "ivit_tile_operand_i8", "bad operand", lambda b: (b.x, K + 8, M, K, b.s, b.st))
    add("ld<K", "ivit_untile_operand_i8", "bad operand", lambda b: (b.x, M, K, b.s, K - 16, b.st))
    add("ld%16", "ivit_untile_operand_i8", "bad operand", lambda b: (b.x, M, K, b.s, K + 8, b.st))
    return c


class _Bufs:
    """operands of a refused call: zeros of every kind (never read: the entry returns before any launch) and the sentinel buffer"""

    def __init__(self):
        self.x = p(dev(np.zeros(1 << 16, np.int8)))
        self.f = p(dev(np.zeros(4096, f32)))
        self.i = p(dev(np.zeros(4096, np.int32)))
        self.sent = torch.full((1 << 16,), 0x5A, dtype=torch.int8, device=DEV)
        _KEEP.append(self.sent)
        self.s = p(self.sent)
        self.st = st()


@pytest.mark.parametrize("name,match,build", _refusal_cases())
def test_bad_leading_dimensions_are_refused(name, match, build):
    """IVIT_ERR_INVALID with the entry's documented message; the buffer every output pointer points into keeps its sentinel"""
    b = _Bufs()
    refused(match, name, *build(b))
    torch.cuda.synchronize()
    assert bool((b.sent == 0x5A).all()), f"{name}: a refused call wrote to its output"
