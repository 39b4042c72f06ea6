"""The launcher conditions that guard the 32-bit fast paths, one case on each side of each bound, with real buffers of the full size
(tests/far.py with zones=False: the same guards and the same whole-allocation check, the leading dimension set by the bound).
Expectations are the oracle's, bit for bit, and the same on both sides of a bound that only selects another kernel.

Which kernel each case reaches, from the launcher's own condition:
  int8 LayerNorm, rows = 15 627, C = 768 (csrc/ln_stream.h): ln_stream_pays holds (rows * C >= 12 000 000); ln_stream_takes wants
    rows * ldx < 2^31 and (rows + 15) * ldo < 2^31.  The largest multiple of 16 that satisfies one of them streams, with x_bytes
    (o_bytes) just below 2^31; 16 more and the launcher falls back to the register kernel (v2), also under lab form 4.
  skinny-K GEMM, M = 8197, N = 96 (csrc/gemm.hip launch_gemm): admitted while M * ldo < 2^32 (its row-major stores are 64-bit, (int64_t)t * ldo; only its head-major offsets are 32-bit), so its stores reach
    [2^31, 2^32); 16 more and gemm_i8_kernel takes the call (N = 96 is below the persistent kernel's 128 channels).  No condition mentions M * lda: the A rows are addressed in 64
    bits, shown with a far lda.
  IVIT_W_FRAGS16, M = 2125, N = K = 192: (M + 16) * ldo < 2^32 and (M + 16) * ldr < 2^32 or IVIT_ERR_INVALID; IVIT_W_FRAGS (the
    32x32x32 form) has no bound and runs beyond 2^32 (test_gpu_far_rows.py has its other operands).
  head-major q/k/v outputs: M * N < 2^31 (planes form: 3 * M * heads * head_dim) or IVIT_ERR_INVALID; just below, the skinny-K form.
  patchify: the 32-bit index chain below 2^31 groups of four pixels, the 64-bit chain from there; float pixels on both sides.
  block-layout outputs: (rows + 15) * C < 2^31 or IVIT_ERR_INVALID, before anything is launched; just below it at C = 768 the
    streaming LayerNorm kernel.
What the fall-back pairs (LayerNorm, skinny-K) cannot show: both sides expect the same bytes and no hook reports which kernel ran,
so they hold both kernels to the oracle on either side of the bound but would also pass with the bound itself misplaced; the bound's
value is pinned only where crossing it is a refusal (IVIT_W_FRAGS16, q/k/v, block layout)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import phi_tables  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import test_gpu_strides as S  # noqa: E402
from test_gpu_far_rows import far_in, room  # noqa: E402

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


def at_bound(rows, ld, width, dtype=np.int8, expected=None, data=None, poison=127):
    """an operand whose leading dimension a bound sets: far.py's layout, whatever zones its rows reach"""
    room(far.need_bytes(rows, ld, np.dtype(dtype).itemsize))
    if data is not None:
        return far.input(data, ld, poison, device=DEV, zones=False)
    return far.output(rows, width, ld, dtype, expected=expected, device=DEV, zones=False)


def largest_ld(bound, factor, multiple=16):
    """the largest multiple of `multiple` with factor * ld < bound"""
    return (bound - 1) // factor // multiple * multiple


# =========================================================================================== streaming int8 LayerNorm
LN_ROWS, LN_C = 15627, 768


@functools.lru_cache(maxsize=None)
def ln_stream_case(compat):
    """the rows of test_layernorm_i8_streaming_threshold (and their natural-scale twin): computed once for all sides and forms"""
    rows, C = LN_ROWS, LN_C
    assert rows * C >= 12_000_000
    if compat:
        q, s, gamma, beta, s_out, exp, lay = S.ln8_compat_case(C, rows=rows)
        return q, gamma, beta, s_out, exp, S.ln_oracle(gamma, beta, s_out, lay), phi_tables(s)
    rng = np.random.default_rng(rows)
    k = np.clip(np.rint(rng.normal(rng.normal(0, 10, size=(rows, 1)), rng.uniform(1, 50, size=(rows, 1)), size=(rows, C))), -128, 127).astype(np.int8)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    y, s_ln, _ = orc.layernorm(k.astype(np.int32), gamma, beta)
    s_out = f32(2.0 ** np.ceil(np.log2(np.abs(y * s_ln).max() / 127 * 0.8)))
    orac = S.ln_oracle(gamma, beta, s_out)
    return k, gamma, beta, s_out, orac(k), orac, None


@pytest.fixture(params=[0, 4], ids=["product", "lab_streaming"])
def ln_form(request):
    if request.param == 0:
        yield 0
        return
    with _lib.lab_session():
        _lib.call("ivit_debug_ln_wave_per_row", request.param)
        yield request.param


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("operand", ["ldx", "ldo"])
@pytest.mark.parametrize("compat", [False, True], ids=["ex", "compat"])
def test_layernorm_i8_streaming_bound(compat, operand, side, ln_form):
    """ivit_layernorm_i8_ex / _compat on both sides of rows * ldx < 2^31 and of (rows + 15) * ldo < 2^31: the same bytes"""
    rows, C = LN_ROWS, LN_C
    k, gamma, beta, s_out, exp, orac, tabs = ln_stream_case(compat)
    ldx, ldo = 784, 800
    if operand == "ldx":
        ldx = largest_ld(2 ** 31, rows) + (16 if side == "at" else 0)
        assert (rows * ldx < 2 ** 31) == (side == "below") and rows * (ldx - 16) < 2 ** 31 <= rows * (ldx + 16) and ldx % 16 == 0
        x = at_bound(rows, ldx, C, data=k)
        o = S.fout(rows, C, ldo, np.int8, exp)
    else:
        ldo = largest_ld(2 ** 31, rows + 15) + (16 if side == "at" else 0)
        assert ((rows + 15) * ldo < 2 ** 31) == (side == "below") and (rows + 15) * (ldo - 16) < 2 ** 31 <= (rows + 15) * (ldo + 16)
        x = S.fin(k, ldx, 127)
        o = at_bound(rows, ldo, C, expected=exp)
    fenced.poison_effective(k[:64], 127, orac, exp[:64])
    t = S.Tables(gamma, beta, s_out)
    if compat:
        _lib.call("ivit_layernorm_i8_compat", x.ptr, x.ld, rows, C, *t.args, p(dev(tabs[0])), p(dev(tabs[1])), o.ptr, o.ld, 0, st())
    else:
        _lib.call("ivit_layernorm_i8_ex", x.ptr, x.ld, rows, C, *t.args, o.ptr, o.ld, 0, st())
    far.check(o, exp) if operand == "ldo" else fenced.check(o, exp)
    if operand == "ldx":
        far.check(x)


# =========================================================================================== skinny-K GEMM
@pytest.mark.parametrize("case", ["ldo_below", "ldo_at", "lda_far"])
@pytest.mark.parametrize("K", [64, 128])
def test_gemm_skinny_k_output_bound_and_far_a(K, case):
    """ivit_gemm_i8_requant_ex, M = 8197, N = 96: M * ldo just below 2^32 (the skinny kernel stores beyond 2^31),
    at 2^32 (gemm_i8_kernel), and A with rows beyond 2^32 bytes (still the skinny kernel)"""
    M, N = 8197, 96
    g = S.Gemm(M, N, K, K + 16, K + 16, 10 + K)
    if case == "lda_far":
        g.a = far_in(g.A, 16, 0, 127)
        o = S.fout(M, N, N + 16, np.int8, g.k8)
    else:
        ldo = largest_ld(2 ** 32, M) + (16 if case == "ldo_at" else 0)
        assert (M * ldo < 2 ** 32) == (case == "ldo_below") and M * (ldo - 16) < 2 ** 32 <= M * (ldo + 16) and (M - 1) * ldo > 2 ** 31
        o = at_bound(M, ldo, N, expected=g.k8)
    _lib.call("ivit_gemm_i8_requant_ex", *g.head, *g.me, o.ptr, o.ld, M, N, K, 0, st())
    far.check(o, g.k8) if isinstance(o, far.Buffer) else fenced.check(o, g.k8)
    far.check(g.a) if isinstance(g.a, far.Buffer) else fenced.check(g.a)
    fenced.check(g.w)


# =========================================================================================== IVIT_W_FRAGS16
FR16_MSG = "IVIT_W_FRAGS16 addresses its output .and residual. with 32-bit offsets"


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("epi,operand", [("requant", "ldo"), ("residual", "ldo"), ("residual", "ldr")])
def test_gemm_frags16_offset_bound(epi, operand, side):
    """(M + 16) * ldo < 2^32 and (M + 16) * ldr < 2^32: runs below (the last rows' offsets beyond 2^31), refused at the bound with
    IVIT_ERR_INVALID; the refused call's output keeps its sentinel"""
    M, N, K = 2125, 192, 192
    g = S.Gemm(M, N, K, K + 16, K + 64, 30)
    Wf = S._pack(g, 16)
    ld = largest_ld(2 ** 32, M + 16) + (16 if side == "at" else 0)
    assert ((M + 16) * ld < 2 ** 32) == (side == "below") and (M + 16) * (ld - 16) < 2 ** 32 <= (M + 16) * (ld + 16) and (M - 1) * ld > 2 ** 31
    res, sc, exp_r = g.residual(8)
    exp = g.k8 if epi == "requant" else exp_r
    o = at_bound(M, ld, N, expected=exp) if operand == "ldo" else S.fout(M, N, N + 16, np.int8, exp)
    r = at_bound(M, ld, N, data=res) if operand == "ldr" else S.fin(res, N + 32)
    if epi == "requant":
        args = ("ivit_gemm_i8_requant_ex", g.a.ptr, g.a.ld, p(Wf), K, p(g.db), *g.me, o.ptr, o.ld, M, N, K, 16, st())
    else:
        args = ("ivit_gemm_i8_requant_residual_ex", g.a.ptr, g.a.ld, p(Wf), K, p(g.db), *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 16, st())
    if side == "below":
        _lib.call(*args)
        far.check(o, exp) if operand == "ldo" else fenced.check(o, exp)
    else:
        S.refused(FR16_MSG, *args)
        if operand == "ldo":
            far.untouched(o)
        else:
            torch.cuda.synchronize()
            assert (o.fetch() == o.host).all(), "a refused call wrote to its output"
    if operand == "ldr":
        far.check(r)
    g.check_inputs()


@pytest.mark.parametrize("operand", ["ldo", "ldr"])
def test_gemm_frags_has_no_offset_bound(operand):
    """IVIT_W_FRAGS (32x32x32) beyond the bound of IVIT_W_FRAGS16, rows on both sides of 2^32: its epilogue addresses in 64 bits"""
    M, N, K = 2125, 192, 192
    g = S.Gemm(M, N, K, K + 16, K + 64, 30)
    Wf = S._pack(g, 8)
    ld = far.ld_for(M, 1, 16)
    assert (M + 16) * ld >= 2 ** 32 and (M - 2) * ld > 2 ** 32
    res, sc, exp = g.residual(8)
    o = at_bound(M, ld, N, expected=exp) if operand == "ldo" else S.fout(M, N, N + 16, np.int8, exp)
    r = at_bound(M, ld, N, data=res) if operand == "ldr" else S.fin(res, N + 32)
    _lib.call("ivit_gemm_i8_requant_residual_ex", g.a.ptr, g.a.ld, p(Wf), K, p(g.db), *g.me, r.ptr, r.ld, *sc, o.ptr, o.ld, M, N, K, 8, st())
    far.check(o, exp) if operand == "ldo" else fenced.check(o, exp)
    if operand == "ldr":
        far.check(r)
    g.check_inputs()


# =========================================================================================== head-major q/k/v outputs
QKV_T, QKV_HD, QKV_K = 2, 16, 64          # the smallest N the entries admit: 3 planes x 1 head x 16


@pytest.mark.parametrize("entry", ["qkv_ex", "qkv_planes_ex"])
def test_gemm_head_major_output_bound(entry):
    """ivit_gemm_i8_requant_qkv_ex (M * N < 2^31) and ivit_gemm_i8_requant_qkv_planes_ex (3 * M * heads * head_dim < 2^31), N = 48,
    K = 64, tokens = 2: M = 44 739 242 runs (M >= 8192, K = 64: the skinny-K form, whose head-major offsets are 32-bit), with a
    dense output one row short of 2 GiB; two rows more are refused, with real buffers of the full size, and leave them untouched.
    Expectations: the oracle on one period of 1021 rows of A; with one head, plane p of the output is the dense [M, 16] matrix
    of the channels 16 p .. 16 p + 15 in row order, so each plane is that period's, repeated"""
    from test_gpu_far_flat import Flat
    T, hd, K, N = QKV_T, QKV_HD, QKV_K, 3 * QKV_HD
    M = (2 ** 31 - 1) // N // T * T
    M_at = M + T
    assert M * N < 2 ** 31 <= M_at * N and M % T == 0 and M >= 8192
    rng = np.random.default_rng(48)
    Ab = rng.integers(-128, 127, size=(1021, K)).astype(np.int8)
    W = rng.integers(-128, 127, size=(N, K)).astype(np.int8)
    b = rng.integers(-50000, 50000, size=N).astype(np.int32)
    m, e = S.rand_me(rng, N, -16, -9)
    k8 = orc.requant(orc.gemm_i8(Ab, W, b), m.astype(np.float64), e, 8).astype(np.int8)
    a = Flat(M_at * K, np.int8, 127).tile(Ab.reshape(-1))
    o = Flat(M_at * N, np.int8, 85)
    w, db, dm, de = dev(W), dev(b), dev(m.view(np.int32)), dev(e)
    if entry == "qkv_ex":
        planes = (0, 1, 2)
        run = lambda rows: _lib.call("ivit_gemm_i8_requant_qkv_ex", a.ptr, K, p(w), K, p(db), p(dm), p(de), o.ptr, T, 1, hd, rows, N, K, 0, st())      # noqa: E731
        match = "exceeds the 2 GiB the 32-bit head-major offsets cover"
    else:
        planes = (1, 2)
        run = lambda rows: _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", a.ptr, K, p(w[hd:]), K, p(db[hd:]), p(dm[hd:]), p(de[hd:]), o.ptr,      # noqa: E731
                                     T, 1, hd, 1, 2, rows, 2 * hd, K, 0, st())
        match = "a q/k/v buffer beyond 2 GiB"
    with pytest.raises(_lib.IvitError, match=match) as ei:
        run(M_at)
    assert "(-1)" in str(ei.value)
    torch.cuda.synchronize()
    assert int((o.body != 85).sum()) == 0 and o.guards_hold(), "a refused call wrote to its output"
    run(M)
    torch.cuda.synchronize()
    for pl in range(3):
        plane = Flat.__new__(Flat)
        plane.n, plane.body = M * hd, o.body[pl * M * hd:(pl + 1) * M * hd]
        if pl in planes:
            bad, first = plane.mismatches(np.ascontiguousarray(k8[:, pl * hd:(pl + 1) * hd]).reshape(-1))
            assert bad == 0, f"plane {pl}: {bad} bytes differ, the first at row {first // hd}, column {first % hd}"
        else:
            assert int((plane.body != 85).sum()) == 0, f"plane {pl} is not selected and was written"
    assert int((o.body[3 * M * hd:] != 85).sum()) == 0 and o.guards_hold(), "bytes beyond the three planes were written"


# =========================================================================================== patchify
@pytest.mark.parametrize("B", [2730, 2731], ids=["below", "beyond"])
def test_patchify_hw_f32_on_both_sides_of_2_31_pixel_groups(B):
    """ivit_quantize_patchify_hw_f32_i8 with the shapes of test_gpu_rect.py::test_patchify_hw_u8_beyond_2_31_pixel_groups: B images
    of 3 x 512 x 2048 float pixels are 2^31 - 786 432 groups of four pixels at B = 2730 (the 32-bit index chain) and
    2^31 + 262 144 at B = 2731 (the 64-bit chain, which the float entry shares with the uint8 one): no product
    B * C * h * (w / 4) lies closer, 2^31 - 1 being prime.  34 GB in, 8.6 GB out; expected values by torch on the device, 32 images
    at a time: q = clamp(round(inv_scale * x)) (float32 product, ties to even), in im2col order"""
    C, h, w, patch = 3, 512, 2048, 16
    total = B * C * h * (w // 4)
    assert (total < 2 ** 31) == (B == 2730) and 2731 * C * h * (w // 4) >= 2 ** 31 > 2730 * C * h * (w // 4)
    room(B * C * h * w * 5 + 2 ** 32)
    inv = f32(1.0) / f32(0.0371)
    g = torch.Generator(device=DEV).manual_seed(B)
    img = torch.empty((B, C, h, w), dtype=torch.float32, device=DEV)
    for b0 in range(0, B, 256):
        img[b0:b0 + 256].normal_(0.0, 1.6, generator=g)
    K, gh, gw = C * patch * patch, h // patch, w // patch
    out = torch.full((B * gh * gw + 1, K), 85, dtype=torch.int8, device=DEV)
    _lib.call("ivit_quantize_patchify_hw_f32_i8", p(img), p(out), K, B, C, h, w, patch, float(inv), st())
    torch.cuda.synchronize()
    bad, seen = 0, 0
    for b0 in range(0, B, 32):
        b1 = min(B, b0 + 32)
        q = (img[b0:b1] * float(inv)).round_().clamp_(-128, 127).to(torch.int8)
        want = q.view(b1 - b0, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape((b1 - b0) * gh * gw, K)
        bad += int((out[b0 * gh * gw:b1 * gh * gw] != want).sum())
        seen += int((want == 127).sum()) + int((want == -128).sum())
    assert bad == 0, f"{bad} bytes differ"
    assert seen > 0 and bool((out[-1] == 85).all()) and bool((out[-2] != out[0]).any())


# =========================================================================================== block-layout outputs
def test_layernorm_i8_block_layout_just_below_2_gib():
    """ivit_layernorm_i8_ex, C = 768, out_blocks = 1, the most rows with (rows + 15) * C < 2^31: ln_stream_pays and ln_stream_takes
    hold (rows * ldx < 2^31 as well), so the streaming kernel runs with o_bytes just below 2^31 and block offsets up to it.
    Expectations: the oracle on a period of 1021 rows, repeated, at the documented block offsets"""
    from test_gpu_far_flat import Flat, blocks_mismatch
    C = 768
    rows = (2 ** 31 - 1) // C - 15
    assert (rows + 15) * C < 2 ** 31 <= (rows + 16) * C and rows * C >= 12_000_000
    rng = np.random.default_rng(49)
    kb = np.clip(np.rint(rng.normal(rng.normal(0, 10, size=(1021, 1)), rng.uniform(1, 50, size=(1021, 1)), size=(1021, C))), -128, 127).astype(np.int8)
    gamma = rng.uniform(0.5, 1.5, size=C).astype(f32)
    beta = rng.normal(0, 0.1, size=C).astype(f32)
    y, s_ln, _ = orc.layernorm(kb.astype(np.int32), gamma, beta)
    s_out = f32(2.0 ** np.ceil(np.log2(np.abs(y * s_ln).max() / 127 * 0.8)))
    exp = S.ln_oracle(gamma, beta, s_out)(kb).astype(np.int8)
    assert (exp.reshape(-1) != np.roll(exp.reshape(-1), -(2 ** 31 % exp.size))).mean() > 0.2
    t = S.Tables(gamma, beta, s_out)
    x = Flat(rows * C, np.int8, 127).tile(kb.reshape(-1))
    R16 = (rows + 15) // 16 * 16
    o = Flat(R16 * C, np.int8, 85)
    _lib.call("ivit_layernorm_i8_ex", x.ptr, C, rows, C, *t.args, o.ptr, C, 1, st())
    torch.cuda.synchronize()
    want = Flat(rows * C, np.int8, 85).tile(exp.reshape(-1))
    bad = blocks_mismatch(o.body, want.body, rows, C)
    assert bad == 0, f"{bad} bytes of the block-layout output differ"
    assert o.guards_hold()


def _block_refusals():
    """(entry, match, args(x, f, i, out, rows, C)): x / f / i are zeroed int8 / float32 / int32 operands of the full extent of a
    [rows, C] matrix (tables: of 4096 entries), out a real block-layout buffer: were the bound ever lost, the call would run on
    memory it owns"""
    blk = "block-layout output needs"
    c = [("ivit_layernorm_i8_ex", blk, lambda x, f, i, o, rows, C: (x, C, rows, C, f, f, i, i, o, C, 1)),
         ("ivit_layernorm_i8_compat", blk, lambda x, f, i, o, rows, C: (x, C, rows, C, f, f, i, i, x, f, o, C, 1)),
         ("ivit_ibert_layernorm_i8", blk, lambda x, f, i, o, rows, C: (x, C, rows, C, 0.0625, f, f, 1.0, i, i, o, C, 1)),
         ("ivit_shiftgelu_lut_i8_ex", blk, lambda x, f, i, o, rows, C: (x, C, rows, C, x, o, C, 1)),
         ("ivit_gemm_i8_requant_ex", "ldo == N", lambda x, f, i, o, rows, C: (x, 64, x, 64, i, i, i, o, C, rows, C, 64, 4)),
         ("ivit_gemm_i8_requant_lut_ex", "ldo == N", lambda x, f, i, o, rows, C: (x, 192, x, 192, i, i, i, x, o, C, rows, C, 192, 8 | 4))]
    return [pytest.param(*v, id=v[0]) for v in c]


@pytest.mark.parametrize("name,match,build", _block_refusals())
def test_block_layout_output_of_2_gib_is_refused(name, match, build):
    """(rows + 15) * C >= 2^31 at C = 128 -> IVIT_ERR_INVALID, nothing written"""
    from test_gpu_far_flat import Flat
    C = 128
    rows = -(-2 ** 31 // C) - 15
    assert (rows + 15) * C >= 2 ** 31 > (rows + 14) * C
    o = Flat((rows + 15) // 16 * 16 * C, np.int8, 85)
    x = torch.zeros(rows * 192, dtype=torch.int8, device=DEV)
    f = torch.zeros(4096, dtype=torch.float32, device=DEV)
    i = torch.zeros(4096, dtype=torch.int32, device=DEV)
    S.refused(match, name, *build(p(x), p(f), p(i), o.ptr, rows, C), st())
    torch.cuda.synchronize()
    assert int((o.body != 85).sum()) == 0 and o.guards_hold(), f"{name}: a refused call wrote to its output"


def _attention_block_refusals():
    rq = (1 << 30, 40)
    sm = lambda q, o, B, H, T, tab: (q, o, B, H, T, 64, *rq, 0.25, *rq)      # noqa: E731
    ib = lambda q, o, B, H, T, tab: (q, o, B, H, T, 64, *rq, *rq, tab, None, 0)      # noqa: E731
    c = [("ivit_attention_fused_i8_ex", 197, lambda *a: (*sm(*a), 1)),
         ("ivit_attention_fused_i8_compat", 197, lambda *a: (*sm(*a), None, 1)),
         ("ivit_attention_fused_i8_compat_band", 197, lambda *a: (*sm(*a), None, None, 0, 1)),
         ("ivit_attention_fused_i8_wide", 197, lambda *a: (*sm(*a), None, None, 0, 8, 1)),
         ("ivit_attention_fused_i8_long", 577, lambda *a: (*sm(*a), None, None, 0, 1)),
         ("ivit_attention_fused_i8_wide_long", 577, lambda *a: (*sm(*a), None, None, 0, 8, 1)),
         ("ivit_attention_fused_i8_ibert", 197, lambda *a: (*ib(*a), 1)),
         ("ivit_attention_fused_i8_ibert_wide", 197, lambda *a: (*ib(*a), 8, 1)),
         ("ivit_attention_fused_i8_ibert_long", 577, lambda *a: (*ib(*a), 1))]
    return [pytest.param(*v, id=v[0]) for v in c]


@pytest.mark.parametrize("name,T,build", _attention_block_refusals())
def test_attention_block_layout_output_of_2_gib_is_refused(name, T, build):
    """(batch * tokens + 15) * heads * 64 >= 2^31 with out_blocks = 1 -> IVIT_ERR_INVALID for every fused attention entry; qkv and
    the output are real buffers of the full size"""
    from test_gpu_far_flat import Flat
    H = 12
    B = -(-(-(-2 ** 31 // (H * 64)) - 15) // T)
    assert (B * T + 15) * H * 64 >= 2 ** 31 > ((B - 1) * T + 15) * H * 64
    room(4 * B * T * H * 64 + 2 ** 32)
    qkv = torch.zeros(3 * B * T * H * 64, dtype=torch.int8, device=DEV)
    tab = torch.zeros(65536, dtype=torch.float32, device=DEV)
    o = Flat((B * T + 15) // 16 * 16 * H * 64, np.int8, 85)
    S.refused("block-layout buffers stay below 2 GiB", name, *build(p(qkv), o.ptr, B, H, T, p(tab)), st())
    torch.cuda.synchronize()
    assert int((o.body != 85).sum()) == 0 and o.guards_hold(), f"{name}: a refused call wrote to its output"
