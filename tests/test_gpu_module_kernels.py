"""The module-level I-ViT kernels of the C ABI, each against the CPU oracle (or, for the element-wise ones, the one-line numpy
statement of the operation): the stand-alone Shiftmax family, the literal LayerNorm, the batched products behind QuantMatMul, the
embedding assembly and the element-wise pieces.  Shapes are chosen for what the whole-model vectors never reach: leading dimensions
larger than the row, row counts that are no multiple of a workgroup's four, inputs large enough for a second trip of the grid-stride
loops (the launchers cap their grids at 8192 / 4096 workgroups), the scalar tail of the vectorised quantiser, and the extremes the
launchers accept.  Every output buffer is pre-filled with a sentinel that must survive outside the written region; every refusal
asserted here is an IVIT_REQUIRE in front of the launch."""
import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

gpu = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
_KEEP = []  # device tensors whose raw pointers were handed to the C ABI stay alive until the test's final synchronize


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


def filled(shape, dtype, value):
    t = torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    if _KEEP:
        torch.cuda.synchronize()
        _KEEP.clear()


def st():
    return _lib.stream_ptr()


def fbits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def padded(a, ld, fill):
    """[rows, L] -> [rows, ld] with `fill` in the pad columns (values a kernel that read them would trip over)"""
    out = np.full((a.shape[0], ld), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


# =========================================================================================== Shiftmax family
SM_L = [2, 3, 49, 63, 64, 65, 144, 197, 577, 1024]
S_X0_MIN = f32(1.0 / 65534.5)       # floor(-1 / s) = -65535: the last scale the integer forms accept
SM_SCALES = [2.0 ** -p for p in range(7)] + [0.0437, 0.0571, float(S_X0_MIN)]


def x0_of(s):
    return float(np.floor((f32(1.0) / f32(s)) * f32(-1.0)))


def sm_rows(L, rows, seed, lo=-128, hi=127):
    """random scores plus the rows kernels go wrong on: flat, one-hot, all at the lower end, maximum in the last column, maximum
    repeated"""
    rng = np.random.default_rng(seed)
    k = np.clip(np.rint(rng.normal(0, 40, size=(rows, L))), lo, hi).astype(np.int32)
    k[0] = 7
    k[1] = lo
    k[1, L // 2] = hi
    k[2] = lo
    k[3] = rng.integers(lo, hi, size=L)
    k[3, L - 1] = hi
    k[4] = -3
    k[4, 0] = k[4, L - 1] = 60
    return k


def sm_mask(s, L):
    """Swin's shift mask on every other column: -100 / s, an integer at the power-of-two scales"""
    m = np.zeros(L, np.int32)
    m[1::2] = int(np.rint(-100.0 / float(s)))
    return m


def _shiftmax_int(name, k, s, ldx_pad=3, ldo_pad=5):
    rows, L = k.shape
    dt, fill = (np.int8, 127) if name == "ivit_shiftmax_i8" else (np.int32, 2 ** 27)
    out = filled((rows, L + ldo_pad), torch.int8, -99)
    args = (_lib.ptr(dev(padded(k.astype(dt), L + ldx_pad, fill))), L + ldx_pad, rows, L, float(s), _lib.ptr(out), L + ldo_pad, st())
    if name == "ivit_shiftmax_i8":
        _lib.call("ivit_shiftmax_i8", *args)
    else:
        _lib.call("ivit_shiftmax_i32_i8", *args)
    got = out.cpu().numpy()
    assert (got[:, L:] == -99).all(), "pad columns of the output were written"
    return got[:, :L].astype(np.int32)


def _shiftmax_f32(x, s, bit, ldx_pad=3, ldo_pad=5):
    rows, L = x.shape
    out = filled((rows, L + ldo_pad), torch.int8 if bit == 8 else torch.int16, -99)
    xp = _lib.ptr(dev(padded(x.astype(f32), L + ldx_pad, f32(3e38))))
    if bit == 8:
        _lib.call("ivit_shiftmax_f32_i8", xp, L + ldx_pad, rows, L, float(s), _lib.ptr(out), L + ldo_pad, st())
    else:
        _lib.call("ivit_shiftmax_f32_i16", xp, L + ldx_pad, rows, L, float(s), bit, _lib.ptr(out), L + ldo_pad, st())
    got = out.cpu().numpy()
    assert (got[:, L:] == -99).all(), "pad columns of the output were written"
    return got[:, :L].astype(np.int32)


@pytest.mark.parametrize("s", [1.0, 2.0 ** -2, 2.0 ** -4, 2.0 ** -6])
def test_the_two_shiftmax_references_agree_on_masked_scores(s):
    """CPU: orc.shiftmax on int32 scores and orc.shiftmax_xint on the same values as float32 are one function on the masked inputs
    used below, so the integer and the literal kernels are held to the same thing"""
    for L in (49, 144):
        k = sm_rows(L, 37, L) + sm_mask(s, L)
        for bit in (8, 16):
            assert np.array_equal(orc.shiftmax(k, s, output_bit=bit), orc.shiftmax_xint(k.astype(f32), s, output_bit=bit))


@gpu
@pytest.mark.parametrize("s", SM_SCALES)
@pytest.mark.parametrize("L", SM_L + [1500])
def test_shiftmax_integer_forms(L, s):
    """ivit_shiftmax_i8 / _i32_i8: any L >= 2 (beyond the 1024 the header once promised too), rows not a multiple of 4, every accepted
    scale from x0 = -1 to x0 = -65535 -- where the exponent sum of a row with a repeated maximum passes 2^32"""
    s = f32(s)
    k = sm_rows(L, 37, L)
    want = orc.shiftmax(k, s)
    assert want.min() >= 0 and want.max() <= 127 and want.max() > 0
    got = _shiftmax_int("ivit_shiftmax_i8", k, s)
    assert np.array_equal(got, want), f"i8: {(got != want).sum()} of {want.size} differ"
    got = _shiftmax_int("ivit_shiftmax_i32_i8", k, s)
    assert np.array_equal(got, want), f"i32, 8-bit scores: {(got != want).sum()} of {want.size} differ"
    km = k + sm_mask(s, L)
    assert np.abs(km).max() < 2 ** 28
    want = orc.shiftmax(km, s)
    got = _shiftmax_int("ivit_shiftmax_i32_i8", km, s)
    assert np.array_equal(got, want), f"i32, masked scores: {(got != want).sum()} of {want.size} differ"
    if s == S_X0_MIN and L >= 144:      # the 64-bit accumulator and its two-half lane reduction
        assert x0_of(s) == -65535.0 and 2 * 65535 * 2 ** 15 * (L // 2) > 2 ** 32


@gpu
@pytest.mark.parametrize("s", [2.0 ** -p for p in range(7)] + [0.0437, 0.0571])
@pytest.mark.parametrize("L", SM_L)
def test_shiftmax_literal_forms(L, s):
    """ivit_shiftmax_f32_i8 / _f32_i16 on the float view q * s (the reference's own float32 sequence on x / s): 8-bit scores at
    power-of-two and natural scales, and scores under Swin's float mask; output_bit 8, 9, 12, 16"""
    s = f32(s)
    k = sm_rows(L, 37, L + 1)
    x = (k.astype(f32) * s).astype(f32)
    xm = (x + np.where(np.arange(L) % 2 == 1, f32(-100.0), f32(0.0))).astype(f32)      # swin_quant.py:151-156
    for bit in (8, 9, 12, 16):
        want = orc.shiftmax_compat(k, s, output_bit=bit)
        assert np.array_equal(want, orc.shiftmax_xint((x / s).astype(f32), s, output_bit=bit))
        assert want.min() >= 0 and want.max() < 1 << (bit - 1)
        got = _shiftmax_f32(x, s, bit)
        assert np.array_equal(got, want), f"bit {bit}: {(got != want).sum()} of {want.size} differ"
        want = orc.shiftmax_xint((xm / s).astype(f32), s, output_bit=bit)
        got = _shiftmax_f32(xm, s, bit)
        assert np.array_equal(got, want), f"bit {bit}, masked: {(got != want).sum()} of {want.size} differ"


@gpu
def test_shiftmax_second_trip_of_the_row_loop():
    """rows > 4 * 8192 at L = 49: every form's row loop takes a second trip (grids are capped at 4096 / 8192 workgroups of 4 rows)"""
    L, rows = 49, 4 * 8192 + 5
    k = sm_rows(L, rows, 9)
    for s in (f32(2.0 ** -3), f32(0.0437)):
        want = orc.shiftmax(k, s)
        for name in ("ivit_shiftmax_i8", "ivit_shiftmax_i32_i8"):
            got = _shiftmax_int(name, k, s)
            assert np.array_equal(got, want), name
        x = (k.astype(f32) * s).astype(f32)
        for bit in (8, 16):
            want_l = orc.shiftmax_compat(k, s, output_bit=bit)
            assert np.array_equal(_shiftmax_f32(x, s, bit), want_l), bit
        assert not np.array_equal(want[-5:], want[:5])


def shiftexp_int(d, x0, n=15):
    """int_exp_shift on an integer distance d <= 0 to the row maximum (ivit_modules.py:150-162), in exact integers"""
    x = max(d + (d >> 1) - (d >> 4), n * x0)
    q = x // x0
    r = x - x0 * q
    return ((r - 2 * x0) << (n - q)) >> 1


def sum_beyond_32_bits_row(L=1024):
    """x0 = -65535, one maximum and L - 1 scores 150 below it: every exponent is just under 2^31, the exact sum is far beyond 2^32
    (clamped to 2^31: factor 1), and the same sum wrapped to 32 bits is below 2^30 (factor >= 2: every output at least doubles)"""
    k = np.full((1, L), -50, np.int32)
    k[0, 0] = 100
    x0 = int(x0_of(S_X0_MIN))
    terms = [shiftexp_int(int(v) - 100, x0) for v in k[0]]
    return k, terms


def test_row_sum_beyond_32_bits_is_what_it_claims():
    k, terms = sum_beyond_32_bits_row()
    total = sum(terms)
    assert x0_of(S_X0_MIN) == -65535.0 and total > 2 ** 32 and 0 < total % 2 ** 32 < 2 ** 30 and max(terms) < 2 ** 31
    want = orc.shiftmax(k, S_X0_MIN)
    assert np.array_equal(want[0], [t >> 24 for t in terms])                  # the clamped exact sum: factor 1
    assert want[0, 0] == 127 and (2 * np.array(terms) >> 24 != want[0]).all()     # factor 2 would change every output
    lanes = [sum(terms[i::64]) % 2 ** 32 for i in range(64)]                  # a 32-bit accumulator per lane wraps too
    assert sum(lanes) != total


@gpu
def test_shiftmax_row_sum_beyond_32_bits():
    """the 64-bit accumulator of shiftmax_kernel and its two-half lane reduction: a sum kept in 32 bits gives another factor"""
    k, _ = sum_beyond_32_bits_row()
    want = orc.shiftmax(k, S_X0_MIN)
    rows = np.repeat(k, 5, axis=0)
    for name in ("ivit_shiftmax_i8", "ivit_shiftmax_i32_i8"):
        got = _shiftmax_int(name, rows, S_X0_MIN)
        assert np.array_equal(got, np.repeat(want, 5, axis=0)), name


@gpu
def test_shiftmax_refusals():
    """the bounds of the launchers (csrc/rowops.hip launch_shiftmax, csrc/literal.hip), one value past each; a one-column row, whose
    only probability 2^(output_bit - 1) fits neither output type, is refused by every form"""
    a = filled(8192, torch.float32, 0.0)
    p = _lib.ptr(a)
    assert x0_of(2.0 ** -16) == -65536.0 and x0_of(float("inf")) == 0.0 and x0_of(2.0 ** -21) < -1048576.0
    for name in ("ivit_shiftmax_i8", "ivit_shiftmax_i32_i8"):
        for s in (2.0 ** -16, float("inf")):
            with pytest.raises(_lib.IvitError, match="outside"):
                _lib.call(name, p, 64, 4, 64, s, p, 64, st())
        with pytest.raises(_lib.IvitError, match="L must be > 1"):
            _lib.call(name, p, 1, 4, 1, 0.25, p, 1, st())
        with pytest.raises(_lib.IvitError, match="bad operand"):
            _lib.call(name, p, 60, 4, 64, 0.25, p, 64, st())
        with pytest.raises(_lib.IvitError, match="positive"):
            _lib.call(name, p, 64, 4, 64, 0.0, p, 64, st())
    for s in (2.0 ** -21, float("inf")):
        with pytest.raises(_lib.IvitError, match="out of range"):
            _lib.call("ivit_shiftmax_f32_i8", p, 64, 4, 64, s, p, 64, st())
        with pytest.raises(_lib.IvitError, match="out of range"):
            _lib.call("ivit_shiftmax_f32_i16", p, 64, 4, 64, s, 16, p, 64, st())
    with pytest.raises(_lib.IvitError, match="L must be > 1"):
        _lib.call("ivit_shiftmax_f32_i8", p, 1, 4, 1, 0.25, p, 1, st())
    with pytest.raises(_lib.IvitError, match="L must be > 1"):
        _lib.call("ivit_shiftmax_f32_i16", p, 1, 4, 1, 0.25, 16, p, 1, st())
    for bit in (1, 17):
        with pytest.raises(_lib.IvitError, match="output_bit"):
            _lib.call("ivit_shiftmax_f32_i16", p, 64, 4, 64, 0.25, bit, p, 64, st())
    # the reference's answer on a one-column row is 1.0 (128 at scale 2^-7; 32768 at 16 bits)
    assert orc.shiftmax(np.array([[5]], np.int32), 0.25)[0, 0] == 128
    assert orc.shiftmax(np.array([[5]], np.int32), 0.25, output_bit=16)[0, 0] == 32768
    import ivit_amd.quantization_utils as q
    for bit in (8, 16):
        with pytest.raises(_lib.IvitError, match="L must be > 1"):       # never -1.0
            q.IVITIntSoftmax(bit).to(DEV)(torch.full((3, 1), 1.25, device=DEV), torch.tensor([0.25], device=DEV))


# =========================================================================================== LayerNorm, literal form
def ln_literal_expected(xint, C, bias_int, s_ln, rowsum):
    """ivit_modules.py:36-63 on xint = x / s with the float32 sum of every row taken by `rowsum` -> the module's float output"""
    S = np.array([rowsum(r, i) for i, r in enumerate(xint)], f32).reshape(-1, 1)
    mean_int = np.rint((S / f32(C)).astype(f32)).astype(np.int64)                       # :37
    d = np.trunc(xint).astype(np.int64) - mean_int                                      # :38-40
    varf = (d * d).sum(axis=1, keepdims=True).astype(f32)                               # :41-42
    t = np.full_like(varf, 65536.0)
    for _ in range(10):                                                                 # :45-49
        t = np.floor(((t + np.floor((varf / t).astype(f32))).astype(f32) * f32(0.5)).astype(f32))
    factor = np.floor(((f32(1.0) / t).astype(f32) * f32(2147483648.0)).astype(f32))     # :51
    v = np.floor(((d.astype(f32) * factor).astype(f32) * f32(0.5)).astype(f32))         # :52
    return ((v + bias_int).astype(f32) * s_ln).astype(f32)                              # :61-63


def ln_rows(rows, C, seed, bits=8):
    """rows of varying mean and spread; every third one an exact .5 tie of the mean"""
    rng = np.random.default_rng(seed)
    lim = 2 ** (bits - 1)
    sc = lim / 128
    q = np.clip(np.rint(rng.normal(rng.normal(0, 10 * sc, size=(rows, 1)), rng.uniform(1, 50, size=(rows, 1)) * sc, size=(rows, C))),
                -lim, lim - 1).astype(np.int32)
    if C % 2 == 0:
        for r in range(0, rows, 3):
            d = C // 2 + C * int(rng.integers(-10, 10)) - int(q[r].sum())
            for c in rng.permutation(C):
                if d == 0:
                    break
                nv = int(np.clip(q[r, c] + d, -lim, lim - 1))
                d -= nv - q[r, c]
                q[r, c] = nv
    return q


def _affine(C, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, size=C).astype(f32), rng.normal(0, 0.1, size=C).astype(f32)


def _ln_literal(x, s_vec, bias_int, s_ln, outer=None, ldx_pad=3, ldo_pad=5):
    rows, C = x.shape
    out = filled((rows, C + ldo_pad), torch.float32, 12345.5)
    args = [_lib.ptr(dev(padded(x, C + ldx_pad, f32(3e38)))), C + ldx_pad, rows, C, _lib.ptr(dev(s_vec)), s_vec.size, _lib.ptr(dev(bias_int)),
            _lib.ptr(dev(s_ln)), _lib.ptr(out), C + ldo_pad]
    if outer is None:
        _lib.call("ivit_layernorm_f32_f32", *args, st())
    else:
        _lib.call("ivit_layernorm_f32_f32_ex", *args, outer, st())
    got = out.cpu().numpy()
    assert (got[:, C:] == 12345.5).all(), "pad columns of the output were written"
    return got[:, :C]


@pytest.mark.parametrize("C", [96, 100, 192, 768, 1024])
def test_layernorm_restatement_equals_the_oracle(C):
    """CPU: ln_literal_expected with torch's contiguous-row order is orc.layernorm_compat / orc.layernorm_scaled, tie rows included"""
    gamma, beta = _affine(C, C)
    for s, bits in ((0.0371, 8), (2.0 ** -4, 8), (0.00213, 16)):
        q = ln_rows(60, C, C + bits, bits)
        if bits == 8:
            y, s_ln, bias_int, ties = orc.layernorm_compat(q, s, gamma, beta)
            assert C % 2 or ties >= 15
        else:
            y, s_ln, bias_int = orc.layernorm_scaled(q, s, gamma, beta)
        xint = ((q.astype(f32) * f32(s)).astype(f32) / f32(s)).astype(f32)
        mine = ln_literal_expected(xint, C, bias_int, s_ln, lambda r, i: orc.torch_rowsum(r))
        assert np.array_equal(fbits(mine), fbits((y * s_ln).astype(f32)))


@gpu
@pytest.mark.parametrize("C", [96, 100, 192, 768, 1024])
def test_layernorm_literal_form(C):
    gamma, beta = _affine(C, C)
    rows = 61
    for s, bits in ((0.0371, 8), (0.11873, 8), (2.0 ** -4, 8), (0.00213, 16), (2.0 ** -9, 16)):
        q = ln_rows(rows, C, C + bits, bits)
        if bits == 8:
            y, s_ln, bias_int, _ = orc.layernorm_compat(q, s, gamma, beta)
        else:
            y, s_ln, bias_int = orc.layernorm_scaled(q, s, gamma, beta)
        want = (y * s_ln).astype(f32)
        x = (q.astype(f32) * f32(s)).astype(f32)
        s_vec = np.array([s], f32)
        got = _ln_literal(x, s_vec, bias_int, s_ln)
        assert np.array_equal(fbits(got), fbits(want)), f"s={s}: {(fbits(got) != fbits(want)).any(axis=1).sum()} rows differ"
        assert np.array_equal(fbits(_ln_literal(x, s_vec, bias_int, s_ln, outer=0)), fbits(want))      # the wrapper is _ex(.., 0)
        # outer_mean = L: the mean of row (image, column) in torch's outer-reduction order, the tail columns in its four-partial form
        L = 61
        xint = (x / f32(s)).astype(f32)
        want_o = ln_literal_expected(xint, C, bias_int, s_ln, lambda r, i: orc.torch_outer_rowsum(r, (i % L) >= (L // 32) * 32))
        got_o = _ln_literal(x, s_vec, bias_int, s_ln, outer=L)
        assert np.array_equal(fbits(got_o), fbits(want_o)), f"outer, s={s}: {(fbits(got_o) != fbits(want_o)).any(axis=1).sum()} rows differ"
    # per-channel input scales (n_s = C), powers of two: x / s is the integer again and the plain integer oracle applies
    q = ln_rows(rows, C, C + 1)
    s_vec = (2.0 ** -np.random.default_rng(C).integers(3, 7, size=C)).astype(f32)
    y, s_ln, bias_int = orc.layernorm(q, gamma, beta)
    got = _ln_literal((q.astype(f32) * s_vec).astype(f32), s_vec, bias_int, s_ln)
    assert np.array_equal(fbits(got), fbits((y * s_ln).astype(f32)))
    with pytest.raises(_lib.IvitError, match="bad shape"):
        _ln_literal(np.zeros((rows, C), f32), s_vec[:2], bias_int, s_ln)
    with pytest.raises(_lib.IvitError, match="bad shape"):
        _ln_literal(np.zeros((rows, C), f32), s_vec, bias_int, s_ln, outer=7)              # rows % outer_mean != 0


def test_layernorm_outer_order_differs_from_the_inner_one():
    """CPU: on the tie rows the two orders give different means somewhere, so the outer_mean case above is a case of its own"""
    C, L, s = 96, 61, f32(0.0371)
    q = ln_rows(61 * 8, C, 3)
    xint = ((q.astype(f32) * s).astype(f32) / s).astype(f32)
    a = np.array([orc.torch_rowsum(r) for r in xint], f32)
    b = np.array([orc.torch_outer_rowsum(r, (i % L) >= (L // 32) * 32) for i, r in enumerate(xint)], f32)
    assert (np.rint(a / f32(C)) != np.rint(b / f32(C))).any()


# =========================================================================================== batched products (QuantMatMul)
BG_SHAPES = [(6, 17, 17, 64), (6, 197, 197, 64), (12, 49, 49, 32), (2, 144, 144, 32), (1, 577, 577, 64), (1, 5, 300, 64), (3, 7, 9, 5),
             (2, 33, 1, 64)]


def _bgemm(name, X, Y, Tq, Tk, D, *extra):
    """X: Q [b, Tq, D] (qk) or P [b, Tq, Tk] (pv); Y: K [b, Tk, D] or V [b, Tk, D]"""
    batch = X.shape[0]
    cols = Tk if name == "ivit_bgemm_qk_i8" else D
    n = batch * Tq * cols
    out = filled(n + 9, torch.int32, -77777777)
    args = (_lib.ptr(dev(X)), _lib.ptr(dev(Y)), _lib.ptr(out), batch, Tq, Tk, D, *extra, st())
    if name == "ivit_bgemm_qk_i8":
        _lib.call("ivit_bgemm_qk_i8", *args)
    elif name == "ivit_bgemm_pv_i8":
        _lib.call("ivit_bgemm_pv_i8", *args)
    elif name == "ivit_bgemm_pv_i16_i8":
        _lib.call("ivit_bgemm_pv_i16_i8", *args)
    else:
        _lib.call("ivit_bgemm_pv_i32_i8", *args)
    got = out.cpu().numpy()
    assert (got[n:] == -77777777).all()
    return got[:n].reshape(batch, Tq, cols)


def _fits(a):
    assert np.abs(a).max() < 2 ** 31
    return a.astype(np.int32)


@gpu
@pytest.mark.parametrize("batch,Tq,Tk,D", BG_SHAPES + [(16, 600, 600, 8), (16, 600, 16, 224)])
def test_bgemm_equals_integer_einsum(batch, Tq, Tk, D):
    """the last two shapes: batch * Tq * Tk (qk) resp. batch * Tq * D (pv) beyond 8192 * 256 outputs, a second trip of the loop"""
    rng = np.random.default_rng(batch + Tq + Tk + D)
    Q = rng.integers(-128, 128, size=(batch, Tq, D)).astype(np.int8)
    K = rng.integers(-128, 128, size=(batch, Tk, D)).astype(np.int8)
    P = rng.integers(-128, 128, size=(batch, Tq, Tk)).astype(np.int8)
    Q[0, 0], K[0, 0], P[0, 0] = -128, -128, -128                   # the extremes against each other
    K[0, :, 0] = -128
    if batch * Tq * Tk > 8192 * 256 or batch * Tq * D > 8192 * 256:
        assert (batch * Tq * Tk > 8192 * 256) != (batch * Tq * D > 8192 * 256)
    want = _fits(Q.astype(np.int64) @ K.astype(np.int64).transpose(0, 2, 1))
    got = _bgemm("ivit_bgemm_qk_i8", Q, K, Tq, Tk, D)
    assert np.array_equal(got, want), f"qk: {(got != want).sum()} of {want.size} differ"
    assert want[0, 0, 0] == 128 * 128 * D
    want = _fits(P.astype(np.int64) @ K.astype(np.int64))
    got = _bgemm("ivit_bgemm_pv_i8", P, K, Tq, Tk, D)
    assert np.array_equal(got, want), f"pv: {(got != want).sum()} of {want.size} differ"
    assert want[0, 0, 0] == 128 * 128 * Tk
    for name, dt, extra in (("ivit_bgemm_pv_i16_i8", np.int16, ()), ("ivit_bgemm_pv_i32_i8", np.int32, (128,))):
        got = _bgemm(name, P.astype(dt), K, Tq, Tk, D, *extra)
        assert np.array_equal(got, want), name


@gpu
@pytest.mark.parametrize("batch,Tq,Tk,D", [(3, 50, 197, 64), (2, 64, 577, 64), (4, 49, 49, 32)])
def test_bgemm_pv_wide_probabilities(batch, Tq, Tk, D):
    """_pv_i16_i8 on its documented contract -- rows of Shiftmax(output_bit = 16), a one-hot row against V = -128 included -- and
    _pv_i32_i8 on I-BERT's 16-bit softmax, whose one-hot rows reach 2^15"""
    rng = np.random.default_rng(Tk)
    k = sm_rows(Tk, batch * Tq, Tk)
    V = rng.integers(-128, 128, size=(batch, Tk, D)).astype(np.int8)
    V[:, Tk // 2] = -128
    P = orc.shiftmax(k, 2.0 ** -3, output_bit=16).reshape(batch, Tq, Tk)
    assert P.max() <= 32767 and P[0, 1, Tk // 2] > 32000 and P.sum(axis=2).max() <= 2 ** 15 + Tk
    want = _fits(P.astype(np.int64) @ V.astype(np.int64))
    assert want[0, 1].max() < -128 * 32000
    got = _bgemm("ivit_bgemm_pv_i16_i8", P.astype(np.int16), V, Tq, Tk, D)
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} differ"
    Pb = ib.softmax(k, 2.0 ** -4, 0.0, float(ib.softmax_constants(f32(2.0 ** -4), 0.0, 1.0)[2]) * 2.0 ** 30, output_bit=16)[0]
    Pb = Pb.astype(np.int32).reshape(batch, Tq, Tk)
    Pb[0, 1] = 0
    Pb[0, 1, Tk // 2] = 32768                                      # a one-hot row at the upper end
    assert Pb.max() == 32768
    want = _fits(Pb.astype(np.int64) @ V.astype(np.int64))
    if 32768 * 128 * Tk >= 2 ** 31:               # 577 keys: the bound cannot be given, the launcher refuses in front of the launch
        with pytest.raises(_lib.IvitError, match="overflows int32"):
            _bgemm("ivit_bgemm_pv_i32_i8", Pb, V, Tq, Tk, D, 32768)
        return
    got = _bgemm("ivit_bgemm_pv_i32_i8", Pb, V, Tq, Tk, D, 32768)
    assert np.array_equal(got, want) and want[0, 1, 0] == -128 * 32768


@gpu
def test_bgemm_refusals():
    a = filled(1 << 16, torch.int32, 0)
    p = _lib.ptr(a)
    # |P| <= 2^15 over 512 keys: 2^15 * 128 * 512 = 2^31 does not fit; over 511 keys it does (accepted above with fewer)
    with pytest.raises(_lib.IvitError, match="overflows int32"):
        _lib.call("ivit_bgemm_pv_i32_i8", p, p, p, 1, 4, 512, 8, 32768, st())
    with pytest.raises(_lib.IvitError, match="overflows int32"):
        _lib.call("ivit_bgemm_pv_i32_i8", p, p, p, 1, 4, 8, 8, -1, st())
    out = filled(4 * 8 + 3, torch.int32, -5)
    _lib.call("ivit_bgemm_pv_i32_i8", p, p, _lib.ptr(out), 1, 4, 511, 8, 32768, st())
    assert (out.cpu().numpy() == [0] * 32 + [-5] * 3).all()
    for name in ("ivit_bgemm_qk_i8", "ivit_bgemm_pv_i8", "ivit_bgemm_pv_i16_i8"):
        with pytest.raises(_lib.IvitError, match="bad operand"):
            _lib.call(name, p, None, p, 1, 4, 4, 8, st())
        with pytest.raises(_lib.IvitError, match="bad operand"):
            _lib.call(name, p, p, p, 1, 4, 0, 8, st())


@gpu
def test_quant_matmul_regimes_equal_the_direct_calls():
    """QuantMatMul picks the entry point by the largest |A|: 8 bit, 16 bit, beyond.  Same integers as the int64 product"""
    import ivit_amd.quantization_utils as q
    rng = np.random.default_rng(2)
    batch, Tq, Tk, D = 3, 20, 33, 16
    sA, sB = f32(2.0 ** -7), f32(2.0 ** -4)
    V = rng.integers(-128, 128, size=(batch, Tk, D)).astype(np.int32)
    for amax in (127, 32767, 32768):
        A = rng.integers(0, min(amax, 400), size=(batch, Tq, Tk)).astype(np.int32)
        A[0, 0, 0] = amax
        want = _fits(A.astype(np.int64) @ V.astype(np.int64))
        mm = q.QuantMatMul()
        y, s = mm(torch.from_numpy((A.astype(f32) * sA).astype(f32)).to(DEV), torch.tensor([float(sA)], device=DEV),
                  torch.from_numpy((V.astype(f32) * sB).astype(f32)).to(DEV), torch.tensor([float(sB)], device=DEV))
        assert float(s) == float(sA * sB)
        assert np.array_equal(y.cpu().numpy(), (want.astype(f32) * f32(sA * sB)).astype(f32)), amax
        assert np.abs(want).max() < 2 ** 24           # so that the float view above is exact


# =========================================================================================== cls token + position embedding
EMB_SHAPES = [(1, 2, 4), (3, 197, 192), (2, 577, 768), (2, 50, 1024), (64, 197, 768)]
#  name                 (m, e)                            M
EMB_MULT = {"half": (1 << 30, 31),                      # 1/2 exactly: odd inputs are ties
            "generic": tuple(int(v[0]) for v in dyadic(f32(0.0371), f32(0.0532))),
            "above_one": tuple(int(v[0]) for v in dyadic(f32(1.7), f32(1.0)))}


def _embed(bits, patch, pos_add, cls_row, m, e, B, T, C):
    n = B * T * C
    out = filled(n + 16, torch.int8 if bits == 8 else torch.int16, 99)
    args = (_lib.ptr(dev(patch)), _lib.ptr(dev(pos_add)), _lib.ptr(dev(cls_row)), m, e, _lib.ptr(out), B, T, C, st())
    if bits == 8:
        _lib.call("ivit_embed_assemble_i8", *args)
    else:
        _lib.call("ivit_embed_assemble_i16", *args)
    got = out.cpu().numpy()
    assert (got[n:] == 99).all()
    return got[:n].reshape(B, T, C).astype(np.int64)


def _embed_expected(bits, patch, pos_add, cls_row, m, e, B, T, C):
    lim = 2 ** (bits - 1)
    prod = patch.astype(np.float64).reshape(B, T - 1, C) * (float(m) / 2.0 ** e)        # exact: at most 47 significant bits
    want = np.empty((B, T, C), np.int64)
    want[:, 1:] = np.clip(np.rint(prod).astype(np.int64) + pos_add[None, 1:].astype(np.int64), -lim, lim - 1)
    want[:, 0] = cls_row
    return want


@gpu
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("B,T,C", EMB_SHAPES)
def test_embed_assemble(B, T, C, bits):
    """(64, 197, 768): more than 8192 * 256 quads, a second trip of the loop"""
    rng = np.random.default_rng(B + T + C + bits)
    lim = 2 ** (bits - 1)
    np_dt, pos_dt = (np.int8, np.int16) if bits == 8 else (np.int16, np.int32)
    patch = rng.integers(-lim, lim, size=(B * (T - 1), C)).astype(np_dt)
    patch.reshape(-1)[:4] = [lim - 1, -lim, 1, -1]
    cls_row = rng.integers(-lim, lim, size=C).astype(np_dt)
    reach = 32767 if bits == 8 else 100000                         # pos_add up to the end of int16 (i8 form), beyond 16 bits (i16 form)
    pos_add = rng.integers(-lim // 4, lim // 4, size=(T, C)).astype(pos_dt)
    pos_add[1:, 0::7] = reach
    pos_add[1:, 3::7] = -reach
    pos_add[0] = 12345 % lim                                       # row 0 belongs to the class token: never added
    largest = ((1 << 31) - 1, 11 if bits == 8 else 16)             # just below the launcher's bound 2^20 / 2^15
    cases = dict(EMB_MULT, largest=largest) if B * T * C < 10 ** 6 else {"generic": EMB_MULT["generic"]}
    for name, (m, e) in cases.items():
        want = _embed_expected(bits, patch, pos_add, cls_row, m, e, B, T, C)
        got = _embed(bits, patch, pos_add, cls_row, m, e, B, T, C)
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} of {want.size} differ"
        if T * C >= 1000:
            assert (want == lim - 1).any() and (want == -lim).any(), name      # saturation both ways
    assert (patch.astype(np.int64) % 2 == 1).any()                 # odd inputs: exact ties under the multiplier 1/2
    with pytest.raises(_lib.IvitError, match="multiplier too large"):
        _embed(bits, patch, pos_add, cls_row, 1 << 30, 10 if bits == 8 else 15, B, T, C)
    with pytest.raises(_lib.IvitError, match="bad shape"):
        _embed(bits, patch, pos_add, cls_row, 1 << 30, 31, B, 1, C)


# =========================================================================================== element-wise
@gpu
@pytest.mark.parametrize("batch,chans,hw,patch,lda", [(2, 3, 224, 16, 768), (3, 3, 56, 4, 64), (1, 4, 8, 4, 64), (1, 1, 32, 8, 68), (57, 3, 224, 16, 768)])
def test_quantize_patchify_u8(batch, chans, hw, patch, lda):
    """uint8 pixels through a per-channel 256-entry table into the im2col operand; pad columns [K, lda) are not written; 57 images of
    224 x 224: more than 8192 * 256 pixel quads, a second trip of the loop"""
    rng = np.random.default_rng(batch + hw)
    img = rng.integers(0, 256, size=(batch, chans, hw, hw), dtype=np.uint8)
    img[0, :, 0, :4] = [0, 255, 1, 254]
    lut = rng.integers(-128, 128, size=(chans, 256)).astype(np.int8)
    g, K = hw // patch, chans * patch * patch
    rows = batch * g * g
    want = lut[np.arange(chans)[None, :, None, None], img].reshape(batch, chans, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(rows, K)
    A = filled((rows, lda), torch.int8, 99)
    _lib.call("ivit_quantize_patchify_u8_i8", _lib.ptr(dev(img)), _lib.ptr(A), lda, batch, chans, hw, patch, _lib.ptr(dev(lut)), st())
    got = A.cpu().numpy()
    assert np.array_equal(got[:, :K], want) and (got[:, K:] == 99).all()
    with pytest.raises(_lib.IvitError, match="bad shape"):
        _lib.call("ivit_quantize_patchify_u8_i8", _lib.ptr(dev(img)), _lib.ptr(A), lda, batch, 5, hw, patch, _lib.ptr(dev(lut)), st())
    with pytest.raises(_lib.IvitError, match="lda too small"):
        _lib.call("ivit_quantize_patchify_u8_i8", _lib.ptr(dev(img)), _lib.ptr(A), K - 4, batch, chans, hw, patch, _lib.ptr(dev(lut)), st())


@gpu
def test_residual_requant_i8_exhaustive():
    """all 65 536 (a, b) pairs under the residual scale pairs of test_gpu_ops.test_gemm_requant_residual: the usual kind, ratios with
    exact ties, identity, an arbitrary drawn triple, another fixed one"""
    rng = np.random.default_rng(344)
    pairs = [(0.7 * 2 ** -4, 2 ** -5, 2 ** -4), (2 ** -5, 2 ** -5, 2 ** -4), (1.0, 1.0, 1.0),
             (float(rng.uniform(0.01, 0.3)), float(rng.uniform(0.01, 0.3)), float(rng.uniform(0.05, 0.2))), (0.3337, 0.0421, 0.0517)]
    v = np.arange(-128, 128, dtype=np.int32)
    a, b = np.repeat(v, 256).reshape(256, 256), np.tile(v, 256).reshape(256, 256)
    for s_a, s_b, s_out in pairs:
        m1, e1 = dyadic(f32(s_a), f32(s_out))
        m2, e2 = dyadic(f32(s_b), f32(s_out))
        want = orc.requant(a, m1.astype(np.float64), e1, 8, z2=b, m2=m2.astype(np.float64), e2=e2)
        out = filled(65536 + 13, torch.int8, 99)
        _lib.call("ivit_residual_requant_i8", _lib.ptr(dev(a.astype(np.int8))), int(m1[0]), int(e1[0]), _lib.ptr(dev(b.astype(np.int8))),
                  int(m2[0]), int(e2[0]), _lib.ptr(out), 65536, st())
        got = out.cpu().numpy()
        assert np.array_equal(got[:65536].reshape(256, 256).astype(np.int32), want) and (got[65536:] == 99).all(), (s_a, s_b, s_out)
    with pytest.raises(_lib.IvitError, match="multiplier too large"):
        _lib.call("ivit_residual_requant_i8", _lib.ptr(out), 1 << 30, 10, _lib.ptr(out), 1 << 30, 31, _lib.ptr(out), 16, st())


def _f32_to_i32_inputs(C, s_vec):
    rng = np.random.default_rng(C)
    z = rng.integers(-40000, 40000, size=(23, C)).astype(np.int64)
    blocks = [z.astype(f32) * s_vec,                               # exact multiples
              (z.astype(f32) + f32(0.5)) * s_vec,                  # exact ties at a power-of-two scale
              (-rng.uniform(0.01, 0.99, size=(23, C)).astype(f32) - (z % 3).astype(f32)) * s_vec,      # negative fractions
              rng.normal(0, 300, size=(23, C)).astype(f32),
              np.where(rng.integers(0, 2, size=(23, C)) == 1, f32(1), f32(-1)) * f32(2.0 ** 31) * rng.uniform(0.9, 40, size=(23, C)).astype(f32) * s_vec]
    return np.concatenate(blocks).astype(f32)


@gpu
@pytest.mark.parametrize("C,per_channel", [(96, False), (96, True), (1, False), (33, True)])
@pytest.mark.parametrize("natural", [False, True])
def test_f32_to_i32_and_back(C, per_channel, natural):
    """z = round(x / s) / trunc(x / s) with the float32 quotient; beyond int32 the kernel saturates at -2^31 and at 2147483520, the
    largest float32 below 2^31.  Then y = float(z) * s, with |z| > 2^24 (the conversion rounds)"""
    rng = np.random.default_rng(C + per_channel)
    n_s = C if per_channel else 1
    s_vec = (rng.uniform(0.01, 0.2, size=n_s) if natural else 2.0 ** -rng.integers(2, 9, size=n_s)).astype(f32)
    x = _f32_to_i32_inputs(C, s_vec)
    rows = x.shape[0]
    q = (x / s_vec).astype(f32)
    assert (np.abs(q) > 2.0 ** 31).any() and (q < 0).any()
    if not natural:
        assert (np.abs(q - np.trunc(q)) == 0.5).any()
    for mode, fn in ((0, np.rint), (1, np.trunc)):
        want = np.clip(fn(q), f32(-2147483648.0), f32(2147483520.0)).astype(np.int64).astype(np.int32)
        out = filled(rows * C + 5, torch.int32, -77777777)
        _lib.call("ivit_f32_to_i32", _lib.ptr(dev(x)), rows, C, _lib.ptr(dev(s_vec)), n_s, mode, _lib.ptr(out), st())
        got = out.cpu().numpy()
        assert np.array_equal(got[:rows * C].reshape(rows, C), want) and (got[rows * C:] == -77777777).all(), mode
        assert want.max() == 2147483520 and want.min() == -2 ** 31
    assert not np.array_equal(np.rint(q), np.trunc(q)) and not np.array_equal(np.trunc(q), np.floor(q))
    z = rng.integers(-2 ** 31, 2 ** 31, size=(rows, C)).astype(np.int32)
    z.reshape(-1)[:3] = [2 ** 24 + 1, -2 ** 31, 2 ** 31 - 1]
    y = filled(rows * C + 5, torch.float32, 12345.5)
    _lib.call("ivit_i32_to_f32", _lib.ptr(dev(z)), rows, C, _lib.ptr(dev(s_vec)), n_s, _lib.ptr(y), st())
    got = y.cpu().numpy()
    assert np.array_equal(fbits(got[:rows * C].reshape(rows, C)), fbits((z.astype(f32) * s_vec).astype(f32))) and (got[rows * C:] == 12345.5).all()
    with pytest.raises(_lib.IvitError, match="bad operand"):
        _lib.call("ivit_f32_to_i32", _lib.ptr(dev(x)), rows, C, _lib.ptr(dev(s_vec)), n_s, 2, _lib.ptr(out), st())


@gpu
def test_f32_to_i32_second_trip():
    rows, C = 8192 * 256 // 64 + 3, 64
    rng = np.random.default_rng(1)
    x = rng.normal(0, 50, size=(rows, C)).astype(f32)
    s_vec = (2.0 ** -rng.integers(2, 9, size=C)).astype(f32)
    out = filled(rows * C + 5, torch.int32, -77777777)
    _lib.call("ivit_f32_to_i32", _lib.ptr(dev(x)), rows, C, _lib.ptr(dev(s_vec)), C, 0, _lib.ptr(out), st())
    got = out.cpu().numpy()
    assert np.array_equal(got[:rows * C].reshape(rows, C), np.rint((x / s_vec).astype(f32)).astype(np.int32)) and (got[rows * C:] == -77777777).all()
    y = filled(rows * C + 5, torch.float32, 12345.5)
    _lib.call("ivit_i32_to_f32", _lib.ptr(out), rows, C, _lib.ptr(dev(s_vec)), C, _lib.ptr(y), st())
    goty = y.cpu().numpy()
    assert np.array_equal(fbits(goty[:rows * C].reshape(rows, C)), fbits((got[:rows * C].reshape(rows, C).astype(f32) * s_vec).astype(f32)))
    assert (goty[rows * C:] == 12345.5).all()


@gpu
@pytest.mark.parametrize("n", [1, 5, 1000, 8192 * 256 + 77])
def test_narrow_i32_i8(n):
    """saturates and raises the flag to 1 on overflow only; the flag keeps its previous value otherwise and may be NULL"""
    rng = np.random.default_rng(n)
    inside = rng.integers(-128, 128, size=n).astype(np.int32)
    if n >= 5:
        inside[:2] = [-128, 127]
    outside = inside.copy()
    outside[n - 1] = 128 if n % 2 else -129
    wide = rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)
    for z, flag0, flag1 in ((inside, 0, 0), (inside, 7, 7), (outside, 0, 1), (wide, 0, 1), (outside, None, None)):
        out = filled(n + 7, torch.int8, 99)
        flag = None if flag0 is None else filled(3, torch.int32, flag0)
        _lib.call("ivit_narrow_i32_i8", _lib.ptr(dev(z)), _lib.ptr(out), n, _lib.ptr(flag), st())
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], np.clip(z, -128, 127).astype(np.int8)) and (got[n:] == 99).all()
        if flag is not None:
            assert flag.cpu().numpy().tolist() == [flag1, flag0, flag0]


QN = [1, 2, 3, 5, 1023, 4 * 8192 * 256 + 7]


@gpu
@pytest.mark.parametrize("n", QN)
def test_quantize_input(n):
    """n = 1, 2, 3: the scalar tail of the float4 kernel alone; 5, 1023: after full vectors; the last: a second trip of the loop and a
    tail.  bits 8 (both entry points), 16, 32"""
    rng = np.random.default_rng(n)
    x = rng.normal(0, 1.5, size=n).astype(f32)
    x[:min(n, 3)] = [4.5, -4.6, 0.0317][:min(n, 3)]
    x[n - 1] = -0.7531
    s = f32(0.0317)
    inv = f32(1.0) / s
    for bits in (8, 16, 32):
        lo, hi = f32(-2.0 ** (bits - 1)), f32(2.0 ** (bits - 1) - 1)
        xs = x if bits < 32 else (x * f32(1000.0)).astype(f32)
        want = np.clip(np.rint((inv * xs).astype(f32)), lo, hi).astype(np.int64)
        if n <= 1023:
            assert np.array_equal(want, orc.quant_sym(xs, s, bits).reshape(-1))
        if bits == 8 and n > 3:
            assert want.max() == 127 and want.min() == -128
        out = filled(n + 9, torch.int32, -77777777)
        _lib.call("ivit_quantize_input_f32_i32", _lib.ptr(dev(xs)), _lib.ptr(out), n, float(inv), bits, st())
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == -77777777).all(), bits
    out8 = filled(n + 9, torch.int8, 99)
    _lib.call("ivit_quantize_input_f32_i8", _lib.ptr(dev(x)), _lib.ptr(out8), n, float(inv), st())
    got = out8.cpu().numpy()
    want = np.clip(np.rint((inv * x).astype(f32)), -128, 127).astype(np.int8)
    assert np.array_equal(got[:n], want), f"{(got[:n] != want).sum()} of {n} differ, the last {n % 4} in the scalar tail"
    assert (got[n:] == 99).all()
    assert want[n - 1] == -24
