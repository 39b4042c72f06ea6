"""ivit_weight_quant_rows_f32_i8 and ivit_bias_quant_f32_i32 (csrc/calib.hip) against their specification, prepare.weight_scale /
quant_sym / LinearParams, bit for bit: scale, w8, w_int, s_acc, b32 and b_int, over the row lengths at which the kernel changes its
path (dword loads, 16-byte loads with and without a partial last group, rows kept in registers up to 4096 columns, rows read twice
above), with strided, fenced operands (tests/fenced.py), on crafted rows (zeros, ties, denormals, the FLT_EPSILON floor, saturating
biases), on the reference's operator fixture, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import LinearParams, quant_sym, weight_scale  # noqa: E402

import fenced  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
EPS = np.finfo(np.float32).eps
SHAPES = [(1, 1), (5, 3), (7, 97), (96, 48), (192, 384), (10, 768), (1001, 64), (16, 3072), (3, 4096), (3, 4100)]
_REF = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def reference(rows, cols):
    """weights, bias, input scale and the host form's results for one shape: computed once, shared, never changed"""
    if (rows, cols) not in _REF:
        rng = np.random.default_rng(1000 * rows + cols)
        W = (rng.standard_normal((rows, cols)) * rng.uniform(0.01, 0.5, (rows, 1))).astype(f32)
        b = (rng.standard_normal(rows) * 0.3).astype(f32)
        s_in = f32(rng.uniform(0.01, 0.06))
        lp, lp0 = LinearParams(W, b, s_in), LinearParams(W, None, s_in)
        assert lp0.b32 is None and same(lp0.s_acc, lp.s_acc)
        ref = dict(W=W, b=b, s_in=s_in, scale=lp.sw, w8=lp.W8, w_int=lp.W8.astype(f32), s_acc=lp.s_acc, b32=lp.b32, b_int=lp.b32.astype(f32))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[rows, cols] = ref
    return _REF[rows, cols]


def t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def run_weights(W, with_int=True):
    """dense call on torch tensors -> scale, w8, w_int (or None) as numpy"""
    rows, cols = W.shape
    w = t(W)
    scale = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
    w8 = torch.full((rows, cols), 85, dtype=torch.int8, device=DEV)
    w_int = torch.full((rows, cols), 7.0, dtype=torch.float32, device=DEV) if with_int else None
    _lib.call("ivit_weight_quant_rows_f32_i8", _lib.ptr(w), cols, rows, cols, _lib.ptr(scale), _lib.ptr(w8), cols, _lib.ptr(w_int),
              _lib.stream_ptr())
    return scale.cpu().numpy(), w8.cpu().numpy(), None if w_int is None else w_int.cpu().numpy()


def run_bias(bias, scale, s_in, with_int=True):
    n = scale.size
    bias_t, scale_t = None if bias is None else t(bias), t(scale)
    s_acc = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
    b32 = None if bias is None else torch.full((n,), 85, dtype=torch.int32, device=DEV)
    b_int = torch.full((n,), 7.0, dtype=torch.float32, device=DEV) if (with_int and bias is not None) else None
    _lib.call("ivit_bias_quant_f32_i32", _lib.ptr(bias_t), _lib.ptr(scale_t), n, float(s_in), _lib.ptr(s_acc),
              _lib.ptr(b32), _lib.ptr(b_int), _lib.stream_ptr())
    return s_acc.cpu().numpy(), None if b32 is None else b32.cpu().numpy(), None if b_int is None else b_int.cpu().numpy()


# ---------------------------------------------------------------------------- the kernels against the host form
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("with_int", [True, False], ids=["wint", "nowint"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_kernels_equal_the_host_form(rows, cols, with_int, with_bias):
    """dense operands into sentinel-filled, guarded outputs: every result bit for bit, nothing written outside"""
    r = reference(rows, cols)
    w = t(r["W"])
    scale = fenced.output(1, rows, rows, np.float32, expected=r["scale"][None])
    w8 = fenced.output(rows, cols, cols, np.int8, expected=r["w8"])
    w_int = fenced.output(rows, cols, cols, np.float32, expected=r["w_int"]) if with_int else None
    _lib.call("ivit_weight_quant_rows_f32_i8", _lib.ptr(w), cols, rows, cols, scale.ptr, w8.ptr, cols, w_int.ptr if with_int else None,
              _lib.stream_ptr())
    fenced.check(scale, r["scale"][None])
    fenced.check(w8, r["w8"])
    if with_int:
        fenced.check(w_int, r["w_int"])
    assert np.array_equal(w.cpu().numpy(), r["W"])
    s_acc = fenced.output(1, rows, rows, np.float32, expected=r["s_acc"][None])
    b32 = fenced.output(1, rows, rows, np.int32, expected=r["b32"][None]) if with_bias else None
    b_int = fenced.output(1, rows, rows, np.float32, expected=r["b_int"][None]) if (with_bias and with_int) else None
    b = t(r["b"]) if with_bias else None
    _lib.call("ivit_bias_quant_f32_i32", _lib.ptr(b), scale.ptr, rows, float(r["s_in"]), s_acc.ptr,
              b32.ptr if b32 else None, b_int.ptr if b_int else None, _lib.stream_ptr())
    fenced.check(s_acc, r["s_acc"][None])
    if with_bias:
        fenced.check(b32, r["b32"][None])
    if b_int:
        fenced.check(b_int, r["b_int"][None])


# ---------------------------------------------------------------------------- strided rows between poison, padded outputs
def _pad(n, m):
    return (n + m - 1) // m * m


# (ldw - cols or "pad4": the next multiple of 4 plus 4; lead bytes of w; ldo - cols or "pad64": pad64(cols) + 64; lead bytes of w8)
STRIDES = {"ldw+1_ldo+1": (1, 0, 1, 0), "ldw+4_ldo_pad64": (4, 0, "pad64", 0), "ldw_pad4_w8_odd": ("pad4", 0, 1, 3),
           "w_off_16_bytes": (4, 4, "pad64", 0)}


@pytest.mark.parametrize("strides", list(STRIDES), ids=list(STRIDES))
@pytest.mark.parametrize("rows,cols", SHAPES, ids=lambda v: str(v))
def test_strided_fenced_operands(rows, cols, strides):
    """w with ldw > cols between poison that would change every row's scale (shown on the CPU first); w8 with ldo > cols into a
    sentinel-filled buffer: pad columns, guards and slack keep their fill.  ldw = cols + 1 takes rows off the 16-byte grid (dword
    loads); pad4(cols) + 4 keeps them on it with a partial last group where cols % 4 != 0"""
    dw, lead_w, do, lead_o = STRIDES[strides]
    ldw = _pad(cols, 4) + 4 if dw == "pad4" else cols + dw
    ldo = _pad(cols, 64) + 64 if do == "pad64" else cols + do
    r = reference(rows, cols)
    w = fenced.input(r["W"], ldw, 1e30, lead_bytes=lead_w, oracle=lambda a: weight_scale(a).reshape(-1, 1), expected=r["scale"].reshape(-1, 1))
    scale = fenced.output(1, rows, rows, np.float32, expected=r["scale"][None])
    w8 = fenced.output(rows, cols, ldo, np.int8, expected=r["w8"], lead_bytes=lead_o)
    w_int = fenced.output(rows, cols, cols, np.float32, expected=r["w_int"])
    _lib.call("ivit_weight_quant_rows_f32_i8", w.ptr, ldw, rows, cols, scale.ptr, w8.ptr, ldo, w_int.ptr, _lib.stream_ptr())
    fenced.check(scale, r["scale"][None])
    fenced.check(w8, r["w8"])
    fenced.check(w_int, r["w_int"])
    fenced.check(w)


# ---------------------------------------------------------------------------- crafted rows
def _crafted():
    cols = 16
    rows, what = [], []

    def row(name, vals):
        v = np.zeros(cols, f32)
        v[:len(vals)] = np.asarray(vals, f32)
        rows.append(v)
        what.append(name)
    row("zeros", [])
    row("negative extreme", [-1.0, 0.5, 0.25, -0.75, 1.0 / 3])
    s = 2.0 ** -5                                   # mx = 127 * 2^-5: the scale is exactly 2^-5, every product below is exact
    row("ties", [127 * s, 0.5 * s, -0.5 * s, 1.5 * s, -1.5 * s, 2.5 * s, -2.5 * s, 126.5 * s, -126.5 * s, 3.5 * s, 64.5 * s, -127 * s])
    tiny = np.array([1, 2 ** 22, 2 ** 23 - 1], np.int32).view(f32)                   # denormals: 1.4e-45 .. 1.17e-38
    row("denormals only", np.concatenate([tiny, -tiny]))
    row("one denormal", [0.7, -0.3, tiny[1], -tiny[0], 0.011])
    edge = f32(127.0) * f32(EPS)                    # mx / 127 == FLT_EPSILON exactly; its neighbours fall on either side
    for k in (-3, -2, -1, 0, 1, 2, 3):
        mx = edge
        for _ in range(abs(k)):
            mx = np.nextafter(mx, f32(0.0) if k < 0 else f32(1.0))
        row(f"eps edge {k:+d}", [mx, -mx / 2, mx / 3, EPS, -EPS / 2, EPS / 2, 1.5 * EPS])
    return np.stack(rows), what


def test_crafted_rows():
    W, what = _crafted()
    exp_scale = weight_scale(W)
    exp_w8 = quant_sym(W, exp_scale[:, None], 8).astype(np.int8)
    i = {n: k for k, n in enumerate(what)}
    # the host form itself does what the cases are about
    assert exp_scale[i["zeros"]] == EPS and not exp_w8[i["zeros"]].any()
    assert exp_w8[i["negative extreme"]].min() == -127 and exp_w8.min() == -127
    assert exp_scale[i["ties"]] == f32(2.0 ** -5)
    assert exp_w8[i["ties"]][:12].tolist() == [127, 0, 0, 2, -2, 2, -2, 126, -126, 4, 64, -127]
    assert exp_scale[i["denormals only"]] == EPS and not exp_w8[i["denormals only"]].any()
    assert exp_scale[i["eps edge -3"]] == EPS and exp_scale[i["eps edge +3"]] > EPS
    for pad, lead in ((0, 0), (1, 0), (4, 4)):      # 16-byte loads, dword loads, dword loads off the 16-byte grid
        w = fenced.input(W, W.shape[1] + pad, 1e30, lead_bytes=lead)
        scale = fenced.output(1, W.shape[0], W.shape[0], np.float32, expected=exp_scale[None])
        w8 = fenced.output(W.shape[0], W.shape[1], W.shape[1], np.int8, expected=exp_w8)
        w_int = fenced.output(W.shape[0], W.shape[1], W.shape[1], np.float32, sentinel=fenced.SENTINELS[4][0])
        _lib.call("ivit_weight_quant_rows_f32_i8", w.ptr, W.shape[1] + pad, W.shape[0], W.shape[1], scale.ptr, w8.ptr, W.shape[1], w_int.ptr,
                  _lib.stream_ptr())
        fenced.check(scale, exp_scale[None])
        fenced.check(w8, exp_w8)
        fenced.check(w_int, exp_w8.astype(f32))       # bit patterns: every zero is +0.0
        got = w_int.rows2d(w_int.fetch())
        assert not np.signbit(got[got == 0]).any()


def test_crafted_biases():
    """|bias / s_acc| beyond 2^31 at both ends (s_acc near 1e-12), and quotients that land on +-2^31 exactly and just inside"""
    scale = np.array([1e-6, 1e-6, 1e-6, 1e-6, 2.0 ** -20, 2.0 ** -20, 2.0 ** -20, 2.0 ** -20, 2.0 ** -20], f32)
    s_in = [f32(1e-6), f32(2.0 ** -11)]
    bias = np.array([1.0, -1.0, 3e-3, -2.2e-3, 1.0, -1.0, 1.0 - 2.0 ** -24, -(1.0 - 2.0 ** -24), 0.0], f32)
    for s in s_in:
        lp_s_acc = (scale * s).astype(f32)
        exp = quant_sym(bias, lp_s_acc, 32)
        s_acc, b32, b_int = run_bias(bias, scale, s)
        assert same(s_acc, lp_s_acc) and same(b32, exp) and same(b_int, exp.astype(f32))
    # with s_in = 2^-11 the last five have s_acc = 2^-31: quotients 2^31, -2^31, 2^31 - 128, -(2^31 - 128), 0
    assert exp[4:].tolist() == [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 128, -(2 ** 31 - 128), 0]
    exp1 = quant_sym(bias, (scale * s_in[0]).astype(f32), 32)
    assert exp1[:4].tolist() == [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31] and abs(float(scale[0] * s_in[0]) - 1e-12) < 1e-15
    s_acc, b32, b_int = run_bias(None, scale, s_in[0])
    assert same(s_acc, (scale * s_in[0]).astype(f32)) and b32 is None and b_int is None
    s_acc, b32, b_int = run_bias(bias, scale, s_in[0], with_int=False)
    assert same(b32, exp1) and b_int is None


# ---------------------------------------------------------------------------- the reference's operator fixture
def test_reference_fixture(golden_dir):
    """the operator KAT recorded from the reference (tests/golden/ops_kat.npz): its QuantLinear's weight_integer, bias_integer and
    scales, and the bias scale of its QuantConv2d (the fixture holds no integers for the convolution)"""
    kat = np.load(os.path.join(golden_dir, "ops_kat.npz"))
    scale, w8, w_int = run_weights(kat["lin_W"])
    assert same(scale, kat["lin_sw"]) and np.array_equal(w8.astype(np.int32), kat["lin_wint"]) and same(w_int, kat["lin_wint"].astype(f32))
    s_acc, b32, b_int = run_bias(kat["lin_b"], scale, kat["lin_sin"])
    assert same(s_acc, kat["lin_sacc"]) and np.array_equal(b32, kat["lin_bint"]) and same(b_int, kat["lin_bint"].astype(f32))
    cW = kat["conv_W"].reshape(kat["conv_W"].shape[0], -1)
    lp = LinearParams(kat["conv_W"], kat["conv_b"], kat["conv_sin"])
    scale, w8, w_int = run_weights(cW, with_int=False)
    assert same(scale, lp.sw) and np.array_equal(w8, lp.W8) and w_int is None
    s_acc, b32, _ = run_bias(kat["conv_b"], scale, kat["conv_sin"])
    assert same(s_acc, kat["conv_sacc"]) and same(b32, lp.b32)


# ---------------------------------------------------------------------------- refusals
def test_refusals():
    """every bad argument returns IVIT_ERR_INVALID before anything is launched: the sentinel-filled outputs stay what they were"""
    L = _lib.lib()
    rows, cols = 6, 40
    r = reference(rows, cols)
    w = t(r["W"])
    b = t(r["b"])
    scale = fenced.output(1, rows, rows, np.float32, sentinel=fenced.SENTINELS[4][0])
    w8 = fenced.output(rows, cols, cols, np.int8, sentinel=fenced.SENTINELS[1][0])
    w_int = fenced.output(rows, cols, cols, np.float32, sentinel=fenced.SENTINELS[4][0])
    s_acc = fenced.output(1, rows, rows, np.float32, sentinel=fenced.SENTINELS[4][0])
    b32 = fenced.output(1, rows, rows, np.int32, sentinel=fenced.SENTINELS[4][0])
    b_int = fenced.output(1, rows, rows, np.float32, sentinel=fenced.SENTINELS[4][0])
    outs = [scale, w8, w_int, s_acc, b32, b_int]
    before = [o.fetch().copy() for o in outs]
    st = _lib.stream_ptr()

    def off(p, n):
        return C.c_void_p(p.value + n)
    wp = C.c_void_p(w.data_ptr())
    good = dict(w=wp, ldw=cols, rows=rows, cols=cols, scale=scale.ptr, w8=w8.ptr, ldo=cols, w_int=w_int.ptr)
    bad_w = {"rows 0": dict(rows=0), "rows negative": dict(rows=-1), "cols 0": dict(cols=0), "ldw below cols": dict(ldw=cols - 1),
             "ldo below cols": dict(ldo=cols - 1), "NULL w": dict(w=None), "NULL scale": dict(scale=None), "NULL w8": dict(w8=None),
             "w misaligned": dict(w=off(wp, 2)), "scale misaligned": dict(scale=off(scale.ptr, 1)), "w_int misaligned": dict(w_int=off(w_int.ptr, 2))}
    for what, change in bad_w.items():
        a = dict(good, **change)
        rc = L.ivit_weight_quant_rows_f32_i8(a["w"], a["ldw"], a["rows"], a["cols"], a["scale"], a["w8"], a["ldo"], a["w_int"], st)
        assert rc == -1, what                                           # IVIT_ERR_INVALID
        assert L.ivit_last_error_string().decode().startswith("ivit_weight_quant_rows_f32_i8"), what
    bp = C.c_void_p(b.data_ptr())
    sc = t(r["scale"])
    goodb = dict(bias=bp, scale=C.c_void_p(sc.data_ptr()), n=rows, s_acc=s_acc.ptr, b32=b32.ptr, b_int=b_int.ptr)
    bad_b = {"n 0": dict(n=0), "n negative": dict(n=-3), "NULL scale": dict(scale=None), "NULL s_acc": dict(s_acc=None),
             "b32 without bias": dict(bias=None, b_int=None), "b_int without bias": dict(bias=None, b32=None),
             "both without bias": dict(bias=None), "bias without b32": dict(b32=None, b_int=None),
             "bias misaligned": dict(bias=off(bp, 2)), "scale misaligned": dict(scale=off(goodb["scale"], 1)),
             "s_acc misaligned": dict(s_acc=off(s_acc.ptr, 2)), "b32 misaligned": dict(b32=off(b32.ptr, 2)),
             "b_int misaligned": dict(b_int=off(b_int.ptr, 1))}
    for what, change in bad_b.items():
        a = dict(goodb, **change)
        rc = L.ivit_bias_quant_f32_i32(a["bias"], a["scale"], a["n"], 0.03, a["s_acc"], a["b32"], a["b_int"], st)
        assert rc == -1, what
        assert L.ivit_last_error_string().decode().startswith("ivit_bias_quant_f32_i32"), what
    with pytest.raises(_lib.IvitError, match="ivit_weight_quant_rows_f32_i8"):
        _lib.call("ivit_weight_quant_rows_f32_i8", wp, cols - 1, rows, cols, scale.ptr, w8.ptr, cols, None, st)
    torch.cuda.synchronize()
    for o, was in zip(outs, before):
        assert np.array_equal(o.fetch(), was)
    # w8 may have any alignment: one byte off, accepted
    w8o = fenced.output(rows, cols, cols + 3, np.int8, expected=r["w8"], lead_bytes=1)
    _lib.call("ivit_weight_quant_rows_f32_i8", wp, cols, rows, cols, scale.ptr, w8o.ptr, cols + 3, None, st)
    fenced.check(w8o, r["w8"])
    fenced.check(scale, r["scale"][None])
