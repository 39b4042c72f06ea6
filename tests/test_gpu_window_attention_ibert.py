"""ivit_window_attention_i8_ibert (Swin's WindowAttention with IBERTIntSoftmax(8)) against a CPU restatement: integer matmuls, the
oracle's dyadic requantisation (oracle.requant), and the I-BERT softmax of oracle/ibert.py line by line on the float view the
reference's tensor holds -- fl(q * s), minus 100 under the shift mask -- with its row sum in torch's CPU order (oracle.torch_rowsum),
all in numpy.  Bit-exact, no tolerance.

Every case holds, beside random windows, queries with one dominant score (a one-hot row: p = 128, one more than an int8 operand holds)
and queries whose scores are the bias alone (near-flat rows).  The scales sit on both sides of the mask precondition
(prepare.ibert_window_mask_ok, about s_attn <= 0.29): on the refused side the host proof says no and nothing is launched."""
import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import ibert_window_mask_ok  # noqa: E402
from ivit_amd.swin_engine import (key_pad, shift_mask_regions, window_attention_ibert, window_attention_ibert_spec,  # noqa: E402
                                  window_row_map)

DEV = "cuda:0"
f32 = np.float32
HD = 32
# (s_S, s_at, s_A = s_attn, s_tab, s_qkv, s_a3): the scores' scale, qact_attn1, qact2, the bias table, qkv, qact3
SCALES = {"pow2": (2.0 ** -12, 2.0 ** -2, 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -5),
          "natural": (3.1e-4, 0.0731, 0.1173, 0.0317, 0.061, 0.043),
          "fine": (1.7e-4, 0.0291, 0.0391, 0.0211, 0.047, 0.037),       # 30 |x0_int| > 255: no unmasked score reaches the clamp
          "clipped": (3.1e-4, 0.0731, 0.1173, 0.0317, 0.061, 0.043)}    # "natural" with a clipped internal QuantAct: see act_range
REFUSED = {"pow2": 0.5, "natural": 0.37}
# (heads, windows per image, images, shifted, image order, form): every value of each axis the issue lists, in six launches
COMBOS = [(1, 1, 2, False, False, "table"), (3, 4, 2, True, False, "band"), (3, 1, 1, True, True, "table"),
          (1, 4, 1, False, True, "band"), (3, 4, 1, True, True, "table"), (1, 1, 3, True, False, "band")]


def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def act_range(s_A, regime):
    """range of the softmax's internal QuantAct(16): what a calibration pass leaves (the row maximum's c_int * 2^30); "pow2": the
    next range whose scale is a power of two; "clipped": 2^-15 of it -- most exponents then clamp at 32767 and, what no calibrated
    range does, the saturated value of a masked score is not 0"""
    emax = float(ib.softmax_constants(f32(s_A), 0.0, 1.0)[2]) * 2.0 ** 30
    if regime == "pow2":
        return (0.0, 32767 * 2.0 ** np.ceil(np.log2(emax / 32767)))
    return (0.0, emax * 2.0 ** -15 if regime == "clipped" else emax)


def make_inputs(N, nH, nwin, seed):
    rng = np.random.default_rng(seed)
    qkv = rng.integers(-128, 128, size=(3, nwin, nH, N, HD), dtype=np.int64).astype(np.int8)
    # window 0: key 0 dominates every query of the first half (scores saturate at +127 / -128); the second half has q = 0 (bias alone)
    qkv[0, 0, :, :N // 2] = 127
    qkv[0, 0, :, N // 2:] = 0
    qkv[1, 0, :, 0] = 127
    qkv[1, 0, :, 1:] = -127
    bias = rng.integers(-40, 41, size=(nH, N, N)).astype(np.int32)
    bias[:, N // 2:] = rng.integers(-2, 3, size=(nH, N - N // 2, N))        # near-flat rows
    return qkv, bias


def regions(N, nW, shifted, rng):
    if not shifted:
        return None
    ws = int(round(N ** 0.5))
    if ws * ws == N:
        side = ws * int(round(nW ** 0.5))
        return shift_mask_regions(side, side, ws, max(ws // 2, 1)).astype(np.uint8)
    return rng.integers(0, 3, size=(nW, N)).astype(np.uint8)          # no window geometry: any region table


def ibert_softmax_float_view(x, s, lo, hi):
    """oracle/ibert.py softmax (:303-314, output_bit 8) on the float view x itself, row sums in torch's order -> p in [0, 128]"""
    s = f32(s)
    n = 30
    x0_int, b_int, c_int, exp_sf, act_sf, m, e = ib.softmax_constants(s, lo, hi)
    x_int = (x.astype(f32) / s).astype(f32)
    x_int = (x_int - x_int.max(axis=-1, keepdims=True)).astype(f32)
    x_int = np.maximum(x_int, f32(n * x0_int)).astype(f32)
    q = np.floor((x_int / x0_int).astype(f32))
    r = (x_int - (x0_int * q).astype(f32)).astype(f32)
    z = ((r * (r + b_int).astype(f32)).astype(f32) + c_int).astype(f32)
    ex = np.maximum(np.floor((z * np.exp2((n - q).astype(f32)).astype(f32)).astype(f32)), f32(0))
    z_int = np.rint((ex / exp_sf).astype(f32))
    q16 = np.clip(np.rint(z_int.astype(np.float64) * m / 2.0 ** e), -32768, 32767).astype(f32)
    exp_int = ((q16 * act_sf).astype(f32) / act_sf).astype(f32)
    flat = exp_int.reshape(-1, exp_int.shape[-1])
    ssum = np.array([orc.torch_rowsum(row) for row in flat], f32).reshape(*exp_int.shape[:-1], 1)
    factor = np.floor((f32(2 ** 32) / ssum).astype(f32))
    return np.floor(((exp_int * factor).astype(f32) / f32(2 ** 25)).astype(f32)).astype(np.int64)


def reference(qkv, bias, region, nW, sc, rng_act):
    """[nwin, N, nH * 32] int8 in window order, and the probabilities"""
    s_S, s_at, s_A, s_tab, s_qkv, s_a3 = sc
    q, k, v = (t.astype(np.int64) for t in qkv)
    nwin, nH, N, _ = q.shape
    S = np.einsum("whid,whjd->whij", q, k).astype(np.int32)
    kS = orc.requant(S, *orc.dyadic(s_S, s_at), 8)                                              # qact_attn1
    b = np.broadcast_to(bias[None], S.shape).astype(np.int32)
    ka = orc.requant(kS, *orc.dyadic(s_at, s_A), 8, b, *orc.dyadic(s_tab, s_A))                # qact2 with the bias as identity
    x = (ka.astype(f32) * f32(s_A)).astype(f32)
    if region is not None:
        reg = region[np.arange(nwin) % nW]                                                      # [nwin, N]
        masked = reg[:, None, :, None] != reg[:, None, None, :]
        x = np.where(masked, (x + f32(-100.0)).astype(f32), x)                                  # swin_quant.py:149-155
    p = ibert_softmax_float_view(x, s_A, *rng_act)
    O = np.einsum("whij,whjd->whid", p, v).astype(np.int32)
    o = orc.requant(O, *orc.dyadic(f32(f32(2.0 ** -7) * f32(s_qkv)), s_a3), 8)
    return o.transpose(0, 2, 1, 3).reshape(nwin, N, nH * HD).astype(np.int8), p


def launch(spec, qkv, nH, nwin, nW, N, image_order, shifted):
    ws = int(round(N ** 0.5))
    geo = (0, 0, 0, 0)
    if ws * ws == N:
        side = ws * int(round(nW ** 0.5))
        geo = (side, side, ws, max(ws // 2, 1) if shifted else 0)
    C = nH * HD
    out = torch.full((nwin * N, C), 99, dtype=torch.int8, device=DEV)
    window_attention_ibert(spec, upload(qkv), out, C, nwin, nW, nH, N, *geo, image_order, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), geo


@pytest.mark.parametrize("regime", ["pow2", "natural", "fine", "clipped"])
@pytest.mark.parametrize("N", [2, 49, 64, 65, 144])
def test_window_attention_ibert_equals_the_restatement(N, regime):
    sc = SCALES[regime]
    s_S, s_at, s_A, s_tab, s_qkv, s_a3 = sc
    rng_act = act_range(s_A, regime)
    square = int(round(N ** 0.5)) ** 2 == N
    saw128 = flat = False
    for ci, (nH, nW, imgs, shifted, image_order, form) in enumerate(COMBOS):
        nwin = nW * imgs
        rng = np.random.default_rng(1000 * N + ci)
        qkv, bias = make_inputs(N, nH, nwin, 7 * N + ci)
        region = regions(N, nW, shifted, rng)
        assert region is None or ibert_window_mask_ok(s_A, ib.softmax_constants(f32(s_A), *rng_act)[0])
        want, p = reference(qkv, bias, region, nW, sc, rng_act)
        saw128 |= bool((p == 128).any())
        flat |= bool((p.max(axis=-1) <= max(4, 512 // N)).any())
        spec = window_attention_ibert_spec(upload, DEV, _lib.stream_ptr(), bias, f32(s_tab), f32(s_S), f32(s_at), f32(s_A),
                                           f32(f32(2.0 ** -7) * f32(s_qkv)), f32(s_a3), region, N, rng_act, form=form)
        assert spec is not None and (spec["band_w"] > 0) == (form == "band") and spec["bias"].shape[-1] == key_pad(N)
        image_order = image_order and square
        got, geo = launch(spec, qkv, nH, nwin, nW, N, image_order, shifted)
        want = want.reshape(nwin * N, nH * HD)
        if image_order:      # rows at their image positions: window reverse + roll back
            rows = window_row_map(imgs, geo[0], geo[1], geo[2], geo[3])
            want = want[rows]
        assert np.array_equal(got, want), (N, regime, ci, int((got != want).sum()), got.size)
    # p = 128 needs fl(e_max * floor(2^32 / e_max)) = 2^32: the calibrated range's e_max = 32767 gives it, a power-of-two or clipped
    # range need not, and at the fine scale no exponent reaches the clamp within 255 steps of the maximum
    assert (saw128 or regime != "natural") and flat, "the inputs must reach p = 128 and hold a near-flat row"


@pytest.mark.parametrize("regime", ["pow2", "natural"])
def test_mask_beyond_the_precondition_is_refused_on_the_host(regime):
    """s_attn above 0.31: a masked score does not reach int_exp's clamp for every row maximum -- the proof says no, the spec is None
    and no window attention is launched; without a mask the same scale is served"""
    s_S, s_at, _, s_tab, s_qkv, s_a3 = SCALES[regime]
    s_A = REFUSED[regime]
    rng_act = act_range(s_A, regime)
    assert not ibert_window_mask_ok(s_A, ib.softmax_constants(f32(s_A), *rng_act)[0])
    N, nH, nW = 49, 3, 4
    qkv, bias = make_inputs(N, nH, nW, 5)
    region = regions(N, nW, True, None)
    launched, real_call = [], _lib.call
    try:
        _lib.call = lambda name, *a: (launched.append(name), real_call(name, *a))[1]
        spec = window_attention_ibert_spec(upload, DEV, _lib.stream_ptr(), bias, f32(s_tab), f32(s_S), f32(s_at), f32(s_A),
                                           f32(s_qkv / 128), f32(s_a3), region, N, rng_act)
    finally:
        _lib.call = real_call
    assert spec is None and not [n for n in launched if "window_attention" in n], launched
    sc = (s_S, s_at, s_A, s_tab, s_qkv, s_a3)
    want, _ = reference(qkv, bias, None, nW, sc, rng_act)
    spec = window_attention_ibert_spec(upload, DEV, _lib.stream_ptr(), bias, f32(s_tab), f32(s_S), f32(s_at), f32(s_A),
                                       f32(f32(2.0 ** -7) * f32(s_qkv)), f32(s_a3), None, N, rng_act)
    got, _ = launch(spec, qkv, nH, nW, nW, N, False, False)
    assert np.array_equal(got, want.reshape(nW * N, nH * HD))


def test_window_attention_ibert_argument_errors():
    nwin, nH, N = 4, 3, 49
    qkv = torch.zeros(3, nwin, nH, N, HD, dtype=torch.int8, device=DEV)
    out = torch.zeros(nwin * N, nH * HD, dtype=torch.int8, device=DEV)
    bias = torch.zeros(nH, N, 64, dtype=torch.int16, device=DEV)
    region = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    table = torch.ones(65536 + 4, dtype=torch.float32, device=DEV)
    p = _lib.ptr

    def call(qkv_=qkv, out_=out, bias_=bias, table_=p(table), tokens=N, hd=HD, band_w=0, geo=(14, 14, 7, 3), order=0, wpi=4, sat=1.0):
        _lib.call("ivit_window_attention_i8_ibert", p(qkv_), p(out_), nH * HD, p(bias_), p(region), sat, nwin, wpi, nH, tokens, hd,
                  1 << 30, 30, 1 << 30, 30, 1 << 30, 30, table_, band_w, *geo, order, _lib.stream_ptr())

    for kw in (dict(tokens=1), dict(tokens=145), dict(hd=64)):
        with pytest.raises(_lib.IvitError, match="unsupported geometry"):
            call(**kw)
    for kw in (dict(geo=(14, 14, 6, 3)), dict(geo=(14, 14, 7, 7)), dict(geo=(14, 21, 7, 3)), dict(wpi=2)):
        with pytest.raises(_lib.IvitError, match="do not describe"):
            call(**kw)
    for kw in (dict(qkv_=None), dict(out_=None), dict(bias_=None), dict(table_=None)):
        with pytest.raises(_lib.IvitError, match="NULL operand"):
            call(**kw)
    with pytest.raises(_lib.IvitError, match="bad band table"):
        call(band_w=24)
    with pytest.raises(_lib.IvitError, match="misaligned table"):
        call(table_=table.data_ptr() + 4, band_w=64)
    with pytest.raises(_lib.IvitError, match="image_order"):
        call(geo=(0, 0, 0, 0), order=1)
    with pytest.raises(_lib.IvitError, match="masked_exp"):
        call(sat=-1.0)
    call()                                  # and the same call with nothing wrong is served, in both orders
    call(order=1)
    call(geo=(0, 0, 0, 0))
    torch.cuda.synchronize()
