"""Swin with 12 x 12 (and 10 x 10) windows on the GPU: ivit_window_attention_i8_long against the oracle in every Shiftmax form and
both output orders, ivit_avgpool_requant_i8_literal against its host restatement, and IntSwinEngine at 384 px against the
module-by-module path."""
from functools import partial

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.prepare import dyadic, window_shiftexp_band  # noqa: E402
from ivit_amd.swin_engine import pool_literal_host, window_row_map  # noqa: E402
import ivit_amd.quantization_utils as qu  # noqa: E402

DEV = "cuda:0"
_KEEP = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


def sme(pre, z):
    m, e = dyadic(np.float32(pre), np.float32(z))
    return int(m[0]), int(e[0])


def ome(pre, z):
    return orc.dyadic(np.float32(pre), np.float32(z))


GRID = {1: (1, 1), 2: (1, 2), 4: (2, 2)}


def _setup(ws, B_, nW, nH, s_attn, masked, pow2_scores, seed):
    N = ws * ws
    kp = (N + 15) // 16 * 16
    rng = np.random.default_rng(seed)
    hd = 32
    qkv = rng.integers(-128, 128, size=(3, B_, nH, N, hd)).astype(np.int8)
    qkv[0, 0, 0, 0] = 127
    qkv[1, 0, 0] = 127
    s_S = np.float32(2.0 ** -9 * (1.0 if pow2_scores else 0.9))
    s_at = np.float32(s_attn)
    ratio = np.float32(0.5 if pow2_scores else 0.75)
    me = dict(ms=sme(s_S, s_at), omS=ome(s_S, s_at), mb=sme(s_at * ratio, s_at), omB=ome(s_at * ratio, s_at),
              mo=sme(np.float32(2.0 ** -7 * 0.05), 0.043), omO=ome(np.float32(2.0 ** -7 * 0.05), 0.043))
    bias_add = rng.integers(-60, 61, size=(nH, N, N)).astype(np.int16)
    bias_pad = np.full((nH, N, kp), 99, np.int16)      # pad entries must never be used
    bias_pad[:, :, :N] = bias_add
    region = None
    if masked:
        region = np.full((nW, kp), 200, np.uint8)
        region[:, :N] = rng.integers(0, 4, size=(nW, N))
    return qkv, s_at, me, bias_add, bias_pad, region


def _scores(qkv, me, bias_add):
    _, B_, nH, N, _ = qkv.shape
    S = np.einsum("bhqd,bhkd->bhqk", qkv[0].astype(np.int64), qkv[1].astype(np.int64)).astype(np.int32)
    kS = orc.requant(S.reshape(-1, N), me["omS"][0], me["omS"][1], 8).reshape(B_, nH, N, N)
    lin = orc.requant(kS.reshape(-1, N), me["omB"][0], me["omB"][1], 32).reshape(B_, nH, N, N)
    return np.clip(lin + bias_add[None].astype(np.int32), -128, 127)


def _pv(qkv, Pm, me):
    _, B_, nH, N, hd = qkv.shape
    O = np.einsum("bhqk,bhkd->bqhd", Pm.astype(np.int64), qkv[2].astype(np.int64)).astype(np.int32)
    return orc.requant(O.reshape(-1, hd), me["omO"][0], me["omO"][1], 8).reshape(B_, N, nH * hd)


def _call(qkv, out, ld, bias_pad, region, mval, nW, s_at, me, H, W, ws, shift, image_order, phi=None, phim=None, band=None):
    _, B_, nH, N, hd = qkv.shape
    _lib.call("ivit_window_attention_i8_long", _lib.ptr(dev(qkv)), _lib.ptr(out), ld, _lib.ptr(dev(bias_pad)),
              _lib.ptr(None if region is None else dev(region)), mval, B_, nW, nH, N, hd, me["ms"][0], me["ms"][1], me["mb"][0],
              me["mb"][1], float(s_at), me["mo"][0], me["mo"][1], _lib.ptr(None if phi is None else dev(phi)),
              _lib.ptr(None if phim is None else dev(phim)), _lib.ptr(None if band is None else dev(band)),
              0 if band is None else band.shape[1], 0 if band is None else band.shape[0], H, W, ws, shift, image_order, st())


def _both_orders(qkv, ref, bias_pad, region, mval, nW, s_at, me, ws, **tables):
    """window order against the oracle, then image order (every shift the block could have) against the window-ordered rows"""
    _, B_, nH, N, hd = qkv.shape
    gh, gw = GRID[nW]
    H, W = gh * ws, gw * ws
    ld = nH * hd + 32
    out = torch.zeros(B_ * N, ld, dtype=torch.int8, device=DEV)
    _call(qkv, out, ld, bias_pad, region, mval, nW, s_at, me, H, W, ws, 0, 0, **tables)
    got = out.cpu().numpy()
    g32 = got[:, : nH * hd].astype(np.int32).reshape(B_, N, nH * hd)
    assert np.array_equal(g32, ref), f"{(g32 != ref).sum()} of {ref.size} differ"
    assert not got[:, nH * hd:].any()
    for shift in sorted({0, ws // 2}):
        out2 = torch.zeros(B_ * N, ld, dtype=torch.int8, device=DEV)
        _call(qkv, out2, ld, bias_pad, region, mval, nW, s_at, me, H, W, ws, shift, 1, **tables)
        dst = window_row_map(B_ // nW, H, W, ws, shift)
        assert np.array_equal(out2.cpu().numpy(), got[dst]), shift


@pytest.mark.parametrize("ws,B_,nW,nH,s_attn,masked", [(12, 8, 4, 2, 0.25, True), (12, 3, 1, 3, 0.125, False), (10, 8, 4, 2, 0.5, True),
                                                       (10, 2, 1, 2, 0.0625, False), (11, 4, 2, 2, 0.25, True), (9, 2, 2, 1, 1.0, True),
                                                       (12, 8, 4, 2, 2.0 ** -6, True), (12, 4, 4, 2, 2.0 ** -8, True)])
@pytest.mark.parametrize("pow2_scores", [False, True])
def test_window_attention_long_power_of_two(ws, B_, nW, nH, s_attn, masked, pow2_scores):
    """the integer Shiftmax (distance table), the integer shift mask -100 / s; pow2_scores: both score multipliers powers of two
    (the float32 requantisation, RQ32), else float64.  s = 2^-6, 2^-8: x0 = -64, -256, Shiftmax saturates only beyond distance 255,
    where every masked score lies"""
    qkv, s_at, me, bias_add, bias_pad, region = _setup(ws, B_, nW, nH, s_attn, masked, pow2_scores, ws * 1000 + B_)
    N = ws * ws
    kA = _scores(qkv, me, bias_add)
    mval = 0
    if masked:
        mval = int(np.float32(-100.0) / s_at)
        mask_add = np.where(region[:, :N, None] != region[:, None, :N], mval, 0).astype(np.int32)
        kA = (kA.reshape(B_ // nW, nW, nH, N, N) + mask_add[None, :, None]).reshape(B_, nH, N, N)
    Pm = orc.shiftmax(kA, s_at)
    assert Pm.max() > 0
    _both_orders(qkv, _pv(qkv, Pm, me), bias_pad, region, mval, nW, s_at, me, ws)


@pytest.mark.parametrize("ws,B_,nW,nH,s_attn,masked", [(12, 8, 4, 2, 0.271, True), (12, 4, 4, 2, 1.3, True), (10, 8, 4, 2, 0.1173, True),
                                                       (10, 3, 1, 2, 0.3391, False), (12, 8, 4, 2, 0.0613, True),
                                                       (12, 2, 1, 4, 0.1173, False)])
def test_window_attention_long_natural_scale(ws, B_, nW, nH, s_attn, masked):
    """the literal Shiftmax on phi / phi_masked (1.3: -100 / s = -77, a masked score can be the row maximum) and, where the host
    proves it equal, the band table with 256 rows or its one-row form"""
    qkv, s_at, me, bias_add, bias_pad, region = _setup(ws, B_, nW, nH, s_attn, masked, False, ws * 1000 + B_ + 7)
    N = ws * ws
    kA = _scores(qkv, me, bias_add).astype(np.float32)
    maskb = np.zeros((nW, N, N), bool) if region is None else region[:, :N, None] != region[:, None, :N]
    mfull = np.broadcast_to(maskb[None, :, None], (B_ // nW, nW, nH, N, N)).reshape(B_, nH, N, N)
    x = ((kA * s_at).astype(np.float32) + np.where(mfull, np.float32(-100.0), np.float32(0.0))).astype(np.float32)
    xs = (x / s_at).astype(np.float32)
    Pm = orc.shiftmax_xint(xs, s_at)
    ref = _pv(qkv, Pm, me)
    if s_attn == 1.3:        # some row's maximum is a masked score
        plain = np.where(mfull, -np.inf, xs).max(axis=-1)
        assert (xs.max(axis=-1) > plain).any() or (np.isinf(plain)).any()
    qv = np.arange(-128, 128, dtype=np.float32)
    phi = ((qv * s_at).astype(np.float32) / s_at).astype(np.float32)
    phim = ((((qv * s_at).astype(np.float32) + np.float32(-100.0)).astype(np.float32)) / s_at).astype(np.float32)
    _both_orders(qkv, ref, bias_pad, region, -1, nW, s_at, me, ws, phi=phi, phim=phim)
    band, bw = window_shiftexp_band(s_at, masked)
    assert (band is None) == (s_attn == 1.3)
    if band is not None:
        _both_orders(qkv, ref, bias_pad, region, -1, nW, s_at, me, ws, band=band)
        if band.shape[0] == 1:      # the same values as 256 identical rows
            _both_orders(qkv, ref, bias_pad, region, -1, nW, s_at, me, ws, band=np.repeat(band, 256, axis=0))


@pytest.mark.parametrize("tokens,hd,H,ws,band_w,match", [(64, 32, 8, 8, 0, r"failed \(-2\).*unsupported geometry"),
                                                         (169, 32, 13, 13, 0, r"failed \(-2\).*unsupported geometry"),
                                                         (144, 64, 12, 12, 0, r"failed \(-2\).*unsupported geometry"),
                                                         (144, 32, 18, 12, 0, r"failed \(-2\).*do not describe"),
                                                         (144, 32, 12, 12, 24, r"failed \(-2\).*band")])
def test_window_attention_long_argument_errors(tokens, hd, H, ws, band_w, match):
    q = torch.zeros(3 * 169 * 64 + 64, dtype=torch.int8, device=DEV)
    b = torch.zeros(169 * 176 * 2, dtype=torch.int16, device=DEV)
    band = torch.zeros(256 * 32, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_window_attention_i8_long", _lib.ptr(q), _lib.ptr(q), 64, _lib.ptr(b), None, 0, 1, 1, 1, tokens, hd,
                  1 << 30, 40, 1 << 30, 31, 0.25, 1 << 30, 40, None, None, _lib.ptr(band) if band_w else None, band_w, 256 if band_w else 0,
                  H, H, ws, 0, 1, st())


# ----------------------------------------------------------------------------------- literal pooling
def _tie_rows(rng, B, L, C):
    q = rng.integers(-100, 101, size=(B, L, C)).astype(np.int64)
    if L % 2 == 0:
        for b, c in zip(*np.nonzero(rng.random((B, C)) < 0.5)):
            for t in range(int((q[b, :, c].sum() - L // 2) % L)):
                q[b, t % L, c] -= 1
    return q.astype(np.int8)


@pytest.mark.parametrize("B,L,C,s", [(4, 144, 512, 0.0123457), (3, 144, 100, 0.0371), (2, 100, 1024, 0.00917), (5, 49, 72, 0.0211),
                                     (64, 144, 1024, 0.0123457)])
def test_avgpool_literal_against_restatement(B, L, C, s):
    rng = np.random.default_rng(B * L + C)
    q = _tie_rows(rng, B, L, C)
    s = np.float32(s)
    s3 = np.float32(s * np.float32(1.37))
    m, e = sme(s, s3)
    out = torch.empty(B * C, dtype=torch.int8, device=DEV)
    _lib.call("ivit_avgpool_requant_i8_literal", _lib.ptr(dev(q)), _lib.ptr(out), B, L, C, float(s), m, e, st())
    mean = pool_literal_host(q, s)
    z = np.rint((mean / s).astype(np.float32)).astype(np.int32)
    om = ome(s, s3)
    ref = orc.requant(z.reshape(B, C), om[0], om[1], 8)
    got = out.cpu().numpy().astype(np.int32).reshape(B, C)
    assert np.array_equal(got, ref), f"{(got != ref).sum()} of {got.size} differ"
    if L % 2 == 0:       # the float order matters here: the integer mean differs on some tie column
        zi = np.rint(q.astype(np.int64).sum(axis=1) / L).astype(np.int32)
        assert (zi != z).any()


# ----------------------------------------------------------------------------------- engine against the module path
def _images(n, img, g):
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def _calibrated(embed_dim, heads, pow2, seed, img=384, ws=12):
    torch.manual_seed(seed)
    model = ivit.SwinTransformer(img_size=img, patch_size=4, window_size=ws, embed_dim=embed_dim, depths=(2, 2, 2, 2), num_heads=heads,
                                 num_classes=40, norm_layer=partial(qu.IntLayerNorm, eps=1e-6)).to(DEV).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
            elif name.endswith("relative_position_bias_table"):
                p.mul_(20.0)
        g = torch.Generator(device="cpu").manual_seed(seed)
        calib = _images(2, img, g)
        model(calib)
        model(calib.flip(0) * 0.7)
    if pow2:
        for mod in model.modules():
            if isinstance(mod, qu.QuantAct):
                qmax = 2 ** (mod.activation_bit - 1) - 1
                a = max(-float(mod.x_min), float(mod.x_max)) / qmax
                p = 2.0 ** np.ceil(np.log2(a))
                mod.x_max.fill_(qmax * p)
                mod.x_min.fill_(-qmax * p)
    ivit.freeze_model(model)
    return model, g


def _module_run(model, x, lazy_on):
    from ivit_amd.quantization_utils import lazy
    got = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            if isinstance(y, lazy.QT):
                y = y.to_float()
            got[name] = torch.round(y / s).to(torch.int32)
        return fn

    hooks = [mod.register_forward_hook(hook(name)) for name, mod in model.named_modules()
             if isinstance(mod, qu.QuantAct) and name != "act_out"]
    old = lazy.ENABLED
    model.use_engine = False
    try:
        lazy.ENABLED = lazy_on
        y = model(x)
    finally:
        lazy.ENABLED = old
        model.use_engine = True
        for h in hooks:
            h.remove()
    return y, got


def _compare_taps(model, taps, got, names):
    for name in names:
        a, b = taps[name].cpu().numpy().astype(np.int32).reshape(-1), got[name].cpu().numpy().reshape(-1)
        assert a.size == b.size and np.array_equal(a, b), f"tap {name}: {(a != b).sum()} of {a.size} differ"


def _check_tail(model, taps, got, ye, B):
    """qact3 of the engine against torch's CPU pooling (one thread: the serial order) of the engine's own qact2 tap, the logits against
    the module head on that; returns how many qact3 outputs the module path (CUDA's mean: the sum times fl(1 / T)) decides otherwise"""
    s2 = np.float32(model.qact2.act_scaling_factor.reshape(-1)[0].item())
    s3t = model.qact3.act_scaling_factor
    s3 = np.float32(s3t.reshape(-1)[0].item())
    q2 = taps["qact2"].cpu().numpy().astype(np.float32).reshape(B, 144, -1)
    y2 = torch.from_numpy((q2 * s2).astype(np.float32))
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        mean = torch.nn.AdaptiveAvgPool1d(1)(y2.transpose(1, 2))[:, :, 0].numpy()
    finally:
        torch.set_num_threads(prev)
    z = np.rint((mean / s2).astype(np.float32)).astype(np.int32)
    om = ome(s2, s3)
    q3 = orc.requant(z, om[0], om[1], 8)
    assert np.array_equal(taps["qact3"].cpu().numpy().astype(np.int32).reshape(B, -1), q3)
    yh, _ = model.head(torch.from_numpy((q3.astype(np.float32) * s3).astype(np.float32)).to(DEV), s3t)
    assert torch.equal(ye, yh)
    return int((got["qact3"].cpu().numpy().reshape(B, -1) != q3).sum())


@pytest.mark.parametrize("embed_dim,heads", [(64, (2, 4, 8, 16)), (128, (4, 8, 16, 32))])
def test_engine_384_power_of_two_equals_module_path(embed_dim, heads):
    """384 px, 12 x 12 windows: every block on ivit_window_attention_i8_long; the engine equals the int8-carrying and the literal module
    paths bit for bit, taps and logits (the tail also against torch's CPU pooling of the engine's own tap); forward_topk and graph replay
    equal the eager forward.  embed 128: the Swin-B widths"""
    model, g = _calibrated(embed_dim, heads, True, 3 + embed_dim)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    x = _images(2, 384, g)
    with torch.no_grad():
        ye = model(x)
        eng = model._engine[2]
        assert eng.img_size == 384 and not eng.pool_literal and eng.natural_sites == 0
        assert all(b["attn"]["long"] for stg in eng.stages for b in stg["blocks"])
        yl, got = _module_run(model, x, True)
        ym, got_m = _module_run(model, x, False)
        taps = {}
        eng.forward(x.contiguous().float(), taps)
        names = synth.swin_qact_names((2, 2, 2, 2))
        pre = [n for n in names[: names.index("qact2") + 1] if n in taps and n in got]
        _compare_taps(model, taps, got, pre)
        _compare_taps(model, taps, got_m, pre)
        d3 = _check_tail(model, taps, got_m, ye, 2)
    print(f"pow2 C0={embed_dim}: module path (CUDA mean) vs CPU-order pooling: {d3} of {2 * eng.C_last} qact3 outputs differ")
    assert d3 == 0 and torch.equal(ye, ym) and torch.equal(yl, ym)
    assert not torch.equal(ye[0], ye[1]) and ye.abs().max() > 0
    xi = x.contiguous().float()
    li, lf, t1 = (t.clone() for t in eng.forward(xi))
    assert torch.equal(lf, ye)
    ki, kf, tk = (t.clone() for t in eng.forward_topk(xi, k=5))
    assert torch.equal(ki, li) and torch.equal(kf, lf) and torch.equal(tk[:, 0], t1)
    gi, gf, gt = (t.clone() for t in eng.forward_graph(xi))
    assert torch.equal(gi, li) and torch.equal(gf, lf) and torch.equal(gt, t1)
    torch.cuda.synchronize()


def test_engine_384_natural_scales():
    """calibrated (natural) ranges: the taps through the pre-pool qact2 equal the module path; qact3 and the logits equal torch's CPU
    pooling of the engine's own qact2 tap followed by the module head.  (The module path pools with CUDA's mean, whose order can
    decide a .5 tie differently; the engine restates the CPU order.)"""
    model, g = _calibrated(64, (2, 4, 8, 16), False, 21)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    x = _images(3, 384, g)
    with torch.no_grad():
        ye = model(x)
        eng = model._engine[2]
        assert eng.pool_literal and eng.natural_sites > 0
        taps = {}
        eng.forward(x.contiguous().float(), taps)
        ym, got = _module_run(model, x, False)
        names = synth.swin_qact_names((2, 2, 2, 2))
        _compare_taps(model, taps, got, [n for n in names[: names.index("qact2") + 1] if n in taps and n in got])
        d3 = _check_tail(model, taps, got, ye, 3)
    print(f"natural: module path (CUDA mean) vs CPU-order pooling: {d3} of {3 * eng.C_last} qact3 outputs differ; "
          f"logits equal: {torch.equal(ye, ym)}")
