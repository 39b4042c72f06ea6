"""Feature maps (forward_intermediates): the four ivit_tokens_to_nchw_* entries against numpy bit for bit -- partial tiles in both
directions, strided fenced sources down to the element's own alignment (the scalar loads) and 16- / 8- / 4-byte aligned ones (the
vector loads), sentinel-filled fenced outputs, every argument error -- and the engine / model methods of DeiT / ViT and Swin against
the engines' own taps, against the module path with forward hooks (the reference's tensor), with the logits and the launches of the
plain forward unchanged."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import tokens_to_nchw  # noqa: E402
from ivit_amd.swin_engine import engine_from_model  # noqa: E402

import fenced  # noqa: E402
import test_gpu_swin_ibert_lazy as swin_ibert  # noqa: E402
import test_gpu_swin_lazy as swin_lazy  # noqa: E402
from test_gpu_vit16_lazy import W8, W16, _calibrated, _images  # noqa: E402
from test_gpu_w4_lazy import W4, _calibrated as _calibrated_w4  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
ENTRIES = {"ivit_tokens_to_nchw_i8_f32": (np.int8, np.float32), "ivit_tokens_to_nchw_i16_f32": (np.int16, np.float32),
           "ivit_tokens_to_nchw_i8": (np.int8, np.int8), "ivit_tokens_to_nchw_i16": (np.int16, np.int16)}
# (B, T_all, t0, T, C): smallest possible; ViT class-token offset; one whole tile; one over in both directions; DeiT-T geometry;
# channels no multiple of 16 with an odd token offset; Swin stage 0 at 224 px (49 token tiles, C = 96)
SHAPES = [(1, 1, 0, 1, 1), (2, 5, 1, 4, 64), (2, 64, 0, 64, 64), (1, 65, 0, 65, 65), (3, 197, 1, 196, 192), (2, 130, 2, 127, 200),
          (1, 3136, 0, 3136, 96)]
SCALES = (f32(2.0 ** -4), f32(0.0571))


def st():
    return _lib.stream_ptr()


def _source(shape, dtype, seed):
    """full-range random integers [B, T_all, C] (the rows outside the selection too), the extremes in the first and the last element
    of the selection"""
    B, T_all, t0, T, C = shape
    info = np.iinfo(dtype)
    q = np.random.default_rng(seed).integers(info.min, info.max + 1, size=(B, T_all, C)).astype(dtype)
    q[0, t0, 0] = info.min
    q[B - 1, t0 + T - 1, C - 1] = info.max
    return q


def _expected(q, shape, out_dtype, s):
    B, T_all, t0, T, C = shape
    sel = np.ascontiguousarray(q[:, t0:t0 + T].transpose(0, 2, 1))
    return sel.astype(f32) * f32(s) if out_dtype == np.float32 else sel


def _layouts(C, item):
    """(ldx, lead_bytes) of the source: C + 3 at the allocation's alignment and at the smallest one the element admits (element
    loads, but for a C + 3 that happens to be a multiple of four bytes), then rows whose stride and start are multiples of 16, 8
    and 4 bytes only (the three vector loads)"""
    row16 = (C * item + 15) // 16 * 16
    return [(C + 3, 0), (C + 3, item)] + [((row16 + 16 + extra) // item, 0) for extra in (0, 8, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}_Tall{}_t0{}_T{}_C{}".format(*s))
def test_entries_against_numpy_fenced(shape):
    B, T_all, t0, T, C = shape

    def run(name, x, s, o):
        if name == "ivit_tokens_to_nchw_i8_f32":
            _lib.call("ivit_tokens_to_nchw_i8_f32", x.ptr, x.ld, B, T_all, t0, T, C, float(s), o.ptr, st())
        elif name == "ivit_tokens_to_nchw_i16_f32":
            _lib.call("ivit_tokens_to_nchw_i16_f32", x.ptr, x.ld, B, T_all, t0, T, C, float(s), o.ptr, st())
        elif name == "ivit_tokens_to_nchw_i8":
            _lib.call("ivit_tokens_to_nchw_i8", x.ptr, x.ld, B, T_all, t0, T, C, o.ptr, st())
        else:
            _lib.call("ivit_tokens_to_nchw_i16", x.ptr, x.ld, B, T_all, t0, T, C, o.ptr, st())

    for name, (di, do) in ENTRIES.items():
        item = np.dtype(di).itemsize
        q = _source(shape, di, seed=sum(shape) + item)
        for k, (ldx, lead) in enumerate(_layouts(C, item)):
            for s in (SCALES if do == np.float32 else (None,)):
                exp = _expected(q, shape, do, s).reshape(B * C, T)
                x = fenced.input(q.reshape(B * T_all, C), ldx, fenced.POISON[np.dtype(di)], lead_bytes=lead)
                # the destination once off the allocation's alignment too: dense rows, aligned to the element alone
                o = fenced.output(B * C, T, T, do, expected=exp, lead_bytes=np.dtype(do).itemsize if k == 1 else 0)
                run(name, x, s, o)
                torch.cuda.synchronize()
                fenced.check(o, exp)
                fenced.check(x)


def test_float_forms_are_torchs_multiplication():
    """q.float() * s of torch, bit for bit, at a natural scale over every int16 value"""
    q = torch.arange(-32768, 32768, dtype=torch.int16, device=DEV).view(1, 512, 128)
    out = torch.empty(1, 128, 512, dtype=torch.float32, device=DEV)
    s = float(SCALES[1])
    tokens_to_nchw(q, 128, 1, 512, 0, 512, 128, s, out, st())
    want = q.permute(0, 2, 1).float().mul(s).contiguous()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_argument_errors_launch_nothing():
    L = _lib.lib()
    B, T_all, t0, T, C = 2, 9, 1, 8, 24
    for name, (di, do) in ENTRIES.items():
        fn = getattr(L, name)
        x = torch.zeros(B * T_all * (C + 2) + 8, dtype=getattr(torch, np.dtype(di).name), device=DEV)
        exp = np.zeros((B * C, T), do)
        o = fenced.output(B * C, T, T, do, expected=exp)
        scale = (ctypes.c_float(0.5),) if do == np.float32 else ()
        xi, oi = np.dtype(di).itemsize, np.dtype(do).itemsize

        def rc(xp=x.data_ptr(), ldx=C + 2, B=B, T_all=T_all, t0=t0, T=T, C=C, op=None):
            op = o.t.data_ptr() + o.start if op is None else op
            return fn(ctypes.c_void_p(xp), ldx, B, T_all, t0, T, C, *scale, ctypes.c_void_p(op), st())

        # NULL x, NULL out, B / T / C below 1, t0 < 0, t0 + T > T_all (twice), ldx < C
        bad = [rc(xp=0), rc(op=0), rc(B=0), rc(T=0), rc(C=0), rc(t0=-1), rc(t0=2), rc(T=T_all), rc(ldx=C - 1)]
        if xi > 1:
            bad.append(rc(xp=x.data_ptr() + 1))
        if oi > 1:
            bad.append(rc(op=o.t.data_ptr() + o.start + 1))
        assert bad == [-1] * len(bad), (name, bad)       # IVIT_ERR_INVALID
        assert name in L.ivit_last_error_string().decode()
        torch.cuda.synchronize()
        assert (o.fetch() == o.host).all(), f"{name}: a refused call wrote to the sentinel-filled output"
        assert rc() == 0                                  # the same arguments, unbroken
        torch.cuda.synchronize()
        fenced.check(o, exp)


# =========================================================================================== DeiT / ViT
class _Calls:
    """the names _lib.call is asked for, calling through"""

    def __enter__(self):
        self.names, self.orig = [], _lib.call
        _lib.call = lambda name, *a: (self.names.append(name), self.orig(name, *a))[1]
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig
        return False


def _fallback(model, x, indices=None, integers=False):
    model.use_engine = False
    try:
        assert not model.takes_engine(x)
        return model.forward_intermediates(x, indices, integers)
    finally:
        model.use_engine = True


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def _from_tap(tap, t0, hw, s):
    """[B, T, C] integers of a tap -> the float map, by numpy"""
    q = tap.cpu().numpy()
    q = q.reshape(q.shape[0], -1, q.shape[-1])[:, t0:]
    m = np.ascontiguousarray(q.transpose(0, 2, 1)).astype(f32) * f32(s)
    return m.reshape(m.shape[0], m.shape[1], *hw)


_MODELS = {}


def _vit(img, depth, family, widths, pow2):
    """the calibrated, frozen model, built once per configuration and shared -- no test changes it for good"""
    key = (img, depth, family, id(widths), pow2)
    if key not in _MODELS:
        make = _calibrated_w4 if widths is W4 else _calibrated      # the 4-bit twin of the helper draws a class token 4 bits can hold
        _MODELS[key] = make(img, 16, 128, depth, 2, pow2, 11, family, widths)
    return _MODELS[key]


VIT_CASES = {
    "ivit64_natural": (64, 3, 3, "ivit", W8, False), "ivit64_pow2": (64, 3, 3, "ivit", W8, True), "ivit80": (80, 3, 3, "ivit", W8, False),
    "w16": (64, 3, 3, "ivit", W16, False), "w4": (64, 3, 3, "ivit", W4, False), "ibert224": (224, 1, 2, "ibert", W8, False)}


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_vit_engine_maps(case):
    img, depth, B, family, widths, pow2 = VIT_CASES[case]
    G = img // 16
    model, g = _vit(img, depth, family, widths, pow2)
    assert model.engine_unsupported_reason() is None
    x = _images(B, img, g)
    with torch.no_grad():
        y = model(x)
        assert model.takes_engine(x)
        eng = model.engine(B)
        wide = eng.stream_bits == 16
        assert eng.stream_bits == {id(W8): 8, id(W16): 16, id(W4): 4}[id(widths)]
        taps = None
        if not wide:
            taps = {}
            eng.forward(x.contiguous(), taps=taps)
        for indices in (None, (depth - 1, 0) if depth > 1 else (0,)):
            idx = list(range(depth)) if indices is None else list(indices)
            maps, scales = eng.forward_intermediates(x.contiguous(), indices)
            logits = eng.ws["logits_f"][:B, :eng.num_classes].clone()
            ints, scales_i = eng.forward_intermediates(x.contiguous(), indices, integers=True)
            m_maps, m_scales = model.forward_intermediates(x, indices)
            ref, ref_s = _fallback(model, x, indices)
            ref_i, ref_si = _fallback(model, x, indices, integers=True)
            assert list(maps) == list(ints) == list(m_maps) == list(ref) == list(ref_i) == idx
            assert scales == scales_i == m_scales == ref_s == ref_si and list(scales) == idx
            assert torch.equal(logits, y), "the logits left in the workspace"
            for i in idx:
                s_mod = model.blocks[i].qact4.act_scaling_factor.reshape(-1)
                assert isinstance(scales[i], float) and s_mod.dtype == torch.float32 and scales[i] == float(s_mod[0])
                assert maps[i].dtype == torch.float32 and tuple(maps[i].shape) == (B, 128, G, G) and maps[i].is_contiguous()
                assert ints[i].dtype == (torch.int16 if wide else torch.int8) and ints[i].shape == maps[i].shape
                if taps is not None:
                    want = _from_tap(taps[f"blocks.{i}.qact4"], 1, (G, G), scales[i])
                    assert np.array_equal(maps[i].cpu().numpy().view(np.int32), want.view(np.int32)), f"block {i} against the tap"
                assert _same(maps[i], ref[i]), f"block {i}: {int((maps[i] != ref[i]).sum())} of {maps[i].numel()} differ from the module path"
                assert _same(ints[i], ref_i[i]) and _same(m_maps[i], maps[i])
                assert len(torch.unique(ints[i])) > 4, "a live stream"
        assert torch.equal(model(x), y)


# =========================================================================================== Swin
def _swin_check(model, x, eng, taps):
    """engine maps against the engine's taps (where given), against the module path with hooks, logits left as forward() leaves them"""
    B, nst = x.shape[0], len(model.depths)
    with torch.no_grad():
        y = eng.forward(x.contiguous())[1].clone()
        for indices in (None, (nst - 1, 0) if nst > 1 else (0,)):
            idx = list(range(nst)) if indices is None else list(indices)
            maps, scales = eng.forward_intermediates(x.contiguous(), indices)
            logits = eng.ws["logits_f"][:B, :eng.num_classes].clone()
            ints, scales_i = eng.forward_intermediates(x.contiguous(), indices, integers=True)
            ref, ref_s = _fallback(model, x, indices)
            ref_i, ref_si = _fallback(model, x, indices, integers=True)
            assert list(maps) == list(ints) == list(ref) == list(ref_i) == idx and scales == scales_i == ref_s == ref_si
            assert torch.equal(logits, y)
            for li in idx:
                H, W = model.layers[li].input_resolution
                C = model.embed_dim * 2 ** li
                last = model.layers[li].blocks[-1]
                assert scales[li] == float(last.qact4.act_scaling_factor.reshape(-1)[0])
                assert maps[li].dtype == torch.float32 and tuple(maps[li].shape) == (B, C, H, W) and ints[li].dtype == torch.int16
                if taps is not None:
                    want = _from_tap(taps[f"layers.{li}.blocks.{model.depths[li] - 1}.qact4"].view(B, H * W, C), 0, (H, W), scales[li])
                    assert np.array_equal(maps[li].cpu().numpy().view(np.int32), want.view(np.int32)), f"stage {li} against the tap"
                assert _same(maps[li], ref[li]), f"stage {li}: {int((maps[li] != ref[li]).sum())} of {maps[li].numel()} differ from the module path"
                assert _same(ints[li], ref_i[li]) and len(torch.unique(ints[li])) > 16


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_engine_maps_model_a(pow2):
    model, x = swin_lazy.built("A", pow2)
    assert model.engine_unsupported_reason() is None and model.takes_engine(x)
    eng = model.engine(x.shape[0])
    taps = {}
    with torch.no_grad():
        eng.forward(x.contiguous(), taps=taps)
        _swin_check(model, x, eng, taps)
        m_maps, m_scales = model.forward_intermediates(x, (1, 0))
        e_maps, e_scales = eng.forward_intermediates(x.contiguous(), (1, 0))
    assert m_scales == e_scales and all(_same(m_maps[li], e_maps[li]) for li in (1, 0))


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_model_b_takes_the_hooks(pow2):
    """model B (96 px, 144-token windows) ends with 96 features, which no fused Swin engine takes (the classifier GEMM): its
    forward_intermediates is the module path.  Its map against the module path's own qact4 integers (tests/test_gpu_swin_lazy.py
    module_run), by numpy and through the engines' launcher on those integers"""
    model, x = swin_lazy.built("B", pow2)
    assert model.engine_unsupported_reason() is not None
    B, (H, W), C = x.shape[0], model.layers[0].input_resolution, model.embed_dim
    taps = {}
    swin_lazy.module_run(model, x, True, taps)
    with torch.no_grad():
        maps, scales = model.forward_intermediates(x)
        ints, _ = model.forward_intermediates(x, (0,), integers=True)
    tap = taps["layers.0.blocks.1.qact4"].reshape(B, H * W, C)
    assert list(maps) == [0] and scales[0] == float(model.layers[0].blocks[-1].qact4.act_scaling_factor.reshape(-1)[0])
    want = _from_tap(tap, 0, (H, W), scales[0])
    assert np.array_equal(maps[0].cpu().numpy().view(np.int32), want.view(np.int32))
    assert ints[0].dtype == torch.int16 and torch.equal(ints[0].to(torch.int32), tap.permute(0, 2, 1).reshape(B, C, H, W))
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=DEV)
    tokens_to_nchw(tap.to(torch.int16).contiguous(), C, B, H * W, 0, H * W, C, scales[0], out, st())
    assert _same(out, maps[0])


def test_swin_ibert_engine_maps():
    model, x = swin_ibert.built("A", False)
    assert "operator family" in model.engine_unsupported_reason()
    eng = engine_from_model(model, max_batch=4)
    assert eng.family == "ibert"
    _swin_check(model, x, eng, None)


# =========================================================================================== errors, the default path
def test_bad_indices_raise_before_anything_is_launched():
    model, g = _vit(64, 3, "ivit", W8, False)
    x = _images(2, 64, g)
    smodel, sx = swin_lazy.built("A", False)
    with torch.no_grad():
        eng, seng = model.engine(2), smodel.engine(sx.shape[0])
        with _Calls() as c:
            for target, arg, n in ((eng, x.contiguous(), 3), (model, x, 3), (seng, sx.contiguous(), 2), (smodel, sx, 2)):
                for bad in ((n,), (-1,), (1, 1)):
                    with pytest.raises(ValueError, match="indices"):
                        target.forward_intermediates(arg, bad)
            model.use_engine = False
            try:
                with pytest.raises(ValueError, match="indices"):
                    model.forward_intermediates(x, (3,))
            finally:
                model.use_engine = True
        assert c.names == []


def test_the_plain_forward_is_unchanged():
    model, g = _vit(64, 3, "ivit", W8, False)
    smodel, sx = swin_lazy.built("A", False)
    for m, x in ((model, _images(3, 64, g)), (smodel, sx)):
        x = x.contiguous()
        with torch.no_grad():
            eng = m.engine(x.shape[0])
            with _Calls() as before:
                y0 = eng.forward(x)[1].clone()
            keys = {k: (v.data_ptr(), v.numel()) for k, v in eng.ws.items() if torch.is_tensor(v)}
            with _Calls() as between:
                eng.forward_intermediates(x)
                eng.forward_intermediates(x, (0,), integers=True)
            with _Calls() as after:
                y1 = eng.forward(x)[1].clone()
        added = [n for n in between.names if n.startswith("ivit_tokens_to_nchw")]
        n_all = len(eng.blocks) if hasattr(eng, "blocks") else len(eng.stages)
        assert len(added) == n_all + 1 and [n for n in between.names if n not in added] == before.names * 2
        assert after.names == before.names and not [n for n in before.names if n.startswith("ivit_tokens_to_nchw")]
        assert torch.equal(y0, y1)
        assert keys == {k: (v.data_ptr(), v.numel()) for k, v in eng.ws.items() if torch.is_tensor(v)}, "the workspace is the same buffers"
