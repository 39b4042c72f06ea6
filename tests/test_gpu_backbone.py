"""Backbone mode: ivit_dequant_rows_i8_f32 against numpy bit for bit (dense, fenced and strided, off the 16-byte alignment on both
sides, every refused argument); forward_features of both engines against their own taps and against the module path (the
reference's tensor); `out=` into a slice of a feature bank; headless models; forward_intermediates_early (the early stop); the feature
graph next to the logits graph; extract_features over an uneven last batch.

Models are those of the suite's other model-path checks (tests/test_gpu_vit16_lazy.py::_calibrated, tests/test_gpu_swin_lazy.py::built):
ViT embed_dim 128, depth 2, 2 heads; Swin 56 px, 7 x 7 windows, depths (2, 2); B = 3; ranges as calibrated and rounded up to powers
of two.  The DeiT-T CRC case runs the synthetic golden model of tests/golden/."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.inference import extract_features  # noqa: E402
from ivit_amd.swin_engine import engine_from_model  # noqa: E402

import fenced  # noqa: E402
import test_gpu_swin_ibert_lazy as swin_ibert  # noqa: E402
import test_gpu_swin_lazy as swin_lazy  # noqa: E402
from test_gpu_model import crc  # noqa: E402
from test_gpu_vit16_lazy import W8, W16  # noqa: E402
from test_gpu_w4_lazy import W4, _small as _small_w4  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
B = 3


def st():
    return _lib.stream_ptr()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


class Calls:
    """the names _lib.call is asked for, calling through"""

    def __enter__(self):
        self.names, self.orig = [], _lib.call
        _lib.call = lambda name, *a: (self.names.append(name), self.orig(name, *a))[1]
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig
        return False


# =========================================================================================== the kernel
ROWS, CS, SCALES = (1, 3, 257), (1, 15, 16, 17, 192, 1000), (f32(2.0 ** -5), f32(0.0123))


def _q(rows, C, seed):
    """the full int8 range, -128 and 127 in the corners"""
    q = np.random.default_rng(seed).integers(-128, 128, size=(rows, C)).astype(np.int8)
    q[0, 0], q[-1, -1] = -128, 127
    return q


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_dequant_rows_dense(rows, C):
    q = _q(rows, C, rows * 1009 + C)
    x = torch.from_numpy(q).to(DEV)
    for s in SCALES:
        out = torch.full((rows, C), float("nan"), dtype=torch.float32, device=DEV)
        _lib.call("ivit_dequant_rows_i8_f32", _lib.ptr(x), C, rows, C, float(s), _lib.ptr(out), C, st())
        exp = q.astype(f32) * f32(s)
        assert np.array_equal(out.cpu().numpy().view(np.int32), exp.view(np.int32))


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_dequant_rows_fenced(rows, C):
    """ldx = C + 13, ldo = C + 5: rows that reach a 16-byte boundary together, rows that never do; then both base pointers off the
    allocation's alignment (1 byte, 4 bytes): the scalar head.  Pads and guard rows keep their fill"""
    q = _q(rows, C, rows * 7 + C)
    for s in SCALES:
        exp = q.astype(f32) * f32(s)
        for lead_x, lead_o in ((0, 0), (1, 4), (1, 0), (0, 4)):
            # (an elementwise operator: no result depends on a neighbouring element, so there is no poison condition to show;
            # a read past channel C - 1 that mattered would be a store past it, which the output's pads catch)
            x = fenced.input(q, C + 13, 127, lead_bytes=lead_x)
            o = fenced.output(rows, C, C + 5, np.float32, expected=exp, lead_bytes=lead_o)
            _lib.call("ivit_dequant_rows_i8_f32", x.ptr, x.ld, rows, C, float(s), o.ptr, o.ld, st())
            torch.cuda.synchronize()
            fenced.check(o, exp)
            fenced.check(x)
    # every row on the wide path: strides that keep the 16-byte alignment of both sides
    ldx, ldo = (C + 15) // 16 * 16 + 16, (C + 3) // 4 * 4 + 4
    exp = q.astype(f32) * SCALES[1]
    x = fenced.input(q, ldx, 127)
    o = fenced.output(rows, C, ldo, np.float32, expected=exp)
    _lib.call("ivit_dequant_rows_i8_f32", x.ptr, x.ld, rows, C, float(SCALES[1]), o.ptr, o.ld, st())
    torch.cuda.synchronize()
    fenced.check(o, exp)
    fenced.check(x)


def test_dequant_rows_is_torchs_multiplication():
    q = torch.arange(-128, 128, dtype=torch.int8, device=DEV).repeat(5).view(5, 256)
    out = torch.empty(5, 256, dtype=torch.float32, device=DEV)
    _lib.call("ivit_dequant_rows_i8_f32", _lib.ptr(q), 256, 5, 256, float(SCALES[1]), _lib.ptr(out), 256, st())
    assert same(out, q.float() * float(SCALES[1]))


def test_dequant_rows_argument_errors_launch_nothing():
    L = _lib.lib()
    rows, C = 5, 24
    x = torch.zeros(rows * (C + 2) + 16, dtype=torch.int8, device=DEV)
    exp = np.zeros((rows, C), f32)
    o = fenced.output(rows, C, C + 3, np.float32, expected=exp)

    def rc(xp=x.data_ptr(), ldx=C + 2, rows=rows, C=C, op=None, ldo=C + 3):
        op = o.t.data_ptr() + o.start if op is None else op
        return L.ivit_dequant_rows_i8_f32(ctypes.c_void_p(xp), ldx, rows, C, ctypes.c_float(0.5), ctypes.c_void_p(op), ldo, st())

    # NULL x, NULL out, C < 1, rows < 0, ldx < C, ldo < C, out off a float's alignment
    bad = [rc(xp=0), rc(op=0), rc(C=0), rc(rows=-1), rc(ldx=C - 1), rc(ldo=C - 1), rc(op=o.t.data_ptr() + o.start + 2)]
    assert bad == [-1] * len(bad), bad
    assert "ivit_dequant_rows_i8_f32" in L.ivit_last_error_string().decode()
    assert rc(rows=0) == 0                                # IVIT_OK without a launch
    torch.cuda.synchronize()
    assert (o.fetch() == o.host).all(), "a refused call wrote to the sentinel-filled output"
    assert rc() == 0
    torch.cuda.synchronize()
    fenced.check(o, exp)


# =========================================================================================== DeiT / ViT
_MODELS = {}


def _hw(img):
    return tuple(img) if isinstance(img, tuple) else (img, img)


def _images(n, img, g):
    h, w = _hw(img)
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, h, w, generator=g)).to(DEV)


def _pow2_ranges(model):
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            qmax = 2 ** (mod.activation_bit - 1) - 1
            a = max(-float(mod.x_min), float(mod.x_max)) / qmax
            assert a > 0
            p2 = 2.0 ** np.ceil(np.log2(a))
            mod.x_max.fill_(qmax * p2)
            mod.x_min.fill_(-qmax * p2)


def _vit(img, family, widths, pow2):
    """the calibrated, frozen model (as tests/test_gpu_vit16_lazy.py::_calibrated builds it, with an img_size that may be a pair) and a
    batch for it; built once per configuration and shared"""
    key = (img, family, id(widths), pow2)
    if key not in _MODELS and widths is W4:      # the 4-bit model of tests/test_gpu_w4_lazy.py, whose attention holds a probability of 1/8
        model, g = _small_w4(img, family, W4, pow2)
        _MODELS[key] = (model, _images(B, img, g))
    if key not in _MODELS:
        torch.manual_seed(sum(_hw(img)) + 16 + 128)
        model = ivit.VisionTransformer(img_size=img, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                       num_classes=40, gelu_type=family, softmax_type=family, layernorm_type=family,
                                       **widths).to(DEV).eval()
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() > 1:
                    p.mul_(3.0)
            for blk in model.blocks:      # peaked attention
                blk.attn.qkv.weight.mul_(4.0)
            g = torch.Generator(device="cpu").manual_seed(11)
            calib = _images(4, img, g)
            model(calib)
            model(calib.flip(0) * 0.7)
        if pow2:
            _pow2_ranges(model)
        ivit.freeze_model(model)
        _MODELS[key] = (model, _images(B, img, g))
    return _MODELS[key]


def _headless(model, make):
    """the same weights and ranges without the classifier"""
    twin = make(num_classes=0).to(DEV).eval()
    missing, unexpected = twin.load_state_dict(model.state_dict(), strict=False)
    assert not missing and all(k.startswith("head.") for k in unexpected)
    ivit.freeze_model(twin)
    return twin


def _module_features(model, x):
    model.use_engine = False
    try:
        assert not model.takes_engine_for_features(x)
        with torch.no_grad():
            return model.forward_features(x)
    finally:
        model.use_engine = True


VIT_CASES = {"ivit197": (224, "ivit", W8), "ivit50": (112, "ivit", W8), "ivit257": (256, "ivit", W8), "ivit_64x96": ((64, 96), "ivit", W8),
             "ibert197": (224, "ibert", W8), "w16_197": (224, "ivit", W16), "w4_197": (224, "ivit", W4)}


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
@pytest.mark.parametrize("case", list(VIT_CASES))
def test_vit_forward_features(case, pow2):
    img, family, widths = VIT_CASES[case]
    model, x = _vit(img, family, widths, pow2)
    assert model.engine_unsupported_reason() is None and model.features_unsupported_reason() is None
    x = x.contiguous()
    eng = model.engine(B)
    assert eng.stream_bits == {id(W8): 8, id(W16): 16, id(W4): 4}[id(widths)]
    with torch.no_grad():
        if eng.stream_bits == 16:      # no taps on the 16-bit stream: the tensor the tap clones, behind the plain forward
            eng.forward(x)
            tap = eng.ws["cls"][:B].clone()
        else:
            taps = {}
            eng.forward(x, taps=taps)
            tap = taps["qact2"]
        with Calls() as c:
            q, s_q = eng.forward_features(x, integers=True)
        with Calls() as cf:
            f, s = eng.forward_features(x)
        m_f, m_s = model.features(x)
        m_q, _ = model.features(x, integers=True)
        ref, ref_s = _module_features(model, x)
    assert isinstance(s, float) and s == s_q == m_s == float(ref_s.reshape(-1)[0]) == float(model.qact2.act_scaling_factor.reshape(-1)[0])
    assert q.dtype == torch.int8 and tuple(q.shape) == (B, 128) and torch.equal(q, tap.view(B, 128))
    assert f.dtype == torch.float32 and same(f, tap.view(B, 128).float() * torch.tensor(s, dtype=torch.float32, device=DEV))
    assert np.array_equal(f.cpu().numpy().view(np.int32), (tap.view(B, 128).cpu().numpy().astype(f32) * f32(s)).view(np.int32))
    ref = ref.to_float(boundary=True) if hasattr(ref, "to_float") else ref
    assert same(f, ref), f"{int((f != ref).sum())} of {f.numel()} differ from the module path"
    assert same(m_f, f) and same(m_q, q) and len(torch.unique(q)) > 4
    # a fresh tensor, no workspace view
    lo, hi = eng.ws["cls"].data_ptr(), eng.ws["cls"].data_ptr() + eng.ws["cls"].numel()
    assert not lo <= q.data_ptr() < hi and not lo <= f.data_ptr() < hi
    # nothing behind the final LayerNorm but the one dequantisation; the class-row tail wherever it exists
    for names in (c.names, cf.names):
        assert "ivit_gemm_i8_i32" not in names and not [n for n in names if n.startswith("ivit_head_")]
    assert cf.names[-1] == "ivit_dequant_rows_i8_f32" and cf.names[:-1] == c.names
    assert ("ivit_attention_cls_i8" in c.names) == eng.cls_tail_ok
    assert eng.cls_tail_ok == (case in ("ivit197", "ivit50", "ivit_64x96")), "I-ViT, 8-bit stream, at most 207 tokens"


def test_deit_tiny_features_match_the_golden_qact2():
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=meta["n_images"])
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    q, _ = eng.forward_features(imgs, integers=True)
    gold = dict(zip([str(x) for x in z["tap_names"]], z["tap_crc32"]))
    assert "qact2" in gold, "the fixture lists the tap"
    assert crc(q.cpu().numpy().astype(np.int32)) == int(gold["qact2"])


# =========================================================================================== Swin
def _swin_features(model, x, eng):
    x = x.contiguous()
    C = eng.C_last
    with torch.no_grad():
        taps = {}
        eng.forward(x, taps=taps)
        tap = taps["qact3"].reshape(B, C)
        with Calls() as c:
            q, s_q = eng.forward_features(x, integers=True)
        with Calls() as cf:
            f, s = eng.forward_features(x)
        ref, ref_s = _module_features(model, x)
    assert s == s_q == float(ref_s.reshape(-1)[0]) == float(model.qact3.act_scaling_factor.reshape(-1)[0])
    assert q.dtype == torch.int8 and torch.equal(q, tap)
    assert np.array_equal(f.cpu().numpy().view(np.int32), (tap.cpu().numpy().astype(f32) * f32(s)).view(np.int32))
    ref = ref.to_float(boundary=True) if hasattr(ref, "to_float") else ref
    assert same(f, ref), f"{int((f != ref).sum())} of {f.numel()} differ from the module path"
    assert len(torch.unique(q)) > 4
    pool = [i for i, n in enumerate(c.names) if n.startswith("ivit_avgpool_requant_i8")]
    assert pool == [len(c.names) - 1], "nothing behind the pooling launch"
    assert cf.names == c.names + ["ivit_dequant_rows_i8_f32"]
    return f, q, s


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_forward_features(pow2):
    model, x = swin_lazy.built("A", pow2)
    assert model.features_unsupported_reason() is None and model.takes_engine_for_features(x)
    f, q, s = _swin_features(model, x, model.engine(B))
    with torch.no_grad():
        m_f, m_s = model.features(x)
        m_q, _ = model.features(x, integers=True)
    assert m_s == s and same(m_f, f) and same(m_q, q)


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_ibert_forward_features(pow2):
    """model.features answers module by module, as attention_maps does for this family; the engine is engine_from_model's"""
    model, x = swin_ibert.built("A", pow2)
    assert "operator family" in model.features_unsupported_reason() and not model.takes_engine_for_features(x)
    eng = engine_from_model(model, max_batch=4)
    assert eng.family == "ibert"
    f, q, s = _swin_features(model, x, eng)
    with torch.no_grad():
        m_f, m_s = model.features(x)
        m_q, _ = model.features(x, integers=True)
    assert m_s == s and same(m_f, f) and same(m_q, q)


# =========================================================================================== out=
@pytest.mark.parametrize("integers", [False, True])
def test_out_is_a_slice_of_a_bank(integers):
    model, x = _vit(224, "ivit", W8, False)
    eng, x = model.engine(B), x.contiguous()
    dt, sentinel = (torch.int8, 85) if integers else (torch.float32, -1.5e30)
    with torch.no_grad():
        want, s = eng.forward_features(x, integers)
        bank = torch.full((B + 2, 128 + 7), sentinel, dtype=dt, device=DEV)
        rows = bank[1:1 + B, 3:3 + 128]
        got, s2 = eng.forward_features(x, integers, out=rows)
    assert got is rows and s2 == s and same(rows, want)
    mask = torch.ones_like(bank, dtype=torch.bool)
    mask[1:1 + B, 3:3 + 128] = False
    assert bool((bank[mask] == sentinel).all()), "only the slice changes"
    smodel, sx = swin_lazy.built("A", False)
    seng = smodel.engine(B)
    with torch.no_grad():
        want, _ = seng.forward_features(sx.contiguous(), integers)
        bank = torch.full((B + 2, seng.C_last + 7), sentinel, dtype=dt, device=DEV)
        seng.forward_features(sx.contiguous(), integers, out=bank[2:, 7:])
    assert same(bank[2:, 7:], want) and bool((bank[:2] == sentinel).all()) and bool((bank[:, :7] == sentinel).all())


def test_bad_out_raises_before_anything_is_launched():
    model, x = _vit(224, "ivit", W8, False)
    smodel, sx = swin_lazy.built("A", False)
    for eng, xx, C in ((model.engine(B), x.contiguous(), 128), (smodel.engine(B), sx.contiguous(), smodel.engine(B).C_last)):
        bad = [torch.empty(B, C, dtype=torch.int8, device=DEV),                       # dtype (float asked for)
               torch.empty(B, C, dtype=torch.float64, device=DEV),
               torch.empty(B + 1, C, dtype=torch.float32, device=DEV),                # shape
               torch.empty(B, C + 1, dtype=torch.float32, device=DEV),
               torch.empty(B * C, dtype=torch.float32, device=DEV),
               torch.empty(C, B, dtype=torch.float32, device=DEV).t(),                # inner stride
               torch.empty(B, 2 * C, dtype=torch.float32, device=DEV)[:, ::2],
               torch.empty(B, C, dtype=torch.float32)]                                # device
        with Calls() as c:
            for out in bad:
                with pytest.raises((TypeError, ValueError), match="out"):
                    eng.forward_features(xx, out=out)
            with pytest.raises(TypeError, match="out"):
                eng.forward_features(xx, integers=True, out=torch.empty(B, C, dtype=torch.float32, device=DEV))
        assert c.names == []


# =========================================================================================== headless
def test_headless_vit_reaches_the_engine():
    model, x = _vit(224, "ivit", W8, False)
    twin = _headless(model, partial(ivit.VisionTransformer, img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
                                    qkv_bias=True, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8))
    assert twin.features_unsupported_reason() is None and "no classification head" in twin.engine_unsupported_reason()
    assert twin.takes_engine_for_features(x) and not twin.takes_engine(x)
    with torch.no_grad():
        for integers in (False, True):
            a, sa = model.features(x, integers)
            b, sb = twin.features(x, integers)
            assert sa == sb and same(a, b)
            (ma, msa), (mb, msb) = model.forward_intermediates(x, None, integers), twin.forward_intermediates(x, None, integers)
            assert msa == msb and list(ma) == list(mb) == [0, 1] and all(same(ma[i], mb[i]) for i in ma)
        (pa, _), (pb, _) = model.attention_maps(x, rows="all"), twin.attention_maps(x, rows="all")
        assert list(pa) == list(pb) == [0, 1] and all(torch.equal(pa[i], pb[i]) for i in pa)
        eng = twin.engine(B)
        assert eng.head is None and eng.num_classes == 0 and "logits" not in eng.ws and eng.int8_weight_bytes > 0
        with Calls() as c:
            for call in (lambda: eng.forward(x.contiguous()), lambda: eng(x.contiguous()), lambda: eng.forward_topk(x.contiguous(), 1),
                         lambda: eng.forward_graph(x.contiguous()), lambda: eng.forward_topk_graph(x.contiguous(), 1)):
                with pytest.raises(ValueError, match="no classification head"):
                    call()
        assert c.names == []
        g, _ = twin.features_graph(x)
        assert same(g, model.features(x)[0])


def test_headless_swin_reaches_the_engine():
    model, x = swin_lazy.built("A", False)
    twin = _headless(model, partial(ivit.SwinTransformer, patch_size=4, embed_dim=96, norm_layer=partial(qu.IntLayerNorm, eps=1e-6),
                                    **swin_lazy.MODELS["A"]))
    assert twin.features_unsupported_reason() is None and "no classification head" in twin.engine_unsupported_reason()
    assert twin.takes_engine_for_features(x) and not twin.takes_engine(x)
    with torch.no_grad():
        for integers in (False, True):
            a, sa = model.features(x, integers)
            b, sb = twin.features(x, integers)
            assert sa == sb and same(a, b)
            (ma, msa), (mb, msb) = model.forward_intermediates(x, None, integers), twin.forward_intermediates(x, None, integers)
            assert msa == msb and list(ma) == list(mb) == [0, 1] and all(same(ma[i], mb[i]) for i in ma)
        (pa, _), (pb, _) = model.attention_maps(x), twin.attention_maps(x)
        assert list(pa) == list(pb) and all(torch.equal(pa[k], pb[k]) for k in pa)
        eng = twin.engine(B)
        assert eng.head is None
        with Calls() as c:
            with pytest.raises(ValueError, match="no classification head"):
                eng.forward(x.contiguous())
        assert c.names == []


# =========================================================================================== stop_early
def test_stop_early_vit():
    model, x = _vit(224, "ivit", W8, False)          # depth 2: D - 2 == 0; the three-block model below has a block in between
    torch.manual_seed(5)
    deep = ivit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                  num_classes=40, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit").to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(3)
    with torch.no_grad():
        for p in deep.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        deep(_images(4, 64, g))
    ivit.freeze_model(deep)
    for m, xx, D in ((model, x.contiguous(), 2), (deep, _images(B, 64, g).contiguous(), 3)):
        eng = m.engine(B)
        with torch.no_grad():
            with Calls() as one:
                eng.forward(xx)
            per_block = (len(one.names) - 6) // D      # patchify, patch GEMM, assembly in front; final norm, head GEMM, argmax behind
            for indices in ((0,),) + (((0, D - 2),) if D > 2 else ()):      # (D == 2: (0, D - 2) repeats block 0)
                for integers in (False, True):
                    full, fs_ = eng.forward_intermediates(xx, indices, integers)
                    with Calls() as c:
                        early, es = eng.forward_intermediates_early(xx, indices, integers)
                    assert fs_ == es and list(full) == list(early) and all(same(full[i], early[i]) for i in full)
                    last = max(indices)
                    assert c.names[-1].startswith("ivit_tokens_to_nchw"), "the last launch fills the last selected map"
                    assert len(c.names) == 3 + per_block * (last + 1) + len(set(indices))
                    assert c.names.count("ivit_gemm_i8_requant_qkv_ex") == last + 1
                    assert "ivit_gemm_i8_i32" not in c.names and not [n for n in c.names if n.startswith("ivit_head_")]
                    m_early, _ = m.forward_intermediates_early(xx, indices, integers)
                    assert all(same(full[i], m_early[i]) for i in full)


def test_stop_early_swin():
    model, x = swin_lazy.built("A", False)
    eng, x = model.engine(B), x.contiguous()
    with torch.no_grad():
        for integers in (False, True):
            full, fs_ = eng.forward_intermediates(x, (0,), integers)
            with Calls() as c:
                early, es = eng.forward_intermediates_early(x, (0,), integers)
            assert fs_ == es and same(full[0], early[0])
            assert c.names[-1].startswith("ivit_tokens_to_nchw") and c.names.count("ivit_gemm_i8_requant_qkv_ex") == 2
            assert "ivit_patch_merge_i16" not in c.names and "ivit_gemm_i8_i32" not in c.names
            assert not [n for n in c.names if n.startswith(("ivit_avgpool", "ivit_head_"))]
            m_early, _ = model.forward_intermediates_early(x, (0,), integers)
            assert same(full[0], m_early[0])


# =========================================================================================== graph
@pytest.mark.parametrize("which", ["vit", "swin"])
def test_feature_graph_next_to_the_logits_graph(which):
    model, x = _vit(224, "ivit", W8, False) if which == "vit" else swin_lazy.built("A", False)
    eng, x = model.engine(B), x.contiguous()
    x2 = (x.flip(0) * 0.8).contiguous()
    with torch.no_grad():
        logits = [eng.forward(v)[0].clone() for v in (x, x2)]
        assert torch.equal(eng.forward_graph(x)[0], logits[0])
        for integers in (False, True):
            for v in (x, x2, x):
                want, s = eng.forward_features(v, integers)
                got, sg = eng.forward_features_graph(v, integers)
                assert sg == s and same(got, want)
        assert len([k for k in eng._graphs if "features" in k]) == 2, "one capture per (batch size, integers)"
        for v, want in ((x2, logits[1]), (x, logits[0])):
            assert torch.equal(eng.forward_graph(v)[0], want), "the logits graph still replays"
        mg, _ = model.features_graph(x2)
        assert same(mg, eng.forward_features(x2)[0])
    eng.drop_graphs()


# =========================================================================================== extract_features
@pytest.mark.parametrize("which", ["vit", "swin"])
def test_extract_features_uneven_last_batch(which):
    model, x = _vit(224, "ivit", W8, False) if which == "vit" else swin_lazy.built("A", False)
    g = torch.Generator(device="cpu").manual_seed(21)
    imgs = _images(7, x.shape[-1], g).cpu()
    targets = torch.tensor([5, 0, 3, 9, 9, 1, 7])
    loader = [(imgs[i:i + 3], targets[i:i + 3]) for i in range(0, 7, 3)]
    with torch.no_grad():
        per_batch = [model.features(b.to(DEV)) for b, _ in loader]
        per_batch_q = [model.features(b.to(DEV), integers=True)[0] for b, _ in loader]
        f, labels, s = extract_features(model, loader, DEV)
        q, labels_q, s_q = extract_features(model, loader, DEV, integers=True)
        fg, labels_g, s_g = extract_features(model, loader, DEV, graph=True)
        qg, _, _ = extract_features(model, loader, DEV, graph=True, integers=True)
    assert tuple(f.shape) == (7, model.num_features) and f.dtype == torch.float32 and q.dtype == torch.int8
    assert s == s_q == s_g == per_batch[0][1]
    assert same(f, torch.cat([p[0] for p in per_batch])) and same(q, torch.cat(per_batch_q)), "rows in loader order"
    for lab in (labels, labels_q, labels_g):
        assert lab.dtype == torch.int64 and lab.device.type == "cuda" and torch.equal(lab.cpu(), targets)
    assert same(fg, f) and same(qg, q)
    model.drop_graphs()
