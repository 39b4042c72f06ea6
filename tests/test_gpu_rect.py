"""Images that are not square, on the GPU.

  kernels   ivit_quantize_patchify_hw_f32_i8 / _u8_i8 against a numpy im2col of the reference's rounding (quant_utils.py:49) or of the
            table, byte for byte, into fenced operands (tests/fenced.py) with lda = width and lda = width + 64; h = w against the square
            entries; every argument error of the contract, with nothing launched; one launch of 2^31 + 262 144 pixel groups (the
            64-bit form of the index chain)
  ViT       the fused engine against the int8-carrying and the literal module path on models calibrated here (which goes through
            QuantConv2d._slow at H != W), 8-bit, 16-bit stream and every knob at 4; forward_graph; the reference's own forward
            (tests/golden/deit_rect*.npz, scripts/gen_rect_golden.py) through both paths
  Swin      the reference's own forward (tests/golden/swin_rect*.npz: a shifted 14 x 28 map, a 24 x 8 map whose second stage has 4 x 4
            windows) through the engine and the module path; an I-BERT Swin through swin_engine.engine_from_model;
            ivit_avgpool_f32_literal (the module path's token pooling in torch's CPU order) against torch on the CPU
  maps      forward_intermediates and attention_maps of both engines against the hook path
Nothing here has a tolerance."""
import json
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_dims_model  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402
from ivit_amd.swin_engine import engine_from_model  # noqa: E402

import fenced  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
HW_F32, HW_U8 = "ivit_quantize_patchify_hw_f32_i8", "ivit_quantize_patchify_hw_u8_i8"
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


def p(t):
    return _lib.ptr(t)


def bits(x):
    return x.detach().cpu().numpy().view(np.int32)


def crc(t):
    return zlib.crc32(np.ascontiguousarray(t.detach().cpu().numpy().astype(np.int32)).tobytes())


# =========================================================================================== the two kernels
# (batch, chans, h, w, patch): both orientations at patch 4 and 16, a patch as wide as half the image, one channel; (3, 3, 48, 16, 16)
# is 1728 pixel groups, seven workgroups
F32_CASES = [(2, 3, 8, 16, 4), (2, 3, 16, 8, 4), (1, 3, 16, 48, 16), (3, 3, 48, 16, 16), (1, 3, 32, 64, 32), (2, 1, 8, 24, 8)]
U8_CASES = F32_CASES + [(2, 4, 8, 16, 4), (1, 4, 48, 16, 16)]
INV_SCALES = (f32(16.0), f32(1.0) / f32(0.0371))      # a power of two (exact .5 ties below) and a calibrated scale


def case_id(c):
    return "B{}_C{}_{}x{}_p{}".format(*c)


def im2col(q, patch):
    """[B, C, h, w] -> [B * gh * gw, C * patch * patch]: row (b, py, px), column (c, kh, kw)"""
    B, C, h, w = q.shape
    gh, gw = h // patch, w // patch
    return np.ascontiguousarray(q.reshape(B, C, gh, patch, gw, patch).transpose(0, 2, 4, 1, 3, 5)).reshape(B * gh * gw, C * patch * patch)


def quant_ref(img, inv):
    """quant_utils.py:49 + the clamp of :79-97 in float32: clamp(round(1/s * x), -128, 127), round half to even"""
    return np.clip(np.rint((f32(inv) * img.astype(f32)).astype(f32)), -128, 127).astype(np.int8)


def float_image(case, inv):
    B, C, h, w, _ = case
    rng = np.random.default_rng(sum(case))
    img = (rng.standard_normal((B, C, h, w)) * 40.0 / float(inv)).astype(f32)
    flat = img.reshape(-1)
    k = rng.integers(-120, 120, size=flat.size // 5)
    flat[::5][:k.size] = ((k + 0.5) / float(inv)).astype(f32)          # exact ties at the power-of-two scale
    flat[1::97] = 1e6
    flat[2::89] = -1e6                                                 # saturation both ways
    return img


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("case", F32_CASES, ids=case_id)
def test_patchify_hw_f32(case, pad):
    B, C, h, w, patch = case
    K = C * patch * patch
    rows = B * (h // patch) * (w // patch)
    for inv in INV_SCALES:
        img = float_image(case, inv)
        want = im2col(quant_ref(img, inv), patch)
        assert (want == 127).any() and (want == -128).any() and len(np.unique(want)) > 100
        x = fenced.input(img.reshape(B * C * h, w), w, fenced.POISON[np.dtype(f32)], device=DEV)       # dense rows between poisoned guards
        o = fenced.output(rows, K, K + pad, np.int8, expected=want, device=DEV)
        _lib.call("ivit_quantize_patchify_hw_f32_i8", x.ptr, o.ptr, o.ld, B, C, h, w, patch, float(inv), st())
        fenced.check(o, want)
        fenced.check(x)
        if inv == f32(16.0):      # the ties are real: rounding half away from zero would give other bytes
            away = np.clip(np.trunc(inv * img + np.copysign(f32(0.5), img)), -128, 127).astype(np.int8)
            assert (im2col(away, patch) != want).any()


@pytest.mark.parametrize("pad", [0, 64])
@pytest.mark.parametrize("case", U8_CASES, ids=case_id)
def test_patchify_hw_u8(case, pad):
    B, C, h, w, patch = case
    K = C * patch * patch
    rows = B * (h // patch) * (w // patch)
    rng = np.random.default_rng(sum(case) + 1)
    img = rng.integers(0, 256, size=(B, C, h, w), dtype=np.uint8)
    img[0, :, 0, :4] = [0, 255, 1, 254]
    lut = rng.integers(-128, 128, size=(C, 256)).astype(np.int8)
    want = im2col(lut[np.arange(C)[None, :, None, None], img], patch)
    x = fenced.input(img.reshape(B * C * h, w), w, 0xA5, device=DEV)
    o = fenced.output(rows, K, K + pad, np.int8, expected=want, device=DEV)
    _lib.call("ivit_quantize_patchify_hw_u8_i8", x.ptr, o.ptr, o.ld, B, C, h, w, patch, p(dev(lut)), st())
    fenced.check(o, want)
    fenced.check(x)


def test_patchify_hw_u8_beyond_2_31_pixel_groups():
    """2731 images of 3 x 512 x 2048 uint8 pixels are 2^31 + 262 144 groups of 4 pixels: the 64-bit form of the index chain (the only
    size at which it runs; both pixel types share the chain).  8.6 GB in, 8.6 GB out; expected values by torch on the device, from a
    table that is an arithmetic map of (channel, value): lut[c][v] = int8((v + 64 c) mod 256 - 128)"""
    B, C, h, w, patch = 2731, 3, 512, 2048, 16
    assert B * C * h * (w // 4) >= 2 ** 31 > (B - 1) * C * h * (w // 4)
    g = torch.Generator(device=DEV).manual_seed(3)
    img = torch.randint(0, 256, (B, C, h, w), dtype=torch.uint8, device=DEV, generator=g)
    v = np.arange(256)
    lut = np.stack([((v + 64 * c) % 256 - 128) for c in range(C)]).astype(np.int8)
    K, gh, gw = C * patch * patch, h // patch, w // patch
    out = torch.empty(B * gh * gw, K, dtype=torch.int8, device=DEV)
    _lib.call("ivit_quantize_patchify_hw_u8_i8", p(img), p(out), K, B, C, h, w, patch, p(dev(lut)), st())
    img += (64 * torch.arange(C, device=DEV, dtype=torch.uint8)).view(1, C, 1, 1)          # wraps modulo 256
    img ^= 128                                                                             # v - 128 as the int8 bit pattern
    want = img.view(torch.int8).view(B, C, gh, patch, gw, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, K)
    assert torch.equal(out, want)
    assert bool((out[-1] != out[0]).any())


@pytest.mark.parametrize("B,C,hw,patch,lda", [(2, 3, 16, 4, 64), (1, 3, 32, 16, 768), (2, 4, 8, 4, 64)])
def test_square_images_give_the_bytes_of_the_square_entries(B, C, hw, patch, lda):
    rng = np.random.default_rng(hw + patch)
    inv = INV_SCALES[1]
    imgf = dev((rng.standard_normal((B, C, hw, hw)) * 40.0 / float(inv)).astype(f32))
    imgu = dev(rng.integers(0, 256, size=(B, C, hw, hw), dtype=np.uint8))
    lut = dev(rng.integers(-128, 128, size=(C, 256)).astype(np.int8))
    rows = B * (hw // patch) ** 2
    a, b, c, d = (torch.full((rows, lda), 77, dtype=torch.int8, device=DEV) for _ in range(4))
    _lib.call("ivit_quantize_patchify_ld_f32_i8", p(imgf), p(a), lda, B, C, hw, patch, float(inv), st())
    _lib.call("ivit_quantize_patchify_hw_f32_i8", p(imgf), p(b), lda, B, C, hw, hw, patch, float(inv), st())
    _lib.call("ivit_quantize_patchify_u8_i8", p(imgu), p(c), lda, B, C, hw, patch, p(lut), st())
    _lib.call("ivit_quantize_patchify_hw_u8_i8", p(imgu), p(d), lda, B, C, hw, hw, patch, p(lut), st())
    assert torch.equal(a, b) and torch.equal(c, d)
    assert len(torch.unique(a)) > 50 and len(torch.unique(c)) > 50


def test_argument_errors_launch_nothing():
    """every clause of the contract (include/ivit_hip.h): IVIT_ERR_INVALID (-1), the entry's name in the message, the output untouched"""
    L = _lib.lib()
    B, C, h, w, patch = 2, 3, 8, 16, 4
    imgf = dev(np.ones((B, C, h, w), f32))
    imgu = dev(np.ones((B, 4, h, w), np.uint8))
    lut = dev(np.ones((4, 256), np.int8))
    out = torch.full((B * 2 * 4, 64 + 16), 66, dtype=torch.int8, device=DEV)
    ok = dict(A=out, lda=80, batch=B, chans=C, h=h, w=w, patch=patch, lut=lut)

    def rc(name, **kw):
        a = dict(ok, img=imgf if name == HW_F32 else imgu)
        a.update(kw)
        last = (1.0,) if name == HW_F32 else (p(a["lut"]),)
        return getattr(L, name)(p(a["img"]), p(a["A"]), a["lda"], a["batch"], a["chans"], a["h"], a["w"], a["patch"], *last, st())

    bad = [dict(h=10), dict(w=18), dict(h=0), dict(patch=6, h=12, w=12), dict(patch=2), dict(patch=0), dict(lda=44), dict(lda=50),
           dict(batch=0), dict(chans=0), dict(img=None), dict(A=None), dict(A=out.view(-1)[1:])]
    for name in (HW_F32, HW_U8):
        extra = [dict(img=imgf.view(-1)[1:])] if name == HW_F32 else [dict(chans=5, lda=80), dict(lut=None), dict(img=imgu.view(-1)[1:])]
        for kw in bad + extra:
            assert rc(name, **kw) == -1, (name, kw)
            msg = L.ivit_last_error_string().decode()
            assert msg.startswith(name + ":"), (name, kw, msg)
    torch.cuda.synchronize()
    assert bool((out == 66).all())
    assert rc(HW_F32) == 0 and rc(HW_U8) == 0 and rc(HW_U8, chans=4) == 0
    torch.cuda.synchronize()
    assert bool((out[:, 64:] == 66).all()) and bool((out[:, :64] == 1).all())


# =========================================================================================== the float mean of the module path's pooling
@pytest.mark.parametrize("B,T,C", [(3, 98, 128), (3, 48, 128), (2, 48, 100), (8, 144, 72), (3, 49, 40), (1, 2, 4)])
def test_avgpool_f32_literal_equals_torchs_cpu_mean(B, T, C):
    """ivit_avgpool_f32_literal against the reference's own call on the CPU, avgpool(y.transpose(1, 2)) of y = fl(q s) (one thread:
    torch's serial order), bit for bit -- columns whose mean is an exact .5 tie of rint(mean / s) among them, full 32-column groups
    and tail columns (C = 100, 72, 40, 4), the token counts of the (56, 112) and (96, 32) models"""
    from test_swin_384_cpu import _tie_rows
    rng = np.random.default_rng(B * 10000 + T * 100 + C)
    s = f32(0.0123457)
    q = _tie_rows(rng, B, T, C)
    y = torch.from_numpy((q.astype(f32) * s).astype(f32))
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(1)
        ref = torch.nn.AdaptiveAvgPool1d(1)(y.transpose(1, 2))[:, :, 0].contiguous()
    finally:
        torch.set_num_threads(prev)
    out = torch.full((B + 1, C), float("nan"), dtype=torch.float32, device=DEV)
    yd = y.to(DEV)
    _lib.call("ivit_avgpool_f32_literal", p(yd), p(out), B, T, C, st())
    assert np.array_equal(bits(out[:B]), bits(ref)), f"{int((bits(out[:B]) != bits(ref)).sum())} of {B * C} means differ"
    assert bool(torch.isnan(out[B]).all())                               # nothing behind the last row
    if T % 2 == 0 and T > 2:      # the ties are real: CUDA's mean rounds some qact3 inputs the other way
        z_ref, z_cuda = torch.round(ref / float(s)), torch.round(yd.transpose(1, 2).mean(dim=2).cpu() / float(s))
        print(f"B={B} T={T} C={C}: rint(mean / s) differs between CUDA's mean and the CPU order in {int((z_ref != z_cuda).sum())} of {B * C}")
    L = _lib.lib()
    for bad in ((None, p(out), B, T, C), (p(yd), None, B, T, C), (p(yd), p(out), 0, T, C), (p(yd), p(out), B, 0, C), (p(yd), p(out), B, T, 0)):
        assert L.ivit_avgpool_f32_literal(*bad, st()) == -1 and L.ivit_last_error_string().decode().startswith("ivit_avgpool_f32_literal:")


# =========================================================================================== models calibrated here
W8 = dict(patch_embed_bw=8, pos_encoding_bw=8, block_input_bw=8, attention_out_bw=8, softmax_bw=8, mlp_out_bw=8, norm2_in_bw=8, att_block_out_bw=8)
W16 = dict(W8, patch_embed_bw=16, block_input_bw=16, attention_out_bw=16, mlp_out_bw=16, norm2_in_bw=16, att_block_out_bw=16)   # the 16-bit stream
W4 = {k: 4 for k in W8}                                                                                                        # every knob at 4
_BUILT = {}


def _images(n, hw, g):
    """smooth random patterns plus noise: image content at the scale of patches"""
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=tuple(hw), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, *hw, generator=g)).to(DEV)


def snap_pow2(model):
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            qmax = 2 ** (mod.activation_bit - 1) - 1
            a = max(-float(mod.x_min), float(mod.x_max)) / qmax
            if a == 0.0:
                continue                                   # Swin's act_out: constructed, never called
            s = 2.0 ** np.ceil(np.log2(a))
            mod.x_max.fill_(qmax * s)
            mod.x_min.fill_(-qmax * s)


def _vit(hw, patch, widths):
    """VisionTransformer(img_size=(H, W)) calibrated on the GPU -- an unfrozen forward is QuantConv2d._slow at H != W -- and frozen;
    built once per configuration and shared, no test changes it for good.  -> (model, generator for its images)"""
    key = ("vit", hw, patch, id(widths))
    if key not in _BUILT:
        torch.manual_seed(hw[0] * 1000 + hw[1] + patch)
        model = ivit.VisionTransformer(img_size=hw, patch_size=patch, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                       num_classes=40, **widths).to(DEV).eval()
        with torch.no_grad():
            for prm in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
                if prm.dim() > 1:
                    prm.mul_(3.0)
            if widths is W4:                        # a class token and a position embedding that 4 bits can hold, a sharp softmax
                model.cls_token.normal_(0.0, 2.0)
                model.pos_embed.normal_(0.0, 0.7)
            for blk in model.blocks:
                blk.attn.qkv.weight.mul_(16.0 if widths is W4 else 4.0)
            g = torch.Generator(device="cpu").manual_seed(5)
            calib = _images(6, hw, g)
            model(calib)
            model(calib.flip(0) * 0.7)
        ivit.freeze_model(model)
        _BUILT[key] = (model, g)
    return _BUILT[key]


def _module_path(model, x, lazy_on, taps=None):
    """the module-by-module forward (int8-carrying with lazy_on, else literal); taps receives every QuantAct output as integers"""
    hooks = []
    if taps is not None:
        def hook(name):
            def fn(mod, inp, outp):
                y, s = outp
                taps[name] = y.q.to(torch.int32) if isinstance(y, lazy.QT) and y.q is not None else \
                    torch.round((y.to_float() if isinstance(y, lazy.QT) else y) / s).to(torch.int32)
            return fn
        hooks = [mod.register_forward_hook(hook(name)) for name, mod in model.named_modules()
                 if isinstance(mod, qu.QuantAct) and name != "act_out" and not name.endswith("int_softmax.act")]
    old, model.use_engine = lazy.ENABLED, False
    try:
        lazy.ENABLED = lazy_on
        with torch.no_grad():
            return model(x)
    finally:
        lazy.ENABLED = old
        model.use_engine = True
        for hk in hooks:
            hk.remove()


VIT_CASES = {"64x96": ((64, 96), 16, W8), "96x64": ((96, 64), 16, W8), "32x64_p8": ((32, 64), 8, W8), "64x96_w16": ((64, 96), 16, W16),
             "96x64_w4": ((96, 64), 16, W4)}


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_vit_engine_equals_both_module_paths(case):
    """test_engine_other_geometries_equal_the_module_path of tests/test_gpu_modules.py for H != W (25, 25 and 33 tokens)"""
    hw, patch, widths = VIT_CASES[case]
    model, g = _vit(hw, patch, widths)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    x = _images(6, hw, g)
    with torch.no_grad():
        assert model.takes_engine(x)
        ye = model(x)
        eng = model.engine(6)
    tokens = (hw[0] // patch) * (hw[1] // patch) + 1
    assert eng.T == tokens and eng.grid == (hw[0] // patch, hw[1] // patch) and eng.IMG == hw
    assert eng.stream_bits == {id(W8): 8, id(W16): 16, id(W4): 4}[id(widths)]
    yl = _module_path(model, x, True)
    ym = _module_path(model, x, False)
    assert torch.equal(ye, ym), f"engine against the literal module path: {int((ye != ym).sum())} logits differ"
    assert torch.equal(yl, ym), f"int8-carrying against the literal module path: {int((yl != ym).sum())} logits differ"
    assert len(torch.unique(ye.argmax(dim=1))) > 1
    xc = x.contiguous()
    li, lf, t1 = (t.clone() for t in eng.forward(xc))
    assert torch.equal(lf[:, :40], ye)
    for _ in range(2):                                     # capture, then a replay of the cached graph
        gi, gf, g1 = eng.forward_graph(xc)
        assert torch.equal(gi, li) and torch.equal(gf, lf) and torch.equal(g1, t1)
    eng.drop_graphs()


def test_vit_uint8_pixels():
    """uint8 [B, 3, H, W] through ivit_quantize_patchify_hw_u8_i8 and the engine's 3 x 256 table: the logits of the float pipeline"""
    hw = (64, 96)
    model, _ = _vit(hw, 16, W8)
    eng = model.engine(3)
    eng.set_input_normalisation()
    u8 = torch.from_numpy(np.random.default_rng(8).integers(0, 256, size=(3, 3, *hw), dtype=np.uint8)).to(DEV)
    lut = eng.input_lut.cpu().numpy().reshape(3, 256)
    q = lut[np.arange(3)[None, :, None, None], u8.cpu().numpy()]                      # what the table makes of the pixels
    xf = torch.from_numpy((q.astype(f32) * f32(eng.s0)).astype(f32)).to(DEV)          # floats that quantise to exactly those integers
    want = eng.forward(xf.contiguous())[0].clone()
    assert torch.equal(eng.forward(u8)[0], want) and len(torch.unique(want)) > 3


# =========================================================================================== the reference's fixtures
def _fixture_model(tag):
    key = ("fixture", tag)
    if key not in _BUILT:
        fs, ranges, meta, z = load_dims_model(tag)
        d, ops = meta["dims"], meta["operators"]
        names = dict(gelu_type=ops, softmax_type=ops, layernorm_type=ops)
        if meta["kind"] == "vit":
            model = ivit.VisionTransformer(img_size=tuple(meta["img_size"]), patch_size=d["patch"], embed_dim=d["embed_dim"], depth=d["depth"],
                                           num_heads=d["num_heads"], mlp_ratio=4, qkv_bias=True, num_classes=meta["num_classes"], **names)
        else:
            model = ivit.SwinTransformer(img_size=tuple(meta["img_size"]), patch_size=4, window_size=d["window"], embed_dim=d["embed_dim"],
                                         depths=tuple(d["depths"]), num_heads=tuple(d["num_heads"]), num_classes=meta["num_classes"], **names)
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
        assert not unexpected, unexpected
        for name, mod in model.named_modules():
            if isinstance(mod, qu.QuantAct) and name in ranges:
                mod.x_min.fill_(float(ranges[name][0]))
                mod.x_max.fill_(float(ranges[name][1]))
        model.to(DEV).eval()
        ivit.freeze_model(model)
        x = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"], img_size=tuple(meta["img_size"]))).to(DEV)
        _BUILT[key] = (model, x, meta, z)
    return _BUILT[key]


def _check_against_fixture(y, taps, z, what, min_taps):
    """INT32 logits, top-1 and the CRC32 of every tap the fixture knows.  The float logits bit for bit at power-of-two ranges only: at
    calibrated ranges the reference's are a float32 matrix product over fl(q * s), a fraction of an integer step away from acc * scale"""
    pow2 = json.loads(str(z["meta"]))["regime"] == "pow2"
    gold = dict(zip([str(n) for n in z["tap_names"]], z["tap_crc32"]))
    n = z["logits_int32"].shape[1]
    li = torch.round(y.cpu()[:, :n].double() / torch.from_numpy(z["head_scale"]).double()).to(torch.int32).numpy() if y.dtype == torch.float32 \
        else y.cpu().numpy()[:, :n]
    assert np.array_equal(li, z["logits_int32"]), f"{what}: {int((li != z['logits_int32']).sum())} INT32 logits differ"
    if y.dtype == torch.float32:
        assert not pow2 or np.array_equal(bits(y[:, :n]), z["logits_f32_bits"]), f"{what}: float logits"
        assert np.array_equal(y[:, :n].argmax(dim=1).cpu().numpy(), z["top1"]), what
    checked = [name for name in taps if name in gold]
    bad = [name for name in checked if crc(taps[name]) != int(gold[name])]
    assert not bad and len(checked) >= min_taps, f"{what}: {len(checked)} taps checked, differing {bad[:6]} ({len(bad)})"


@pytest.mark.parametrize("tag", ["deit_rect", "deit_rect_natural", "deit_rect_ibert", "deit_rect_ibert_natural"])
def test_vit_matches_the_reference(tag):
    model, x, meta, z = _fixture_model(tag)
    depth = meta["dims"]["depth"]
    assert model.engine_unsupported_reason() is None and model.takes_engine(x)
    with torch.no_grad():
        ye = model(x)                                      # the engine
        eng = model.engine(x.shape[0])
        assert eng.family == meta["operators"] and eng.IMG == tuple(meta["img_size"])
        taps = {}
        li, lf, t1 = eng.forward(x.contiguous(), taps)
    assert np.array_equal(t1.cpu().numpy().astype(np.int64), z["top1"])
    _check_against_fixture(li, taps, z, "engine", 7 * depth + 3)          # 7 QuantAct taps per block + stem + tail
    _check_against_fixture(ye, {}, z, "model(x)", 0)
    for lazy_on in (True, False):
        mt = {}
        ym = _module_path(model, x, lazy_on, mt)
        _check_against_fixture(ym, mt, z, f"module path (lazy {lazy_on})", len(z["tap_names"]))
        assert torch.equal(ym, ye)


SWIN_TAGS = ["swin_rect", "swin_rect_natural", "swin_rect_tall", "swin_rect_tall_natural"]


@pytest.mark.parametrize("tag", SWIN_TAGS)
def test_swin_engine_matches_the_reference(tag):
    model, x, meta, z = _fixture_model(tag)
    depths = tuple(meta["dims"]["depths"])
    assert model.engine_unsupported_reason() is None and model.takes_engine(x)
    with torch.no_grad():
        ye = model(x)
        eng = model.engine(x.shape[0])
        assert eng.img_size == tuple(meta["img_size"]) and eng.pool_literal == (meta["regime"] == "natural")      # 98 / 48 tokens at the pool
        got = [[(b["win"], b["shift"]) for b in s["blocks"]] for s in eng.stages]
        assert got == [[tuple(v) for v in g[1]] for g in meta["grids"]], "the reference's own windows and shifts"
        taps = {}
        li, lf, t1 = eng.forward(x.contiguous(), taps)
    assert np.array_equal(t1.cpu().numpy().astype(np.int64), z["top1"])
    # per block qact1, attn.qact1, attn.qact3, qact2, qact3, mlp.qact_gelu, mlp.qact1, mlp.qact2, qact4; per merging two; stem 3, tail 2
    _check_against_fixture(li, taps, z, "engine", 9 * sum(depths) + 2 * (len(depths) - 1) + 5)
    _check_against_fixture(ye, {}, z, "model(x)", 0)


@pytest.mark.parametrize("lazy_on", [True, False], ids=["int8-carrying", "literal"])
@pytest.mark.parametrize("tag", SWIN_TAGS)
def test_swin_module_path_matches_the_reference(tag, lazy_on):
    """The module path against the fixture's INT32 logits, top-1 and every tap, and against the engine's logits.  The two natural
    fixtures pool an even token count (98 and 48), where a column's float mean can be an exact .5 tie of qact3: the fixture is the
    reference on the CPU, and SwinTransformer._pool_tokens takes that mean in the CPU's order (ivit_avgpool_f32_literal).  With
    CUDA's own mean `qact3` -- and only it -- missed the fixture: 995 of 3000 INT32 logits in swin_rect_natural (image 2), 1992 of
    3000 in swin_rect_tall_natural (images 0 and 1), top-1 unchanged."""
    model, x, meta, z = _fixture_model(tag)
    with torch.no_grad():
        ye = model(x)
    mt = {}
    ym = _module_path(model, x, lazy_on, mt)
    gold = dict(zip([str(n) for n in z["tap_names"]], z["tap_crc32"]))
    bad = sorted(n for n in gold if crc(mt[n]) != int(gold[n]))
    li = torch.round(ym.cpu().double() / torch.from_numpy(z["head_scale"]).double()).to(torch.int32).numpy()
    print(f"{tag} lazy={lazy_on}: taps differing from the fixture {bad} of {len(gold)}; INT32 logits differing {int((li != z['logits_int32']).sum())} "
          f"of {li.size} in images {sorted(set(np.nonzero(li != z['logits_int32'])[0].tolist()))}; top-1 {ym.argmax(dim=1).cpu().tolist()} "
          f"against {z['top1'].tolist()}; logits differing from the engine's {int((ym != ye).sum())}")
    _check_against_fixture(ym, mt, z, f"module path (lazy {lazy_on})", len(z["tap_names"]))
    assert torch.equal(ym, ye)


def test_swin_ibert_engine_equals_its_module_path():
    """gelu / softmax / layernorm 'ibert' at (56, 112): swin_engine.engine_from_model (model(x) dispatches the I-ViT family only).
    Ranges snapped to powers of two: the 98-token tail pools in integers on both paths"""
    torch.manual_seed(56112)
    model = ivit.SwinTransformer(img_size=(56, 112), patch_size=4, window_size=7, embed_dim=64, depths=(2, 2), num_heads=(2, 4), num_classes=10,
                                 gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert").to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(9)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if prm.dim() > 1:
                prm.mul_(3.0)
            elif name.endswith("relative_position_bias_table"):
                prm.mul_(20.0)
        calib = _images(4, (56, 112), g)
        model(calib)
        model(calib.flip(0) * 0.7)
    snap_pow2(model)
    ivit.freeze_model(model)
    x = _images(3, (56, 112), g)
    assert "operator family" in model.engine_unsupported_reason() and model.engine_structure_reason() is None
    eng = engine_from_model(model, max_batch=4)
    assert eng.family == "ibert" and eng.img_size == (56, 112) and not eng.pool_literal
    t_mod, t_eng = {}, {}
    y = _module_path(model, x, True, t_mod)
    lf = eng.forward(x.contiguous(), taps=t_eng)[1].clone()
    assert torch.equal(lf[:, :10], y) and len(torch.unique(y)) > 3
    assert len(t_eng) == 9 * 4 + 2 + 5 and set(t_eng) <= set(t_mod)
    for name, t in t_eng.items():
        a, b = t.reshape(-1).to(torch.int32), t_mod[name].reshape(-1)
        assert a.numel() == b.numel() and torch.equal(a, b), f"tap {name}: {int((a != b).sum())} of {a.numel()} differ"
    assert torch.equal(eng.forward(x.contiguous())[1][:, :10], y)          # without taps: the fused projection


# =========================================================================================== feature maps, attention maps
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def _hooked(model, fn):
    model.use_engine = False
    try:
        with torch.no_grad():
            return fn()
    finally:
        model.use_engine = True


@pytest.mark.parametrize("integers", [False, True])
def test_vit_feature_maps_equal_the_hook_path(integers):
    model, g = _vit((64, 96), 16, W8)
    x = _images(3, (64, 96), g)
    with torch.no_grad():
        assert model.takes_engine(x)
        maps, scales = model.forward_intermediates(x, None, integers)
    ref, ref_s = _hooked(model, lambda: model.forward_intermediates(x, None, integers))
    assert list(maps) == list(ref) == [0, 1] and scales == ref_s
    for i in maps:
        assert tuple(maps[i].shape) == (3, 128, 4, 6) and maps[i].dtype == (torch.int8 if integers else torch.float32)
        assert _same(maps[i], ref[i]), f"block {i}: {int((maps[i] != ref[i]).sum())} of {maps[i].numel()} differ from the hook path"
        assert len(torch.unique(maps[i])) > 4


@pytest.mark.parametrize("integers", [False, True])
def test_swin_feature_maps_equal_the_hook_path(integers):
    model, x, meta, _ = _fixture_model("swin_rect")
    with torch.no_grad():
        assert model.takes_engine(x)
        maps, scales = model.forward_intermediates(x, None, integers)
    ref, ref_s = _hooked(model, lambda: model.forward_intermediates(x, None, integers))
    assert list(maps) == list(ref) == [0, 1] and scales == ref_s
    B = x.shape[0]
    assert [tuple(m.shape) for m in maps.values()] == [(B, 64, 14, 28), (B, 128, 7, 14)]
    for li in maps:
        assert maps[li].dtype == (torch.int16 if integers else torch.float32)
        assert _same(maps[li], ref[li]), f"stage {li}: {int((maps[li] != ref[li]).sum())} of {maps[li].numel()} differ from the hook path"
        assert len(torch.unique(maps[li])) > 16


def test_swin_attention_maps_equal_the_hook_path():
    model, x, meta, _ = _fixture_model("swin_rect")
    with torch.no_grad():
        assert model.takes_engine(x)
        maps, scale = model.attention_maps(x)
    ref, ref_scale = _hooked(model, lambda: model.attention_maps(x))
    B = x.shape[0]
    assert scale == ref_scale == 2.0 ** -7 and list(maps) == list(ref) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [tuple(m.shape) for m in maps.values()] == [(B, 8, 2, 49, 49)] * 2 + [(B, 2, 4, 49, 49)] * 2
    for key in maps:
        assert maps[key].dtype == torch.uint8 and torch.equal(maps[key], ref[key]), \
            f"{key}: {int((maps[key] != ref[key]).sum())} of {maps[key].numel()} probabilities differ from the hook path"
        assert len(torch.unique(maps[key])) > 8
    assert bool((maps[(0, 1)] == 0).any())                 # the shift mask of the 14 x 28 map


def test_vit_attention_maps_equal_the_hook_path():
    model, g = _vit((64, 96), 16, W8)
    x = _images(3, (64, 96), g)
    with torch.no_grad():
        assert model.takes_engine(x)
        maps, scale = model.attention_maps(x, rows="all")
    ref, ref_scale = _hooked(model, lambda: model.attention_maps(x, rows="all"))
    assert scale == ref_scale == 2.0 ** -7 and list(maps) == list(ref) == [0, 1]
    for i in maps:
        assert tuple(maps[i].shape) == (3, 2, 25, 25) and torch.equal(maps[i], ref[i]), \
            f"block {i}: {int((maps[i] != ref[i]).sum())} of {maps[i].numel()} probabilities differ from the hook path"
        assert len(torch.unique(maps[i])) > 8
