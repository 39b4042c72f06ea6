"""Images that are not square, without a GPU: the prototypes of the two ivit_quantize_patchify_hw_* entries against the ctypes table
(the helper pattern of tests/test_feature_maps_cpu.py), the geometry rules of both engines and both model classes, the host row maps
and shift masks for H != W against the mirror's window_partition / torch.roll / attention mask (test_row_maps_for_large_windows of
tests/test_swin_384_cpu.py restated), the launches both engines issue with the native library stubbed (as
tests/test_attention_long_cpu.py stubs it), and the schema of the fixtures of scripts/gen_rect_golden.py.
(The kernels and the models themselves: tests/test_gpu_rect.py.)"""
import ctypes
import json
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import ivit_amd as ivit
from ivit_amd import _lib, synth
from ivit_amd.checkpoint import GOLDEN_DIR, load_dims_model
from ivit_amd.engine import IntViTEngine
from ivit_amd.quantization_utils import IntLayerNorm
from ivit_amd.swin_engine import IntSwinEngine, shift_mask_regions, unsupported_geometry, window_row_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW_F32, HW_U8 = "ivit_quantize_patchify_hw_f32_i8", "ivit_quantize_patchify_hw_u8_i8"
SQUARE = ("ivit_quantize_patchify_f32_i8", "ivit_quantize_patchify_ld_f32_i8", "ivit_quantize_patchify_u8_i8")
TAGS = [t + r for t in ("deit_rect", "deit_rect_ibert", "swin_rect", "swin_rect_tall") for r in ("", "_natural")]


# ---------------------------------------------------------------------------- prototypes
def _prototype(name):
    """(ctypes kinds, parameter names) `name` is declared with in include/ivit_hip.h"""
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\s*\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const float*": _lib.vp, "const uint8_t*": _lib.vp, "const int8_t*": _lib.vp, "int8_t*": _lib.vp, "int": _lib.ci,
             "int64_t": _lib.i64, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    return [kinds[re.sub(r"\s+\w+$", "", p)] for p in params], [re.findall(r"\w+", p)[-1] for p in params]


def test_pooling_prototype_matches_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int ivit_avgpool_f32_literal\(([^)]*)\);", hdr)
    assert m, "ivit_avgpool_f32_literal is not declared"
    kinds = {"const float*": _lib.vp, "float*": _lib.vp, "int": _lib.ci, "ivit_stream_t": _lib.vp}
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert _lib.SIGNATURES["ivit_avgpool_f32_literal"] == [kinds[re.sub(r"\s+\w+$", "", p)] for p in params]
    assert [re.findall(r"\w+", p)[-1] for p in params] == ["x", "out", "batch", "tokens", "C", "stream"]


def test_module_path_pools_in_cpu_order_only_where_ties_can_differ(monkeypatch):
    """SwinTransformer._pool_tokens: ivit_avgpool_f32_literal for a dense tensor on the GPU with an even token count at a scale that
    is not a power of two; torch's own avgpool everywhere else (CPU tensors, odd counts, power-of-two scales, strided tensors)"""
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: rec.append((name, a)))
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    m = ivit.SwinTransformer(img_size=(56, 112), patch_size=4, window_size=7, num_classes=10, embed_dim=64, depths=(1, 1), num_heads=(2, 4))
    nat, p2 = torch.tensor([0.0371]), torch.tensor([0.03125])
    x = torch.randn(2, 98, 128)
    want = m.avgpool(x.transpose(1, 2))
    assert torch.equal(m._pool_tokens(x, nat), want) and rec == []                      # a CPU tensor: the reference's call
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    out = m._pool_tokens(x, nat)
    (name, a), = rec
    assert name == "ivit_avgpool_f32_literal" and a[0] == x.data_ptr() and a[2:5] == (2, 98, 128) and tuple(out.shape) == (2, 128, 1)
    del rec[:]
    assert torch.equal(m._pool_tokens(x, p2), want) and rec == []                       # a power-of-two scale
    assert torch.equal(m._pool_tokens(x[:, :49], nat), m.avgpool(x[:, :49].transpose(1, 2))) and rec == []      # an odd count
    xt = torch.randn(2, 128, 98).transpose(1, 2)                                        # the transposed layout of a one-stage model
    assert torch.equal(m._pool_tokens(xt, nat), m.avgpool(xt.transpose(1, 2))) and rec == []


@pytest.mark.parametrize("name,last", [(HW_F32, "inv_scale"), (HW_U8, "lut")])
def test_prototypes_match_ctypes_table(name, last):
    kinds, names = _prototype(name)
    assert _lib.SIGNATURES[name] == kinds
    assert names == ["img", "A", "lda", "batch", "chans", "h", "w", "patch", last, "stream"]


# ---------------------------------------------------------------------------- geometry rules
@pytest.mark.parametrize("img,window,stages", [((56, 112), 7, 2), ((112, 56), 7, 2), ((96, 32), 8, 2), ((224, 448), 7, 4), (224, 7, 4),
                                               ((56, 56), 7, 2)])
def test_swin_geometry_accepted(img, window, stages):
    assert unsupported_geometry(img, 4, window, stages) is None
    assert unsupported_geometry(img, (4, 4), window, stages) is None


@pytest.mark.parametrize("img,window,stages,what", [
    ((56, 100), 7, 2, "whole number"),          # 25 columns are not a multiple of 7
    ((56, 120), 7, 2, "whole number"),          # 30 (and stage 1's 15) columns are not whole windows
    ((72, 216), 9, 3, "cannot be merged"),      # stage 1's 9 x 27 map
    ((104, 208), 13, 1, "169 tokens"),          # a window above 144 tokens
    ((56, 114), 7, 2, "multiple of the patch"),
])
def test_swin_geometry_refused(img, window, stages, what):
    why = unsupported_geometry(img, 4, window, stages)
    assert why is not None and "geometry" in why and what in why, why


def test_swin_refuses_non_square_patches():
    for patch in ((4, 8), (8, 4), 8):
        assert "geometry" in unsupported_geometry((56, 112), patch, 7, 2)
    kw = dict(window_size=7, num_classes=10, norm_layer=partial(IntLayerNorm, eps=1e-6), embed_dim=64, depths=(2, 2), num_heads=(2, 4))
    assert "geometry" in ivit.SwinTransformer(img_size=(56, 112), patch_size=(4, 8), **kw).engine_unsupported_reason()
    assert ivit.SwinTransformer(img_size=(56, 112), patch_size=4, **kw).engine_unsupported_reason() is None
    assert ivit.SwinTransformer(img_size=(112, 56), patch_size=4, **kw).engine_structure_reason() is None
    # 14 x 25 map: not whole windows (one unshifted block per stage: the mirror builds no mask for it, so it can be constructed)
    assert "geometry" in ivit.SwinTransformer(img_size=(56, 100), patch_size=4, **dict(kw, depths=(1, 1))).engine_unsupported_reason()


def test_vit_rule():
    kw = dict(patch_size=16, embed_dim=128, depth=1, num_heads=2, num_classes=10)
    m = ivit.VisionTransformer(img_size=(64, 96), **kw)
    assert m.engine_unsupported_reason() is None and m.geometry[0] == (64, 96)
    assert ivit.VisionTransformer(img_size=(96, 64), **kw).engine_unsupported_reason() is None
    assert ivit.VisionTransformer(img_size=64, **kw).engine_unsupported_reason() is None
    assert "geometry" in ivit.VisionTransformer(img_size=(64, 100), **kw).engine_unsupported_reason()
    assert "geometry" in ivit.VisionTransformer(img_size=(512, 528), **kw).engine_unsupported_reason()      # 1057 tokens
    # I-BERT: 193 .. 207 tokens, counted on both axes
    ib = dict(kw, gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
    assert ivit.VisionTransformer(img_size=(192, 256), **ib).engine_unsupported_reason() is None
    assert "193 .. 207" in ivit.VisionTransformer(img_size=(64, 96), **ib).engine_unsupported_reason()


# ---------------------------------------------------------------------------- row maps and masks
@pytest.mark.parametrize("H,W,ws,shift", [(14, 28, 7, 3), (28, 14, 7, 3), (24, 8, 8, 0), (16, 32, 8, 4)])
def test_row_maps_and_masks_for_rectangular_maps(H, W, ws, shift):
    """window_row_map / shift_mask_regions against the mirror's window_partition / torch.roll and its attention mask"""
    from ivit_amd.swin_quant import SwinTransformerBlock, window_partition
    B = 2
    tok = torch.arange(B * H * W).reshape(B, H, W, 1)
    rolled = torch.roll(tok, shifts=(-shift, -shift), dims=(1, 2)) if shift else tok
    order = window_partition(rolled, ws).reshape(-1).numpy()        # window-ordered row -> image row
    dst = window_row_map(B, H, W, ws, shift)                         # image row -> window-ordered row
    assert sorted(dst.tolist()) == list(range(B * H * W))
    assert np.array_equal(order[dst], np.arange(B * H * W))
    blk = SwinTransformerBlock(32, (H, W), 1, window_size=ws, shift_size=shift)
    assert (blk.window_size, blk.shift_size) == (ws, shift)
    if shift:
        reg = shift_mask_regions(H, W, ws, shift)
        assert reg.shape == ((H // ws) * (W // ws), ws * ws)
        mask = blk.attn_mask.numpy()
        assert np.array_equal(mask != 0, reg[:, :, None] != reg[:, None, :]) and (mask != 0).any()
    else:
        assert blk.attn_mask is None


# ---------------------------------------------------------------------------- launches, with the library stubbed
@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(name, *args):
        if name == "ivit_ibert_softmax_build_table":      # engine_common reads the table back to choose the band form
            ctypes.memset(args[-2], 0, 65536 * 4)
        rec.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "lib", lambda: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return rec


def _patchify_calls(calls):
    return [(n, a) for n, a in calls if "patchify" in n]


def test_vit_engine_issues_the_hw_entry_for_rectangular_images_only(calls):
    fs, ranges, meta, _ = load_dims_model("deit_rect")
    d = meta["dims"]
    eng = IntViTEngine(fs, ranges, d["embed_dim"], d["depth"], d["num_heads"], device="cpu", max_batch=2, img_size=(64, 96), patch_size=16)
    assert (eng.NP, eng.T, eng.grid, eng.IMG) == (24, 25, (4, 6), (64, 96))
    del calls[:]
    eng.forward(torch.zeros(2, 3, 64, 96))
    (name, a), = _patchify_calls(calls)
    assert name == HW_F32 and len(a) == len(_lib.SIGNATURES[HW_F32])
    assert a[2:8] == (768, 2, 3, 64, 96, 16) and a[8] == eng.inv_s0
    gemm = next(a for n, a in calls if n.startswith("ivit_gemm"))
    assert 2 * 24 in gemm                                                 # the patch GEMM runs B * Gh * Gw rows
    del calls[:]
    eng.set_input_normalisation()
    eng.forward(torch.zeros(2, 3, 64, 96, dtype=torch.uint8))
    (name, a), = _patchify_calls(calls)
    assert name == HW_U8 and a[2:8] == (768, 2, 3, 64, 96, 16) and a[8] == eng.input_lut.data_ptr()
    # the transposed model is another model: (96, 64) images, the same token count
    fs_t = synth.make_float_state_dims(d["embed_dim"], d["depth"], meta["weight_seed"], (96, 64), 16)
    eng_t = IntViTEngine(fs_t, ranges, d["embed_dim"], d["depth"], d["num_heads"], device="cpu", max_batch=2, img_size=[96, 64], patch_size=16)
    del calls[:]
    eng_t.forward(torch.zeros(1, 3, 96, 64))
    (name, a), = _patchify_calls(calls)
    assert name == HW_F32 and a[2:8] == (768, 1, 3, 96, 64, 16) and eng_t.grid == (6, 4)
    with pytest.raises(AssertionError):
        eng_t.forward(torch.zeros(1, 3, 64, 96))
    # a square engine keeps the square entries, whether img_size is an int or a pair of equal ints
    fs_s = synth.make_float_state_dims(d["embed_dim"], d["depth"], meta["weight_seed"], 64, 16)
    for size in (64, (64, 64)):
        sq = IntViTEngine(fs_s, ranges, d["embed_dim"], d["depth"], d["num_heads"], device="cpu", max_batch=2, img_size=size, patch_size=16)
        assert sq.IMG == 64 and sq.T == 17
        del calls[:]
        sq.forward(torch.zeros(2, 3, 64, 64))
        (name, a), = _patchify_calls(calls)
        assert name == "ivit_quantize_patchify_f32_i8" and a[2:6] == (2, 3, 64, 16)
    with pytest.raises(ValueError, match="geometry"):
        IntViTEngine(fs, ranges, d["embed_dim"], d["depth"], d["num_heads"], device="cpu", max_batch=2, img_size=(64, 100), patch_size=16)


def test_vit_engine_feature_maps_are_gh_by_gw(calls):
    fs, ranges, meta, _ = load_dims_model("deit_rect")
    d = meta["dims"]
    eng = IntViTEngine(fs, ranges, d["embed_dim"], d["depth"], d["num_heads"], device="cpu", max_batch=2, img_size=(64, 96), patch_size=16)
    maps, scales = eng.forward_intermediates(torch.zeros(2, 3, 64, 96), (1,))
    assert tuple(maps[1].shape) == (2, 128, 4, 6) and list(scales) == [1]
    probs, _ = eng.attention_maps(torch.zeros(2, 3, 64, 96), rows="all")
    assert all(tuple(p.shape) == (2, 2, 25, 25) for p in probs.values())


def test_swin_engine_issues_the_hw_entry_for_rectangular_images_only(calls):
    fs, ranges, meta, _ = load_dims_model("swin_rect")
    d = meta["dims"]
    args = (d["embed_dim"], tuple(d["depths"]), tuple(d["num_heads"]), d["window"])
    eng = IntSwinEngine(fs, ranges, *args, device="cpu", max_batch=2, img_size=(56, 112))
    assert eng.img_size == (56, 112) and eng.T_last == 7 * 14 and eng.C_last == 128
    del calls[:]
    eng.forward(torch.zeros(2, 3, 56, 112))
    (name, a), = _patchify_calls(calls)
    assert name == HW_F32 and a[2:8] == (64, 2, 3, 56, 112, 4) and a[8] == eng.inv_s0
    stem_ln = next(a for n, a in calls if "layernorm" in n)
    assert 2 * 14 * 28 in stem_ln                                         # the stem's M
    merge = next(a for n, a in calls if n == "ivit_patch_merge_i16")
    assert merge[2:6] == (2, 14, 28, 64)
    pool = next(a for n, a in calls if n.startswith("ivit_avgpool"))
    assert pool[2:5] == (2, 98, 128)
    del calls[:]
    eng.set_input_normalisation()
    eng.forward(torch.zeros(1, 3, 56, 112, dtype=torch.uint8))
    (name, a), = _patchify_calls(calls)
    assert name == HW_U8 and a[2:8] == (64, 1, 3, 56, 112, 4)
    maps, _ = eng.forward_intermediates(torch.zeros(2, 3, 56, 112))
    assert [tuple(m.shape) for m in maps.values()] == [(2, 64, 14, 28), (2, 128, 7, 14)]
    probs, _ = eng.attention_maps(torch.zeros(2, 3, 56, 112))
    assert [tuple(p.shape) for p in probs.values()] == [(2, 8, 2, 49, 49)] * 2 + [(2, 2, 4, 49, 49)] * 2
    # square: the entries it always called
    fs_s = synth.make_swin_float_state_dims(*args, meta["weight_seed"], 56)
    for size in (56, (56, 56)):
        sq = IntSwinEngine(fs_s, ranges, *args, device="cpu", max_batch=2, img_size=size)
        assert sq.img_size == 56
        del calls[:]
        sq.forward(torch.zeros(2, 3, 56, 56))
        (name, a), = _patchify_calls(calls)
        assert name == "ivit_quantize_patchify_ld_f32_i8" and a[2:7] == (64, 2, 3, 56, 4)
    with pytest.raises(ValueError, match="geometry"):
        IntSwinEngine(fs, ranges, *args, device="cpu", max_batch=2, img_size=(56, 100))


def test_swin_engine_stage_geometry_equals_the_mirrors_blocks(calls):
    """(96, 32) / 8: a 24 x 8 map in three 8 x 8 windows, then a 12 x 4 map in 4 x 4 windows -- min(H, W), not min(window, H)"""
    fs, ranges, meta, _ = load_dims_model("swin_rect_tall")
    d = meta["dims"]
    args = (d["embed_dim"], tuple(d["depths"]), tuple(d["num_heads"]), d["window"])
    eng = IntSwinEngine(fs, ranges, *args, device="cpu", max_batch=2, img_size=(96, 32))
    model = ivit.SwinTransformer(img_size=(96, 32), patch_size=4, window_size=8, num_classes=10, norm_layer=partial(IntLayerNorm, eps=1e-6),
                                 embed_dim=64, depths=(2, 2), num_heads=(2, 4))
    got = [(s["H"], s["W"], b["win"], b["shift"], b["attn"]["nW"]) for s in eng.stages for b in s["blocks"]]
    want = [(*layer.input_resolution, blk.window_size, blk.shift_size, (layer.input_resolution[0] // blk.window_size) *
             (layer.input_resolution[1] // blk.window_size)) for layer in model.layers for blk in layer.blocks]
    assert got == want == [(24, 8, 8, 0, 3)] * 2 + [(12, 4, 4, 0, 3)] * 2
    assert [[tuple(x) for x in g[1]] for g in meta["grids"]] == [[(8, 0), (8, 0)], [(4, 0), (4, 0)]]      # the reference's own blocks
    for s in eng.stages:
        for b in s["blocks"]:
            assert tuple(b["attn"]["bias"].shape)[:2] == (s["nH"], b["win"] ** 2)
    # the shifted wide model: the mirror's blocks again
    fs, ranges, meta, _ = load_dims_model("swin_rect")
    eng = IntSwinEngine(fs, ranges, *args[:3], 7, device="cpu", max_batch=2, img_size=(56, 112))
    got = [(s["H"], s["W"], b["win"], b["shift"], b["attn"]["nW"]) for s in eng.stages for b in s["blocks"]]
    assert got == [(14, 28, 7, 0, 8), (14, 28, 7, 3, 8), (7, 14, 7, 0, 2), (7, 14, 7, 0, 2)]
    assert tuple(eng.stages[0]["blocks"][1]["attn"]["region"].shape)[0] == 8 and eng.stages[1]["blocks"][1]["attn"]["region"] is None


# ---------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_schema(tag):
    z = np.load(os.path.join(GOLDEN_DIR, f"{tag}.npz"), allow_pickle=False)
    assert os.path.getsize(os.path.join(GOLDEN_DIR, f"{tag}.npz")) < 64 * 1024
    meta = json.loads(str(z["meta"]))
    ih, iw = meta["img_size"]
    assert ih != iw and meta["tag"] == tag and meta["regime"] == ("natural" if tag.endswith("_natural") else "pow2")
    assert meta["kind"] in ("vit", "swin") and list(meta["dims"]["img_size"]) == [ih, iw]
    n = meta["n_images"]
    assert z["logits_int32"].shape == (n, meta["num_classes"]) and z["logits_int32"].dtype == np.int32
    assert z["top1"].shape == (n,) and np.array_equal(z["top1"], z["logits_f32_bits"].view(np.float32).argmax(1))
    assert z["head_scale"].shape == (meta["num_classes"],) and len(z["tap_names"]) == len(z["tap_crc32"]) > 10
    assert len(z["range_names"]) == len(z["x_min"]) == len(z["x_max"]) == len(z["range_bits"])
    pow2 = np.log2(z["x_max"].astype(np.float64) / (2.0 ** (z["range_bits"] - 1) - 1))
    assert bool((pow2 == np.rint(pow2)).all()) == (meta["regime"] == "pow2")
    fs, ranges, meta2, _ = load_dims_model(tag)
    assert meta2 == meta and set(ranges) == {str(s) for s in z["range_names"]}
    if meta["kind"] == "vit":
        gh, gw = ih // meta["dims"]["patch"], iw // meta["dims"]["patch"]
        assert fs["pos_embed"].shape == (1, gh * gw + 1, meta["dims"]["embed_dim"]) and meta["grids"] == [[gh, gw]]
        assert list(ranges) == synth.qact_names(meta["dims"]["depth"], meta["operators"])
        assert (len(z["shift_names"]) > 0) == (meta["operators"] == "ibert")
    else:
        assert list(ranges) == synth.swin_qact_names(tuple(meta["dims"]["depths"]))
        assert [g[0] for g in meta["grids"]] == [[ih // 4, iw // 4], [ih // 8, iw // 8]]
