"""GPU: the evaluation transform with an h x w crop, an exact-size resize and zero padding (ivit_resize_crop_bicubic_hw_u8) against
the numpy restatement (tests/eval_rect_ref.py) and Pillow's own bytes (tests/golden/eval_transform_rect_pil.npz), byte for byte;
the square entry on square crops; shards; compressed input; argument errors; a non-square DeiT and Swin evaluated from packed and
compressed batches through the engine, the module path and graph replay.  No Pillow needed."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference  # noqa: E402
from ivit_amd.transforms import (EvalTransform, ImageFolderJPEG, ImageFolderU8, encode_images, eval_geometry_hw,  # noqa: E402
                                 pack_images)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_rect_ref as E  # noqa: E402
import pil_resample_ref as R  # noqa: E402
from test_jpeg_cpu import CASES  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_transform_rect_pil.npz")
A5, WS_FILL, TAIL = 0xA5, 0x5A, 64

# (h, w): 33 to 200 px in both orientations, and two thin ones whose exact-size resizes need 39 taps and more
SIZES = [(33, 33), (200, 150), (47, 120), (120, 47), (97, 64), (64, 181), (150, 200), (33, 200), (199, 35), (81, 81), (600, 37), (37, 600)]
_CACHE = {}


def _images():
    if "images" not in _CACHE:
        rng = np.random.default_rng(41)
        _CACHE["images"] = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if i % 2 else R.smooth_image(rng, h, w)
                            for i, (h, w) in enumerate(SIZES)]
    return _CACHE["images"]


def _want(i, resize, crop, pad):
    """the restatement's crop of image i, computed once"""
    key = (i, resize, crop, pad)
    if key not in _CACHE:
        _CACHE[key] = E.resize_crop_hw(_images()[i], resize, crop, pad)
    return _CACHE[key]


def _resize_of(i, k, crop, pad):
    """image i's resize in the batch of crop number k: the sweep's ints and pairs in rotation; without pad, where that one would pad,
    an int or a pair just large enough; with pad, two images that are padded under every crop (odd differences 5 and 3 on both
    axes; a short side 2 below the crop's)"""
    r = E.SWEEP_RESIZES[(i + k) % len(E.SWEEP_RESIZES)]
    if pad and i in (8, 9):
        r = (crop[0] - 5, crop[1] - 3) if i == 9 else min(crop) - 2
    if not pad:
        nh, nw = E.resized_size(*SIZES[i], r)
        if crop[0] > nh or crop[1] > nw:
            r = (crop[0] + i, crop[1] + 2 * i + 1) if i % 2 else max(crop) + i
    return r


def _rows(sizes, resizes, crop, pad):
    """the geometry table of a batch with one resize per image, row by row from the library's host function"""
    L = _lib.lib()
    g = np.empty((len(sizes), 6), np.int32)
    out4 = (C.c_int32 * 4)()
    for b, ((h, w), r) in enumerate(zip(sizes, resizes)):
        rh, rw = (r, 0) if isinstance(r, int) else r
        assert L.ivit_eval_geometry_hw(h, w, rh, rw, crop[0], crop[1], int(pad), out4) == 0, L.ivit_last_error_string().decode()
        g[b] = (h, w, *out4)
    return g


def _run_hw(packed, geom, crop):
    """ivit_resize_crop_bicubic_hw_u8 into an output pre-filled with 0xA5, sentinel bytes behind it and behind a workspace of exactly
    the planned size -> (uint8 [n, 3, ch, cw], plan)"""
    L = _lib.lib()
    n, (ch, cw) = len(geom), crop
    plan, nb = (C.c_int32 * 3)(), C.c_int64()
    assert L.ivit_resize_crop_workspace_hw(geom.ctypes.data_as(C.c_void_p), n, ch, cw, plan, C.byref(nb)) == 0, \
        L.ivit_last_error_string().decode()
    assert nb.value % 16 == 0 and nb.value > 0
    src = packed.data.to(DEV)
    offs = torch.from_numpy(packed.offsets).to(DEV)
    g = torch.from_numpy(geom).to(DEV)
    ws = torch.full((nb.value + TAIL,), WS_FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((n * 3 * ch * cw + TAIL,), A5, dtype=torch.uint8, device=DEV)
    _lib.call("ivit_resize_crop_bicubic_hw_u8", _lib.ptr(src), _lib.ptr(offs), _lib.ptr(g), n, ch, cw, plan[0], plan[1], plan[2],
              _lib.ptr(ws), nb.value, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((ws[nb.value:] == WS_FILL).all()), "bytes behind the workspace were written"
    assert bool((out[n * 3 * ch * cw:] == A5).all()), "bytes behind out were written"
    return out[:n * 3 * ch * cw].view(n, 3, ch, cw).cpu().numpy(), tuple(plan)


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "nopad"])
@pytest.mark.parametrize("k", range(len(E.CROPS)), ids=["%dx%d" % c for c in E.CROPS])
def test_kernel_equals_restatement_on_a_mixed_batch(k, pad):
    crop = E.CROPS[k]
    images = _images()
    resizes = [_resize_of(i, k, crop, pad) for i in range(len(images))]
    assert any(isinstance(r, int) for r in resizes) and any(isinstance(r, tuple) for r in resizes)
    geom = _rows(SIZES, resizes, crop, pad)
    padded = (geom[:, 4] < 0) | (geom[:, 5] < 0)
    assert padded[[8, 9]].all() if pad else not padded.any(), "the pad batches pad, the others do not"
    got, plan = _run_hw(pack_images(images), geom, crop)
    for i, r in enumerate(resizes):
        want = _want(i, r, crop, pad)
        assert geom[i].tolist() == [*SIZES[i], *E.eval_geometry_hw(*SIZES[i], r, crop, pad)]
        assert np.array_equal(got[i], want), (SIZES[i], r, crop, pad, int((got[i] != want).sum()))
        top, left = int(geom[i, 4]), int(geom[i, 5])
        assert not want[:, :max(0, -top)].any() and not want[:, :, :max(0, -left)].any()          # the zeros in front
    if k == 0:
        assert min(plan[:2]) >= 39, plan          # the thin sources at an exact size: 39 taps per pixel on either axis
    # the same rows through EvalTransform when the batch has one resize: image by image
    for i in (1, 10, 11):
        t = EvalTransform(resizes[i], crop, pad=True)          # (pad only permits padding: the bytes of an image that needs none are the same)
        assert np.array_equal(t(pack_images([images[i]]), device=DEV).cpu().numpy()[0], _want(i, resizes[i], crop, pad)), (i, resizes[i])


@pytest.mark.parametrize("s,c", [(37, 33), (73, 64), (65, 65), (96, 65)])
def test_square_crops_give_the_bytes_of_the_square_entry(s, c):
    images = _images()
    packed = pack_images(images)
    old = EvalTransform(s, c)
    assert old._square and not EvalTransform(s, (c, c))._square
    a = old(packed, device=DEV).cpu().numpy()
    geom = packed.geometry(s, (c, c))
    assert np.array_equal(geom, packed.geometry(s, c))
    b, _ = _run_hw(packed, geom, (c, c))
    assert np.array_equal(a, b)
    assert np.array_equal(a, EvalTransform(s, (c, c))(packed, device=DEV).cpu().numpy())
    assert np.array_equal(a[2], R.resize_crop(images[2], s, c)) and len(np.unique(a)) > 200


def test_kernel_equals_pillow_fixture():
    z = np.load(GOLDEN)
    images = E.fixture_images()
    for i, (img, ((h, w), r, crop)) in enumerate(zip(images, E.FIXTURE_CASES)):
        assert hashlib.sha256(img.tobytes()).digest() == z[f"sha256_{i}"].tobytes(), "fixture sources regenerated differently"
        t = EvalTransform(r, crop, pad=True)
        out = torch.full((1, 3, *t.crop_hw), A5, dtype=torch.uint8, device=DEV)
        got = t(pack_images([img]), device=DEV, out=out)
        assert got is out and np.array_equal(out.cpu().numpy()[0], z[f"crop_{i}"]), (i, (h, w), r, crop)
    # the cases that share a crop as one batch, each row with its own resize
    idx = [i for i, case in enumerate(E.FIXTURE_CASES) if case[2] == (64, 96)]
    assert len(idx) >= 3
    geom = _rows([E.FIXTURE_CASES[i][0] for i in idx], [E.FIXTURE_CASES[i][1] for i in idx], (64, 96), True)
    got, _ = _run_hw(pack_images([images[i] for i in idx]), geom, (64, 96))
    for j, i in enumerate(idx):
        assert np.array_equal(got[j], z[f"crop_{i}"]), i


def test_shards_batch_one_and_batch_zero():
    images = _images()
    packed = pack_images(images)
    k, crop = 4, E.CROPS[4]
    for r, pad in ((48, True), ((65, 34), True), (109, False)):
        t = EvalTransform(r, crop, pad=pad)
        whole = t(packed, device=DEV).cpu().numpy()
        assert whole.shape == (len(images), 3, *crop)
        for i in (0, 3, 10):
            assert np.array_equal(whole[i], _want(i, r, crop, pad)), (i, r)
        for lo, hi in ((0, 12), (3, 9), (11, 12), (0, 1), (5, 5), (12, 12)):
            got = t(packed, lo, hi, device=DEV)
            assert got.shape == (hi - lo, 3, *crop) and np.array_equal(got.cpu().numpy(), whole[lo:hi]), (r, lo, hi)
        with pytest.raises(IndexError):
            t(packed, 5, 13, device=DEV)
        with pytest.raises(ValueError, match=r"\[6, 3, 64, 96\]"):
            t(packed, 3, 9, device=DEV, out=torch.empty(6, 3, 96, 64, dtype=torch.uint8, device=DEV))
    # batch 0 through the entry itself: nothing launched, nothing written
    L = _lib.lib()
    plan, nb = (C.c_int32 * 3)(), C.c_int64()
    geom = packed.geometry(48, crop, True)
    assert L.ivit_resize_crop_workspace_hw(geom.ctypes.data_as(C.c_void_p), 0, *crop, plan, C.byref(nb)) == 0 and tuple(plan) == (1, 1, 1)
    ws = torch.full((max(nb.value, 16),), WS_FILL, dtype=torch.uint8, device=DEV)
    out = torch.full((64,), A5, dtype=torch.uint8, device=DEV)
    assert L.ivit_resize_crop_bicubic_hw_u8(_lib.ptr(packed.data.to(DEV)), _lib.ptr(torch.zeros(1, dtype=torch.int64, device=DEV)),
                                            _lib.ptr(torch.from_numpy(geom).to(DEV)), 0, *crop, *plan, _lib.ptr(ws), nb.value,
                                            _lib.ptr(out), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out == A5).all()) and bool((ws == WS_FILL).all())


def _small_jpegs():
    cases = [c for c in CASES if c["supported"] and c["pixels"] is not None and c["h"] * c["w"] > 1]
    assert len(cases) >= 10
    return cases


def test_encoded_images_equal_packed_images():
    cases = _small_jpegs()
    enc = encode_images([c["data"] for c in cases])
    assert not enc.fallback
    packed = pack_images([c["pixels"] for c in cases])
    for r, crop, pad in ((40, (34, 65), True), ((40, 56), (40, 56), False), (109, (64, 96), False), ((35, 50), (64, 96), True)):
        t = EvalTransform(r, crop, pad=pad)
        a = t(packed, device=DEV).cpu().numpy()
        assert np.array_equal(t(enc, device=DEV).cpu().numpy(), a), (r, crop)
        assert np.array_equal(enc.geometry(r, crop, pad), packed.geometry(r, crop, pad))
        for lo, hi in ((0, 4), (4, 5), (5, len(cases))):
            assert np.array_equal(t(enc, lo, hi, device=DEV).cpu().numpy(), a[lo:hi]), (r, crop, lo, hi)
        assert np.array_equal(a[3], E.resize_crop_hw(cases[3]["pixels"], r, crop, pad))


def test_argument_errors():
    L = _lib.lib()
    rng = np.random.default_rng(3)
    packed = pack_images([rng.integers(0, 256, (90, 120, 3), dtype=np.uint8)])
    ch, cw = 64, 96
    geom = packed.geometry(70, (ch, cw), True)                      # 70 x 93: no rows padded, 3 columns padded
    assert geom[0].tolist() == [90, 120, 70, 93, 3, -1]
    plan, nb = (C.c_int32 * 3)(), C.c_int64()

    def workspace(g=geom, batch=1, crop=(ch, cw), plan_=plan, nb_=C.byref(nb)):
        return L.ivit_resize_crop_workspace_hw(None if g is None else g.ctypes.data_as(C.c_void_p), batch, *crop, plan_, nb_)

    assert workspace() == 0
    src = packed.data.to(DEV)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    g = torch.from_numpy(geom).to(DEV)
    ws = torch.empty(nb.value + 16, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, ch, cw), A5, dtype=torch.uint8, device=DEV)
    p = _lib.ptr

    def run(src_=p(src), offs_=p(offs), g_=p(g), batch=1, crop=(ch, cw), plan_=tuple(plan), ws_=p(ws), nbytes=nb.value, out_=p(out)):
        return L.ivit_resize_crop_bicubic_hw_u8(src_, offs_, g_, batch, *crop, *plan_, ws_, nbytes, out_, _lib.stream_ptr())

    def invalid(rc):
        return rc == -1 and L.ivit_last_error_string().decode().startswith("ivit_resize_crop_bicubic_hw_u8:")

    assert invalid(run(src_=None)) and invalid(run(offs_=None)) and invalid(run(g_=None)) and invalid(run(ws_=None)) and invalid(run(out_=None))
    assert invalid(run(ws_=C.c_void_p(ws.data_ptr() + 4))) and "misaligned" in L.ivit_last_error_string().decode()
    assert invalid(run(offs_=C.c_void_p(offs.data_ptr() + 4))) and invalid(run(g_=C.c_void_p(g.data_ptr() + 2)))
    assert invalid(run(nbytes=nb.value - 1)) and invalid(run(batch=-1)) and invalid(run(batch=65536))
    assert invalid(run(plan_=(0, plan[1], plan[2]))) and invalid(run(plan_=(plan[0], 0, plan[2]))) and invalid(run(plan_=(plan[0], plan[1], 0)))
    assert invalid(run(crop=(262141, cw)))
    for crop in ((32, cw), (ch, 32), (0, 0)):
        assert run(crop=crop) == -2 and "unsupported geometry" in L.ivit_last_error_string().decode()
    torch.cuda.synchronize()
    assert bool((out == A5).all()), "a refused call wrote to out"
    assert run(batch=0) == 0
    assert run() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy()[0], E.resize_crop_hw(packed.data.numpy().reshape(90, 120, 3), 70, (ch, cw), True))

    # the workspace function: per axis 0 <= off <= n - c, or c > n and -(c - n) <= off <= 0
    def row(**kw):
        r = dict(h=90, w=120, nh=70, nw=93, top=3, left=-1)
        r.update(kw)
        return np.array([[r[k] for k in ("h", "w", "nh", "nw", "top", "left")]], np.int32)

    for ok in (row(), row(top=0), row(top=6), row(left=0), row(left=-3), row(nh=64, top=0), row(nh=33, top=-31, nw=96, left=0)):
        assert workspace(g=ok) == 0, ok
    for bad in (row(top=-1), row(top=7), row(left=1), row(left=-4), row(h=0), row(w=0), row(nh=0, top=-32), row(nw=0, left=-48),
                row(nh=33, top=-32), row(nh=33, top=1), row(nw=96, left=1), row(nw=96, left=-1)):
        assert workspace(g=bad) == -2 and "unsupported geometry" in L.ivit_last_error_string().decode(), bad
    for crop in ((32, cw), (ch, 32)):
        assert workspace(crop=crop) == -2 and "unsupported geometry" in L.ivit_last_error_string().decode()
    assert workspace(g=None) == -1 and workspace(plan_=None) == -1 and workspace(nb_=None) == -1 and workspace(batch=-1) == -1
    # the square entries keep their refusals: a crop that leaves the resized image, a negative offset
    sq = row(nh=70, nw=93, top=3, left=-1)
    assert L.ivit_resize_crop_workspace(sq.ctypes.data_as(C.c_void_p), 1, 64, plan, C.byref(nb)) == -2
    assert L.ivit_resize_crop_workspace(row(nh=60, nw=93, top=-2, left=0).ctypes.data_as(C.c_void_p), 1, 64, plan, C.byref(nb)) == -2
    assert L.ivit_eval_geometry_hw(90, 120, 60, 0, 64, 64, 0, (C.c_int32 * 4)()) == -2
    with pytest.raises(ValueError):
        eval_geometry_hw(90, 120, 60, 64)
    with pytest.raises(ValueError, match="torchvision would pad"):
        EvalTransform(60, (64, 96))
    # a table on the device that disagrees with the plan (a larger source, more taps, more rows): every index is clamped
    big = pack_images([rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)])
    gb = torch.from_numpy(big.geometry((66, 100), (ch, cw))).to(DEV)
    assert workspace() == 0
    wsf = torch.full((nb.value + TAIL,), WS_FILL, dtype=torch.uint8, device=DEV)
    outf = torch.full((3 * ch * cw + TAIL,), A5, dtype=torch.uint8, device=DEV)
    assert run(src_=p(big.data.to(DEV)), g_=p(gb), ws_=p(wsf), out_=p(outf)) == 0
    torch.cuda.synchronize()
    assert bool((wsf[nb.value:] == WS_FILL).all()) and bool((outf[3 * ch * cw:] == A5).all())


# ---------------------------------------------------------------------------------------------------- end to end
def _eval_images(n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(120, 160), (160, 120), (75, 200), (200, 60), (90, 90), (64, 96), (150, 110), (57, 113)]
    return [R.smooth_image(rng, *sizes[i % len(sizes)], noise=12.0) for i in range(n)]


def _calibrate_and_freeze(model, t, seed):
    """synthetic weights, ranges from two batches of transformed images (the reference's post-training calibration), frozen"""
    crops = torch.from_numpy(np.stack([E.resize_crop_hw(im, t.resize, t.crop) for im in _eval_images(6, seed)])).to(DEV)
    with torch.no_grad():
        for prm in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if prm.dim() > 1:
                prm.mul_(3.0)
        x = t.to_float(crops)
        model(x)
        model(x.flip(0) * 0.7)
    ivit.freeze_model(model)
    return model


def _deit_rect():
    torch.manual_seed(6496)
    model = ivit.VisionTransformer(img_size=(64, 96), patch_size=16, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                   num_classes=40).to(DEV).eval()
    return _calibrate_and_freeze(model, EvalTransform.for_model(model), 51)


def _swin_rect():
    torch.manual_seed(56112)
    model = ivit.SwinTransformer(img_size=(56, 112), patch_size=4, window_size=7, embed_dim=64, depths=(2, 2), num_heads=(2, 4),
                                 num_classes=10).to(DEV).eval()
    return _calibrate_and_freeze(model, EvalTransform.for_model(model), 52)


@pytest.mark.parametrize("build,size,resize", [(_deit_rect, (64, 96), 109), (_swin_rect, (56, 112), 128)], ids=["deit_64x96", "swin_56x112"])
def test_evaluate_dataset_on_a_non_square_model(build, size, resize):
    model = build()
    t = EvalTransform.for_model(model)
    assert (t.resize, t.crop, t.pad) == (resize, size, False)
    assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
    images = _eval_images(8, 77)
    crops = torch.from_numpy(np.stack([E.resize_crop_hw(im, t.resize, t.crop) for im in images])).to(DEV)     # the helper's
    xf = t.to_float(crops)
    with torch.no_grad():
        assert model.takes_engine(xf)
        want = model(xf).clone()
    assert len(torch.unique(want.argmax(dim=1))) > 1
    # model(x) on the device's crops (the engine on the uint8 pixels) and on to_float of them: the same bits
    packed = pack_images(images)
    u8 = t(packed, device=DEV)
    assert u8.shape == (8, 3, *size) and torch.equal(u8, crops)
    with torch.no_grad():
        assert torch.equal(inference._forward_transformed(model, t, packed, 0, 8, DEV), want)
        assert torch.equal(model(t.to_float(u8)), want)
    # three batches, targets drawn from the helper's logits so that top-1 < top-3 < top-5 < 100 %
    top = np.argsort(-want.float().cpu().numpy(), axis=1, kind="stable")
    pick = np.array([0, 1, 3, 6, 0, 4, 2, 6])
    classes = want.shape[1]
    tgt = torch.from_numpy(np.where(pick < 5, top[np.arange(8), np.minimum(pick, 4)], top[:, classes - 1]))
    cuts = [(0, 3), (3, 6), (6, 8)]
    loader = [ImageFolderU8.collate([(images[i], int(tgt[i])) for i in range(a, b)]) for a, b in cuts]
    float_loader = [(xf[a:b].cpu(), tgt[a:b]) for a, b in cuts]
    counts = inference.evaluate_dataset(model, float_loader, DEV, print_batch_stats=False)
    print("top-1 / 3 / 5 from the helper's crops:", counts)
    assert 0 < counts[2] and counts[0] < 100 and counts[0] <= counts[1] <= counts[2]
    runs = {"engine": inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t),
            "engine, graph": inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t, graph=True),
            "parallel": inference.evaluate_dataset_parallel(model, loader, DEV, print_batch_stats=False, transform=t)}
    model.use_engine = False
    try:
        with torch.no_grad():
            assert torch.equal(model(t.to_float(u8)), want), "the module path on the device's crops"
        runs["module path"] = inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t)
        runs["module path, graph"] = inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t, graph=True)
    finally:
        model.use_engine = True
        model.drop_graphs()
    assert all(v == counts for v in runs.values()), (counts, runs)


def test_evaluate_dataset_from_compressed_files():
    """ImageFolderJPEG.collate -> EncodedImages -> the device decoder -> the h x w transform -> the engine"""
    model = _deit_rect()
    t = EvalTransform.for_model(model)
    cases = _small_jpegs()[:9]
    crops = torch.from_numpy(np.stack([E.resize_crop_hw(c["pixels"], t.resize, t.crop) for c in cases])).to(DEV)
    with torch.no_grad():
        want = model(t.to_float(crops)).clone()
    tgt = want.argmax(dim=1).cpu()
    tgt[::2] = (tgt[::2] + 1) % want.shape[1]
    cuts = [(0, 4), (4, 5), (5, 9)]
    loader = [ImageFolderJPEG.collate([(cases[i]["data"], int(tgt[i])) for i in range(a, b)]) for a, b in cuts]
    float_loader = [(t.to_float(crops[a:b]).cpu(), tgt[a:b]) for a, b in cuts]
    counts = inference.evaluate_dataset(model, float_loader, DEV, print_batch_stats=False)
    assert 0 < counts[0] < 100
    assert inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t) == counts
    model.use_engine = False
    try:
        assert inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False, transform=t) == counts
    finally:
        model.use_engine = True
