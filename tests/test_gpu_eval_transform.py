"""GPU: the evaluation transform (ivit_resize_crop_bicubic_u8) against the numpy restatement of Pillow's bicubic resize + center crop
(tests/pil_resample_ref.py) and Pillow's own bytes (tests/golden/eval_transform_pil.npz); argument errors; the engines on the crops;
the evaluation harness with transform=.  No Pillow needed."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference, synth  # noqa: E402
from ivit_amd.checkpoint import load_fixture, load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.swin_engine import IntSwinEngine  # noqa: E402
from ivit_amd.transforms import EvalTransform, pack_images  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resample_ref as R  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_transform_pil.npz")


def _reference(images, s, c):
    return np.stack([R.resize_crop(im, s, c) for im in images])


def test_kernel_equals_restatement_on_a_mixed_batch():
    rng = np.random.default_rng(11)
    sizes = [(1, 1), (50, 2000), (2000, 50), (3000, 4000), (256, 256), (256, 300), (300, 256), (375, 500), (500, 375),
             (333, 500), (120, 160), (37, 41), (224, 224), (257, 1024)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if i % 2 else R.smooth_image(rng, h, w) for i, (h, w) in enumerate(sizes)]
    packed = pack_images(images)
    for n in (224, 384):
        t = EvalTransform.for_input_size(n)
        got = t(packed, device=DEV).cpu().numpy()
        want = _reference(images, t.resize, t.crop)
        for i in range(len(images)):
            assert np.array_equal(got[i], want[i]), (n, sizes[i])
    # a shard [lo, hi) of the packed batch, and an odd crop size / resize pair
    t = EvalTransform(300, 257)
    got = t(packed, 3, 9, device=DEV).cpu().numpy()
    assert np.array_equal(got, _reference(images[3:9], 300, 257))


def test_kernel_equals_pillow_fixture():
    z = np.load(GOLDEN)
    images = R.fixture_images()
    for i, img in enumerate(images):
        assert hashlib.sha256(img.tobytes()).digest() == z[f"sha256_{i}"].tobytes(), "fixture sources regenerated differently"
    packed = pack_images(images)
    for n in (224, 384):
        got = EvalTransform.for_input_size(n)(packed, device=DEV).cpu().numpy()
        keys = [i for i in range(len(images)) if f"crop{n}_{i}" in z.files]
        assert keys
        for i in keys:
            assert np.array_equal(got[i], z[f"crop{n}_{i}"]), (n, i)


def test_argument_errors():
    L = _lib.lib()
    rng = np.random.default_rng(3)
    packed = pack_images([rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)])
    geom = packed.geometry(256, 224)
    plan, nb = (C.c_int32 * 3)(), C.c_int64()
    assert L.ivit_resize_crop_workspace(geom.ctypes.data_as(C.c_void_p), 1, 224, plan, C.byref(nb)) == 0
    src = packed.data.to(DEV)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    g = torch.from_numpy(geom).to(DEV)
    ws = torch.empty(nb.value + 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1, 3, 224, 224, dtype=torch.uint8, device=DEV)
    p = _lib.ptr

    def run(src_=src, offs_=p(offs), g_=p(g), batch=1, crop=224, plan_=tuple(plan), ws_=p(ws), nbytes=nb.value):
        return L.ivit_resize_crop_bicubic_u8(p(src_) if isinstance(src_, torch.Tensor) else src_, offs_, g_, batch, crop, *plan_, ws_,
                                             nbytes, p(out), _lib.stream_ptr())

    assert run() == 0
    torch.cuda.synchronize()
    assert out.sum() > 0
    assert run(src_=None) == -1
    assert run(g_=None) == -1
    assert run(ws_=C.c_void_p(ws.data_ptr() + 4)) == -1 and "misaligned" in L.ivit_last_error_string().decode()
    assert run(offs_=C.c_void_p(offs.data_ptr() + 4)) == -1
    assert run(nbytes=nb.value - 1) == -1
    assert run(plan_=(0, plan[1], plan[2])) == -1
    assert run(batch=-1) == -1
    assert run(crop=32) == -2 and "unsupported geometry" in L.ivit_last_error_string().decode()
    assert run(batch=0) == 0
    bad = geom.copy()
    bad[0, 4] = bad[0, 2] - 223    # the crop leaves the resized image
    assert L.ivit_resize_crop_workspace(bad.ctypes.data_as(C.c_void_p), 1, 224, plan, C.byref(nb)) == -2
    assert "unsupported geometry" in L.ivit_last_error_string().decode()
    with pytest.raises(ValueError):
        EvalTransform.for_input_size(32)
    torch.cuda.synchronize()


def _batch(seed, n):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500), (500, 375), (333, 500), (480, 640), (768, 1024), (200, 150), (256, 256), (90, 1200)]
    return [R.smooth_image(rng, *sizes[i % len(sizes)]) for i in range(n)]


def test_engines_on_transformed_crops_equal_the_float_pipeline():
    images = _batch(21, 5)
    packed = pack_images(images)
    t = EvalTransform()
    u8 = t(packed, device=DEV)
    xf = t.to_float(torch.from_numpy(_reference(images, 256, 224)).to(DEV))
    # to_float is torchvision's ToTensor + Normalize, as they run on the CPU (float32 division, not a reciprocal multiply)
    mean = torch.tensor(t.mean).view(1, 3, 1, 1)
    std = torch.tensor(t.std).view(1, 3, 1, 1)
    assert torch.equal(xf.cpu(), (u8.cpu().float().div(255) - mean) / std)

    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=5)
    li_u = eng.forward(u8)[0].clone()
    li_f = eng.forward(xf)[0].clone()
    assert torch.equal(li_u, li_f) and li_f.abs().max() > 0

    z, meta, ranges = load_fixture("swin_tiny")
    scfg = synth.SWIN_CONFIGS[meta["factory"]]
    sfs = synth.make_swin_float_state(meta["factory"], meta["weight_seed"])
    seng = IntSwinEngine(sfs, ranges, scfg["embed_dim"], scfg["depths"], scfg["num_heads"], scfg["window"], device=DEV, max_batch=5)
    sli_u = seng.forward(u8)[0].clone()
    sli_f = seng.forward(xf)[0].clone()
    assert torch.equal(sli_u, sli_f) and sli_f.abs().max() > 0


def _frozen_deit_tiny():
    import ivit_amd.quantization_utils as q
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    model = ivit.deit_tiny_patch16_224()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV)
    ivit.freeze_model(model)
    return model


def test_evaluate_dataset_parallel_with_transform_equals_float_batches():
    model = _frozen_deit_tiny()
    images = _batch(33, 11)
    t = EvalTransform()
    crops = torch.from_numpy(_reference(images, 256, 224))
    xf = t.to_float(crops.to(DEV)).cpu()
    with torch.no_grad():
        lf = model(xf.to(DEV)).float().cpu().numpy()
    top = np.argsort(-lf, axis=1, kind="stable")
    rng = np.random.default_rng(2)
    pick = rng.integers(0, 7, len(images))
    tgt = torch.from_numpy(np.where(pick < 5, top[np.arange(len(images)), np.minimum(pick, 4)], 999 - top[:, 0]))
    cuts = [(0, 4), (4, 5), (5, 11)]
    packed_loader = [(pack_images(images[a:b]), tgt[a:b]) for a, b in cuts]
    float_loader = [(xf[a:b], tgt[a:b]) for a, b in cuts]
    want = inference.evaluate_dataset_parallel(model, float_loader, DEV, print_batch_stats=False)
    got = inference.evaluate_dataset_parallel(model, packed_loader, DEV, print_batch_stats=False, transform=t)
    assert got == want and want[2] > 0
    assert inference.evaluate_dataset(model, packed_loader, DEV, print_batch_stats=False, transform=t) == want
    # the module path (no fused engine): model(transform.to_float(crops))
    model.use_engine = False
    try:
        assert inference.evaluate_dataset_parallel(model, packed_loader, DEV, print_batch_stats=False, transform=t) == \
            inference.evaluate_dataset_parallel(model, float_loader, DEV, print_batch_stats=False)
    finally:
        model.use_engine = True
    # a transform with another Normalize sets the engine's input table, and the default one restores it
    t2 = EvalTransform(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
    xf2 = t2.to_float(crops.to(DEV)).cpu()
    assert inference.evaluate_dataset_parallel(model, packed_loader, DEV, print_batch_stats=False, transform=t2) == \
        inference.evaluate_dataset_parallel(model, [(xf2[a:b], tgt[a:b]) for a, b in cuts], DEV, print_batch_stats=False)
    assert inference.evaluate_dataset_parallel(model, packed_loader, DEV, print_batch_stats=False, transform=t) == want
