"""CPU: the evaluation transform's contract -- the numpy restatement of Pillow's bicubic resize + center crop against Pillow itself
and the stored fixture, the geometry rule of the C ABI (a host function) against torchvision's, the C ABI declarations, the packed
batch layout, ImageFolderU8's indexing, and evaluate_dataset_parallel's default path."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resample_ref as R  # noqa: E402

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference  # noqa: E402
from ivit_amd.transforms import EvalTransform, ImageFolderU8, eval_geometry, pack_images  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_transform_pil.npz")


def _pairs():
    """(h, w, s, c) cases: 1 x 1, extreme aspect ratios, an unchanged short side, input size 384, odd crop margins, random"""
    cases = [(1, 1, 256, 224), (2, 3, 256, 224), (90, 1200, 256, 224), (1200, 90, 256, 224), (4000, 3000, 256, 224),
             (3000, 4000, 438, 384), (256, 341, 256, 224), (341, 256, 256, 224), (256, 256, 256, 224), (375, 500, 438, 384),
             (500, 375, 256, 224), (333, 500, 256, 224), (1, 700, 256, 224), (700, 1, 256, 33), (224, 224, 256, 224)]
    rng = np.random.default_rng(5)
    while len(cases) < 210:
        h, w = (int(v) for v in rng.integers(1, 900, 2))
        n = int(rng.choice([33, 64, 160, 224, 256, 384]))
        s, c = R.input_size_rule(n)
        if rng.random() < 0.3:
            s = int(rng.integers(c, c + 60))
        cases.append((h, w, s, c))
    return cases


def _torchvision_geometry(h, w, s, c):
    """torchvision's Resize([s]) output size and CenterCrop's offsets, spelled as its functional code does"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = s, int(s * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w, int(round((new_h - c) / 2.0)), int(round((new_w - c) / 2.0))


def test_restatement_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for k, (h, w, s, c) in enumerate(_pairs()):
        if h * w > 1_000_000 and k % 2:
            continue
        img = R.smooth_image(rng, h, w) if k % 3 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw, top, left = R.eval_geometry(h, w, s, c)
        full = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
        want = full[top:top + c, left:left + c].transpose(2, 0, 1)
        assert np.array_equal(R.resize_crop(img, s, c), want), (h, w, s, c)
    # whole resizes, one or both axes unchanged (Pillow skips that pass; the identity taps give the same bytes), upscales
    for (h, w), (nh, nw) in [((1, 1), (5, 7)), ((2, 3), (5, 7)), ((40, 60), (40, 90)), ((40, 60), (25, 60)), ((33, 33), (33, 33)),
                             ((1200, 90), (300, 40)), ((17, 300), (256, 17))]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(R.resize_full(img, nh, nw), np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC)))


def test_restatement_equals_fixture():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 1 << 20
    n = 0
    for i, img in enumerate(R.fixture_images()):
        assert hashlib.sha256(img.tobytes()).digest() == z[f"sha256_{i}"].tobytes()
        for size in (224, 384):
            key = f"crop{size}_{i}"
            if key in z.files:
                s, c = R.input_size_rule(size)
                assert np.array_equal(R.resize_crop(img, s, c), z[key]), key
                n += 1
    assert n >= 8


def test_geometry_rule_of_the_library_equals_torchvision():
    for h, w, s, c in _pairs():
        want = _torchvision_geometry(h, w, s, c)
        assert eval_geometry(h, w, s, c) == want == R.eval_geometry(h, w, s, c), (h, w, s, c)
    # round half to even: margins 117 -> 58, 119 -> 60 (floor((d + 1) / 2) would give 59 and 60)
    assert eval_geometry(375, 500, 256, 224)[3] == 58                # new width 341
    assert eval_geometry(256, 343, 256, 224)[3] == 60                # new width 343
    assert R.input_size_rule(384) == (438, 384) and R.input_size_rule(224) == (256, 224)
    t = EvalTransform.for_input_size(384)
    assert (t.resize, t.crop) == (438, 384)
    L = _lib.lib()
    out = (C.c_int32 * 4)()
    assert L.ivit_eval_geometry(100, 100, 256, 32, out) == -2 and "unsupported geometry" in L.ivit_last_error_string().decode()
    assert L.ivit_eval_geometry(0, 100, 256, 224, out) == -2
    assert L.ivit_eval_geometry(100, 100, 200, 224, out) == -2     # crop > short side: torchvision would pad
    assert L.ivit_eval_geometry(100, 100, 256, 224, None) == -1
    with pytest.raises(ValueError):
        EvalTransform.for_input_size(32)
    with pytest.raises(ValueError):
        eval_geometry(5, 5, 200, 224)


def test_header_prototypes_match_signatures():
    text = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    kinds = {"int": C.c_int, "int64_t": C.c_int64}
    for name in ("ivit_eval_geometry", "ivit_resize_crop_workspace", "ivit_resize_crop_bicubic_u8"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [C.c_void_p if "*" in p or p.startswith("ivit_stream_t") else kinds[p.rsplit(" ", 1)[0]] for p in params]
        assert _lib.SIGNATURES[name] == want, name


def test_pack_images_layout():
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(5, 7), (1, 1), (300, 200)]]
    p = pack_images(imgs, pin=False)
    assert len(p) == 3 and p.size(0) == 3
    assert p.offsets.tolist() == [0, 105, 108] and p.sizes.tolist() == [[5, 7], [1, 1], [300, 200]]
    assert p.data.dtype == torch.uint8 and p.data.numel() == 108 + 300 * 200 * 3
    for b, im in enumerate(imgs):
        assert np.array_equal(p.data.numpy()[p.offsets[b]:p.offsets[b] + im.size].reshape(im.shape), im)
    g = p.geometry(256, 224)
    assert g.dtype == np.int32 and g.shape == (3, 6)
    assert g[2].tolist() == [300, 200, *_torchvision_geometry(300, 200, 256, 224)]
    with pytest.raises(ValueError):
        pack_images([np.zeros((4, 4), np.uint8)], pin=False)


def test_to_float_is_totensor_normalize():
    rng = np.random.default_rng(4)
    u8 = torch.from_numpy(rng.integers(0, 256, (2, 3, 40, 40), dtype=np.uint8))
    u8[0, :, 0, :] = torch.arange(40, dtype=torch.uint8) + 216
    for t in (EvalTransform(), EvalTransform(mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.3))):
        mean = torch.tensor(t.mean).view(1, 3, 1, 1)
        std = torch.tensor(t.std).view(1, 3, 1, 1)
        want = (u8.float().div(255) - mean) / std             # torchvision ToTensor + Normalize on a CPU tensor
        assert torch.equal(t.to_float(u8), want)


def test_image_folder_u8(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2)
    (tmp_path / "zebra" / "sub").mkdir(parents=True)
    (tmp_path / "ant").mkdir()
    (tmp_path / "notes.txt").write_text("not a class")
    rgb = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, (4, 5), dtype=np.uint8)
    rgba = rng.integers(0, 256, (3, 2, 4), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "zebra" / "b.png")
    Image.fromarray(gray, "L").save(tmp_path / "zebra" / "sub" / "a.PNG")
    Image.fromarray(rgba, "RGBA").save(tmp_path / "ant" / "x.png")
    (tmp_path / "ant" / "readme.md").write_text("skipped")
    ds = ImageFolderU8(tmp_path)
    assert ds.classes == ["ant", "zebra"] and ds.class_to_idx == {"ant": 0, "zebra": 1}
    assert [os.path.relpath(p, tmp_path) for p, _ in ds.samples] == ["ant/x.png", "zebra/b.png", "zebra/sub/a.PNG"]
    assert ds.targets == [0, 1, 1] and len(ds) == 3
    x, t = ds[0]
    assert t == 0 and np.array_equal(x, np.asarray(Image.fromarray(rgba, "RGBA").convert("RGB")))
    x, t = ds[1]
    assert t == 1 and np.array_equal(x, rgb)
    x, t = ds[2]
    assert x.shape == (4, 5, 3) and np.array_equal(x, np.repeat(gray[:, :, None], 3, axis=2))
    packed, targets = ImageFolderU8.collate([ds[i] for i in range(3)], pin=False)
    assert targets.tolist() == [0, 1, 1] and packed.sizes.tolist() == [[3, 2], [6, 9], [4, 5]]


class _Stub(torch.nn.Module):
    def forward(self, x):
        v = x.reshape(x.shape[0], -1)[:, :1]
        return (v * torch.arange(10.0) % 7)


def _scorer(logits, targets, hits, k=5):
    tk = torch.sort(logits, dim=1, descending=True, stable=True).indices[:, :k]
    hits += (tk == targets.reshape(-1, 1).long()).sum(dim=0)


def test_transform_none_keeps_evaluate_dataset_parallel():
    g = torch.Generator().manual_seed(3)
    loader = [(torch.randint(0, 9, (b, 3, 2, 2), generator=g).float(), torch.randint(0, 10, (b,), generator=g)) for b in (4, 1, 6)]
    a = inference.evaluate_dataset_parallel(_Stub(), loader, "cpu", scorer=_scorer, print_batch_stats=False)
    b = inference.evaluate_dataset_parallel(_Stub(), loader, "cpu", scorer=_scorer, print_batch_stats=False, transform=None)
    assert a == b and a[2] > 0
    assert inference.evaluate_dataset(_Stub(), loader, "cpu", print_batch_stats=False, transform=None) == \
        inference.evaluate_dataset(_Stub(), loader, "cpu", print_batch_stats=False)
