"""CPU: the evaluation transform with an h x w crop, an exact-size resize and zero padding -- the library's geometry rule
(ivit_eval_geometry_hw, a host function) against the numpy restatement (tests/eval_rect_ref.py), the restatement against Pillow +
torchvision's center_crop arithmetic and against the stored fixture, EvalTransform's constructors, the geometry cache, the C ABI
declarations."""
import ctypes as C
import hashlib
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_rect_ref as E  # noqa: E402
import pil_resample_ref as R  # noqa: E402

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.transforms import EvalTransform, eval_geometry, eval_geometry_hw, pack_images  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_transform_rect_pil.npz")
NEW_ENTRIES = ("ivit_eval_geometry_hw", "ivit_resize_crop_workspace_hw", "ivit_resize_crop_bicubic_hw_u8")


def _library(h, w, resize, crop, pad):
    """ivit_eval_geometry_hw -> (rc, out4)"""
    rh, rw = (resize, 0) if isinstance(resize, int) else resize
    ch, cw = E._pair(crop)
    out = (C.c_int32 * 4)()
    rc = _lib.lib().ivit_eval_geometry_hw(h, w, rh, rw, ch, cw, int(pad), out)
    return rc, tuple(out)


def _geometry_cases():
    """(h, w, resize, crop): the sweep of the Pillow test; square resized images with margins 1, 3, 5, 7 (half to even: 0, 2, 2,
    4) and padding differences 1, 3, 5, 7 on either axis; crop sides 32 and 33; extreme aspect ratios; random ones"""
    cases = [(h, w, r, c) for (h, w), r, c in itertools.product(E.SWEEP_SOURCES, E.SWEEP_RESIZES, E.CROPS)]
    for d in (1, 3, 5, 7):
        cases += [(80, 80, 64 + d, 64), (80, 80, (64 + d, 70), (64, 64 + d)), (80, 80, 64 - d, 64), (80, 80, (64 - d, 64), (64, 64 + d)),
                  (100, 50, 40 + d, (40, 96)), (50, 100, 40 + d, (96, 40))]
    cases += [(50, 50, 40, (32, 40)), (50, 50, 40, (40, 32)), (50, 50, 40, 32), (50, 50, 40, 33), (50, 50, 33, (33, 40)),
              (1, 1, 40, (40, 56)), (1, 700, 37, (33, 65)), (700, 1, 37, (33, 65)), (3000, 4000, 256, (224, 320)),
              (0, 50, 40, 40), (50, 50, 0, 40), (50, 50, (40, -1), 40), (50, 50, (0, 40), 40)]
    rng = np.random.default_rng(17)
    for _ in range(150):
        h, w = (int(v) for v in rng.integers(1, 500, 2))
        r = int(rng.integers(20, 300)) if rng.random() < 0.5 else tuple(int(v) for v in rng.integers(20, 300, 2))
        c = int(rng.integers(33, 300)) if rng.random() < 0.3 else tuple(int(v) for v in rng.integers(33, 300, 2))
        cases.append((h, w, r, c))
    return cases


def test_geometry_rule_of_the_library_equals_the_restatement():
    L = _lib.lib()
    seen = {"ok": 0, "refused": 0, "padded": 0, "odd_pad": 0}
    for h, w, r, c in _geometry_cases():
        for pad in (False, True):
            try:
                want = E.eval_geometry_hw(h, w, r, c, pad)
            except ValueError:
                want = None
            rc, got = _library(h, w, r, c, pad)
            if want is None:
                assert rc == -2 and "unsupported geometry" in L.ivit_last_error_string().decode(), (h, w, r, c, pad)
                with pytest.raises(ValueError):
                    eval_geometry_hw(h, w, r, c, pad)
                seen["refused"] += 1
                continue
            assert rc == 0 and got == want == eval_geometry_hw(h, w, r, c, pad), (h, w, r, c, pad, got, want)
            seen["ok"] += 1
            ch, cw = E._pair(c)
            seen["padded"] += want[2] < 0 or want[3] < 0
            seen["odd_pad"] += (want[2] < 0 and (ch - want[0]) % 2) or (want[3] < 0 and (cw - want[1]) % 2)
            # the signed offset is torchvision's pad-then-slice: the same window of a labelled image
            lab = np.arange(1, want[0] * want[1] + 1, dtype=np.int64).reshape(want[0], want[1], 1) if want[0] * want[1] <= 40000 else None
            if lab is not None:
                out = np.zeros((ch, cw, 1), np.int64)
                y0, y1 = E._inside(want[0], ch, want[2])
                x0, x1 = E._inside(want[1], cw, want[3])
                out[y0:y1, x0:x1] = lab[want[2] + y0:want[2] + y1, want[3] + x0:want[3] + x1]
                assert np.array_equal(out, E.center_crop(lab, ch, cw)), (h, w, r, c)
    assert min(seen.values()) > 10, seen
    # half to even, and the padding split: the smaller half in front
    assert [_library(80, 80, 64 + d, 64, False)[1][2] for d in (1, 3, 5, 7)] == [0, 2, 2, 4]
    assert [_library(80, 80, 64 - d, 64, True)[1][2:] for d in (1, 3, 5, 7)] == [(0, 0), (-1, -1), (-2, -2), (-3, -3)]
    # pad = 0 refuses what pad = 1 takes; crop side 32 is refused either way, 33 is taken
    assert _library(80, 80, 60, 64, False)[0] == -2 and _library(80, 80, 60, 64, True) == (0, (60, 60, -2, -2))
    assert _library(80, 80, (70, 60), (64, 64), False)[0] == -2 and _library(80, 80, (70, 60), (64, 64), True) == (0, (70, 60, 3, -2))
    for pad in (False, True):
        assert _library(50, 50, 40, (32, 40), pad)[0] == -2 and _library(50, 50, 40, (40, 32), pad)[0] == -2
        assert _library(50, 50, 40, (33, 40), pad) == (0, (40, 40, 4, 0))
    assert L.ivit_eval_geometry_hw(50, 50, 40, 0, 40, 40, 0, None) == -1


def test_square_rule_is_the_hw_rule_on_the_diagonal():
    """eval_geometry(h, w, s, c) == eval_geometry_hw(h, w, s, (c, c)) wherever the former does not raise, and it raises exactly where
    it did: where the restatement of the square rule (pil_resample_ref.eval_geometry) raises"""
    rng = np.random.default_rng(23)
    cases = [(1, 1, 256, 224), (90, 1200, 256, 224), (1200, 90, 256, 224), (375, 500, 438, 384), (256, 343, 256, 224), (100, 100, 200, 224),
             (100, 100, 256, 32), (0, 100, 256, 224), (100, 100, 0, 224), (100, 100, 224, 224), (50, 100, 64, 65)]
    for _ in range(200):
        h, w = (int(v) for v in rng.integers(1, 900, 2))
        cases.append((h, w, int(rng.integers(30, 300)), int(rng.integers(30, 300))))
    raised = 0
    for h, w, s, c in cases:
        try:
            want = R.eval_geometry(h, w, s, c)
        except ValueError:
            want = None
        if want is None:
            raised += 1
            with pytest.raises(ValueError):
                eval_geometry(h, w, s, c)
            with pytest.raises(ValueError):
                eval_geometry_hw(h, w, s, (c, c))
        else:
            assert eval_geometry(h, w, s, c) == want == eval_geometry_hw(h, w, s, (c, c)) == eval_geometry_hw(h, w, s, c, pad=True), (h, w, s, c)
    assert 20 < raised < len(cases) - 20


def test_restatement_equals_pillow_and_center_crop():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(29)
    n = 0
    for k, ((h, w), r) in enumerate(itertools.product(E.SWEEP_SOURCES, E.SWEEP_RESIZES)):
        img = R.smooth_image(rng, h, w) if k % 3 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        nh, nw = E.resized_size(h, w, r)
        full = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
        for c in E.CROPS:
            want = E.center_crop(full, *c).transpose(2, 0, 1)
            assert np.array_equal(E.resize_crop_hw(img, r, c, pad=True), want), (h, w, r, c)
            n += 1
    assert n == 180


def test_fixture_sources_and_restatement_equal_the_fixture():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 1 << 20
    images = E.fixture_images()
    assert len(images) == len(E.FIXTURE_CASES) == len(z["cases"])
    kinds = set()
    for i, (img, ((h, w), r, c)) in enumerate(zip(images, E.FIXTURE_CASES)):
        assert hashlib.sha256(img.tobytes()).digest() == z[f"sha256_{i}"].tobytes(), "fixture sources regenerated differently"
        rh, rw = (r, 0) if isinstance(r, int) else r
        assert z["cases"][i].tolist() == [h, w, rh, rw, *E._pair(c)]
        assert np.array_equal(E.resize_crop_hw(img, r, c, pad=True), z[f"crop_{i}"]), i
        nh, nw, top, left = E.eval_geometry_hw(h, w, r, c, True)
        ch, cw = E._pair(c)
        kinds.add(("pad", top < 0, left < 0))
        if top < 0 and left < 0 and (ch - nh) % 2 and (cw - nw) % 2:
            kinds.add("odd both")
        if rw and nh * w > nw * h:
            kinds.add("taller")
        if rw and nh * w < nw * h:
            kinds.add("wider")
        if nh > h and nw > w:
            kinds.add("upscale")
        if ch != cw and top >= 0 and left >= 0:
            kinds.add("h x w")
    assert kinds >= {("pad", False, False), ("pad", False, True), ("pad", True, True), "odd both", "taller", "wider", "upscale", "h x w"}, kinds


def test_constructor():
    # two ints without pad: as before -- ints stay ints, the same ValueErrors
    t = EvalTransform()
    assert (t.resize, t.crop, t.pad, t.crop_hw) == (256, 224, False, (224, 224)) and type(t.resize) is int and type(t.crop) is int
    t = EvalTransform(np.int64(300), np.int32(257))
    assert (t.resize, t.crop) == (300, 257) and type(t.resize) is int and type(t.crop) is int
    with pytest.raises(ValueError, match="<= 32"):
        EvalTransform(256, 32)
    with pytest.raises(ValueError, match="torchvision would pad"):
        EvalTransform(200, 224)
    # pairs
    t = EvalTransform(109, (64, 96))
    assert (t.resize, t.crop, t.crop_hw) == (109, (64, 96), (64, 96))
    t = EvalTransform((384, 384), 384)
    assert (t.resize, t.crop, t.crop_hw) == ((384, 384), 384, (384, 384))
    t = EvalTransform([40, 56], [40, 56])
    assert (t.resize, t.crop) == ((40, 56), (40, 56))
    for kw in (dict(resize=95, crop=(64, 96)), dict(resize=95, crop=(96, 64)), dict(resize=(64, 95), crop=(64, 96)),
               dict(resize=(63, 96), crop=(64, 96)), dict(resize=(40, 300), crop=64)):
        with pytest.raises(ValueError, match="torchvision would pad"):
            EvalTransform(**kw)
        assert EvalTransform(pad=True, **kw).pad
    assert EvalTransform(96, (64, 96)).crop == (64, 96) and EvalTransform((64, 96), (64, 96)).resize == (64, 96)
    assert EvalTransform(200, 224, pad=True).crop == 224
    for crop in ((32, 96), (96, 32), 32):
        with pytest.raises(ValueError, match="<= 32"):
            EvalTransform(300, crop, pad=True)
    with pytest.raises(ValueError):
        EvalTransform((0, 40), 40, pad=True)
    with pytest.raises(ValueError):
        EvalTransform((1, 2, 3), 40)


def test_for_input_size_and_for_model():
    assert (EvalTransform.for_input_size(224).resize, EvalTransform.for_input_size(224).crop) == (256, 224)
    for h, w in [(64, 96), (96, 64), (56, 112), (384, 384), (224, 320), (33, 34)]:
        t = EvalTransform.for_input_size((h, w))
        assert (t.resize, t.crop, t.pad) == (int((256 / 224) * max(h, w)), (h, w), False)
        # no image is padded, whatever its aspect ratio, and at h == w the geometry is the reference's
        for ih, iw in [(1, 1000), (1000, 1), (37, 41), (500, 375)]:
            nh, nw, top, left = eval_geometry_hw(ih, iw, t.resize, t.crop)
            assert top >= 0 and left >= 0 and nh >= h and nw >= w
            if h == w:
                assert (nh, nw, top, left) == eval_geometry(ih, iw, *R.input_size_rule(h))
    for bad in ((32, 96), (96, 32), 32):
        with pytest.raises(ValueError):
            EvalTransform.for_input_size(bad)

    class _Embed:
        def __init__(self, size):
            self.img_size = size

    class _Model:
        def __init__(self, size):
            self.patch_embed = _Embed(size)

    t = EvalTransform.for_model(_Model((64, 96)))
    assert (t.resize, t.crop) == (109, (64, 96))
    t = EvalTransform.for_model(_Model((224, 224)))
    assert (t.resize, t.crop) == (256, 224) and type(t.crop) is int
    with pytest.raises(TypeError):
        EvalTransform.for_model(object())
    vit = ivit.VisionTransformer(img_size=(64, 96), patch_size=16, embed_dim=32, depth=1, num_heads=2, num_classes=4)
    assert EvalTransform.for_model(vit).crop == (64, 96)
    swin = ivit.SwinTransformer(img_size=(56, 112), patch_size=4, window_size=7, embed_dim=16, depths=(1,), num_heads=(2,), num_classes=4)
    assert EvalTransform.for_model(swin).crop == (56, 112) and EvalTransform.for_model(swin).resize == 128


def test_geometry_cache_keys_hold_the_full_tuple():
    rng = np.random.default_rng(1)
    p = pack_images([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(50, 70), (300, 200)]], pin=False)
    a = p.geometry(256, 224)
    assert a[1].tolist() == [300, 200, *eval_geometry(300, 200, 256, 224)] and p.geometry(256, 224) is a
    b = p.geometry(256, (224, 224))
    c = p.geometry(256, 224, True)
    d = p.geometry((256, 256), 224)
    e = p.geometry(60, (64, 96), pad=True)
    assert set(p._geom) == {(256, 224, False), (256, (224, 224), False), (256, 224, True), ((256, 256), 224, False), (60, (64, 96), True)}
    assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a, d)
    assert e.dtype == np.int32 and e.tolist() == [[h, w, *E.eval_geometry_hw(h, w, 60, (64, 96), True)] for h, w in [(50, 70), (300, 200)]]
    assert e[0, 4] < 0 or e[0, 5] < 0
    assert p.geometry(np.int64(60), [64, 96], pad=1) is e
    with pytest.raises(ValueError):
        p.geometry(60, (64, 96))                   # would pad
    with pytest.raises(ValueError):
        p.geometry(200, 224)                       # the square rule's refusal, as before
    from ivit_amd.transforms import EncodedImages
    enc = EncodedImages(None, np.zeros(2, np.int64), np.zeros(2, np.int64), p.offsets, p.sizes)
    assert np.array_equal(enc.geometry(60, (64, 96), True), e) and set(enc._geom) == {(60, (64, 96), True)}


def _prototype_kinds(name):
    """the ctypes kinds of the parameters `name` is declared with in include/ivit_hip.h (the method of test_attention_long_cpu)"""
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const uint8_t*": _lib.vp, "uint8_t*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "const int32_t*": _lib.vp,
             "int32_t*": _lib.vp, "void*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64, "ivit_stream_t": _lib.vp}
    params = [p.strip() for p in m.group(1).split(",")]
    return [kinds[re.sub(r"\s+\w+$", "", p)] for p in params], [p.rsplit(" ", 1)[1] for p in params]


@pytest.mark.parametrize("name", NEW_ENTRIES)
def test_header_prototypes_match_signatures(name):
    kinds, names = _prototype_kinds(name)
    assert _lib.SIGNATURES[name] == kinds
    assert not [n for n in names if re.fullmatch(r"ld.?", n)], "the output is dense: no leading dimensions"
    assert getattr(_lib.lib(), name).argtypes == kinds
