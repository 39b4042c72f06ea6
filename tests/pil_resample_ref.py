"""numpy restatement of the reference's evaluation resize + crop (helper module of the eval-transform tests, not collected).

torchvision `Resize([s], BICUBIC)` on a PIL image, then `CenterCrop(c)`: the geometry rule of eval_geometry and Pillow's 8-bit
bicubic resample (separable, horizontal pass first, uint8 between the passes, 22-bit fixed-point coefficients), evaluated in
float64 in Pillow's operation order.  Plain Python loops where the order of a float64 sum matters."""
import math

import numpy as np

PRECISION_BITS = 22


def eval_geometry(h, w, s, c):
    """(new_h, new_w, top, left) of Resize([s]) then CenterCrop(c); ValueError where the device entry says "unsupported geometry"."""
    if h < 1 or w < 1 or s < 1 or c <= 32:
        raise ValueError("unsupported geometry")
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(s * long / short)
    new_h, new_w = (new_long, s) if w <= h else (s, new_long)
    if c > min(new_h, new_w):
        raise ValueError("unsupported geometry")
    return new_h, new_w, int(round((new_h - c) / 2.0)), int(round((new_w - c) / 2.0))


def input_size_rule(n):
    """data_utils.build_transform: (resize short side, crop) for input size n > 32"""
    if n <= 32:
        raise ValueError("input size <= 32 (no resize) is out of scope")
    return int((256 / 224) * n), n


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(n_in, n_out):
    """per output index o: (xmin, int64 kk[xmax]) of one axis"""
    scale = filterscale = n_in / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    out = []
    for o in range(n_out):
        center = (o + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((i + xmin - center + 0.5) * ss) for i in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = [v / ww for v in w] if ww != 0.0 else w
        kk = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in k]
        out.append((xmin, np.array(kk, np.int64)))
    return out


def _pass(src, taps, axis):
    """one resample pass over `axis` (0 = rows, 1 = columns) of an int64 [rows, cols, 3] image -> uint8 values"""
    rows = []
    for xmin, kk in taps:
        sl = np.take(src, np.arange(xmin, xmin + len(kk)), axis=axis)
        shape = [1, 1, 1]
        shape[axis] = len(kk)
        acc = (1 << (PRECISION_BITS - 1)) + (sl * kk.reshape(shape)).sum(axis=axis)
        rows.append(np.clip(acc >> PRECISION_BITS, 0, 255))
    return np.stack(rows, axis=axis)


def resize_crop(img, s, c):
    """uint8 HxWx3 -> uint8 [3, c, c]: Resize([s], BICUBIC) + CenterCrop(c), only the crop's pixels computed"""
    h, w = img.shape[:2]
    new_h, new_w, top, left = eval_geometry(h, w, s, c)
    cx = coeffs(w, new_w)[left:left + c]
    cy = coeffs(h, new_h)[top:top + c]
    r0 = cy[0][0]
    r1 = cy[-1][0] + len(cy[-1][1])
    mid = _pass(img[r0:r1].astype(np.int64), cx, 1)                 # horizontal: [rows, c, 3], uint8 range
    out = _pass(mid, [(y0 - r0, kk) for y0, kk in cy], 0)            # vertical on the clipped intermediate
    return np.ascontiguousarray(out.astype(np.uint8).transpose(2, 0, 1))


def resize_full(img, new_h, new_w):
    """the whole Pillow resize (no crop): for the comparison with Image.resize"""
    mid = _pass(img.astype(np.int64), coeffs(img.shape[1], new_w), 1)
    return _pass(mid, coeffs(img.shape[0], new_h), 0).astype(np.uint8)


def smooth_image(rng, h, w, noise=6.0, fmax=6.0):
    """a mostly smooth RGB test image (gradients + low-frequency waves + a little noise), uint8 HxWx3"""
    y = np.linspace(0, 1, h).reshape(-1, 1, 1)
    x = np.linspace(0, 1, w).reshape(1, -1, 1)
    ph = rng.uniform(0, 2 * math.pi, size=(1, 1, 3))
    f = rng.uniform(1, fmax, size=(2, 3))
    v = 127.5 + 90 * np.sin(2 * math.pi * (f[0] * x + f[1] * y) + ph) + 30 * (x - y)
    v = v + rng.normal(0, noise, size=(h, w, 3))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# tests/golden/eval_transform_pil.npz (scripts/make_eval_transform_golden.py): Pillow's crops of these sources, which the fixture
# does not store -- they are regenerated here (numpy's PCG64 uniform stream) and checked against the stored SHA-256
FIXTURE_SEED = 20261015
FIXTURE_SIZES = [(375, 500), (500, 375), (333, 500), (160, 120), (90, 1200), (451, 600)]   # (h, w): upscale, 1:13, odd margins
FIXTURE_WITH_384 = (1, 3)     # the 384 crops (442 KB each) of two images only: the fixture stays under 1 MB


def fixture_images():
    rng = np.random.default_rng(FIXTURE_SEED)
    return [smooth_image(rng, h, w, noise=0.0, fmax=2.0) for h, w in FIXTURE_SIZES]
