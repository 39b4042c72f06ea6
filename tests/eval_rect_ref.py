"""numpy restatement of the evaluation transform with an h x w crop, an exact-size resize and torchvision's zero padding (helper
module of the eval-transform tests, not collected).

torchvision `Resize(s or (h, w), BICUBIC)` on a PIL image, then `CenterCrop((ch, cw))`.  torchvision is not a dependency of the
tests, so its arithmetic is restated twice here, in two forms that the CPU test holds against each other and against Pillow:
  center_crop            torchvision.transforms.functional.center_crop as it is written: pad the image, then slice it
  eval_geometry_hw       the library's form of the same rule: one signed offset per axis, output pixel y = resized pixel y + offset
  resize_crop_hw         the crop computed the way the device computes it: taps only for the pixels inside the resized image
The resample itself is pil_resample_ref's (coeffs / _pass)."""
import numpy as np

import pil_resample_ref as R


def _pair(v):
    try:
        a, b = v
    except TypeError:
        return int(v), int(v)
    return int(a), int(b)


def resized_size(h, w, resize):
    """torchvision Resize: an int s -> short side s, long side int(s * long / short); a pair -> exactly that size"""
    try:
        rh, rw = resize
        return int(rh), int(rw)
    except TypeError:
        s = int(resize)
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(s * long / short)
    return (new_long, s) if w <= h else (s, new_long)


def crop_offset(n, c):
    """one axis of CenterCrop: offset of the crop in a resized axis of n pixels; negative = minus the zeros padded in front"""
    if c <= n:
        return int(round((n - c) / 2.0))          # Python's round: half to even
    return -((c - n) // 2)                        # (c - n) // 2 zeros in front, (c - n + 1) // 2 behind


def eval_geometry_hw(h, w, resize, crop, pad=False):
    """(new_h, new_w, top, left); ValueError where the library says "unsupported geometry" """
    ch, cw = _pair(crop)
    if h < 1 or w < 1 or min(_pair(resize)) < 1 or ch <= 32 or cw <= 32:
        raise ValueError("unsupported geometry")
    new_h, new_w = resized_size(h, w, resize)
    if not pad and (ch > new_h or cw > new_w):
        raise ValueError("unsupported geometry")
    return new_h, new_w, crop_offset(new_h, ch), crop_offset(new_w, cw)


def center_crop(img, ch, cw):
    """torchvision.transforms.functional.center_crop on an H x W x C array, statement for statement"""
    h, w = img.shape[:2]
    if cw > w or ch > h:
        left = (cw - w) // 2 if cw > w else 0
        top = (ch - h) // 2 if ch > h else 0
        right = (cw - w + 1) // 2 if cw > w else 0
        bottom = (ch - h + 1) // 2 if ch > h else 0
        img = np.pad(img, ((top, bottom), (left, right), (0, 0)))          # fill 0
        h, w = img.shape[:2]
        if cw == w and ch == h:
            return img
    top = int(round((h - ch) / 2.0))
    left = int(round((w - cw) / 2.0))
    return img[top:top + ch, left:left + cw]


def _inside(n, c, off):
    """crop indices [lo, hi) that lie inside the resized axis"""
    return max(0, -off), min(c, n - off)


def resize_crop_hw(img, resize, crop, pad=False):
    """uint8 HxWx3 -> uint8 [3, ch, cw]: Resize(resize, BICUBIC) + CenterCrop(crop); zeros outside the resized image, taps only inside"""
    h, w = img.shape[:2]
    ch, cw = _pair(crop)
    new_h, new_w, top, left = eval_geometry_hw(h, w, resize, crop, pad)
    x0, x1 = _inside(new_w, cw, left)
    y0, y1 = _inside(new_h, ch, top)
    cx = R.coeffs(w, new_w)[left + x0:left + x1]
    cy = R.coeffs(h, new_h)[top + y0:top + y1]
    r0 = cy[0][0]
    r1 = cy[-1][0] + len(cy[-1][1])
    mid = R._pass(img[r0:r1].astype(np.int64), cx, 1)
    part = R._pass(mid, [(ymin - r0, kk) for ymin, kk in cy], 0).astype(np.uint8)
    out = np.zeros((ch, cw, 3), np.uint8)
    out[y0:y1, x0:x1] = part
    return np.ascontiguousarray(out.transpose(2, 0, 1))


# the sweep the rule was checked on against Pillow + center_crop: 6 sources x 6 resizes x 5 crops, pad on
SWEEP_SOURCES = [(33, 33), (200, 150), (47, 120), (120, 47), (97, 64), (64, 181)]          # (h, w), 33 to 200 px
SWEEP_RESIZES = [37, 48, 73, (40, 56), (65, 34), (96, 64)]
CROPS = [(33, 33), (34, 65), (65, 37), (40, 56), (64, 96)]

# tests/golden/eval_transform_rect_pil.npz (scripts/make_eval_transform_rect_golden.py): Pillow's resize, then center_crop, of
# these sources -- regenerated here from the seed and checked against the stored SHA-256.  ((h, w), resize, crop): all with pad
FIXTURE_SEED = 20261020
FIXTURE_CASES = [
    ((120, 160), 109, (64, 96)),          # h x w crop, no padding (for_input_size((64, 96)))
    ((150, 60), 64, (64, 96)),            # portrait into a landscape crop: 32 zero columns, none on the other axis
    ((100, 80), (41, 51), (64, 96)),      # padding on both axes, odd differences 23 and 45: 11 + 12 rows, 22 + 23 columns
    ((90, 120), (96, 64), (65, 37)),      # exact size, landscape made portrait
    ((120, 90), (40, 100), (40, 56)),     # exact size, portrait made landscape
    ((33, 45), 73, (65, 37)),             # an upscale (33 -> 73), odd margins
    ((70, 50), (64, 64), 64),             # Resize((n, n)) with no crop left to take: how Swin's 384 px checkpoints are fed
    ((37, 600), 48, (34, 65)),            # 1 : 16, 33 taps per column; the crop's 65 columns are a second, one-column tile
]


def fixture_images():
    rng = np.random.default_rng(FIXTURE_SEED)
    return [R.smooth_image(rng, h, w, noise=2.0, fmax=3.0) for (h, w), _, _ in FIXTURE_CASES]
