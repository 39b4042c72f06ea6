"""Writes tests/golden/eval_transform_rect_pil.npz: Pillow's Image.resize(BICUBIC), then torchvision's CenterCrop arithmetic (zero
padding and slicing in numpy: tests/eval_rect_ref.py center_crop), of a few small seeded RGB images -- an h x w crop, padding on
one axis and on both (odd differences), exact-size resizes that change the aspect ratio either way, an upscale, a 1 : 16 source.
Run on a machine with Pillow; the fixture is data only, and the tests compare the device transform and the numpy restatement with
it without Pillow.  The sources are not stored: they are regenerated from the seed and pinned by SHA-256.

    python scripts/make_eval_transform_rect_golden.py
"""
import hashlib
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_rect_ref as E  # noqa: E402


def main():
    cases = []
    out = {}
    for i, (img, ((h, w), resize, crop)) in enumerate(zip(E.fixture_images(), E.FIXTURE_CASES)):
        assert img.shape == (h, w, 3)
        nh, nw = E.resized_size(h, w, resize)
        ch, cw = E._pair(crop)
        full = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
        out[f"sha256_{i}"] = np.frombuffer(hashlib.sha256(img.tobytes()).digest(), np.uint8)
        out[f"crop_{i}"] = np.ascontiguousarray(E.center_crop(full, ch, cw).transpose(2, 0, 1))
        rh, rw = (resize, 0) if isinstance(resize, int) else resize          # rw = 0: the short-side rule
        cases.append((h, w, rh, rw, ch, cw))
    out["cases"] = np.array(cases, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "eval_transform_rect_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
