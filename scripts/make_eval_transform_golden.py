"""Writes tests/golden/eval_transform_pil.npz: Pillow's Resize(BICUBIC) + CenterCrop of a few seeded, smooth RGB images of mixed
sizes (an upscale, a 1:13 aspect ratio, odd crop margins), at input size 224 (Resize 256) and, for two of them, 384 (Resize 438).
Run on a machine with Pillow; the fixture is data only, and the GPU tests compare the device transform with it without Pillow.

    python scripts/make_eval_transform_golden.py
"""
import hashlib
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pil_resample_ref as R  # noqa: E402


def main():
    out = {"sizes": np.array(R.FIXTURE_SIZES, np.int32)}
    for i, img in enumerate(R.fixture_images()):
        h, w = img.shape[:2]
        out[f"sha256_{i}"] = np.frombuffer(hashlib.sha256(img.tobytes()).digest(), np.uint8)
        for n in ((224, 384) if i in R.FIXTURE_WITH_384 else (224,)):
            s, c = R.input_size_rule(n)
            nh, nw, top, left = R.eval_geometry(h, w, s, c)
            full = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BICUBIC))
            out[f"crop{n}_{i}"] = np.ascontiguousarray(full[top:top + c, left:left + c].transpose(2, 0, 1))
    path = os.path.join(ROOT, "tests", "golden", "eval_transform_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
