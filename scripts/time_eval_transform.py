"""Time the device evaluation transform (ivit_resize_crop_bicubic_u8: Resize 256 BICUBIC -> CenterCrop 224) on a batch of 256
ImageNet-like sizes, event-timed on cuda:0, next to the single-thread Pillow cost of the same images (Image.resize + crop), when
Pillow is installed.  One JSON line.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python scripts/time_eval_transform.py [--batch 256] [--iters 50] [--pil-images 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ivit_amd  # noqa: E402,F401
from ivit_amd.transforms import EvalTransform, eval_geometry, pack_images  # noqa: E402

SIZES = [(375, 500), (500, 375), (333, 500), (480, 640), (768, 1024), (375, 500), (500, 333), (200, 150), (180, 240), (256, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pil-images", type=int, default=64)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (*SIZES[i % len(SIZES)], 3), dtype=np.uint8) for i in range(a.batch)]
    packed = pack_images(images)
    t = EvalTransform()
    out = torch.empty(a.batch, 3, 224, 224, dtype=torch.uint8, device="cuda:0")
    for _ in range(5):
        t(packed, device="cuda:0", out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        t(packed, device="cuda:0", out=out)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.iters
    res = {"batch": a.batch, "device_ms_per_batch": round(dev_ms, 4), "device_us_per_image": round(dev_ms * 1000 / a.batch, 3),
           "input_mb_per_batch": round(packed.data.numel() / 1e6, 1), "note": "includes the host-to-device copy of the packed batch"}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        torch.set_num_threads(1)
        pil = [Image.fromarray(im) for im in images[:a.pil_images]]
        t0 = time.perf_counter()
        for im in pil:
            w, h = im.size
            nh, nw, top, left = eval_geometry(h, w, 256, 224)
            im.resize((nw, nh), Image.BICUBIC).crop((left, top, left + 224, top + 224)).tobytes()
        res["pil_ms_per_image_1thread"] = round((time.perf_counter() - t0) * 1000 / len(pil), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
