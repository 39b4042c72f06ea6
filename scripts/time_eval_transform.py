"""Time the device evaluation transform (ivit_resize_crop_bicubic_u8: Resize 256 BICUBIC -> CenterCrop 224) on a batch of 256
ImageNet-like sizes, event-timed on cuda:0, next to the single-thread Pillow cost of the same images (Image.resize + crop), when
Pillow is installed.  One JSON line.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python scripts/time_eval_transform.py [--batch 256] [--iters 50] [--pil-images 64]

--resize S | H W, --crop C | H W and --pad time the h x w entry (ivit_resize_crop_bicubic_hw_u8) instead: a pair for --resize is an
exact-size resize, a pair for --crop an h x w crop, --pad lets CenterCrop pad with zeros.  --runs N repeats the timed window
and prints the median and the range of the N figures.

    python scripts/time_eval_transform.py --resize 109 --crop 64 96             # EvalTransform.for_input_size((64, 96))
    python scripts/time_eval_transform.py --resize 384 384 --crop 384           # Swin's 384 px checkpoints: no crop
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
from ivit_amd.transforms import EvalTransform, pack_images  # noqa: E402

SIZES = [(375, 500), (500, 375), (333, 500), (480, 640), (768, 1024), (375, 500), (500, 333), (200, 150), (180, 240), (256, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pil-images", type=int, default=64)
    ap.add_argument("--resize", type=int, nargs="+", default=[256], help="S (short side) or H W (exact size)")
    ap.add_argument("--crop", type=int, nargs="+", default=[224], help="C or H W")
    ap.add_argument("--pad", action="store_true")
    ap.add_argument("--runs", type=int, default=1)
    a = ap.parse_args()
    if len(a.resize) > 2 or len(a.crop) > 2:
        ap.error("--resize and --crop take one or two integers")
    resize = a.resize[0] if len(a.resize) == 1 else tuple(a.resize)
    crop = a.crop[0] if len(a.crop) == 1 else tuple(a.crop)
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (*SIZES[i % len(SIZES)], 3), dtype=np.uint8) for i in range(a.batch)]
    packed = pack_images(images)
    t = EvalTransform(resize, crop, pad=a.pad)
    ch, cw = t.crop_hw
    out = torch.empty(a.batch, 3, ch, cw, dtype=torch.uint8, device="cuda:0")
    for _ in range(5):
        t(packed, device="cuda:0", out=out)
    torch.cuda.synchronize()
    runs = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            t(packed, device="cuda:0", out=out)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / a.iters)
    dev_ms = float(np.median(runs))
    res = {"batch": a.batch, "resize": resize, "crop": crop, "pad": a.pad, "device_ms_per_batch": round(dev_ms, 4),
           "device_us_per_image": round(dev_ms * 1000 / a.batch, 3), "input_mb_per_batch": round(packed.data.numel() / 1e6, 1),
           "note": "includes the host-to-device copy of the packed batch"}
    if a.runs > 1:
        res["runs_ms_per_batch"] = [round(v, 4) for v in runs]
        res["range_ms_per_batch"] = [round(min(runs), 4), round(max(runs), 4)]
    try:
        from PIL import Image
        from ivit_amd.transforms import eval_geometry_hw
    except ImportError:
        Image = None
    if Image is not None:
        torch.set_num_threads(1)
        pil = [Image.fromarray(im) for im in images[:a.pil_images]]
        t0 = time.perf_counter()
        for im in pil:
            w, h = im.size
            nh, nw, top, left = eval_geometry_hw(h, w, resize, crop, a.pad)
            im.resize((nw, nh), Image.BICUBIC).crop((left, top, left + cw, top + ch)).tobytes()       # PIL's crop pads with zeros too
        res["pil_ms_per_image_1thread"] = round((time.perf_counter() - t0) * 1000 / len(pil), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
