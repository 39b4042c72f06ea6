"""Time evaluation input with device JPEG decoding (compressed copy + ivit_jpeg_decode_u8 + resize/crop) against the decoded path
(copy of the decoded batch + resize/crop) on b256 batches of the ImageNet-size JPEGs of tests/golden/jpeg_decode_pil.npz,
event-timed on cuda:0; and Pillow's decode (Image.open(f).convert("RGB")) of the same files with 16 worker processes, when Pillow is
installed.  One JSON line.  For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python ...`.

    python scripts/time_jpeg_decode.py [--batch 256] [--iters 20]
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
from ivit_amd.transforms import EvalTransform, decode_images, decode_jpeg_host, encode_images, pack_images  # noqa: E402

NAMES = ("333x500_420_q90_opt", "500x375_444_q75", "500x375_gray_q90_rows1", "375x500_422_q50_rst3")


def _files():
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode_pil.npz"))
    names = [str(n) for n in z["names"]]
    return [z["data"][z["data_off"][names.index(n)]:z["data_off"][names.index(n) + 1]].tobytes() for n in NAMES]


def _pil_decode(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).shape


def _timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    files = _files()
    batch = [files[i % len(files)] for i in range(a.batch)]
    t0 = time.perf_counter()
    enc = encode_images(batch)
    plan_ms = (time.perf_counter() - t0) * 1000
    packed = pack_images([decode_jpeg_host(f) for f in batch])
    t = EvalTransform()
    out = torch.empty(a.batch, 3, 224, 224, dtype=torch.uint8, device="cuda:0")
    dec_ms = _timed(lambda: decode_images(enc, device="cuda:0"), a.iters)
    jpeg_ms = _timed(lambda: t(enc, device="cuda:0", out=out), a.iters)
    u8_ms = _timed(lambda: t(packed, device="cuda:0", out=out), a.iters)
    res = {"batch": a.batch, "jpeg_mb_per_batch": round(sum(len(f) for f in batch) / 1e6, 2),
           "plan_mb_per_batch": round(enc.plan.numel() / 1e6, 2), "decoded_mb_per_batch": round(packed.data.numel() / 1e6, 1),
           "host_plan_ms_per_batch_1thread": round(plan_ms, 2),
           "jpeg_copy_decode_ms": round(dec_ms, 3),
           "jpeg_copy_decode_resize_crop_ms": round(jpeg_ms, 3), "jpeg_images_per_s": round(a.batch / jpeg_ms * 1000),
           "decoded_copy_resize_crop_ms": round(u8_ms, 3), "decoded_images_per_s": round(a.batch / u8_ms * 1000),
           "note": "device times include the error-flag readback of every decode (a synchronisation)"}
    try:
        import PIL  # noqa: F401
        from multiprocessing import get_context
        with get_context("spawn").Pool(16) as pool:
            pool.map(_pil_decode, batch[:32])
            t0 = time.perf_counter()
            n = 0
            for _ in range(4):
                n += len(pool.map(_pil_decode, batch, chunksize=4))
            res["pil_16_processes_images_per_s"] = round(n / (time.perf_counter() - t0))
    except ImportError:
        res["pil_16_processes_images_per_s"] = "not measured (no Pillow)"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
