#!/usr/bin/env python3
"""Times what follows TokenMemory.propagate for one sequence of the DAVIS protocol, two ways on the same seeded soft labels and masks:
  torch tail   per frame F.interpolate (bilinear, align_corners=False) of the [1, K, Gh, Gw] soft labels, argmax, and per object two
               boolean reductions fetched with int(...): the scoring lines of inference.evaluate_video_segmentation (J only)
  new path     per frame propagate.upsample_argmax into one [L, H, W] buffer, ONE propagate.mask_scores for the sequence (J and F)
               and one readback (davis_measures)

    python scripts/time_davis_score.py [--shapes 480x848x16 480x848x8] [--K 4] [--frames 64] [--repeats 10] [--out FILE.json]

Device events around a window that ends in the readback both paths need; the timed shape is warmed up first; the two paths alternate
inside one process and every repeat is reported, one JSON line per shape.  The kernels alone (no readback) are timed as a third
line.  Before timing, the label maps of the two paths are compared: `pixels_differ` counts the pixels where torch's float32
interpolation and the exact float64 one pick another class."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime  # noqa: E402
from ivit_amd.propagate import bound_radius, davis_measures, mask_scores, upsample_argmax  # noqa: E402


def timed(fn):
    st = _lib.stream_ptr()
    a, b = hiptime.Event(), hiptime.Event()
    torch.cuda.synchronize()
    a.record(st)
    out = fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_ms(b), out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": [round(x, 3) for x in ms]}


def torch_tail(segs, truth, Gh, Gw, r, K):
    inter = torch.zeros(K - 1, dtype=torch.float64, device=truth.device)
    preds = []
    for t, seg in enumerate(segs):
        up = torch.nn.functional.interpolate(seg.t().reshape(1, K, Gh, Gw), scale_factor=r, mode="bilinear", align_corners=False)
        pred = up[0].argmax(dim=0)
        preds.append(pred)
        for o in range(1, K):
            p, g = pred == o, truth[t] == o
            u = int((p | g).sum())
            inter[o - 1] += 1.0 if u == 0 else int((p & g).sum()) / u
    return float(inter.sum()), preds


def new_kernels(segs, truth, pred, Gh, Gw, r, K):
    for t, seg in enumerate(segs):
        upsample_argmax(seg, (Gh, Gw), r, out=pred[t])
    return mask_scores(pred, truth, K - 1)


def case(a, H, W, r, dev):
    Gh, Gw, K, L = H // r, W // r, a.K, a.frames
    g = torch.Generator(device=dev).manual_seed(H + W + r)
    segs = [torch.softmax(4 * torch.randn(Gh * Gw, K, generator=g, device=dev), dim=1) for _ in range(L)]
    coarse = torch.randint(0, K, (L, 1, H // 32, W // 32), generator=g, device=dev).float()      # blobs of 32 x 32 pixels
    truth = torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[:, 0].to(torch.uint8).contiguous()
    pred = torch.empty_like(truth)

    total, preds = torch_tail(segs, truth, Gh, Gw, r, K)                    # warm-up of both paths at the timed shape
    J, _ = davis_measures(new_kernels(segs, truth, pred, Gh, Gw, r, K))
    differ = int(sum((p != q).sum() for p, q in zip(preds, pred)))
    if differ == 0:
        assert abs(total - float(J.sum())) < 1e-9, "equal label maps, different J"
    base, new, kern = [], [], []
    for _ in range(a.repeats):
        base.append(timed(lambda: torch_tail(segs, truth, Gh, Gw, r, K))[0])
        new.append(timed(lambda: davis_measures(new_kernels(segs, truth, pred, Gh, Gw, r, K)))[0])
        kern.append(timed(lambda: new_kernels(segs, truth, pred, Gh, Gw, r, K))[0])
    return {"H": H, "W": W, "r": r, "K": K, "frames": L, "bound_radius": bound_radius(0.008, H, W), "pixels_differ": differ,
            "pixels": L * H * W, "torch_tail": spread(base), "new_path": spread(new), "new_kernels_alone": spread(kern),
            "torch_over_new": statistics.median(base) / statistics.median(new)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["480x848x16", "480x848x8"])
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    for shape in a.shapes:
        H, W, r = (int(v) for v in shape.split("x"))
        line = json.dumps(case(a, H, W, r, "cuda:0"))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
