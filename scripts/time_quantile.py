"""Times ivit_quantile_pair_f32: device events, warmed up, inputs resident, median of seven windows.

    python scripts/time_quantile.py [all | entry | model | profile_normal | profile_ties] [output directory]

entry:   the entry at n = 2^24 against torch.quantile on the same device and tensor (called twice, as the reference does), and at the
         fc1 shape of DeiT-T at batch 128 (19.4 M elements, where torch refuses), on normal and on tie-heavy quantised data
model:   one calibration forward of DeiT-T at batch 128 with percentile 99.99 against the same forward with min / max
profile_*: ten calls at 2^24 and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/time_quantile.py profile_ties`"""
import json
import os
import sys
import statistics

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ivit_amd as ivit  # noqa
from ivit_amd import _lib, inference, synth  # noqa
import quantile_ref as qr  # noqa

DEV = "cuda:0"
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
os.makedirs(OUT, exist_ok=True)
WS = _lib.QUANTILE_WS_BYTES
ws = torch.empty(WS, dtype=torch.uint8, device=DEV)
out = torch.empty(2, dtype=torch.float32, device=DEV)
res = {}


def timed(fn, reps, rounds=7, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / reps)     # us per call
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def data(kind, n):
    g = torch.Generator(device=DEV).manual_seed(3)
    t = torch.randn(n, device=DEV, generator=g) * 3
    if kind == "ties":
        t = torch.round(t * 14) * 0.0173          # ~ +-128 multiples of one scale
        t = t.clamp(-128 * 0.0173, 127 * 0.0173)
    return t.contiguous()


q_lo, q_hi = (float(v) for v in qr.percentile_qs(99.99))


def native(t):
    _lib.call("ivit_quantile_pair_f32", _lib.ptr(t), t.numel(), q_lo, q_hi, _lib.ptr(out), _lib.ptr(ws), WS, _lib.stream_ptr())


def by_torch(t):
    torch.quantile(t, q_lo)
    torch.quantile(t, q_hi)


mode = sys.argv[1] if len(sys.argv) > 1 else "all"
if mode in ("all", "entry"):
    for n, name in ((2 ** 24, "2^24"), (128 * 197 * 768, "fc1_deit_t_b128")):
        for kind in ("normal", "ties"):
            t = data(kind, n)
            r = {"n": n, "distinct": int(torch.unique(t).numel()) if kind == "ties" else None}
            r["native"] = timed(lambda: native(t), reps=20)
            r["bytes_4_passes"] = 4 * 4 * n
            r["native_TBps"] = r["bytes_4_passes"] / (r["native"]["median_us"] * 1e-6) / 1e12
            if n <= 2 ** 24:
                r["torch_x2"] = timed(lambda: by_torch(t), reps=3, rounds=5, warm=2)
                native(t)
                want = [float(torch.quantile(t, q_lo)), float(torch.quantile(t, q_hi))]
                r["equal_torch_gpu"] = out.cpu().tolist() == want
            res[f"{name}/{kind}"] = r
            print(name, kind, json.dumps(r), flush=True)
            del t

if mode in ("profile_normal", "profile_ties"):
    t = data(mode.split("_")[1], 2 ** 24)
    for _ in range(10):
        native(t)
    torch.cuda.synchronize()
    sys.exit(0)

if mode in ("all", "model"):
    torch.manual_seed(1)
    model = ivit.deit_tiny_patch16_224().to(DEV).eval()
    nq = sum(isinstance(m, ivit.QuantAct) for m in model.modules())
    imgs = torch.from_numpy(synth.make_images(128, 77)).to(DEV)
    r = {"quantacts": nq}
    for label, p in (("minmax", None), ("p99.99", 99.99), ("minmax_again", None), ("p99.99_again", 99.99)):
        inference.set_act_percentile(model, p)
        with torch.no_grad():
            r[label] = timed(lambda: model(imgs), reps=1, rounds=5, warm=2)
        print("calibration forward", label, json.dumps(r[label]), flush=True)
    r["added_us_per_quantact"] = (r["p99.99"]["median_us"] - r["minmax"]["median_us"]) / nq
    res["calibration_forward_deit_t_b128"] = r
    print(json.dumps(r), flush=True)

with open(os.path.join(OUT, f"quantile_timing_{mode}.json"), "w") as f:
    json.dump(res, f, indent=1)
