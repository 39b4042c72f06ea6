"""Times calibration forwards: an unfrozen model with running statistics, so that every QuantLinear and
QuantConv2d re-derives its integer parameters on every batch.

    python scripts/time_calibration_forward.py [--configs NAMES] [--batch 128] [--forwards 5] [--warmup 2] [--label TEXT]
                                               [--params-timer] [--out FILE.json]

Per configuration: a fresh model with random weights (the factories' initialisation), `warmup` forwards, then `forwards` timed ones,
each on a new random batch with another amplitude, so that every range moves and every input scale changes.  Each forward is timed
by device events around `model(x)` and by the host's wall clock around the same call plus the synchronisation behind it.  Reported:
every forward, and the range (fastest, slowest) of both clocks.

Configurations: deit_tiny, deit_base, deit_base_ibert (the I-BERT operator family), swin_tiny; all at --batch.
--params-timer: additionally the host's wall clock spent inside QuantLinear._params (device synchronised on entry and exit), summed
per forward: the cost of deriving the linear layers' integer parameters.  It adds synchronisations, so it runs as forwards of its
own behind the timed ones.
Only the package's public interface is used (and, for --params-timer, the one method it wraps), so the same file times an older tree:
    python scripts/time_calibration_forward.py --root OLDER_TREE ...
For the kernels' durations: rocprofv3 --kernel-trace --stats -- python scripts/time_calibration_forward.py --configs deit_base"""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="deit_tiny,deit_base,deit_base_ibert,swin_tiny")
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--forwards", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--label", default="")
ap.add_argument("--params-timer", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the tree whose package is timed")
ap.add_argument("--out", default=None)
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import ivit_amd as ivit  # noqa: E402

DEV = "cuda:0"
IBERT = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
CONFIGS = {"deit_tiny": lambda: ivit.deit_tiny_patch16_224(), "deit_base": lambda: ivit.deit_base_patch16_224(),
           "deit_base_ibert": lambda: ivit.deit_base_patch16_224(**IBERT), "swin_tiny": lambda: ivit.swin_tiny_patch4_window7_224()}


def batch(g, i):
    return torch.randn(args.batch, 3, 224, 224, device=DEV, generator=g) * (1.0 + 0.25 * (i % 5))


def one(model, x):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    with torch.no_grad():
        model(x)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def run(name):
    torch.manual_seed(0)
    model = CONFIGS[name]().to(DEV).eval()
    weights = sum(m.weight.numel() for m in model.modules() if isinstance(m, (ivit.QuantLinear, ivit.QuantConv2d)))
    g = torch.Generator(device=DEV).manual_seed(1)
    for i in range(args.warmup):
        one(model, batch(g, i))
    dev, wall = [], []
    for i in range(args.forwards):
        d, w = one(model, batch(g, args.warmup + i))
        dev.append(round(d, 3))
        wall.append(round(w, 3))
    res = {"config": name, "batch": args.batch, "label": args.label, "linear_weights": weights, "device_ms": dev, "wall_ms": wall,
           "device_ms_range": [min(dev), max(dev)], "wall_ms_range": [min(wall), max(wall)]}
    if args.params_timer:
        spent = [0.0]
        orig = ivit.QuantLinear._params

        def timed(self, s_in):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = orig(self, s_in)
            torch.cuda.synchronize()
            spent[0] += (time.perf_counter() - t0) * 1e3
            return r
        ivit.QuantLinear._params = timed
        try:
            per = []
            for i in range(3):
                spent[0] = 0.0
                one(model, batch(g, 100 + i))
                per.append(round(spent[0], 3))
        finally:
            ivit.QuantLinear._params = orig
        res["params_host_ms"] = per
    print(json.dumps(res), flush=True)
    return res


results = [run(n) for n in args.configs.split(",")]
if args.out:
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
