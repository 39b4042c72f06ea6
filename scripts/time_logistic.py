#!/usr/bin/env python3
"""Times one step of the logistic probe (csrc/logistic.hip: ivit_probe_ce_forward_i8, ivit_probe_sgd_update_i8) and one epoch over
an ImageNet-sized synthetic int8 bank, beside the route that was possible before: a float32 copy of the bank, a torch gather of
the batch, F.linear, F.cross_entropy, backward and torch.optim.SGD with momentum.

    python scripts/time_logistic.py [--N 1281167 --C 1536 --K 1000 --B 1024] [--repeats 5] [--out profiles/logistic_timing.json]

Same seeded random int8 rows and labels for both; device events around windows of `--window` launches, a host clock around whole
epochs that end in a synchronise; every timed shape is warmed up first; the two routes alternate inside one process and every
repeat is reported.  The float route's extra memory is the float32 copy of the bank (4 N C bytes), reported."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime, probe  # noqa: E402


def window_ms(fn, n):
    st = _lib.stream_ptr()
    a, b = hiptime.Event(), hiptime.Event()
    torch.cuda.synchronize()
    a.record(st)
    for _ in range(n):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_ms(b) / n


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1281167)
    ap.add_argument("--C", type=int, default=1536)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev, s = "cuda:0", 2.0 ** -5
    g = torch.Generator(device=dev).manual_seed(1234)
    bank = torch.randint(-128, 128, (a.N, a.C), generator=g, dtype=torch.int8, device=dev)
    labels = torch.randint(0, a.K, (a.N,), generator=g, dtype=torch.int64, device=dev)
    fbank = bank.float() * s
    steps = (a.N + a.B - 1) // a.B

    tr = probe.LogisticTrainer(a.C, a.K, s, dev)
    idx = torch.randperm(a.N, device=dev)[:a.B].to(torch.int32)
    y = labels[idx.long()].to(torch.int32)
    loss, top1 = tr.step(bank, idx, y, 0.01)
    st, x, ldx = _lib.stream_ptr(), _lib.ptr(bank), bank.stride(0)

    def forward():
        _lib.call("ivit_probe_ce_forward_i8", x, ldx, a.C, _lib.ptr(idx), _lib.ptr(y), a.B, a.K, s, _lib.ptr(tr.Wh), _lib.ptr(tr.b), _lib.ptr(tr.G),
                  _lib.ptr(loss), _lib.ptr(top1), None, st)

    def update():
        _lib.call("ivit_probe_sgd_update_i8", x, ldx, a.C, _lib.ptr(idx), a.B, a.K, s, _lib.ptr(tr.G), 0.01, 0.9, 0.0, _lib.ptr(tr.W), _lib.ptr(tr.b),
                  _lib.ptr(tr.mW), _lib.ptr(tr.mb), _lib.ptr(tr.Wh), st)

    head = torch.nn.Linear(a.C, a.K, device=dev)
    torch.nn.init.zeros_(head.weight), torch.nn.init.zeros_(head.bias)
    opt = torch.optim.SGD(head.parameters(), lr=0.01, momentum=0.9)

    def torch_step(i=None, t=None):
        i = idx.long() if i is None else i
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(F.linear(fbank[i], head.weight, head.bias), labels[i] if t is None else t).backward()
        opt.step()

    def epoch_hip():
        perm = torch.randperm(a.N, device=dev)
        yp, perm = labels[perm].to(torch.int32), perm.to(torch.int32)
        for k in range(steps):
            tr.step(bank, perm[k * a.B:(k + 1) * a.B], yp[k * a.B:(k + 1) * a.B], probe.cosine_lr(0.01, k, steps))

    def epoch_torch():
        perm = torch.randperm(a.N, device=dev)
        yp = labels[perm]
        for k in range(steps):
            torch_step(perm[k * a.B:(k + 1) * a.B], yp[k * a.B:(k + 1) * a.B])

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in (forward, update, torch_step):      # warm-up of every path at the timed shape
        window_ms(fn, 20)
    t = {k: [] for k in ("forward", "update", "hip_step", "torch_step", "hip_epoch", "torch_epoch")}
    for _ in range(a.repeats):
        t["forward"].append(window_ms(forward, a.window))
        t["update"].append(window_ms(update, a.window))
        t["hip_step"].append(window_ms(lambda: tr.step(bank, idx, y, 0.01), a.window))
        t["torch_step"].append(window_ms(torch_step, a.window))
        t["hip_epoch"].append(host_ms(epoch_hip))
        t["torch_epoch"].append(host_ms(epoch_torch))
    med = {k: statistics.median(v) for k, v in t.items()}
    Kp = (a.K + 63) // 64 * 64
    res = {"N": a.N, "C": a.C, "K": a.K, "B": a.B, "steps_per_epoch": steps, "window": a.window,
           "forward_ms": spread(t["forward"]), "update_ms": spread(t["update"]), "hip_step_ms": spread(t["hip_step"]),
           "torch_step_ms": spread(t["torch_step"]), "hip_epoch_ms": spread(t["hip_epoch"]), "torch_epoch_ms": spread(t["torch_epoch"]),
           "step_speedup_median": med["torch_step"] / med["hip_step"], "epoch_speedup_median": med["torch_epoch"] / med["hip_epoch"],
           "forward_Wh_stream_TB_per_s": (a.B + 15) // 16 * Kp * a.C * 2 / (med["forward"] * 1e-3) / 1e12,
           "update_state_TB_per_s": Kp * a.C * 18 / (med["update"] * 1e-3) / 1e12,
           "bank_bytes_int8": a.N * a.C, "float_route_extra_bytes": 4 * a.N * a.C}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
