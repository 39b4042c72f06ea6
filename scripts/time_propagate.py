#!/usr/bin/env python3
"""Times propagate.TokenMemory.propagate (the windowed int8 similarity + top-k of csrc/propagate.hip and the label mix) against what
a user did before it existed, the float path of the DAVIS protocol on the same tokens: normalise, bmm to the [hw, F * hw] affinity
matrix, the window mask, torch.topk along the long axis, exp and renormalise, mm with the labels.

    python scripts/time_propagate.py [--C 384 768] [--grids 24x40 60x106] [--F 8 --radius 12 --k 5 --K 8] [--repeats 20] [--out FILE.json]

Same seeded random int8 tokens for both; device events around a synchronised window; the timed shape is warmed up first; the two
paths alternate inside one process and every repeat is reported, one JSON line per (C, grid).  The neighbours of the two paths are
compared for every target whose float32 cosines have no tie among its first k + 1 candidates.  The float path is timed WITH its mask
built beforehand (a protocol run builds it once per sequence) and with the float copy of the tokens made beforehand: what is timed is
the per-frame work of either path.  `workgroups` and `splits`: what the launcher chose for the search (splits = 0)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime  # noqa: E402
from ivit_amd.knn import knn_weights  # noqa: E402
from ivit_amd.propagate import TokenMemory  # noqa: E402


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


def window_mask(Gh, Gw, F, radius, dev):
    y, x = torch.arange(Gh * Gw, device=dev) // Gw, torch.arange(Gh * Gw, device=dev) % Gw
    near = ((y[:, None] - y[None, :]).abs() <= radius) & ((x[:, None] - x[None, :]).abs() <= radius)
    return near.repeat(1, F)


def float_propagate(qn, bn, mask, seg, k, T):
    """-> (labels [hw, K], idx [hw, k + 1], cos [hw, k + 1]) from normalised float tokens"""
    aff = torch.mm(qn, bn.T).masked_fill_(~mask, float("-inf"))
    v, i = torch.topk(aff, k + 1, dim=1)
    w = torch.exp(v[:, :k] / T)
    w = w / w.sum(dim=1, keepdim=True)
    return torch.bmm(w[:, None, :], seg[i[:, :k]])[:, 0], i, v


def auto_splits(Gh, Gw, F, k):
    need = C.c_int64()
    _lib.call("ivit_local_topk_workspace_bytes", Gh, Gw, F, k, 0, C.byref(need))
    return max(1, need.value // (Gh * Gw * k * 8))


def case(a, Cc, Gh, Gw, dev):
    hw = Gh * Gw
    g = torch.Generator(device=dev).manual_seed(1234 + Cc + hw)
    ctx = torch.randint(-128, 128, (a.F, hw, Cc), generator=g, dtype=torch.int8, device=dev)
    q = torch.randint(-128, 128, (hw, Cc), generator=g, dtype=torch.int8, device=dev)
    seg = torch.softmax(torch.randn(a.F * hw, a.K, generator=g, device=dev), dim=1)
    mem = TokenMemory(Gh, Gw, Cc, a.K, a.F, dev)
    for f in range(a.F):
        mem.put(f, ctx[f], seg[f * hw:(f + 1) * hw])
    qn = torch.nn.functional.normalize(q.float(), dim=1)
    bn = torch.nn.functional.normalize(ctx.reshape(-1, Cc).float(), dim=1)
    mask = window_mask(Gh, Gw, a.F, a.radius, dev)

    idx, cos = mem.neighbours(q, a.radius, a.k)                     # warm-up of both paths at the timed shape, and they agree
    out = mem.propagate(q, a.radius, a.k, a.T)
    fout, fidx, fval = float_propagate(qn, bn, mask, seg, a.k, a.T)
    torch.cuda.synchronize()
    untied = (fval[:, :-1] - fval[:, 1:] > 1e-6).all(dim=1)
    same = (fidx[:, :a.k] == idx.long()).all(dim=1)
    assert bool(same[untied].all()), f"{int((~same[untied]).sum())} targets without a near tie differ between the two paths"
    assert float((out - fout)[untied].abs().max()) < 1e-3, "the labels of the two paths differ"
    fused, base, search = [], [], []
    for _ in range(a.repeats):
        fused.append(timed(lambda: mem.propagate(q, a.radius, a.k, a.T))[0])
        base.append(timed(lambda: float_propagate(qn, bn, mask, seg, a.k, a.T))[0])
        search.append(timed(lambda: mem.neighbours(q, a.radius, a.k))[0])
    sp = auto_splits(Gh, Gw, a.F, a.k)
    tiles = ((Gh + 3) // 4) * ((Gw + 7) // 8)
    return {"C": Cc, "grid": [Gh, Gw], "F": a.F, "radius": a.radius, "k": a.k, "K": a.K, "splits": sp, "workgroups": tiles * sp,
            "targets_compared": int(untied.sum()), "propagate": spread(fused), "neighbours_alone": spread(search), "float_path": spread(base),
            "float_over_propagate": statistics.median(base) / statistics.median(fused),
            "float_affinity_bytes": 4 * hw * a.F * hw, "float_mask_bytes": hw * a.F * hw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--grids", nargs="+", default=["24x40", "60x106"])
    ap.add_argument("--F", type=int, default=8)
    ap.add_argument("--radius", type=int, default=12)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--T", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    for Cc in a.C:
        for grid in a.grids:
            Gh, Gw = (int(v) for v in grid.split("x"))
            line = json.dumps(case(a, Cc, Gh, Gw, "cuda:0"))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
