#!/usr/bin/env python3
"""Times discover.discover_objects (csrc/discover.hip: the degree pass on the int8 MFMA and the one-workgroup-per-image tail) against
what a user did before it existed, LOST's float path on the same tokens: bmm to the [B, hw, hw] affinity matrix, > 0, sum, argsort,
gather, sum, > 0, then the connected component of the seed per image on the host (a flood fill on the row words: the stand-in
for scipy.ndimage.label, which costs the same readback).

    python scripts/time_discover.py [--C 384 768] [--grids 14x14 32x32 60x64] [--B 64] [--k 100] [--repeats 10] [--out FILE.json]

Same seeded random int8 tokens for both; device events around a synchronised window (the float path's host tail included: it ends in
the synchronise of its readback); the timed shape is warmed up first; the two paths alternate inside one process and every repeat is
reported, one JSON line per (C, grid).  The boxes of the two paths are compared where the float path is exact (its float32 dot
products of int8 values below 2^24 are) -- the float path breaks equal degrees by argsort's order, so only images whose seed agrees
are compared."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, discover, hiptime  # noqa: E402


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


def host_component(mask, sy, sx):
    """the 4-connected component of (sy, sx) in a mask given as Gh lists of Gw bools, on the host -> (x0, y0, x1, y1)"""
    Gh, Gw = len(mask), len(mask[0])
    words = [sum(1 << x for x in range(Gw) if mask[y][x]) for y in range(Gh)]
    cur = [0] * Gh
    cur[sy] = (1 << sx)
    if words[sy] >> sx & 1:
        while True:
            new = [(cur[y] | cur[y] << 1 | cur[y] >> 1 | (cur[y - 1] if y else 0) | (cur[y + 1] if y + 1 < Gh else 0)) & words[y] for y in range(Gh)]
            if new == cur:
                break
            cur = new
    orw = 0
    for w in cur:
        orw |= w
    ys = [y for y in range(Gh) if cur[y]]
    return (orw & -orw).bit_length() - 1, ys[0], orw.bit_length() - 1, ys[-1]


def float_discover(f, Gh, Gw, k):
    """-> (boxes list, seed int64 [B]) from float32 tokens [B, hw, C]"""
    B, hw, _ = f.shape
    A = torch.bmm(f, f.transpose(1, 2))
    deg = (A > 0).sum(-1) - (A.diagonal(dim1=1, dim2=2) > 0).long()
    order = torch.argsort(deg, dim=1, stable=True)
    seed, pot = order[:, 0], order[:, :min(k, hw)]
    sim = torch.gather(A, 1, seed[:, None, None].expand(B, 1, hw))[:, 0].gather(1, pot) > 0
    sim[:, 0] = True
    M = (torch.gather(A, 1, pot[:, :, None].expand(B, pot.shape[1], hw)) * sim[:, :, None]).sum(1)
    mask, seeds = (M > 0).reshape(B, Gh, Gw).cpu().tolist(), seed.cpu().tolist()      # the readback
    return [host_component(mask[b], seeds[b] // Gw, seeds[b] % Gw) for b in range(B)], seed


def case(a, Cc, Gh, Gw, dev):
    hw = Gh * Gw
    g = torch.Generator(device=dev).manual_seed(4321 + Cc + hw)
    tok = torch.randint(-128, 128, (a.B, hw, Cc), generator=g, dtype=torch.int8, device=dev)
    f = tok.float()

    boxes, seed, deg = discover.discover_objects(tok, (Gh, Gw), a.k)      # warm-up of both paths at the timed shape
    fboxes, fseed = float_discover(f, Gh, Gw, a.k)
    torch.cuda.synchronize()
    same_seed = (fseed == seed.long()).cpu().tolist()
    got = boxes.cpu().tolist()
    differ = sum(1 for b in range(a.B) if same_seed[b] and tuple(got[b]) != tuple(fboxes[b]))
    new, degrees, base = [], [], []
    for _ in range(a.repeats):
        new.append(timed(lambda: discover.discover_objects(tok, (Gh, Gw), a.k)[0].cpu())[0])      # with its one readback
        base.append(timed(lambda: float_discover(f, Gh, Gw, a.k))[0])
        degrees.append(timed(lambda: discover.token_degrees(tok, (Gh, Gw)))[0])
    return {"C": Cc, "grid": [Gh, Gw], "B": a.B, "k": a.k, "workgroups": a.B * ((hw + 63) // 64), "macs": a.B * hw * hw * Cc,
            "images_compared": sum(same_seed), "images_differing": differ, "discover_objects": spread(new), "token_degrees_alone": spread(degrees),
            "float_path": spread(base), "float_over_discover": statistics.median(base) / statistics.median(new),
            "float_affinity_bytes": 4 * a.B * hw * hw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--grids", nargs="+", default=["14x14", "32x32", "60x64"])
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "discover_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for Cc in a.C:
        for grid in a.grids:
            Gh, Gw = (int(v) for v in grid.split("x"))
            line = json.dumps(case(a, Cc, Gh, Gw, "cuda:0"))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
