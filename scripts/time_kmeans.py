#!/usr/bin/env python3
"""Times k-means on the int8 feature bank (csrc/kmeans.hip, cluster.py): the assign launch alone and one full iteration (assign,
stable sort of the labels, group sums, update), beside the float path on the same data -- `x.float() @ c.T`, `argmin`, `index_add_`,
the division -- and beside the search kernel run in the assignment's shape (every bank row a query, the centroids' hi plane as the
bank, k = 1: its traffic, not its answer) as a sanity bound.

    python scripts/time_kmeans.py [--C 384 768] [--K 100 1000] [--N 100000 1281167] [--repeats 7] [--out FILE.json]

Seeded random int8 rows around K planted centres, the centroids after one iteration from K of the rows; device events around a
synchronised window; every path is warmed up at the timed shape, the paths take turns inside one process and every repeat is
reported, one JSON line per (C, K, N).  Before timing the float path's labels are compared with the kernel's (they can differ
where float32 rounds a near-tie the other way; the count is reported)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, cluster, hiptime, knn  # noqa: E402

PEAK_INT8_OPS = 5.033e15      # the dense int8 MFMA peak the other kernels are held against


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


def float_iteration(xf, c, K):
    """one Lloyd iteration on a float32 copy of the bank -> (label, new centroids)"""
    d = (c * c).sum(dim=1)[None, :] - 2.0 * (xf @ c.T)
    label = d.argmin(dim=1)
    sums = torch.zeros_like(c).index_add_(0, label, xf)
    n = torch.bincount(label, minlength=K).to(torch.float32)
    return label, torch.where(n[:, None] > 0, sums / n.clamp(min=1.0)[:, None], c)


def case(a, Cc, K, N, dev):
    g = torch.Generator(device=dev).manual_seed(97 + Cc + K + N)
    centres = torch.randint(-100, 101, (K, Cc), generator=g, device=dev, dtype=torch.int16)
    x = (centres[torch.randint(0, K, (N,), generator=g, device=dev)] + torch.randint(-20, 21, (N, Cc), generator=g, device=dev, dtype=torch.int16)).clamp(-128, 127).to(torch.int8)
    km = cluster.KMeans(Cc, K, dev)
    km.init_from_rows(x, torch.randperm(N, generator=torch.Generator().manual_seed(1))[:K])
    km._iterate(x, N)                                   # centroids with both planes in use; warms every launch of an iteration
    planes = (km.hi.clone(), km.lo.clone(), km.cnorm.clone())

    def restore():
        for dst, src in zip((km.hi, km.lo, km.cnorm), planes):
            dst.copy_(src)

    xf = x.float()
    c = km.centroids.clone()
    flabel, _ = float_iteration(xf, c, K)               # warm-up of the float path
    label, _ = cluster.assign(x, km)
    bank = knn.FeatureBank(km.hi, torch.zeros(K, dtype=torch.int64, device=dev), 1.0)
    bank.search(x, 1)
    torch.cuda.synchronize()
    differ = int((flabel.to(torch.int32) != label).sum())
    t_assign, t_iter, t_float, t_conv, t_search = [], [], [], [], []
    for _ in range(a.repeats):
        t_assign.append(timed(lambda: cluster.assign(x, km))[0])
        t_float.append(timed(lambda: float_iteration(xf, c, K))[0])
        t_iter.append(timed(lambda: int(km._iterate(x, N)[2].sum()))[0])      # with the readback of `changed`, as fit pays it
        restore()
        t_conv.append(timed(lambda: x.float())[0])
        t_search.append(timed(lambda: bank.search(x, 1))[0])
    ops = 2.0 * N * K * Cc * 2                          # both planes, multiply and add
    med = statistics.median(t_assign)
    return {"C": Cc, "K": K, "N": N, "workgroups": (N + 127) // 128, "assign": spread(t_assign), "iteration": spread(t_iter),
            "float_iteration_on_a_resident_float_copy": spread(t_float), "float_copy_of_the_bank": spread(t_conv),
            "search_kernel_in_this_shape": spread(t_search), "assign_int8_ops": ops, "assign_ops_per_s": ops / (med * 1e-3),
            "assign_share_of_int8_peak": ops / (med * 1e-3) / PEAK_INT8_OPS, "centroid_bytes_through_lds": ((N + 127) // 128) * 2.0 * K * Cc,
            "float_labels_differing": differ, "float_over_iteration": statistics.median(t_float) / statistics.median(t_iter)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, nargs="+", default=[384, 768])
    ap.add_argument("--K", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--N", type=int, nargs="+", default=[100000, 1281167])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kmeans_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for Cc in a.C:
        for K in a.K:
            for N in a.N:
                line = json.dumps(case(a, Cc, K, N, "cuda:0"))
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
