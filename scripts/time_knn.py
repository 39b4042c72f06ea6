#!/usr/bin/env python3
"""Times FeatureBank.search (the fused int8 similarity + top-k of csrc/knn.hip) against what a user did before it existed: the bank
as float32, torch.matmul over chunks of bank rows, times rnorm, torch.topk per chunk, and a merge of the chunks' lists.

    python scripts/time_knn.py [--N 1281167 --C 768 --Q 8192 --k 200] [--repeats 5] [--out FILE.json]
    python scripts/time_knn.py --N 100000 --Q 1000 --k 20 --splits-ab        # also: automatic segments against one segment

Same seeded random int8 inputs for both; device events around a synchronised window; the timed shape is warmed up first; the two
paths alternate inside one process and every repeat is reported.  The indices of the two paths are compared for every query whose
float32 scores have no tie among its first k + 1 neighbours (there the order is the same by construction: at C <= 1024 the float32
dot products are exact integers, so both paths form the same score bits).  `share_of_int8_peak`: 2 Q N C operations over the time of
the search, against 5.0e15 op/s (the dense INT8 MFMA rate: twice the 2.5 PF of BF16) -- the whole search call, query norms and the
merge of the segments included, so a kernel alone is slightly better than this figure."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime  # noqa: E402
from ivit_amd.knn import FeatureBank  # noqa: E402

INT8_PEAK = 5.0e15


def timed(fn):
    st = _lib.stream_ptr()
    a, b = hiptime.Event(), hiptime.Event()
    torch.cuda.synchronize()
    a.record(st)
    out = fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_ms(b), out


def float_search(bank_f, rnorm, q_f, k, chunk):
    """the float path: scores of one chunk of bank rows at a time, its top-k, then the top-k of the chunks' lists"""
    vals, idxs = [], []
    for lo in range(0, bank_f.shape[0], chunk):
        s = torch.matmul(q_f, bank_f[lo:lo + chunk].T) * rnorm[None, lo:lo + chunk]
        v, i = torch.topk(s, min(k + 1, s.shape[1]), dim=1)
        vals.append(v)
        idxs.append(i + lo)
    v, i = torch.cat(vals, dim=1), torch.cat(idxs, dim=1)
    top, pos = torch.topk(v, k + 1 if v.shape[1] > k else k, dim=1)
    return torch.gather(i, 1, pos), top


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": [round(x, 3) for x in ms]}


def auto_splits(fb, Q, k):
    need = C.c_int64()
    _lib.call("ivit_knn_workspace_bytes", Q, fb.N, k, 0, C.byref(need))
    return max(1, need.value // (Q * k * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1281167)
    ap.add_argument("--C", type=int, default=768)
    ap.add_argument("--Q", type=int, default=8192)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=6e9, help="float32 scores of one chunk of the float path")
    ap.add_argument("--splits-ab", action="store_true", help="also time one bank segment against the automatic choice")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1234)
    bank = torch.randint(-128, 128, (a.N, a.C), generator=g, dtype=torch.int8, device=dev)
    q = torch.randint(-128, 128, (a.Q, a.C), generator=g, dtype=torch.int8, device=dev)
    fb = FeatureBank(bank, torch.zeros(a.N, dtype=torch.int64, device=dev), 1.0)
    bank_f, q_f = bank.float(), q.float()
    chunk = max(a.k + 1, int(a.chunk_bytes // (4 * a.Q)))

    idx, cos = fb.search(q, a.k)                                    # warm-up of both paths at the timed shape
    fidx, fval = float_search(bank_f, fb.rnorm, q_f, a.k, chunk)
    torch.cuda.synchronize()
    untied = (fval[:, :-1] != fval[:, 1:]).all(dim=1) if fval.shape[1] > a.k else torch.ones(a.Q, dtype=torch.bool, device=dev)
    same = (fidx[:, :a.k] == idx.long()).all(dim=1)
    assert bool(same[untied].all()), f"{int((~same[untied]).sum())} queries without a tie differ between the two paths"

    fused, base, one = [], [], []
    for _ in range(a.repeats):
        fused.append(timed(lambda: fb.search(q, a.k))[0])
        base.append(timed(lambda: float_search(bank_f, fb.rnorm, q_f, a.k, chunk))[0])
        if a.splits_ab:
            one.append(timed(lambda: fb.search(q, a.k, splits=1))[0])
    ops = 2.0 * a.Q * a.N * a.C
    res = {"N": a.N, "C": a.C, "Q": a.Q, "k": a.k, "auto_splits": auto_splits(fb, a.Q, a.k), "float_chunk_rows": chunk,
           "queries_compared": int(untied.sum()), "queries_with_a_float_tie": int((~untied).sum()),
           "fused_search": spread(fused), "float_path": spread(base),
           "speedup_median": statistics.median(base) / statistics.median(fused),
           "share_of_int8_peak": ops / (statistics.median(fused) * 1e-3) / INT8_PEAK,
           "bank_bytes_int8": a.N * a.C, "bank_bytes_float32": 4 * a.N * a.C}
    if one:
        res["fused_search_one_segment"] = spread(one)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
