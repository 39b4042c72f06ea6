#!/usr/bin/env python3
"""Times the exact statistics of the linear probe (csrc/probe.hip: ivit_gram_i8_i64, ivit_group_sums_i8_i64) against the route that
was possible before they existed: the bank converted to float32 one chunk of rows at a time, torch.matmul for the Gram matrix
(accumulated in float32: neither exact nor reproducible), index_add_ for the class sums.

    python scripts/time_probe.py [--N 1281167 --C 768 --K 1000] [--repeats 5] [--out profiles/probe_timing.json]
    python scripts/time_probe.py --N 100000 --C 192 --K 1000

Same seeded random int8 rows and labels for both; device events around a synchronised window; every timed shape is warmed up first;
the paths alternate inside one process and every repeat is reported.  The CSR form of the labels (a stable sort, a bincount and a
cumulative sum in torch) is timed as its own line: BankStats.update pays it once per batch.  The float class sums are compared
with the exact ones (they are exact too while every sum stays below 2^24); the float Gram is reported with its largest deviation.
`gram_share_of_int8_peak`: 2 N C^2 operations (the dense count: the kernel computes the upper triangle, half of them) over the
time of the whole call, the reducer included, against 5.0e15 op/s.  `gram_over_bank_read`: the same time over that of reading the
bank once (an int64 torch.sum over the bank's bytes, measured here)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime  # noqa: E402

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


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": [round(x, 3) for x in ms]}


def csr(labels, K):
    perm = torch.sort(labels, stable=True).indices.to(torch.int32)
    ptr = torch.zeros(K + 1, dtype=torch.int64, device=labels.device)
    ptr[1:] = torch.cumsum(torch.bincount(labels, minlength=K), 0)
    return perm, ptr


def float_gram(bank, chunk):
    G = torch.zeros(bank.shape[1], bank.shape[1], dtype=torch.float32, device=bank.device)
    for lo in range(0, bank.shape[0], chunk):
        x = bank[lo:lo + chunk].float()
        G.addmm_(x.T, x)
    return G


def float_sums(bank, labels, K, chunk):
    S = torch.zeros(K, bank.shape[1], dtype=torch.float32, device=bank.device)
    for lo in range(0, bank.shape[0], chunk):
        S.index_add_(0, labels[lo:lo + chunk], bank[lo:lo + chunk].float())
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1281167)
    ap.add_argument("--C", type=int, default=768)
    ap.add_argument("--K", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk-bytes", type=float, default=1e9, help="float32 copy of one chunk of bank rows on the float route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1234)
    bank = torch.randint(-128, 128, (a.N, a.C), generator=g, dtype=torch.int8, device=dev)
    labels = torch.randint(0, a.K, (a.N,), generator=g, dtype=torch.int64, device=dev)
    chunk = max(1, int(a.chunk_bytes // (4 * a.C)))
    need = C.c_int64()
    _lib.call("ivit_gram_workspace_bytes", a.N, a.C, 0, C.byref(need))
    ws = torch.empty(max(need.value // 4, 1), dtype=torch.int32, device=dev)
    gram = torch.zeros(a.C, a.C, dtype=torch.int64, device=dev)
    sums = torch.zeros(a.K, a.C, dtype=torch.int64, device=dev)
    perm, ptr = csr(labels, a.K)
    words = bank.view(-1)[:a.N * a.C // 8 * 8].view(torch.int64)

    def run_gram():
        _lib.call("ivit_gram_i8_i64", _lib.ptr(bank), a.C, a.N, a.C, 0, 0, _lib.ptr(gram), _lib.ptr(ws), need.value, _lib.stream_ptr())

    def run_sums():
        _lib.call("ivit_group_sums_i8_i64", _lib.ptr(bank), a.C, a.N, a.C, _lib.ptr(perm), _lib.ptr(ptr), a.K, 0, _lib.ptr(sums), _lib.stream_ptr())

    run_gram(), run_sums(), csr(labels, a.K), words.sum()            # warm-up of every path at the timed shape
    Gf, Sf = float_gram(bank, chunk), float_sums(bank, labels, a.K, chunk)
    torch.cuda.synchronize()
    assert torch.equal(gram, gram.T) and int(gram.diagonal().min()) > 0
    sums_equal = bool((Sf.to(torch.int64) == sums).all())             # exact in float32 while |sum| < 2^24
    gram_dev = float((Gf.double() - gram.double()).abs().max())

    t = {k: [] for k in ("gram", "sums", "csr", "float_gram", "float_sums", "read")}
    for _ in range(a.repeats):
        t["gram"].append(timed(run_gram)[0])
        t["float_gram"].append(timed(lambda: float_gram(bank, chunk))[0])
        t["sums"].append(timed(run_sums)[0])
        t["float_sums"].append(timed(lambda: float_sums(bank, labels, a.K, chunk))[0])
        t["csr"].append(timed(lambda: csr(labels, a.K))[0])
        t["read"].append(timed(lambda: words.sum())[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"N": a.N, "C": a.C, "K": a.K, "float_chunk_rows": chunk, "gram_workspace_bytes": need.value,
           "gram_segments_x_slabs": need.value // (4 * a.C * a.C),
           "ivit_gram_i8_i64": spread(t["gram"]), "ivit_group_sums_i8_i64": spread(t["sums"]), "labels_to_csr_torch": spread(t["csr"]),
           "float_gram_matmul": spread(t["float_gram"]), "float_sums_index_add": spread(t["float_sums"]), "bank_read_int64_sum": spread(t["read"]),
           "gram_speedup_median": med["float_gram"] / med["gram"], "sums_speedup_median": med["float_sums"] / med["sums"],
           "sums_with_csr_speedup_median": med["float_sums"] / (med["sums"] + med["csr"]),
           "gram_share_of_int8_peak": 2.0 * a.N * a.C * a.C / (med["gram"] * 1e-3) / INT8_PEAK,
           "gram_over_bank_read": med["gram"] / med["read"], "bank_read_TB_per_s": a.N * a.C / (med["read"] * 1e-3) / 1e12,
           "float_sums_equal_exact": sums_equal, "float_gram_max_abs_deviation": gram_dev,
           "bank_bytes_int8": a.N * a.C, "bank_bytes_float32": 4 * a.N * a.C}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
