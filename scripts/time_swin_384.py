"""Swin at 384 px with 12 x 12 windows: time per (query, key) score of ivit_window_attention_i8_long (144 tokens) against the 49-token
window attention of 224 px, and Swin-B at 384 px, batch 64: the engine's forward (eager and graph replay) against the module path's.
Torch events time each case here; the numbers to quote come from the kernel trace of one run:

    rocprofv3 --kernel-trace --output-format csv -d prof -o run -- python scripts/time_swin_384.py [kernels] [model]
    python scripts/time_swin_384.py summary prof/<host>/<pid>_kernel_trace.csv   (the path rocprofv3 prints)

`summary` reads the trace and prints, per window-attention kernel form and grid, the dispatch durations and the time per score (the
launches of the `kernels` cases run with B_ = 4096 windows of 4 heads; the model's rows are the natural-scale forms)."""
import csv
import os
import re
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402

DEV = "cuda:0"
hd = 32
rng = np.random.default_rng(0)
st = _lib.stream_ptr
KERNEL_CASES = [(4096, 4, 49), (4096, 4, 144), (4096, 4, 100)]     # (windows, heads, tokens): 64 images x 64 windows (stage 0)


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def window_attention(nwin, H, T):
    """us per launch: power-of-two scales (float32 score requantisation), window order, no shift mask"""
    ws = int(round(T ** 0.5))
    kp = 64 if T <= 64 else (T + 15) // 16 * 16
    qkv = torch.from_numpy(rng.integers(-128, 128, size=(3, nwin, H, T, hd)).astype(np.int8)).to(DEV)
    bias = torch.from_numpy(rng.integers(-60, 61, size=(H, T, kp)).astype(np.int16)).to(DEV)
    out = torch.empty(nwin * T, H * hd, dtype=torch.int8, device=DEV)
    ms, es = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))
    mb, eb = dyadic(np.float32(2.0 ** -2), np.float32(2.0 ** -2))
    mo, eo = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -3))
    a = (_lib.ptr(qkv), _lib.ptr(out), H * hd, _lib.ptr(bias), None, 0, nwin, 1, H, T, hd, int(ms[0]), int(es[0]), int(mb[0]), int(eb[0]),
         0.25, int(mo[0]), int(eo[0]))
    if T <= 64:
        return timeit(lambda: _lib.call("ivit_window_attention_i8", *a, st()))
    return timeit(lambda: _lib.call("ivit_window_attention_i8_long", *a, None, None, None, 0, 0, ws, ws, ws, 0, 0, st()))


def swin_b_384(batch=64):
    """Swin-B widths and depths at 384 px / 12, random weights (scaled as tests/test_gpu_swin_384.py does), ranges calibrated on two
    images (natural scales)"""
    torch.manual_seed(0)
    m = ivit.SwinTransformer(img_size=384, patch_size=4, window_size=12, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32),
                             num_classes=1000, norm_layer=partial(ivit.quantization_utils.IntLayerNorm, eps=1e-6)).to(DEV).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():      # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
            elif name.endswith("relative_position_bias_table"):
                p.mul_(20.0)
        m(torch.randn(2, 3, 384, 384, device=DEV))
    ivit.freeze_model(m)
    assert m.engine_unsupported_reason() is None
    x = torch.randn(batch, 3, 384, 384, device=DEV)
    with torch.no_grad():
        m(x)
        eng = m._engine[2]
        t_eng = timeit(lambda: eng.forward(x), n=10)
        t_graph = timeit(lambda: eng.forward_graph(x), n=10)
        m.use_engine = False
        t_mod = timeit(lambda: m(x), n=2)
        m.use_engine = True
    print(f"Swin-B 384 b{batch}: engine {t_eng / 1e3:.2f} ms, graph replay {t_graph / 1e3:.2f} ms, module path {t_mod / 1e3:.1f} ms")


def summary(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "window_attention" not in name:
                continue
            m = re.search(r"(window_attention\w*)<([^>]*)>", name)
            form = f"{m.group(1)}<{m.group(2)}>" if m else name[:60]
            key = (form, int(r.get("Grid_Size_X", r.get("Grid_Size", 0)) or 0))
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (form, grid), d in sorted(rows.items()):
        d = np.array(d)
        print(f"{form:60s} grid {grid:8d}  n {d.size:4d}  median {np.median(d):9.2f} us  min {d.min():9.2f} us")
    print("time per score = median / (windows * heads * T^2); kernels cases: 4096 windows x 4 heads")


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "model"]
    if what[0] == "summary":
        summary(what[1])
        sys.exit(0)
    if "kernels" in what:
        for nwin, H, T in KERNEL_CASES:
            us = window_attention(nwin, H, T)
            print(f"window attention T={T:3d} windows={nwin} heads={H}: {us:8.1f} us  {us * 1e6 / (nwin * H * T * T):.3f} ps/score")
    if "model" in what:
        swin_b_384()
