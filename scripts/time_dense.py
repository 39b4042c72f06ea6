"""DenseProbe.segment(conf=...) against the torch route (float logits, permute, F.interpolate, argmax, bincount) on the same tokens at
14 x 14 patches, r = 16, K = 150, C = 768, batch 64: device-scope events around back-to-back calls, the paths taking turns, five
repeats each; the torch route's peak allocation and the share of pixels its float32 labels differ on.  python scripts/time_dense.py [out.json]"""
import json, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ivit_amd import _lib, hiptime
from ivit_amd.dense import DenseProbe
from ivit_amd.probe import LinearProbe

DEV = "cuda:0"
B, G, R, K, C = 64, 14, 16, 150, 768
rng = np.random.default_rng(0)
scale = 0.05
W = (rng.normal(0, 0.02, size=(K, C)) / scale).astype(np.float32)
b = rng.normal(0, 0.5, size=K).astype(np.float32)
probe = LinearProbe(W, b, scale, DEV)
dp = DenseProbe(probe)
tok = torch.from_numpy(np.clip(np.rint(rng.normal(0, 40, size=(B * G * G, C))), -128, 127).astype(np.int8)).to(DEV)
target = torch.from_numpy(rng.integers(0, K, size=(B, G * R, G * R)).astype(np.uint8)).to(DEV)
conf = torch.zeros(K, K, dtype=torch.int64, device=DEV)
s_acc = probe.s_acc[:K]

def ours():
    return dp.segment(tok, (G, G), R, target=target, conf=conf)

def torch_route():
    acc = probe._acc(tok, "m")
    logits = acc[:, :K].float() * s_acc
    up = torch.nn.functional.interpolate(logits.view(B, G, G, K).permute(0, 3, 1, 2), scale_factor=R, mode="bilinear", align_corners=False)
    lab = up.argmax(1)
    cm = torch.bincount(target.reshape(-1).long() * K + lab.reshape(-1), minlength=K * K).view(K, K)
    return lab, cm

def timed(fn, n):
    st = _lib.stream_ptr()
    e0, e1 = hiptime.Event(), hiptime.Event()
    e0.record(st)
    for _ in range(n):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_ms(e1) / n

for _ in range(3):
    ours(); torch_route()
torch.cuda.synchronize()
res = {"ours_ms": [], "torch_ms": [], "argmax_only_ms": []}
acc = probe._acc(tok, "m")
out = torch.empty(B, G * R, G * R, dtype=torch.uint8, device=DEV)
def kernel_only():
    _lib.call("ivit_dense_argmax_u8", _lib.ptr(acc), _lib.ptr(probe.s_acc), B, G, G, probe.Np, K, R, _lib.ptr(out), _lib.ptr(target), 255, _lib.ptr(conf), _lib.stream_ptr())
for rep in range(5):
    res["ours_ms"].append(timed(ours, 20))
    res["torch_ms"].append(timed(torch_route, 5))
    res["argmax_only_ms"].append(timed(kernel_only, 20))
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
lab_t, cm = torch_route()
torch.cuda.synchronize()
res["torch_peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
lab_o = ours()
torch.cuda.synchronize()
res["ours_peak_bytes_above_inputs"] = torch.cuda.max_memory_allocated() - base
res["disagree_share"] = float((lab_t.to(torch.uint8) != lab_o).float().mean())
res["pixels"] = B * G * R * G * R
conf.zero_(); ours(); torch.cuda.synchronize()
res["conf_equal_torch_where_labels_equal"] = bool(res["disagree_share"] > 0 or torch.equal(conf, cm))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
print(json.dumps(res))
