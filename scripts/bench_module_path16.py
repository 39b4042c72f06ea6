"""Module-by-module forward of DeiT-B with every width knob at 16 (what the reference's `--bitwidth 16` sets, vit_quant.py:180-187),
next to the fused engine where the engine takes the geometry.

    bench_module_path16.py --bitwidth 16 [--img 224|384] [batch] [--depth N]

224 px (197 tokens; default batch 256): the engine takes the model, its time is printed beside the module path's.  384 px (577
tokens; default batch 64): the engine declines the 16-bit stream, the module path is all there is.  Every figure is the median of
seven event-timed windows of three forwards after a warm-up forward, with the smallest and largest window; the host time to issue
one forward is printed next to it (a forward whose issue time equals its duration is host-bound, not kernel-bound)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import synth  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402

DEV = "cuda:0"


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


bw, img, depth = opt("--bitwidth", 16), opt("--img", 224), opt("--depth", 12)
skip = {i + 1 for i, a in enumerate(sys.argv) if a.startswith("--")}
pos = [a for i, a in enumerate(sys.argv) if i and i not in skip and a.isdigit()]
B = int(pos[0]) if pos else (256 if img == 224 else 64)
assert bw in (8, 16) and img % 16 == 0
widths = {k: bw for k in ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw",
                          "norm2_in_bw", "att_block_out_bw")}
T = (img // 16) ** 2 + 1
fs = synth.make_float_state("deit_base_patch16_224", 7)
if img != 224:
    fs["pos_embed"] = np.random.default_rng(1).normal(0, 0.02, size=(1, T, 768)).astype(np.float32)
model = ivit.VisionTransformer(img_size=img, patch_size=16, embed_dim=768, depth=depth, num_heads=12, mlp_ratio=4, qkv_bias=True, **widths)
model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
model.to(DEV).eval()
imgs = torch.from_numpy(synth.make_images(16, 99)).to(DEV)
if img != 224:
    imgs = torch.nn.functional.interpolate(imgs, size=(img, img), mode="bilinear", align_corners=False)
imgs = imgs.repeat((B + 15) // 16, 1, 1, 1)[:B].float().contiguous()


def windows(fn, n=3, reps=7):
    """(median, min, max) in ms per forward of `reps` event-timed windows of n forwards; the host's issue time of one forward"""
    with torch.no_grad():
        fn()
        torch.cuda.synchronize()
        out, host = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            host.append((time.perf_counter() - t0) / n * 1e3)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / n)
    out.sort()
    return out[reps // 2], out[0], out[-1], sorted(host)[reps // 2]


with torch.no_grad():
    model(imgs[:8])                   # calibration forward (running min / max)
ivit.freeze_model(model)
reason = model.engine_unsupported_reason()
model.use_engine = False
lazy.STATS.update(fused=0, materialised=0)
med, lo, hi, host = windows(lambda: model(imgs))
print(f"bitwidth {bw} DeiT-B depth {depth} {img} px batch {B} module path: {med:8.2f} ms / forward (min {lo:.2f}, max {hi:.2f}), host issue "
      f"{host:.2f} ms; materialised per forward {lazy.STATS['materialised'] / 22:.1f}", flush=True)
if reason is None:
    model.use_engine = True
    med, lo, hi, host = windows(lambda: model(imgs))
    print(f"bitwidth {bw} DeiT-B depth {depth} {img} px batch {B} engine:      {med:8.2f} ms / forward (min {lo:.2f}, max {hi:.2f})", flush=True)
else:
    print(f"engine not taken: {reason}", flush=True)
