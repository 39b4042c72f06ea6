"""Module-path forward of frozen Swin models: the integer-carrying path (quantization_utils/lazy.py) with the row kernel on and off,
the float module path (lazy.ENABLED = False) and the fused engine.  Device events, profiler off, median of seven windows after warm-up:

    python scripts/time_swin_module_path.py                       # Swin-T 224 px b128, Swin-B widths 384 px / 12 b64 -> one JSON line each

Kernel times of the row gather against the torch roll / copy kernels it replaces (Swin-T, four forwards):

    rocprofv3 --kernel-trace --stats -d prof_on  -o run -- python scripts/time_swin_module_path.py profile on
    rocprofv3 --kernel-trace --stats -d prof_off -o run -- python scripts/time_swin_module_path.py profile off

Numbers: DESIGN.md section 5 ("Swin module path"), profiles/r05a_*."""
import json
import os
import sys
import warnings
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402

DEV = "cuda:0"
MODELS = {"swin_t_224_b128": (dict(img=224, ws=7, embed=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24)), 128),
          "swin_b_384_b64": (dict(img=384, ws=12, embed=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32)), 64)}


def build(img, ws, embed, depths, heads, seed=3):
    torch.manual_seed(seed)
    m = ivit.SwinTransformer(img_size=img, patch_size=4, window_size=ws, embed_dim=embed, depths=depths, num_heads=heads,
                             num_classes=1000, norm_layer=partial(qu.IntLayerNorm, eps=1e-6)).to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        c = torch.randn(2, 3, img, img, generator=g).to(DEV)
        m(c)
        m(c.flip(0) * 0.7)
    ivit.freeze_model(m)
    return m, g


def timed(fn, reps, windows=7):
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3))


def main():
    warnings.simplefilter("ignore")
    if sys.argv[1:2] == ["profile"]:
        lazy.ROW_KERNEL = sys.argv[2:3] != ["off"]
        cfg, B = MODELS["swin_t_224_b128"]
        m, g = build(**cfg)
        m.use_engine = False
        x = torch.randn(B, 3, cfg["img"], cfg["img"], generator=g).to(DEV)
        with torch.no_grad():
            for _ in range(4):
                m(x)
        torch.cuda.synchronize()
        return
    for name, (cfg, B) in MODELS.items():
        m, g = build(**cfg)
        x = torch.randn(B, 3, cfg["img"], cfg["img"], generator=g).to(DEV)
        res = dict(model=name, batch=B)
        with torch.no_grad():
            ye = m(x)
            m(x)
            res["engine"] = timed(lambda: m(x), 3)
            m.use_engine = False
            yl = m(x)
            m(x)
            res["equal_engine"] = bool(torch.equal(ye, yl))
            res["lazy_row_kernel"] = timed(lambda: m(x), 3)
            lazy.ROW_KERNEL = False
            m(x)
            m(x)
            res["lazy_torch_rows"] = timed(lambda: m(x), 3)
            lazy.ROW_KERNEL = True
            res["lazy_row_kernel_again"] = timed(lambda: m(x), 3)
            lazy.ENABLED = False
            res["equal_ordinary"] = bool(torch.equal(m(x), yl))
            res["ordinary_module_path"] = timed(lambda: m(x), 1, windows=3)
            lazy.ENABLED = True
        print(json.dumps(res), flush=True)
        del m, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
