"""Frozen models called module by module with I-BERT operators: the integer-carrying path (quantization_utils/lazy.py) against the
literal module path (lazy.ENABLED = False).  Device events, profiler off, median of seven windows after warm-up:

    python scripts/time_ibert_module_paths.py            # Swin-T b128 all 'ibert'; DeiT-B b256 with gelu_type='ibert' -> one JSON line each

The window-attention kernels alone, I-BERT softmax against Shiftmax at the same shapes (49 tokens: Swin-T stage 0 at batch 128; 144
tokens: Swin-B at 384 px stage 0 at batch 64), 20 launches each, for a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats -d prof -o run -- python scripts/time_ibert_module_paths.py kernels

Numbers: DESIGN.md section 5 ("I-BERT operators on the module path")."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402
from ivit_amd.swin_engine import (shift_mask_regions, window_attention, window_attention_ibert, window_attention_ibert_spec,  # noqa: E402
                                  window_attention_spec)

DEV = "cuda:0"
f32 = np.float32


def calibrate(m, img, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        c = torch.randn(2, 3, img, img, generator=g).to(DEV)
        m(c)
        m(c.flip(0) * 0.7)
    ivit.freeze_model(m)
    return g


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


def both_paths(name, m, x):
    res = dict(model=name, batch=x.shape[0], engine=m.engine_unsupported_reason())
    launched, real_call = [], _lib.call
    with torch.no_grad():
        m.use_engine = False
        m(x)
        try:
            _lib.call = lambda n, *a: (launched.append(n), real_call(n, *a))[1]
            lazy.STATS.update(fused=0, materialised=0)
            yl = m(x)
        finally:
            _lib.call = real_call
        res["stats"] = dict(lazy.STATS)
        res["attention_launches"] = {n: launched.count(n) for n in sorted(set(launched)) if "attention" in n}
        res["lazy"] = timed(lambda: m(x), 3)
        lazy.ENABLED = False
        res["equal"] = bool(torch.equal(m(x), yl))
        res["literal"] = timed(lambda: m(x), 1, windows=3)
        lazy.ENABLED = True
    print(json.dumps(res), flush=True)


def kernels():
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    st = _lib.stream_ptr()
    rng = np.random.default_rng(0)
    s_S, s_at, s_A, s_tab, s_pv, s_a3 = f32(2.0 ** -12), f32(2.0 ** -3), f32(2.0 ** -3), f32(2.0 ** -5), f32(2.0 ** -11), f32(2.0 ** -5)
    for N, ws, nH, B in ((49, 7, 3, 128), (144, 12, 4, 64)):
        nW, side = 64, 8 * ws
        nwin = nW * B
        bias = rng.integers(-40, 41, size=(nH, N, N)).astype(np.int32)
        region = shift_mask_regions(side, side, ws, ws // 2).astype(np.uint8)
        qkv = torch.randint(-128, 128, (3, nwin, nH, N, 32), dtype=torch.int8, device=DEV)
        out = torch.empty(nwin * N, nH * 32, dtype=torch.int8, device=DEV)
        a_sm, _ = window_attention_spec(up, bias, s_tab, s_S, s_at, s_A, s_pv, s_a3, region, N)
        a_ib = window_attention_ibert_spec(up, DEV, st, bias, s_tab, s_S, s_at, s_A, s_pv, s_a3, region, N, (0.0, 32767 * 2.0 ** 23))
        for _ in range(20):
            window_attention(a_sm, qkv, out, nH * 32, nwin, nW, nH, N, side, side, ws, ws // 2, False, st)
            window_attention_ibert(a_ib, qkv, out, nH * 32, nwin, nW, nH, N, side, side, ws, ws // 2, False, st)
        torch.cuda.synchronize()
        print(json.dumps(dict(tokens=N, windows=nwin, heads=nH, ibert_band_w=a_ib["band_w"])), flush=True)


def main():
    warnings.simplefilter("ignore")
    if sys.argv[1:2] == ["kernels"]:
        return kernels()
    ib = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
    torch.manual_seed(3)
    m = ivit.SwinTransformer(img_size=224, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                             num_classes=1000, **ib).to(DEV).eval()
    g = calibrate(m, 224, 3)
    both_paths("swin_t_224_ibert", m, torch.randn(128, 3, 224, 224, generator=g).to(DEV))
    del m
    torch.cuda.empty_cache()
    torch.manual_seed(4)
    m = ivit.deit_base_patch16_224(gelu_type="ibert", softmax_type="ivit", layernorm_type="ivit").to(DEV).eval()
    g = calibrate(m, 224, 4)
    both_paths("deit_b_gelu_ibert", m, torch.randn(256, 3, 224, 224, generator=g).to(DEV))


if __name__ == "__main__":
    main()
