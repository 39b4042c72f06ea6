"""DeiT-B at batch 256 with every width knob at 4 (`--bitwidth 4`), three ways -- the literal module path (lazy.ENABLED = False),
the integer-carrying module path (quantization_utils/lazy.py) and the fused engine (IntViTEngine(stream_bits=4)) -- and the 8-bit
engine in the same session.  Device events, profiler off, median of seven windows after warm-up (three for the literal path):

    python scripts/time_w4_paths.py [out.json]           # default profiles/w4_timing.json; one JSON object

The expectation under test: a narrow form costs what its 8-bit twin costs (only constants differ), i.e. engine_w4 / engine_w8
is about 1.  For a kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats -d prof -o run -- python scripts/time_w4_paths.py /dev/null

Numbers: DESIGN.md section 5 ("4-bit width entries")."""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402

DEV = "cuda:0"
BATCH = 256
KNOBS = ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw", "norm2_in_bw",
         "att_block_out_bw")


def calibrated(bits, seed=4):
    """DeiT-B, weights x 3, q / k x 4 and a class token the 4-bit step can see (as the 4-bit fixtures), calibrated on two batches"""
    torch.manual_seed(seed)
    m = ivit.deit_base_patch16_224(**{k: bits for k in KNOBS}).to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        m.cls_token.normal_(0.0, 2.0)
        m.pos_embed.normal_(0.0, 0.7)
        for blk in m.blocks:
            blk.attn.qkv.weight.mul_(16.0)
        c = torch.randn(2, 3, 224, 224, generator=g).to(DEV)
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


def engine_time(m, x):
    assert m.engine_unsupported_reason() is None and m.takes_engine(x), m.engine_unsupported_reason()
    eng = m.engine(x.shape[0])
    for _ in range(3):
        eng.forward_graph(x, resident=True)
    # the graph replay (the 8-bit engine's prunes its last block to the class rows, the 4-bit one has no such tail), and the full
    # forward launched eagerly: the like-for-like comparison of the narrow kernels with their 8-bit twins
    return eng, timed(lambda: eng.forward_graph(x, resident=True), 10), timed(lambda: eng.forward(x), 10)


def main():
    warnings.simplefilter("ignore")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "w4_timing.json")
    res = dict(model="deit_base_patch16_224", batch=BATCH)
    with torch.no_grad():
        m4, g = calibrated(4)
        x = torch.randn(BATCH, 3, 224, 224, generator=g).to(DEV)
        res["engine_widths_w4"] = list(m4._engine_widths) if m4.engine_unsupported_reason() is None else m4.engine_unsupported_reason()
        eng4, res["engine_w4"], res["engine_w4_full_forward"] = engine_time(m4, x)
        y_eng = m4(x)
        m4.use_engine = False
        launched, real_call = [], _lib.call
        m4(x)
        try:
            _lib.call = lambda n, *a: (launched.append(n), real_call(n, *a))[1]
            lazy.STATS.update(fused=0, materialised=0)
            y_lazy = m4(x)
        finally:
            _lib.call = real_call
        res["carried_stats"] = dict(lazy.STATS)
        res["carried_narrow_launches"] = {n: launched.count(n) for n in sorted(set(launched)) if "_bits" in n or "attention" in n}
        res["carried_w4"] = timed(lambda: m4(x), 3)
        lazy.ENABLED = False
        try:
            y_lit = m4(x)
            res["literal_w4"] = timed(lambda: m4(x), 1, windows=3)
        finally:
            lazy.ENABLED = True
        res["equal"] = dict(engine_vs_carried=bool(torch.equal(y_eng, y_lazy)), carried_vs_literal=bool(torch.equal(y_lazy, y_lit)))
        del m4, eng4
        torch.cuda.empty_cache()
        m8, _ = calibrated(8)
        _, res["engine_w8"], res["engine_w8_full_forward"] = engine_time(m8, x)
    res["ratio_engine_w4_over_w8"] = round(res["engine_w4"]["median_ms"] / res["engine_w8"]["median_ms"], 4)
    res["ratio_full_forward_w4_over_w8"] = round(res["engine_w4_full_forward"]["median_ms"] / res["engine_w8_full_forward"]["median_ms"], 4)
    print(json.dumps(res), flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
