"""The h x w patchify entries against the square ones, device-event times in one process:

    python scripts/time_patchify_hw.py [--out FILE]          # one JSON line

batch 256, 3 channels, patch 16, lda = 768.  Per pixel type four launches of the same pixel count: the square entry at 224 x 224
(ivit_quantize_patchify_f32_i8 / ivit_quantize_patchify_u8_i8, whose kernels this change does not touch), the h x w entry at
224 x 224 and at 112 x 448, and the square entry once more (its own repeatability).  One repetition is the event time around 50
back-to-back launches divided by 50; five repetitions per launch kind, the kinds taking turns inside each repetition.  `spread_us` is
max - min of the square entry's five; `criterion` says whether each h x w median is within that spread of the square median."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ivit_amd import _lib  # noqa: E402

DEV = "cuda:0"
B, C, P, REPS, LAUNCHES = 256, 3, 16, 5, 50


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    p, st = _lib.ptr, _lib.stream_ptr()
    g = torch.Generator(device="cpu").manual_seed(1)
    imgf = torch.randn(B * C * 224 * 224, generator=g).to(DEV)
    imgu = torch.randint(0, 256, (B * C * 224 * 224,), generator=g, dtype=torch.uint8).to(DEV)
    lut = torch.from_numpy(np.random.default_rng(2).integers(-128, 128, size=(C, 256)).astype(np.int8)).to(DEV)
    K = C * P * P
    out = {k: torch.empty(B * 196, K, dtype=torch.int8, device=DEV) for k in ("square", "hw_224x224", "hw_112x448", "square_again")}
    inv = 1.0 / 0.0371
    kinds = {
        "f32": {"square": lambda: _lib.call("ivit_quantize_patchify_f32_i8", p(imgf), p(out["square"]), B, C, 224, P, inv, st),
                "hw_224x224": lambda: _lib.call("ivit_quantize_patchify_hw_f32_i8", p(imgf), p(out["hw_224x224"]), K, B, C, 224, 224, P, inv, st),
                "hw_112x448": lambda: _lib.call("ivit_quantize_patchify_hw_f32_i8", p(imgf), p(out["hw_112x448"]), K, B, C, 112, 448, P, inv, st),
                "square_again": lambda: _lib.call("ivit_quantize_patchify_f32_i8", p(imgf), p(out["square_again"]), B, C, 224, P, inv, st)},
        "u8": {"square": lambda: _lib.call("ivit_quantize_patchify_u8_i8", p(imgu), p(out["square"]), K, B, C, 224, P, p(lut), st),
               "hw_224x224": lambda: _lib.call("ivit_quantize_patchify_hw_u8_i8", p(imgu), p(out["hw_224x224"]), K, B, C, 224, 224, P, p(lut), st),
               "hw_112x448": lambda: _lib.call("ivit_quantize_patchify_hw_u8_i8", p(imgu), p(out["hw_112x448"]), K, B, C, 112, 448, P, p(lut), st),
               "square_again": lambda: _lib.call("ivit_quantize_patchify_u8_i8", p(imgu), p(out["square_again"]), K, B, C, 224, P, p(lut), st)},
    }
    res = dict(batch=B, chans=C, patch=P, launches_per_repetition=LAUNCHES, repetitions=REPS)
    for pix, launches in kinds.items():
        for fn in launches.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(out["square"], out["hw_224x224"]) and torch.equal(out["square"], out["square_again"])
        us = {k: [] for k in launches}
        for _ in range(REPS):
            for k, fn in launches.items():
                us[k].append(event_ms(lambda: [fn() for _ in range(LAUNCHES)]) / LAUNCHES * 1e3)
        sq = us["square"]
        spread = max(sq) - min(sq)
        r = {k: dict(us=[round(v, 2) for v in vals], median_us=round(statistics.median(vals), 2)) for k, vals in us.items()}
        r["spread_us"] = round(spread, 2)
        r["criterion"] = {k: bool(statistics.median(us[k]) - statistics.median(sq) <= spread) for k in ("hw_224x224", "hw_112x448")}
        res[pix] = r
    print(json.dumps(res), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
