"""What attention maps cost, DeiT-B with the fixture ranges of bench.py (power-of-two; --natural: as calibrated), batch 256, one process:

    python scripts/time_attention_maps.py events [--natural]     # one JSON line: device-event times, median of the timed calls
        forward_ms        the plain eager IntViTEngine.forward
        maps_cls_all_ms   attention_maps(rows="cls") over all 12 layers  (forward + 12 launches of the probability kernel)
        maps_all_l11_ms   attention_maps(rows="all", layers=[11])        (forward + one launch that writes 119 MB)
        hook_b32_ms       the hook form of the same model (use_engine = False) at batch 32, rows="cls", all layers
    python scripts/time_attention_maps.py kernels [--natural]    # the calls alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_attention_maps.py kernels

The model is the fixture's float state and ranges loaded into vit_quant.VisionTransformer and frozen; its engine is the one bench.py
builds from the same two."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

DEV = "cuda:0"
BATCH, HOOK_BATCH = 256, 32


def timed(fn, warmup, n):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3), n=n)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "events"
    tag = "deit_base" + ("_natural" if "--natural" in sys.argv else "")
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    model = ivit.deit_base_patch16_224()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct):
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    images = torch.from_numpy(synth.make_images(BATCH, 5000)).to(DEV)
    assert model.takes_engine(images), model.engine_unsupported_reason()
    eng = model.engine(BATCH)
    with torch.no_grad():
        if mode == "kernels":
            for _ in range(5):
                eng.attention_maps(images, rows="cls")
                eng.attention_maps(images, rows="all", layers=[11])
            torch.cuda.synchronize()
            return
        out = dict(model=tag, batch=BATCH, hook_batch=HOOK_BATCH)
        out["forward_ms"] = timed(lambda: eng.forward(images), 5, 20)
        out["maps_cls_all_ms"] = timed(lambda: eng.attention_maps(images, rows="cls"), 5, 20)
        out["maps_all_l11_ms"] = timed(lambda: eng.attention_maps(images, rows="all", layers=[11]), 5, 20)
        model.use_engine = False
        small = images[:HOOK_BATCH].contiguous()
        out["hook_b32_ms"] = timed(lambda: model.attention_maps(small, rows="cls"), 1, 3)
        model.use_engine = True
        # the two forms agree on the images both saw
        a, _ = model.attention_maps(small, rows="cls")
        model.use_engine = False
        b, _ = model.attention_maps(small, rows="cls")
        out["hook_equals_engine"] = all(torch.equal(a[i], b[i]) for i in a)
        out["per_image_us"] = dict(maps_cls_all=round(out["maps_cls_all_ms"]["median"] / BATCH * 1e3, 1),
                                   hook=round(out["hook_b32_ms"]["median"] / HOOK_BATCH * 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
