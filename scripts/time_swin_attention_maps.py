"""What Swin attention maps cost: Swin-T with the I-ViT operators and the fixture ranges of tests/golden/swin_tiny.npz (power-of-two;
--natural: as calibrated), batch 128, one process:

    python scripts/time_swin_attention_maps.py events [--natural]     # one JSON line: device-event times, median of the timed calls
        forward_ms          the plain eager IntSwinEngine.forward
        maps_all_ms         attention_maps() over all 12 blocks   (forward + 12 launches of the window probability kernel, ~280 MB of maps)
        maps_last_ms        attention_maps(blocks=[(3, 1)])       (forward + one launch)
        module_forward_ms   model(x) with use_engine = False: the module-by-module forward the hooks used to ride on
        hook_maps_ms        model.attention_maps(x) with use_engine = False (forward hooks on every attn.log_int_softmax)
    python scripts/time_swin_attention_maps.py kernels [--natural]    # the engine calls alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_swin_attention_maps.py kernels

The model is the fixture's float state and ranges loaded into swin_quant.SwinTransformer and frozen; its engine is the one the
fixture tests build from the same two."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import synth  # noqa: E402
from ivit_amd.checkpoint import load_fixture  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

DEV = "cuda:0"
BATCH = 128


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
    tag = "swin_tiny" + ("_natural" if "--natural" in sys.argv else "")
    _, meta, ranges = load_fixture(tag)
    fs = synth.make_swin_float_state(meta["factory"], meta["weight_seed"])
    model = ivit.swin_tiny_patch4_window7_224()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    images = torch.from_numpy(synth.make_images(BATCH, 5000)).to(DEV)
    assert model.takes_engine(images), model.engine_unsupported_reason()
    eng = model.engine(BATCH)
    last = (len(model.depths) - 1, model.depths[-1] - 1)
    with torch.no_grad():
        if mode == "kernels":
            for _ in range(5):
                eng.attention_maps(images)
                eng.attention_maps(images, blocks=[last])
            torch.cuda.synchronize()
            return
        out = dict(model=tag, batch=BATCH, forms=list(eng.window_softmax_forms))
        out["forward_ms"] = timed(lambda: eng.forward(images), 5, 20)
        out["maps_all_ms"] = timed(lambda: eng.attention_maps(images), 5, 20)
        out["maps_last_ms"] = timed(lambda: eng.attention_maps(images, blocks=[last]), 5, 20)
        maps, _ = eng.attention_maps(images)
        out["maps_bytes"] = int(sum(m.numel() for m in maps.values()))
        small = images[:8].contiguous()
        a, _ = model.attention_maps(small)
        del maps
        model.use_engine = False
        out["module_forward_ms"] = timed(lambda: model(images), 1, 5)
        out["hook_maps_ms"] = timed(lambda: model.attention_maps(images), 1, 3)
        b, _ = model.attention_maps(small)      # the two forms agree on the images both saw
        model.use_engine = True
        out["hook_equals_engine"] = all(torch.equal(a[k], b[k]) for k in a)
        out["maps_all_below_module_forward"] = out["maps_all_ms"]["median"] < out["module_forward_ms"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
