"""What feature maps cost, with the fixture ranges of bench.py, one process, device-event times (median of the timed calls):

    python scripts/time_forward_intermediates.py events [--natural] [--out FILE]     # one JSON line
      per case -- deit_base at batch 256, blocks (2, 5, 8, 11); swin_tiny at batch 128, all four stages, float32 maps:
        forward_ms        (a) the plain eager engine forward
        intermediates_ms  (b) engine.forward_intermediates
        taps_torch_ms     (c) forward(taps=...) and, per map, t[:, t0:].permute(0, 2, 1).float().mul(s).contiguous()
        hooks_ms          (d) the model with forward hooks on the module path (use_engine = False), at hook_batch images
        per map: the kernel alone (kernel_us), the bytes it reads and writes over that time (kernel_GBps), and a device-to-device
        copy of the output's bytes timed in the same run, alternating with it (copy_us, copy_GBps: read + written bytes)
        maps_equal        (b), (c) and (d) agree bit for bit on the images all three saw
    python scripts/time_forward_intermediates.py kernels [--natural]                  # the calls alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_forward_intermediates.py kernels

The models are the fixtures' float state and ranges loaded into the model classes and frozen; their engines are the ones bench.py
builds from the same two."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine_common import tokens_to_nchw  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

DEV = "cuda:0"
CASES = {"deit_base": dict(batch=256, hook_batch=32, indices=(2, 5, 8, 11)), "swin_tiny": dict(batch=128, hook_batch=32, indices=(0, 1, 2, 3))}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, warmup, n):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [event_ms(fn) for _ in range(n)]
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3), n=n)


def load(tag):
    fs, ranges, cfg, meta, _ = load_synthetic_model(tag)
    model = getattr(ivit, meta["factory"])()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    return model


def tap_of(model, eng, taps, i, B):
    """(the [B, T_all, C] integers of map i's tap, t0)"""
    if hasattr(eng, "stages"):
        stg = eng.stages[i]
        return taps[f"layers.{i}.blocks.{model.depths[i] - 1}.qact4"].view(B, stg["H"] * stg["W"], stg["C"]), 0
    return taps[f"blocks.{i}.qact4"], 1


def from_taps(model, eng, images, indices, scales, shapes):
    taps = {}
    eng.forward(images, taps=taps)
    out = {}
    for i in indices:
        t, t0 = tap_of(model, eng, taps, i, images.shape[0])
        out[i] = t[:, t0:].permute(0, 2, 1).float().mul(scales[i]).contiguous().view(shapes[i])
    return out


def kernel_alone(t, t0, scale, ref):
    """the launch of one map by itself on the [B, T_all, C] integers of its tap, alternating with a device-to-device copy of the
    output's bytes"""
    B, T_all, C = t.shape
    out, dst = torch.empty_like(ref), torch.empty_like(ref)
    st = _lib.stream_ptr()
    launch = lambda: tokens_to_nchw(t, C, B, T_all, t0, T_all - t0, C, scale, out, st)      # noqa: E731
    copy = lambda: dst.copy_(ref)      # noqa: E731
    for _ in range(3):
        launch()
        copy()
    torch.cuda.synchronize()
    k, c = [], []
    for _ in range(20):
        k.append(event_ms(launch))
        c.append(event_ms(copy))
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    k_us, c_us = statistics.median(k) * 1e3, statistics.median(c) * 1e3
    moved = B * (T_all - t0) * C * (t.element_size() + 4)
    return dict(shape=list(ref.shape), bytes_read=B * (T_all - t0) * C * t.element_size(), bytes_written=ref.numel() * 4,
                kernel_us=round(k_us, 1), kernel_GBps=round(moved / k_us * 1e-3, 1), copy_us=round(c_us, 1),
                copy_GBps=round(2 * ref.numel() * 4 / c_us * 1e-3, 1))


def case(tag, spec, mode):
    model = load(tag)
    B, HB, idx = spec["batch"], spec["hook_batch"], spec["indices"]
    images = torch.from_numpy(synth.make_images(B, 5000)).to(DEV)
    assert model.takes_engine(images), model.engine_unsupported_reason()
    eng = model.engine(B)
    if mode == "kernels":
        for _ in range(5):
            eng.forward_intermediates(images, idx)
        torch.cuda.synchronize()
        return None
    out = dict(model=tag, batch=B, hook_batch=HB, indices=list(idx))
    out["forward_ms"] = timed(lambda: eng.forward(images), 5, 20)
    out["intermediates_ms"] = timed(lambda: eng.forward_intermediates(images, idx), 5, 20)
    maps, scales = eng.forward_intermediates(images, idx)
    shapes = {i: maps[i].shape for i in idx}
    out["forward_again_ms"] = timed(lambda: eng.forward(images), 2, 20)       # the spread of (a) within the run
    wide = getattr(eng, "stream_bits", 8) == 16
    if not wide:
        out["taps_torch_ms"] = timed(lambda: from_taps(model, eng, images, idx, scales, shapes), 2, 10)
        out["taps_forward_ms"] = timed(lambda: eng.forward(images, taps={}), 2, 10)      # of which the forward that records the taps
        mt = from_taps(model, eng, images, idx, scales, shapes)
    small = images[:HB].contiguous()
    model.use_engine = False
    out["hooks_ms"] = timed(lambda: model.forward_intermediates(small, idx), 1, 3)
    mh, sh = model.forward_intermediates(small, idx)
    model.use_engine = True
    differ = lambda a, b: int((a.view(torch.int32) != b.view(torch.int32)).sum())      # noqa: E731
    out["maps_equal"] = dict(scales=sh == scales, hooks_differ={i: differ(mh[i], maps[i][:HB]) for i in idx},
                             taps_differ=None if wide else {i: differ(mt[i], maps[i]) for i in idx})
    taps = {}
    eng.forward(images, taps=taps)
    streams = {i: tap_of(model, eng, taps, i, B) for i in idx}
    streams = {i: (t.contiguous(), t0) for i, (t, t0) in streams.items()}
    del taps
    out["per_map"] = {str(i): kernel_alone(*streams[i], scales[i], maps[i]) for i in idx}
    a = out["forward_ms"]["median"]
    out["added_ms"] = dict(intermediates=round(out["intermediates_ms"]["median"] - a, 3),
                           taps_torch=None if wide else round(out["taps_torch_ms"]["median"] - a, 3),
                           copies=round(sum(m["copy_us"] for m in out["per_map"].values()) * 1e-3, 3),
                           kernels=round(sum(m["kernel_us"] for m in out["per_map"].values()) * 1e-3, 3))
    out["per_image_us"] = dict(intermediates=round(out["intermediates_ms"]["median"] / B * 1e3, 1),
                               hooks=round(out["hooks_ms"]["median"] / HB * 1e3, 1))
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "events"
    suffix = "_natural" if "--natural" in sys.argv else ""
    res = []
    with torch.no_grad():
        for tag, spec in CASES.items():
            r = case(tag + suffix, spec, mode)
            if r is not None:
                res.append(r)
                print(json.dumps(r), flush=True)
    if "--out" in sys.argv and res:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
