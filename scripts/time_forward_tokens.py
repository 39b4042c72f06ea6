"""What token features cost, with the fixture ranges of bench.py, one process, device-event times (median of the timed calls):

    python scripts/time_forward_tokens.py events [--natural] [--out FILE]     # one JSON line per case
      deit_base at batch 256, blocks (2, 5, 8, 11), NLC and NCHW; swin_tiny at batch 128 (the last stage), NLC and NCHW:
        forward_ms     (a) the plain eager engine forward
        tokens_ms      (b) engine.forward_tokens (prefix=False)
        composed_ms    (c) what the engines allowed before: forward_intermediates(integers=True), then per map torch's widening and
                           permute back to token rows, then ivit_layernorm_i32_f32 (and, for NCHW, torch's permute of the result)
        hooks_ms       (d) the model with forward hooks on the module path (use_engine = False), at hook_batch images
        per map: the float-emitting LayerNorm launch alone (kernel_us) and the bytes it reads and writes over that time
        equal          (b), (c) and (d) agree bit for bit on the images all three saw
    python scripts/time_forward_tokens.py kernels [--natural]                  # the calls alone, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_forward_tokens.py kernels"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.engine_common import layernorm_f32  # noqa: E402

from time_forward_intermediates import DEV, event_ms, load, timed  # noqa: E402

CASES = {"deit_base": dict(batch=256, hook_batch=32, indices=(2, 5, 8, 11)), "swin_tiny": dict(batch=128, hook_batch=32, indices=None)}


def differ(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


def composed(eng, images, idx, fmt, swin):
    """the composition the engines allowed before this kernel family: integer maps, torch widening, the module-level entry"""
    st = _lib.stream_ptr()
    if swin:
        li = len(eng.stages) - 1
        maps, _ = eng.forward_intermediates(images, (li,), integers=True)
        todo = {None: (maps[li], eng.ln_f)}
    else:
        maps, _ = eng.forward_intermediates(images, idx, integers=True)
        todo = {i: (maps[i], eng._ln_tokens(i)) for i in idx}
    out = {}
    for i, (m, ln) in todo.items():
        B, C = m.shape[:2]
        rows = m.reshape(B, C, -1).permute(0, 2, 1).to(torch.int32).contiguous()      # [B, T, C] widened
        y = torch.empty(rows.shape, dtype=torch.float32, device=rows.device)
        _lib.call("ivit_layernorm_i32_f32", _lib.ptr(rows), C, B * rows.shape[1], C, _lib.ptr(ln["bias"]), _lib.ptr(ln["s"]), _lib.ptr(y), C, st)
        out[i] = y if fmt == "NLC" else y.permute(0, 2, 1).reshape(m.shape).contiguous()
    return out


def kernel_alone(eng, ln, x, B, T_all, t0, C, fmt, ref):
    out = torch.empty_like(ref)
    T = T_all - t0
    st = _lib.stream_ptr()
    launch = lambda: layernorm_f32(ln, x, C, B, T_all, t0, T, C, out, C if fmt == "NLC" else T, st, fmt=fmt)      # noqa: E731
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    us = statistics.median(event_ms(launch) for _ in range(20)) * 1e3
    assert differ(out, ref) == 0
    moved = B * T * C * (x.element_size() + 4)
    return dict(shape=list(ref.shape), kernel_us=round(us, 1), GBps=round(moved / us * 1e-3, 1))


def case(tag, spec, mode):
    model = load(tag)
    B, HB, idx = spec["batch"], spec["hook_batch"], spec["indices"]
    images = torch.from_numpy(synth.make_images(B, 5000)).to(DEV)
    assert model.takes_engine(images), model.engine_unsupported_reason()
    eng = model.engine(B)
    swin = hasattr(eng, "stages")
    run = (lambda fmt: {None: eng.forward_tokens(images, fmt)[0]}) if swin else (lambda fmt: eng.forward_tokens(images, idx, fmt, prefix=False)[0])
    if mode == "kernels":
        for _ in range(5):
            run("NLC")
            run("NCHW")
        torch.cuda.synchronize()
        return None
    out = dict(model=tag, batch=B, hook_batch=HB, indices=None if swin else list(idx))
    out["forward_ms"] = timed(lambda: eng.forward(images), 5, 20)
    small = images[:HB].contiguous()
    for fmt in ("NLC", "NCHW"):
        r = out[fmt] = {}
        r["tokens_ms"] = timed(lambda: run(fmt), 5, 20)
        r["composed_ms"] = timed(lambda: composed(eng, images, idx, fmt, swin), 2, 10)
        model.use_engine = False
        hooked = (lambda: {None: model.forward_tokens(small, fmt=fmt)[0]}) if swin else (lambda: model.forward_tokens(small, idx, fmt, prefix=False)[0])
        r["hooks_ms"] = timed(hooked, 1, 3)
        mh = hooked()
        model.use_engine = True
        mine, mc = run(fmt), composed(eng, images, idx, fmt, swin)
        r["equal"] = dict(composed_differ={str(i): differ(mc[i], mine[i]) for i in mine}, hooks_differ={str(i): differ(mh[i], mine[i][:HB]) for i in mine})
        a = out["forward_ms"]["median"]
        r["added_ms"] = dict(tokens=round(r["tokens_ms"]["median"] - a, 3), composed=round(r["composed_ms"]["median"] - a, 3))
        r["per_image_us"] = dict(tokens=round(r["tokens_ms"]["median"] / B * 1e3, 1), hooks=round(r["hooks_ms"]["median"] / HB * 1e3, 1))
        # the launch alone, on the stream the last forward left behind its last block / stage
        if swin:
            eng.forward(images)
            x, ln, T_all, t0, C = eng.ws["x"], eng.ln_f, eng.T_last, 0, eng.C_last
        else:
            eng.forward(images)
            x = eng.ws["x16"] if eng.stream_bits == 16 else eng.ws["x"]
            ln, T_all, t0, C = eng._ln_tokens(eng.D - 1), eng.T, 1, eng.C
        ref = torch.empty((B, T_all - t0, C) if fmt == "NLC" else (B, C, T_all - t0), dtype=torch.float32, device=DEV)
        layernorm_f32(ln, x, C, B, T_all, t0, T_all - t0, C, ref, C if fmt == "NLC" else T_all - t0, _lib.stream_ptr(), fmt=fmt)
        r["kernel"] = kernel_alone(eng, ln, x, B, T_all, t0, C, fmt, ref)
    out["forward_again_ms"] = timed(lambda: eng.forward(images), 2, 20)       # the spread of (a) within the run
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
