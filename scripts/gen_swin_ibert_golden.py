"""Writes tests/golden/swin_ibert_small.npz: the reference's own Swin forward with its I-BERT operators, on the CPU.

The reference's models/swin_quant.py is imported unmodified through the four harness-side shims of oracle/gen_golden.py (reused by
import: the .cuda() stub, the tkinter stub, the Int* aliases, the bias-free QuantLinear weight function); the three operator names
its assembly reads are then bound to its I-BERT classes -- IntLayerNorm = IBERTIntLayerNorm, IntGELU = IBERTIntGELU, IntSoftmax =
partial(IBERTIntSoftmax, 8) -- which is what `layernorm_type = gelu_type = softmax_type = 'ibert'` means for Swin.

Model: synth.SWIN_CONFIGS["swin_ibert_small"] (56 px, 7 x 7 windows, depths (2, 2), heads (3, 6)), weights from
synth.make_swin_float_state(seed), calibrated on one seeded batch, every QuantAct range snapped to the next power of two, frozen.
The fixture holds data only: the 3 seeded images, the ranges and LayerNorm shifts, INT32 logits, top-1 and the CRC32 of every
QuantAct tap.  Run from the repository root:  python scripts/gen_swin_ibert_golden.py"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (shim 1 on import)

TAG, CONFIG, WEIGHT_SEED, CALIB_SEED, IMAGE_SEED, N_IMAGES, IMG = "swin_ibert_small", "swin_ibert_small", 31, 301, 3001, 3, 56


def images(n, seed):
    """smooth blobs plus noise, as the module-path tests draw them"""
    rng = np.random.default_rng(seed)
    low = rng.standard_normal((n, 3, 7, 7)).astype(np.float32).repeat(8, axis=2).repeat(8, axis=3)
    return (low + np.float32(0.3) * rng.standard_normal((n, 3, IMG, IMG)).astype(np.float32)).astype(np.float32)


def main():
    rq, synth = gg.rq, gg.synth
    sq = gg._import_swin()                                                                 # shims 2 and 3
    sq.IntLayerNorm, sq.IntGELU, sq.IntSoftmax = rq.IBERTIntLayerNorm, rq.IBERTIntGELU, partial(rq.IBERTIntSoftmax, 8)
    cfg = synth.SWIN_CONFIGS[CONFIG]
    model = sq.SwinTransformer(img_size=IMG, patch_size=4, window_size=cfg["window"], embed_dim=cfg["embed_dim"], depths=cfg["depths"],
                               num_heads=cfg["num_heads"], num_classes=synth.NUM_CLASSES, norm_layer=partial(sq.IntLayerNorm, eps=1e-6))
    for mod in model.modules():                                                            # shim 4
        if isinstance(mod, rq.QuantLinear) and mod.bias is None:
            mod.weight_function = lambda x, *a: None if x is None else gg.SymmetricQuantFunction.apply(x, *a)
    fs = synth.make_swin_float_state(CONFIG, WEIGHT_SEED)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected, unexpected
    model.eval()
    model(torch.from_numpy(images(2, CALIB_SEED)))
    ranges = {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct):
            mx = float(torch.max(-mod.x_min, mod.x_max))
            if mx == 0.0:
                continue                                   # act_out: never called
            q = 2 ** (mod.activation_bit - 1) - 1
            p = int(np.ceil(np.log2(mx / q)))
            mod.x_max.fill_(q * 2.0 ** p)
            mod.x_min.fill_(-q * 2.0 ** p)
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
    shifts = {n: np.float32(m.shift.item()) for n, m in model.named_modules() if isinstance(m, rq.IBERTIntLayerNorm)}
    gg.ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            taps[name] = gg.to_int(y, s)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct) and name != "act_out" and not name.endswith("log_int_softmax.act"):
            mod.register_forward_hook(hook(name))
    imgs = images(N_IMAGES, IMAGE_SEED)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact3.act_scaling_factor).float()
    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=TAG, config=CONFIG, weight_seed=WEIGHT_SEED, calib_seed=CALIB_SEED, image_seed=IMAGE_SEED,
                                         n_images=N_IMAGES, img_size=IMG, operators="ibert", regime="pow2", torch=torch.__version__))),
        "images": imgs,
        "range_names": np.array(list(ranges)), "ranges": np.array(list(ranges.values()), np.float32),
        "shift_names": np.array(list(shifts)), "shifts": np.array(list(shifts.values()), np.float32),
        "logits_int32": torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64), "head_scale": s_head.numpy().astype(np.float32),
        "tap_names": np.array(names), "tap_crc32": np.array([gg.crc(taps[n]) for n in names], np.uint32),
        "tap_absmax": np.array([int(np.abs(taps[n]).max()) for n in names], np.int64),
    }
    path = os.path.join(gg.GOLD, f"{TAG}.npz")
    np.savez_compressed(path, **out)
    print(f"[{TAG}] {len(names)} taps, top1 = {out['top1'].tolist()}, shifts {sorted(set(float(v) for v in shifts.values()))}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
