"""Writes tests/golden/{deit_rect, deit_rect_ibert, swin_rect, swin_rect_tall}{, _natural}.npz: the reference's own forward on images
that are not square, on the CPU.

The reference takes img_size as an int or a pair (height, width) everywhere (layers_quant.py:168-175, vit_quant.py:204-214,
swin_quant.py:200-203, 462-488).  Its models are imported unmodified through the harness-side shims of oracle/gen_golden.py (reused
by import, as scripts/gen_swin_ibert_golden.py does); nothing of it is copied and oracle/ is untouched.

  deit_rect         DeiT-like, (64, 96) / 16: 4 x 6 patches + cls = 25 tokens, embed 128, depth 2, 2 heads, I-ViT operators
  deit_rect_ibert   DeiT-like, (192, 256) / 16: 193 tokens (the fused I-BERT attention's lower bound), depth 1, I-BERT operators
  swin_rect         Swin, (56, 112), window 7, embed 64, depths (2, 2), heads (2, 4): stage 0 shifted on a 14 x 28 map, stage 1 a
                    7 x 14 map in two unshifted windows
  swin_rect_tall    Swin, (96, 32), window 8, the same widths: stage 0 a 24 x 8 map in three windows, stage 1 a 12 x 4 map in 4 x 4
                    windows (min(H, W) of swin_quant.py:200-203)

Weights: synth.make_float_state_dims / make_swin_float_state_dims (seeded draws).  Each model is written twice: calibrated on one
seeded batch with every QuantAct range snapped to the next power of two (`<tag>`), and calibrated on two batches with the ranges as
they come out (`<tag>_natural`).  A fixture holds data only: the meta record (both image sizes, the dimensions, the seeds the
images are redrawn from with synth.make_images), the ranges, the I-BERT LayerNorm shifts, INT32 logits, top-1, the head scale and
the CRC32 of every QuantAct tap.  Run from the repository root:  python scripts/gen_rect_golden.py [tag ...]"""
import json
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (shim 1 on import)

WIDTHS = dict(embed_dim=64, depths=(2, 2), num_heads=(2, 4))
PLAN = {
    # tag: kind, dimensions, operators, weight seed, calibration seeds (pow2 uses the first), calibration batch, image seed, images
    "deit_rect": ("vit", dict(img_size=(64, 96), patch=16, embed_dim=128, depth=2, num_heads=2), "ivit", 41, (401, 411), 4, 4001, 3),
    "deit_rect_ibert": ("vit", dict(img_size=(192, 256), patch=16, embed_dim=128, depth=1, num_heads=2), "ibert", 42, (402, 412), 2,
                        4002, 2),
    "swin_rect": ("swin", dict(img_size=(56, 112), window=7, **WIDTHS), "ivit", 43, (403, 413), 4, 4003, 3),
    "swin_rect_tall": ("swin", dict(img_size=(96, 32), window=8, **WIDTHS), "ivit", 44, (404, 414), 4, 4004, 3),
}


def build(kind, dims, ops):
    rq, synth = gg.rq, gg.synth
    if kind == "vit":
        return gg.ref_models.vit_quant.VisionTransformer(
            img_size=dims["img_size"], patch_size=dims["patch"], embed_dim=dims["embed_dim"], depth=dims["depth"],
            num_heads=dims["num_heads"], mlp_ratio=4, qkv_bias=True, num_classes=synth.NUM_CLASSES, gelu_type=ops, softmax_type=ops,
            layernorm_type=ops)
    sq = gg._import_swin()                                                                 # shims 2 and 3 (I-ViT operators)
    model = sq.SwinTransformer(img_size=dims["img_size"], patch_size=4, window_size=dims["window"], embed_dim=dims["embed_dim"],
                               depths=dims["depths"], num_heads=dims["num_heads"], num_classes=synth.NUM_CLASSES,
                               norm_layer=partial(sq.IntLayerNorm, eps=1e-6))
    for mod in model.modules():                                                            # shim 4
        if isinstance(mod, rq.QuantLinear) and mod.bias is None:
            mod.weight_function = lambda x, *a: None if x is None else gg.SymmetricQuantFunction.apply(x, *a)
    return model


def float_state(kind, dims, seed):
    synth = gg.synth
    if kind == "vit":
        return synth.make_float_state_dims(dims["embed_dim"], dims["depth"], seed, dims["img_size"], dims["patch"])
    return synth.make_swin_float_state_dims(dims["embed_dim"], dims["depths"], dims["num_heads"], dims["window"], seed, dims["img_size"])


def generate(tag, natural):
    rq, synth = gg.rq, gg.synth
    kind, dims, ops, wseed, cseeds, cb, iseed, nimg = PLAN[tag]
    model = build(kind, dims, ops)
    fs = float_state(kind, dims, wseed)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("scaling_factor" in k or "integer" in k or "x_min" in k or "x_max" in k or k.endswith(".shift")
                or k.endswith("relative_position_index") or k.endswith("attn_mask")) for k in missing), missing[:5]
    model.eval()
    grids = ([tuple(model.patch_embed.grid_size)] if kind == "vit" else
             [(tuple(layer.input_resolution), [(b.window_size, b.shift_size) for b in layer.blocks]) for layer in model.layers])
    for cs in (cseeds if natural else cseeds[:1]):
        model(torch.from_numpy(synth.make_images(cb, cs, img_size=dims["img_size"])))
    ranges, bitsof = {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct):
            mx = float(torch.max(-mod.x_min, mod.x_max))
            if mx == 0.0:
                continue                                   # Swin's act_out: never called
            if not natural:
                q = 2 ** (mod.activation_bit - 1) - 1
                p = int(np.ceil(np.log2(mx / q)))
                mod.x_max.fill_(q * 2.0 ** p)
                mod.x_min.fill_(-q * 2.0 ** p)
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
            bitsof[name] = int(mod.activation_bit)
    shifts = {n: np.float32(m.shift.item()) for n, m in model.named_modules() if isinstance(m, rq.IBERTIntLayerNorm)}
    gg.ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            taps[name] = gg.to_int(y, s)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct) and name != "act_out" and not name.endswith("int_softmax.act"):
            mod.register_forward_hook(hook(name))
    imgs = synth.make_images(nimg, iseed, img_size=dims["img_size"])
    y = model(torch.from_numpy(imgs))
    tail = model.qact2 if kind == "vit" else model.qact3
    s_head = (model.head.fc_scaling_factor * tail.act_scaling_factor).float()
    names = sorted(taps)
    full = tag + ("_natural" if natural else "")
    meta = dict(tag=full, kind=kind, operators=ops, regime="natural" if natural else "pow2", weight_seed=wseed,
                calib_seeds=list(cseeds if natural else cseeds[:1]), calib_batch=cb, image_seed=iseed, n_images=nimg,
                img_size=list(dims["img_size"]), num_classes=synth.NUM_CLASSES, qkv_gain=synth.QKV_GAIN,
                dims={k: (list(v) if isinstance(v, tuple) else v) for k, v in dims.items()}, grids=grids, torch=torch.__version__)
    out = {
        "meta": np.array(json.dumps(meta)),
        "range_names": np.array(list(ranges)), "range_bits": np.array([bitsof[n] for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32), "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "shift_names": np.array(list(shifts), dtype=str), "shifts": np.array(list(shifts.values()), np.float32),
        "logits_int32": torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32),
        "logits_f32_bits": y.numpy().astype(np.float32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64), "head_scale": s_head.numpy().astype(np.float32),
        "tap_names": np.array(names), "tap_crc32": np.array([gg.crc(taps[n]) for n in names], np.uint32),
        "tap_absmax": np.array([int(np.abs(taps[n]).max()) for n in names], np.int64),
    }
    path = os.path.join(gg.GOLD, f"{full}.npz")
    np.savez_compressed(path, **out)
    digest = gg.crc(np.array(out["tap_crc32"], np.int64) & 0x7fffffff)
    print(f"[{full}] grids {grids}; {len(names)} taps (crc of crcs {digest:08x}), logits crc {gg.crc(out['logits_int32']):08x}, "
          f"top1 = {out['top1'].tolist()}, shifts {sorted(set(float(v) for v in shifts.values()))}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for t in (sys.argv[1:] or list(PLAN)):
        for nat in (False, True):
            generate(t, nat)
