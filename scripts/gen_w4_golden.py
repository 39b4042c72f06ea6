"""Writes the four 4-bit fixtures of tests/golden/: the reference's own DeiT-Tiny forward with all eight width knobs at 4
(vit_quant.py:180-187, what `--bitwidth 4` sets), on the CPU.

    deit_tiny_w4.npz                I-ViT operators, every QuantAct range snapped to the next power of two
    deit_tiny_w4_natural.npz        I-ViT operators, ranges as calibrated
    deit_tiny_ibert_w4.npz          I-BERT operators, power-of-two ranges
    deit_tiny_ibert_w4_natural.npz  I-BERT operators, ranges as calibrated

The reference's models/vit_quant.py is imported unmodified through the harness-side shims of oracle/gen_golden.py (reused by
import).  Weights from synth.make_float_state(seed), q / k and the class token scaled as checkpoint.sharpen_float_state
says (recorded in the fixture's meta), calibrated on seeded batches, frozen.  A fixture holds data only, in the
layout of deit_tiny_ibert_w16all.npz: the seeds of its images (synth.make_images), the ranges and their widths, the LayerNorm shifts
of the I-BERT family, INT32 logits, top-1 and the CRC32 of every QuantAct tap.  oracle/gen_golden.py offers no CPU-oracle check for
its 16-bit model fixtures (gen_w16 / gen_ibert_natural record the reference alone), so none is asserted here either; what is
asserted is that the fixture is not degenerate: every tap of a 4-bit QuantAct stays inside [-8, 7], the residual stream uses more than one
step of it in every block, and the logits of different images differ.  Run from the repository root:  python scripts/gen_w4_golden.py"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402  (the shims, on import)
from ivit_amd.checkpoint import sharpen_float_state  # noqa: E402

FACTORY, WEIGHT_SEED, CALIB_SEEDS, CALIB_BATCH, IMAGE_SEED, N_IMAGES = "deit_tiny_patch16_224", 11, (101, 111), 4, 1001, 3
W4 = dict(patch_embed_bw=4, pos_encoding_bw=4, block_input_bw=4, attention_out_bw=4, softmax_bw=4, mlp_out_bw=4, norm2_in_bw=4,
          att_block_out_bw=4)
# checkpoint.sharpen_float_state: a class token the 4-bit step can see and, for Shiftmax, peaked attention rows (the I-BERT softmax
# keeps synth's q / k: its float32 sequence breaks down at the input scale that sharper scores would need)
QK_GAIN, CLS_GAIN = {"ivit": 4.0, "ibert": 1.0}, 30.0
TAGS = {"deit_tiny_w4": ("ivit", True), "deit_tiny_w4_natural": ("ivit", False),
        "deit_tiny_ibert_w4": ("ibert", True), "deit_tiny_ibert_w4_natural": ("ibert", False)}


def generate(tag):
    family, pow2 = TAGS[tag]
    rq, synth = gg.rq, gg.synth
    model = getattr(gg.ref_models, FACTORY)(pretrained=False, gelu_type=family, softmax_type=family, layernorm_type=family, **W4)
    fs = sharpen_float_state(synth.make_float_state(FACTORY, WEIGHT_SEED), dict(qk_gain=QK_GAIN[family], cls_gain=CLS_GAIN))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    for cs in CALIB_SEEDS:
        model(torch.from_numpy(synth.make_images(CALIB_BATCH, cs)))
    acts = {n: m for n, m in model.named_modules() if isinstance(m, rq.QuantAct)}
    if pow2:
        for name, mod in acts.items():
            mx = float(torch.max(-mod.x_min, mod.x_max))
            assert mx > 0.0, f"{name} saw nothing but zeros in calibration"
            q = float(2 ** (mod.activation_bit - 1) - 1)
            p = int(np.ceil(np.log2(mx / q)))
            mod.x_max.fill_(q * 2.0 ** p)
            mod.x_min.fill_(-q * 2.0 ** p)
    ranges = {n: (np.float32(m.x_min.item()), np.float32(m.x_max.item())) for n, m in acts.items()}
    bits = {n: int(m.activation_bit) for n, m in acts.items()}
    shifts = {n: float(m.shift) for n, m in model.named_modules() if family == "ibert" and isinstance(m, rq.IBERTIntLayerNorm)}
    gg.ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, sc = outp
            taps[name] = gg.to_int(y, sc)
        return fn

    for name, mod in acts.items():
        if not name.endswith("int_softmax.act"):
            mod.register_forward_hook(hook(name))
    imgs = synth.make_images(N_IMAGES, IMAGE_SEED)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact2.act_scaling_factor).float()
    logits = torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32)
    names = sorted(taps)
    narrow = [n for n in names if bits[n] == 4 and n != "qact_pos"]
    assert len(narrow) == 2 + 4 * len(model.blocks), narrow
    for n in narrow:
        stream = n == "qact1" or n.endswith((".qact2", ".qact4")) and ".attn." not in n and ".mlp." not in n
        assert -8 <= taps[n].min() and taps[n].max() <= 7 and (np.abs(taps[n]).max() >= 2 or not stream), (n, taps[n].min(), taps[n].max())
    assert all((logits[i] != logits[j]).any() for i in range(N_IMAGES) for j in range(i)) and np.abs(logits).max() > 100, logits[:, :6]
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=FACTORY, family=family, weight_seed=WEIGHT_SEED, calib_seeds=list(CALIB_SEEDS),
                                         calib_batch=CALIB_BATCH, image_seed=IMAGE_SEED, n_images=N_IMAGES, qkv_gain=synth.QKV_GAIN,
                                         qk_gain=QK_GAIN[family], cls_gain=CLS_GAIN,
                                         regime="pow2" if pow2 else "natural", ln_shifts=shifts, widths=W4, torch=torch.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([bits[n] for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": logits,
        "logits_f32_bits": y.detach().numpy().astype(np.float32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64), "head_scale": s_head.numpy().astype(np.float32),
        "tap_names": np.array(names), "tap_crc32": np.array([gg.crc(taps[n]) for n in names], np.uint32),
        "tap_absmax": np.array([int(np.abs(taps[n]).max()) for n in names], np.int64),
    }
    path = os.path.join(gg.GOLD, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"[{tag}] {len(names)} taps ({len(narrow)} at 4 bits), top1 = {out['top1'].tolist()}, |logits| <= {int(np.abs(logits).max())}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    with torch.no_grad():
        for t in (sys.argv[1:] or list(TAGS)):
            generate(t)
