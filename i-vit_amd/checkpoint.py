"""Calibration ranges ("checkpoint minus weights") for the synthetic models.

A frozen I-ViT model is its float parameters plus one (x_min, x_max) pair per QuantAct
(/root/reference/models/quantization_utils/quant_modules.py:264-266, 290-294).  With no
network there are no trained checkpoints, so the ranges that go with the synthetic weights
(i-vit_amd/synth.py) were produced by running the reference's own calibration forward in the
build container and snapping to +-127*2^p (oracle/gen_golden.py); they are stored next to the
golden vectors under tests/golden/<tag>.npz.
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

TAGS = {"deit_tiny": "deit_tiny_patch16_224", "deit_small": "deit_small_patch16_224",
        "deit_base": "deit_base_patch16_224", "vit_base": "vit_base_patch16_224",
        "swin_tiny": "swin_tiny_patch4_window7_224", "deit_tiny_ibert": "deit_tiny_patch16_224",
        "deit_tiny_natural": "deit_tiny_patch16_224", "deit_tiny_w16": "deit_tiny_patch16_224", "deit_tiny_w16all": "deit_tiny_patch16_224", "deit_tiny_ibert_w16all": "deit_tiny_patch16_224", "swin_tiny_natural": "swin_tiny_patch4_window7_224", "deit_small_natural": "deit_small_patch16_224",
        "deit_base_natural": "deit_base_patch16_224", "deit_tiny_ibert_natural": "deit_tiny_patch16_224",
        "vit_large": "vit_large_patch16_224", "vit_large_natural": "vit_large_patch16_224",
        "swin_small": "swin_small_patch4_window7_224", "swin_small_natural": "swin_small_patch4_window7_224",
        # I-BERT operators with layernorm_type 'ibert_use-int-sqrt_true' (scripts/make_ibert_intsqrt_golden.py)
        "deit_tiny_ibert_isqrt": "deit_tiny_patch16_224", "deit_tiny_ibert_isqrt_natural": "deit_tiny_patch16_224",
        "deit_tiny_ibert_isqrt_w16all": "deit_tiny_patch16_224",
        # every width knob at 4 (scripts/gen_w4_golden.py)
        "deit_tiny_w4": "deit_tiny_patch16_224", "deit_tiny_w4_natural": "deit_tiny_patch16_224",
        "deit_tiny_ibert_w4": "deit_tiny_patch16_224", "deit_tiny_ibert_w4_natural": "deit_tiny_patch16_224"}


def load_fixture(tag: str):
    z = np.load(os.path.join(GOLDEN_DIR, f"{tag}.npz"))
    meta = json.loads(str(z["meta"]))
    ranges = {str(n): (np.float32(lo), np.float32(hi)) for n, lo, hi in zip(z["range_names"], z["x_min"], z["x_max"])}
    return z, meta, ranges


def sharpen_float_state(fs, meta):
    """The 4-bit fixtures' weights: synth.make_float_state's with the q and k rows of every attn.qkv scaled by meta["qk_gain"] and
    the class token by meta["cls_gain"] (absent: 1).  At 4 bits a softmax row of 197 keys whose largest probability is below 1/8 is
    all zeros, and a class token far below the activation step is a zero row: the plain synthetic weights give both."""
    qk, cg = float(meta.get("qk_gain", 1.0)), float(meta.get("cls_gain", 1.0))
    if qk == 1.0 and cg == 1.0:
        return fs
    fs = dict(fs)
    for k in list(fs):
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            v = np.array(fs[k], np.float32)
            v[:2 * v.shape[0] // 3] *= np.float32(qk)
            fs[k] = v
    fs["cls_token"] = (np.asarray(fs["cls_token"], np.float32) * np.float32(cg)).astype(np.float32)
    return fs


def load_synthetic_model(tag: str):
    """-> (float_state, ranges, cfg, meta, fixture) for one of the committed synthetic models."""
    z, meta, ranges = load_fixture(tag)
    if meta["factory"] in synth.SWIN_CONFIGS:
        cfg = synth.SWIN_CONFIGS[meta["factory"]]
        fs = synth.make_swin_float_state(meta["factory"], meta["weight_seed"])
    else:
        cfg = synth.MODEL_CONFIGS[meta["factory"]]
        fs = sharpen_float_state(synth.make_float_state(meta["factory"], meta["weight_seed"]), meta)
    return fs, ranges, cfg, meta, z


def load_dims_model(tag: str):
    """-> (float_state, ranges, meta, fixture) for a fixture whose meta record carries the model's dimensions instead of a factory
    name (scripts/gen_rect_golden.py: meta["kind"] "vit" | "swin", meta["dims"], meta["img_size"] = [height, width]).  The I-BERT
    LayerNorm shifts the fixture holds go into the float state under their state_dict names (`<module>.shift`)."""
    z, meta, ranges = load_fixture(tag)
    d = meta["dims"]
    img = tuple(meta["img_size"])
    if meta["kind"] == "swin":
        fs = synth.make_swin_float_state_dims(d["embed_dim"], tuple(d["depths"]), tuple(d["num_heads"]), d["window"], meta["weight_seed"],
                                              img, meta["num_classes"])
    else:
        fs = synth.make_float_state_dims(d["embed_dim"], d["depth"], meta["weight_seed"], img, d["patch"], meta["num_classes"])
    for name, sh in zip(z["shift_names"], z["shifts"]):
        fs[str(name) + ".shift"] = np.array([sh], np.float32)
    return fs, ranges, meta, z
