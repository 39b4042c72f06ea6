"""GPU: the device JPEG decoder (ivit_jpeg_decode_u8) against Pillow's pixels in tests/golden/jpeg_decode_pil.npz and the host
decoder: every supported case alone, all cases in one mixed batch with the fallback images, the large file across many workgroups,
EvalTransform on an EncodedImages against the PackedImages of the same pixels (shards, 224 and 384), the engine's logits and the
evaluation harness on an ImageFolderJPEG.  No Pillow needed."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.transforms import (EvalTransform, ImageFolderJPEG, decode_images, decode_jpeg_host, encode_images,  # noqa: E402
                                 pack_images)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_jpeg_cpu import CASES  # noqa: E402

DEV = "cuda:0"
SUPPORTED = [c for c in CASES if c["supported"]]


def _fallback(cases):
    return lambda b, data: cases[b]["pixels"]


def _check(px, c):
    assert px.shape == (c["h"], c["w"], 3), c["name"]
    assert hashlib.sha256(np.ascontiguousarray(px).tobytes()).digest() == c["sha"], c["name"]
    if c["pixels"] is not None:
        assert np.array_equal(px, c["pixels"]), c["name"]


def _unpack(packed):
    data = packed.data.cpu().numpy()
    return [data[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(packed.offsets, packed.sizes)]


def test_each_supported_case_alone():
    for c in SUPPORTED:
        enc = encode_images([c["data"]])
        assert enc.sec_offsets[0] >= 0, c["name"]
        px = _unpack(decode_images(enc, device=DEV))[0]
        _check(px, c)
        assert np.array_equal(px, decode_jpeg_host(c["data"])), c["name"]


def test_mixed_batch_with_fallback_images():
    cases = CASES + CASES[::-1]
    enc = encode_images([c["data"] for c in cases], decode_fallback=_fallback(cases))
    assert sorted(enc.fallback) == [b for b, c in enumerate(cases) if not c["supported"]]
    packed = decode_images(enc, device=DEV)
    assert packed.data.device.type == "cuda"
    for px, c in zip(_unpack(packed), cases):
        _check(px, c)
    # a shard [lo, hi): offsets relative to lo, the same pixels
    for lo, hi in ((0, 1), (3, 17), (18, 22), (len(cases) - 2, len(cases))):
        for px, c in zip(_unpack(decode_images(enc, lo, hi, DEV)), cases[lo:hi]):
            _check(px, c)


def test_large_file_many_workgroups():
    c = next(c for c in CASES if c["name"] == "1200x1600_420_q90")
    enc = encode_images([c["data"]] * 3)
    _check(_unpack(decode_images(enc, device=DEV))[1], c)


def test_corrupt_data_never_launches_what_the_probe_rejects():
    c = next(c for c in CASES if c["name"] == "37x53_420_rst1")
    trunc = c["data"][:len(c["data"]) // 2]
    enc = encode_images([trunc, c["data"]], decode_fallback=lambda b, d: np.zeros((5, 6, 3), np.uint8))
    assert enc.sec_offsets[0] == -1 and "truncated" in enc.reasons[0]
    px = _unpack(decode_images(enc, device=DEV))
    assert px[0].shape == (5, 6, 3) and not px[0].any()
    _check(px[1], c)


def _reference_pixels(cases):
    out = []
    for c in cases:
        px = c["pixels"] if c["pixels"] is not None else decode_jpeg_host(c["data"])
        _check(px, c)
        out.append(px)
    return out


def test_eval_transform_on_encoded_equals_packed():
    cases = [c for c in CASES if c["h"] * c["w"] > 1] + CASES[:1]
    enc = encode_images([c["data"] for c in cases], decode_fallback=_fallback(cases))
    packed = pack_images(_reference_pixels(cases))
    for n in (224, 384):
        t = EvalTransform.for_input_size(n)
        assert np.array_equal(t(enc, device=DEV).cpu().numpy(), t(packed, device=DEV).cpu().numpy()), n
        for lo, hi in ((0, 5), (5, 6), (6, len(cases))):
            assert np.array_equal(t(enc, lo, hi, device=DEV).cpu().numpy(), t(packed, lo, hi, device=DEV).cpu().numpy()), (n, lo, hi)


def test_engine_logits_and_evaluation_on_image_folder(tmp_path):
    cases = SUPPORTED[:12]
    for k, c in enumerate(cases):
        d = tmp_path / f"class{k % 4}"
        d.mkdir(exist_ok=True)
        (d / f"{k:02d}.jpg").write_bytes(c["data"])
    folder = ImageFolderJPEG(str(tmp_path))
    by_path = {os.path.join(str(tmp_path), f"class{k % 4}", f"{k:02d}.jpg"): c for k, c in enumerate(cases)}
    ordered = [by_path[p] for p, _ in folder.samples]
    pixels = _reference_pixels(ordered)
    t = EvalTransform()
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=len(ordered))
    enc, targets = ImageFolderJPEG.collate([folder[i] for i in range(len(folder))])
    u8_enc = t(enc, device=DEV)
    u8_ref = t(pack_images(pixels), device=DEV)
    assert torch.equal(u8_enc, u8_ref)
    li_e = eng.forward(u8_enc)[0].clone()
    li_r = eng.forward(u8_ref)[0].clone()
    assert torch.equal(li_e, li_r) and li_r.abs().max() > 0

    model = _frozen_deit_tiny()
    cuts = [(0, 5), (5, 6), (6, len(folder))]
    enc_loader = [ImageFolderJPEG.collate([folder[i] for i in range(a, b)]) for a, b in cuts]
    ref_loader = [(pack_images(pixels[a:b]), targets[a:b]) for a, b in cuts]
    want = inference.evaluate_dataset_parallel(model, ref_loader, DEV, print_batch_stats=False, transform=t)
    got = inference.evaluate_dataset_parallel(model, enc_loader, DEV, print_batch_stats=False, transform=t)
    assert got == want
    assert inference.evaluate_dataset(model, enc_loader, DEV, print_batch_stats=False, transform=t) == want


def _frozen_deit_tiny():
    import ivit_amd.quantization_utils as q
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    model = ivit.deit_tiny_patch16_224()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV)
    ivit.freeze_model(model)
    return model


def test_decode_argument_errors():
    enc = encode_images([SUPPORTED[0]["data"]])
    with pytest.raises(IndexError):
        decode_images(enc, 0, 2, DEV)
    L = _lib.lib()
    assert L.ivit_jpeg_decode_u8(None, None, 1, 0, 0, 0, None, 0, None, None, None) == -1
