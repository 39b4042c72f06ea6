"""The fused DeiT / ViT engine with the 4-bit stream (IntViTEngine(stream_bits=4): the width knobs of vit_quant.py:180-187 at 4, what
`--bitwidth 4` sets): the reference's fixtures (tests/golden/deit_tiny_w4*, deit_tiny_ibert_w4*: INT32 logits, top-1, the CRC32 of every
QuantAct tap) by direct construction, forward / forward_graph / forward_topk_graph agreeing; model(x) of a `--bitwidth 4` model taking
the engine and equalling the module path bit for bit; long rows through ivit_attention_fused_i8_wide_long; batch invariance."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

from test_gpu_vit16_lazy import _Trace, _images, bits  # noqa: E402
from test_gpu_w4_lazy import W4, _calibrated  # noqa: E402

DEV = "cuda:0"
TAGS = ["deit_tiny_w4", "deit_tiny_w4_natural", "deit_tiny_ibert_w4", "deit_tiny_ibert_w4_natural"]
BITS = ("ivit_gemm_i8_requant_bits_ex", "ivit_embed_assemble_i8_bits", "ivit_gemm_i8_requant_residual_bits_ex")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def _engine(tag, max_batch=4):
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=max_batch,
                       family=meta["family"], stream_bits=4, softmax_bits=4, pos_bits=4)
    return eng, cfg, meta, z


@pytest.mark.parametrize("tag", TAGS)
def test_engine_reproduces_the_reference_fixtures(tag):
    """every QuantAct tap the reference recorded and the engine materialises, INT32 logits and top-1; then the two graph replays"""
    eng, cfg, meta, z = _engine(tag)
    n = meta["n_images"]
    imgs = torch.from_numpy(synth.make_images(n, meta["image_seed"])).to(DEV)
    taps = {}
    with _Trace() as tr:
        li, lf, t1 = eng.forward(imgs, taps)
    torch.cuda.synchronize()
    gold = dict(zip([str(x) for x in z["tap_names"]], z["tap_crc32"]))
    bad = [name for name, t in taps.items() if name in gold and crc(t.cpu().numpy().astype(np.int32)) != int(gold[name])]
    assert not bad, bad[:5]
    assert sum(1 for name in taps if name in gold) == 7 * cfg["depth"] + 3
    li0, lf0, t10 = li.clone(), lf.clone(), t1.clone()
    assert np.array_equal(li0.cpu().numpy(), z["logits_int32"]), f"{tag}: INT32 logits differ"
    assert np.array_equal(t10.cpu().numpy().astype(np.int64), z["top1"])
    # the six stream sites go through the `_bits` entries, attention through the wide entry with softmax_bits = 4
    D = cfg["depth"]
    assert [tr.names.count(n) for n in BITS] == [1, 1, 2 * D]
    wide = "ivit_attention_fused_i8_ibert_wide" if meta["family"] == "ibert" else "ivit_attention_fused_i8_wide"
    assert [n for n in tr.names if "attention" in n] == [wide] * D
    assert not [n for n in tr.names if n in ("ivit_gemm_i8_requant_residual_ex", "ivit_embed_assemble_i8")]
    assert not eng.cls_tail_ok
    with pytest.raises(ValueError, match="cls_tail"):
        eng.forward(imgs, cls_tail=True)
    lg = eng.forward_graph(imgs)
    assert torch.equal(lg[0], li0) and torch.equal(lg[1], lf0) and torch.equal(lg[2], t10)
    lk = eng.forward_topk_graph(imgs, k=3)
    assert torch.equal(lk[0], li0) and torch.equal(lk[2].view(n, -1)[:, 0], t10)


@pytest.mark.parametrize("tag", ["deit_tiny_w4_natural", "deit_tiny_ibert_w4"])
def test_logits_do_not_depend_on_the_batch(tag):
    eng, cfg, meta, z = _engine(tag)
    imgs = torch.from_numpy(synth.make_images(3, meta["image_seed"])).to(DEV)
    all3 = eng.forward(imgs)[0].clone()
    for i in range(3):
        assert torch.equal(eng.forward(imgs[i:i + 1].contiguous())[0][0], all3[i]), i
    assert np.array_equal(all3.cpu().numpy(), z["logits_int32"])


def _frozen_bitwidth4(tag):
    """inference.build_model(cfg, bitwidth=4) with the fixture's weights and ranges, frozen"""
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    fam = meta["family"]
    model = inference.build_model(dict(model_name="deit_tiny", gelu_type=fam, softmax_type=fam, layernorm_type=fam), bitwidth=4)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    mods = dict(model.named_modules())
    for name, mod in mods.items():
        if isinstance(mod, q.QuantAct) and name in ranges:
            assert int(mod.activation_bit) == int(dict(zip(z["range_names"], z["range_bits"]))[name]), name
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    for name, sh in meta.get("ln_shifts", {}).items():
        mods[name].shift.fill_(float(sh))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    return model, meta, z


@pytest.mark.parametrize("tag", TAGS)
def test_bitwidth_4_model_takes_the_engine_and_equals_the_module_path(tag):
    model, meta, z = _frozen_bitwidth4(tag)
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    assert model.engine_unsupported_reason() is None and model._engine_widths == (4, 4, 4)
    assert model.takes_engine(imgs), model.engine_unsupported_reason()
    with torch.no_grad(), _Trace() as tr:
        y = model(imgs)
    assert "ivit_gemm_i8_requant_residual_bits_ex" in tr.names and "ivit_i32_to_f32" not in tr.names      # the engine ran
    model.use_engine = False
    with torch.no_grad():
        y_mod = model(imgs)
    assert (bits(y) == bits(y_mod)).all()
    li = np.rint(y.cpu().numpy().astype(np.float64) / z["head_scale"].astype(np.float64)).astype(np.int32)
    assert np.array_equal(li, z["logits_int32"]) and np.array_equal(y.argmax(dim=1).cpu().numpy(), z["top1"])


@pytest.mark.parametrize("widths,expect", [(dict(W4, softmax_bw=8, pos_encoding_bw=8), (4, 8, 8)), (dict(W4, pos_encoding_bw=8), (4, 4, 8)),
                                           (dict(W4, softmax_bw=8), (4, 8, 4))])
def test_the_other_engine_patterns_equal_the_module_path(widths, expect):
    model, g = _calibrated(224, 16, 128, 2, 2, True, 3, "ivit", widths)
    x = _images(3, 224, g)
    assert model.engine_unsupported_reason() is None and model._engine_widths == expect and model.takes_engine(x)
    with torch.no_grad():
        y = model(x)
        model.use_engine = False
        y_mod = model(x)
    assert (bits(y) == bits(y_mod)).all() and int((y != 0).sum()) > y.numel() // 2


def test_long_rows_go_through_the_wide_long_entry():
    """384 px / 16: 577 tokens, depth 2: one ivit_attention_fused_i8_wide_long per block, the module path's logits"""
    model, g = _calibrated(384, 16, 128, 2, 2, True, 3, "ivit", W4)
    x = _images(2, 384, g)
    assert model.takes_engine(x), model.engine_unsupported_reason()
    with torch.no_grad(), _Trace() as tr:
        y = model(x)
    assert [n for n in tr.names if "attention" in n] == ["ivit_attention_fused_i8_wide_long"] * 2
    model.use_engine = False
    with torch.no_grad():
        y_mod = model(x)
    assert (bits(y) == bits(y_mod)).all() and int((y != 0).sum()) > y.numel() // 2


def test_refused_geometries_stay_refused():
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny_ibert_w4")
    with pytest.raises(ValueError, match="207 tokens"):
        IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, family="ibert", stream_bits=4, img_size=384)
    with pytest.raises(ValueError, match="softmax_bits / pos_bits"):
        IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, stream_bits=4, softmax_bits=16)
