"""IBERTIntLayerNorm(use_int_sqrt=True) -- layernorm_type 'ibert_use-int-sqrt_true' -- on the CPU: the numpy restatement of
integer_sqrt against the reference's values, construction through the registry / build_model, and, with the native library stubbed,
that the fused engine and the integer-carrying module path accept such a model and carry IVIT_IBERT_LN_INT_SQRT on every LayerNorm
launch.  (The kernels are compared on the GPU in tests/test_gpu_ibert_intsqrt.py.)"""
import math
import os
import warnings

import numpy as np
import pytest
import torch

import ivit_amd as ivit
import ivit_amd.quantization_utils as qu
from ivit_amd import _lib
from ivit_amd.engine_common import IBERT_LN_INT_SQRT
from ivit_amd.inference import build_model
from ivit_amd.quantization_utils import get_gelu, get_layernorm, get_softmax, lazy

import ibert_intsqrt_ref as R
from test_engine_launch_trace import stubbed  # noqa: F401  (the fixture: recorder, pointers of host tensors)

ISQRT = "ibert_use-int-sqrt_true"
LN_ENTRIES = {"ivit_ibert_layernorm_i8": 12, "ivit_ibert_layernorm_i16_i8_ex": 12}      # name -> index of the int that carries the flag


def test_restatement_equals_the_reference_on_every_kat_entry(golden_dir):
    z = np.load(os.path.join(golden_dir, "ibert_intsqrt_kat.npz"))
    n, want = z["n"], z["isqrt"]
    assert n.dtype == np.float32 and n.size > 20000 and n[0] == 0 and want[0] == 0
    got = R.integer_sqrt(n)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, n[bad[:5]], got[bad[:5]], want[bad[:5]])
    # what makes shortcuts wrong is in the fixture: results above floor(sqrt(n)), and a start value the bit length would not give
    isq = np.array([math.isqrt(int(v)) for v in n])
    assert (want != isq).sum() > 500 and set(want - isq) == {0, 1}
    for v, r in ((3, 2), (15, 4), (80, 9), (255, 16), (16777215, 4096), (4194303, 2047)):
        assert want[np.nonzero(n == v)[0][0]] == r, v
    assert R.log2_bits(np.array([2097151, 8388603, 8388602, 16777205, 16777204], np.float32)).tolist() == [22, 24, 23, 25, 24]


def test_restatement_equals_the_reference_layernorm_rows(golden_dir):
    """every output row of the reference's module, by CRC-32, for the seeded inputs of ibert_intsqrt_ref.CASES"""
    z = np.load(os.path.join(golden_dir, "ibert_intsqrt_ops.npz"))
    seen_large = 0
    for case in R.CASES[::3]:                            # a third of the cases here; the GPU tests walk all of them
        d, key = R.make_case(case), R.case_key(case)
        bias_int, s_out = R.layernorm_constants(d["gamma"], d["beta"])
        mean_int, var_int = z[key + "/mean_int"].reshape(-1, 1), z[key + "/var_int"].reshape(-1, 1)
        y = R.layernorm(R.x_int_of(d["q"], d["s_in"]), bias_int, s_out, d["shift_pow2"], mean_int=mean_int, var_int=var_int)
        assert np.array_equal(R.row_crcs(y), z[key + "/row_crc32"]), key
        assert np.isnan(y[0]).all()                      # the constant row: std = 0
        seen_large += int((var_int >= 2 ** 24).sum())
        if case[1] != "q16":                             # sums below 2^24: order-free, the restatement's own sums are the fixture's
            assert np.array_equal(R.row_crcs(R.layernorm(R.x_int_of(d["q"], d["s_in"]), bias_int, s_out, d["shift_pow2"])), z[key + "/row_crc32"])
    assert seen_large > 300


def test_registry_builds_the_parameterised_layernorm():
    ln = get_layernorm(ISQRT)(192)
    assert isinstance(ln, qu.IBERTIntLayerNorm) and ln.use_int_sqrt is True
    assert qu.IBERTIntLayerNorm(192).use_int_sqrt is False and get_layernorm("ibert")(192).use_int_sqrt is False
    assert get_layernorm("ibert_use-int-sqrt_false")(192).use_int_sqrt is False
    for get in (get_gelu, get_softmax, get_layernorm):
        with pytest.raises(KeyError):
            get("ppoly")


def test_build_model_with_the_name():
    plain = build_model({"model_name": "deit_tiny"})
    for model in (build_model({"model_name": "deit_tiny", "layernorm_type": ISQRT}), build_model({"model_name": "deit_tiny"}, layernorm_type=ISQRT)):
        assert model.state_dict().keys() == plain.state_dict().keys()
        lns = [m for m in model.modules() if isinstance(m, qu.IBERTIntLayerNorm)]
        assert len(lns) == 25 and all(m.use_int_sqrt for m in lns)
        assert model.op_types == ("ibert",) * 3 and model.op_params == ({}, {}, {"use_int_sqrt": True}) and model.ln_int_sqrt
        assert model.engine_unsupported_reason() is None          # 224 / 16
    assert plain.op_types == ("ibert",) * 3 and not plain.ln_int_sqrt and plain.engine_unsupported_reason() is None


def _small(layernorm_type, widths=None):
    torch.manual_seed(0)
    model = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                   num_classes=40, gelu_type="ibert", softmax_type="ibert", layernorm_type=layernorm_type,
                                   **(widths or {})).eval()
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            mod.x_min.fill_(-1.0)
            mod.x_max.fill_(1.0)
    ivit.freeze_model(model)
    return model


def _forward(model, calls, use_engine):
    model.use_engine = use_engine
    x = torch.zeros(2, 3, 224, 224)
    for _ in range(2):                                   # the second forward: caches warm, no table builds
        del calls[:]
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model(x)
    return list(calls)


def _strip(calls):
    return [(n, tuple(a & ~IBERT_LN_INT_SQRT if n in LN_ENTRIES and i == LN_ENTRIES[n] else a for i, a in enumerate(args))) for n, args in calls]


W16ALL = {k: 16 for k in ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw",
                          "norm2_in_bw", "att_block_out_bw")}


@pytest.mark.parametrize("use_engine", [True, False])
@pytest.mark.parametrize("widths,entry", [(None, "ivit_ibert_layernorm_i8"), (W16ALL, "ivit_ibert_layernorm_i16_i8_ex")])
def test_every_layernorm_launch_carries_the_flag(stubbed, monkeypatch, use_engine, widths, entry):  # noqa: F811
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    model = _small(ISQRT, widths)
    assert model.engine_unsupported_reason() is None and model.takes_engine(torch.zeros(1)) is True
    flagged = _forward(model, stubbed, use_engine)
    if use_engine:
        assert model.engine(2).int_sqrt is True
    lns = [(n, a) for n, a in flagged if "layernorm" in n]
    assert [n for n, _ in lns] == [entry] * 5            # norm1, norm2 of two blocks, the final norm
    for n, a in lns:
        assert len(a) == len(_lib.SIGNATURES[n]) and a[LN_ENTRIES[n]] & IBERT_LN_INT_SQRT, (n, a[LN_ENTRIES[n]])
        assert a[LN_ENTRIES[n]] & ~IBERT_LN_INT_SQRT in (0, 1)
    # the plain model: the same launches without the flag, which is what it launched before the flag existed
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    model = _small("ibert", widths)
    plain = _forward(model, stubbed, use_engine)
    if use_engine:
        assert model.engine(2).int_sqrt is False
    assert [n for n, _ in plain] == [n for n, _ in flagged]
    for n, a in plain:
        if n in LN_ENTRIES:
            assert a[LN_ENTRIES[n]] in (0, 1)
    assert len(plain) == len(flagged)
    for (n, a), (_, b) in zip(_strip(flagged), plain):   # pointers differ between two models; every integer and float argument agrees
        assert [(x, y) for x, y in zip(a, b) if isinstance(x, (int, float)) and not isinstance(x, bool) and abs(x) < 2 ** 31 and x != y] == [], n


def test_the_literal_module_calls_the_ex_entry(stubbed):  # noqa: F811
    for flag, name in ((True, "ivit_ibert_layernorm_f32_f32_ex"), (False, "ivit_ibert_layernorm_f32_f32")):
        ln = qu.IBERTIntLayerNorm(64, use_int_sqrt=flag)
        ln.fix()
        del stubbed[:]
        ln(torch.zeros(1, 3, 64), torch.tensor([0.25]))
        assert [n for n, _ in stubbed] == [name]
        args = stubbed[0][1]
        assert len(args) == len(_lib.SIGNATURES[name]) and (args[-2] == IBERT_LN_INT_SQRT) == flag


@pytest.mark.parametrize("kw,word", [(dict(layernorm_type="ibert_overflow-handling_false"), "overflow_handling"),
                                     (dict(layernorm_type="ibert_use-int-sqrt_true_eps_1"), "eps"),
                                     (dict(softmax_type="ibert_quant-mode_symmetric"), "quant_mode")])
def test_other_parameters_keep_the_module_path(stubbed, monkeypatch, kw, word):  # noqa: F811
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    torch.manual_seed(0)
    model = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=1, num_heads=2, num_classes=40,
                                   **{**dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert"), **kw}).eval()
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            mod.x_min.fill_(-1.0)
            mod.x_max.fill_(1.0)
    ivit.freeze_model(model)
    reason = model.engine_unsupported_reason()
    assert reason is not None and word in reason and not model.takes_engine(torch.zeros(1))
    calls = _forward(model, stubbed, True)
    names = [n for n, _ in calls]
    # module by module, literally: no fused launch, the float-view LayerNorm kernel
    assert not [n for n in names if n in LN_ENTRIES] and [n for n in names if n.startswith("ivit_ibert_layernorm_f32_f32")]


def test_engine_refuses_the_flag_for_the_ivit_family(stubbed):  # noqa: F811
    from ivit_amd.checkpoint import load_synthetic_model
    from ivit_amd.engine import IntViTEngine
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    with pytest.raises(ValueError, match="int_sqrt"):
        IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=2, int_sqrt=True)


@pytest.mark.parametrize("tag", ["deit_tiny_ibert_isqrt", "deit_tiny_ibert_isqrt_natural", "deit_tiny_ibert_isqrt_w16all"])
def test_model_fixtures_load(tag):
    from ivit_amd.checkpoint import TAGS, load_synthetic_model
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    assert TAGS[tag] == meta["factory"] and meta["layernorm_type"] == ISQRT and meta["n_images"] == 4
    assert z["logits_int32"].shape == (4, 1000) and z["top1"].shape == (4,) and len(ranges) == len(z["range_bits"])
    assert set(meta["ln_shifts"].values()) == ({1.0, 2.0} if tag.endswith("w16all") else {0.0})
