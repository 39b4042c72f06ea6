"""The 16-bit softmax above 207 tokens on the CPU, native library stubbed: which entry point engine_common.attention selects per
(operator family, softmax_bits, token count), and the ctypes row of ivit_attention_fused_i8_wide_long."""
import pytest
import torch

from ivit_amd import _lib
from ivit_amd.engine_common import attention


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    return rec


def _spec(family):
    a = dict(ms=(1 << 30, 34), mo=(1 << 30, 38), s_attn=0.125, exp2d=None, band=None, band_w=0)
    if family == "ibert":
        a["ib_table"] = torch.zeros(65536)
    return a


def _launch(family, T, softmax_bits, B=2, H=3):
    qkv = torch.zeros(3, B, H, T, 64, dtype=torch.int8)
    out = torch.zeros(B * T, H * 64, dtype=torch.int8)
    attention(_spec(family), family, qkv, out, B, H, T, 64, None, softmax_bits=softmax_bits)


@pytest.mark.parametrize("T,bits,name", [(577, 16, "ivit_attention_fused_i8_wide_long"), (208, 16, "ivit_attention_fused_i8_wide_long"),
                                         (1025, 8, "ivit_attention_fused_i8_wide_long"), (197, 16, "ivit_attention_fused_i8_wide"),
                                         (207, 16, "ivit_attention_fused_i8_wide"), (577, None, "ivit_attention_fused_i8_long"),
                                         (197, None, "ivit_attention_fused_i8_compat_band")])
def test_attention_selects_the_entry_point(calls, T, bits, name):
    _launch("ivit", T, bits)
    assert [n for n, _ in calls] == [name]
    args = calls[0][1]
    assert len(args) == len(_lib.SIGNATURES[name]) and args[2:6] == (2, 3, T, 64)
    if bits is not None:
        assert args[-3:] == (bits, 0, None)        # softmax_bits in front of the layout flag and the stream


def test_ibert_wide_rows_above_207_tokens_launch_nothing(calls):
    with pytest.raises(NotImplementedError, match="tokens=577"):
        _launch("ibert", 577, 16)
    assert calls == []
    _launch("ibert", 197, 16)
    _launch("ibert", 577, None)
    assert [n for n, _ in calls] == ["ivit_attention_fused_i8_ibert_wide", "ivit_attention_fused_i8_ibert_long"]


def test_ctypes_row_is_the_wide_one():
    assert _lib.SIGNATURES["ivit_attention_fused_i8_wide_long"] == _lib.SIGNATURES["ivit_attention_fused_i8_wide"]
    long = _lib.SIGNATURES["ivit_attention_fused_i8_long"]
    assert len(_lib.SIGNATURES["ivit_attention_fused_i8_wide_long"]) == len(long) + 1


# ----------------------------------------------------------------------------------- the module path's launches, library stubbed
import warnings  # noqa: E402

import ivit_amd as ivit  # noqa: E402
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402
from test_engine_launch_trace import stubbed  # noqa: E402,F401  (the fixture: recorder, pointers of host tensors)

W16ALL = {k: 16 for k in ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw",
                          "norm2_in_bw", "att_block_out_bw")}
LITERAL = ("ivit_bgemm_", "ivit_shiftmax_", "ivit_f32_to_i32", "ivit_requant_i32", "ivit_narrow_i32_i8")


def _steady_names(img, embed_dim, heads, batch, family, widths, calls):
    """launch names of the second module-by-module forward of a frozen depth-2 model whose ranges are all [-1, 1]"""
    torch.manual_seed(0)
    model = ivit.VisionTransformer(img_size=img, patch_size=16, embed_dim=embed_dim, depth=2, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                                   num_classes=40, gelu_type=family, softmax_type=family, layernorm_type=family, **widths).eval()
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            mod.x_min.fill_(-1.0)
            mod.x_max.fill_(1.0)
    ivit.freeze_model(model)
    model.use_engine = False
    x = torch.zeros(batch, 3, img, img)
    for _ in range(2):
        del calls[:]
        lazy.STATS.update(fused=0, materialised=0)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            model(x)
    return [n for n, _ in calls], dict(lazy.STATS)


@pytest.mark.parametrize("img,softmax_bw,attn", [(224, 16, "ivit_attention_fused_i8_wide"), (384, 16, "ivit_attention_fused_i8_wide_long"),
                                                 (384, 8, "ivit_attention_fused_i8_long")])
def test_16bit_stream_is_carried_module_by_module(stubbed, monkeypatch, img, softmax_bw, attn):  # noqa: F811
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    names, stats = _steady_names(img, 128, 2, 2, "ivit", dict(W16ALL, softmax_bw=softmax_bw, pos_encoding_bw=softmax_bw), stubbed)
    assert stats["materialised"] == 1 and not [n for n in names if n.startswith(LITERAL)]
    assert [n for n in names if n.startswith("ivit_attention_fused")] == [attn] * 2
    assert names.count("ivit_embed_assemble_i16") == 1 and names.count("ivit_gemm_i8_requant_i16") == 5
    assert names.count("ivit_residual_requant_i16") == 4 and names.count("ivit_layernorm_i16_i8") == 5
    assert names.count("ivit_i32_to_f32") == 1 and names[-1] == "ivit_i32_to_f32"          # the logits, at the boundary


def test_deit_base_width_defers_the_16bit_gemm_into_the_residual(stubbed, monkeypatch):  # noqa: F811
    """2308 rows at C = 768: projection / fc2 + their 16-bit QuantAct + the residual QuantAct are one launch each"""
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    names, stats = _steady_names(384, 768, 12, 4, "ivit", W16ALL, stubbed)
    assert stats["materialised"] == 1 and not [n for n in names if n.startswith(LITERAL)]
    assert names.count("ivit_gemm_i8_requant_i16_residual_i16_ex") == 4 and "ivit_residual_requant_i16" not in names
    assert names.count("ivit_gemm_i8_requant_i16") == 1                                     # the patch embedding
    assert names.count("ivit_attention_fused_i8_wide_long") == 2 and names.count("ivit_gemm_i8_requant_qkv_ex") == 2


def test_ibert_16bit_softmax_at_577_tokens_stays_literal_and_reenters(stubbed, monkeypatch):  # noqa: F811
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    names, stats = _steady_names(384, 128, 2, 2, "ibert", W16ALL, stubbed)
    assert not [n for n in names if n.startswith("ivit_attention_fused")]
    assert names.count("ivit_ibert_softmax_f32_f32") == 2                                   # the literal softmax, once per block
    assert names.count("ivit_residual_requant_i16") == 4 and names.count("ivit_ibert_layernorm_i16_i8_ex") == 5
