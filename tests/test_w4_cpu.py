"""The 4-bit width entries without a GPU: their prototypes in include/ivit_hip.h against _lib.SIGNATURES, the header's other
declarations still there, the width check ahead of everything else (a refused call touches nothing, so it needs no device), and the
module path's choice of entry per QuantAct width."""
import ctypes
import os
import re

import pytest

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
# new entry -> (the entry it extends, the width parameters it adds in front of the stream)
NEW = {"ivit_gemm_i8_requant_bits_ex": ("ivit_gemm_i8_requant_ex", ["int bits"]),
       "ivit_gemm_i8_requant_residual_bits_ex": ("ivit_gemm_i8_requant_residual_ex", ["int bits_mid", "int bits_out"]),
       "ivit_residual_requant_i8_bits": ("ivit_residual_requant_i8", ["int bits"]),
       "ivit_embed_assemble_i8_bits": ("ivit_embed_assemble_i8", ["int bits"])}


def _proto(name):
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", HEADER)
    assert decl, f"{name} is not declared in include/ivit_hip.h"
    return [" ".join(prm.split()) for prm in decl.group(1).split(",")]


def _kind(prm):
    return (ctypes.c_void_p if "*" in prm or prm.startswith("ivit_stream_t") else ctypes.c_float if prm.startswith("float") else
            ctypes.c_int64 if prm.startswith("int64_t") else ctypes.c_uint32 if prm.startswith("uint32_t") else
            ctypes.c_int32 if prm.startswith("int32_t") else ctypes.c_int)


@pytest.mark.parametrize("name", sorted(NEW))
def test_prototype_is_the_extended_entry_plus_its_widths(name):
    base, widths = NEW[name]
    proto, old = _proto(name), _proto(base)
    assert proto == old[:-1] + widths + [old[-1]]
    assert _lib.SIGNATURES[name] == [_kind(prm) for prm in proto]
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[base][:-1] + [ctypes.c_int] * len(widths) + [_lib.SIGNATURES[base][-1]]


def test_header_still_declares_every_bound_entry():
    declared = set(re.findall(r"\b(?:int|const char\*)\s+(ivit_[a-z0-9_]+)\s*\(", HEADER))
    missing = sorted(set(_lib.SIGNATURES) - declared)
    assert not missing, missing
    assert set(NEW) <= declared and len(declared) >= len(_lib.SIGNATURES)
    for wide in ("ivit_attention_fused_i8_wide", "ivit_attention_fused_i8_wide_long", "ivit_attention_fused_i8_ibert_wide"):
        text = HEADER[:HEADER.index("int " + wide + "(")]
        assert "softmax_bits = 4" in text[text.rindex("/*"):], wide


@pytest.mark.parametrize("bits", [0, 2, 6, 16])
def test_other_widths_are_refused_ahead_of_everything_else(bits):
    """IVIT_ERR_INVALID from the width alone: every pointer is NULL, nothing could have been launched"""
    L = _lib.lib()
    n = None
    calls = {"ivit_gemm_i8_requant_bits_ex": [(n, 0, n, 0, n, n, n, n, 0, 0, 0, 0, 0, bits, n)],
             "ivit_gemm_i8_requant_residual_bits_ex": [(n, 0, n, 0, n, n, n, n, 0, 1, 1, 1, 1, n, 0, 0, 0, 0, 0, bm, bo, n)
                                                       for bm, bo in ((bits, 8), (4, bits))],
             "ivit_residual_requant_i8_bits": [(n, 1, 1, n, 1, 1, n, 0, bits, n)],
             "ivit_embed_assemble_i8_bits": [(n, n, n, 1, 1, n, 0, 0, 0, bits, n)]}
    for name, argsets in calls.items():
        for args in argsets:
            assert getattr(L, name)(*args) == -1, name
            msg = L.ivit_last_error_string().decode()
            assert name in msg and "bits" in msg and "must be 4 or 8" in msg, msg


def test_softmax_width_message_names_the_three_widths():
    L = _lib.lib()
    for bits in (0, 12, 32):
        assert L.ivit_attention_fused_i8_wide(None, None, 1, 1, 197, 64, 1 << 30, 40, 0.25, 1 << 30, 40, None, None, 0, bits, 0, None) == -1
        assert "softmax_bits must be 4, 8 or 16" in L.ivit_last_error_string().decode()


# ----------------------------------------------------------------------------------- native library stubbed
from test_engine_launch_trace import _deit, _digest, _fixture, stubbed, trace_case  # noqa: E402,F401  (stubbed: the fixture)

W8 = {k: 8 for k in ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw", "norm2_in_bw",
                     "att_block_out_bw")}
W4 = {k: 4 for k in W8}


def test_frozen_quantact_at_4_bits_takes_the_fast_path(stubbed):
    """a frozen QuantAct(4) on a float tensor inside lazy.scope: _fast quantises with ivit_quantize_input_f32_i32 at bits = 4 and
    returns an int8-carrying tensor at scale range / 7; a width the reference does not clamp at (6) keeps the ordinary path"""
    import torch

    import ivit_amd.quantization_utils as q
    from ivit_amd.quantization_utils import lazy
    x = torch.linspace(-3.5, 2.0, 64).reshape(4, 16)
    got = {}
    for bits in (4, 6):
        act = q.QuantAct(bits)
        act.x_min.fill_(-3.5)
        act.x_max.fill_(2.0)
        act.fix()
        del stubbed[:]
        with lazy.scope(True), torch.no_grad():
            y, s = act(x)
        got[bits] = (isinstance(y, lazy.QT), [(n, a) for n, a in stubbed if n.startswith("ivit_quantize_input")], float(s.reshape(-1)[0]))
    carried, calls, scale = got[4]
    assert carried and [n for n, _ in calls] == ["ivit_quantize_input_f32_i32"] and calls[0][1][4] == 4
    assert scale == pytest.approx(3.5 / 7, rel=1e-6)
    assert not got[6][0]


@pytest.mark.parametrize("widths,expect", [(W4, (4, 4, 4)), (dict(W4, softmax_bw=8, pos_encoding_bw=8), (4, 8, 8)),
                                           (dict(W4, pos_encoding_bw=8), (4, 4, 8)), (dict(W4, softmax_bw=8), (4, 8, 4))])
@pytest.mark.parametrize("family", ["ivit", "ibert"])
def test_engine_patterns_are_recognised(widths, expect, family):
    m = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=10,
                               gelu_type=family, softmax_type=family, layernorm_type=family, **widths)
    assert m.engine_unsupported_reason() is None and m._engine_widths == expect


@pytest.mark.parametrize("widths", [dict(W8, block_input_bw=4), dict(W4, mlp_out_bw=8), dict(W4, patch_embed_bw=8), dict(W4, softmax_bw=16),
                                    dict(W4, pos_encoding_bw=16), dict(W4, norm2_in_bw=16)],
                         ids=["block_input_only", "mlp_out_8", "patch_embed_8", "softmax_16", "position_16", "norm2_in_16"])
def test_other_4_bit_patterns_keep_the_module_path_and_name_a_quantact(widths):
    m = ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=10,
                               **widths)
    why = m.engine_unsupported_reason()
    assert why is not None and (why.startswith("QuantAct ") and "-bit" in why or "output width" in why), why
    if why.startswith("QuantAct "):
        name = why.split()[1]
        assert int(dict(m.named_modules())[name].activation_bit) != 8, why       # the QuantAct it names is one of the odd ones


def test_long_rows_at_4_bits_ivit_only():
    kw = dict(img_size=384, patch_size=16, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=10, **W4)
    assert ivit.VisionTransformer(**kw).engine_unsupported_reason() is None
    ib = ivit.VisionTransformer(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert", **kw)
    assert "193 .. 207" in ib.engine_unsupported_reason()


@pytest.mark.parametrize("tag,family", [("deit_tiny_w4", "ivit"), ("deit_tiny_ibert_w4_natural", "ibert")])
def test_engine_launch_trace_at_stream_bits_4(stubbed, tag, family):
    """the `_bits` entries at the six stream sites with their widths in the right argument positions, the wide attention entry with
    softmax_bits = 4; no class-row tail"""
    import torch
    eng = _deit(tag, family=family, stream_bits=4, softmax_bits=4, pos_bits=4)
    assert not eng.cls_tail_ok
    x = torch.zeros(16, 3, 224, 224)
    with pytest.raises(ValueError, match="cls_tail"):
        eng.forward(x, cls_tail=True)
    del stubbed[:]
    eng.forward(x)
    names = [n for n, _ in stubbed]
    D, sig = eng.D, _lib.SIGNATURES
    by = {n: [a for m, a in stubbed if m == n] for n in set(names)}
    assert all(len(a) == len(sig[n]) for n, args in by.items() for a in args)
    assert len(by["ivit_gemm_i8_requant_bits_ex"]) == 1 and by["ivit_gemm_i8_requant_bits_ex"][0][-2] == 4          # patch_embed.qact
    assert len(by["ivit_embed_assemble_i8_bits"]) == 1 and by["ivit_embed_assemble_i8_bits"][0][-2] == 4             # qact1
    res = by["ivit_gemm_i8_requant_residual_bits_ex"]                         # attn.qact3 + qact2, mlp.qact2 + qact4 per block
    assert len(res) == 2 * D and all(a[-3:-1] == (4, 4) for a in res)
    wide = "ivit_attention_fused_i8_ibert_wide" if family == "ibert" else "ivit_attention_fused_i8_wide"
    assert [n for n in names if "attention" in n] == [wide] * D and all(a[-3] == 4 for a in by[wide])
    assert not {"ivit_gemm_i8_requant_residual_ex", "ivit_embed_assemble_i8", "ivit_attention_cls_i8"} & set(names)
    # qkv and fc1 keep the 8-bit entries (their QuantActs are no width knobs)
    assert names.count("ivit_gemm_i8_requant_qkv_ex") == D


def test_engine_launch_trace_at_stream_bits_8_is_the_golden_one(stubbed, monkeypatch):
    """tests/golden/engine_launch_trace.json, through the trace test's own machinery"""
    got = {f"deit_tiny/{phase}": _digest(lines) for phase, lines in trace_case("deit_tiny", stubbed, monkeypatch).items()}
    want = {k: v for k, v in _fixture().items() if k.startswith("deit_tiny/")}
    assert got == want and len(want) >= 8
