"""Long-row attention (208 .. 1025 tokens) on the CPU: the launches the engine issues at 384 / 16 (577 tokens) with the native library
stubbed (as tests/test_engine_launch_trace.py does), the engine-routing predicate of vit_quant.VisionTransformer across operator family,
stream width and token count, and the C prototype of ivit_attention_fused_i8_long against the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine
import ivit_amd.vit_quant as vq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN = ("ivit_attention_fused_i8", "ivit_attention_fused_i8_ex", "ivit_attention_fused_i8_compat", "ivit_attention_fused_i8_compat_band",
        "ivit_attention_fused_i8_wide", "ivit_attention_fused_i8_ibert", "ivit_attention_fused_i8_ibert_wide", "ivit_attention_fused_i8_long")


@pytest.fixture
def calls(monkeypatch):
    rec = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: rec.append((name, args)))
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "lib", lambda: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return rec


def _engine(img, patch, tag="deit_tiny", **kw):
    """deit_tiny's weights and ranges with a position embedding of the geometry's token count"""
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    fs = dict(fs)
    T = (img // patch) ** 2 + 1
    fs["pos_embed"] = np.random.default_rng(T).normal(0, 0.02, size=(1, T, cfg["embed_dim"])).astype(np.float32)
    return IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=2,
                        img_size=img, patch_size=patch, **kw), cfg


@pytest.mark.parametrize("tag", ["deit_tiny", "deit_tiny_natural"])
def test_engine_at_384_issues_one_long_attention_per_block(calls, tag):
    eng, cfg = _engine(384, 16, tag)
    assert eng.T == 577
    calls.clear()
    eng.forward(torch.zeros(2, 3, 384, 384))
    attn = [(n, a) for n, a in calls if n in ATTN]
    assert [n for n, _ in attn] == ["ivit_attention_fused_i8_long"] * cfg["depth"]
    for _, a in attn:
        assert a[2:6] == (2, cfg["num_heads"], 577, 64) and len(a) == len(_lib.SIGNATURES["ivit_attention_fused_i8_long"])


def test_engine_at_224_keeps_the_short_kernel(calls):
    eng, cfg = _engine(224, 16)
    calls.clear()
    eng.forward(torch.zeros(2, 3, 224, 224))
    assert [n for n, _ in calls if n in ATTN] == ["ivit_attention_fused_i8_compat_band"] * cfg["depth"]


@pytest.mark.parametrize("kw", [dict(family="ibert"), dict(stream_bits=16)])
def test_engine_rejects_long_rows_outside_ivit_8bit(calls, kw):
    with pytest.raises(ValueError, match="207 tokens"):
        _engine(384, 16, **kw)


def test_engine_rejects_more_than_1025_tokens(calls):
    with pytest.raises(ValueError, match="1025 tokens"):
        _engine(528, 16)                  # 33^2 + 1 = 1090 tokens


# the reference's width knobs of its 16-bit residual stream (vit_quant.py:180-187; '--bitwidth 16' without the softmax / position ones)
WIDE = dict(patch_embed_bw=16, block_input_bw=16, attention_out_bw=16, mlp_out_bw=16, norm2_in_bw=16, att_block_out_bw=16)


@pytest.mark.parametrize("img,patch,tokens", [(224, 16, 197), (160, 16, 101), (224, 32, 50), (256, 16, 257), (384, 16, 577),
                                              (224, 8, 785), (512, 16, 1025), (528, 16, 1090)])
@pytest.mark.parametrize("family", ["ivit", "ibert"])
@pytest.mark.parametrize("stream", [8, 16])
def test_engine_unsupported_reason_across_family_width_tokens(img, patch, tokens, family, stream):
    """models built with the reference's constructor arguments: operator family (gelu / softmax / layernorm_type) and stream width"""
    m = vq.VisionTransformer(img_size=img, patch_size=patch, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True,
                             num_classes=10, gelu_type=family, softmax_type=family, layernorm_type=family,
                             **(WIDE if stream == 16 else {}))
    assert (img // patch) ** 2 + 1 == tokens
    reason = m.engine_unsupported_reason()
    if tokens > 1025:
        ok = False
    elif family == "ibert":
        ok = 193 <= tokens <= 207
    else:
        ok = stream == 8 or tokens <= 207
    assert (reason is None) == ok, reason
    if not ok:
        assert "tokens" in reason
    else:
        assert m._engine_widths[0] == stream


def _prototype_kinds(name):
    """the ctypes kinds of the parameters `name` is declared with in include/ivit_hip.h"""
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "int8_t*": _lib.vp, "const uint32_t*": _lib.vp, "const float*": _lib.vp, "int": _lib.ci,
             "int64_t": _lib.i64, "uint32_t": _lib.u32, "int32_t": _lib.i32, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    return [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]


def test_long_attention_prototype_matches_ctypes_table():
    assert _lib.SIGNATURES["ivit_attention_fused_i8_long"] == _prototype_kinds("ivit_attention_fused_i8_long")
    # the arguments of ivit_attention_fused_i8_compat_band, out_blocks and the stream included
    assert _lib.SIGNATURES["ivit_attention_fused_i8_long"] == _lib.SIGNATURES["ivit_attention_fused_i8_compat_band"]


ENTRIES = ATTN + ("ivit_attention_fused_i8_wide_long", "ivit_attention_fused_i8_ibert_long", "ivit_attention_cls_i8")


@pytest.mark.parametrize("name", ENTRIES)
def test_attention_prototypes_match_ctypes_table(name):
    """every exported attention entry: the header's prototype is the row _lib.call converts its arguments by"""
    assert len(ENTRIES) == len(set(ENTRIES)) == 11
    assert _lib.SIGNATURES[name] == _prototype_kinds(name)


# ----------------------------------------------------------------------------------- which entry serves which rows
S, L = "ivit_attention_fused_i8_", "_long"
# (family, softmax_bits) -> the entry per token count, written from the expressions of engine_common.attention (T > 207: long rows;
# softmax_bits given: the wide entries; I-BERT wide and long: none) and lazy._resolve_attention (I-BERT: 192 < T <= 1025) as they
# stood before attention_entry, and from the launchers' ranges (Shiftmax 1 .. 1025)
TOKENS = (1, 192, 193, 207, 208, 1025, 1026)
ENTRY_TABLE = {
    ("ivit", None): (S + "compat_band",) * 4 + (S[:-1] + L,) * 2 + (None,),
    ("ivit", 8): (S + "wide",) * 4 + (S + "wide" + L,) * 2 + (None,),
    ("ivit", 16): (S + "wide",) * 4 + (S + "wide" + L,) * 2 + (None,),
    ("ibert", None): (None, None, S + "ibert", S + "ibert", S + "ibert" + L, S + "ibert" + L, None),
    ("ibert", 8): (None, None, S + "ibert_wide", S + "ibert_wide", None, None, None),
    ("ibert", 16): (None, None, S + "ibert_wide", S + "ibert_wide", None, None, None),
}


@pytest.mark.parametrize("family,bits", sorted(ENTRY_TABLE, key=str))
def test_attention_entry_table(family, bits):
    from ivit_amd.engine_common import attention_entry
    assert tuple(attention_entry(family, T, bits) for T in TOKENS) == ENTRY_TABLE[(family, bits)]
    for name in ENTRY_TABLE[(family, bits)]:
        assert name is None or name in ENTRIES
