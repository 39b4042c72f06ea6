"""IntSwinEngine with the I-BERT operators, on the host (the native library stubbed as in tests/test_engine_launch_trace.py): the
default family issues exactly the launches of an engine built without the argument; what the I-BERT engine launches; what
swin_engine.engine_from_model refuses, and why; the new LayerNorm entry's prototype against its binding."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.swin_engine import IntSwinEngine, engine_from_model, operator_family  # noqa: E402

from test_engine_launch_trace import Canon, _lines, stubbed  # noqa: E402, F401  (the recorder that stands in for _lib.call)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "swin_ibert_small.npz")
WIN = "ivit_ibert_layernorm_i16_i8_win"
EX = "ivit_ibert_layernorm_i16_i8_ex"
SMALL = dict(img_size=56, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2), num_heads=(3, 6), num_classes=10)
IBERT = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")


def fixture_state():
    """the model of tests/golden/swin_ibert_small.npz: seeded weights, the ranges the reference calibrated, its LayerNorm shifts"""
    z = np.load(GOLDEN, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = synth.SWIN_CONFIGS[meta["config"]]
    fs = synth.make_swin_float_state(meta["config"], meta["weight_seed"])
    ranges = {str(n): (float(lo), float(hi)) for n, (lo, hi) in zip(z["range_names"], z["ranges"])}
    shifts = {str(n) + ".shift": np.array([sh], np.float32) for n, sh in zip(z["shift_names"], z["shifts"])}
    args = (cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window"])
    return fs, ranges, shifts, args, dict(device="cpu", max_batch=2, img_size=meta["img_size"])


def trace(calls, make, taps):
    """the canonical lines (name and every argument) of building an engine and of one forward of two images"""
    del calls[:]
    eng = make()
    built = _lines(calls, Canon(eng, {}))
    x = torch.zeros(2, 3, eng.img_size, eng.img_size, dtype=torch.float32)
    del calls[:]
    eng.forward(x, taps={} if taps else None)
    return built, _lines(calls, Canon(eng, dict(images=x))), [name for name, _ in calls], eng


@pytest.mark.parametrize("taps", [False, True], ids=["fused", "taps"])
def test_default_family_is_todays_engine(stubbed, taps):      # noqa: F811
    fs, ranges, _, args, kw = fixture_state()
    a = trace(stubbed, lambda: IntSwinEngine(fs, ranges, *args, **kw), taps)
    b = trace(stubbed, lambda: IntSwinEngine(fs, ranges, *args, family="ivit", int_sqrt=False, **kw), taps)
    assert a[0] == b[0] and a[1] == b[1] and len(a[1]) > 40
    assert b[3].family == "ivit" and not [n for n in a[2] if "ibert" in n]


@pytest.mark.parametrize("int_sqrt", [False, True], ids=["float_sqrt", "int_sqrt"])
def test_ibert_engine_launches(stubbed, int_sqrt):      # noqa: F811
    fs, ranges, shifts, args, kw = fixture_state()
    depths = args[1]
    nblk = sum(depths)
    built, _, names, eng = trace(stubbed, lambda: IntSwinEngine({**fs, **shifts}, ranges, *args, family="ibert", int_sqrt=int_sqrt, **kw), False)
    build_names = [ln.split("(")[0] for ln in built]
    both = build_names + names
    assert names.count("ivit_window_attention_i8_ibert") == nblk
    assert not [n for n in both if n.startswith("ivit_window_attention_i8") and n != "ivit_window_attention_i8_ibert"]
    assert not [n for n in both if n == "ivit_window_rows" or "shiftmax" in n or n.startswith("ivit_shiftgelu_build")]
    assert names.count(WIN) == nblk and names.count(EX) == nblk + len(depths) and names.count("ivit_ibert_layernorm_i8") == 1
    assert not [n for n in names if n.startswith("ivit_layernorm")]
    assert build_names.count("ivit_ibert_gelu_build_lut") == nblk == build_names.count("ivit_ibert_softmax_build_table")
    assert names.count("ivit_gemm_i8_requant_i16_residual_i16_ex") == nblk
    # two images: 392 rows at stage 0, below the 2048 of the fragment weight copy -- fc1, then the table kernel
    assert names.count("ivit_shiftgelu_lut_i8") == nblk and "ivit_gemm_i8_requant_lut_ex" not in names
    flag = 0x100 if int_sqrt else 0
    sigs = _lib.SIGNATURES
    wins = [a for n, a in stubbed if n == WIN]
    geo = [a[13:17] for a in wins]
    assert geo == [(14, 14, 7, 0), (14, 14, 7, 3), (7, 7, 7, 0), (7, 7, 7, 0)], geo
    assert all(len(a) == len(sigs[WIN]) and a[12] & 0x100 == flag and a[12] & ~0x101 == 0 for a in wins)
    assert [a[11] for a in wins] == [128, 128, 192, 192]                            # ldo = _pad64(C): the engine's `h` buffer
    assert all(len(a) == len(sigs[EX]) and a[12] & 0x100 == flag for n, a in stubbed if n == EX)
    ln8 = [a for n, a in stubbed if n == "ivit_ibert_layernorm_i8"][0]
    assert ln8[12] & 0x100 == flag
    # the LayerNorm shifts of the fixture reach the launches: 2^shift of each module, in launch order
    want = [2.0 ** float(shifts[f"layers.{li}.blocks.{bi}.norm1.shift"][0]) for li, d in enumerate(depths) for bi in range(d)]
    assert [a[7] for a in wins] == want
    # the attention output goes to its image rows (image_order = 1) in front of the one residual GEMM
    att = [a for n, a in stubbed if n == "ivit_window_attention_i8_ibert"]
    assert all(len(a) == len(sigs["ivit_window_attention_i8_ibert"]) and a[-2] == 1 for a in att)
    del stubbed[:]
    eng.forward(torch.zeros(2, 3, 56, 56), taps={})
    assert all(a[-2] == 0 for n, a in stubbed if n == "ivit_window_attention_i8_ibert")       # taps: window order


def test_missing_shift_is_shift_zero(stubbed):      # noqa: F811
    fs, ranges, _, args, kw = fixture_state()
    IntSwinEngine(fs, ranges, *args, family="ibert", **kw).forward(torch.zeros(1, 3, 56, 56))
    assert {a[7] for n, a in stubbed if n in (WIN, EX, "ivit_ibert_layernorm_i8")} == {1.0}


def test_int_sqrt_and_family_arguments(stubbed):      # noqa: F811
    fs, ranges, _, args, kw = fixture_state()
    with pytest.raises(ValueError, match="int_sqrt"):
        IntSwinEngine(fs, ranges, *args, int_sqrt=True, **kw)
    with pytest.raises(ValueError, match="int_sqrt"):
        IntSwinEngine(fs, ranges, *args, family="ivit", int_sqrt=True, **kw)
    with pytest.raises(ValueError, match="operator family 'ppoly'"):
        IntSwinEngine(fs, ranges, *args, family="ppoly", **kw)
    assert not stubbed                                                             # refused before anything is launched
    no_act = {k: v for k, v in ranges.items() if not k.endswith("log_int_softmax.act")}
    with pytest.raises(KeyError, match="log_int_softmax.act"):
        IntSwinEngine(fs, no_act, *args, family="ibert", **kw)


def test_the_softmax_range_name_is_the_models():
    m = ivit.SwinTransformer(**IBERT, **SMALL)
    assert "layers.0.blocks.1.attn.log_int_softmax.act" in m.ranges() and int(m.layers[0].blocks[1].attn.log_int_softmax.act.activation_bit) == 16
    assert "layers.1.blocks.0.norm1.shift" in m.state_dict() and "patch_embed.norm.shift" in m.state_dict()


def test_engine_from_model_refuses_with_the_reason():
    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            engine_from_model(ivit.SwinTransformer(**{**SMALL, **kw}), device="cpu")
    refused(r"operator family \('ibert', 'ivit', 'ivit'\)", gelu_type="ibert")
    refused(r"operator family \('ivit', 'ibert', 'ibert'\)", softmax_type="ibert", layernorm_type="ibert")
    refused("layernorm parameter overflow_handling=False of 'ibert'", **{**IBERT, "layernorm_type": "ibert_overflow-handling_false"})
    refused("absolute position embedding", ape=True, **IBERT)
    refused("absolute position embedding / no patch norm", patch_norm=False, **IBERT)
    refused(r"geometry: 14x14 windows \(196 tokens", img_size=448, window_size=14, **IBERT)
    m = ivit.SwinTransformer(**IBERT, **SMALL)
    m.layers[0].blocks[0].attn.qact3.activation_bit = 16
    with pytest.raises(ValueError, match="QuantAct layers.0.blocks.0.attn.qact3 is 16-bit"):
        engine_from_model(m, device="cpu")
    with pytest.raises(ValueError, match="not frozen"):
        engine_from_model(ivit.SwinTransformer(**IBERT, **SMALL), device="cpu")
    # the families it takes, and that model(x)'s own dispatch still refuses the I-BERT one
    assert operator_family(ivit.SwinTransformer(**SMALL)) == ("ivit", False)
    assert operator_family(ivit.SwinTransformer(**IBERT, **SMALL)) == ("ibert", False)
    isq = ivit.SwinTransformer(**{**SMALL, **IBERT, "layernorm_type": "ibert_use-int-sqrt_true"})
    assert operator_family(isq) == ("ibert", True) and isq.engine_structure_reason() is None
    assert "operator family" in isq.engine_unsupported_reason()


def test_new_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    kinds = lambda prm: (ctypes.c_void_p if "*" in prm or prm.startswith("ivit_stream_t") else ctypes.c_float if prm.startswith("float") else      # noqa: E731
                         ctypes.c_int64 if prm.startswith("int64_t") else ctypes.c_uint32 if prm.startswith("uint32_t") else ctypes.c_int)
    protos = {}
    for name in (WIN, EX):
        decl = re.search(r"int " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared in include/ivit_hip.h"
        protos[name] = [prm.strip() for prm in decl.group(1).replace("\n", " ").split(",")]
        assert _lib.SIGNATURES[name] == [kinds(prm) for prm in protos[name]], name
    # the _ex entry's arguments, then int H, int W, int ws, int shift in front of the stream
    assert protos[WIN] == protos[EX][:-1] + ["int H", "int W", "int ws", "int shift", protos[EX][-1]]
    assert "IVIT_ERR_UNSUPPORTED" in header[header.index("ivit_ibert_layernorm_i16_i8_ex with the rows of"):header.index("int " + WIN)]
    if os.path.exists(_lib.LIB_PATH):          # built trees: the product and the lab library export it
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), WIN) and hasattr(ctypes.CDLL(_lib.LAB_PATH), WIN)
        assert getattr(_lib.lib(), WIN).argtypes == _lib.SIGNATURES[WIN]
