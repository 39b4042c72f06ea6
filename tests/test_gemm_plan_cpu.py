"""CPU: the GEMM launcher's decision (csrc/gemm.hip gemm_plan, exported as the host function ivit_gemm_plan) against its Python
mirror (ivit_amd/gemm_forms.py), and both against the forms the shipped models ran before the rule had one home.

The callers hand the launcher the weight copy that matches the kernel it will pick, so the rule exists twice: in C, where it
launches, and in gemm_forms, where the copy is chosen.  The sweep holds the two together for every epilogue kind and every value of
the layout word; the table is the record of what DeiT-T/S/B and Swin-T/S launched at batch 1, 64 and 128, written down from the
rules as they stood in engine.py, swin_engine.py, engine_common.py and launch_gemm before gemm_forms existed."""
import ctypes as C

import pytest

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, gemm_forms as gf  # noqa: E402
from ivit_amd.gemm_forms import I32, PERS, QKV, RESID, RESID16, RQ, RQ16, RQ16_RES16, SKINNY, SMALL, WREG, WREG16  # noqa: E402,F401

SWEEP_M = (1, 16, 2047, 2048, 8191, 8192, 12723, 33200)
SWEEP_N = (16, 64, 96, 128, 192, 288, 320, 336, 384, 768, 1024, 1152)
SWEEP_K = (32, 64, 96, 128, 160, 192, 384, 768)


def plan(epi, M, N, K, layouts):
    """ivit_gemm_plan -> its eight numbers, or None where the launcher refuses (IVIT_ERR_INVALID)"""
    out = (C.c_int32 * 8)()
    rc = _lib.lib().ivit_gemm_plan(epi, M, N, K, layouts, out)
    assert rc in (0, -1), (rc, epi, M, N, K, layouts)
    return list(out) if rc == 0 else None


def test_names_match_the_header():
    """the layout bits, epilogue kinds and form numbers of gemm_forms are the header's"""
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ivit_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (IVIT_\w+) (\d+)\b", header)}
    for name in ("A_BLOCKS", "W_BLOCKS", "OUT_BLOCKS", "W_FRAGS", "W_FRAGS16"):
        assert getattr(gf, name) == defs["IVIT_" + name], name
    for name in ("RQ", "RESID", "QKV", "I32", "RESID16", "RQ16", "RQ16_RES16"):
        assert getattr(gf, name) == defs["IVIT_GEMM_EPI_" + name], name
    for name in ("SMALL", "PERS", "WREG", "WREG16", "SKINNY"):
        assert getattr(gf, name) == defs["IVIT_GEMM_FORM_" + name], name
    assert "ivit_gemm_plan" in _lib.SIGNATURES and len(_lib.SIGNATURES["ivit_gemm_plan"]) == 6


@pytest.mark.parametrize("epi", range(7))
def test_mirror_names_the_launchers_form(epi):
    """every value of the layout word (the combinations the entry accepts and the ones it refuses) x the sweep: gemm_forms.form
    and ivit_gemm_plan name the same form, or both refuse; the tile-fit rule agrees wherever the plan answers"""
    forms = set()
    for layouts in range(32):
        accepted = not (layouts & ~gf.LAYOUTS[epi] or layouts & gf.FRAGS == gf.FRAGS)
        for M in SWEEP_M:
            for N in SWEEP_N:
                for K in SWEEP_K:
                    got, want = gf.form(epi, M, N, K, layouts), plan(epi, M, N, K, layouts)
                    assert got == (None if want is None else want[0]), (epi, M, N, K, layouts, got, want)
                    assert accepted or want is None, (epi, M, N, K, layouts)
                    if want is not None:
                        forms.add(want[0])
                        assert gf.tiles_fit(N) == bool(want[7]), N
                    # the skinny-K predicate on its own, as swin_engine's weight choice reads it
                    if want is not None and not layouts:
                        assert gf.skinny_applies(epi, M, N, K) == (want[0] == gf.SKINNY), (epi, M, N, K)
    # the sweep reaches every form this epilogue has
    want_forms = {RQ: {0, 1, 2, 3, 4}, RESID: {0, 1, 2, 3}, QKV: {0, 1, 2, 3, 4}, I32: {0}, RESID16: {0, 1, 2, 3}, RQ16: {0}, RQ16_RES16: {0, 2}}
    assert forms == want_forms[epi]


def test_query_refuses_what_it_cannot_describe():
    L = _lib.lib()
    out = (C.c_int32 * 8)()
    assert L.ivit_gemm_plan(RQ, 4096, 768, 768, 0, None) == -1
    assert L.ivit_gemm_plan(7, 4096, 768, 768, 0, out) == -1 and L.ivit_gemm_plan(-1, 4096, 768, 768, 0, out) == -1
    assert L.ivit_gemm_plan(RQ, 4096, 768, 768, gf.W_BLOCKS | gf.W_FRAGS, out) == -1
    assert "fragment-packed weight needs" in L.ivit_last_error_string().decode()      # the launcher's own text
    assert L.ivit_gemm_plan(RQ, 100, 768, 768, gf.A_BLOCKS, out) == -1
    assert "block-layout operands need the persistent kernel" in L.ivit_last_error_string().decode()


# (model, batch, site, epilogue, M, N of the linear, K, fragment copy held (0 / W_FRAGS / W_FRAGS16), block copy held, caller allows
#  copies, N of the launch, layout bits of the weight, form).  DeiT: 197 tokens, K = 768 patches; the cls.* rows are the last block on
# the class rows (cls.kv: planes 1-2 of attn.qkv).  Swin-T and Swin-S differ in depth only: K is padded to 64-byte slabs (96 -> 128).
MODEL_GEMMS = [
    ("deit_tiny", 1, "patch", RQ, 196, 192, 768, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "qkv", QKV, 197, 576, 192, 16, 1, 0, 576, 0, SMALL),
    ("deit_tiny", 1, "proj", RESID, 197, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "fc1", RQ, 197, 768, 192, 16, 1, 0, 768, 0, SMALL),
    ("deit_tiny", 1, "fc2", RESID, 197, 192, 768, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "cls.kv", QKV, 197, 576, 192, 16, 1, 0, 384, 0, SMALL),
    ("deit_tiny", 1, "cls.q", RQ, 1, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "cls.proj", RESID, 1, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "cls.fc1", RQ, 1, 768, 192, 16, 1, 0, 768, 0, SMALL),
    ("deit_tiny", 1, "cls.fc2", RESID, 1, 192, 768, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 1, "head", I32, 1, 1000, 192, 0, 0, 0, 1000, 0, SMALL),
    ("deit_small", 1, "patch", RQ, 196, 384, 768, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "qkv", QKV, 197, 1152, 384, 16, 1, 0, 1152, 0, SMALL),
    ("deit_small", 1, "proj", RESID, 197, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "fc1", RQ, 197, 1536, 384, 16, 1, 0, 1536, 0, SMALL),
    ("deit_small", 1, "fc2", RESID, 197, 384, 1536, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "cls.kv", QKV, 197, 1152, 384, 16, 1, 0, 768, 0, SMALL),
    ("deit_small", 1, "cls.q", RQ, 1, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "cls.proj", RESID, 1, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "cls.fc1", RQ, 1, 1536, 384, 16, 1, 0, 1536, 0, SMALL),
    ("deit_small", 1, "cls.fc2", RESID, 1, 384, 1536, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 1, "head", I32, 1, 1000, 384, 0, 0, 0, 1000, 0, SMALL),
    ("deit_base", 1, "patch", RQ, 196, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "qkv", QKV, 197, 2304, 768, 16, 1, 0, 2304, 0, SMALL),
    ("deit_base", 1, "proj", RESID, 197, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "fc1", RQ, 197, 3072, 768, 16, 1, 0, 3072, 0, SMALL),
    ("deit_base", 1, "fc2", RESID, 197, 768, 3072, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "cls.kv", QKV, 197, 2304, 768, 16, 1, 0, 1536, 0, SMALL),
    ("deit_base", 1, "cls.q", RQ, 1, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "cls.proj", RESID, 1, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "cls.fc1", RQ, 1, 3072, 768, 16, 1, 0, 3072, 0, SMALL),
    ("deit_base", 1, "cls.fc2", RESID, 1, 768, 3072, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 1, "head", I32, 1, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
    ("swin_tiny/small", 1, "patch", RQ, 3136, 96, 64, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 1, "s0.qkv", QKV, 3136, 288, 128, 0, 1, 1, 288, 2, PERS),
    ("swin_tiny/small", 1, "s0.proj", RQ16_RES16, 3136, 96, 128, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 1, "s0.fc1", RQ, 3136, 384, 128, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 1, "s0.fc2", RESID16, 3136, 96, 384, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 1, "s0.red", RQ, 784, 192, 384, 0, 1, 1, 192, 0, SMALL),
    ("swin_tiny/small", 1, "s1.qkv", QKV, 784, 576, 192, 16, 1, 1, 576, 0, SMALL),
    ("swin_tiny/small", 1, "s1.proj", RQ16_RES16, 784, 192, 192, 0, 1, 1, 192, 0, SMALL),
    ("swin_tiny/small", 1, "s1.fc1", RQ, 784, 768, 192, 16, 1, 1, 768, 0, SMALL),
    ("swin_tiny/small", 1, "s1.fc2", RESID16, 784, 192, 768, 0, 1, 1, 192, 0, SMALL),
    ("swin_tiny/small", 1, "s1.red", RQ, 196, 384, 768, 0, 1, 1, 384, 0, SMALL),
    ("swin_tiny/small", 1, "s2.qkv", QKV, 196, 1152, 384, 16, 1, 1, 1152, 0, SMALL),
    ("swin_tiny/small", 1, "s2.proj", RQ16_RES16, 196, 384, 384, 0, 1, 1, 384, 0, SMALL),
    ("swin_tiny/small", 1, "s2.fc1", RQ, 196, 1536, 384, 16, 1, 1, 1536, 0, SMALL),
    ("swin_tiny/small", 1, "s2.fc2", RESID16, 196, 384, 1536, 0, 1, 1, 384, 0, SMALL),
    ("swin_tiny/small", 1, "s2.red", RQ, 49, 768, 1536, 16, 1, 1, 768, 0, SMALL),
    ("swin_tiny/small", 1, "s3.qkv", QKV, 49, 2304, 768, 16, 1, 1, 2304, 0, SMALL),
    ("swin_tiny/small", 1, "s3.proj", RQ16_RES16, 49, 768, 768, 8, 1, 1, 768, 0, SMALL),
    ("swin_tiny/small", 1, "s3.fc1", RQ, 49, 3072, 768, 16, 1, 1, 3072, 0, SMALL),
    ("swin_tiny/small", 1, "s3.fc2", RESID16, 49, 768, 3072, 16, 1, 1, 768, 0, SMALL),
    ("swin_tiny/small", 1, "head", I32, 1, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
    ("deit_tiny", 64, "patch", RQ, 12544, 192, 768, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 64, "qkv", QKV, 12608, 576, 192, 16, 1, 1, 576, 16, WREG16),
    ("deit_tiny", 64, "proj", RESID, 12608, 192, 192, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 64, "fc1", RQ, 12608, 768, 192, 16, 1, 1, 768, 16, WREG16),
    ("deit_tiny", 64, "fc2", RESID, 12608, 192, 768, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 64, "cls.kv", QKV, 12608, 576, 192, 16, 1, 1, 384, 16, WREG16),
    ("deit_tiny", 64, "cls.q", RQ, 64, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 64, "cls.proj", RESID, 64, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 64, "cls.fc1", RQ, 64, 768, 192, 16, 1, 0, 768, 0, SMALL),
    ("deit_tiny", 64, "cls.fc2", RESID, 64, 192, 768, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 64, "head", I32, 64, 1000, 192, 0, 0, 0, 1000, 0, SMALL),
    ("deit_small", 64, "patch", RQ, 12544, 384, 768, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 64, "qkv", QKV, 12608, 1152, 384, 16, 1, 1, 1152, 16, WREG16),
    ("deit_small", 64, "proj", RESID, 12608, 384, 384, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 64, "fc1", RQ, 12608, 1536, 384, 16, 1, 1, 1536, 16, WREG16),
    ("deit_small", 64, "fc2", RESID, 12608, 384, 1536, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 64, "cls.kv", QKV, 12608, 1152, 384, 16, 1, 1, 768, 16, WREG16),
    ("deit_small", 64, "cls.q", RQ, 64, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 64, "cls.proj", RESID, 64, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 64, "cls.fc1", RQ, 64, 1536, 384, 16, 1, 0, 1536, 0, SMALL),
    ("deit_small", 64, "cls.fc2", RESID, 64, 384, 1536, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 64, "head", I32, 64, 1000, 384, 0, 0, 0, 1000, 0, SMALL),
    ("deit_base", 64, "patch", RQ, 12544, 768, 768, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 64, "qkv", QKV, 12608, 2304, 768, 16, 1, 1, 2304, 16, WREG16),
    ("deit_base", 64, "proj", RESID, 12608, 768, 768, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 64, "fc1", RQ, 12608, 3072, 768, 16, 1, 1, 3072, 16, WREG16),
    ("deit_base", 64, "fc2", RESID, 12608, 768, 3072, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 64, "cls.kv", QKV, 12608, 2304, 768, 16, 1, 1, 1536, 16, WREG16),
    ("deit_base", 64, "cls.q", RQ, 64, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 64, "cls.proj", RESID, 64, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 64, "cls.fc1", RQ, 64, 3072, 768, 16, 1, 0, 3072, 0, SMALL),
    ("deit_base", 64, "cls.fc2", RESID, 64, 768, 3072, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 64, "head", I32, 64, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
    ("swin_tiny/small", 64, "patch", RQ, 200704, 96, 64, 0, 0, 1, 96, 0, SKINNY),
    ("swin_tiny/small", 64, "s0.qkv", QKV, 200704, 288, 128, 0, 1, 1, 288, 0, SKINNY),
    ("swin_tiny/small", 64, "s0.proj", RQ16_RES16, 200704, 96, 128, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 64, "s0.fc1", RQ, 200704, 384, 128, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 64, "s0.fc2", RESID16, 200704, 96, 384, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 64, "s0.red", RQ, 50176, 192, 384, 0, 1, 1, 192, 2, PERS),
    ("swin_tiny/small", 64, "s1.qkv", QKV, 50176, 576, 192, 16, 1, 1, 576, 16, WREG16),
    ("swin_tiny/small", 64, "s1.proj", RQ16_RES16, 50176, 192, 192, 0, 1, 1, 192, 0, SMALL),
    ("swin_tiny/small", 64, "s1.fc1", RQ, 50176, 768, 192, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 64, "s1.fc2", RESID16, 50176, 192, 768, 0, 1, 1, 192, 2, PERS),
    ("swin_tiny/small", 64, "s1.red", RQ, 12544, 384, 768, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 64, "s2.qkv", QKV, 12544, 1152, 384, 16, 1, 1, 1152, 16, WREG16),
    ("swin_tiny/small", 64, "s2.proj", RQ16_RES16, 12544, 384, 384, 0, 1, 1, 384, 0, SMALL),
    ("swin_tiny/small", 64, "s2.fc1", RQ, 12544, 1536, 384, 16, 1, 1, 1536, 16, WREG16),
    ("swin_tiny/small", 64, "s2.fc2", RESID16, 12544, 384, 1536, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 64, "s2.red", RQ, 3136, 768, 1536, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 64, "s3.qkv", QKV, 3136, 2304, 768, 16, 1, 1, 2304, 16, WREG16),
    ("swin_tiny/small", 64, "s3.proj", RQ16_RES16, 3136, 768, 768, 8, 1, 1, 768, 8, WREG),
    ("swin_tiny/small", 64, "s3.fc1", RQ, 3136, 3072, 768, 16, 1, 1, 3072, 16, WREG16),
    ("swin_tiny/small", 64, "s3.fc2", RESID16, 3136, 768, 3072, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 64, "head", I32, 64, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
    ("deit_tiny", 128, "patch", RQ, 25088, 192, 768, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 128, "qkv", QKV, 25216, 576, 192, 16, 1, 1, 576, 16, WREG16),
    ("deit_tiny", 128, "proj", RESID, 25216, 192, 192, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 128, "fc1", RQ, 25216, 768, 192, 16, 1, 1, 768, 16, WREG16),
    ("deit_tiny", 128, "fc2", RESID, 25216, 192, 768, 16, 1, 1, 192, 16, WREG16),
    ("deit_tiny", 128, "cls.kv", QKV, 25216, 576, 192, 16, 1, 1, 384, 16, WREG16),
    ("deit_tiny", 128, "cls.q", RQ, 128, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 128, "cls.proj", RESID, 128, 192, 192, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 128, "cls.fc1", RQ, 128, 768, 192, 16, 1, 0, 768, 0, SMALL),
    ("deit_tiny", 128, "cls.fc2", RESID, 128, 192, 768, 16, 1, 0, 192, 0, SMALL),
    ("deit_tiny", 128, "head", I32, 128, 1000, 192, 0, 0, 0, 1000, 0, SMALL),
    ("deit_small", 128, "patch", RQ, 25088, 384, 768, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 128, "qkv", QKV, 25216, 1152, 384, 16, 1, 1, 1152, 16, WREG16),
    ("deit_small", 128, "proj", RESID, 25216, 384, 384, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 128, "fc1", RQ, 25216, 1536, 384, 16, 1, 1, 1536, 16, WREG16),
    ("deit_small", 128, "fc2", RESID, 25216, 384, 1536, 16, 1, 1, 384, 16, WREG16),
    ("deit_small", 128, "cls.kv", QKV, 25216, 1152, 384, 16, 1, 1, 768, 16, WREG16),
    ("deit_small", 128, "cls.q", RQ, 128, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 128, "cls.proj", RESID, 128, 384, 384, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 128, "cls.fc1", RQ, 128, 1536, 384, 16, 1, 0, 1536, 0, SMALL),
    ("deit_small", 128, "cls.fc2", RESID, 128, 384, 1536, 16, 1, 0, 384, 0, SMALL),
    ("deit_small", 128, "head", I32, 128, 1000, 384, 0, 0, 0, 1000, 0, SMALL),
    ("deit_base", 128, "patch", RQ, 25088, 768, 768, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 128, "qkv", QKV, 25216, 2304, 768, 16, 1, 1, 2304, 16, WREG16),
    ("deit_base", 128, "proj", RESID, 25216, 768, 768, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 128, "fc1", RQ, 25216, 3072, 768, 16, 1, 1, 3072, 16, WREG16),
    ("deit_base", 128, "fc2", RESID, 25216, 768, 3072, 16, 1, 1, 768, 16, WREG16),
    ("deit_base", 128, "cls.kv", QKV, 25216, 2304, 768, 16, 1, 1, 1536, 16, WREG16),
    ("deit_base", 128, "cls.q", RQ, 128, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 128, "cls.proj", RESID, 128, 768, 768, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 128, "cls.fc1", RQ, 128, 3072, 768, 16, 1, 0, 3072, 0, SMALL),
    ("deit_base", 128, "cls.fc2", RESID, 128, 768, 3072, 16, 1, 0, 768, 0, SMALL),
    ("deit_base", 128, "head", I32, 128, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
    ("swin_tiny/small", 128, "patch", RQ, 401408, 96, 64, 0, 0, 1, 96, 0, SKINNY),
    ("swin_tiny/small", 128, "s0.qkv", QKV, 401408, 288, 128, 0, 1, 1, 288, 0, SKINNY),
    ("swin_tiny/small", 128, "s0.proj", RQ16_RES16, 401408, 96, 128, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 128, "s0.fc1", RQ, 401408, 384, 128, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 128, "s0.fc2", RESID16, 401408, 96, 384, 0, 0, 1, 96, 0, SMALL),
    ("swin_tiny/small", 128, "s0.red", RQ, 100352, 192, 384, 0, 1, 1, 192, 2, PERS),
    ("swin_tiny/small", 128, "s1.qkv", QKV, 100352, 576, 192, 16, 1, 1, 576, 16, WREG16),
    ("swin_tiny/small", 128, "s1.proj", RQ16_RES16, 100352, 192, 192, 0, 1, 1, 192, 0, SMALL),
    ("swin_tiny/small", 128, "s1.fc1", RQ, 100352, 768, 192, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 128, "s1.fc2", RESID16, 100352, 192, 768, 0, 1, 1, 192, 2, PERS),
    ("swin_tiny/small", 128, "s1.red", RQ, 25088, 384, 768, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 128, "s2.qkv", QKV, 25088, 1152, 384, 16, 1, 1, 1152, 16, WREG16),
    ("swin_tiny/small", 128, "s2.proj", RQ16_RES16, 25088, 384, 384, 0, 1, 1, 384, 0, SMALL),
    ("swin_tiny/small", 128, "s2.fc1", RQ, 25088, 1536, 384, 16, 1, 1, 1536, 16, WREG16),
    ("swin_tiny/small", 128, "s2.fc2", RESID16, 25088, 384, 1536, 0, 1, 1, 384, 2, PERS),
    ("swin_tiny/small", 128, "s2.red", RQ, 6272, 768, 1536, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 128, "s3.qkv", QKV, 6272, 2304, 768, 16, 1, 1, 2304, 16, WREG16),
    ("swin_tiny/small", 128, "s3.proj", RQ16_RES16, 6272, 768, 768, 8, 1, 1, 768, 8, WREG),
    ("swin_tiny/small", 128, "s3.fc1", RQ, 6272, 3072, 768, 16, 1, 1, 3072, 16, WREG16),
    ("swin_tiny/small", 128, "s3.fc2", RESID16, 6272, 768, 3072, 16, 1, 1, 768, 16, WREG16),
    ("swin_tiny/small", 128, "head", I32, 128, 1000, 768, 0, 0, 0, 1000, 0, SMALL),
]


def _lin(N, K, wf, wb):
    """a linear's copies as gemm_forms.weight reads them; the tensors are stand-ins"""
    return dict(N=N, K=K, W="W", Wf="Wf" if wf else None, Wf_bit=wf or None, Wb="Wb" if wb else None)


def test_shipped_models_keep_their_forms():
    """every GEMM of DeiT-T/S/B and Swin-T/S at batch 1, 64, 128: the weight copy gemm_forms.weight picks carries the layout bits the
    engines used to pick, and mirror and launcher run it in the form it used to run in"""
    assert len(MODEL_GEMMS) == 162 and {r[-1] for r in MODEL_GEMMS} == {SMALL, PERS, WREG, WREG16, SKINNY}
    for (model, B, site, epi, M, N, K, wf, wb, allow, nl, lay, form) in MODEL_GEMMS:
        what = (model, B, site)
        W, bits = gf.weight(_lin(N, K, wf, wb), epi, M, frags=bool(allow), blocks=bool(allow))
        assert bits == lay and W == {0: "W", gf.W_BLOCKS: "Wb"}.get(bits, "Wf"), what
        assert gf.form(epi, M, nl, K, bits) == form, what
        assert plan(epi, M, nl, K, bits)[0] == form, what
        # the copies themselves exist where the parent's conditions made them
        assert gf.blocks_shape(N, K) == bool(wb) and (not wf or gf.frags_shape(N, K)), what
    # engine_common.frag_copy's tile rule at the widths of these models: 256-channel tiles fit 768, 1152, 1536, 2304 and 3072
    # channels and not 192, 384 and 576, which only the 128-channel items of the 16x16x64 order with an int8 epilogue take
    assert [n for n in (192, 384, 576, 768, 1152, 1536, 2304, 3072) if gf.tiles_fit(n)] == [768, 1152, 1536, 2304, 3072]
    assert gf.frag_items_ok(gf.W_FRAGS16, True, 384) and not gf.frag_items_ok(gf.W_FRAGS16, False, 384)
    assert not gf.frag_items_ok(gf.W_FRAGS, True, 384) and gf.frag_items_ok(gf.W_FRAGS, False, 768)
