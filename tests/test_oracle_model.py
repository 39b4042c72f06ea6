"""Whole-model CPU oracle vs the reference's golden vectors, in both regimes:
  * power-of-two activation ranges (tests/golden/deit_tiny.npz): the plain integer algorithm;
  * ranges as calibrated (deit_tiny_natural.npz, the regime of a real checkpoint): the compat restatement, in which
    I-LayerNorm / ShiftGELU / Shiftmax see phi_s(q) = fl(fl(q*s)/s) and the LayerNorm mean follows torch's float32
    reduction order (oracle/ivit_oracle.c, second half).
and the operator-level compat known-answer vectors (compat_kat.npz), all produced by oracle/gen_golden.py from the
reference itself."""
import os

import numpy as np
import pytest

from ivit_amd import synth
from ivit_amd.checkpoint import load_synthetic_model
from oracle import oracle as orc


@pytest.fixture(scope="module")
def ckat(golden_dir):
    return np.load(os.path.join(golden_dir, "compat_kat.npz"))


def _check_model(tag, compat, n):
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    imgs = synth.make_images(meta["n_images"], meta["image_seed"])[:n]
    om = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], compat=compat)
    taps = {}
    res = om.forward(imgs, taps)
    assert np.array_equal(res["logits_int32"], z["logits_int32"][:n])
    assert np.array_equal(res["top1"], z["top1"][:n])
    if n == meta["n_images"]:
        crcs = dict(zip([str(t) for t in z["tap_names"]], z["tap_crc32"]))
        bad = [t for t in taps if t in crcs and orc.crc(taps[t]) != int(crcs[t])]
        assert not bad, bad[:5]
    return res, om


def test_oracle_deit_tiny_pow2_matches_reference():
    res, _ = _check_model("deit_tiny", False, 8)
    z = load_synthetic_model("deit_tiny")[4]
    assert np.array_equal(res["logits_f32"].view(np.int32), z["logits_f32_bits"])


def test_compat_oracle_equals_plain_oracle_at_pow2_scales():
    """phi is the identity for power-of-two scales: the compat restatement must not change anything there"""
    _check_model("deit_tiny", True, 8)


def test_compat_oracle_deit_tiny_natural_matches_reference():
    _, om = _check_model("deit_tiny_natural", True, 8)
    assert om.ln_tie_rows > 0          # the fixture does exercise rows decided by the float32 reduction order


def test_compat_oracle_deit_base_natural_matches_reference():
    """headline model, ranges as calibrated, one image (C = 768: the level-cascade branch of the reduction order)"""
    _check_model("deit_base_natural", True, 1)


def test_plain_integer_algorithm_is_not_the_reference_at_natural_scales():
    """what the compat restatement is for: without phi the logits differ (SURVEY finding 8)"""
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny_natural")
    imgs = synth.make_images(2, meta["image_seed"])
    res = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"]).forward(imgs)
    assert not np.array_equal(res["logits_int32"], z["logits_int32"][:2])
    assert not bool(meta["logits_int32_equal"])


def test_phi_table_properties():
    for p in range(-10, 3):
        assert orc.phi_is_identity(np.float32(2.0 ** p))
    assert not orc.phi_is_identity(np.float32(0.0371))
    ph = orc.phi_table(np.float32(0.0371))
    assert np.all(np.diff(ph) > 0) and np.abs(ph - np.arange(-128, 128)).max() < 1e-4


def test_compat_layernorm_kat(ckat):
    for ci in ckat["ln_cases"]:
        c = f"ln{ci}_"
        q = ckat[c + "q"].astype(np.int32)
        y, s_ln, _, ties = orc.layernorm_compat(q, ckat[c + "s"], ckat[c + "gamma"], ckat[c + "beta"])
        assert ties >= q.shape[0] // 2
        assert np.array_equal((y * s_ln).astype(np.float32).view(np.int32), ckat[c + "y_bits"]), ci
        lo, hi = ckat[c + "range"]
        s_out = orc.sym_scale(lo, hi, 8)
        m, e = orc.dyadic(s_ln, s_out)
        assert np.array_equal(orc.requant(orc.roundtrip(y, s_ln), m, e, 8), ckat[c + "q_out"]), ci


def test_compat_gelu_and_shiftmax_kat(ckat):
    for ci in ckat["gelu_cases"]:
        c = f"gelu{ci}_"
        out, _ = orc.shiftgelu_compat(ckat[c + "q"].astype(np.int32), ckat[c + "s"])
        assert np.array_equal(out, ckat[c + "out"]), ci
    for ci in ckat["sm_cases"]:
        c = f"sm{ci}_"
        assert np.array_equal(orc.shiftmax_compat(ckat[c + "q"].astype(np.int32), ckat[c + "s"]), ckat[c + "out"]), ci


def test_torch_outer_rowsum_equals_torch_on_a_transposed_view():
    """the order csrc/rowsum.h torch_outer_rowsum / ivo_torch_outer_rowsum_f32 restate IS what this torch build does for
    `x.mean(axis=2)` over a [B, L, C] view with strides (L*C, 1, L) (the Swin patch embedding): bitwise on order-sensitive data,
    for the Swin geometry (C = 96, L = 3136) and other sizes, and different from the contiguous-row order on the same numbers.
    Above 32768 elements ATen splits the columns over its threads, and a split that leaves the tail columns in a chunk narrower
    than one vector sums them in yet another order: the order depends on the thread count, so the test pins torch to the counts
    the reference's fixtures were checked with (1, 4 and 8 threads: oracle/gen_golden.py) instead of the host's default."""
    import torch
    nthreads = torch.get_num_threads()
    try:
        for nt in (1, 4, 8):
            torch.set_num_threads(nt)
            rng = np.random.default_rng(7)
            differs = 0
            for C, L in ((96, 3136), (96, 64), (192, 784), (128, 32), (48, 96), (768, 64), (1000, 32), (96, 50), (384, 196), (97, 77)):
                x = (rng.standard_normal((2, C, L)) * rng.uniform(1, 1e4, size=(2, C, 1))).astype(np.float32)
                xt = torch.from_numpy(x).transpose(1, 2)                 # [B, L, C], strides (C*L, 1, L)
                assert xt.stride(-1) != 1
                got = xt.sum(dim=2).numpy()
                rows = x.transpose(0, 2, 1).reshape(-1, C)               # the same rows, contiguous
                step = max(1, len(rows) // 400)
                idx = np.concatenate([np.arange(0, len(rows), step), np.arange(max(0, L - 40), L)])      # incl. the tail columns of image 0
                exp = np.array([orc.torch_outer_rowsum(rows[i], (i % L) >= (L // 32) * 32) for i in idx], np.float32)
                assert np.array_equal(got.reshape(-1)[idx].view(np.int32), exp.view(np.int32)), (C, L, nt)
                inner = np.array([orc.torch_rowsum(r) for r in rows[:200]], np.float32)
                differs += int((inner.view(np.int32) != got.reshape(-1)[:200].view(np.int32)).sum())
                assert np.array_equal(torch.from_numpy(rows[:200].copy()).sum(dim=1).numpy().view(np.int32), inner.view(np.int32))
            assert differs > 0
    finally:
        torch.set_num_threads(nthreads)


def test_torch_rowsum_order_is_not_plain_left_to_right():
    """the restated reduction order is observable: it differs from a sequential float32 sum on fuzzy near-integers"""
    rng = np.random.default_rng(5)
    ph = orc.phi_table(np.float32(0.0371))
    diff = 0
    for _ in range(50):
        x = ph[rng.integers(0, 256, size=768)]
        seq = np.float32(0)
        for v in x:
            seq = np.float32(seq + v)
        diff += int(orc.torch_rowsum(x) != seq)
    assert diff > 0


def test_shiftexp2d_host_table_matches_reference_softmax(ckat):
    """product host code (prepare.shiftexp2d, the table the attention kernel gathers from at natural scales) vs the
    reference module's outputs: P = floor(e * factor / 2^24) rebuilt from the table equals IVITIntSoftmax"""
    from ivit_amd.prepare import shiftexp2d
    for ci in ckat["sm_cases"]:
        c = f"sm{ci}_"
        q, s = ckat[c + "q"].astype(np.int32), np.float32(ckat[c + "s"])
        tab = shiftexp2d(s)
        e = tab[q.max(axis=1)[:, None] + 128, q + 128].astype(np.float32)
        S = np.array([orc.torch_rowsum(r) for r in e], np.float32)          # ivit_modules.py:171
        factor = np.floor((np.float32(1.0) / S) * np.float32(2147483648.0))
        P = np.floor((e * factor[:, None]).astype(np.float32) / np.float32(16777216.0)).astype(np.int32)
        assert np.array_equal(P, ckat[c + "out"]), ci


def test_compat_ln16_and_masked_shiftmax_kat(ckat):
    """Swin's natural-scale operators: I-LayerNorm on the 16-bit stream (every other row an exact tie of the mean) and
    Shiftmax behind the float shift mask, against the reference modules' outputs"""
    for ci in ckat["ln16_cases"]:
        c = f"ln16_{ci}_"
        y, s_ln, _ = orc.layernorm_scaled(ckat[c + "q"].astype(np.int32), ckat[c + "s"], ckat[c + "gamma"], ckat[c + "beta"])
        lo, hi = ckat[c + "range"]
        m, e = orc.dyadic(s_ln, orc.sym_scale(lo, hi, 8))
        assert np.array_equal(orc.requant(orc.roundtrip(y, s_ln), m, e, 8), ckat[c + "q_out"]), ci
    for ci in ckat["smm_cases"]:
        c = f"smm{ci}_"
        q, s, mask = ckat[c + "q"].astype(np.float32), np.float32(ckat[c + "s"]), ckat[c + "mask"]
        x = ((q * s).astype(np.float32) + np.where(mask, np.float32(-100.0), np.float32(0.0))).astype(np.float32)
        assert np.array_equal(orc.shiftmax_xint((x / s).astype(np.float32), s), ckat[c + "out"]), ci


def test_oracle_vit_large_matches_reference():
    """the widest factory (vit_quant.py:391-406; C = 1024, 24 blocks, 16 heads), one golden image, power-of-two ranges"""
    _check_model("vit_large", False, 1)
