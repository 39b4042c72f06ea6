"""ivit_attention_fused_i8_wide (softmax_bits = 16: Shiftmax probabilities up to 2^15 carried into P.V as three 7-bit planes) against
the oracle, per (image, head): matmul -> requant -> Shiftmax(output_bit = 16) -> int64 P.V -> requant.  Token counts of the tuned
form (193 .. 208) and of the general one, both requantisations of the scores, the three Shiftmax regimes, both output layouts, and
rows whose probabilities use every plane."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
import attention_ref as A  # noqa: E402
from attention_ref import DEV, HD, KEEP as _KEEP, release, st  # noqa: E402,F401  (release: the autouse fixture)


def _check(B, H, T, s_mult, form, blocks, bits=16, name="ivit_attention_fused_i8_wide"):
    rng = np.random.default_rng(500 + 7 * B * H + T)
    natural = form != "pow2"
    qkv = A.inputs(rng, B, H, T)
    s_at, ms, es, mo, eo = A.scales(natural, s_mult, bits)
    exp, P, _ = A.expected(qkv, s_at, ms, es, mo, eo, natural, bits)
    if T > 17 and bits == 16:
        # checked on the EXPECTED probabilities, before the GPU runs: a dropped 7-bit plane could not pass
        assert P[5, 17] >= 1 << 14 and P[5].sum() - P[5, 17] < 64, "query 5 is not a one-hot row"
        assert len(set(P[6].tolist())) == 1 and P[6, 0] > 0, "query 6 is not a flat row"
        for plane in (P[5] & 127, (P[5] >> 7) & 127, P[5] >> 14):
            assert plane.any()
        assert ((P[6] >> 7) & 127).any()
    got = A.run(name, qkv, s_at, ms, es, mo, eo, form, bits, blocks)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"
    assert np.abs(exp).max() > 5
    if T > 17:
        assert np.array_equal(got[0, 5, :HD], exp[0, 5, :HD]) and np.abs(exp[0, 5, :HD]).max() > 20


# tokens 193 .. 208: the tuned form (only the last key tile is partial); fewer: the general form
@pytest.mark.parametrize("blocks", [0, 1], ids=["rows", "blocks"])
@pytest.mark.parametrize("form", ["pow2", "exp2d", "band"])
@pytest.mark.parametrize("s_mult", [1.0, 1.37], ids=["pow2_score_multiplier", "odd_score_multiplier"])
@pytest.mark.parametrize("T", [197, 193, 208, 145, 50, 17, 5])
def test_attention_wide_equals_oracle(T, s_mult, form, blocks):
    B, H = ((2, 3), (1, 2), (3, 1))[T % 3]
    _check(B, H, T, s_mult, form, blocks)


@pytest.mark.parametrize("B,H,T,s_mult,form,blocks", [(22, 12, 197, 1.37, "band", 1), (43, 6, 197, 1.0, "pow2", 0),
                                                      (64, 4, 50, 1.37, "exp2d", 0), (16, 16, 145, 1.0, "band", 1)])
def test_attention_wide_many_heads(B, H, T, s_mult, form, blocks):
    """B * H >= 256: more (image, head) pairs than one wave of workgroups"""
    assert B * H >= 256
    _check(B, H, T, s_mult, form, blocks)


@pytest.mark.parametrize("form", ["pow2", "exp2d", "band"])
@pytest.mark.parametrize("T", [197, 145, 5])
def test_attention_wide_with_8_bits_is_the_8_bit_entry(T, form):
    """softmax_bits = 8 through _wide and ivit_attention_fused_i8_compat_band: both equal the oracle's 8-bit result"""
    for name in ("ivit_attention_fused_i8_wide", "ivit_attention_fused_i8_compat_band"):
        _check(2, 2, T, 1.37, form, 0, bits=8, name=name)


@pytest.mark.parametrize("T,hd,bits,null,match", [(197, 64, 12, False, "softmax_bits"), (197, 64, 0, False, "softmax_bits"),
                                                  (197, 64, 32, False, "softmax_bits"), (209, 64, 16, False, "unsupported geometry"),
                                                  (0, 64, 16, False, "unsupported geometry"), (197, 32, 16, False, "unsupported geometry"),
                                                  (197, 64, 16, True, "NULL")])
def test_attention_wide_argument_errors(T, hd, bits, null, match):
    """every case is refused in front of the launch (csrc/attention.hip, attention_check)"""
    a = torch.zeros(3 * 209 * 64 + 64, dtype=torch.int8, device=DEV)
    _KEEP.append(a)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_attention_fused_i8_wide", None if null else _lib.ptr(a), _lib.ptr(a), 1, 1, T, hd, 1 << 30, 40, 0.25, 1 << 30, 40,
                  None, None, 0, bits, 0, st())
    with pytest.raises(_lib.IvitError, match="NULL"):
        _lib.call("ivit_attention_fused_i8_wide", _lib.ptr(a), None, 1, 1, 197, 64, 1 << 30, 40, 0.25, 1 << 30, 40, None, None, 0, 16, 0, st())
