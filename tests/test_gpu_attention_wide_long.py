"""ivit_attention_fused_i8_wide_long (208 .. 1025 tokens; softmax_bits = 16: Shiftmax probabilities up to 2^15 carried into P.V as
three 7-bit planes on the long kernel's row organisation) against the oracle, per (image, head): matmul -> requant ->
Shiftmax(output_bit = 16) -> int64 P.V -> requant.  Token counts on both sides of the launcher's form boundary (655 / 656), both
requantisations of the scores, the three Shiftmax regimes, both output layouts, rows whose probabilities use every plane, and a row
sum beyond 32 bits."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402
import attention_ref as A  # noqa: E402
from attention_ref import DEV, HD, KEEP as _KEEP, release, st  # noqa: E402,F401  (release: the autouse fixture)
from attention_ref import expected as _expected  # noqa: E402


def _run(qkv, s_at, ms, es, mo, eo, form, bits, blocks):
    return A.run("ivit_attention_fused_i8_wide_long", qkv, s_at, ms, es, mo, eo, form, bits, blocks)


# the flat row's probability at power-of-two scales, per token count
FLAT_POW2 = {209: 156, 256: 128, 577: 56, 656: 48, 785: 40, 1025: 28}


def _check(B, H, T, s_mult, form, blocks, bits=16):
    rng = np.random.default_rng(500 + 7 * B * H + T)
    natural = form != "pow2"
    qkv = A.inputs(rng, B, H, T)
    s_at, ms, es, mo, eo = A.scales(natural, s_mult, bits)
    exp, P, omax = _expected(qkv, s_at, ms, es, mo, eo, natural, bits)
    if bits == 16:
        # checked on the EXPECTED probabilities, before the GPU runs: a dropped 7-bit plane could not pass
        assert P[5, 17] >= 1 << 14 and P[5].sum() == P[5, 17], "query 5 is not a one-hot row"
        assert len(set(P[6].tolist())) == 1 and P[6, 0] > 0, "query 6 is not a flat row"
        if not natural and T in FLAT_POW2:
            assert P[6, 0] == FLAT_POW2[T]
        assert P.sum(axis=1).max() <= 1 << 15 and omax < 1 << 23
        planes = (P[5] & 127) | (P[6] & 127), ((P[5] >> 7) & 127) | ((P[6] >> 7) & 127), (P[5] >> 14) | (P[6] >> 14)
        if not natural and T in (256, 785):
            # P[5, 17] is 32512 / 32000 there: plane c of that row is empty, and the flat row (128 / 40) fills one plane only
            assert P[5, 17] == {256: 32512, 785: 32000}[T]
            assert planes[1].any() and planes[2].any()
        else:
            assert (P[5] & 127).any() and ((P[5] >> 7) & 127).any() and (P[5] >> 14).any(), "query 5 does not fill all three planes"
    got = _run(qkv, s_at, ms, es, mo, eo, form, bits, blocks)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"
    assert np.abs(exp).max() > 5
    assert np.array_equal(got[0, 5, :HD], exp[0, 5, :HD]) and np.abs(exp[0, 5, :HD]).max() > 20


# 655 / 656 tokens: the last token count of the 40-key-tile form and the first of the 64-tile one.  Every T sees every Shiftmax
# regime; the score multiplier (1.0: a power of two, the float32 requantisation; 1.37: float64) and the output layout rotate so
# that every regime sees both of each; B * H of 1 .. 4: several workgroups per head.
TOKENS = [209, 256, 577, 655, 656, 785, 1025]
FORMS = ["pow2", "exp2d", "band"]
CASES = [(*((2, 2), (1, 3), (1, 2), (1, 1))[(i + j) % 4], T, (1.0, 1.37)[(i + j) % 2], form, (i // 2 + j) % 2)
         for i, T in enumerate(TOKENS) for j, form in enumerate(FORMS)]
for _form in FORMS:
    assert {(c[3], c[5]) for c in CASES if c[4] == _form} == {(1.0, 0), (1.0, 1), (1.37, 0), (1.37, 1)}


@pytest.mark.parametrize("B,H,T,s_mult,form,blocks", CASES)
def test_attention_wide_long_equals_oracle(B, H, T, s_mult, form, blocks):
    _check(B, H, T, s_mult, form, blocks)


def test_attention_wide_long_one_workgroup_per_head():
    """25 x 12 heads at 209 tokens: more (image, head) pairs than CUs, so every head is one workgroup"""
    _check(25, 12, 209, 1.37, "pow2", 1)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("T", [209, 785])
def test_attention_wide_long_with_8_bits_is_the_8_bit_kernel(T, form):
    """softmax_bits = 8 through the new entry equals the oracle's 8-bit result"""
    _check(1, 2, T, 1.37, form, T == 785, bits=8)


def _probability16(e, S):
    """Shiftmax's 16-bit p of an exponent e in a row whose exponent sum is S (ivit_modules.py:171-175 with output_bit = 16): S rounded
    to float32, clamped at 2^31, factor = floor(2^31 / S), p = floor(fl32(e * factor) / 2^16)"""
    S = min(np.float32(S), np.float32(2.0 ** 31))
    factor = np.floor(np.float32(np.float32(1.0) / S) * np.float32(2.0 ** 31))
    return int(np.floor(np.float32(np.float32(e) * factor) / np.float32(2.0 ** 16)))


def test_attention_wide_long_row_sum_beyond_32_bits():
    """x0 = -520 and flat scores at 1025 tokens: every exponent is e0 = 520 * 2^15, the exact row sum 1025 * e0 exceeds 2^32 and
    clamps to 2^31 (factor 1, p16 = 260).  The sum wrapped to 32 bits is below 2^31 (factor 7, p16 = 1820): a 32-bit accumulator,
    or a lost high half in the lane reduction, changes every output of that head"""
    B, H, T = 1, 2, 1025
    rng = np.random.default_rng(7)
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, HD))), -128, 127).astype(np.int8)
    qkv[1, 0, 0] = 0                                   # head 0: every score 0
    s_a1 = np.float32(2.0 ** -4)
    s_S = np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125))
    s_at = np.float32(1.0 / 519.5)                     # floor(-1 / s) = -520
    assert np.floor(np.float32(np.float32(1.0) / s_at) * np.float32(-1.0)) == -520
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(np.float32(np.float32(2.0 ** -15) * s_a1), np.float32(2.0 ** -6))
    e0 = 520 * 2 ** 15
    exact, wrapped = T * e0, (T * e0) % 2 ** 32
    assert exact > 2 ** 32 and wrapped < 2 ** 31
    assert _probability16(e0, exact) == 260 and _probability16(e0, wrapped) == 1820
    S = orc.gemm_i8(qkv[0, 0, 0], qkv[1, 0, 0])
    P = orc.shiftmax(orc.requant(S, ms.astype(np.float64), es, 8), s_at, output_bit=16)
    assert (P == 260).all()                            # the oracle agrees: the clamped exact sum
    # the two sums give different outputs for this head: p16 = 260 against 1820 on every key
    O1 = qkv[2, 0, 0].astype(np.int64).sum(axis=0)
    r260 = orc.requant((260 * O1).reshape(1, -1).astype(np.int32), mo.astype(np.float64), eo, 8)
    r1820 = orc.requant((1820 * O1).reshape(1, -1).astype(np.int32), mo.astype(np.float64), eo, 8)
    assert not np.array_equal(r260, r1820)
    exp, _, _ = _expected(qkv, s_at, ms, es, mo, eo, False, 16)
    assert np.array_equal(exp[0, :, :HD], np.broadcast_to(r260, (T, HD)))
    got = _run(qkv, s_at, ms, es, mo, eo, "pow2", 16, 0)
    assert np.array_equal(got, exp), f"{(got != exp).sum()} of {got.size} differ"


@pytest.mark.parametrize("T,hd,bits,null,match", [(207, 64, 16, False, "unsupported geometry"), (1026, 64, 16, False, "unsupported geometry"),
                                                  (577, 32, 16, False, "unsupported geometry"), (577, 64, 12, False, "softmax_bits"),
                                                  (577, 64, 0, False, "softmax_bits"), (577, 64, 16, True, "NULL")])
def test_attention_wide_long_argument_errors(T, hd, bits, null, match):
    """every case is refused in front of the launch (csrc/attention.hip, attention_check)"""
    a = torch.zeros(3 * 1026 * 64 + 64, dtype=torch.int8, device=DEV)
    _KEEP.append(a)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_attention_fused_i8_wide_long", None if null else _lib.ptr(a), _lib.ptr(a), 1, 1, T, hd, 1 << 30, 40, 0.25, 1 << 30, 40, None, None, 0, bits, 0, st())
    with pytest.raises(_lib.IvitError, match="NULL"):
        _lib.call("ivit_attention_fused_i8_wide_long", _lib.ptr(a), None, 1, 1, 577, 64, 1 << 30, 40, 0.25, 1 << 30, 40, None, None, 0, 16, 0, st())
