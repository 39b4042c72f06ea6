"""ivit_attention_fused_i8_wide (softmax_bits = 16: Shiftmax probabilities up to 2^15 carried into P.V as three 7-bit planes) against
the oracle, per (image, head): matmul -> requant -> Shiftmax(output_bit = 16) -> int64 P.V -> requant.  Token counts of the tuned
form (193 .. 208) and of the general one, both requantisations of the scores, the three Shiftmax regimes, both output layouts, and
rows whose probabilities use every plane."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic, shiftexp2d, shiftexp_band  # noqa: E402

DEV = "cuda:0"
HD = 64
SENTINEL = 99
_KEEP = []  # device tensors whose raw pointers were handed to the C ABI stay alive until the test's final synchronize


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


@functools.lru_cache(maxsize=None)
def _tables(s_at):
    tab = shiftexp2d(np.float32(s_at))
    bt, bw = shiftexp_band(tab)
    assert 16 <= bw <= 256
    return tab, bt, bw


def _block_valid(rows, K):
    """True at the bytes of the block-layout buffer that hold an element of a [rows, K] operand (include/ivit_hip.h:
    IVIT_LAYOUT_BLOCKS), False at the padding rows of the last 16-row block"""
    r = np.arange((rows + 15) // 16 * 16)[:, None]
    k = np.arange(K)[None, :]
    c = (k % 64) // 16
    off = ((r // 16) * (K // 64) + k // 64) * 1024 + (4 * (r % 16) + (c ^ (((r % 16) >> 2) & 3))) * 16 + k % 16
    v = np.zeros(off.size, bool)
    v[off[:rows].reshape(-1)] = True
    assert v.sum() == rows * K
    return v


def _scales(natural, s_mult, bits):
    s_a1 = np.float32(0.0571 if natural else 2.0 ** -4)
    s_S = np.float32(np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125)) * np.float32(s_mult))
    s_at = np.float32(0.0437 if natural else 2.0 ** -3)
    s_pv = np.float32(np.float32(2.0 ** -(bits - 1)) * s_a1)          # Shiftmax output scale 2^-(bits-1) times the scale of V
    s_a2 = np.float32(0.1173 if natural else 2.0 ** -3)
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(s_pv, s_a2)
    return s_at, ms, es, mo, eo


def _inputs(rng, B, H, T):
    """random q, k, v; in (image 0, head 0) query 5 sees key 17 at +127 and every other key at -128 after the requantisation (a
    one-hot row), query 6 sees every key at 0 (a flat row); V is -128 on the dominant key"""
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, HD))), -128, 127).astype(np.int8)
    if T > 17:
        qkv[0, 0, 0, 5] = 0
        qkv[0, 0, 0, 5, :8] = 127
        qkv[1, 0, 0, :, :8] = -127
        qkv[1, 0, 0, 17, :8] = 127
        qkv[0, 0, 0, 6] = 0
        qkv[2, 0, 0, 17] = -128
    return qkv


def _expected(qkv, s_at, ms, es, mo, eo, natural, bits):
    _, B, H, T, _ = qkv.shape
    exp = np.empty((B, T, H * HD), np.int32)
    P00 = None
    for b in range(B):
        for h in range(H):
            S = orc.gemm_i8(qkv[0, b, h], qkv[1, b, h])
            ka = orc.requant(S, ms.astype(np.float64), es, 8)
            P = (orc.shiftmax_compat if natural else orc.shiftmax)(ka, s_at, output_bit=bits)
            assert P.min() >= 0 and P.max() <= 1 << (bits - 1)
            O = P.astype(np.int64) @ qkv[2, b, h].astype(np.int64)
            assert np.abs(O).max() < 2 ** 31
            exp[b, :, h * HD:(h + 1) * HD] = orc.requant(O.astype(np.int32), mo.astype(np.float64), eo, 8)
            if b == 0 and h == 0:
                P00 = P
    return exp, P00


def _run(name, qkv, s_at, ms, es, mo, eo, form, bits, blocks):
    """-> (row-major result [B, T, C], the raw output buffer as written)"""
    _, B, H, T, _ = qkv.shape
    M, C = B * T, H * HD
    exp2d, band, bw = None, None, 0
    if form != "pow2":
        tab, bt, bw_ = _tables(float(s_at))
        if form == "band":
            band, bw = dev(bt.view(np.int32)), bw_
        else:
            exp2d = dev(tab.view(np.int32))
    rows = (M + 15) // 16 * 16 if blocks else M
    out = torch.full((rows * C + 64,), SENTINEL, dtype=torch.int8, device=DEV)      # 64 guard bytes behind the buffer
    _KEEP.append(out)
    args = [_lib.ptr(dev(qkv)), _lib.ptr(out), B, H, T, HD, int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0]), _lib.ptr(exp2d),
            _lib.ptr(band), bw]
    if name == "ivit_attention_fused_i8_wide":
        args.append(bits)
    _lib.call(name, *args, int(blocks), st())
    rm = out[:M * C]
    if blocks:
        rm = torch.full((M * C,), SENTINEL, dtype=torch.int8, device=DEV)
        _KEEP.append(rm)
        _lib.call("ivit_untile_operand_i8", _lib.ptr(out), M, C, _lib.ptr(rm), C, st())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[rows * C:] == SENTINEL).all(), "bytes behind the output buffer were written"
    if blocks:
        assert (raw[:rows * C][~_block_valid(M, C)] == SENTINEL).all(), "padding rows of the last block were written"
    return rm.cpu().numpy().astype(np.int32).reshape(B, T, C)


def _check(B, H, T, s_mult, form, blocks, bits=16, name="ivit_attention_fused_i8_wide"):
    rng = np.random.default_rng(500 + 7 * B * H + T)
    natural = form != "pow2"
    qkv = _inputs(rng, B, H, T)
    s_at, ms, es, mo, eo = _scales(natural, s_mult, bits)
    if not natural:
        assert ((int(ms[0]) & (int(ms[0]) - 1)) == 0) == (s_mult == 1.0)
    exp, P = _expected(qkv, s_at, ms, es, mo, eo, natural, bits)
    if T > 17 and bits == 16:
        # checked on the EXPECTED probabilities, before the GPU runs: a dropped 7-bit plane could not pass
        assert P[5, 17] >= 1 << 14 and P[5].sum() - P[5, 17] < 64, "query 5 is not a one-hot row"
        assert len(set(P[6].tolist())) == 1 and P[6, 0] > 0, "query 6 is not a flat row"
        for plane in (P[5] & 127, (P[5] >> 7) & 127, P[5] >> 14):
            assert plane.any()
        assert ((P[6] >> 7) & 127).any()
    got = _run(name, qkv, s_at, ms, es, mo, eo, form, bits, blocks)
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
    """every case is refused in front of the launch (csrc/attention.hip, ivit_attention_fused_i8_wide)"""
    a = torch.zeros(3 * 209 * 64 + 64, dtype=torch.int8, device=DEV)
    _KEEP.append(a)
    with pytest.raises(_lib.IvitError, match=match):
        _lib.call("ivit_attention_fused_i8_wide", None if null else _lib.ptr(a), _lib.ptr(a), 1, 1, T, hd, 1 << 30, 40, 0.25, 1 << 30, 40,
                  None, None, 0, bits, 0, st())
    with pytest.raises(_lib.IvitError, match="NULL"):
        _lib.call("ivit_attention_fused_i8_wide", _lib.ptr(a), None, 1, 1, 197, 64, 1 << 30, 40, 0.25, 1 << 30, 40, None, None, 0, 16, 0, st())
