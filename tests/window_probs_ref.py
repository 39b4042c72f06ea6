"""The softmax probabilities of Swin's window attention (swin_quant.py, WindowAttention.forward :121-169) as a numpy specification,
for both operator families: what ivit_window_attention_probs_u8 / _ibert must write, byte for byte.

Built from the oracle alone: oracle.gemm_i8 (scores), oracle.requant (qact_attn1; qact2 in its two-operand form with the 8-bit bias
table as the identity), then on the float view the reference's tensor holds -- fl(q * s), minus 100 under the shift mask --
  Shiftmax: oracle.shiftmax (power-of-two scale, no mask), oracle.shiftmax_compat (natural scale, no mask), oracle.shiftmax_xint
            (any scale, with the mask) -- the three agree where more than one applies (tests/test_window_probs_cpu.py);
  I-BERT:   oracle/ibert.py's softmax line by line with its row sum in torch's CPU order (oracle.torch_rowsum).
No GPU.  `problem()` makes the inputs the tests share: random windows, one window with one-hot and near-flat rows."""
import numpy as np

from oracle import ibert as ib
from oracle import oracle as orc

f32 = np.float32
HD = 32


def scores(qkv, bias, s_S, s_at, s_A, s_tab):
    """qkv int8 [3, nwin, nH, N, 32]; bias: the 8-bit relative position bias [nH, N, N] at scale s_tab -> ka int32 [nwin, nH, N, N],
    the output of attn.qact2 (query, key)"""
    _, nwin, nH, N, _ = qkv.shape
    S = np.empty((nwin, nH, N, N), np.int32)
    for w in range(nwin):
        for h in range(nH):
            S[w, h] = orc.gemm_i8(np.ascontiguousarray(qkv[0, w, h]), np.ascontiguousarray(qkv[1, w, h]))      # Q . K^T
    kS = orc.requant(S, *orc.dyadic(s_S, s_at), 8)                                               # qact_attn1
    b = np.ascontiguousarray(np.broadcast_to(bias[None], S.shape)).astype(np.int32)
    return orc.requant(kS, *orc.dyadic(s_at, s_A), 8, b, *orc.dyadic(s_tab, s_A))               # qact2, the bias as identity


def masked_pairs(region, nwin, nW):
    """region uint8 [nW, N] (or None) -> bool [nwin, 1, N, N]: key under the shift mask for that query (swin_quant.py:223-249)"""
    if region is None:
        return None
    reg = region[np.arange(nwin) % nW]
    return reg[:, None, :, None] != reg[:, None, None, :]


def float_view(ka, s_A, masked):
    """the tensor the softmax module receives: fl(q * s), and fl(fl(q * s) - 100) under the mask (:149-156)"""
    x = (ka.astype(f32) * f32(s_A)).astype(f32)
    if masked is not None:
        x = np.where(masked, (x + f32(-100.0)).astype(f32), x)
    return x


def shiftmax_probs(ka, s_A, masked):
    """-> int32 [nwin, nH, N, N] in [0, 127]"""
    s_A = f32(s_A)
    if masked is None:
        return (orc.shiftmax if orc.phi_is_identity(s_A) else orc.shiftmax_compat)(ka, s_A)
    return orc.shiftmax_xint((float_view(ka, s_A, masked) / s_A).astype(f32), s_A)


def ibert_probs(ka, s_A, masked, act_range):
    """oracle/ibert.py softmax (:303-314, output_bit 8) on the float view, row sums in torch's order -> int64 in [0, 128]"""
    s = f32(s_A)
    n = 30
    x0_int, b_int, c_int, exp_sf, act_sf, m, e = ib.softmax_constants(s, *act_range)
    x_int = (float_view(ka, s, masked) / s).astype(f32)
    x_int = (x_int - x_int.max(axis=-1, keepdims=True)).astype(f32)
    x_int = np.maximum(x_int, f32(n * x0_int)).astype(f32)
    q = np.floor((x_int / x0_int).astype(f32))
    r = (x_int - (x0_int * q).astype(f32)).astype(f32)
    z = ((r * (r + b_int).astype(f32)).astype(f32) + c_int).astype(f32)
    ex = np.maximum(np.floor((z * np.exp2((n - q).astype(f32)).astype(f32)).astype(f32)), f32(0))
    z_int = np.rint((ex / exp_sf).astype(f32))
    q16 = np.clip(np.rint(z_int.astype(np.float64) * m / 2.0 ** e), -32768, 32767).astype(f32)
    exp_int = ((q16 * act_sf).astype(f32) / act_sf).astype(f32)
    flat = exp_int.reshape(-1, exp_int.shape[-1])
    ssum = np.array([orc.torch_rowsum(row) for row in flat], f32).reshape(*exp_int.shape[:-1], 1)
    factor = np.floor((f32(2 ** 32) / ssum).astype(f32))
    return np.floor(((exp_int * factor).astype(f32) / f32(2 ** 25)).astype(f32)).astype(np.int64)


def probs(family, qkv, bias, region, nW, s_S, s_at, s_A, s_tab, act_range=None):
    """the specification: uint8-valued [nwin, nH, N, N], scale 2^-7"""
    ka = scores(qkv, bias, f32(s_S), f32(s_at), f32(s_A), f32(s_tab))
    masked = masked_pairs(region, qkv.shape[1], nW)
    return ibert_probs(ka, s_A, masked, act_range) if family == "ibert" else shiftmax_probs(ka, s_A, masked)


def problem(N, nH, nwin, seed):
    """-> (qkv int8 [3, nwin, nH, N, 32], bias int32 [nH, N, N]).  Window 0: key 0 dominates every query of the first half (scores
    saturate at +127 / -128: one-hot rows), the second half has q = 0 and a small bias (near-flat rows); the rest random."""
    rng = np.random.default_rng(seed)
    qkv = rng.integers(-128, 128, size=(3, nwin, nH, N, HD), dtype=np.int64).astype(np.int8)
    qkv[0, 0, :, :N // 2] = 127
    qkv[0, 0, :, N // 2:] = 0
    qkv[1, 0, :, 0] = 127
    qkv[1, 0, :, 1:] = -127
    bias = rng.integers(-40, 41, size=(nH, N, N)).astype(np.int32)
    bias[:, N // 2:] = rng.integers(-2, 3, size=(nH, N - N // 2, N))
    return qkv, bias


def one_hot_rows(p):
    """rows with exactly one non-zero probability"""
    return (p > 0).sum(axis=-1) == 1


def near_flat_rows(p):
    """rows whose largest probability stays within a few steps of the uniform 128 / N"""
    return p.max(axis=-1) <= max(4, 512 // p.shape[-1])
