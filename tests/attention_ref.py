"""What the GPU tests of the fused ViT attention entries share (test_gpu_attention_long / _wide / _wide_long / _ibert_long /
_entries): device buffers that outlive a launch, the scales and crafted rows of the Shiftmax cases, their expectation from the
oracle per (image, head) -- matmul -> requant -> Shiftmax(output_bit) -> int64 P.V -> requant -- and one guarded launch."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from ivit_amd import _lib
from ivit_amd.prepare import dyadic, shiftexp2d, shiftexp_band

DEV = "cuda:0"
HD = 64
SENTINEL = 99
KEEP = []  # device tensors whose raw pointers were handed to the C ABI stay alive until the test's final synchronize


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def release():
    """imported by a test module: autouse there"""
    yield
    torch.cuda.synchronize()
    KEEP.clear()


def st():
    return _lib.stream_ptr()


@functools.lru_cache(maxsize=None)
def tables(s_at):
    tab = shiftexp2d(np.float32(s_at))
    bt, bw = shiftexp_band(tab)
    assert 16 <= bw <= 256
    return tab, bt, bw


def block_valid(rows, K):
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


def scales(natural, s_mult, bits):
    """-> s_at, (ms, es), (mo, eo) flattened.  s_mult 1 at a power-of-two scale: Ms a power of two (the float32 requantisation of
    the scores), otherwise float64"""
    s_a1 = np.float32(0.0571 if natural else 2.0 ** -4)
    s_S = np.float32(np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125)) * np.float32(s_mult))
    s_at = np.float32(0.0437 if natural else 2.0 ** -3)
    s_pv = np.float32(np.float32(2.0 ** -(bits - 1)) * s_a1)          # Shiftmax output scale 2^-(bits-1) times the scale of V
    s_a2 = np.float32(0.1173 if natural else 2.0 ** -3)
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(s_pv, s_a2)
    if not natural:
        assert ((int(ms[0]) & (int(ms[0]) - 1)) == 0) == (s_mult == 1.0)
    return s_at, ms, es, mo, eo


def inputs(rng, B, H, T):
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


def expected(qkv, s_at, ms, es, mo, eo, natural, bits, pmax=None):
    """-> (expected output [B, T, C], the probabilities of (image 0, head 0), max |O| over all heads); pmax: the largest probability
    the case may hold (default: 2^(bits-1), which a one-hot row reaches)"""
    _, B, H, T, _ = qkv.shape
    exp = np.empty((B, T, H * HD), np.int32)
    P00, omax = None, 0
    for b in range(B):
        for h in range(H):
            S = orc.gemm_i8(qkv[0, b, h], qkv[1, b, h])
            ka = orc.requant(S, ms.astype(np.float64), es, 8)
            P = (orc.shiftmax_compat if natural else orc.shiftmax)(ka, s_at, output_bit=bits)
            assert P.min() >= 0 and P.max() <= (1 << (bits - 1) if pmax is None else pmax)
            O = P.astype(np.int64) @ qkv[2, b, h].astype(np.int64)
            omax = max(omax, int(np.abs(O).max()))
            assert omax < 2 ** 31
            exp[b, :, h * HD:(h + 1) * HD] = orc.requant(O.astype(np.int32), mo.astype(np.float64), eo, 8)
            if b == 0 and h == 0:
                P00 = P
    return exp, P00, omax


def launch(name, qkv, tail, blocks):
    """One entry on head-major qkv [3, B, H, T, 64]; tail: the entry's arguments between head_dim and out_blocks.  -> the row-major
    result [B, T, C]; the bytes behind the buffer and the padding rows of the last block stay untouched"""
    _, B, H, T, _ = qkv.shape
    M, C = B * T, H * HD
    rows = (M + 15) // 16 * 16 if blocks else M
    out = torch.full((rows * C + 64,), SENTINEL, dtype=torch.int8, device=DEV)      # 64 guard bytes behind the buffer
    KEEP.append(out)
    args = [_lib.ptr(dev(qkv)), _lib.ptr(out), B, H, T, HD, *tail]
    if name != "ivit_attention_fused_i8":       # the first entry: row-major only, no layout flag
        args.append(int(blocks))
    _lib.call(name, *args, st())
    rm = out[:M * C]
    if blocks:
        rm = torch.full((M * C,), SENTINEL, dtype=torch.int8, device=DEV)
        KEEP.append(rm)
        _lib.call("ivit_untile_operand_i8", _lib.ptr(out), M, C, _lib.ptr(rm), C, st())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[rows * C:] == SENTINEL).all(), "bytes behind the output buffer were written"
    if blocks:
        assert (raw[:rows * C][~block_valid(M, C)] == SENTINEL).all(), "padding rows of the last block were written"
    return rm.cpu().numpy().astype(np.int32).reshape(B, T, C)


def shiftmax_tables(s_at, form):
    """-> (exp2d pointer, band pointer, band_w) of a Shiftmax regime: "pow2" (no table), "exp2d", "band" """
    if form == "pow2":
        return None, None, 0
    tab, bt, bw = tables(float(s_at))
    if form == "band":
        return None, _lib.ptr(dev(bt.view(np.int32))), bw
    return _lib.ptr(dev(tab.view(np.int32))), None, 0


def run(name, qkv, s_at, ms, es, mo, eo, form, bits, blocks):
    """A Shiftmax entry that takes the tables (_compat_band, _wide, _long, _wide_long); bits goes to the wide ones"""
    wide = (bits,) if "wide" in name else ()
    return launch(name, qkv, (int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0]), *shiftmax_tables(s_at, form), *wide), blocks)


def run_ibert(name, qkv, ms, es, mo, eo, tab, band, blocks):
    """An I-BERT entry on the float32 (row max, q) table `tab` [256][256], `band`: in its band form"""
    bandt, bw = None, 0
    if band:
        bt, bw = shiftexp_band(tab.view(np.uint32))
        assert bw and 16 <= bw <= 128
        bandt = dev(bt.view(np.float32).reshape(-1))
    wide = (8,) if "wide" in name else ()
    return launch(name, qkv, (int(ms[0]), int(es[0]), int(mo[0]), int(eo[0]), _lib.ptr(dev(tab.reshape(-1))), _lib.ptr(bandt), bw, *wide),
                  blocks)
