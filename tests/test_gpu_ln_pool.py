"""The pooled-LayerNorm entries (csrc/ln_pool.h, csrc/pool.hip): ivit_layernorm_pool_i8 / _i16, ivit_ibert_layernorm_pool_i8 / _i16.
Reference: the int8-emitting LayerNorm entry of the same kind (pinned to the oracle elsewhere) on every token, a numpy int64 sum
over the selected tokens and floor((2 * sum + T) / (2 * T)) in integers.  Everything is integers: equality only."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ibert as ib
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT, layernorm  # noqa: E402
from ivit_amd.prepare import dyadic, markstein_division_ok  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
FAMILIES = ["ivit", "ibert", "ibert_intsqrt"]
#         (B, T_all, t0, T, C)
SHAPES = [(1, 2, 1, 1, 64), (3, 6, 1, 5, 192), (2, 66, 1, 65, 384), (2, 197, 1, 196, 768), (1, 578, 1, 577, 1024), (2, 130, 2, 127, 192),
          (40, 130, 1, 129, 64)]      # the last one: more than 4096 rows, slabs longer than a workgroup's four waves


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_ln(family, bits, C, beta0=0.0, s_next=4.0 / 127.0):
    """an engine_common ln dict (ln_spec's shape) with random affine parameters; the QuantAct behind it has scale s_next"""
    rng = np.random.default_rng(C + bits)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(f32), (rng.normal(0, 0.3, C) + beta0).astype(f32)
    if family == "ivit":
        _, s, bias = orc.layernorm(np.arange(C, dtype=np.int32)[None], gamma, beta)
        ln = dict(kind=f"i{bits}")
    else:
        bias, s = ib.layernorm_constants(gamma, beta)
        s_in = float(f32(0.0371) if bits == 8 else f32(1.37e-4))
        ln = dict(kind=f"ibert_i{bits}", s_in=s_in, shift_pow2=1.0 if bits == 8 else 4.0,
                  flags=IBERT_LN_INT_SQRT if family == "ibert_intsqrt" else 0, fast_div=int(bits == 16 and markstein_division_ok(s_in, 16)))
    m, e = dyadic(s, s_next)
    ln.update(bias=dev(bias), s=dev(s), m=dev(m.view(np.int32)), e=dev(e))
    return ln


def rows(bits, n, C, seed=0):
    rng = np.random.default_rng(seed + n + C)
    sig, mu, top = (rng.uniform(0.5, 60.0, (n, 1)), 20, 127) if bits == 8 else (300.0, 200, 32767)
    k = np.clip(np.rint(rng.normal(rng.normal(0, mu, (n, 1)), sig, (n, C))), -top - 1, top)
    return k.astype(np.int8 if bits == 8 else np.int16)


def reference(ln, k, sel):
    """(sum int64 [B, C], mean int64 [B, C]) from the int8-emitting entry on all B * T_all rows of k"""
    B, T_all, t0, T = sel
    C = k.shape[1]
    q = torch.empty(B * T_all, C, dtype=torch.int8, device=DEV)
    layernorm(ln, dev(k), C, B * T_all, C, q, C, _lib.stream_ptr(), blocks=False)
    s = q.cpu().numpy().astype(np.int64).reshape(B, T_all, C)[:, t0:t0 + T].sum(1)
    return s, (2 * s + T) // (2 * T)


def pool_args(ln, sel, C):
    """(entry, arguments between C and sum, flags, workspace) of the C ABI call for an ln dict"""
    n = ctypes.c_int64()
    _lib.call("ivit_layernorm_pool_workspace_bytes", sel[0], sel[3], C, ctypes.byref(n))
    ws = torch.empty(n.value // 4, dtype=torch.int32, device=DEV)
    p, tail = _lib.ptr, (_lib.ptr(ln["m"]), _lib.ptr(ln["e"]))
    if ln["kind"] == "i8":
        return "ivit_layernorm_pool_i8", (p(ln["bias"]), p(ln["s"]), None, None) + tail, 0, ws
    if ln["kind"] == "i16":
        return "ivit_layernorm_pool_i16", (0.0, p(ln["bias"]), p(ln["s"])) + tail, 0, ws
    flags = ln["flags"] | (2 if ln["fast_div"] else 0)      # IVIT_LN_F32_FAST_DIV
    return f"ivit_ibert_layernorm_pool_i{ln['kind'][7:]}", (ln["s_in"], p(ln["bias"]), p(ln["s"]), ln["shift_pow2"]) + tail, flags, ws


def pooled(ln, x, ldx, sel, C, out=None, ldo=None, col0=0):
    B = sel[0]
    total = torch.full((B, C), -1, dtype=torch.int32, device=DEV)
    out = torch.full((B, C), 99, dtype=torch.int8, device=DEV) if out is None else out
    ldo = C if ldo is None else ldo
    name, mid, flags, ws = pool_args(ln, sel, C)
    _lib.call(name, _lib.ptr(x), ldx, *sel, C, *mid, _lib.ptr(total), _lib.ptr(out), ldo, col0, flags, _lib.ptr(ws), ws.numel() * 4,
              _lib.stream_ptr())      # (each entry is called by its name in tests/test_gpu_far_pool.py)
    return total.cpu().numpy().astype(np.int64), out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("family", FAMILIES)
def test_pool_equals_the_int8_entry_summed(family, bits, shape):
    B, T_all, t0, T, C = shape
    ln, k = make_ln(family, bits, C), rows(bits, B * T_all, C)
    want_sum, want_mean = reference(ln, k, shape[:4])
    got_sum, got_mean = pooled(ln, dev(k), C, shape[:4], C)
    assert np.array_equal(got_sum, want_sum)
    assert np.array_equal(got_mean, want_mean)


def test_shapes_cover_the_slab_rule():
    """a last slab of a single row, exactly full slabs, and slabs of more rows than a workgroup has waves -- for the rule as the
    library states it"""
    L = []
    for B, _, _, T, _ in SHAPES:
        n = ctypes.c_int()
        _lib.call("ivit_layernorm_pool_slab_rows", B, T, ctypes.byref(n))
        L.append((T, n.value))
    assert any(T > n and T % n == 1 for T, n in L) and any(T > n and T % n == 0 for T, n in L) and any(4 < n < T for T, n in L), L


@pytest.mark.parametrize("bits", [8, 16])
def test_strided_rows_and_a_column_range_between_canaries(bits):
    sel, C = (2, 30, 1, 29), 128
    ln, k = make_ln("ivit", bits, C), rows(bits, 60, C)
    x = torch.full((60, C + 16), 77, dtype=dev(k).dtype, device=DEV)
    x[:, :C] = dev(k)
    out = torch.full((2, C + 128), 55, dtype=torch.int8, device=DEV)
    want_sum, want_mean = reference(ln, k, sel)
    got_sum, got = pooled(ln, x, C + 16, sel, C, out=out, ldo=C + 128, col0=64)
    assert np.array_equal(got_sum, want_sum) and np.array_equal(got[:, 64:64 + C], want_mean)
    assert (got[:, :64] == 55).all() and (got[:, 64 + C:] == 55).all()


@pytest.mark.parametrize("beta0,rail", [(60.0, 127), (-60.0, -128)])
@pytest.mark.parametrize("family,bits", [("ivit", 8), ("ibert", 16)])
def test_saturated_rows(family, bits, beta0, rail):
    sel, C = (2, 14, 1, 13), 192
    got_sum, got_mean = pooled(make_ln(family, bits, C, beta0=beta0), dev(rows(bits, 28, C)), C, sel, C)
    assert (got_sum == 13 * rail).all() and (got_mean == rail).all()


def test_negative_halves_round_up():
    """two rows alternating over six tokens: sum = 3 (qA + qB), an exact half wherever qA + qB is odd -- about half the channels of a
    random draw, a good part of them negative"""
    C, T = 192, 6
    ln, ab = make_ln("ivit", 8, C), rows(8, 2, C, seed=5)
    k = np.tile(ab, (T // 2, 1))
    want_sum, want_mean = reference(ln, k, (1, T, 0, T))
    half = ((2 * want_sum + T) % (2 * T) == 0) & (want_sum % T != 0)
    assert (half & (want_sum < 0)).any() and (half & (want_sum > 0)).any()
    got_sum, got_mean = pooled(ln, dev(k), C, (1, T, 0, T), C)
    assert np.array_equal(got_sum, want_sum) and np.array_equal(got_mean, want_mean)
    assert np.array_equal(got_mean[half] * 2 * T, 2 * want_sum[half] + T)      # k + 1/2 -> k + 1, on either side of zero


def test_refusals_launch_nothing():
    L, C = _lib.lib(), 64
    ln = make_ln("ivit", 8, C)
    x = torch.zeros(8 * 1100, C, dtype=torch.int8, device=DEV)
    out = torch.full((8, C + 8), 55, dtype=torch.int8, device=DEV)
    ws = torch.full((1 << 18,), -3, dtype=torch.int32, device=DEV)
    V, I = ctypes.c_void_p, ctypes.c_int64

    def call(sel=(2, 8, 1, 7), C=C, o=out.data_ptr(), ldo=C + 8, col0=0, wsb=ws.numel() * 4):
        return L.ivit_layernorm_pool_i8(V(x.data_ptr()), I(C), *sel, C, _lib.ptr(ln["bias"]), _lib.ptr(ln["s"]), None, None, _lib.ptr(ln["m"]),
                                        _lib.ptr(ln["e"]), None, V(o), I(ldo), I(col0), 0, _lib.ptr(ws), I(wsb), _lib.stream_ptr())

    INVALID, UNSUPPORTED = -1, -2
    for rc, want in [(call(sel=(2, 8, 1, 0)), INVALID), (call(sel=(2, 1100, 1, 1026)), UNSUPPORTED), (call(sel=(2, 8, 2, 7)), INVALID),
                     (call(C=2052, ldo=2052), UNSUPPORTED), (call(C=66), UNSUPPORTED), (call(o=out.data_ptr() + 1), INVALID),
                     (call(col0=12), INVALID), (call(wsb=16), INVALID)]:
        assert rc == want and b"ivit_layernorm_pool_i8" in L.ivit_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 55).all()) and bool((ws == -3).all()), "a refused call wrote"
    assert call() == 0
