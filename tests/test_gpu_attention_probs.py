"""Attention maps on the GPU: the integer softmax probabilities of ivit_attention_probs_u8 / ivit_attention_probs_u8_ibert against the
oracle (Shiftmax) and the numpy restatement of tests/ibert_long_ref.py (I-BERT, crafted rows on which the ORDER of the float32 row sum
decides probabilities), P . V of the written map against the fused entries that never write it, strided rows between fences, the
argument errors, and IntViTEngine / VisionTransformer.attention_maps against the module path's forward hooks.

Token counts: the smallest rows (1, 5: the scalar form of the row sum), 17 and 50 (one / three 16-key tiles, a partial last one), both
sides of 192 | 193 (where the fused I-BERT kernels begin) and of 207 | 208 | 209 (short | long fused kernels; 192 and 208 are whole tiles
and rows of whole dwords), 577 and 1025 (the cascade of the row sum, 65 key tiles: the largest LDS image)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.engine_common import attention_entry  # noqa: E402
from ivit_amd.prepare import dyadic, shiftexp_band  # noqa: E402
import attention_ref as A  # noqa: E402
import fenced  # noqa: E402
import ibert_long_ref as R  # noqa: E402
from attention_ref import DEV, dev, release, st  # noqa: E402,F401  (release: the autouse fixture)
from test_gpu_vit16_lazy import W8, W16ALL, _calibrated, _images  # noqa: E402

SHIFTMAX, IBERT = "ivit_attention_probs_u8", "ivit_attention_probs_u8_ibert"
TOKENS = (1, 5, 17, 50, 192, 193, 197, 207, 208, 209, 577, 1025)
HD = 64
FILL = 0xA5          # no probability: they end at 128
# Shiftmax regimes: a power-of-two input scale (the 256-entry table in LDS), and two natural scales of tests/test_gpu_compat.py -- one
# handed over in the band form, one as the full [256][256] table
S_ATTN = {"pow2": 2.0 ** -3, "band": 0.3127, "exp2d": 0.0571}


def _bh(T):
    return (2, 2) if T <= 209 else (1, 2)


def _q_rows(T):
    """1 (the class row), T (the full map) and one count between them that ends inside a 16-query tile"""
    mid = T // 2 + (1 if (T // 2) % 16 == 0 else 0)
    return [1] + ([mid] if 1 < mid < T else []) + ([T] if T > 1 else [])


def _frozen(*arrays):
    """the shared expectations are read-only (the inputs go through torch.from_numpy, which wants writable arrays)"""
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _launch(name, qkv_t, B, H, T, q_rows, tail):
    """one dense launch (ldp = T) -> uint8 [B, H, q_rows, T]; the bytes behind the buffer keep their fill"""
    n = B * H * q_rows * T
    out = torch.full((n + 64,), FILL, dtype=torch.uint8, device=DEV)
    A.KEEP.append(out)
    _lib.call(name, _lib.ptr(qkv_t), _lib.ptr(out), T, B, H, T, HD, q_rows, *tail, st())
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[n:] == FILL).all(), "bytes behind the output buffer were written"
    return raw[:n].reshape(B, H, q_rows, T)


# ----------------------------------------------------------------------------------- Shiftmax
def _shiftmax_scales(regime):
    natural = regime != "pow2"
    s_a1 = np.float32(0.0571 if natural else 2.0 ** -4)
    s_S = np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125))
    s_at = np.float32(S_ATTN[regime])
    ms, es = dyadic(s_S, s_at)
    mo, eo = dyadic(np.float32(np.float32(2.0 ** -7) * s_a1), np.float32(0.1173 if natural else 2.0 ** -3))
    return s_at, ms, es, mo, eo


@functools.lru_cache(maxsize=None)
def _shiftmax_case(T, regime):
    """-> qkv int8 [3, B, H, T, 64], P uint8 [B, H, T, T] by the oracle: matmul -> requant -> Shiftmax, as tests/test_gpu_ops.py and
    tests/attention_ref.py compose the fused kernels' reference.  Computed once per (T, regime), read-only"""
    B, H = _bh(T)
    qkv = A.inputs(np.random.default_rng(900 + T), B, H, T)
    s_at, ms, es, _, _ = _shiftmax_scales(regime)
    P = np.empty((B, H, T, T), np.uint8)
    for b in range(B):
        for h in range(H):
            ka = orc.requant(orc.gemm_i8(qkv[0, b, h], qkv[1, b, h]), ms.astype(np.float64), es, 8)
            p = (orc.shiftmax if regime == "pow2" else orc.shiftmax_compat)(ka, s_at)
            # 127 at most, except a row of ONE key at a power-of-two scale: e * floor(2^31 / e) = 2^31, p = 128 (an unsigned byte holds it)
            assert p.min() >= 0 and p.max() <= (128 if T == 1 else 127)
            P[b, h] = p
    return (qkv,) + _frozen(P)


def _shiftmax_tail(regime):
    s_at, ms, es, _, _ = _shiftmax_scales(regime)
    return (int(ms[0]), int(es[0]), float(s_at), *A.shiftmax_tables(s_at, regime))


@pytest.mark.parametrize("regime", sorted(S_ATTN))
@pytest.mark.parametrize("T", TOKENS)
def test_shiftmax_probabilities_equal_the_oracle(T, regime):
    qkv, P = _shiftmax_case(T, regime)
    B, H = _bh(T)
    if T > 17:
        assert P[0, 0, 5, 17] > 120 and P[0, 0, 5].sum() == P[0, 0, 5, 17]      # the one-hot row of attention_ref.inputs
    assert P.max() > 20 and len(np.unique(P)) > 8 or T == 1
    qkv_t, tail = dev(qkv), _shiftmax_tail(regime)
    for q_rows in _q_rows(T):
        got = _launch(SHIFTMAX, qkv_t, B, H, T, q_rows, tail)
        exp = P[:, :, :q_rows]
        assert np.array_equal(got, exp), f"q_rows={q_rows}: {(got != exp).sum()} of {got.size} bytes differ"


# ----------------------------------------------------------------------------------- I-BERT
def small_row(T, seed, x_bits=None):
    """ibert_long_ref.crafted_row for rows shorter than its 13 near keys: T keys at the distinct distances 0 .. T - 1 from the row
    maximum, full-mantissa table entries that add up to about 0.6 * 2^30 without the dominant key's, whose entry is x_bits"""
    rng = np.random.default_rng(seed * 7919 + T)
    qm = int(rng.integers(40, 100))
    dist = rng.permutation(T)
    w = rng.uniform(0.5, 1.0, size=256)
    scale = 0.6 * 2.0 ** 30 / (w[dist].sum() - w[0])
    tabrow = np.zeros(256, np.float32)
    tabrow[qm + 128 - np.arange(qm + 129)] = (w[:qm + 129] * scale).astype(np.float32)
    tabrow[qm + 128] = np.float32(0.0) if x_bits is None else np.array([x_bits], np.uint32).view(np.float32)[0]
    return dict(t=(qm - dist).astype(np.int8), qm=qm, pos=int(np.argmin(dist)), tabrow=tabrow)


# T -> (row constructor, seed, bits of the dominant key's table entry): found on the CPU with the method of
# scripts/find_rowsum_rows.py (bisection of torch's sum to 2^30, then a scan of the floats around the crossing), seed 0 each.  577 and
# 1025 are the rows of ibert_long_ref.CRAFTED
CRAFTED = {5: (small_row, 0, 0x4dcccccf), 17: (R.crafted_row, 0, 0x4dcccccf), 50: (R.crafted_row, 0, 0x4dccccd0),
           192: (R.crafted_row, 0, 0x4dcccccd), 193: (R.crafted_row, 0, 0x4dccccce), 197: (R.crafted_row, 0, 0x4dccccd1),
           207: (R.crafted_row, 0, 0x4dcccccd), 208: (R.crafted_row, 0, 0x4dccccd0), 209: (R.crafted_row, 0, 0x4dcccccf),
           **{T: (R.crafted_row, seed, bits) for T, seed, bits in R.CRAFTED if T in TOKENS}}
IBERT_MS = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))         # 2^-9: a score row t arrives exactly as 8 * 64 * t / 512


def _crafted_queries(T):
    return sorted({0, (16 * 7 + 3) % T, T - 1})       # the same row in up to three query tiles, the last (partial) one included


@functools.lru_cache(maxsize=None)
def _ibert_case(T, crafted=True):
    """-> qkv, table float32 [256][256], P uint8 [B, H, T, T] by the restatement (table lookup over (row max, q), torch's row sum,
    factor, floor), number of p == 128.  Head (0, 0) carries the crafted row of T as the score row of the crafted queries (q = 64 on
    eight dimensions, K = t on the same eight, multiplier 2^-9); head (0, 1) the one-hot row of tests/test_gpu_attention_ibert_long.py"""
    B, H = _bh(T)
    rng = np.random.default_rng(700 + T)
    qkv = np.clip(np.rint(rng.normal(0, 30, size=(3, B, H, T, HD))), -128, 127).astype(np.int8)
    tab = R.synthetic_table(T)
    ms, es = IBERT_MS
    if T > 17:
        qkv[0, 0, 1, 5] = 0
        qkv[0, 0, 1, 5, :8] = 127
        qkv[1, 0, 1] = np.clip(qkv[1, 0, 1], -10, 10)
        qkv[1, 0, 1, 17, :8] = 127
    if crafted and T in CRAFTED:
        make, seed, bits = CRAFTED[T]
        row = make(T, seed, bits)
        qkv[1, 0, 0] = 0
        qkv[1, 0, 0, :, :8] = row["t"][:, None]
        for i in _crafted_queries(T):
            qkv[0, 0, 0, i] = 0
            qkv[0, 0, 0, i, :8] = 64
        tab[row["qm"] + 128] = row["tabrow"]
    P = np.empty((B, H, T, T), np.uint8)
    for b in range(B):
        for h in range(H):
            ka = orc.requant(orc.gemm_i8(qkv[0, b, h], qkv[1, b, h]), ms.astype(np.float64), es, 8)
            E = tab[ka.max(axis=1)[:, None] + 128, ka + 128].astype(np.float32)
            for i in range(T):
                p = R.probabilities(E[i], orc.torch_rowsum(E[i]))
                assert p.min() >= 0 and p.max() <= 128
                P[b, h, i] = p
    return (qkv, tab) + _frozen(P) + (int((P == 128).sum()),)


def _ibert_tail(tab, band):
    ms, es = IBERT_MS
    bandt, bw = None, 0
    if band:
        bt, bw = shiftexp_band(tab.view(np.uint32))
        assert bw and 16 <= bw <= 256
        bandt = dev(bt.view(np.float32).reshape(-1))
    return (int(ms[0]), int(es[0]), _lib.ptr(dev(tab.reshape(-1))), _lib.ptr(bandt), bw)


def test_restatement_holds_a_one_hot_row_and_order_sensitive_rows():
    """from the restatement alone, before any launch: (a) p == 128 occurs; (b) the crafted rows of ibert_long_ref at 301 tokens and
    above sit in the score rows and give other probabilities under a left-to-right sum; (c) below 208 and below 8 tokens a row is
    present whose probabilities under a left-to-right sum or a per-lane tree differ from those of torch's order"""
    assert sum(_ibert_case(T)[3] for T in TOKENS if 17 < T <= 209) > 0
    ms, es = IBERT_MS
    seen = []
    for T in TOKENS:
        if T not in CRAFTED:
            continue
        qkv, tab, P, _ = _ibert_case(T)
        make, seed, bits = CRAFTED[T]
        row = make(T, seed, bits)
        e = R.crafted_exponents(row)
        ka = orc.requant(orc.gemm_i8(qkv[0, 0, 0], qkv[1, 0, 0]), ms.astype(np.float64), es, 8)
        pt = R.probabilities(e, orc.torch_rowsum(e))
        pa, pb = R.probabilities(e, R.sum_left_to_right(e)), R.probabilities(e, R.sum_lane_tree(e))
        for i in _crafted_queries(T):
            assert np.array_equal(ka[i], row["t"].astype(np.int32)), (T, i)          # the wanted scores, exactly
            assert np.array_equal(P[0, 0, i], pt)
        if T >= 301:
            assert (T, seed, bits) in R.CRAFTED and not np.array_equal(pt, pa), T
        assert not np.array_equal(pt, pa) or not np.array_equal(pt, pb), T
        seen.append(T)
    assert any(T < 8 for T in seen) and any(8 <= T < 208 for T in seen) and {577, 1025} <= set(seen)


@pytest.mark.parametrize("band", [False, True], ids=["table", "band"])
@pytest.mark.parametrize("T", TOKENS)
def test_ibert_probabilities_equal_the_restatement(T, band):
    qkv, tab, P, n128 = _ibert_case(T)
    B, H = _bh(T)
    if T > 17:
        assert n128 > 0 and P[0, 1, 5, 17] == 128
    qkv_t, tail = dev(qkv), _ibert_tail(tab, band)
    for q_rows in _q_rows(T):
        got = _launch(IBERT, qkv_t, B, H, T, q_rows, tail)
        exp = P[:, :, :q_rows]
        assert np.array_equal(got, exp), f"q_rows={q_rows}: {(got != exp).sum()} of {got.size} bytes differ"


# ----------------------------------------------------------------------------------- the map is what the hot kernels use
def _pv(P, qkv, mo, eo):
    """P . V in int64 on the host, requantised by the oracle -> [B, T, H * 64]"""
    B, H, T, _ = P.shape
    out = np.empty((B, T, H * HD), np.int32)
    for b in range(B):
        for h in range(H):
            O = P[b, h].astype(np.int64) @ qkv[2, b, h].astype(np.int64)
            assert np.abs(O).max() < 2 ** 31
            out[b, :, h * HD:(h + 1) * HD] = orc.requant(O.astype(np.int32), mo.astype(np.float64), eo, 8)
    return out


@pytest.mark.parametrize("regime", sorted(S_ATTN))
@pytest.mark.parametrize("T", [197, 577])
def test_shiftmax_map_times_v_is_the_fused_output(T, regime):
    qkv, _ = _shiftmax_case(T, regime)
    B, H = _bh(T)
    s_at, ms, es, mo, eo = _shiftmax_scales(regime)
    P = _launch(SHIFTMAX, dev(qkv), B, H, T, T, _shiftmax_tail(regime))
    name = attention_entry("ivit", T)
    assert name == ("ivit_attention_fused_i8_long" if T > 207 else "ivit_attention_fused_i8_compat_band")
    fused = A.run(name, qkv, s_at, ms, es, mo, eo, regime, 8, 0)
    exp = _pv(P, qkv, mo, eo)
    assert np.abs(exp).max() > 5
    assert np.array_equal(fused, exp), f"{(fused != exp).sum()} of {exp.size} differ"


@pytest.mark.parametrize("band", [False, True], ids=["table", "band"])
@pytest.mark.parametrize("T", [197, 577])
def test_ibert_map_times_v_is_the_fused_output(T, band):
    qkv, tab, _, n128 = _ibert_case(T, False)          # the plain synthetic table: its band is at most 128 wide, as the fused kernels need
    B, H = _bh(T)
    assert n128 > 0
    ms, es = IBERT_MS
    mo, eo = dyadic(np.float32(2.0 ** -10), np.float32(2.0 ** -3))
    P = _launch(IBERT, dev(qkv), B, H, T, T, _ibert_tail(tab, band))
    name = attention_entry("ibert", T)
    assert name == ("ivit_attention_fused_i8_ibert_long" if T > 207 else "ivit_attention_fused_i8_ibert")
    fused = A.run_ibert(name, qkv, ms, es, mo, eo, tab, band, 0)
    exp = _pv(P, qkv, mo, eo)
    assert np.abs(exp).max() > 5
    assert np.array_equal(fused, exp), f"{(fused != exp).sum()} of {exp.size} differ"


# ----------------------------------------------------------------------------------- strided rows between fences
@pytest.mark.parametrize("T,lead", [(197, 3), (199, 0)], ids=["bytes", "dwords"])
@pytest.mark.parametrize("full", [False, True], ids=["cls", "all"])
def test_probabilities_into_fenced_strided_rows(T, lead, full):
    """ldp = T + 13 with guard rows around: pads, guards and the slack keep their fill.  197 tokens from an odd address: ldp = 210,
    every byte stored on its own; 199 tokens: ldp = 212 from an aligned address, packed dwords and the three last bytes of a row"""
    B, H = _bh(T)
    ldp, q_rows = T + 13, T if full else 1
    assert (ldp % 4 == 0 and lead == 0) == (T == 199)
    qkv, P = _shiftmax_case(T, "pow2")
    exp = P[:, :, :q_rows].reshape(B * H * q_rows, T)
    o = fenced.output(B * H * q_rows, T, ldp, np.uint8, expected=exp, lead_bytes=lead)
    s_at, ms, es, _, _ = _shiftmax_scales("pow2")
    _lib.call("ivit_attention_probs_u8", _lib.ptr(dev(qkv)), o.ptr, ldp, B, H, T, HD, q_rows, int(ms[0]), int(es[0]), float(s_at),
              None, None, 0, st())
    torch.cuda.synchronize()
    fenced.check(o, exp)
    qkv, tab, P, _ = _ibert_case(T, False)
    exp = P[:, :, :q_rows].reshape(B * H * q_rows, T)
    o = fenced.output(B * H * q_rows, T, ldp, np.uint8, expected=exp, lead_bytes=lead)
    ms, es = IBERT_MS
    _lib.call("ivit_attention_probs_u8_ibert", _lib.ptr(dev(qkv)), o.ptr, ldp, B, H, T, HD, q_rows, int(ms[0]), int(es[0]),
              _lib.ptr(dev(tab.reshape(-1))), None, 0, st())
    torch.cuda.synchronize()
    fenced.check(o, exp)


# ----------------------------------------------------------------------------------- argument errors
INVALID, UNSUPPORTED = -1, -2
GOOD = dict(qkv=True, probs=True, ldp=197, tokens=197, head_dim=64, q_rows=197, m_s=1 << 30, e_s=40, s_attn=0.125, table=True, band=None,
            band_w=0, qkv_off=0, table_off=0)
# (what changes, status, entries it applies to)
REJECTED = [(dict(head_dim=32), UNSUPPORTED, "both"), (dict(tokens=0, q_rows=1), UNSUPPORTED, "both"),
            (dict(tokens=1026, ldp=1026), UNSUPPORTED, "both"),
            (dict(qkv=False), INVALID, "both"), (dict(probs=False), INVALID, "both"), (dict(table=False), INVALID, "ibert"),
            (dict(q_rows=0), INVALID, "both"), (dict(q_rows=198), INVALID, "both"), (dict(ldp=196), INVALID, "both"),
            (dict(qkv_off=8), INVALID, "both"), (dict(table_off=2), INVALID, "both"),
            (dict(band=True, band_w=24), INVALID, "both"), (dict(band=True, band_w=272), INVALID, "both"),
            (dict(band=None, band_w=32), INVALID, "both"), (dict(band=True, band_w=32, band_off=4), INVALID, "both"),
            (dict(m_s=1 << 31, e_s=20), INVALID, "both"),                    # multiplier 2048
            (dict(s_attn=0.0), INVALID, "ivit"), (dict(s_attn=-0.5), INVALID, "ivit"),
            (dict(s_attn=2.0 ** -13), INVALID, "ivit"),                      # x0 = -8192
            (dict(s_attn=1.0 / 700), INVALID, "ivit")]                       # 197 * 700 * 2^15 passes 2^32: the short rows' bound


@pytest.mark.parametrize("case", range(len(REJECTED)))
@pytest.mark.parametrize("family", ["ivit", "ibert"])
def test_rejections_return_their_status_and_write_nothing(case, family):
    change, status, applies = REJECTED[case]
    if applies not in ("both", family):
        return
    a = dict(GOOD, **change)
    T = max(a["tokens"], 1)
    qkv = torch.zeros(3 * T * HD + 64, dtype=torch.int8, device=DEV)
    tab = torch.zeros(65536 + 64, dtype=torch.float32, device=DEV)       # stands for exp2d, the I-BERT table and a band alike
    out = torch.full((max(a["ldp"], 1) * max(a["q_rows"], 1) + 64,), FILL, dtype=torch.uint8, device=DEV)
    A.KEEP.extend([qkv, tab, out])
    p_qkv = qkv.data_ptr() + a["qkv_off"] if a["qkv"] else None
    p_out = out.data_ptr() if a["probs"] else None
    p_tab = tab.data_ptr() + a["table_off"] if a["table"] else None
    p_band = tab.data_ptr() + a.get("band_off", 0) if a["band"] else None
    L = _lib.lib()
    if family == "ivit":
        rc = L.ivit_attention_probs_u8(p_qkv, p_out, a["ldp"], 1, 1, a["tokens"], a["head_dim"], a["q_rows"], a["m_s"], a["e_s"],
                                       a["s_attn"], p_tab if change.get("table_off") else None, p_band, a["band_w"], st())
    else:
        rc = L.ivit_attention_probs_u8_ibert(p_qkv, p_out, a["ldp"], 1, 1, a["tokens"], a["head_dim"], a["q_rows"], a["m_s"], a["e_s"],
                                             p_tab, p_band, a["band_w"], st())
    assert rc == status, (rc, L.ivit_last_error_string())
    assert L.ivit_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()), "a rejected call wrote to its output"


def test_the_unchanged_arguments_are_accepted():
    """the rejections above change one thing each in a call that succeeds"""
    a, T = GOOD, GOOD["tokens"]
    qkv = torch.zeros(3 * T * HD, dtype=torch.int8, device=DEV)
    tab = torch.ones(65536, dtype=torch.float32, device=DEV)
    out = torch.full((T * T,), FILL, dtype=torch.uint8, device=DEV)
    A.KEEP.extend([qkv, tab, out])
    _lib.call(SHIFTMAX, _lib.ptr(qkv), _lib.ptr(out), T, 1, 1, T, 64, T, a["m_s"], a["e_s"], a["s_attn"], None, None, 0, st())
    torch.cuda.synchronize()
    assert bool((out != FILL).all())
    out.fill_(FILL)
    _lib.call(IBERT, _lib.ptr(qkv), _lib.ptr(out), T, 1, 1, T, 64, T, a["m_s"], a["e_s"], _lib.ptr(tab), None, 0, st())
    torch.cuda.synchronize()
    assert bool((out != FILL).all())


# ----------------------------------------------------------------------------------- engine and model
def _hook_maps(model, x, rows):
    model.use_engine = False
    try:
        return model.attention_maps(x, rows=rows)
    finally:
        model.use_engine = True


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "natural"])
@pytest.mark.parametrize("family,img", [("ivit", 224), ("ivit", 160), ("ivit", 256), ("ibert", 224)])
def test_engine_maps_equal_the_module_paths_softmax_output(family, img, pow2):
    """a frozen depth-2 DeiT (embed 128, 2 heads): the maps of the engine call are, byte for byte, what forward hooks on the int_softmax
    modules of the same model see on the module path -- the reference's own tensor; the class rows are row 0 of them; the forward that
    produced them left the logits of model(x)"""
    depth, heads, B = 2, 2, 2
    T = (img // 16) ** 2 + 1
    model, g = _calibrated(img, 16, 128, depth, heads, pow2, 11, family, W8)
    assert model.engine_unsupported_reason() is None
    x = _images(B, img, g)
    with torch.no_grad():
        y = model(x)
        assert model.takes_engine(x)
        maps, scale = model.attention_maps(x, rows="all")
        eng = model.engine(B)
        logits = eng.ws["logits_f"][:B, :eng.num_classes].clone()
        cls, scale_c = model.attention_maps(x, rows="cls")
        one, _ = model.attention_maps(x, layers=[1], rows="cls")
        ref, scale_r = _hook_maps(model, x, "all")
        ref_c, _ = _hook_maps(model, x, "cls")
    assert scale == scale_c == scale_r == 2.0 ** -7
    assert sorted(maps) == sorted(cls) == sorted(ref) == list(range(depth)) and sorted(one) == [1]
    assert torch.equal(logits, y)
    for i in range(depth):
        assert maps[i].dtype == ref[i].dtype == torch.uint8 and tuple(maps[i].shape) == tuple(ref[i].shape) == (B, heads, T, T)
        assert torch.equal(maps[i], ref[i]), f"block {i}: {int((maps[i] != ref[i]).sum())} of {maps[i].numel()} bytes differ"
        assert tuple(cls[i].shape) == (B, heads, 1, T) and torch.equal(cls[i], ref[i][:, :, :1]) and torch.equal(ref_c[i], cls[i])
        assert int(ref[i].max()) > 8 and int(ref[i].max()) <= 128       # a live attention
    assert torch.equal(one[1], cls[1])
    assert torch.equal(model(x), y)


def test_a_16_bit_softmax_is_refused_on_both_paths():
    model, g = _calibrated(224, 16, 128, 2, 2, True, 11, "ivit", W16ALL)
    assert model.engine_unsupported_reason() is None and model._engine_widths == (16, 16, 16)
    x = _images(2, 224, g)
    with torch.no_grad():
        assert model.takes_engine(x)
        with pytest.raises(ValueError, match="16 bits"):
            model.attention_maps(x)
        model.use_engine = False
        try:
            with pytest.raises(ValueError, match="16 bits"):
                model.attention_maps(x)
        finally:
            model.use_engine = True


def test_ibert_model_outside_the_engines_range_takes_the_hooks():
    """101 tokens: no fused I-BERT attention, so no engine; the call still answers, from the module path"""
    model, g = _calibrated(160, 16, 128, 2, 2, False, 11, "ibert", W8)
    assert "tokens" in model.engine_unsupported_reason()
    x = _images(2, 160, g)
    with torch.no_grad():
        maps, scale = model.attention_maps(x, rows="all")
        cls, _ = model.attention_maps(x, layers=[0])
    assert scale == 2.0 ** -7 and sorted(maps) == [0, 1] and sorted(cls) == [0]
    for m in maps.values():
        assert m.dtype == torch.uint8 and tuple(m.shape) == (2, 2, 101, 101) and 8 < int(m.max()) <= 128
    assert torch.equal(cls[0], maps[0][:, :, :1])
