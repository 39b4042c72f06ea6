"""The last block on the class rows only (IntViTEngine cls_tail): the single-query attention kernel and the q/k/v GEMM for a
subset of the planes against the CPU oracle and against the full-size kernels, then the engine's pruned forward and the graph
replays against the eager forward and the reference's golden logits.  Bit-exact: these are integer results."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.prepare import dyadic, shiftexp2d, shiftexp_band  # noqa: E402

DEV = "cuda:0"
HD = 64
_KEEP = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_tensors():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return _lib.stream_ptr()


# ------------------------------------------------------------------------------------------------ single-query attention
# (regime, Shiftmax input scale, activation scale, output scale, score multiplier): the power-of-two cases of
# test_gpu_ops.test_attention_fused (x0 = -4: a row of T >= 128 equal scores sums to T * 2^17 > 2^24) and the natural ones of
# test_gpu_compat.test_attention_fused_compat with x0 = floor(-1 / s) = -4, -5, -9
REGIMES = {
    "pow2": (2.0 ** -2, 2.0 ** -4, 2.0 ** -3, 1.0),
    "pow2_odd_multiplier": (2.0 ** -3, 2.0 ** -4, 2.0 ** -3, 1.37),
    "natural_x0_-4": (0.3127, 0.0571, 0.1173, 1.0),
    "natural_x0_-5": (0.2113, 0.0571, 0.1173, 1.0),
    "natural_x0_-9": (0.11873, 0.0571, 0.1173, 1.0),
}


def _scales(regime):
    s_at, s_a1, s_a2, mult = (np.float32(v) for v in REGIMES[regime])
    s_S = np.float32(np.float32(np.float32(s_a1 * s_a1) * np.float32(0.125)) * mult)
    s_pv = np.float32(np.float32(1 / 128.0) * s_a1)
    return s_at, dyadic(s_S, s_at), dyadic(s_pv, s_a2)


def _crafted(kind, rng, B, H, T):
    """qkv [3, B, H, T, 64] whose query 0 meets keys of chosen scores: q0 = 64 in every d and key j = a_j in every d give
    S_j = 4096 a_j, so the requantised scores are proportional to a_j (V and the other queries stay random)"""
    qkv = np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, HD))), -128, 127).astype(np.int8)
    if kind == "random":
        return qkv
    a = np.empty((B, H, T), np.int64)
    if kind == "equal":                       # all scores equal: every exponent is the largest one, the row sum the largest possible
        a[:] = 3
    elif kind == "one_far_above":             # every other key at the saturated exponent
        a[:] = -16
        a[..., T // 2] = 15
    elif kind == "saturated":                 # half of the keys at the maximum, half beyond the clamp of the exponent's argument
        a[:] = -16
        a[..., ::2] = 15
    elif kind == "all_but_one":               # one key at the saturated exponent |x0|: for an odd x0 the row sum is odd
        a[:] = 15
        a[..., 1] = -16
    elif kind == "clamped":                   # scores beyond the 8-bit range on both sides
        a[:] = rng.integers(-128, 128, size=a.shape)
    qkv[0, :, :, 0, :] = 64
    qkv[1] = a[..., None].astype(np.int8)
    return qkv


def _expected_row0(qkv, regime):
    s_at, (ms, es), (mo, eo) = _scales(regime)
    _, B, H, T, _ = qkv.shape
    exp = np.empty((B, H * HD), np.int32)
    ka_all = np.empty((B, H, T), np.int32)
    for b in range(B):
        for h in range(H):
            S = orc.gemm_i8(qkv[0, b, h, :1], qkv[1, b, h])
            ka = orc.requant(S, ms.astype(np.float64), es, 8)
            P = (orc.shiftmax_compat if regime.startswith("natural") else orc.shiftmax)(ka, s_at)
            assert P.max() <= 127
            O = orc.gemm_i8(P.astype(np.int8), qkv[2, b, h], transB=False)
            exp[b, h * HD:(h + 1) * HD] = orc.requant(O, mo.astype(np.float64), eo, 8)
            ka_all[b, h] = ka[0]
    return exp, ka_all


def _run_cls(qkv, regime, table):
    """-> (ivit_attention_cls_i8's rows with their padding, row 0 of ivit_attention_fused_i8_compat_band) on the same inputs"""
    s_at, (ms, es), (mo, eo) = _scales(regime)
    _, B, H, T, _ = qkv.shape
    d = dev(qkv)
    exp2d = band = None
    bw = 0
    if regime.startswith("natural"):
        tab = shiftexp2d(s_at)
        if table == "band":
            bnd, bw = shiftexp_band(tab)
            assert 16 <= bw <= 256
            band = dev(bnd.view(np.int32))
        else:
            exp2d = dev(tab.view(np.int32))
    q_cls = dev(np.ascontiguousarray(qkv[0, :, :, 0, :]).reshape(B, H * HD))
    ldo = H * HD + 32
    out = torch.full((B, ldo), 99, dtype=torch.int8, device=DEV)
    args = (int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0]), _lib.ptr(exp2d), _lib.ptr(band), bw)
    _lib.call("ivit_attention_cls_i8", _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(q_cls), _lib.ptr(out), ldo, B, H, T, HD, *args, st())
    full = torch.full((B * T, H * HD), 99, dtype=torch.int8, device=DEV)
    _lib.call("ivit_attention_fused_i8_compat_band", _lib.ptr(d), _lib.ptr(full), B, H, T, HD, *args, 0, st())
    return out.cpu().numpy().astype(np.int32), full.view(B, T, H * HD)[:, 0].cpu().numpy().astype(np.int32)


@pytest.mark.parametrize("T", [5, 50, 197, 207, 208])
@pytest.mark.parametrize("H", [3, 12])
@pytest.mark.parametrize("regime,table", [("pow2", None), ("pow2_odd_multiplier", None), ("natural_x0_-4", "band"), ("natural_x0_-5", "band"),
                                          ("natural_x0_-9", "band"), ("natural_x0_-4", "full"), ("natural_x0_-5", "full"),
                                          ("natural_x0_-9", "full")])
def test_attention_cls_against_oracle_and_full_kernel(T, H, regime, table):
    B = 3 if H == 3 else 2          # 9 and 24 (image, head) pairs: a last workgroup with one wave, and whole workgroups
    qkv = _crafted("random", np.random.default_rng(300 + T + H), B, H, T)
    exp, _ = _expected_row0(qkv, regime)
    got, row0 = _run_cls(qkv, regime, table)
    assert np.array_equal(got[:, :H * HD], exp), f"{(got[:, :H * HD] != exp).sum()} of {exp.size} differ from the oracle"
    assert np.array_equal(row0, exp)
    assert (got[:, H * HD:] == 99).all()          # the padding of the output rows is not written
    assert np.abs(exp).max() > 5


@pytest.mark.parametrize("T", [5, 50, 197, 207, 208])
@pytest.mark.parametrize("kind", ["equal", "one_far_above", "saturated", "all_but_one", "clamped"])
@pytest.mark.parametrize("regime,table", [("pow2", None), ("natural_x0_-4", "band"), ("natural_x0_-4", "full"), ("natural_x0_-5", "band"),
                                          ("natural_x0_-9", "band"), ("natural_x0_-9", "full")])
def test_attention_cls_crafted_rows(T, kind, regime, table):
    B, H = (1, 12) if T >= 197 else (2, 3)
    qkv = _crafted(kind, np.random.default_rng(400 + T), B, H, T)
    exp, ka = _expected_row0(qkv, regime)
    # the rows are what they are meant to be
    if kind == "equal":
        assert (ka == ka[..., :1]).all()
        if T >= 197:       # T times exp_int(0) = |x0| * 2^15: the exact integer sum needs more than float32's 24 bits
            assert T * int(-np.floor(np.float32(-1.0) / _scales(regime)[0])) * 32768 > 2 ** 24
    elif kind == "one_far_above":
        assert ((ka == ka.max(-1, keepdims=True)).sum(-1) == 1).all() and (ka.max(-1) - ka.min(-1) >= 100).all()
    elif kind == "all_but_one":
        assert ((ka == ka.max(-1, keepdims=True)).sum(-1) == T - 1).all() and (ka.max(-1) - ka.min(-1) >= 100).all()
        if T >= 197 and regime in ("natural_x0_-5", "natural_x0_-9"):
            # the exact row sum (the table the kernels read, summed in Python integers) is above 2^24 and no float32: the one
            # rounding of the sum to float32 happens, and the oracle decides which way
            tab, k0 = shiftexp2d(_scales(regime)[0]), ka[0, 0]
            total = sum(int(tab[int(k0.max()) + 128, int(k) + 128]) for k in k0)
            assert total > 2 ** 24 and int(np.float32(total)) != total
    elif kind == "saturated":
        assert (ka.max(-1) - ka.min(-1) >= 100).all() and ((ka == ka.max(-1, keepdims=True)).sum(-1) >= 2).all()
    else:
        assert ka.max() == 127 and ka.min() == -128
    got, row0 = _run_cls(qkv, regime, table)
    assert np.array_equal(got[:, :H * HD], exp), f"{(got[:, :H * HD] != exp).sum()} of {exp.size} differ from the oracle"
    assert np.array_equal(row0, exp)


def test_attention_cls_rejects_bad_arguments():
    k = torch.zeros(208 * HD + 16, dtype=torch.int8, device=DEV)
    q = torch.zeros(HD, dtype=torch.int8, device=DEV)
    out = torch.zeros(HD, dtype=torch.int8, device=DEV)

    def call(k_=k, T=197, hd=HD, ldo=HD):
        _lib.call("ivit_attention_cls_i8", _lib.ptr(k_), _lib.ptr(k), _lib.ptr(q), _lib.ptr(out), ldo, 1, 1, T, hd, 1 << 20, 29, 0.25,
                  1 << 20, 25, None, None, 0, st())

    call()
    for kw, match in ((dict(T=209), "unsupported geometry"), (dict(T=0), "unsupported geometry"), (dict(hd=32), "unsupported geometry"),
                      (dict(k_=None), "NULL"), (dict(k_=k[8:]), "misaligned"), (dict(ldo=48), "misaligned")):
        with pytest.raises(_lib.IvitError, match=match):
            call(**kw)


# ------------------------------------------------------------------------------------------------ q/k/v GEMM, some planes
def _qkv_problem(B, H, K, seed):
    rng = np.random.default_rng(seed)
    T, Cn = 197, H * HD
    M, N = B * T, 3 * Cn
    A = rng.integers(-128, 128, size=(M, K)).astype(np.int8)
    W = rng.integers(-128, 128, size=(N, K)).astype(np.int8)
    b = rng.integers(-50000, 50000, size=N).astype(np.int32)
    pre = (rng.uniform(0.5, 1.0, size=N) * 2.0 ** rng.integers(-16, -9, size=N)).astype(np.float32)
    m, e = dyadic(pre, np.float32(1.0))
    return T, Cn, M, N, A, W, b, m, e


def _planes_case(B, H, K, layouts, oracle_rows):
    """planes (1, 2) and (0, 1, 2) through ivit_gemm_i8_requant_qkv_planes_ex: the selected planes equal those of
    ivit_gemm_i8_requant_qkv_ex byte for byte and the oracle's GEMM + requantisation on `oracle_rows`, the others keep their fill"""
    T, Cn, M, N, A, W, b, m, e = _qkv_problem(B, H, K, 50 + B + H)
    dA, dW, db, dm, de = dev(A), dev(W), dev(b), dev(m.view(np.int32)), dev(e)
    if layouts & 1:
        At = torch.zeros((M + 15) // 16 * 16 * K, dtype=torch.int8, device=DEV)
        _lib.call("ivit_tile_operand_i8", _lib.ptr(dA), K, M, K, _lib.ptr(At), st())
        dA = At
    if layouts & 16:
        Wf = torch.empty(N * K, dtype=torch.int8, device=DEV)
        _lib.call("ivit_pack_weight_frags16_i8", _lib.ptr(dW), K, N, K, _lib.ptr(Wf), st())
        dW = Wf
    elif layouts & 2:
        Wb = torch.empty(N * K, dtype=torch.int8, device=DEV)
        _lib.call("ivit_tile_operand_i8", _lib.ptr(dW), K, N, K, _lib.ptr(Wb), st())
        dW = Wb
    dW = dW.view(-1)
    full = torch.full((3, M * Cn), 99, dtype=torch.int8, device=DEV)
    _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(dA), K, _lib.ptr(dW), K, _lib.ptr(db), _lib.ptr(dm), _lib.ptr(de), _lib.ptr(full),
              T, H, HD, M, N, K, layouts, st())
    rows = np.asarray(oracle_rows)
    exp = orc.requant(orc.gemm_i8(A[rows], W, b), m.astype(np.float64), e, 8).reshape(len(rows), 3, H, HD)
    got = full.view(3, B, H, T, HD).cpu().numpy().astype(np.int32)
    # (two index arrays around a slice: numpy puts their common axis first -> [row, plane, head, d])
    assert np.array_equal(got[:, rows // T, :, rows % T], exp), "the full q/k/v GEMM differs from the oracle"
    for plane0, nplanes in ((1, 2), (0, 3), (0, 1), (2, 1)):
        out = torch.full((3, M * Cn), 77, dtype=torch.int8, device=DEV)
        c0 = plane0 * Cn
        _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", _lib.ptr(dA), K, _lib.ptr(dW[c0 * K:]), K, _lib.ptr(db[c0:]), _lib.ptr(dm[c0:]),
                  _lib.ptr(de[c0:]), _lib.ptr(out), T, H, HD, plane0, nplanes, M, nplanes * Cn, K, layouts, st())
        for p in range(3):
            if plane0 <= p < plane0 + nplanes:
                assert torch.equal(out[p], full[p]), (plane0, nplanes, p)
            else:
                assert bool((out[p] == 77).all()), (plane0, nplanes, p)


@pytest.mark.parametrize("B,H", [(3, 3), (10, 12), (1, 6)])
def test_qkv_planes_small_form(B, H):
    """M < 2048: the 128 x 128-tile kernel, row-major operands"""
    _planes_case(B, H, H * HD, 0, np.arange(B * 197))


@pytest.mark.parametrize("layouts", [0, 3, 17], ids=["row_major", "block_operands", "weight_fragments"])
@pytest.mark.parametrize("H", [3, 12])
def test_qkv_planes_headline_rows(H, layouts):
    """M = 256 * 197 = 50 432: the persistent kernels (block-layout operands, fragment-packed weights)"""
    M = 256 * 197
    rows = np.unique(np.concatenate([np.arange(300), np.arange(M - 300, M), np.arange(0, M, 997)]))
    _planes_case(256, H, H * HD, layouts, rows)


def test_qkv_planes_rejects_bad_planes():
    T, Cn, M, N, A, W, b, m, e = _qkv_problem(1, 1, 64, 3)
    dA, dW, db, dm, de = dev(A), dev(W), dev(b), dev(m.view(np.int32)), dev(e)
    out = torch.zeros(3 * M * Cn, dtype=torch.int8, device=DEV)
    for plane0, nplanes, n, match in ((2, 2, 2 * Cn, "outside q, k, v"), (-1, 1, Cn, "outside q, k, v"), (0, 0, 0, "outside q, k, v"),
                                      (1, 2, 3 * Cn, "heads\\*head_dim")):
        with pytest.raises(_lib.IvitError, match=match):
            _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", _lib.ptr(dA), 64, _lib.ptr(dW), 64, _lib.ptr(db), _lib.ptr(dm), _lib.ptr(de),
                      _lib.ptr(out), T, 1, HD, plane0, nplanes, M, n, 64, 0, st())
    with pytest.raises(_lib.IvitError, match="heads\\*head_dim"):     # the three-plane entry keeps its refusal
        _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(dA), 64, _lib.ptr(dW), 64, _lib.ptr(db), _lib.ptr(dm), _lib.ptr(de),
                  _lib.ptr(out), T, 1, HD, M, 2 * Cn, 64, 0, st())


# ------------------------------------------------------------------------------------------------ engine
def _engine(tag, max_batch, **kw):
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=max_batch, **kw)
    return eng, meta, z


def _host(out):
    return tuple(t.cpu().numpy().copy() for t in out)


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: INT32 logits differ"
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), f"{what}: float logits differ bitwise"
    assert np.array_equal(a[2], b[2]), f"{what}: top-1 differs"


@pytest.mark.parametrize("tag", ["deit_tiny", "deit_small", "deit_base", "vit_base", "deit_tiny_natural", "deit_small_natural",
                                 "deit_base_natural", "vit_large_natural"])
def test_pruned_tail_equals_full_forward_and_golden(tag):
    eng, meta, z = _engine(tag, 16)
    assert eng.cls_tail_ok
    n = meta["n_images"]
    gold = torch.from_numpy(synth.make_images(n, meta["image_seed"])).to(DEV)
    eager = _host(eng.forward(gold))
    for name, run in (("forward(cls_tail=True)", lambda x: eng.forward(x, cls_tail=True)), ("forward_graph", eng.forward_graph)):
        got = _host(run(gold))
        # the reference's integers; its float logits are the eager forward's bit for bit only at power-of-two scales
        # (test_gpu_compat.test_natural_scale_model_matches_reference), so those are held against the eager forward
        assert np.array_equal(got[0], z["logits_int32"]), f"{tag} {name}: INT32 logits differ from the reference's"
        assert np.array_equal(got[2].astype(np.int64), z["top1"]), f"{tag} {name}"
        _same(got, eager, f"{tag} {name}")
    if not tag.endswith("_natural"):
        assert np.array_equal(eager[1].view(np.int32), z["logits_f32_bits"])
    imgs = torch.from_numpy(synth.make_images(16, 2718)).to(DEV)
    for B in (1, 2, 16):
        x = imgs[:B].contiguous()
        full = _host(eng.forward(x))
        _same(_host(eng.forward(x, cls_tail=True)), full, f"{tag} B={B} cls_tail")
        _same(_host(eng.forward_graph(x)), full, f"{tag} B={B} graph")
        if B == 16:
            assert len(set(full[2].tolist())) > 1


def test_pruned_tail_headline_batch_and_permutation():
    eng, meta, z = _engine("deit_base", 256)
    imgs = torch.from_numpy(synth.make_images(256, 31337)).to(DEV)
    full = _host(eng.forward(imgs))
    _same(_host(eng.forward(imgs, cls_tail=True)), full, "B=256 cls_tail")
    _same(_host(eng.forward_graph(imgs)), full, "B=256 graph")
    _same(_host(eng.forward_graph(imgs, resident=True)), full, "B=256 resident graph")
    perm = np.random.default_rng(1).permutation(256)
    got = _host(eng.forward_graph(imgs[torch.from_numpy(perm).to(DEV)].contiguous()))
    _same(got, tuple(a[perm] for a in full), "permuted batch")
    assert len(set(full[2].tolist())) > 10


def test_pruned_tail_other_geometry():
    """160 / 16: 101 tokens, the general-T attention in the full blocks"""
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    fs = dict(fs)
    fs["pos_embed"] = np.random.default_rng(101).normal(0, 0.02, size=(1, 101, cfg["embed_dim"])).astype(np.float32)
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=16, img_size=160, patch_size=16)
    assert eng.T == 101 and eng.cls_tail_ok
    imgs = torch.from_numpy(np.random.default_rng(5).normal(0, 1, size=(16, 3, 160, 160)).astype(np.float32)).to(DEV)
    for B in (2, 16):
        x = imgs[:B].contiguous()
        full = _host(eng.forward(x))
        _same(_host(eng.forward(x, cls_tail=True)), full, f"160/16 B={B} cls_tail")
        _same(_host(eng.forward_graph(x)), full, f"160/16 B={B} graph")


@pytest.mark.parametrize("tag", ["deit_tiny", "deit_base_natural"])
def test_topk_graph_equals_forward_topk(tag):
    eng, meta, z = _engine(tag, 16)
    imgs = torch.from_numpy(synth.make_images(16, 99)).to(DEV)
    li, lf, tk = _host(eng.forward_topk(imgs, k=5))
    targets = torch.from_numpy(tk[:, 2].astype(np.int32)).to(DEV)      # every image's target is its rank-2 class
    hits = torch.zeros(5, dtype=torch.int64, device=DEV)
    got = _host(eng.forward_topk_graph(imgs, k=5, targets=targets, hits=hits))
    _same(got, (li, lf, tk), f"{tag} top-k graph")
    assert hits.cpu().tolist() == [0, 0, 16, 0, 0]
    assert np.array_equal(tk[:, 0], _host(eng.forward(imgs))[2])


@pytest.mark.parametrize("tag,kw", [("deit_tiny_ibert", dict(family="ibert")), ("deit_tiny_w16", dict(stream_bits=16))])
def test_other_engines_keep_the_full_tail(tag, kw):
    eng, meta, z = _engine(tag, 8, **kw)
    assert not eng.cls_tail_ok
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    full = _host(eng.forward(imgs))
    assert np.array_equal(full[2].astype(np.int64), z["top1"])
    _same(_host(eng.forward_graph(imgs)), full, f"{tag} graph")
    with pytest.raises(ValueError, match="cls_tail"):
        eng.forward(imgs, cls_tail=True)
