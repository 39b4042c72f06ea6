"""GPU: the classifier top-k (ivit_head_topk / ivit_logits_topk_f32) against torch's stable sort on the CPU, ties included;
hit counting; argument errors; the engines' forward_topk (eager and graph replay) against the reference's golden logits; the
data-parallel evaluation and driver at world 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference, synth, topk  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.parallel import DataParallelTopK  # noqa: E402
from ivit_amd.swin_engine import IntSwinEngine  # noqa: E402

DEV = "cuda:0"


def st():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stable_topk(lf, N, k):
    """the contract: torch.sort(stable=True) on the CPU of the first N columns"""
    return torch.sort(torch.from_numpy(np.ascontiguousarray(lf[:, :N])), dim=1, descending=True, stable=True).indices[:, :k].numpy()


def torch_hits(ref_topk, targets, k):
    return np.array([(ref_topk[:, r] == targets).sum() for r in range(k)], np.int64)


def head_topk(acc, s, N, k, targets=None, hits=None):
    B, ld = acc.shape
    a, sd = dev(acc), dev(s)
    lf = torch.empty(B, ld, dtype=torch.float32, device=DEV)
    tk = torch.empty(B, k, dtype=torch.int32, device=DEV)
    tg = None if targets is None else dev(targets.astype(np.int32))
    _lib.call("ivit_head_topk", _lib.ptr(a), _lib.ptr(sd), B, ld, N, k, _lib.ptr(lf), _lib.ptr(tk), _lib.ptr(tg), _lib.ptr(hits), st())
    return lf.cpu().numpy(), tk.cpu().numpy()


def head_argmax(acc, s):
    B, N = acc.shape
    a, sd = dev(acc), dev(s)
    lf = torch.empty(B, N, dtype=torch.float32, device=DEV)
    t1 = torch.empty(B, dtype=torch.int32, device=DEV)
    _lib.call("ivit_head_argmax", _lib.ptr(a), _lib.ptr(sd), B, N, _lib.ptr(lf), _lib.ptr(t1), st())
    return lf.cpu().numpy(), t1.cpu().numpy()


def logits_topk(lf, N, k, targets=None, hits=None):
    B, ld = lf.shape
    x = dev(lf.astype(np.float32))
    tk = torch.empty(B, k, dtype=torch.int32, device=DEV)
    tg = None if targets is None else dev(targets.astype(np.int32))
    _lib.call("ivit_logits_topk_f32", _lib.ptr(x), B, ld, N, k, _lib.ptr(tk), _lib.ptr(tg), _lib.ptr(hits), st())
    return tk.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------------- kernel vs stable sort
SHAPES = [(1, 1000, 1000, 5), (256, 1000, 1000, 5), (3, 21843, 21844, 5), (4, 5, 8, 5)] + [(7, 10, 12, k) for k in range(1, 9)]


@pytest.mark.parametrize("B,N,ld,k", SHAPES)
def test_head_topk_equals_stable_sort(B, N, ld, k):
    rng = np.random.default_rng(B * 7 + N + k)
    acc = rng.integers(-300000, 300000, size=(B, ld)).astype(np.int32)
    s = rng.uniform(1e-6, 2e-6, size=ld).astype(np.float32)
    if ld > N:          # padded classes with logits that would win if the selection read them
        acc[:, N:] = 2 ** 30
        s[N:] = 1.0
    lf, tk = head_topk(acc, s, N, k)
    exp = (acc.astype(np.float32) * s[None]).astype(np.float32)
    assert np.array_equal(bits(lf), bits(exp))                       # every column up to ld, padded ones too
    assert np.array_equal(tk, stable_topk(exp, N, k))
    assert tk.max() < N
    # the float entry on the same logits selects the same classes
    assert np.array_equal(logits_topk(exp, N, k), tk)
    if ld == N:
        lfa, t1 = head_argmax(acc, s)
        assert np.array_equal(bits(lf), bits(lfa))
        assert np.array_equal(tk[:, 0], t1)


# ----------------------------------------------------------------------------------- ties
def test_ties_all_equal_rows_and_duplicated_maxima_across_rank_k():
    B, N = 6, 1000
    acc = np.full((B, N), 5, np.int32)
    s = np.full(N, 0.25, np.float32)
    # row 1: seven classes share the maximum (five of them make the cut, by ascending index)
    acc[1, [900, 3, 50, 7, 600, 20, 11]] = 100
    # row 2: one clear maximum, then four classes tied for ranks 2-5 and two more with the same value
    acc[2, 999] = 200
    acc[2, [640, 64, 6, 333, 1, 998]] = 100
    # row 3: the tie straddles rank 5 from below: ranks 1-3 distinct, six equal values compete for ranks 4-5
    acc[3, [10, 20, 30]] = [300, 250, 200]
    acc[3, [700, 500, 300, 100, 40, 41]] = 150
    # row 4: the maximum repeated at the last and the first column (the wave's lane 0 and lane 39 of the last pass)
    acc[4, [N - 1, 0]] = 10 ** 6
    for k in (1, 5, 8):
        lf, tk = head_topk(acc, s, N, k)
        exp = (acc.astype(np.float32) * s[None]).astype(np.float32)
        assert np.array_equal(tk, stable_topk(exp, N, k)), k
        _, t1 = head_argmax(acc, s)
        assert np.array_equal(tk[:, 0], t1)
    assert tk[0].tolist() == list(range(8))
    assert tk[1, :5].tolist() == [3, 7, 11, 20, 50]
    assert tk[2, :5].tolist() == [999, 1, 6, 64, 333]
    assert tk[3, :5].tolist() == [10, 20, 30, 40, 41]
    assert tk[4, :2].tolist() == [0, N - 1]


def test_ties_from_the_float_conversion_and_the_per_class_scale():
    """int32 accumulators above 2^24 that round to the same float, and different integers that a per-class scale maps to the
    same float"""
    B, N = 4, 1000
    rng = np.random.default_rng(11)
    acc = rng.integers(-1000, 1000, size=(B, N)).astype(np.int32)
    s = np.ones(N, np.float32)
    big = 2 ** 24
    acc[0, [5, 900, 17, 400, 2, 77]] = [big + 1, big, big + 3, big + 4, big + 2, big - 1]
    acc[1, :] = rng.integers(big, big + 64, size=N)        # many collisions among the ~32 distinct floats
    third = np.float32(1.0) / np.float32(3.0)
    s[[10, 20, 30]] = third
    acc[2, acc[2] > 0] = -5
    acc[2, [10, 20, 30]] = 3                              # fl(3 * fl(1/3)) = 1.0
    acc[2, [15, 5, 25]] = 1                               # = 1.0 with scale 1
    acc[3, [10, 20, 30, 40]] = [3 * 2 ** 20, 3 * 2 ** 20, 3, 2 ** 20]
    s[40] = np.float32(1.0)
    for k in (5, 8):
        lf, tk = head_topk(acc, s, N, k)
        exp = (acc.astype(np.float32) * s[None]).astype(np.float32)
        assert np.array_equal(bits(lf), bits(exp))
        assert np.array_equal(tk, stable_topk(exp, N, k)), k
        _, t1 = head_argmax(acc, s)
        assert np.array_equal(tk[:, 0], t1)
    assert len(set(exp[0, [5, 900]].tolist())) == 1 and len(set(exp[2, [5, 10, 15]].tolist())) == 1   # the ties are real
    assert tk[0, :5].tolist() == [17, 400, 2, 5, 900]
    assert tk[2, :5].tolist() == [5, 10, 15, 20, 25]


def test_signed_zeros_are_one_value_through_the_float_entry():
    N = 70
    lf = np.full((3, N), -1.0, np.float32)
    lf[0, [3, 64, 9, 66, 1]] = [-0.0, 0.0, 0.0, -0.0, -0.0]
    lf[1, :] = -0.0
    lf[1, [2, 5, 69]] = 0.0
    lf[2, [40, 4, 68]] = [0.0, -0.0, 2.0]
    for k in (1, 3, 5, 8):
        tk = logits_topk(lf, N, k)
        assert np.array_equal(tk, stable_topk(lf, N, k)), k
    assert tk[0, :5].tolist() == [1, 3, 9, 64, 66]
    assert tk[1].tolist() == list(range(8))
    assert tk[2, :3].tolist() == [68, 4, 40]


# ----------------------------------------------------------------------------------- hits
@pytest.mark.parametrize("k", [1, 5, 8])
def test_hits_accumulate_and_equal_a_torch_count(k):
    B, N = 200, 1000
    rng = np.random.default_rng(k)
    hits = torch.zeros(k, dtype=torch.int64, device=DEV)
    want = np.zeros(k, np.int64)
    for call in range(2):
        acc = rng.integers(-50, 50, size=(B, N)).astype(np.int32)           # ties everywhere
        s = np.full(N, 0.5, np.float32)
        exp = (acc.astype(np.float32) * s[None]).astype(np.float32)
        ref = stable_topk(exp, N, k)
        pick = rng.integers(0, k + 3, size=B)
        targets = np.where(pick < k, ref[np.arange(B), np.minimum(pick, k - 1)],
                           np.where(pick == k, -1, np.where(pick == k + 1, N, rng.integers(0, N, size=B)))).astype(np.int32)
        _, tk = head_topk(acc, s, N, k, targets, hits)
        assert np.array_equal(tk, ref)
        want += torch_hits(ref, targets, k)
        torch.cuda.synchronize()
        assert np.array_equal(hits.cpu().numpy(), want), call
    assert want.sum() > 0
    # the float entry: same counts on the same logits
    h2 = torch.zeros(k, dtype=torch.int64, device=DEV)
    logits_topk(exp, N, k, targets, h2)
    assert np.array_equal(h2.cpu().numpy(), torch_hits(ref, targets, k))


def test_count_hits_and_topk_front():
    rng = np.random.default_rng(3)
    lf = rng.integers(-30, 30, size=(50, 100)).astype(np.float32)
    ref = stable_topk(lf, 100, 5)
    x = dev(lf)
    assert np.array_equal(topk.topk(x, 5).cpu().numpy(), ref)
    assert np.array_equal(topk.topk(x, 3, n_classes=60).cpu().numpy(), stable_topk(lf, 60, 3))
    targets = np.where(rng.random(50) < 0.7, ref[np.arange(50), rng.integers(0, 5, 50)], -1).astype(np.int32)
    hits = torch.zeros(5, dtype=torch.int64, device=DEV)
    topk.count_hits(x, dev(targets), hits, k=5)
    topk.count_hits(x, dev(targets), hits, k=5)
    assert np.array_equal(hits.cpu().numpy(), 2 * torch_hits(ref, targets, 5))


# ----------------------------------------------------------------------------------- argument errors
def test_bad_arguments_raise_and_leave_outputs_untouched():
    B, N, ld = 4, 10, 12
    acc, s = dev(np.ones((B, ld), np.int32)), dev(np.ones(ld, np.float32))
    lfin = dev(np.ones((B, ld), np.float32))
    lf = torch.full((B, ld), 7.0, device=DEV)
    tk = torch.full((B, 8), -7, dtype=torch.int32, device=DEV)
    tg = torch.zeros(B, dtype=torch.int32, device=DEV)
    hits = torch.full((8,), 13, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    bad = [dict(k=0), dict(k=9), dict(k=11), dict(N=4), dict(N=13), dict(targets=tg, hits=None), dict(targets=None, hits=hits),
           dict(tk=None)]
    for b in bad:
        a = dict(k=5, N=N, targets=None, hits=None, tk=tk)
        a.update(b)
        with pytest.raises(_lib.IvitError):
            _lib.call("ivit_head_topk", _lib.ptr(acc), _lib.ptr(s), B, ld, a["N"], a["k"], _lib.ptr(lf), _lib.ptr(a["tk"]),
                      _lib.ptr(a["targets"]), _lib.ptr(a["hits"]), st())
        with pytest.raises(_lib.IvitError):
            _lib.call("ivit_logits_topk_f32", _lib.ptr(lfin), B, ld, a["N"], a["k"], _lib.ptr(a["tk"]), _lib.ptr(a["targets"]),
                      _lib.ptr(a["hits"]), st())
    torch.cuda.synchronize()
    assert (lf == 7.0).all() and (tk == -7).all() and (hits == 13).all()
    with pytest.raises(ValueError):
        topk.topk(lfin, 11)


# ----------------------------------------------------------------------------------- engines vs the reference goldens
def _engine(tag, max_batch):
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    if tag == "swin_tiny":
        eng = IntSwinEngine(fs, ranges, cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window"], device=DEV,
                            max_batch=max_batch)
    elif tag == "deit_tiny_w16":       # the 16-bit residual stream: the engine the module dispatch builds for these widths
        import ivit_amd.quantization_utils as q
        model = ivit.deit_tiny_patch16_224(**meta["widths"])
        model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
        for name, mod in model.named_modules():
            if isinstance(mod, q.QuantAct):
                mod.x_min.fill_(float(ranges[name][0]))
                mod.x_max.fill_(float(ranges[name][1]))
        model.to(DEV)
        ivit.freeze_model(model)
        eng = model.engine(max_batch)
        assert eng.stream_bits == 16
    else:
        eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=max_batch,
                           family=meta.get("family", "ivit"))
    return eng, meta, z


@pytest.mark.parametrize("tag", ["deit_tiny", "deit_tiny_w16", "deit_tiny_ibert", "swin_tiny"])
def test_engine_forward_topk_against_golden(tag):
    eng, meta, z = _engine(tag, 8)
    n = meta["n_images"]
    imgs = torch.from_numpy(synth.make_images(n, meta["image_seed"])).to(DEV)
    gold = z["logits_f32_bits"][:n].view(np.float32)
    ref = stable_topk(gold, gold.shape[1], 5)
    li, lf, t1 = eng.forward(imgs)
    li, lf, t1 = li.cpu().numpy().copy(), lf.cpu().numpy().copy(), t1.cpu().numpy().copy()
    assert np.array_equal(bits(lf), z["logits_f32_bits"][:n])
    targets = torch.from_numpy(ref[np.arange(n), np.arange(n) % 5].astype(np.int32)).to(DEV)
    hits = torch.zeros(5, dtype=torch.int64, device=DEV)
    li2, lf2, tk = eng.forward_topk(imgs, 5, targets, hits)
    assert tk.shape == (n, 5) and tk.dtype == torch.int32
    assert np.array_equal(li2.cpu().numpy(), li)
    assert np.array_equal(bits(lf2.cpu().numpy()), bits(lf))
    tk = tk.cpu().numpy()
    assert np.array_equal(tk, ref)
    assert np.array_equal(tk[:, 0], t1)
    assert np.array_equal(hits.cpu().numpy(), torch_hits(ref, targets.cpu().numpy(), 5))
    for k in (1, 8):
        assert np.array_equal(eng.forward_topk(imgs, k)[2].cpu().numpy(), stable_topk(gold, gold.shape[1], k))


def test_graph_replay_topk_equals_eager_and_accumulates_hits():
    eng, meta, z = _engine("deit_tiny", 8)
    n = meta["n_images"]
    imgs_np = synth.make_images(n, meta["image_seed"])
    imgs = torch.from_numpy(imgs_np).to(DEV)
    gold = z["logits_f32_bits"].view(np.float32)
    ref = stable_topk(gold, 1000, 5)
    targets = torch.zeros(n, dtype=torch.int32, device=DEV)
    hits = torch.zeros(5, dtype=torch.int64, device=DEV)
    want = np.zeros(5, np.int64)
    rng = np.random.default_rng(5)
    for rep in range(3):
        t = np.where(rng.random(n) < 0.8, ref[np.arange(n), rng.integers(0, 5, n)], 1000).astype(np.int32)
        targets.copy_(torch.from_numpy(t))
        li, lf, tk = eng.forward_topk_graph(imgs, 5, targets, hits)
        assert np.array_equal(tk.cpu().numpy(), ref)
        assert np.array_equal(li.cpu().numpy(), z["logits_int32"])
        want += torch_hits(ref, t, 5)
        assert np.array_equal(hits.cpu().numpy(), want), rep
    assert len(eng._graphs) == 1
    # other images through the same graph; a second k is its own graph; the top-1 graph is unaffected
    perm = np.arange(n)[::-1].copy()
    _, _, tk = eng.forward_topk_graph(torch.from_numpy(imgs_np[perm]).to(DEV), 5, targets, hits)
    assert np.array_equal(tk.cpu().numpy(), ref[perm])
    _, _, tk3 = eng.forward_topk_graph(imgs, 3)
    assert np.array_equal(tk3.cpu().numpy(), ref[:, :3])
    g1, _, t1 = eng.forward_graph(imgs)
    assert np.array_equal(g1.cpu().numpy(), z["logits_int32"]) and np.array_equal(t1.cpu().numpy(), ref[:, 0])
    # the uncaptured warm-up of a new graph does not count: hits moved only by the replay above
    assert hits.sum().item() == want.sum() + sum((ref[perm][:, r] == targets.cpu().numpy()).sum() for r in range(5))


# ----------------------------------------------------------------------------------- harness at world 1
def _frozen_deit_tiny():
    import ivit_amd.quantization_utils as q
    fs, ranges, cfg, meta, z = load_synthetic_model("deit_tiny")
    model = ivit.deit_tiny_patch16_224()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, q.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV)
    ivit.freeze_model(model)
    return model, meta


def test_evaluate_dataset_parallel_world1_equals_evaluate_dataset():
    model, meta = _frozen_deit_tiny()
    imgs = torch.from_numpy(synth.make_images(12, 4242))
    with torch.no_grad():
        lf = model(imgs.to(DEV)).float().cpu().numpy()
    srt = np.sort(lf, axis=1)[:, ::-1]
    # torch.topk (evaluate_dataset) leaves the order of equal logits open: use rows without a tie among their top 6
    assert (np.diff(srt[:, :6], axis=1) < 0).all()
    ref = stable_topk(lf, lf.shape[1], 5)
    rng = np.random.default_rng(1)
    pick = rng.integers(0, 7, 12)
    tgt = torch.from_numpy(np.where(pick < 5, ref[np.arange(12), np.minimum(pick, 4)], np.where(pick == 5, -1, 999 - ref[:, 0])))
    loader = [(imgs[:5], tgt[:5]), (imgs[5:6], tgt[5:6]), (imgs[6:], tgt[6:])]
    want = inference.evaluate_dataset(model, loader, DEV, print_batch_stats=False)
    got = inference.evaluate_dataset_parallel(model, loader, DEV, print_batch_stats=False)
    assert got == want
    assert 0 < want[0] < want[1] < want[2] < 100


def test_data_parallel_topk_world1_equals_forward_topk():
    eng, meta, z = _engine("deit_tiny", 8)
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    _, _, tk = eng.forward_topk(imgs, 5)
    want = tk.cpu().numpy().copy()
    for graph in (False, True):
        dp = DataParallelTopK(eng, 1, k=5, graph=graph)
        assert np.array_equal(dp.step(imgs).cpu().numpy(), want), graph
