"""k-NN on the int8 feature bank, on the GPU: ivit_rows_rnorm_i8_f32, ivit_knn_topk_i8 (with ivit_knn_workspace_bytes) and
ivit_knn_vote_f32 against tests/knn_ref.py, bit for bit and element for element -- the geometry sweep over every number of bank
segments, short and empty segments, ties across tile and segment boundaries, the insertion and value extremes, the refusals with
sentinel-filled outputs, fenced strided operands, and inference.evaluate_knn end to end on a synthetic DeiT-Tiny."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_synthetic_model  # noqa: E402
from ivit_amd.engine import IntViTEngine  # noqa: E402
from ivit_amd.inference import evaluate_knn, extract_features  # noqa: E402
from ivit_amd.knn import FeatureBank, knn_classify, knn_weights  # noqa: E402

import fenced  # noqa: E402
import knn_ref  # noqa: E402

DEV = "cuda:0"
SPLITS = (0, 1, 3, 64)


def st():
    return _lib.stream_ptr()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def workspace(Q, N, k, splits):
    need = C.c_int64(-1)
    _lib.call("ivit_knn_workspace_bytes", Q, N, k, splits, C.byref(need))
    assert need.value >= 0 and need.value % 8 == 0
    return torch.empty(max(need.value // 8, 1), dtype=torch.int64, device=DEV), need.value


def rnorm_gpu(x):
    """rnorm of the rows of a dense device tensor [rows, C]"""
    out = torch.empty(x.shape[0], dtype=torch.float32, device=DEV)
    _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(x), x.stride(0), x.shape[0], x.shape[1], _lib.ptr(out), st())
    return out


def search(qd, bd, rn, k, splits):
    """dense device operands -> (idx, score) as numpy"""
    Q, N = qd.shape[0], bd.shape[0]
    ws, need = workspace(Q, N, k, splits)
    idx = torch.full((Q, k), -7, dtype=torch.int32, device=DEV)
    score = torch.full((Q, k), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call("ivit_knn_topk_i8", _lib.ptr(qd), qd.stride(0), Q, _lib.ptr(bd), bd.stride(0), N, bd.shape[1], _lib.ptr(rn), k, splits,
              _lib.ptr(idx), _lib.ptr(score), _lib.ptr(ws), need, st())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy()


def check_all(q, bank, ks, splits=SPLITS, what=""):
    """every k of ks and every number of segments against the reference (one reference at max(ks): the order is total)"""
    qd, bd = dev(q), dev(bank)
    rn = rnorm_gpu(bd)
    ref_rn = knn_ref.rnorm(bank)
    assert np.array_equal(knn_ref.bits(rn.cpu().numpy()), knn_ref.bits(ref_rn)), f"{what}: rnorm"
    ridx, rsc = knn_ref.topk(q, bank, max(ks), ref_rn)
    for k in ks:
        for sp in splits:
            idx, sc = search(qd, bd, rn, k, sp)
            assert np.array_equal(idx, ridx[:, :k]), f"{what}: indices, k={k} splits={sp}"
            assert np.array_equal(knn_ref.bits(sc), knn_ref.bits(rsc[:, :k])), f"{what}: scores, k={k} splits={sp}"
    return ridx, rsc


def rand8(rng, rows, c):
    return rng.integers(-128, 128, size=(rows, c)).astype(np.int8)


# =========================================================================================== geometry sweep
@pytest.mark.parametrize("N", [1, 15, 257, 1003])
@pytest.mark.parametrize("Cc", [64, 192, 1024])
def test_geometry_sweep(Cc, N):
    rng = np.random.default_rng(1000 * Cc + N)
    bank = rand8(rng, N, Cc)
    ks = [k for k in (1, 5, 20, 256) if k <= N]
    for Q in (1, 33, 130):
        check_all(rand8(rng, Q, Cc), bank, ks, what=f"C={Cc} N={N} Q={Q}")


def test_no_queries_is_ok_without_a_launch():
    bank = dev(rand8(np.random.default_rng(1), 20, 64))
    rn = rnorm_gpu(bank)
    idx = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
    score = torch.zeros(1, 4, dtype=torch.float32, device=DEV)
    _lib.call("ivit_knn_topk_i8", _lib.ptr(bank), 64, 0, _lib.ptr(bank), 64, 20, 64, _lib.ptr(rn), 4, 0, _lib.ptr(idx), _lib.ptr(score), None, 0, st())
    torch.cuda.synchronize()
    assert (idx == -7).all()


# =========================================================================================== short and empty segments
def test_segments_shorter_than_k():
    rng = np.random.default_rng(2)
    check_all(rand8(rng, 37, 128), rand8(rng, 300, 128), [256], splits=(4,), what="N=300 k=256 splits=4")


def test_empty_segments():
    rng = np.random.default_rng(3)
    check_all(rand8(rng, 37, 128), rand8(rng, 5, 128), [1, 5], splits=(64,), what="N=5 splits=64")


# =========================================================================================== ties
def test_equal_rows_across_tile_and_segment_boundaries():
    rng = np.random.default_rng(4)
    N, Cc = 300, 64                         # splits = 2: segments of 192 rows; bank tiles of 64
    bank = rand8(rng, N, Cc)
    twin = (10, 63, 64, 100, 191, 192, 250)
    bank[list(twin)] = bank[10]
    q = rand8(rng, 20, Cc)
    q[0] = bank[10]                         # its own row: the best score, seven times
    ridx, _ = check_all(q, bank, [3, 5, 7, 20], splits=(0, 1, 2, 3, 64), what="twins")
    assert tuple(ridx[0, :7]) == twin


def test_all_equal_rows_return_ascending_indices():
    rng = np.random.default_rng(5)
    bank = np.repeat(rand8(rng, 1, 192), 300, axis=0)
    ridx, _ = check_all(rand8(rng, 33, 192), bank, [1, 256], splits=(1, 3, 64), what="all equal")
    assert (ridx == np.arange(256)[None, :]).all()


def test_zero_rows_score_plus_zero():
    rng = np.random.default_rng(6)
    bank = rand8(rng, 130, 64)
    bank[[0, 64, 129]] = 0
    q = rand8(rng, 17, 64)
    q[3] = 0                                # a zero query ties with every row: indices 0 .. k - 1
    ridx, rsc = check_all(q, bank, [130], splits=(1, 3), what="zero rows")
    for i in range(17):
        z = [list(ridx[i]).index(j) for j in (0, 64, 129)]
        assert (knn_ref.bits(rsc[i, z]) == 0).all()
    assert (ridx[3] == np.arange(130)).all()


# =========================================================================================== insertion extremes
def _graded(n):
    """n bank rows (a, b, 0, ...) whose score against the query (1, 0, ...) strictly ascends with the index"""
    a, b = np.meshgrid(np.arange(-128, 128), np.arange(0, 128), indexing="ij")
    rows = np.zeros((a.size, 64), np.int8)
    rows[:, 0], rows[:, 1] = a.reshape(-1), b.reshape(-1)
    q = np.zeros((1, 64), np.int8)
    q[0, 0] = 1
    s = knn_ref.scores(q, rows)[0]
    _, first = np.unique(s, return_index=True)          # ascending distinct scores
    pick = first[np.linspace(0, first.size - 1, n).astype(int)]
    assert np.all(np.diff(s[pick]) > 0)
    return q, rows[pick]


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_insertion_extremes(order):
    q, bank = _graded(1003)                 # ascending: every row enters the list; descending: none after the first k
    if order == "descending":
        bank = bank[::-1].copy()
    q = np.repeat(q, 33, axis=0)
    q[1::2, 0] = -1                         # every other query sees the opposite order
    ridx, _ = check_all(q, bank, [20, 256], splits=(1, 3), what=order)
    assert tuple(ridx[0, :3]) == ((1002, 1001, 1000) if order == "ascending" else (0, 1, 2))


# =========================================================================================== value extremes
def test_value_extremes():
    rng = np.random.default_rng(7)
    bank = rand8(rng, 70, 1024)
    bank[0], bank[1], bank[2], bank[65] = -128, 127, -127, -128
    q = rand8(rng, 20, 1024)
    q[0], q[1], q[2] = -128, 127, -127
    ridx, rsc = check_all(q, bank, [1, 70], splits=(1, 2), what="extremes")
    # dot = n2 = 2^24 for rows 0 and 65; row 2 (all -127) is parallel to them: the same score 4096, by index
    assert tuple(ridx[0, :3]) == (0, 2, 65) and (rsc[0, :3] == np.float32(4096.0)).all() and ridx[0, -1] == 1


# =========================================================================================== rnorm alone
@pytest.mark.parametrize("Cc,lead", [(100, 1), (768, 0), (1024, 0), (77, 3)])
def test_rnorm(Cc, lead):
    rng = np.random.default_rng(Cc)
    x = rand8(rng, 3001, Cc)
    x[0], x[1], x[2], x[3] = -128, 127, 0, -127
    x[4] = 0
    x[4, Cc - 1] = 1
    x[5:900] = rng.integers(-3, 4, size=(895, Cc))      # small norms, zero rows among them
    exp = knn_ref.rnorm(x)
    assert exp[2] == 0 and exp[4] == 1
    ldx = Cc + (16 - Cc % 16 if lead == 0 else 5)
    xin = fenced.input(x, ldx, 127, lead_bytes=lead, oracle=lambda m: knn_ref.rnorm(m)[:, None], expected=exp[:, None])
    out = fenced.output(1, 3001, 3001, np.float32, expected=exp[None, :])
    _lib.call("ivit_rows_rnorm_i8_f32", xin.ptr, xin.ld, 3001, Cc, out.ptr, st())
    torch.cuda.synchronize()
    fenced.check(out, exp[None, :])
    fenced.check(xin)


def test_rnorm_refusals():
    L = _lib.lib()
    x = dev(np.ones((4, 64), np.int8))
    out = torch.full((4,), 7.0, dtype=torch.float32, device=DEV)
    p, o = _lib.ptr(x), _lib.ptr(out)
    assert L.ivit_rows_rnorm_i8_f32(None, 64, 4, 64, o, st()) == -1
    assert L.ivit_rows_rnorm_i8_f32(p, 63, 4, 64, o, st()) == -1
    assert L.ivit_rows_rnorm_i8_f32(p, 64, -1, 64, o, st()) == -1
    assert L.ivit_rows_rnorm_i8_f32(p, 64, 4, 0, o, st()) == -1
    assert L.ivit_rows_rnorm_i8_f32(p, 64, 4, 64, C.c_void_p(out.data_ptr() + 2), st()) == -1
    assert L.ivit_rows_rnorm_i8_f32(p, 64, 0, 64, o, st()) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# =========================================================================================== vote
def vote_gpu(idx, labels, w, r):
    Q, k = idx.shape
    classes = torch.full((Q, r), -9, dtype=torch.int32, device=DEV)
    votes = torch.full((Q, r), float("nan"), dtype=torch.float32, device=DEV)
    di, dl, dw = dev(idx), dev(labels), dev(w)          # held until the synchronisation: the pointers are all the call gets
    _lib.call("ivit_knn_vote_f32", _lib.ptr(di), _lib.ptr(dl), _lib.ptr(dw), Q, labels.size, k, r, _lib.ptr(classes), _lib.ptr(votes), st())
    torch.cuda.synchronize()
    return classes.cpu().numpy(), votes.cpu().numpy()


def check_vote(idx, labels, w, r):
    classes, votes = vote_gpu(idx, labels, w, r)
    rc, rv = knn_ref.vote(idx, labels, w, r)
    assert np.array_equal(classes, rc) and np.array_equal(knn_ref.bits(votes), knn_ref.bits(rv))
    return rc, rv


@pytest.mark.parametrize("k,r", [(1, 1), (5, 5), (20, 5), (200, 5), (256, 256)])
def test_vote_random(k, r):
    rng = np.random.default_rng(k)
    N, Q = 1000, 67
    labels = rng.integers(0, 13 if k < 200 else 1000, size=N).astype(np.int32)
    idx = np.stack([rng.permutation(N)[:k] for _ in range(Q)]).astype(np.int32)
    w = np.exp(rng.uniform(-1, 1, size=(Q, k)) / 0.07).astype(np.float32)      # 12 orders of magnitude: the order of the sum shows
    check_vote(idx, labels, w, r)


def test_vote_planted_ties_padding_and_supplied_weights():
    labels = np.array([9, 4, 9, 4, 2, 7, 7, 7], np.int32)
    idx = np.array([[0, 1, 2, 3, 4], [5, 6, 7, 5, 6], [4, 3, 2, 1, 0], [1, 3, 0, 2, 4]], np.int32)
    w = np.array([[1.0, 1.5, 0.5, 0.0, 1.5],          # labels 9, 4 and 2 all reach 1.5: ascending label
                  [0.25, 0.5, 1.0, 2.0, 4.0],         # one label: (7, 7.75) and four pads
                  [2.0 ** 24, 1.0, 1.0, 1.0, 1.0],    # float32, in rank order: 4 gets 1 + 1, 9 gets 1 + 1
                  [1.0, 2.0 ** 24, 1.0, 1.0, 0.0]], np.float32)
    rc, rv = check_vote(idx, labels, w, 5)
    assert rc[0].tolist() == [2, 4, 9, -1, -1] and rv[0].tolist() == [1.5, 1.5, 1.5, 0.0, 0.0]
    assert rc[1].tolist() == [7, -1, -1, -1, -1] and rv[1].tolist() == [7.75, 0.0, 0.0, 0.0, 0.0]
    assert rc[2].tolist()[:3] == [2, 4, 9] and rv[3, 0] == np.float32(2.0 ** 24)
    check_vote(idx[:, :1], labels, w[:, :1], 1)       # k = 1


def test_vote_refusals():
    L = _lib.lib()
    idx, lab, w = dev(np.zeros((2, 4), np.int32)), dev(np.zeros(8, np.int32)), dev(np.ones((2, 4), np.float32))
    classes = torch.full((2, 4), -9, dtype=torch.int32, device=DEV)
    votes = torch.full((2, 4), 3.0, dtype=torch.float32, device=DEV)
    a = (_lib.ptr(idx), _lib.ptr(lab), _lib.ptr(w))
    o = (_lib.ptr(classes), _lib.ptr(votes), st())
    assert L.ivit_knn_vote_f32(*a, 2, 8, 4, 0, *o) == -1
    assert L.ivit_knn_vote_f32(*a, 2, 8, 4, 5, *o) == -1
    assert L.ivit_knn_vote_f32(*a, 2, 8, 0, 1, *o) == -1
    assert L.ivit_knn_vote_f32(*a, 2, 8, 257, 1, *o) == -1
    assert L.ivit_knn_vote_f32(None, a[1], a[2], 2, 8, 4, 1, *o) == -1
    assert L.ivit_knn_vote_f32(*a, 0, 8, 4, 1, *o) == 0
    torch.cuda.synchronize()
    assert (classes == -9).all() and (votes == 3.0).all()


# =========================================================================================== refusals
def test_topk_refusals_leave_the_outputs_untouched():
    L = _lib.lib()
    rng = np.random.default_rng(8)
    N, Q, Cc = 300, 9, 128
    wide = dev(rand8(rng, N, 1088))                   # rows wide enough for every C tried
    qd = dev(rand8(rng, Q, 1088))
    rn = torch.ones(N, dtype=torch.float32, device=DEV)
    idx = torch.full((Q, 257), -7, dtype=torch.int32, device=DEV)
    score = torch.full((Q, 257), 5.0, dtype=torch.float32, device=DEV)
    ws = torch.full((Q * 64 * 257 + 8,), -3, dtype=torch.int64, device=DEV)
    big = ws.numel() * 8

    def run(q=qd, ldq=1088, Qn=Q, bank=wide, ldb=1088, Nn=N, Cn=Cc, rnorm=rn, k=5, splits=0, i=idx, s=score, w=ws, wb=big):
        p = _lib.ptr
        return L.ivit_knn_topk_i8(p(q), ldq, Qn, p(bank), ldb, Nn, Cn, p(rnorm), k, splits, p(i), p(s), p(w), wb, st())

    assert run(k=0) == -1 and run(k=301) == -1 and run(Nn=4, k=5) == -1
    assert run(k=257) == -2
    assert run(Cn=96) == -2 and run(Cn=1088) == -2 and run(Cn=0) == -2
    assert b"unsupported geometry" in L.ivit_last_error_string()
    assert run(splits=65) == -1 and run(splits=-1) == -1
    assert run(ldb=1088 + 8) == -1 and run(ldq=1088 + 4) == -1 and run(ldb=64) == -1
    assert run(bank=None) == -1 and run(q=None) == -1 and run(rnorm=None) == -1 and run(i=None) == -1 and run(s=None) == -1
    assert run(Qn=-1) == -1 and run(Nn=0) == -1
    need = C.c_int64()
    _lib.call("ivit_knn_workspace_bytes", Q, N, 5, 3, C.byref(need))
    assert need.value == Q * 3 * 5 * 8
    assert run(splits=3, wb=need.value - 1) == -1 and run(splits=3, w=None) == -1
    assert L.ivit_knn_workspace_bytes(Q, N, 301, 3, C.byref(need)) == -1 and L.ivit_knn_workspace_bytes(Q, N, 5, 65, C.byref(need)) == -1
    assert L.ivit_knn_workspace_bytes(Q, N, 257, 3, C.byref(need)) == -2 and L.ivit_knn_workspace_bytes(Q, N, 5, 3, None) == -1
    _lib.call("ivit_knn_workspace_bytes", Q, N, 5, 1, C.byref(need))
    assert need.value == 0
    torch.cuda.synchronize()
    assert (idx == -7).all() and (score == 5.0).all() and (ws == -3).all()
    assert run(splits=3, wb=Q * 3 * 5 * 8) == 0          # ... and the same call with the workspace it asked for runs
    torch.cuda.synchronize()
    ridx, _ = knn_ref.topk(qd.cpu().numpy()[:, :Cc], wide.cpu().numpy()[:, :Cc], 5, np.ones(N, np.float32))
    assert np.array_equal(idx.view(-1)[:Q * 5].view(Q, 5).cpu().numpy(), ridx)


# =========================================================================================== fenced operands
@pytest.mark.parametrize("splits", [1, 3])
def test_topk_fenced_operands(splits):
    rng = np.random.default_rng(9)
    N, Q, Cc, k = 150, 37, 128, 9
    bank, q = rand8(rng, N, Cc), rand8(rng, Q, Cc)
    q[0] = bank[0]
    rn = knn_ref.rnorm(bank)
    ridx, rsc = knn_ref.topk(q, bank, k, rn)

    def ones(a, width):
        return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=1)

    qf = fenced.input(q, Cc + 16, 127, oracle=lambda m: knn_ref.topk(m, ones(bank, m.shape[1]), k)[1], expected=rsc)
    bf = fenced.input(bank, Cc + 48, 127, oracle=lambda m: knn_ref.scores(ones(q, m.shape[1]), m).T, expected=knn_ref.scores(q, bank, rn).T)
    more = np.vstack([bank, bank[:1]])                # a kernel that reads rnorm[N] scores one row more, with the poison
    rf = fenced.input(rn[None, :], N, 1e30, oracle=lambda m: knn_ref.scores(q, more, m[0]).max(axis=1)[None, :], expected=rsc[:, 0][None, :])
    idx = fenced.output(Q, k, k, np.int32, expected=ridx)
    score = fenced.output(Q, k, k, np.float32, expected=rsc)
    ws, need = workspace(Q, N, k, splits)
    ldq = qf.ld
    ldb = bf.ld
    _lib.call("ivit_knn_topk_i8", qf.ptr, ldq, Q, bf.ptr, ldb, N, Cc, rf.ptr, k, splits, idx.ptr, score.ptr, _lib.ptr(ws), need, st())
    torch.cuda.synchronize()
    fenced.check(idx, ridx)
    fenced.check(score, rsc)
    for x in (qf, bf, rf):
        fenced.check(x)


# =========================================================================================== the Python layer and end to end
def test_feature_bank_search_and_classify():
    rng = np.random.default_rng(10)
    bank, q = rand8(rng, 500, 192), rand8(rng, 41, 192)
    labels = rng.integers(0, 10, size=500)
    store = dev(np.pad(bank, ((0, 0), (0, 64))))      # the bank as a view of a wider buffer: used in place
    fb = FeatureBank(store[:, :192], torch.from_numpy(labels).to(DEV), 0.04)
    assert fb.rows.data_ptr() == store.data_ptr() and fb.rows.stride(0) == 256
    ridx, rsc = knn_ref.topk(q, bank, 20)
    for sp in (0, 5):
        idx, cos = fb.search(dev(q), 20, splits=sp)
        assert np.array_equal(idx.cpu().numpy(), ridx)
        assert np.array_equal(knn_ref.bits(cos.cpu().numpy()), knn_ref.bits(knn_ref.cosine(rsc, q)))
    w = knn_weights(cos, 0.07)
    classes, votes = knn_classify(fb, dev(q), k=20, T=0.07, r=5)
    rc, rv = knn_ref.vote(ridx, labels.astype(np.int32), w.cpu().numpy(), 5)
    assert np.array_equal(classes.cpu().numpy(), rc) and np.array_equal(knn_ref.bits(votes.cpu().numpy()), knn_ref.bits(rv))
    with pytest.raises(TypeError, match="integers=True"):
        FeatureBank(store[:, :192].float(), torch.from_numpy(labels).to(DEV), 0.04)


class _Backbone:
    """a frozen synthetic DeiT-Tiny behind the interface extract_features drives"""

    def __init__(self, max_batch):
        fs, ranges, cfg, self.meta, _ = load_synthetic_model("deit_tiny")
        self.eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=DEV, max_batch=max_batch)
        self.num_features = cfg["embed_dim"]

    def eval(self):
        return self

    def features(self, x, integers=False, out=None):
        return self.eng.forward_features(x.contiguous().float(), integers, out=out)


def test_evaluate_knn_end_to_end():
    model = _Backbone(16)
    n = 48
    imgs = torch.from_numpy(synth.make_images(n, model.meta["image_seed"] + 1))
    labels = torch.arange(n) % 6
    loader = [(imgs[i:i + 16], labels[i:i + 16]) for i in range(0, n, 16)]
    feats = extract_features(model, loader, DEV, integers=True)[0].cpu().numpy()
    assert np.unique(feats, axis=0).shape[0] == n, "the test wants images with distinct embeddings"
    out = evaluate_knn(model, loader, loader, DEV, k=1)
    assert out == {1: (100.0, 100.0)}, "every image is its own nearest neighbour"
    # k = (1, 5): the classes are the reference vote on the neighbours and weights the calls produce
    rows, lab, scale = extract_features(model, loader, DEV, integers=True)
    assert rows.dtype == torch.int8 and rows.shape == (n, 192)
    fb = FeatureBank(rows, lab, scale)
    idx, cos = fb.search(rows, 5)
    ridx, rsc = knn_ref.topk(rows.cpu().numpy(), rows.cpu().numpy(), 5)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(knn_ref.bits(cos.cpu().numpy()), knn_ref.bits(knn_ref.cosine(rsc, rows.cpu().numpy())))
    w = knn_weights(cos, 0.07)
    got = evaluate_knn(model, loader, loader, DEV, k=(1, 5), T=0.07)
    for k in (1, 5):
        r = min(5, k)
        classes, _ = fb.vote(idx[:, :k], w[:, :k], r)
        rc, _ = knn_ref.vote(ridx[:, :k], lab.cpu().numpy().astype(np.int32), w.cpu().numpy()[:, :k], r)
        assert np.array_equal(classes.cpu().numpy(), rc)
        hit = rc == lab.cpu().numpy()[:, None]
        assert got[k] == (100.0 * hit[:, 0].sum() / n, 100.0 * hit.any(axis=1).sum() / n)
    assert got[1] == (100.0, 100.0)
