"""Linear probe on the int8 feature bank, without a GPU: the header's prototypes against the ctypes table, the numpy reference
(tests/probe_ref.py) against a direct int64 evaluation, and probe.py / inference.evaluate_linear_probe with `_lib.call` stubbed (as
tests/test_knn_cpu.py does) -- here by numpy stand-ins that work on the operands' memory, so that the whole pipeline runs.

The ridge bound.  numpy.linalg.solve is LU with partial pivoting, backward stable: the relative residual
|A V - R| / (|A| |V| + |R|) is of the order of C * 2^-53 = 2e-14 at C = 192; the test allows a margin of 50: 1e-12.  (The
generator's systems have condition numbers of about ten and residuals of about 1e-16 where this was written.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ivit_amd import _lib
import ivit_amd.inference as inference
import ivit_amd.probe as probe
from ivit_amd.prepare import LinearParams, pad_head

import probe_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ivit_gram_i8_i64", "ivit_gram_workspace_bytes", "ivit_group_sums_i8_i64")


def _prototype_kinds(name):
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ivit_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "const int32_t*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "void*": _lib.vp,
             "int": _lib.ci, "int64_t": _lib.i64, "ivit_stream_t": _lib.vp}
    return [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_prototypes_match_ctypes_table(name):
    assert _lib.SIGNATURES[name] == _prototype_kinds(name)


def test_header_constants_match_module():
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    assert int(re.search(r"#define IVIT_GROUPS_MAX (\d+)", header).group(1)) == probe.GROUPS_MAX == 2 ** 20
    assert int(re.search(r"#define IVIT_GRAM_SPLITS_MAX (\d+)", header).group(1)) == 64
    assert "ivit_stream_t" not in re.search(r"ivit_gram_workspace_bytes\s*\(([^)]*)\)", header).group(1)      # a host function


def test_package_exports():
    import ivit_amd
    assert ivit_amd.BankStats is probe.BankStats and ivit_amd.LinearProbe is probe.LinearProbe
    assert callable(inference.evaluate_linear_probe)


# ---------------------------------------------------------------------------- the reference against a direct int64 evaluation
@pytest.mark.parametrize("rows,C", [(0, 64), (1, 64), (65, 64), (300, 128)])
def test_reference_gram_equals_int64_evaluation(rows, C):
    rng = np.random.default_rng(rows + C)
    x = rng.integers(-128, 128, size=(rows, C)).astype(np.int8)
    if rows > 2:
        x[0], x[1, ::2], x[1, 1::2] = -128, -128, 127
    g = probe_ref.gram(x)
    assert g.dtype == np.int64 and np.array_equal(g, probe_ref.gram_direct(x)) and np.array_equal(g, g.T)


def test_reference_gram_beyond_int32():
    x = np.full((140000, 64), -128, np.int8)
    assert (probe_ref.gram(x) == 140000 * 2 ** 14).all() and 140000 * 2 ** 14 > 2 ** 31


def test_reference_group_sums_equal_a_loop_over_labels():
    rng = np.random.default_rng(3)
    x = rng.integers(-128, 128, size=(200, 64)).astype(np.int8)
    labels = rng.integers(2, 7, size=200)              # classes 0, 1, 7, 8 are empty
    perm, ptr = probe_ref.csr(labels, 9)
    assert ptr[0] == 0 and ptr[-1] == 200 and (np.diff(ptr) >= 0).all() and sorted(perm) == list(range(200))
    got = probe_ref.group_sums(x, perm, ptr)
    for k in range(9):
        assert np.array_equal(got[k], x[labels == k].astype(np.int64).sum(axis=0))
    G, S, n = probe_ref.stats(x, labels, 9)
    assert np.array_equal(S, got) and np.array_equal(n, np.bincount(labels, minlength=9))
    assert np.array_equal(S.sum(axis=0), x.astype(np.int64).sum(axis=0))


def test_reference_topk_rule():
    lg = np.array([[1.0, 3.0, 3.0, -0.0, 0.0], [2.0, 2.0, 2.0, 2.0, 2.0]], np.float32)
    assert probe_ref.topk(lg, 5).tolist() == [[1, 2, 0, 3, 4], [0, 1, 2, 3, 4]]
    assert probe_ref.hits(probe_ref.topk(lg, 3), [2, 0]).tolist() == [1, 1, 0]


# ---------------------------------------------------------------------------- probe.py with the library stubbed by numpy stand-ins
def _mem(addr, count, dtype):
    dtype = np.dtype(dtype)
    if count == 0:
        return np.empty(0, dtype)
    return np.frombuffer((ctypes.c_char * (count * dtype.itemsize)).from_address(addr), dtype=dtype)


def _rows(addr, rows, width, ld, dtype):
    if rows == 0:
        return np.empty((0, width), dtype)
    flat = _mem(addr, (rows - 1) * ld + width, dtype)
    return np.lib.stride_tricks.as_strided(flat, (rows, width), (ld * flat.itemsize, flat.itemsize))


def _fake(name, a):
    """the documented result of an entry, computed by probe_ref on the operands' memory"""
    if name == "ivit_gram_workspace_bytes":
        a[3]._obj.value = 4 * a[1] * a[1] if a[0] else 0
    elif name == "ivit_gram_i8_i64":
        x, ldx, rows, C, splits, accumulate, gram = a[:7]
        g = _mem(gram, C * C, np.int64)
        g[:] = (g if accumulate else 0) + probe_ref.gram(_rows(x, rows, C, ldx, np.int8)).reshape(-1)
    elif name == "ivit_group_sums_i8_i64":
        x, ldx, rows, C, perm, gptr, groups, accumulate, sums = a[:9]
        ptr = _mem(gptr, groups + 1, np.int64)
        s = _mem(sums, groups * C, np.int64)
        s[:] = (s if accumulate else 0) + probe_ref.group_sums(_rows(x, rows, C, ldx, np.int8), _mem(perm, int(ptr[-1]), np.int32), ptr).reshape(-1)
    elif name == "ivit_gemm_i8_i32":
        A, lda, W, ldw, bias, out, ldo, M, N, K = a[:10]
        acc = _rows(A, M, K, lda, np.int8).astype(np.int64) @ _rows(W, N, K, ldw, np.int8).astype(np.int64).T + _mem(bias, N, np.int32)[None, :]
        _rows(out, M, N, ldo, np.int32)[:] = acc
    elif name in ("ivit_head_topk", "ivit_head_argmax"):
        if name == "ivit_head_argmax":
            acc, s_acc, batch, ld, logits, top = a[:6]
            N, k, targets, hits = ld, 1, None, None
        else:
            acc, s_acc, batch, ld, N, k, logits, top, targets, hits = a[:10]
        lg = (_rows(acc, batch, ld, ld, np.int32).astype(np.float32) * _mem(s_acc, ld, np.float32)[None, :]).astype(np.float32)
        if logits is not None:
            _rows(logits, batch, ld, ld, np.float32)[:] = lg
        t = probe_ref.topk(lg[:, :N], k)
        _rows(top, batch, k, k, np.int32)[:] = t
        if targets is not None:
            _mem(hits, k, np.int64)[:] += probe_ref.hits(t, _mem(targets, batch, np.int32))
    else:
        raise AssertionError(f"unexpected call {name}")


@pytest.fixture
def calls(monkeypatch):
    rec = []

    def call(name, *args):
        rec.append((name, args))
        _fake(name, args)

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return rec


def names(calls):
    return [c[0] for c in calls]


def _batch(n=40, c=64, K=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 128, (n, c), generator=g, dtype=torch.int8), torch.randint(0, K, (n,), generator=g)


def test_update_argument_lists_and_statistics(calls):
    rows, labels = _batch()
    store = torch.zeros(40, 80, dtype=torch.int8)      # the rows as a view of a wider buffer: used in place
    store[:, :64] = rows
    st = probe.BankStats(64, 7, "cpu").update(store[:, :64], labels, 0.05)
    assert names(calls) == ["ivit_gram_workspace_bytes", "ivit_gram_i8_i64", "ivit_group_sums_i8_i64"]
    w, g, s = (c[1] for c in calls)
    assert w[:3] == (40, 64, 0)
    assert g[0] == store.data_ptr() and g[1:6] == (80, 40, 64, 0, 1) and g[6] == st.gram.data_ptr() and g[7] == st.workspace.data_ptr()
    assert g[8] == 4 * 64 * 64 <= st.workspace.numel() * 4
    assert s[0] == store.data_ptr() and s[1:4] == (80, 40, 64) and s[6:8] == (7, 1) and s[8] == st.sums.data_ptr()
    G, S, n = probe_ref.stats(rows.numpy(), labels.numpy(), 7)
    assert np.array_equal(st.gram.numpy(), G) and np.array_equal(st.sums.numpy(), S) and np.array_equal(st.counts.numpy(), n)
    assert st.gram.dtype == st.sums.dtype == st.counts.dtype == torch.int64 and st.scale == float(np.float32(0.05))      # scales are float32


def test_batches_and_merge_equal_one_update(calls):
    rows, labels = _batch(100)
    whole = probe.BankStats(64, 7, "cpu").update(rows, labels, 0.05)
    parts = probe.BankStats(64, 7, "cpu")
    for lo, hi in ((0, 16), (16, 16), (16, 70)):       # an empty batch among them: no call
        parts.update(rows[lo:hi], labels[lo:hi], 0.05)
    other = probe.BankStats(64, 7, "cpu").update(rows[70:], labels[70:], 0.05)
    parts.merge(other).all_reduce()                    # no process group: all_reduce changes nothing
    for a, b in ((whole.gram, parts.gram), (whole.sums, parts.sums), (whole.counts, parts.counts)):
        assert torch.equal(a, b)
    assert names(calls).count("ivit_gram_i8_i64") == 4
    with pytest.raises(ValueError, match="merge"):
        parts.merge(probe.BankStats(128, 7, "cpu"))
    with pytest.raises(ValueError, match="scale"):
        parts.merge(probe.BankStats(64, 7, "cpu").update(rows[:4], labels[:4], 0.06))


def test_from_bank(calls, monkeypatch):
    import ivit_amd.knn as knn
    rows, labels = _batch()
    fb = knn.FeatureBank.__new__(knn.FeatureBank)
    fb.rows, fb.labels, fb.scale, fb.N, fb.C = rows, labels.to(torch.int32), 0.05, 40, 64
    st = probe.BankStats.from_bank(fb, 7)
    assert np.array_equal(st.gram.numpy(), probe_ref.gram(rows.numpy())) and st.scale == float(np.float32(0.05)) and int(st.counts.sum()) == 40


def test_refusals_launch_nothing(calls):
    rows, labels = _batch()
    st = probe.BankStats(64, 7, "cpu")
    with pytest.raises(TypeError, match="integers=True"):
        st.update(rows.float(), labels)
    with pytest.raises(ValueError, match="multiple of 64"):
        probe.BankStats(96, 7, "cpu")
    with pytest.raises(ValueError, match="num_classes"):
        probe.BankStats(64, 0, "cpu")
    with pytest.raises(ValueError, match="channels"):
        st.update(torch.zeros(8, 128, dtype=torch.int8), labels[:8])
    with pytest.raises(ValueError, match="16-byte"):
        st.update(torch.zeros(8, 128, dtype=torch.int8)[:, 8:72], labels[:8])
    with pytest.raises(ValueError, match="labels"):
        st.update(rows, labels[:5])
    for bad in (-1, 7):
        lab = labels.clone()
        lab[11] = bad
        with pytest.raises(ValueError, match=f"label {bad} "):
            st.update(rows, lab)
    assert calls == [] and st.scale is None
    st.update(rows, labels, 0.05)
    n = len(calls)
    with pytest.raises(ValueError, match="scale"):
        st.update(rows, labels, torch.tensor([0.051]))
    assert len(calls) == n
    with pytest.raises(ValueError, match="scale is unknown"):
        probe.BankStats(64, 7, "cpu").update(rows, labels).ridge(0.1)


# ---------------------------------------------------------------------------- ridge, ncm and the integer parameters
GEN = probe_ref.generator()
LAMS = (1e-3, 1e-1, 1.0)


@pytest.fixture(scope="module")
def gen_stats():
    bank, labels = GEN[0], GEN[1]
    return probe_ref.stats(bank, labels, 10)


@pytest.mark.parametrize("lam", (1e-4,) + LAMS)
def test_ridge_residual(gen_stats, lam):
    G, S, n = gen_stats
    A, R, mu, N = probe_ref.ridge_system(G, S, n, lam)
    W, b = probe.ridge_solve(G.astype(np.float64), S.astype(np.float64), n.astype(np.float64), lam, GEN[4])
    rW, rb, V = probe_ref.ridge(G, S, n, lam, GEN[4])
    assert np.array_equal(W, rW) and np.array_equal(b, rb) and W.dtype == b.dtype == np.float32 and W.shape == (10, 192)
    res = np.linalg.norm(A @ V - R) / (np.linalg.norm(A) * np.linalg.norm(V) + np.linalg.norm(R))
    print(f"lam={lam}: relative residual {res:.3g}, condition number {np.linalg.cond(A):.3g}")
    assert res <= 1e-12


@pytest.mark.parametrize("lam", LAMS)
def test_reference_classifies_the_generator(gen_stats, lam):
    G, S, n = gen_stats
    bank, labels, q, targets, scale = GEN
    W, b, V = probe_ref.ridge(G, S, n, lam, scale)
    a = n / n.sum() - V.T @ (S.sum(axis=0) / n.sum())
    assert (np.argmax(q.astype(np.float64) @ V + a[None, :], axis=1) == targets).all()          # the float64 head
    acc, lg = probe_ref.int_logits(q, W, b, scale)
    assert (probe_ref.topk(lg, 1)[:, 0] == targets).all()                                         # the int8 head


def test_ridge_degenerate_cases_and_empty_class(calls):
    rows, labels = _batch(60, 64, 5)
    labels[labels == 3] = 2                             # class 3 is empty
    st = probe.BankStats(64, 5, "cpu").update(rows, labels, 0.05)
    p = st.ridge(0.1)
    assert not p.W[3].any() and p.b[3] == 0 and p.W[2].any()
    assert not st.ncm().W[3].any() and not st.ncm().b.any()
    with pytest.raises(ValueError, match="no rows"):
        probe.BankStats(64, 5, "cpu").update(rows[:0], labels[:0], 0.05).ridge(0.1)
    same = torch.full((9, 64), -128, dtype=torch.int8)
    with pytest.raises(ValueError, match="equal"):
        probe.BankStats(64, 5, "cpu").update(same, labels[:9], 0.05).ridge(0.1)


def test_ncm_equals_reference(calls):
    rows, labels = _batch(60, 64, 5)
    st = probe.BankStats(64, 5, "cpu").update(rows, labels, 0.05)
    G, S, n = probe_ref.stats(rows.numpy(), labels.numpy(), 5)
    W, b = probe_ref.ncm(S, n, st.scale)              # the scale as float32 holds it
    p = st.ncm()
    assert np.array_equal(p.W, W) and np.array_equal(p.b, b)
    assert np.allclose(np.linalg.norm(W.astype(np.float64) * st.scale, axis=1), 1.0, atol=1e-6)


def test_linear_probe_integer_parameters_are_linear_params(calls):
    rng = np.random.default_rng(1)
    W, b = rng.normal(size=(10, 64)).astype(np.float32), rng.normal(size=10).astype(np.float32)      # 10 classes: padded to 12
    p = probe.LinearProbe(W, b, 0.0371, "cpu")
    lp = LinearParams(W, b, 0.0371)
    W8, b32, s_acc, _ = pad_head(lp.W8, lp.b32, lp.s_acc)
    assert np.array_equal(p.params.W8, lp.W8) and np.array_equal(p.params.b32, lp.b32) and np.array_equal(p.params.s_acc, lp.s_acc)
    assert np.array_equal(p.W8.numpy(), W8) and np.array_equal(p.b32.numpy(), b32) and np.array_equal(p.s_acc.numpy(), s_acc)
    assert p.W8.dtype == torch.int8 and p.b32.dtype == torch.int32 and p.s_acc.dtype == torch.float32 and p.Np == 12
    q = torch.from_numpy(rng.integers(-128, 128, size=(9, 64)).astype(np.int8))
    acc, lg = p.logits(q)
    racc, rlg = probe_ref.int_logits(q.numpy(), W, b, 0.0371)
    assert np.array_equal(acc.numpy(), racc) and np.array_equal(lg.numpy(), rlg) and acc.shape == (9, 10)
    g = [c[1] for c in calls if c[0] == "ivit_gemm_i8_i32"][-1]
    assert g[0] == q.data_ptr() and g[1] == 64 and g[2] == p.W8.data_ptr() and g[3] == 64 and g[4] == p.b32.data_ptr() and g[6:10] == (12, 9, 12, 64)
    hits = torch.zeros(5, dtype=torch.int64)
    top = p.topk(q, 5, torch.arange(9, dtype=torch.int32), hits)
    assert np.array_equal(top.numpy(), probe_ref.topk(rlg, 5)) and hits.tolist() == probe_ref.hits(top.numpy(), np.arange(9)).tolist()
    t = [c[1] for c in calls if c[0] == "ivit_head_topk"][-1]
    assert t[3:6] == (12, 10, 5)                        # the padded classes never enter the selection
    for k in (0, 9):
        with pytest.raises(ValueError, match="k="):
            p.topk(q, k)
    with pytest.raises(ValueError, match="channels"):
        p.logits(torch.zeros(3, 128, dtype=torch.int8))


def test_load_into_copies_in_place(calls):
    rng = np.random.default_rng(2)
    p = probe.LinearProbe(rng.normal(size=(10, 64)).astype(np.float32), rng.normal(size=10).astype(np.float32), 0.05, "cpu")

    class M:
        head = torch.nn.Linear(64, 10)
    w, v = M.head.weight, M.head.weight._version
    p.load_into(M)
    assert M.head.weight is w and w._version > v and np.array_equal(w.detach().numpy(), p.W) and np.array_equal(M.head.bias.detach().numpy(), p.b)
    M.head = torch.nn.Linear(64, 11)
    with pytest.raises(ValueError, match="model.head"):
        p.load_into(M)


# ---------------------------------------------------------------------------- evaluate_linear_probe
def _fake_extract(scales):
    it = iter(scales)

    def extract(model, loader, device, *, transform=None, graph=False, integers=False):
        assert integers is True
        rows, labels = (GEN[0], GEN[1]) if loader == "bank" else (GEN[2], GEN[3])
        return torch.from_numpy(rows), torch.from_numpy(labels), next(it)
    return extract


def test_evaluate_linear_probe_equals_the_numpy_pipeline(calls, monkeypatch, gen_stats):
    s = torch.tensor([GEN[4]], dtype=torch.float32)
    monkeypatch.setattr(inference, "extract_features", _fake_extract([s, s]))
    out = inference.evaluate_linear_probe(None, "bank", "query", "cpu", 10, lam=LAMS)
    G, S, n = gen_stats
    scale = float(s[0])
    for lam in LAMS:
        W, b, _ = probe_ref.ridge(G, S, n, lam, scale)
        _, lg = probe_ref.int_logits(GEN[2], W, b, scale)
        assert out[lam] == probe_ref.percentages(probe_ref.topk(lg, 5), GEN[3]) == (100.0, 100.0)
    assert list(out) == list(LAMS)
    assert names(calls).count("ivit_gram_i8_i64") == 1 and names(calls).count("ivit_group_sums_i8_i64") == 1      # the statistics once
    assert names(calls).count("ivit_gemm_i8_i32") == len(LAMS) == names(calls).count("ivit_head_topk")              # one head GEMM per lam
    monkeypatch.setattr(inference, "extract_features", _fake_extract([s, s]))
    out = inference.evaluate_linear_probe(None, "bank", "query", "cpu", 10, kind="ncm")
    W, b = probe_ref.ncm(S, n, scale)
    assert list(out) == [None] and out[None] == probe_ref.percentages(probe_ref.topk(probe_ref.int_logits(GEN[2], W, b, scale)[1], 5), GEN[3])


def test_evaluate_linear_probe_refusals(calls, monkeypatch):
    monkeypatch.setattr(inference, "extract_features", _fake_extract([0.05, 0.051]))
    with pytest.raises(ValueError, match="scale"):
        inference.evaluate_linear_probe(None, "bank", "query", "cpu", 10)
    with pytest.raises(ValueError, match="kind"):
        inference.evaluate_linear_probe(None, "bank", "query", "cpu", 10, kind="logistic")
    monkeypatch.setattr(inference, "extract_features", _fake_extract([0.05, 0.05]))
    with pytest.raises(ValueError, match="label 9 "):
        inference.evaluate_linear_probe(None, "bank", "query", "cpu", 9)
    assert calls == []
