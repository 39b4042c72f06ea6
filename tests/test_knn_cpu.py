"""k-NN on the int8 feature bank, without a GPU: the header's prototypes against the ctypes table, knn.py and inference.evaluate_knn
with `_lib.call` stubbed (as tests/test_attention_long_cpu.py does), and the numpy reference (tests/knn_ref.py) against a brute-force
loop on a small case with planted ties."""
import os
import re

import numpy as np
import pytest
import torch

from ivit_amd import _lib
import ivit_amd.inference as inference
import ivit_amd.knn as knn

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ivit_rows_rnorm_i8_f32", "ivit_knn_topk_i8", "ivit_knn_workspace_bytes", "ivit_knn_vote_f32")


def _prototype_kinds(name):
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ivit_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "const int32_t*": _lib.vp, "int32_t*": _lib.vp, "const float*": _lib.vp, "float*": _lib.vp, "void*": _lib.vp,
             "int64_t*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64, "ivit_stream_t": _lib.vp}
    return [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_prototypes_match_ctypes_table(name):
    assert _lib.SIGNATURES[name] == _prototype_kinds(name)


def test_header_constants_match_module():
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    assert int(re.search(r"#define IVIT_KNN_K_MAX (\d+)", header).group(1)) == knn.K_MAX == 256
    assert int(re.search(r"#define IVIT_KNN_SPLITS_MAX (\d+)", header).group(1)) == knn.SPLITS_MAX == 64
    assert "ivit_stream_t" not in re.search(r"ivit_knn_workspace_bytes\s*\(([^)]*)\)", header).group(1)      # a host function


# ---------------------------------------------------------------------------- knn.py with the library stubbed
@pytest.fixture
def calls(monkeypatch):
    class Rec(list):
        pass
    rec = Rec()
    ws_per = {"bytes": lambda Q, N, k, splits: Q * max(splits, 2) * k * 8}

    def call(name, *args):
        rec.append((name, args))
        if name == "ivit_knn_workspace_bytes":
            args[-1]._obj.value = ws_per["bytes"](*args[:4])

    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    rec.ws = ws_per
    return rec


def _bank(n=40, c=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 128, (n, c), generator=g, dtype=torch.int8), torch.arange(n) % 7


def names(calls):
    return [c[0] for c in calls]


def test_bank_is_a_view_and_rnorm_is_computed_once(calls):
    rows, labels = _bank()
    fb = knn.FeatureBank(rows, labels, 0.05)
    assert fb.rows.data_ptr() == rows.data_ptr() and names(calls) == ["ivit_rows_rnorm_i8_f32"]
    name, a = calls[0]
    assert a[0] == rows.data_ptr() and a[1:4] == (64, 40, 64) and a[4] == fb.rnorm.data_ptr()
    fb.search(rows[:5], 3)
    fb.search(rows[:5], 3)
    assert names(calls).count("ivit_rows_rnorm_i8_f32") == 3          # the bank's once, the queries' per search
    assert [c[1][0] for c in calls if c[0] == "ivit_rows_rnorm_i8_f32"][1:] == [rows.data_ptr()] * 2


def test_search_arguments_and_workspace_regrowth(calls):
    rows, labels = _bank()
    fb = knn.FeatureBank(rows, labels, 0.05)
    idx, cos = fb.search(rows[:5], 3, splits=4)
    assert idx.shape == cos.shape == (5, 3) and idx.dtype == torch.int32 and cos.dtype == torch.float32
    a = [c[1] for c in calls if c[0] == "ivit_knn_topk_i8"][-1]
    assert a[1:3] == (64, 5) and a[3] == rows.data_ptr() and a[4:7] == (64, 40, 64) and a[7] == fb.rnorm.data_ptr() and a[8:10] == (3, 4)
    assert a[12] == fb.workspace.data_ptr() and a[13] == 5 * 4 * 3 * 8 and fb.workspace.numel() * 8 >= a[13]
    first = fb.workspace
    fb.search(rows[:4], 2, splits=4)                                   # smaller: the workspace is kept
    assert fb.workspace is first
    fb.search(rows[:9], 7, splits=8)                                   # larger: regrown
    a = [c[1] for c in calls if c[0] == "ivit_knn_topk_i8"][-1]
    assert fb.workspace is not first and fb.workspace.numel() * 8 >= 9 * 8 * 7 * 8 == a[13] and a[12] == fb.workspace.data_ptr()
    calls.ws["bytes"] = lambda Q, N, k, splits: 0                      # one segment: no workspace is handed over
    fb.search(rows[:9], 7)
    a = [c[1] for c in calls if c[0] == "ivit_knn_topk_i8"][-1]
    assert a[12] is None and a[13] == 0
    n = len(calls)
    idx, cos = fb.search(rows[:0], 3)                                  # no queries: no call
    assert idx.shape == (0, 3) and len(calls) == n


def test_refusals(calls):
    rows, labels = _bank()
    with pytest.raises(TypeError, match="integers=True"):
        knn.FeatureBank(rows.float(), labels, 0.05)
    fb = knn.FeatureBank(rows, labels, 0.05)
    with pytest.raises(TypeError, match="integers=True"):
        fb.search(rows[:3].float(), 2)
    for k in (0, 41, 300):
        with pytest.raises(ValueError, match="k="):
            fb.search(rows[:3], k)
    with pytest.raises(ValueError, match="splits"):
        fb.search(rows[:3], 2, splits=65)
    with pytest.raises(ValueError, match="channels"):
        fb.search(torch.zeros(3, 128, dtype=torch.int8), 2)
    with pytest.raises(ValueError, match="multiple of 64"):
        knn.FeatureBank(torch.zeros(8, 96, dtype=torch.int8), labels[:8], 0.05)
    with pytest.raises(ValueError, match="16-byte"):
        knn.FeatureBank(torch.zeros(8, 128, dtype=torch.int8)[:, 8:72], labels[:8], 0.05)      # a view that is not aligned: no copy is made
    with pytest.raises(ValueError, match="labels"):
        knn.FeatureBank(rows, labels[:5], 0.05)
    with pytest.raises(ValueError, match="r="):
        fb.vote(torch.zeros(3, 4, dtype=torch.int32), torch.ones(3, 4), 5)
    assert "ivit_knn_topk_i8" not in names(calls) and "ivit_knn_vote_f32" not in names(calls)


def test_knn_classify_calls(calls):
    rows, labels = _bank()
    fb = knn.FeatureBank(rows, labels, 0.05)
    classes, votes = knn.knn_classify(fb, rows[:6], k=10, r=5)
    assert classes.shape == votes.shape == (6, 5)
    a = [c[1] for c in calls if c[0] == "ivit_knn_vote_f32"][-1]
    assert a[1] == fb.labels.data_ptr() and a[3:7] == (6, 40, 10, 5) and fb.labels.dtype == torch.int32


def _fake_extract(scales, n_bank=50, n_query=9):
    it = iter(scales)

    def extract(model, loader, device, *, transform=None, graph=False, integers=False):
        assert integers is True
        rows, labels = _bank(n_bank if loader == "bank" else n_query, seed=1 if loader == "bank" else 2)
        return rows, labels.to(torch.int64), next(it)
    return extract


def test_evaluate_knn_makes_one_search_at_max_k(calls, monkeypatch):
    monkeypatch.setattr(inference, "extract_features", _fake_extract([torch.tensor([0.05]), torch.tensor([0.05])]))
    out = inference.evaluate_knn(None, "bank", "query", "cpu", k=(20, 3, 10), T=0.07)
    assert sorted(out) == [3, 10, 20] and all(len(v) == 2 for v in out.values())
    searches = [c[1] for c in calls if c[0] == "ivit_knn_topk_i8"]
    assert len(searches) == 1 and searches[0][8] == 20 and searches[0][2] == 9
    votes = [c[1] for c in calls if c[0] == "ivit_knn_vote_f32"]
    assert [(v[5], v[6]) for v in votes] == [(3, 3), (10, 5), (20, 5)]          # prefixes of the one search, r = min(5, k)


def test_evaluate_knn_refuses_a_scale_mismatch_and_k_above_n(calls, monkeypatch):
    monkeypatch.setattr(inference, "extract_features", _fake_extract([0.05, 0.051]))
    with pytest.raises(ValueError, match="scale"):
        inference.evaluate_knn(None, "bank", "query", "cpu", k=(5,))
    monkeypatch.setattr(inference, "extract_features", _fake_extract([0.05, 0.05]))
    with pytest.raises(ValueError, match="k=51"):
        inference.evaluate_knn(None, "bank", "query", "cpu", k=(5, 51))
    assert "ivit_knn_topk_i8" not in names(calls)


def test_package_exports():
    import ivit_amd
    assert ivit_amd.FeatureBank is knn.FeatureBank and ivit_amd.knn_classify is knn.knn_classify


# ---------------------------------------------------------------------------- the reference helper against a brute-force loop
def _planted():
    rng = np.random.default_rng(5)
    q = rng.integers(-128, 128, size=(7, 64)).astype(np.int8)
    bank = rng.integers(-128, 128, size=(9, 64)).astype(np.int8)
    bank[4] = bank[1]            # equal rows: equal scores for every query
    bank[7] = bank[1]
    bank[6] = 0                  # a zero row: rnorm 0, score +0
    bank[3] = 0
    q[2] = 0                     # a zero query: every score is 0, indices ascend
    return q, bank


def test_reference_equals_brute_force_with_planted_ties():
    q, bank = _planted()
    for k in (1, 4, 9):
        idx, sc = knn_ref.topk(q, bank, k)
        bidx, bsc = knn_ref.topk_brute(q, bank, k)
        assert np.array_equal(idx, bidx) and np.array_equal(knn_ref.bits(sc), knn_ref.bits(bsc))
    idx, sc = knn_ref.topk(q, bank, 9)
    assert list(idx[2]) == list(range(9)) and not sc[2].any()
    for i in (0, 1, 3, 4, 5, 6):           # the planted equal rows follow each other in index order (query 2 ties with everything)
        pos = [list(idx[i]).index(j) for j in (1, 4, 7)]
        assert pos == list(range(pos[0], pos[0] + 3))
    rn = knn_ref.rnorm(bank)
    assert rn[3] == 0 and rn[6] == 0 and rn.dtype == np.float32
    full = np.full((1, 1024), -128, np.int8)
    assert knn_ref.rnorm(full)[0] == np.float32(2.0 ** -12) and knn_ref.scores(full, full)[0, 0] == np.float32(4096.0)


def test_reference_vote():
    idx = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32)
    labels = np.array([5, 2, 5, 2], np.int32)
    w = np.array([[1.0, 1.5, 0.5, 0.0], [0.25, 0.25, 0.25, 0.25]], np.float32)
    classes, votes = knn_ref.vote(idx, labels, w, 3)
    assert classes.tolist() == [[2, 5, -1], [2, 5, -1]] and votes.tolist() == [[1.5, 1.5, 0.0], [0.5, 0.5, 0.0]]
    # float32, sequential: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not
    w = np.array([[2.0 ** 24, 1.0, 1.0], [1.0, 1.0, 2.0 ** 24]], np.float32)
    classes, votes = knn_ref.vote(np.array([[0, 2, 2], [0, 2, 2]], np.int32), labels, w, 1)
    assert votes[:, 0].tolist() == [2.0 ** 24, 2.0 ** 24 + 2]
