"""Retrieval scoring without a GPU: knn.retrieval_ap against a plain loop of the original Oxford compute_ap on a hand-made case, and
the refusals of FeatureBank.ranks and inference.evaluate_retrieval that need no device."""
import numpy as np
import pytest
import torch

import ivit_amd
import ivit_amd.knn as knn
from ivit_amd import inference


def compute_ap(ranked, pos, junk):
    """the Oxford buildings compute_ap, line for line: ranked = the database rows in ranking order"""
    old_recall, old_precision, ap, intersect, j = 0.0, 1.0, 0.0, 0, 0
    for x in ranked:
        if x in junk:
            continue
        if x in pos:
            intersect += 1
        recall, precision = intersect / len(pos), intersect / (j + 1.0)
        ap += (recall - old_recall) * ((old_precision + precision) / 2.0)
        old_recall, old_precision = recall, precision
        j += 1
    return ap


def test_retrieval_ap_is_the_oxford_compute_ap():
    rankings = [[5, 2, 9, 0, 7, 3, 1, 8, 4, 6],      # junk (5) above the first positive (2), junk (7) between, junk (6) below
                [4, 8, 1, 0, 2, 3, 5, 6, 7, 9],      # the first positive at adjusted rank 0, one junk row
                [3, 1, 4, 0, 5, 9, 2, 6, 8, 7]]      # no junk
    pos, junk = [{2, 0, 1}, {4, 2}, {1, 9, 7}], [{5, 7, 6}, {0}, set()]
    ranks, flags, tptr = [], [], [0]
    for r, p, j in zip(rankings, pos, junk):
        listed = sorted(p) + sorted(j)
        ranks += [r.index(x) for x in listed]
        flags += [True] * len(p) + [False] * len(j)
        tptr.append(len(ranks))
    ap, prec = knn.retrieval_ap(torch.tensor(ranks, dtype=torch.int32), tptr, flags)
    assert ap.dtype == np.float64
    want = [compute_ap(r, p, j) for r, p, j in zip(rankings, pos, junk)]
    assert np.abs(ap - want).max() <= 1e-12
    # adjusted ranks: query 0 -> 0, 2, 4; query 1 -> 0, 3; query 2 -> 1, 5, 9
    assert np.abs(prec - [[1, 3 / 5, 3 / 5], [1, 2 / 4, 2 / 4], [0, 1 / 5, 3 / 10]]).max() <= 1e-12
    assert abs(knn.retrieval_ap(ranks, tptr, flags, junk=[False] * len(flags))[0][0] - compute_ap(rankings[0], pos[0], set())) <= 1e-12
    assert np.isnan(knn.retrieval_ap([3], [0, 0, 1], [True])[0][0])                # a query without a positive


def test_ranks_refuses_on_the_host():
    fb = knn.FeatureBank.__new__(knn.FeatureBank)
    fb.N, fb.C = 50, 64
    q = torch.zeros(2, 64, dtype=torch.int8)
    for bad in ([[1, 50], [2]], [[-1], [2]], [[1]], (np.array([0, 2, 1]), np.array([1, 2]))):
        with pytest.raises(ValueError, match="target"):
            fb.ranks(q, bad)
    fb.C = 1088
    with pytest.raises(ValueError, match="at most 1024"):
        fb.ranks(torch.zeros(2, 1088, dtype=torch.int8), [[1], [2]])
    assert ivit_amd.retrieval_ap is knn.retrieval_ap and knn.RANK_TARGETS_MAX == 256


def test_evaluate_retrieval_refuses_wide_features_before_the_loaders():
    model = type("Model", (), {"num_features": 768})()
    for kw in ({"n_last": 2}, {"wide": True}):          # (None for a loader: touching one is a TypeError)
        with pytest.raises(ValueError, match="1024"):
            inference.evaluate_retrieval(model, None, None, "cpu", [[0]], **kw)
