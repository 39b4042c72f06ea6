"""k-means without a GPU: prototypes against the ctypes table, host refusals, partition_scores by hand, evaluate_clustering's refusals."""
import math
import os
import re

import pytest
import torch

from ivit_amd import _lib, cluster
import ivit_amd.inference as inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ("ivit_kmeans_assign_i8", "ivit_kmeans_update_i16"))
def test_prototypes_match_ctypes_table(name):
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "int8_t*": _lib.vp, "const int64_t*": _lib.vp, "int64_t*": _lib.vp, "int32_t*": _lib.vp, "int": _lib.ci,
             "int64_t": _lib.i64, "ivit_stream_t": _lib.vp}
    assert _lib.SIGNATURES[name] == [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]
    assert hasattr(_lib.lib(), name) and int(re.search(r"#define IVIT_KMEANS_K_MAX (\d+)", header).group(1)) == cluster.K_MAX == 65536


I8 = torch.zeros(10, 64, dtype=torch.int8)


@pytest.mark.parametrize("C,K,rows,text", [
    (1088, 3, I8, "C=1088"),
    (64, 65537, I8, "K=65537"),
    (64, 3, torch.zeros(10, 64), "float32"),
    (64, 11, I8, "K=11 above the N=10"),
    (64, 3, torch.zeros(10, 80, dtype=torch.int8)[:, 8:72], "misaligned rows"),
    (64, 3, I8, "on the device"),      # no fallback on the host
])
def test_host_refusals(C, K, rows, text):
    with pytest.raises(_lib.IvitError, match=text):
        cluster.KMeans(C, K, "cpu").fit(rows)


def test_partition_scores_on_a_hand_made_table():
    """n = 12, every margin 4: purity = 10 / 12; pairs: sum C(nij, 2) = 12, both margins 18, C(12, 2) = 66, expected 18 * 18 / 66 =
    54 / 11, ARI = (12 - 54 / 11) / (18 - 54 / 11) = 78 / 144; H = ln 3 twice, I = ln(3) / 3 + ln(9 / 4) / 2 + ln(3 / 4) / 6"""
    table = [[4, 0, 0], [0, 3, 1], [0, 1, 3]]
    labels = [i for i, row in enumerate(table) for n in row for _ in range(n)]
    targets = [j for row in table for j, n in enumerate(row) for _ in range(n)]
    got = cluster.partition_scores(torch.tensor(labels, dtype=torch.int32), torch.tensor(targets))
    mi = math.log(3) / 3 + math.log(9 / 4) / 2 + math.log(3 / 4) / 6
    assert got["purity"] == 10 / 12 and got["ARI"] == pytest.approx(78 / 144, rel=1e-12) and got["NMI"] == pytest.approx(mi / math.log(3), rel=1e-12)


@pytest.mark.parametrize("width,kw,text", [(1088, {}, "C=1088"), (192, dict(wide=True), "no wide assignment kernel"),
                                           (384, dict(n_last=4), "W=1536"), (192, dict(num_clusters=0), "num_clusters=0")])
def test_evaluate_clustering_refuses_before_the_loader(width, kw, text):
    class Model(torch.nn.Module):
        num_features = width

    def loader():
        raise AssertionError("the loader was touched")
        yield

    with pytest.raises(ValueError, match=text):
        inference.evaluate_clustering(Model(), loader(), "cpu", **{"num_clusters": 5, **kw})
