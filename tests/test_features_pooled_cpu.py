"""Pooled features on the CPU: the prototypes of the new entries against the ctypes table, the width check of the harness before any
loader is touched, the rounding rule, and the default keywords of extract_features on the path they always took."""
import os
import re

import pytest
import torch

from ivit_amd import _lib
from ivit_amd.engine_common import round_half_up_div
from ivit_amd.inference import extract_features, extract_features_parallel, pooled_width

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ivit_layernorm_pool_i8", "ivit_layernorm_pool_i16", "ivit_ibert_layernorm_pool_i8", "ivit_ibert_layernorm_pool_i16",
           "ivit_layernorm_pool_slab_rows", "ivit_layernorm_pool_workspace_bytes"]


@pytest.mark.parametrize("name", ENTRIES)
def test_prototypes_match_the_ctypes_table(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ivit_hip.h")).read(), flags=re.S)
    m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
    assert m, f"{name} is not declared"
    kind = lambda p: _lib.vp if "*" in p or "ivit_stream_t" in p else {"int": _lib.ci, "int64_t": _lib.i64, "float": _lib.f32}[p.split()[0]]
    assert _lib.SIGNATURES[name] == [kind(p.strip()) for p in m.group(1).split(",")]


class Stub:
    """a model without an engine: features() fills the rows, features_pooled() must not be reached by the defaults"""
    num_features = 512

    def eval(self):
        return self

    def features(self, x, integers=False, out=None):
        out.copy_(x[:, :1].to(out.dtype).expand_as(out))
        return out, 0.25

    def features_pooled(self, *a, **k):
        raise AssertionError("the default keywords must take the existing path")


class NoLoader:
    def __iter__(self):
        raise AssertionError("the loader was touched")

    __len__ = __iter__


@pytest.mark.parametrize("extract", [extract_features, extract_features_parallel])
@pytest.mark.parametrize("C,n_last,avgpool,W", [(768, 1, True, 1536), (192, 5, True, 1152), (96, 2, True, 288)])
def test_width_is_checked_before_the_loader(extract, C, n_last, avgpool, W):
    model = Stub()
    model.num_features = C
    with pytest.raises(ValueError, match=rf"W={W}\b.*64\.\.1024"):
        extract(model, NoLoader(), "cpu", integers=True, n_last=n_last, avgpool=avgpool)
    assert [pooled_width(Stub(), 1, True), pooled_width(Stub(), 2, False)] == [1024, 1024]


@pytest.mark.parametrize("s,T,want", [(0, 196, 0), (98, 196, 1), (97, 196, 0), (-98, 196, 0), (-99, 196, -1), (-294, 196, -1), (-295, 196, -2),
                                      (3, 2, 2), (-3, 2, -1), (-1, 2, 0), (127 * 1025, 1025, 127), (-128 * 1025, 1025, -128), (-7, 5, -1)])
def test_rounding_rule(s, T, want):
    assert round_half_up_div(s, T) == want


def test_default_keywords_take_the_existing_path():
    loader = [(torch.full((2, 3), 7.0), torch.tensor([1, 2])), (torch.full((1, 3), -3.0), torch.tensor([0]))]
    bank, labels, scale = extract_features(Stub(), loader, "cpu", integers=True)
    assert bank.dtype == torch.int8 and tuple(bank.shape) == (3, 512) and scale == 0.25
    assert bank[:, 0].tolist() == [7, 7, -3] and labels.tolist() == [1, 2, 0]
