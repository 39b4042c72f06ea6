"""The wide feature-bank range on the CPU: the wide= keyword of the harness' width check and the prototypes of the four wide entries
against the ctypes table."""
import pytest

from ivit_amd.inference import extract_features, pooled_width
from test_features_pooled_cpu import NoLoader, Stub, test_prototypes_match_the_ctypes_table as _prototype


def test_wide_keyword_of_the_width_check():
    model = Stub()
    model.num_features = 768
    assert pooled_width(model, 1, True, wide=True) == 1536 and pooled_width(model, 4, True, wide=True) == 3840
    with pytest.raises(ValueError, match=r"W=1536\b.*64\.\.1024.*pass wide=True"):
        pooled_width(model, 1, True)
    model.num_features = 1024
    for extract in (pooled_width, lambda m, *a, **k: extract_features(m, NoLoader(), "cpu", integers=True, n_last=a[0], avgpool=a[1], **k)):
        with pytest.raises(ValueError, match=r"W=5120\b.*64\.\.4096"):
            extract(model, 4, True, wide=True)


@pytest.mark.parametrize("name", ["ivit_knn_topk_i8_wide", "ivit_gram_i8_i64_wide", "ivit_gram_wide_workspace_bytes", "ivit_group_sums_i8_i64_wide"])
def test_prototypes_match_the_ctypes_table(name):
    _prototype(name)
