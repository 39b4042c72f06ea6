"""Object discovery without a GPU: the header's prototypes against the ctypes table, the host-side scoring (boxes_to_pixels, corloc)
on hand-made boxes, and the refusals that need no device."""
import os
import re

import pytest
import torch

from ivit_amd import _lib, discover
import ivit_amd.inference as inference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ("ivit_token_degrees_i8", "ivit_discover_boxes_i8"))
def test_prototypes_match_ctypes_table(name):
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert m, f"{name} is not declared"
    kinds = {"const int8_t*": _lib.vp, "const int32_t*": _lib.vp, "int32_t*": _lib.vp, "uint64_t*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64,
             "ivit_stream_t": _lib.vp}
    assert _lib.SIGNATURES[name] == [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]
    assert hasattr(_lib.lib(), name)
    assert int(re.search(r"#define IVIT_DISCOVER_GRID_MAX (\d+)", header).group(1)) == discover.GRID_MAX == 64
    assert int(re.search(r"#define IVIT_DISCOVER_K_MAX (\d+)", header).group(1)) == discover.K_MAX == 128


def test_boxes_to_pixels_and_corloc():
    px = discover.boxes_to_pixels(torch.tensor([[1, 2, 3, 2], [0, 0, 0, 0], [0, 0, 13, 13]], dtype=torch.int32), 16)
    assert px.tolist() == [[16, 32, 64, 48], [0, 0, 16, 16], [0, 0, 224, 224]]
    gts = [[[0, 0, 10, 10], [16, 32, 64, 64]],      # the second box: inter 48 * 16, union 48 * 32 -> 0.5, a hit
           [[8, 0, 24, 16]],                        # inter 8 * 16, union 24 * 16 -> 1 / 3
           []]                                      # no ground truth: 0
    hits, iou = discover.corloc(px, gts)
    assert hits.tolist() == [True, False, False] and iou.dtype == torch.float64
    assert iou.tolist() == [0.5, (8 * 16) / (24 * 16), 0.0]
    with pytest.raises(ValueError, match="3 boxes for 1 images"):
        discover.corloc(px, [[]])


@pytest.mark.parametrize("tokens,grid,k,text", [
    (torch.zeros(1, 65, 1088, dtype=torch.int8), (5, 13), 5, "C=1088"),
    (torch.zeros(1, 65, 64, dtype=torch.int8), (1, 65), 5, "Gw=65"),
    (torch.zeros(1, 65, 64, dtype=torch.int8), (5, 13), 0, "k=0"),
    (torch.zeros(1, 65, 64, dtype=torch.int8), (5, 13), 129, "k=129"),
    (torch.zeros(1, 65, 64), (5, 13), 5, "float32"),
    (torch.zeros(1, 64, 64, dtype=torch.int8), (5, 13), 5, r"\(1, 64, 64\)"),
    (torch.zeros(1, 65, 64, dtype=torch.int8), (5, 13), 5, "on the device"),      # no fallback on the host
])
def test_host_refusals(tokens, grid, k, text):
    with pytest.raises(_lib.IvitError, match=text):
        discover.discover_objects(tokens, grid, k)


def test_evaluate_object_discovery_refuses_before_the_loader():
    class NoEngine(torch.nn.Module):
        def forward_tokens(self, x, integers=False):
            raise AssertionError("not reached")

        def features_unsupported_reason(self):
            return "head_dim != 64"

    def loader():
        raise AssertionError("the loader was touched")
        yield

    with pytest.raises(ValueError, match="head_dim != 64"):
        inference.evaluate_object_discovery(NoEngine(), loader(), "cpu")
