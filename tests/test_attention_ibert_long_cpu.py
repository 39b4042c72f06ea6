"""Long-row I-BERT attention (ivit_attention_fused_i8_ibert_long, 208 .. 1025 tokens) on the CPU: the C prototype against the ctypes
table, the yardstick of the GPU test (oracle torch_rowsum against torch.sum at every token count that test uses), the crafted rows
of tests/ibert_long_ref.py (each must discriminate the order of the row sum)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as orc

from ivit_amd import _lib
import ibert_long_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every token count of tests/test_gpu_attention_ibert_long.py (random cases and crafted rows)
TOKENS = (208, 209, 256, 301, 577, 655, 656, 785, 1000, 1024, 1025)


def test_ibert_long_prototype_matches_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int ivit_attention_fused_i8_ibert_long\(([^)]*)\);", hdr)
    assert m, "ivit_attention_fused_i8_ibert_long is not declared"
    kinds = {"const int8_t*": _lib.vp, "int8_t*": _lib.vp, "const float*": _lib.vp, "int": _lib.ci, "uint32_t": _lib.u32,
             "int32_t": _lib.i32, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    types = [re.sub(r"\s+\w+$", "", p.strip()) for p in m.group(1).split(",")]
    assert _lib.SIGNATURES["ivit_attention_fused_i8_ibert_long"] == [kinds[t] for t in types]
    # the arguments of ivit_attention_fused_i8_ibert, out_blocks and the stream included
    assert _lib.SIGNATURES["ivit_attention_fused_i8_ibert_long"] == _lib.SIGNATURES["ivit_attention_fused_i8_ibert"]


@pytest.mark.parametrize("T", TOKENS)
def test_oracle_rowsum_is_torch_sum(T):
    """the order the kernel is held to is torch's on the machine that runs this: bit for bit on non-integer rows, single rows (the
    softmax's view) and a batch of rows alike; and the rows are such that the order matters"""
    rng = np.random.default_rng(T)
    x = (rng.uniform(0.5, 1.5, size=(64, T)) * np.exp(-rng.uniform(0, 8, size=(64, T))) * 16384.0).astype(np.float32)
    ts = torch.from_numpy(x).sum(dim=-1).numpy()
    ours = np.array([orc.torch_rowsum(r) for r in x], np.float32)
    assert np.array_equal(ts.view(np.uint32), ours.view(np.uint32))
    single = np.array([torch.from_numpy(r).sum().item() for r in x[:8]], np.float32)
    assert np.array_equal(single.view(np.uint32), ours[:8].view(np.uint32))
    ltr = np.array([R.sum_left_to_right(r) for r in x], np.float32)
    assert (ltr != ours).any()


def test_crafted_rows_cover_the_cascade_classes():
    assert {R.cascade_class(T) for T, _, _ in R.CRAFTED} == {0, 1, 2}
    assert len(R.CRAFTED_B) >= 1 and set(R.CRAFTED_B) <= set(R.CRAFTED)
    assert {T for T, _, _ in R.CRAFTED} <= set(TOKENS)


@pytest.mark.parametrize("T,seed,bits", R.CRAFTED)
def test_crafted_row_discriminates_the_order_of_the_sum(T, seed, bits):
    """from the oracle alone: the probabilities with torch's order differ from those of the left-to-right float32 sum, and (rows of
    CRAFTED_B) from those of the per-lane sums joined by a tree; the row is a legal input (unique maximum, int8 scores)"""
    row = R.crafted_row(T, seed, bits)
    t = row["t"]
    assert t.dtype == np.int8 and t.size == T and int(t.max()) == row["qm"] and int((t == row["qm"]).sum()) == 1
    e = R.crafted_exponents(row)
    assert (e > 0).all() and e[row["pos"]] == np.array([bits], np.uint32).view(np.float32)[0]
    pt = R.probabilities(e, orc.torch_rowsum(e))
    pa = R.probabilities(e, R.sum_left_to_right(e))
    assert not np.array_equal(pt, pa)
    # x is about 0.4 * 2^30 and factor 3 or 4: the dominant key alone holds 38 or 51 of the 128
    assert 0 <= pt.min() and pt.max() <= 128 and pt.sum() <= 128 and pt[row["pos"]] >= 32 and pt[row["pos"]] != pa[row["pos"]]
    if (T, seed, bits) in R.CRAFTED_B:
        assert not np.array_equal(pt, R.probabilities(e, R.sum_lane_tree(e)))
    # torch itself agrees with the oracle on this row
    assert np.float32(torch.from_numpy(e).sum().item()) == orc.torch_rowsum(e)
