"""The wrapper entries of the fused ViT attention agree byte for byte: every exported entry fills the same launcher's descriptor, so
ivit_attention_fused_i8 == _ex == _compat == _compat_band == _wide(8), _long == _wide_long(8), _ibert == _ibert_wide(8).  The first
member of each group is also compared with the oracle.  B = 1, H = 2; a one-hot row, a flat row and random rows (attention_ref.inputs);
T = 50: the general-T form, 197: the 13-tile form, 209: a partial key tile in the narrow long form, 657: the first wide long form
with a partial tile."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402
import attention_ref as A  # noqa: E402
from attention_ref import release  # noqa: E402,F401  (the autouse fixture)
import ibert_long_ref as R  # noqa: E402

S = "ivit_attention_fused_i8"


def _ibert_table():
    """the synthetic (row max, q) table of tests/test_gpu_ops.py::test_attention_fused_ibert"""
    prof = np.floor(16384.0 * np.exp(-np.arange(256) / 9.0))                # exp-like, 0 beyond ~90 steps
    tab = np.zeros((256, 256), np.float32)
    for qm in range(256):
        for qq in range(qm + 1):
            v = prof[qm - qq]
            tab[qm, qq] = np.float32(v) if (qm - qq == 0 and qm % 3 == 0) else np.float32(v * (1.0 + ((qm * 7 + qq) % 5 - 2) * 2.0 ** -22))
    return tab


def _shiftmax_group(T, form):
    """-> [(entry, the arguments between head_dim and out_blocks)] of the entries that must agree, the reference one first"""
    natural = form != "pow2"
    s_at, ms, es, mo, eo = A.scales(natural, 1.0, 8)
    head = (int(ms[0]), int(es[0]), float(s_at), int(mo[0]), int(eo[0]))
    exp2d, band, bw = A.shiftmax_tables(s_at, form)
    if T > 207:
        group = [(S + "_long", head + (exp2d, band, bw)), (S + "_wide_long", head + (exp2d, band, bw, 8))]
    elif natural:
        group = [(S + "_compat_band", head + (exp2d, band, bw)), (S + "_wide", head + (exp2d, band, bw, 8))]
    else:
        group = [(S, head), (S + "_ex", head), (S + "_compat", head + (None,)), (S + "_compat_band", head + (None, None, 0)),
                 (S + "_wide", head + (None, None, 0, 8))]
    return group, (s_at, ms, es, mo, eo, natural)


@pytest.mark.parametrize("T,form", [(50, "pow2"), (197, "pow2"), (50, "band"), (197, "band"), (209, "pow2"), (657, "pow2"),
                                    (209, "band"), (657, "band")])
def test_shiftmax_entries_agree(T, form):
    qkv = A.inputs(np.random.default_rng(900 + T), 1, 2, T)
    group, (s_at, ms, es, mo, eo, natural) = _shiftmax_group(T, form)
    exp, P, _ = A.expected(qkv, s_at, ms, es, mo, eo, natural, 8)
    # on the EXPECTED probabilities: key 17 alone carries query 5 (close to the 8-bit one, 127), query 6 gives every key the same
    assert P[5].sum() == P[5, 17] >= 100 and len(set(P[6].tolist())) == 1, "query 5 is not a one-hot row, or query 6 not a flat one"
    first = A.launch(group[0][0], qkv, group[0][1], 0)
    assert np.array_equal(first, exp), f"{group[0][0]}: {(first != exp).sum()} of {exp.size} differ from the oracle"
    assert np.abs(exp).max() > 5
    for name, tail in group[1:]:
        got = A.launch(name, qkv, tail, 0)
        assert np.array_equal(got, first), f"{name} != {group[0][0]}: {(got != first).sum()} of {got.size} bytes"


@pytest.mark.parametrize("band", [False, True], ids=["table", "band"])
def test_ibert_entries_agree(band):
    T = 197
    rng = np.random.default_rng(900 + T)
    qkv = np.clip(np.rint(rng.normal(0, 30, size=(3, 1, 2, T, A.HD))), -128, 127).astype(np.int8)
    qkv[0, 0, 0, 5] = 0
    qkv[0, 0, 0, 5, :8] = 127                       # a query with one dominant key -> one-hot row, p = 128
    qkv[1, 0, 0] = np.clip(qkv[1, 0, 0], -20, 20)
    qkv[1, 0, 0, 17, :8] = 127
    qkv[0, 0, 0, 6] = 0                             # a flat row
    ms, es = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))
    mo, eo = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -3))
    tab = _ibert_table()
    exp, n128, _ = R.expected(qkv, ms, es, mo, eo, tab)
    assert n128 > 0 and np.abs(exp).max() > 20
    first = A.run_ibert(S + "_ibert", qkv, ms, es, mo, eo, tab, band, 0)
    assert np.array_equal(first, exp), f"{(first != exp).sum()} of {exp.size} differ from the specification"
    got = A.run_ibert(S + "_ibert_wide", qkv, ms, es, mo, eo, tab, band, 0)
    assert np.array_equal(got, first), f"{(got != first).sum()} of {got.size} bytes"
