"""Percentile calibration, without a GPU: the formula ivit_quantile_pair_f32 implements is pinned against torch.quantile (through its
numpy restatement, tests/quantile_ref.py -- not through the code under test), and QuantAct / the harness launch what they should
(`_lib.call` stubbed)."""
import os
import re

import numpy as np
import pytest
import torch

import ivit_amd as ivit
import ivit_amd.quantization_utils as qu
from ivit_amd import _lib, inference
from ivit_amd.quantization_utils import quant_modules as qm

import quantile_ref as qr
from test_engine_launch_trace import stubbed  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = (50, 99, 99.9, 99.99, 99.999, 100)
NS = (1, 2, 3, 7, 100, 1001, 65537, 2 ** 20)


def _inputs(n, rng):
    s = np.float32(0.0173)
    yield "normal", (rng.standard_normal(n) * 3).astype(np.float32)
    yield "ties", (s * rng.integers(-128, 128, n).astype(np.float32)).astype(np.float32)
    yield "equal", np.full(n, 1.25, np.float32)
    yield "two", np.where(rng.random(n) < 0.3, np.float32(-2.5), np.float32(7.0)).astype(np.float32)
    yield "negative", (-np.abs(rng.standard_normal(n)) - 0.5).astype(np.float32)


@pytest.mark.parametrize("n", NS)
def test_restatement_equals_torch_quantile(n):
    rng = np.random.default_rng(1000 + n)
    for kind, x in _inputs(n, rng):
        xt = torch.from_numpy(x)
        for p in PS:
            q_lo, q_hi = qr.percentile_qs(p)
            want = [torch.quantile(xt, float(q)).numpy() for q in (q_lo, q_hi)]
            got = qr.quantile_pair(x, q_lo, q_hi)
            assert qr.same_bits(got, want), (kind, n, p, got, want)
            assert qr.same_bits([qr.quantile(x, q_lo), qr.quantile(x, q_hi)], want), (kind, n, p)


def test_one_sort_for_many_q_gives_the_same_bits():
    """torch.quantile with a tensor of q (one sort; what the GPU tests compare with) equals the scalar calls the reference makes"""
    rng = np.random.default_rng(5)
    for n in (2, 3, 1001, 65537):
        x = torch.from_numpy((rng.standard_normal(n) * 3).astype(np.float32))
        qs = np.array([v for p in PS for v in qr.percentile_qs(p)], np.float32)
        many = torch.quantile(x, torch.from_numpy(qs)).numpy()
        one = np.array([torch.quantile(x, float(v)).numpy() for v in qs], np.float32)
        assert np.array_equal(many.view(np.int32), one.view(np.int32))


def test_restatement_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for x, q in (([1, inf, 2], 1.0), ([1, inf, 2], 0.75), ([-inf, 0, 3, inf], 0.5), ([1, nan, 2], 0.3), ([-0.0, 0.0, -0.0], 0.5)):
        x = np.array(x, np.float32)
        want = torch.quantile(torch.from_numpy(x), float(np.float32(q))).numpy()
        assert qr.same_bits(qr.quantile(x, q), want), (x, q, want)
    assert np.isnan(torch.quantile(torch.tensor([1.0, float("inf"), 2.0]), 1.0))       # the case the header cites


def test_percentile_qs_are_the_references_expressions():
    for p in PS + (99.5, 0):
        lo, hi = qm.percentile_qs(p)
        assert lo == float(np.float32((100 - p) / 2 / 100.0)) and hi == float(np.float32((100 - (100 - p) / 2) / 100.0))
        assert (np.float32(lo), np.float32(hi)) == qr.percentile_qs(p)


# ----------------------------------------------------------------------------------- launches (stubbed _lib.call)
@pytest.fixture
def launches(stubbed, monkeypatch):  # noqa: F811
    """the stubbed `_lib.call`, except that the two statistics entries also leave (-1, 1) in their output"""
    def record(name, *args):
        if name == "ivit_minmax_f32":
            args[2].tensor.copy_(torch.tensor([-1.0, 1.0]))
        if name == "ivit_quantile_pair_f32":
            args[4].tensor.copy_(torch.tensor([-1.0, 1.0]))
        stubbed.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    monkeypatch.setattr(qm, "_QUANTILE_WS", {})
    return stubbed


def _stat_calls(calls):
    return [(n, a) for n, a in calls if n in ("ivit_minmax_f32", "ivit_quantile_pair_f32")]


def test_quantact_percentile_launches_one_quantile_pair(launches):
    qa = qu.QuantAct()
    assert qa.percentile is None
    qa.percentile = 99.9
    x = torch.randn(2, 5, 8)
    qa(x, torch.ones(1))
    (name, a), = _stat_calls(launches)
    assert name == "ivit_quantile_pair_f32" and len(a) == len(_lib.SIGNATURES[name])
    assert a[1] == x.numel() == 80
    assert (np.float32(a[2]), np.float32(a[3])) == (np.float32((100 - 99.9) / 2 / 100.0), np.float32((100 - (100 - 99.9) / 2) / 100.0))
    assert a[5].tensor.numel() * a[5].tensor.element_size() == a[6] == _lib.QUANTILE_WS_BYTES
    assert a[4].tensor.dtype == torch.float32 and a[4].tensor.numel() == 2
    assert (float(qa.x_min), float(qa.x_max)) == (-1.0, 1.0)
    # with an identity: the sum is what is observed, once
    del launches[:]
    ident = torch.randn(1, 5, 8)
    qa(x, torch.ones(1), identity=ident, identity_scaling_factor=torch.ones(1))
    (name, a2), = _stat_calls(launches)
    assert name == "ivit_quantile_pair_f32" and a2[1] == 80
    assert torch.equal(a2[0].tensor, (ident + x).contiguous())
    assert a2[5].tensor is a[5].tensor                     # the workspace is allocated once per device
    # input mode
    del launches[:]
    qa(x)
    assert [n for n, _ in _stat_calls(launches)] == ["ivit_quantile_pair_f32"]
    # a fixed QuantAct observes nothing
    del launches[:]
    qa.fix()
    qa(x, torch.ones(1))
    assert _stat_calls(launches) == []


def test_quantact_without_percentile_launches_one_minmax(launches):
    qa = qu.QuantAct()
    x = torch.randn(3, 7)
    qa(x, torch.ones(1))
    (name, a), = _stat_calls(launches)
    assert name == "ivit_minmax_f32" and a[1] == 21


def test_per_channel_still_raises():
    with pytest.raises(NotImplementedError):
        qu.QuantAct(per_channel=True, channel_len=4)


def test_set_act_percentile_reaches_every_quantact():
    model = ivit.VisionTransformer(embed_dim=192, depth=2, num_heads=3, num_classes=10, gelu_type="ibert", softmax_type="ibert",
                                   layernorm_type="ibert")
    acts = [m for m in model.modules() if isinstance(m, qu.QuantAct)]
    inner = model.blocks[0].attn.int_softmax.act
    assert type(model.blocks[0].attn.int_softmax).__name__ == "IBERTIntSoftmax" and isinstance(inner, qu.QuantAct)
    assert len(acts) > 20 and all(m.percentile is None for m in acts)
    assert inference.set_act_percentile(model, 99.9) is model
    assert all(m.percentile == 99.9 for m in acts) and inner.percentile == 99.9
    assert not any("percentile" in k for k in model.state_dict())          # an attribute, not a buffer: never saved
    inference.set_act_percentile(model, None)
    assert all(m.percentile is None for m in acts)


def test_calibrate_model_act_percentile_keyword():
    class Probe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.act = qu.QuantAct()
            self.seen = []

        def forward(self, x):
            self.seen.append(self.act.percentile)
            return x

    m = Probe()
    inference.calibrate_model(m, "cpu", [torch.zeros(1)])
    inference.calibrate_model(m, "cpu", [torch.zeros(1), (torch.zeros(1), 0)], act_percentile=99.99)
    assert m.seen == [None, 99.99, 99.99]


def test_reference_trace_through_the_restatement(launches, monkeypatch):
    """tests/golden/qact_percentile_trace.npz (the reference's QuantAct, step by step) against this package's QuantAct with the kernel
    replaced by the numpy restatement: q values, what is observed (identity + x), the update rule and the scale, bit for bit"""
    import json
    tr = np.load(os.path.join(ROOT, "tests", "golden", "qact_percentile_trace.npz"))
    meta = json.loads(str(tr["meta"]))
    assert len(meta) == 6

    def record(name, *args):
        if name == "ivit_quantile_pair_f32":
            x = args[0].tensor.numpy().reshape(-1)
            assert x.size == args[1]
            args[4].tensor.copy_(torch.from_numpy(np.array(qr.quantile_pair(x, args[2], args[3]), np.float32)))
        launches.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    for m in meta:
        c = m["case"]
        qa = qu.QuantAct(8, act_range_momentum=m["momentum"])
        qa.percentile = m["percentile"]
        pre, idpre = (torch.tensor([v]) for v in tr[c + "/pre"])
        for s in range(m["steps"]):
            x = torch.from_numpy(tr[f"{c}/x{s}"])
            if m["kind"] == "input":
                _, sc = qa(x)
            elif m["kind"] == "identity":
                _, sc = qa(x, pre, identity=torch.from_numpy(tr[f"{c}/id{s}"]), identity_scaling_factor=idpre)
            else:
                _, sc = qa(x, pre)
            got = np.array([float(qa.x_min), float(qa.x_max)], np.float32)
            assert np.array_equal(got.view(np.int32), tr[c + "/post"][s].view(np.int32)), (c, s, got, tr[c + "/post"][s])
            assert np.float32(float(sc)).view(np.int32) == tr[c + "/scale"][s].view(np.int32), (c, s)


# ----------------------------------------------------------------------------------- the ABI row
def test_prototype_matches_ctypes_table_and_workspace_constant():
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int ivit_quantile_pair_f32\(([^)]*)\);", hdr)
    assert m, "ivit_quantile_pair_f32 is not declared"
    kinds = {"const float*": _lib.vp, "float*": _lib.vp, "void*": _lib.vp, "int64_t": _lib.i64, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    assert _lib.SIGNATURES["ivit_quantile_pair_f32"] == [kinds[re.sub(r"\s+\w+$", "", p.strip())] for p in m.group(1).split(",")]
    ws = re.search(r"#define IVIT_QUANTILE_WS_BYTES (\d+)", hdr)
    assert ws and int(ws.group(1)) == _lib.QUANTILE_WS_BYTES
