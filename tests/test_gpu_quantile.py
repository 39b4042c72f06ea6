"""Percentile calibration on the device: ivit_quantile_pair_f32 against torch.quantile of the CPU copy (bitwise, except the sign of a
zero), QuantAct in percentile mode against a trace of the reference's own QuantAct (tests/golden/qact_percentile_trace.npz, written by
scripts/gen_percentile_trace.py), and a small model calibrated with set_act_percentile."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, inference, synth  # noqa: E402
import ivit_amd.quantization_utils as q  # noqa: E402

import quantile_ref as qr  # noqa: E402

DEV = "cuda:0"
WS = _lib.QUANTILE_WS_BYTES
PS = (50, 99, 99.9, 99.999, 100)
QS = [qq for p in PS for qq in qr.percentile_qs(p)]           # float32, (lo, hi) per p
TILE = 4096                                                   # elements one workgroup takes per round of a pass (csrc/calib.hip QTILE)
GUARD = 777.0


class Runner:
    """one workspace (with guard bytes behind it) and one output (with guard floats around it)"""

    def __init__(self):
        self.ws = torch.empty(WS + 64, dtype=torch.uint8, device=DEV)
        self.out = torch.empty(6, dtype=torch.float32, device=DEV)

    def poison(self):
        self.ws.fill_(0xA5)
        self.out.fill_(GUARD)

    def call(self, t, q_lo, q_hi):
        _lib.call("ivit_quantile_pair_f32", _lib.ptr(t), t.numel(), float(q_lo), float(q_hi), _lib.ptr(self.out[2:4]), _lib.ptr(self.ws),
                  WS, _lib.stream_ptr())

    def result(self):
        o = self.out.cpu().numpy()
        assert (o[[0, 1, 4, 5]] == GUARD).all(), "guard floats around out2 were written"
        assert bool((self.ws[WS:] == 0xA5).all()), "bytes behind the workspace were written"
        return o[2:4].copy()

    def pair(self, t, q_lo, q_hi):
        """poisoned workspace, two calls in a row on it (the second sees what the first left), then a poisoned one again"""
        self.poison()
        self.call(t, q_lo, q_hi)
        r1 = self.result()
        self.call(t, q_lo, q_hi)
        r2 = self.result()
        assert np.array_equal(r1.view(np.int32), r2.view(np.int32)), ("second call on the same workspace differs", r1, r2)
        return r1


@pytest.fixture(scope="module")
def run():
    return Runner()


def kinds(n, rng):
    s = np.float32(0.0173)
    normal = (rng.standard_normal(n) * 3).astype(np.float32)
    yield "normal", normal
    yield "ties", (s * rng.integers(-128, 128, n).astype(np.float32)).astype(np.float32)
    yield "equal", np.full(n, 1.25, np.float32)
    yield "two", np.where(rng.random(n) < 0.3, np.float32(-2.5), np.float32(7.0)).astype(np.float32)
    yield "low8", (np.uint32(0x40490000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)     # only the last pass tells them apart
    yield "signexp", (np.ldexp(1.0, rng.integers(-20, 21, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)   # only the first pass does
    yield "denormal", (rng.integers(1, 2 ** 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    yield "zeros", rng.choice(np.array([-0.0, 0.0, -1.0, 1.0], np.float32), n, p=[0.45, 0.45, 0.05, 0.05])
    yield "negative", (-np.abs(rng.standard_normal(n)) - 0.5).astype(np.float32)
    x = normal.copy()
    x[rng.integers(0, n)] = np.inf
    yield "inf", x
    x = normal.copy()
    x[rng.integers(0, n)] = np.nan
    yield "nan", x


def torch_quantiles(x_cpu):
    """torch.quantile at every q of QS with one sort -> {q: value}"""
    v = torch.quantile(x_cpu, torch.tensor(np.array(QS, np.float32))).numpy()
    return np.asarray(v, np.float32).reshape(len(PS), 2)


def check_against_torch(run, t, x_cpu, what, minmax=True):
    want = torch_quantiles(x_cpu)
    for i, p in enumerate(PS):
        q_lo, q_hi = qr.percentile_qs(p)
        got = run.pair(t, q_lo, q_hi)
        assert qr.same_bits(got, want[i]), (what, p, got.tolist(), want[i].tolist())
        if p == 100 and minmax:
            mm = torch.empty(2, dtype=torch.float32, device=DEV)
            _lib.call("ivit_minmax_f32", _lib.ptr(t), t.numel(), _lib.ptr(mm), _lib.stream_ptr())
            assert qr.same_bits(got, mm.cpu().numpy()), (what, "p = 100 is min / max", got.tolist(), mm.cpu().numpy().tolist())


# one workgroup's share of a pass +- 1; 1003 is read from a pointer one element behind a 16-byte boundary and is no multiple of 4
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 1003, 2 ** 20 + 3)


@pytest.mark.parametrize("n", SIZES)
def test_quantile_pair_equals_torch(n, run):
    """every kind of data at every p; `inf`: torch's rule gives NaN where an infinity meets itself (b - a), so p = 100 is not min / max
    there, and `nan` makes both results NaN -- both follow torch, not ivit_minmax_f32"""
    rng = np.random.default_rng(4000 + n)
    for kind, x in kinds(n, rng):
        if n == 1003:
            buf = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), x])).to(DEV)
            t = buf[1:]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.from_numpy(x).to(DEV)
        check_against_torch(run, t, torch.from_numpy(x), (kind, n), minmax=kind not in ("inf", "nan"))
        if kind == "nan":
            assert np.isnan(run.pair(t, *qr.percentile_qs(99))).all()


def _mixed_on_device(n, seed):
    """half normal, half multiples of one scale (the regime of real activations), made on the device"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(n, device=DEV, generator=g) * 3
    t[: n // 2] = torch.round(t[: n // 2] * 20) * 0.0173
    return t


def test_quantile_pair_at_torchs_limit(run):
    n = 2 ** 24
    t = _mixed_on_device(n, 11)
    check_against_torch(run, t, t.cpu(), ("mixed", n))


def test_quantile_pair_above_torchs_limit(run):
    """torch.quantile refuses n > 2^24: the reference is the numpy restatement (np.partition), which test_quantile_cpu.py pins against
    torch wherever torch answers"""
    n = 2 ** 24 + 4099
    t = _mixed_on_device(n, 12)
    x = t.cpu().numpy()
    with pytest.raises(RuntimeError):
        torch.quantile(t.cpu(), 0.5)
    for p in PS:
        q_lo, q_hi = qr.percentile_qs(p)
        got = run.pair(t, q_lo, q_hi)
        want = qr.quantile_pair(x, q_lo, q_hi)
        assert qr.same_bits(got, want), (p, got.tolist(), want)


def test_refusals_launch_nothing(run):
    t = torch.arange(100, dtype=torch.float32, device=DEV)
    L = _lib.lib()
    st = _lib.stream_ptr()
    out2 = _lib.ptr(run.out[2:4])
    bad = {
        "short workspace": (_lib.ptr(t), 100, 0.25, 0.75, out2, _lib.ptr(run.ws), WS - 4, st),
        "q = 1.5": (_lib.ptr(t), 100, 0.25, 1.5, out2, _lib.ptr(run.ws), WS, st),
        "q < 0": (_lib.ptr(t), 100, -0.25, 0.5, out2, _lib.ptr(run.ws), WS, st),
        "q = NaN": (_lib.ptr(t), 100, float("nan"), 0.5, out2, _lib.ptr(run.ws), WS, st),
        "n = 0": (_lib.ptr(t), 0, 0.25, 0.75, out2, _lib.ptr(run.ws), WS, st),
        "NULL out2": (_lib.ptr(t), 100, 0.25, 0.75, None, _lib.ptr(run.ws), WS, st),
        "NULL x": (None, 100, 0.25, 0.75, out2, _lib.ptr(run.ws), WS, st),
        "NULL workspace": (_lib.ptr(t), 100, 0.25, 0.75, out2, None, WS, st),
        "misaligned x": (C.c_void_p(t.data_ptr() + 2), 50, 0.25, 0.75, out2, _lib.ptr(run.ws), WS, st),
    }
    for what, args in bad.items():
        run.poison()
        assert L.ivit_quantile_pair_f32(*args) == -1, what            # IVIT_ERR_INVALID
        assert L.ivit_last_error_string().decode().startswith("ivit_quantile_pair_f32"), what
        torch.cuda.synchronize()
        assert bool((run.ws == 0xA5).all()) and bool((run.out == GUARD).all()), f"{what}: something was launched"
        with pytest.raises(_lib.IvitError):
            _lib.call("ivit_quantile_pair_f32", *args)


# ----------------------------------------------------------------------------------- QuantAct against the reference's trace
def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def test_quantact_percentile_against_the_reference_trace(golden_dir):
    tr = np.load(os.path.join(golden_dir, "qact_percentile_trace.npz"))
    meta = json.loads(str(tr["meta"]))
    assert {(m["percentile"], m["momentum"]) for m in meta} == {(p, mo) for p in (99.0, 99.99, 100.0) for mo in (0.95, -1)}
    assert {"identity", "input", "plain"} == {m["kind"] for m in meta}
    for m in meta:
        c = m["case"]
        qa = q.QuantAct(8, act_range_momentum=m["momentum"]).to(DEV)
        qa.percentile = m["percentile"]
        pre, idpre = (torch.tensor([v], device=DEV) for v in tr[c + "/pre"])
        for s in range(m["steps"]):
            x = torch.from_numpy(tr[f"{c}/x{s}"]).to(DEV)
            assert x.numel() <= 4096
            if m["kind"] == "input":
                _, sc = qa(x)
            elif m["kind"] == "identity":
                _, sc = qa(x, pre, identity=torch.from_numpy(tr[f"{c}/id{s}"]).to(DEV), identity_scaling_factor=idpre)
            else:
                _, sc = qa(x, pre)
            got = np.array([float(qa.x_min), float(qa.x_max)], np.float32)
            assert np.array_equal(_bits(got), _bits(tr[c + "/post"][s])), (c, s, got.tolist(), tr[c + "/post"][s].tolist())
            assert np.array_equal(_bits(sc.cpu().numpy().reshape(-1)), _bits(tr[c + "/scale"][s:s + 1])), (c, s)


# ----------------------------------------------------------------------------------- a model
def _ranges(model):
    return {n: np.array([float(m.x_min), float(m.x_max)], np.float32) for n, m in model.named_modules() if isinstance(m, q.QuantAct)}


def _observe_with_torch(mod):
    def observe(x_act):
        xf = x_act.detach().float().flatten().cpu()
        q_lo, q_hi = q.quant_modules.percentile_qs(mod.percentile)
        lo, hi = torch.quantile(xf, q_lo), torch.quantile(xf, q_hi)
        q.QuantAct._observe_update(mod, lo.to(x_act.device), hi.to(x_act.device))
    return observe


@pytest.mark.parametrize("family", ["ivit", "ibert"])
def test_model_percentile_calibration(family):
    torch.manual_seed(5)
    base = ivit.VisionTransformer(embed_dim=192, depth=2, num_heads=3, num_classes=10, gelu_type=family, softmax_type=family,
                                  layernorm_type=family).to(DEV).eval()
    batches = [torch.from_numpy(synth.make_images(4, seed)).to(DEV) for seed in (31, 32)]
    native, by_torch, minmax = copy.deepcopy(base), copy.deepcopy(base), copy.deepcopy(base)
    assert inference.set_act_percentile(native, 99.9) is native
    inference.calibrate_model(native, DEV, batches)
    inference.set_act_percentile(by_torch, 99.9)
    for _, m in by_torch.named_modules():
        if isinstance(m, q.QuantAct):
            m._observe = _observe_with_torch(m)
    inference.calibrate_model(by_torch, DEV, batches)
    inference.calibrate_model(minmax, DEV, batches)
    a, b, c = _ranges(native), _ranges(by_torch), _ranges(minmax)
    assert len(a) > 20 and list(a) == list(b) == list(c)
    if family == "ibert":
        assert "blocks.0.attn.int_softmax.act" in a
    bad = [(n, a[n].tolist(), b[n].tolist()) for n in a if not qr.same_bits(a[n], b[n])]
    assert not bad, f"{len(bad)} of {len(a)} ranges differ from torch.quantile's: {bad[:3]}"
    differ = [n for n in a if not np.array_equal(a[n], c[n])]
    assert len(differ) > len(a) // 2, f"only {differ} differ from a min / max calibration"
    ivit.freeze_model(native)
    assert native.takes_engine(batches[0]), native.engine_unsupported_reason()
    with torch.no_grad():
        y = native(batches[0])
    assert y.shape == (4, 10) and bool(torch.isfinite(y).all())
    assert native._engine is not None
