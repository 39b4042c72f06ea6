"""The calibration forward derives every linear layer's integer parameters on the device (lazy.device_linear_params behind
QuantLinear._params, QuantConv2d._slow and lazy.linear_consts): the same buffers, scales and logits as the host form
(quant_modules.LINEAR_PARAMS_ON_DEVICE = False), bit for bit, through calibration, freeze and the frozen module path; no weight goes
to the host; the weight kernel runs once per module and weight version, the bias kernel once per moved input scale; graph replay of
the frozen module path is what it was.  A tiny DeiT (embed_dim 128, depth 2, 10 classes: the head's N % 4 row padding) with both
operator families, and the small Swin of tests/test_swin_registry_cpu.py (K = 48 and 96, a reduction without bias)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.quantization_utils import lazy, quant_modules  # noqa: E402

from test_swin_registry_cpu import SMALL  # noqa: E402

DEV = "cuda:0"
TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=64, patch_size=16, num_classes=10)
WEIGHT, BIAS = "ivit_weight_quant_rows_f32_i8", "ivit_bias_quant_f32_i32"
CONFIGS = ["deit-ivit", "deit-ibert", "swin"]


def build(which):
    torch.manual_seed(7 + len(which))
    if which == "swin":
        model = ivit.SwinTransformer(**SMALL)
    else:
        fam = which.split("-")[1]
        model = ivit.VisionTransformer(gelu_type=fam, softmax_type=fam, layernorm_type=fam, **TINY)
    model = model.to(DEV).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():          # wider weights than the init's 0.02: activations that use their ranges
            if p.dim() > 1:
                p.mul_(3.0)
            elif name.endswith("relative_position_bias_table"):
                p.mul_(20.0)
    return model


def twin(model, which):
    """a second model with the same state dict"""
    other = build(which)
    other.load_state_dict(model.state_dict())
    return other


def batches(which, n=3, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    img = SMALL["img_size"] if which == "swin" else TINY["img_size"]
    out = []
    for i in range(n):          # a different amplitude per batch: the ranges move on every forward
        low = torch.nn.functional.interpolate(torch.randn(4, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
        out.append(((low + 0.3 * torch.randn(4, 3, img, img, generator=g)) * (1.0 + 0.5 * i)).to(DEV))
    return out


def forward(model, x, on_device=True):
    old = quant_modules.LINEAR_PARAMS_ON_DEVICE
    quant_modules.LINEAR_PARAMS_ON_DEVICE = on_device
    try:
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return model(x).clone()
    finally:
        quant_modules.LINEAR_PARAMS_ON_DEVICE = old


def freeze(model):
    ivit.freeze_model(model)
    model.use_engine = False          # the frozen forward module by module: lazy.linear_consts, not the engines' build


def linears(model):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, (qu.QuantLinear, qu.QuantConv2d))]


def assert_same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        x, y = sa[k], sb[k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, k
        if x.is_floating_point():
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), k


class Calls:
    """records (name, first pointer argument) of every _lib.call, and calls through"""

    def __enter__(self):
        self.calls, self.orig = [], _lib.call

        def call(name, *args):
            self.calls.append((name, getattr(args[0], "value", None) if args else None))
            return self.orig(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig
        return False

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


# ---------------------------------------------------------------------------- equivalence with the host form
@pytest.mark.parametrize("which", CONFIGS)
def test_device_params_equal_the_host_form(which):
    dev_model = build(which)
    host_model = twin(dev_model, which)
    assert [n for n, m in linears(dev_model) if m.bias is None] == (["layers.0.downsample.reduction"] if which == "swin" else [])
    for x in batches(which):
        with Calls() as tr:
            want = forward(host_model, x, on_device=False)
        assert tr.count(WEIGHT) == 0 and tr.count(BIAS) == 0          # the switch selects the host path on a GPU
        got = forward(dev_model, x)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert_same_state(dev_model, host_model)
    head = dict(linears(dev_model))["head"]
    assert head.weight_integer.shape == head.weight.shape and head.bias_integer.shape == (10,) and head.fc_scaling_factor.shape == (10,)
    assert float(head.weight_integer.abs().max()) == 127.0
    freeze(dev_model)
    freeze(host_model)
    x = batches(which, 1, seed=9)[0]
    with Calls() as tr:
        want = forward(host_model, x, on_device=False)
    assert tr.count(WEIGHT) == 0 and tr.count(BIAS) == 0
    got = forward(dev_model, x)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert_same_state(dev_model, host_model)
    assert any("lin" == k[0] for _, m in linears(dev_model) for k in m.__dict__.get("_lazy_cache", {})), "linear_consts was not reached"


# ---------------------------------------------------------------------------- no weight leaves the device
@pytest.mark.parametrize("which", CONFIGS)
def test_no_weight_goes_to_the_host(which, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("prepare.LinearParams was called: a weight went to the host")
    monkeypatch.setattr(quant_modules, "LinearParams", refuse)
    monkeypatch.setattr(lazy, "LinearParams", refuse)
    model = build(which)
    for x in batches(which):
        assert torch.isfinite(forward(model, x)).all()
    freeze(model)
    assert torch.isfinite(forward(model, batches(which, 1, seed=9)[0])).all()
    for _, m in linears(model):
        assert m.weight_integer.is_cuda and float(m.weight_integer.abs().max()) == 127.0


# ---------------------------------------------------------------------------- launch counts
@pytest.mark.parametrize("which", CONFIGS)
def test_launch_counts(which):
    model = build(which)
    mods = linears(model)
    seen, moved = {}, []

    def pre(mod, args):          # the input scale each module is handed, forward by forward
        s = float(args[1].reshape(-1)[0])
        if seen.get(mod) != s:
            moved.append(mod)
        seen[mod] = s
    hooks = [m.register_forward_pre_hook(pre) for _, m in mods]
    xs = batches(which, 4)
    with Calls() as tr:
        for x in xs[:3]:
            forward(model, x)
    assert tr.count(WEIGHT) == len(mods)                               # once per module: the weights did not change
    assert tr.count(BIAS) == len(moved) and len(moved) > 2 * len(mods)  # once per module and forward in which its s_in changed

    # an in-place edit of one module's weight: that module's weight kernel runs again, no other
    name, lin = next((n, m) for n, m in mods if n.endswith("mlp.fc1"))
    before = {n: (m.weight_integer, m.weight_integer.clone()) for n, m in mods}      # (the old tensors stay alive: no address is reused)
    scale_was = lin.fc_scaling_factor.clone()
    with torch.no_grad():
        lin.weight.mul_(2)
    del moved[:]
    with Calls() as tr:
        forward(model, xs[3])
    assert [p for n, p in tr.calls if n == WEIGHT] == [lin.weight.data_ptr()]
    assert tr.count(BIAS) == len(set(moved) | {lin})                   # its bias part follows the weight version too
    for n, m in mods:
        assert (m.weight_integer.data_ptr() == before[n][0].data_ptr()) == (m is not lin), n
    # twice the weights: twice the row maxima, so the scale doubles exactly and the integers are the ones they were
    assert torch.equal(lin.fc_scaling_factor, 2 * scale_was) and torch.equal(lin.weight_integer, before[name][1])
    # ... and an edit that does change them
    with torch.no_grad():
        lin.weight[0].mul_(-1)
    with Calls() as tr:
        forward(model, xs[3])
    assert [p for n, p in tr.calls if n == WEIGHT] == [lin.weight.data_ptr()]
    assert torch.equal(lin.weight_integer[0], -before[name][1][0]) and torch.equal(lin.weight_integer[1:], before[name][1][1:])

    # ranges that do not move: neither kernel runs, eager or frozen
    for h in hooks:
        h.remove()
    for m in model.modules():
        if isinstance(m, qu.QuantAct):
            m.running_stat = False
    with Calls() as tr:
        forward(model, xs[3])
        freeze(model)
        forward(model, xs[3])
    assert tr.count(WEIGHT) == 0 and tr.count(BIAS) == 0


# ---------------------------------------------------------------------------- graph replay
@pytest.mark.parametrize("fam", ["ivit", "ibert"])
def test_forward_graph_of_the_frozen_tiny_model(fam):
    which = "deit-" + fam
    model = build(which)
    xs = batches(which)
    for x in xs:
        forward(model, x)
    for mod in model.modules():          # ranges snapped to powers of two, as tests/test_gpu_module_graph.py freezes its models
        if isinstance(mod, qu.QuantAct):
            qmax = 2 ** (mod.activation_bit - 1) - 1
            a = max(-float(mod.x_min), float(mod.x_max)) / qmax
            assert a > 0
            p2 = 2.0 ** np.ceil(np.log2(a))
            mod.x_max.fill_(qmax * p2)
            mod.x_min.fill_(-qmax * p2)
    freeze(model)
    assert not model.takes_engine(xs[0])
    want = [forward(model, x) for x in xs]
    assert not torch.equal(want[0], want[1])
    try:
        with Calls() as tr, warnings.catch_warnings():
            warnings.simplefilter("ignore")
            first = model.forward_graph(xs[0]).clone()
            n = len(tr.calls)
            got = [model.forward_graph(x).clone() for x in xs]
        assert len(tr.calls) == n, "a replay launched through Python"
        assert tr.count(WEIGHT) == 0 and tr.count(BIAS) == 0          # built by the eager forwards above, outside the capture
        assert torch.equal(first.view(torch.int32), want[0].view(torch.int32))
        for y, w in zip(got, want):
            assert torch.equal(y.view(torch.int32), w.view(torch.int32))
        model.graph_status()
    finally:
        model.drop_graphs()
