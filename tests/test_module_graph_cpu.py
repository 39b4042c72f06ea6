"""graph.ModuleGraph on the CPU: the signature, the refusals, the `graph=` keyword of the evaluation functions, and the capture
itself with the native library stubbed as tests/test_engine_launch_trace.py stubs it and `torch.cuda`'s streams and graphs
replaced by stand-ins.  The stand-in for `torch.cuda.graph` makes every way a tensor reaches the host, and every upload, an ERROR
while it is open -- what a HIP graph capture does to a synchronising call -- so a forward that passes here took nothing to the host
inside its capture; the GPU cases (tests/test_gpu_module_graph.py) check the bits."""
import contextlib
import warnings

import pytest
import torch

import ivit_amd as ivit
import ivit_amd.quantization_utils as qu
from ivit_amd import _lib, inference
from ivit_amd.quantization_utils import lazy
from test_engine_launch_trace import stubbed  # noqa: F401  (the fixture)
from test_module_launch_trace import load_model
from test_swin_registry_cpu import SMALL

DEIT = dict(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
IBERT = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")


def _frozen(model, lo=-1.0, hi=1.0):
    for m in model.modules():
        if isinstance(m, qu.QuantAct):
            m.x_min.fill_(lo)
            m.x_max.fill_(hi)
    ivit.freeze_model(model)
    return model.eval()


# ----------------------------------------------------------------------------------- signature
@pytest.mark.parametrize("make", [lambda: ivit.VisionTransformer(**DEIT), lambda: ivit.VisionTransformer(**DEIT, **IBERT),
                                  lambda: ivit.SwinTransformer(**SMALL), lambda: ivit.SwinTransformer(**SMALL, **IBERT)],
                         ids=["deit", "deit_ibert", "swin", "swin_ibert"])
def test_signature_covers_every_parameter_and_buffer(make):
    model = make()
    named = list(model.named_parameters()) + list(model.named_buffers())
    assert any(n.endswith("x_max") for n, _ in named) and any(n.endswith(".weight") for n, _ in named)
    if model.op_types[2] == "ibert":
        assert any(n.endswith("norm1.shift") for n, _ in named)
    if isinstance(model, ivit.SwinTransformer):
        assert any(n.endswith("relative_position_bias_table") for n, _ in named) and any(n.endswith("attn_mask") for n, _ in named)
    sig = model.graph_signature()
    assert model.graph_signature() == sig
    with torch.no_grad():
        for name, t in named:
            t.add_(0)                                   # an in-place write: the values stay, the version counter moves
            new = model.graph_signature()
            assert new != sig, f"{name}: an in-place write leaves the signature unchanged"
            sig = new


def test_signature_follows_replacements_and_switches():
    model = ivit.VisionTransformer(**DEIT)
    sig = model.graph_signature()
    qa = model.blocks[1].attn.qact2
    qa.x_max = qa.x_max.clone()                         # a buffer replaced by an equal one (what a running QuantAct does)
    assert model.graph_signature() != sig
    sig = model.graph_signature()
    lin = model.blocks[0].mlp.fc1
    lin.weight = torch.nn.Parameter(lin.weight.detach().clone())
    assert model.graph_signature() != sig
    sig = model.graph_signature()
    model.use_engine = False
    assert model.graph_signature() != sig
    sig = model.graph_signature()
    lazy.enable_everywhere(True)
    try:
        assert model.graph_signature() != sig
    finally:
        lazy.enable_everywhere(False)
    assert model.graph_signature() == sig


# ----------------------------------------------------------------------------------- refusals
def test_refusals_name_their_reason_and_capture_nothing():
    x = torch.zeros(2, 3, 32, 32)
    model = ivit.VisionTransformer(**DEIT).eval()
    with pytest.raises(ValueError, match=r"forward_graph: the model is not frozen \(QuantAct qact_input"):
        model.forward_graph(x)
    _frozen(model)
    model.train()
    with pytest.raises(ValueError, match="forward_graph: the model is in training mode"):
        model.forward_graph(x)
    model.eval()
    h = model.blocks[0].attn.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(ValueError, match=r"forward_graph: module blocks\.0\.attn carries a forward hook"):
        model.forward_graph(x)
    h.remove()
    h = model.blocks[1].mlp.fc1.register_forward_pre_hook(lambda m, i: None)
    with pytest.raises(ValueError, match=r"forward_graph: module blocks\.1\.mlp\.fc1 carries a forward pre-hook"):
        model.forward_graph(x)
    h.remove()
    with pytest.raises(ValueError, match="forward_graph: the input is not on the GPU"):
        model.forward_graph(x)
    assert model._graphs == {}
    swin = ivit.SwinTransformer(**SMALL, **IBERT).eval()
    with pytest.raises(ValueError, match="not frozen"):
        swin.forward_graph(torch.zeros(1, 3, 56, 56))
    for m in swin.modules():
        if isinstance(m, qu.QuantAct):
            m.fix()                                     # every QuantAct fixed, the LayerNorms' overflow handling still on
    with pytest.raises(ValueError, match=r"forward_graph: IBERTIntLayerNorm patch_embed\.norm still handles overflow"):
        swin.forward_graph(torch.zeros(1, 3, 56, 56))
    assert swin._graphs == {}


# ----------------------------------------------------------------------------------- the evaluation keyword
class _Scripted(torch.nn.Module):
    """logits that put class `i % 7` first for the i-th image seen; records how it is called"""

    def __init__(self):
        super().__init__()
        self.calls, self.seen = [], 0

    def _logits(self, x):
        idx = (torch.arange(x.shape[0]) + self.seen) % 7
        self.seen += x.shape[0]
        return torch.nn.functional.one_hot(idx, 10).float() + torch.arange(10) * 1e-3

    def forward(self, x):
        self.calls.append(("forward", x.shape[0]))
        return self._logits(x)

    def forward_graph(self, x, resident=False):
        self.calls.append(("forward_graph", x.shape[0]))
        return self._logits(x)

    def graph_status(self):
        self.calls.append(("graph_status",))


def _loader():
    g = torch.Generator().manual_seed(2)
    return [(torch.randn(n, 3, 8, 8, generator=g), torch.randint(0, 7, (n,), generator=g)) for n in (4, 4, 4, 4, 3)]


def _count(logits, targets, hits, k):
    pred = logits.topk(k, dim=1).indices
    hits += (pred == targets.reshape(-1, 1).long()).sum(dim=0)


@pytest.mark.parametrize("fn,extra", [(inference.evaluate_dataset, {}), (inference.evaluate_dataset_parallel, {"scorer": _count})],
                         ids=["evaluate_dataset", "evaluate_dataset_parallel"])
def test_graph_keyword_defaults_to_the_eager_calls(fn, extra):
    import inspect
    assert inspect.signature(fn).parameters["graph"].default is False
    eager, explicit, replayed = _Scripted(), _Scripted(), _Scripted()
    a = fn(eager, _loader(), "cpu", print_batch_stats=False, **extra)
    b = fn(explicit, _loader(), "cpu", print_batch_stats=False, graph=False, **extra)
    c = fn(replayed, _loader(), "cpu", print_batch_stats=False, graph=True, **extra)
    assert eager.calls == explicit.calls == [("forward", 4)] * 4 + [("forward", 3)]
    assert replayed.calls == [("forward_graph", 4)] * 4 + [("forward_graph", 3), ("graph_status",)]
    assert a == b == c and a[0] > 0


# ----------------------------------------------------------------------------------- the capture, stubbed
class _FakeStream:
    def __init__(self, device=None):
        pass

    def wait_stream(self, other):
        pass


class _FakeGraph:
    replays = 0

    def replay(self):
        type(self).replays += 1


def _host_access(what):
    def refuse(*a, **k):
        raise AssertionError(f"{what} inside the capture: a HIP graph capture would abort here")
    return refuse


@pytest.fixture
def fake_cuda(stubbed, monkeypatch):  # noqa: F811
    """-> the stubbed library's call list; torch.cuda's streams and graphs replaced, host access refused while a capture is open"""
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(_FakeGraph, "replays", 0)

    @contextlib.contextmanager
    def capture(graph):
        with pytest.MonkeyPatch.context() as mp:
            for name in ("item", "cpu", "numpy", "tolist", "__float__", "__int__", "__bool__", "__index__"):
                mp.setattr(torch.Tensor, name, _host_access(f"Tensor.{name}"))
            mp.setattr(torch, "from_numpy", _host_access("torch.from_numpy (an upload)"))
            mp.setattr(torch, "tensor", _host_access("torch.tensor (an upload)"))
            yield
    monkeypatch.setattr(torch.cuda, "graph", capture)
    monkeypatch.setattr(lazy, "_ROWPLAN", {})
    return stubbed


def _names(calls):
    return [name for name, _ in calls]


def _eager_names(model, x, calls):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model(x)
        del calls[:]
        model(x)
    names = _names(calls)
    del calls[:]
    return names


def _graph_run(model, x, calls, **kw):
    del calls[:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = model.forward_graph(x, **kw)
    names = _names(calls)
    del calls[:]
    return y, names


@pytest.mark.parametrize("tag,size", [("deit_tiny", 224), ("deit_tiny_ibert_natural", 224), ("swin_tiny_natural", 224)])
def test_carried_forward_is_captured_once_and_replayed(tag, size, fake_cuda):
    """a model whose forward is carried as integers: the capture issues the steady forward's launches, takes nothing to the host,
    and a second call, another input included, launches nothing; another batch size gets its own graph; drop_graphs frees them"""
    model = load_model(tag)
    x = torch.zeros(2, 3, size, size)
    steady = _eager_names(model, x, fake_cuda)
    y, names = _graph_run(model, x, fake_cuda)
    assert names == steady * 3 and _FakeGraph.replays == 1            # two warm-up forwards and the captured one
    assert tuple(y.shape) == (2, model.num_classes) and y.dtype == torch.float32 and type(y) is torch.Tensor
    assert list(model._graphs) == [(2, torch.float32)] and model._graphs[(2, torch.float32)][3].messages == []
    y2, names = _graph_run(model, torch.ones(2, 3, size, size), fake_cuda)
    assert names == [] and y2 is y and _FakeGraph.replays == 2
    assert torch.equal(model._graphs[(2, torch.float32)][1], torch.ones(2, 3, size, size))      # copied into the static input
    model.graph_status()                                                # no check on the device: nothing to read
    _graph_run(model, torch.zeros(1, 3, size, size), fake_cuda)
    assert sorted(model._graphs) == [(1, torch.float32), (2, torch.float32)]
    model.drop_graphs()
    assert model._graphs == {}


def test_resident_input_and_invalidation(fake_cuda):
    model = load_model("deit_tiny")
    x = torch.zeros(2, 3, 224, 224)
    model.forward_graph(x, resident=True)
    key = (2, torch.float32, x.data_ptr())
    assert list(model._graphs) == [key] and model._graphs[key][1] is x
    _, names = _graph_run(model, x, fake_cuda, resident=True)
    assert names == []
    # an in-place range edit: the graphs go, the next call captures again
    graph = model._graphs[key][0]
    model.blocks[3].attn.qact2.x_max.fill_(float(model.blocks[3].attn.qact2.x_max) * 2)
    _, names = _graph_run(model, x, fake_cuda, resident=True)
    assert names and list(model._graphs) == [key] and model._graphs[key][0] is not graph
    # use_engine is part of the key as well
    _, names = _graph_run(model, x, fake_cuda, resident=True)
    assert names == []


def _literal_swin():
    """the small Swin with the I-BERT operators and, in the shifted block, attn.qact2 at s = 0.5: prepare.ibert_window_mask_ok
    fails there and that block's attention core runs its literal form (tests/test_gpu_swin_ibert_lazy.py)"""
    torch.manual_seed(3)
    model = _frozen(ivit.SwinTransformer(**SMALL, **IBERT))
    qa = model.layers[0].blocks[1].attn.qact2
    qa.x_min.fill_(-127 * 0.5)
    qa.x_max.fill_(127 * 0.5)
    model.use_engine = False
    return model


def test_literal_steps_are_taped_and_their_checks_move_to_the_status_word(fake_cuda):
    """the literal attention core inside a capture: every scale, range and (m, e) upload comes from the
    warm-up forward's tape, narrow_i8's overflow flag is the graph's status word, QuantMatMul takes its int32 form and checks the
    bound on the device; graph_status raises the eager message for a word that is set"""
    model = _literal_swin()
    x = torch.zeros(2, 3, 56, 56)
    steady = _eager_names(model, x, fake_cuda)
    assert "ivit_ibert_softmax_f32_f32" in steady and "ivit_narrow_i32_i8" in steady
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.forward_graph(x)
    calls = list(fake_cuda)
    n = len(steady)
    assert _names(calls[:2 * n]) == steady * 2
    captured = calls[2 * n:]
    # the same launches but for QuantMatMul's kernel, which the activations no longer choose
    assert [c for c in _names(captured) if not c.startswith("ivit_bgemm_pv")] == [c for c in steady if not c.startswith("ivit_bgemm_pv")]
    assert {c for c in _names(captured) if c.startswith("ivit_bgemm_pv")} == {"ivit_bgemm_pv_i32_i8"}
    tape = model._graphs[(2, torch.float32)][3]
    status = tape.status
    narrow = [args for name, args in captured if name == "ivit_narrow_i32_i8"]
    assert len(narrow) == steady.count("ivit_narrow_i32_i8") == 2      # matmul_1's k^T, matmul_2's v
    base, words = status.data_ptr(), [a[3].value for a in narrow]
    assert all(w is not None and base <= w < base + 4 * status.numel() and (w - base) % 4 == 0 for w in words) and len(set(words)) == 2
    assert len(tape.messages) == status.numel() == 4 and tape.complete()
    labels = {label for label, _ in tape.items}
    assert labels == {"QuantAct range", "QuantAct (m, e)", "QuantAct input scale sign", "IBERTIntSoftmax input scale",
                      "IBERTIntSoftmax range", "IBERTIntSoftmax output scale"}, labels
    status.zero_()              # (the stubbed kernels leave the fill pattern behind, which QuantMatMul's torch check has looked at)
    model.graph_status()
    status[(words[1] - base) // 4] = 1
    with pytest.raises(_lib.IvitError, match=r"QuantMatMul B: integer activations exceed 8 bits.*batch size 2"):
        model.graph_status()
    model.graph_status()                                                # read and cleared


@pytest.mark.parametrize("make,size", [(lambda: ivit.VisionTransformer(**DEIT), 32), (lambda: ivit.VisionTransformer(**DEIT, **IBERT), 32),
                                       (lambda: ivit.SwinTransformer(**SMALL), 56), (lambda: ivit.SwinTransformer(**SMALL, **IBERT), 56)],
                         ids=["deit", "deit_ibert", "swin", "swin_ibert"])
def test_every_literal_form_can_be_captured(make, size, fake_cuda, monkeypatch):
    """the integer-carrying path switched off (IVIT_LAZY=0): every module runs its literal form, and the capture of that forward
    takes nothing to the host either -- every read-back and upload of every `_slow` is on the tape"""
    monkeypatch.setattr(lazy, "ENABLED", False)
    torch.manual_seed(5)
    model = _frozen(make())
    model.use_engine = False
    x = torch.zeros(2, 3, size, size)
    steady = _eager_names(model, x, fake_cuda)
    _, names = _graph_run(model, x, fake_cuda)
    assert len(names) == 3 * len(steady) and names[:len(steady)] == steady
    tape = model._graphs[(2, torch.float32)][3]
    assert tape.complete() and len(tape.messages) == steady.count("ivit_narrow_i32_i8") + len([n for n in steady if n.startswith("ivit_bgemm_pv")])
    _, names = _graph_run(model, x, fake_cuda)
    assert names == []
    monkeypatch.setattr(lazy, "ENABLED", True)           # the switch is part of the signature
    _, names = _graph_run(model, x, fake_cuda)
    assert names


def test_all_zero_probabilities_keep_a_literal_core_inside_the_capture(fake_cuda):
    """softmax_bw = 4 with attn.qact2 calibrated on zeros (tests/test_gpu_w4_lazy.py): Shiftmax's literal form inside the capture"""
    torch.manual_seed(1)
    model = _frozen(ivit.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10, softmax_bw=4))
    for blk in model.blocks:
        blk.attn.qact2.x_min.fill_(0.0)
        blk.attn.qact2.x_max.fill_(0.0)
    assert model.engine_unsupported_reason() is not None
    x = torch.zeros(2, 3, 224, 224)
    steady = _eager_names(model, x, fake_cuda)
    assert "ivit_shiftmax_f32_i16" in steady and not [n for n in steady if "attention_fused" in n]
    _, names = _graph_run(model, x, fake_cuda)
    assert len(names) == 3 * len(steady)
    assert {"Shiftmax input scale", "Shiftmax output scale"} <= {label for label, _ in model._graphs[(2, torch.float32)][3].items}
    _, names = _graph_run(model, x, fake_cuda)
    assert names == []


def test_engine_models_replay_the_engines_own_graph(fake_cuda, monkeypatch):
    model = load_model("deit_tiny")
    model.use_engine = True
    x = torch.zeros(2, 3, 224, 224)
    assert model.takes_engine(x)
    y = model.forward_graph(x)
    eng = model._engine[2]
    assert model._graphs == {} and len(eng._graphs) == 1 and tuple(y.shape) == (2, 1000) and y.dtype == torch.float32
    assert y.data_ptr() == eng.forward_graph(x)[1].data_ptr()
    model.drop_graphs()
    assert "_graphs" not in eng.__dict__
