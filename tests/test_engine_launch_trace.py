"""Launch trace of the fused engines, on the CPU: every `_lib.call` the engines issue while they are built and during one
forward, with every argument, against tests/golden/engine_launch_trace.json.

The native library is stubbed: the recorder stands in for `_lib.call`, the engines are built on device="cpu", and
deterministic torch fills the never-written buffers (`torch.empty`), so the trace is the same in every process.
Arguments are written in a form that does not depend on addresses or on how the engine names its internals:
ints and floats as they are; a pointer into the workspace as `ws:<key>+<byte offset>`; a pointer into any other tensor
the engine holds as `<dtype>[<shape>]#<content digest>+<byte offset>`; the caller's tensors as `images`, `targets`,
`hits`; a construction-time temporary (a table the engine builds from and drops) as `tmp:` + its description.  A
pointer that maps to none of these fails the test.

The fixture pins the launches so that host-side refactors of engine.py / swin_engine.py can be checked without a GPU.  It
keeps, per case and phase, the number of launches and the SHA-256 of the trace lines joined by newlines.  To see what
differs, write the readable traces of two trees and diff them:

    IVIT_LAUNCH_TRACE_DUMP=/tmp/a python -m pytest tests/test_engine_launch_trace.py     # one file per case

When a change alters launches on purpose, regenerate the fixture from the changed tree and review the dumps' diff:

    IVIT_WRITE_LAUNCH_TRACE=1 python -m pytest tests/test_engine_launch_trace.py
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine
from ivit_amd.swin_engine import IntSwinEngine
from ivit_amd.synth import IMG_SIZE

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_launch_trace.json")


def _tensors(obj, out):
    """every tensor reachable from obj through dicts / lists / tuples"""
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _tensors(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    return out


def _describe(t):
    digest = hashlib.sha1(t.detach().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:12]
    return f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}#{digest}"


class _Ptr(ctypes.c_void_p):
    """what the stubbed `_lib.ptr` returns: the address, plus the tensor it came from"""


def _ptr(t):
    if t is None:
        return None
    p = _Ptr(t.data_ptr())
    p.tensor = t
    return p


def _extent(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


class Canon:
    """pointer -> stable name, built from the engine's state and the caller's tensors"""

    def __init__(self, eng, named):
        self.ranges = []      # (nbytes, name-or-describer, lo, hi)
        ws = eng.__dict__.get("ws", {})
        for k, t in sorted((k, v) for k, v in ws.items() if isinstance(v, torch.Tensor)):
            self._add(t, f"ws:{k}")
        for k, t in sorted(ws.get("_own", {}).items()):
            self._add(t, f"ws:_own.{k}")
        for t in _tensors([v for k, v in sorted(eng.__dict__.items()) if k not in ("ws", "_graphs")], []):
            if t.numel():
                self._add(t, _describe(t))
        for name, t in named.items():
            self._add(t, name)

    def _add(self, t, name):
        lo, hi = _extent(t)
        if hi > lo:
            self.ranges.append((hi - lo, name, lo, hi))

    def arg(self, a):
        if isinstance(a, ctypes.c_void_p):
            t, a = getattr(a, "tensor", None), a.value
            if a is None:
                return None
            hits = sorted((n, name, a - lo) for n, name, lo, hi in self.ranges if lo <= a < hi)
            if not hits and t is not None:
                return f"tmp:{_describe(t)}+0"
            assert hits, f"pointer {a:#x} is not in the engine's workspace, its tensors or the caller's"
            _, name, off = hits[0]
            return f"{name}+{off}"
        if isinstance(a, (bool, np.bool_)):
            return int(a)
        if isinstance(a, (int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(a)
        assert a is None, f"unexpected argument {a!r}"
        return None


@pytest.fixture
def stubbed(monkeypatch):
    """-> calls: the list the recorder appends (name, args) to"""
    calls = []

    def record(name, *args):
        if name == "ivit_ibert_softmax_build_table":      # engine.py reads the table back to choose the band form
            ctypes.memset(args[-2].value, 0, 65536 * 4)
        calls.append((name, args))

    monkeypatch.setattr(_lib, "call", record)
    monkeypatch.setattr(_lib, "ptr", _ptr)
    monkeypatch.setattr(_lib, "lib", lambda: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    det, fill = torch.are_deterministic_algorithms_enabled(), torch.utils.deterministic.fill_uninitialized_memory
    torch.use_deterministic_algorithms(True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        yield calls
    finally:
        torch.use_deterministic_algorithms(det)
        torch.utils.deterministic.fill_uninitialized_memory = fill


def _lines(calls, canon):
    return [f"{name}({', '.join(repr(canon.arg(a)) for a in args)})" for name, args in calls]


def _deit(tag, **kw):
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    return IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=16, **kw)


def _swin(tag):
    fs, ranges, cfg, _, _ = load_synthetic_model(tag)
    return IntSwinEngine(fs, ranges, cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window"], device="cpu", max_batch=2)


# case -> (engine factory, [(variant, B, knobs, run)]); run(eng, images) -> the caller's tensors to name
def _fwd(eng, x):
    eng.forward(x)
    return {}


def _taps(eng, x):
    eng.forward(x, taps={})
    return {}


def _topk(eng, x):
    targets = torch.zeros(x.shape[0], dtype=torch.int32)
    hits = torch.zeros(5, dtype=torch.int64)
    eng.forward_topk(x, k=5, targets=targets, hits=hits)
    return dict(targets=targets, hits=hits)


CASES = {
    "deit_tiny": (lambda: _deit("deit_tiny"), [
        ("B16", 16, {}, _fwd), ("B2", 2, {}, _fwd), ("B16_rowmajor", 16, dict(block_operands=False), _fwd),
        ("B16_gelu_copy", 16, dict(gelu_in_place=False), _fwd), ("B16_uncompact", 16, dict(_compact=False), _fwd),
        ("B16_topk5", 16, {}, _topk), ("B16_taps", 16, {}, _taps), ("B2_taps", 2, {}, _taps)]),
    "deit_tiny_frags32": (lambda: _deit("deit_tiny"), [("B16", 16, {}, _fwd)]),
    "deit_tiny_ibert": (lambda: _deit("deit_tiny_ibert", family="ibert"), [
        ("B16", 16, {}, _fwd), ("B16_gelu_unfused", 16, dict(fuse_ibert_gelu=False), _fwd)]),
    "deit_tiny_w16": (lambda: _deit("deit_tiny_w16", stream_bits=16), [
        ("B16", 16, {}, _fwd), ("B16_res_unfused", 16, dict(fuse_res16=False), _fwd)]),
    "deit_tiny_ibert_w16all": (lambda: _deit("deit_tiny_ibert_w16all", family="ibert", stream_bits=16, softmax_bits=16,
                                             pos_bits=16), [
        ("B16", 16, {}, _fwd), ("B16_unfused", 16, dict(fuse_res16=False, fuse_ibert_gelu=False), _fwd)]),
    # natural (non power-of-two) scales: the compat LayerNorm / Shiftmax / GELU forms
    "deit_tiny_natural": (lambda: _deit("deit_tiny_natural"), [("B16", 16, {}, _fwd)]),
    "deit_tiny_ibert_natural": (lambda: _deit("deit_tiny_ibert_natural", family="ibert"), [("B16", 16, {}, _fwd)]),
    "deit_tiny_w16all": (lambda: _deit("deit_tiny_w16all", stream_bits=16, softmax_bits=16, pos_bits=16), [("B16", 16, {}, _fwd)]),
    "swin_tiny_natural": (lambda: _swin("swin_tiny_natural"), [("B2", 2, {}, _fwd), ("B2_taps", 2, {}, _taps)]),
    "swin_tiny": (lambda: _swin("swin_tiny"), [
        ("B2", 2, {}, _fwd), ("B2_proj_unfused", 2, dict(proj_fused=False), _fwd),
        ("B2_proj_i32", 2, dict(proj_fused=False, proj_i16=False), _fwd), ("B2_taps", 2, {}, _taps)]),
}


def trace_case(case, calls, monkeypatch):
    make, variants = CASES[case]
    monkeypatch.setattr(IntViTEngine, "frags16", case != "deit_tiny_frags32")
    del calls[:]
    eng = make()
    out = {"build": _lines(calls, Canon(eng, {}))}
    for variant, B, knobs, run in variants:
        saved = {k: getattr(eng, k) for k in knobs if k != "_compact"}
        for k, v in knobs.items():
            if k == "_compact":
                eng._compact(v)
            else:
                setattr(eng, k, v)
        img = IMG_SIZE if isinstance(eng, IntSwinEngine) else eng.IMG
        x = torch.zeros(B, 3, img, img, dtype=torch.float32)
        del calls[:]
        named = run(eng, x)
        out[variant] = _lines(calls, Canon(eng, dict(images=x, **named)))
        for k, v in saved.items():
            setattr(eng, k, v)
        if "_compact" in knobs:
            eng._compact(True)
    return out


def _digest(lines):
    return [len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()]


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_trace(case, stubbed, monkeypatch):
    got = trace_case(case, stubbed, monkeypatch)
    dump = os.environ.get("IVIT_LAUNCH_TRACE_DUMP")
    if dump:
        os.makedirs(dump, exist_ok=True)
        with open(os.path.join(dump, f"{case}.json"), "w") as f:
            json.dump(got, f, indent=1)
    got = {f"{case}/{phase}": _digest(lines) for phase, lines in got.items()}
    if os.environ.get("IVIT_WRITE_LAUNCH_TRACE") == "1":
        data = _fixture() if os.path.exists(FIXTURE) else {}
        data = {k: v for k, v in data.items() if not k.startswith(case + "/")}
        data.update(got)
        with open(FIXTURE, "w") as f:     # one line per phase, in trace order within a case
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in data.items()) + "\n}\n")
        return
    want = {k: v for k, v in _fixture().items() if k.startswith(case + "/")}
    assert list(got) == list(want), f"{case}: traced phases differ"
    for phase in want:
        assert got[phase] == want[phase], (f"{phase}: [launches, sha256] {got[phase]}, fixture {want[phase]} "
                                           "(IVIT_LAUNCH_TRACE_DUMP: see the module docstring)")
