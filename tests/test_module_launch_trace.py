"""Launch trace of the integer-carrying module path (quantization_utils/lazy.py), on the CPU: every `_lib.call` of two
module-by-module forwards of a frozen model, with every argument, against tests/golden/module_launch_trace.json.

The recorder, the canonical argument form and the fixture format are those of test_engine_launch_trace.py (see its docstring,
also for IVIT_LAUNCH_TRACE_DUMP / IVIT_WRITE_LAUNCH_TRACE).  The module path keeps no workspace: every pointer is `images` or
`tmp:<dtype>[shape]#<content digest>`, which pins the contents of every constant next to the scalars.  Two phases per case:
`warmup`, the first forward, which builds and caches every constant (its build launches are in the trace), and `steady`, the
second.  Below 2048 rows the deferred Requant node, its fused residual GEMM and the head-major qkv epilogue are not reached:
`deit_tiny_B16` (3152 rows) is there for them.
"""
import json
import os
import types
import warnings

import pytest
import torch

import ivit_amd as ivit
import ivit_amd.quantization_utils as qu
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.quantization_utils import lazy
from ivit_amd.synth import IMG_SIZE
from test_engine_launch_trace import Canon, _digest, _lines, stubbed  # noqa: F401  (stubbed: the fixture)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "module_launch_trace.json")

# case -> (model tag, batch)
CASES = {
    "deit_tiny": ("deit_tiny", 2), "deit_tiny_natural": ("deit_tiny_natural", 2), "deit_tiny_ibert": ("deit_tiny_ibert", 2),
    "deit_tiny_ibert_natural": ("deit_tiny_ibert_natural", 2), "swin_tiny": ("swin_tiny", 2),
    "swin_tiny_natural": ("swin_tiny_natural", 2), "deit_tiny_B16": ("deit_tiny", 16),
}


def load_model(tag):
    """tests/test_gpu_modules.py load_model, on the CPU, module path selected"""
    fs, ranges, cfg, meta, z = load_synthetic_model(tag)
    fam = meta.get("family", "ivit")
    kw = dict(gelu_type=fam, softmax_type=fam, layernorm_type=fam) if fam != "ivit" else {}
    model = getattr(ivit, meta["factory"])(**kw)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected
    for name, mod in model.named_modules():
        if isinstance(mod, qu.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    ivit.freeze_model(model)
    model.use_engine = False
    return model


def trace_case(case, calls, monkeypatch):
    tag, B = CASES[case]
    monkeypatch.setattr(lazy, "_ROWPLAN", {})          # process-wide row-plan cache: every case starts from an empty one
    model = load_model(tag)
    x = torch.zeros(B, 3, IMG_SIZE, IMG_SIZE, dtype=torch.float32)
    out = {}
    for phase in ("warmup", "steady"):
        del calls[:]
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")            # Swin materialises twice by design (float pooling, logits) and says so once
            model(x)
        out[phase] = _lines(calls, Canon(types.SimpleNamespace(), dict(images=x)))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_module_launch_trace(case, stubbed, monkeypatch):  # noqa: F811
    got = trace_case(case, stubbed, monkeypatch)
    dump = os.environ.get("IVIT_LAUNCH_TRACE_DUMP")
    if dump:
        os.makedirs(dump, exist_ok=True)
        with open(os.path.join(dump, f"module_{case}.json"), "w") as f:
            json.dump(got, f, indent=1)
    got = {f"{case}/{phase}": _digest(lines) for phase, lines in got.items()}
    data = {}
    if os.path.exists(FIXTURE):
        with open(FIXTURE) as f:
            data = json.load(f)
    if os.environ.get("IVIT_WRITE_LAUNCH_TRACE") == "1":
        data = {k: v for k, v in data.items() if k.split("/")[0] != case}
        data.update(got)
        with open(FIXTURE, "w") as f:     # one line per phase, in trace order within a case
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in data.items()) + "\n}\n")
        return
    want = {k: v for k, v in data.items() if k.split("/")[0] == case}
    assert list(got) == list(want), f"{case}: traced phases differ"
    for phase in want:
        assert got[phase] == want[phase], (f"{phase}: [launches, sha256] {got[phase]}, fixture {want[phase]} "
                                           "(IVIT_LAUNCH_TRACE_DUMP: see test_engine_launch_trace.py's docstring)")
