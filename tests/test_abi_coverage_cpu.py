"""The ratchet of the C ABI: every function declared in include/ivit_hip.h is called BY NAME in a GPU test file
(tests/test_gpu_*.py) -- as `_lib.call("NAME", ...)` or as an attribute call `X.NAME(...)`, found in the syntax tree, so a mention in a
comment, a docstring or a list of names does not count.  A new export without a test fails here, on the CPU.

The exemption table below may hold only functions that launch nothing on the GPU (host functions); it names the CPU test file that
calls each of them, and that is checked the same way.  The JPEG host helpers that were reached only through transforms.py get their
direct calls in this file.  include/ivit_hip_debug.h (the lab build's measurement hooks, exported by libivit_hip_lab.so only) is out
of scope: those are knobs for tests and scripts, not entry points a caller of the product depends on."""
import ast
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from ivit_amd import _lib

from test_jpeg_cpu import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")

# host functions (no kernel launch, no HIP runtime call) -> the CPU test file that calls them by name
HOST_ONLY = {
    "ivit_version": "test_host_logic.py",
    "ivit_last_error_string": "test_host_logic.py",
    "ivit_eval_geometry": "test_eval_transform_cpu.py",
    "ivit_gemm_plan": "test_gemm_plan_cpu.py",
    "ivit_jpeg_probe": "test_abi_coverage_cpu.py",
    "ivit_jpeg_plan_image": "test_abi_coverage_cpu.py",
    "ivit_jpeg_workspace": "test_abi_coverage_cpu.py",
    "ivit_jpeg_decode_host": "test_abi_coverage_cpu.py",
}


def declared_names():
    pat = r"\b(?:int|const char\*)\s+(ivit_[a-z0-9_]+)\s*\("
    return sorted(set(re.findall(pat, open(os.path.join(ROOT, "include", "ivit_hip.h")).read())))


def called_names(path):
    """names a file calls: the string constant that is the first argument of a `.call(...)`, and the attribute of every `X.name(...)`"""
    names = set()
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute):
            if node.func.attr == "call" and node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str):
                names.add(node.args[0].value)
            elif node.func.attr.startswith("ivit_"):
                names.add(node.func.attr)
    return names


def test_called_names_sees_calls_only(tmp_path):
    p = tmp_path / "t.py"
    p.write_text('"""ivit_in_docstring"""\n# _lib.call("ivit_in_comment")\nNAMES = ["ivit_in_list"]\n'
                 'def f(L, _lib):\n    "L.ivit_in_string()"\n    _lib.call("ivit_a", 1)\n    return L.ivit_b(2)\n')
    assert called_names(str(p)) == {"ivit_a", "ivit_b"}


def test_every_export_is_called_by_a_gpu_test():
    declared = declared_names()
    assert len(declared) > 80 and set(HOST_ONLY) <= set(declared)
    called = set()
    for path in sorted(glob.glob(os.path.join(TESTS, "test_gpu_*.py"))):
        called |= called_names(path)
    missing = [n for n in declared if n not in called and n not in HOST_ONLY]
    assert not missing, f"{len(missing)} exported functions no GPU test calls: {missing}"


def test_exemptions_are_host_functions_with_a_cpu_test():
    header = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    for name, fname in HOST_ONLY.items():
        assert name in called_names(os.path.join(TESTS, fname)), f"{fname} does not call {name}"
        # a host function takes no stream: nothing it could launch on
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header).group(1)
        assert "ivit_stream_t" not in proto, name


# ---------------------------------------------------------------------------- the JPEG host helpers, called directly
def _buf(data):
    return (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")


def test_jpeg_probe_direct():
    L = _lib.lib()
    for c in CASES:
        info = (C.c_int32 * 4)(-7, -7, -7, -7)
        rc = L.ivit_jpeg_probe(_buf(c["data"]), len(c["data"]), info)
        assert (rc == 0) == c["supported"], c["name"]
        if rc == 0:
            assert (info[0], info[1]) == (c["h"], c["w"]) and info[2] in (1, 3) and 0 <= info[3] <= 3, c["name"]
        else:
            assert rc == -2 and c["reason"] in L.ivit_last_error_string().decode(), c["name"]
    data = next(c for c in CASES if c["supported"])["data"]
    info = (C.c_int32 * 4)()
    for cut in (0, 2, 20, len(data) // 2):                       # truncated files are refused with a reason
        assert L.ivit_jpeg_probe(_buf(data[:cut]), cut, info) == -2 and L.ivit_last_error_string()


def _plan(L, data):
    nb = C.c_int64(-1)
    rc = L.ivit_jpeg_plan_image(_buf(data), len(data), None, 0, C.byref(nb))
    if rc != 0:
        return rc, None
    assert nb.value > 0 and nb.value % 16 == 0
    sec = np.zeros(nb.value + 32, np.uint8)
    sec[nb.value:] = 0xA5
    nb2 = C.c_int64(-1)
    assert L.ivit_jpeg_plan_image(_buf(data), len(data), sec.ctypes.data_as(C.c_void_p), nb.value, C.byref(nb2)) == 0
    assert nb2.value == nb.value and (sec[nb.value:] == 0xA5).all()
    return 0, sec[:nb.value]


def test_jpeg_plan_image_direct():
    L = _lib.lib()
    for c in CASES:
        rc, sec = _plan(L, c["data"])
        assert (rc == 0) == c["supported"], c["name"]
        if rc == 0:       # the section starts with its own size, then (h, w)
            assert int(sec[:8].view(np.int64)[0]) == sec.size and tuple(sec[8:16].view(np.int32)) == (c["h"], c["w"]), c["name"]
        else:
            assert rc == -2, c["name"]
    data = next(c for c in CASES if c["supported"])["data"]
    nb = C.c_int64()
    assert L.ivit_jpeg_plan_image(_buf(data), len(data), None, 0, C.byref(nb)) == 0
    small = np.zeros(nb.value, np.uint8)
    assert L.ivit_jpeg_plan_image(_buf(data), len(data), small.ctypes.data_as(C.c_void_p), nb.value - 16, C.byref(nb)) == -1
    assert L.ivit_jpeg_plan_image(_buf(data[:len(data) // 2]), len(data) // 2, None, 0, C.byref(nb)) == -2


def test_jpeg_workspace_direct():
    L = _lib.lib()
    good = [c for c in CASES if c["supported"]]
    secs = [_plan(L, c["data"])[1] for c in good]
    plan = np.concatenate(secs)
    n = len(good) + 1                                             # one more image that is not decoded on the device
    sec_off = np.array(list(np.cumsum([0] + [s.size for s in secs[:-1]])) + [-1], np.int64)
    px = np.array([c["h"] * c["w"] * 3 for c in good] + [5 * 7 * 3], np.int64)
    out_off = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
    index = np.zeros(n * 40 + 8, np.uint8)
    index[n * 40:] = 0xA5
    sizes4 = (C.c_int64 * 4)()
    rc = L.ivit_jpeg_workspace(plan.ctypes.data_as(C.c_void_p), plan.size, sec_off.ctypes.data_as(C.c_void_p),
                               out_off.ctypes.data_as(C.c_void_p), n, index.ctypes.data_as(C.c_void_p), sizes4)
    assert rc == 0, L.ivit_last_error_string()
    assert (index[n * 40:] == 0xA5).all()
    assert sizes4[0] > 0 and sizes4[1] > 0 and sizes4[2] > 0
    assert sizes4[3] == max(c["h"] * c["w"] for c in good)


def test_jpeg_decode_host_direct():
    L = _lib.lib()
    for c in CASES:
        if not c["supported"] or c["pixels"] is None:
            continue
        out = np.zeros(c["h"] * c["w"] * 3 + 16, np.uint8)
        out[c["h"] * c["w"] * 3:] = 0xA5
        assert L.ivit_jpeg_decode_host(_buf(c["data"]), len(c["data"]), out.ctypes.data_as(C.c_void_p), c["h"] * c["w"] * 3) == 0
        assert np.array_equal(out[:-16].reshape(c["h"], c["w"], 3), c["pixels"]) and (out[-16:] == 0xA5).all(), c["name"]
        assert L.ivit_jpeg_decode_host(_buf(c["data"]), len(c["data"]), out.ctypes.data_as(C.c_void_p), c["h"] * c["w"] * 3 - 1) == -1
