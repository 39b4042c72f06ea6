"""The ratchet of the far rows, built on the helpers of test_strides_coverage_cpu.py: every function of include/ivit_hip.h with a
leading dimension is called BY NAME inside a GPU test function of tests/test_gpu_far_*.py that builds a tests/far.py operand
(directly or through a function of the same file that does).  There is no table of exceptions: a new strided export fails here
until it has its case, and deleting the only far case of an entry fails here too (shown on the real files).

The ratchet counts entries, not leading dimensions: which operand of an entry is far is the parametrisation of its test, which a
syntax tree does not show.  BOUNDS ties the launcher bounds -- they belong to a layout or an output form (IVIT_W_FRAGS16, block
layout, head-major q/k/v), none to one entry's own leading dimension -- to their sentence of the header and to the test that
crosses them.  DENSE lists the entries the issue names that have no `ld` parameter and so are not in ld_exports(), with the test
of the far dimension they do have."""
import ast
import glob
import os
import re

from test_abi_coverage_cpu import ROOT, TESTS
from test_strides_coverage_cpu import _entry_of, _function, ld_exports

# entry without a leading dimension -> "file::function" of its test beyond 2^31 elements / 2^32 bytes
DENSE = {
    "ivit_window_rows": "test_gpu_far_flat.py::test_window_rows_beyond_2_32_bytes",
    "ivit_patch_merge_i16": "test_gpu_far_flat.py::test_patch_merge_i16_beyond_2_31_elements",
}


def _is_far(call):
    """far.input(...) / far.output(...), or Flat(...) of tests/test_gpu_far_flat.py (a dense operand with the same guards)"""
    f = call.func
    if isinstance(f, ast.Name) and f.id == "Flat":
        return True
    return isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "far" and f.attr in ("input", "output")


def far_calls(path):
    """{entry: [test functions]}: entries called by name inside a top-level test function of `path` that builds a far operand,
    directly or through a function of the same file (or one imported by name from another test file) that does"""
    tree = ast.parse(open(path).read(), path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    makers = {d.name for d in defs if any(isinstance(n, ast.Call) and _is_far(n) for n in ast.walk(d))}
    for n in tree.body:      # from test_gpu_far_rows import far_in: a maker of that file
        if isinstance(n, ast.ImportFrom) and n.module and n.module.startswith("test_gpu_"):
            other = os.path.join(TESTS, n.module + ".py")
            theirs = _makers(other) if os.path.exists(other) else set()
            makers |= {a.asname or a.name for a in n.names if a.name in theirs}
    makers |= {d.name for d in defs if not d.name.startswith("test_")
               and any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in makers for n in ast.walk(d))}
    out = {}
    for d in defs:
        if not d.name.startswith("test_"):
            continue
        calls = [n for n in ast.walk(d) if isinstance(n, ast.Call)]
        if not any(_is_far(c) or (isinstance(c.func, ast.Name) and c.func.id in makers) for c in calls):
            continue
        for c in calls:
            e = _entry_of(c)
            if e:
                out.setdefault(e[0], []).append(d.name)
    return out


def _makers(path):
    tree = ast.parse(open(path).read(), path)
    return {d.name for d in tree.body if isinstance(d, ast.FunctionDef) and any(isinstance(n, ast.Call) and _is_far(n) for n in ast.walk(d))}


def all_far_calls():
    out = {}
    for path in sorted(glob.glob(os.path.join(TESTS, "test_gpu_far_*.py"))):
        for k, v in far_calls(path).items():
            out.setdefault(k, []).extend(f"{os.path.basename(path)}::{f}" for f in v)
    return out


def test_far_calls_sees_calls_inside_far_tests_only(tmp_path):
    f = tmp_path / "test_gpu_far_demo.py"
    f.write_text('import far\nimport fenced\n'
                 'def far_out(*a):\n    return far.output(*a)\n'
                 'def wrapped(*a):\n    return far_out(*a)\n'
                 'def test_direct(_lib):\n    o = far.input(1, 2, 3)\n    _lib.call("ivit_a", o)\n'
                 'def test_through_maker(_lib):\n    o = wrapped(1)\n    _lib.call("ivit_b", o)\n'
                 'def test_near_only(_lib):\n    o = fenced.output(1, 2, 3, 4)\n    _lib.call("ivit_c", o)\n'
                 'def test_by_variable(_lib):\n    o = far.output(1)\n    for n in ["ivit_d"]:\n        _lib.call(n, o)\n')
    assert far_calls(str(f)) == {"ivit_a": ["test_direct"], "ivit_b": ["test_through_maker"]}


def missing_entries(covered):
    ex = ld_exports()
    return [n for n in ex if n not in covered]


def test_every_strided_export_has_a_far_case():
    ex = ld_exports()
    covered = all_far_calls()
    missing = missing_entries(covered)
    assert not missing, f"{len(missing)} exports with a leading dimension have no far-row GPU test: {missing}"
    for entry, where in DENSE.items():
        assert entry not in ex, f"{entry} has a leading dimension now: give it a far-row case"
        fname, func = where.split("::")
        fn = _function(os.path.join(TESTS, fname), func)
        assert fn is not None and entry in ast.dump(fn), f"{where} does not call {entry}"


def test_deleting_a_far_case_fails_the_ratchet(tmp_path, monkeypatch):
    """every top-level test function of the far files removed in turn (the file re-parsed without it): whenever that takes the
    last far case of an entry away, the ratchet names the entry"""
    import test_far_coverage_cpu as me
    ex = ld_exports()
    full = all_far_calls()
    sole = {}          # test function -> entries only it covers
    for entry, tests in full.items():
        if entry in ex and len(set(tests)) == 1:
            sole.setdefault(tests[0], []).append(entry)
    assert sole, "no entry is covered by exactly one test: nothing to delete"
    for where, entries in sole.items():
        fname, func = where.split("::")
        tree = ast.parse(open(os.path.join(TESTS, fname)).read())
        tree.body = [n for n in tree.body if not (isinstance(n, ast.FunctionDef) and n.name == func)]
        for other in glob.glob(os.path.join(TESTS, "test_gpu_far_*.py")):
            dst = tmp_path / os.path.basename(other)
            dst.write_text(ast.unparse(tree) if os.path.basename(other) == fname else open(other).read())
        monkeypatch.setattr(me, "TESTS", str(tmp_path))
        assert sorted(missing_entries(all_far_calls())) == sorted(entries), where
        monkeypatch.undo()


# ---------------------------------------------------------------------------- the bounds that are not an entry's own
# sentence of include/ivit_hip.h -> "file::function" of the test that runs below the bound and is refused at it
BOUNDS = {
    "(M + 16) * ldo < 2^32 and (M + 16) * ldr < 2^32, otherwise IVIT_ERR_INVALID": "test_gpu_far_bounds.py::test_gemm_frags16_offset_bound",
    "every entry that writes the layout wants (rows + 15) * K < 2^31 and is IVIT_ERR_INVALID beyond": "test_gpu_far_bounds.py::test_block_layout_output_of_2_gib_is_refused",
    "the dense head-major q/k/v outputs (M * N < 2^31 bytes; planes form 3 * M * heads * head_dim < 2^31)": "test_gpu_far_bounds.py::test_gemm_head_major_output_bound",
    "row_bytes % 16 != 0 or row_bytes > 2^20": "test_gpu_far_flat.py::test_window_rows_beyond_2_32_bytes",
}


def _header_text():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ivit_hip.h")).read().replace("\n *", " "))


def test_bounds_are_stated_in_the_header_and_checked():
    header = _header_text()
    for sentence, where in BOUNDS.items():
        assert sentence in header, f"the header does not say: {sentence}"
        fname, func = where.split("::")
        fn = _function(os.path.join(TESTS, fname), func)
        assert fn is not None, f"{where} does not exist"
        src = ast.dump(fn)
        assert "refused" in src or "raises" in src, f"{where} checks no refusal"
