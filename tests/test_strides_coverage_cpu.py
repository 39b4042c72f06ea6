"""The ratchet of the leading dimensions, in the spirit of test_abi_coverage_cpu.py: every function of include/ivit_hip.h that takes a
parameter named `ld` or `ld?` (lda, ldw, ldo, ldr, ldx) is called BY NAME -- found in the syntax tree -- inside a GPU test function
that also builds a fenced operand (tests/fenced.py: strided rows between poisoned pads, sentinel-filled outputs, guard rows), or is
listed in ALREADY_FENCED with the function whose own padded buffers do that job.  A new strided entry without such a test fails
here, on the CPU.

ALREADY_FENCED is checked too: the named function exists, calls the entry by name, and the leading dimension it passes is not the
bare width, i.e. not the expression it passes as any other argument of the same call."""
import ast
import glob
import os
import re

from test_abi_coverage_cpu import ROOT, TESTS, declared_names

# entry -> "file::function": tests from before tests/fenced.py that run the entry with ld > width into padded, value-filled buffers
# and assert that the pads keep their fill
ALREADY_FENCED = {
    "ivit_quantize_patchify_ld_f32_i8": "test_gpu_swin.py::test_patchify_ld",
    "ivit_quantize_patchify_u8_i8": "test_gpu_module_kernels.py::test_quantize_patchify_u8",
    "ivit_attention_cls_i8": "test_gpu_cls_tail.py::_run_cls",
    "ivit_layernorm_f32_f32": "test_gpu_module_kernels.py::_ln_literal",
    "ivit_layernorm_f32_f32_ex": "test_gpu_module_kernels.py::_ln_literal",
    "ivit_shiftmax_i8": "test_gpu_module_kernels.py::_shiftmax_int",
    "ivit_shiftmax_i32_i8": "test_gpu_module_kernels.py::_shiftmax_int",
    "ivit_shiftmax_f32_i8": "test_gpu_module_kernels.py::_shiftmax_f32",
    "ivit_shiftmax_f32_i16": "test_gpu_module_kernels.py::_shiftmax_f32",
    "ivit_head_topk": "test_gpu_topk.py::head_topk",
    "ivit_logits_topk_f32": "test_gpu_topk.py::logits_topk",
    "ivit_ibert_softmax_i32": "test_gpu_ibert_ops.py::_softmax_run",
    "ivit_ibert_softmax_f32_f32": "test_gpu_ibert_ops.py::_softmax_run",
    "ivit_ibert_layernorm_i32_f32": "test_gpu_ibert_ops.py::_ln_run",
    "ivit_ibert_layernorm_f32_f32": "test_gpu_ibert_ops.py::_ln_run",
    # window attention: ld = nH * hd + 32 into a zero-filled buffer, pads asserted zero (the image-ordered form is compared whole,
    # pads included, with the window-ordered one); the other four entries have fenced cases in test_gpu_strides.py
    "ivit_window_attention_i8": "test_gpu_swin.py::test_window_attention",
    "ivit_window_attention_i8_unwindow": "test_gpu_swin.py::test_window_attention",
}

LD = re.compile(r"^ld[a-z]?$")


def ld_exports(header=None):
    """{entry: [parameter names]} for every export with a leading dimension"""
    text = header if header is not None else open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(ivit_[a-z0-9_]+)\s*\(([^)]*)\)", text):
        names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", prm)[-1] for prm in params.split(",") if prm.strip() and prm.strip() != "void"]
        if any(LD.match(n) for n in names):
            out[name] = names
    return out


def _entry_of(call):
    """the entry a Call node calls by name: `.call("NAME", ...)` -> (NAME, its arguments) or `X.ivit_name(...)`; else None"""
    if not isinstance(call.func, ast.Attribute):
        return None
    if call.func.attr == "call" and call.args and isinstance(call.args[0], ast.Constant) and isinstance(call.args[0].value, str):
        return call.args[0].value, call.args[1:]
    if call.func.attr.startswith("ivit_"):
        return call.func.attr, call.args
    return None


def _is_fence(call):
    f = call.func
    return isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "fenced" and f.attr in ("input", "output", "input_blocks")


def fenced_calls(path):
    """{entry: [test functions]} -- entries called by name inside a top-level test function of `path` that builds a fenced operand,
    directly or through a function (or a class) of the same file that does"""
    tree = ast.parse(open(path).read(), path)
    defs = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
    makers = {d.name for d in defs if any(isinstance(n, ast.Call) and _is_fence(n) for n in ast.walk(d))}
    for _ in range(2):      # a class whose constructor calls such a function, one more level
        makers |= {d.name for d in defs
                   if any(isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in makers for n in ast.walk(d))
                   and not d.name.startswith("test_")}
    out = {}
    for d in defs:
        if not (isinstance(d, ast.FunctionDef) and d.name.startswith("test_")):
            continue
        calls = [n for n in ast.walk(d) if isinstance(n, ast.Call)]
        if not any(_is_fence(c) or (isinstance(c.func, ast.Name) and c.func.id in makers) for c in calls):
            continue
        for c in calls:
            e = _entry_of(c)
            if e:
                out.setdefault(e[0], []).append(d.name)
    return out


def all_fenced_calls():
    out = {}
    for path in sorted(glob.glob(os.path.join(TESTS, "test_gpu_*.py"))):
        for k, v in fenced_calls(path).items():
            out.setdefault(k, []).extend(f"{os.path.basename(path)}::{f}" for f in v)
    return out


def test_header_parse_sees_the_strided_entries():
    ex = ld_exports()
    assert len(ex) >= 50 and set(ex) <= set(declared_names())
    assert ex["ivit_untile_operand_i8"] == ["src", "rows", "K", "dst", "ld", "stream"]
    assert [n for n in ex["ivit_gemm_i8_requant_residual"] if LD.match(n)] == ["lda", "ldw", "ldr", "ldo"]
    assert "ivit_residual_requant_i8" not in ex and "ivit_layernorm_i16_i8" in ex and "ivit_head_topk" in ex
    demo = "int ivit_x(const int8_t* a /* [n] (dense) */, int64_t ldq, int n);\nint ivit_y(const float* ldexp_table, int n);\n"
    assert ld_exports(demo) == {"ivit_x": ["a", "ldq", "n"]}


def test_fenced_calls_sees_calls_inside_fencing_tests_only(tmp_path):
    f = tmp_path / "test_gpu_demo.py"
    f.write_text('import fenced\n'
                 'def fout(*a):\n    return fenced.output(*a)\n'
                 'class G:\n    def __init__(self):\n        self.a = fout(1)\n'
                 'def helper(_lib):\n    _lib.call("ivit_in_helper", fenced.input(1, 2, 3))\n'
                 'def test_direct(_lib):\n    o = fenced.output(1, 2, 3, 4)\n    _lib.call("ivit_a", o)\n'
                 'def test_through_wrapper(_lib, L):\n    o = fout(1)\n    L.ivit_b(o)\n'
                 'def test_through_class(_lib):\n    g = G()\n    _lib.call("ivit_c", g)\n'
                 'def test_unfenced(_lib):\n    "fenced.output"\n    _lib.call("ivit_d", 1)\n'
                 'def test_by_variable(_lib):\n    o = fenced.output(1, 2, 3, 4)\n    NAMES = ["ivit_e"]\n    for n in NAMES:\n        _lib.call(n, o)\n')
    got = fenced_calls(str(f))
    assert got == {"ivit_a": ["test_direct"], "ivit_b": ["test_through_wrapper"], "ivit_c": ["test_through_class"]}


def test_every_strided_export_has_a_fenced_test():
    covered = all_fenced_calls()
    missing = [n for n in ld_exports() if n not in covered and n not in ALREADY_FENCED]
    assert not missing, f"{len(missing)} exports with a leading dimension have no fenced GPU test: {missing}"
    both = [n for n in ALREADY_FENCED if n in covered]
    assert not both, f"listed in ALREADY_FENCED and covered by a fenced test (drop the listing): {both}"
    stale = [n for n in ALREADY_FENCED if n not in ld_exports()]
    assert not stale, stale


# ---------------------------------------------------------------------------- the table
def _function(path, name):
    for n in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(n, ast.FunctionDef) and n.name == name:
            return n
    return None


def _assigned(fn, name):
    """the expression a plain `name = expr` inside fn assigns (the last one), else None"""
    val = None
    for n in ast.walk(fn):
        if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name) and n.targets[0].id == name:
            val = n.value
    return val


def _spliced(fn, args):
    """positional arguments with `*name` replaced by the tuple / list literal assigned to name in fn; None if one cannot be resolved"""
    out = []
    for a in args:
        if isinstance(a, ast.Starred):
            v = _assigned(fn, a.value.id) if isinstance(a.value, ast.Name) else a.value
            if not isinstance(v, (ast.Tuple, ast.List)):
                return out, False          # what follows cannot be placed
            out.extend(v.elts)
        else:
            out.append(a)
    return out, True


def strided_lds(fn, entry, params):
    """for every call of `entry` in fn: the ld parameters whose argument is not the expression of any other argument of that call
    (a plainly assigned name counts as the expression assigned to it)"""
    found = []
    for c in ast.walk(fn):
        if not isinstance(c, ast.Call) or (_entry_of(c) or (None,))[0] != entry:
            continue
        args, _ = _spliced(fn, _entry_of(c)[1])

        def expr(a):
            v = _assigned(fn, a.id) if isinstance(a, ast.Name) else None
            return ast.dump(v if v is not None else a)
        dumps = [expr(a) for a in args]
        for i, prm in enumerate(params[:len(args)]):
            if LD.match(prm) and dumps[i] not in dumps[:i] + dumps[i + 1:]:
                found.append(prm)
    return found


def test_strided_lds_tells_a_bare_width_from_a_padded_one(tmp_path):
    f = tmp_path / "t.py"
    f.write_text('def bare(_lib, x, o, L):\n    _lib.call("ivit_s", x, L, 4, L, o, L)\n'
                 'def padded(_lib, x, o, L):\n    ldo = L + 5\n    args = (x, L + 3, 4, L)\n    _lib.call("ivit_s", *args, o, ldo)\n'
                 'def renamed(_lib, x, o, L):\n    ld = L\n    _lib.call("ivit_s", x, ld, 4, L, o, ld)\n')
    prm = ["x", "ldx", "rows", "L", "out", "ldo"]
    assert strided_lds(_function(str(f), "bare"), "ivit_s", prm) == []
    assert strided_lds(_function(str(f), "padded"), "ivit_s", prm) == ["ldx", "ldo"]
    assert strided_lds(_function(str(f), "renamed"), "ivit_s", prm) == []


def test_already_fenced_table_is_true():
    ex = ld_exports()
    for entry, where in ALREADY_FENCED.items():
        fname, func = where.split("::")
        fn = _function(os.path.join(TESTS, fname), func)
        assert fn is not None, f"{where} does not exist"
        assert strided_lds(fn, entry, ex[entry]), f"{where} does not call {entry} with a leading dimension other than the bare width"
