"""Operands of more than 4 GiB for the four token-feature LayerNorm entries (csrc/ln_tokens.h): once with the token rows of `x` far
(ldx beyond 2^32 / rows bytes: a row starts below 2^31, between 2^31 and 2^32 and beyond 2^32 bytes), once with the rows of a
rows-form `out` far, once with the channel rows of a channel-major `out` far -- tests/far.py buffers, as tests/test_gpu_far_rows.py
builds them; the other operand is a near fenced buffer.  Problems and expectations are those of tests/test_gpu_layernorm_f32.py.
tests/test_far_coverage_cpu.py keeps the list complete."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import test_gpu_layernorm_f32 as K  # noqa: E402
from test_gpu_far_rows import far_in, far_out  # noqa: E402

CM, FAST, ISQ, p, st = K.CM, K.FAST, K.ISQ, K.p, K.st
OPERANDS = ["x", "out", "out_channel_major"]
SEL = (2, 5, 1, 4)      # 10 token rows, 8 selected; channel-major: 2 * C channel rows of 4 tokens


@pytest.fixture(autouse=True)
def _release():
    yield
    far.release()


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


def operands(case, operand, multiple):
    """-> (x, out, expected [rows, width], channel-major?) with the named operand far"""
    B, T_all, t0, T = SEL
    cm = operand == "out_channel_major"
    src = case.k[: B * T_all]
    exp = case.expected(SEL, cm)
    exp = exp.reshape(-1, exp.shape[-1])
    if operand == "x":
        x = far_in(src, multiple)
        o = fenced.output(exp.shape[0], exp.shape[1], exp.shape[1] + 3, np.float32, expected=exp, device=K.DEV)
    else:
        x = fenced.input(src, case.C + 8, fenced.POISON[src.dtype], device=K.DEV)
        o = far_out(exp.shape[0], exp.shape[1], np.float32, exp)
    return x, o, exp, cm


def finish(x, o, exp):
    far.check(o, exp) if isinstance(o, far.Buffer) else fenced.check(o, exp)
    far.check(x) if isinstance(x, far.Buffer) else fenced.check(x)


@pytest.mark.parametrize("operand", OPERANDS)
@pytest.mark.parametrize("kind,scale", [("i8", "pow2"), ("i8_compat", "natural")])
def test_layernorm_i8_f32_far(kind, scale, operand):
    case = K.Case(kind, 96, scale)
    x, o, exp, cm = operands(case, operand, 4)
    r, ph = (None, None) if case.tabs is None else (p(case.tabs[0]), p(case.tabs[1]))
    _lib.call("ivit_layernorm_i8_f32", x.ptr, x.ld, *SEL, case.C, p(case.d_bias), p(case.d_s), r, ph, o.ptr, o.ld, CM if cm else 0, st())
    finish(x, o, exp)


@pytest.mark.parametrize("operand", OPERANDS)
@pytest.mark.parametrize("kind,scale", [("i16", "pow2"), ("i16_compat", "natural")])
def test_layernorm_i16_f32_far(kind, scale, operand):
    case = K.Case(kind, 100, scale, fast=kind == "i16_compat")
    x, o, exp, cm = operands(case, operand, 1)
    _lib.call("ivit_layernorm_i16_f32", x.ptr, x.ld, *SEL, case.C, float(case.s_in) if case.fast else 0.0, p(case.d_bias), p(case.d_s),
              o.ptr, o.ld, (CM if cm else 0) | (FAST if case.fast else 0), st())
    finish(x, o, exp)


@pytest.mark.parametrize("operand", OPERANDS)
def test_ibert_layernorm_i8_f32_far(operand):
    case = K.Case("ibert_i8", 100, "natural", isq=True)
    x, o, exp, cm = operands(case, operand, 1)
    _lib.call("ivit_ibert_layernorm_i8_f32", x.ptr, x.ld, *SEL, case.C, float(case.s_in), p(case.d_bias), p(case.d_s),
              float(case.shift_pow2), o.ptr, o.ld, (CM if cm else 0) | ISQ, st())
    finish(x, o, exp)


@pytest.mark.parametrize("operand", OPERANDS)
def test_ibert_layernorm_i16_f32_far(operand):
    case = K.Case("ibert_i16", 100, "natural", fast=True)
    x, o, exp, cm = operands(case, operand, 1)
    _lib.call("ivit_ibert_layernorm_i16_f32", x.ptr, x.ld, *SEL, case.C, float(case.s_in), p(case.d_bias), p(case.d_s),
              float(case.shift_pow2), o.ptr, o.ld, (CM if cm else 0) | FAST, st())
    finish(x, o, exp)
