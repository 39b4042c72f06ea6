"""Operands of more than 4 GiB for the four pooled-LayerNorm entries (csrc/ln_pool.h, csrc/pool.hip): once with the token rows of `x`
far (a row starts below 2^31, between 2^31 and 2^32 and beyond 2^32 bytes), once with the rows of the int8 `out` far -- tests/far.py
buffers, as tests/test_gpu_far_rows.py builds them; the other operand is a near fenced buffer (ldx > C, ldo > C between sentinels).  Problems and expectations are those of tests/test_gpu_ln_pool.py.
tests/test_far_coverage_cpu.py keeps the list complete."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import test_gpu_ln_pool as K  # noqa: E402
from test_gpu_far_rows import far_in, far_out  # noqa: E402

SEL, C = (3, 4, 1, 3), 96      # 12 token rows; three rows of means


@pytest.fixture(autouse=True)
def _release():
    yield
    far.release()


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


def operands(family, bits, operand):
    """-> (ln, entry arguments, flags, workspace, x pointer, ldx, out pointer, ldo, sums, finish())"""
    ln, k = K.make_ln(family, bits, C), K.rows(bits, SEL[0] * SEL[1], C)
    want_sum, want_mean = K.reference(ln, k, SEL)
    _, mid, flags, ws = K.pool_args(ln, SEL, C)
    total = torch.full((SEL[0], C), -1, dtype=torch.int32, device=K.DEV)
    x = far_in(k, 4) if operand == "x" else fenced.input(k, C + 8, fenced.POISON[k.dtype], device=K.DEV)
    mean8 = want_mean.astype(np.int8)
    o = far_out(SEL[0], C, np.int8, mean8, 4) if operand == "out" else fenced.output(SEL[0], C, C + 4, np.int8, expected=mean8, device=K.DEV)

    def finish():
        assert np.array_equal(total.cpu().numpy(), want_sum)
        far.check(o, mean8) if isinstance(o, far.Buffer) else fenced.check(o, mean8)
        far.check(x) if isinstance(x, far.Buffer) else fenced.check(x)

    return (x.ptr, x.ld, *SEL, C, *mid, _lib.ptr(total), o.ptr, o.ld, 0, flags, _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), finish


@pytest.mark.parametrize("operand", ["x", "out"])
def test_layernorm_pool_i8_far(operand):
    args, finish = operands("ivit", 8, operand)
    _lib.call("ivit_layernorm_pool_i8", *args)
    finish()


@pytest.mark.parametrize("operand", ["x", "out"])
def test_layernorm_pool_i16_far(operand):
    args, finish = operands("ivit", 16, operand)
    _lib.call("ivit_layernorm_pool_i16", *args)
    finish()


@pytest.mark.parametrize("operand", ["x", "out"])
def test_ibert_layernorm_pool_i8_far(operand):
    args, finish = operands("ibert_intsqrt", 8, operand)
    _lib.call("ivit_ibert_layernorm_pool_i8", *args)
    finish()


@pytest.mark.parametrize("operand", ["x", "out"])
def test_ibert_layernorm_pool_i16_far(operand):
    args, finish = operands("ibert", 16, operand)
    _lib.call("ivit_ibert_layernorm_pool_i16", *args)
    finish()
