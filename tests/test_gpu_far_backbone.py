"""ivit_dequant_rows_i8_f32 with ONE operand as a tests/far.py buffer: twelve rows of which one starts below 2^31, some between 2^31
and 2^32 and some beyond 2^32 bytes -- of the int8 input, or of the float32 output; the other operand is a near `fenced` buffer.  A
row offset that lost its upper bits shows as a wrong or never-stored value or as a damaged fill (far.py: never as a fault).
Sizes, the skip and the release of the buffers follow tests/test_gpu_far_rows.py.

Which path the rows take: a leading dimension that is a multiple of 16 bytes keeps every row on the wide path (16 int8 in one load,
four float4 stores); the smallest granularity of the entry (1 byte of input, one float of output) mixes wide rows with rows that go
element by element."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
from test_gpu_far_rows import done, far_in, far_out, same  # noqa: E402

DEV = "cuda:0"
f32 = np.float32
ROWS, C, S = 12, 1000, f32(0.0123)


def st():
    return _lib.stream_ptr()


@pytest.fixture(autouse=True)
def _release():
    yield
    far.release()


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


@pytest.mark.parametrize("strides", ["al16", "min"])
@pytest.mark.parametrize("operand", ["x", "out"])
def test_dequant_rows_far_rows(operand, strides):
    q = np.random.default_rng(12).integers(-128, 128, size=(ROWS, C)).astype(np.int8)
    q[0, 0], q[-1, -1] = -128, 127
    exp = q.astype(f32) * S
    al = strides == "al16"

    # (an elementwise operator: no poison condition to show -- a row read at a truncated offset is the fill, 127, in every channel)
    if operand == "x":      # rows of the input beyond 2^31 (and 2^32) bytes
        x = far_in(q, 16 if al else 1, 0 if al else 1, 127)
        o = fenced.output(ROWS, C, C + (4 if al else 5), np.float32, expected=exp, lead_bytes=0 if al else 4)
    else:                   # rows of the output beyond 2^32 bytes
        x = fenced.input(q, C + (24 if al else 13), 127, lead_bytes=0 if al else 1)
        o = far_out(ROWS, C, np.float32, exp, 4 if al else 1, 0 if al else 4)
    assert (ROWS - 1) * (x.ld if operand == "x" else 4 * o.ld) > 2 ** 32
    _lib.call("ivit_dequant_rows_i8_f32", x.ptr, x.ld, ROWS, C, float(S), o.ptr, o.ld, st())
    torch.cuda.synchronize()
    done(o, exp)
    same(x)
