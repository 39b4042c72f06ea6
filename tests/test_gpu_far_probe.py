"""ivit_gram_i8_i64 and ivit_group_sums_i8_i64 with the bank as a tests/far.py buffer: five rows of 64 channels of which one starts
below 2^31, one between 2^31 and 2^32 and the others beyond 2^32 bytes; the other operands are near `fenced` buffers.  A row offset
that lost its upper bits reads the fill (127 in every channel: another product, another sum) and shows as a failed comparison
(far.py: never as a fault).  Only the 16-byte stride exists: both entries want x and ldx on 16-byte boundaries.  Sizes, the skip
and the release of the buffers follow tests/test_gpu_far_knn.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import probe_ref  # noqa: E402
from test_gpu_far_rows import far_in, same  # noqa: E402

DEV = "cuda:0"
ROWS, CH = 5, 64


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


def _rows(seed):
    a = np.random.default_rng(seed).integers(-100, 101, size=(ROWS, CH)).astype(np.int8)      # (no row could pass for the fill, 127)
    a[0, 0], a[-1, -1] = -128, 127
    return a


def as_dwords(a64):
    a64 = np.ascontiguousarray(a64, np.int64)
    return a64.view(np.int32).reshape(a64.shape[0], -1)


@pytest.mark.parametrize("splits", [1, 2])
def test_gram_far_rows(splits):
    x = _rows(41)
    exp = probe_ref.gram(x)
    # the poison: a row read from the fill instead (what a truncated offset finds) changes every row of the Gram
    xf = far_in(x, 16, 0, 127, oracle=lambda m: as_dwords(probe_ref.gram(np.vstack([m[:, :CH], np.full((1, CH), 127, np.int8)]))),
                expected=as_dwords(exp))
    assert (ROWS - 1) * xf.ld > 2 ** 32
    out = fenced.output(CH, 2 * CH, 2 * CH, np.int32, expected=as_dwords(exp))
    need = C.c_int64()
    _lib.call("ivit_gram_workspace_bytes", ROWS, CH, splits, C.byref(need))
    ws = torch.empty(need.value // 4, dtype=torch.int32, device=DEV)
    _lib.call("ivit_gram_i8_i64", xf.ptr, xf.ld, ROWS, CH, splits, 0, out.ptr, _lib.ptr(ws), need.value, st())
    torch.cuda.synchronize()
    fenced.check(out, as_dwords(exp))
    same(xf)


def test_group_sums_far_rows():
    x = _rows(42)
    perm, ptr = probe_ref.csr([1, 0, 1, 2, 0], 3)
    exp = probe_ref.group_sums(x, perm, ptr)
    xf = far_in(x, 16, 0, 127, oracle=lambda m: as_dwords(probe_ref.group_sums(m[:, 4:], perm, ptr)), expected=as_dwords(exp))
    assert (ROWS - 1) * xf.ld > 2 ** 32
    pf = fenced.input(perm[None, :], ROWS, 0)
    gf = fenced.input(as_dwords(ptr[None, :]), 2 * len(ptr), 2 ** 30)
    out = fenced.output(3, 2 * CH, 2 * CH, np.int32, expected=as_dwords(exp))
    _lib.call("ivit_group_sums_i8_i64", xf.ptr, xf.ld, ROWS, CH, pf.ptr, gf.ptr, 3, 0, out.ptr, st())
    torch.cuda.synchronize()
    fenced.check(out, as_dwords(exp))
    same(xf)
    fenced.check(pf)
    fenced.check(gf)
