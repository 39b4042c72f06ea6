"""ivit_rows_rnorm_i8_f32 and ivit_knn_topk_i8 with ONE operand as a tests/far.py buffer: five rows of 64 channels of which one starts
below 2^31, one between 2^31 and 2^32 and the others beyond 2^32 bytes -- the rows of x, of the bank, or of the queries; the other
operands are near `fenced` buffers.  A row offset that lost its upper bits reads the fill (127 in every channel: another norm,
another score) and shows as a failed comparison (far.py: never as a fault).  Sizes, the skip and the release of the buffers follow
tests/test_gpu_far_rows.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
import fenced  # noqa: E402
import knn_ref  # noqa: E402
from test_gpu_far_rows import done, far_in, same  # noqa: E402

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


@pytest.mark.parametrize("strides", ["al16", "min"])
def test_rows_rnorm_far_rows(strides):
    x = _rows(31)
    exp = knn_ref.rnorm(x)
    al = strides == "al16"
    xf = far_in(x, 16 if al else 1, 0 if al else 1, 127, oracle=lambda m: knn_ref.rnorm(m)[:, None], expected=exp[:, None])
    assert (ROWS - 1) * xf.ld > 2 ** 32
    out = fenced.output(1, ROWS, ROWS, np.float32, expected=exp[None, :])
    _lib.call("ivit_rows_rnorm_i8_f32", xf.ptr, xf.ld, ROWS, CH, out.ptr, st())
    torch.cuda.synchronize()
    done(out, exp[None, :])
    same(xf)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("operand", ["bank", "q"])
def test_knn_topk_far_rows(operand, splits):
    bank, q = _rows(32), _rows(33)
    k = 4
    rn = knn_ref.rnorm(bank)
    ridx, rsc = knn_ref.topk(q, bank, k, rn)

    def ones(a, width):
        return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=1)

    if operand == "bank":
        bf = far_in(bank, 16, 0, 127, oracle=lambda m: knn_ref.scores(ones(q, m.shape[1]), m).T, expected=knn_ref.scores(q, bank, rn).T)
        qf = fenced.input(q, CH + 16, 127)
        assert (ROWS - 1) * bf.ld > 2 ** 32
    else:
        qf = far_in(q, 16, 0, 127, oracle=lambda m: knn_ref.topk(m, ones(bank, m.shape[1]), k)[1], expected=rsc)
        bf = fenced.input(bank, CH + 16, 127)
        assert (ROWS - 1) * qf.ld > 2 ** 32
    rnd = torch.from_numpy(rn).to(DEV)
    idx = fenced.output(ROWS, k, k, np.int32, expected=ridx)
    score = fenced.output(ROWS, k, k, np.float32, expected=rsc)
    need = C.c_int64()
    _lib.call("ivit_knn_workspace_bytes", ROWS, ROWS, k, splits, C.byref(need))
    ws = torch.empty(max(need.value // 8, 1), dtype=torch.int64, device=DEV)
    _lib.call("ivit_knn_topk_i8", qf.ptr, qf.ld, ROWS, bf.ptr, bf.ld, ROWS, CH, _lib.ptr(rnd), k, splits, idx.ptr, score.ptr, _lib.ptr(ws),
              need.value, st())
    torch.cuda.synchronize()
    done(idx, ridx)
    done(score, rsc)
    same(qf)
    same(bf)
