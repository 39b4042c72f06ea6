"""The three wide entries with a leading dimension -- ivit_knn_topk_i8_wide, ivit_gram_i8_i64_wide, ivit_group_sums_i8_i64_wide -- with
ONE operand as a tests/far.py buffer: five rows of 1088 channels of which one starts below 2^31, one between 2^31 and 2^32 and the
others beyond 2^32 bytes.  A row offset that lost its upper bits reads the fill (127 in every channel) and shows as a failed
comparison.  The cases, sizes and the release of the buffers follow tests/test_gpu_far_knn.py and tests/test_gpu_far_probe.py."""
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
import probe_ref  # noqa: E402
from test_gpu_far_probe import DEV, as_dwords, st  # noqa: E402
from test_gpu_far_rows import done, far_in, same  # noqa: E402

ROWS, CH = 5, 1088


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


@pytest.mark.parametrize("operand", ["bank", "q"])
def test_knn_topk_wide_far_rows(operand):
    bank, q, k = _rows(32), _rows(33), 4
    rn = knn_ref.rnorm(bank)
    ridx, rsc = knn_ref.topk(q, bank, k, rn)
    ones = lambda a, width: np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=1)      # noqa: E731
    if operand == "bank":
        bf = far_in(bank, 16, 0, 127, oracle=lambda m: knn_ref.scores(ones(q, m.shape[1]), m).T, expected=knn_ref.scores(q, bank, rn).T)
        qf = fenced.input(q, CH + 16, 127)
    else:
        qf = far_in(q, 16, 0, 127, oracle=lambda m: knn_ref.topk(m, ones(bank, m.shape[1]), k)[1], expected=rsc)
        bf = fenced.input(bank, CH + 16, 127)
    assert (ROWS - 1) * max(bf.ld, qf.ld) > 2 ** 32
    rnd = torch.from_numpy(rn).to(DEV)
    idx = fenced.output(ROWS, k, k, np.int32, expected=ridx)
    score = fenced.output(ROWS, k, k, np.float32, expected=rsc)
    need = C.c_int64()
    _lib.call("ivit_knn_workspace_bytes", ROWS, ROWS, k, 2, C.byref(need))
    ws = torch.empty(max(need.value // 8, 1), dtype=torch.int64, device=DEV)
    _lib.call("ivit_knn_topk_i8_wide", qf.ptr, qf.ld, ROWS, bf.ptr, bf.ld, ROWS, CH, _lib.ptr(rnd), k, 2, idx.ptr, score.ptr, _lib.ptr(ws),
              need.value, st())
    torch.cuda.synchronize()
    done(idx, ridx)
    done(score, rsc)
    same(qf)
    same(bf)


def test_gram_and_group_sums_wide_far_rows():
    x = _rows(41)
    exp = probe_ref.gram(x)
    perm, ptr = probe_ref.csr([1, 0, 1, 2, 0], 3)
    sums = probe_ref.group_sums(x, perm, ptr)
    xf = far_in(x, 16, 0, 127, oracle=lambda m: as_dwords(probe_ref.gram(np.vstack([m[:, :CH], np.full((1, CH), 127, np.int8)]))),
                expected=as_dwords(exp))
    assert (ROWS - 1) * xf.ld > 2 ** 32
    out = fenced.output(CH, 2 * CH, 2 * CH, np.int32, expected=as_dwords(exp))
    need = C.c_int64()
    _lib.call("ivit_gram_wide_workspace_bytes", ROWS, CH, 2, C.byref(need))
    ws = torch.empty(need.value // 4, dtype=torch.int32, device=DEV)
    _lib.call("ivit_gram_i8_i64_wide", xf.ptr, xf.ld, ROWS, CH, 2, 0, out.ptr, _lib.ptr(ws), need.value, st())
    pd, gd = torch.from_numpy(perm).to(DEV), torch.from_numpy(ptr).to(DEV)
    sout = fenced.output(3, 2 * CH, 2 * CH, np.int32, expected=as_dwords(sums))
    _lib.call("ivit_group_sums_i8_i64_wide", xf.ptr, xf.ld, ROWS, CH, _lib.ptr(pd), _lib.ptr(gd), 3, 0, sout.ptr, st())
    torch.cuda.synchronize()
    fenced.check(out, as_dwords(exp))
    fenced.check(sout, as_dwords(sums))
    same(xf)
