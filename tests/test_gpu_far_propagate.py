"""ivit_local_topk_i8 with ONE operand -- the context tokens, or the targets -- as a tests/far.py buffer whose rows start below 2^31,
between 2^31 and 2^32 and beyond 2^32 bytes; the other operand and both outputs are near `fenced` buffers.  A grid of 1 x 5 tokens, one
frame, radius 4: every target sees all five rows.  Follows tests/test_gpu_far_ranks.py."""
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
import propagate_ref  # noqa: E402
from test_gpu_far_knn import CH, DEV, ROWS, _release, _release_all, _rows, st  # noqa: E402, F401
from test_gpu_far_rows import done, far_in, same  # noqa: E402


@pytest.mark.parametrize("operand", ["bank", "q"])
def test_local_topk_far_rows(operand):
    bank, q = _rows(36), _rows(37)
    k = 4
    rn = knn_ref.rnorm(bank)
    ridx, rsc = propagate_ref.local_topk(q, bank, rn, 1, ROWS, 1, 4, k)

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
    _lib.call("ivit_local_topk_workspace_bytes", 1, ROWS, 1, k, 1, C.byref(need))
    _lib.call("ivit_local_topk_i8", qf.ptr, qf.ld, 1, ROWS, bf.ptr, bf.ld, 1, CH, _lib.ptr(rnd), 4, k, 1, idx.ptr, score.ptr, None, need.value, st())
    torch.cuda.synchronize()
    done(idx, ridx)
    done(score, rsc)
    same(qf)
    same(bf)
