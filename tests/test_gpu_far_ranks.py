"""ivit_knn_ranks_i8 with ONE operand -- the bank, or the queries -- as a tests/far.py buffer whose rows start below 2^31, between 2^31 and
2^32 and beyond 2^32 bytes; the other operands and both outputs are near `fenced` buffers.  Follows tests/test_gpu_far_knn.py."""
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
from test_gpu_far_knn import CH, DEV, ROWS, _release, _release_all, _rows, st  # noqa: E402, F401
from test_gpu_far_rows import done, far_in, same  # noqa: E402


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("operand", ["bank", "q"])
def test_knn_ranks_far_rows(operand, splits):
    bank, q = _rows(34), _rows(35)
    rn = knn_ref.rnorm(bank)
    s = knn_ref.scores(q, bank, rn)
    tptr = np.arange(0, 4 * ROWS + 1, 4, dtype=np.int32)                            # four targets per query, every row far and near
    tidx = np.concatenate([np.delete(np.arange(ROWS), i) for i in range(ROWS)]).astype(np.int32)
    order = np.stack([np.lexsort((np.arange(ROWS), -(s[i] + np.float32(0)))) for i in range(ROWS)])
    rrank = np.concatenate([np.argsort(order[i])[np.delete(np.arange(ROWS), i)] for i in range(ROWS)]).astype(np.int32)[None, :]
    rsc = np.concatenate([s[i, np.delete(np.arange(ROWS), i)] for i in range(ROWS)])[None, :]

    def ones(a, width):
        return np.pad(a, ((0, 0), (0, width - a.shape[1])), constant_values=1)

    if operand == "bank":
        bf = far_in(bank, 16, 0, 127, oracle=lambda m: knn_ref.scores(ones(q, m.shape[1]), m).T, expected=s.T)
        qf = fenced.input(q, CH + 16, 127)
        assert (ROWS - 1) * bf.ld > 2 ** 32
    else:
        qf = far_in(q, 16, 0, 127, oracle=lambda m: knn_ref.scores(m, ones(bank, m.shape[1])), expected=s)
        bf = fenced.input(bank, CH + 16, 127)
        assert (ROWS - 1) * qf.ld > 2 ** 32
    rnd, tp, ti = (torch.from_numpy(a).to(DEV) for a in (rn, tptr, tidx))
    rank = fenced.output(1, tidx.size, tidx.size, np.int32, expected=rrank)
    score = fenced.output(1, tidx.size, tidx.size, np.float32, expected=rsc)
    need = C.c_int64()
    _lib.call("ivit_knn_ranks_workspace_bytes", ROWS, ROWS, tidx.size, splits, C.byref(need))
    ws = torch.empty(need.value // 8, dtype=torch.int64, device=DEV)
    _lib.call("ivit_knn_ranks_i8", qf.ptr, qf.ld, ROWS, bf.ptr, bf.ld, ROWS, CH, _lib.ptr(rnd), _lib.ptr(tp), _lib.ptr(ti), tidx.size, splits,
              rank.ptr, score.ptr, _lib.ptr(ws), need.value, st())
    torch.cuda.synchronize()
    done(rank, rrank)
    done(score, rsc)
    same(qf)
    same(bf)
