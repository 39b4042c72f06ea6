"""ivit_kmeans_assign_i8 with the bank as a tests/far.py buffer whose rows start below 2^31, up to 2^32 and beyond 2^32 bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import fenced  # noqa: E402
import kmeans_ref  # noqa: E402
from test_gpu_far_knn import CH, ROWS, _release, _release_all, _rows, st  # noqa: E402, F401
from test_gpu_far_rows import done, far_in, same  # noqa: E402


def test_kmeans_assign_far_rows():
    x, c16 = _rows(51), 128 * _rows(52)[:3].astype(np.int64) + 5
    label, dist = kmeans_ref.assign(x, c16)
    words = lambda d: np.ascontiguousarray(d, np.int64).view(np.int32).reshape(ROWS, 2)      # noqa: E731
    wider = lambda m: np.pad(c16, ((0, 0), (0, m.shape[1] - CH)), constant_values=128)       # noqa: E731 (a row read from the fill moves its dist)
    xf = far_in(x, 16, 0, 127, oracle=lambda m: words(kmeans_ref.assign(m, wider(m))[1]), expected=words(dist))
    assert (ROWS - 1) * xf.ld > 2 ** 32
    hi, lo, cnorm = (torch.from_numpy(p).to("cuda:0") for p in (*kmeans_ref.planes(c16), (c16 ** 2).sum(axis=1)))
    out_l = fenced.output(1, ROWS, ROWS, np.int32, expected=label[None])
    out_d = fenced.output(1, 2 * ROWS, 2 * ROWS, np.int32, expected=words(dist).reshape(1, -1))
    _lib.call("ivit_kmeans_assign_i8", xf.ptr, xf.ld, ROWS, CH, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(cnorm), 3, out_l.ptr, out_d.ptr, st())
    torch.cuda.synchronize()
    done(out_l, label[None]), done(out_d, words(dist).reshape(1, -1))
    same(xf)
