"""ivit_token_degrees_i8 and ivit_discover_boxes_i8 with the tokens as a tests/far.py buffer whose rows start below 2^31, between 2^31
and 2^32 and beyond 2^32 bytes (a 1 x 5 grid, one image); the outputs are near `fenced` buffers.  Follows tests/test_gpu_far_knn.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import discover_ref  # noqa: E402
import fenced  # noqa: E402
from test_gpu_far_knn import CH, ROWS, _release, _release_all, _rows, st  # noqa: E402, F401
from test_gpu_far_rows import done, far_in, same  # noqa: E402


def test_discover_far_rows():
    t = _rows(41)
    d = discover_ref.affinity(t)
    box, seed, deg, _ = discover_ref.discover(d, 1, ROWS, 3)
    # a row read from the fill changes every product
    tf = far_in(t, 16, 0, 127, oracle=lambda m: discover_ref.affinity(m).astype(np.int32), expected=d.astype(np.int32))
    assert (ROWS - 1) * tf.ld > 2 ** 32
    want = {"deg": deg[None], "box": np.array([box]), "seed": np.array([[seed]])}
    out = {n: fenced.output(1, e.shape[1], e.shape[1], np.int32, expected=e) for n, e in want.items()}
    _lib.call("ivit_token_degrees_i8", tf.ptr, tf.ld, 0, 1, 1, ROWS, CH, out["deg"].ptr, st())
    _lib.call("ivit_discover_boxes_i8", tf.ptr, tf.ld, 0, 1, 1, ROWS, CH, out["deg"].ptr, 3, out["box"].ptr, out["seed"].ptr, None, st())
    torch.cuda.synchronize()
    for n, e in want.items():
        done(out[n], e)
    same(tf)
