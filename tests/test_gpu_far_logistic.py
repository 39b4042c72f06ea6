"""One step of the logistic probe with the bank as a tests/far.py buffer: five rows of 64 channels, one below 2^31, one between 2^31
and 2^32 and the others beyond 2^32 bytes, gathered by idx in a mixed order with a repeat.  The same step on a dense copy of the
rows must give the same bits in every output (the arithmetic is a function of the gathered values alone); a row offset that lost
its upper bits gathers the fill (127 in every channel) instead and shows as a difference, never as a fault (far.py).  Sizes, the
skip and the release of the buffers follow tests/test_gpu_far_probe.py; the arithmetic itself is tests/test_gpu_logistic.py's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402

import far  # noqa: E402
from test_gpu_far_rows import far_in, same  # noqa: E402
from test_gpu_logistic import DEV, S_X, problem  # noqa: E402

ROWS, CH, K, B = 5, 64, 3, 6


@pytest.fixture(autouse=True, scope="module")
def _release_all():
    yield
    far.release(all=True)


def test_step_far_rows():
    x, _, y, W, b, mW, mb = problem(CH, K, B, n=ROWS)
    x = np.clip(x, -100, 100).astype(np.int8)                               # (no row could pass for the fill, 127)
    idx = np.array([4, 0, 3, 1, 2, 4], np.int32)
    xf = far_in(x, 16, 0, 127)
    assert (ROWS - 1) * xf.ld > 2 ** 32

    def run(xptr, ldx):
        t = {k: torch.from_numpy(v).to(DEV) for k, v in dict(idx=idx, y=y, W=W, b=b, mW=mW, mb=mb).items()}
        t["Wh"] = t["W"].to(torch.bfloat16)
        t.update(G=torch.empty(64 * 64, dtype=torch.bfloat16, device=DEV), z=torch.empty(B, 64, device=DEV), loss=torch.empty(B, device=DEV),
                 top1=torch.empty(B, dtype=torch.int32, device=DEV))
        p = {k: _lib.ptr(v) for k, v in t.items()}
        _lib.call("ivit_probe_ce_forward_i8", xptr, ldx, CH, p["idx"], p["y"], B, K, S_X, p["Wh"], p["b"], p["G"], p["loss"], p["top1"], p["z"],
                  _lib.stream_ptr())
        _lib.call("ivit_probe_sgd_update_i8", xptr, ldx, CH, p["idx"], B, K, S_X, p["G"], 0.05, 0.9, 1e-3, p["W"], p["b"], p["mW"], p["mb"],
                  p["Wh"], _lib.stream_ptr())
        torch.cuda.synchronize()
        return {k: v.view(torch.int16).cpu() if v.dtype == torch.bfloat16 else v.cpu() for k, v in t.items()}

    near = torch.from_numpy(x).to(DEV)
    want, got = run(_lib.ptr(near), CH), run(xf.ptr, xf.ld)
    poisoned = run(_lib.ptr(torch.full_like(near, 127)), CH)
    for k in ("z", "G", "loss", "W", "mW", "Wh"):
        assert torch.equal(got[k], want[k]), k
        assert not torch.equal(poisoned[k], want[k]), f"{k}: the fill would pass for the rows"
    assert torch.equal(got["top1"], want["top1"]) and torch.equal(got["b"], want["b"]) and torch.equal(got["mb"], want["mb"])
    same(xf)
    far.release()
