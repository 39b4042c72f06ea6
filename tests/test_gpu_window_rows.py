"""Operator test of ivit_window_rows (csrc/swin.hip): the window partition + cyclic shift of whole rows, and the way back, against
torch.roll + window_partition / window_reverse on the CPU -- exact equality for int8 and int16 rows, both directions, the round
trip, one tensor large enough for a second trip of the kernel's grid-stride loop, and every refusal of the entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.swin_engine import window_row_map  # noqa: E402
from ivit_amd.swin_quant import window_partition, window_reverse  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0x5A

# (B, H, W, ws, shift, row_bytes); the last: Swin-T stage 0 at batch 64, 19 MB = 1 204 224 chunks of 16 bytes, more than the
# 2048 workgroups x 256 lanes the launcher caps its grid at (WINDOW_ROWS_MAX_GRID) -> a second trip of the loop
CASES = [(3, 14, 14, 7, 3, 96), (2, 14, 14, 7, 0, 192), (1, 24, 24, 12, 6, 64), (2, 7, 7, 7, 0, 1536), (1, 14, 14, 7, 6, 16),
         (64, 56, 56, 7, 3, 96)]


def st():
    return _lib.stream_ptr()


def forward_cpu(x, B, H, W, ws, shift):
    """[B * H * W, C] in image order -> window order, as SwinTransformerBlock.forward does it"""
    t = x.reshape(B, H, W, -1)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    return window_partition(t, ws).reshape(B * H * W, -1)


def inverse_cpu(x, B, H, W, ws, shift):
    t = window_reverse(x.reshape(-1, ws, ws, x.shape[-1]), ws, H, W)
    if shift:
        t = torch.roll(t, shifts=(shift, shift), dims=(1, 2))
    return t.reshape(B * H * W, -1)


def run(src, B, H, W, row_bytes, ws, shift, inverse):
    dst = torch.full_like(src, SENTINEL)
    _lib.call("ivit_window_rows", _lib.ptr(src), _lib.ptr(dst), B, H, W, row_bytes, ws, shift, inverse, st())
    return dst


@pytest.mark.parametrize("dtype", [torch.int8, torch.int16])
@pytest.mark.parametrize("B,H,W,ws,shift,row_bytes", CASES)
def test_window_rows_matches_roll_and_partition(B, H, W, ws, shift, row_bytes, dtype):
    cols = row_bytes // torch.empty(0, dtype=dtype).element_size()
    rows = B * H * W
    g = torch.Generator().manual_seed(rows * 31 + row_bytes + shift)
    info = torch.iinfo(dtype)
    x = torch.randint(info.min, info.max + 1, (rows, cols), generator=g, dtype=torch.int32).to(dtype)
    xd = x.to(DEV)
    fwd = run(xd, B, H, W, row_bytes, ws, shift, 0)
    assert torch.equal(fwd.cpu(), forward_cpu(x, B, H, W, ws, shift))
    inv = run(xd, B, H, W, row_bytes, ws, shift, 1)
    assert torch.equal(inv.cpu(), inverse_cpu(x, B, H, W, ws, shift))
    assert torch.equal(run(fwd, B, H, W, row_bytes, ws, shift, 1), xd)
    if H == ws and W == ws:
        assert shift == 0 and torch.equal(fwd, xd)          # one window: the identity
    # the engine's statement of the same map: row r of the image goes to row map[r] of the window order
    m = torch.from_numpy(window_row_map(B, H, W, ws, shift))
    assert torch.equal(fwd.cpu()[m], x)


def test_window_rows_refusals():
    B, H, W, ws, shift, rb = 2, 14, 14, 7, 3, 96
    n = B * H * W * rb
    buf = torch.zeros(2 * n + 64, dtype=torch.int8, device=DEV)      # torch allocations are aligned to at least 256 bytes
    src, dst = buf[:n], buf[n:2 * n + 64]
    dst.fill_(SENTINEL)
    L = _lib.lib()

    def refused(s, d, *args):
        rc = L.ivit_window_rows(s, d, *args, st())
        msg = L.ivit_last_error_string().decode()
        assert rc != 0 and "ivit_window_rows" in msg, (rc, msg)
        return msg

    p, q = src.data_ptr(), dst.data_ptr()
    assert p % 16 == 0 and q % 16 == 0
    vp = C.c_void_p
    assert "NULL" in refused(None, vp(q), B, H, W, rb, ws, shift, 0)
    assert "NULL" in refused(vp(p), None, B, H, W, rb, ws, shift, 0)
    assert "misaligned" in refused(vp(p + 8), vp(q), B, H, W, rb, ws, shift, 0)
    assert "misaligned" in refused(vp(p), vp(q + 4), B, H, W, rb, ws, shift, 0)
    assert "row_bytes" in refused(vp(p), vp(q), B, H, W, rb + 8, ws, shift, 0)
    assert "row_bytes" in refused(vp(p), vp(q), B, H, W, 0, ws, shift, 0)
    assert "divide" in refused(vp(p), vp(q), B, H + 1, W, rb, ws, shift, 0)
    assert "divide" in refused(vp(p), vp(q), B, H, W - 2, rb, ws, shift, 0)
    assert "divide" in refused(vp(p), vp(q), B, H, W, rb, 0, 0, 0)
    assert "shift" in refused(vp(p), vp(q), B, H, W, rb, ws, ws, 0)
    assert "shift" in refused(vp(p), vp(q), B, H, W, rb, ws, -1, 1)
    assert "overlap" in refused(vp(p), vp(p), B, H, W, rb, ws, shift, 0)
    assert "overlap" in refused(vp(p), vp(p + 16 * rb), B, H, W, rb, ws, shift, 1)
    assert "inverse" in refused(vp(p), vp(q), B, H, W, rb, ws, shift, 2)
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all()) and bool((src == 0).all())
    with pytest.raises(_lib.IvitError, match="shift outside"):
        _lib.call("ivit_window_rows", vp(p), vp(q), B, H, W, rb, ws, ws, 0, st())
