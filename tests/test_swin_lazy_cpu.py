"""The host side of the Swin int8 / int16-carrying module path (quantization_utils/lazy.py), without a GPU: the shape operations
SwinTransformerBlock applies between its QuantActs are recorded on a payload and compose to the engine's window row map, anything
else is classified as what it is, an int16-carrying QT answers like the float tensor it stands for, the float layout travels with
the carrier, and the new export's prototype matches its ctypes signature."""
import os
import re

import numpy as np
import pytest
import torch

from ivit_amd import _lib
from ivit_amd.quantization_utils import lazy
from ivit_amd.swin_engine import window_row_map
from ivit_amd.swin_quant import window_partition, window_reverse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QT, QS = lazy.QT, lazy.QS

# (B, H, W, ws, shift, row_bytes): the cases of tests/test_gpu_window_rows.py
CASES = [(3, 14, 14, 7, 3, 96), (2, 14, 14, 7, 0, 192), (1, 24, 24, 12, 6, 64), (2, 7, 7, 7, 0, 1536), (1, 14, 14, 7, 6, 16)]


def block_forward_ops(x, B, H, W, C, ws, sh):
    """SwinTransformerBlock.forward between qact1 and attn.qkv (swin_quant.py:258-271)"""
    x = x.reshape(B, H, W, C)
    if sh > 0:
        x = torch.roll(x, shifts=(-sh, -sh), dims=(1, 2))
    return window_partition(x, ws).reshape(-1, ws * ws, C)


def block_inverse_ops(x, B, H, W, C, ws, sh):
    """... and between attn.qact4 and the residual qact2 (:278-289)"""
    x = window_reverse(x.reshape(-1, ws, ws, C), ws, H, W)
    if sh > 0:
        x = torch.roll(x, shifts=(sh, sh), dims=(1, 2))
    return x.reshape(B, H * W, C)


def carrier(shape, dtype):
    n = int(np.prod(shape))
    q = (torch.arange(n, dtype=torch.int32) % 251 - 125).to(dtype).reshape(shape)
    kw = {"q8": q} if dtype == torch.int8 else {"q16": q}
    return QT.wrap(shape, "cpu", scale=QS.make(0.02, "cpu"), **kw), q


@pytest.mark.parametrize("B,H,W,ws,shift,row_bytes", CASES)
def test_recorded_shape_ops_compose_to_the_window_row_map(B, H, W, ws, shift, row_bytes):
    C = row_bytes
    x, q = carrier((B, H * W, C), torch.int8)
    y = block_forward_ops(x, B, H, W, C, ws, shift)
    assert isinstance(y, QT) and y.shape == (B * (H // ws) * (W // ws), ws * ws, C) and len(y.rops) >= 3
    assert y._q8 is q                                              # recorded, not executed
    plan = lazy.row_plan(tuple(q.shape), y.rops)
    m = window_row_map(B, H, W, ws, shift)
    if ws == H and ws == W:
        assert plan == ("identity",)
    else:
        assert plan == ("window", B, H, W, ws, shift, 0)
        fwd = np.empty_like(m)
        fwd[m] = np.arange(m.size)                                 # destination row map[r] takes source row r
        want = q.reshape(-1, C)[torch.from_numpy(fwd)].reshape(y.shape)
        assert torch.equal(want, block_forward_ops(q, B, H, W, C, ws, shift))
    x16, q16 = carrier((B * (H // ws) * (W // ws), ws * ws, C // 2), torch.int16)
    z = block_inverse_ops(x16, B, H, W, C // 2, ws, shift)
    assert z.shape == (B, H * W, C // 2) and z._q8 is None and z._q16 is q16
    plan = lazy.row_plan(tuple(q16.shape), z.rops)
    if ws == H and ws == W:
        assert plan == ("identity",)
    else:
        assert plan == ("window", B, H, W, ws, shift, 1)
        want = q16.reshape(-1, C // 2)[torch.from_numpy(m)].reshape(z.shape)    # destination row r takes source row map[r]
        assert torch.equal(want, block_inverse_ops(q16, B, H, W, C // 2, ws, shift))
    # executed on the CPU (no kernel here: lazy.ROW_KERNEL off): the payload the torch operations give
    old = lazy.ROW_KERNEL
    try:
        lazy.ROW_KERNEL = False
        assert torch.equal(y.q8, block_forward_ops(q, B, H, W, C, ws, shift)) and not y.rops
        assert torch.equal(z.q16, block_inverse_ops(q16, B, H, W, C // 2, ws, shift)) and z.q is z.q16 and z.q8 is None
    finally:
        lazy.ROW_KERNEL = old
    # ... and through the composed map (on the CPU an index_select with it; on the GPU one ivit_window_rows launch)
    y2 = block_forward_ops(carrier((B, H * W, C), torch.int8)[0], B, H, W, C, ws, shift)
    assert torch.equal(y2.q8, y.q8)


def test_other_row_permutations_and_non_permutations_are_classified():
    x, q = carrier((2, 6, 4, 16), torch.int8)
    t = x.transpose(1, 2)                                          # rows move, no window map does that
    plan = lazy.row_plan(tuple(q.shape), t.rops)
    assert plan[0] == "index"
    assert torch.equal(q.reshape(-1, 16)[torch.from_numpy(plan[1])].reshape(t.shape), q.transpose(1, 2))
    flipped = x.roll(shifts=(1,), dims=(1,))                       # a cyclic shift alone: a permutation, not the window map
    assert lazy.row_plan(tuple(q.shape), flipped.rops)[0] == "index"
    assert lazy.row_plan(tuple(q.shape), x.reshape(2, 24, 16).contiguous().rops) == ("identity",)
    # the last dimension is touched: not a row permutation -- the operations run on the payload as they are
    assert lazy.row_plan(tuple(q.shape), x.permute(0, 3, 1, 2).rops) == ("torch",)
    assert lazy.row_plan(tuple(q.shape), x.reshape(2, 6, 8, 8).rops) == ("torch",)
    assert lazy.row_plan(tuple(q.shape), x.roll(shifts=(3,), dims=(-1,)).rops) == ("torch",)
    old = lazy.ROW_KERNEL
    try:
        lazy.ROW_KERNEL = False
        assert torch.equal(x.permute(0, 3, 1, 2).q8, q.permute(0, 3, 1, 2))
        assert torch.equal(x.roll(shifts=(3,), dims=(-1,)).q8, q.roll(shifts=(3,), dims=(-1,)))
    finally:
        lazy.ROW_KERNEL = old
    # slicing is not recorded: it acts on the payload (PatchMerging's strided slices stay views of it)
    s = x[:, 0::2, 1::2]
    assert not s.rops and s.q8.data_ptr() == q[:, 0::2, 1::2].data_ptr() and torch.equal(s.q8, q[:, 0::2, 1::2])


def test_int16_carrier_answers_like_the_float_tensor():
    x, q = carrier((2, 5, 24), torch.int16)
    assert x.shape == (2, 5, 24) and x.dim() == 3 and x.dtype == torch.float32 and x.numel() == 240 and x.stride() == (120, 24, 1)
    assert x.q8 is None and x.q16 is q and x.q is q
    f = x.to_float()
    assert f.dtype == torch.float32 and torch.equal(f, q.float() * np.float32(0.02))
    a, b = x.reshape(2, 5, 2, 12).permute(2, 0, 1, 3).unbind(0)
    assert isinstance(b, QT) and b.q8 is None and torch.equal(b.q16, q.reshape(2, 5, 2, 12).permute(2, 0, 1, 3)[1])
    assert torch.nn.functional.dropout(x, 0.1, False) is x
    assert type(x + 1) is torch.Tensor and torch.equal(x + 1, f + 1)
    with lazy.scope(True):
        cat = torch.cat([x[:, 0::2][:, :2], x[:, 1::2]], -1)       # both parts carry int16: pending
    assert isinstance(cat, QT) and cat.shape == (2, 2, 48) and lazy.int_width(cat) == 16
    x8, q8 = carrier((2, 5, 24), torch.int8)
    assert x8.q16 is None and x8.q is q8 and lazy.int_width(x8) == 8 and lazy.int_width(f) is None


def test_float_layout_travels_with_the_carrier():
    """PatchEmbed.forward's flatten(2).transpose(1, 2) of the NCHW convolution output (layers_quant.py:198): the LayerNorm behind it
    reduces in the outer order, and every QuantAct / LayerNorm result keeps that layout until something makes it contiguous"""
    B, C, g = 2, 8, 3
    x, q = carrier((B, C, g, g), torch.int8)
    t = x.flatten(2).transpose(1, 2)
    assert t.shape == (B, g * g, C) and tuple(t.fl.stride()) == (C * g * g, 1, g * g)
    assert lazy.ln_outer(t.fl) == g * g and lazy.ln_outer(x.fl) == 0
    out = lazy.act_layout(t.fl)                                    # a QuantAct's result keeps it ...
    assert tuple(out.stride()) == tuple(t.fl.stride())
    ident = torch.empty(B, g * g, C, device="meta")
    assert lazy.act_layout(ident, t.fl).stride() == t.fl.stride()  # ... the identity's layout wins in the two-operand form ...
    assert lazy.act_layout(t.fl, ident).is_contiguous()
    win = t.reshape(B, g, g, C)
    assert lazy.ln_outer(win.fl) is None                           # ... a layout that is neither is not guessed at
    assert lazy.ln_outer(win.roll(shifts=(1, 1), dims=(1, 2)).fl) == 0      # torch.roll returns a contiguous tensor
    assert lazy.ln_outer(win.reshape(B, 1, g, 1, g, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, g * g, C).fl) in (0, g * g)
    f = t.to_float()                                               # materialised with the strides the reference's tensor has
    assert tuple(f.stride()) == (C * g * g, 1, g * g) and torch.equal(f, q.flatten(2).transpose(1, 2).float() * np.float32(0.02))
    assert lazy.ln_outer(torch.empty(4, 6, device="meta").t()) is None


def test_window_rows_prototype_matches_its_signature():
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    proto = re.search(r"\bint\s+ivit_window_rows\s*\(([^)]*)\)", hdr).group(1)
    kinds = {"const void*": _lib.vp, "void*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64, "ivit_stream_t": _lib.vp}
    types = [" ".join(a.split()[:-1]) for a in proto.replace("\n", " ").split(",")]
    names = [a.split()[-1] for a in proto.replace("\n", " ").split(",")]
    assert names == ["src", "dst", "batch", "H", "W", "row_bytes", "ws", "shift", "inverse", "stream"]
    assert _lib.SIGNATURES["ivit_window_rows"] == [kinds[t] for t in types]
