"""Unsupervised single-object discovery on the int8 patch tokens (include/ivit_hip.h, "object discovery on int8 patch tokens";
DESIGN.md section 4): the seed expansion of LOST (Simeoni et al., 2021), scored by CorLoc.

    tok = model.forward_tokens(x, integers=True)                         # int8 patch tokens [B, Gh * Gw, C]
    boxes, seed, deg = discover_objects(tok, (Gh, Gw), k=100)            # int32 [B, 4] grid cells, [B], [B, Gh * Gw]
    hits, iou = corloc(boxes_to_pixels(boxes, r), gt_boxes_per_image)    # on the host, float64

Per image: the degree of a token is the number of other tokens it has a positive dot product with; the token of smallest degree
is the seed, the k tokens of smallest degree the potentials, the potentials that correlate positively with the seed are summed, and
the box is drawn around the connected region of tokens that correlate positively with that sum and contains the seed.  On int8
tokens every step is an exact integer statement, so the result is one answer whatever the tiling; the [hw, hw] affinity matrix
never exists (csrc/discover.hip: the degrees on the int8 MFMA, the tail in one workgroup per image).  Equal degrees go by the
lower token index.  There is no fallback: anything the kernels do not take raises IvitError with the offending value named."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import IvitError

GRID_MAX = 64        # IVIT_DISCOVER_GRID_MAX
K_MAX = 128          # IVIT_DISCOVER_K_MAX
C_MAX = 1024


def _operands(who, tokens, grid):
    """-> (tokens, B, Gh, Gw, C) after the checks the entries would make, before anything is allocated"""
    if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int8:
        raise IvitError(f"{who}: int8 integers wanted, got {getattr(tokens, 'dtype', type(tokens).__name__)} -- take the tokens from "
                        "forward_tokens(..., integers=True)")
    Gh, Gw = (int(v) for v in grid)
    if not (1 <= Gh <= GRID_MAX and 1 <= Gw <= GRID_MAX):
        raise IvitError(f"{who}: a grid of Gh={Gh} x Gw={Gw} tokens outside [1, {GRID_MAX}] x [1, {GRID_MAX}]")
    if tokens.dim() != 3 or int(tokens.shape[0]) < 1 or int(tokens.shape[1]) != Gh * Gw:
        raise IvitError(f"{who}: tokens of shape [B, {Gh} * {Gw}, C] wanted, got {tuple(tokens.shape)}")
    C = int(tokens.shape[2])
    if C % 64 != 0 or not 64 <= C <= C_MAX:
        raise IvitError(f"{who}: C={C} is not a multiple of 64 between 64 and {C_MAX}")
    if not tokens.is_cuda:
        raise IvitError(f"{who}: tokens on the device wanted, got {tokens.device}")
    if tokens.stride(2) != 1 or tokens.stride(1) % 16 or tokens.stride(0) % 16 or tokens.stride(0) < 0 or tokens.data_ptr() % 16:
        raise IvitError(f"{who}: misaligned rows: strides {tuple(tokens.stride())} and address {tokens.data_ptr():#x} (unit channel stride, "
                        "row stride, image stride and address multiples of 16 bytes)")
    return tokens, int(tokens.shape[0]), Gh, Gw, C


def _degrees(t, B, Gh, Gw, C):
    deg = torch.empty(B, Gh * Gw, dtype=torch.int32, device=t.device)
    _lib.call("ivit_token_degrees_i8", _lib.ptr(t), t.stride(1), t.stride(0), B, Gh, Gw, C, _lib.ptr(deg), _lib.stream_ptr())
    return deg


def token_degrees(tokens_int8, grid):
    """-> int32 [B, Gh * Gw]: deg[b, i] = the number of tokens j != i of image b with dot(t_i, t_j) > 0 (ivit_token_degrees_i8)"""
    return _degrees(*_operands("token_degrees", tokens_int8, grid))


def discover_objects(tokens_int8, grid, k=100, return_mask=False):
    """-> (boxes int32 [B, 4], seed int32 [B], deg int32 [B, Gh * Gw][, rows int64 [B, Gh]]): per image the box (x0, y0, x1, y1) in grid
    cells, inclusive, of the seed's component, the seed token and the degrees; with return_mask the component itself, bit x of
    rows[b, y] for the cell (y, x) (the uint64 row words, carried in int64).  Two launches, nothing read back."""
    who = "discover_objects"
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise IvitError(f"{who}: k={k} outside [1, {K_MAX}]")
    t, B, Gh, Gw, C = _operands(who, tokens_int8, grid)
    deg = _degrees(t, B, Gh, Gw, C)
    boxes = torch.empty(B, 4, dtype=torch.int32, device=t.device)
    seed = torch.empty(B, dtype=torch.int32, device=t.device)
    rows = torch.empty(B, Gh, dtype=torch.int64, device=t.device) if return_mask else None
    _lib.call("ivit_discover_boxes_i8", _lib.ptr(t), t.stride(1), t.stride(0), B, Gh, Gw, C, _lib.ptr(deg), k, _lib.ptr(boxes), _lib.ptr(seed),
              _lib.ptr(rows), _lib.stream_ptr())
    return (boxes, seed, deg, rows) if return_mask else (boxes, seed, deg)


def boxes_to_pixels(boxes, r):
    """grid-cell boxes (x0, y0, x1, y1), inclusive -> pixel boxes (x0 * r, y0 * r, (x1 + 1) * r, (y1 + 1) * r), int64 on the host"""
    r = int(r)
    if r < 1:
        raise ValueError(f"boxes_to_pixels: r={r} pixels per token below 1")
    b = torch.as_tensor(boxes).detach().cpu().to(torch.int64).reshape(-1, 4)
    return (b + torch.tensor([0, 0, 1, 1])) * r


def corloc(boxes_px, gt_boxes_per_image):
    """-> (hits bool [B], iou float64 [B]) on the host: per image the largest intersection over union of its box (x0, y0, x1, y1 in
    pixels, the far edges exclusive) with any of its ground-truth boxes, in float64, and hit = iou >= 0.5.  An image without a
    ground-truth box scores 0.  CorLoc is hits.double().mean()."""
    p = torch.as_tensor(boxes_px).detach().cpu().to(torch.float64).reshape(-1, 4)
    if len(gt_boxes_per_image) != int(p.shape[0]):
        raise ValueError(f"corloc: {int(p.shape[0])} boxes for {len(gt_boxes_per_image)} images")
    iou = torch.zeros(int(p.shape[0]), dtype=torch.float64)
    for i, gts in enumerate(gt_boxes_per_image):
        g = torch.as_tensor(gts, dtype=torch.float64).reshape(-1, 4)
        if g.numel() == 0:
            continue
        w = (torch.minimum(p[i, 2], g[:, 2]) - torch.maximum(p[i, 0], g[:, 0])).clamp(min=0)
        h = (torch.minimum(p[i, 3], g[:, 3]) - torch.maximum(p[i, 1], g[:, 1])).clamp(min=0)
        inter = w * h
        union = (p[i, 2] - p[i, 0]) * (p[i, 3] - p[i, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter
        iou[i] = (inter / union.clamp(min=1e-300)).max()
    return iou >= 0.5, iou
