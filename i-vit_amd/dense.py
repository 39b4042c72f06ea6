"""Dense linear probe on the int8 patch tokens (include/ivit_hip.h, "dense linear probe").

    tokens, _, scale = model.forward_tokens(x, integers=True)          # int8 [B, Gh * Gw, C]
    stats.update(rows[keep], patch_labels(target, r, K).reshape(-1)[keep], scale)      # the training side: probe.BankStats as it is
    dp = DenseProbe(stats.ridge(1e-2))
    conf = torch.zeros(K, K, dtype=torch.int64, device=device)
    labels = dp.segment(tokens, (Gh, Gw), r, target=target, conf=conf)  # uint8 [B, Gh * r, Gw * r]; conf accumulated
    miou_, pixel_acc, iou = miou(conf)

The label map is the argmax of the head's logits upsampled bilinearly (torch's align_corners=False) by the patch size r.  The kernel
combines the head's int32 accumulators with the integer bilinear weights in int64 and makes one float64 product per class, so the
upsampled [B, K, H, W] logits never exist and the labels are exact and unique; the confusion matrix is a sum of integers, additive
over calls, batches and ranks.  There is no fallback: anything the kernels do not take raises."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .probe import LinearProbe

CLASSES_MAX = 255         # IVIT_DENSE_CLASSES_MAX
R_MAX = 32                # IVIT_DENSE_R_MAX


def _map_ok(t, who, what):
    if t.dtype != torch.uint8 or t.dim() != 3 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{who}: {what} must be a contiguous uint8 tensor [B, H, W] on the device, got {t.dtype} {tuple(t.shape)} on {t.device}")


def patch_labels(target_u8, r, num_classes, ignore_index=255):
    """uint8 target maps [B, Gh * r, Gw * r] -> uint8 [B, Gh, Gw]: per r x r patch the most frequent valid class (below num_classes
    and not ignore_index), equal counts to the lower class; ignore_index where fewer than half of the patch's pixels are valid"""
    who = "patch_labels"
    _map_ok(target_u8, who, "target")
    r = int(r)
    B, H, W = (int(v) for v in target_u8.shape)
    if r < 1 or H % r or W % r or B < 1 or H < 1 or W < 1:
        raise ValueError(f"{who}: maps of {B} x {H} x {W} are not whole patches of {r} x {r}")
    out = torch.empty(B, H // r, W // r, dtype=torch.uint8, device=target_u8.device)
    _lib.call("ivit_patch_mode_u8", _lib.ptr(target_u8), B, H // r, W // r, r, int(num_classes), int(ignore_index), _lib.ptr(out), _lib.stream_ptr())
    return out


class DenseProbe:
    """a probe.LinearProbe evaluated per pixel: the head GEMM on the patch tokens, then ivit_dense_argmax_u8"""

    def __init__(self, probe: LinearProbe):
        if not 1 <= probe.K <= CLASSES_MAX:
            raise ValueError(f"DenseProbe: {probe.K} classes outside [1, {CLASSES_MAX}] (labels are uint8)")
        self.probe = probe

    def segment(self, tokens_int8, grid, r, target=None, conf=None, labels=True, ignore_index=255):
        """tokens_int8: int8 [B, Gh * Gw, C] (or [B * Gh * Gw, C]), grid = (Gh, Gw), r the patch size -> the uint8 label map
        [B, Gh * r, Gw * r] (None with labels=False).  conf: int64 [K, K] on the device, accumulated: conf[t, p] += 1 for every
        pixel of label p whose target t (uint8 [B, Gh * r, Gw * r]) is below K and not ignore_index.  One ivit_gemm_i8_i32 launch
        and one ivit_dense_argmax_u8 launch."""
        who = "DenseProbe.segment"
        p, K = self.probe, self.probe.K
        gh, gw, r = int(grid[0]), int(grid[1]), int(r)
        if gh < 1 or gw < 1 or not 1 <= r <= R_MAX:
            raise ValueError(f"{who}: grid {gh} x {gw} with r={r} (grid at least 1 x 1, r in [1, {R_MAX}])")
        rows = tokens_int8.reshape(-1, tokens_int8.shape[-1])
        n = int(rows.shape[0])
        if n == 0 or n % (gh * gw):
            raise ValueError(f"{who}: {n} token rows are not images of {gh} x {gw} patches")
        B = n // (gh * gw)
        if not labels and conf is None:
            raise ValueError(f"{who}: neither labels nor conf is asked for")
        if conf is not None:
            if target is None:
                raise ValueError(f"{who}: conf needs a target")
            _map_ok(target, who, "target")
            if tuple(target.shape) != (B, gh * r, gw * r):
                raise ValueError(f"{who}: target {tuple(target.shape)} for label maps {(B, gh * r, gw * r)}")
            if conf.dtype != torch.int64 or tuple(conf.shape) != (K, K) or not conf.is_contiguous() or not conf.is_cuda:
                raise TypeError(f"{who}: conf must be a contiguous int64 tensor [{K}, {K}] on the device")
        acc = p._acc(rows, who)
        out = torch.empty(B, gh * r, gw * r, dtype=torch.uint8, device=acc.device) if labels else None
        _lib.call("ivit_dense_argmax_u8", _lib.ptr(acc), _lib.ptr(p.s_acc), B, gh, gw, p.Np, K, r, _lib.ptr(out),
                  _lib.ptr(target if conf is not None else None), int(ignore_index), _lib.ptr(conf), _lib.stream_ptr())
        return out


def miou(conf):
    """confusion matrix [K, K] (rows: target, columns: prediction) -> (mIoU, pixel accuracy, per-class IoU float64 [K]) on the host in
    float64.  IoU_k = conf[k, k] / (row_k + column_k - conf[k, k]); a class absent from both target and prediction has IoU nan and
    is left out of the mean; (nan, nan, ...) for an empty matrix."""
    c = (conf.cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)).astype(np.float64)
    tp = np.diag(c)
    union = c.sum(axis=0) + c.sum(axis=1) - tp
    iou = np.where(union > 0, tp / np.where(union > 0, union, 1.0), np.nan)
    total = c.sum()
    return (float(np.nanmean(iou)) if (union > 0).any() else float("nan")), (float(tp.sum() / total) if total > 0 else float("nan")), iou
