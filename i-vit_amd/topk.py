"""Top-k classes of float32 logits rows and top-k hit counting, on the HIP kernel `ivit_logits_topk_f32`
(include/ivit_hip.h): value descending, equal values by ascending class index -- the order of
torch.sort(logits, descending=True, stable=True).  The fused engines take the same selection straight from their int32
head accumulators (IntViTEngine.forward_topk / IntSwinEngine.forward_topk, `ivit_head_topk`)."""
from __future__ import annotations

import torch

from . import _lib

TOPK_MAX = 8      # IVIT_TOPK_MAX


def _check_logits(logits: torch.Tensor, k: int, n_classes):
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a float32 tensor [B, classes]")
    N = logits.shape[1] if n_classes is None else int(n_classes)
    if not 0 < N <= logits.shape[1]:
        raise ValueError(f"n_classes={N} outside [1, {logits.shape[1]}]")
    if not 1 <= k <= min(N, TOPK_MAX):
        raise ValueError(f"k={k} outside [1, min(classes={N}, {TOPK_MAX})]")
    if not logits.is_cuda:
        raise ValueError("logits must be on a GPU")
    if logits.stride(1) != 1:
        raise ValueError("logits rows must be contiguous")
    return N, (logits.stride(0) if logits.shape[0] > 1 else logits.shape[1])


def topk(logits_f32: torch.Tensor, k: int, n_classes=None) -> torch.Tensor:
    """-> int32 [B, k]: the k largest of logits_f32[:, :n_classes] per row (stable order on ties)."""
    N, ld = _check_logits(logits_f32, k, n_classes)
    B = logits_f32.shape[0]
    out = torch.empty(B, k, dtype=torch.int32, device=logits_f32.device)
    if B:
        _lib.call("ivit_logits_topk_f32", _lib.ptr(logits_f32), B, ld, N, k, _lib.ptr(out), None, None,
                  _lib.stream_ptr())
    return out


def count_hits(logits_f32: torch.Tensor, targets: torch.Tensor, hits: torch.Tensor, k: int = 5) -> None:
    """hits[r] += number of rows whose target is their rank-r class (int64 [k] device tensor, accumulated in place on the
    device: no host synchronisation).  Top-j accuracy counts are hits[:j].sum().  A target outside [0, classes) never hits."""
    B = logits_f32.shape[0] if isinstance(logits_f32, torch.Tensor) else None
    if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int32 or targets.shape != (B,):
        raise TypeError(f"targets must be an int32 tensor [{B}]")
    if not isinstance(hits, torch.Tensor) or hits.dtype != torch.int64 or hits.shape != (k,) or not hits.is_contiguous():
        raise TypeError(f"hits must be a contiguous int64 tensor [{k}]")
    N, ld = _check_logits(logits_f32, k, None)
    if targets.device != logits_f32.device or hits.device != logits_f32.device:
        raise ValueError("logits, targets and hits must be on the same device")
    if not targets.is_contiguous():
        raise ValueError("targets must be contiguous")
    if B == 0:
        return
    out = torch.empty(B, k, dtype=torch.int32, device=logits_f32.device)
    _lib.call("ivit_logits_topk_f32", _lib.ptr(logits_f32), B, ld, N, k, _lib.ptr(out), _lib.ptr(targets),
              _lib.ptr(hits), _lib.stream_ptr())


def check_request(n_classes: int, B: int, device, k: int, targets, hits) -> None:
    """Arguments of a top-k request to an engine's head (forward_topk / forward_topk_graph)."""
    if not 1 <= k <= min(n_classes, TOPK_MAX):
        raise ValueError(f"k={k} outside [1, min(classes={n_classes}, {TOPK_MAX})]")
    if (targets is None) != (hits is None):
        raise ValueError("targets and hits go together")
    if targets is not None:
        if not isinstance(targets, torch.Tensor) or targets.dtype != torch.int32 or targets.shape != (B,) or not targets.is_contiguous():
            raise TypeError(f"targets must be a contiguous int32 tensor [{B}]")
        if not isinstance(hits, torch.Tensor) or hits.dtype != torch.int64 or hits.shape != (k,) or not hits.is_contiguous():
            raise TypeError(f"hits must be a contiguous int64 tensor [{k}]")
        dev = torch.device(device)
        for t in (targets, hits):
            if t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index):
                raise ValueError(f"targets and hits must be on {dev}")


class HeadTopK:
    """Mixin for IntViTEngine / IntSwinEngine: the classifier launch that ends a forward.  `forward` ends with
    `ivit_head_argmax`; `forward_topk` runs the same launches with that one replaced by `ivit_head_topk` over the true class
    count (the padded classes of `prepare.pad_head` never enter the selection).  The engines keep a flat int32 workspace
    ws["topk"] of max_batch * TOPK_MAX entries for the result."""

    def forward_topk(self, images: torch.Tensor, k: int = 5, targets=None, hits=None):
        """-> (logits_int32 [B, classes], logits_f32 [B, classes], topk int32 [B, k]): views of the engine's workspace,
        valid until the next call.  topk: value descending, equal logits by ascending class (column 0 = forward's top-1).
        targets int32 [B] with hits int64 [k] (both or neither, on the engine's device): hits[r] += the rows whose target
        is their rank-r class, accumulated on the device."""
        self._require_head("forward_topk")
        check_request(self.num_classes, images.shape[0], self.dev, k, targets, hits)
        return self._forward(images, None, (k, targets, hits))

    def _classify(self, B: int, st, req):
        ws, hd, nc = self.ws, self.head, self.num_classes
        if req is None:
            _lib.call("ivit_head_argmax", _lib.ptr(ws["logits"]), _lib.ptr(self.head_scale), B, hd["N"],
                      _lib.ptr(ws["logits_f"]), _lib.ptr(ws["top1"]), st)
            return ws["logits"][:B, :nc], ws["logits_f"][:B, :nc], ws["top1"][:B]
        k, targets, hits = req
        out = ws["topk"][: B * k].view(B, k)
        _lib.call("ivit_head_topk", _lib.ptr(ws["logits"]), _lib.ptr(self.head_scale), B, hd["N"], nc, k,
                  _lib.ptr(ws["logits_f"]), _lib.ptr(out), _lib.ptr(targets), _lib.ptr(hits), st)
        return ws["logits"][:B, :nc], ws["logits_f"][:B, :nc], out
