"""Label propagation on the int8 patch tokens (include/ivit_hip.h, "label propagation on int8 patch tokens"):
semi-supervised video object segmentation as the DINO evaluation runs it on DAVIS.

    tok = model.forward_tokens(frames, integers=True)[0]                 # int8 patch tokens, one [Gh * Gw, C] block per frame
    mem = TokenMemory(Gh, Gw, C, K, frames=1 + n_last, device=device)
    mem.put(0, tok_first, onehot_first)                                  # slot 0: the first frame and its given labels
    seg = mem.propagate(tok_t, radius=12, k=5, T=0.1, frames=used)       # float32 [Gh * Gw, K]: the frame's soft labels
    mem.put(1 + (t - 1) % n_last, tok_t, seg)                            # the ring of the previous frames

Every token of the target frame looks at the context tokens within `radius` grid positions of its own, in every context frame,
keeps the k of largest cosine and mixes their soft labels with the weights exp(cos / T).  The tokens stay int8; the similarity
runs on the int8 MFMA and the selection in the kernel's epilogue, so neither the [hw, F * hw] affinity matrix nor its mask exists.
The neighbours are exactly k in the unique order of knn.FeatureBank.search (the float protocol keeps every tie with the k-th
value).  There is no fallback: anything the kernels do not take raises.

Scoring (include/ivit_hip.h, "video segmentation scoring"; csrc/davis.hip):

    upsample_argmax(seg, (Gh, Gw), r, out=pred[t])                       # the frame's label map, uint8 [Gh * r, Gw * r]
    counts = mask_scores(pred[1:], truth[1:], num_objects)               # int64 [n, O, 6]: one launch for the sequence
    J, F = davis_measures(counts)                                        # float64 [n, O] each, on the host"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from .knn import SPLITS_MAX, knn_weights

K_MAX = 32           # IVIT_LOCAL_K_MAX
CLASSES_MAX = 256    # IVIT_PROPAGATE_CLASSES_MAX
C_MAX = 1024         # the widest rows of ivit_local_topk_i8
R_MAX = 32           # IVIT_UPSAMPLE_R_MAX
OBJECTS_MAX = 255    # IVIT_SCORES_OBJECTS_MAX
RADIUS_MAX = 24      # IVIT_SCORES_RADIUS_MAX


class TokenMemory:
    """`frames` slots of context: int8 tokens [frames, Gh * Gw, C], their rnorm [frames * Gh * Gw] and their soft labels float32
    [frames * Gh * Gw, K].  Searches look at the first `frames` slots given to them: fill the slots from 0."""

    def __init__(self, Gh, Gw, C, K, frames, device):
        Gh, Gw, C, K, frames = int(Gh), int(Gw), int(C), int(K), int(frames)
        if Gh < 1 or Gw < 1 or frames < 1 or frames * Gh * Gw >= 2 ** 31:
            raise ValueError(f"TokenMemory: {frames} frames of a {Gh} x {Gw} grid (at least 1 each, below 2^31 tokens in all)")
        if C % 64 != 0 or not 64 <= C <= C_MAX:
            raise ValueError(f"TokenMemory: C={C} is not a multiple of 64 between 64 and {C_MAX}")
        if not 1 <= K <= CLASSES_MAX:
            raise ValueError(f"TokenMemory: {K} classes outside [1, {CLASSES_MAX}]")
        if torch.device(device).type != "cuda":
            raise ValueError(f"TokenMemory: a device wanted, got {device}")
        self.Gh, self.Gw, self.C, self.K, self.frames, self.hw = Gh, Gw, C, K, frames, Gh * Gw
        self.tokens = torch.zeros(frames, self.hw, C, dtype=torch.int8, device=device)
        self.rnorm = torch.zeros(frames * self.hw, dtype=torch.float32, device=device)
        self.seg = torch.zeros(frames * self.hw, K, dtype=torch.float32, device=device)
        self.workspace = None

    def _tokens_ok(self, t, who):
        if t.dtype != torch.int8:
            raise TypeError(f"{who}: int8 integers wanted, got {t.dtype} -- take the tokens from forward_tokens(..., integers=True)")
        if t.dim() != 2 or not t.is_cuda or tuple(t.shape) != (self.hw, self.C):
            raise ValueError(f"{who}: a [{self.hw}, {self.C}] tensor on the device wanted ({self.Gh} x {self.Gw} tokens), got shape "
                             f"{tuple(t.shape)} on {t.device}")

    def put(self, slot, tokens_int8, seg):
        """one frame into `slot`: its int8 tokens [Gh * Gw, C] (any strides: they are copied) and soft labels [Gh * Gw, K]"""
        who = "TokenMemory.put"
        if not 0 <= int(slot) < self.frames:
            raise ValueError(f"{who}: slot {slot} outside [0, {self.frames})")
        self._tokens_ok(tokens_int8, who)
        if tuple(seg.shape) != (self.hw, self.K):
            raise ValueError(f"{who}: labels of shape {tuple(seg.shape)} for {self.hw} tokens and {self.K} classes")
        s, rows = int(slot), self.tokens[int(slot)]
        rows.copy_(tokens_int8)
        self.seg[s * self.hw:(s + 1) * self.hw].copy_(seg.to(torch.float32))
        _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(rows), self.C, self.hw, self.C, _lib.ptr(self.rnorm[s * self.hw:]), _lib.stream_ptr())

    def _frames(self, frames, who):
        F = self.frames if frames is None else int(frames)
        if not 1 <= F <= self.frames:
            raise ValueError(f"{who}: frames={frames} outside [1, {self.frames}]")
        return F

    def neighbours(self, q_int8, radius, k, frames=None, splits=0):
        """-> (idx int32 [Gh * Gw, k], cos float32 [Gh * Gw, k]): per target token the k context tokens (rows of the first `frames`
        slots, frame-major) of largest cosine within `radius` grid positions, descending, equal scores by ascending row.  splits:
        frame segments (0: chosen by the launcher); the result does not depend on it."""
        who = "TokenMemory.neighbours"
        self._tokens_ok(q_int8, who)
        F, radius, k, splits = self._frames(frames, who), int(radius), int(k), int(splits)
        if radius < 0:
            raise ValueError(f"{who}: radius={radius} below 0")
        corner = F * (min(radius, self.Gh - 1) + 1) * (min(radius, self.Gw - 1) + 1)
        if not 1 <= k <= corner:
            raise ValueError(f"{who}: k={k} outside [1, {corner}], the window of a corner token")
        if k > K_MAX:
            raise ValueError(f"{who}: k={k} above {K_MAX}")
        if not 0 <= splits <= min(F, SPLITS_MAX):
            raise ValueError(f"{who}: splits={splits} outside [0, {min(F, SPLITS_MAX)}]")
        q = q_int8 if q_int8.stride(1) == 1 and q_int8.stride(0) % 16 == 0 and q_int8.data_ptr() % 16 == 0 else q_int8.contiguous()
        dev = self.tokens.device
        idx = torch.empty(self.hw, k, dtype=torch.int32, device=dev)
        score = torch.empty(self.hw, k, dtype=torch.float32, device=dev)
        qnorm = torch.empty(self.hw, dtype=torch.float32, device=dev)
        need = C.c_int64(0)
        _lib.call("ivit_local_topk_workspace_bytes", self.Gh, self.Gw, F, k, splits, C.byref(need))
        if need.value and (self.workspace is None or self.workspace.numel() * 8 < need.value):
            self.workspace = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
        st = _lib.stream_ptr()
        _lib.call("ivit_local_topk_i8", _lib.ptr(q), q.stride(0), self.Gh, self.Gw, _lib.ptr(self.tokens), self.C, F, self.C, _lib.ptr(self.rnorm),
                  radius, k, splits, _lib.ptr(idx), _lib.ptr(score), _lib.ptr(self.workspace) if need.value else None, need.value, st)
        _lib.call("ivit_rows_rnorm_i8_f32", _lib.ptr(q), q.stride(0), self.hw, self.C, _lib.ptr(qnorm), st)
        return idx, score * qnorm[:, None]          # one more float32 product: the cosine

    def mix(self, idx, w, frames=None):
        """-> float32 [Gh * Gw, K]: out[t] = sum_j w[t, j] * seg[idx[t, j]] / sum_j w[t, j], both sums in rank order"""
        who = "TokenMemory.mix"
        if idx.shape != w.shape or idx.dim() != 2 or not 1 <= int(idx.shape[1]) <= K_MAX:
            raise ValueError(f"{who}: idx {tuple(idx.shape)} and w {tuple(w.shape)} (k at most {K_MAX})")
        F = self._frames(frames, who)
        idx, w = idx.to(torch.int32).contiguous(), w.to(torch.float32).contiguous()
        T, k = int(idx.shape[0]), int(idx.shape[1])
        out = torch.empty(T, self.K, dtype=torch.float32, device=self.seg.device)
        _lib.call("ivit_propagate_labels_f32", _lib.ptr(idx), _lib.ptr(w), T, k, _lib.ptr(self.seg), F * self.hw, self.K, _lib.ptr(out), _lib.stream_ptr())
        return out

    def propagate(self, q_int8, radius=12, k=5, T=0.1, frames=None):
        """-> float32 [Gh * Gw, K]: the soft labels of the target frame's tokens, mixed from their k neighbours in the first `frames`
        slots with the weights exp(cos / T) (knn.knn_weights), normalised"""
        idx, cos = self.neighbours(q_int8, radius, k, frames)
        return self.mix(idx, knn_weights(cos, T), frames)


def upsample_argmax(seg, grid, r, out=None):
    """-> uint8 [Gh * r, Gw * r]: the argmax over the K classes of seg (float32 [Gh * Gw, K], what TokenMemory.propagate returns)
    upsampled bilinearly by r with align_corners=False -- the library's exact float64 definition (ivit_upsample_argmax_u8), the
    lowest class among equals; the upsampled planes never exist.  out: a dense uint8 [Gh * r, Gw * r] tensor to write into."""
    who = "upsample_argmax"
    (Gh, Gw), r = (int(v) for v in grid), int(r)
    if seg.dim() != 2 or not seg.is_cuda or seg.dtype != torch.float32 or int(seg.shape[0]) != Gh * Gw or Gh < 1 or Gw < 1:
        raise ValueError(f"{who}: float32 soft labels [{Gh} * {Gw}, K] on the device wanted, got {seg.dtype} {tuple(seg.shape)} on {seg.device}")
    K = int(seg.shape[1])
    if not 1 <= r <= R_MAX or not 1 <= K <= CLASSES_MAX:
        raise ValueError(f"{who}: r={r} outside [1, {R_MAX}] or K={K} classes outside [1, {CLASSES_MAX}]")
    seg = seg.contiguous()
    if out is None:
        out = torch.empty(Gh * r, Gw * r, dtype=torch.uint8, device=seg.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (Gh * r, Gw * r) or not out.is_contiguous() or out.device != seg.device:
        raise ValueError(f"{who}: out must be a dense uint8 [{Gh * r}, {Gw * r}] tensor on {seg.device}, got {out.dtype} {tuple(out.shape)}")
    _lib.call("ivit_upsample_argmax_u8", _lib.ptr(seg), Gh, Gw, r, K, _lib.ptr(out), _lib.stream_ptr())
    return out


def bound_radius(bound_th, H, W):
    """the boundary tolerance in pixels of davis2017-evaluation's f_measure: bound_th itself from 1, else ceil(bound_th * |(H, W)|)"""
    return int(bound_th) if bound_th >= 1 else int(math.ceil(bound_th * math.sqrt(H * H + W * W)))


def mask_scores(pred, truth, num_objects, bound_th=0.008):
    """-> int64 [n, O, 6] on the device: inter, union, n_fg, n_gt, fg_match, gt_match of the object masks (label == o, o = 1 .. O) of two
    uint8 [n, H, W] stacks of label maps (ivit_mask_scores_u8): the counts of the region similarity J and of the boundary measure F
    with the tolerance bound_radius(bound_th, H, W).  One launch for all frames and objects, no host synchronisation."""
    who = "mask_scores"
    if pred.dim() != 3 or pred.shape != truth.shape or pred.dtype != torch.uint8 or truth.dtype != torch.uint8 or not pred.is_cuda \
            or truth.device != pred.device:
        raise ValueError(f"{who}: two uint8 [n, H, W] stacks on one device wanted, got {pred.dtype} {tuple(pred.shape)} on {pred.device} and "
                         f"{truth.dtype} {tuple(truth.shape)} on {truth.device}")
    n, H, W = (int(v) for v in pred.shape)
    O = int(num_objects)
    if not 1 <= O <= OBJECTS_MAX or H < 2 or W < 2 or H * W >= 2 ** 31:
        raise ValueError(f"{who}: {O} objects outside [1, {OBJECTS_MAX}] or frames of {H} x {W} pixels (at least 2 each, below 2^31)")
    R = bound_radius(bound_th, H, W)
    if not 0 <= R <= RADIUS_MAX:
        raise ValueError(f"{who}: bound_th={bound_th} is a radius of R={R} pixels at {H} x {W}, outside [0, {RADIUS_MAX}]")
    counts = torch.empty(n, O, 6, dtype=torch.int64, device=pred.device)
    _lib.call("ivit_mask_scores_u8", _lib.ptr(pred.contiguous()), _lib.ptr(truth.contiguous()), n, H, W, O, R, _lib.ptr(counts), _lib.stream_ptr())
    return counts


def davis_measures(counts):
    """counts [n, O, 6] (mask_scores) -> (J, F), float64 [n, O] each, on the host.  J = inter / union, 1 where the union is empty.
    F = 2 P R / (P + R) (0 where P + R = 0) of the precision P = fg_match / n_fg and the recall R = gt_match / n_gt, with the
    reference's empty cases: no predicted boundary gives P = 1, R = 0; no true boundary P = 0, R = 1; neither P = R = 1."""
    c = torch.as_tensor(counts).detach().cpu().to(torch.float64)
    if c.dim() != 3 or c.shape[2] != 6:
        raise ValueError(f"davis_measures: counts of shape [n, O, 6] wanted, got {tuple(c.shape)}")
    inter, union, n_fg, n_gt, fg_match, gt_match = c.unbind(2)
    one, zero = torch.ones_like(inter), torch.zeros_like(inter)
    J = torch.where(union == 0, one, inter / union.clamp(min=1))
    P = torch.where(n_fg == 0, one, torch.where(n_gt == 0, zero, fg_match / n_fg.clamp(min=1)))
    Rc = torch.where(n_gt == 0, one, torch.where(n_fg == 0, zero, gt_match / n_gt.clamp(min=1)))
    F = torch.where(P + Rc == 0, zero, 2 * P * Rc / torch.where(P + Rc == 0, one, P + Rc))
    return J, F
