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
value).  There is no fallback: anything the kernels do not take raises."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .knn import SPLITS_MAX, knn_weights

K_MAX = 32           # IVIT_LOCAL_K_MAX
CLASSES_MAX = 256    # IVIT_PROPAGATE_CLASSES_MAX
C_MAX = 1024         # the widest rows of ivit_local_topk_i8


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
