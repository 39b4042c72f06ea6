"""Data-parallel driver: images are independent units, so each rank runs the whole integer forward on
its own shard with replicated weights; the ONLY exchange is one all-gather of the per-image top-1
indices (int32[B/rank]) per batch -- RCCL over xGMI on GPUs (torch.distributed backend "nccl"),
gloo in the CPU tests.  SURVEY.md §8e.  (The reference has no distributed path at all: its NCCL
helpers in /root/reference/utils/utils.py:215-237 are dead code.)"""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_bounds(n: int, world: int, rank: int):
    """Contiguous shard [lo, hi) of n images for `rank` (sizes differ by at most one)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def gather_top1(local_top1: torch.Tensor, world: int, counts=None) -> torch.Tensor:
    """all-gather of the per-rank top-1 vectors -> [sum of the shard sizes] in rank order.  `counts`: shard size of every rank
    when they differ (shard_bounds of a batch that the world does not divide): every rank pads its vector to the largest shard,
    ONE all_gather_into_tensor as for equal shards, and the padding is cut out of the result."""
    if world == 1 and not (dist.is_available() and dist.is_initialized()):
        return local_top1      # no process group: a plain single-GPU run (a one-rank group still runs the collective)
    if counts is not None and len(set(counts)) > 1:
        assert len(counts) == world and local_top1.numel() == counts[dist.get_rank()]
        width = max(counts)
        padded = torch.zeros(width, dtype=local_top1.dtype, device=local_top1.device)
        padded[: local_top1.numel()] = local_top1
        out = torch.empty(world * width, dtype=local_top1.dtype, device=local_top1.device)
        dist.all_gather_into_tensor(out, padded)
        return torch.cat([out[r * width: r * width + c] for r, c in enumerate(counts)])
    out = torch.empty(world * local_top1.numel(), dtype=local_top1.dtype, device=local_top1.device)
    dist.all_gather_into_tensor(out, local_top1.contiguous())
    return out


class DataParallelTop1:
    """graph=True: the local forward is a HIP-graph replay reading `local_images` in place (the caller refills that tensor
    between steps); the all-gather stays an ordinary stream-ordered RCCL call after it.  counts: see gather_top1."""

    def __init__(self, engine, world: int, graph: bool = False, counts=None):
        self.engine, self.world, self.graph, self.counts = engine, world, graph, counts

    def step(self, local_images: torch.Tensor) -> torch.Tensor:
        if self.graph:
            _, _, top1 = self.engine.forward_graph(local_images, resident=True)
        else:
            _, _, top1 = self.engine(local_images)
        return gather_top1(top1, self.world, self.counts)


def gather_rows(local: torch.Tensor, world: int, counts=None) -> torch.Tensor:
    """all-gather of per-rank row blocks [B_local, w] -> [sum of the shard sizes, w] in rank order: ONE
    all_gather_into_tensor, uneven shards padded to the largest as in gather_top1 (`counts`: every rank's shard size)."""
    assert local.dim() == 2
    if world == 1 and not (dist.is_available() and dist.is_initialized()):
        return local
    w = local.shape[1]
    if counts is not None and len(set(counts)) > 1:
        assert len(counts) == world and local.shape[0] == counts[dist.get_rank()]
        rows = max(counts)
        padded = torch.zeros(rows, w, dtype=local.dtype, device=local.device)
        padded[: local.shape[0]] = local
        out = torch.empty(world * rows, w, dtype=local.dtype, device=local.device)
        dist.all_gather_into_tensor(out, padded)
        return torch.cat([out[r * rows: r * rows + c] for r, c in enumerate(counts)])
    out = torch.empty(world * local.shape[0], w, dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, local.contiguous())
    return out


def gather_topk(local_topk: torch.Tensor, world: int, counts=None) -> torch.Tensor:
    """per-rank top-k class indices (int32 [B_local, k]) -> [B_global, k] in rank order"""
    return gather_rows(local_topk, world, counts)


def gather_logits(local_logits: torch.Tensor, world: int, counts=None) -> torch.Tensor:
    """per-rank INT32 logits [B_local, classes] -> [B_global, classes] in rank order (the float logits are the same
    integers times the per-class scale: gather the integers, scale once)"""
    if local_logits.dtype != torch.int32:
        raise TypeError("gather_logits takes the int32 logits")
    return gather_rows(local_logits, world, counts)


def gather_feature_rows(local_q: torch.Tensor, local_labels: torch.Tensor, scale, sizes, world: int):
    """The end of a data-parallel feature extraction (inference.extract_features_parallel) -> (q int8 [N, C], labels int64 [N],
    scale) on every rank, rows in loader order.  local_q int8 [n, C] / local_labels int64 [n]: this rank's shard_bounds slices of
    the global batches, one after the other; sizes: the size of every global batch (each rank saw the same loader); scale: the
    float32 scale of the integers, None on a rank whose slices were all empty.

    ONE all_gather_into_tensor (gather_rows): a row travels as its C integers followed by the 8 bytes of its label, and one more
    row per rank carries its scale; uneven shards are padded to the largest and trimmed by `counts`, as gather_top1 does.  The
    rank-major result is then indexed back into loader order."""
    assert local_q.dtype == torch.int8 and local_q.dim() == 2 and local_labels.dtype == torch.int64
    n, C = local_q.shape
    w = C + 8
    bounds = [[shard_bounds(B, world, r) for B in sizes] for r in range(world)]
    counts = [sum(hi - lo for lo, hi in bounds[r]) for r in range(world)]
    rank = dist.get_rank() if world > 1 else 0
    assert n == counts[rank] == local_labels.numel()
    packed = torch.zeros(n + 1, w, dtype=torch.int8, device=local_q.device)
    packed[:n, :C] = local_q
    packed[:n, C:] = local_labels.contiguous().view(torch.int8).view(n, 8)
    if scale is not None:
        packed[n, :4] = torch.tensor([float(scale)], dtype=torch.float32).view(torch.int8).to(local_q.device)
        packed[n, 4] = 1
    got = gather_rows(packed, world, [c + 1 for c in counts])
    base = [sum(counts[:r]) + r for r in range(world)]      # first row of rank r in `got`
    order, seen = [], [0] * world
    for j in range(len(sizes)):
        for r in range(world):
            lo, hi = bounds[r][j]
            order.append(torch.arange(base[r] + seen[r], base[r] + seen[r] + hi - lo))
            seen[r] += hi - lo
    order = torch.cat(order).to(got.device) if order else torch.zeros(0, dtype=torch.int64, device=got.device)
    rows = got[order]
    for r in range(world):      # the scale of the first rank that has one (every rank computes the same)
        tail = got[base[r] + counts[r]]
        if int(tail[4]):
            scale = float(tail[:4].contiguous().view(torch.float32)[0])
            break
    return rows[:, :C].contiguous(), rows[:, C:].contiguous().view(torch.int64).reshape(-1), scale


def allreduce_hits(hits: torch.Tensor, total) -> tuple:
    """ONE all_reduce(SUM) of [hits[0..k), total] -> (hits int64 [k] summed over ranks, total summed over ranks) on every
    rank.  hits: the int64 rank-r hit counts of topk.count_hits / forward_topk; total: this rank's image count."""
    buf = torch.empty(hits.numel() + 1, dtype=torch.int64, device=hits.device)
    buf[:-1] = hits
    buf[-1] = int(total)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
    return buf[:-1], int(buf[-1])


class DataParallelTopK:
    """DataParallelTop1 with the top-k classes of every image: each rank runs forward_topk (graph=True: its graph replay,
    reading `local_images` -- and `targets` / `hits` -- in place) and ONE all-gather of the int32 [B_local, k] rows follows.
    targets (int32 [B_local]) with hits (int64 [k]): the rank's hit counts accumulate on its device (allreduce_hits at the
    end of an evaluation)."""

    def __init__(self, engine, world: int, k: int = 5, graph: bool = False, counts=None):
        self.engine, self.world, self.k, self.graph, self.counts = engine, world, k, graph, counts

    def step(self, local_images: torch.Tensor, targets=None, hits=None) -> torch.Tensor:
        if self.graph:
            _, _, topk = self.engine.forward_topk_graph(local_images, self.k, targets, hits, resident=True)
        else:
            _, _, topk = self.engine.forward_topk(local_images, self.k, targets, hits)
        return gather_topk(topk, self.world, self.counts)
