"""HIP-graph replay of an engine's forward: the ~100 kernel launches of one forward are captured once per batch size on a
capture stream and replayed with a single graph launch (launch-bound shapes gain most; at batch 256 it removes the
host's ~100 ctypes calls per step from the picture).  All launches go through the C ABI on
`torch.cuda.current_stream()`, the engines allocate nothing inside `forward`, so the capture is exact; results are the
same workspace views `forward` returns."""
from __future__ import annotations

import torch

from .topk import check_request


class GraphReplay:
    """Mixin for IntViTEngine / IntSwinEngine."""

    def forward_graph(self, images: torch.Tensor, resident: bool = False):
        """resident=False: `images` is copied into the graph's own input buffer before every replay.
        resident=True: the graph reads `images` itself (the caller keeps that tensor alive and refills it in place,
        e.g. a loader's device-side staging buffer) -- no copy per step."""
        return self._replay(images, resident, (), lambda x, warm: self._graph_forward(x))

    def forward_topk_graph(self, images: torch.Tensor, k: int = 5, targets=None, hits=None, resident: bool = False):
        """forward_topk as a graph replay.  `targets` / `hits` are read and accumulated in place like a resident image tensor:
        one graph per (batch size, k, targets pointer, hits pointer); the caller refills `targets` between replays and reads
        `hits` when it likes.  The warm-up forward outside the capture runs without them, so `hits` only counts replays."""
        check_request(self.num_classes, images.shape[0], self.dev, k, targets, hits)
        tag = ("topk", k, 0 if targets is None else targets.data_ptr(), 0 if hits is None else hits.data_ptr())
        return self._replay(images, resident, tag, lambda x, warm: self._graph_forward_topk(x, k, None if warm else targets,
                                                                                           None if warm else hits))

    # what the replays capture: an engine may override these with a forward that issues other launches for the same results
    # (IntViTEngine: the last block on the class rows)
    def _graph_forward(self, images):
        return self.forward(images)

    def _graph_forward_topk(self, images, k, targets, hits):
        return self.forward_topk(images, k, targets, hits)

    def _replay(self, images, resident, tag, run):
        """run(x, warm): the forward to capture (warm=True: the uncaptured warm-up call); tag: extends the cache key"""
        B = images.shape[0]
        cache = self.__dict__.setdefault("_graphs", {})
        key = ((B, images.dtype, images.data_ptr()) if resident else (B, images.dtype)) + tag
        if key not in cache:
            if resident:
                static_in = images
            else:
                static_in = torch.empty_like(images)
                static_in.copy_(images)
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(side):           # warm-up outside the capture (lazy module loads, first-use paths)
                run(static_in, True)
            torch.cuda.current_stream(self.dev).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = run(static_in, False)
            cache[key] = (graph, static_in, out)
        graph, static_in, out = cache[key]
        if not resident:
            static_in.copy_(images)
        graph.replay()
        return out

    def drop_graphs(self):
        self.__dict__.pop("_graphs", None)
