"""HIP-graph replay of an engine's forward: the ~100 kernel launches of one forward are captured once per batch size on a
capture stream and replayed with a single graph launch (launch-bound shapes gain most; at batch 256 it removes the
host's ~100 ctypes calls per step from the picture).  All launches go through the C ABI on
`torch.cuda.current_stream()`, the engines allocate nothing inside `forward`, so the capture is exact; results are the
same workspace views `forward` returns.

ModuleGraph does the same for the frozen module-by-module forward of the model mirrors (the ~200 launches of a Swin-T forward,
each behind tensor subclasses and `__torch_function__` dispatch on the host): every configuration the engines decline."""
from __future__ import annotations

import torch

from .topk import check_request


class GraphReplay:
    """Mixin for IntViTEngine / IntSwinEngine."""

    def forward_graph(self, images: torch.Tensor, resident: bool = False):
        """resident=False: `images` is copied into the graph's own input buffer before every replay.
        resident=True: the graph reads `images` itself (the caller keeps that tensor alive and refills it in place,
        e.g. a loader's device-side staging buffer) -- no copy per step."""
        self._require_head("forward_graph")
        return self._replay(images, resident, (), lambda x, warm: self._graph_forward(x))

    def forward_features_graph(self, images: torch.Tensor, integers: bool = False, resident: bool = False):
        """forward_features as a graph replay -> (features [B, C], scale), the bytes of the eager call.  One graph per (batch size,
        input dtype, integers) -- a key of its own, so the logits graph of the same batch size stays what it is -- and, with
        resident=True, input pointer.  features is the graph's own output tensor, valid until the next replay of the same graph."""
        return self._replay(images, resident, ("features", bool(integers)), lambda x, warm: self._graph_features(x, bool(integers)))

    def forward_topk_graph(self, images: torch.Tensor, k: int = 5, targets=None, hits=None, resident: bool = False):
        """forward_topk as a graph replay.  `targets` / `hits` are read and accumulated in place like a resident image tensor:
        one graph per (batch size, k, targets pointer, hits pointer); the caller refills `targets` between replays and reads
        `hits` when it likes.  The warm-up forward outside the capture runs without them, so `hits` only counts replays."""
        self._require_head("forward_topk_graph")
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


class ModuleGraph:
    """Mixin for vit_quant.VisionTransformer / swin_quant.SwinTransformer: graph replay of the frozen module-by-module forward, for
    every configuration the fused engines decline (dispatch.EngineDispatch.takes_engine).

    A frozen model's module path (quantization_utils/lazy.py) is a fixed launch sequence: its constants are built on the host once
    and cached by `_version` keys, every launch goes through `_lib.call` on `torch.cuda.current_stream()`.  `forward_graph`
    captures that sequence once per batch size -- GraphReplay's scheme: warm-up on a side stream outside the capture, one
    `torch.cuda.graph` on one capture stream (a single chain, nothing forked), a cache per key -- and replays it with one graph
    launch, without the tensor subclasses, the dispatch and the ctypes call per launch of the eager forward.

    What a literal step of the path takes to the host (lazy.Tape) is recorded at the warm-up forward where it depends on frozen
    constants only, and kept on the device, in the graph's status word, where it depends on the activations."""

    @property
    def _graphs(self):
        """key -> (graph, static input, static output, tape)"""
        return self.__dict__.setdefault("_module_graphs", {})

    def _graph_modules(self):
        """[(name, module)] of the whole tree, walked once (the walk costs as much as a small model's replay) and kept until
        drop_graphs(); the modules' parameter and buffer dictionaries are read afresh on every call"""
        mods = self.__dict__.get("_module_graph_mods")
        if mods is None:
            mods = self.__dict__["_module_graph_mods"] = list(self.named_modules())
        return mods

    def graph_signature(self):
        """Everything the constants of a captured forward were built from: `data_ptr()` and `_version` of every parameter and
        buffer (weights, QuantAct ranges, the I-BERT LayerNorm shift, relative position tables, shift masks, and the buffers the
        modules publish), whether the integer-carrying path is on, and `use_engine`."""
        from .quantization_utils import lazy
        sig = [(t.data_ptr(), t._version) for _, m in self._graph_modules() for d in (m._parameters, m._buffers)
               for t in d.values() if t is not None]
        sig.append((lazy.ENABLED, lazy.active(), bool(self.use_engine)))
        return tuple(sig)

    def graph_refusal(self):
        """why forward_graph cannot capture this model as it stands, or None"""
        if not self.is_frozen():
            n = next(n for n, m in self._quant_acts() if m.running_stat)
            return f"the model is not frozen (QuantAct {n} still updates its range): freeze_model first"
        if self.training:
            return "the model is in training mode: a replay cannot draw dropout masks or update statistics; call model.eval()"
        for n, m in self._graph_modules():
            if m._forward_hooks or m._forward_pre_hooks:
                return (f"module {n or '(the model itself)'} carries a forward {'hook' if m._forward_hooks else 'pre-hook'}: a replay "
                        "cannot run hooks; remove it, or call model(x)")
            if m.__dict__.get("overflow_handling", False) and "shift" in m._buffers:      # (no getattr: nn.Module's fallback is slow)
                return (f"IBERTIntLayerNorm {n} still handles overflow (it raises its shift from the activations on the host): "
                        "freeze_model first")
        return None

    def forward_graph(self, x: torch.Tensor, resident: bool = False):
        """What `model(x)` returns -- float logits [B, classes], bit for bit -- from a graph replay.

        Where `takes_engine(x)` holds this is the fused engine's own `forward_graph`.  Otherwise the module-by-module forward that
        `model(x)` runs at this moment is captured, once per (batch size, input dtype) and, with resident=True, input pointer: the
        graph then reads `x` itself (the caller keeps that tensor alive and refills it in place); with resident=False `x` is copied
        into the graph's own input buffer before every replay.

        The key also holds `graph_signature()`: an in-place write to, or a replacement of, any parameter or buffer drops this
        model's graphs, and the next call captures again -- a graph never outlives a range or weight it baked in.  (A literal step
        publishes a freshly allocated scale buffer on every eager call, so for a model with such steps an eager `model(x)` between
        two replays costs a capture.  Tensors edited through `.data` bypass version counters, and the module tree is walked once and
        kept: call `drop_graphs()` after such surgery or after replacing a sub-module.)

        The result is the graph's static output buffer, valid until the next replay of the same graph (the engines' contract).
        Refused with a ValueError, before anything is captured: a model that is not frozen, training mode, a forward hook or
        pre-hook on any sub-module, an input that is not on the GPU.  Checks the eager forward makes on the activations on the host
        (8-bit overflow in front of a literal GEMM) are made on the device instead: see `graph_status()`."""
        from .quantization_utils import lazy
        reason = self.graph_refusal()
        if reason is None and not x.is_cuda:
            reason = "the input is not on the GPU"
        if reason:
            raise ValueError(f"forward_graph: {reason}")
        if self.takes_engine(x):
            xin = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()
            return self.engine(x.shape[0]).forward_graph(xin, resident)[1]
        sig = self.graph_signature()
        if self.__dict__.get("_module_graph_sig") != sig:
            self._graphs.clear()
            self.__dict__["_module_graph_sig"] = sig
        cache = self._graphs
        B = x.shape[0]
        key = (B, x.dtype, x.data_ptr()) if resident else (B, x.dtype)
        if key not in cache:
            dev = x.device
            if resident:
                static_in = x
            else:
                static_in = torch.empty_like(x)
                static_in.copy_(x)
            tape = lazy.Tape()
            with torch.no_grad():
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    self(static_in)       # builds and caches every constant (read-backs, uploads, first-use paths)
                    with lazy.taping(tape):
                        self(static_in)   # the steady forward, as it will be captured: its literal steps are recorded
                torch.cuda.current_stream(dev).wait_stream(side)
                status = torch.zeros(max(1, len(tape.messages)), dtype=torch.int32, device=dev)
                tape.replay(status)
                graph = torch.cuda.CUDAGraph()
                with lazy.taping(tape), torch.cuda.graph(graph):
                    out = self(static_in)
            if not tape.complete():
                raise RuntimeError("module graph: the captured forward ended before its warm-up forward's literal steps did")
            cache[key] = (graph, static_in, out, tape)
            self.__dict__["_module_graph_sig"] = self.graph_signature()     # the capture's own literal steps published buffers
        graph, static_in, out, _ = cache[key]
        if not resident:
            static_in.copy_(x)
        graph.replay()
        return out

    def graph_status(self):
        """Raises what the eager forward would have raised from a look at the activations, for any replay since the last call:
        the captured kernels set one word per check in their graph's status tensor.  One device -> host read of those words, when
        the caller chooses (after an evaluation loop, say); a model whose forward is carried as integers throughout has no such
        check and nothing is read."""
        from . import _lib
        live = [(key, g[3]) for key, g in self._graphs.items() if g[3].messages]
        if not live:
            return
        words = torch.cat([t.status for _, t in live]).cpu().tolist()
        at = 0
        for key, t in live:
            for i, message in enumerate(t.messages):
                if words[at + i]:
                    t.status.zero_()
                    raise _lib.IvitError(f"{message} (graph replay at batch size {key[0]})")
            at += len(t.messages)

    def drop_graphs(self):
        """Frees this model's graphs (the fused engine's too).  A module-path graph's private pool keeps EVERY intermediate of the
        forward alive -- the module path allocates each activation where the engines reuse one workspace -- so a graph holds
        about the peak-free sum of one eager forward's allocations per batch size until it is dropped."""
        self.__dict__.pop("_module_graphs", None)
        self.__dict__.pop("_module_graph_sig", None)
        self.__dict__.pop("_module_graph_mods", None)
        eng = self.__dict__.get("_engine")
        if eng is not None and hasattr(eng[2], "drop_graphs"):
            eng[2].drop_graphs()
