"""Which execution path a model mirror takes, and when its fused engine must be rebuilt.

The reference has one path (module by module, /root/reference/models/vit_quant.py:285-312).  The mirrors have two that
must agree bit for bit: the module path and the fused integer engine.  The engine is a snapshot of the model (integer
weights, requantisers, tables derived from the float parameters and the QuantAct ranges), so it is only taken

  * when it implements exactly what the module tree would compute -- `engine_unsupported_reason()` returns None:
    I-ViT operators, every QuantAct / Shiftmax / ShiftGELU width that the kernels hard-wire (the eight width knobs of
    vit_quant.py:180-187 / quant_train.py:295-306 change some of them), supported geometry; anything else runs module by
    module, which honours every width it can represent and raises for those it cannot;
  * while the snapshot is current -- the cache is keyed on the device and on a fingerprint of every parameter's and
    buffer's autograd version counter, and dropped by `load_state_dict`, `.to()/.cuda()` (`_apply`), `train()`,
    `fix()/unfix()` (freeze_model / unfreeze_model).  Tensors edited through `.data` bypass version counters: call
    `invalidate_engine()` after such surgery.
"""
from __future__ import annotations

import torch

from .quantization_utils import QuantAct
from .quantization_utils import quant_modules as _qm


class EngineDispatch:
    """Mixin for VisionTransformer / SwinTransformer (nn.Module subclasses)."""

    # QuantActs that never gate the engine (Swin's unused act_out, swin_quant.py:518)
    _frozen_exempt = ()

    def _init_dispatch(self):
        self._engine = None          # (device, fingerprint, engine)
        self._tracked = None         # flat tensor list behind the fingerprint
        self._qacts = None
        self.use_engine = True       # frozen models take the fused engine when it is exact for them
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_engine())

    # -- invalidation ---------------------------------------------------------------------------------------------
    def invalidate_engine(self):
        self._engine = None
        self._tracked = None

    def _apply(self, fn, *a, **k):          # .to() / .cuda() / .float(): parameters move or change
        self.invalidate_engine()
        return super()._apply(fn, *a, **k)

    def train(self, mode: bool = True):
        self.invalidate_engine()
        return super().train(mode)

    def fix(self):
        self.invalidate_engine()

    def unfix(self):
        self.invalidate_engine()

    def _fingerprint(self):
        if self._tracked is None:
            self._tracked = list(self.parameters()) + list(self.buffers())
        # version counters only grow, so their sum over a fixed tensor list changes whenever any tensor is written in place
        return sum(t._version for t in self._tracked)

    # -- state ----------------------------------------------------------------------------------------------------
    def _quant_acts(self):
        if self._qacts is None:
            self._qacts = [(n, m) for n, m in self.named_modules() if isinstance(m, QuantAct) and n not in self._frozen_exempt]
        return self._qacts

    def is_frozen(self):
        return all(not m.running_stat for _, m in self._quant_acts())

    def engine_unsupported_reason(self):
        raise NotImplementedError

    def _build_engine(self, device, max_batch):
        raise NotImplementedError

    def _width_mismatch(self, expected: dict):
        """first QuantAct whose activation_bit differs from what the fused kernels hard-wire (`expected`: full module name ->
        width; every QuantAct not listed is 8 bit)"""
        for n, m in self._quant_acts():
            want = expected.get(n, 8)
            if int(m.activation_bit) != want:
                return f"QuantAct {n} is {int(m.activation_bit)}-bit (fused engine: {want})"
        return None

    def engine(self, max_batch):
        """The fused engine for the model's CURRENT parameters and ranges (rebuilt when either changed)."""
        device = next(self.parameters()).device
        fp = self._fingerprint()
        cur = self._engine
        if cur is not None and cur[0] == device and cur[1] == fp and cur[2].max_batch >= max_batch:
            return cur[2]
        if cur is not None and cur[0] == device and cur[1] == fp:
            max_batch = max(max_batch, cur[2].max_batch)     # grow, never thrash between batch sizes
        eng = self._build_engine(device, max_batch)
        self._engine = (device, fp, eng)
        return eng

    def features_unsupported_reason(self):
        """engine_unsupported_reason() without its head condition: None when the fused engine computes this model's backbone outputs
        (features, forward_intermediates, attention_maps) exactly, with or without a classifier"""
        raise NotImplementedError

    def _reason_cached(self, features=False):
        """engine_unsupported_reason() (features: features_unsupported_reason()), re-evaluated only when a QuantAct's width changed
        (it builds 4 * depth dictionaries; this predicate runs on every forward, and a DeiT-T batch-1 forward is 0.7 ms)"""
        key = tuple(int(m.activation_bit) for _, m in self._quant_acts())
        slot = "_features_reason_cache" if features else "_reason_cache"
        c = self.__dict__.get(slot)
        if c is None or c[0] != key:
            c = self.__dict__[slot] = (key, self.features_unsupported_reason() if features else self.engine_unsupported_reason())
        return c[1]

    def _engine_state_ok(self, x):
        """what both predicates ask of the moment: no io-stat collection, use_engine, eval mode, a GPU input, frozen ranges"""
        if getattr(self, "_io_stat_hooks", False) and _qm.io_stats_enabled():
            return False      # attach_io_stat_hooks: the collector's hooks sit on the sub-modules, which the fused engine never calls
        return bool(self.use_engine and not self.training and x.is_cuda and self.is_frozen())

    def takes_engine(self, x: torch.Tensor) -> bool:
        return self._engine_state_ok(x) and self._reason_cached() is None

    def takes_engine_for_features(self, x: torch.Tensor) -> bool:
        """takes_engine for the calls that never reach the classifier (features, features_graph, forward_intermediates,
        attention_maps): the same conditions with features_unsupported_reason(), so a headless model (num_classes=0) passes"""
        return self._engine_state_ok(x) and self._reason_cached(features=True) is None

    # -- backbone outputs -----------------------------------------------------------------------------------------
    def _carries(self, x):
        """the lazy.scope condition of forward(): a frozen model in eval mode on the GPU carries integers between its modules"""
        return x.is_cuda and not self.training and self.is_frozen()

    def _feature_bits(self):
        """width of the QuantAct whose output forward_features returns (8 in both references)"""
        raise NotImplementedError

    def features(self, x, integers=False, out=None):
        """The embedding a frozen backbone is used for -> (features [B, C], scale): the first value of forward_features(x) --
        float32, integers times scale -- or with integers=True those integers (int8), and the float32 act_scaling_factor of the
        QuantAct that produced them as a float.  Where takes_engine_for_features(x) holds this is the fused engine's
        forward_features (no head GEMM, no classifier launch; a headless model included).  Otherwise forward_features runs module by
        module, under the lazy.scope condition forward() uses; integers=True then converts its float tensor back and checks, as
        forward_intermediates' module path does, that it is integers of that width times the scale.
        out: a [B, C] view to write the features into (rows of a feature bank; the engine's `out=`, which the module path fills
        with a copy)."""
        from .quantization_utils import lazy
        if self.takes_engine_for_features(x):
            return self.engine(x.shape[0]).forward_features(x.contiguous().float(), integers, out)
        if not self.is_frozen():
            self.invalidate_engine()
        with lazy.scope(self._carries(x)):
            f, s = self.forward_features(x)
        f = f.to_float(boundary=True) if isinstance(f, lazy.QT) else f
        s = s.as_subclass(torch.Tensor).reshape(-1)      # (a lazy.QS scale: the plain tensor)
        assert s.numel() == 1 and s.dtype == torch.float32, "forward_features: a per-tensor float32 scale"
        if integers:
            bits = self._feature_bits()
            q = torch.round(f / s)
            assert bool((q * s == f).all()) and bool((q >= -2 ** (bits - 1)).all()) and bool((q < 2 ** (bits - 1)).all()), \
                f"forward_features: the output is not a {bits}-bit integer times its scale"
            f = q.to(torch.int16 if bits > 8 else torch.int8)
        if out is not None:
            if out.dtype != f.dtype or tuple(out.shape) != tuple(f.shape):
                raise ValueError(f"out must be a {f.dtype} tensor {list(f.shape)}")
            out.copy_(f)
            f = out
        return f, float(s[0])

    def features_graph(self, x, integers=False, resident=False):
        """features(x) from a graph replay of the fused engine (GraphReplay.forward_features_graph): the same bytes, in the graph's
        own output tensor, valid until the next replay of that graph.  ValueError where takes_engine_for_features(x) does not hold
        (the module path's graph replays logits: ModuleGraph.forward_graph)."""
        if not self.takes_engine_for_features(x):
            why = self._reason_cached(features=True) or "model not frozen, in training mode, use_engine off, or input not on the GPU"
            raise ValueError(f"features_graph: the fused engine does not take this call ({why})")
        xin = x if (x.dtype == torch.float32 and x.is_contiguous()) else x.contiguous().float()
        return self.engine(x.shape[0]).forward_features_graph(xin, integers, resident)

    def ranges(self):
        return {n: (float(m.x_min.reshape(-1)[0]), float(m.x_max.reshape(-1)[0]))
                for n, m in self.named_modules() if isinstance(m, QuantAct)}

    def _hooked_outputs(self, x, modules):
        """forward_tokens off the engine: the modules are called one by one as the reference's forward calls them (the whole forward,
        then the head where there is one), with a forward hook on each of modules = {key: module} -> {key: what it returned};
        the hooks are removed in any case"""
        got, handles = {}, []
        for key, mod in modules.items():
            handles.append(mod.register_forward_hook(lambda m, a, out, key=key: got.__setitem__(key, out)))
        try:
            with torch.no_grad():
                if not self.is_frozen():
                    self.invalidate_engine()
                f, s = self.forward_features(x)
                if self.num_classes > 0:
                    self.head(f, s)
        finally:
            for h in handles:
                h.remove()
        return got

    def _hooked_intermediates(self, x, sites, integers):
        """forward_intermediates off the engine: the modules are called one by one as the reference's forward calls them, with a
        forward hook on each selected module.  sites = {key: (module, its name, the QuantAct whose output it returns, t0, (H, W))};
        the hooked (x [B, t0 + H * W, C], s) is checked to be integers of that QuantAct's width times s, its first t0 tokens are
        dropped and the rest goes to [B, C, H, W].  -> {key: (map, scale)}; the hooks are removed in any case.
        This path always runs the whole forward (forward_features, then the head where there is one), for forward_intermediates_early too: the
        modules are the reference's and are called as it calls them."""
        got, handles = {}, []

        def hook(key, name, qact, t0, hw):
            def record(mod, args, out):
                v, s = out
                s = s.reshape(-1)
                assert s.numel() == 1 and s.dtype == torch.float32, f"{name}: a per-tensor float32 scale"
                bits = int(qact.activation_bit)
                q = torch.round(v / s)
                assert bool((q * s == v).all()) and bool((q >= -2 ** (bits - 1)).all()) and bool((q < 2 ** (bits - 1)).all()), \
                    f"{name}: the output is not a {bits}-bit integer times its scale"
                B, C = v.shape[0], v.shape[-1]
                assert v.shape[1] == t0 + hw[0] * hw[1], f"{name}: {v.shape[1]} tokens"
                keep = (q.to(torch.int16 if bits > 8 else torch.int8) if integers else v)[:, t0:]
                got[key] = (keep.permute(0, 2, 1).reshape(B, C, *hw).contiguous(), float(s[0]))
            return record

        for key, (mod, name, qact, t0, hw) in sites.items():
            handles.append(mod.register_forward_hook(hook(key, name, qact, t0, hw)))
        try:
            with torch.no_grad():
                if not self.is_frozen():
                    self.invalidate_engine()
                f, s = self.forward_features(x)
                if self.num_classes > 0:
                    self.head(f, s)
        finally:
            for h in handles:
                h.remove()
        return got
