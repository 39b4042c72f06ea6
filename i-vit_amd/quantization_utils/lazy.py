"""The frozen module-by-module path without float round trips: integer-carrying tensors and fusion at the QuantAct.

The reference's model files (/root/reference/models/vit_quant.py:61-90, 142-155, 285-312; swin_quant.py:121-169, 251-301, 328-349,
539-564) call QuantLinear, QuantAct, IVITIntLayerNorm, ... one by one and move float32 `value = integer * scale` tensors between
them.  Executed literally that is a float -> integer conversion, an integer kernel and an integer -> float conversion per module,
plus host read-backs of every scale: 250 ms for a DeiT-B batch of 256 that the fused engine does in 6.5 ms.  This module keeps the
calls and removes the round trips, for a FROZEN model (every QuantAct fixed):

  * a frozen QuantAct returns a `QT` -- a torch.Tensor subclass with the float tensor's shape / dtype / device but an **integer
    payload** (no float storage): int8 (`q8`) behind an 8-bit QuantAct, int16 (`q16`) behind a 16-bit one in the Swin patterns
    below, `q` for either -- and a `QS` scale tensor that carries its value on the host as well;
  * a module whose input is a QT does not compute: it returns a QT holding a **pending node** (linear, conv, layer norm, GELU,
    the matmul -> scale -> QuantAct -> softmax -> matmul chain of attention, with Swin's bias QuantAct and `+ mask` in it);
  * the shape operations the model files apply in between (reshape, permute, transpose, roll, flatten, contiguous) are recorded
    on the payload, or on the pending node, and not executed; indexing, unbind, eval-mode dropout and `* scalar` act on the payload;
  * the next consumer of a payload composes the recorded operations into ONE row permutation (replayed once per shape and
    sequence on an int32 row-index tensor on the host): Swin's window partition / cyclic shift and their inverse become one
    `ivit_window_rows` launch, any other row permutation one index_select, anything else the torch operations themselves;
  * the NEXT QuantAct launches ONE fused integer kernel for the node (GEMM + requantisation to 8 or 16 bits, LayerNorm on the
    8- or 16-bit stream + requantisation, GELU table, fused (window) attention, residual add, residual GEMM) -- the kernels of
    the fused engines -- and returns a QT again;
  * a QT also carries `fl`, the strides the reference's FLOAT tensor would have (each recorded view replayed on a meta tensor; a
    QuantAct / LayerNorm result keeps its input's layout as the elementwise chain does): IVITIntLayerNorm's float32 mean runs in
    the outer order over the transposed view behind Swin's patch embedding (ivit_modules.py:56-61), and every LayerNorm of Swin's
    first stage inherits that layout.  A layout that is neither contiguous nor that transpose materialises;
  * anything else that touches a QT (an unexpected torch function, a hook, the float pooling of Swin's tail, the caller reading
    the logits) materialises the float tensor the reference would have produced, through the module's ordinary path, with the
    reference's strides, and continues from there.

Every (m, e) pair, table, row map, bias / mask table and integer weight is derived on the host from host-side scales and cached
per module, so after the first (warm-up) forward a frozen forward reads nothing back from the device: it runs under
`torch.cuda.set_sync_debug_mode("error")` and can be captured into a HIP graph (tests/test_gpu_modules.py, test_gpu_swin_lazy.py).
Covers the I-ViT and the I-BERT operator families (ivit_modules.py, ibert_modules.py) at 8-bit QuantAct widths, ViT's 16-bit
configurations (vit_quant.py:180-187: the 16-bit residual stream with softmax and position embedding at 8 or 16 bits, resolve16)
and Swin with either family (8-bit QuantActs, 16-bit residual stream), in any mixture: every site is resolved by the class of its own
module.  Other configurations (other width mixtures, operator names with constructor parameters) take the ordinary module path through
the materialisation rule above wherever a step is not one of the patterns.  Such a literal step does read scales and ranges back on
every call; `Tape` (below) is what lets graph.ModuleGraph capture a forward that contains one.
"""
from __future__ import annotations

import os

import threading
import warnings

import numpy as np
import torch

from .. import _lib, gemm_forms
from ..engine_common import attention, attention_entry, attention_spec, frag_copy, gelu_lut, layernorm, ln_spec, long_multipliers_ok
from ..prepare import LayerNormParams, LinearParams, dyadic, dyadic1, f32, quant_sym, sym_scale

ENABLED = os.environ.get("IVIT_LAZY", "1") != "0"
_ALWAYS = [os.environ.get("IVIT_LAZY") == "always"]      # enable_everywhere(): process-wide, independent of any open scope
_TLS = threading.local()                                  # .depth: open `scope(True)` blocks of THIS thread; .mat: nested to_float calls
STATS = {"fused": 0, "materialised": 0}     # fused launches at a QuantAct / float tensors materialised, since the last reset
_WARNED = set()
ROW_KERNEL = True       # pure row permutations of a payload (Swin's window partition / shift) as one launch; False: the torch ops


def active() -> bool:
    """inside `with lazy.scope(True):` (this thread) -- the model mirror opens it around the module-by-module forward of a frozen
    I-ViT model -- or after enable_everywhere()"""
    return ENABLED and (_ALWAYS[0] or getattr(_TLS, "depth", 0) > 0)


def enable_everywhere(on: bool = True):
    """Frozen QuantActs carry integers wherever they are called from -- for callers that drive the modules themselves, e.g. the
    reference's own models/vit_quant.py or swin_quant.py imported on top of this package.  The mirrors'
    VisionTransformer.forward and SwinTransformer.forward open the scope by themselves; nothing else does by default.  Same as
    IVIT_LAZY=always in the environment."""
    _ALWAYS[0] = bool(on)       # never touches the scope depth: switching it off inside an open scope leaves the scope intact


class scope:
    def __init__(self, on: bool):
        self.on = bool(on) and ENABLED

    def __enter__(self):
        _TLS.depth = getattr(_TLS, "depth", 0) + int(self.on)

    def __exit__(self, *exc):
        _TLS.depth = getattr(_TLS, "depth", 0) - int(self.on)
        return False


# ----------------------------------------------------------------------------------------------------------- graph capture
class Tape:
    """What a literal step (a module's `_slow`) of a frozen forward takes to the host, for graph.ModuleGraph: the modules' ordinary
    forms read scales, ranges and the I-BERT LayerNorm shift back from the device and upload (m, e) pairs on every call, and two of
    them decide on the activations (narrow_i8's overflow flag, QuantMatMul's choice of kernel by the largest probability).  A
    capture allows neither.  Both kinds go through the tape of the thread:

      * `take(label, build)`: a value that depends on frozen constants only.  While the tape RECORDS (the warm-up forward, run
        eagerly) `build()` runs and its result is kept, device tensors included; while it REPLAYS (the capture) the recorded value
        is returned in the same order, and a forward that asks for anything else than its warm-up did is an error.  The graph is
        keyed on everything those constants were built from (graph.ModuleGraph.graph_signature);
      * `flag(message)`: a check on the activations.  Recording: None -- the eager check runs, and raises as ever.  Replaying: one
        int32 word of the graph's status tensor, which the captured kernel (or torch operation) sets to non-zero instead;
        ModuleGraph.graph_status() reads the words and raises `message`.

    Without a tape -- every eager call -- nothing changes."""

    def __init__(self):
        self.items, self.messages, self.recording, self.pos, self.used, self.status = [], [], True, 0, 0, None

    def replay(self, status):
        """status: int32 [max(1, len(self.messages))], zeroed"""
        self.recording, self.pos, self.used, self.status = False, 0, 0, status

    def take(self, label, build):
        if self.recording:
            v = build()
            self.items.append((label, v))
            return v
        if self.pos >= len(self.items) or self.items[self.pos][0] != label:
            raise RuntimeError(f"module graph: the captured forward asks for {label!r} where its warm-up forward asked for "
                               f"{self.items[self.pos][0] if self.pos < len(self.items) else 'nothing more'!r}")
        self.pos += 1
        return self.items[self.pos - 1][1]

    def flag(self, message):
        if self.recording:
            self.messages.append(message)
            return None
        if self.used >= len(self.messages) or self.messages[self.used] != message:
            raise RuntimeError(f"module graph: the captured forward checks {message!r}, which its warm-up forward did not")
        self.used += 1
        return self.status[self.used - 1:self.used]

    def complete(self):
        return self.pos == len(self.items) and self.used == len(self.messages)


class taping:
    """`with lazy.taping(tape):` -- the literal steps of this thread's forwards go through `tape`"""

    def __init__(self, tape):
        self.tape = tape

    def __enter__(self):
        self.prev = getattr(_TLS, "tape", None)
        _TLS.tape = self.tape
        return self.tape

    def __exit__(self, *exc):
        _TLS.tape = self.prev
        return False


def tape():
    return getattr(_TLS, "tape", None)


def taped(label, build):
    """build(), or under a Tape its recorded result (Tape.take)"""
    t = getattr(_TLS, "tape", None)
    return build() if t is None else t.take(label, build)


def _st():
    return _lib.stream_ptr()


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ----------------------------------------------------------------------------------------------------------- scale tensors
class QS(torch.Tensor):
    """a scale tensor (real float32 storage on the device) that also knows its value on the host (`.host`, float32 array)"""

    @staticmethod
    def make(host, device):
        host = np.atleast_1d(np.asarray(host, dtype=f32)).copy()
        r = torch.Tensor._make_subclass(QS, torch.from_numpy(host.copy()).to(device))
        r.host = host
        r._mul = {}
        return r

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name in ("mul", "__mul__", "__rmul__") and len(args) == 2:
            a, b = (args[0], args[1]) if isinstance(args[0], QS) else (args[1], args[0])
            if isinstance(a, QS) and isinstance(b, (int, float)) and not isinstance(b, bool):
                key = float(b)
                if key not in a._mul:        # float32 tensor * python scalar: the scalar is taken at float32
                    a._mul[key] = QS.make((a.host * f32(key)).astype(f32), a.device)
                return a._mul[key]
            if isinstance(a, QS) and isinstance(b, QS) and a.host.size == 1 and b.host.size == 1:
                key = ("qs", id(b))
                if key not in a._mul:
                    a._mul[key] = QS.make((a.host * b.host).astype(f32), a.device)
                    a._mul[key]._keep = b      # keeps id(b) valid
                return a._mul[key]
        if name in ("view", "reshape") and isinstance(args[0], QS):
            with torch._C.DisableTorchFunctionSubclass():
                t = func(*args, **kwargs)
            r = torch.Tensor._make_subclass(QS, t)
            r.host = args[0].host
            r._mul = args[0]._mul
            return r
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **kwargs)
        if isinstance(out, QS):                 # any other op: a plain tensor, the host value is not carried on
            out = out.as_subclass(torch.Tensor)
        return out


def host_of(s):
    """host value of a scale tensor, or None if it is not a QS (the caller then takes the ordinary path)"""
    return s.host if isinstance(s, QS) else None


# ----------------------------------------------------------------------------------------------------------- int-carrying tensors
_VIEW = {"reshape", "view", "permute", "transpose", "__getitem__", "flatten", "contiguous", "unbind", "squeeze", "unsqueeze",
         "select", "narrow", "expand", "roll"}
_ROWOPS = {"reshape", "view", "permute", "transpose", "flatten", "contiguous", "roll"}      # recorded on a payload, not executed
_META = {"size", "dim", "numel", "__len__", "is_floating_point", "element_size", "is_contiguous", "stride", "storage_offset",
         "ndimension", "nelement", "is_complex", "get_device", "type"}


def _sig(name, args, kwargs):
    """hashable description of one recorded shape operation (cache key of the composed row permutation, of the bias integers)"""
    def one(a):
        if isinstance(a, torch.Tensor):
            return ("T", a.data_ptr(), tuple(a.shape), tuple(a.stride()), str(a.dtype), a._version)
        if isinstance(a, (tuple, list)):
            return tuple(one(b) for b in a)
        if isinstance(a, slice):
            return ("S", a.start, a.stop, a.step)
        if a is None or a is Ellipsis or isinstance(a, (int, float, str, bool)):
            return a
        return repr(a)
    return (name, tuple(one(a) for a in args), tuple(sorted((k, one(v)) for k, v in kwargs.items())))


def _meta_replay(fn, fl, name):
    """the float layout (a meta tensor: shape and strides of the tensor the reference would hold) after one shape operation"""
    if name == "roll":                    # torch.roll returns a contiguous tensor
        return torch.empty(fl.shape, device="meta")
    return fn(fl)


def _dense_strides(fl):
    """strides of a non-contiguous but dense float layout (a permuted tensor: elementwise results keep it), else None"""
    if fl.is_contiguous():
        return None
    st = fl.stride()
    return st if torch.empty_like(fl).stride() == st else None


def act_layout(x_fl, id_fl=None):
    """layout of a QuantAct's result (quant_modules.py QuantAct._slow): the identity's when it has the result's shape, else the
    input's; a dense permuted layout is kept, anything else comes out contiguous"""
    lay = id_fl if (id_fl is not None and tuple(id_fl.shape) == tuple(x_fl.shape)) else x_fl
    return torch.empty_like(lay) if not lay.is_contiguous() else torch.empty(x_fl.shape, device="meta")


def ln_outer(fl):
    """how IVITIntLayerNorm reduces a row of this layout (ivit_modules.py:56-61): 0 -- the contiguous order; L -- the outer order
    over the [B, L, C] transpose of a contiguous [B, C, L] tensor; None -- neither (the caller materialises)"""
    if fl.dim() < 2 or fl.stride(-1) == 1 or fl.shape[-1] <= 1:
        return 0
    if fl.dim() == 3 and fl.stride(1) == 1 and fl.stride(2) == fl.shape[1] and fl.stride(0) == fl.shape[1] * fl.shape[2]:
        return int(fl.shape[1])
    return None


def _reshapes_only(views):
    """exactly one recorded view, a reshape / view"""
    return len(views) == 1 and getattr(views[0], "view_name", None) in ("reshape", "view")


class QT(torch.Tensor):
    """float32-shaped tensor WITHOUT float storage: an integer payload -- `q8` int8, or `q16` int16 for a frozen 16-bit QuantAct;
    `q` is whichever it holds -- plus `rops`, shape operations recorded on it and not executed yet; or `node`, a pending
    operation, plus `views`, the shape operations recorded since.  `fl` (a meta tensor) carries the strides the reference's float
    tensor would have: the reduction order of a LayerNorm depends on them."""

    @staticmethod
    def wrap(shape, device, q8=None, scale=None, node=None, views=(), q16=None, fl=None, rops=(), origin=None):
        r = torch.Tensor._make_wrapper_subclass(QT, tuple(shape), dtype=torch.float32, device=device, requires_grad=False)
        r._q8, r._q16, r.scale, r.node, r.views, r.rops, r.origin = q8, q16, scale, node, tuple(views), tuple(rops), origin
        r.fl = fl if fl is not None else torch.empty(tuple(shape), device="meta")
        return r

    def _run_rops(self):
        if self.rops:
            out = run_rows(self._q8 if self._q8 is not None else self._q16, self.rops, tuple(self.shape))
            if self._q8 is not None:
                self._q8 = out
            else:
                self._q16 = out
            self.rops = ()

    @property
    def q8(self):
        """the int8 payload (None for an int16 one); a deferred requantising GEMM (Requant) is launched the first time anybody asks
        for it, recorded shape operations are executed"""
        if self._q8 is None and self._q16 is None and isinstance(self.node, Requant):
            self._q8 = self.apply_views(self.node.force())
            self.node, self.views = None, ()
        self._run_rops()
        return self._q8

    @property
    def q16(self):
        """the int16 payload (None for an int8 one); a deferred GEMM with a 16-bit QuantAct (Requant16) is launched the first time
        anybody asks for it"""
        if self._q8 is None and self._q16 is None and isinstance(self.node, Requant16):
            self._q16 = self.apply_views(self.node.force())
            self.node, self.views = None, ()
        self._run_rops()
        return self._q16

    @property
    def q(self):
        """the integer payload of either width"""
        a = self.q8
        return a if a is not None else self.q16

    def _like(self, shape, fl, **kw):
        """a QT of the same width, scale and origin around another payload / more recorded operations"""
        return QT.wrap(shape, self.device, scale=self.scale, fl=fl, **kw)

    # -- materialisation: the float tensor the reference's module would have returned
    def to_float(self, boundary=False):
        """`boundary`: the model hands its result to the caller (the one materialisation a forward is meant to have).  Any other
        outermost call means something inside the model looked at a float tensor -- correct, but that module then runs the float
        round trips the int8-carrying path exists to avoid: one warning per kind of producer (and lazy.STATS counts them all)."""
        STATS["materialised"] += 1
        depth = getattr(_TLS, "mat", 0)
        if depth == 0 and not boundary:
            what = "int8 payload" if self._q8 is not None else "int16 payload" if self._q16 is not None else (
                type(self.node).__name__ + (f"({self.node.kind})" if hasattr(self.node, "kind") else ""))
            if what not in _WARNED:
                _WARNED.add(what)
                warnings.warn(f"ivit_amd.lazy: an int8-carrying activation ({what}) was materialised as float32 inside the model; the "
                              "modules behind it run their float form (about 30x slower per module) -- see lazy.STATS", RuntimeWarning,
                              stacklevel=2)
        _TLS.mat = depth + 1
        try:
            q = self.q
            if q is not None:
                y = q.to(torch.float32) * self.scale.as_subclass(torch.Tensor).reshape(-1)[0]
                st = _dense_strides(self.fl)         # a permuted layout the reference's tensor has (Swin's first stage): consumers
                if st is not None and tuple(y.stride()) != tuple(st):     # that reduce over it depend on it
                    y = torch.empty_strided(tuple(y.shape), tuple(st), dtype=y.dtype, device=y.device).copy_(y)
                elif self.fl.is_contiguous() and not y.is_contiguous() and _dense_strides(y) is not None:
                    y = y.contiguous()
                return y
            t = self.node.to_float()
            for fn in self.views:
                t = fn(t)
            return t
        finally:
            _TLS.mat = depth

    def apply_views(self, t):
        for fn in self.views:
            t = fn(t)
        return t

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        # reached only by an operator that slipped past __torch_function__: materialise and run it on real tensors
        def real(t):
            return t.to_float() if isinstance(t, QT) else t
        return func(*torch.utils._pytree.tree_map(real, args), **torch.utils._pytree.tree_map(real, kwargs or {}))

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        self = args[0] if args and isinstance(args[0], QT) else None
        if name == "__get__" or name in _META:
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)
        if self is not None and name in _VIEW:
            rest = args[1:]

            def fn(t, _f=func, _r=rest, _k=kwargs):
                return _f(t, *_r, **_k)
            fn.view_name = name

            if self._q8 is None and self._q16 is None and isinstance(self.node, Requant16):
                self.q16      # a shape operation on a deferred 16-bit GEMM: launched now, the operation recorded on its payload
            payload = self._q8 if self._q8 is not None else self._q16
            if payload is not None:
                sig = _sig(name, rest, kwargs)
                origin = None if self.origin is None else self.origin + (sig,)
                wide = {"q8": None, "q16": None}
                if name in _ROWOPS:
                    # not executed: the next consumer composes the recorded operations into one row permutation (run_rows)
                    fl = _meta_replay(fn, self.fl, name)
                    wide["q8" if self._q8 is not None else "q16"] = payload
                    return self._like(fl.shape, fl, rops=self.rops + ((name, fn, sig, rest, kwargs),), origin=origin, **wide)
                out = fn(self.q)
                try:
                    fl = _meta_replay(fn, self.fl, name)
                except Exception:          # e.g. an index tensor on the device: the result of such an operation is contiguous
                    fl = None

                def one(o, f):
                    wide["q8" if o.dtype == torch.int8 else "q16"] = o
                    return self._like(o.shape, f if f is not None and tuple(f.shape) == tuple(o.shape) else None, origin=origin, **wide)
                if isinstance(out, (tuple, list)):
                    res = []
                    for i, o in enumerate(out):
                        wide = {"q8": None, "q16": None}
                        res.append(one(o, None if fl is None else fl[i]))
                    return tuple(res)
                return one(out, fl)
            meta = _meta_replay(fn, self.fl, name)
            if isinstance(meta, (tuple, list)):
                return tuple(QT.wrap(m.shape, self.device, scale=self.scale, node=self.node, fl=m,
                                     views=self.views + ((lambda t, _fn=fn, _i=i: _fn(t)[_i]),)) for i, m in enumerate(meta))
            return QT.wrap(meta.shape, self.device, scale=self.scale, node=self.node, views=self.views + (fn,), fl=meta)
        if name in ("dropout", "dropout_", "feature_dropout", "alpha_dropout") and self is not None:
            training = kwargs.get("training", args[2] if len(args) > 2 else kwargs.get("train", True))
            if not training:
                return self
        if name in ("mul", "__mul__", "__rmul__") and len(args) == 2:
            a, b = (args[0], args[1]) if isinstance(args[0], QT) else (args[1], args[0])
            if isinstance(b, (int, float)) and not isinstance(b, bool):
                # value * c with the scale multiplied by c alongside (vit_quant.py:74-75): the integers stay what they are
                if a.q8 is not None:
                    return QT.wrap(a.shape, a.device, q8=a.q8, scale=a.scale * b, fl=a.fl)
                if a._q16 is None:
                    return QT.wrap(a.shape, a.device, node=Scaled(a, float(b)))
        if name in ("add", "__add__", "__radd__") and len(args) == 2 and ENABLED:
            a, b = (args[0], args[1]) if isinstance(args[0], QT) else (args[1], args[0])
            # `+ mask` on the pending, biased scores of a shifted window (swin_quant.py:149-155): stays pending
            # the scores reshaped to [B, nW, nH, N, N], the mask [1, nW, 1, N, N] (mask.unsqueeze(1).unsqueeze(0)): nothing else
            if (isinstance(a, QT) and isinstance(a.node, Biased) and _reshapes_only(a.views) and type(b) is torch.Tensor
                    and b.dtype == torch.float32 and not kwargs and a.dim() == 5 and a.shape[3] == a.shape[4]
                    and tuple(b.shape) == (1, a.shape[1], 1, a.shape[3], a.shape[4])):
                return QT.wrap(a.shape, a.device, node=Masked(a, b))
        if name == "cat" and ENABLED:
            tensors = args[0]
            dim = kwargs.get("dim", args[1] if len(args) > 1 else 0)
            if all(isinstance(t, QT) and t.q is not None or not isinstance(t, QT) for t in tensors):
                shapes = [torch.empty(t.shape, device="meta") for t in tensors]
                meta = torch.cat(shapes, dim=dim)
                return QT.wrap(meta.shape, next(t.device for t in tensors if isinstance(t, QT)), node=Cat(list(tensors), dim))

        def real(t):
            return t.to_float() if isinstance(t, QT) else t

        args = torch.utils._pytree.tree_map(real, args)
        kwargs = torch.utils._pytree.tree_map(real, kwargs)
        return func(*args, **kwargs)


# ----------------------------------------------------------------------------------------------------------- row permutations
_ROWPLAN = {}


_TORCH_PLAN = ("torch",)


def row_plan(shape, rops):
    """What the recorded shape operations `rops` do to the rows (the last dimension, left whole) of a contiguous tensor of `shape`,
    found by replaying them on an int32 row-index tensor on the host:
      ("identity",) | ("window", B, H, W, ws, shift, inverse) -- swin_engine.window_row_map or its inverse, one ivit_window_rows
      launch | ("index", perm) -- any other row permutation: destination row j takes source row perm[j] | ("torch",) -- not a
      row permutation: the operations run on the payload as they are"""
    from ..swin_engine import window_row_map
    C = shape[-1]
    if len(shape) < 2:
        return _TORCH_PLAN
    rows = int(np.prod(shape[:-1]))
    if rows >= 2 ** 31:
        return _TORCH_PLAN
    idx = torch.arange(rows, dtype=torch.int32).reshape(*shape[:-1], 1)
    meta = torch.empty(shape, device="meta")
    cands = [tuple(shape)]
    for name, fn, _, args, kwargs in rops:
        nd = meta.dim()
        try:
            new = _meta_replay(fn, meta, name)
            if new.shape[-1] != C or new.numel() != meta.numel():
                return _TORCH_PLAN
            if name in ("reshape", "view", "flatten"):
                idx = idx.reshape(*new.shape[:-1], 1)
            elif name == "permute":
                dims = args[0] if len(args) == 1 and isinstance(args[0], (tuple, list)) else args
                if kwargs or int(dims[-1]) % nd != nd - 1:
                    return _TORCH_PLAN
                idx = fn(idx)
            elif name == "transpose":
                if kwargs or len(args) != 2 or any(int(d) % nd == nd - 1 for d in args):
                    return _TORCH_PLAN
                idx = fn(idx)
            elif name == "roll":
                dims = kwargs.get("dims", args[1] if len(args) > 1 else None)
                if dims is None:
                    return _TORCH_PLAN
                dims = dims if isinstance(dims, (tuple, list)) else (dims,)
                if any(int(d) % nd == nd - 1 for d in dims):
                    return _TORCH_PLAN
                idx = fn(idx)
            elif name != "contiguous":
                return _TORCH_PLAN
        except Exception:
            return _TORCH_PLAN
        if tuple(idx.shape[:-1]) != tuple(new.shape[:-1]):
            return _TORCH_PLAN
        meta = new
        cands.append(tuple(meta.shape))
    perm = idx.reshape(-1).numpy().astype(np.int64)
    if perm.size != rows or not np.array_equal(np.sort(perm), np.arange(rows)):
        return _TORCH_PLAN
    if np.array_equal(perm, np.arange(rows)):
        return ("identity",)
    for B, H, W in dict.fromkeys(c[:3] for c in cands if len(c) == 4 and c[0] * c[1] * c[2] == rows):
        L = H * W
        first = perm[:L]
        if first.max() >= L:
            continue
        g = int(np.gcd(H, W))
        for ws in (d for d in range(2, g + 1) if g % d == 0):
            for shift in range(ws):
                m1 = window_row_map(1, H, W, ws, shift)
                inverse = np.array_equal(first, m1)                 # dst row r = src row map[r]
                if not inverse:
                    inv = np.empty(L, np.int64)
                    inv[m1] = np.arange(L)
                    if not np.array_equal(first, inv):              # dst row map[r] = src row r
                        continue
                m = window_row_map(B, H, W, ws, shift)
                if not inverse:
                    inv = np.empty(rows, np.int64)
                    inv[m] = np.arange(rows)
                    m = inv
                if np.array_equal(perm, m):
                    return ("window", B, H, W, ws, shift, int(inverse))
    return ("index", perm)


def run_rows(base, rops, out_shape):
    """executes the shape operations recorded on a payload: one row gather where they compose to a row permutation"""
    plan = None
    if ROW_KERNEL and base.dim() >= 2 and base.is_contiguous():
        key = (tuple(base.shape), tuple(r[2] for r in rops))
        plan = _ROWPLAN.get(key)
        if plan is None:
            if len(_ROWPLAN) >= 256:
                _ROWPLAN.clear()
            plan = _ROWPLAN[key] = [row_plan(tuple(base.shape), rops), {}]
        plan, dev_maps = plan
        if plan[0] == "identity":
            return base.reshape(out_shape)
        row_bytes = base.shape[-1] * base.element_size()
        if plan[0] == "window" and base.is_cuda and row_bytes % 16 == 0 and base.data_ptr() % 16 == 0:
            _, B, H, W, ws, shift, inverse = plan
            out = torch.empty(out_shape, dtype=base.dtype, device=base.device)
            _lib.call("ivit_window_rows", _lib.ptr(base), _lib.ptr(out), B, H, W, row_bytes, ws, shift, inverse, _st())
            return out
        if plan[0] in ("window", "index"):
            dk = str(base.device)
            if dk not in dev_maps:
                if plan[0] == "window":
                    from ..swin_engine import window_row_map
                    _, B, H, W, ws, shift, inverse = plan
                    perm = window_row_map(B, H, W, ws, shift)
                    if not inverse:
                        inv = np.empty(perm.size, np.int64)
                        inv[perm] = np.arange(perm.size)
                        perm = inv
                else:
                    perm = plan[1]
                dev_maps[dk] = _dev(perm.astype(np.int64), base.device)
            return base.reshape(-1, base.shape[-1]).index_select(0, dev_maps[dk]).reshape(out_shape)
    t = base
    for r in rops:
        t = r[1](t)
    return t


# ----------------------------------------------------------------------------------------------------------- pending nodes
class Node:
    def to_float(self):
        raise NotImplementedError


class Scaled(Node):
    """x * c on a pending node (attn * self.scale): only the scale changes, which the model code multiplies itself"""

    def __init__(self, x, c):
        self.x, self.c = x, c

    def to_float(self):
        return self.x.to_float() * self.c


class Cat(Node):
    def __init__(self, parts, dim):
        self.parts, self.dim = parts, dim

    def to_float(self):
        return torch.cat([p.to_float() if isinstance(p, QT) else p for p in self.parts], dim=self.dim)


class Biased(Node):
    """WindowAttention.qact2 on the pending scores with the float relative position bias as its identity (swin_quant.py:143-147):
    pending until Shiftmax and the second matmul arrive"""

    def __init__(self, x, pre_sf, identity, identity_sf, s_out, s_out_qs, qact):
        self.x, self.pre_sf, self.identity, self.identity_sf, self.qact = x, pre_sf, identity, identity_sf, qact
        self.s_in, self.s_id, self.s_out, self.s_out_qs = pre_sf.host, identity_sf.host, s_out, s_out_qs

    def to_float(self):
        return self.qact._slow(self.x.to_float(), self.pre_sf, self.identity.to_float(), self.identity_sf)[0]


class Masked(Node):
    """`+ mask` on the biased scores of a shifted window (swin_quant.py:149-155)"""

    def __init__(self, x, mask):
        self.x, self.mask = x, mask
        self.s_out_qs = x.node.s_out_qs

    def to_float(self):
        return self.x.to_float() + self.mask


class ModNode(Node):
    """the pending call of a module: `mod._slow(*float inputs)` reproduces what the ordinary path returns"""

    def __init__(self, kind, mod, shape, inputs, scales, out_scale):
        self.kind, self.mod, self.shape, self.inputs, self.scales, self.out_scale = kind, mod, tuple(shape), inputs, scales, out_scale

    def to_float(self):
        if self.kind == "linear":          # the classifier head: int32 GEMM and one conversion, nothing read back
            y = linear_to_float(self.mod, self.inputs[0], self.scales[0])
            if y is not None:
                return y
        xs = [x.to_float() if isinstance(x, QT) else x for x in self.inputs]
        return self.mod._slow(*xs, *self.scales)[0]


def pending(kind, mod, shape, device, inputs, scales, out_scale, fl=None):
    """-> (QT holding the pending call, out_scale): what the module's forward returns"""
    return QT.wrap(shape, device, node=ModNode(kind, mod, shape, inputs, scales, out_scale), fl=fl), out_scale


def q8_contig(x):
    """int8 payload of a QT as a contiguous tensor (None if x is not an int8-carrying QT)"""
    if isinstance(x, QT) and x.q8 is not None:
        return x.q8 if x.q8.is_contiguous() else x.q8.contiguous()
    return None


def q16_contig(x):
    if isinstance(x, QT) and x.q16 is not None:
        return x.q16 if x.q16.is_contiguous() else x.q16.contiguous()
    return None


def _merged_patches(parts, dim):
    """PatchMerging's cat of the four strided slices of one int16 [B, H, W, C] payload (swin_quant.py:337-344) as one
    ivit_patch_merge_i16 launch; None if the parts are anything else"""
    if len(parts) != 4 or any(p.dim() != 4 or p.dtype != torch.int16 for p in parts) or dim not in (-1, 3):
        return None
    B, H2, W2, C = parts[0].shape
    H, W = 2 * H2, 2 * W2
    p0 = parts[0]
    base = p0.data_ptr()
    for p, (dy, dx) in zip(parts, ((0, 0), (1, 0), (0, 1), (1, 1))):
        if (tuple(p.shape) != (B, H2, W2, C) or tuple(p.stride()) != (H * W * C, 2 * W * C, 2 * C, 1)
                or p.data_ptr() - base != 2 * (dy * W + dx) * C or p.untyped_storage().data_ptr() != p0.untyped_storage().data_ptr()):
            return None
    if C % 4 or base % 8:
        return None
    out = torch.empty(B, H2, W2, 4 * C, dtype=torch.int16, device=p0.device)
    _lib.call("ivit_patch_merge_i16", _lib.ptr(p0), _lib.ptr(out), B, H, W, C, _st())
    return out


def int_width(x):
    """8 / 16: x holds (or is a cat of parts that hold) an integer payload of that width; None otherwise"""
    if not isinstance(x, QT):
        return None
    if x.q is not None:
        return 8 if x._q8 is not None else 16
    if isinstance(x.node, Cat) and x.node.parts and all(isinstance(p, QT) and p.q is not None for p in x.node.parts):
        widths = {8 if p._q8 is not None else 16 for p in x.node.parts}
        if len(widths) == 1:
            return widths.pop()
    return None


def int_payload(x):
    """the contiguous integer payload of a QT for which int_width(x) is not None"""
    q = x.q
    if q is None:
        parts = [p.q for p in x.node.parts]
        q = _merged_patches(parts, x.node.dim)
        if q is None:
            q = torch.cat(parts, dim=x.node.dim)
        q = x.apply_views(q)
    return q if q.is_contiguous() else q.contiguous()


# ----------------------------------------------------------------------------------------------------------- the fused launches
def _cache(mod, key, build):
    c = mod.__dict__.setdefault("_lazy_cache", {})
    if key not in c:
        if len(c) >= 64:       # a model whose ranges keep changing (re-calibrated and re-frozen again and again): start over
            c.clear()
        c[key] = build()
    return c[key]


def _key(*hosts):
    return tuple(np.asarray(h, f32).tobytes() if h is not None else None for h in hosts)


def params_on_device(mod) -> bool:
    """the integer parameters of this QuantLinear / QuantConv2d are derived on the device (quant_modules.LINEAR_PARAMS_ON_DEVICE)"""
    from . import quant_modules
    return mod.weight.device.type == "cuda" and quant_modules.LINEAR_PARAMS_ON_DEVICE


def device_linear_params(mod, s_in):
    """Integer parameters of a QuantLinear / QuantConv2d whose weight lives on a GPU, for input scale s_in, without a weight crossing
    the bus: prepare.LinearParams bit for bit, by ivit_weight_quant_rows_f32_i8 and ivit_bias_quant_f32_i32.  Two caches on the module:
      weight part, key (weight._version, device): W [Np, Kp] int8, zero-filled, K padded to the GEMM's 64-byte slabs and, for a
          QuantLinear, N to a multiple of 4 (its callers slice [:N] where they want no row padding); scale [N]; w_int [N, K] float32;
      bias part, key (weight._version, bias._version, s_in, device): s_acc [N]; b [Np] int32 (zero behind N) and b_int [N] float32,
          both None without a bias.
    A batch that only moved the ranges launches the bias kernel alone.  -> (weight part, bias part)"""
    w, bias = mod.weight, mod.bias
    dev = w.device
    N = w.shape[0]
    Kin = w.numel() // N
    wkey = (w._version, str(dev))
    wp = mod.__dict__.get("_dev_weight_part")
    if wp is None or wp["key"] != wkey:
        wf = w.detach().reshape(N, Kin).contiguous().float()
        K = (Kin + 63) // 64 * 64
        Np = N + (-N % 4 if isinstance(mod, torch.nn.Linear) else 0)     # the GEMM wants N % 4 == 0: zero rows (QuantLinear._slow)
        W = torch.zeros(Np, K, dtype=torch.int8, device=dev)
        scale = torch.empty(N, dtype=torch.float32, device=dev)
        w_int = torch.empty(N, Kin, dtype=torch.float32, device=dev)
        _lib.call("ivit_weight_quant_rows_f32_i8", _lib.ptr(wf), Kin, N, Kin, _lib.ptr(scale), _lib.ptr(W), K, _lib.ptr(w_int), _st())
        # scale feeds the bias kernel of every later batch: the module's buffer gets a copy of its own (scale_out), made once here
        wp = mod.__dict__["_dev_weight_part"] = dict(key=wkey, N=N, Np=Np, K=K, Kin=Kin, W=W, scale=scale, scale_out=scale.clone(),
                                                     w_int=w_int)
    s = float(np.asarray(s_in, f32).reshape(-1)[0])
    bkey = (w._version, None if bias is None else bias._version, s, str(dev))
    bp = mod.__dict__.get("_dev_bias_part")
    if bp is None or bp["key"] != bkey:
        s_acc = torch.empty(N, dtype=torch.float32, device=dev)
        b = b_int = bf = None
        if bias is not None:
            bf = bias.detach().contiguous().float()
            b = torch.zeros(wp["Np"], dtype=torch.int32, device=dev)
            b_int = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.call("ivit_bias_quant_f32_i32", _lib.ptr(bf), _lib.ptr(wp["scale"]), N, s, _lib.ptr(s_acc), _lib.ptr(b), _lib.ptr(b_int), _st())
        bp = mod.__dict__["_dev_bias_part"] = dict(key=bkey, s_acc=s_acc, b=b, b_int=b_int)
    return wp, bp


def linear_consts(lin, s_in, device):
    """integer weights of a QuantLinear / QuantConv2d for input scale s_in (host float32): W8 row-major (+ the 16x16x64
    fragment copy where the weights-in-registers GEMM applies), b32, s_acc (and its host copy for the per-channel multipliers)"""
    def build():
        if params_on_device(lin):
            wp, bp = device_linear_params(lin, s_in)
            lin._publish_device(wp, bp)
            N, K, Kin = wp["N"], wp["K"], wp["Kin"]
            s_acc = bp["s_acc"].cpu().numpy()      # N floats: QS and dyadic (_gemm_me) want them on the host
            d = dict(N=N, K=K, Kin=Kin, W=wp["W"][:N], b=None if bp["b"] is None else bp["b"][:N], s_acc=QS.make(s_acc, device),
                     s_acc_host=s_acc)
            d["Wf"], d["Wf_bit"] = frag_copy(d["W"], _st())
            return d
        lp = LinearParams(lin.weight.detach().cpu().numpy(), None if lin.bias is None else lin.bias.detach().cpu().numpy(), s_in)
        N, Kin = lp.W8.shape
        K = (Kin + 63) // 64 * 64          # the GEMM kernels step K in 64-byte slabs: zero columns (Swin: K = 96, 48)
        W8 = lp.W8
        if K != Kin:
            W8 = np.zeros((N, K), np.int8)
            W8[:, :Kin] = lp.W8
        lin._publish(lp, device)           # the buffers the reference rewrites on every call
        d = dict(N=N, K=K, Kin=Kin, W=_dev(W8, device), b=None if lp.b32 is None else _dev(lp.b32, device),
                 s_acc=QS.make(lp.s_acc, device), s_acc_host=lp.s_acc)
        d["Wf"], d["Wf_bit"] = frag_copy(d["W"], _st())       # 128-channel work items for the int8 epilogues (gemm_forms.weight)
        return d
    return _cache(lin, ("lin", lin.weight._version, None if lin.bias is None else lin.bias._version, _key(s_in), str(device)), build)


def _gemm_me(lin, s_in, s_out, device, need_e31=True):
    """device (m, e) tables of the per-channel requantisation s_acc -> s_out, or None outside the int8 epilogues' contract (e < 31;
    need_e31 = False: the 16-bit epilogue, which takes any pair)"""
    c = linear_consts(lin, s_in, device)

    def build():
        m, e = dyadic(c["s_acc_host"], s_out)
        if need_e31 and np.any(e < 31):
            return None
        return _dev(m.view(np.int32), device), _dev(e, device)
    # keyed on the weight / bias versions as linear_consts is: an in-place weight edit under unchanged ranges rebuilds W8 and
    # s_acc there, and the per-channel multipliers must follow (round-3 advisor finding: they did not)
    return _cache(lin, ("rq", need_e31, lin.weight._version, None if lin.bias is None else lin.bias._version, _key(s_in, s_out),
                        str(device)), build)


def _frag_rows(c, epi, M):
    """M rows of this linear through epilogue `epi` run the weights-in-registers GEMM: the launch can be deferred (Requant,
    Requant16) so that a residual QuantAct behind it joins the kernel"""
    return bool(gemm_forms.weight(c, epi, M)[1] & gemm_forms.FRAGS)


def _operand(a8, c):
    """the A operand of a GEMM whose K was padded to the kernels' 64-byte slabs: zero columns to match"""
    return a8 if c["K"] == c["Kin"] else torch.nn.functional.pad(a8, (0, c["K"] - c["Kin"]))


def gemm_requant(lin, a8, s_in, s_out, device, bits=8):
    """a8 [M, K] int8 contiguous -> int8 [M, N]: GEMM + per-channel requantisation to s_out in one kernel; None if outside the
    kernels' contract.  bits = 4: the QuantAct clamps to [-8, 7] (ivit_gemm_i8_requant_bits_ex); the 8-bit launch is as it was"""
    c = linear_consts(lin, s_in, device)
    N, K = c["N"], c["K"]
    if N % 16 != 0:
        return None
    me = _gemm_me(lin, s_in, s_out, device)
    if me is None:
        return None
    a8 = _operand(a8, c)
    M = a8.shape[0]
    out = torch.empty(M, N, dtype=torch.int8, device=device)
    W, lay = gemm_forms.weight(c, gemm_forms.RQ, M)
    if bits == 8:
        _lib.call("ivit_gemm_i8_requant_ex", _lib.ptr(a8), K, _lib.ptr(W), K, _lib.ptr(c["b"]),
                  _lib.ptr(me[0]), _lib.ptr(me[1]), _lib.ptr(out), N, M, N, K, lay, _st())
    else:
        _lib.call("ivit_gemm_i8_requant_bits_ex", _lib.ptr(a8), K, _lib.ptr(W), K, _lib.ptr(c["b"]),
                  _lib.ptr(me[0]), _lib.ptr(me[1]), _lib.ptr(out), N, M, N, K, lay, bits, _st())
    return out


def resolve(qact, x, pre_sf, identity, identity_sf, s_out, s_out_qs):
    """The frozen 8-bit QuantAct on a QT: one fused launch -> int8 QT.  None: not a recognised pattern (ordinary path).
    A 4-bit QuantAct (a width knob of vit_quant.py:180-187 at 4: the clamp is [-8, 7], the payload still int8) is carried at the
    sites the knobs reach -- a linear or the patch convolution, the residual add alone or fused into the GEMM, the cat + position
    identity of qact1; behind any other producer it takes the ordinary path."""
    device = x.device
    s_in = host_of(pre_sf)
    if s_in is None:
        return None
    node = x.node
    bits = qact.activation_bit
    if bits != 8 and not (isinstance(node, (Requant, Cat)) or x._q8 is not None
                          or (isinstance(node, ModNode) and node.kind in ("linear", "conv"))):
        return None
    out = None
    fl = act_layout(x.fl, identity.fl if isinstance(identity, QT) else None)
    if isinstance(node, Scores) and identity is not None:
        # WindowAttention.qact2: the scores plus the float relative position bias (swin_quant.py:143-147); stays pending
        if (not x.views and isinstance(identity, QT) and identity.origin is not None and host_of(identity_sf) is not None
                and s_in is node.s_out_qs.host and host_of(identity_sf).size == 1 and s_in.size == 1):
            return QT.wrap(x.shape, device, node=Biased(x, pre_sf, identity, identity_sf, s_out, s_out_qs, qact))
        return None
    if isinstance(node, Requant) and x._q8 is None and identity is not None and not x.views:
        out = node.with_residual(identity, host_of(identity_sf), s_in, s_out, device, bits)
        if out is not None:
            STATS["fused"] += 1
            return QT.wrap(out.shape, device, q8=out, scale=s_out_qs, fl=fl)
    if x.q8 is not None:
        if identity is None:
            return None
        x8, i8 = q8_contig(x), q8_contig(identity)
        s_id = host_of(identity_sf)
        if i8 is None or s_id is None or i8.shape != x8.shape or s_in.size != 1 or s_id.size != 1:
            return None
        out = torch.empty_like(x8)
        if bits == 8:
            _lib.call("ivit_residual_requant_i8", _lib.ptr(x8), *dyadic1(s_in, s_out), _lib.ptr(i8), *dyadic1(s_id, s_out),
                      _lib.ptr(out), x8.numel(), _st())
        else:
            _lib.call("ivit_residual_requant_i8_bits", _lib.ptr(x8), *dyadic1(s_in, s_out), _lib.ptr(i8), *dyadic1(s_id, s_out),
                      _lib.ptr(out), x8.numel(), bits, _st())
        STATS["fused"] += 1
        return QT.wrap(out.shape, device, q8=out, scale=s_out_qs, fl=fl)
    if isinstance(node, Cat):
        out = _resolve_cat(qact, node, s_in, identity, identity_sf, s_out, device, bits)
    elif isinstance(node, ModNode) and identity is None:
        if s_in is not host_of(node.out_scale):     # the scale handed in must be the one the pending module returned
            return None
        if node.kind in ("linear", "conv"):
            s_a = host_of(node.scales[0])
            a8 = None
            if s_a is not None and s_a.size == 1:
                if node.kind == "conv":
                    a8 = _patchify_i8(node.mod, node.inputs[0])
                else:
                    a8 = q8_contig(node.inputs[0])
                    a8 = None if a8 is None else a8.reshape(-1, a8.shape[-1])
            if (a8 is not None and node.kind == "linear" and not x.views
                    and _frag_rows(linear_consts(node.mod, s_a, device), gemm_forms.RQ, a8.shape[0])):
                # not launched yet: if the next QuantAct adds a residual (Block.qact2 / qact4, vit_quant.py:147,153) the GEMM,
                # this requantisation and that one are ONE kernel; any other consumer launches the GEMM as it is
                rq = Requant(node.mod, a8, s_a, s_out, node.shape, s_out_qs, bits)
                if rq.ok:
                    return QT.wrap(x.shape, device, scale=s_out_qs, node=rq, fl=fl)
            o = gemm_requant(node.mod, a8, s_a, s_out, device, bits) if a8 is not None else None
            if o is not None:
                sh = node.shape
                out = o.view(*sh) if node.kind == "linear" else o.view(sh[0], sh[2], sh[3], sh[1]).permute(0, 3, 1, 2)
        elif node.kind == "ln":
            out = _resolve_ln(node, s_out, device)
        elif node.kind == "ibln":
            out = _resolve_ibert_ln(node, s_out, device)
        elif node.kind in ("gelu", "ibgelu"):
            out = _resolve_gelu(node, s_out, device)
        elif node.kind == "matmul":
            out = _resolve_attention(node, s_in, s_out, device)
            if out is None:      # the first matmul of the attention chain: stays pending as the Shiftmax input
                base = node.inputs[0]
                if isinstance(base, QT) and not x.views:
                    return QT.wrap(x.shape, device, node=Scores(x, pre_sf, s_out, s_out_qs, qact))
                if isinstance(base, QT) and isinstance(base.node, Probs) and (
                        base.node.mod.output_bit in (4, 16) or (type(base.node.mod).__name__ == "IBERTIntSoftmax"
                                                           and isinstance(base.node.x.node, (Biased, Masked)))):
                    # 4- or 16-bit probabilities without a fused kernel (I-BERT's softmax outside 193 .. 207 tokens, multipliers beyond
                    # the long-row kernels' bounds), or Swin's I-BERT softmax under a shift mask the window kernel cannot take
                    # (prepare.ibert_window_mask_ok): the attention core runs literally, its float result re-enters the integer
                    # stream here, so the rest of the forward is still carried
                    return resolve_float(qact, x.to_float(), pre_sf, s_out, s_out_qs)
    elif isinstance(node, Scaled) and identity is None and not x.views:
        return QT.wrap(x.shape, device, node=Scores(x, pre_sf, s_out, s_out_qs, qact))
    if out is None:
        return None
    STATS["fused"] += 1
    out = x.apply_views(out)
    return QT.wrap(out.shape, device, q8=out, scale=s_out_qs, fl=fl if tuple(fl.shape) == tuple(out.shape) else None)


def resolve_float(qact, x, pre_sf, s_out, s_out_qs):
    """The frozen 8-bit QuantAct on a float tensor whose scale is known on the host (Swin's qact3 behind the float pooling,
    swin_quant.py:554-555): round(x / s), the requantisation, int8 out -- nothing read back.  None: ordinary path."""
    s_in = host_of(pre_sf)
    if s_in is None or s_in.size != 1 or s_in[0] <= 0 or x.dtype != torch.float32 or x.dim() < 1:
        return None
    device = x.device
    m, e = dyadic(s_in, s_out)
    md, ed = _cache(qact, ("me", _key(s_in, np.asarray(s_out)), str(device)), lambda: (_dev(m.view(np.int32), device), _dev(e, device)))
    xin = x.contiguous()
    C = xin.shape[-1]
    z = torch.empty(xin.shape, dtype=torch.int32, device=device)
    _lib.call("ivit_f32_to_i32", _lib.ptr(xin), xin.numel() // C, C, _lib.ptr(pre_sf.as_subclass(torch.Tensor).reshape(-1)), 1, 0,
              _lib.ptr(z), _st())
    q = torch.empty_like(z)
    _lib.call("ivit_requant_i32", _lib.ptr(z), z.numel() // C, C, _lib.ptr(md), _lib.ptr(ed), 1, None, None, None, 0, 8, _lib.ptr(q), _st())
    STATS["fused"] += 1
    return QT.wrap(q.shape, device, q8=q.to(torch.int8), scale=s_out_qs, fl=act_layout(torch.empty_like(x, device="meta")))


def gemm_requant_i16(lin, a8, s_in, s_out, device):
    """a8 [M, K] int8 contiguous -> int16 [M, N]: GEMM + per-channel requantisation to the 16-bit scale s_out in one kernel; None
    outside the kernel's contract"""
    c = linear_consts(lin, s_in, device)
    me = _gemm_me(lin, s_in, s_out, device, need_e31=False)
    N, K = c["N"], c["K"]
    if N % 8:
        return None
    a8 = _operand(a8, c)
    M = a8.shape[0]
    o = torch.empty(M, N, dtype=torch.int16, device=device)
    _lib.call("ivit_gemm_i8_requant_i16", _lib.ptr(a8), K, _lib.ptr(c["W"]), K, _lib.ptr(c["b"]), _lib.ptr(me[0]), _lib.ptr(me[1]),
              _lib.ptr(o), N, M, N, K, _st())
    return o


def _frags32(lin, s_in, device, M):
    """linear_consts with "Wf32", the 32x32x32 fragment copy of the weight: the order the 16-bit-stream epilogue of
    ivit_gemm_i8_requant_i16_residual_i16_ex exists for (engine.py does the same for attn.proj / mlp.fc2), in 256-channel tiles
    where they fit (engine_common.frag_copy); None otherwise.  Built the first time a 16-bit QuantAct behind the linear asks with
    as many rows M as the weights-in-registers GEMM takes"""
    c = linear_consts(lin, s_in, device)
    if "Wf32" not in c and gemm_forms.frags_apply(gemm_forms.RQ16_RES16, M, c["N"], c["K"], gemm_forms.W_FRAGS):
        c["Wf32"] = frag_copy(c["W"], _st(), order16=False, narrow=False)[0] if c["K"] == c["Kin"] else None
    return c


def resolve16(qact, x, pre_sf, identity, identity_sf, s_out, s_out_qs):
    """The frozen 16-bit QuantAct on a QT, in the patterns of the Swin forward (swin_quant.py) and of ViT's 16-bit configurations
    (vit_quant.py:180-187): one launch -> int16 QT.
      int8 payload                                  -> ivit_requant_i8_i16               (Swin's qact1, :546)
      pending linear / patch convolution            -> ivit_gemm_i8_requant_i16          (attn.proj -> attn.qact4, :166; ViT's
                                                       patch_embed.qact, attn.qact3, mlp.qact2), where the rows reach the fragment
                                                       weight copy deferred (Requant16) for the residual QuantAct behind it
      cat(cls, int16 patches) + position identity   -> ivit_embed_assemble_i16           (ViT's qact1, vit_quant.py:293-297)
      int16 / int8 payload + int16 / int8 identity  -> ivit_residual_requant_i16         (the residual qact2, :291)
      deferred fc2 + mlp.qact2 (Requant) + identity -> ivit_gemm_i8_requant_residual_i16_ex   (the residual qact4, :297-299)
      deferred Requant16 + int16 identity           -> ivit_gemm_i8_requant_i16_residual_i16_ex   (ViT's residual qact2 / qact4)
    None: not one of these (ordinary path)."""
    device = x.device
    s_in = host_of(pre_sf)
    if s_in is None:
        return None
    fl = act_layout(x.fl, identity.fl if isinstance(identity, QT) else None)
    node = x.node
    out = None
    if isinstance(node, Cat) and x._q8 is None and x._q16 is None:
        if identity is None or x.views:
            return None
        out = _resolve_embed16(qact, node, s_in, identity, host_of(identity_sf), s_out, device)
    elif identity is not None:
        s_id = host_of(identity_sf)
        if (not isinstance(identity, QT) or s_id is None or s_id.size != 1 or s_in.size != 1
                or tuple(identity.shape) != tuple(x.shape)):
            return None
        i16 = q16_contig(identity)
        if i16 is None:
            i8 = q8_contig(identity)
            if i8 is None:
                return None
            i16 = torch.empty(i8.shape, dtype=torch.int16, device=device)      # an 8-bit stream (behind a PatchMerging): widened
            _lib.call("ivit_requant_i8_i16", _lib.ptr(i8), 1 << 30, 30, _lib.ptr(i16), i8.numel(), _st())
        C = x.shape[-1]
        (m1, e1), (m2, e2) = dyadic1(s_in, s_out), dyadic1(s_id, s_out)
        if isinstance(node, Requant) and x._q8 is None and not x.views and node.out is None:
            out = node.with_residual16(i16, s_in, (m1, e1, m2, e2), device)
        elif isinstance(node, Requant16) and x._q16 is None and not x.views and node.out is None:
            out = node.with_residual(i16, s_in, (m1, e1, m2, e2), device)
        if out is None:
            a = x.q
            if a is None or C % 4:
                return None
            a = a if a.is_contiguous() else a.contiguous()
            out = torch.empty(a.shape, dtype=torch.int16, device=device)
            _lib.call("ivit_residual_requant_i16", _lib.ptr(a), 8 * a.element_size(), None, None, m1, e1, _lib.ptr(i16), m2, e2, _lib.ptr(out),
                      a.numel() // C, C, 0, 0, 0, 0, _st())
    elif x.q8 is not None:
        if s_in.size != 1:
            return None
        a = q8_contig(x)
        m, e = dyadic1(s_in, s_out)
        out = torch.empty(a.shape, dtype=torch.int16, device=device)
        _lib.call("ivit_requant_i8_i16", _lib.ptr(a), m, e, _lib.ptr(out), a.numel(), _st())
    elif isinstance(node, ModNode) and node.kind in ("linear", "conv") and s_in is host_of(node.out_scale):
        s_a = host_of(node.scales[0])
        if s_a is None or s_a.size != 1:
            return None
        if node.kind == "conv":
            a8 = _patchify_i8(node.mod, node.inputs[0])
        else:
            a8 = q8_contig(node.inputs[0])
            a8 = None if a8 is None else a8.reshape(-1, a8.shape[-1])
        if a8 is None:
            return None
        if node.kind == "linear" and not x.views and _frag_rows(_frags32(node.mod, s_a, device, a8.shape[0]), gemm_forms.RQ16_RES16, a8.shape[0]):
            # not launched yet: if the next QuantAct adds the 16-bit residual (Block.qact2 / qact4 with attention_out_bw = mlp_out_bw =
            # norm2_in_bw = att_block_out_bw = 16, vit_quant.py:147,153) the GEMM, this requantisation and that one are ONE kernel;
            # any other consumer launches the GEMM as it is
            rq = Requant16(node.mod, a8, s_a, s_out, node.shape, s_out_qs)
            if rq.ok:
                return QT.wrap(x.shape, device, scale=s_out_qs, node=rq, fl=fl)
        o = gemm_requant_i16(node.mod, a8, s_a, s_out, device)
        if o is None:
            return None
        sh = node.shape
        out = x.apply_views(o.view(*sh) if node.kind == "linear" else o.view(sh[0], sh[2], sh[3], sh[1]).permute(0, 3, 1, 2))
    if out is None:
        return None
    STATS["fused"] += 1
    return QT.wrap(out.shape, device, q16=out, scale=s_out_qs, fl=fl if tuple(fl.shape) == tuple(out.shape) else None)


def _resolve_embed16(qact, node, s_in, identity, s_id, s_out, device):
    """qact1(cat(cls_token, patches), s, pos, s_pos) at 16 bits (vit_quant.py:293-297, block_input_bw = 16) on the int16 patch
    embedding: ivit_embed_assemble_i16, as engine.IntViTEngine launches it.  Its constants -- the position term
    RNE(k_pos * m2 / 2^e2) per (token, channel) and the finished class row -- are built once per (position payload, class token,
    scales) from one read-back of each at the warm-up forward.  None: anything but that pattern"""
    if (len(node.parts) != 2 or node.dim != 1 or s_in.size != 1 or s_id is None or s_id.size != 1 or not isinstance(identity, QT)
            or identity.q is None or identity.origin is None):
        return None
    cls, pe = node.parts
    if isinstance(cls, QT) or not isinstance(pe, QT) or pe.q16 is None or pe.dim() != 3 or cls.dtype != torch.float32:
        return None
    B, NP, C = pe.shape
    T = NP + 1
    if (tuple(cls.shape) != (B, 1, C) or (B > 1 and cls.stride(0) != 0) or tuple(identity.shape) != (1, T, C) or C % 8
            or B * T >= 2 ** 31 // C):
        return None

    def build():
        kpos = identity.q.reshape(T, C).cpu().numpy().astype(np.int64)
        m1, e1 = dyadic(s_in, s_out)
        m2, e2 = dyadic(s_id, s_out)
        pos_add = np.rint(kpos.astype(np.float64) * np.float64(m2[0]) / np.exp2(np.float64(e2[0])))      # quant_utils.py:229-230
        z_cls = np.rint((cls.detach()[0, 0].cpu().numpy().astype(f32) / f32(s_in[0])).astype(f32))     # :220 on the raw class row
        row = np.rint(z_cls.astype(np.float64) * np.float64(m1[0]) / np.exp2(np.float64(e1[0]))) + pos_add[0]
        if np.abs(pos_add).max() >= 2 ** 31:
            return None
        return (_dev(pos_add.astype(np.int32), device), _dev(np.clip(row, -32768, 32767).astype(np.int16), device), int(m1[0]), int(e1[0]))
    k = _cache(qact, ("embed16", identity.origin, _sig("cls", (cls,), {}), _key(s_in, s_id, np.asarray(s_out)), str(device)), build)
    if k is None:
        return None
    pe16 = q16_contig(pe)
    out = torch.empty(B, T, C, dtype=torch.int16, device=device)
    _lib.call("ivit_embed_assemble_i16", _lib.ptr(pe16), _lib.ptr(k[0]), _lib.ptr(k[1]), k[2], k[3], _lib.ptr(out), B, T, C, _st())
    return out


class Requant16(Node):
    """a linear + its 16-bit QuantAct, not launched yet (see resolve16)"""

    def __init__(self, lin, a8, s_a, s_out, shape, s_out_qs):
        self.lin, self.a8, self.s_a, self.s_out, self.shape, self.s_out_qs = lin, a8, s_a, s_out, shape, s_out_qs
        c = linear_consts(lin, s_a, a8.device)
        self.ok = c["N"] % 8 == 0 and c["K"] == c["Kin"]
        self.out = None

    def force(self):
        if self.out is None:
            STATS["fused"] += 1
            self.out = gemm_requant_i16(self.lin, self.a8, self.s_a, self.s_out, self.a8.device).view(*self.shape)
        return self.out

    def to_float(self):
        return self.force().to(torch.float32) * self.s_out_qs.as_subclass(torch.Tensor).reshape(-1)[0]

    def with_residual(self, i16, s_in, mes, device):
        """out = clamp16(RNE(clamp16(RNE(acc * M)) * m1 / 2^e1) + RNE(identity * m2 / 2^e2)): ivit_gemm_i8_requant_i16_residual_i16_ex
        with the fragment weight copy; int16 out, or None"""
        M = self.a8.shape[0]
        c = _frags32(self.lin, self.s_a, device, M)
        N, K = c["N"], c["K"]
        Wf, bit = gemm_forms.weight(c, gemm_forms.RQ16_RES16, M)
        if s_in[0] != f32(self.s_out) or tuple(i16.shape) != tuple(self.shape) or not bit & gemm_forms.FRAGS:
            return None
        me = _gemm_me(self.lin, self.s_a, self.s_out, device, need_e31=False)
        out = torch.empty(M, N, dtype=torch.int16, device=device)
        _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", _lib.ptr(self.a8), K, _lib.ptr(Wf), K, _lib.ptr(c["b"]), _lib.ptr(me[0]),
                  _lib.ptr(me[1]), _lib.ptr(i16), N, mes[0], mes[1], mes[2], mes[3], _lib.ptr(out), N, M, N, K, bit, _st())
        return out.view(*self.shape)


class Requant(Node):
    """a linear + its 8-bit (or, bits = 4, its 4-bit) QuantAct, not launched yet (see resolve)"""

    def __init__(self, lin, a8, s_a, s_out, shape, s_out_qs, bits=8):
        self.lin, self.a8, self.s_a, self.s_out, self.shape, self.s_out_qs, self.bits = lin, a8, s_a, s_out, shape, s_out_qs, bits
        self.ok = _gemm_me(lin, s_a, s_out, a8.device) is not None
        self.out = None

    def force(self):
        if self.out is None:
            STATS["fused"] += 1
            self.out = gemm_requant(self.lin, self.a8, self.s_a, self.s_out, self.a8.device, self.bits).view(*self.shape)
        return self.out

    def head_major(self, q, kT, v, head_dim=64, max_tokens=1025, frags=True):
        """q, k^T and v of vit_quant.py:66-70 as recorded views of THIS linear's output [B, N, 3 H hd]: the GEMM writes them head-major
        ([3, B, H, N, hd], what the attention kernel reads) itself -> that tensor; None if the views are anything else.
        frags = False (Swin's windows, head_dim 32): row-major weights where the fragment copy does not apply"""
        if self.out is not None or self.bits != 8 or len(self.shape) != 3 or any(t._q8 is not None or t.node is not self for t in (q, kT, v)):
            return None
        B, N, C3 = self.shape
        base = torch.empty(self.shape, dtype=torch.int8, device="meta")
        mq, mk, mv = q.apply_views(base), kT.apply_views(base).transpose(-2, -1), v.apply_views(base)
        if mq.dim() != 4:
            return None
        H, hd = mq.shape[1], mq.shape[3]
        C = H * hd
        if 3 * C != C3 or hd != head_dim or N > max_tokens or any(tuple(m.shape) != (B, H, N, hd) or m.stride() != (N * C3, hd, C3, 1)
                                                                 or m.storage_offset() != i * C for i, m in enumerate((mq, mk, mv))):
            return None
        device = self.a8.device
        c = linear_consts(self.lin, self.s_a, device)
        me = _gemm_me(self.lin, self.s_a, self.s_out, device)
        W, lay = gemm_forms.weight(c, gemm_forms.QKV, B * N)
        if (frags and not lay & gemm_forms.FRAGS) or c["Kin"] != C:
            return None
        hm = torch.empty(3, B, H, N, hd, dtype=torch.int8, device=device)
        _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(_operand(self.a8, c)), c["K"], _lib.ptr(W), c["K"],
                  _lib.ptr(c["b"]), _lib.ptr(me[0]), _lib.ptr(me[1]), _lib.ptr(hm), N, H, hd, B * N, C3, c["K"], lay, _st())
        STATS["fused"] += 1
        return hm

    def to_float(self):
        return self.force().to(torch.float32) * self.s_out_qs.as_subclass(torch.Tensor).reshape(-1)[0]

    def with_residual(self, identity, s_id, s_in, s_out2, device, bits_out=8):
        """out = clamp8(RNE(RNE(acc * M) * m1 / 2^e1) + RNE(identity * m2 / 2^e2)): ivit_gemm_i8_requant_residual_ex; with either of
        the two QuantActs at 4 bits ivit_gemm_i8_requant_residual_bits_ex"""
        i8 = q8_contig(identity)
        c = linear_consts(self.lin, self.s_a, device)
        N, K, M = c["N"], c["K"], self.a8.shape[0]
        Wf, lay = gemm_forms.weight(c, gemm_forms.RESID, M)
        if (i8 is None or s_id is None or s_id.size != 1 or s_in.size != 1 or s_in[0] != f32(self.s_out) or not lay & gemm_forms.FRAGS
                or tuple(i8.shape) != tuple(self.shape)):
            return None
        me = _gemm_me(self.lin, self.s_a, self.s_out, device)
        out = torch.empty(M, N, dtype=torch.int8, device=device)
        if self.bits == 8 and bits_out == 8:
            _lib.call("ivit_gemm_i8_requant_residual_ex", _lib.ptr(self.a8), K, _lib.ptr(Wf), K, _lib.ptr(c["b"]), _lib.ptr(me[0]),
                      _lib.ptr(me[1]), _lib.ptr(i8), N, *dyadic1(s_in, s_out2), *dyadic1(s_id, s_out2), _lib.ptr(out), N, M, N, K, lay, _st())
        else:
            _lib.call("ivit_gemm_i8_requant_residual_bits_ex", _lib.ptr(self.a8), K, _lib.ptr(Wf), K, _lib.ptr(c["b"]), _lib.ptr(me[0]),
                      _lib.ptr(me[1]), _lib.ptr(i8), N, *dyadic1(s_in, s_out2), *dyadic1(s_id, s_out2), _lib.ptr(out), N, M, N, K, lay,
                      self.bits, bits_out, _st())
        return out.view(*self.shape)

    def with_residual16(self, i16, s_in, mes, device):
        """mlp.fc2 + mlp.qact2 + the 16-bit residual QuantAct in one kernel (swin_engine.py does the same): int16 out, or None"""
        c = linear_consts(self.lin, self.s_a, device)
        N, K = c["N"], c["K"]
        if self.bits != 8 or s_in[0] != f32(self.s_out) or tuple(i16.shape) != tuple(self.shape) or N % 8:
            return None
        me = _gemm_me(self.lin, self.s_a, self.s_out, device)
        a8 = _operand(self.a8, c)
        M = a8.shape[0]
        # the fragment copy with a 16-bit-residual epilogue works in 256-channel tiles: where they fit (gemm_forms.frag_items_ok)
        W, lay = gemm_forms.weight(c, gemm_forms.RESID16, M)
        out = torch.empty(M, N, dtype=torch.int16, device=device)
        _lib.call("ivit_gemm_i8_requant_residual_i16_ex", _lib.ptr(a8), K, _lib.ptr(W), K, _lib.ptr(c["b"]),
                  _lib.ptr(me[0]), _lib.ptr(me[1]), _lib.ptr(i16), N, mes[0], mes[1], mes[2], mes[3], _lib.ptr(out), N, M, N, K,
                  lay, _st())
        return out.view(*self.shape)


class Scores(Node):
    """qact_attn1 on the (scaled) q . k^T: pending until Shiftmax and the second matmul arrive (vit_quant.py:72-82)"""

    def __init__(self, x, pre_sf, s_out, s_out_qs, qact):
        self.x, self.pre_sf, self.s_in, self.s_out, self.s_out_qs, self.qact = x, pre_sf, pre_sf.host, s_out, s_out_qs, qact

    def to_float(self):
        return self.qact._slow(self.x.to_float(), self.pre_sf)[0]


class Probs(Node):
    def __init__(self, scores_qt, mod):
        self.x, self.mod = scores_qt, mod

    def to_float(self):
        sc = self.x.node
        return self.mod._slow(self.x.to_float(), sc.s_out_qs)[0]


def _patchify_i8(conv, x):
    """[B, Cin, H, W] int8 QT -> the im2col operand [B * g * g, Cin * k * k] of the non-overlapping patch convolution"""
    x8 = x.q8 if isinstance(x, QT) else None
    if x8 is None:
        return None
    kh, kw = conv.kernel_size
    B, Cin, H, W = x8.shape
    if not (kh == kw == conv.stride[0] == conv.stride[1] and conv.padding == (0, 0) and H % kh == 0 and W % kw == 0):
        return None
    g, h = H // kh, W // kw
    return x8.reshape(B, Cin, g, kh, h, kw).permute(0, 2, 4, 1, 3, 5).reshape(B * g * h, Cin * kh * kw)


def _layernorm(ln, x, s_in, s_out, bits, device, outer=0, ibert=False):
    """LayerNorm (I-ViT's, or with `ibert` IBERTIntLayerNorm) of the contiguous `bits`-wide payload x + the QuantAct behind it ->
    int8: engine_common's ln_spec, cached per weights, scales and device, and its launcher.  None outside the kernels' contract"""
    def build():
        lp = LayerNormParams(ln.weight.detach().cpu().numpy(), ln.bias.detach().cpu().numpy(), s_out)
        return ln_spec(lp, lambda a: _dev(a, device), s_in[0], bits, float(ln.shift.reshape(-1)[0]) if ibert else None,
                       int_sqrt=ibert and bool(ln.use_int_sqrt))
    key = ("ibln", id(ln.shift), ln.shift._version, bool(ln.use_int_sqrt)) if ibert else ("ln", bits)
    try:
        spec = _cache(ln, key + (ln.weight._version, ln.bias._version, _key(s_in, s_out), str(device)), build)
    except ValueError:
        return None
    C = x.shape[-1]
    out = torch.empty(x.shape, dtype=torch.int8, device=device)
    layernorm(spec, x, C, x.numel() // C, C, out, C, _st(), blocks=False, outer=outer)
    return out


def _resolve_ln(node, s_out, device):
    ln, x = node.mod, node.inputs[0]
    s_in = host_of(node.scales[0])
    bits = int_width(x)
    outer = ln_outer(x.fl) if isinstance(x, QT) else None       # the reduction order follows the FLOAT tensor's layout
    if bits is None or outer is None or s_in is None or s_in.size != 1:
        return None
    return _layernorm(ln, int_payload(x), s_in, s_out, bits, device, outer=outer)


def _resolve_ibert_ln(node, s_out, device):
    """IBERTIntLayerNorm (ibert_modules.py:126-153) + the QuantAct behind it on int8 or on the int16 stream: ivit_ibert_layernorm_i8 /
    ivit_ibert_layernorm_i16_i8_ex (csrc/ibert.hip), which work on fl(q * s_in) literally -- any input scale; the module's
    use_int_sqrt goes with the launch as IVIT_IBERT_LN_INT_SQRT"""
    ln, x = node.mod, node.inputs[0]
    bits = int_width(x)
    s_in = host_of(node.scales[0])
    if bits is None or s_in is None or s_in.size != 1 or ln.overflow_handling:
        return None
    return _layernorm(ln, int_payload(x), s_in, s_out, bits, device, ibert=True)


def _resolve_gelu(node, s_out, device):
    """ShiftGELU ("gelu") or IBERTIntGELU ("ibgelu") + mlp.qact1: a gather from engine_common's gelu_lut"""
    x8 = q8_contig(node.inputs[0])
    s_g = host_of(node.scales[0])
    if x8 is None or s_g is None or s_g.size != 1:
        return None
    family = "ibert" if node.kind == "ibgelu" else "ivit"
    lut = _cache(node.mod, (node.kind, _key(s_g, s_out), str(device)),
                 lambda: gelu_lut(family, s_g[0], s_out, lambda a: _dev(a, device), device, _st())[0])
    L = x8.shape[-1]
    out = torch.empty_like(x8)
    _lib.call("ivit_shiftgelu_lut_i8_ex", _lib.ptr(x8), L, x8.numel() // L, L, _lib.ptr(lut), _lib.ptr(out), L, 0, _st())
    return out


def _resolve_attention(node, s_pv, s_out, device):
    """matmul_2(probs, v) behind qact2, where probs = Shiftmax(qact_attn1(matmul_1(q, k^T) * scale)): the fused attention kernel"""
    P, v = node.inputs
    if not (isinstance(P, QT) and isinstance(P.node, Probs) and not P.views and isinstance(v, QT)):
        return None
    sc_qt = P.node.x
    if isinstance(sc_qt.node, (Biased, Masked)):
        return _resolve_window_attention(P, sc_qt, v, s_pv, s_out, device)
    chain = _score_operands(sc_qt.node)
    if chain is None:
        return None
    sc, _, q, kT = chain
    hm = _head_major(q, kT, v, device)
    if hm is None:
        return None
    B, H, T, hd = hm.shape[1:]
    s_S, s_at = sc.s_in, sc.s_out
    if s_S.size != 1 or s_pv.size != 1:
        return None
    sm = P.node.mod
    if sm.output_bit not in (4, 8, 16):
        return None
    # softmax_bw = 16 (vit_quant.py:184): the "wide" entries, whose probabilities reach 2^15 at scale 2^-15 (s_pv is 2^-15 * s_v);
    # softmax_bw = 4: the same entries, probabilities below 8 (I-BERT: up to 8) at scale 2^-3
    softmax_bits = sm.output_bit if sm.output_bit in (4, 16) else None
    family, act, key = "ivit", None, ("attn",)
    if type(sm).__name__ == "IBERTIntSoftmax":
        # IBERTIntSoftmax (ibert_modules.py:237-319): exp_int after its internal 16-bit QuantAct as a (row max, q) table, row sum in
        # torch's float32 order inside the kernel (attention.hip MODE 3 / 4, attention_long_kernel MODE 2)
        if sm.act.running_stat:
            return None
        family, act = "ibert", sm.act
        key = ("ibattn", id(act.x_min), act.x_min._version, id(act.x_max), act.x_max._version)
    if attention_entry(family, T, softmax_bits) is None:      # token counts without a fused kernel stay literal
        return None

    def build():
        lo_hi = None if act is None else (float(act.x_min.reshape(-1)[0]), float(act.x_max.reshape(-1)[0]))
        d = attention_spec(family, s_S, s_at, s_pv, s_out, lambda a: _dev(a, device), device, _st(), lo_hi)
        if act is not None:
            act.act_scaling_factor = torch.full((1,), d["act_sf"], dtype=torch.float32, device=device)
        return d
    a = _cache(sc.qact, key + (_key(s_S, np.asarray(s_at), s_pv, np.asarray(s_out)), str(device)), build)
    # (4-bit probabilities: a row of many keys easily rounds to all zeros, and a calibration on such rows leaves qact2 no range)
    if (T > 207 or softmax_bits == 4) and not long_multipliers_ok(a):
        return None
    out = torch.empty(B * T, H * hd, dtype=torch.int8, device=device)
    attention(a, family, hm, out, B, H, T, hd, _st(), softmax_bits=softmax_bits)
    return out.view(B, T, H, hd).permute(0, 2, 1, 3)


def _score_operands(sc):
    """the walk from qact_attn1's pending node `sc` back to matmul_1: Scores -> (Scaled ->) matmul, where the scale the scores
    arrive with must be the matmul's s_q * s_k, times the model's factor -> (sc, matmul node, q, k^T), or None"""
    if not isinstance(sc, Scores):
        return None
    scaled = sc.x.node if isinstance(sc.x.node, Scaled) else None
    mm = scaled.x.node if scaled is not None else sc.x.node
    if not (isinstance(mm, ModNode) and mm.kind == "matmul") or (scaled is not None and scaled.x.views):
        return None
    s_mm = host_of(mm.out_scale)
    if s_mm is None or not np.array_equal(sc.s_in, s_mm if scaled is None else (s_mm * f32(scaled.c)).astype(f32)):
        return None
    q, kT = mm.inputs
    if not (isinstance(q, QT) and isinstance(kT, QT)):
        return None
    return sc, mm, q, kT


def _head_major(q, kT, v, device, head_dim=64, max_tokens=1025, frags=True):
    """q, k, v as the attention kernels read them, one int8 [3, B, H, N, hd]: written by the qkv GEMM itself (Requant.head_major),
    else three copies of the payloads; None if they are not [B, H, N, head_dim] payloads of at most max_tokens tokens"""
    hm = q.node.head_major(q, kT, v, head_dim=head_dim, max_tokens=max_tokens, frags=frags) if isinstance(q.node, Requant) else None
    if hm is None:
        if q.q8 is None or kT.q8 is None or v.q8 is None:
            return None
        q8, k8, v8 = q.q8, kT.q8.transpose(-2, -1), v.q8
        if q8.dim() != 4 or q8.shape != k8.shape or q8.shape != v8.shape or q8.shape[-1] != head_dim or q8.shape[-2] > max_tokens:
            return None
        hm = torch.empty(3, *q8.shape, dtype=torch.int8, device=device)
        hm[0].copy_(q8)
        hm[1].copy_(k8)
        hm[2].copy_(v8)
    return hm


def _mask_regions(mask, nW, N):
    """region ids [nW, N] of a float shift mask that is exactly where(region_i != region_j, -100, 0) (swin_quant.py:223-246), else
    None.  One read-back, at the warm-up forward."""
    if mask.numel() != nW * N * N:
        return None
    m = mask.detach().reshape(nW, N, N).cpu().numpy()
    if not np.all((m == 0) | (m == f32(-100.0))):
        return None
    same = m == 0
    region = np.argmax(same, axis=1)               # first token every token shares a region with
    if not np.array_equal(same, region[:, :, None] == region[:, None, :]):
        return None
    return region.astype(np.uint8)


def _resolve_window_attention(P, top, v, s_pv, s_out, device):
    """WindowAttention (swin_quant.py:137-161): matmul_1 -> * scale -> qact_attn1 -> qact2 with the relative position bias ->
    (+ mask) -> Shiftmax -> matmul_2 behind qact3, as one launch of the ivit_window_attention_i8* family, selected as
    swin_engine.IntSwinEngine selects it (window order out); with IBERTIntSoftmax(8) in Shiftmax's place (softmax_type='ibert'),
    ivit_window_attention_i8_ibert.  None -- the attention core then runs literally -- for any other softmax, and for a shift mask
    the I-BERT entry cannot take (prepare.ibert_window_mask_ok)"""
    from ..swin_engine import (HEAD_DIM, LONG_WINDOW, window_attention, window_attention_ibert, window_attention_ibert_spec,
                               window_attention_spec)
    sm = P.node.mod
    ibert = type(sm).__name__ == "IBERTIntSoftmax"
    if not (ibert or type(sm).__name__ == "IVITIntSoftmax") or sm.output_bit != 8 or (ibert and sm.act.running_stat):
        return None
    mask = None
    if isinstance(top.node, Masked):
        if not _reshapes_only(top.views):
            return None
        mask, biased = top.node.mask, top.node.x
    else:
        if top.views:
            return None
        biased = top
    bn = biased.node
    chain = None if bn.x.views else _score_operands(bn.x.node)
    if chain is None or not isinstance(chain[0].x.node, Scaled) or len(chain[2].shape) != 4:      # Swin always scales the scores
        return None
    sc, _, q, kT = chain
    B_, nH, N, hd = q.shape
    if hd != HEAD_DIM or not 2 <= N <= LONG_WINDOW or tuple(top.shape) != (B_, nH, N, N) or tuple(v.shape) != (B_, nH, N, hd):
        return None
    ws = int(round(N ** 0.5))
    if N > 64 and ws * ws != N and not ibert:
        return None
    nW = 1
    if mask is not None:
        nW = mask.shape[1]
        if tuple(mask.shape) != (1, nW, 1, N, N) or B_ % nW or tuple(biased.shape) != (B_ // nW, nW, nH, N, N):
            return None
    # ---- constants: once per (bias table version and path, mask tensor, ranges, device)
    ident = bn.identity
    s_S, s_at, s_tab, s_A = sc.s_in, sc.s_out, bn.s_id, bn.s_out
    mkey = None if mask is None else _sig("mask", (mask,), {})

    def build():
        i8 = ident.q8                          # the bias integers as the model code gathered them: read back once
        if i8 is None or i8.numel() != nH * N * N:
            return None
        bias = i8.reshape(nH, N, N).cpu().numpy().astype(np.int32)
        region = None
        if mask is not None:
            region = _mask_regions(mask, nW, N)
            if region is None:
                return None
        if ibert:      # the range of the softmax's internal 16-bit QuantAct from its frozen buffers, as _resolve_attention takes it
            act = sm.act
            spec = window_attention_ibert_spec(lambda a: _dev(a, device), device, _st(), bias, s_tab, s_S, s_at, s_A, s_pv, s_out, region, N,
                                               (float(act.x_min.reshape(-1)[0]), float(act.x_max.reshape(-1)[0])))
            if spec is not None:
                act.act_scaling_factor = torch.full((1,), spec["act_sf"], dtype=torch.float32, device=device)
            return spec
        spec, _ = window_attention_spec(lambda a: _dev(a, device), bias, s_tab, s_S, s_at, s_A, s_pv, s_out, region, N)
        return spec
    akey = (id(sm.act.x_min), sm.act.x_min._version, id(sm.act.x_max), sm.act.x_max._version) if ibert else ()
    a = _cache(bn.qact, ("wattn", ident.origin, mkey, _key(s_S, np.asarray(s_at), s_tab, np.asarray(s_A), s_pv, np.asarray(s_out)),
                         str(device)) + akey, build)
    if a is None:
        return None
    # ---- q, k, v head-major per window
    hm = _head_major(q, kT, v, device, head_dim=HEAD_DIM, max_tokens=LONG_WINDOW, frags=False)
    if hm is None:
        return None
    C = nH * hd
    out = torch.empty(B_ * N, C, dtype=torch.int8, device=device)
    # window order out; the long entry takes the windows' geometry regardless (one row of nW windows), the band entry none
    if ibert:
        window_attention_ibert(a, hm, out, C, B_, nW, nH, N, 0, 0, 0, 0, False, _st())
    else:
        geometry = (ws * nW, ws, ws, 0) if a["long"] else (0, 0, 0, 0)
        window_attention(a, hm, out, C, B_, nW, nH, N, *geometry, False, _st())
    return out.view(B_, N, nH, hd).permute(0, 2, 1, 3)


def _resolve_cat(qact, node, s_in, identity, identity_sf, s_out, device, bits=8):
    """qact1(cat(cls_token, patches), s, pos, s_pos) (vit_quant.py:293-297): the raw float rows go through round(x / s), the
    int8 part is widened, then the two-operand requantisation"""
    s_id = host_of(identity_sf)
    if s_in.size != 1 or node.dim != 1 or (identity is not None and (s_id is None or s_id.size != 1)):
        return None
    parts = []
    for p in node.parts:
        if isinstance(p, QT):
            if p.q8 is None:          # an int16 patch embedding in front of an 8-bit block input: not a pattern
                return None
            parts.append(p.q8.to(torch.int32))
        else:
            pf = p.detach()
            z = torch.round(pf.to(torch.float32) / float(s_in[0])).to(torch.int32)      # quant_utils.py:220
            parts.append(z)
    z = torch.cat(parts, dim=1).contiguous()
    C = z.shape[-1]
    m, e = dyadic(s_in, s_out)
    md, ed = _cache(qact, ("me", _key(s_in, np.asarray(s_out)), str(device)), lambda: (_dev(m.view(np.int32), device), _dev(e, device)))
    z2 = m2d = e2d = None
    n2 = 0
    if identity is not None:
        i8 = identity.q8 if isinstance(identity, QT) else None
        if i8 is None:
            return None
        z2 = i8.to(torch.int32).expand_as(z).contiguous()
        m2, e2 = dyadic(s_id, s_out)
        m2d, e2d = _cache(qact, ("me2", _key(s_id, np.asarray(s_out)), str(device)), lambda: (_dev(m2.view(np.int32), device), _dev(e2, device)))
        n2 = 1
    q = torch.empty_like(z)
    _lib.call("ivit_requant_i32", _lib.ptr(z), z.numel() // C, C, _lib.ptr(md), _lib.ptr(ed), 1, _lib.ptr(z2), _lib.ptr(m2d),
              _lib.ptr(e2d), n2, bits, _lib.ptr(q), _st())
    return q.to(torch.int8)


def linear_to_float(lin, x, s_in_qs):
    """a pending linear read as floats (the classifier head): int32 GEMM, then acc * s_acc"""
    a8 = q8_contig(x)
    s_in = host_of(s_in_qs)
    if a8 is None or s_in is None or s_in.size != 1:
        return None
    c = linear_consts(lin, s_in, a8.device)
    N, K = c["N"], c["K"]
    Np = (N + 3) // 4 * 4
    W, b = c["W"], c["b"]
    if Np != N:          # the GEMM wants N % 4 == 0: zero rows, sliced off again below (as QuantLinear._params does)
        if "Wp" not in c:
            c["Wp"] = torch.cat([W, torch.zeros(Np - N, K, dtype=W.dtype, device=W.device)])
            c["bp"] = None if b is None else torch.cat([b, torch.zeros(Np - N, dtype=b.dtype, device=b.device)])
        W, b = c["Wp"], c["bp"]
    a2 = _operand(a8.reshape(-1, c["Kin"]), c)
    acc = torch.empty(a2.shape[0], Np, dtype=torch.int32, device=a8.device)
    _lib.call("ivit_gemm_i8_i32", _lib.ptr(a2), K, _lib.ptr(W), K, _lib.ptr(b), _lib.ptr(acc), Np, a2.shape[0], Np, K, _st())
    if Np != N:
        acc = acc[:, :N].contiguous()
    y = torch.empty(acc.shape, dtype=torch.float32, device=a8.device)
    s = c["s_acc"].as_subclass(torch.Tensor)
    _lib.call("ivit_i32_to_f32", _lib.ptr(acc), acc.shape[0], N, _lib.ptr(s), N, _lib.ptr(y), _st())
    return y.view(*x.shape[:-1], N)
