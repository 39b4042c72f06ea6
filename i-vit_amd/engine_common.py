"""Host code shared by the fused engines (engine.IntViTEngine, swin_engine.IntSwinEngine) and the module path
(quantization_utils/lazy.py): device uploads, the LayerNorm specs and their one launcher, and the GEMM weight copies."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .graph import GraphReplay
from .prepare import IMAGENET_MEAN, IMAGENET_STD, input_lut_u8, markstein_division_ok, phi_is_identity, phi_tables
from .topk import HeadTopK


def _np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


# ----------------------------------------------------------------------------------------------------------- GEMM weights
def block_copy(W: torch.Tensor, st):
    """Block-layout copy of a row-major int8 weight [N, K] (include/ivit_hip.h IVIT_LAYOUT_BLOCKS): the persistent GEMM then
    reads 1 KB contiguous per LDS-DMA instruction instead of 16 half cache lines.  None where block operands do not apply."""
    N, K = W.shape
    if K % 64 or N % 16 or N < 128:
        return None
    Wb = torch.empty_like(W)
    _lib.call("ivit_tile_operand_i8", _lib.ptr(W), K, N, K, _lib.ptr(Wb), st)
    return Wb


def frag_copy(W: torch.Tensor, st, order16: bool = True, narrow: bool = True):
    """MFMA-fragment copy of a row-major int8 weight [N, K] for the weights-in-registers GEMM -> (Wf, Wf_bit), or (None, None).
    order16: the v_mfma_i32_16x16x64_i8 order (IVIT_W_FRAGS16; the chip holds a higher clock on that shape), else the
    32x32x32 one (IVIT_W_FRAGS).  narrow: the consuming epilogue can use 128-channel work items.

    The kernel needs K % 192 == 0, N % 64 == 0 and N >= 128.  Its 128-channel work items exist only for the 16x16x64 order
    with an int8 epilogue; every other consumer (the 32x32x32 order, a 16-bit-residual epilogue) works in 256-channel tiles,
    which are used only where they waste at most an eighth of their columns."""
    N, K = W.shape
    if K % 192 or N % 64 or N < 128 or not ((narrow and order16) or (N + 255) // 256 * 256 * 8 <= N * 9):
        return None, None
    Wf = torch.empty((N + 63) // 64 * 64 * K, dtype=torch.int8, device=W.device)
    _lib.call("ivit_pack_weight_frags16_i8" if order16 else "ivit_pack_weight_frags_i8", _lib.ptr(W), K, N, K, _lib.ptr(Wf), st)
    return Wf, 16 if order16 else 8


# ----------------------------------------------------------------------------------------------------------- LayerNorm
def ln_spec(lp, upload, s_in, bits: int, ibert_shift=None) -> dict:
    """Device constants of one LayerNorm (prepare.LayerNormParams `lp`) on a `bits`-wide input of scale s_in, with its
    `kind`: "i8" / "i16" (I-LayerNorm on integers); "i8_compat" / "i16_compat" (natural input scale: the reference's
    operator sees fl(fl(q * s_in) / s_in), not q -- the table form on 8 bits, the literal / Markstein-quotient form on 16);
    "ibert_i8" / "ibert_i16" (ibert_shift given: IBERTIntLayerNorm, the same per-channel constants plus its overflow shift
    buffer, ibert_modules.py:134-153; the kernel works on fl(q * s_in) literally)."""
    d = dict(bias=upload(lp.bias_int), s=upload(lp.s_ln), m=upload(lp.m.view(np.int32)), e=upload(lp.e))
    if ibert_shift is not None:
        d.update(kind=f"ibert_i{bits}", s_in=float(s_in), shift_pow2=float(2.0 ** ibert_shift))
        if bits == 16:
            d["fast_div"] = int(markstein_division_ok(s_in, 16))
    elif phi_is_identity(s_in, bits):
        d["kind"] = f"i{bits}"
    elif bits == 16:
        d.update(kind="i16_compat", s_in=float(s_in), fast_div=int(markstein_division_ok(s_in, 16)))
    else:
        remap, phi = phi_tables(s_in)
        d.update(kind="i8_compat", remap=upload(remap), phi=upload(phi))
    return d


def layernorm(ln, x, ldx, rows, C, out, ldo, st, blocks=None, H=0, W=0, ws=0, shift=0, outer=0):
    """LayerNorm + requantisation of `rows` rows of x to int8, for every kind of ln_spec.
    blocks: the int8-input kinds write `out` in the block layout (None: the "i8" kind goes through the entry point without a
    layout argument).  H, W, ws, shift: the Swin window map of the 16-bit kinds (0: rows in order).  outer:
    IVIT_LN_OUTER_MEAN(outer) of the compat kinds -- the float32 mean in torch's outer-reduction order."""
    kind, p = ln["kind"], _lib.ptr
    bias, s, m, e = p(ln["bias"]), p(ln["s"]), p(ln["m"]), p(ln["e"])
    if kind == "i8" and blocks is None:
        _lib.call("ivit_layernorm_i8", p(x), ldx, rows, C, bias, s, m, e, p(out), ldo, st)
    elif kind == "i8":
        _lib.call("ivit_layernorm_i8_ex", p(x), ldx, rows, C, bias, s, m, e, p(out), ldo, int(blocks), st)
    elif kind == "i8_compat":
        _lib.call("ivit_layernorm_i8_compat", p(x), ldx, rows, C, bias, s, m, e, p(ln["remap"]), p(ln["phi"]), p(out), ldo,
                  int(blocks or 0) | (outer << 8), st)
    elif kind == "ibert_i8":
        _lib.call("ivit_ibert_layernorm_i8", p(x), ldx, rows, C, ln["s_in"], bias, s, ln["shift_pow2"], m, e, p(out), ldo,
                  int(blocks or 0), st)
    elif kind == "ibert_i16":
        _lib.call("ivit_ibert_layernorm_i16_i8_ex", p(x), ldx, rows, C, ln["s_in"], bias, s, ln["shift_pow2"], m, e, p(out), ldo,
                  ln["fast_div"], st)
    elif kind == "i16_compat":
        _lib.call("ivit_layernorm_i16_i8_compat", p(x), rows, C, ln["s_in"], ln["fast_div"] | (outer << 8), bias, s, m, e, p(out),
                  ldo, H, W, ws, shift, st)
    elif kind == "i16":
        _lib.call("ivit_layernorm_i16_i8", p(x), rows, C, bias, s, m, e, p(out), ldo, H, W, ws, shift, st)
    else:
        raise ValueError(f"LayerNorm kind {kind!r}")


# ----------------------------------------------------------------------------------------------------------- engines
class EngineBase(GraphReplay, HeadTopK):
    """What IntViTEngine and IntSwinEngine share beyond their mixins.  Subclasses set self.dev, self.s0, self.input_lut and
    self.natural_sites."""

    def _stream(self):
        return _lib.stream_ptr()

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _ln_spec(self, lp, s_in, bits, ibert_shift=None):
        d = ln_spec(lp, self._upload, s_in, bits, ibert_shift)
        self.natural_sites += int(d["kind"].endswith("_compat"))
        return d

    def set_input_normalisation(self, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """uint8 input: the (mean, std) of the Normalize transform in front of the model (default: ImageNet's).  forward() then
        accepts uint8 [B,3,H,W] pixel tensors -- a quarter of the bytes of the float32 input -- and quantises them through a
        3 x 256 table that holds the float pipeline's result per (channel, pixel value): same integers as the float path."""
        self.input_lut = torch.from_numpy(input_lut_u8(self.s0, mean, std)).to(self.dev)
        self.input_norm = (tuple(float(v) for v in mean), tuple(float(v) for v in std))   # what the table was built for
