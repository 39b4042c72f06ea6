"""Host code shared by the fused engines (engine.IntViTEngine, swin_engine.IntSwinEngine) and the module path
(quantization_utils/lazy.py), written once per operator: the GEMM weight copies (block_copy, frag_copy); the LayerNorm constants
and their launchers (ln_spec, layernorm; layernorm_f32: the float32 output of the same kinds, forward_tokens); the ViT attention constants and their launchers (attention_spec, attention,
attention_probs: the probabilities alone); the GELU
table of both families (gelu_lut); the feature-map launcher and its index check (tokens_to_nchw, intermediate_indices); the
embedding's dequantisation (dequant_rows); what the two engines share as classes (EngineBase: the headless refusal and
forward_features' destination among it).  Window attention's pair
(window_attention_spec, window_attention) lives in swin_engine.py; the scalar dyadic pair is prepare.dyadic1."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, gemm_forms
from .graph import GraphReplay
from .prepare import (IMAGENET_MEAN, IMAGENET_STD, dyadic1, f32, input_lut_u8, markstein_division_ok, phi_is_identity, phi_tables,
                      shiftexp2d, shiftexp_band)
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
    if not gemm_forms.blocks_shape(N, K):
        return None
    Wb = torch.empty_like(W)
    _lib.call("ivit_tile_operand_i8", _lib.ptr(W), K, N, K, _lib.ptr(Wb), st)
    return Wb


def frag_copy(W: torch.Tensor, st, order16: bool = True, narrow: bool = True):
    """MFMA-fragment copy of a row-major int8 weight [N, K] for the weights-in-registers GEMM -> (Wf, Wf_bit), or (None, None).
    order16: the v_mfma_i32_16x16x64_i8 order (IVIT_W_FRAGS16; the chip holds a higher clock on that shape), else the
    32x32x32 one (IVIT_W_FRAGS).  narrow: the consuming epilogue can use 128-channel work items.

    Where the kernel takes the weight at all (gemm_forms.frags_shape) and its work items fit N (gemm_forms.frag_items_ok)."""
    N, K = W.shape
    bit = gemm_forms.W_FRAGS16 if order16 else gemm_forms.W_FRAGS
    if not (gemm_forms.frags_shape(N, K) and gemm_forms.frag_items_ok(bit, narrow, N)):
        return None, None
    Wf = torch.empty((N + 63) // 64 * 64 * K, dtype=torch.int8, device=W.device)
    _lib.call("ivit_pack_weight_frags16_i8" if order16 else "ivit_pack_weight_frags_i8", _lib.ptr(W), K, N, K, _lib.ptr(Wf), st)
    return Wf, bit


# ----------------------------------------------------------------------------------------------------------- LayerNorm
IBERT_LN_INT_SQRT = 0x100     # IVIT_IBERT_LN_INT_SQRT of include/ivit_hip.h


def ln_spec(lp, upload, s_in, bits: int, ibert_shift=None, int_sqrt: bool = False) -> dict:
    """Device constants of one LayerNorm (prepare.LayerNormParams `lp`) on a `bits`-wide input of scale s_in, with its
    `kind`: "i8" / "i16" (I-LayerNorm on integers); "i8_compat" / "i16_compat" (natural input scale: the reference's
    operator sees fl(fl(q * s_in) / s_in), not q -- the table form on 8 bits, the literal / Markstein-quotient form on 16);
    "ibert_i8" / "ibert_i16" (ibert_shift given: IBERTIntLayerNorm, the same per-channel constants plus its overflow shift
    buffer, ibert_modules.py:134-153; the kernel works on fl(q * s_in) literally; int_sqrt: its use_int_sqrt = True form, std from
    integer_sqrt, carried as `flags` = IVIT_IBERT_LN_INT_SQRT)."""
    if int_sqrt and ibert_shift is None:
        raise ValueError("int_sqrt is a parameter of IBERTIntLayerNorm (ibert_shift)")
    d = dict(bias=upload(lp.bias_int), s=upload(lp.s_ln), m=upload(lp.m.view(np.int32)), e=upload(lp.e))
    if ibert_shift is not None:
        d.update(kind=f"ibert_i{bits}", s_in=float(s_in), shift_pow2=float(2.0 ** ibert_shift),
                 flags=IBERT_LN_INT_SQRT if int_sqrt else 0)
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
    layout argument).  H, W, ws, shift: the Swin window map of the 16-bit kinds, "ibert_i16" included (0: rows in order).  outer:
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
                  int(blocks or 0) | ln["flags"], st)
    elif kind == "ibert_i16" and ws:
        _lib.call("ivit_ibert_layernorm_i16_i8_win", p(x), ldx, rows, C, ln["s_in"], bias, s, ln["shift_pow2"], m, e, p(out), ldo,
                  ln["fast_div"] | ln["flags"], H, W, ws, shift, st)
    elif kind == "ibert_i16":
        _lib.call("ivit_ibert_layernorm_i16_i8_ex", p(x), ldx, rows, C, ln["s_in"], bias, s, ln["shift_pow2"], m, e, p(out), ldo,
                  ln["fast_div"] | ln["flags"], st)
    elif kind == "i16_compat":
        _lib.call("ivit_layernorm_i16_i8_compat", p(x), rows, C, ln["s_in"], ln["fast_div"] | (outer << 8), bias, s, m, e, p(out),
                  ldo, H, W, ws, shift, st)
    elif kind == "i16":
        _lib.call("ivit_layernorm_i16_i8", p(x), rows, C, bias, s, m, e, p(out), ldo, H, W, ws, shift, st)
    else:
        raise ValueError(f"LayerNorm kind {kind!r}")


LN_F32_CHANNEL_MAJOR, LN_F32_FAST_DIV = 1, 2     # IVIT_LN_F32_* of include/ivit_hip.h
TOKEN_FORMATS = ("NLC", "NCHW")


def token_format(fmt):
    """forward_tokens' `fmt`, checked: ValueError for anything but "NLC" / "NCHW" """
    if fmt not in TOKEN_FORMATS:
        raise ValueError(f"fmt={fmt!r}: 'NLC' (tokens as rows) or 'NCHW' (channels first, the patch grid)")
    return fmt


def layernorm_f32(ln, x, ldx, B, T_all, t0, T, C, out, ldo, st, fmt="NLC"):
    """The LayerNorm's own float32 output (the tensor the module returns, y_int * s_ln) for every kind of ln_spec, straight from
    the integer stream x (element (b, t, c) at (b * T_all + t) * ldx + c), tokens t0 .. t0 + T - 1 of each of the B images.
    fmt "NLC": out[(b * T + t) * ldo + c]; "NCHW": out[(b * C + c) * ldo + t] (ldo = T: dense [B, C, T]).  One launch
    (ivit_layernorm_i8_f32 / _i16_f32, ivit_ibert_layernorm_i8_f32 / _i16_f32: csrc/ln_tokens.h)."""
    kind, p = ln["kind"], _lib.ptr
    flags = LN_F32_CHANNEL_MAJOR if token_format(fmt) == "NCHW" else 0
    sel, bias, s = (p(x), ldx, B, T_all, t0, T, C), p(ln["bias"]), p(ln["s"])
    if kind == "i8":
        _lib.call("ivit_layernorm_i8_f32", *sel, bias, s, None, None, p(out), ldo, flags, st)
    elif kind == "i8_compat":
        _lib.call("ivit_layernorm_i8_f32", *sel, bias, s, p(ln["remap"]), p(ln["phi"]), p(out), ldo, flags, st)
    elif kind == "i16":
        _lib.call("ivit_layernorm_i16_f32", *sel, 0.0, bias, s, p(out), ldo, flags, st)
    elif kind == "i16_compat":
        _lib.call("ivit_layernorm_i16_f32", *sel, ln["s_in"], bias, s, p(out), ldo, flags | (LN_F32_FAST_DIV if ln["fast_div"] else 0), st)
    elif kind == "ibert_i8":
        _lib.call("ivit_ibert_layernorm_i8_f32", *sel, ln["s_in"], bias, s, ln["shift_pow2"], p(out), ldo, flags | ln["flags"], st)
    elif kind == "ibert_i16":
        _lib.call("ivit_ibert_layernorm_i16_f32", *sel, ln["s_in"], bias, s, ln["shift_pow2"], p(out), ldo,
                  flags | ln["flags"] | (LN_F32_FAST_DIV if ln["fast_div"] else 0), st)
    else:
        raise ValueError(f"LayerNorm kind {kind!r}")


# ----------------------------------------------------------------------------------------------------------- ViT attention
def attention_spec(family, s_S, s_at, s_pv, s_out, upload, device, st, ibert_range=None) -> dict:
    """Device constants of one fused ViT attention (vit_quant.py:72-82).  s_S: the scale the scores arrive with, s_at that of
    qact_attn1, s_pv / s_out those around qact2.  -> ms, mo (the two requantisations), s_attn, and Softmax's exponent as a table
    where it needs one:
      family "ivit", natural s_at: Shiftmax on phi(q), tabulated over (row max, q) -- `band` / `band_w` (rows staged in LDS per query
        tile, 34 KB per workgroup at width 128) when the exponent saturates within 128 steps of the row maximum, else `exp2d`, the
        full-table gather of a very fine input scale;
      family "ibert": IBERTIntSoftmax (output_bit 8, scale 2 / 2^8 = 2^-7 like Shiftmax's) -- exp_int after its internal 16-bit
        QuantAct of range ibert_range = (x_min, x_max), tabulated over (row max, q) with the reference's float32 sequence
        (csrc/ibert.hip) in `ib_table`, its band form as above, and `act_sf`, that QuantAct's scale."""
    d = dict(ms=dyadic1(s_S, s_at), s_attn=float(s_at), mo=dyadic1(s_pv, s_out), exp2d=None, band=None, band_w=0)
    if family == "ibert":
        from .quantization_utils.ibert_modules import softmax_constants
        x0i, bi, ci, exp_sf, act_sf, ma, ea = softmax_constants(s_at, *ibert_range)
        tab = torch.empty(65536, dtype=torch.float32, device=device)
        _lib.call("ivit_ibert_softmax_build_table", float(s_at), x0i, bi, ci, float(exp_sf), float(act_sf), ma, ea, _lib.ptr(tab), st)
        d.update(ib_table=tab, act_sf=float(act_sf))
        band, bw = shiftexp_band(tab.cpu().numpy().view(np.uint32).reshape(256, 256))
        if bw and bw <= 128:
            d.update(band=upload(band.view(np.float32)), band_w=bw)
    elif phi_tables(s_at) is not None:
        tab = shiftexp2d(s_at)
        band, bw = shiftexp_band(tab)
        if bw and bw <= 128:
            d.update(band=upload(band.view(np.int32)), band_w=bw)
        else:
            d["exp2d"] = upload(tab.view(np.int32))
    return d


def attention_entry(family, T, softmax_bits=None):
    """The fused attention entry that serves rows of T tokens, or None where no fused kernel exists: the one Python statement of the
    token ranges of csrc/attention.hip.  Shiftmax ("ivit"): the short kernels up to 207 tokens, the long-row ones 208 .. 1025.
    I-BERT: 193 .. 207 short, 208 .. 1025 long.  softmax_bits: given where the softmax output may be 16 bits wide (the 16-bit stream
    of the engine, a 16-bit softmax on the module path): the "wide" entries, which take it before the layout flag; I-BERT's softmax
    has no wide long-row kernel."""
    wide, long = softmax_bits is not None, T > 207
    if family == "ibert":
        if not 193 <= T <= 1025 or (wide and long):
            return None
        return "ivit_attention_fused_i8_ibert_wide" if wide else "ivit_attention_fused_i8_ibert_long" if long else "ivit_attention_fused_i8_ibert"
    if not 1 <= T <= 1025:
        return None
    return ("ivit_attention_fused_i8_wide_long" if wide and long else "ivit_attention_fused_i8_wide" if wide else
            "ivit_attention_fused_i8_long" if long else "ivit_attention_fused_i8_compat_band")


def long_multipliers_ok(a):
    """the long-row kernels' bounds on the two requantisation multipliers of an attention_spec (score < 2048, output < 512).  A model
    whose attention output range collapsed in calibration (all probabilities 0) breaks the second; such rows ran the literal path
    before the long-row kernels were routed to the module path and still do"""
    return a["ms"][0] / 2.0 ** a["ms"][1] < 2048.0 and a["mo"][0] / 2.0 ** a["mo"][1] < 512.0


def attention(a, family, qkv, out, B, H, T, hd, st, blocks=False, softmax_bits=None):
    """Fused attention of an attention_spec `a` on head-major qkv [3, B, H, T, hd] -> out [B * T, H * hd] (`blocks`: in the block
    layout) through attention_entry's kernel (the same arguments for short and long rows).  No entry: an error, nothing is
    launched."""
    p, name = _lib.ptr, attention_entry(family, T, softmax_bits)
    if name is None:
        raise NotImplementedError(f"no fused {'I-BERT' if family == 'ibert' else 'Shiftmax'} attention for these rows "
                                  f"(softmax_bits={softmax_bits}, tokens={T})")
    sm = () if softmax_bits is None else (softmax_bits,)
    if family == "ibert":
        _lib.call(name, p(qkv), p(out), B, H, T, hd, a["ms"][0], a["ms"][1], a["mo"][0], a["mo"][1], p(a["ib_table"]), p(a["band"]),
                  a["band_w"], *sm, int(blocks), st)
    else:
        _lib.call(name, p(qkv), p(out), B, H, T, hd, a["ms"][0], a["ms"][1], a["s_attn"], a["mo"][0], a["mo"][1], p(a["exp2d"]),
                  p(a["band"]), a["band_w"], *sm, int(blocks), st)


def attention_probs(a, family, qkv, probs, B, H, T, hd, q_rows, st):
    """The softmax probabilities of an attention_spec `a` on head-major qkv [3, B, H, T, hd] -> probs uint8 [B, H, q_rows, T]
    (dense), scale 2^-7: the P that attention()'s kernel multiplies with V, for the first q_rows queries of every (image, head).
    One launch; any T in 1 .. 1025 for both families (8-bit softmax output only)."""
    p = _lib.ptr
    if family == "ibert":
        _lib.call("ivit_attention_probs_u8_ibert", p(qkv), p(probs), T, B, H, T, hd, q_rows, a["ms"][0], a["ms"][1],
                  p(a["ib_table"]), p(a["band"]), a["band_w"], st)
    else:
        _lib.call("ivit_attention_probs_u8", p(qkv), p(probs), T, B, H, T, hd, q_rows, a["ms"][0], a["ms"][1], a["s_attn"],
                  p(a["exp2d"]), p(a["band"]), a["band_w"], st)


# ----------------------------------------------------------------------------------------------------------- GELU
def gelu_lut(family, s_g, s_m1, upload, device, st):
    """The 65536-entry table ivit_shiftgelu_lut_i8* gathers from: GELU on an int8 input of scale s_g + the QuantAct behind it
    (mlp.qact1, scale s_m1).  -> (lut, natural).  family "ivit": ShiftGELU, which sees trunc(phi(q)) at a natural s_g
    (ivit_modules.py:106-107; `natural`) and has the output scale s_g / 128 (:121,124).  family "ibert": IBERTIntGELU + mlp.qact1
    depend on q alone -- one 256-entry map, replicated over the table's row-max axis; its output scale is negative
    (ibert_modules.py:213, 232): requant(z, s) == requant(-z, -s) (quant_modules.QuantAct)."""
    lut = torch.empty(65536, dtype=torch.int8, device=device)
    if family == "ibert":
        from .quantization_utils.ibert_modules import gelu_constants
        gb, gc, gsh, gso = gelu_constants(s_g)
        mg, eg = dyadic1(abs(f32(gso)), s_m1)
        _lib.call("ivit_ibert_gelu_build_lut", float(s_g), gb, gc, gsh, float(gso), mg, eg, _lib.ptr(lut), st)
        return lut, False
    mg, eg = dyadic1(f32(s_g * f32(1.0 / 128.0)), s_m1)
    t = phi_tables(s_g)
    _lib.call("ivit_shiftgelu_build_lut_ex", float(s_g), mg, eg, _lib.ptr(None if t is None else upload(t[0])), _lib.ptr(lut), st)
    return lut, t is not None


# ----------------------------------------------------------------------------------------------------------- feature maps
def tokens_to_nchw(x, ldx, B, T_all, t0, T, C, scale, out, st):
    """Tokens t0 .. t0 + T - 1 of a token-major integer stream x (int8 / int16, element (b, t, c) at (b * T_all + t) * ldx + c) ->
    out, dense [B, C, T] (a [B, C, H, W] tensor): float32 out = q * scale in one float32 multiplication, or -- an out of x's own
    dtype -- the integers.  One launch (ivit_tokens_to_nchw_*, csrc/features.hip)."""
    name = {(torch.int8, torch.float32): "ivit_tokens_to_nchw_i8_f32", (torch.int16, torch.float32): "ivit_tokens_to_nchw_i16_f32",
            (torch.int8, torch.int8): "ivit_tokens_to_nchw_i8", (torch.int16, torch.int16): "ivit_tokens_to_nchw_i16"}[(x.dtype, out.dtype)]
    assert out.is_contiguous() and out.numel() == B * C * T
    if out.dtype == torch.float32:
        _lib.call(name, _lib.ptr(x), ldx, B, T_all, t0, T, C, float(scale), _lib.ptr(out), st)
    else:
        _lib.call(name, _lib.ptr(x), ldx, B, T_all, t0, T, C, _lib.ptr(out), st)


def dequant_rows(x, ldx, rows, C, scale, out, ldo, st):
    """rows x C int8 integers with row stride ldx -> float32 out with row stride ldo (both in elements), out = q * scale in one
    float32 multiplication: the tensor a QuantAct returns.  One launch (ivit_dequant_rows_i8_f32, csrc/features.hip)."""
    assert x.dtype == torch.int8 and out.dtype == torch.float32
    _lib.call("ivit_dequant_rows_i8_f32", _lib.ptr(x), ldx, rows, C, float(scale), _lib.ptr(out), ldo, st)


def intermediate_indices(indices, n, what):
    """forward_intermediates' `indices` (None: all of 0 .. n - 1) as a list; ValueError for one out of range or repeated"""
    idx = list(range(n)) if indices is None else [int(i) for i in indices]
    if any(not 0 <= i < n for i in idx) or len(set(idx)) != len(idx):
        raise ValueError(f"indices {idx}: distinct {what} indices in 0..{n - 1}")
    return idx


# ----------------------------------------------------------------------------------------------------------- engines
class EngineBase(GraphReplay, HeadTopK):
    """What IntViTEngine and IntSwinEngine share beyond their mixins.  Subclasses set self.dev, self.s0, self.input_lut and
    self.natural_sites."""

    def _stream(self):
        return _lib.stream_ptr()

    def _upload(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _ln_spec(self, lp, s_in, bits, ibert_shift=None, int_sqrt=False):
        d = ln_spec(lp, self._upload, s_in, bits, ibert_shift, int_sqrt)
        self.natural_sites += int(d["kind"].endswith("_compat"))
        return d

    def _gelu_lut(self, family, s_g, s_m1):
        lut, natural = gelu_lut(family, s_g, s_m1, self._upload, self.dev, self._stream())
        self.natural_sites += int(natural)
        return lut

    def _require_head(self, what):
        """the calls that end in the classifier, on an engine built from a source without head.weight: refused before any launch"""
        if self.head is None:
            raise ValueError(f"{what}: this engine has no classification head (its source holds no head.weight: a backbone); "
                             "forward_features, forward_intermediates and attention_maps are what it answers")

    def _features_out(self, B, C, integers, out):
        """forward_features' destination: a fresh [B, C] tensor, or the caller's `out` once it is seen to be a [B, C] view of the right
        dtype on the engine's device with unit inner stride (TypeError / ValueError otherwise: before anything is launched)"""
        dt = torch.int8 if integers else torch.float32
        if out is None:
            return torch.empty(B, C, dtype=dt, device=self.dev)
        if not isinstance(out, torch.Tensor) or out.dtype != dt:
            raise TypeError(f"out must be a {dt} tensor (integers={bool(integers)})")
        if out.device.type != self.dev.type or (self.dev.index is not None and out.device.index != self.dev.index):
            raise ValueError(f"out must be on {self.dev}")
        if tuple(out.shape) != (B, C):
            raise ValueError(f"out must be [{B}, {C}], not {list(out.shape)}")
        if out.stride(1) != 1 or (B > 1 and out.stride(0) < C):
            raise ValueError(f"out: strides {tuple(out.stride())}; rows of {C} contiguous elements, row stride at least {C}")
        return out

    def _features_emit(self, q, B, C, scale, out):
        """the int8 embedding q (workspace, dense [>= B, C]) -> out as _features_out passed it: one ivit_dequant_rows_i8_f32 launch
        for float32, a strided device copy of the integers for int8"""
        if out.dtype == torch.float32:
            dequant_rows(q, C, B, C, scale, out, out.stride(0) if B > 1 else C, self._stream())
        else:
            out.copy_(q.view(-1)[: B * C].view(B, C))
        return out

    def set_input_normalisation(self, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """uint8 input: the (mean, std) of the Normalize transform in front of the model (default: ImageNet's).  forward() then
        accepts uint8 [B,3,H,W] pixel tensors -- a quarter of the bytes of the float32 input -- and quantises them through a
        3 x 256 table that holds the float pipeline's result per (channel, pixel value): same integers as the float path."""
        self.input_lut = torch.from_numpy(input_lut_u8(self.s0, mean, std)).to(self.dev)
        self.input_norm = (tuple(float(v) for v in mean), tuple(float(v) for v in std))   # what the table was built for
