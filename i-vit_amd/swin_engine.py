"""Integer-only Swin forward on MI355X (config 5): int8 GEMM operands, int16 residual stream, every operator a
hand-written HIP kernel reached through the C ABI (include/ivit_hip.h, second half).

Dataflow = the reference's frozen-model forward (/root/reference/models/swin_quant.py:539-564; WindowAttention
:121-169; SwinTransformerBlock :251-301; PatchMerging :328-349; PatchEmbed with norm, layers_quant.py:191-203):

  images f32 [B, 3, H, W] (224 x 224 below; any multiple of the windows, see unsupported_geometry)
    --quantize+im2col(4x4)--> int8 [B*3136, 48|64] --GEMM+requant--> qact_before_norm int8
    --I-LayerNorm+requant--> patch_embed.qact int8 --requant 8->16--> x int16 [B*3136, 96]
  per block { LN16->8 written in window order (partition + cyclic shift are a row map inside the kernel)
              -> GEMM qkv (+requant, head-major per window) -> window attention (bias, mask, Shiftmax, P.V)
              -> GEMM proj (int32) -> qact4(16) + window reverse + residual QuantAct(16) in one pass
              -> LN16->8 -> GEMM fc1 -> ShiftGELU table -> GEMM fc2 (+requant) -> residual QuantAct(16) }
  per stage end { 2x2 patch-merge gather int16 -> LN16->8 -> GEMM reduction (+requant) -> widen to int16 }
  LN16->8 -> token average pool + requant -> GEMM head -> INT32 logits -> scale + argmax

family="ibert" (gelu_type = softmax_type = layernorm_type = 'ibert', the reference fork's default) keeps this dataflow and replaces
the three operators: every LayerNorm is IBERTIntLayerNorm with its overflow shift (ivit_ibert_layernorm_i8 for the patch norm,
ivit_ibert_layernorm_i16_i8_ex on the stream, norm1 through ivit_ibert_layernorm_i16_i8_win, which stores in window order), the window
attention is ivit_window_attention_i8_ibert (IBERTIntSoftmax(8)), and IBERTIntGELU + mlp.qact1 is a 256-entry map applied in the fc1
epilogue (ivit_gemm_i8_requant_lut_ex) where fc1 takes the fragment weight copy, by ivit_shiftgelu_lut_i8 elsewhere.

There is no fallback path: a missing libivit_hip.so or a kernel error raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, gemm_forms
from .engine_common import (EngineBase, _np, block_copy, frag_copy, intermediate_indices, layernorm, layernorm_f32, token_format,
                            tokens_to_nchw)
from .prepare import (LayerNormParams, LinearParams, dyadic, dyadic1, f32, ibert_saturated_exp, ibert_window_mask_ok, pad_head,
                      phi_is_identity, phi_table, quant_sym, requant_host, shiftexp_band, sym_scale, window_shiftexp_band)
from .topk import TOPK_MAX

PATCH = 4
HEAD_DIM = 32
IDENT = (1 << 30, 30)  # dyadic 1.0
SHORT_WINDOW = 64      # tokens per window of the one-wave-per-window entries (ivit_window_attention_i8*); above: *_long
LONG_WINDOW = 144      # ivit_window_attention_i8_long: 65..144 tokens (windows of 9x9 .. 12x12)


def key_pad(N: int) -> int:
    """key length of a row of the bias / region tables: 64 for the short entries, whole key tiles of 16 for the long one"""
    return 64 if N <= SHORT_WINDOW else (N + 15) // 16 * 16


def image_hw(img_size) -> tuple:
    """img_size as the reference takes it (to_2tuple, layers_quant.py:168): an int or a pair (height, width)"""
    if isinstance(img_size, (tuple, list)):
        ih, iw = img_size
        return int(ih), int(iw)
    return int(img_size), int(img_size)


def block_window(H: int, W: int, window: int, bi: int) -> tuple:
    """(window, shift) of block bi of a stage on an H x W map: SwinTransformerBlock's rule (swin_quant.py:200-203) -- a map whose
    shorter side is no longer than the window is covered by windows of that side, unshifted"""
    if min(H, W) <= window:
        return min(H, W), 0
    return window, (0 if bi % 2 == 0 else window // 2)


def unsupported_geometry(img_size, patch, window: int, stages: int) -> str | None:
    """None when IntSwinEngine can run this geometry: images of (height, width) or one int for both, patch 4 x 4, and at every stage
    either a map whose shorter side is no longer than the window (windows of that side, no shift: SwinTransformerBlock's rule) or a
    window that divides both sides; both sides a whole number of the block's windows, of at most 144 tokens, and even where the
    stage is merged (the reference pads nothing)"""
    ph, pw = image_hw(patch)
    if ph != pw or ph != PATCH:
        return f"geometry: patch {ph}x{pw} (fused engine: {PATCH}x{PATCH})"
    ih, iw = image_hw(img_size)
    if ih <= 0 or iw <= 0 or ih % PATCH or iw % PATCH:
        return f"geometry: image size {ih}x{iw} is not a multiple of the patch"
    H, W = ih // PATCH, iw // PATCH
    for li in range(stages):
        win, _ = block_window(H, W, window, 0)
        if H % win or W % win:
            return f"geometry: stage {li} map {H}x{W} is not a whole number of {win}x{win} windows"
        if win * win > LONG_WINDOW:
            return f"geometry: {win}x{win} windows ({win * win} tokens; fused window attention: <= {LONG_WINDOW})"
        if li < stages - 1:
            if H % 2 or W % 2:
                return f"geometry: stage {li} map {H}x{W} cannot be merged"
            H, W = H // 2, W // 2
    return None


def _pad64(k):
    return (k + 63) // 64 * 64


def rel_position_index(ws: int) -> np.ndarray:
    """relative_position_index of WindowAttention (swin_quant.py:73-88): [ws*ws, ws*ws] into the (2ws-1)^2 table."""
    yy, xx = np.divmod(np.arange(ws * ws), ws)
    dy = yy[:, None] - yy[None, :] + (ws - 1)
    dx = xx[:, None] - xx[None, :] + (ws - 1)
    return dy * (2 * ws - 1) + dx


def shift_mask_regions(H: int, W: int, ws: int, shift: int) -> np.ndarray:
    """Region id of every window token of a shifted block (swin_quant.py:223-243): [nW, ws*ws]."""
    def band(n):
        b = np.zeros(n, np.int64)
        b[n - ws:n - shift] = 1
        b[n - shift:] = 2
        return b
    img = band(H)[:, None] * 3 + band(W)[None, :]
    return img.reshape(H // ws, ws, W // ws, ws).transpose(0, 2, 1, 3).reshape(-1, ws * ws)


def window_row_map(B: int, H: int, W: int, ws: int, shift: int) -> np.ndarray:
    """Host restatement of the kernels' win_row (csrc/swin.hip): destination row, in window order, of token (b,y,x)."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ys, xs = (y - shift) % H, (x - shift) % W
    idx = ((ys // ws) * (W // ws) + xs // ws) * (ws * ws) + (ys % ws) * ws + xs % ws
    return (np.arange(B)[:, None] * (H * W) + idx.reshape(-1)[None, :]).reshape(-1)


def _bias_pad(bias, s_tab, s_A, N):
    """the identity operand of attn.qact2 (swin_quant.py:143-147) as the kernels read it: RNE(k_tab * m / 2^e), int16 [nH, N, kp]"""
    m2, e2 = dyadic(s_tab, s_A)
    bias_add = requant_host(bias, m2[0], e2[0])
    assert np.abs(bias_add).max() < 32768
    kp = key_pad(N)
    bias_pad = np.zeros((bias.shape[0], N, kp), np.int16)
    bias_pad[:, :, :N] = bias_add
    return bias_pad, kp


def window_attention_spec(upload, bias, s_tab, s_S, s_at, s_A, s_pv, s_a3, region, N):
    """Constants of one window-attention launch (the ivit_window_attention_i8* family), shared by the engine and the module path
    (quantization_utils/lazy.py).  bias: the 8-bit relative position bias [nH, N, N] at scale s_tab (the identity operand of
    attn.qact2, swin_quant.py:143-147); s_S the scale the scores arrive with, s_at / s_A the scales of qact_attn1 / qact2, s_pv /
    s_a3 those around qact3; region [nW, N] the region ids of a shifted block's mask, or None.
    -> (dict of launch arguments, form): form is None on the integer kernel, else the natural-scale Shiftmax form ("band1xW" /
    "band256xW" / "literal", prepare.window_shiftexp_band)."""
    bias_pad, kp = _bias_pad(bias, s_tab, s_A, N)
    region_pad, mask_value = None, 0
    # Shiftmax input: phi(q) = fl(fl(q*s)/s) for a plain score, fl(fl(fl(q*s) - 100)/s) for one under the shift
    # mask (:149-156 adds float -100 to q*s, ivit_modules.py:165 divides by s).  Integer kernel when phi is the
    # identity and -100/s an integer; else the literal float sequence on the two 256-entry tables
    qv = np.arange(-128, 128, dtype=f32)
    phi_m = ((((qv * s_A).astype(f32) + f32(-100.0)).astype(f32)) / s_A).astype(f32)
    att_nat = not phi_is_identity(s_A)
    if region is not None:
        mval = f32(-100.0) / s_A                                    # :149-155: (k*s + (-100)) / s
        if mval != np.rint(mval) or abs(mval) >= 32768:
            att_nat = True
            mask_value = -1                                         # unused by the literal form
        else:
            mask_value = int(mval)
        # the integer form of the short entries reads Shiftmax's exp_int from a table over the 256 distances to the row maximum and
        # gives a masked score (|mask_value| or more below it) the LAST entry: right only if the table has saturated by then, i.e.
        # -d - floor(d / 2) + floor(d / 16) <= 15 x0 for some d <= 255 (ivit_modules.py:151-155; x0 = floor(-1 / s) <= -25 never
        # does).  Otherwise the literal form, which is exact at any scale.  The rule's home is shiftmax_ksat (csrc/common.h), which
        # win_attn_check (csrc/win_attn_host.h) applies to the short entries; this copy stays because the form is chosen here, before
        # any launch, and tests/test_window_attention_plan_cpu.py holds it to the launcher's answer
        x0 = int(np.floor(f32(-1.0) / s_A))
        if N <= SHORT_WINDOW and not any(-d + (-d >> 1) - (-d >> 4) <= 15 * x0 for d in range(256)):
            att_nat = True
        region_pad = np.zeros((region.shape[0], kp), np.uint8)
        region_pad[:, :N] = region
    band, band_w, form = None, 0, None
    if att_nat:
        # table form of the natural-scale Shiftmax where it is provably what the reference computes (every masked score
        # saturated, no masked row maximum); else the kernel's literal float sequence on phi / phi_m
        band, band_w = window_shiftexp_band(s_A, region is not None)
        form = "literal" if band is None else f"band{band.shape[0]}x{band_w}"
    spec = dict(ms=dyadic1(s_S, s_at), mb=dyadic1(s_at, s_A), s_attn=float(s_A), mo=dyadic1(s_pv, s_a3),
                bias=upload(bias_pad), region=None if region_pad is None else upload(region_pad),
                mask_value=mask_value, phi=upload(phi_table(s_A)) if att_nat else None, phim=upload(phi_m) if att_nat else None,
                band=None if band is None else upload(band), band_w=band_w, long=N > SHORT_WINDOW)
    return spec, form


def window_attention(a, qkv, out, ldo, nwin, nW, nH, N, H, W, win, shift, fuse_proj, st):
    """One window attention of a window_attention_spec `a` on qkv, head-major per window [3, nwin, nH, N, HEAD_DIM] -> out, row
    stride ldo.  H, W, win, shift: the map's geometry for the forms that store to image rows or take it regardless (the long and the
    band entry); fuse_proj: the output goes straight to its image rows (window reverse + roll back in the store address), so that
    attn.proj + attn.qact4 + the residual QuantAct qact2 are then ONE GEMM, in place on the residual stream -- else window order."""
    p, band = _lib.ptr, a["band"]
    head = (p(qkv), p(out), ldo, p(a["bias"]), p(a["region"]))
    dims = (nwin, nW, nH, N, HEAD_DIM, a["ms"][0], a["ms"][1], a["mb"][0], a["mb"][1], a["s_attn"], a["mo"][0], a["mo"][1])
    if a["long"]:
        # windows of 65..144 tokens: one entry for every Shiftmax form and both output orders
        _lib.call("ivit_window_attention_i8_long", *head, a["mask_value"], *dims, p(None if band is not None else a["phi"]),
                  p(None if band is not None else a["phim"]), p(band), a["band_w"], 0 if band is None else int(band.shape[0]),
                  H, W, win, shift, int(fuse_proj), st)
    elif band is not None:
        _lib.call("ivit_window_attention_i8_band", *head, *dims, p(band), a["band_w"], int(band.shape[0]), H, W,
                  win if fuse_proj else 0, shift, st)
    elif fuse_proj:
        _lib.call("ivit_window_attention_i8_unwindow", *head, a["mask_value"], *dims, p(a["phi"]), p(a["phim"]), H, W, win, shift, st)
    else:
        _lib.call("ivit_window_attention_i8_compat", *head, a["mask_value"], *dims, p(a["phi"]), p(a["phim"]), st)


def window_attention_ibert_spec(upload, device, st, bias, s_tab, s_S, s_at, s_A, s_pv, s_a3, region, N, act_range, form=None):
    """window_attention_spec for a WindowAttention whose softmax is IBERTIntSoftmax(8) (ivit_window_attention_i8_ibert).  act_range:
    (x_min, x_max) of the softmax's internal 16-bit QuantAct.  form: "table" the [256][256] table of
    ivit_ibert_softmax_build_table, "band" its band form, None the band where it is at most 128 wide (as engine_common.attention_spec
    chooses).  -> the dict of launch arguments (`act_sf`: that QuantAct's scale), or None where the entry's precondition does not
    hold: a shift mask whose scores do not all land on int_exp's clamp (prepare.ibert_window_mask_ok) -- nothing may be launched."""
    from .quantization_utils.ibert_modules import softmax_constants
    x0i, bi, ci, exp_sf, act_sf, ma, ea = softmax_constants(s_A, *act_range)
    if region is not None and not ibert_window_mask_ok(s_A, x0i):
        return None
    bias_pad, kp = _bias_pad(bias, s_tab, s_A, N)
    region_pad = None
    if region is not None:
        region_pad = np.zeros((region.shape[0], kp), np.uint8)
        region_pad[:, :N] = region
    tab = torch.empty(65536, dtype=torch.float32, device=device)
    _lib.call("ivit_ibert_softmax_build_table", float(s_A), x0i, bi, ci, float(exp_sf), float(act_sf), ma, ea, _lib.ptr(tab), st)
    band_w = 0
    if form != "table":
        band, bw = shiftexp_band(tab.cpu().numpy().view(np.uint32).reshape(256, 256))
        if form == "band" and not bw:
            raise ValueError("the exponent table has no band form at this scale")
        if bw and (form == "band" or bw <= 128):
            tab, band_w = upload(band.view(np.float32)), bw
    return dict(ms=dyadic1(s_S, s_at), mb=dyadic1(s_at, s_A), mo=dyadic1(s_pv, s_a3), bias=upload(bias_pad),
                region=None if region_pad is None else upload(region_pad), table=tab, band_w=band_w, act_sf=float(act_sf),
                masked_exp=float(ibert_saturated_exp(x0i, bi, ci, exp_sf, act_sf, ma, ea)))


def window_attention_ibert(a, qkv, out, ldo, nwin, nW, nH, N, H, W, win, shift, image_order, st):
    """One window attention of a window_attention_ibert_spec `a`: operands as window_attention; win == 0: no geometry, window order"""
    p = _lib.ptr
    _lib.call("ivit_window_attention_i8_ibert", p(qkv), p(out), ldo, p(a["bias"]), p(a["region"]), a["masked_exp"], nwin, nW, nH, N,
              HEAD_DIM, *a["ms"], *a["mb"], *a["mo"], p(a["table"]), a["band_w"], H, W, win, shift, int(image_order), st)


def window_attention_probs(a, family, qkv, probs, nwin, nW, nH, N, st):
    """The softmax probabilities of one window attention: the P that window_attention / window_attention_ibert multiply with V for
    the same spec `a` (family "ivit": a window_attention_spec, "ibert": a window_attention_ibert_spec) and the same head-major qkv,
    written to probs, uint8 [nwin, nH, N, ldp >= N] (scale 2^-7; row stride = probs.stride(-2)).  One launch."""
    p = _lib.ptr
    head = (p(qkv), p(probs), int(probs.stride(-2)), p(a["bias"]), p(a["region"]))
    if family == "ibert":
        _lib.call("ivit_window_attention_probs_u8_ibert", *head, a["masked_exp"], nwin, nW, nH, N, HEAD_DIM, *a["ms"], *a["mb"],
                  p(a["table"]), a["band_w"], st)
    else:
        band = a["band"]      # form selection as window_attention: a band table first, then the phi tables, else the integer form
        _lib.call("ivit_window_attention_probs_u8", *head, a["mask_value"], nwin, nW, nH, N, HEAD_DIM, *a["ms"], *a["mb"], a["s_attn"],
                  p(None if band is not None else a["phi"]), p(None if band is not None else a["phim"]), p(band), a["band_w"],
                  0 if band is None else int(band.shape[0]), st)


def map_blocks(blocks, depths):
    """the (stage, block) pairs of an attention_maps call, validated: None = every block; ValueError for a pair out of range or
    repeated"""
    every = [(li, bi) for li, d in enumerate(depths) for bi in range(d)]
    if blocks is None:
        return every
    sel = []
    for pair in blocks:
        try:
            li, bi = (int(v) for v in pair)
        except (TypeError, ValueError):
            raise ValueError(f"blocks: {pair!r} is not a (stage, block) pair") from None
        if (li, bi) not in every:
            raise ValueError(f"blocks: {(li, bi)} is outside the model's blocks (depths {tuple(depths)})")
        if (li, bi) in sel:
            raise ValueError(f"blocks: {(li, bi)} is repeated")
        sel.append((li, bi))
    return sel


def pool_literal_host(q: np.ndarray, s: float) -> np.ndarray:
    """Host restatement of ivit_avgpool_requant_i8_literal's float32 mean (csrc/swin.hip, rowsum.h torch_outer_rowsum): q int8
    [B, T, C], s the input scale -> float32 [B, C], torch's CPU mean over the transposed view of y = fl(q * s) (serial order)."""
    B, T, C = q.shape
    y = (q.astype(f32) * f32(s)).astype(f32)

    def cascade(v):          # v [n, ...]: rowsum.h torch_cascade_sum along axis 0
        n = v.shape[0]
        lg = max(0, int(np.ceil(np.log2(n)))) if n > 1 else 0
        lp = max(4, lg // 4)
        step, mask = 1 << lp, (1 << lp) - 1
        a0 = np.zeros(v.shape[1:], f32)
        a1, a2, a3 = a0.copy(), a0.copy(), a0.copy()
        i = 0
        while i + step <= n:
            for _ in range(step):
                a0 = (a0 + v[i]).astype(f32)
                i += 1
            a1, a0 = (a1 + a0).astype(f32), np.zeros_like(a0)
            if (i & (mask << lp)) == 0:
                a2, a1 = (a2 + a1).astype(f32), np.zeros_like(a1)
                if (i & (mask << (2 * lp))) == 0:
                    a3, a2 = (a3 + a2).astype(f32), np.zeros_like(a2)
        for j in range(i, n):
            a0 = (a0 + v[j]).astype(f32)
        return (((a0 + a1).astype(f32) + a2).astype(f32) + a3).astype(f32)

    v = y.transpose(1, 0, 2)                       # [T, B, C]
    out = cascade(v)
    cf = C & ~31
    if cf < C:                                     # tail columns: four interleaved partials, the T % 4 last elements into the first
        t = v[:, :, cf:]
        n4 = T // 4
        p = [cascade(t[k:4 * n4:4]) if n4 else np.zeros(t.shape[1:], f32) for k in range(4)]
        for j in range(4 * n4, T):
            p[0] = (p[0] + t[j]).astype(f32)
        out[:, cf:] = (((p[0] + p[1]).astype(f32) + p[2]).astype(f32) + p[3]).astype(f32)
    return (out / f32(T)).astype(f32)


class IntSwinEngine(EngineBase):
    def __init__(self, float_state, ranges, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window=7,
                 device="cuda:0", max_batch: int = 64, img_size=224, family: str = "ivit", int_sqrt: bool = False):
        """float_state: name -> float32 array (the model's state_dict); ranges: QuantAct name -> (x_min, x_max) of the frozen model.
        img_size: an int or (height, width) (swin_quant.py:462-488 through layers_quant.py:168-175).
        family: the operator family of LayerNorm / Softmax / GELU, "ivit" or "ibert" (all three); int_sqrt: IBERTIntLayerNorm's
        use_int_sqrt (layernorm_type 'ibert_use-int-sqrt_true')."""
        self.C0, self.depths, self.heads, self.window = embed_dim, tuple(depths), tuple(num_heads), window
        if family not in ("ivit", "ibert"):
            raise ValueError(f"operator family {family!r}: the fused engine implements 'ivit' and 'ibert'")
        if int_sqrt and family != "ibert":
            raise ValueError("int_sqrt (use_int_sqrt) is a parameter of the 'ibert' LayerNorm")
        self.family, self.int_sqrt = family, bool(int_sqrt)
        ibert = family == "ibert"
        why = unsupported_geometry(img_size, PATCH, window, len(self.depths))
        if why is not None:
            raise ValueError(why)
        self.img_hw = image_hw(img_size)
        self.img_size = self.img_hw[0] if self.img_hw[0] == self.img_hw[1] else self.img_hw      # the int of a square model
        self.dev = torch.device(device)
        self.max_batch = max_batch
        _lib.lib()  # fail loudly now if the HIP library is absent
        P = {k: _np(v).astype(np.float32) for k, v in float_state.items()}
        R = ranges

        def s(name, bits=8):
            lo, hi = R[name]
            return sym_scale(lo, hi, bits)

        dev = self._upload

        def lin_host(name, s_in):
            lp = LinearParams(P[name + ".weight"], P.get(name + ".bias"), s_in)
            Kp = _pad64(lp.K)
            W = np.zeros((lp.W8.shape[0], Kp), np.int8)   # zero K-padding: the operand's pad columns never contribute
            W[:, :lp.K] = lp.W8
            d = dict(W=dev(W), b=None if lp.b32 is None else dev(lp.b32), K=Kp, N=W.shape[0])
            d["Wb"] = block_copy(d["W"], self._stream())      # for the calls that reach the persistent GEMM
            # MFMA-fragment copy (qkv / fc1 of stages 1-3, all of stage 3): the 16x16x64 order except for attn.proj, whose fused
            # 16-bit epilogue exists for the 32x32x32 order only; 128-channel work items for the int8 epilogues of qkv / fc1
            d["Wf"], d["Wf_bit"] = frag_copy(d["W"], self._stream(), order16=not name.endswith("attn.proj"),
                                             narrow=name.endswith(("attn.qkv", "mlp.fc1")))
            return lp, d

        def lin_dev(name, s_in, s_out):
            lp, d = lin_host(name, s_in)
            m, e = lp.requant_to(s_out)
            d.update(m=dev(m.view(np.int32)), e=dev(e))
            return d

        self.proj_fused = True     # attention output in image order + attn.proj / attn.qact4 / qact2 in one GEMM (False: A/B, tests)
        self.proj_i16 = True       # attn.proj writes the 16-bit attn.qact4 output instead of raw accumulators
        self.natural_sites = 0     # operators whose input scale is not a power of two: literal / table-driven kernels
        self.window_softmax_forms = []     # per natural-scale attention block: "band1xW" / "band256xW" / "literal" (prepare.window_shiftexp_band)

        def ln_dev(prefix, s_out, s_in, bits_in=16):
            """s_in: scale of the LayerNorm's input.  If fl(fl(q*s_in)/s_in) != q for some q of that width, the reference's
            LayerNorm sees those neighbouring floats (ivit_modules.py:36-38): 16-bit inputs take the literal kernel, the 8-bit
            patch norm the table form of the DeiT engine.  family "ibert": IBERTIntLayerNorm works on fl(q * s_in) at any scale; its
            overflow shift is the module's frozen buffer (ibert_modules.py:134-140; absent from the state: 0)."""
            lp = LayerNormParams(P[prefix + ".weight"], P[prefix + ".bias"], s_out)
            if not ibert:
                return self._ln_spec(lp, s_in, bits_in)
            shift = float(P[prefix + ".shift"].reshape(-1)[0]) if prefix + ".shift" in P else 0.0
            return self._ln_spec(lp, s_in, bits_in, ibert_shift=shift, int_sqrt=self.int_sqrt)

        # ---- stem (layers_quant.py:191-203 with norm_layer; swin_quant.py:541-546)
        s0 = s("qact_input")
        self.inv_s0 = float(f32(1.0) / s0)
        self.s0 = float(s0)
        self.input_lut = None
        s_bn = s("patch_embed.qact_before_norm")
        self.patch = lin_dev("patch_embed.proj", s0, s_bn)
        s_pq = s("patch_embed.qact")
        self.patch_ln = ln_dev("patch_embed.norm", s_pq, s_bn, 8)
        s_x = s("qact1", 16)
        self.stem_me = dyadic1(s_pq, s_x)

        # ---- stages
        self.stages = []
        H, W = self.img_hw[0] // PATCH, self.img_hw[1] // PATCH
        C = embed_dim
        for li, (depth, nH) in enumerate(zip(self.depths, self.heads)):
            if C // nH != HEAD_DIM:
                raise ValueError("window attention kernel supports head_dim 32 only")
            st = dict(H=H, W=W, C=C, nH=nH, blocks=[], down=None)
            for bi in range(depth):
                p = f"layers.{li}.blocks.{bi}."
                win, shift = block_window(H, W, window, bi)
                N = win * win
                blk = dict(win=win, shift=shift)
                s_q1 = s(p + "qact1")
                blk["ln1"] = ln_dev(p + "norm1", s_q1, s_x)
                s_a1 = s(p + "attn.qact1")
                blk["qkv"] = lin_dev(p + "attn.qkv", s_q1, s_a1)
                s_S = f32(f32(s_a1 * s_a1) * f32(HEAD_DIM ** -0.5))            # swin_quant.py:139-141
                s_at = s(p + "attn.qact_attn1")
                s_tab = s(p + "attn.qact_table")
                s_A = s(p + "attn.qact2")
                ktab = quant_sym(P[p + "attn.relative_position_bias_table"], s_tab, 8)   # [(2ws-1)^2, nH]
                bias = ktab[rel_position_index(win).reshape(-1)].reshape(N, N, nH).transpose(2, 0, 1)
                region = shift_mask_regions(H, W, win, shift) if shift else None
                s_pv = f32(f32(1.0 / 128.0) * s_a1)
                s_a3 = s(p + "attn.qact3")
                if ibert:
                    act = p + "attn.log_int_softmax.act"        # the softmax's internal 16-bit QuantAct (ibert_modules.py:260)
                    if act not in R:
                        raise KeyError(f"the 'ibert' engine needs the range of {act} (the softmax's internal 16-bit QuantAct)")
                    blk["attn"], form = window_attention_ibert_spec(dev, self.dev, self._stream(), bias, s_tab, s_S, s_at, s_A, s_pv,
                                                                    s_a3, region, N, (float(R[act][0]), float(R[act][1]))), None
                    if blk["attn"] is None:
                        # no literal attention core in the engine: such a model runs module by module
                        raise ValueError(f"{p[:-1]}: the shift mask at s_attn = {float(s_A):.6g} is outside what "
                                         "ivit_window_attention_i8_ibert takes (prepare.ibert_window_mask_ok, about s_attn <= 0.29)")
                else:
                    blk["attn"], form = window_attention_spec(dev, bias, s_tab, s_S, s_at, s_A, s_pv, s_a3, region, N)
                blk["attn"]["nW"] = (H // win) * (W // win)
                if form is not None:
                    self.natural_sites += 1
                    self.window_softmax_forms.append(form)
                lp, d = lin_host(p + "attn.proj", s_a3)
                s_a4 = s(p + "attn.qact4", 16)
                mp, ep = dyadic(lp.s_acc, s_a4)
                d.update(m=dev(mp.view(np.int32)), e=dev(ep))
                blk["proj"] = d
                s_b2 = s(p + "qact2", 16)
                blk["res1"] = dyadic1(s_a4, s_b2) + dyadic1(s_x, s_b2)
                s_b3 = s(p + "qact3")
                blk["ln2"] = ln_dev(p + "norm2", s_b3, s_b2)
                s_g = s(p + "mlp.qact_gelu")
                blk["fc1"] = lin_dev(p + "mlp.fc1", s_b3, s_g)
                s_m1 = s(p + "mlp.qact1")
                blk["gelu_lut"] = self._gelu_lut(family, s_g, s_m1)
                s_m2 = s(p + "mlp.qact2")
                blk["fc2"] = lin_dev(p + "mlp.fc2", s_m1, s_m2)
                s_b4 = s(p + "qact4", 16)
                blk["res2"] = dyadic1(s_m2, s_b4) + dyadic1(s_b2, s_b4)
                s_x = s_b4
                st["blocks"].append(blk)
            st["s_out"] = float(s_x)      # the float32 act_scaling_factor of the stage's last qact4 (forward_intermediates)
            if li < len(self.depths) - 1:
                p = f"layers.{li}.downsample."
                s_d1 = s(p + "qact1")
                s_d2 = s(p + "qact2")
                st["down"] = dict(ln=ln_dev(p + "norm", s_d1, s_x), red=lin_dev(p + "reduction", s_d1, s_d2))
                s_x = s_d2
            self.stages.append(st)
            if st["down"] is not None:
                H, W, C = H // 2, W // 2, 2 * C
        self.C_last, self.T_last = C, H * W

        # ---- tail (swin_quant.py:552-563)
        s_q2 = s("qact2")
        self.ln_f = ln_dev("norm", s_q2, s_x)
        s_q3 = s("qact3")
        self.pool_me = dyadic1(s_q2, s_q3)
        # the tail's float mean over an even token count can land on an exact .5 tie; at a natural scale its float32 rounding then decides
        # qact3: the literal pooling restates torch's CPU order (ivit_avgpool_requant_i8_literal).  224 px (49 tokens): the integer form
        self.pool_literal = self.T_last % 2 == 0 and not phi_is_identity(s_q2)
        self.s_pool = float(s_q2)
        if self.pool_literal:
            self.natural_sites += 1
        self.s_feat = float(s_q3)     # the float32 act_scaling_factor of qact3 (forward_features)
        if "head.weight" in P:
            lp = LinearParams(P["head.weight"], P.get("head.bias"), s_q3)
            hW, hb, hs, self.num_classes = pad_head(lp.W8, lp.b32, lp.s_acc)      # any class count
            self.head = dict(W=dev(hW), b=dev(hb), K=lp.K, N=hW.shape[0])
            self.head_scale = dev(hs)
        else:      # a backbone (num_classes=0): forward_features / forward_intermediates / attention_maps
            self.head, self.head_scale, self.num_classes = None, None, 0
        self._alloc(max_batch)
        self._compact(True)
        torch.cuda.synchronize(self.dev)

    # ------------------------------------------------------------------ plumbing
    def _alloc(self, B):
        C0 = self.C0
        M0 = B * (self.img_hw[0] // PATCH) * (self.img_hw[1] // PATCH)
        ld0 = _pad64(C0)
        i8 = dict(dtype=torch.int8, device=self.dev)
        i16 = dict(dtype=torch.int16, device=self.dev)
        slack = 256  # GEMM K-padding reads up to ld - C bytes past the last row of a C-strided operand
        self.ws = dict(
            a0=torch.zeros(M0 * 64 + slack, **i8),
            pe=torch.empty(M0 * C0, **i8), pn=torch.empty(M0 * C0, **i8),
            x=torch.empty(M0 * C0, **i16), x2=torch.empty(M0 * C0, **i16),
            h=torch.zeros(M0 * ld0 + slack, **i8), ao=torch.zeros(M0 * ld0 + slack, **i8),
            qkv=torch.empty(3 * M0 * C0, **i8),
            acc=torch.empty(M0 * C0, dtype=torch.int32, device=self.dev),
            f1=torch.empty(M0 * 4 * C0, **i8), g=torch.empty(M0 * 4 * C0, **i8), f2=torch.empty(M0 * C0, **i8),
            xm=torch.empty(M0 * C0, **i16), hm=torch.empty(M0 * C0, **i8), red=torch.empty(M0 * C0 // 2, **i8),
            hN=torch.empty(B * self.T_last * self.C_last, **i8), pooled=torch.empty(B * self.C_last, **i8),
            **({} if self.head is None else dict(
                logits=torch.empty(B, self.head["N"], dtype=torch.int32, device=self.dev),
                logits_f=torch.empty(B, self.head["N"], dtype=torch.float32, device=self.dev))),
            top1=torch.empty(B, dtype=torch.int32, device=self.dev),
            topk=torch.empty(B * TOPK_MAX, dtype=torch.int32, device=self.dev),
        )

    def _compact(self, on=True):
        """Alias workspaces whose lifetimes do not overlap (see IntViTEngine._compact): the 16-bit residual QuantActs and the
        GELU run in place, the attention output reuses the LayerNorm buffer, q/k/v and the projection's int32 accumulators
        live inside the fc1 / GELU buffer.  One stage-0 block touches ~330 MB instead of ~870 MB at batch 128."""
        ws = self.ws
        if "_own" not in ws:
            ws["_own"] = {k: ws[k] for k in ("x2", "ao", "qkv", "acc", "g")}
        if on:
            ws["x2"] = ws["x"]
            ws["ao"] = ws["h"]
            ws["g"] = ws["f1"]
            ws["qkv"] = ws["f1"][: ws["_own"]["qkv"].numel()]
            ws["acc"] = ws["f1"].view(torch.int32)[: ws["_own"]["acc"].numel()]
        else:
            ws.update(ws["_own"])

    @staticmethod
    def _w(lin, epi, M):
        """(weight pointer, layouts) for M rows through epilogue `epi`: the copy that matches the kernel the launcher picks
        (gemm_forms.weight -- row-major for the skinny-K form of stage 0, which keeps the whole W in LDS)"""
        W, lay = gemm_forms.weight(lin, epi, M)
        return _lib.ptr(W), lay

    def _gemm(self, A, lda, lin, out, ldo, M, st):
        w, lay = self._w(lin, gemm_forms.RQ, M)
        _lib.call("ivit_gemm_i8_requant_ex", _lib.ptr(A), lda, w, lin["K"], _lib.ptr(lin["b"]),
                  _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(out), ldo, M, lin["N"], lin["K"], lay, st)

    # ------------------------------------------------------------------ forward
    def forward(self, images: torch.Tensor, taps: dict | None = None):
        """images: float32 [B,3,height,width] on the engine's device.  Returns (logits_int32 [B,1000], logits_f32, top1)
        -- views of the engine's workspace, valid until the next call.  `taps` (tests) receives clones of the
        intermediate integer tensors in the reference's layouts."""
        return self._forward(images, taps)

    def forward_features(self, images: torch.Tensor, integers: bool = False, out: torch.Tensor | None = None):
        """The pooled embedding -> (features [B, C_last], scale): the tensor qact3 returns behind norm -> qact2 -> avgpool, the
        first value of the reference's forward_features (swin_quant.py:551-558).  features: float32, the integers times scale in one
        float32 multiplication (ivit_dequant_rows_i8_f32) -- that tensor bit for bit; integers=True: the int8 integers.  scale: the
        float32 act_scaling_factor of qact3.  out=None: a fresh tensor (no workspace view).  out: a [B, C_last] view of that dtype on
        the engine's device with stride(1) == 1 and any row stride >= C_last (rows of a feature bank) to write into; TypeError /
        ValueError for any other, before anything is launched.  The forward stops behind the pooling launch: no head GEMM, no
        classifier launch; the workspace logits are left as they were.  Both operator families; a headless engine answers this too."""
        B = images.shape[0]
        out = self._features_out(B, self.C_last, integers, out)
        self._forward(images, stop="features")
        return self._features_emit(self.ws["pooled"], B, self.C_last, self.s_feat, out), self.s_feat

    def _graph_features(self, images, integers):
        """what forward_features_graph captures -> (features, scale), features in a tensor the graph owns"""
        return self.forward_features(images, integers)

    def forward_intermediates_early(self, images: torch.Tensor, indices=None, integers: bool = False):
        """forward_intermediates with an early stop: nothing behind the last selected stage is launched -- no patch merging, later
        stage, final norm, pooling, head or classifier.  The maps and scales are those of forward_intermediates; the workspace
        logits (and the pooled embedding) are then STALE, those of an earlier call.  (A method of its own: forward_intermediates
        keeps its parameters.)"""
        return self._intermediates(images, indices, integers, True)

    def forward_intermediates(self, images: torch.Tensor, indices=None, integers: bool = False):
        """The residual stream behind the last block of the selected stages as feature maps -> (maps, scales): maps = {stage:
        float32 [B, C_li, H_li, W_li]}, the tensor layers.li.blocks[-1].qact4 returns in the reference (integers times its scale,
        before the patch merging), channels first; integers=True: the int16 integers themselves.  scales = {stage: float}, that
        QuantAct's float32 act_scaling_factor.  indices: stage indices (None: every stage); ValueError for one out of range or
        repeated, before anything is launched.  The ordinary eager forward runs (fused projection included) -- its logits stay in
        the workspace as after forward() -- plus one launch per selected stage (engine_common.tokens_to_nchw).  Not part of taps
        or of the graph replays.  A headless engine stops behind the last selected stage (forward_intermediates_early)."""
        return self._intermediates(images, indices, integers, self.head is None)

    def _intermediates(self, images, indices, integers, stop_early):
        idx = intermediate_indices(indices, len(self.stages), "stage")
        B = images.shape[0]
        dt = torch.int16 if integers else torch.float32
        feats = {li: torch.empty(B, self.stages[li]["C"], self.stages[li]["H"], self.stages[li]["W"], dtype=dt, device=self.dev)
                 for li in idx}
        self._forward(images, feats=feats, stop=max(idx) if stop_early else None)
        return feats, {li: self.stages[li]["s_out"] for li in idx}

    def attention_maps(self, images: torch.Tensor, blocks=None):
        """The integer softmax probabilities of the selected blocks -> ({(stage, block): uint8 [B, nW, nH, N, N]}, scale 2^-7): nW
        windows per image in the order of window_partition on the rolled map, N = win * win tokens, queries and keys in window
        order -- the tensor attn.log_int_softmax returns in the reference, divided by its scale.  blocks: (stage, block) pairs (None:
        every block); ValueError for a pair out of range or repeated, before anything is launched.  The ordinary eager forward runs
        (fused projection included) -- its logits stay in the workspace as after forward() -- and behind the qkv GEMM of each
        selected block one more launch (window_attention_probs) writes the P that the fused window attention multiplies with V
        into a fresh tensor.  Both operator families; not part of taps or of the graph replays."""
        sel = map_blocks(blocks, self.depths)
        B = images.shape[0]
        maps = {}
        for li, bi in sel:
            stg, blk = self.stages[li], self.stages[li]["blocks"][bi]
            N = blk["win"] * blk["win"]
            maps[(li, bi)] = torch.empty(B, blk["attn"]["nW"], stg["nH"], N, N, dtype=torch.uint8, device=self.dev)
        self._forward(images, maps=maps, stop="features" if self.head is None else None)      # (a headless engine ends behind the pooling)
        return maps, 2.0 ** -7

    def forward_tokens(self, images: torch.Tensor, fmt: str = "NLC", integers: bool = False):
        """The final-normed token sequence of the last stage -> (tokens, scale).  Float form: the tensor model.norm returns
        (swin_quant.py:551), float32 [B, L, C_last] (fmt "NLC") or [B, C_last, H, W] ("NCHW"), with the float32 [C_last] per-channel
        scaling factor it returns beside it -- one launch (engine_common.layernorm_f32) from the 16-bit stream, both operator
        families.  integers=True: the int8 tensor qact2 gives (:552), which the engine computes in front of its pooling, in the same
        shapes, with the float scale of qact2.  The ordinary eager forward runs: pooled features and logits of the same call stay as
        forward_features / forward leave them (a headless engine stops behind the pooling).  There is no prefix token.  Not part of
        taps or of the graph replays."""
        token_format(fmt)
        B, C, T = images.shape[0], self.C_last, self.T_last
        hw = (self.stages[-1]["H"], self.stages[-1]["W"])
        dt = torch.int8 if integers else torch.float32
        out = torch.empty((B, T, C) if fmt == "NLC" else (B, C, *hw), dtype=dt, device=self.dev)

        def emit(x, q, st):
            if not integers:
                layernorm_f32(self.ln_f, x, C, B, T, 0, T, C, out, C if fmt == "NLC" else T, st, fmt=fmt)
            elif fmt == "NLC":
                out.copy_(q.view(-1)[: B * T * C].view(B, T, C))
            else:
                tokens_to_nchw(q, C, B, T, 0, T, C, 1.0, out, st)

        self._forward(images, toks=emit, stop="features" if self.head is None else None)
        return out, (self.s_pool if integers else self.ln_f["s"])

    def _forward(self, images: torch.Tensor, taps: dict | None = None, topk=None, feats: dict | None = None,
                 maps: dict | None = None, stop=None, toks=None):
        """forward; topk = (k, targets, hits): the classifier launch is the top-k selection (forward_topk).
        stop: None the whole forward; "features": return behind the pooling launch (forward_features); a stage index: return behind
        that stage's last block (forward_intermediates_early).  A headless engine needs one.
        feats: {stage index: [B, C, H, W]} to fill with the stream behind the last block of those stages (forward_intermediates)
        maps: {(stage, block): uint8 [B, nW, nH, N, N]} to fill with the softmax probabilities of those blocks (attention_maps)"""
        assert images.is_cuda and images.dtype in (torch.float32, torch.uint8) and images.is_contiguous()
        B = images.shape[0]
        ih, iw = self.img_hw
        assert images.shape[1:] == (3, ih, iw) and 0 < B <= self.max_batch
        if stop is None:
            self._require_head("forward")
        ws = self.ws
        st = self._stream()
        C0 = self.C0
        M = B * (ih // PATCH) * (iw // PATCH)

        def tap(name, t, rows, C, ld=None, perm=None):
            if taps is None:
                return
            ld = C if ld is None else ld
            v = t[: rows * ld].view(rows, ld)[:, :C]
            if perm is not None:
                v = v[perm]
            taps[name] = v.clone()

        if images.dtype == torch.uint8:      # uint8 pixels: ToTensor + Normalize + the input QuantAct as a 3 x 256 table (engine.py)
            if self.input_lut is None:
                self.set_input_normalisation()
            if ih != iw:      # the h x w entries; a square model keeps the launches it always had
                _lib.call("ivit_quantize_patchify_hw_u8_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 64, B, 3, ih, iw, PATCH,
                          _lib.ptr(self.input_lut), st)
            else:
                _lib.call("ivit_quantize_patchify_u8_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 64, B, 3, ih, PATCH,
                          _lib.ptr(self.input_lut), st)
        elif ih != iw:
            _lib.call("ivit_quantize_patchify_hw_f32_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 64, B, 3, ih, iw, PATCH,
                      self.inv_s0, st)
        else:
            _lib.call("ivit_quantize_patchify_ld_f32_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 64, B, 3, ih, PATCH,
                      self.inv_s0, st)
        self._gemm(ws["a0"], 64, self.patch, ws["pe"], C0, M, st)
        tap("patch_embed.qact_before_norm", ws["pe"], M, C0)
        # outer: the reference reduces over the transposed view of layers_quant.py:198
        layernorm(self.patch_ln, ws["pe"], C0, M, C0, ws["pn"], C0, st, outer=M // B)
        tap("patch_embed.qact", ws["pn"], M, C0)
        x, x2 = ws["x"], ws["x2"]
        _lib.call("ivit_requant_i8_i16", _lib.ptr(ws["pn"]), self.stem_me[0], self.stem_me[1], _lib.ptr(x), M * C0, st)
        tap("qact1", x, M, C0)

        for li, stg in enumerate(self.stages):
            H, W, C, nH = stg["H"], stg["W"], stg["C"], stg["nH"]
            M = B * H * W
            ld = _pad64(C)
            for bi, blk in enumerate(stg["blocks"]):
                p = f"layers.{li}.blocks.{bi}."
                win, shift = blk["win"], blk["shift"]
                N = win * win
                nwin = M // N
                perm = None
                if taps is not None:
                    perm = torch.from_numpy(window_row_map(B, H, W, win, shift)).to(self.dev)
                # every LayerNorm of stage 0 still sees the patch embedding's transposed layout in the reference: elementwise ops keep
                # the strides of layers_quant.py:198's view, and the residual QuantActs add `identity + x` with the identity (the
                # strided stream) as the first operand, whose layout torch then gives the sum; only the patch merging's cat makes the
                # stream contiguous.  Their float32 means run in torch's outer-reduction order (IVIT_LN_OUTER_MEAN)
                outer = H * W if li == 0 else 0
                layernorm(blk["ln1"], x, C, M, C, ws["h"], ld, st, H=H, W=W, ws=win, shift=shift, outer=outer)
                tap(p + "qact1", ws["h"], M, C, ld, perm)
                q = blk["qkv"]
                qw, qlay = self._w(q, gemm_forms.QKV, M)
                _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(ws["h"]), ld, qw, q["K"], _lib.ptr(q["b"]),
                          _lib.ptr(q["m"]), _lib.ptr(q["e"]), _lib.ptr(ws["qkv"]), N, nH, HEAD_DIM, M, 3 * C, q["K"], qlay, st)
                if taps is not None:   # reference layout [B_, N, 3C] (swin_quant.py:131-133)
                    hm = ws["qkv"][: 3 * M * C].view(3, nwin, nH, N, HEAD_DIM)
                    taps[p + "attn.qact1"] = hm.permute(1, 3, 0, 2, 4).reshape(nwin, N, 3 * C).clone()
                a = blk["attn"]
                if maps is not None and (li, bi) in maps:
                    window_attention_probs(a, self.family, ws["qkv"], maps[(li, bi)], nwin, a["nW"], nH, N, st)
                fuse_proj = self.proj_fused and taps is None
                if self.family == "ibert":
                    window_attention_ibert(a, ws["qkv"], ws["ao"], ld, nwin, a["nW"], nH, N, H, W, win, shift, fuse_proj, st)
                else:
                    window_attention(a, ws["qkv"], ws["ao"], ld, nwin, a["nW"], nH, N, H, W, win, shift, fuse_proj, st)
                tap(p + "attn.qact3", ws["ao"], M, C, ld)
                pj = blk["proj"]
                r = blk["res1"]
                if fuse_proj:
                    w_, lay = self._w(pj, gemm_forms.RQ16_RES16, M)
                    _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", _lib.ptr(ws["ao"]), ld, w_, pj["K"], _lib.ptr(pj["b"]),
                              _lib.ptr(pj["m"]), _lib.ptr(pj["e"]), _lib.ptr(x), C, r[0], r[1], r[2], r[3], _lib.ptr(x2), C, M, C,
                              pj["K"], lay, st)
                elif self.proj_i16:
                    # attn.proj + the 16-bit attn.qact4 in the GEMM epilogue (int16 [M, C] in window order, half the bytes of
                    # raw accumulators), then window reverse / un-shift + the residual QuantAct
                    _lib.call("ivit_gemm_i8_requant_i16", _lib.ptr(ws["ao"]), ld, _lib.ptr(pj["W"]), pj["K"], _lib.ptr(pj["b"]),
                              _lib.ptr(pj["m"]), _lib.ptr(pj["e"]), _lib.ptr(ws["acc"]), C, M, C, pj["K"], st)
                    _lib.call("ivit_residual_requant_i16", _lib.ptr(ws["acc"]), 16, None, None,
                              r[0], r[1], _lib.ptr(x), r[2], r[3], _lib.ptr(x2), M, C, H, W, win, shift, st)
                else:      # A/B: raw int32 accumulators, attn.qact4 inside the residual kernel
                    _lib.call("ivit_gemm_i8_i32", _lib.ptr(ws["ao"]), ld, _lib.ptr(pj["W"]), pj["K"], _lib.ptr(pj["b"]),
                              _lib.ptr(ws["acc"]), C, M, C, pj["K"], st)
                    _lib.call("ivit_residual_requant_i16", _lib.ptr(ws["acc"]), 32, _lib.ptr(pj["m"]), _lib.ptr(pj["e"]),
                              r[0], r[1], _lib.ptr(x), r[2], r[3], _lib.ptr(x2), M, C, H, W, win, shift, st)
                tap(p + "qact2", x2, M, C)
                layernorm(blk["ln2"], x2, C, M, C, ws["h"], ld, st, outer=outer)
                tap(p + "qact3", ws["h"], M, C, ld)
                f1 = blk["fc1"]
                f1w, f1lay = self._w(f1, gemm_forms.RQ, M) if self.family == "ibert" and taps is None else (None, 0)
                if f1lay & gemm_forms.FRAGS:
                    # I-BERT GELU + mlp.qact1 is a map of the requantised byte alone (no row maximum): applied in the fc1 epilogue
                    # of the weights-in-registers GEMM, the GELU kernel and its pass over the 4C-wide intermediate disappear
                    _lib.call("ivit_gemm_i8_requant_lut_ex", _lib.ptr(ws["h"]), ld, f1w, f1["K"], _lib.ptr(f1["b"]),
                              _lib.ptr(f1["m"]), _lib.ptr(f1["e"]), _lib.ptr(blk["gelu_lut"]), _lib.ptr(ws["g"]), 4 * C, M, f1["N"],
                              f1["K"], f1lay, st)
                else:
                    self._gemm(ws["h"], ld, f1, ws["f1"], 4 * C, M, st)
                    tap(p + "mlp.qact_gelu", ws["f1"], M, 4 * C)
                    _lib.call("ivit_shiftgelu_lut_i8", _lib.ptr(ws["f1"]), 4 * C, M, 4 * C, _lib.ptr(blk["gelu_lut"]),
                              _lib.ptr(ws["g"]), 4 * C, st)
                tap(p + "mlp.qact1", ws["g"], M, 4 * C)
                r = blk["res2"]
                f2 = blk["fc2"]
                if taps is not None:   # tests: the 8-bit mlp.qact2 tensor is not materialised on the fused path below
                    self._gemm(ws["g"], 4 * C, f2, ws["f2"], C, M, st)
                    tap(p + "mlp.qact2", ws["f2"], M, C)
                # mlp.fc2 + mlp.qact2 + the 16-bit residual QuantAct qact4 in one kernel (swin_quant.py:297-299)
                f2w, f2lay = self._w(f2, gemm_forms.RESID16, M)
                _lib.call("ivit_gemm_i8_requant_residual_i16_ex", _lib.ptr(ws["g"]), 4 * C, f2w, f2["K"],
                          _lib.ptr(f2["b"]), _lib.ptr(f2["m"]), _lib.ptr(f2["e"]), _lib.ptr(x2), C, r[0], r[1], r[2], r[3],
                          _lib.ptr(x), C, M, f2["N"], f2["K"], f2lay, st)
                tap(p + "qact4", x, M, C)
            if feats is not None and li in feats:
                tokens_to_nchw(x, C, B, H * W, 0, H * W, C, stg["s_out"], feats[li], st)
            if stop == li:      # (never "features": stage indices are ints)
                return None
            dn = stg["down"]
            if dn is not None:
                p = f"layers.{li}.downsample."
                _lib.call("ivit_patch_merge_i16", _lib.ptr(x), _lib.ptr(ws["xm"]), B, H, W, C, st)
                M4 = M // 4
                layernorm(dn["ln"], ws["xm"], 4 * C, M4, 4 * C, ws["hm"], 4 * C, st)
                tap(p + "qact1", ws["hm"], M4, 4 * C)
                self._gemm(ws["hm"], 4 * C, dn["red"], ws["red"], 2 * C, M4, st)
                tap(p + "qact2", ws["red"], M4, 2 * C)
                _lib.call("ivit_requant_i8_i16", _lib.ptr(ws["red"]), IDENT[0], IDENT[1], _lib.ptr(x), M4 * 2 * C, st)

        C, T = self.C_last, self.T_last
        layernorm(self.ln_f, x, C, B * T, C, ws["hN"], C, st)
        tap("qact2", ws["hN"], B * T, C)
        if toks is not None:
            toks(x, ws["hN"], st)
        if self.pool_literal:
            _lib.call("ivit_avgpool_requant_i8_literal", _lib.ptr(ws["hN"]), _lib.ptr(ws["pooled"]), B, T, C, self.s_pool,
                      self.pool_me[0], self.pool_me[1], st)
        else:
            _lib.call("ivit_avgpool_requant_i8", _lib.ptr(ws["hN"]), _lib.ptr(ws["pooled"]), B, T, C, self.pool_me[0],
                      self.pool_me[1], st)
        tap("qact3", ws["pooled"], B, C)
        if stop == "features":
            return None
        hd = self.head
        _lib.call("ivit_gemm_i8_i32", _lib.ptr(ws["pooled"]), C, _lib.ptr(hd["W"]), hd["K"], _lib.ptr(hd["b"]),
                  _lib.ptr(ws["logits"]), hd["N"], B, hd["N"], hd["K"], st)
        return self._classify(B, st, topk)

    __call__ = forward


def _model_img_size(model):
    """img_size of a SwinTransformer as the engine takes it: the int of a square model (today's argument), else (height, width)"""
    ih, iw = model.patch_embed.img_size
    return ih if ih == iw else (ih, iw)


def operator_family(model):
    """("ivit" | "ibert", int_sqrt) of a SwinTransformer whose three operators IntSwinEngine implements together; raises ValueError
    with the reason for a mixture of families and for a constructor parameter in an operator name other than the I-BERT LayerNorm's
    use_int_sqrt"""
    if len(set(model.op_types)) != 1 or model.op_types[0] not in ("ivit", "ibert"):
        raise ValueError(f"operator family {model.op_types} (fused engine: all three operators 'ivit', or all three 'ibert')")
    for kind, base, params in zip(("gelu", "softmax", "layernorm"), model.op_types, model.op_params):
        for k, v in params.items():
            if not ((kind, base, k) == ("layernorm", "ibert", "use_int_sqrt") and isinstance(v, bool)):
                raise ValueError(f"{kind} parameter {k}={v!r} of '{base}' (fused engine: default constructor arguments, or use_int_sqrt "
                                 "of the 'ibert' layernorm)")
    return model.op_types[0], bool(getattr(model.norm, "use_int_sqrt", False))


def engine_from_model(model, device=None, max_batch: int = 64):
    """IntSwinEngine for a frozen SwinTransformer of either operator family (all three operators 'ivit', or all three 'ibert' with
    or without the LayerNorm's use_int_sqrt): a snapshot of its parameters, ranges and LayerNorm shifts.  model(x) itself dispatches
    the I-ViT family only; this is how the I-BERT family reaches the engine.  Raises ValueError with the reason for a model the engine
    does not implement (operator mixture, another operator parameter, edited QuantAct widths, ape, no patch norm, geometry) and for
    a shift mask outside ivit_window_attention_i8_ibert's precondition (the block is named)."""
    family, int_sqrt = operator_family(model)
    why = model.engine_structure_reason(head=False)      # (a headless model gives a headless engine)
    if why is not None:
        raise ValueError(why)
    if not model.is_frozen():
        raise ValueError("the model is not frozen (freeze_model): its QuantAct ranges are still running statistics")
    if device is None:
        device = next(model.parameters()).device
    # a plain I-ViT model's engine is built with the arguments SwinTransformer._build_engine passes
    ops = dict(family=family, int_sqrt=int_sqrt) if family == "ibert" else {}
    return IntSwinEngine(dict(model.state_dict()), model.ranges(), model.embed_dim, model.depths, model.num_heads, model.window_size,
                         device=device, max_batch=max_batch, img_size=_model_img_size(model), **ops)
