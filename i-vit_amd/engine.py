"""Integer-only DeiT/ViT forward on MI355X: int8 activations end to end, every operator a
hand-written HIP kernel reached through the C ABI (include/ivit_hip.h).

Dataflow = the reference's frozen-model forward
(/root/reference/models/vit_quant.py:285-312, Attention :61-90, Block :142-155,
 /root/reference/models/layers_quant.py:145-154, 191-203), restated on integers:

  images f32 --quantize+im2col--> int8 [B*196, 768]
    --GEMM(patch_embed.proj)+requant(patch_embed.qact)--> int8 [B*196, C]
    --cls/pos assemble (qact_pos, qact1)--> x int8 [B*197, C]
  12 x { LN+requant -> GEMM qkv (+requant, head-major) -> fused attention
         -> GEMM proj (+requant +residual requant) -> LN+requant -> GEMM fc1 (+requant)
         -> ShiftGELU table gather (+requant) -> GEMM fc2 (+requant +residual requant) }
    --LN(cls rows)+requant--> GEMM head --> INT32 logits --scale+argmax--> top-1

The logits read token 0 of the last block's output alone, and every operator of a block but attention's K and V works row by
row: with cls_tail (the graph replays, forward(images, cls_tail=True)) the last block computes K and V for every token and
everything else for the B class rows only (_cls_block) -- the same logits, bit for bit.

There is no fallback path: a missing libivit_hip.so or a kernel error raises.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib, gemm_forms
from .engine_common import (EngineBase, _np, attention, attention_probs, attention_spec, block_copy, frag_copy, intermediate_indices,
                            layernorm, layernorm_f32, ln_spec, token_format, tokens_to_nchw)
from .prepare import dyadic, dyadic1, f32, pad_head, quant_sym, requant_host
from .topk import TOPK_MAX


class IntViTEngine(EngineBase):
    # fragment-packed weights in the 16x16x64 MFMA order (False / IVIT_FRAGS16=0: the 32x32x32 order everywhere; A/B, tests)
    frags16 = os.environ.get("IVIT_FRAGS16", "1") != "0"
    LONG_TOKENS = 1025     # ivit_attention_fused_i8_long (208 .. 1025 tokens); the other attention entries stop at 207

    def __init__(self, float_state=None, ranges=None, embed_dim: int = 768, depth: int = 12, num_heads: int = 12,
                 device="cuda:0", max_batch: int = 256, source=None, family: str = "ivit", stream_bits: int = 8,
                 softmax_bits: int = 8, pos_bits: int = 8, img_size=224, patch_size: int = 16, int_sqrt: bool = False):
        """float_state: name -> float32 array (the reference's state_dict names);
        ranges: QuantAct name -> (x_min, x_max) of the frozen model.  Alternatively `source`: any object with the
        FloatSource interface of export.py (e.g. export.ExportSource: integer parameters + scale table, no floats)."""
        self.C, self.D, self.H = embed_dim, depth, num_heads
        # geometry (vit_quant.py:158-166: img_size, patch_size): images of any height and width, square non-overlapping patches.
        # The patch GEMM steps K in 64-byte slabs.  The fused attention kernels hold a whole Shiftmax row of at most 207 keys in four lanes; I-ViT with the
        # 8-bit stream takes up to 1025 tokens (ivit_attention_fused_i8_long above 207: packed 8-bit scores)
        # img_size: an int or (height, width) (layers_quant.py:168-175); IMG keeps the int of a square model
        ih, iw = (int(v) for v in img_size) if isinstance(img_size, (tuple, list)) else (int(img_size),) * 2
        self.IMG_H, self.IMG_W, self.P = ih, iw, int(patch_size)
        self.IMG = ih if ih == iw else (ih, iw)
        tokens = (ih // self.P) * (iw // self.P) + 1 if self.P > 0 else 0
        if self.P <= 0 or ih % self.P or iw % self.P or (3 * self.P * self.P) % 64 or tokens > self.LONG_TOKENS:
            raise ValueError(f"geometry {self.IMG} / {self.P}: needs height and width % patch_size == 0, 3 * patch_size^2 % 64 == 0 and "
                             f"at most {self.LONG_TOKENS} tokens")
        self.grid = (ih // self.P, iw // self.P)
        self.NP = self.grid[0] * self.grid[1]
        self.T = self.NP + 1
        # operator family of LayerNorm / Softmax / GELU: "ivit" (I-ViT: IVITIntLayerNorm, Shiftmax, ShiftGELU) or "ibert" (the
        # fork's default, ibert_modules.py: literal float32 sequences on fl(q * s), any activation scale)
        if family not in ("ivit", "ibert"):
            raise ValueError(f"operator family {family!r}: the fused engine implements 'ivit' and 'ibert'")
        self.family = family
        # IBERTIntLayerNorm(use_int_sqrt=True) (layernorm_type 'ibert_use-int-sqrt_true'): norm1, norm2 and the final norm of the
        # model take std from integer_sqrt (ibert_modules.py:85-109, 143), on the 8- and on the 16-bit stream
        if int_sqrt and family != "ibert":
            raise ValueError("int_sqrt (use_int_sqrt) is a parameter of the 'ibert' LayerNorm")
        self.int_sqrt = bool(int_sqrt)
        # width of the residual stream and of the QuantActs that feed it (vit_quant.py:180-187): 8, or 16 = patch_embed_bw,
        # block_input_bw, attention_out_bw, mlp_out_bw, norm2_in_bw, att_block_out_bw all 16 (softmax_bw, pos_encoding_bw 8): the
        # GEMM operands stay int8, the stream and the projection / fc2 outputs are int16 (the kernels of the Swin engine)
        # stream_bits = 4: the same six QuantActs at 4 bits ('--bitwidth 4').  A 4-bit activation is an int8 byte clamped to [-8, 7]:
        # the 8-bit engine's dataflow, buffers and layouts, with the `_bits` entries at the six sites
        if stream_bits not in (4, 8, 16):
            raise ValueError("stream_bits must be 4, 8 or 16")
        if self.T > 207 and (family != "ivit" or stream_bits == 16):
            raise ValueError(f"geometry {self.IMG} / {self.P}: {self.T} tokens; the I-BERT softmax and the 16-bit stream take at most "
                             "207 tokens (more: family 'ivit' with stream_bits = 8 or 4)")
        self.stream_bits = sb = stream_bits
        # softmax_bw / pos_encoding_bw (vit_quant.py:181, 184) may be 16 on the 16-bit-stream path ('--bitwidth 16' sets all eight),
        # and 4 on the 4-bit-stream path
        other = {8: (8,), 16: (8, 16), 4: (4, 8)}[sb]
        if softmax_bits not in other or pos_bits not in other:
            raise ValueError("softmax_bits / pos_bits: 8, or 16 together with stream_bits = 16, or 4 together with stream_bits = 4")
        self.softmax_bits, self.pos_bits = softmax_bits, pos_bits
        self.hd = embed_dim // num_heads
        if self.hd != 64:
            raise ValueError("fused attention kernel supports head_dim 64 only")
        self.dev = torch.device(device)
        self.max_batch = max_batch
        _lib.lib()  # fail loudly now if the HIP library is absent
        if source is None:
            from .export import FloatSource
            source = FloatSource({k: _np(v) for k, v in float_state.items()}, ranges)
        C, H, hd = self.C, self.H, self.hd
        T = self.T
        s = source.act_scale

        dev = self._upload

        def lin_dev(lp, s_out):
            m, e = lp.requant_to(s_out)
            return dict(W=dev(lp.W8), b=dev(lp.b32), m=dev(m.view(np.int32)), e=dev(e), K=lp.K, N=lp.W8.shape[0])

        def ln_shift(prefix):
            if family != "ibert":
                return None
            try:
                return float(np.asarray(source.tensor(prefix + ".shift")).reshape(-1)[0])
            except KeyError:
                return 0.0

        def ln_dev(prefix, s_out, s_in):
            return self._ln_spec(source.layernorm(prefix, s_out), s_in, 16 if sb == 16 else 8, ln_shift(prefix), self.int_sqrt)   # payload width

        def ranges_of(name):
            if ranges is None or name not in ranges:
                raise KeyError(f"the 'ibert' engine needs the range of {name} (the softmax's internal 16-bit QuantAct)")
            return float(ranges[name][0]), float(ranges[name][1])

        self.natural_sites = 0     # operators whose input scale is not a power of two (compat kernels / tables)
        # ---- stem
        s0 = s("qact_input")
        self.inv_s0 = float(f32(1.0) / s0)
        self.s0 = float(s0)
        self.input_lut = None
        pe = source.linear("patch_embed.proj", s0)
        s_pe = s("patch_embed.qact", sb)
        self.patch = lin_dev(pe, s_pe)
        s_pos, s_x = s("qact_pos", pos_bits), s("qact1", sb)
        m1, e1 = dyadic(s_pe, s_x)
        m2, e2 = dyadic(s_pos, s_x)
        kpos = quant_sym(source.tensor("pos_embed").reshape(T, C), s_pos, pos_bits)
        pos_add = requant_host(kpos, m2[0], e2[0])                       # RNE(k_pos * m2 / 2^e2)
        z_cls = np.rint((source.tensor("cls_token").reshape(C) / s_pe).astype(f32))   # quant_utils.py:220 on the raw cls row
        qlim = 2 ** (sb - 1)
        cls_row = np.clip(requant_host(z_cls, m1[0], e1[0]) + pos_add[0], -qlim, qlim - 1)
        if sb == 16:
            assert np.abs(pos_add).max() < 2 ** 31
            self.pos_add = dev(pos_add.astype(np.int32))
            self.cls_row = dev(cls_row.astype(np.int16))
        else:
            assert np.abs(pos_add).max() < 32768
            self.pos_add = dev(pos_add.astype(np.int16))
            self.cls_row = dev(cls_row.astype(np.int8))
        self.embed_me = (int(m1[0]), int(e1[0]))

        # ---- blocks
        self.blocks = []
        for i in range(depth):
            p = f"blocks.{i}."
            blk = {}
            s_q1 = s(p + "qact1")
            blk["ln1"] = ln_dev(p + "norm1", s_q1, s_x)
            s_a1 = s(p + "attn.qact1")
            blk["qkv"] = lin_dev(source.linear(p + "attn.qkv", s_q1), s_a1)
            s_S = f32(f32(s_a1 * s_a1) * f32(hd ** -0.5))                 # vit_quant.py:72-75
            s_at = s(p + "attn.qact_attn1")
            s_pv = f32(f32(1.0 / 2 ** (softmax_bits - 1)) * s_a1)         # Shiftmax scale 2^-(bits-1) (:176) x value scale
            s_a2 = s(p + "attn.qact2")
            blk["attn"] = a = attention_spec(family, s_S, s_at, s_pv, s_a2, dev, self.dev, self._stream(),
                                             ranges_of(p + "attn.int_softmax.act") if family == "ibert" else None)
            self.natural_sites += int(family == "ivit" and (a["band"] is not None or a["exp2d"] is not None))
            s_a3 = s(p + "attn.qact3", sb)
            blk["proj"] = lin_dev(source.linear(p + "attn.proj", s_a2), s_a3)
            s_b2 = s(p + "qact2", sb)
            blk["res1"] = dyadic1(s_a3, s_b2) + dyadic1(s_x, s_b2)
            s_b3 = s(p + "qact3")
            blk["ln2"] = ln_dev(p + "norm2", s_b3, s_b2)
            s_g = s(p + "mlp.qact_gelu")
            blk["fc1"] = lin_dev(source.linear(p + "mlp.fc1", s_b3), s_g)
            s_m1 = s(p + "mlp.qact1")
            blk["gelu_lut"] = self._gelu_lut(family, s_g, s_m1)
            s_m2 = s(p + "mlp.qact2", sb)
            blk["fc2"] = lin_dev(source.linear(p + "mlp.fc2", s_m1), s_m2)
            s_b4 = s(p + "qact4", sb)
            blk["res2"] = dyadic1(s_m2, s_b4) + dyadic1(s_b2, s_b4)
            s_x = s_b4
            blk["s_out"] = float(s_b4)      # the float32 act_scaling_factor of blocks.i.qact4 (forward_intermediates)
            self.blocks.append(blk)

        # ---- tail
        s_q2 = s("qact2")
        self.ln_f = ln_dev("norm", s_q2, s_x)
        # forward_tokens: the final norm on the stream behind ANY block -- its host parameters and, for "ibert", its frozen shift
        # buffer; the device constants are derived per block from that block's output scale when first asked for (_ln_tokens)
        self._norm_lp = source.layernorm("norm", s_q2)
        self._norm_shift = ln_shift("norm")
        self._ln_tok = {depth - 1: self.ln_f}
        self.s_feat = float(s_q2)     # the float32 act_scaling_factor of qact2 (forward_features)
        try:
            head = source.linear("head", s_q2)
        except KeyError:              # a backbone (num_classes=0: no head.weight): forward_features / forward_intermediates / attention_maps
            head = None
        if head is None:
            self.head, self.head_scale, self.num_classes = None, None, 0
        else:
            hW, hb, hs, self.num_classes = pad_head(head.W8, head.b32, head.s_acc)    # any class count (num_classes=... of the factory)
            self.head = dict(W=dev(hW), b=dev(hb), K=head.K, N=hW.shape[0])
            self.head_scale = dev(hs)
        self.int8_weight_bytes = sum(int(b[k]["W"].numel()) for b in self.blocks for k in ("qkv", "proj", "fc1", "fc2")) \
            + int(self.patch["W"].numel()) + (0 if self.head is None else int(self.head["W"].numel()))
        # block-layout and MFMA-fragment copies of the GEMM weights (engine_common).  The 16x16x64 fragment order wherever the
        # epilogue writes int8; the 16-bit-stream epilogue of proj / fc2 exists for the 32x32x32 order only
        lins = [self.patch] + [b[k] for b in self.blocks for k in ("qkv", "proj", "fc1", "fc2")]
        for lin in lins:
            lin["Wb"] = block_copy(lin["W"], self._stream())
        wide = {id(b[k]) for b in self.blocks for k in ("proj", "fc2")} if self.stream_bits == 16 else set()
        for lin in lins:
            narrow = id(lin) not in wide
            lin["Wf"], lin["Wf_bit"] = frag_copy(lin["W"], self._stream(), order16=self.frags16 and narrow, narrow=narrow)
        for b in self.blocks:
            b["q"] = dict(b["qkv"], N=C)      # the first C rows of attn.qkv, row-major: Q of the class rows (_cls_block)
        self.weight_frags = True      # False: block-layout weights through the LDS-DMA kernel (A/B timing)
        self.block_operands = True    # False: row-major activations / weights everywhere (tests, A/B timing)
        # which producers write their output (a GEMM A operand) in the block layout.  Measured per producer / consumer pair
        # (DESIGN.md section 5): the GEMM gains 4-6 % from a block-layout A, the producer pays for 64-byte row segments
        self.block_a = {"ln": True, "attn": True, "gelu": True}
        self.gelu_in_place = True     # GELU overwrites the fc1 output (same layout on both sides)
        self.fuse_res16 = True        # 16-bit stream: projection / fc2 + both QuantActs in one kernel (False: A/B, tests)
        self.fuse_ibert_gelu = True   # family "ibert": GELU + mlp.qact1 as a byte map in the fc1 epilogue (False: A/B, tests)
        self.probe = None
        self._alloc(max_batch)
        self._compact(True)
        torch.cuda.synchronize(self.dev)

    # ------------------------------------------------------------------ plumbing
    def _alloc(self, B):
        C, T = self.C, self.T
        M = B * T
        M16 = (M + 15) // 16 * 16   # block-layout operands pad their rows to a multiple of 16
        i8 = dict(dtype=torch.int8, device=self.dev)
        self.ws = dict(
            a0=torch.empty(B * self.NP, 3 * self.P * self.P, **i8),
            pe=torch.empty(B * self.NP, C, **i8),
            x=torch.empty(M, C, **i8), x2=torch.empty(M, C, **i8), h=torch.empty(M16, C, **i8),
            qkv=torch.empty(3 * M * C, **i8), ao=torch.empty(M16, C, **i8),
            f1=torch.empty(M16, 4 * C, **i8), g=torch.empty(M16, 4 * C, **i8), untile=torch.empty(M, 4 * C, **i8),
            cls=torch.empty(B, C, **i8),
            # the last block on the class rows (_cls_block): LayerNorm output, query, attention output, the stream after the
            # projection and after fc2, fc1 / GELU
            c_h=torch.empty(B, C, **i8), c_q=torch.empty(B, C, **i8), c_ao=torch.empty(B, C, **i8), c_x=torch.empty(B, C, **i8),
            c_y=torch.empty(B, C, **i8), c_f1=torch.empty(B, 4 * C, **i8),
            **({} if self.stream_bits == 8 else dict(
                pe16=torch.empty(B * self.NP, C, dtype=torch.int16, device=self.dev),
                x16=torch.empty(M, C, dtype=torch.int16, device=self.dev), y16=torch.empty(M, C, dtype=torch.int16, device=self.dev),
                k16=torch.empty(M, C, dtype=torch.int16, device=self.dev),
                cls16=torch.empty(B, C, dtype=torch.int16, device=self.dev))),
            **({} if self.head is None else dict(
                logits=torch.empty(B, self.head["N"], dtype=torch.int32, device=self.dev),
                logits_f=torch.empty(B, self.head["N"], dtype=torch.float32, device=self.dev))),
            top1=torch.empty(B, dtype=torch.int32, device=self.dev),
            topk=torch.empty(B * TOPK_MAX, dtype=torch.int32, device=self.dev),
        )

    def _w(self, lin, epi, M, blocks, row0=0):
        """(weight pointer, layout bit) for M rows through epilogue `epi` (gemm_forms.weight); blocks = False: row-major whatever
        the shape (the class rows, the block_operands switch).  row0: the weight from that output channel on (a multiple of 64:
        the same byte offset row0 * K in all three layouts)"""
        W, bit = gemm_forms.weight(lin, epi, M, frags=blocks and self.weight_frags, blocks=blocks)
        assert row0 % 64 == 0
        return _lib.ptr(W.view(-1)[row0 * lin["K"]:] if row0 else W), bit

    def _compact(self, on=True):
        """Alias workspaces whose lifetimes do not overlap, so that one layer touches ~230 MB instead of ~430 MB at batch
        256 (the Infinity Cache holds 256 MB): the residual QuantActs run in place (x2 = x; the epilogue's thread reads a
        residual chunk and writes the same chunk), the attention output reuses the LayerNorm buffer (consumed by the qkv
        GEMM before attention starts), q/k/v live inside the fc1 / GELU buffer (dead before fc1 writes it)."""
        ws = self.ws
        if "_own" not in ws:
            ws["_own"] = {k: ws[k] for k in ("x2", "ao", "qkv")}
        if on:
            ws["x2"] = ws["x"]
            ws["ao"] = ws["h"]
            ws["qkv"] = ws["f1"].view(-1)[: ws["_own"]["qkv"].numel()]
        else:
            ws.update(ws["_own"])

    def _gemm(self, A, lda, lin, out, ldo, M, st, a_blocks=False, blocks=False, out_blocks=False, bits=8):
        """GEMM + its QuantAct; bits = 4: a stream site of the 4-bit engine (the patch embedding)"""
        w, lay = self._w(lin, gemm_forms.RQ, M, blocks)
        lay |= (gemm_forms.A_BLOCKS if a_blocks else 0) | (gemm_forms.OUT_BLOCKS if out_blocks else 0)
        if bits == 8:
            _lib.call("ivit_gemm_i8_requant_ex", _lib.ptr(A), lda, w, lin["K"], _lib.ptr(lin["b"]),
                      _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(out), ldo, M, lin["N"], lin["K"], lay, st)
        else:
            _lib.call("ivit_gemm_i8_requant_bits_ex", _lib.ptr(A), lda, w, lin["K"], _lib.ptr(lin["b"]),
                      _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(out), ldo, M, lin["N"], lin["K"], lay, bits, st)

    def _gemm_res(self, A, lda, lin, res, me4, out, M, st, blocks=False, a_blocks=False, ldr=None):
        """projection / fc2 + its QuantAct + the block's residual QuantAct (in place when out is res).  On the 16-bit stream the
        GEMM requantises to 16 bits per channel; without fuse_res16 that GEMM and the two-operand residual kernel are separate.
        ldr: row stride of `res` on the 8-bit stream (default C)"""
        C, r = self.C, me4
        ldr = C if ldr is None else ldr
        if self.stream_bits == 16 and not self.fuse_res16:
            k16 = self.ws["k16"]
            _lib.call("ivit_gemm_i8_requant_i16", _lib.ptr(A), lda, _lib.ptr(lin["W"]), lin["K"], _lib.ptr(lin["b"]),
                      _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(k16), C, M, C, lin["K"], st)
            _lib.call("ivit_residual_requant_i16", _lib.ptr(k16), 16, None, None, r[0], r[1], _lib.ptr(res), r[2], r[3],
                      _lib.ptr(out), M, C, 0, 0, 0, 0, st)
            return
        probe = self.probe
        if probe is not None:
            # bench.py's separate instrumented pass (never inside its timed region): HIP events around the dominant kernel
            probe.begin("gemm_resid", st)
        w, lay = self._w(lin, gemm_forms.RESID if self.stream_bits != 16 else gemm_forms.RQ16_RES16, M, blocks)
        lay |= gemm_forms.A_BLOCKS if a_blocks else 0
        if self.stream_bits == 8:
            _lib.call("ivit_gemm_i8_requant_residual_ex", _lib.ptr(A), lda, w, lin["K"],
                      _lib.ptr(lin["b"]), _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(res), ldr,
                      r[0], r[1], r[2], r[3], _lib.ptr(out), C, M, lin["N"], lin["K"], lay, st)
        elif self.stream_bits == 4:      # attn.qact3 / mlp.qact2 and the block's residual QuantAct, both at 4 bits
            _lib.call("ivit_gemm_i8_requant_residual_bits_ex", _lib.ptr(A), lda, w, lin["K"],
                      _lib.ptr(lin["b"]), _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(res), ldr,
                      r[0], r[1], r[2], r[3], _lib.ptr(out), C, M, lin["N"], lin["K"], lay, 4, 4, st)
        else:
            # the weights-in-registers form where it applies, else the 128 x 128-tile kernel (any shape; no block layouts)
            _lib.call("ivit_gemm_i8_requant_i16_residual_i16_ex", _lib.ptr(A), lda, w,
                      lin["K"], _lib.ptr(lin["b"]), _lib.ptr(lin["m"]), _lib.ptr(lin["e"]), _lib.ptr(res), C, r[0], r[1], r[2], r[3],
                      _lib.ptr(out), C, M, C, lin["K"], lay, st)
        if probe is not None:
            probe.end("gemm_resid", st, (M, lin["N"], lin["K"]))

    def _patchify(self, images, B, st):
        ws = self.ws
        if images.dtype == torch.uint8 and self.input_lut is None:
            self.set_input_normalisation()
        if self.IMG_H != self.IMG_W:      # the h x w entries; a square model keeps the launches it always had
            if images.dtype == torch.uint8:
                _lib.call("ivit_quantize_patchify_hw_u8_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 3 * self.P * self.P, B, 3, self.IMG_H,
                          self.IMG_W, self.P, _lib.ptr(self.input_lut), st)
            else:
                _lib.call("ivit_quantize_patchify_hw_f32_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 3 * self.P * self.P, B, 3, self.IMG_H,
                          self.IMG_W, self.P, self.inv_s0, st)
        elif images.dtype == torch.uint8:
            _lib.call("ivit_quantize_patchify_u8_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), 3 * self.P * self.P, B, 3, self.IMG, self.P,
                      _lib.ptr(self.input_lut), st)
        else:
            _lib.call("ivit_quantize_patchify_f32_i8", _lib.ptr(images), _lib.ptr(ws["a0"]), B, 3, self.IMG, self.P, self.inv_s0, st)

    # ------------------------------------------------------------------ forward
    def forward(self, images: torch.Tensor, taps: dict | None = None, cls_tail: bool = False):
        """images: float32 (or uint8) [B,3,H,W] on the engine's device (224 x 224 unless img_size says otherwise).  Returns (logits_int32 [B,classes],
        logits_f32 [B,classes], top1 int32 [B]) -- views of the engine's workspace, valid until the
        next call.  `taps` (debug/tests) receives clones of intermediate int8 tensors.
        cls_tail: the last block on the class rows only, as the graph replays run it (tests, profiling); the same results."""
        return self._forward(images, taps, cls_tail=cls_tail)

    @property
    def cls_tail_ok(self):
        """the engines whose last block can run on the class rows alone (_cls_block)"""
        return self.family == "ivit" and self.stream_bits == 8 and self.T <= 207

    # what forward_graph / forward_topk_graph capture (graph.py): the pruned last block wherever it exists
    def _graph_forward(self, images):
        return self._forward(images, cls_tail=self.cls_tail_ok)

    def _graph_forward_topk(self, images, k, targets, hits):
        return self._forward(images, None, (k, targets, hits), cls_tail=self.cls_tail_ok)

    def _cls_block(self, blk, x, B, st, a_ln, blk_l):
        """The last block when only token 0 of its output is read (vit_quant.py:302-304): K and V for every token, everything
        else -- Q, attention, projection, MLP, both residual QuantActs -- for the B class rows (row b * T of x).  Every operator
        on that path is row-wise except attention, which ivit_attention_cls_i8 runs for the one query: the rows computed are
        bit for bit those of the full block.  -> the block's output for the class rows, dense [B, C]"""
        C, H, hd, T = self.C, self.H, self.hd, self.T
        M, ws, q = B * T, self.ws, blk["qkv"]
        layernorm(blk["ln1"], x, C, M, C, ws["h"], C, st, blocks=a_ln)
        kvw, kvlay = self._w(q, gemm_forms.QKV, M, blk_l, row0=C)
        _lib.call("ivit_gemm_i8_requant_qkv_planes_ex", _lib.ptr(ws["h"]), C, kvw, q["K"], _lib.ptr(q["b"][C:]),
                  _lib.ptr(q["m"][C:]), _lib.ptr(q["e"][C:]), _lib.ptr(ws["qkv"]), T, H, hd, 1, 2, M, 2 * C, C, kvlay | (gemm_forms.A_BLOCKS if a_ln else 0), st)
        layernorm(blk["ln1"], x, T * C, B, C, ws["c_h"], C, st, blocks=False)
        self._gemm(ws["c_h"], C, blk["q"], ws["c_q"], C, B, st)
        a = blk["attn"]
        _lib.call("ivit_attention_cls_i8", _lib.ptr(ws["qkv"][M * C:]), _lib.ptr(ws["qkv"][2 * M * C:]), _lib.ptr(ws["c_q"]),
                  _lib.ptr(ws["c_ao"]), C, B, H, T, hd, a["ms"][0], a["ms"][1], a["s_attn"], a["mo"][0], a["mo"][1],
                  _lib.ptr(a["exp2d"]), _lib.ptr(a["band"]), a["band_w"], st)
        self._gemm_res(ws["c_ao"], C, blk["proj"], x, blk["res1"], ws["c_x"], B, st, ldr=T * C)
        layernorm(blk["ln2"], ws["c_x"], C, B, C, ws["c_h"], C, st, blocks=False)
        self._gemm(ws["c_h"], C, blk["fc1"], ws["c_f1"], 4 * C, B, st)
        _lib.call("ivit_shiftgelu_lut_i8_ex", _lib.ptr(ws["c_f1"]), 4 * C, B, 4 * C, _lib.ptr(blk["gelu_lut"]),
                  _lib.ptr(ws["c_f1"]), 4 * C, 0, st)
        self._gemm_res(ws["c_f1"], 4 * C, blk["fc2"], ws["c_x"], blk["res2"], ws["c_y"], B, st)
        return ws["c_y"]

    def attention_maps(self, images: torch.Tensor, layers=None, rows: str = "cls"):
        """The integer softmax probabilities of the selected blocks -> ({layer: uint8 [B, H, R, T]}, scale 2^-7): R = 1 (rows="cls":
        the class token's attention over every token) or R = T (rows="all": the full map).  layers: block indices (None: every
        block).  The ordinary eager forward runs -- its logits stay in the workspace as after forward() -- and behind the qkv GEMM
        of each selected block one more launch (engine_common.attention_probs) writes the P that the fused attention kernel
        multiplies with V into a fresh tensor.  8-bit softmax output only; not part of taps, of the graph replays or of cls_tail."""
        if self.softmax_bits != 8:
            raise ValueError(f"attention_maps: the softmax output is {self.softmax_bits} bits wide (the probability kernel writes 8-bit "
                             "probabilities only)")
        if rows not in ("cls", "all"):
            raise ValueError(f"rows={rows!r}: 'cls' (the class token's row) or 'all' (the full map)")
        layers = range(self.D) if layers is None else [int(i) for i in layers]
        if any(not 0 <= i < self.D for i in layers):
            raise ValueError(f"layers {list(layers)}: block indices in 0..{self.D - 1}")
        B, R = images.shape[0], 1 if rows == "cls" else self.T
        maps = {i: torch.empty(B, self.H, R, self.T, dtype=torch.uint8, device=self.dev) for i in layers}
        self._forward(images, maps=maps, stop="features" if self.head is None else None)      # (a headless engine ends behind the final norm)
        return maps, 2.0 ** -7

    def forward_features(self, images: torch.Tensor, integers: bool = False, out: torch.Tensor | None = None):
        """The class embedding -> (features [B, C], scale): the tensor qact2 returns behind the final norm, the first value of the
        reference's forward_features (vit_quant.py:302-305).  features: float32, the integers times scale in one float32
        multiplication (ivit_dequant_rows_i8_f32) -- that tensor bit for bit; integers=True: the int8 integers.  scale: the float32
        act_scaling_factor of qact2.  out=None: a fresh tensor (no workspace view).  out: a [B, C] view of that dtype on the engine's
        device with stride(1) == 1 and any row stride >= C (rows of a feature bank) to write into; TypeError / ValueError for any
        other, before anything is launched.  The forward stops behind the final LayerNorm: no head GEMM, no classifier launch, and
        the last block runs on the class rows alone wherever cls_tail_ok holds.  The workspace logits are left as they were.  A
        headless engine (no head.weight in its source) answers this too."""
        B = images.shape[0]
        out = self._features_out(B, self.C, integers, out)
        self._forward(images, cls_tail=self.cls_tail_ok, stop="features")
        return self._features_emit(self.ws["cls"], B, self.C, self.s_feat, out), self.s_feat

    def _graph_features(self, images, integers):
        """what forward_features_graph captures -> (features, scale), features in a tensor the graph owns"""
        return self.forward_features(images, integers)

    def forward_intermediates_early(self, images: torch.Tensor, indices=None, integers: bool = False):
        """forward_intermediates with an early stop: nothing behind the last selected block is launched -- no later block, final
        norm, head or classifier.  The maps and scales are those of forward_intermediates; the workspace logits (and the class
        embedding) are then STALE, those of an earlier call.  (A method of its own: forward_intermediates keeps its parameters.)"""
        return self._intermediates(images, indices, integers, True)

    def forward_intermediates(self, images: torch.Tensor, indices=None, integers: bool = False):
        """The residual stream behind the selected blocks as feature maps -> (maps, scales): maps = {index: float32 [B, C, Gh, Gw]}
        (the patch grid: (H / P, W / P)), the tensor blocks.i.qact4 returns in the reference (integers times its scale) without the class token, channels first;
        integers=True: the integers themselves (int8; int16 on the 16-bit stream).  scales = {index: float}, the float32
        act_scaling_factor of blocks.i.qact4.  indices: block indices (None: every block); ValueError for one out of range or
        repeated, before anything is launched.  The ordinary eager forward runs -- its logits stay in the workspace as after
        forward() -- and behind the second residual GEMM of each selected block one more launch (engine_common.tokens_to_nchw)
        writes the stream into a fresh tensor.  Not part of taps, of the graph replays or of cls_tail (which never computes the
        last block's stream).  A headless engine stops behind the last selected block (forward_intermediates_early)."""
        return self._intermediates(images, indices, integers, self.head is None)

    def _intermediates(self, images, indices, integers, stop_early):
        idx = intermediate_indices(indices, self.D, "block")
        B = images.shape[0]
        dt = torch.float32 if not integers else torch.int16 if self.stream_bits == 16 else torch.int8
        feats = {i: torch.empty(B, self.C, *self.grid, dtype=dt, device=self.dev) for i in idx}
        self._forward(images, feats=feats, stop=max(idx) if stop_early else None)
        return feats, {i: self.blocks[i]["s_out"] for i in idx}

    def _ln_tokens(self, i):
        """the constants of the final norm on the output of block i (ln_spec at that block's output scale), cached per index"""
        if i not in self._ln_tok:
            self._ln_tok[i] = ln_spec(self._norm_lp, self._upload, self.blocks[i]["s_out"], 16 if self.stream_bits == 16 else 8,
                                      self._norm_shift, self.int_sqrt)
        return self._ln_tok[i]

    def forward_tokens(self, images: torch.Tensor, indices=None, fmt: str = "NLC", prefix: bool = True, integers: bool = False):
        """The final-normed token sequence behind the selected blocks -> (tokens, prefix_tokens, scale): for block index i what
        model.norm returns when called on the pair blocks[i] returns -- for i = D - 1 the reference's own tensor (vit_quant.py:302
        before its [:, 0]), for i < D - 1 timm's norm=True.  tokens = {i: float32 [B, Gh * Gw, C]} (fmt "NLC") or {i: float32
        [B, C, Gh, Gw]} ("NCHW"), the patch tokens; prefix_tokens = {i: float32 [B, 1, C]}, the class token (prefix=False: {});
        scale: float32 [C], the per-channel scaling factor the module returns beside it (the same for every index).
        indices: block indices (None: the last block); ValueError for one out of range or repeated, before anything is launched.
        The ordinary eager forward runs -- its logits stay in the workspace as after forward() -- and behind the second residual
        GEMM of each selected block one launch (engine_common.layernorm_f32: the LayerNorm straight from the integer stream to
        float32, no float intermediate) writes the tokens, under NCHW one more small one the class rows.  A headless engine stops
        behind the last selected block.  Not part of taps, of the graph replays or of cls_tail.
        integers=True (the last block alone: ValueError otherwise): the tensor qact2 gives for the whole normed sequence -- int8
        tokens and class rows in the same shapes, scale = the float s_feat; the class row is forward_features(integers=True) bit
        for bit, the rows can go into a knn.FeatureBank."""
        token_format(fmt)
        idx = [self.D - 1] if indices is None else intermediate_indices(indices, self.D, "block")
        if integers and idx != [self.D - 1]:
            raise ValueError(f"integers=True: qact2 belongs to the last block's norm; indices must be ({self.D - 1},) or None, not {idx}")
        B, C, T, NP = images.shape[0], self.C, self.T, self.NP
        tokens, prefixes = {}, {}

        def emit(i, x, st):
            if integers:
                q = torch.empty(B * T, C, dtype=torch.int8, device=self.dev)
                layernorm(self.ln_f, x, C, B * T, C, q, C, st, blocks=False)
                q = q.view(B, T, C)
                if prefix:
                    prefixes[i] = q[:, :1]
                if fmt == "NLC":
                    tokens[i] = q[:, 1:]
                else:
                    tokens[i] = torch.empty(B, C, *self.grid, dtype=torch.int8, device=self.dev)
                    tokens_to_nchw(q, C, B, T, 1, NP, C, 1.0, tokens[i], st)
                return
            ln = self._ln_tokens(i)
            if fmt == "NLC":
                t0 = 0 if prefix else 1
                full = torch.empty(B, T - t0, C, dtype=torch.float32, device=self.dev)
                layernorm_f32(ln, x, C, B, T, t0, T - t0, C, full, C, st)
                tokens[i] = full[:, 1 - t0:]
                if prefix:
                    prefixes[i] = full[:, :1]
                return
            tokens[i] = torch.empty(B, C, *self.grid, dtype=torch.float32, device=self.dev)
            layernorm_f32(ln, x, C, B, T, 1, NP, C, tokens[i], NP, st, fmt="NCHW")
            if prefix:
                prefixes[i] = torch.empty(B, 1, C, dtype=torch.float32, device=self.dev)
                layernorm_f32(ln, x, C, B, T, 0, 1, C, prefixes[i], C, st)

        self._forward(images, toks={i: emit for i in idx}, stop=max(idx) if self.head is None else None)
        return {i: tokens[i] for i in idx}, {i: prefixes[i] for i in idx if prefix}, (self.s_feat if integers else self.ln_f["s"])

    def _forward(self, images: torch.Tensor, taps: dict | None = None, topk=None, cls_tail: bool = False, maps: dict | None = None,
                 feats: dict | None = None, stop=None, toks: dict | None = None):
        """forward; topk = (k, targets, hits): the classifier launch is the top-k selection (forward_topk).
        stop: None the whole forward; "features": return behind the final LayerNorm (forward_features: no head GEMM, no classifier
        launch); a block index: return behind that block (forward_intermediates_early).  A headless engine needs one.
        cls_tail: the last block through _cls_block (cls_tail_ok engines, no taps).
        maps: {block index: uint8 [B, H, R, T]} to fill with the softmax probabilities of those blocks (attention_maps).
        feats: {block index: [B, C, Gh, Gw]} to fill with the stream behind those blocks, class token dropped (forward_intermediates).
        toks: {block index: emit(index, stream, hip stream)} called behind those blocks (forward_tokens).
        stream_bits = 4: the 8-bit dataflow; the six stream QuantActs clamp to [-8, 7] (the `_bits` entries), attention is the
        "wide" form with softmax_bits.
        stream_bits = 16: the same dataflow with an int16 residual stream.  The patch GEMM, the embedding assembly and the
        projection / fc2 GEMMs write 16 bits (csrc/swin.hip's kernels), LayerNorm reads int16 rows, attention is the "wide"
        form (softmax_bits); qkv / fc1 / GELU are the int8 kernels unchanged, every operand in row-major order."""
        assert images.is_cuda and images.dtype in (torch.float32, torch.uint8) and images.is_contiguous()
        B = images.shape[0]
        assert images.shape[1:] == (3, self.IMG_H, self.IMG_W) and 0 < B <= self.max_batch
        if stop is None:
            self._require_head("forward")
        wide = self.stream_bits == 16
        if wide and taps is not None:
            raise NotImplementedError("taps are not recorded on the 16-bit-stream path")
        if cls_tail and (taps is not None or not self.cls_tail_ok):
            raise ValueError("cls_tail: I-ViT operators, 8-bit stream, at most 207 tokens, no taps (ivit_attention_cls_i8 has no width)")
        C, H, hd, T = self.C, self.H, self.hd, self.T
        M = B * T
        ws = self.ws
        st = self._stream()

        # GEMM operands in the block layout whenever the calls go to the tile-looping kernels (C is the narrowest GEMM's N and K)
        blk_l = bool(self.block_operands) and gemm_forms.block_operands_apply(M, C, C)    # weights (always) and, per producer, activations
        a_ln, a_at, a_ge = (blk_l and not wide and self.block_a[k] for k in ("ln", "attn", "gelu"))

        def tap(name, t, shape, blocks=False):
            if taps is not None:
                if blocks:   # back to rows for the caller
                    rows, K = int(np.prod(shape[:-1])), shape[-1]
                    _lib.call("ivit_untile_operand_i8", _lib.ptr(t), rows, K, _lib.ptr(ws["untile"]), K, st)
                    t = ws["untile"]
                taps[name] = t.reshape(-1)[: int(np.prod(shape))].view(shape).clone()

        self._patchify(images, B, st)
        if wide:
            pt = self.patch
            _lib.call("ivit_gemm_i8_requant_i16", _lib.ptr(ws["a0"]), 3 * self.P * self.P, _lib.ptr(pt["W"]), pt["K"], _lib.ptr(pt["b"]),
                      _lib.ptr(pt["m"]), _lib.ptr(pt["e"]), _lib.ptr(ws["pe16"]), C, B * self.NP, C, pt["K"], st)
            # the fused epilogue's thread reads a residual chunk and writes the same chunk: in place unless fuse_res16 is off
            x, x2 = ws["x16"], (ws["x16"] if self.fuse_res16 else ws["y16"])
        else:
            self._gemm(ws["a0"], 3 * self.P * self.P, self.patch, ws["pe"], C, B * self.NP, st,
                       blocks=bool(self.block_operands), bits=self.stream_bits)
            tap("patch_embed.qact", ws["pe"], (B, self.NP, C))
            x, x2 = ws["x"], ws["x2"]
        if self.stream_bits == 4:
            _lib.call("ivit_embed_assemble_i8_bits", _lib.ptr(ws["pe"]), _lib.ptr(self.pos_add), _lib.ptr(self.cls_row), self.embed_me[0],
                      self.embed_me[1], _lib.ptr(x), B, T, C, 4, st)
        else:
            _lib.call("ivit_embed_assemble_i16" if wide else "ivit_embed_assemble_i8", _lib.ptr(ws["pe16" if wide else "pe"]),
                      _lib.ptr(self.pos_add), _lib.ptr(self.cls_row), self.embed_me[0], self.embed_me[1], _lib.ptr(x), B, T, C, st)
        tap("qact1", x, (B, T, C))
        y_cls = None
        for i, blk in enumerate(self.blocks):
            p = f"blocks.{i}."
            if cls_tail and i == self.D - 1:
                y_cls = self._cls_block(blk, x, B, st, a_ln, blk_l)
                break
            layernorm(blk["ln1"], x, C, M, C, ws["h"], C, st, blocks=a_ln)
            tap(p + "qact1", ws["h"], (B, T, C), a_ln)
            q = blk["qkv"]
            qw, qlay = self._w(q, gemm_forms.QKV, M, blk_l)
            _lib.call("ivit_gemm_i8_requant_qkv_ex", _lib.ptr(ws["h"]), C, qw, q["K"], _lib.ptr(q["b"]),
                      _lib.ptr(q["m"]), _lib.ptr(q["e"]), _lib.ptr(ws["qkv"]), T, H, hd, M, 3 * C, C, qlay | (gemm_forms.A_BLOCKS if a_ln else 0), st)
            tap(p + "attn.qkv_headmajor", ws["qkv"], (3, B, H, T, hd))
            if maps is not None and i in maps:
                attention_probs(blk["attn"], self.family, ws["qkv"], maps[i], B, H, T, hd, maps[i].shape[2], st)
            attention(blk["attn"], self.family, ws["qkv"], ws["ao"], B, H, T, hd, st, blocks=a_at,
                      softmax_bits=self.softmax_bits if self.stream_bits != 8 else None)
            tap(p + "attn.qact2", ws["ao"], (B, T, C), a_at)
            self._gemm_res(ws["ao"], C, blk["proj"], x, blk["res1"], x2, M, st, blocks=blk_l, a_blocks=a_at)
            tap(p + "qact2", x2, (B, T, C))
            layernorm(blk["ln2"], x2, C, M, C, ws["h"], C, st, blocks=a_ln)
            tap(p + "qact3", ws["h"], (B, T, C), a_ln)
            # mlp.fc1 writes the block layout and GELU works IN PLACE on it: the 155 MB intermediate exists once, so the pair
            # (GELU output, fc2 operand) stays inside the 256 MB Infinity Cache (separate buffers: 310 MB; -0.18 ms / forward)
            f1 = blk["fc1"]
            f1w, f1lay = self._w(f1, gemm_forms.RQ, M, blk_l) if self.family == "ibert" and self.fuse_ibert_gelu and taps is None else (None, 0)
            if f1lay & gemm_forms.FRAGS:
                # I-BERT GELU + mlp.qact1 is a map of the requantised byte alone (no row maximum): applied in the fc1 epilogue,
                # the GELU kernel and its pass over the 4C-wide intermediate disappear
                g_buf = ws["f1"]
                _lib.call("ivit_gemm_i8_requant_lut_ex", _lib.ptr(ws["h"]), C, f1w, f1["K"], _lib.ptr(f1["b"]),
                          _lib.ptr(f1["m"]), _lib.ptr(f1["e"]), _lib.ptr(blk["gelu_lut"]), _lib.ptr(g_buf), 4 * C, M, f1["N"], f1["K"],
                          f1lay | (gemm_forms.A_BLOCKS if a_ln else 0) | (gemm_forms.OUT_BLOCKS if a_ge else 0), st)
            else:
                self._gemm(ws["h"], C, f1, ws["f1"], 4 * C, M, st, a_blocks=a_ln, blocks=blk_l, out_blocks=a_ge)
                tap(p + "mlp.qact_gelu", ws["f1"], (B, T, 4 * C), a_ge)
                g_buf = ws["f1"] if self.gelu_in_place or wide else ws["g"]
                _lib.call("ivit_shiftgelu_lut_i8_ex", _lib.ptr(ws["f1"]), 4 * C, M, 4 * C, _lib.ptr(blk["gelu_lut"]),
                          _lib.ptr(g_buf), 4 * C, 3 if a_ge else 0, st)
            tap(p + "mlp.qact1", g_buf, (B, T, 4 * C), a_ge)
            self._gemm_res(g_buf, 4 * C, blk["fc2"], x2, blk["res2"], x, M, st, blocks=blk_l, a_blocks=a_ge)
            tap(p + "qact4", x, (B, T, C))
            if feats is not None and i in feats:
                tokens_to_nchw(x, C, B, T, 1, T - 1, C, blk["s_out"], feats[i], st)
            if toks is not None and i in toks:
                toks[i](i, x, st)
            if stop == i:      # (never "features": block indices are ints)
                return None
        # final LayerNorm is row-wise and only the cls row is consumed (vit_quant.py:302-304); the int16 kernels want dense rows
        if wide:
            ws["cls16"][:B].copy_(x.view(-1, T, C)[:B, 0])
            layernorm(self.ln_f, ws["cls16"], C, B, C, ws["cls"], C, st, blocks=False)
        elif y_cls is not None:
            layernorm(self.ln_f, y_cls, C, B, C, ws["cls"], C, st, blocks=False)
        else:
            layernorm(self.ln_f, x, T * C, B, C, ws["cls"], C, st, blocks=False)
        tap("qact2", ws["cls"], (B, C))
        if stop == "features":
            return None
        hd_ = self.head
        _lib.call("ivit_gemm_i8_i32", _lib.ptr(ws["cls"]), C, _lib.ptr(hd_["W"]), hd_["K"], _lib.ptr(hd_["b"]),
                  _lib.ptr(ws["logits"]), hd_["N"], B, hd_["N"], C, st)
        return self._classify(B, st, topk)

    __call__ = forward
