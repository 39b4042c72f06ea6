"""DeiT / ViT assembly with the reference's module tree and checkpoint keys
(/root/reference/models/vit_quant.py:23-406), running on the MI355X integer kernels.

Two execution paths give bit-identical results:
  * a frozen model (every QuantAct fixed, `freeze_model`) forwards through the fused int8 engine
    (engine.IntViTEngine): int8 activations end to end, ~100 kernel launches per batch;
  * otherwise (calibration, debugging, module-level tests) the modules are called one by one exactly as the
    reference's forward does, each converting float <-> integer views around its HIP kernel.
"""
from __future__ import annotations

from functools import partial

import torch
from torch import nn

from .dispatch import EngineDispatch
from .graph import ModuleGraph
from .layers_quant import DropPath, Mlp, PatchEmbed, trunc_normal_
from .quantization_utils import (QuantAct, QuantLinear, QuantMatMul, get_gelu, get_layernorm, get_softmax)
from .quantization_utils import lazy
from .quantization_utils.layer_selection import _parse_layer_name

__all__ = ["deit_tiny_patch16_224", "deit_small_patch16_224", "deit_base_patch16_224", "vit_base_patch16_224",
           "vit_large_patch16_224", "VisionTransformer"]


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0.0, proj_drop=0.0, bitwidth_out=8,
                 bitwidth_softmax=8, softmax_cls=nn.Softmax):
        super().__init__()
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = QuantLinear(dim, dim * 3, bias=qkv_bias)
        self.qact1 = QuantAct()
        self.qact_attn1 = QuantAct()
        self.qact2 = QuantAct()
        self.proj = QuantLinear(dim, dim)
        self.qact3 = QuantAct(bitwidth_out)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj_drop = nn.Dropout(proj_drop)
        self.int_softmax = softmax_cls(bitwidth_softmax)
        self.matmul_1 = QuantMatMul()
        self.matmul_2 = QuantMatMul()

    def forward(self, x, act_scaling_factor):
        B, N, C = x.shape
        x, s = self.qkv(x, act_scaling_factor)
        x, s_qkv = self.qact1(x, s)
        q, k, v = x.reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        attn, s = self.matmul_1(q, s_qkv, k.transpose(-2, -1), s_qkv)
        attn, s = self.qact_attn1(attn * self.scale, s * self.scale)
        attn, s = self.int_softmax(attn, s)
        x, s = self.matmul_2(self.attn_drop(attn), s, v, s_qkv)
        x, s = self.qact2(x.transpose(1, 2).reshape(B, N, C), s)
        x, s = self.proj(x, s)
        x, s = self.qact3(x, s)
        return self.proj_drop(x), s


class Block(nn.Module):
    def __init__(self, dim, num_heads, softmax_cls, mlp_ratio=4.0, qkv_bias=False, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, act_layer=nn.GELU, norm_layer=nn.LayerNorm, attention_out_bw=8,
                 softmax_bw=8, mlp_out_bw=8, norm2_in_bw=8, att_block_out_bw=8):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.qact1 = QuantAct()
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                              proj_drop=drop, bitwidth_out=attention_out_bw, bitwidth_softmax=softmax_bw,
                              softmax_cls=softmax_cls)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.qact2 = QuantAct(norm2_in_bw)
        self.norm2 = norm_layer(dim)
        self.qact3 = QuantAct()
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop,
                       bitwidth_out=mlp_out_bw)
        self.qact4 = QuantAct(att_block_out_bw)

    def forward(self, x_1, s_1):
        x, s = self.norm1(x_1, s_1)
        x, s = self.qact1(x, s)
        x, s = self.attn(x, s)
        x_2, s_2 = self.qact2(self.drop_path(x), s, x_1, s_1)      # residual 1
        x, s = self.norm2(x_2, s_2)
        x, s = self.qact3(x, s)
        x, s = self.mlp(x, s)
        return self.qact4(self.drop_path(x), s, x_2, s_2)          # residual 2


class VisionTransformer(EngineDispatch, ModuleGraph, nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, representation_size=None, drop_rate=0.0,
                 attn_drop_rate=0.0, drop_path_rate=0.0, patch_embed_bw=8, pos_encoding_bw=8, block_input_bw=8,
                 attention_out_bw=8, softmax_bw=8, mlp_out_bw=8, norm2_in_bw=8, att_block_out_bw=8,
                 gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit"):
        super().__init__()
        if representation_size:
            raise NotImplementedError("pre_logits representation layers are not part of the integer path")
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.depth, self.num_heads = depth, num_heads
        self.geometry = (img_size, patch_size, in_chans, float(mlp_ratio), bool(qkv_bias), qk_scale)
        # 'base_arg_value...' names (layer_selection.py): the family is the base name; the constructor parameters are kept beside it
        parsed = [_parse_layer_name(str(t)) for t in (gelu_type, softmax_type, layernorm_type)]
        self.op_types = tuple(base for base, _ in parsed)
        self.op_params = tuple(params for _, params in parsed)
        gelu_layer, softmax_cls, norm_layer = get_gelu(gelu_type), get_softmax(softmax_type), get_layernorm(layernorm_type)

        self.qact_input = QuantAct()
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      bitwidth_out=patch_embed_bw)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_rate)
        self.qact_pos = QuantAct(pos_encoding_bw)
        self.qact1 = QuantAct(block_input_bw)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], act_layer=gelu_layer,
                  norm_layer=norm_layer, softmax_cls=softmax_cls, attention_out_bw=attention_out_bw,
                  softmax_bw=softmax_bw, mlp_out_bw=mlp_out_bw, norm2_in_bw=norm2_in_bw,
                  att_block_out_bw=att_block_out_bw) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.qact2 = QuantAct()
        self.pre_logits = nn.Identity()
        self.head = QuantLinear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        trunc_normal_(self.pos_embed, std=0.02)
        trunc_normal_(self.cls_token, std=0.02)
        self.apply(self._init_weights)
        self._init_dispatch()

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # ---------------------------------------------------------------- module-by-module path
    def forward_features(self, x):
        B = x.shape[0]
        x, s = self.qact_input(x)
        x, s = self.patch_embed(x, s)
        x = torch.cat((self.cls_token.expand(B, -1, -1), x), dim=1)   # raw float cls row shares the patch scale
        x_pos, s_pos = self.qact_pos(self.pos_embed)
        x, s = self.qact1(x, s, x_pos, s_pos)
        x = self.pos_drop(x)
        for blk in self.blocks:
            x, s = blk(x, s)
        x, s = self.norm(x, s)
        x, s = self.qact2(x[:, 0], s)
        return self.pre_logits(x), s

    # ---------------------------------------------------------------- fused engine path (dispatch.py)
    def _operator_reason(self):
        """None when the fused engine and the integer-carrying module path (lazy.scope) implement this choice of operators: all
        three 'ivit' or all three 'ibert', no constructor parameter in a name but the I-BERT LayerNorm's use_int_sqrt."""
        if len(set(self.op_types)) != 1 or self.op_types[0] not in ("ivit", "ibert"):
            return f"operator family {self.op_types} (fused engine: all three operators 'ivit', or all three 'ibert')"
        for kind, base, params in zip(("gelu", "softmax", "layernorm"), self.op_types, self.op_params):
            for k, v in params.items():
                if not ((kind, base, k) == ("layernorm", "ibert", "use_int_sqrt") and isinstance(v, bool)):
                    return (f"{kind} parameter {k}={v!r} of '{base}' (fused engine: default constructor arguments, or use_int_sqrt "
                            "of the 'ibert' layernorm)")
        return None

    def _carries_integers(self):
        """the integer-carrying module path (lazy.scope) resolves every site by its own module, so it takes any combination of
        'ivit' / 'ibert' operators; a name with constructor parameters other than the I-BERT LayerNorm's use_int_sqrt keeps the
        literal path"""
        for kind, base, params in zip(("gelu", "softmax", "layernorm"), self.op_types, self.op_params):
            if base not in ("ivit", "ibert"):
                return False
            if any(not ((kind, base, k) == ("layernorm", "ibert", "use_int_sqrt") and isinstance(v, bool)) for k, v in params.items()):
                return False
        return True

    @property
    def ln_int_sqrt(self):
        """IBERTIntLayerNorm(use_int_sqrt=True): every LayerNorm of the model takes std from integer_sqrt (ibert_modules.py:143)"""
        return bool(getattr(self.norm, "use_int_sqrt", False))

    def engine_unsupported_reason(self):
        """None when the fused int8 engine computes exactly what this module tree would; else why not."""
        return self._engine_reason(head=True)

    def features_unsupported_reason(self):
        """engine_unsupported_reason() without its head condition: what features, forward_intermediates and attention_maps ask"""
        return self._engine_reason(head=False)

    def _feature_bits(self):
        return int(self.qact2.activation_bit)

    def _carries(self, x):
        return super()._carries(x) and self._carries_integers()

    def _engine_reason(self, head):
        """the checks of both; head: the classifier must exist"""
        bad = self._operator_reason()
        if bad:
            return bad
        if self.embed_dim // self.num_heads != 64 or self.embed_dim % 64:
            return "head_dim != 64"
        img, patch = self.geometry[0], self.geometry[1]
        # img_size: an int or a pair (height, width) (vit_quant.py:204-214 through layers_quant.py:168-175)
        ih, iw = img if isinstance(img, (tuple, list)) and len(img) == 2 else (img, img)
        if (self.geometry[2:] != (3, 4.0, True, None) or not isinstance(ih, int) or not isinstance(iw, int) or not isinstance(patch, int)
                or patch <= 0 or ih % patch or iw % patch or (3 * patch * patch) % 64 or (ih // patch) * (iw // patch) + 1 > 1025):
            return (f"geometry {self.geometry} (fused engine: square patches, 3 channels, height and width % patch_size == 0, "
                    "3 * patch_size^2 % 64 == 0, at most 1025 tokens, mlp_ratio 4, qkv bias)")
        tokens = (ih // patch) * (iw // patch) + 1
        if head and self.num_classes <= 0:
            return "no classification head"
        # every QuantAct of the DeiT / ViT engine is 8 bit, except the 16-bit one inside IBERTIntSoftmax (ibert_modules.py:247) ...
        inner = {f"blocks.{i}.attn.int_softmax.act": 16 for i in range(self.depth)} if self.op_types[0] == "ibert" else {}
        bad = self._width_mismatch(inner)
        self._engine_widths = (8, 8, 8)        # (stream, softmax, position embedding)
        a, m = self.blocks[0].attn.int_softmax, self.blocks[0].mlp.act
        sm_bits = int(getattr(a, "output_bit", 8))
        if bad:
            # ... or the 16-bit residual stream: patch_embed_bw = block_input_bw = attention_out_bw = mlp_out_bw = norm2_in_bw =
            # att_block_out_bw = 16 (vit_quant.py:180-187), softmax_bw and pos_encoding_bw 8 or 16: engine stream_bits = 16
            w16 = {"patch_embed.qact": 16, "qact1": 16, **inner}
            for i in range(self.depth):
                w16.update({f"blocks.{i}.attn.qact3": 16, f"blocks.{i}.mlp.qact2": 16, f"blocks.{i}.qact2": 16, f"blocks.{i}.qact4": 16})
            for pos_bits in (8, 16):
                if self._width_mismatch({**w16, "qact_pos": pos_bits}) is None and sm_bits in (8, 16):
                    bad, self._engine_widths = None, (16, sm_bits, pos_bits)
        if bad:
            # ... or the same six QuantActs at 4 ('--bitwidth 4'), softmax_bw and pos_encoding_bw 4 or 8: engine stream_bits = 4
            w4 = {k: (4 if v == 16 and k not in inner else v) for k, v in w16.items()}
            for pos_bits in (8, 4):
                if self._width_mismatch({**w4, "qact_pos": pos_bits}) is None and sm_bits in (4, 8):
                    bad, self._engine_widths = None, (4, sm_bits, pos_bits)
        if bad:
            return bad
        if (sm_bits != 8 and self._engine_widths[0] == 8) or getattr(m, "output_bit", 8) != 8:
            return "Shiftmax / ShiftGELU output width != 8"
        # the fused I-BERT attention covers 193 .. 207 tokens (csrc/attention.hip), the 16-bit stream's up to 207; only I-ViT on the
        # 8-bit stream has the long-row kernel (208 .. 1025 tokens)
        if self.op_types[0] == "ibert" and not 193 <= tokens <= 207:
            return f"geometry {self.geometry}: {tokens} tokens (fused I-BERT attention: 193 .. 207 tokens)"
        if tokens > 207 and self._engine_widths[0] == 16:
            return f"geometry {self.geometry}: {tokens} tokens (16-bit residual stream: at most 207 tokens)"
        return None

    def _build_engine(self, device, max_batch):
        from .engine import IntViTEngine
        return IntViTEngine(dict(self.state_dict()), self.ranges(), self.embed_dim, self.depth, self.num_heads,
                            device=device, max_batch=max_batch, family=self.op_types[0], **self._engine_operator_args(),
                            img_size=self.geometry[0], patch_size=self.geometry[1],
                            **dict(zip(("stream_bits", "softmax_bits", "pos_bits"),
                                       self._engine_widths if self.features_unsupported_reason() is None else (8, 8, 8))))

    def _engine_operator_args(self):
        return dict(int_sqrt=True) if self.ln_int_sqrt else {}      # a plain model's engine is built with today's arguments

    def forward(self, x):
        if self.takes_engine(x):
            _, logits_f32, _ = self.engine(x.shape[0])(x.contiguous().float())
            return logits_f32.clone()
        if not self.is_frozen():
            self.invalidate_engine()     # running-stat QuantActs replace their range buffers: any snapshot is stale
        # a frozen model run module by module carries int8 between its modules (quantization_utils/lazy.py)
        with lazy.scope(self._carries(x)):
            x, s = self.forward_features(x)
            x, _ = self.head(x, s)
        return x.to_float(boundary=True) if isinstance(x, lazy.QT) else x

    def attention_maps(self, x, layers=None, rows="cls"):
        """The integer softmax probabilities of the selected blocks -> ({layer: uint8 [B, H, R, T]}, scale 2^-7); R = 1 for
        rows="cls" (the class token's attention), R = T for rows="all"; layers: block indices (None: every block).
        Where forward() takes the fused engine this is IntViTEngine.attention_maps: the eager engine forward plus one launch per
        selected block.  Otherwise the modules are called one by one as the reference's forward calls them, with forward hooks on
        the selected int_softmax modules, and their float output is converted back to its integers: the reference's own tensor, at
        the module path's speed.  8-bit softmax output only."""
        if rows not in ("cls", "all"):
            raise ValueError(f"rows={rows!r}: 'cls' (the class token's row) or 'all' (the full map)")
        layers = list(range(self.depth)) if layers is None else [int(i) for i in layers]
        if any(not 0 <= i < self.depth for i in layers):
            raise ValueError(f"layers {layers}: block indices in 0..{self.depth - 1}")
        bits = int(getattr(self.blocks[0].attn.int_softmax, "output_bit", 8))
        if bits != 8:          # on either path, and before an engine is built for it
            raise ValueError(f"attention_maps: the softmax output is {bits} bits wide (8-bit probabilities only)")
        if self.takes_engine_for_features(x):      # (takes_engine's answer for a model with a head)
            return self.engine(x.shape[0]).attention_maps(x.contiguous().float(), layers, rows)
        maps, handles = {}, []

        def hook(i):
            def record(mod, args, out):
                p, s = out
                if isinstance(p, lazy.QT):
                    p = p.to_float()
                q = torch.round(p / s)
                assert bool((q * s == p).all()) and bool((q >= 0).all()) and bool((q <= 128).all()), \
                    f"blocks.{i}.attn.int_softmax: the output is not an integer in [0, 128] times its scale"
                maps[i] = (q[:, :, :1] if rows == "cls" else q).to(torch.uint8).contiguous()
            return record

        for i in layers:
            handles.append(self.blocks[i].attn.int_softmax.register_forward_hook(hook(i)))
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
        return {i: maps[i] for i in layers}, 2.0 ** -7

    def forward_tokens(self, x, indices=None, fmt="NLC", prefix=True, integers=False):
        """The final-normed token sequence behind the selected blocks -> (tokens, prefix_tokens, scale): for block index i what
        self.norm returns when called on the pair blocks[i] returns (i = depth - 1: the tensor of forward_features before its
        [:, 0]; i < depth - 1: timm's norm=True).  tokens = {i: float32 [B, Gh * Gw, C]} (fmt "NLC") or {i: [B, C, Gh, Gw]}
        ("NCHW"); prefix_tokens = {i: float32 [B, 1, C]}, the class token ({} with prefix=False); scale: the float32 [C] scaling
        factor self.norm returns.  indices: block indices (None: the last block); ValueError for one out of range or repeated.
        integers=True (the last block alone): the int8 tensor self.qact2 gives for the whole sequence, with its float scale.
        Where takes_engine_for_features(x) holds this is IntViTEngine.forward_tokens: the eager engine forward plus one launch per
        selected block.  Otherwise the modules are called one by one as the reference's forward calls them, with forward hooks on
        the selected blocks, and self.norm is called on each captured pair: the same tensors bit for bit, at the module path's
        speed."""
        from .engine_common import intermediate_indices, token_format
        token_format(fmt)
        idx = [self.depth - 1] if indices is None else intermediate_indices(indices, self.depth, "block")
        if integers and idx != [self.depth - 1]:
            raise ValueError(f"integers=True: qact2 belongs to the last block's norm; indices must be ({self.depth - 1},) or None, not {idx}")
        if self.takes_engine_for_features(x):
            return self.engine(x.shape[0]).forward_tokens(x.contiguous().float(), idx, fmt, prefix, integers)
        got = self._hooked_outputs(x, {i: self.blocks[i] for i in idx})
        grid = tuple(self.patch_embed.grid_size)
        tokens, prefixes, scale = {}, {}, None
        with torch.no_grad():
            for i in idx:
                y, scale = self.norm(*got[i])
                if integers:
                    y, scale = self.qact2(y, scale)
                    y = torch.round(y / scale).to(torch.int8)
                B, _, C = y.shape
                tokens[i] = y[:, 1:] if fmt == "NLC" else y[:, 1:].permute(0, 2, 1).reshape(B, C, *grid).contiguous()
                if prefix:
                    prefixes[i] = y[:, :1]
        scale = scale.reshape(-1)
        return tokens, prefixes, (float(scale[0]) if integers else scale)

    def forward_intermediates_early(self, x, indices=None, integers=False):
        """forward_intermediates with an early stop: where the fused engine is taken it launches nothing behind the last selected
        block (IntViTEngine.forward_intermediates_early: the same maps and scales; its workspace logits are then stale).  The
        module path (_hooked_intermediates) runs the whole forward regardless."""
        return self._intermediates(x, indices, integers, True)

    def forward_intermediates(self, x, indices=None, integers=False):
        """The residual stream behind the selected blocks as feature maps -> (maps, scales): maps = {index: float32 [B, C, Gh, Gw]}
        (patch_embed.grid_size), what blocks[i] returns (blocks.i.qact4: integers times its scale) without the class token, channels first; integers=True:
        the integers (int8; int16 where that QuantAct is wider than 8 bits).  scales = {index: float}, its float32
        act_scaling_factor.  indices: block indices (None: every block); ValueError for one out of range or repeated.
        Where forward() takes the fused engine this is IntViTEngine.forward_intermediates: the eager engine forward plus one
        launch per selected block.  Otherwise the modules are called one by one as the reference's forward calls them, with
        forward hooks on the selected blocks: the reference's own tensor, at the module path's speed."""
        return self._intermediates(x, indices, integers, False)

    def _intermediates(self, x, indices, integers, stop_early):
        from .engine_common import intermediate_indices
        idx = intermediate_indices(indices, self.depth, "block")
        if self.takes_engine_for_features(x):      # (takes_engine's answer for a model with a head)
            eng = self.engine(x.shape[0])
            return (eng.forward_intermediates_early if stop_early else eng.forward_intermediates)(x.contiguous().float(), idx, integers)
        grid = tuple(self.patch_embed.grid_size)
        got = self._hooked_intermediates(x, {i: (self.blocks[i], f"blocks.{i}", self.blocks[i].qact4, 1, grid) for i in idx}, integers)
        return {i: got[i][0] for i in idx}, {i: got[i][1] for i in idx}


def _factory(embed_dim, depth, num_heads, name):
    def make(pretrained=False, **kwargs):
        if pretrained:
            raise RuntimeError(f"{name}(pretrained=True) downloads weights (vit_quant.py:325-331); there is no network "
                               "here -- load a state_dict instead")
        return VisionTransformer(patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4,
                                 qkv_bias=True, **kwargs)
    make.__name__ = name
    return make


deit_tiny_patch16_224 = _factory(192, 12, 3, "deit_tiny_patch16_224")
deit_small_patch16_224 = _factory(384, 12, 6, "deit_small_patch16_224")
deit_base_patch16_224 = _factory(768, 12, 12, "deit_base_patch16_224")
vit_base_patch16_224 = _factory(768, 12, 12, "vit_base_patch16_224")
vit_large_patch16_224 = _factory(1024, 24, 16, "vit_large_patch16_224")
