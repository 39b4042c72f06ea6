"""forward_tokens at model level: the final-normed token sequence from the fused engines (one float-emitting LayerNorm launch per
selected block, csrc/ln_tokens.h) bit for bit against the literal module path -- use_engine off, no integer carrying, forward hooks
on blocks[i], model.norm called on each captured pair, patch tokens and prefix split by slicing, NCHW by permute.  DeiT models 128
wide, depth 2, 2 heads, patch 16 at 224 px (197 tokens) and 64 x 96 (25 tokens): both operator families and the integer square root,
the 8-, 16- and 4-bit streams, power-of-two and calibrated ranges (the 16-bit stream at calibrated ranges: snapped to powers of two
its projection requantisers leave the GEMM's contract, e >= 31, in these small models).  An I-BERT model at 101 tokens (which the engine declines) from
the module path; Swin of both families (56 px / window 7, and 224 px at Swin-T width, depths (1, 1, 1, 1)) against hooks on
model.norm and model.qact2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd.swin_engine import engine_from_model  # noqa: E402

import test_gpu_swin_ibert_lazy as swin_ibert  # noqa: E402
import test_gpu_swin_lazy as swin_lazy  # noqa: E402
from test_gpu_vit16_lazy import W8, W16  # noqa: E402
from test_gpu_w4_lazy import W4  # noqa: E402

DEV = "cuda:0"
WIDTHS = {8: W8, 16: W16, 4: W4}
_MODELS = {}


def _images(n, hw, g):
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=hw, mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, *hw, generator=g)).to(DEV)


def snap_pow2(model):
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            qmax = 2 ** (mod.activation_bit - 1) - 1
            a = max(-float(mod.x_min), float(mod.x_max)) / qmax
            if a == 0.0:
                continue
            p = 2.0 ** torch.ceil(torch.log2(torch.tensor(a, dtype=torch.float64))).item()
            mod.x_max.fill_(qmax * p)
            mod.x_min.fill_(-qmax * p)


def _vit(hw, family, bits, pow2, int_sqrt=False):
    """the calibrated, frozen DeiT (128 wide, depth 2, 2 heads, patch 16) and a batch of 2, built once per configuration"""
    key = (hw, family, bits, pow2, int_sqrt)
    if key not in _MODELS:
        torch.manual_seed(sum(hw) + bits)
        ln = "ibert_use-int-sqrt_true" if int_sqrt else family
        model = ivit.VisionTransformer(img_size=hw[0] if hw[0] == hw[1] else hw, patch_size=16, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4,
                                       qkv_bias=True, num_classes=40, gelu_type=family, softmax_type=family, layernorm_type=ln,
                                       **WIDTHS[bits]).to(DEV).eval()
        with torch.no_grad():
            for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
                if p.dim() > 1:
                    p.mul_(3.0)
            if bits == 4:                         # (tests/test_gpu_w4_lazy.py: a class row 4 bits can hold)
                model.cls_token.normal_(0.0, 2.0)
                model.pos_embed.normal_(0.0, 0.7)
            for blk in model.blocks:
                blk.attn.qkv.weight.mul_(16.0 if bits == 4 else 4.0)
            g = torch.Generator(device="cpu").manual_seed(11)
            calib = _images(4, hw, g)
            model(calib)
            model(calib.flip(0) * 0.7)
        if pow2:
            snap_pow2(model)
        ivit.freeze_model(model)
        _MODELS[key] = (model, _images(2, hw, g))
    return _MODELS[key]


def _same(a, b):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def _literal_vit(model, x, idx):
    """{i: what model.norm returns on the pair blocks[i] returned}, off the engine and without integer carrying"""
    got, handles = {}, []
    for i in idx:
        handles.append(model.blocks[i].register_forward_hook(lambda m, a, out, i=i: got.__setitem__(i, out)))
    model.use_engine = False
    try:
        with torch.no_grad():
            assert not model.takes_engine_for_features(x)
            model.forward_features(x)
            return {i: model.norm(*got[i]) for i in idx}
    finally:
        model.use_engine = True
        for h in handles:
            h.remove()


VIT_CASES = {
    "ivit8_natural_224": ((224, 224), "ivit", 8, False, False), "ivit8_pow2_rect": ((64, 96), "ivit", 8, True, False),
    "ivit16_natural_rect": ((64, 96), "ivit", 16, False, False), "ivit16_natural_224": ((224, 224), "ivit", 16, False, False),
    "ivit4_natural_rect": ((64, 96), "ivit", 4, False, False), "ivit4_pow2_224": ((224, 224), "ivit", 4, True, False),
    "ibert8_natural_224": ((224, 224), "ibert", 8, False, False), "ibert8_pow2_224": ((224, 224), "ibert", 8, True, False),
    "ibert8_intsqrt_natural_224": ((224, 224), "ibert", 8, False, True), "ibert16_natural_224": ((224, 224), "ibert", 16, False, False),
    "ibert16_intsqrt_natural_224": ((224, 224), "ibert", 16, False, True), "ibert4_natural_224": ((224, 224), "ibert", 4, False, False),
}


@pytest.mark.parametrize("case", list(VIT_CASES))
def test_vit_forward_tokens_equal_the_literal_module_path(case):
    hw, family, bits, pow2, int_sqrt = VIT_CASES[case]
    model, x = _vit(hw, family, bits, pow2, int_sqrt)
    G, B, C, D = (hw[0] // 16, hw[1] // 16), x.shape[0], 128, 2
    assert model.features_unsupported_reason() is None, "these configurations are the fused engine's"
    ref = _literal_vit(model, x, (0, 1))
    with torch.no_grad():
        y = model(x).clone()
        assert model.takes_engine_for_features(x)
        for fmt in ("NLC", "NCHW"):
            tokens, prefixes, scale = model.forward_tokens(x, indices=(0, 1), fmt=fmt)
            assert list(tokens) == list(prefixes) == [0, 1]
            for i in (0, 1):
                want, want_s = ref[i]
                assert scale.dtype == torch.float32 and tuple(scale.shape) == (C,) and torch.equal(scale, want_s.reshape(-1))
                patches = want[:, 1:] if fmt == "NLC" else want[:, 1:].permute(0, 2, 1).reshape(B, C, *G)
                assert tuple(tokens[i].shape) == ((B, G[0] * G[1], C) if fmt == "NLC" else (B, C, *G))
                assert _same(tokens[i], patches), f"block {i} {fmt}: {int((tokens[i] != patches).sum())} of {patches.numel()} differ"
                assert _same(prefixes[i], want[:, :1]), f"block {i} {fmt}: the prefix row"
                assert len(torch.unique(tokens[i])) > 16, "a live tensor"
            assert torch.equal(model(x), y), "the logits of a call right after"
        # defaults: the last block; without the prefix
        tokens, prefixes, _ = model.forward_tokens(x, prefix=False)
        assert list(tokens) == [D - 1] and prefixes == {} and _same(tokens[D - 1], ref[D - 1][0][:, 1:])
        # integers: the whole normed sequence through qact2; its class row is the embedding
        feats, s_feat = model.features(x, integers=True)
        for fmt in ("NLC", "NCHW"):
            q, qp, s = model.forward_tokens(x, fmt=fmt, integers=True)
            assert s == s_feat and q[D - 1].dtype == torch.int8 and torch.equal(qp[D - 1][:, 0], feats)
            f2, s2 = model.qact2(*ref[D - 1])
            want_q = torch.round(f2 / s2).to(torch.int8)
            patches = want_q[:, 1:] if fmt == "NLC" else want_q[:, 1:].permute(0, 2, 1).reshape(B, C, *G)
            assert _same(q[D - 1], patches)
        assert torch.equal(model(x), y)
        # the module path answers the same call with the same contract
        model.use_engine = False
        try:
            tokens, prefixes, scale = model.forward_tokens(x, indices=(1, 0), fmt="NCHW")
            q, qp, s = model.forward_tokens(x, integers=True)
        finally:
            model.use_engine = True
        assert list(tokens) == [1, 0] and torch.equal(scale, ref[0][1].reshape(-1)) and s == s_feat
        for i in (0, 1):
            assert _same(tokens[i], ref[i][0][:, 1:].permute(0, 2, 1).reshape(B, C, *G)) and _same(prefixes[i], ref[i][0][:, :1])
        assert torch.equal(qp[D - 1][:, 0], feats)


def test_a_headless_model_answers_from_the_engine():
    model, x = _vit((64, 96), "ivit", 8, False)
    ref = _literal_vit(model, x, (0,))
    eng = model.engine(x.shape[0])
    head, eng.head = eng.head, None
    try:
        with torch.no_grad():
            tokens, prefixes, _ = eng.forward_tokens(x.contiguous(), (0,))
    finally:
        eng.head = head
    assert _same(tokens[0], ref[0][0][:, 1:]) and _same(prefixes[0], ref[0][0][:, :1])


def test_an_ibert_model_the_engine_declines_answers_from_the_module_path():
    model, x = _vit((160, 160), "ibert", 8, False)      # 101 tokens: below the fused I-BERT attention's 193
    assert model.features_unsupported_reason() is not None
    ref = _literal_vit(model, x, (0, 1))
    with torch.no_grad():
        y = model(x).clone()
        tokens, prefixes, scale = model.forward_tokens(x, indices=(0, 1))
        q, qp, s = model.forward_tokens(x, integers=True)
        feats, s_feat = model.features(x, integers=True)
        assert torch.equal(model(x), y)
    for i in (0, 1):
        assert _same(tokens[i], ref[i][0][:, 1:]) and _same(prefixes[i], ref[i][0][:, :1]) and torch.equal(scale, ref[i][1].reshape(-1))
    assert s == s_feat and torch.equal(qp[1][:, 0], feats)


# =========================================================================================== Swin
def _literal_swin(model, x):
    """(what model.norm returned, what model.qact2 returned) in the module-by-module forward, off the engine"""
    got = {}
    handles = [model.norm.register_forward_hook(lambda m, a, out: got.__setitem__("norm", out)),
               model.qact2.register_forward_hook(lambda m, a, out: got.__setitem__("qact2", out))]
    model.use_engine = False
    try:
        with torch.no_grad():
            model.forward_features(x)
    finally:
        model.use_engine = True
        for h in handles:
            h.remove()
    return got["norm"], got["qact2"]


def _swin_check(model, x, target):
    """target: the model (its dispatch) or an engine"""
    (want, want_s), (qf, qs) = _literal_swin(model, x)
    B, L, C = want.shape
    H, W = model.layers[-1].input_resolution
    want_q = torch.round(qf / qs).to(torch.int8)
    xin = x.contiguous()
    with torch.no_grad():
        for fmt in ("NLC", "NCHW"):
            t, scale = target.forward_tokens(xin, fmt=fmt)
            assert torch.equal(scale, want_s.reshape(-1)) and tuple(scale.shape) == (C,)
            exp = want if fmt == "NLC" else want.permute(0, 2, 1).reshape(B, C, H, W)
            assert _same(t, exp), f"{fmt}: {int((t != exp).sum())} of {exp.numel()} differ"
            q, s = target.forward_tokens(xin, fmt=fmt, integers=True)
            assert s == float(qs.reshape(-1)[0])
            assert _same(q, want_q if fmt == "NLC" else want_q.permute(0, 2, 1).reshape(B, C, H, W))
        assert len(torch.unique(t)) > 16


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_forward_tokens_small(pow2):
    model, x = swin_lazy.built("A", pow2)
    assert model.takes_engine_for_features(x)
    with torch.no_grad():
        y = model(x).clone()
        f0, s0 = model.features(x, integers=True)
    _swin_check(model, x, model)
    _swin_check(model, x, model.engine(x.shape[0]))
    with torch.no_grad():
        f1, s1 = model.features(x, integers=True)
        assert torch.equal(model(x), y) and torch.equal(f0, f1) and s0 == s1


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_swin_ibert_forward_tokens_small(pow2):
    model, x = swin_ibert.built("A", pow2)
    assert not model.takes_engine_for_features(x)
    _swin_check(model, x, model)                                        # routed module by module
    _swin_check(model, x, engine_from_model(model, max_batch=4))       # the engine of the I-BERT family


@pytest.mark.parametrize("family", ["ivit", "ibert"])
def test_swin_t_width_at_224(family):
    torch.manual_seed(224)
    names = swin_ibert.IBERT if family == "ibert" else {}
    model = ivit.SwinTransformer(img_size=224, patch_size=4, embed_dim=96, depths=(1, 1, 1, 1), num_heads=(3, 6, 12, 24), window_size=7,
                                 num_classes=10, **names).to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(7)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
            elif name.endswith("relative_position_bias_table"):
                p.mul_(20.0)
        calib = _images(2, (224, 224), g)
        model(calib)
        model(calib.flip(0) * 0.7)
    ivit.freeze_model(model)
    x = _images(2, (224, 224), g)
    _swin_check(model, x, model if family == "ivit" else engine_from_model(model, max_batch=2))
