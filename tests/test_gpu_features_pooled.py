"""VisionTransformer.features_pooled at model level: the class tokens of the last n blocks and the pooled patch-token mean from the
fused engine, against the literal module path -- use_engine off, forward hooks on the blocks, model.norm then model.qact2 on each
captured pair, the result divided by its scale and rounded, an int64 sum over the patch tokens and floor((2 * sum + T) / (2 * T)).
DeiT-shaped models of depth 3 with synthetic weights and calibrated ranges; integers only, so equality only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")

from test_gpu_vit16_lazy import W8, W16  # noqa: E402

DEV = "cuda:0"
D = 3
#        embed, heads, image, family, stream bits
CASES = {"ivit8_rect": (192, 3, (64, 96), "ivit", 8), "ivit8_224": (192, 3, (224, 224), "ivit", 8),
         "ibert8_224": (192, 3, (224, 224), "ibert", 8), "ivit16_224": (128, 2, (224, 224), "ivit", 16)}
_BUILT = {}


def _images(n, hw, g):
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=hw, mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, *hw, generator=g)).to(DEV)


def _literal(model, x):
    """int8 [B, D * C + C]: every block's class row behind norm + qact2, then the pooled mean of the last block; and qact2's scale"""
    got, handles = {}, []
    for i in range(D):
        handles.append(model.blocks[i].register_forward_hook(lambda m, a, out, i=i: got.__setitem__(i, out)))
    model.use_engine = False
    try:
        with torch.no_grad():
            assert not model.takes_engine_for_features(x)
            model.forward_features(x)
            segs = []
            for i in range(D):
                y, s = model.qact2(*model.norm(*got[i]))
                q = torch.round(y / s).to(torch.int64)
                assert int(q.abs().max()) <= 128
                segs.append(q[:, 0])
            T = q.shape[1] - 1
            segs.append(torch.div(2 * q[:, 1:].sum(1) + T, 2 * T, rounding_mode="floor"))
            return torch.cat(segs, 1).to(torch.int8), float(s.reshape(-1)[0])
    finally:
        model.use_engine = True
        for h in handles:
            h.remove()


def _case(name):
    """(frozen model, images [2, 3, h, w], literal reference, scale), built once per case"""
    if name not in _BUILT:
        C, heads, hw, family, bits = CASES[name]
        torch.manual_seed(sum(hw) + bits)
        model = ivit.VisionTransformer(img_size=hw[0] if hw[0] == hw[1] else hw, patch_size=16, embed_dim=C, depth=D, num_heads=heads,
                                       mlp_ratio=4, qkv_bias=True, num_classes=40, gelu_type=family, softmax_type=family,
                                       layernorm_type=family, **(W16 if bits == 16 else W8)).to(DEV).eval()
        with torch.no_grad():
            for p in model.parameters():          # wider weights than the init's 0.02: activations that use their ranges
                if p.dim() > 1:
                    p.mul_(3.0)
            for blk in model.blocks:
                blk.attn.qkv.weight.mul_(4.0)
            g = torch.Generator(device="cpu").manual_seed(11)
            calib = _images(4, hw, g)
            model(calib)
            model(calib.flip(0) * 0.7)
        ivit.freeze_model(model)
        x = _images(2, hw, g)
        assert model.features_unsupported_reason() is None, "these configurations are the fused engine's"
        _BUILT[name] = (model, x) + _literal(model, x)
    return _BUILT[name]


def _columns(ref, C, n_last, avgpool):
    return torch.cat([ref[:, (D - n_last) * C:D * C]] + ([ref[:, D * C:]] if avgpool else []), 1)


@pytest.mark.parametrize("avgpool", [False, True])
@pytest.mark.parametrize("n_last", [1, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_features_pooled_equal_the_literal_module_path(name, n_last, avgpool):
    model, x, ref, s = _case(name)
    C = CASES[name][0]
    with torch.no_grad():
        q, scale = model.features_pooled(x, n_last, avgpool)
    want = _columns(ref, C, n_last, avgpool)
    assert q.dtype == torch.int8 and tuple(q.shape) == tuple(want.shape)
    assert torch.equal(q, want)
    assert scale.dtype == torch.float32 and torch.equal(scale.cpu(), torch.full((want.shape[1],), s, dtype=torch.float32))


@pytest.mark.parametrize("name", list(CASES))
def test_out_rows_of_a_wider_bank_and_the_class_feature(name):
    model, x, ref, _ = _case(name)
    C = CASES[name][0]
    W = 3 * C
    bank = torch.full((5 + 2 + 1, W + 64), 91, dtype=torch.int8, device=DEV)
    with torch.no_grad():
        q, _ = model.features_pooled(x, 2, True, out=bank[5:7, :W])
        assert q.data_ptr() == bank[5:7].data_ptr()
        assert torch.equal(bank[5:7, :W], _columns(ref, C, 2, True))
        assert bool((bank[:5] == 91).all()) and bool((bank[7:] == 91).all()) and bool((bank[:, W:] == 91).all())
        assert torch.equal(model.features_pooled(x, 1, False)[0], model.features(x, integers=True)[0])
