"""inference.evaluate_video_segmentation end to end on a synthetic DeiT of depth 2: the protocol's loop (first frame in slot 0, a ring of
the previous frames with their propagated labels) restated step by step on propagate.TokenMemory, whose kernels
tests/test_gpu_propagate.py pins to numpy."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd.dense import patch_labels  # noqa: E402
from ivit_amd.inference import evaluate_video_segmentation  # noqa: E402
from ivit_amd.propagate import TokenMemory  # noqa: E402

DEV = "cuda:0"


def test_evaluate_video_segmentation_end_to_end():
    from test_gpu_vit16_lazy import W8, _images
    r, H, W, L, objects, radius, k, T = 16, 64, 96, 3, 2, 2, 3, 0.1
    torch.manual_seed(7)
    model = ivit.VisionTransformer(img_size=(H, W), patch_size=r, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   num_classes=5, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
    imgs = _images(8, 224, torch.Generator(device="cpu").manual_seed(3))[:, :, :H, :W].contiguous()
    with torch.no_grad():
        model(imgs[:4])
    ivit.freeze_model(model)
    frames = imgs[:L]
    masks = torch.randint(0, objects + 1, (L, H // 8, W // 8), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    masks = masks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)
    got = evaluate_video_segmentation(model, [(frames, masks[0], masks, objects)], DEV, n_last=1, radius=radius, k=k, T=T, batch=2)

    Gh, Gw, K = H // r, W // r, objects + 1
    tok = model.forward_tokens(frames.to(DEV), integers=True)[0]
    tok = tok[max(tok)]
    lab = patch_labels(masks[:1].to(DEV).contiguous(), r, K).reshape(-1).long()
    mem = TokenMemory(Gh, Gw, 192, K, 2, DEV)
    mem.put(0, tok[0], torch.nn.functional.one_hot(lab, K).float())
    seg1 = mem.propagate(tok[1], radius, k, T, frames=1)
    mem.put(1, tok[1], seg1)
    seg2 = mem.propagate(tok[2], radius, k, T, frames=2)
    ious = []
    for t, seg in ((1, seg1), (2, seg2)):
        up = torch.nn.functional.interpolate(seg.t().reshape(1, K, Gh, Gw), scale_factor=r, mode="bilinear", align_corners=False)
        pred = up[0].argmax(dim=0).cpu()
        for o in range(1, K):
            p, g = pred == o, masks[t] == o
            ious.append(float((p & g).sum()) / float((p | g).sum()) if (p | g).any() else 1.0)
    assert got["per_sequence"] == [pytest.approx(100.0 * sum(ious) / len(ious), abs=1e-9)] and got["J_mean"] == got["per_sequence"][0]


def test_a_model_the_kernels_do_not_take_is_refused_before_a_sequence_is_touched():
    class Narrow:
        num_features = 96

        def forward_tokens(self, x, integers=False):
            raise AssertionError("called")

    def sequences():
        raise AssertionError("touched")
        yield

    with pytest.raises(ValueError, match="C=96"):
        evaluate_video_segmentation(Narrow(), sequences(), DEV)
