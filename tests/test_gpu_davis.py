"""Video segmentation scoring on the GPU: ivit_upsample_argmax_u8, ivit_mask_scores_u8 and inference.evaluate_davis against numpy
(tests/davis_ref.py).  Every comparison is exact equality."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.propagate import TokenMemory, bound_radius, davis_measures, mask_scores, upsample_argmax  # noqa: E402

import davis_ref  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def soft_labels(kind, Gh, Gw, K, rng):
    seg = rng.random((Gh * Gw, K), dtype=np.float32)
    if kind == "tie" and K > 1:          # two classes equal on every cell and above the rest: the lower index wins
        seg[:, K - 1] = seg[:, K // 2 - 1] = seg[:, K // 2 - 1] + np.float32(2.0)
    if kind == "last bit":               # magnitudes 2^-20 .. 2^20 per cell, the classes of a cell 0 .. 3 float32 steps apart
        base = np.ldexp(seg[:, :1] + np.float32(1.0), rng.integers(-20, 21, size=(Gh * Gw, 1))).astype(np.float32)
        seg = (base.view(np.int32) + rng.integers(0, 4, size=seg.shape, dtype=np.int32)).view(np.float32)
    return seg


# the issue's shapes, and one of r = 1: three slabs of classes and two blocks of cells per row
@pytest.mark.parametrize("kind", ["random", "tie", "last bit"])
@pytest.mark.parametrize("Gh,Gw,r,K", [(1, 1, 1, 1), (2, 3, 2, 2), (3, 5, 8, 3), (5, 4, 16, 7), (2, 2, 32, 256), (9, 17, 4, 5), (3, 70, 1, 9)])
def test_upsample_argmax_matches_float64(Gh, Gw, r, K, kind):
    seg = soft_labels(kind, Gh, Gw, K, np.random.default_rng(100 * Gh + r + K))
    want = davis_ref.upsample_argmax(seg, Gh, Gw, r)
    if kind == "tie" and K > 1:
        assert (want == K // 2 - 1).all()
    out = torch.full((Gh * r + 1, Gw * r), 0xA5, dtype=torch.uint8, device=DEV)
    got = upsample_argmax(dev(seg), (Gh, Gw), r, out=out[:Gh * r])
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
    assert (out[Gh * r] == 0xA5).all()


def maps(n, H, W, O, seed):
    truth = davis_ref.blobs(np.random.default_rng(seed), n, H, W, O)
    pred = np.roll(truth, (1, -2), axis=(1, 2))          # boundaries a few pixels from their match
    pred[:, H // 2:, : W // 2] = davis_ref.blobs(np.random.default_rng(seed + 1), n, H, W, O)[:, H // 2:, : W // 2]
    return pred, truth


def check_scores(pred, truth, O, R):
    got = mask_scores(dev(pred), dev(truth), O, bound_th=R)          # (0: ceil(0 * diagonal) = 0 pixels)
    want = davis_ref.mask_scores(pred, truth, O, R)
    assert np.array_equal(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:8]
    return want


@pytest.mark.parametrize("n,H,W,O,R", [(1, 2, 2, 1, 0), (1, 5, 63, 1, 1), (2, 33, 64, 2, 3), (1, 40, 65, 3, 8), (1, 70, 129, 2, 24), (3, 17, 200, 255, 2)])
def test_mask_scores_match_the_reference(n, H, W, O, R):
    assert check_scores(*maps(n, H, W, O, 10 * H + R), O, R)[:, :, 1].any()


def test_mask_scores_empty_cases_and_foreign_labels():
    pred, truth = maps(4, 40, 65, 3, 5)
    pred[0][pred[0] == 2], truth[0][truth[0] == 3] = 0, 0           # object 2 in truth only, object 3 in pred only
    pred[1, 3:9, 3:9], truth[1, 5:12, 2:8] = 7, 200                 # labels above O in both maps
    pred[2] = truth[2]                                              # a perfect frame
    pred[3], truth[3] = 0, 0                                        # all background
    want = check_scores(pred, truth, 3, 2)
    assert want[0, 1, 2] == 0 < want[0, 1, 3] and want[0, 2, 3] == 0 < want[0, 2, 2] and not want[3].any()
    J, F = davis_measures(want)
    assert (J[2] == 1).all() and (F[2] == 1).all() and (J[3] == 1).all() and (F[3] == 1).all() and F[0, 1] == 0 and F[0, 2] == 0


def test_mask_scores_across_tile_seams():
    """single mask pixels (a 2 x 2 boundary each) at R and R + 1 columns / rows, and at the disk's corner, across the seam between
    the tiles: R = 3 puts it behind row 119 (128 - 2 (R + 1) rows per tile) and column 63"""
    R, offsets = 3, [(0, 3), (0, 4), (3, 0), (4, 0), (2, 2), (3, 1), (-3, 0), (0, -4)]
    pred, truth = np.zeros((len(offsets), 130, 70), np.uint8), np.zeros((len(offsets), 130, 70), np.uint8)
    for f, (dy, dx) in enumerate(offsets):
        truth[f, 119, 63], pred[f, 119 + dy + (dy > 0), 63 + dx + (dx > 0)] = 1, 1      # the nearest boundary pixels are (dy, dx) apart
    want = check_scores(pred, truth, 1, R)
    assert want[0, 0, 4] > want[1, 0, 4] and want[2, 0, 4] > want[3, 0, 4] and want[4, 0, 4] > want[5, 0, 4]


@pytest.mark.parametrize("entry,bad,code,word", [("mask", {"R": 25}, -2, "radius=25"), ("up", {"r": 33}, -2, "r=33"), ("up", {"K": 257}, -2, "K=257"),
                                                 ("mask", {"O": 0}, -2, "num_objects=0"), ("mask", {"H": 1}, -2, "H=1"), ("up", {"seg": None}, -1, "NULL")])
def test_refusals(entry, bad, code, word):
    L = _lib.lib()
    seg = torch.zeros(4 * 257, dtype=torch.float32, device=DEV)
    maps8 = torch.full((3, 64, 64), 0xA5, dtype=torch.uint8, device=DEV)
    counts = torch.full((6,), -7, dtype=torch.int64, device=DEV)
    if entry == "up":
        a = {"seg": _lib.ptr(seg), "Gh": 2, "Gw": 2, "r": 2, "K": 2, **bad}
        rc = L.ivit_upsample_argmax_u8(a["seg"], a["Gh"], a["Gw"], a["r"], a["K"], _lib.ptr(maps8[0]), _lib.stream_ptr())
    else:
        a = {"H": 4, "O": 1, "R": 1, **bad}
        rc = L.ivit_mask_scores_u8(_lib.ptr(maps8[1]), _lib.ptr(maps8[2]), 1, a["H"], 4, a["O"], a["R"], _lib.ptr(counts), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code and word in L.ivit_last_error_string().decode()
    assert (maps8 == 0xA5).all() and (counts == -7).all()
    with pytest.raises(ValueError, match="R=25"):
        mask_scores(maps8, maps8, 1, bound_th=25)


def test_evaluate_davis_end_to_end():
    """The wiring of inference.evaluate_davis, not an independent protocol: the same loop restated on TokenMemory, with the numpy
    references in place of the two kernels."""
    from ivit_amd.dense import patch_labels
    from ivit_amd.inference import evaluate_davis
    from test_gpu_vit16_lazy import W8, _images
    r, H, W, L, radius, k, T = 16, 64, 96, 3, 2, 3, 0.1
    torch.manual_seed(7)
    model = ivit.VisionTransformer(img_size=(H, W), patch_size=r, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   num_classes=5, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
    imgs = _images(8, 224, torch.Generator(device="cpu").manual_seed(3))[:, :, :H, :W].contiguous()
    with torch.no_grad():
        model(imgs[:4])
    ivit.freeze_model(model)
    seqs = []
    for s, objects in enumerate((2, 1)):
        masks = torch.randint(0, objects + 1, (L, H // 8, W // 8), generator=torch.Generator().manual_seed(s), dtype=torch.uint8)
        seqs.append((imgs[3 * s:3 * s + L], masks.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2), objects))
    got = evaluate_davis(model, [(f, m[0], m, o) for f, m, o in seqs], DEV, n_last=1, radius=radius, k=k, T=T, batch=2, return_masks=True)

    Gh, Gw, want = H // r, W // r, []
    for (frames, masks, objects), kept in zip(seqs, got["masks"]):
        K = objects + 1
        tok = model.forward_tokens(frames.to(DEV), integers=True)[0]
        tok = tok[max(tok)]
        mem = TokenMemory(Gh, Gw, 192, K, 2, DEV)
        mem.put(0, tok[0], torch.nn.functional.one_hot(patch_labels(masks[:1].to(DEV).contiguous(), r, K).reshape(-1).long(), K).float())
        seg1 = mem.propagate(tok[1], radius, k, T, frames=1)
        mem.put(1, tok[1], seg1)
        seg2 = mem.propagate(tok[2], radius, k, T, frames=2)
        pred = np.stack([davis_ref.upsample_argmax(s.cpu().numpy(), Gh, Gw, r) for s in (seg1, seg2)])
        assert np.array_equal(kept.cpu().numpy(), np.concatenate([masks[:1].numpy(), pred]))
        J, F = davis_measures(davis_ref.mask_scores(pred, masks[1:].numpy(), objects, bound_radius(0.008, H, W)))
        want.append(tuple(100.0 * sum(m.reshape(-1).tolist()) / (2 * objects) for m in (J, F)))
    assert got["per_sequence"] == want
    assert got["J_mean"] == (want[0][0] + want[1][0]) / 2 and got["F_mean"] == (want[0][1] + want[1][1]) / 2
    assert got["JF_mean"] == (got["J_mean"] + got["F_mean"]) / 2
