"""Object discovery on the GPU: ivit_token_degrees_i8 and ivit_discover_boxes_i8 through discover.py against numpy
(tests/discover_ref.py), every output exactly."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, discover  # noqa: E402

import discover_ref  # noqa: E402

DEV = "cuda:0"
GRIDS = ((1, 1), (3, 5), (9, 13), (16, 16), (17, 64), (64, 64))      # hw: 1, no multiple of 16, one tile, several tiles, the caps
KS = (1, 5, 128)


@functools.lru_cache(maxsize=None)
def problem(grid, Cc, B=3):
    rng = np.random.default_rng(100 * grid[0] + grid[1] + Cc)
    t = rng.integers(-20, 21, size=(B, grid[0] * grid[1], Cc)).astype(np.int8)      # mixed signs, many equal degrees
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference(grid, Cc):
    """{k: [(box, seed, deg, comp) per image]}: one affinity matrix per image for all k"""
    ds = [discover_ref.affinity(img) for img in problem(grid, Cc)]
    return {k: [discover_ref.discover(d, *grid, k) for d in ds] for k in KS}


def strided(t, pad_rows=3, fill=0):
    """the images of t inside a larger buffer: a non-contiguous image stride, `fill` in the rows between them"""
    B, hw, Cc = t.shape
    buf = torch.full((B, hw + pad_rows, Cc), fill, dtype=torch.int8, device=DEV)
    buf[:, :hw] = torch.from_numpy(np.array(t)).to(DEV)
    return buf[:, :hw]


def check(tokens, grid, k, want):
    boxes, seed, deg, rows = discover.discover_objects(tokens, grid, k, return_mask=True)
    assert torch.equal(deg, discover.token_degrees(tokens, grid))
    boxes, seed, deg, rows = (v.cpu().numpy() for v in (boxes, seed, deg, rows))
    for b, (box, sd, dg, comp) in enumerate(want):
        assert np.array_equal(deg[b], dg), (b, np.argwhere(deg[b] != dg)[:8])
        assert seed[b] == sd and tuple(boxes[b]) == box, (b, seed[b], sd, boxes[b], box)
        assert np.array_equal(rows[b], discover_ref.row_words(comp)), b


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("Cc", (64, 1024))
@pytest.mark.parametrize("grid", GRIDS)
def test_matches_reference(grid, Cc, k):
    check(strided(problem(grid, Cc)), grid, k, reference(grid, Cc)[k])


def blob_image(grid, cells, Cc=64):
    """tokens whose mask is exactly `cells` (fewer than half of the grid): +3 in channel 0 inside, -3 outside, so inside tokens
    agree with each other alone, have the smaller, EQUAL degrees, and the seed is the first of them in index order"""
    t = np.zeros((grid[0] * grid[1], Cc), dtype=np.int8)
    t[:, 0] = -3
    for y, x in cells:
        t[y * grid[1] + x, 0] = 3
    return t


def serpentine(Gh, Gw):
    cells = []
    for i, y in enumerate(range(0, Gh, 3)):      # full rows three apart, joined at alternating ends
        cells += [(y, x) for x in range(Gw)]
        if y + 3 < Gh:
            cells += [(y + 1, Gw - 1 if i % 2 == 0 else 0), (y + 2, Gw - 1 if i % 2 == 0 else 0)]
    return cells


ZERO_SEED = blob_image((5, 7), [(1, 1), (1, 2), (2, 1)])
ZERO_SEED[3 * 7 + 4] = 0      # degree 0, below everything else: the seed, M == 0 everywhere
CRAFTED = {      # name: (grid, tokens, k, seed, box)
    "equal degrees: seed by index": ((5, 7), blob_image((5, 7), [(1, 2), (1, 3), (2, 2), (2, 3)]), 100, 1 * 7 + 2, (2, 1, 3, 2)),
    "all-zero seed row": ((5, 7), ZERO_SEED, 100, 3 * 7 + 4, (4, 3, 4, 3)),
    "two components": ((6, 9), blob_image((6, 9), [(0, 1), (0, 2), (1, 1), (4, 6), (4, 7), (5, 7)]), 100, 1, (1, 0, 2, 1)),
    "diagonal neighbours stay apart": ((5, 5), blob_image((5, 5), [(1, 1), (2, 2)]), 100, 6, (1, 1, 1, 1)),
    "columns 0 to 63": ((3, 64), blob_image((3, 64), [(1, x) for x in range(64)]), 128, 64, (0, 1, 63, 1)),
    "serpentine": ((16, 16), blob_image((16, 16), serpentine(16, 16)), 128, 0, (0, 0, 15, 15)),
    "int32 bound of M": ((9, 16), np.full((144, 1024), 127, dtype=np.int8), 128, 0, (0, 0, 15, 8)),
}


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_images(name):
    grid, t, k, seed, box = CRAFTED[name]
    want = discover_ref.discover(discover_ref.affinity(t), *grid, k)
    assert (want[1], want[0]) == (seed, box)      # the reference agrees with what the image was built for
    check(strided(t[None], fill=127), grid, k, [want])


def test_padding_is_inert():
    t, want = problem((5, 7), 64), reference((5, 7), 64)[5]      # hw = 35
    check(torch.from_numpy(np.array(t)).to(DEV), (5, 7), 5, want)
    check(strided(t, pad_rows=40, fill=127), (5, 7), 5, want)


@pytest.mark.parametrize("what", ("C", "Gw", "k0", "k129", "float"))
def test_refusals(what):
    wide = torch.zeros(1, 65, 1088, dtype=torch.int8, device=DEV)      # 65 = 5 x 13 = 1 x 65 tokens
    t = wide[:, :, :64]
    calls = {"C": lambda: discover.discover_objects(wide, (5, 13), 5), "Gw": lambda: discover.token_degrees(t, (1, 65)),
             "k0": lambda: discover.discover_objects(t, (5, 13), 0), "k129": lambda: discover.discover_objects(t, (5, 13), 129),
             "float": lambda: discover.discover_objects(t.float(), (5, 13), 5)}
    with pytest.raises(_lib.IvitError, match={"C": "C=1088", "Gw": "Gw=65", "k0": "k=0", "k129": "k=129", "float": "float32"}[what]):
        calls[what]()
    if what != "float":      # the entries themselves refuse the same values
        Gh, Gw, Cc, k = {"C": (5, 13, 1088, 5), "Gw": (1, 65, 64, 5), "k0": (5, 13, 64, 0), "k129": (5, 13, 64, 129)}[what]
        out, text = torch.zeros(70, dtype=torch.int32, device=DEV), {"C": "C=1088", "Gw": "1 x 65", "k0": "k=0", "k129": "k=129"}[what]
        with pytest.raises(_lib.IvitError, match=text):
            _lib.call("ivit_discover_boxes_i8", _lib.ptr(wide), 1088, 0, 1, Gh, Gw, Cc, _lib.ptr(out), k, _lib.ptr(out[65:]), _lib.ptr(out[69:]), None, None)
        if what in ("C", "Gw"):
            with pytest.raises(_lib.IvitError, match=text):
                _lib.call("ivit_token_degrees_i8", _lib.ptr(wide), 1088, 0, 1, Gh, Gw, Cc, _lib.ptr(out), None)


def test_evaluate_object_discovery_end_to_end():
    """the wiring of inference.evaluate_object_discovery on a synthetic DeiT of depth 2: the reference's boxes on the model's own tokens"""
    from ivit_amd.inference import evaluate_object_discovery
    from test_gpu_vit16_lazy import W8, _images
    r, H, W = 16, 64, 96
    torch.manual_seed(7)
    model = ivit.VisionTransformer(img_size=(H, W), patch_size=r, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   num_classes=5, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
    imgs = _images(8, 224, torch.Generator(device="cpu").manual_seed(3))[:, :, :H, :W].contiguous()
    with torch.no_grad():
        model(imgs[:4])
    ivit.freeze_model(model)
    gts = [[[0, 0, W, H]], [[16, 16, 48, 48], [0, 0, 16, 16]], []]
    got = evaluate_object_discovery(model, [(imgs[:2], gts[:2]), (imgs[2:3], gts[2:])], DEV, k=4)
    tok = model.forward_tokens(imgs[:3].to(DEV), integers=True)[0]
    tok = tok[max(tok)].cpu().numpy()
    boxes = [discover_ref.discover(discover_ref.affinity(t), H // r, W // r, 4)[0] for t in tok]
    hits, iou = discover.corloc(discover.boxes_to_pixels(torch.tensor(boxes), r), gts)
    assert got["per_image"] == list(zip(hits.tolist(), iou.tolist())) and got["CorLoc"] == 100.0 * sum(hits.tolist()) / 3
