"""k-means on the int8 feature bank on the GPU against numpy int64 (tests/kmeans_ref.py), every output exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, cluster  # noqa: E402

import fenced  # noqa: E402
import kmeans_ref  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def words(d):      # int64 [N] as the int32 words fenced.py compares
    return np.ascontiguousarray(d, np.int64).view(np.int32)[None]


def random_case(N, K, Cc):
    rng = np.random.default_rng(1000 * N + 10 * K + Cc)
    centres = rng.integers(-100, 101, size=(K, Cc))
    c16 = rng.integers(-16384, 16384, size=(K, Cc))                       # the full range ...
    c16[::2] = 128 * centres[::2] + rng.integers(0, 128, size=centres[::2].shape)      # ... and every other one near a planted centre
    c16[0, 0], c16[-1, -1] = -128 * 128 + 127, -16384                     # hi = -128 with lo = 127, and with lo = 0
    x = np.clip(centres[2 * rng.integers(0, (K + 1) // 2, size=N)] + rng.integers(-3, 4, size=(N, Cc)), -128, 127).astype(np.int8)
    return x, c16, lambda label, dist: K < 3 or len(np.unique(label)) > 1


def extremes():      # C = 1024, every row all -128, one centroid all -16384 among random others: 128 * dot_hi = 2^31 does not fit int32
    c16 = np.random.default_rng(5).integers(-16384, 16384, size=(5, 1024))
    c16[3] = -16384
    return np.full((5, 1024), -128, np.int8), c16, lambda label, dist: (label == 3).all() and (dist == 0).all()


def ties(Cc):      # centroids 3 and 67 are equal (tiles apart in both forms), 5 and 10 equidistant from the zero row and its nearest: the lower wins
    rng = np.random.default_rng(6)
    c16 = rng.integers(-16384, 16384, size=(70, Cc))
    c16[67] = c16[3] = 128 * rng.integers(-100, 101, size=Cc)
    c16[5] = rng.integers(-200, 201, size=Cc)
    c16[10] = -c16[5]
    x = np.zeros((40, Cc), np.int8)
    x[1::2] = c16[3] // 128
    return x, c16, lambda label, dist: (label[0::2] == 5).all() and (label[1::2] == 3).all()


# rows: 1, a partial tile, one past, several workgroups; K: 1, a masked tile, one past (33: of the C > 512 form), several tiles; C: 64 .. 1024
@pytest.mark.parametrize("make,args", [(random_case, a) for a in ((1, 1, 64), (127, 63, 192), (129, 65, 64), (300, 200, 192), (300, 63, 1024), (129, 200, 1024),
                                                                  (127, 33, 1024), (129, 65, 576))] + [(extremes, ()), (ties, (64,)), (ties, (1024,))])
def test_assign_matches_reference(make, args):      # on a fenced bank of row stride C + 32 into fenced outputs
    x, c16, built_for = make(*args)
    N, Cc = x.shape
    label, dist = kmeans_ref.assign(x, c16)
    assert built_for(label, dist)      # the reference agrees with what the case was built for
    wider = lambda m: np.pad(c16, ((0, 0), (0, m.shape[1] - Cc)), constant_values=128)      # noqa: E731 (a pad column that is read moves every dist)
    bank = fenced.input(x, Cc + 32, 127, oracle=lambda m: words(kmeans_ref.assign(m, wider(m))[1]).reshape(N, 2), expected=words(dist).reshape(N, 2))
    hi, lo, cnorm = (dev(p) for p in (*kmeans_ref.planes(c16), (c16.astype(np.int64) ** 2).sum(axis=1)))
    out_l = fenced.output(1, N, N, np.int32, expected=label[None])
    out_d = fenced.output(1, 2 * N, 2 * N, np.int32, expected=words(dist))
    _lib.call("ivit_kmeans_assign_i8", bank.ptr, bank.ld, N, Cc, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(cnorm), len(c16), out_l.ptr, out_d.ptr,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    fenced.check(out_l, label[None])
    fenced.check(out_d, words(dist))
    fenced.check(bank)


@pytest.mark.parametrize("Cc", (64, 192))
def test_update_matches_reference(Cc):
    K, rng = 5, np.random.default_rng(Cc)
    n = np.array([2, 17, 0, 50, 9], np.int64)                             # cluster 2 is empty
    S = rng.integers(-128, 128, size=(K, Cc)) * n[:, None]
    S[0, :2] = (-1, -3)                                                   # negative half-way numerators: -64, -192
    old = rng.integers(-16384, 16384, size=(K, Cc))
    old[4] = 128 * rng.integers(-128, 128, size=Cc)
    S[4] = old[4] // 128 * n[4]                                           # the mean is the old centroid: not moved
    new, changed = kmeans_ref.update(S, n, old)
    assert tuple(new[0, :2]) == (-64, -192) and changed.tolist() == [1, 1, 0, 1, 0] and (new[2] == old[2]).all()
    hi, lo = (dev(p) for p in kmeans_ref.planes(old))
    Sd, nd, cnorm, ch = dev(S), dev(n), dev((old ** 2).sum(axis=1)), torch.full((K,), -7, dtype=torch.int32, device=DEV)
    _lib.call("ivit_kmeans_update_i16", _lib.ptr(Sd), _lib.ptr(nd), K, Cc, _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(cnorm), _lib.ptr(ch),
              _lib.stream_ptr())
    assert all(np.array_equal(got.cpu().numpy(), want) for got, want in zip((hi, lo), kmeans_ref.planes(new)))
    assert np.array_equal(cnorm.cpu().numpy(), (new ** 2).sum(axis=1)) and ch.cpu().tolist() == changed.tolist()


@pytest.mark.parametrize("iters", (1, 50))
def test_fit_follows_the_reference_trajectory(iters):      # 300 rows around 7 well-separated planted centres: the inertia does not increase
    rng = np.random.default_rng(11)
    x = np.clip(rng.integers(-90, 91, size=(7, 64))[rng.integers(0, 7, size=300)] + rng.integers(-8, 9, size=(300, 64)), -128, 127).astype(np.int8)
    init = rng.choice(300, size=7, replace=False)
    label, c16, history, inertia = kmeans_ref.fit(x, init, iters)
    assert all(b <= a for a, b in zip(history, history[1:] + [inertia])) and (iters == 1 or 1 < len(history) < 50)
    km = cluster.KMeans(64, 7, DEV)
    got = km.fit(dev(x), iters=iters, init=init)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), label) and torch.equal(cluster.assign(dev(x), km)[0], got)
    assert np.array_equal(km.c16.cpu().numpy(), c16) and np.array_equal(km.cnorm.cpu().numpy(), (c16 ** 2).sum(axis=1))
    assert km.history == history and km.inertia == inertia and torch.equal(km.centroids, km.c16.float() / 128)


def test_evaluate_clustering_end_to_end():
    """the wiring of inference.evaluate_clustering on a synthetic DeiT of depth 2: the reference fit on the model's own features"""
    from ivit_amd.inference import evaluate_clustering, extract_features
    from test_gpu_vit16_lazy import W8, _images
    torch.manual_seed(7)
    model = ivit.VisionTransformer(img_size=(64, 96), patch_size=16, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   num_classes=5, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
    imgs = _images(8, 224, torch.Generator(device="cpu").manual_seed(3))[:, :, :64, :96].contiguous()
    with torch.no_grad():
        model(imgs[:4])
    ivit.freeze_model(model)
    targets = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1])
    loader = [(imgs[:5], targets[:5]), (imgs[5:], targets[5:])]
    got = evaluate_clustering(model, loader, DEV, 3, iters=10, seed=4)
    rows = extract_features(model, loader, DEV, integers=True)[0].cpu().numpy()
    init = torch.randperm(8, generator=torch.Generator().manual_seed(4))[:3].numpy()
    label, _, history, inertia = kmeans_ref.fit(rows, init, 10)
    assert got == {**cluster.partition_scores(label, targets), "inertia": inertia, "iterations": len(history)}
