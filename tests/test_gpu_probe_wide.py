"""The wide statistics of the linear probe on the GPU: ivit_gram_i8_i64_wide (with ivit_gram_wide_workspace_bytes) and
ivit_group_sums_i8_i64_wide against tests/probe_ref.py at 1088, 1536 and 4096 channels (3, 2 and 1 row slots in the group sums), their
refusals, LinearProbe's int32 accumulators at K = 1536, and inference.evaluate_linear_probe(wide=True) on a pooled bank of W = 1152."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.inference import evaluate_linear_probe, extract_features  # noqa: E402
from ivit_amd.probe import BankStats, LinearProbe  # noqa: E402

import probe_ref  # noqa: E402
from test_gpu_probe import DEV, SENT, dev, rand8, st  # noqa: E402

_POOLED = []


def pooled_model():
    """(a calibrated, frozen DeiT-Tiny-width ViT of depth 5 on 64 x 96 images, a loader of 24 images with 4 classes, 24), built once"""
    if not _POOLED:
        from test_gpu_features_pooled import _images
        from test_gpu_vit16_lazy import W8
        torch.manual_seed(1152)
        model = ivit.VisionTransformer(img_size=(64, 96), patch_size=16, embed_dim=192, depth=5, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                       num_classes=4, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
        g = torch.Generator(device="cpu").manual_seed(11)
        imgs = _images(24, (64, 96), g)
        with torch.no_grad():
            for p in model.parameters():
                if p.dim() > 1:
                    p.mul_(3.0)
            model(imgs[:4])
            model(imgs[4:8].flip(0) * 0.7)
        ivit.freeze_model(model)
        labels = torch.arange(24) % 4
        _POOLED.append((model, [(imgs[i:i + 8], labels[i:i + 8]) for i in range(0, 24, 8)], 24))
    return _POOLED[0]


@pytest.mark.parametrize("rows", [1, 130])
@pytest.mark.parametrize("Cc", [1088, 1536, 4096])
def test_gram_and_group_sums(Cc, rows):
    rng = np.random.default_rng(Cc + rows)
    x = rand8(rng, rows, Cc)
    x[0, 0], x[-1, -1] = -128, 127
    xd, p = dev(x), _lib.ptr
    exp = probe_ref.gram(x)                           # float64 X^T X: exact (probe_ref's header)
    start = rng.integers(-2 ** 62, 2 ** 62, size=(Cc, Cc))
    for sp in (0, 3):
        need = C.c_int64(-1)
        _lib.call("ivit_gram_wide_workspace_bytes", rows, Cc, sp, C.byref(need))
        assert need.value > 0 and need.value % (4 * Cc * Cc) == 0
        ws = torch.empty(need.value // 4, dtype=torch.int32, device=DEV)
        for acc in (0, 1):
            out = dev(start)
            _lib.call("ivit_gram_i8_i64_wide", p(xd), Cc, rows, Cc, sp, acc, p(out), p(ws), need.value, st())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), exp + acc * start), f"gram splits={sp} accumulate={acc}"
    perm, ptr = probe_ref.csr(rng.integers(0, 4, size=rows) * 2, 8)      # four groups of rows, four empty ones
    exp, pd, gd = probe_ref.group_sums(x, perm, ptr), dev(perm), dev(ptr)
    for acc in (0, 1):
        out = dev(start[:8])
        _lib.call("ivit_group_sums_i8_i64_wide", p(xd), Cc, rows, Cc, p(pd), p(gd), 8, acc, p(out), st())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), exp + acc * start[:8]), f"group sums accumulate={acc}"


def test_refusals_leave_the_outputs_untouched():
    L, p = _lib.lib(), _lib.ptr
    x = dev(rand8(np.random.default_rng(3), 70, 4160))
    gram = torch.full((1088 * 1088,), SENT, dtype=torch.int64, device=DEV)
    ws = torch.full((1088 * 1088,), -3, dtype=torch.int32, device=DEV)
    perm, ptr = dev(np.arange(70, dtype=np.int32)), dev(np.array([0, 30, 70], np.int64))
    need = C.c_int64(-1)

    def g(xp=p(x), ldx=4160, Cn=1088, w=p(ws)):
        return L.ivit_gram_i8_i64_wide(xp, ldx, 70, Cn, 1, 0, p(gram), w, ws.numel() * 4, st())

    def s(xp=p(x), ldx=4160, Cn=1088):
        return L.ivit_group_sums_i8_i64_wide(xp, ldx, 70, Cn, p(perm), p(ptr), 2, 0, p(gram), st())

    for run in (g, s):
        assert run(Cn=4160) == -2 and run(Cn=96) == -2 and run(ldx=1024) == -1 and run(xp=x.data_ptr() + 8) == -1
    assert g(w=None) == -1 and L.ivit_gram_wide_workspace_bytes(70, 4160, 1, C.byref(need)) == -2
    torch.cuda.synchronize()
    assert (gram == SENT).all() and (ws == -3).all()
    assert g() == 0 and L.ivit_gram_wide_workspace_bytes(70, 1088, 1, C.byref(need)) == 0 and need.value == 4 * 1088 * 1088
    torch.cuda.synchronize()
    assert np.array_equal(gram.view(1088, 1088).cpu().numpy(), probe_ref.gram(x.cpu().numpy()[:, :1088]))


def test_linear_probe_accumulators_at_1536_channels():
    rng = np.random.default_rng(5)
    probe = LinearProbe(rng.normal(0, 1, size=(10, 1536)).astype(np.float32), rng.normal(0, 1, size=10).astype(np.float32), 0.04, DEV)
    q = rand8(rng, 37, 1536)
    acc, _ = probe.logits(dev(q))
    want = (q.astype(np.int64) @ probe.W8.cpu().numpy().astype(np.int64).T + probe.b32.cpu().numpy().astype(np.int64)[None, :])[:, :10]
    assert np.abs(want).max() < 2 ** 31 and np.array_equal(acc.cpu().numpy(), want)      # (the padded classes beyond 10 carry a bias of -2^31)


def test_evaluate_linear_probe_on_a_pooled_bank_of_1152_channels():
    model, loader, n = pooled_model()
    got = evaluate_linear_probe(model, loader, loader, DEV, 4, lam=(1e-2,), n_last=5, avgpool=True, wide=True)
    rows, lab, scale = extract_features(model, loader, DEV, integers=True, n_last=5, avgpool=True, wide=True)
    stats = BankStats(1152, 4, DEV).update(rows, lab, scale)
    G, S, cnt = probe_ref.stats(rows.cpu().numpy(), lab.cpu().numpy(), 4)
    assert np.array_equal(stats.gram.cpu().numpy(), G) and np.array_equal(stats.sums.cpu().numpy(), S)
    hits = torch.zeros(4, dtype=torch.int64, device=DEV)
    stats.ridge(1e-2).topk(rows, 4, lab.to(torch.int32).contiguous(), hits)
    assert got == {1e-2: (100.0 * int(hits[0]) / n, 100.0 * int(hits.sum()) / n)}
