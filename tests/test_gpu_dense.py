"""Dense linear probe on the GPU: ivit_dense_argmax_u8 and ivit_patch_mode_u8 against tests/dense_ref.py, byte for byte and integer
for integer -- the geometry sweep (all-clamped grids, the 16-column chunk boundary and its halo, byte and dword label stores), the
crafted value cases, the refusals -- then inference.evaluate_dense_probe end to end on a synthetic DeiT of depth 2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.dense import DenseProbe, miou, patch_labels  # noqa: E402
from ivit_amd.inference import evaluate_dense_probe  # noqa: E402
from ivit_amd.probe import BankStats  # noqa: E402

import dense_ref  # noqa: E402

DEV = "cuda:0"
SENT = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(acc, s, classes, r, target=None, conf=None, labels=True, ignore_index=255):
    """-> (labels uint8 [B, H, W] or None, conf int64 or None) as numpy; conf: the starting values (accumulated into)"""
    B, gh, gw, np_ = acc.shape
    out = torch.empty(B, gh * r, gw * r, dtype=torch.uint8, device=DEV) if labels else None
    ad, sd, td, cd = (None if v is None else dev(v) for v in (acc, s, target, conf))      # held until the launch has finished
    _lib.call("ivit_dense_argmax_u8", _lib.ptr(ad), _lib.ptr(sd), B, gh, gw, np_, classes, r, _lib.ptr(out), _lib.ptr(td), ignore_index,
              _lib.ptr(cd), _lib.stream_ptr())
    torch.cuda.synchronize()
    return None if out is None else out.cpu().numpy(), None if cd is None else cd.cpu().numpy()


@pytest.mark.parametrize("B,gh,gw,r,classes,np_", dense_ref.CASES)
def test_argmax_conf_and_patch_mode_equal_the_reference(B, gh, gw, r, classes, np_):
    rng = np.random.default_rng(B + 10 * gh + 100 * gw + 1000 * r + classes)
    acc, s = dense_ref.random_case(rng.integers(1 << 30), B, gh, gw, classes, np_)
    exp = dense_ref.argmax(acc, s, classes, r)
    target = rng.integers(0, min(classes + 2, 256), size=exp.shape).astype(np.uint8)      # with values at or above classes
    target[rng.random(exp.shape) < 0.1] = 255
    econf = dense_ref.confusion(exp, target, classes)
    start = rng.integers(-2 ** 40, 2 ** 40, size=(classes, classes))
    got, conf = run(acc, s, classes, r, target, start)
    assert np.array_equal(got, exp) and np.array_equal(conf, start + econf)
    assert np.array_equal(run(acc, s, classes, r)[0], exp)                                          # conf = NULL
    _, conf = run(acc, s, classes, r, target, conf, labels=False)                                  # labels = NULL, a second call
    assert np.array_equal(conf, start + 2 * econf)
    ig = int(rng.integers(0, classes))                                                              # a class as ignore_index
    assert np.array_equal(run(acc, s, classes, r, target, 0 * start, labels=False, ignore_index=ig)[1], dense_ref.confusion(exp, target, classes, ig))
    for ignore in (255, ig):
        pm = patch_labels(dev(target), r, classes, ignore).cpu().numpy()
        assert np.array_equal(pm, dense_ref.patch_mode(target, r, classes, ignore))


def test_equal_scores_go_to_the_lower_class_and_one_pair_fills_the_table():
    acc = np.random.default_rng(0).integers(-1000, 1000, size=(1, 2, 17, 1)).astype(np.int32).repeat(64, axis=3)
    s = np.full(64, 0.01, np.float32)
    target = np.zeros((1, 32, 272), np.uint8)
    got, conf = run(acc, s, 2, 16, target, np.zeros((2, 2), np.int64))
    assert not got.any() and np.array_equal(got, dense_ref.argmax(acc, s, 2, 16))
    assert conf.tolist() == [[32 * 272, 0], [0, 0]]


def test_int32_extremes_at_r_32_need_the_int64_combination():
    rng = np.random.default_rng(1)
    acc = rng.choice(np.array([-(2 ** 31 - 1), 2 ** 31 - 1], np.int64), size=(1, 2, 3, 64)).astype(np.int32)
    s = rng.uniform(1e-6, 2e-6, size=64).astype(np.float32)
    assert np.abs(dense_ref.interpolate(acc, 32)).max() == 4096 * (2 ** 31 - 1)
    assert np.array_equal(run(acc, s, 5, 32)[0], dense_ref.argmax(acc, s, 5, 32))


def test_scores_that_differ_beyond_float32_are_told_apart():
    acc = np.zeros((1, 2, 2, 64), np.int32)
    acc[..., 0], acc[..., 1] = 2 ** 30, 2 ** 30 + 1
    s = np.full(64, 0.37, np.float32)
    I = dense_ref.interpolate(acc[..., :2], 4)
    assert (np.float32(I[:, 0]) * s[0] == np.float32(I[:, 1]) * s[1]).all()        # a float32 score ties: class 0
    assert (run(acc, s, 2, 4)[0] == 1).all() and (dense_ref.argmax(acc, s, 2, 4) == 1).all()


BAD = [(dict(classes=0), -2), (dict(classes=256), -2), (dict(r=0), -2), (dict(r=33), -2), (dict(np_=18), -1), (dict(gh=0), -1),
       (dict(B=0), -1), (dict(ignore_index=256), -1), (dict(ignore_index=-1), -1), (dict(labels=False), -1), (dict(conf=True), -1),
       (dict(acc=None), -1), (dict(s=None), -1), (dict(B=2 ** 15, gh=2 ** 8, gw=2 ** 8, r=1), -1)]


@pytest.mark.parametrize("bad,rc", BAD)
def test_argument_errors(bad, rc):
    L = _lib.lib()
    acc, s = dev(np.zeros((2, 3, 4, 64), np.int32)), dev(np.ones(64, np.float32))
    out = torch.full((2 * 6 * 8,), SENT, dtype=torch.uint8, device=DEV)
    conf = torch.zeros(19, 19, dtype=torch.int64, device=DEV)
    a = dict(acc=acc, s=s, B=2, gh=3, gw=4, np_=64, classes=19, r=2, labels=True, conf=False, ignore_index=255)
    a.update(bad)
    got = L.ivit_dense_argmax_u8(_lib.ptr(a["acc"]), _lib.ptr(a["s"]), a["B"], a["gh"], a["gw"], a["np_"], a["classes"], a["r"],
                                 _lib.ptr(out if a["labels"] else None), None, a["ignore_index"], _lib.ptr(conf if a["conf"] else None),
                                 _lib.stream_ptr())
    assert got == rc and L.ivit_last_error_string()
    if "acc" not in bad and "s" not in bad and "labels" not in bad and "conf" not in bad and "np_" not in bad:
        assert L.ivit_patch_mode_u8(_lib.ptr(out), a["B"], a["gh"], a["gw"], a["r"], a["classes"], a["ignore_index"], _lib.ptr(out), _lib.stream_ptr()) == rc
    torch.cuda.synchronize()
    assert (out == SENT).all() and not conf.any()


def test_evaluate_dense_probe_end_to_end():
    from test_gpu_vit16_lazy import W8, _images
    K, r, H, W = 5, 16, 64, 96
    torch.manual_seed(7)
    model = ivit.VisionTransformer(img_size=(H, W), patch_size=r, embed_dim=192, depth=2, num_heads=3, mlp_ratio=4, qkv_bias=True,
                                   num_classes=K, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **W8).to(DEV).eval()
    imgs = _images(12, 224, torch.Generator(device="cpu").manual_seed(3))[:, :, :H, :W].contiguous()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        model(imgs[:4])
        model(imgs[4:8].flip(0) * 0.7)
    ivit.freeze_model(model)
    rng = np.random.default_rng(5)
    coarse = rng.integers(0, K, size=(12, H // 8, W // 8)).astype(np.uint8)          # 8 x 8 blobs: patches with mixed classes
    coarse[rng.random(coarse.shape) < 0.15] = 255
    targets = torch.from_numpy(coarse.repeat(8, axis=1).repeat(8, axis=2))
    loader = [(imgs[i:i + 4], targets[i:i + 4]) for i in range(0, 12, 4)]
    lams = (1e-2, 1.0)
    got = evaluate_dense_probe(model, loader, loader, DEV, K, lam=lams)
    # the same tokens and the same probe through the numpy reference
    tok, _, scale = model.forward_tokens(imgs, integers=True)
    rows = tok[max(tok)].reshape(-1, 192).contiguous()
    lab = dense_ref.patch_mode(targets.numpy(), r, K).reshape(-1)
    keep = torch.from_numpy(lab != 255).to(DEV)
    stats = BankStats(192, K, DEV).update(rows[keep].contiguous(), dev(lab)[keep], scale)
    assert int(stats.counts.sum()) == int(keep.sum()) > 0
    for lam in lams:
        probe = stats.ridge(lam)
        acc = probe._acc(rows, "test").cpu().numpy().reshape(12, H // r, W // r, probe.Np)
        exp = dense_ref.argmax(acc, probe.s_acc.cpu().numpy(), K, r)
        assert torch.equal(DenseProbe(probe).segment(rows, (H // r, W // r), r).cpu(), torch.from_numpy(exp))
        m, pa, _ = miou(dense_ref.confusion(exp, targets.numpy(), K))
        assert got[lam] == (100.0 * m, 100.0 * pa)
