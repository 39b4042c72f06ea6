"""The logistic probe without a GPU: what the two entries refuse (nothing is launched: the pointers are never followed), the
trainer's own refusals, the cosine schedule, and tests/logistic_ref.py against plain float64 softmax regression."""
import numpy as np
import pytest
import torch

from ivit_amd import _lib
import ivit_amd.probe as probe

import logistic_ref as ref

P = 4096      # an aligned address that is never followed


def fwd(x=P, ldx=64, C=64, idx=P, y=P, B=8, K=10, Wh=P, b=P, G=P, loss=P, top1=P, z=None):
    return _lib.lib().ivit_probe_ce_forward_i8(x, ldx, C, idx, y, B, K, 0.05, Wh, b, G, loss, top1, z, None)


def upd(x=P, ldx=64, C=64, idx=P, B=8, K=10, G=P, W=P, b=P, mW=P, mb=P, Wh=P):
    return _lib.lib().ivit_probe_sgd_update_i8(x, ldx, C, idx, B, K, 0.05, G, 0.1, 0.9, 0.0, W, b, mW, mb, Wh, None)


@pytest.mark.parametrize("entry", [fwd, upd])
def test_entries_refuse(entry):
    for kw in (dict(x=None), dict(G=None), dict(Wh=None), dict(x=P + 8), dict(ldx=72), dict(ldx=48), dict(idx=P + 2), dict(b=P + 4),
               dict(B=0), dict(B=4097), dict(K=0)):
        assert entry(**kw) == -1, kw
    for kw in (dict(C=96, ldx=96), dict(C=32), dict(C=4160, ldx=4160), dict(K=1025)):
        assert entry(**kw) == -2 and b"unsupported geometry" in _lib.lib().ivit_last_error_string(), kw
    assert fwd(loss=None) == fwd(y=None) == fwd(z=P + 4) == upd(mb=None) == upd(W=P + 8) == -1


def test_trainer_refusals():
    for bad in (dict(C=96), dict(num_classes=0), dict(num_classes=1025), dict(scale=0.0)):
        with pytest.raises(ValueError):
            probe.LogisticTrainer(**{**dict(C=64, num_classes=10, scale=0.05, device="cpu"), **bad})
    with pytest.raises(ValueError, match="init"):
        probe.LogisticTrainer(64, 10, 0.05, "cpu", init=probe.LinearProbe(np.ones((9, 64)), np.ones(9), 0.05, "cpu"))
    rows, labels = torch.zeros(8, 64, dtype=torch.int8), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(TypeError, match="integers=True"):
        probe.fit_logistic(rows.float(), labels, 0.05, 10, epochs=1, lr=0.1)
    with pytest.raises(ValueError, match="on the device"):
        probe.fit_logistic(rows, labels, 0.05, 10, epochs=1, lr=0.1)


def test_cosine_schedule():
    assert [probe.cosine_lr(0.5, t, 4) for t in range(5)] == pytest.approx([0.5, 0.25 * (1 + 2 ** -0.5), 0.25, 0.25 * (1 - 2 ** -0.5), 0.0])


def test_reference_is_softmax_regression_up_to_bf16():
    rng = np.random.default_rng(0)
    x, y = rng.integers(-128, 128, size=(6, 64)).astype(np.int8), rng.integers(0, 3, size=6)
    W, b = rng.normal(size=(3, 64)) * 0.02, rng.normal(size=3)
    got = ref.step(x, y, 0.05, W, b, W * 0, b * 0, 0.1, 0.9, 1e-3)
    want = ref.step(x, y, 0.05, W, b, W * 0, b * 0, 0.1, 0.9, 1e-3, rounding=False)
    z = 0.05 * x.astype(np.float64) @ W.T + b
    p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    p[np.arange(6), y] -= 1
    assert np.allclose(want[2], p.T @ x * (0.05 / 6) + 1e-3 * W, rtol=1e-12, atol=0) and np.allclose(want[0], W - 0.1 * want[2], rtol=1e-12)
    # two roundings of 2^-9 relative each: Wh moves every logit by at most 2^-9 sum |x W| s, G by 2^-9 of itself
    dz = 2.0 ** -9 * 0.05 * np.abs(x.astype(np.float64)) @ np.abs(W).T
    tol = (2.0 ** -8 * np.abs(p) + 2 * dz.max()).T @ np.abs(x) * (0.05 / 6)
    assert (np.abs(got[2] - want[2]) <= tol).all() and (got[2] != want[2]).any()
    assert np.array_equal(ref.bf16_rne(np.float32([1.0, 1.00390625, 1.01171875, -2.5])), np.uint16([0x3f80, 0x3f80, 0x3f82, 0xc020]))
