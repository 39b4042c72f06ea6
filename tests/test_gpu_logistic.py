"""ivit_probe_ce_forward_i8 / ivit_probe_sgd_update_i8 stage by stage against float64 (tests/logistic_ref.py) on each stage's ACTUAL
inputs, so every bound is derived (u = 2^-24, one float32 rounding):
  logits    |z_out - z64| <= (C + 4) u (s sum|x||Wh| + |b|): C float32 additions inside the MFMAs and the three of the epilogue
  gradient  p64 from the kernel's own z_out: |G - (p64 - onehot)| <= 2^-8 |p64 - onehot| + 2^-20 (a bf16 ulp, the float32 exp / sum)
  loss      <= (K + 8) u (1 + |loss64|);  top1 = the float64 argmax wherever the float64 top-two gap exceeds twice the logit bound
  update    D64 from the kernel's own G: mW' within e_m = (B + 4) u (s / B) sum|G||x| + 6 u (|D s / B| + |wd W| + |mu mW|) (the sum,
            then fl(s / B) and the five operations of the chain, each on a value of at most that magnitude); W' within lr e_m +
            2 u (|W| + lr |mW'|); the bias alike with sum|G| / B.  Wh' is bf16_rne of the kernel's own W', bit for bit.
The bank: 300 rows, ldx = C + 16, every row leaning towards one class so that the top-two gap is wide; idx non-monotone with repeats."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib, probe  # noqa: E402

import fenced  # noqa: E402
import logistic_ref as ref  # noqa: E402

DEV, U, S_X, N = "cuda:0", 2.0 ** -24, 2.0 ** -5, 300
CASES = [(64, 2, 1), (64, 65, 33), (192, 10, 64), (1536, 1000, 130), (4096, 1024, 257)]
LR, MU, WD = 0.05, 0.9, 1e-3


def problem(C, K, B, n=N):
    rng = np.random.default_rng(C + K + B)
    Kp = -(-K // 64) * 64
    W, mW, b, mb = np.zeros((Kp, C), np.float32), np.zeros((Kp, C), np.float32), np.zeros(Kp, np.float32), np.zeros(Kp, np.float32)
    W[:K] = rng.normal(size=(K, C)) * (100.0 / (S_X * 74.0 * np.sqrt(C)))      # logits of standard deviation 100
    mW[:K], b[:K], mb[:K] = rng.normal(size=(K, C)) * 0.1, rng.normal(size=K), rng.normal(size=K) * 0.1
    x = np.clip(rng.integers(-128, 128, size=(n, C)) + 20 * np.sign(W[np.arange(n) % K]).astype(np.int64), -128, 127).astype(np.int8)
    x[0, 0], x[1, 1] = -128, 127
    idx = rng.integers(0, n, size=B).astype(np.int32)
    idx[:2] = (1, 0)[:B]
    idx[-1] = 1
    return x, idx, rng.integers(0, K, size=B).astype(np.int32), W, b, mW, mb


@pytest.mark.parametrize("C,K,B", CASES)
def test_step_stage_by_stage(C, K, B):
    x, idx, y, W, b, mW, mb = problem(C, K, B)
    Kp, Bp, ldx, r = W.shape[0], -(-B // 64) * 64, C + 16, np.arange(B)
    Wh = ref.bf16_rne(W)

    def launch():
        f = dict(x=fenced.input(x, ldx, 127), W=fenced.input(W, C, 1e30), Wh=fenced.input(Wh.view(np.int16), C, 32767),
                 G=fenced.output(Kp, Bp, Bp, np.int16, fenced.SENTINELS[2][0]), z=fenced.output(B, Kp, Kp, np.float32, fenced.SENTINELS[4][0]),
                 loss=fenced.output(1, B, B, np.float32, fenced.SENTINELS[4][0]), top1=fenced.output(1, B, B, np.int32, fenced.SENTINELS[4][0]))
        t = {k: torch.from_numpy(v).to(DEV) for k, v in dict(idx=idx, y=y, b=b, mW=mW, mb=mb).items()}
        st = _lib.stream_ptr()
        _lib.call("ivit_probe_ce_forward_i8", f["x"].ptr, ldx, C, _lib.ptr(t["idx"]), _lib.ptr(t["y"]), B, K, S_X, f["Wh"].ptr, _lib.ptr(t["b"]),
                  f["G"].ptr, f["loss"].ptr, f["top1"].ptr, f["z"].ptr, st)
        _lib.call("ivit_probe_sgd_update_i8", f["x"].ptr, ldx, C, _lib.ptr(t["idx"]), B, K, S_X, f["G"].ptr, LR, MU, WD, f["W"].ptr,
                  _lib.ptr(t["b"]), _lib.ptr(t["mW"]), _lib.ptr(t["mb"]), f["Wh"].ptr, st)
        torch.cuda.synchronize()
        out = {k: v.rows2d(v.fetch())[:, :v.width].copy() for k, v in f.items()}
        for k, v in f.items():      # every dword of an output was stored; nothing outside any extent changed
            fenced.check(v, None if k == "x" else out[k])
        return {**out, **{k: t[k].cpu().numpy() for k in ("b", "mW", "mb")}}

    o = launch()
    again = launch()
    assert all(np.array_equal(o[k].view(np.uint8), again[k].view(np.uint8)) for k in o), "two runs differ"

    xg, Wv = x[idx].astype(np.float64), ref.bf16_value(Wh)
    z64 = S_X * (xg @ Wv.T) + b
    tol_z = (C + 4) * U * (S_X * (np.abs(xg) @ np.abs(Wv).T) + np.abs(b))
    assert (z64[:, :K].max(axis=1) - z64[:, :K].min(axis=1)).max() > 90
    assert (np.abs(o["z"] - z64)[:, :K] <= tol_z[:, :K]).all() and not o["z"][:, K:].any()

    g64, loss64, _, _ = ref.softmax_grad(o["z"][:, :K].astype(np.float64), y)
    G = ref.bf16_value(o["G"].view(np.uint16))
    assert (np.abs(G[:K, :B].T - g64) <= 2.0 ** -8 * np.abs(g64) + 2.0 ** -20).all() and not G[K:].any() and not G[:, B:].any()
    assert (np.abs(o["loss"][0] - loss64) <= (K + 8) * U * (1 + np.abs(loss64))).all()
    top2 = np.sort(z64[:, :K], axis=1)[:, -2:]
    sure = top2[:, 1] - top2[:, 0] > 2 * tol_z[:, :K].max(axis=1)
    assert (~sure).mean() <= 0.01 and np.array_equal(o["top1"][0][sure], z64[:, :K].argmax(axis=1)[sure])

    W64, b64, mW64, mb64 = ref.chain(G[:, :B] @ xg, G.sum(axis=1), B, S_X, *(v.astype(np.float64) for v in (W, b, mW, mb)), LR, MU, WD)
    e_m = (B + 4) * U * (S_X / B) * (np.abs(G[:, :B]) @ np.abs(xg)) + 6 * U * (np.abs(G[:, :B] @ xg) * S_X / B + WD * np.abs(W) + MU * np.abs(mW))
    e_mb = (B + 4) * U * np.abs(G).sum(axis=1) / B + 4 * U * (np.abs(G.sum(axis=1)) / B + MU * np.abs(mb))
    assert (np.abs(o["mW"] - mW64) <= e_m).all() and (np.abs(o["W"] - W64) <= LR * e_m + 2 * U * (np.abs(W) + LR * np.abs(mW64))).all()
    assert (np.abs(o["mb"] - mb64) <= e_mb).all() and (np.abs(o["b"] - b64) <= LR * e_mb + 2 * U * (np.abs(b) + LR * np.abs(mb64))).all()
    assert np.array_equal(o["Wh"].view(np.uint16), ref.bf16_rne(o["W"]))
    assert not any(o[k][K:].any() for k in ("W", "Wh", "mW", "b", "mb"))


def test_fit_logistic_follows_the_float64_trajectory():
    """C = 64, K = 5, 400 cluster rows, 3 epochs of batches of 64 (the last of an epoch has 16 rows).  On the CPU the float32
    restatement of the same trajectory ends within 1.9e-7 of the float64 one in W, relative to max|W|: the kernels get four times that."""
    rng = np.random.default_rng(5)
    labels = np.arange(400) % 5
    x = np.clip(np.rint(rng.normal(size=(5, 64))[labels] * 40 + rng.normal(size=(400, 64)) * 25), -128, 127).astype(np.int8)
    rows = torch.from_numpy(x).to(DEV)
    got = probe.fit_logistic(rows, torch.from_numpy(labels).to(DEV), S_X, 5, epochs=3, batch_size=64, lr=0.05, weight_decay=1e-4, seed=7)
    st, t = [np.zeros((5, 64)), np.zeros(5), np.zeros((5, 64)), np.zeros(5)], 0
    for epoch in range(3):
        perm = torch.randperm(400, generator=torch.Generator().manual_seed(7 + epoch)).numpy()
        for i in range(0, 400, 64):
            p = perm[i:i + 64]
            st = list(ref.step(x[p], labels[p], S_X, *st, probe.cosine_lr(0.05, t, 21), 0.9, 1e-4)[:4])
            t += 1
    drift = np.abs(got.W - st[0]).max() / np.abs(st[0]).max()
    print(f"final W: relative distance to the float64 trajectory {drift:.3g}")
    assert drift <= 4 * 1.9e-7
    z = S_X * x.astype(np.float64) @ st[0].T + st[1]
    assert np.array_equal(got.topk(rows, 1)[:, 0].cpu().numpy(), z.argmax(axis=1))
