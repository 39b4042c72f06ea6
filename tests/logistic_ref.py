"""The logistic probe's step (include/ivit_hip.h, "logistic linear probe") restated in numpy: float64 by default, with the two bf16
rounding points of the contract (Wh = bf16_rne(W), G = bf16_rne(p - onehot)) done on the bits of float32.  dtype=np.float32 runs the
same statements in float32 (the reference against itself: how far plain float32 drifts); rounding=False is plain softmax regression."""
import numpy as np


def bf16_rne(a):
    """float32 -> bf16 bit patterns (uint16), round to nearest even, on the integers"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def softmax_grad(z, y):
    """logits [B, K], labels [B] -> (g = p - onehot, loss, m, S) in the dtype of z"""
    r = np.arange(len(y))
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    S = e.sum(axis=1)
    g = e / S[:, None]
    g[r, y] -= 1
    return g, np.log(S) - (z[r, y] - m), m, S


def chain(D, T, B, s, W, b, mW, mb, lr, mu, wd):
    """D = G^T x [K, C] and T = the column sums of G [K] -> (W', b', mW', mb')"""
    t = W.dtype.type
    mW = t(mu) * mW + (D * (t(s) / t(B)) + t(wd) * W)
    mb = t(mu) * mb + T / t(B)
    return W - t(lr) * mW, b - t(lr) * mb, mW, mb


def step(x, y, s, W, b, mW, mb, lr, mu=0.9, wd=0.0, rounding=True, dtype=np.float64):
    """one step on the gathered int8 rows x [B, C] -> (W', b', mW', mb', loss)"""
    W, b, mW, mb = (np.asarray(v, dtype) for v in (W, b, mW, mb))
    xf = x.astype(dtype)
    Wh = bf16_value(bf16_rne(W)).astype(dtype) if rounding else W
    g, loss, _, _ = softmax_grad((xf @ Wh.T) * dtype(s) + b, y)
    G = bf16_value(bf16_rne(g)).astype(dtype) if rounding else g
    return chain(G.T @ xf, G.sum(axis=0), len(y), s, W, b, mW, mb, lr, mu, wd) + (loss,)
