"""ivit_knn_topk_i8_wide on the GPU, bit for bit against tests/knn_ref.py: the geometry sweep over the uneven channel splits (waves
without channels at C = 64 .. 192), the value extremes at C = 4096 where float32(dot) must round, ties across sub-tile, tile and
segment boundaries, the refusals, and a pooled bank of W = 1152 through inference.evaluate_knn(wide=True)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
from ivit_amd import _lib  # noqa: E402
from ivit_amd.inference import evaluate_knn, extract_features  # noqa: E402

import knn_ref  # noqa: E402
from test_gpu_knn import DEV, dev, rand8, rnorm_gpu, st, workspace  # noqa: E402


def search(qd, bd, rn, k, splits, entry="ivit_knn_topk_i8_wide"):
    Q, N = qd.shape[0], bd.shape[0]
    ws, need = workspace(Q, N, k, splits)
    idx = torch.full((Q, k), -7, dtype=torch.int32, device=DEV)
    score = torch.full((Q, k), float("nan"), dtype=torch.float32, device=DEV)
    _lib.call(entry, _lib.ptr(qd), qd.stride(0), Q, _lib.ptr(bd), bd.stride(0), N, bd.shape[1], _lib.ptr(rn), k, splits, _lib.ptr(idx),
              _lib.ptr(score), _lib.ptr(ws), need, st())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), knn_ref.bits(score.cpu().numpy())


def check(q, bank, ks, splits, ridx, rsc, both=False):
    qd, bd = dev(q), dev(bank)
    rn = rnorm_gpu(bd)
    assert np.array_equal(knn_ref.bits(rn.cpu().numpy()), knn_ref.bits(knn_ref.rnorm(bank)))
    for k in ks:
        for sp in splits:
            for entry in ("ivit_knn_topk_i8_wide",) + (("ivit_knn_topk_i8",) if both else ()):
                idx, sc = search(qd, bd, rn, k, sp, entry)
                assert np.array_equal(idx, ridx[:, :k]) and np.array_equal(sc, knn_ref.bits(rsc[:, :k])), f"{entry} k={k} splits={sp}"


@pytest.mark.parametrize("N", [1, 65, 257])
@pytest.mark.parametrize("Cc", [64, 192, 1088, 1536, 4096])
def test_geometry(Cc, N):
    rng = np.random.default_rng(1000 * Cc + N)
    bank = rand8(rng, N, Cc)
    ks = [k for k in (1, 20, 256) if k <= N]
    for Q in (1, 33):
        q = rand8(rng, Q, Cc)
        check(q, bank, ks, (0, 1, 3), *knn_ref.topk(q, bank, max(ks)), both=Cc <= 192)


def test_value_extremes_at_4096():
    rng = np.random.default_rng(7)
    bank, q = rand8(rng, 70, 4096), rand8(rng, 20, 4096)
    bank[0], bank[1], bank[2], bank[3], bank[65] = -128, 127, -127, 0, -128
    q[0], q[1], q[2], q[3] = -128, 127, -127, 127
    q[3, 1000] = 126
    dot = q.astype(np.int64) @ bank.astype(np.int64).T      # knn_ref.scores stops at 2^24: the same three lines without its assertion
    assert dot[0, 0] == 2 ** 26 and dot[3, 1] > 2 ** 25 and dot[3, 1] % 4 and int(np.float32(dot[3, 1])) != dot[3, 1]
    s = (dot.astype(np.float32) * knn_ref.rnorm(bank)[None, :]).astype(np.float32)
    ridx = np.stack([np.lexsort((np.arange(70), -(r + np.float32(0))))[:70] for r in s]).astype(np.int32)
    check(q, bank, (1, 70), (1, 2), ridx, np.take_along_axis(s, ridx.astype(np.int64), 1))
    assert tuple(ridx[0, :3]) == (0, 2, 65) and ridx[3, 0] == 1


def test_equal_rows_across_subtile_tile_and_segment_boundaries():
    rng = np.random.default_rng(4)
    bank = rand8(rng, 300, 1088)                # splits = 2: segments of 192 rows; tiles of 64, sub-tiles of 16
    twin = (10, 15, 16, 63, 64, 100, 191, 192, 250)
    bank[list(twin)] = bank[10]
    q = rand8(rng, 20, 1088)
    q[0] = bank[10]
    ridx, rsc = knn_ref.topk(q, bank, 20)
    assert tuple(ridx[0, :9]) == twin
    check(q, bank, (3, 9, 20), (0, 1, 2, 3), ridx, rsc)


def test_refusals_leave_the_outputs_untouched():
    L, p = _lib.lib(), _lib.ptr
    rng = np.random.default_rng(8)
    N, Q = 300, 9
    bank, qd = dev(rand8(rng, N, 4160)), dev(rand8(rng, Q, 4160))
    rn = torch.ones(N, dtype=torch.float32, device=DEV)
    idx = torch.full((Q, 257), -7, dtype=torch.int32, device=DEV)
    score = torch.full((Q, 257), 5.0, dtype=torch.float32, device=DEV)
    ws = torch.full((Q * 3 * 257,), -3, dtype=torch.int64, device=DEV)

    def run(q=p(qd), b=p(bank), ldb=4160, Cn=1088, k=5, splits=3, w=p(ws)):
        return L.ivit_knn_topk_i8_wide(q, 4160, Q, b, ldb, N, Cn, p(rn), k, splits, p(idx), p(score), w, ws.numel() * 8, st())

    assert run(Cn=4160) == -2 and run(Cn=96) == -2 and run(k=257) == -2 and b"unsupported geometry" in L.ivit_last_error_string()
    assert run(ldb=1024) == -1 and run(q=qd.data_ptr() + 8) == -1 and run(b=bank.data_ptr() + 4) == -1 and run(w=None) == -1
    torch.cuda.synchronize()
    assert (idx == -7).all() and (score == 5.0).all() and (ws == -3).all()
    assert run() == 0
    torch.cuda.synchronize()
    ridx, _ = knn_ref.topk(qd.cpu().numpy()[:, :1088], bank.cpu().numpy()[:, :1088], 5, np.ones(N, np.float32))
    assert np.array_equal(idx.view(-1)[:Q * 5].view(Q, 5).cpu().numpy(), ridx)


def test_evaluate_knn_on_a_pooled_bank_of_1152_channels():
    from test_gpu_probe_wide import pooled_model
    model, loader, n = pooled_model()
    with pytest.raises(ValueError, match="pass wide=True"):
        extract_features(model, loader, DEV, integers=True, n_last=5, avgpool=True)
    rows = extract_features(model, loader, DEV, integers=True, n_last=5, avgpool=True, wide=True)[0]
    assert rows.dtype == torch.int8 and rows.shape == (n, 1152)
    assert np.unique(rows.cpu().numpy(), axis=0).shape[0] == n, "the test wants images with distinct embeddings"
    assert evaluate_knn(model, loader, loader, DEV, k=1, n_last=5, avgpool=True, wide=True) == {1: (100.0, 100.0)}
