"""Top-k outputs on CPU: the multi-rank gathers and the data-parallel evaluation with world-size-2 gloo ranks (real
collectives, shard bounds and arithmetic; a stub model and a torch stable-sort scorer stand in for the GPU), the C ABI
table, and the argument checks of the Python front (they fire before the library is touched)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ivit_amd import _lib, inference, topk
from ivit_amd.parallel import allreduce_hits, gather_logits, gather_rows, gather_topk, shard_bounds


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_two_ranks(target, *args):
    """start `target(rank, world, port, q, *args)` on two spawned gloo ranks -> what each rank put on the queue, by rank"""
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, 2, port, q) + args) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return got


def _init(rank, world, port):
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def stable_topk(logits, k):
    return torch.sort(logits, dim=1, descending=True, stable=True).indices[:, :k].to(torch.int32)


def _logits(n, classes, seed):
    """integer-valued float logits from a small range: many ties, so the stable order matters"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-20, 20, (n, classes), generator=g).float()


# ----------------------------------------------------------------------------------- gathers
def _gather_worker(rank, world, port, q, n, k, classes, uneven):
    _init(rank, world, port)
    logits = _logits(n, classes, 3)
    li = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, classes), generator=torch.Generator().manual_seed(4), dtype=torch.int64).to(torch.int32)
    bounds = [shard_bounds(n, world, r) for r in range(world)]
    counts = [hi - lo for lo, hi in bounds] if uneven else None
    lo, hi = bounds[rank]
    tk = gather_topk(stable_topk(logits[lo:hi], k), world, counts)
    lg = gather_logits(li[lo:hi].contiguous(), world, counts)
    q.put((rank, (tk.numpy(), lg.numpy())))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n,uneven", [(16, False), (1025, True)])
def test_two_rank_gather_topk_and_logits(n, uneven):
    k, classes = 5, 12
    got = _run_two_ranks(_gather_worker, n, k, classes, uneven)
    exp_tk = stable_topk(_logits(n, classes, 3), k).numpy()
    exp_lg = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, classes), generator=torch.Generator().manual_seed(4),
                           dtype=torch.int64).to(torch.int32).numpy()
    for r in range(2):
        tk, lg = got[r]
        assert tk.shape == (n, k) and tk.dtype == np.int32 and np.array_equal(tk, exp_tk)
        assert lg.shape == (n, classes) and np.array_equal(lg, exp_lg)


def test_single_process_gathers_are_identity():
    x = torch.arange(10, dtype=torch.int32).reshape(5, 2)
    assert gather_rows(x, 1) is x and gather_topk(x, 1) is x and gather_logits(x, 1) is x
    with pytest.raises(TypeError):
        gather_logits(x.float(), 1)
    h, tot = allreduce_hits(torch.tensor([3, 1, 0], dtype=torch.int64), 9)
    assert h.tolist() == [3, 1, 0] and tot == 9


# ----------------------------------------------------------------------------------- data-parallel evaluation
class StubModel(torch.nn.Module):
    """logits = a fixed function of each image alone (ties included), so any sharding must give the same counts"""

    def __init__(self, classes):
        super().__init__()
        self.classes = classes

    def forward(self, x):
        v = x.reshape(x.shape[0], -1)[:, :1].round().to(torch.int64)
        c = torch.arange(self.classes)
        return ((v * 7 + c * 3) % 11).float()       # 11 levels over 13 classes: every row has ties


def torch_scorer(logits, targets, hits, k=5):
    assert targets.dtype == torch.int32 and hits.dtype == torch.int64
    tk = stable_topk(logits, k)
    hit = tk == targets.reshape(-1, 1)
    hits += hit.sum(dim=0)


BATCH_SIZES = (7, 1, 16, 3, 1, 5)


def _loader(classes):
    g = torch.Generator().manual_seed(9)
    out = []
    for b in BATCH_SIZES:
        imgs = torch.randint(0, 40, (b, 3, 2, 2), generator=g).float()
        # targets at every rank 0-4 of the stable order, outside it, and -1 / `classes` (never a hit)
        ranked = torch.sort(StubModel(classes)(imgs), dim=1, descending=True, stable=True).indices
        pick = torch.randint(0, 8, (b,), generator=g)
        tgt = torch.where(pick < 5, ranked.gather(1, pick.clamp(max=4).reshape(-1, 1)).reshape(-1),
                          torch.where(pick == 5, -1, torch.where(pick == 6, classes, ranked[:, -1])))
        out.append((imgs, tgt))
    return out


def _expected(classes):
    c1 = c3 = c5 = n = 0
    for imgs, tgt in _loader(classes):
        hit = stable_topk(StubModel(classes)(imgs), 5) == tgt.reshape(-1, 1).to(torch.int32)
        c1 += int(hit[:, 0].sum())
        c3 += int(hit[:, :3].any(dim=1).sum())
        c5 += int(hit.any(dim=1).sum())
        n += imgs.shape[0]
    return 100 * c1 / n, 100 * c3 / n, 100 * c5 / n


def _eval_worker(rank, world, port, q, classes):
    _init(rank, world, port)
    seen = []

    class Recording(StubModel):
        def forward(self, x):
            seen.append(x.shape[0])
            return super().forward(x)

    res = inference.evaluate_dataset_parallel(Recording(classes), _loader(classes), "cpu", scorer=torch_scorer,
                                              print_batch_stats=False)
    q.put((rank, (res, seen)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_evaluate_dataset_parallel_equals_single_process():
    classes = 13
    exp = _expected(classes)
    assert 0 < exp[0] < exp[1] < exp[2] < 100          # the fixture exercises all three counts
    single = inference.evaluate_dataset_parallel(StubModel(classes), _loader(classes), "cpu", scorer=torch_scorer,
                                                 print_batch_stats=False)
    assert single == exp
    got = _run_two_ranks(_eval_worker, classes)
    for r in range(2):
        res, seen = got[r]
        assert res == exp, (r, res, exp)
        # each rank forwarded exactly its shard of every batch; the batches of 1 leave rank 1 without a forward
        assert seen == [hi - lo for b in BATCH_SIZES for lo, hi in [shard_bounds(b, 2, r)] if hi > lo]
    assert sum(got[0][1]) + sum(got[1][1]) == sum(BATCH_SIZES)


def test_evaluate_dataset_parallel_empty_loader():
    assert inference.evaluate_dataset_parallel(StubModel(13), [], "cpu", scorer=torch_scorer,
                                               print_batch_stats=False) == (0.0, 0.0, 0.0)


# ----------------------------------------------------------------------------------- C ABI and argument checks
def test_signatures_of_the_topk_entries():
    vp, ci = C.c_void_p, C.c_int
    assert _lib.SIGNATURES["ivit_head_topk"] == [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES["ivit_logits_topk_f32"] == [vp, ci, ci, ci, ci, vp, vp, vp, vp]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ivit_hip.h")).read()
    assert "#define IVIT_TOPK_MAX 8" in header and topk.TOPK_MAX == 8


@pytest.mark.parametrize("args,msg", [
    ((1, 1000, 1000, 0), "bad k"), ((1, 1000, 1000, 9), "bad k"), ((1, 8, 5, 6), "bad k"), ((1, 8, 9, 5), "bad k"),
])
def test_c_entries_refuse_bad_k_before_any_launch(args, msg):
    """argument validation happens before any HIP call (the pointers are never dereferenced on this path)"""
    fake = C.c_void_p(256)
    B, ld, N, k = args
    with pytest.raises(_lib.IvitError, match=msg):
        _lib.call("ivit_head_topk", fake, fake, B, ld, N, k, None, fake, None, None, None)
    with pytest.raises(_lib.IvitError, match=msg):
        _lib.call("ivit_logits_topk_f32", fake, B, ld, N, k, fake, None, None, None)


def test_c_entries_refuse_targets_without_hits_and_null_output():
    fake = C.c_void_p(256)
    with pytest.raises(_lib.IvitError, match="together"):
        _lib.call("ivit_head_topk", fake, fake, 4, 1000, 1000, 5, None, fake, fake, None, None)
    with pytest.raises(_lib.IvitError, match="together"):
        _lib.call("ivit_logits_topk_f32", fake, 4, 1000, 1000, 5, fake, None, fake, None)
    with pytest.raises(_lib.IvitError, match="bad operand"):
        _lib.call("ivit_head_topk", fake, fake, 4, 1000, 1000, 5, None, None, None, None, None)
    with pytest.raises(_lib.IvitError, match="bad operand"):
        _lib.call("ivit_logits_topk_f32", fake, 4, 1000, 1000, 5, None, None, None, None)


@pytest.fixture
def no_library(monkeypatch):
    def touched(*a, **kw):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", touched)
    monkeypatch.setattr(_lib, "lib", touched)


def test_python_front_checks_arguments_first(no_library):
    x = torch.zeros(4, 5)
    with pytest.raises(ValueError, match="k=6"):
        topk.topk(x, 6)
    with pytest.raises(ValueError, match="k=9"):
        topk.topk(torch.zeros(4, 20), 9)
    with pytest.raises(ValueError, match="k=5"):
        topk.topk(torch.zeros(4, 8), 5, n_classes=4)
    with pytest.raises(ValueError, match="k=0"):
        topk.topk(x, 0)
    with pytest.raises(TypeError, match="float32"):
        topk.topk(x.double(), 3)
    with pytest.raises(TypeError, match="float32"):
        topk.topk(torch.zeros(5), 3)
    with pytest.raises(ValueError, match="GPU"):
        topk.topk(x, 3)
    t, h = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="k=5"):
        topk.count_hits(torch.zeros(4, 3), t, torch.zeros(5, dtype=torch.int64), k=5)
    with pytest.raises(TypeError, match="targets"):
        topk.count_hits(x, t.long(), h)
    with pytest.raises(TypeError, match="targets"):
        topk.count_hits(x, torch.zeros(3, dtype=torch.int32), h)
    with pytest.raises(TypeError, match="hits"):
        topk.count_hits(x, t, h.int())
    with pytest.raises(TypeError, match="hits"):
        topk.count_hits(x, t, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(TypeError, match="float32"):
        topk.count_hits(x.half(), t, h)
    with pytest.raises(ValueError, match="GPU"):
        topk.count_hits(x, t, h)


def test_engine_topk_request_checks():
    t, h = torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)
    topk.check_request(1000, 4, "cpu", 5, t, h)
    topk.check_request(1000, 4, "cpu", 8, None, None)
    with pytest.raises(ValueError, match="k=9"):
        topk.check_request(1000, 4, "cpu", 9, None, None)
    with pytest.raises(ValueError, match="k=5"):
        topk.check_request(4, 4, "cpu", 5, None, None)
    with pytest.raises(ValueError, match="together"):
        topk.check_request(1000, 4, "cpu", 5, t, None)
    with pytest.raises(TypeError, match="targets"):
        topk.check_request(1000, 3, "cpu", 5, t, h)
    with pytest.raises(TypeError, match="hits"):
        topk.check_request(1000, 4, "cpu", 4, t, h)
