"""Backbone mode on the CPU, the native library stubbed as tests/test_engine_launch_trace.py stubs it: the launches of
forward_features (nothing behind the final LayerNorm of a ViT, nothing behind the pooling of a Swin, but the one dequantisation) and of
forward_intermediates_early (the early stop; forward_intermediates keeps its signature), argument errors before any launch, headless engines, features_unsupported_reason() next to
engine_unsupported_reason() over the grid of tests/test_attention_long_cpu.py, the ctypes row of ivit_dequant_rows_i8_f32 against
its prototype, and extract_features_parallel between two gloo ranks with even and uneven shards."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ivit_amd import _lib
from ivit_amd.checkpoint import load_synthetic_model
from ivit_amd.engine import IntViTEngine
from ivit_amd.inference import extract_features, extract_features_parallel
from ivit_amd.swin_engine import IntSwinEngine
from ivit_amd.synth import IMG_SIZE
import ivit_amd.swin_quant as sq
import ivit_amd.vit_quant as vq

from test_attention_long_cpu import WIDE
from test_engine_launch_trace import _deit, _swin, stubbed  # noqa: F401 (stubbed: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(calls):
    return [n for n, _ in calls]


def _run(calls, fn):
    del calls[:]
    out = fn()
    return _names(calls), out


# ----------------------------------------------------------------------------------------------- forward_features
@pytest.mark.parametrize("case,kw", [("deit_tiny", {}), ("deit_tiny_natural", {}), ("deit_tiny_ibert", dict(family="ibert")),
                                     ("deit_tiny_w16", dict(stream_bits=16))])
def test_vit_forward_features_launches(stubbed, case, kw):
    eng = _deit(case, **kw)
    x = torch.zeros(3, 3, eng.IMG, eng.IMG)
    full, _ = _run(stubbed, lambda: eng.forward(x))
    tail, _ = _run(stubbed, lambda: eng.forward(x, cls_tail=True)) if eng.cls_tail_ok else (full, None)
    assert "layernorm" in full[-3] and full[-2:] == ["ivit_gemm_i8_i32", "ivit_head_argmax"]
    ints, (q, s) = _run(stubbed, lambda: eng.forward_features(x, integers=True))
    flt, (f, s2) = _run(stubbed, lambda: eng.forward_features(x))
    # the forward the graph replays run, cut behind its final LayerNorm
    assert ints == tail[:-2] and "layernorm" in ints[-1]
    assert flt == ints + ["ivit_dequant_rows_i8_f32"]
    assert ("ivit_attention_cls_i8" in ints) == eng.cls_tail_ok == (case in ("deit_tiny", "deit_tiny_natural"))
    assert q.dtype == torch.int8 and f.dtype == torch.float32 and tuple(q.shape) == tuple(f.shape) == (3, eng.C)
    assert s == s2 == eng.s_feat and isinstance(s, float)
    name, args = stubbed[-1]
    assert name == "ivit_dequant_rows_i8_f32" and len(args) == len(_lib.SIGNATURES[name])
    assert args[0].value == eng.ws["cls"].data_ptr() and args[1:4] == (eng.C, 3, eng.C) and args[4] == s
    assert args[5].value == f.data_ptr() and args[6] == eng.C
    bank = torch.zeros(5, eng.C + 7)
    _run(stubbed, lambda: eng.forward_features(x, out=bank[1:4, 2:2 + eng.C]))
    args = stubbed[-1][1]
    assert args[5].value == bank[1:4, 2:].data_ptr() and args[6] == eng.C + 7, "the bank's row stride"


@pytest.mark.parametrize("case", ["swin_tiny", "swin_tiny_natural"])
def test_swin_forward_features_launches(stubbed, case):
    eng = _swin(case)
    x = torch.zeros(2, 3, IMG_SIZE, IMG_SIZE)
    full, _ = _run(stubbed, lambda: eng.forward(x))
    assert full[-3].startswith("ivit_avgpool_requant_i8") and full[-2:] == ["ivit_gemm_i8_i32", "ivit_head_argmax"]
    ints, (q, s) = _run(stubbed, lambda: eng.forward_features(x, integers=True))
    flt, (f, _) = _run(stubbed, lambda: eng.forward_features(x))
    assert ints == full[:-2] and flt == ints + ["ivit_dequant_rows_i8_f32"]
    assert tuple(q.shape) == tuple(f.shape) == (2, eng.C_last) and s == eng.s_feat
    args = stubbed[-1][1]
    assert args[0].value == eng.ws["pooled"].data_ptr() and args[1:4] == (eng.C_last, 2, eng.C_last) and args[6] == eng.C_last


# ----------------------------------------------------------------------------------------------- stop_early
def test_vit_stop_early_launches(stubbed):
    eng = _deit("deit_tiny")
    x = torch.zeros(2, 3, eng.IMG, eng.IMG)
    full, _ = _run(stubbed, lambda: eng.forward(x))
    per = (len(full) - 6) // eng.D
    assert len(full) == 6 + per * eng.D
    for indices in ((0,), (0, eng.D - 2), (2, 5, 8)):
        whole, (maps, scales) = _run(stubbed, lambda: eng.forward_intermediates(x, indices))
        early, (maps_e, scales_e) = _run(stubbed, lambda: eng.forward_intermediates_early(x, indices))
        assert scales == scales_e and list(maps) == list(maps_e) == list(indices)
        last = max(indices)
        # the whole call's launches up to the map of the last selected block, and nothing more
        assert len(whole) == len(full) + len(indices)
        assert early == whole[:len(early)] and len(early) == 3 + per * (last + 1) + len(indices)
        assert early[-1] == "ivit_tokens_to_nchw_i8_f32" and "ivit_gemm_i8_i32" not in early and "ivit_head_argmax" not in early


def test_swin_stop_early_launches(stubbed):
    eng = _swin("swin_tiny")
    x = torch.zeros(2, 3, IMG_SIZE, IMG_SIZE)
    full, _ = _run(stubbed, lambda: eng.forward(x))
    for indices in ((0,), (1, 0), (3,)):
        whole, (maps, scales) = _run(stubbed, lambda: eng.forward_intermediates(x, indices))
        early, (maps_e, scales_e) = _run(stubbed, lambda: eng.forward_intermediates_early(x, indices))
        assert scales == scales_e and list(maps) == list(maps_e) == list(indices) and len(whole) == len(full) + len(indices)
        assert early == whole[:len(early)] and early[-1] == "ivit_tokens_to_nchw_i16_f32"
        assert early.count("ivit_patch_merge_i16") == max(indices) and whole.count("ivit_patch_merge_i16") == 3
        assert early.count("ivit_tokens_to_nchw_i16_f32") == len(indices)
        assert not [n for n in early if n.startswith(("ivit_avgpool", "ivit_head_"))] and "ivit_gemm_i8_i32" not in early


# ----------------------------------------------------------------------------------------------- errors, headless engines
def test_argument_errors_before_any_launch(stubbed):
    for eng, x, C in ((_deit("deit_tiny"), torch.zeros(2, 3, 224, 224), 192), (_swin("swin_tiny"), torch.zeros(2, 3, IMG_SIZE, IMG_SIZE), 768)):
        del stubbed[:]
        for out, integers in ((torch.zeros(2, C, dtype=torch.int8), False), (torch.zeros(2, C), True), (torch.zeros(2, C, dtype=torch.float64), False),
                              (torch.zeros(3, C), False), (torch.zeros(2, C + 1), False), (torch.zeros(C, 2).t(), False),
                              (torch.zeros(2, 2 * C)[:, ::2], False), (torch.zeros(2 * C), False)):
            with pytest.raises((TypeError, ValueError), match="out"):
                eng.forward_features(x, integers, out=out)
        n = 12 if isinstance(eng, IntViTEngine) else 4
        for bad in ((n,), (-1,), (0, 0)):
            with pytest.raises(ValueError, match="indices"):
                eng.forward_intermediates_early(x, bad)
        assert stubbed == []


def test_headless_engines(stubbed):
    fs, ranges, cfg, _, _ = load_synthetic_model("deit_tiny")
    fs = {k: v for k, v in fs.items() if not k.startswith("head.")}
    eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device="cpu", max_batch=4)
    headed = _deit("deit_tiny")
    x = torch.zeros(2, 3, 224, 224)
    sfs, sranges, scfg, _, _ = load_synthetic_model("swin_tiny")
    sfs = {k: v for k, v in sfs.items() if not k.startswith("head.")}
    seng = IntSwinEngine(sfs, sranges, scfg["embed_dim"], scfg["depths"], scfg["num_heads"], scfg["window"], device="cpu", max_batch=2)
    sheaded = _swin("swin_tiny")
    sx = torch.zeros(2, 3, IMG_SIZE, IMG_SIZE)
    for e, h, xx in ((eng, headed, x), (seng, sheaded, sx)):
        assert e.head is None and e.head_scale is None and e.num_classes == 0 and "logits" not in e.ws and "logits_f" not in e.ws
        del stubbed[:]
        for call in (lambda: e.forward(xx), lambda: e(xx), lambda: e.forward_topk(xx, 1), lambda: e.forward_graph(xx),
                     lambda: e.forward_topk_graph(xx, 1)):
            with pytest.raises(ValueError, match="no classification head"):
                call()
        assert stubbed == []
        # the launches of the headed engine for the same calls
        assert _run(stubbed, lambda: e.forward_features(xx))[0] == _run(stubbed, lambda: h.forward_features(xx))[0]
        assert _run(stubbed, lambda: e.forward_intermediates(xx, (1, 0)))[0] == \
            _run(stubbed, lambda: h.forward_intermediates_early(xx, (1, 0)))[0]
        maps_e = _run(stubbed, lambda: e.attention_maps(xx))[0]
        maps_h = _run(stubbed, lambda: h.attention_maps(xx))[0]
        assert maps_e == maps_h[:-2] and maps_h[-2:] == ["ivit_gemm_i8_i32", "ivit_head_argmax"]
    assert eng.int8_weight_bytes == headed.int8_weight_bytes - headed.head["W"].numel()


# ----------------------------------------------------------------------------------------------- the two reasons
@pytest.mark.parametrize("img,patch,tokens", [(224, 16, 197), (160, 16, 101), (224, 32, 50), (256, 16, 257), (384, 16, 577),
                                              (224, 8, 785), (512, 16, 1025), (528, 16, 1090)])
@pytest.mark.parametrize("family", ["ivit", "ibert"])
@pytest.mark.parametrize("stream", [8, 16])
def test_features_reason_is_the_engine_reason_without_the_head(img, patch, tokens, family, stream):
    def make(num_classes):
        return vq.VisionTransformer(img_size=img, patch_size=patch, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                    num_classes=num_classes, gelu_type=family, softmax_type=family, layernorm_type=family,
                                    **(WIDE if stream == 16 else {}))
    m, headless = make(10), make(0)
    assert (img // patch) ** 2 + 1 == tokens
    reason = m.engine_unsupported_reason()
    assert m.features_unsupported_reason() == reason                   # a model with a head: the same answer everywhere
    assert headless.features_unsupported_reason() == reason            # the head is the only difference ...
    if tokens > 1025:
        assert "geometry" in headless.engine_unsupported_reason()      # ... and sits where it always sat, behind the geometry
    else:
        assert headless.engine_unsupported_reason() == "no classification head"
    if reason is None:
        assert headless._engine_widths[0] == stream


def test_swin_features_reason():
    kw = dict(img_size=56, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2), num_heads=(3, 6))
    for family in ("ivit", "ibert"):
        ops = dict(gelu_type=family, softmax_type=family, layernorm_type=family)
        m, headless = sq.SwinTransformer(num_classes=10, **kw, **ops), sq.SwinTransformer(num_classes=0, **kw, **ops)
        assert m.features_unsupported_reason() == m.engine_unsupported_reason() == headless.features_unsupported_reason()
        assert (m.engine_unsupported_reason() is None) == (family == "ivit")
        assert m.engine_structure_reason() is None and headless.engine_structure_reason(head=False) is None
        assert headless.engine_structure_reason() == "no classification head"
        assert headless.engine_unsupported_reason() == ("no classification head" if family == "ivit" else m.engine_unsupported_reason())


def test_predicates_share_their_conditions():
    m = vq.VisionTransformer(img_size=224, patch_size=16, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True, num_classes=0)
    x = torch.zeros(1, 3, 224, 224)

    class OnGpu:
        is_cuda = True
    assert not m.is_frozen() and not m.takes_engine_for_features(OnGpu)      # running statistics
    from ivit_amd.model_utils import freeze_model
    freeze_model(m)
    m.eval()
    assert m.takes_engine_for_features(OnGpu) and not m.takes_engine(OnGpu)
    assert not m.takes_engine_for_features(x)                                  # a CPU tensor
    m.use_engine = False
    assert not m.takes_engine_for_features(OnGpu)
    m.use_engine = True
    m.train()
    assert not m.takes_engine_for_features(OnGpu)
    with pytest.raises(ValueError, match="features_graph"):
        m.eval().features_graph(x)


# ----------------------------------------------------------------------------------------------- the ctypes row
def test_dequant_rows_prototype_matches_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "ivit_hip.h")).read()
    m = re.search(r"int ivit_dequant_rows_i8_f32\(([^)]*)\);", hdr)
    assert m, "ivit_dequant_rows_i8_f32 is not declared"
    kinds = {"const int8_t*": _lib.vp, "float*": _lib.vp, "int": _lib.ci, "int64_t": _lib.i64, "float": _lib.f32, "ivit_stream_t": _lib.vp}
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1] for p in params] == ["x", "ldx", "rows", "C", "s", "out", "ldo", "stream"]
    assert _lib.SIGNATURES["ivit_dequant_rows_i8_f32"] == [kinds[re.sub(r"\s+\w+$", "", p)] for p in params]


# ----------------------------------------------------------------------------------------------- two gloo ranks
C_STUB, S_STUB = 24, float(np.float32(0.0123))      # a float32 scale, as the engines' are


class StubModel:
    """features = a deterministic function of the image content, so the gathered bank is checkable"""
    num_features = C_STUB

    def eval(self):
        return self

    def features(self, x, integers=False, out=None):
        base = x.reshape(x.shape[0], -1).sum(dim=1).round().to(torch.int64)
        q = ((base[:, None] * 7 + torch.arange(C_STUB)[None, :] * 13) % 256 - 128).to(torch.int8)
        f = q if integers else q.float() * torch.tensor(S_STUB, dtype=torch.float32)
        if out is not None:
            out.copy_(f)
            f = out
        return f, S_STUB


LOADERS = {"even": (4, 4, 4), "uneven": (5, 3, 1), "one_image": (1,), "empty": ()}


def _loader(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    imgs = torch.randint(0, 50, (n, 3, 4, 4), generator=g).float()
    targets = torch.randint(0, 1000, (n,), generator=g)
    at, out = 0, []
    for b in sizes:
        out.append((imgs[at:at + b], targets[at:at + b]))
        at += b
    return out, imgs, targets


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got = {}
    for i, (name, sizes) in enumerate(LOADERS.items()):
        loader, _, _ = _loader(sizes, i)
        for integers in (False, True):
            f, labels, s = extract_features_parallel(StubModel(), loader, "cpu", integers=integers)
            got[(name, integers)] = (f.numpy(), labels.numpy(), s)
    q.put((rank, got))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_extract_features_parallel():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(results) == [0, 1]
    for i, (name, sizes) in enumerate(LOADERS.items()):
        loader, imgs, targets = _loader(sizes, i)
        for integers in (False, True):
            want_f, want_l, want_s = extract_features(StubModel(), loader, "cpu", integers=integers)      # one process, no group
            direct = StubModel().features(imgs, integers)[0] if len(sizes) else want_f
            assert np.array_equal(want_f.numpy().view(np.uint8), direct.numpy().view(np.uint8)) and torch.equal(want_l, targets)
            for rank in (0, 1):
                f, labels, s = results[rank][(name, integers)]
                assert f.dtype == (np.int8 if integers else np.float32) and f.shape == (sum(sizes), C_STUB), (name, rank)
                assert np.array_equal(f.view(np.uint8), want_f.numpy().view(np.uint8)), (name, integers, rank)
                assert labels.dtype == np.int64 and np.array_equal(labels, targets.numpy())
                assert s == want_s == (S_STUB if sizes else None)
