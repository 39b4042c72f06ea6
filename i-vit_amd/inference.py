"""Checkpoint loading, calibration warm-up and dataset evaluation with the reference's harness semantics
(/root/reference/scripts/inference.py:33-91 calibrate_model, :94-224 load_model, :231-267 evaluate_dataset;
checkpoint layout written by /root/reference/quant_train.py:470-500), on the MI355X integer path.

What is the same: the checkpoint dict (`'model'` state_dict + optional `'model_config'`, or a bare state_dict), the
override arguments, the scalar -> [1] buffer fix-up, `strict_load` skipping the warm-up, `freeze_model` at the end,
and the (top-1, top-3, top-5) percentages `evaluate_dataset` returns.

What differs, deliberately:
  * the reference always instantiates `deit_tiny_patch16_224` whatever `model_config['model_name']` says (:133); here
    the name selects the factory when it is one this package provides (DeiT-T/S/B, ViT-B/L, Swin-T/S/B) and falls back
    to DeiT-T otherwise;
  * operator families: 'ivit' and 'ibert' exist, for DeiT / ViT and for Swin; the reference's DEFAULTS are kept -- 'ibert'
    when the saved configuration lacks a type (:111-113), and for a checkpoint without any configuration the reference
    picks its 'ppoly_...' GELU / softmax (:160-162), which this path does not implement: that case raises with a message
    naming the override to pass, instead of silently substituting another operator;
  * calibration takes any iterable of image batches (no torchvision / ImageNet reader in this environment); the
    single random warm-up forward of `use_random_calibration` is kept as is.
"""
from __future__ import annotations

import time
from typing import Iterable, Optional

import torch
import torch.distributed as dist

from . import swin_quant, topk, vit_quant
from .knn import FeatureBank, knn_weights
from .model_utils import freeze_model
from .parallel import allreduce_hits, shard_bounds
from .probe import BankStats

FACTORIES = {name: getattr(mod, name) for mod in (vit_quant, swin_quant) for name in mod.__all__ if name.endswith("_224")}
_BW_KEYS = ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw",
            "norm2_in_bw", "att_block_out_bw")


def set_act_percentile(model, p):
    """Set `percentile` on every QuantAct of `model` (the one inside IBERTIntSoftmax included): while its statistics run, each then
    observes torch.quantile at (100 - p) / 2 and 100 - (100 - p) / 2 per cent of its flattened input instead of min / max
    (quant_modules.py:319-329; ivit_quantile_pair_f32 on the device).  None restores min / max.  `percentile` is a plain attribute,
    not a buffer: like the reference's it is not part of the state_dict, so a checkpoint does not carry it -- only the ranges it led to."""
    from .quantization_utils.quant_modules import QuantAct
    for m in model.modules():
        if isinstance(m, QuantAct):
            m.percentile = p
    return model


def calibrate_model(model, device, batches: Optional[Iterable[torch.Tensor]] = None, use_random_calibration: bool = False,
                    act_percentile=None):
    """Running-stat forward passes that initialise / update every QuantAct range (inference.py:33-91).  `act_percentile`: call
    set_act_percentile(model, act_percentile) first (the attribute stays set afterwards and is never saved)."""
    if act_percentile is not None:
        set_act_percentile(model, act_percentile)
    model.eval()
    with torch.no_grad():
        if use_random_calibration:
            model(torch.randn(1, 3, 224, 224, device=device))
            return
        if batches is None:
            raise ValueError("batches is required when use_random_calibration=False")
        for imgs in batches:
            if isinstance(imgs, (tuple, list)):   # (images, targets) pairs of a data loader
                imgs = imgs[0]
            model(imgs.to(device))


def build_model(model_config: Optional[dict] = None, num_classes: int = 1000, gelu_type=None, softmax_type=None,
                layernorm_type=None, bitwidth=None):
    """The model construction half of load_model (inference.py:100-189)."""
    cfg = dict(model_config or {})
    name = cfg.get("model_name", "deit_tiny")
    factory = FACTORIES.get(name) or FACTORIES.get(f"{name}_patch16_224") or FACTORIES["deit_tiny_patch16_224"]
    if model_config is None:
        # inference.py:160-162: a configuration-less checkpoint gets the reference's ppoly GELU / softmax and I-BERT LayerNorm
        if gelu_type is None or softmax_type is None:
            raise KeyError("checkpoint without 'model_config': the reference would build its 'ppoly_deg_2_seg_16_...' GELU / "
                           "softmax here (scripts/inference.py:160-162), which the MI355X integer path does not implement -- "
                           "pass gelu_type= / softmax_type= ('ivit' or 'ibert') explicitly")
        ops = dict(gelu_type=gelu_type, softmax_type=softmax_type,
                   layernorm_type=layernorm_type if layernorm_type is not None else "ibert")
    else:
        ops = dict(gelu_type=gelu_type if gelu_type is not None else cfg.get("gelu_type", "ibert"),       # :111-113
                   softmax_type=softmax_type if softmax_type is not None else cfg.get("softmax_type", "ibert"),
                   layernorm_type=layernorm_type if layernorm_type is not None else cfg.get("layernorm_type", "ibert"))
    if factory.__name__.startswith("swin"):      # no per-site width arguments: the reference's Swin fixes its QuantAct widths
        return factory(pretrained=False, num_classes=cfg.get("num_classes", num_classes),
                       drop_rate=cfg.get("drop_rate", 0.0), drop_path_rate=cfg.get("drop_path_rate", 0.1), **ops)
    bws = {k: (bitwidth if bitwidth is not None else cfg.get(k, 8)) for k in _BW_KEYS}
    return factory(pretrained=False, num_classes=cfg.get("num_classes", num_classes), drop_rate=cfg.get("drop_rate", 0.0),
                   drop_path_rate=cfg.get("drop_path_rate", 0.1), **bws, **ops)


def load_model(checkpoint_path, device="cuda", num_classes=1000, gelu_type=None, softmax_type=None, layernorm_type=None,
               bitwidth=None, calibration_batches: Optional[Iterable[torch.Tensor]] = None, strict_load=False,
               use_random_calibration_warmup=False, act_percentile=None):
    """inference.py:94-224: build from the saved configuration (arguments override it), load the weights, warm up the
    quantisation ranges unless `strict_load`, freeze.  `act_percentile`: the warm-up observes percentiles instead of min / max
    (set_act_percentile; an attribute of the modules, not a buffer, so no checkpoint holds it)."""
    checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    has_cfg = isinstance(checkpoint, dict) and "model_config" in checkpoint
    model = build_model(checkpoint["model_config"] if has_cfg else None, num_classes, gelu_type, softmax_type,
                        layernorm_type, bitwidth)
    weights = checkpoint["model"] if isinstance(checkpoint, dict) and "model" in checkpoint else checkpoint
    weights = dict(weights)
    own = model.state_dict()
    for name, param in weights.items():
        if name in own and param.shape == torch.Size([]) and own[name].shape == torch.Size([1]):
            weights[name] = param.unsqueeze(0)   # scalar buffers of older checkpoints (:203-207)
    model.load_state_dict(weights, strict=strict_load)
    model.to(device)
    if act_percentile is not None:
        set_act_percentile(model, act_percentile)
    if not strict_load:
        if use_random_calibration_warmup:
            calibrate_model(model, device, use_random_calibration=True)
        elif calibration_batches is not None:
            calibrate_model(model, device, calibration_batches)
    freeze_model(model)
    return model


def save_checkpoint(model, path, model_config: Optional[dict] = None, **extra):
    """The inference-relevant part of the dict quant_train.py:487-497 saves."""
    d = {"model": model.state_dict()}
    if model_config is not None:
        d["model_config"] = dict(model_config)
    d.update(extra)
    torch.save(d, path)


def _forward_transformed(model, transform, packed, lo, hi, device, graph=False):
    """logits of images [lo, hi) of a transforms.PackedImages batch: the device resize + crop, then the fused engine on the uint8
    crops (its input table set to the transform's Normalize) or, for any other model, the float32 tensor ToTensor + Normalize give
    (`graph`: through model.forward_graph)"""
    u8 = transform(packed, lo, hi, device=device)
    takes = getattr(model, "takes_engine", None)
    if takes is not None and takes(u8):
        eng = model.engine(u8.shape[0])
        norm = (transform.mean, transform.std)
        if getattr(eng, "input_lut", None) is None or getattr(eng, "input_norm", None) != norm:
            eng.set_input_normalisation(*norm)
        _, logits_f32, _ = eng(u8)
        return logits_f32.clone()
    return model.forward_graph(transform.to_float(u8)) if graph else model(transform.to_float(u8))


def _check_graph_status(model, graph):
    """after a graph=True loop: the checks the captured forwards made on the device, read once (graph.ModuleGraph.graph_status)"""
    if graph:
        model.graph_status()


def evaluate_dataset(model, data_loader, device, *, print_batch_stats: bool = True, transform=None, graph: bool = False):
    """inference.py:231-267 -> (top-1, top-3, top-5) accuracy in percent over (images, targets) batches.

    graph: batches go through `model.forward_graph` (graph.ModuleGraph: one captured graph per batch size, so a ragged last batch
    gets its own) instead of `model(imgs)`, and `model.graph_status()` is checked once after the loop.  With a `transform` the
    fused-engine branch is as without it; a model the engine declines replays its module path on the transform's float tensor.

    transform: None (the loader yields image tensors, as the reference's does), or a transforms.EvalTransform -- the loader then
    yields (transforms.PackedImages, targets) and the reference's Resize -> CenterCrop -> ToTensor -> Normalize runs on the device."""
    correct1 = correct3 = correct5 = tot = 0
    batch_times = []
    start_total = time.perf_counter()
    model.eval()
    with torch.no_grad():
        for imgs, targets in data_loader:
            t0 = time.perf_counter()
            if transform is None:
                imgs, targets = imgs.to(device), targets.to(device)
                logits = model.forward_graph(imgs) if graph else model(imgs)
            else:
                logits = _forward_transformed(model, transform, imgs, 0, imgs.size(0), device, graph)
                targets = targets.to(device)
            pred5 = logits.topk(5, dim=1).indices
            hit = pred5 == targets.reshape(-1, 1)
            correct1 += int(hit[:, 0].sum())
            correct3 += int(hit[:, :3].any(dim=1).sum())
            correct5 += int(hit.any(dim=1).sum())
            tot += imgs.size(0)
            batch_times.append(time.perf_counter() - t0)
    _check_graph_status(model, graph)
    total_time = time.perf_counter() - start_total
    if print_batch_stats and batch_times:
        print(f"Finished evaluation: total={total_time:.1f}s | avg/batch={sum(batch_times) / len(batch_times) * 1000:.1f} ms | "
              f"avg/img={(total_time / tot if tot else 0.0) * 1000:.2f} ms")
    if tot == 0:
        return 0.0, 0.0, 0.0
    return 100 * correct1 / tot, 100 * correct3 / tot, 100 * correct5 / tot


def _features_into(model, x, rows, integers, graph, norm=None):
    """features of the image batch x into `rows`, a [b, C] block of rows of a feature bank (int8 for integers, else float32) -> scale.
    The fused engine writes them there itself (forward_features(out=rows)); graph: its replay leaves the int8 embedding in the graph's
    buffer, and the one launch that follows (a dequantisation, or a copy of the integers) has the rows as its destination.  A model
    the engine declines runs module by module (model.features), with or without `graph`.  norm: the (mean, std) a uint8 x was
    meant for -- the engine's input table is set to it, as _forward_transformed does."""
    takes = getattr(model, "takes_engine_for_features", None)
    if takes is None or not takes(x):
        if x.dtype == torch.uint8:
            raise ValueError("uint8 images are what the fused engine takes: convert them (transforms.EvalTransform.to_float)")
        return model.features(x, integers, out=rows)[1]
    eng = model.engine(x.shape[0])
    if x.dtype == torch.uint8:
        if getattr(eng, "input_lut", None) is None or (norm is not None and getattr(eng, "input_norm", None) != norm):
            eng.set_input_normalisation(*(norm or ()))
    else:
        x = x.contiguous().float()
    if not graph:
        return eng.forward_features(x, integers, out=rows)[1]
    q, scale = eng.forward_features_graph(x, integers=True)
    if integers:
        rows.copy_(q)
    else:
        from .engine_common import dequant_rows
        b, C = q.shape
        dequant_rows(q, q.stride(0) if b > 1 else C, b, C, scale, rows, rows.stride(0) if b > 1 else C, eng._stream())
    return scale


def _sized(data_loader):
    """(loader, number of images): from the loader's dataset where it has one, else by holding its batches"""
    ds = getattr(data_loader, "dataset", None)
    if ds is not None and hasattr(ds, "__len__"):
        return data_loader, len(ds)
    batches = list(data_loader)
    return batches, sum(int(t.shape[0]) for _, t in batches)


def extract_features(model, data_loader, device, *, transform=None, graph: bool = False, integers: bool = False):
    """The embeddings of a dataset -> (features [N, C], labels int64 [N], scale), rows in loader order, on `device`: what linear
    probing, a retrieval bank or k-NN evaluation start from.  features: float32, model.features' tensor (integers times scale), or
    with integers=True the int8 integers; scale: the float32 act_scaling_factor they carry (None for an empty loader).

    The bank is allocated once (N: len(data_loader.dataset); a loader without a dataset is held as a list of its batches, and a
    loader that drops its last batch returns the rows it yielded) and every batch is written straight into its rows
    (forward_features(out=...)): no float copy per batch, no concatenation.  transform, graph: as for evaluate_dataset -- a
    transforms.EvalTransform makes the loader's (PackedImages, targets) batches uint8 crops on the device; graph=True replays the
    fused engine's feature graph (a model the engine declines has no feature graph and runs eagerly) and model.graph_status() is
    checked once after the loop."""
    data_loader, N = _sized(data_loader)
    C = int(model.num_features)
    bank = torch.empty(N, C, dtype=torch.int8 if integers else torch.float32, device=device)
    labels = torch.empty(N, dtype=torch.int64, device=device)
    n, scale = 0, None
    model.eval()
    with torch.no_grad():
        for imgs, targets in data_loader:
            b = int(targets.shape[0])
            if b == 0:
                continue
            rows = bank[n:n + b]
            if transform is None:
                scale = _features_into(model, imgs.to(device), rows, integers, graph)
            else:
                u8 = transform(imgs, 0, b, device=device)
                takes = getattr(model, "takes_engine_for_features", None)
                x = u8 if takes is not None and takes(u8) else transform.to_float(u8)
                scale = _features_into(model, x, rows, integers, graph, (transform.mean, transform.std))
            labels[n:n + b] = targets.to(device)
            n += b
    if graph and hasattr(model, "graph_status"):
        model.graph_status()
    return bank[:n], labels[:n], scale


def evaluate_knn(model, bank_loader, query_loader, device, *, k=(10, 20, 100, 200), T: float = 0.07, transform=None, graph: bool = False):
    """Weighted k-NN accuracy of a backbone -> {k: (top-1 %, top-5 %)}.  Both sets go through extract_features(..., integers=True);
    the bank stays int8 (knn.FeatureBank) and ONE search at max(k) serves every k: the neighbour order is total, so the neighbours
    for a smaller k are a prefix.  Per k the neighbours vote with w = exp(cos / T) (knn.knn_weights); top-5 counts a hit among the
    first min(5, k) voted classes.  The two extractions must carry the same scale (the same frozen model): anything else raises."""
    ks = tuple(sorted({int(v) for v in ((k,) if isinstance(k, int) else k)}))
    if not ks or ks[0] < 1:
        raise ValueError(f"evaluate_knn: k={k!r}")
    rows, labels, s_bank = extract_features(model, bank_loader, device, transform=transform, graph=graph, integers=True)
    q, targets, s_query = extract_features(model, query_loader, device, transform=transform, graph=graph, integers=True)
    if s_bank is None or s_query is None:
        raise ValueError("evaluate_knn: an empty bank or query set")
    fb, fq = float(torch.as_tensor(s_bank).reshape(-1)[0]), float(torch.as_tensor(s_query).reshape(-1)[0])
    if fb != fq:
        raise ValueError(f"evaluate_knn: the bank's rows carry scale {fb!r}, the queries' {fq!r}: not the same frozen model")
    if ks[-1] > int(rows.shape[0]):
        raise ValueError(f"evaluate_knn: k={ks[-1]} above the {int(rows.shape[0])} rows of the bank")
    bank = FeatureBank(rows, labels, s_bank)
    idx, cos = bank.search(q, ks[-1])
    w = knn_weights(cos, T)
    targets = targets.to(torch.int32)
    out, n = {}, max(int(q.shape[0]), 1)
    for kk in ks:
        classes, _ = bank.vote(idx[:, :kk], w[:, :kk], min(5, kk))
        hit = classes == targets[:, None]
        out[kk] = (100.0 * int(hit[:, 0].sum()) / n, 100.0 * int(hit.any(dim=1).sum()) / n)
    return out


def evaluate_linear_probe(model, bank_loader, query_loader, device, num_classes, *, lam=(1e-4, 1e-3, 1e-2, 1e-1, 1.0), kind: str = "ridge",
                          transform=None, graph: bool = False):
    """Linear-probe accuracy of a backbone -> {lam: (top-1 %, top-5 %)}.  Both sets go through extract_features(..., integers=True);
    the bank stays int8 and its statistics (probe.BankStats: exact Gram matrix, class sums and counts) are computed ONCE; per lam
    there is one C x C solve on the host (BankStats.ridge) and one int8 head GEMM with the top-5 selection over the queries
    (LinearProbe.topk).  kind="ncm": the class-mean classifier instead, a single entry under the key None.  The two extractions
    must carry the same scale (the same frozen model): anything else raises."""
    if kind not in ("ridge", "ncm"):
        raise ValueError(f"evaluate_linear_probe: kind={kind!r} is neither 'ridge' nor 'ncm'")
    lams = (None,) if kind == "ncm" else tuple(float(v) for v in ((lam,) if isinstance(lam, (int, float)) else lam))
    if not lams:
        raise ValueError(f"evaluate_linear_probe: lam={lam!r}")
    rows, labels, s_bank = extract_features(model, bank_loader, device, transform=transform, graph=graph, integers=True)
    q, targets, s_query = extract_features(model, query_loader, device, transform=transform, graph=graph, integers=True)
    if s_bank is None or s_query is None:
        raise ValueError("evaluate_linear_probe: an empty bank or query set")
    fb, fq = float(torch.as_tensor(s_bank).reshape(-1)[0]), float(torch.as_tensor(s_query).reshape(-1)[0])
    if fb != fq:
        raise ValueError(f"evaluate_linear_probe: the bank's rows carry scale {fb!r}, the queries' {fq!r}: not the same frozen model")
    stats = BankStats(int(rows.shape[1]), num_classes, rows.device).update(rows, labels, s_bank)
    targets = targets.to(torch.int32).contiguous()
    k = min(5, int(num_classes))
    out, n = {}, max(int(q.shape[0]), 1)
    for v in lams:
        probe = stats.ncm() if v is None else stats.ridge(v)
        hits = torch.zeros(k, dtype=torch.int64, device=q.device)
        probe.topk(q, k, targets, hits)
        h = hits.cpu()
        out[v] = (100.0 * int(h[0]) / n, 100.0 * int(h.sum()) / n)
    return out


def extract_features_parallel(model, data_loader, device, *, transform=None, graph: bool = False, integers: bool = False):
    """extract_features data-parallel over the ranks of the default process group (world 1 without one) -> the same (features [N, C],
    labels int64 [N], scale) on every rank, rows in loader order.

    Every rank iterates the SAME loader and keeps its parallel.shard_bounds slice of each global batch, as
    evaluate_dataset_parallel does; it collects the int8 integers of its slices with their labels, and ONE
    parallel.gather_feature_rows at the end (one all_gather_into_tensor: uneven shards padded to the largest and trimmed by their
    counts) brings every rank's rows to every rank, where they are put back into loader order.  integers=False: the gathered
    integers are dequantised once, behind the gather (a quarter of the float32 bytes cross the wire)."""
    from .parallel import gather_feature_rows
    if dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(), dist.get_rank()
    else:
        world, rank = 1, 0
    data_loader, N = _sized(data_loader)
    C = int(model.num_features)
    # this rank's rows: its slice of a batch is at most one image more than an even share
    cap = N // world + len(data_loader) if hasattr(data_loader, "__len__") else N
    local = torch.empty(min(N, cap), C, dtype=torch.int8, device=device)
    local_labels = torch.empty(local.shape[0], dtype=torch.int64, device=device)
    sizes, n, scale = [], 0, None
    model.eval()
    with torch.no_grad():
        for imgs, targets in data_loader:
            B = int(targets.shape[0])
            sizes.append(B)
            lo, hi = shard_bounds(B, world, rank)
            if hi == lo:
                continue
            rows = local[n:n + hi - lo]
            if transform is None:
                scale = _features_into(model, imgs[lo:hi].to(device), rows, True, graph)
            else:
                u8 = transform(imgs, lo, hi, device=device)
                takes = getattr(model, "takes_engine_for_features", None)
                x = u8 if takes is not None and takes(u8) else transform.to_float(u8)
                scale = _features_into(model, x, rows, True, graph, (transform.mean, transform.std))
            local_labels[n:n + hi - lo] = targets[lo:hi].to(device)
            n += hi - lo
    if graph and hasattr(model, "graph_status"):
        model.graph_status()
    q, labels, scale = gather_feature_rows(local[:n], local_labels[:n], scale, sizes, world)
    if integers:
        return q, labels, scale
    if scale is None:
        return q.float(), labels, scale
    if q.is_cuda:
        from . import _lib
        from .engine_common import dequant_rows
        f = torch.empty(q.shape, dtype=torch.float32, device=q.device)
        if q.shape[0]:
            dequant_rows(q, C, q.shape[0], C, scale, f, C, _lib.stream_ptr())
        return f, labels, scale
    return q.float() * torch.tensor(scale, dtype=torch.float32), labels, scale      # (a CPU group: torch's own float32 product)


def evaluate_dataset_parallel(model, data_loader, device, *, scorer=None, print_batch_stats: bool = True, transform=None,
                              graph: bool = False):
    """evaluate_dataset data-parallel over the ranks of the default process group (world 1 without one) -> the same
    (top-1, top-3, top-5) percentages on every rank.

    Every rank iterates the SAME loader and keeps its parallel.shard_bounds slice of each global batch (images and
    targets): the slices partition the batch exactly -- no sampler padding, so no image is counted twice.  The rank
    forwards its slice (an empty slice skips the forward) and the scorer adds that slice's rank-r hits into an int64 [5]
    device tensor, with no host synchronisation per batch; ONE parallel.allreduce_hits at the end sums hits and image
    counts over the ranks.

    scorer(logits, targets int32 [b], hits int64 [5], k=5): default topk.count_hits, the HIP selection over the float
    logits (value descending, equal logits by ascending class -- where evaluate_dataset's torch.topk leaves the order of
    tied logits unspecified).

    transform: as for evaluate_dataset; a rank transforms only its shard_bounds slice of each packed batch.
    graph: as for evaluate_dataset, on the rank's slice (the scorer reads the graph's output buffer before the next replay)."""
    if dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(), dist.get_rank()
    else:
        world, rank = 1, 0
    scorer = topk.count_hits if scorer is None else scorer
    hits = torch.zeros(5, dtype=torch.int64, device=device)
    local = 0
    start_total = time.perf_counter()
    model.eval()
    with torch.no_grad():
        for imgs, targets in data_loader:
            lo, hi = shard_bounds(imgs.size(0), world, rank)
            if hi == lo:
                continue
            if transform is None:
                x = imgs[lo:hi].to(device)
                t = targets[lo:hi].to(device=device, dtype=torch.int32)
                scorer(model.forward_graph(x) if graph else model(x), t, hits, 5)
            else:
                t = targets[lo:hi].to(device=device, dtype=torch.int32)
                scorer(_forward_transformed(model, transform, imgs, lo, hi, device, graph), t, hits, 5)
            local += hi - lo
    _check_graph_status(model, graph)
    hits, tot = allreduce_hits(hits, local)
    total_time = time.perf_counter() - start_total
    if print_batch_stats and rank == 0 and tot:
        print(f"Finished evaluation ({world} rank{'s' if world > 1 else ''}): total={total_time:.1f}s | "
              f"avg/img={total_time / tot * 1000:.2f} ms")
    if tot == 0:
        return 0.0, 0.0, 0.0
    h = hits.tolist()
    correct1, correct3, correct5 = h[0], sum(h[:3]), sum(h)
    return 100 * correct1 / tot, 100 * correct3 / tot, 100 * correct5 / tot
