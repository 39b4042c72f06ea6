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

import numpy as np
import torch
import torch.distributed as dist

from . import swin_quant, topk, vit_quant
from .knn import C_NARROW_MAX, FeatureBank, knn_weights, retrieval_ap
from .model_utils import freeze_model
from .parallel import allreduce_hits, shard_bounds
from .probe import CLASSES_MAX, BankStats, fit_logistic

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


def pooled_width(model, n_last: int = 1, avgpool: bool = False, wide: bool = False):
    """Width W = n_last * C (+ C with avgpool) of model.features_pooled's rows, checked against what the feature-bank kernels take
    (knn.FeatureBank, probe.BankStats: W % 64 == 0 in 64..1024; with wide=True in 64..4096, the range of the wide kernels -- the
    protocol's ViT-S n_last=4, ViT-B + avgpool and ViT-L + avgpool): ValueError otherwise, before anything is extracted"""
    C = int(model.num_features)
    W = int(n_last) * C + (C if avgpool else 0)
    if int(n_last) < 1 or W % 64 or not 64 <= W <= (4096 if wide else 1024):
        raise ValueError(f"pooled features of width W={W} (n_last={n_last}, avgpool={bool(avgpool)}, C={C}): the feature-bank kernels "
                         + ("take rows of W % 64 == 0 channels, W in 64..4096" if wide else
                            "take rows of W % 64 == 0 channels, W in 64..1024 (to 4096: pass wide=True)"))
    return W


def _pooled_into(model, x, rows, n_last, avgpool, norm=None):
    """model.features_pooled of the image batch x into `rows`, a [b, W] int8 block of rows of a feature bank -> scale (a float: every
    segment carries qact2's).  uint8 x and norm: as _features_into; a model the fused engine declines raises (no module path)."""
    takes = getattr(model, "takes_engine_for_features", None)
    if takes is not None and takes(x) and x.dtype == torch.uint8:
        eng = model.engine(x.shape[0])
        if getattr(eng, "input_lut", None) is None or (norm is not None and getattr(eng, "input_norm", None) != norm):
            eng.set_input_normalisation(*(norm or ()))
        return eng.forward_features_pooled(x, n_last, avgpool, out=rows)[1][0].item()
    return model.features_pooled(x, n_last, avgpool, out=rows)[1][0].item()


def _sized(data_loader):
    """(loader, number of images): from the loader's dataset where it has one, else by holding its batches"""
    ds = getattr(data_loader, "dataset", None)
    if ds is not None and hasattr(ds, "__len__"):
        return data_loader, len(ds)
    batches = list(data_loader)
    return batches, sum(int(t.shape[0]) for _, t in batches)


def extract_features(model, data_loader, device, *, transform=None, graph: bool = False, integers: bool = False, n_last: int = 1,
                     avgpool: bool = False, wide: bool = False):
    """The embeddings of a dataset -> (features [N, C], labels int64 [N], scale), rows in loader order, on `device`: what linear
    probing, a retrieval bank or k-NN evaluation start from.  features: float32, model.features' tensor (integers times scale), or
    with integers=True the int8 integers; scale: the float32 act_scaling_factor they carry (None for an empty loader).

    The bank is allocated once (N: len(data_loader.dataset); a loader without a dataset is held as a list of its batches, and a
    loader that drops its last batch returns the rows it yielded) and every batch is written straight into its rows
    (forward_features(out=...)): no float copy per batch, no concatenation.  transform, graph: as for evaluate_dataset -- a
    transforms.EvalTransform makes the loader's (PackedImages, targets) batches uint8 crops on the device; graph=True replays the
    fused engine's feature graph (a model the engine declines has no feature graph and runs eagerly) and model.graph_status() is
    checked once after the loop.
    n_last, avgpool: anything but the defaults extracts model.features_pooled(x, n_last, avgpool) instead -- the class tokens of the
    last n_last blocks and, with avgpool, the mean patch token, W = n_last * C (+ C) columns (pooled_width: ValueError, before the
    loader is touched, for a W the feature-bank kernels do not take; wide=True admits W up to 4096) -- on the fused engine, eagerly
    (graph=True: ValueError)."""
    pooled = int(n_last) != 1 or bool(avgpool)
    C = pooled_width(model, n_last, avgpool, wide) if pooled else int(model.num_features)
    if pooled and graph:
        raise ValueError("extract_features: features_pooled is not part of the graph replays (graph=False)")
    data_loader, N = _sized(data_loader)
    bank = torch.empty(N, C, dtype=torch.int8 if integers or pooled else torch.float32, device=device)
    labels = torch.empty(N, dtype=torch.int64, device=device)
    n, scale = 0, None
    model.eval()
    with torch.no_grad():
        for imgs, targets in data_loader:
            b = int(targets.shape[0])
            if b == 0:
                continue
            rows = bank[n:n + b]
            if pooled and transform is None:
                scale = _pooled_into(model, imgs.to(device), rows, n_last, avgpool)
            elif pooled:
                u8 = transform(imgs, 0, b, device=device)
                takes = getattr(model, "takes_engine_for_features", None)
                x = u8 if takes is not None and takes(u8) else transform.to_float(u8)
                scale = _pooled_into(model, x, rows, n_last, avgpool, (transform.mean, transform.std))
            elif transform is None:
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
    if pooled and not integers and scale is not None:
        bank = bank.float() * torch.tensor(scale, dtype=torch.float32)      # the integers times scale, one float32 product
    return bank[:n], labels[:n], scale


def evaluate_knn(model, bank_loader, query_loader, device, *, k=(10, 20, 100, 200), T: float = 0.07, transform=None, graph: bool = False,
                 n_last: int = 1, avgpool: bool = False, wide: bool = False):
    """Weighted k-NN accuracy of a backbone -> {k: (top-1 %, top-5 %)}.  Both sets go through extract_features(..., integers=True);
    the bank stays int8 (knn.FeatureBank) and ONE search at max(k) serves every k: the neighbour order is total, so the neighbours
    for a smaller k are a prefix.  Per k the neighbours vote with w = exp(cos / T) (knn.knn_weights); top-5 counts a hit among the
    first min(5, k) voted classes.  The two extractions must carry the same scale (the same frozen model): anything else raises.
    n_last, avgpool, wide: the pooled feature of extract_features for both sets (wide=True: rows of up to 4096 channels, searched
    by the kernel that splits the channels over the waves)."""
    ks = tuple(sorted({int(v) for v in ((k,) if isinstance(k, int) else k)}))
    if not ks or ks[0] < 1:
        raise ValueError(f"evaluate_knn: k={k!r}")
    pooled = {} if int(n_last) == 1 and not avgpool else dict(n_last=n_last, avgpool=avgpool)      # (the defaults: the call as it always was)
    if pooled and wide:
        pooled["wide"] = True
    rows, labels, s_bank = extract_features(model, bank_loader, device, transform=transform, graph=graph, integers=True, **pooled)
    q, targets, s_query = extract_features(model, query_loader, device, transform=transform, graph=graph, integers=True, **pooled)
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


def evaluate_retrieval(model, db_loader, query_loader, device, positives, junk=None, **feature_kw):
    """Image retrieval scored the revisited-Oxford way -> {"mAP": %, "mP@1": %, "mP@5": %, "mP@10": %}.  positives / junk: per query
    (in loader order) the database rows (in loader order) that are its positives and the ones to take out of its ranking.  Both
    sets go through extract_features(..., integers=True, **feature_kw) -- transform, graph, n_last, avgpool -- the database stays
    int8 (knn.FeatureBank) and ONE counting pass over it (FeatureBank.ranks) gives the exact rank of every listed row in the
    search's order; knn.retrieval_ap turns the ranks into average precision on the host.  Queries without a positive are left out of
    the means.  The rank kernel takes rows of at most 1024 channels: a wider feature is refused before a loader is touched, and so
    is a query scale that is not the database's."""
    if feature_kw.get("wide"):
        raise ValueError(f"evaluate_retrieval: wide=True: the rank kernel takes rows of at most {C_NARROW_MAX} channels")
    pooled = int(feature_kw.get("n_last", 1)) != 1 or bool(feature_kw.get("avgpool", False))
    W = pooled_width(model, feature_kw.get("n_last", 1), feature_kw.get("avgpool", False)) if pooled else int(model.num_features)
    if W > C_NARROW_MAX:
        raise ValueError(f"evaluate_retrieval: features of {W} channels: the rank kernel takes rows of at most {C_NARROW_MAX}")
    rows, labels, s_db = extract_features(model, db_loader, device, integers=True, **feature_kw)
    q, _, s_query = extract_features(model, query_loader, device, integers=True, **feature_kw)
    if s_db is None or s_query is None:
        raise ValueError("evaluate_retrieval: an empty database or query set")
    fb, fq = float(torch.as_tensor(s_db).reshape(-1)[0]), float(torch.as_tensor(s_query).reshape(-1)[0])
    if fb != fq:
        raise ValueError(f"evaluate_retrieval: the database's rows carry scale {fb!r}, the queries' {fq!r}: not the same frozen model")
    Q = int(q.shape[0])
    junk = [()] * Q if junk is None else junk
    if len(positives) != Q or len(junk) != Q:
        raise ValueError(f"evaluate_retrieval: {len(positives)} positive and {len(junk)} junk lists for {Q} queries")
    flat = [[int(v) for v in torch.as_tensor(t).reshape(-1)] for pair in zip(positives, junk) for t in pair]
    targets = [flat[2 * i] + flat[2 * i + 1] for i in range(Q)]
    is_pos = [flag for i in range(Q) for flag in [True] * len(flat[2 * i]) + [False] * len(flat[2 * i + 1])]
    ranks, _, tptr = FeatureBank(rows, labels, s_db).ranks(q, targets)
    ap, prec = retrieval_ap(ranks, tptr, is_pos)
    ok = ~np.isnan(ap)
    if not ok.any():
        raise ValueError("evaluate_retrieval: no query has a positive")
    out = {"mAP": 100.0 * float(ap[ok].mean())}
    out.update({f"mP@{k}": 100.0 * float(prec[ok, c].mean()) for c, k in enumerate((1, 5, 10))})
    return out


def evaluate_linear_probe(model, bank_loader, query_loader, device, num_classes, *, lam=(1e-4, 1e-3, 1e-2, 1e-1, 1.0), kind: str = "ridge",
                          transform=None, graph: bool = False, n_last: int = 1, avgpool: bool = False, wide: bool = False):
    """Linear-probe accuracy of a backbone -> {lam: (top-1 %, top-5 %)}.  Both sets go through extract_features(..., integers=True);
    the bank stays int8 and its statistics (probe.BankStats: exact Gram matrix, class sums and counts) are computed ONCE; per lam
    there is one C x C solve on the host (BankStats.ridge) and one int8 head GEMM with the top-5 selection over the queries
    (LinearProbe.topk).  kind="ncm": the class-mean classifier instead, a single entry under the key None.  The two extractions
    must carry the same scale (the same frozen model): anything else raises.  n_last, avgpool, wide: the pooled feature of
    extract_features for both sets (wide=True: rows of up to 4096 channels)."""
    if kind not in ("ridge", "ncm"):
        raise ValueError(f"evaluate_linear_probe: kind={kind!r} is neither 'ridge' nor 'ncm'")
    lams = (None,) if kind == "ncm" else tuple(float(v) for v in ((lam,) if isinstance(lam, (int, float)) else lam))
    if not lams:
        raise ValueError(f"evaluate_linear_probe: lam={lam!r}")
    pooled = {} if int(n_last) == 1 and not avgpool else dict(n_last=n_last, avgpool=avgpool)      # (the defaults: the call as it always was)
    if pooled and wide:
        pooled["wide"] = True
    rows, labels, s_bank = extract_features(model, bank_loader, device, transform=transform, graph=graph, integers=True, **pooled)
    q, targets, s_query = extract_features(model, query_loader, device, transform=transform, graph=graph, integers=True, **pooled)
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


def evaluate_logistic_probe(model, bank_loader, query_loader, device, num_classes, *, lrs=(1e-3, 1e-2, 1e-1), epochs: int = 10,
                            batch_size: int = 1024, momentum: float = 0.9, weight_decay: float = 0.0, seed: int = 0, transform=None,
                            graph: bool = False, n_last: int = 1, avgpool: bool = False, wide: bool = False):
    """Logistic linear-probe accuracy of a backbone -> {lr: (top-1 %, top-5 %)}: the protocol's softmax classifier trained with
    minibatch SGD on the frozen features.  Both sets are extracted ONCE (extract_features(..., integers=True)); the bank stays int8
    and per learning rate there is one probe.fit_logistic on it in place (cosine schedule, `epochs` passes) and one int8 head GEMM
    with the top-5 selection over the queries (LinearProbe.topk).  The width of the rows (a multiple of 64 up to 4096) and
    num_classes (up to 1024) are checked before a loader is touched.  n_last, avgpool, wide: as for evaluate_linear_probe."""
    rates = tuple(float(v) for v in ((lrs,) if isinstance(lrs, (int, float)) else lrs))
    if not rates:
        raise ValueError(f"evaluate_logistic_probe: lrs={lrs!r}")
    pooled = {} if int(n_last) == 1 and not avgpool else dict(n_last=n_last, avgpool=avgpool)
    if pooled and wide:
        pooled["wide"] = True
    C = pooled_width(model, n_last, avgpool, wide) if pooled else int(model.num_features)
    if C % 64 != 0 or not 64 <= C <= 4096:
        raise ValueError(f"evaluate_logistic_probe: features of C={C} channels: the logistic probe takes multiples of 64 from 64 to 4096")
    if not 1 <= int(num_classes) <= CLASSES_MAX:
        raise ValueError(f"evaluate_logistic_probe: num_classes={num_classes} outside [1, {CLASSES_MAX}]")
    rows, labels, s_bank = extract_features(model, bank_loader, device, transform=transform, graph=graph, integers=True, **pooled)
    q, targets, s_query = extract_features(model, query_loader, device, transform=transform, graph=graph, integers=True, **pooled)
    if s_bank is None or s_query is None:
        raise ValueError("evaluate_logistic_probe: an empty bank or query set")
    fb, fq = float(torch.as_tensor(s_bank).reshape(-1)[0]), float(torch.as_tensor(s_query).reshape(-1)[0])
    if fb != fq:
        raise ValueError(f"evaluate_logistic_probe: the bank's rows carry scale {fb!r}, the queries' {fq!r}: not the same frozen model")
    targets = targets.to(torch.int32).contiguous()
    k = min(5, int(num_classes))
    out, n = {}, max(int(q.shape[0]), 1)
    for v in rates:
        probe = fit_logistic(rows, labels, fb, num_classes, epochs=epochs, batch_size=batch_size, lr=v, momentum=momentum,
                             weight_decay=weight_decay, seed=seed)
        hits = torch.zeros(k, dtype=torch.int64, device=q.device)
        probe.topk(q, k, targets, hits)
        h = hits.cpu()
        out[v] = (100.0 * int(h[0]) / n, 100.0 * int(h.sum()) / n)
    return out


def _patch_tokens(model, x):
    """-> (int8 tokens [b, Gh * Gw, C], scale, (Gh, Gw), r): forward_tokens(x, integers=True) as the model returns it -- a ViT's
    ({block: tokens}, prefixes, scale), a Swin's (tokens, scale) -- and the geometry of its token grid: r = the pixels per token on
    an axis (the patch size, times 2 per Swin patch merging)"""
    out = model.forward_tokens(x, integers=True)
    tok, scale = out[0], out[-1]
    if isinstance(tok, dict):
        tok = tok[max(tok)]
    ph, pw = model.patch_embed.patch_size
    r = int(ph) * 2 ** (int(getattr(model, "num_layers", 1)) - 1)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    if ph != pw or H % r or W % r or tok.dim() != 3 or int(tok.shape[1]) != (H // r) * (W // r):
        raise ValueError(f"evaluate_dense_probe: {tuple(tok.shape)} tokens for images of {H} x {W} and {r} pixels per token")
    return tok, scale, (H // r, W // r), r


def evaluate_dense_probe(model, train_loader, val_loader, device, num_classes, *, lam=(1e-4, 1e-3, 1e-2, 1e-1, 1.0), ignore_index: int = 255,
                         transform=None):
    """Linear segmentation probe of a frozen backbone -> {lam: (mIoU %, pixel accuracy %)}.  The loaders yield (images, uint8 target
    maps [B, H, W]).  Training side: the int8 patch tokens of model.forward_tokens(x, integers=True) are the rows, dense.patch_labels
    of the target maps their labels (patches labelled ignore_index are dropped), and probe.BankStats sums them batch by batch; the
    statistics are computed ONCE.  Per lam there is one C x C solve on the host and one pass over the validation tokens (kept int8
    on the device): dense.DenseProbe.segment adds every batch's pixels into one int64 confusion matrix -- the upsampled logits
    never exist -- and dense.miou reads it.  transform: as for extract_features, on the images alone (the targets must already
    have the transformed geometry).  All tokens must carry the same scale (the same frozen model): anything else raises."""
    from .dense import DenseProbe, miou, patch_labels
    lams = tuple(float(v) for v in ((lam,) if isinstance(lam, (int, float)) else lam))
    if not lams:
        raise ValueError(f"evaluate_dense_probe: lam={lam!r}")
    K = int(num_classes)

    def batches(loader):
        for imgs, targets in loader:
            b = int(targets.shape[0])
            if b == 0:
                continue
            x = imgs.to(device) if transform is None else transform.to_float(transform(imgs, 0, b, device=device))
            tok, scale, grid, r = _patch_tokens(model, x)
            yield tok, float(torch.as_tensor(scale).reshape(-1)[0]), grid, r, targets.to(device=device, dtype=torch.uint8).contiguous()

    stats, s_train = None, None
    model.eval()
    with torch.no_grad():
        for tok, s, grid, r, tgt in batches(train_loader):
            rows = tok.reshape(-1, tok.shape[-1])
            lab = patch_labels(tgt, r, K, ignore_index).reshape(-1)
            keep = lab != ignore_index
            if stats is None:
                stats, s_train = BankStats(int(rows.shape[1]), K, rows.device), s
            stats.update(rows[keep].contiguous(), lab[keep], s)
        val = [(tok.contiguous(), s, grid, r, tgt) for tok, s, grid, r, tgt in batches(val_loader)]
    if stats is None or not val:
        raise ValueError("evaluate_dense_probe: an empty training or validation set")
    for _, s, _, _, _ in val:
        if s != s_train:
            raise ValueError(f"evaluate_dense_probe: the training tokens carry scale {s_train!r}, the validation tokens {s!r}: not the same frozen model")
    out = {}
    for v in lams:
        dp = DenseProbe(stats.ridge(v))
        conf = torch.zeros(K, K, dtype=torch.int64, device=device)
        for tok, _, grid, r, tgt in val:
            dp.segment(tok, grid, r, target=tgt, conf=conf, labels=False, ignore_index=ignore_index)
        m, pa, _ = miou(conf)
        out[v] = (100.0 * m, 100.0 * pa)
    return out


def _propagated_sequences(who, model, sequences, device, n_last, radius, k, T, transform, batch):
    """The protocol loop evaluate_video_segmentation and evaluate_davis share.  Checks the model and the knobs before a sequence is
    touched, then yields per sequence (L, K, (Gh, Gw), r, masks, segs): segs yields (t, seg) for t = 1 .. L - 1, the frame's float32
    [Gh * Gw, K] soft labels from TokenMemory.propagate, already put into the ring of previous frames."""
    from .dense import patch_labels
    from .propagate import C_MAX, CLASSES_MAX, K_MAX, TokenMemory
    if not hasattr(model, "forward_tokens"):
        raise ValueError(f"{who}: {type(model).__name__} has no forward_tokens")
    Cm, n_last, batch = int(model.num_features), int(n_last), int(batch)
    if Cm % 64 != 0 or not 64 <= Cm <= C_MAX:
        raise ValueError(f"{who}: tokens of C={Cm} channels: the windowed search takes C % 64 == 0 in 64..{C_MAX} (there is no float path)")
    if n_last < 0 or batch < 1 or not 1 <= int(k) <= K_MAX or int(radius) < 0:
        raise ValueError(f"{who}: n_last={n_last} (at least 0), batch={batch} (at least 1), k={k} (1 .. {K_MAX}), radius={radius} (at least 0)")

    def frames_of(mem, toks, L):
        for t in range(1, L):
            used = 1 + min(t - 1, n_last)
            q = toks[t // batch][t % batch]
            seg = mem.propagate(q, radius, k, T, frames=used)
            if n_last:
                mem.put(1 + (t - 1) % n_last, q, seg)
            yield t, seg

    model.eval()
    for frames, first_mask, masks, num_objects in sequences:
        L, K = int(frames.shape[0]), int(num_objects) + 1
        if L < 2 or not 2 <= K <= CLASSES_MAX:
            raise ValueError(f"{who}: a sequence of {L} frames with {num_objects} objects (at least 2 frames, 1 .. {CLASSES_MAX - 1} objects)")
        toks, grid, r = [], None, None
        for lo in range(0, L, batch):
            hi = min(lo + batch, L)
            x = frames[lo:hi].to(device) if transform is None else transform.to_float(transform(frames, lo, hi, device=device))
            tok, _, grid, r = _patch_tokens(model, x)
            toks.append(tok)
        Gh, Gw = grid
        mem = TokenMemory(Gh, Gw, Cm, K, 1 + min(n_last, L - 1), device)
        lab0 = patch_labels(first_mask.to(device=device, dtype=torch.uint8).reshape(1, Gh * r, Gw * r).contiguous(), r, K, 255)
        seg0 = torch.nn.functional.one_hot(lab0.reshape(-1).long().clamp(max=K), K + 1)[:, :K].float()      # an ignored patch: no label at all
        mem.put(0, toks[0][0], seg0)
        yield L, K, (Gh, Gw), r, masks, frames_of(mem, toks, L)


def evaluate_video_segmentation(model, sequences, device, *, n_last: int = 7, radius: int = 12, k: int = 5, T: float = 0.1, transform=None,
                                batch: int = 8):
    """Semi-supervised video object segmentation by label propagation (the DAVIS protocol of the DINO evaluation) ->
    {"J_mean": %, "per_sequence": [%, ...]}: the region similarity J, the mean over a sequence's objects and frames (the first
    frame, whose mask is given, left out) of the intersection over union of the predicted and the true object mask; a pair whose
    union is empty counts 1.  sequences yields (frames uint8 / float [L, 3, H, W], first_mask uint8 [H, W], masks uint8 [L, H, W],
    num_objects): label 0 is the background, 1 .. num_objects the objects.
    Per sequence the frames go through forward_tokens(integers=True) in batches of `batch`, once; the first frame's patch labels
    (dense.patch_labels of first_mask) go one-hot into slot 0 of a propagate.TokenMemory, slots 1 .. n_last are a ring of the previous
    frames with their PROPAGATED soft labels, and every further frame is one TokenMemory.propagate call against the filled slots:
    the tokens stay int8, no affinity matrix exists.  The frame's [K, Gh, Gw] soft labels are upsampled bilinearly by the pixels per
    token and the argmax is its prediction: K <= 256 planes of one frame in torch, off the hot path (evaluate_davis keeps that tail
    on the device and adds the boundary measure F).  transform: as for evaluate_dense_probe, on the frames alone.  Works for ViT and
    Swin backbones (a Swin's last-stage grid).  A model whose tokens the kernels do not take is refused before a sequence is touched."""
    per_seq = []
    with torch.no_grad():
        for L, K, (Gh, Gw), r, masks, segs in _propagated_sequences("evaluate_video_segmentation", model, sequences, device, n_last, radius, k, T,
                                                                    transform, batch):
            truth = masks.to(device)
            inter = torch.zeros(K - 1, dtype=torch.float64, device=device)
            for t, seg in segs:
                up = torch.nn.functional.interpolate(seg.t().reshape(1, K, Gh, Gw), scale_factor=r, mode="bilinear", align_corners=False)
                pred = up[0].argmax(dim=0)
                for o in range(1, K):
                    p, g = pred == o, truth[t] == o
                    u = int((p | g).sum())
                    inter[o - 1] += 1.0 if u == 0 else int((p & g).sum()) / u
            per_seq.append(100.0 * float(inter.sum()) / ((L - 1) * (K - 1)))
    if not per_seq:
        raise ValueError("evaluate_video_segmentation: no sequence")
    return {"J_mean": sum(per_seq) / len(per_seq), "per_sequence": per_seq}


def evaluate_davis(model, sequences, device, *, n_last: int = 7, radius: int = 12, k: int = 5, T: float = 0.1, bound_th: float = 0.008,
                   transform=None, batch: int = 8, return_masks: bool = False):
    """evaluate_video_segmentation's protocol with the scoring on the device -> {"J_mean": %, "F_mean": %, "JF_mean": %,
    "per_sequence": [(J %, F %), ...]} (and "masks": [uint8 [L, H, W], ...] with return_masks; frame 0 is the given mask): the region
    similarity J and the boundary measure F of davis2017-evaluation (no void pixels; tolerance propagate.bound_radius(bound_th, H, W)
    pixels, at most 24), each the mean over a sequence's objects and frames 1 .. L - 1, then over the sequences; JF_mean is the mean of
    the two.  Every frame's label map is written by propagate.upsample_argmax (the exact float64 bilinear upsample + argmax of
    csrc/davis.hip) into one [L, H, W] buffer, and the sequence is scored by ONE propagate.mask_scores launch and ONE readback.  J may
    differ from evaluate_video_segmentation's at pixels where torch's float32 interpolation and the exact one break a near-tie between
    two classes differently."""
    from .propagate import davis_measures, mask_scores, upsample_argmax
    per_seq, kept = [], []
    with torch.no_grad():
        for L, K, grid, r, masks, segs in _propagated_sequences("evaluate_davis", model, sequences, device, n_last, radius, k, T, transform, batch):
            truth = masks.to(device=device, dtype=torch.uint8).contiguous()
            pred = torch.empty_like(truth)
            pred[0] = truth[0]
            for t, seg in segs:
                upsample_argmax(seg, grid, r, out=pred[t])
            J, F = davis_measures(mask_scores(pred[1:], truth[1:], K - 1, bound_th))
            per_seq.append(tuple(100.0 * sum(m.reshape(-1).tolist()) / ((L - 1) * (K - 1)) for m in (J, F)))
            if return_masks:
                kept.append(pred)
    if not per_seq:
        raise ValueError("evaluate_davis: no sequence")
    Jm, Fm = (sum(p[i] for p in per_seq) / len(per_seq) for i in (0, 1))
    out = {"J_mean": Jm, "F_mean": Fm, "JF_mean": (Jm + Fm) / 2, "per_sequence": per_seq}
    if return_masks:
        out["masks"] = kept
    return out


def evaluate_object_discovery(model, loader, device, k: int = 100):
    """Unsupervised single-object discovery (LOST's seed expansion) scored by CorLoc -> {"CorLoc": %, "per_image": [(hit, IoU), ...]}:
    the share of images whose discovered box has an intersection over union of at least 0.5 with one of the image's ground-truth
    boxes.  loader yields (images [B, 3, H, W], a list of B ground-truth box lists, (x0, y0, x1, y1) in pixels).  The int8 patch tokens
    of model.forward_tokens(x, integers=True) (a ViT's last block, a Swin's last stage) go through discover.discover_objects: two
    launches and ONE readback (the boxes) per batch; the IoU is float64 on the host (discover.corloc).  A model without the engine
    path is refused with features_unsupported_reason()'s text before the loader is touched."""
    from .discover import K_MAX, boxes_to_pixels, corloc, discover_objects
    who = "evaluate_object_discovery"
    if not hasattr(model, "forward_tokens") or not hasattr(model, "features_unsupported_reason"):
        raise ValueError(f"{who}: {type(model).__name__} has no forward_tokens")
    reason = model.features_unsupported_reason()
    if reason is not None:
        raise ValueError(f"{who}: the tokens come from the fused engine, which does not take this model: {reason}")
    if not 1 <= int(k) <= K_MAX:
        raise ValueError(f"{who}: k={k} outside [1, {K_MAX}]")
    per_image = []
    model.eval()
    with torch.no_grad():
        for imgs, gts in loader:
            if int(imgs.shape[0]) == 0:
                continue
            tok, _, grid, r = _patch_tokens(model, imgs.to(device))
            if tok.stride(2) != 1 or tok.stride(1) % 16 or tok.stride(0) % 16 or tok.data_ptr() % 16:
                tok = tok.contiguous()
            boxes = discover_objects(tok, grid, k)[0]
            hits, iou = corloc(boxes_to_pixels(boxes, r), gts)
            per_image += list(zip(hits.tolist(), iou.tolist()))
    if not per_image:
        raise ValueError(f"{who}: no image")
    return {"CorLoc": 100.0 * sum(h for h, _ in per_image) / len(per_image), "per_image": per_image}


def evaluate_clustering(model, loader, device, num_clusters, iters: int = 20, seed: int = 0, n_last: int = 1, avgpool: bool = False,
                        wide: bool = False):
    """Unsupervised classification of a backbone's features -> {"NMI", "ARI", "purity", "inertia", "iterations"}: ONE
    extract_features(..., integers=True), ONE cluster.KMeans.fit on the int8 bank in place (integer Lloyd iterations on the int8
    MFMA, csrc/kmeans.hip; the initial centroids are the first num_clusters rows of a CPU randperm seeded with `seed`) and
    cluster.partition_scores of its labels against the loader's targets, float64 on the host.  n_last, avgpool: the pooled feature
    of extract_features.  The width (a multiple of 64 from 64 to 1024) and num_clusters are checked before the loader is touched;
    wide=True is refused: there is no wide assignment kernel.  Patch tokens cluster the same way without this function:
    forward_tokens(x, integers=True) tokens go into KMeans.fit directly after a reshape to [B * hw, C]."""
    from .cluster import K_MAX, KMeans, partition_scores
    who = "evaluate_clustering"
    if wide:
        raise ValueError(f"{who}: wide=True: there is no wide assignment kernel (rows of at most {C_NARROW_MAX} channels)")
    pooled = {} if int(n_last) == 1 and not avgpool else dict(n_last=n_last, avgpool=avgpool)
    C = pooled_width(model, n_last, avgpool) if pooled else int(model.num_features)
    if C % 64 != 0 or not 64 <= C <= C_NARROW_MAX:
        raise ValueError(f"{who}: features of C={C} channels: the assignment kernel takes multiples of 64 from 64 to {C_NARROW_MAX}")
    if not 1 <= int(num_clusters) <= K_MAX:
        raise ValueError(f"{who}: num_clusters={num_clusters} outside [1, {K_MAX}]")
    rows, targets, _ = extract_features(model, loader, device, integers=True, **pooled)
    km = KMeans(C, num_clusters, rows.device)
    labels = km.fit(rows, iters=iters, seed=seed)
    out = partition_scores(labels, targets)
    out.update(inertia=km.inertia, iterations=len(km.history))
    return out


def extract_features_parallel(model, data_loader, device, *, transform=None, graph: bool = False, integers: bool = False,
                              n_last: int = 1, avgpool: bool = False, wide: bool = False):
    """extract_features data-parallel over the ranks of the default process group (world 1 without one) -> the same (features [N, C],
    labels int64 [N], scale) on every rank, rows in loader order.

    Every rank iterates the SAME loader and keeps its parallel.shard_bounds slice of each global batch, as
    evaluate_dataset_parallel does; it collects the int8 integers of its slices with their labels, and ONE
    parallel.gather_feature_rows at the end (one all_gather_into_tensor: uneven shards padded to the largest and trimmed by their
    counts) brings every rank's rows to every rank, where they are put back into loader order.  integers=False: the gathered
    integers are dequantised once, behind the gather (a quarter of the float32 bytes cross the wire).
    n_last, avgpool, wide: as for extract_features (the pooled rows, checked before the loader is touched)."""
    from .parallel import gather_feature_rows
    pooled = int(n_last) != 1 or bool(avgpool)
    C = pooled_width(model, n_last, avgpool, wide) if pooled else int(model.num_features)
    if pooled and graph:
        raise ValueError("extract_features_parallel: features_pooled is not part of the graph replays (graph=False)")
    if dist.is_available() and dist.is_initialized():
        world, rank = dist.get_world_size(), dist.get_rank()
    else:
        world, rank = 1, 0
    data_loader, N = _sized(data_loader)
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
            if pooled and transform is None:
                scale = _pooled_into(model, imgs[lo:hi].to(device), rows, n_last, avgpool)
            elif pooled:
                u8 = transform(imgs, lo, hi, device=device)
                takes = getattr(model, "takes_engine_for_features", None)
                x = u8 if takes is not None and takes(u8) else transform.to_float(u8)
                scale = _pooled_into(model, x, rows, n_last, avgpool, (transform.mean, transform.std))
            elif transform is None:
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
