"""Swin built with the I-BERT operators (gelu_type = softmax_type = layernorm_type = 'ibert'), frozen and called module by module:
the integer-carrying path (quantization_utils/lazy.py) against the literal module path, bit for bit and tap for tap; which kernels it
launches and how often; what it materialises; and the reference's own forward (tests/golden/swin_ibert_small.npz, written by
scripts/gen_swin_ibert_golden.py from the reference's swin_quant.py assembly with its I-BERT classes).

Models A and B are those of tests/test_gpu_swin_lazy.py (56 px, 7 x 7 windows, depths (2, 2); 96 px, 12 x 12 windows, depths (2,)),
calibrated as there."""
import os
import warnings
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402

DEV = "cuda:0"
MODELS = {"A": dict(img_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6)),
          "A4": dict(img_size=56, window_size=7, depths=(4, 2), num_heads=(3, 6)),
          "B": dict(img_size=96, window_size=12, depths=(2,), num_heads=(3,))}
IBERT = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
BATCH = 3
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "swin_ibert_small.npz")
_BUILT = {}


def _images(n, img, g):
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def snap_pow2(model):
    for mod in model.modules():
        if isinstance(mod, qu.QuantAct):
            qmax = 2 ** (mod.activation_bit - 1) - 1
            a = max(-float(mod.x_min), float(mod.x_max)) / qmax
            if a == 0.0:
                continue                                   # act_out: constructed, never called
            p = 2.0 ** np.ceil(np.log2(a))
            mod.x_max.fill_(qmax * p)
            mod.x_min.fill_(-qmax * p)


def built(which, pow2, ops=None):
    """the calibrated, frozen model and a batch for it; built once per (model, regime, operators) and shared -- no test changes it"""
    key = (which, pow2, ops)
    if key not in _BUILT:
        cfg = MODELS[which]
        torch.manual_seed(11 + ord(which[0]) + pow2)
        names = IBERT if ops is None else dict(zip(("gelu_type", "softmax_type", "layernorm_type"), ops))
        model = ivit.SwinTransformer(patch_size=4, embed_dim=96, num_classes=10, **names, **cfg).to(DEV).eval()
        g = torch.Generator(device="cpu").manual_seed(5 + ord(which[0]))
        with torch.no_grad():
            for name, p in model.named_parameters():      # wider weights than the init's 0.02: activations that use their ranges
                if p.dim() > 1:
                    p.mul_(3.0)
                elif name.endswith("relative_position_bias_table"):
                    p.mul_(20.0)
            calib = _images(4, cfg["img_size"], g)
            model(calib)
            model(calib.flip(0) * 0.7)
        if pow2:
            snap_pow2(model)
        ivit.freeze_model(model)
        _BUILT[key] = (model, _images(BATCH, cfg["img_size"], g))
    return _BUILT[key]


def module_run(model, x, lazy_on, taps=None):
    """the module-by-module forward; taps: receives every QuantAct output (except act_out) as integers"""
    hooks = []
    if taps is not None:
        def hook(name):
            def fn(mod, inp, outp):
                y, s = outp
                taps[name] = y.q.to(torch.int32) if isinstance(y, lazy.QT) and y.q is not None else torch.round(y / s).to(torch.int32)
            return fn
        hooks = [mod.register_forward_hook(hook(name)) for name, mod in model.named_modules()
                 if isinstance(mod, qu.QuantAct) and name != "act_out" and not name.endswith("log_int_softmax.act")]
    old, model.use_engine = lazy.ENABLED, False
    try:
        lazy.ENABLED = lazy_on
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return model(x)
    finally:
        lazy.ENABLED = old
        model.use_engine = True
        for h in hooks:
            h.remove()


def expected_fused(model, rows_stage0):
    """launches at QuantActs per forward, counted as tests/test_gpu_swin_lazy.py counts them.  Per block: norm1, qkv, window
    attention, proj -> qact4, the residual qact2, norm2, fc1, GELU, then fc2 and the residual qact4 -- one launch where the residual
    GEMM applies (>= 2048 rows and the fragment weight copy), else two.  Stem: patch GEMM, patch norm, qact1.  Per PatchMerging:
    norm, reduction.  Tail: norm, qact3."""
    n, rows, C = 0, rows_stage0, model.embed_dim
    for li, depth in enumerate(model.depths):
        fused_fc2 = rows >= 2048 and (4 * C) % 192 == 0 and C % 64 == 0 and C >= 128
        n += depth * (9 if fused_fc2 else 10)
        rows, C = rows // 4, 2 * C
    return n + 3 + 2 * (len(model.depths) - 1) + 2


def counted(model, x):
    """lazy.STATS of one forward after a warm-up forward"""
    module_run(model, x, True)
    lazy.STATS.update(fused=0, materialised=0)
    y = module_run(model, x, True)
    return y, dict(lazy.STATS)


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_swin_ibert_lazy_equals_the_literal_path(which, pow2):
    model, x = built(which, pow2)
    assert model.op_types == ("ibert",) * 3 and "operator family" in model.engine_unsupported_reason() and not model.takes_engine(x)
    t_lazy, t_plain, launched = {}, {}, []
    real_call = _lib.call
    try:
        _lib.call = lambda name, *a: (launched.append(name), real_call(name, *a))[1]
        y_lazy = module_run(model, x, True, t_lazy)
    finally:
        _lib.call = real_call
    y_plain = module_run(model, x, False, t_plain)
    assert torch.equal(y_lazy, y_plain) and len(torch.unique(y_plain)) > BATCH
    assert set(t_lazy) == set(t_plain) and len(t_lazy) == 13 * sum(model.depths) + 2 * (len(model.depths) - 1) + 6
    for name in t_plain:
        a, b = t_lazy[name].reshape(-1), t_plain[name].reshape(-1)
        assert a.numel() == b.numel() and torch.equal(a, b), f"tap {name}: {int((a != b).sum())} of {a.numel()} differ"
    # every block's attention, the shifted and masked ones included, is one launch of the new entry; no Shiftmax form, no literal softmax
    assert launched.count("ivit_window_attention_i8_ibert") == sum(model.depths) and "ivit_window_rows" in launched, sorted(set(launched))
    assert not [n for n in launched if n.startswith(("ivit_window_attention_i8", "ivit_ibert_softmax")) and not n.endswith("_ibert")
                and n != "ivit_ibert_softmax_build_table"], sorted(set(launched))
    y, stats = counted(model, x)
    g = model.patch_grid[0]
    assert torch.equal(y, y_plain) and stats["fused"] == expected_fused(model, BATCH * g * g), stats
    assert stats["materialised"] <= 4, stats


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
def test_nothing_inside_a_block_materialises(pow2):
    """two more blocks, the same number of float tensors: the sites that materialise are outside the blocks and the attention -- the
    patch norm behind the per-channel scale of the patch convolution, the float pooling and the logits"""
    (m2, x), (m4, _) = built("A", pow2), built("A4", pow2)
    _, s2 = counted(m2, x)
    _, s4 = counted(m4, x)
    assert s2["materialised"] == s4["materialised"] <= 4, (s2, s4)
    assert s4["fused"] - s2["fused"] == 2 * 10, (s2, s4)


@pytest.mark.parametrize("ops", [("ibert", "ivit", "ivit"), ("ivit", "ibert", "ivit"), ("ivit", "ivit", "ibert")], ids="-".join)
def test_swin_mixtures_carry_integers_too(ops):
    """one I-BERT operator at a time beside two I-ViT ones (model A, ranges as calibrated): every site is resolved by its own module --
    the literal path's logits, the same launch count, nothing more materialised, the window attention of the softmax's family"""
    model, x = built("A", False, ops)
    assert model.op_types == ops and "operator family" in model.engine_unsupported_reason()
    y_plain = module_run(model, x, False)
    launched, real_call = [], _lib.call
    try:
        _lib.call = lambda name, *a: (launched.append(name), real_call(name, *a))[1]
        module_run(model, x, True)
    finally:
        _lib.call = real_call
    y, stats = counted(model, x)
    g = model.patch_grid[0]
    assert torch.equal(y, y_plain) and stats["fused"] == expected_fused(model, BATCH * g * g) and stats["materialised"] <= 4, stats
    assert (launched.count("ivit_window_attention_i8_ibert") == sum(model.depths)) == (ops[1] == "ibert"), sorted(set(launched))
    assert ("ivit_ibert_gelu_build_lut" in launched) == (ops[0] == "ibert")
    assert bool([n for n in launched if n.startswith("ivit_ibert_layernorm_i")]) == (ops[2] == "ibert"), sorted(set(launched))


def test_mask_beyond_the_precondition_runs_that_attention_core_literally():
    """attn.qact2 of the shifted block at s_attn = 0.5: the host proof fails (prepare.ibert_window_mask_ok), that block's attention core
    runs the literal softmax, its float result re-enters the integer stream at attn.qact3 and the forward still equals the literal
    path; the other blocks keep their fused launch, and the restored range is served again"""
    from ivit_amd.prepare import ibert_window_mask_ok
    from ivit_amd.quantization_utils.ibert_modules import softmax_constants
    model, x = built("A", True)
    blk = model.layers[0].blocks[1]
    assert blk.attn_mask is not None and not ibert_window_mask_ok(0.5, softmax_constants(0.5, 0.0, 1.0)[0])
    qa = blk.attn.qact2
    keep = (qa.x_min.clone(), qa.x_max.clone())
    y_ok = module_run(model, x, True)
    launched, real_call = [], _lib.call
    try:
        qa.x_min.fill_(-127 * 0.5)
        qa.x_max.fill_(127 * 0.5)
        module_run(model, x, True)
        lazy.STATS.update(fused=0, materialised=0)
        try:
            _lib.call = lambda name, *a: (launched.append(name), real_call(name, *a))[1]
            y_lazy = module_run(model, x, True)
        finally:
            _lib.call = real_call
        stats = dict(lazy.STATS)
        y_plain = module_run(model, x, False)
    finally:
        qa.x_min.copy_(keep[0])
        qa.x_max.copy_(keep[1])
    assert torch.equal(y_lazy, y_plain)
    assert launched.count("ivit_window_attention_i8_ibert") == sum(model.depths) - 1 and "ivit_ibert_softmax_f32_f32" in launched
    g = model.patch_grid[0]
    # everything else is still carried: the same launches at QuantActs (the re-entry at attn.qact3 counts as that block's attention), and
    # beyond the model's two float tensors only the literal chain of the one block -- at most its twelve pending tensors, each counted
    # once: the product, the probabilities, the masked, biased, requantised, scaled and raw scores, the bias identity, q, k^T, v, qkv
    assert stats["fused"] == expected_fused(model, BATCH * g * g) and 2 < stats["materialised"] <= 2 + 12, stats
    assert torch.equal(module_run(model, x, True), y_ok)


def test_swin_ibert_equals_the_reference_fixture():
    """model A with the fixture's seeded numpy weights (synth.make_swin_float_state), the ranges the reference calibrated, snapped to
    powers of two, and its LayerNorm shifts, on the fixture's 3 seeded images: INT32 logits, top-1 and the CRC32 of every QuantAct tap
    of the reference's own forward"""
    import json
    from ivit_amd import synth
    z = np.load(GOLDEN, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = synth.SWIN_CONFIGS[meta["config"]]
    assert (meta["img_size"], cfg["window"], cfg["depths"], cfg["num_heads"]) == tuple(MODELS["A"].values())
    model = ivit.SwinTransformer(img_size=meta["img_size"], patch_size=4, window_size=cfg["window"], embed_dim=cfg["embed_dim"],
                                 depths=cfg["depths"], num_heads=cfg["num_heads"], **IBERT)
    fs = synth.make_swin_float_state(meta["config"], meta["weight_seed"])
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected and not [k for k in missing if k.endswith((".weight", ".bias", "relative_position_bias_table"))], (missing, unexpected)
    acts = dict(model.named_modules())
    for n, (lo, hi) in zip([str(n) for n in z["range_names"]], z["ranges"]):
        acts[n].x_min.fill_(float(lo))
        acts[n].x_max.fill_(float(hi))
    for n, sh in zip([str(n) for n in z["shift_names"]], z["shifts"]):
        acts[n].shift.fill_(float(sh))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    x = torch.from_numpy(z["images"]).to(DEV)
    taps = {}
    y = module_run(model, x, True, taps)
    li = torch.round(y / torch.from_numpy(z["head_scale"]).to(DEV)).to(torch.int64).cpu().numpy().astype(np.int32)
    assert np.array_equal(li, z["logits_int32"]), int((li != z["logits_int32"]).sum())
    assert np.array_equal(y.argmax(dim=1).cpu().numpy().astype(np.int64), z["top1"])
    gold = dict(zip([str(n) for n in z["tap_names"]], z["tap_crc32"]))
    checked = [n for n in taps if n in gold]
    bad = [n for n in checked if zlib.crc32(np.ascontiguousarray(taps[n].cpu().numpy().astype(np.int32)).tobytes()) != int(gold[n])]
    assert not bad and len(checked) >= 13 * sum(model.depths), (len(checked), bad[:6])
