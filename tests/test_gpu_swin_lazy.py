"""A frozen Swin model called module by module carries int8 / int16 between its modules (quantization_utils/lazy.py): bit equality
with the ordinary module path (lazy.ENABLED = False) and the fused engine, the number of fused launches and materialisations, no
device wait after the warm-up forward, the row kernel switch, the reference's golden fixtures, a mask that is not region-structured,
the float layout the patch embedding's LayerNorm depends on, and a caller that drives the modules itself.

Model A: 56 px, 7 x 7 windows, depths (2, 2): a 2 x 2-window stage with a shifted, masked block, a PatchMerging, a one-window stage.
Model B: 96 px, 12 x 12 windows, depths (2,): 144-token windows with shift 6 (ivit_window_attention_i8_long); its stream keeps the
patch embedding's transposed layout up to the pooling."""
import warnings
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ivit = pytest.importorskip("ivit_amd")
import ivit_amd.quantization_utils as qu  # noqa: E402
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.checkpoint import load_fixture  # noqa: E402
from ivit_amd.quantization_utils import lazy  # noqa: E402
from ivit_amd.swin_quant import window_partition, window_reverse  # noqa: E402

DEV = "cuda:0"
MODELS = {"A": dict(img_size=56, window_size=7, depths=(2, 2), num_heads=(3, 6)),
          "B": dict(img_size=96, window_size=12, depths=(2,), num_heads=(3,))}
BATCH = 3
_BUILT = {}


def _images(n, img, g):
    low = torch.nn.functional.interpolate(torch.randn(n, 3, 6, 6, generator=g), size=(img, img), mode="bilinear", align_corners=False)
    return (low + 0.3 * torch.randn(n, 3, img, img, generator=g)).to(DEV)


def built(which, pow2):
    """the calibrated, frozen model and a batch for it; built once per (model, regime) and shared -- no test changes it for good"""
    key = (which, pow2)
    if key not in _BUILT:
        cfg = MODELS[which]
        torch.manual_seed(11 + ord(which) + pow2)
        model = ivit.SwinTransformer(patch_size=4, embed_dim=96, num_classes=10, norm_layer=partial(qu.IntLayerNorm, eps=1e-6),
                                     **cfg).to(DEV).eval()
        g = torch.Generator(device="cpu").manual_seed(5 + ord(which))
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
            for mod in model.modules():
                if isinstance(mod, qu.QuantAct):
                    qmax = 2 ** (mod.activation_bit - 1) - 1
                    a = max(-float(mod.x_min), float(mod.x_max)) / qmax
                    p = 2.0 ** np.ceil(np.log2(a))
                    mod.x_max.fill_(qmax * p)
                    mod.x_min.fill_(-qmax * p)
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
                 if isinstance(mod, qu.QuantAct) and name != "act_out"]
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
    """launches at QuantActs per forward.  Per block: norm1, qkv, window attention, proj -> qact4, the residual qact2, norm2, fc1,
    GELU, then fc2 and the residual qact4 -- one launch where the residual GEMM applies (>= 2048 rows and the fragment weight
    copy), else two.  Stem: patch GEMM, patch norm, qact1.  Per PatchMerging: norm, reduction.  Tail: norm, qact3."""
    n, rows, C = 0, rows_stage0, model.embed_dim
    for li, depth in enumerate(model.depths):
        fused_fc2 = rows >= 2048 and (4 * C) % 192 == 0 and C % 64 == 0 and C >= 128
        n += depth * (9 if fused_fc2 else 10)
        rows, C = rows // 4, 2 * C
    return n + 3 + 2 * (len(model.depths) - 1) + 2


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_lazy_swin_equals_the_ordinary_path_and_the_engine(which, pow2):
    model, x = built(which, pow2)
    t_lazy, t_plain, launched = {}, {}, set()
    real_call = _lib.call
    try:
        _lib.call = lambda name, *a: (launched.add(name), real_call(name, *a))[1]
        y_lazy = module_run(model, x, True, t_lazy)
    finally:
        _lib.call = real_call
    y_plain = module_run(model, x, False, t_plain)
    assert torch.equal(y_lazy, y_plain) and len(torch.unique(y_plain)) > BATCH
    assert set(t_lazy) == set(t_plain) and len(t_lazy) == 13 * sum(model.depths) + 2 * (len(model.depths) - 1) + 6
    for name in t_plain:
        a, b = t_lazy[name].reshape(-1), t_plain[name].reshape(-1)
        assert a.numel() == b.numel() and torch.equal(a, b), f"tap {name}: {int((a != b).sum())} of {a.numel()} differ"
    assert ("ivit_window_attention_i8_long" in launched) == (which == "B") and "ivit_window_rows" in launched, sorted(launched)
    # the engine, where it takes the model (model B ends at 96 features: its classifier GEMM does not)
    if model.engine_unsupported_reason() is None:
        with torch.no_grad():
            ye = model(x)
        # an even token count at the pool at natural scales: the engine restates torch's CPU pooling order, the module paths pool with
        # CUDA's mean; everywhere else the two orders agree and so must the logits
        if not model._engine[2].pool_literal:
            assert torch.equal(ye, y_lazy)
    else:
        assert which == "B"


@pytest.mark.parametrize("pow2", [False, True], ids=["natural", "pow2"])
@pytest.mark.parametrize("which", ["A", "B"])
def test_lazy_swin_counts_never_syncs_and_row_kernel_switch(which, pow2):
    model, x = built(which, pow2)
    y_plain = module_run(model, x, False)
    model.use_engine = False
    lazy._WARNED.clear()
    try:
        with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            model(x)                                      # warm-up: constants, row maps, bias integers, mask regions
            lazy.STATS.update(fused=0, materialised=0)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                y = model(x)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            stats = dict(lazy.STATS)
            old = lazy.ROW_KERNEL
            try:
                lazy.ROW_KERNEL = False
                y_torch_rows = model(x)
            finally:
                lazy.ROW_KERNEL = old
    finally:
        model.use_engine = True
    assert torch.equal(y, y_plain) and torch.equal(y_torch_rows, y_plain)
    g = model.patch_grid[0]
    assert stats["fused"] == expected_fused(model, BATCH * g * g), stats
    assert stats["materialised"] <= 2, stats              # the float pooling of the tail and the logits
    told = [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning) and "ivit_amd.lazy" in str(w.message)]
    assert len(told) <= 1 and all("int8 payload" in t for t in told), told      # the pooling tail's producer, once


def test_lazy_swin_at_the_residual_gemm_size():
    """model A at batch 44 (8624 rows in stage 0, 2156 in stage 1: mlp.fc2 + mlp.qact2 + qact4 are one residual GEMM there, and the
    qkv GEMM of stage 1 writes head-major itself): the same bits as the ordinary path on the images both see"""
    model, x = built("A", False)
    g = torch.Generator(device="cpu").manual_seed(3)
    big = torch.cat([x, _images(41, 56, g)])
    y_plain = module_run(model, x, False)
    lazy.STATS.update(fused=0, materialised=0)
    y = module_run(model, big, True)
    assert lazy.STATS["fused"] == expected_fused(model, 44 * 14 * 14), lazy.STATS
    assert torch.equal(y[:BATCH], y_plain)


@pytest.mark.parametrize("tag", ["swin_tiny", "swin_tiny_natural"])
def test_lazy_swin_golden_fixtures(tag):
    """the reference's own forward (tests/golden): INT32 / float logits and top-1 through the lazy module path at the fixture's batch,
    and every QuantAct tap the fixture holds.  swin_tiny_natural has 69 patch-embedding rows whose LayerNorm mean is an exact .5
    tie: they are right only in the outer reduction order, i.e. when the carrier hands the float layout on"""
    import zlib
    z, meta, ranges = load_fixture(tag)
    fs = synth.make_swin_float_state(meta["factory"], meta["weight_seed"])
    model = getattr(ivit, meta["factory"])()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    for name, mod in model.named_modules():
        if isinstance(mod, qu.QuantAct) and name in ranges:
            mod.x_min.fill_(float(ranges[name][0]))
            mod.x_max.fill_(float(ranges[name][1]))
    model.to(DEV).eval()
    ivit.freeze_model(model)
    imgs = torch.from_numpy(synth.make_images(meta["n_images"], meta["image_seed"])).to(DEV)
    taps = {}
    y = module_run(model, imgs, True, taps)
    lazy.STATS.update(fused=0, materialised=0)
    assert torch.equal(module_run(model, imgs, True), y) and lazy.STATS["materialised"] <= 2, lazy.STATS      # no hooks attached
    gold = dict(zip([str(n) for n in z["tap_names"]], z["tap_crc32"]))
    checked = [n for n in taps if n in gold]
    bad = [n for n in checked if zlib.crc32(np.ascontiguousarray(taps[n].cpu().numpy().astype(np.int32)).tobytes()) != int(gold[n])]
    assert not bad and len(checked) >= 9 * sum(model.depths), (len(checked), bad[:6])
    if "head_scale" in z.files:
        li = torch.round(y / torch.from_numpy(z["head_scale"]).to(DEV)).to(torch.int64).cpu().numpy().astype(np.int32)
        assert np.array_equal(li, z["logits_int32"])
    if "regime" not in meta:
        assert np.array_equal(y.cpu().numpy().view(np.int32), z["logits_f32_bits"])
    assert np.array_equal(y.argmax(dim=1).cpu().numpy().astype(np.int64), z["top1"])
    if tag == "swin_tiny_natural":
        # the layout: with the carrier's layout ignored (the contiguous reduction order) the patch embedding comes out different
        real = lazy.ln_outer
        t_inner = {}
        try:
            lazy.ln_outer = lambda fl: 0
            module_run(model, imgs, True, t_inner)
        finally:
            lazy.ln_outer = real
        differ = int((t_inner["patch_embed.qact"] != taps["patch_embed.qact"]).sum())
        assert differ > 0, "outer and inner reduction orders agree on every row: the layout check has no teeth"


def test_lazy_swin_mask_that_is_not_region_structured():
    """one entry of a block's attn_mask changed: no region ids describe it, the chain materialises (counted) and still equals the
    ordinary path"""
    model, x = built("A", True)
    blk = model.layers[0].blocks[1]
    assert blk.attn_mask is not None
    keep = blk.attn_mask.clone()
    y_ok = module_run(model, x, True)
    try:
        blk.attn_mask[1, 3, 5] = -100.0 if float(keep[1, 3, 5]) == 0.0 else 0.0
        lazy.STATS.update(fused=0, materialised=0)
        y_lazy = module_run(model, x, True)
        stats = dict(lazy.STATS)
        y_plain = module_run(model, x, False)
    finally:
        blk.attn_mask.copy_(keep)
    assert torch.equal(y_lazy, y_plain) and stats["materialised"] > 2
    assert torch.equal(module_run(model, x, True), y_ok)   # and the restored mask is recognised again


def test_lazy_swin_for_a_caller_that_drives_the_modules_itself():
    """lazy.enable_everywhere(): the block, attention and merging forwards written out against the sub-modules, no scope opened"""
    model, x = built("A", False)
    y_plain = module_run(model, x, False)

    def attention(a, x, s, mask):
        B_, N, C = x.shape
        nH = a.num_heads
        x, s_qkv = a.qact1(*a.qkv(x, s))
        qkv = x.reshape(B_, N, 3, nH, C // nH).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn, s = a.matmul_1(q, s_qkv, k.transpose(-2, -1), s_qkv)
        attn, s = a.qact_attn1(attn * a.scale, s * a.scale)
        table, s_table = a.qact_table(a.relative_position_bias_table)
        bias = table[a.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1).contiguous()
        attn, s = a.qact2(attn, s, bias.unsqueeze(0), s_table)
        if mask is not None:
            nW = mask.shape[0]
            attn = attn.view(B_ // nW, nW, nH, N, N) + mask.unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, nH, N, N)
        attn, s = a.log_int_softmax(attn, s)
        x, s = a.matmul_2(a.attn_drop(attn), s, v, s_qkv)
        x, s = a.qact3(x.transpose(1, 2).reshape(B_, N, C), s)
        x, s = a.qact4(*a.proj(x, s))
        return a.proj_drop(x), s

    def block(b, x_1, s_1):
        H, W = b.input_resolution
        B, L, C = x_1.shape
        ws, sh = b.window_size, b.shift_size
        x, s = b.qact1(*b.norm1(x_1, s_1))
        x = x.view(B, H, W, C)
        if sh > 0:
            x = torch.roll(x, shifts=(-sh, -sh), dims=(1, 2))
        x, s = attention(b.attn, window_partition(x, ws).view(-1, ws * ws, C), s, b.attn_mask)
        x = window_reverse(x.view(-1, ws, ws, C), ws, H, W)
        if sh > 0:
            x = torch.roll(x, shifts=(sh, sh), dims=(1, 2))
        x_2, s_2 = b.qact2(x.view(B, H * W, C), s, x_1, s_1)
        x, s = b.qact3(*b.norm2(x_2, s_2))
        x, s = b.mlp(x, s)
        return b.qact4(x, s, x_2, s_2)

    def features(m, x):
        x, s = m.patch_embed(*m.qact_input(x))
        x, s = m.qact1(x, s)
        for layer in m.layers:
            for b in layer.blocks:
                x, s = block(b, x, s)
            if layer.downsample is not None:
                x, s = layer.downsample(x, s)
        return m.qact2(*m.norm(x, s))

    lazy.enable_everywhere(True)
    try:
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            features(model, x)                             # warm-up
            lazy.STATS.update(fused=0, materialised=0)
            t, s = features(model, x)
            assert isinstance(t, lazy.QT) and t.q8 is not None and lazy.STATS["materialised"] == 0, lazy.STATS
            assert lazy.STATS["fused"] == expected_fused(model, BATCH * 14 * 14) - 1       # all but qact3
            pooled = model.avgpool(t.transpose(1, 2))
            h, s = model.qact3(pooled.transpose(1, 2), s)
            y, _ = model.head(torch.flatten(h, 1), s)
            assert isinstance(y, lazy.QT)
            assert torch.equal(y + 0.0, y_plain)
    finally:
        lazy.enable_everywhere(False)
    assert not lazy.active()


def test_short_window_attention_refuses_the_integer_form_it_cannot_compute():
    """s_attn = 1 / 64 (x0 = -64) with a shift mask: the exponent table has not saturated within its 256 distances, so the integer form
    has no entry for a masked score; the entry refuses (swin_engine.window_attention_spec then hands over the phi tables, which
    model A in the power-of-two regime exercises above), and accepts the same call with s_attn = 1 / 16"""
    nwin, nH, N = 4, 3, 49
    qkv = torch.zeros(3, nwin, nH, N, 32, dtype=torch.int8, device=DEV)
    out = torch.zeros(nwin * N, nH * 32, dtype=torch.int8, device=DEV)
    bias = torch.zeros(nH, N, 64, dtype=torch.int16, device=DEV)
    region = torch.zeros(4, 64, dtype=torch.uint8, device=DEV)
    region[:, 20:] = 1
    args = lambda s: (_lib.ptr(qkv), _lib.ptr(out), nH * 32, _lib.ptr(bias), _lib.ptr(region), int(-100 / s), nwin, 4, nH, N, 32,
                      1 << 30, 30, 1 << 30, 30, s, 1 << 30, 30, _lib.stream_ptr())
    with pytest.raises(_lib.IvitError, match="cannot place masked scores"):
        _lib.call("ivit_window_attention_i8", *args(1.0 / 64))
    _lib.call("ivit_window_attention_i8", *args(1.0 / 16))
    torch.cuda.synchronize()
