#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE itself.

Runs only in the build container (needs /root/reference, CPU only).  The
reference is imported unmodified; the only harness-side shims are the ones
listed in SURVEY.md Appendix E (``Tensor.cuda`` redirect so the hard-coded
``.cuda()`` calls work on CPU).  What is committed are the *numbers* this
script produces (inputs + expected outputs) together with this script -- never
reference source.

Protocol:
  model(pretrained=False, 'ivit' layers) <- synthetic float weights (i-vit_amd/synth.py)
  -> eval, one calibration forward on a seeded batch (initialises x_min/x_max)
  -> snap every QuantAct range to +-127*2^p  ("pow2-calibrated" regime)
  -> freeze_model -> golden forward with hooks on every QuantAct / Shiftmax / ShiftGELU.
Each golden forward is compared against the CPU oracle (oracle/oracle.py) on
the spot; the script fails if any tap or logit differs.

Usage:  python oracle/gen_golden.py [ops] [deit_tiny] [deit_small] [deit_base] [vit_base]
"""
import hashlib
import importlib
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
GOLD = os.path.join(ROOT, "tests", "golden")

# ---- shim 1: hard-coded .cuda() -> stay on the tensor's device
torch.Tensor.cuda = lambda self, device=None, *a, **k: self if device is None else self.to(device)
sys.path.insert(0, "/root/reference")
import models as ref_models  # noqa: E402
import models.quantization_utils as rq  # noqa: E402
from models.quantization_utils.quant_utils import (SymmetricQuantFunction, batch_frexp,  # noqa: E402
                                                    fixedpoint_mul, symmetric_linear_quantization_params)

synth = importlib.import_module("i-vit_amd.synth")
from oracle import oracle as orc  # noqa: E402

torch.set_grad_enabled(False)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, dtype=np.int32).tobytes())


def to_int(y, scale):
    """Integer view of a fake-quant float tensor (exact for the scales used here)."""
    return torch.round(y / scale).to(torch.int64).numpy().astype(np.int32)


# ----------------------------------------------------------------------------- op-level KATs

def gen_ops():
    rng = np.random.default_rng(20260101)
    out = {}

    # --- batch_frexp + fixedpoint_mul (QuantAct requant), per-channel / per-tensor / identity
    cases = []
    for ci, (rows, Cn, per_ch, ident, bits, zmag) in enumerate([
            (64, 96, True, False, 8, 3.0e5), (64, 96, False, False, 8, 2.0e4), (32, 192, False, True, 8, 200),
            (32, 48, True, False, 16, 3.0e5), (16, 40, False, True, 16, 127), (64, 64, True, False, 8, 9.0e8),
            (8, 32, False, False, 32, 1.0e6)]):
        z = np.rint(rng.normal(0, zmag / 3, size=(1, rows, Cn))).astype(np.float32)
        if ci == 5:  # LayerNorm-sized inputs (24 significant bits)
            z = z.astype(np.float32)
        pre = (rng.uniform(0.5, 2.0, size=Cn if per_ch else 1) * 2.0 ** rng.integers(-20, -8)).astype(np.float32)
        if ci == 5:
            pre = (rng.uniform(0.5, 1.5, size=Cn) * np.float32(np.sqrt(np.float32(Cn))) / 2 ** 30).astype(np.float32)
        q = 2 ** (bits - 1) - 1
        target = np.abs(z * pre).max() / q * rng.uniform(0.6, 1.3)
        zsf = np.float32(2.0 ** np.ceil(np.log2(target)))
        x = torch.from_numpy(z) * torch.from_numpy(pre)  # producer output v*scale (float32)
        # the consumer recovers z_int = round(x/pre) -- keep the value the reference sees
        z_seen = torch.round(x / torch.from_numpy(pre)).numpy()
        kw = {}
        if ident:
            z2 = rng.integers(-128, 128, size=(1, rows, Cn)).astype(np.float32)
            pre2 = np.float32(2.0 ** rng.integers(-6, -2))
            kw = dict(identity=torch.from_numpy(z2) * pre2, identity_scaling_factor=torch.tensor([pre2]))
        y = fixedpoint_mul.apply(x, torch.from_numpy(pre), bits, "symmetric", torch.tensor([zsf]),
                                 kw.get("identity"), kw.get("identity_scaling_factor"))
        new_scale = torch.from_numpy(pre).double() / torch.tensor([zsf]).float().double()
        m, e = batch_frexp(new_scale.view(1, 1, -1))
        c = f"rq{ci}_"
        out[c + "z"] = z_seen.astype(np.float32).reshape(rows, Cn)
        out[c + "pre"] = pre
        out[c + "zsf"] = np.float32(zsf)
        out[c + "bits"] = np.int32(bits)
        out[c + "m"] = m.numpy().reshape(-1).astype(np.float64)
        out[c + "e"] = e.numpy().reshape(-1).astype(np.int32)
        if ident:
            out[c + "z2"] = z2.reshape(rows, Cn).astype(np.int32)
            out[c + "pre2"] = pre2
        out[c + "out"] = y.numpy().reshape(rows, Cn).astype(np.int32)
        cases.append(ci)
    out["rq_cases"] = np.array(cases, np.int32)

    # --- tie cases of the dyadic rounding: z*m/2^e exactly at .5 (half-to-even)
    pre = np.array([2.0 ** -9], np.float32)
    zsf = np.float32(2.0 ** -5)   # ratio 1/16 -> m = 2^30, e = 34
    z = np.arange(-64, 65, dtype=np.float32).reshape(1, 1, -1) * 8
    y = fixedpoint_mul.apply(torch.from_numpy(z) * pre[0], torch.from_numpy(pre), 8, "symmetric", torch.tensor([zsf]))
    out["rqtie_z"] = z.reshape(1, -1)
    out["rqtie_pre"] = pre
    out["rqtie_zsf"] = zsf
    out["rqtie_out"] = y.numpy().reshape(1, -1).astype(np.int32)

    # --- SymmetricQuantFunction (input-mode QuantAct and weight quantisation)
    x = rng.normal(0, 1.0, size=(4, 257)).astype(np.float32)
    s = np.float32(4.0 / 127.0)
    out["qs_x"] = x
    out["qs_s"] = s
    out["qs_out"] = SymmetricQuantFunction.apply(torch.from_numpy(x), 8, torch.tensor([s]), False).numpy().astype(np.int32)

    # --- QuantLinear end to end (weight/bias quantisation + integer GEMM)
    lin = rq.QuantLinear(80, 24)
    W = rng.normal(0, 0.05, size=(24, 80)).astype(np.float32)
    b = rng.normal(0, 0.05, size=(24,)).astype(np.float32)
    lin.weight.data = torch.from_numpy(W)
    lin.bias.data = torch.from_numpy(b)
    s_in = np.float32(2.0 ** -4)
    xin = rng.integers(-128, 128, size=(1, 10, 80)).astype(np.float32)
    yl, sl = lin(torch.from_numpy(xin) * s_in, torch.tensor([s_in]))
    out["lin_W"], out["lin_b"], out["lin_sin"], out["lin_x"] = W, b, s_in, xin.reshape(10, 80).astype(np.int32)
    out["lin_wint"] = lin.weight_integer.numpy().astype(np.int32)
    out["lin_bint"] = lin.bias_integer.numpy().astype(np.int32)
    out["lin_sw"] = lin.fc_scaling_factor.numpy().astype(np.float32)
    out["lin_sacc"] = sl.numpy().astype(np.float32)
    out["lin_acc"] = torch.round(yl / sl).numpy().reshape(10, 24).astype(np.int32)

    # --- QuantConv2d 16x16/16 as used by PatchEmbed
    conv = rq.QuantConv2d(3, 8, kernel_size=16, stride=16)
    Wc = rng.normal(0, 0.02, size=(8, 3, 16, 16)).astype(np.float32)
    bc = rng.normal(0, 0.02, size=(8,)).astype(np.float32)
    conv.weight.data = torch.from_numpy(Wc)
    conv.bias.data = torch.from_numpy(bc)
    xin = rng.integers(-128, 128, size=(2, 3, 32, 32)).astype(np.float32)
    s_in = np.float32(2.0 ** -5)
    yc, sc = conv(torch.from_numpy(xin) * s_in, torch.tensor([s_in]))
    out["conv_W"], out["conv_b"], out["conv_sin"], out["conv_x"] = Wc, bc, s_in, xin.astype(np.int32)
    out["conv_acc"] = torch.round(yc / sc).numpy().astype(np.int32)  # [2,8,2,2]
    out["conv_sacc"] = sc.numpy().reshape(-1).astype(np.float32)

    # --- QuantMatMul
    mm = rq.QuantMatMul()
    a = rng.integers(-128, 128, size=(2, 3, 17, 64)).astype(np.float32)
    bb = rng.integers(-128, 128, size=(2, 3, 64, 17)).astype(np.float32)
    sa = np.float32(2.0 ** -4)
    ym, sm = mm(torch.from_numpy(a) * sa, torch.tensor([sa]), torch.from_numpy(bb) * sa, torch.tensor([sa]))
    out["mm_a"], out["mm_b"] = a.astype(np.int32), bb.astype(np.int32)
    out["mm_out"] = torch.round(ym / sm).numpy().astype(np.int32)
    out["mm_s"] = sm.numpy().astype(np.float32)

    # --- IVITIntLayerNorm (float output of the module, bit exact) and LN -> QuantAct(8)
    for ci, (rows, Cn, lo, hi, p) in enumerate([(40, 192, -128, 128, -4), (24, 768, -128, 128, -5),
                                                (16, 384, -40, 41, -3), (8, 96, -30000, 30000, -9)]):
        ln = rq.IVITIntLayerNorm(Cn)
        gamma = rng.uniform(0.5, 1.5, size=Cn).astype(np.float32)
        beta = rng.normal(0, 0.1, size=Cn).astype(np.float32)
        ln.weight.data = torch.from_numpy(gamma)
        ln.bias.data = torch.from_numpy(beta)
        k = rng.integers(lo, hi, size=(1, rows, Cn)).astype(np.float32)
        k[0, 0, :] = 5          # constant row: var = 0
        k[0, 1, :] = np.where(np.arange(Cn) % 2 == 0, 3, 4)  # mean exactly x.5 -> tie
        s = np.float32(2.0 ** p)
        yl, sl = ln(torch.from_numpy(k) * s, torch.tensor([s]))
        qa = rq.QuantAct()
        zsf = 2.0 ** np.ceil(np.log2(np.abs(yl.numpy()).max() / 127))
        qa.x_min.fill_(-127 * zsf)
        qa.x_max.fill_(127 * zsf)
        qa.fix()
        yq, sq = qa(yl, sl)
        c = f"ln{ci}_"
        out[c + "k"] = k.reshape(rows, Cn).astype(np.int32)
        out[c + "gamma"], out[c + "beta"], out[c + "s"] = gamma, beta, s
        out[c + "y_bits"] = yl.numpy().reshape(rows, Cn).view(np.int32)      # float32 bit pattern
        out[c + "sln"] = sl.detach().numpy().reshape(-1).astype(np.float32)
        out[c + "bias_int"] = ln.bias_integer.numpy().astype(np.float32)
        out[c + "q_sf"] = np.float32(sq.item())
        out[c + "q_out"] = torch.round(yq / sq).numpy().reshape(rows, Cn).astype(np.int32)
    out["ln_cases"] = np.arange(4, dtype=np.int32)

    # --- IVITIntGELU
    for ci, (rows, L, p, lo, hi) in enumerate([(32, 768, -4, -128, 128), (16, 3072, -5, -128, 128),
                                               (16, 384, -3, -128, 128), (8, 256, -6, -128, 128),
                                               (8, 100, -2, -128, 128), (4, 64, -4, -128, -100)]):
        g = rq.IVITIntGELU()
        k = rng.integers(lo, hi, size=(1, rows, L)).astype(np.float32)
        if ci == 3:
            k[0, :, :] = np.arange(-128, 128)
        s = np.float32(2.0 ** p)
        yg, sg = g(torch.from_numpy(k) * s, torch.tensor([s]))
        c = f"gelu{ci}_"
        out[c + "k"] = k.reshape(rows, L).astype(np.int32)
        out[c + "s"] = s
        out[c + "out"] = torch.round(yg / sg).numpy().reshape(rows, L).astype(np.int32)
        out[c + "sout"] = np.float32(sg.item())
    out["gelu_cases"] = np.arange(6, dtype=np.int32)

    # --- IVITIntSoftmax
    for ci, (rows, L, p, sd) in enumerate([(64, 197, -2, 30), (64, 197, -3, 50), (32, 49, -2, 25),
                                           (16, 197, -1, 8), (16, 197, 0, 4), (8, 64, -4, 60), (8, 197, -5, 70)]):
        sm = rq.IVITIntSoftmax()
        k = np.clip(np.rint(rng.normal(0, sd, size=(1, 1, rows, L))), -128, 127).astype(np.float32)
        k[0, 0, 0, :] = 7   # uniform row
        k[0, 0, 1, :] = -128
        k[0, 0, 1, 3] = 127  # one-hot row
        s = np.float32(2.0 ** p)
        ys, ss = sm(torch.from_numpy(k) * s, torch.tensor([s]))
        c = f"sm{ci}_"
        out[c + "k"] = k.reshape(rows, L).astype(np.int32)
        out[c + "s"] = s
        out[c + "out"] = torch.round(ys / ss).numpy().reshape(rows, L).astype(np.int32)
    out["sm_cases"] = np.arange(7, dtype=np.int32)

    np.savez_compressed(os.path.join(GOLD, "ops_kat.npz"), **out)
    print("ops_kat.npz written:", len(out), "arrays")


# ----------------------------------------------------------------------------- whole model

MODEL_PLAN = {
    # tag: (factory name, weight seed, calib seed, calib batch, image seed, n golden images, full taps?)
    "deit_tiny": ("deit_tiny_patch16_224", 11, 101, 4, 1001, 8, True),
    "deit_small": ("deit_small_patch16_224", 12, 102, 4, 1002, 4, False),
    "deit_base": ("deit_base_patch16_224", 13, 103, 4, 1003, 4, False),
    "vit_base": ("vit_base_patch16_224", 14, 104, 2, 1004, 2, False),
    "vit_large": ("vit_large_patch16_224", 15, 105, 2, 1005, 2, False),     # round 4: the widest factory (vit_quant.py:391-406)
    # the fork's default operator family (vit_quant.py:188-190), same synthetic weights as deit_tiny
    "deit_tiny_ibert": ("deit_tiny_patch16_224", 11, 101, 4, 1001, 4, False),
}


def gen_model(tag):
    factory, wseed, cseed, cb, iseed, nimg, full = MODEL_PLAN[tag]
    family = "ibert" if tag.endswith("_ibert") else "ivit"
    cfg = synth.MODEL_CONFIGS[factory]
    t0 = time.time()
    model = getattr(ref_models, factory)(pretrained=False, gelu_type=family, softmax_type=family,
                                         layernorm_type=family)
    fs = synth.make_float_state(factory, wseed)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected, unexpected
    assert all(("scaling_factor" in k or "integer" in k or "x_min" in k or "x_max" in k or k.endswith(".shift"))
               for k in missing), missing[:5]
    model.eval()
    # calibration forward (running_stat defaults to True)
    model(torch.from_numpy(synth.make_images(cb, cseed)))
    # pow2 snap
    ranges = {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct):
            mx = float(torch.max(-mod.x_min, mod.x_max))
            assert mx > 0, name
            q = float(2 ** (mod.activation_bit - 1) - 1)     # 127; 32767 for the QuantAct(16) inside IBERTIntSoftmax
            p = int(np.ceil(np.log2(mx / q)))
            mod.x_max.fill_(q * 2.0 ** p)
            mod.x_min.fill_(-q * 2.0 ** p)
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
    assert list(ranges) == synth.qact_names(cfg["depth"], family), "QuantAct order drifted"
    ref_models.freeze_model(model)

    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            taps[name] = to_int(y, s)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, (rq.QuantAct, rq.IVITIntSoftmax, rq.IVITIntGELU, rq.IBERTIntSoftmax, rq.IBERTIntGELU)):
            if not name.endswith("int_softmax.act"):   # internal to IBERTIntSoftmax: its input is not an activation view
                mod.register_forward_hook(hook(name))

    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact2.act_scaling_factor).float()
    logits_int = torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32)
    logits_f32 = y.numpy().astype(np.float32)
    top1 = y.argmax(dim=1).numpy().astype(np.int64)
    t_ref = time.time() - t0

    # ---- check the oracle against the reference right here
    t1 = time.time()
    om = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], family=family)
    otaps = {}
    res = om.forward(imgs, otaps)
    bad = [n for n in taps if n in otaps and not np.array_equal(taps[n].reshape(-1), otaps[n].reshape(-1))]
    miss = [n for n in taps if n not in otaps]
    assert not miss, miss
    assert not bad, f"oracle != reference at {bad[:5]} ({len(bad)} taps)"
    assert np.array_equal(res["logits_int32"], logits_int), "INT32 logits differ"
    assert np.array_equal(res["logits_f32"].view(np.int32), logits_f32.view(np.int32)), "float logits differ"
    assert np.array_equal(res["top1"], top1)
    print(f"[{tag}] reference {t_ref:.1f}s, oracle {time.time()-t1:.1f}s: {len(taps)} taps + logits bit-equal; "
          f"max|acc|={om.max_acc} softmax rows with sum>=2^24: {om.softmax_inexact_rows}, "
          f"LN rows with an inexact float32 sum: {om.ln_inexact_rows}")
    assert om.max_acc < 2 ** 24

    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, family=family, weight_seed=wseed, calib_seed=cseed,
                                         calib_batch=cb, image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN,
                                         max_abs_acc=om.max_acc, softmax_inexact_rows=om.softmax_inexact_rows,
                                         ln_inexact_rows=om.ln_inexact_rows,
                                         torch=torch.__version__, numpy=np.__version__))),
        "range_names": np.array(list(ranges)),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": logits_int,
        "logits_f32_bits": logits_f32.view(np.int32),
        "top1": top1,
        "tap_names": np.array(names),
        "tap_crc32": np.array([crc(taps[n]) for n in names], np.uint32),
        "tap_absmax": np.array([int(np.abs(taps[n]).max()) for n in names], np.int64),
    }
    # digests of the derived integer weights guard the synthetic generator against drift
    wn, wd = [], []
    for name, mod in model.named_modules():
        if isinstance(mod, (rq.QuantLinear, rq.QuantConv2d)):
            for buf in ("weight_integer", "bias_integer"):
                wn.append(f"{name}.{buf}")
                wd.append(hashlib.sha256(getattr(mod, buf).numpy().astype(np.int32).tobytes()).hexdigest()[:16])
    out["wint_names"], out["wint_sha"] = np.array(wn), np.array(wd)
    if full:  # a few complete taps of image 0 for debugging kernels stage by stage
        for n in ["qact_input", "patch_embed.qact", "qact1", "blocks.0.qact1", "blocks.0.attn.qact1",
                  "blocks.0.attn.qact_attn1", "blocks.0.attn.int_softmax", "blocks.0.attn.qact2",
                  "blocks.0.attn.qact3", "blocks.0.qact2", "blocks.0.qact3", "blocks.0.mlp.qact_gelu",
                  "blocks.0.mlp.act", "blocks.0.mlp.qact1", "blocks.0.mlp.qact2", "blocks.0.qact4",
                  "blocks.11.qact4", "qact2"]:
            t = taps[n][:1]
            dt = np.int8 if np.abs(t).max() <= 127 and t.min() >= -128 else np.int16
            out["full/" + n] = t.astype(dt)
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; top1 = {top1.tolist()}")


def _import_swin():
    import types
    sys.modules.setdefault("tkinter", types.SimpleNamespace(X=None))                      # shim 2
    rq.IntLayerNorm, rq.IntSoftmax, rq.IntGELU = rq.IVITIntLayerNorm, rq.IVITIntSoftmax, rq.IVITIntGELU  # shim 3
    import models.swin_quant as sq
    return sq


SWIN_PLAN = {
    # tag: (factory, weight seed, calibration seed, calibration batch, image seed, n golden images)
    "swin_tiny": ("swin_tiny_patch4_window7_224", 21, 201, 2, 2001, 3),
    "swin_small": ("swin_small_patch4_window7_224", 22, 202, 2, 2002, 2),    # round 4 (swin_quant.py:588-606): 18 blocks in stage 2
}
SWIN_NATURAL_PLAN = {
    "swin_tiny_natural": ("swin_tiny_patch4_window7_224", 21, (201, 211), 2, 2001, 2),
    "swin_small_natural": ("swin_small_patch4_window7_224", 22, (202, 212), 2, 2002, 2),
}


def gen_swin(tag="swin_tiny"):
    if tag.endswith("_natural"):
        return gen_swin_natural(tag)
    return gen_swin_pow2(tag)


def gen_swin_natural(tag):
    """Swin-T with its ranges AS CALIBRATED (two batches, EMA), frozen: logits / top-1 / tap digests of the reference.
    There is no compat oracle for Swin; the fixture pins the mirror's module path (literal float kernels) and the fused engine on
    the GPU.  The patch-embed LayerNorm reduces over a transposed view (layers_quant.py:198-201): its exact-tie rows (counted
    into the meta record) are decided by ATen's outer-reduction order, which is deterministic at this batch -- the golden forward
    is repeated with 1 and with 4 threads and must give the same digests."""
    sq = _import_swin()
    factory, wseed, cseeds, cb, iseed, nimg = SWIN_NATURAL_PLAN[tag]
    model = getattr(sq, factory)(pretrained=False)
    for mod in model.modules():                                                            # shim 4
        if isinstance(mod, rq.QuantLinear) and mod.bias is None:
            mod.weight_function = lambda x, *a: None if x is None else SymmetricQuantFunction.apply(x, *a)
    fs = synth.make_swin_float_state(factory, wseed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    for cs in cseeds:
        model(torch.from_numpy(synth.make_images(cb, cs)))
    ranges, bitsof = {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct) and float(torch.max(-mod.x_min, mod.x_max)) > 0:
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
            bitsof[name] = mod.activation_bit
    ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            taps[name] = to_int(y, s)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, (rq.QuantAct, rq.IVITIntSoftmax, rq.IVITIntGELU)) and name != "act_out":
            mod.register_forward_hook(hook(name))
    cap = {}
    model.patch_embed.norm.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("ln_in", (inp[0].detach().clone(), inp[1].detach().clone(), inp[0].stride())))
    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    # the reference against itself: other thread counts, same digests (TensorIterator runs this reduction serially below 32768 outputs)
    first = {n: crc(t) for n, t in taps.items()}
    nthreads = torch.get_num_threads()
    for nt in (1, 4):
        torch.set_num_threads(nt)
        y2 = model(torch.from_numpy(imgs))
        assert torch.equal(y, y2) and all(first[n] == crc(taps[n]) for n in first), f"the reference differs from itself with {nt} threads"
    torch.set_num_threads(nthreads)
    xin, sin, strides = cap["ln_in"]
    assert strides[-1] != 1, "patch_embed.norm no longer sees a transposed view"
    rs = torch.round(xin / sin).to(torch.int64).sum(dim=2)
    Cn = xin.shape[2]
    tie_rows = int(((rs % Cn) == Cn // 2).sum())
    print(f"[{tag}] patch_embed.norm: input strides {tuple(strides)}, {tie_rows} of {rs.numel()} rows are exact ties of the mean")
    s_head = (model.head.fc_scaling_factor * model.qact3.act_scaling_factor).float()
    logits_int = torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32)
    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, weight_seed=wseed, calib_seeds=list(cseeds), calib_batch=cb,
                                         image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN, regime="natural",
                                         patch_norm_tie_rows=tie_rows, patch_norm_rows=int(rs.numel()),
                                         reproducible_with_threads=[1, 4, nthreads], torch=torch.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([bitsof[n] for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": logits_int, "logits_f32_bits": y.numpy().astype(np.float32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64),
        "head_scale": s_head.numpy().astype(np.float32),
        "tap_names": np.array(names), "tap_crc32": np.array([crc(taps[n]) for n in names], np.uint32),
    }
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; top1 = {out['top1'].tolist()}")


def gen_swin_pow2(tag="swin_tiny"):
    """Swin-T (config 5).  The fork's swin_quant.py is dead code (SURVEY finding 6); it runs with the three extra
    harness-side shims of SURVEY Appendix E (tkinter stub, Int* aliases, bias-free QuantLinear weight_function) --
    reference files untouched."""
    sq = _import_swin()
    factory, wseed, cseed, cb, iseed, nimg = SWIN_PLAN[tag]
    cfg = synth.SWIN_CONFIGS[factory]
    t0 = time.time()
    model = getattr(sq, factory)(pretrained=False)
    for mod in model.modules():                                                            # shim 4
        if isinstance(mod, rq.QuantLinear) and mod.bias is None:
            mod.weight_function = lambda x, *a: None if x is None else SymmetricQuantFunction.apply(x, *a)
    fs = synth.make_swin_float_state(factory, wseed)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    assert not unexpected, unexpected
    model.eval()
    model(torch.from_numpy(synth.make_images(cb, cseed)))
    ranges, bitsof = {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct):
            mx = float(torch.max(-mod.x_min, mod.x_max))
            if mx == 0.0:
                continue  # act_out: never called (swin_quant.py:518,563)
            q = 2 ** (mod.activation_bit - 1) - 1
            p = int(np.ceil(np.log2(mx / q)))
            mod.x_max.fill_(q * 2.0 ** p)
            mod.x_min.fill_(-q * 2.0 ** p)
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
            bitsof[name] = mod.activation_bit
    assert list(ranges) == synth.swin_qact_names(cfg["depths"]), "QuantAct order drifted"
    ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, s = outp
            taps[name] = to_int(y, s)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, (rq.QuantAct, rq.IVITIntSoftmax, rq.IVITIntGELU)) and name != "act_out":
            mod.register_forward_hook(hook(name))
    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact3.act_scaling_factor).float()
    logits_int = torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32)
    logits_f32 = y.numpy().astype(np.float32)
    top1 = y.argmax(dim=1).numpy().astype(np.int64)
    t_ref = time.time() - t0

    t1 = time.time()
    om = orc.OracleSwin(fs, ranges, cfg["embed_dim"], cfg["depths"], cfg["num_heads"], cfg["window"])
    otaps = {}
    res = om.forward(imgs, otaps)
    miss = [n for n in taps if n not in otaps]
    bad = [n for n in taps if n in otaps and not np.array_equal(taps[n].reshape(-1), otaps[n].reshape(-1))]
    print(f"[{tag}] reference {t_ref:.1f}s, oracle {time.time()-t1:.1f}s; taps {len(taps)}, missing in oracle {miss[:4]}, "
          f"differing {bad[:6]} ({len(bad)})")
    assert not miss and not bad
    assert np.array_equal(res["logits_int32"], logits_int), "INT32 logits differ"
    assert np.array_equal(res["logits_f32"].view(np.int32), logits_f32.view(np.int32))
    print(f"[{tag}] all taps + logits bit-equal; max|acc|={om.max_acc}, softmax rows sum>=2^24: "
          f"{om.softmax_inexact_rows}, LN rows |sum|>=2^24: {om.ln_big_sum_rows}")
    assert om.max_acc < 2 ** 24
    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, weight_seed=wseed, calib_seed=cseed, calib_batch=cb,
                                         image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN,
                                         max_abs_acc=om.max_acc, softmax_inexact_rows=om.softmax_inexact_rows,
                                         ln_big_sum_rows=om.ln_big_sum_rows, torch=torch.__version__,
                                         numpy=np.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([bitsof[n] for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": logits_int, "logits_f32_bits": logits_f32.view(np.int32), "top1": top1,
        "tap_names": np.array(names), "tap_crc32": np.array([crc(taps[n]) for n in names], np.uint32),
        "tap_absmax": np.array([int(np.abs(taps[n]).max()) for n in names], np.int64),
    }
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; top1 = {top1.tolist()}")



def gen_ibert_ops():
    """Known-answer vectors of the reference's I-BERT operator modules (ibert_modules.py), checked on the spot against
    oracle/ibert.py.  Inputs are integer activations with power-of-two scales (the regime of the parity contract)."""
    from oracle import ibert as ib
    rng = np.random.default_rng(20260202)
    out = {}
    gelu = rq.IBERTIntGELU()
    for i, p in enumerate((-2, -3, -4, -5, -6)):
        s = np.float32(2.0 ** p)
        k = rng.integers(-128, 128, size=(3, 5, 96)).astype(np.int32)
        k[0, 0, :4] = (-128, 127, 0, 1)
        y, so = gelu(torch.from_numpy((k.astype(np.float32) * s).astype(np.float32)), torch.tensor([s]))
        oi, s_o = ib.gelu(k, s)
        assert float(so) == float(s_o) and np.array_equal(y.numpy().view(np.int32), (oi * s_o).astype(np.float32).view(np.int32))
        out[f"gelu{i}_k"], out[f"gelu{i}_s"] = k.astype(np.int16), s
        out[f"gelu{i}_out"], out[f"gelu{i}_sout"] = oi.astype(np.int32), np.float32(s_o)
    sm = rq.IBERTIntSoftmax(8)
    for i, (p, L) in enumerate(((-2, 197), (-3, 197), (-1, 49), (0, 64), (-4, 33))):
        s = np.float32(2.0 ** p)
        k = rng.integers(-128, 128, size=(2, 3, 17, L)).astype(np.int32)
        k[0, 0, 0, :] = 5          # a constant row
        k[0, 0, 1, :] = -128
        k[0, 0, 1, 3] = 127        # one dominant key
        x = torch.from_numpy((k.astype(np.float32) * s).astype(np.float32))
        sm.act.running_stat = True
        sm.act.x_min.zero_()
        sm.act.x_max.zero_()
        sm(x, torch.tensor([s]))                      # first call initialises the internal QuantAct(16) range
        mx = float(torch.max(-sm.act.x_min, sm.act.x_max))
        pp = int(np.ceil(np.log2(mx / 32767.0)))
        if i == 4:                                    # one case with the raw (non power-of-two) calibrated range
            lo, hi = float(sm.act.x_min), float(sm.act.x_max)
        else:
            lo, hi = -32767.0 * 2.0 ** pp, 32767.0 * 2.0 ** pp
        sm.act.x_min.fill_(lo)
        sm.act.x_max.fill_(hi)
        sm.act.running_stat = False
        y, so = sm(x, torch.tensor([s]))
        o, s_o, ninx = ib.softmax(k, s, lo, hi)
        assert ninx == 0 and float(so) == float(s_o)
        assert np.array_equal(y.numpy().view(np.int32), (o * s_o).astype(np.float32).view(np.int32)), (i, p, L)
        out[f"softmax{i}_k"], out[f"softmax{i}_s"] = k.astype(np.int16), s
        out[f"softmax{i}_range"] = np.array([lo, hi], np.float32)
        out[f"softmax{i}_out"] = o.astype(np.int32)
    for i, (C, amp, p) in enumerate(((192, 30, -4), (384, 60, -3), (768, 20, -5), (96, 127, -2))):
        ln = rq.IBERTIntLayerNorm(C)
        ln.weight.data = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32))
        ln.bias.data = torch.from_numpy((rng.standard_normal(C) * 0.1).astype(np.float32))
        ln.fix()
        s = np.float32(2.0 ** p)
        k = np.clip(np.rint(rng.normal(0, amp, size=(2, 9, C))), -128, 127).astype(np.int32)
        k[0, 0, :] = 3                                 # constant row: var = 0 -> std = 0 -> factor = inf (as the reference)
        y, so = ln(torch.from_numpy((k.astype(np.float32) * s).astype(np.float32)), torch.tensor([s]))
        yi, s_o, ninx = ib.layernorm(k, s, ln.weight.numpy(), ln.bias.numpy())
        assert ninx == 0 and np.array_equal(so.numpy(), s_o)
        mine = (yi * s_o).astype(np.float32)
        assert np.array_equal(y.numpy().view(np.int32), mine.view(np.int32)), (i, C)
        out[f"ln{i}_k"], out[f"ln{i}_s"] = k.astype(np.int16), s
        out[f"ln{i}_gamma"], out[f"ln{i}_beta"] = ln.weight.numpy().copy(), ln.bias.numpy().copy()
        out[f"ln{i}_out_bits"] = y.numpy().view(np.int32).copy()
        out[f"ln{i}_sout"] = s_o
    np.savez_compressed(os.path.join(GOLD, "ibert_kat.npz"), **out)
    print("ibert_kat.npz written:", len(out), "arrays; oracle/ibert.py bit-equal to the reference modules on all cases")



# ----------------------------------------------------------------------------- natural (un-snapped) calibration ranges

NATURAL_PLAN = {
    # tag: (factory, weight seed, calibration seeds (one batch each, EMA as quant_modules.py:346-360), batch, image seed, n)
    "deit_tiny_natural": ("deit_tiny_patch16_224", 11, (101, 111, 121), 4, 1001, 8),
    "deit_small_natural": ("deit_small_patch16_224", 12, (102, 112), 4, 1002, 4),
    "deit_base_natural": ("deit_base_patch16_224", 13, (103, 113), 2, 1003, 2),
    "vit_large_natural": ("vit_large_patch16_224", 15, (105, 115), 2, 1005, 2),
}


def gen_natural(tag):
    """The reference with its QuantAct ranges AS CALIBRATED (running min/max + EMA over a few batches, then freeze) -- the
    regime of a real checkpoint (scripts/inference.py:33-91, quant_train.py:470-500), where every activation scale is an
    arbitrary float32.  Stores the reference's logits / top-1 / tap digests plus, per tap, how far the integer-exact
    algorithm (oracle/oracle.py, = the HIP engine) is from it: the reference's own `fl(fl(k*s)/s)` fuzz at its float ->
    integer conversions (SURVEY finding 8) makes them differ, and this fixture is what quantifies it."""
    factory, wseed, cseeds, cb, iseed, nimg = NATURAL_PLAN[tag]
    cfg = synth.MODEL_CONFIGS[factory]
    model = getattr(ref_models, factory)(pretrained=False, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit")
    fs = synth.make_float_state(factory, wseed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    for cs in cseeds:
        model(torch.from_numpy(synth.make_images(cb, cs)))
    ranges = {n: (np.float32(m.x_min.item()), np.float32(m.x_max.item()))
              for n, m in model.named_modules() if isinstance(m, rq.QuantAct)}
    ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, sc = outp
            taps[name] = to_int(y, sc)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, (rq.QuantAct, rq.IVITIntSoftmax, rq.IVITIntGELU)):
            mod.register_forward_hook(hook(name))
    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact2.act_scaling_factor).float()
    logits_int = torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32)
    logits_f32 = y.numpy().astype(np.float32)
    top1 = y.argmax(dim=1).numpy().astype(np.int64)

    # ---- the natural-scale restatement (oracle compat=True) must reproduce the reference bit for bit
    oc = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], compat=True)
    ctaps = {}
    cres = oc.forward(imgs, ctaps)
    cbad = [n for n in taps if not np.array_equal(taps[n].reshape(-1), ctaps[n].reshape(-1))]
    assert not cbad, f"compat oracle != reference at {cbad[:5]} ({len(cbad)} taps)"
    assert np.array_equal(cres["logits_int32"], logits_int), "compat oracle: INT32 logits differ"
    # the reference's float logits are F.linear over phi(q) (quant_modules.py:222-226): sgemm over near-integers, equal to
    # acc * scale only up to its own float32 accumulation -- INT32 logits and top-1 are the contract (BASELINE north_star)
    ulp = np.abs(cres["logits_f32"].view(np.int32).astype(np.int64) - logits_f32.view(np.int32)).max()
    err = float(np.abs(cres["logits_f32"] - logits_f32).max() / float(cres["head_scale"].max()))
    assert err < 0.25, f"compat oracle: float logits off by {err} integer steps"
    assert np.array_equal(cres["top1"], top1)
    print(f"[{tag}] float logits: max {ulp} ulp / {err:.4f} integer steps from the reference's sgemm-over-phi values")
    print(f"[{tag}] compat oracle: {len(taps)} taps + INT32 logits + top-1 bit-equal to the reference "
          f"({oc.ln_tie_rows} LayerNorm rows decided by the float32 reduction order, "
          f"{oc.softmax_inexact_rows} Shiftmax rows with sum >= 2^24, max|acc| {oc.max_acc})")
    assert oc.max_acc < 2 ** 24

    # ---- for the record: how far the plain integer algorithm (compat=False) is from the reference at these scales
    om = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"])
    otaps = {}
    res = om.forward(imgs, otaps)
    order = synth.qact_names(cfg["depth"])
    names = sorted(taps)
    frac = {n: float(np.mean(taps[n].reshape(-1) != otaps[n].reshape(-1))) for n in names}
    maxd = {n: int(np.abs(taps[n].reshape(-1).astype(np.int64) - otaps[n].reshape(-1)).max()) for n in names}
    first = next((n for n in order if frac.get(n, 0.0) > 0), None)
    agree = int((res["top1"] == top1).sum())
    lg_equal = bool(np.array_equal(res["logits_int32"], logits_int))
    rel = float(np.abs(res["logits_f32"] - logits_f32).max() / np.abs(logits_f32).max())
    print(f"[{tag}] plain integer algorithm (no phi) vs reference at natural scales: taps equal {sum(f == 0 for f in frac.values())}/"
          f"{len(names)}, first differing QuantAct {first}, worst tap {max(frac.values()):.4f} of elements, "
          f"INT32 logits equal: {lg_equal}, max |dlogit|/max|logit| {rel:.4f}, top-1 agreement {agree}/{nimg}")
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, family="ivit", weight_seed=wseed, calib_seeds=list(cseeds),
                                         calib_batch=cb, image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN,
                                         regime="natural", first_differing_tap=first, top1_agreement=agree,
                                         logits_int32_equal=lg_equal, logits_rel_err=rel, ln_tie_rows=oc.ln_tie_rows,
                                         softmax_inexact_rows=oc.softmax_inexact_rows, max_abs_acc=oc.max_acc,
                                         torch=torch.__version__, cpu_capability=torch.backends.cpu.get_cpu_capability()))),
        "range_names": np.array(list(ranges)),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": logits_int, "logits_f32_bits": logits_f32.view(np.int32), "top1": top1,
        "tap_names": np.array(names), "tap_crc32": np.array([crc(taps[n]) for n in names], np.uint32),
        "exact_mismatch_frac": np.array([frac[n] for n in names], np.float64),
        "exact_mismatch_maxabs": np.array([maxd[n] for n in names], np.int64),
    }
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; reference top1 = {top1.tolist()}, integer-exact top1 = {res['top1'].tolist()}")
    return taps, otaps, ranges, fs, imgs



def gen_compat_ops():
    """Known-answer vectors of the reference's I-ViT operator modules at NATURAL (non power-of-two) input scales: the input
    is what a QuantAct emits, q * s in float32 (quant_modules.py:387).  Checked on the spot against the compat oracle."""
    rng = np.random.default_rng(20260303)
    out = {}
    scales = [np.float32(v) for v in (0.0371, 0.11873, 0.0052341, 0.3127, 0.0625)]
    # --- IVITIntLayerNorm (+ the QuantAct behind it, natural output range)
    for ci, (rows, Cn, s) in enumerate([(48, 192, scales[0]), (32, 768, scales[1]), (24, 384, scales[2]), (16, 96, scales[3]),
                                        (16, 1024, scales[0])]):
        ln = rq.IVITIntLayerNorm(Cn)
        gamma = rng.uniform(0.5, 1.5, size=Cn).astype(np.float32)
        beta = rng.normal(0, 0.1, size=Cn).astype(np.float32)
        ln.weight.data, ln.bias.data = torch.from_numpy(gamma), torch.from_numpy(beta)
        q = rng.integers(-128, 128, size=(1, rows, Cn)).astype(np.int32)
        for r in range(0, rows, 2):            # every other row: integer sum == C/2 (mod C), the mean is an exact .5 tie
            tgt = Cn // 2 + Cn * int(rng.integers(-20, 20))
            for _ in range(100000):
                d = tgt - int(q[0, r].sum())
                if d == 0:
                    break
                c = int(rng.integers(0, Cn))
                nv = int(np.clip(q[0, r, c] + np.clip(d, -60, 60), -128, 127))
                q[0, r, c] = nv
            assert int(q[0, r].sum()) == tgt
        x = (torch.from_numpy(q.astype(np.float32)) * torch.tensor([s])).float()
        yl, sl = ln(x, torch.tensor([s]))
        qa = rq.QuantAct()
        hi = float(np.abs(yl.numpy()).max()) * 0.93
        qa.x_min.fill_(-hi)
        qa.x_max.fill_(hi)
        qa.fix()
        yq, sq = qa(yl, sl)
        y, s_ln, _, ties = orc.layernorm_compat(q.reshape(rows, Cn), s, gamma, beta)
        assert np.array_equal((y * s_ln).astype(np.float32).view(np.int32), yl.numpy().reshape(rows, Cn).view(np.int32)), ci
        assert ties >= rows // 2
        c = f"ln{ci}_"
        out[c + "q"], out[c + "s"] = q.reshape(rows, Cn).astype(np.int8), s
        out[c + "gamma"], out[c + "beta"] = gamma, beta
        out[c + "y_bits"] = yl.numpy().reshape(rows, Cn).view(np.int32)
        out[c + "range"] = np.array([-hi, hi], np.float32)
        out[c + "q_out"] = torch.round(yq / sq).numpy().reshape(rows, Cn).astype(np.int32)
    out["ln_cases"] = np.arange(5, dtype=np.int32)
    # --- IVITIntGELU
    for ci, (rows, L, s) in enumerate([(16, 768, scales[0]), (8, 3072, scales[1]), (8, 1536, scales[2]), (8, 256, scales[3])]):
        g = rq.IVITIntGELU()
        q = rng.integers(-128, 128, size=(1, rows, L)).astype(np.int32)
        if ci == 3:
            q[0, :, :] = np.arange(-128, 128)
        yg, sg = g((torch.from_numpy(q.astype(np.float32)) * torch.tensor([s])).float(), torch.tensor([s]))
        ref = torch.round(yg / sg).numpy().reshape(rows, L).astype(np.int32)
        mine, _ = orc.shiftgelu_compat(q.reshape(rows, L), s)
        assert np.array_equal(mine, ref), ci
        c = f"gelu{ci}_"
        out[c + "q"], out[c + "s"], out[c + "out"] = q.reshape(rows, L).astype(np.int8), s, ref
    out["gelu_cases"] = np.arange(4, dtype=np.int32)
    # --- IVITIntSoftmax
    for ci, (rows, L, s, sd) in enumerate([(64, 197, scales[3], 30), (64, 197, scales[1], 50), (32, 49, np.float32(0.271), 25),
                                           (16, 197, np.float32(0.9113), 8), (16, 64, scales[0], 60)]):
        sm = rq.IVITIntSoftmax()
        q = np.clip(np.rint(rng.normal(0, sd, size=(1, 1, rows, L))), -128, 127).astype(np.int32)
        q[0, 0, 0, :] = 7
        q[0, 0, 1, :] = -128
        q[0, 0, 1, 3] = 127
        ys, ss = sm((torch.from_numpy(q.astype(np.float32)) * torch.tensor([s])).float(), torch.tensor([s]))
        ref = torch.round(ys / ss).numpy().reshape(rows, L).astype(np.int32)
        mine = orc.shiftmax_compat(q.reshape(rows, L), s)
        assert np.array_equal(mine, ref), ci
        c = f"sm{ci}_"
        out[c + "q"], out[c + "s"], out[c + "out"] = q.reshape(rows, L).astype(np.int8), s, ref
    out["sm_cases"] = np.arange(5, dtype=np.int32)
    # --- IVITIntLayerNorm on a 16-bit stream at a natural scale (Swin's residual stream)
    for ci, (rows, Cn, s) in enumerate([(24, 96, np.float32(0.000913)), (16, 384, np.float32(0.0004471)), (12, 768, np.float32(0.00171))]):
        ln = rq.IVITIntLayerNorm(Cn)
        gamma = rng.uniform(0.5, 1.5, size=Cn).astype(np.float32)
        beta = rng.normal(0, 0.1, size=Cn).astype(np.float32)
        ln.weight.data, ln.bias.data = torch.from_numpy(gamma), torch.from_numpy(beta)
        q = np.clip(np.rint(rng.normal(0, 6000, size=(1, rows, Cn))), -32768, 32767).astype(np.int32)
        for r in range(0, rows, 2):            # every other row: an exact .5 tie of the mean
            tgt = Cn // 2 + Cn * int(rng.integers(-200, 200))
            for _ in range(100000):
                d = tgt - int(q[0, r].sum())
                if d == 0:
                    break
                c = int(rng.integers(0, Cn))
                q[0, r, c] = int(np.clip(q[0, r, c] + np.clip(d, -5000, 5000), -32768, 32767))
            assert int(q[0, r].sum()) == tgt
        x = (torch.from_numpy(q.astype(np.float32)) * torch.tensor([s])).float()
        yl, sl = ln(x, torch.tensor([s]))
        qa = rq.QuantAct()
        hi = float(np.abs(yl.numpy()).max()) * 0.93
        qa.x_min.fill_(-hi)
        qa.x_max.fill_(hi)
        qa.fix()
        yq, sq = qa(yl, sl)
        y, s_ln, _ = orc.layernorm_scaled(q.reshape(rows, Cn), s, gamma, beta)
        assert np.array_equal((y * s_ln).astype(np.float32).view(np.int32), yl.numpy().reshape(rows, Cn).view(np.int32)), ci
        c = f"ln16_{ci}_"
        out[c + "q"], out[c + "s"] = q.reshape(rows, Cn).astype(np.int16), s
        out[c + "gamma"], out[c + "beta"] = gamma, beta
        out[c + "range"] = np.array([-hi, hi], np.float32)
        out[c + "q_out"] = torch.round(yq / sq).numpy().reshape(rows, Cn).astype(np.int32)
    out["ln16_cases"] = np.arange(3, dtype=np.int32)
    # --- IVITIntSoftmax behind Swin's shift mask: x = q*s + mask, mask in {0, -100.0} (swin_quant.py:151-156)
    for ci, (rows, L, s, sd) in enumerate([(49, 49, np.float32(0.271), 30), (49, 49, np.float32(0.1173), 45), (49, 49, np.float32(1.3), 20)]):
        sm = rq.IVITIntSoftmax()
        q = np.clip(np.rint(rng.normal(0, sd, size=(1, 1, rows, L))), -128, 127).astype(np.int32)
        mask = (rng.random(size=(rows, L)) < 0.35)
        mask[np.arange(rows), np.arange(L)] = False                      # a token always attends to itself
        mf = np.where(mask, np.float32(-100.0), np.float32(0.0)).astype(np.float32)
        x = (torch.from_numpy(q.astype(np.float32)) * torch.tensor([s])).float() + torch.from_numpy(mf)[None, None]
        ys, ss = sm(x, torch.tensor([s]))
        ref = torch.round(ys / ss).numpy().reshape(rows, L).astype(np.int32)
        xint = (x / torch.tensor([s])).numpy().reshape(rows, L).astype(np.float32)
        assert np.array_equal(orc.shiftmax_xint(xint, s), ref), ci
        c = f"smm{ci}_"
        out[c + "q"], out[c + "s"], out[c + "mask"], out[c + "out"] = q.reshape(rows, L).astype(np.int8), s, mask, ref
    out["smm_cases"] = np.arange(3, dtype=np.int32)
    np.savez_compressed(os.path.join(GOLD, "compat_kat.npz"), **out)
    print("compat_kat.npz written:", len(out), "arrays; compat oracle bit-equal to the reference modules on all cases")



W16 = dict(patch_embed_bw=16, pos_encoding_bw=8, block_input_bw=16, attention_out_bw=16, softmax_bw=8, mlp_out_bw=16,
           norm2_in_bw=16, att_block_out_bw=16)


W16_ALL = dict(patch_embed_bw=16, pos_encoding_bw=16, block_input_bw=16, attention_out_bw=16, softmax_bw=16, mlp_out_bw=16,
               norm2_in_bw=16, att_block_out_bw=16)       # what `--bitwidth 16` sets (quant_train.py:299-306)


def gen_w16(tag="deit_tiny_w16"):
    """DeiT-T with the reference's width knobs (vit_quant.py:180-187, quant_train.py:295-306) at 16 bits for the residual
    stream and the QuantActs in front of it (softmax and the position embedding stay 8 bit): logits of the reference only.
    The fused int8 engine does not implement these widths; the mirror must route such a model to its module path."""
    factory, wseed, cseed, cb, iseed, nimg = "deit_tiny_patch16_224", 11, 101, 4, 1001, 4
    widths = W16_ALL if tag.endswith("_w16all") else W16
    model = getattr(ref_models, factory)(pretrained=False, gelu_type="ivit", softmax_type="ivit", layernorm_type="ivit", **widths)
    fs = synth.make_float_state(factory, wseed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    model(torch.from_numpy(synth.make_images(cb, cseed)))
    ranges, bits = {}, {}
    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct):
            mx = float(torch.max(-mod.x_min, mod.x_max))
            q = float(2 ** (mod.activation_bit - 1) - 1)
            p = int(np.ceil(np.log2(mx / q)))
            mod.x_max.fill_(q * 2.0 ** p)
            mod.x_min.fill_(-q * 2.0 ** p)
            ranges[name] = (np.float32(mod.x_min.item()), np.float32(mod.x_max.item()))
            bits[name] = int(mod.activation_bit)
    ref_models.freeze_model(model)
    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, family="ivit", weight_seed=wseed, calib_seed=cseed,
                                         calib_batch=cb, image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN,
                                         widths=widths, torch=torch.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([bits[n] for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_f32_bits": y.numpy().astype(np.float32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64),
    }
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; 16-bit QuantActs: {sum(b == 16 for b in bits.values())} of {len(bits)}; top1 = {out['top1'].tolist()}")



def gen_ibert_natural(tag="deit_tiny_ibert_natural"):
    """DeiT-T with the fork's DEFAULT operator family (I-BERT, vit_quant.py:188-190) and its ranges AS CALIBRATED: the
    reference's logits / top-1 / tap digests.  No CPU oracle restates I-BERT at natural scales; the fixture pins the mirror's
    module path (literal float kernels of csrc/ibert.hip) on the GPU.
    tag deit_tiny_ibert_w16all: the same with every width knob at 16 (the authors' INT16 runs, .vscode/launch.json:104-200,
    quant_train.py:299-306): 16-bit residual stream, 16-bit IBERTIntSoftmax output (p reaches 2^15) into P.V, 16-bit pos_embed."""
    factory, wseed, cseeds, cb, iseed, nimg = "deit_tiny_patch16_224", 11, (101, 111), 4, 1001, 2
    widths = W16_ALL if tag.endswith("_w16all") else {}
    model = getattr(ref_models, factory)(pretrained=False, gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert", **widths)
    fs = synth.make_float_state(factory, wseed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    for cs in cseeds:
        model(torch.from_numpy(synth.make_images(cb, cs)))
    ranges = {n: (np.float32(m.x_min.item()), np.float32(m.x_max.item()))
              for n, m in model.named_modules() if isinstance(m, rq.QuantAct)}
    shifts = {n: float(m.shift) for n, m in model.named_modules() if isinstance(m, rq.IBERTIntLayerNorm)}
    ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            y, sc = outp
            taps[name] = to_int(y, sc)
        return fn

    for name, mod in model.named_modules():
        if isinstance(mod, rq.QuantAct) and not name.endswith("int_softmax.act"):
            mod.register_forward_hook(hook(name))
    imgs = synth.make_images(nimg, iseed)
    y = model(torch.from_numpy(imgs))
    s_head = (model.head.fc_scaling_factor * model.qact2.act_scaling_factor).float()
    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, family="ibert", weight_seed=wseed, calib_seeds=list(cseeds),
                                         calib_batch=cb, image_seed=iseed, n_images=nimg, qkv_gain=synth.QKV_GAIN,
                                         regime="natural", ln_shifts=shifts, widths=widths, torch=torch.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([int(dict(model.named_modules())[n].activation_bit) for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], np.float32),
        "x_max": np.array([v[1] for v in ranges.values()], np.float32),
        "logits_int32": torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32),
        "logits_f32_bits": y.numpy().astype(np.float32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64), "head_scale": s_head.numpy().astype(np.float32),
        "tap_names": np.array(names), "tap_crc32": np.array([crc(taps[n]) for n in names], np.uint32),
    }
    np.savez_compressed(os.path.join(GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; LayerNorm shifts {sorted(set(shifts.values()))}; top1 = {out['top1'].tolist()}")


CALIB_TRACE_PLAN = {
    # tag: (factory, operator family, weight seed, calibration seeds, calibration batch) -- the plans of the *_natural fixtures
    "deit_tiny_natural": ("deit_tiny_patch16_224", "ivit", 11, (101, 111, 121), 4),
    "deit_small_natural": ("deit_small_patch16_224", "ivit", 12, (102, 112), 4),
    "deit_tiny_ibert_natural": ("deit_tiny_patch16_224", "ibert", 11, (101, 111), 4),
}


def gen_calib_trace():
    """The reference's calibration, step by step (quant_modules.py:310-360; scripts/inference.py:33-91 runs exactly these
    forwards): for every calibration batch and every QuantAct, the raw (min, max) it observed over its float input and the range
    it held after its update (first batch: initialise; later: EMA with momentum 0.95).  tests/golden/calib_trace.npz; the GPU
    test drives the module mirror through the same batches with each QuantAct forced to the reference's post-update range, so
    that both sides quantise alike, and compares what the mirror OBSERVES and what its update rule MAKES of the observation."""
    out = {}
    for tag, (factory, fam, wseed, cseeds, cb) in CALIB_TRACE_PLAN.items():
        model = getattr(ref_models, factory)(pretrained=False, gelu_type=fam, softmax_type=fam, layernorm_type=fam)
        fs = synth.make_float_state(factory, wseed)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
        model.eval()
        qacts = [(n, m) for n, m in model.named_modules() if isinstance(m, rq.QuantAct)]
        raw, post, order = {}, {}, []

        def pre(name):
            def fn(mod, args, kwargs):
                x = args[0]
                identity = args[2] if len(args) > 2 else kwargs.get("identity")
                xa = x if identity is None else identity + x                     # quant_modules.py:310
                raw.setdefault(name, []).append((float(xa.data.min()), float(xa.data.max())))
                if name not in order:
                    order.append(name)
            return fn

        def after(name):
            def fn(mod, args, outp):
                post.setdefault(name, []).append((float(mod.x_min), float(mod.x_max)))
            return fn

        for n, m in qacts:
            m.register_forward_pre_hook(pre(n), with_kwargs=True)
            m.register_forward_hook(after(n))
        for cs in cseeds:
            model(torch.from_numpy(synth.make_images(cb, cs)))
        names = [n for n, _ in qacts]
        assert set(order) == set(names) and all(len(raw[n]) == len(cseeds) for n in names)
        z = np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=True)
        assert names == [str(x) for x in z["range_names"]]
        fin = np.array([post[n][-1] for n in names], np.float32)
        assert np.array_equal(fin[:, 0], z["x_min"]) and np.array_equal(fin[:, 1], z["x_max"]), "trace != the fixture's final ranges"
        out[tag + "/names"] = np.array(names)
        out[tag + "/call_order"] = np.array(order)
        out[tag + "/raw"] = np.array([[raw[n][b] for n in names] for b in range(len(cseeds))], np.float32)      # [batch, qact, 2]
        out[tag + "/post"] = np.array([[post[n][b] for n in names] for b in range(len(cseeds))], np.float32)
        out[tag + "/meta"] = np.array(json.dumps(dict(factory=factory, family=fam, weight_seed=wseed, calib_seeds=list(cseeds),
                                                      calib_batch=cb, momentum=0.95, torch=torch.__version__)))
        if fam == "ibert":
            lns = [(n, m) for n, m in model.named_modules() if isinstance(m, rq.IBERTIntLayerNorm)]
            out[tag + "/ln_names"] = np.array([n for n, _ in lns])
            out[tag + "/ln_shift"] = np.array([float(m.shift) for _, m in lns], np.float32)
        print(f"[calib_trace] {tag}: {len(names)} QuantActs x {len(cseeds)} batches")
    np.savez_compressed(os.path.join(GOLD, "calib_trace.npz"), **out)


BIGSUM_LENGTHS = (49, 144, 197, 208, 577, 1025)
BIGSUM_SCALES = ((0.25, -4), (0.125, -8), (0.2113, -5), (0.11873, -9), (0.0571, -18))      # (s, x0): two pow2, three natural
BIGSUM_SCALES_49 = ((0.0625, -16),)      # 49 keys reach 2^24 only from |x0| = 11 on: one more pow2 scale, for the window entries


def _bigsum_boundary(smo, f):
    """the two adjacent float32 S1 < S2 with factor(S1) = f and factor(S2) = f - 1"""
    S = np.float32(2.0 ** 31 / f)
    for _ in range(4):
        S = np.nextafter(S, np.float32(0))
    for _ in range(16):
        S2 = np.nextafter(S, np.float32(np.inf))
        if smo.factor_of(S) == f and smo.factor_of(S2) == f - 1:
            return int(S), int(S2)
        S = S2
    return None


def _bigsum_multiset(rng, E, T, lo, hi, force):
    """distances from the row maximum, one per key, whose exponents E[dist] sum to a value in (lo, hi), as near the middle as
    the far keys' small terms allow.  Most keys lie within 3 steps of the maximum; about 12-15 % (more where the target sum is
    small) lie far below and make the fine adjustment.  force: a distance that at least a tenth of the near keys take."""
    mid = (lo + hi) // 2
    near = np.arange(4) if force is None else np.unique(np.append(np.arange(4), force))
    n_far = max(3, int(round(T * rng.uniform(0.12, 0.15))))
    e_near = float(np.mean(E[near]))
    if (T - n_far) * e_near > mid:                                     # a small target: fewer near keys
        n_far = T - int(mid / e_near)
    n_near = T - n_far
    if n_near < 1 or n_far < 3 or n_near * int(E[0]) + n_far * int(E[4]) < mid:
        return None
    d = rng.choice(near, size=n_near)
    d[0] = 0                                                           # the row maximum itself
    if force is not None:
        d[1:1 + max(1, n_near // 10)] = force
    # coarse: move near keys one step until what is left for the far keys is something they can make
    want_lo, want_hi = n_far * 64, (n_far - 2) * int(E[4]) // 2 + 1
    for _ in range(20 * T):
        rest = mid - int(E[d].sum())
        if want_lo <= rest <= want_hi:
            break
        i = int(rng.integers(1, n_near)) if n_near > 1 else 0
        if force is not None and i < 1 + max(1, n_near // 10):
            continue
        if rest < want_lo and d[i] < 3:
            d[i] += 1
        elif rest > want_hi and d[i] > 0 and i > 0:
            d[i] -= 1
    rest = mid - int(E[d].sum())
    if not want_lo <= rest <= want_hi:
        return None
    far_d = np.arange(4, len(E))
    far = []
    e_min = int(E[far_d].min())
    for k in range(n_far - 2):
        left = n_far - 1 - k                                           # keys still to come after this one; each adds e_min at least
        room = rest - 3 * e_min * left
        if left > 12:                                                  # the first: near the even share, with some spread
            want = min(room, rest / (left + 1) * rng.uniform(0.6, 1.4))
        else:                                                          # the last ten: the largest term that still fits
            want = room
        fits = far_d[E[far_d] <= max(want, e_min)]
        j = int(fits[np.argmax(E[fits])])
        far.append(j)
        rest -= int(E[j])
    pair = E[far_d][:, None] + E[far_d][None, :]                       # the last two: every pair of far distances
    a, b = np.unravel_index(np.argmin(np.abs(pair - rest)), pair.shape)
    far += [int(far_d[a]), int(far_d[b])]
    d = np.concatenate([d, np.array(far)])
    return d if lo < int(E[d].sum()) < hi else None


def gen_shiftmax_bigsum():
    """tests/golden/shiftmax_bigsum_kat.npz: IVITIntSoftmax on rows whose exponent sum reaches 2^24, where the float32 sum
    (ivit_modules.py:171) depends on the order of torch's CPU kernel.  Stored per row: the int8 scores, the scale, output_bit,
    the REFERENCE's output, the output that the exact sum rounded once would give, and the row's class (tests/shiftmax_order_ref.py:
    a = order-free, b = the sums differ but not the outputs, c = the outputs differ).  Class (c) rows come from a seeded, directed
    search: a near-flat multiset of scores tuned until its exact sum lies between the two float32 neighbours of a boundary
    2^31 / f, then permuted until the two sums fall on either side of it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shiftmax_order_ref as smo
    rng = np.random.default_rng(20261020)
    t_start = time.time()
    recs = {T: [] for T in BIGSUM_LENGTHS}                             # T -> [(q int8 [T], s, bits, cls, out_torch, out_exact)]

    def take(T, q, s, bits, want, limit):
        """classify the rows q [N, T]; keep up to `limit` rows of class `want` -> number kept"""
        cls, ot, oe = smo.classify(q, s, bits)
        idx = np.flatnonzero(cls == want)[:limit]
        for i in idx:
            recs[T].append((q[i].astype(np.int8), np.float32(s), bits, want, ot[i], oe[i]))
        return len(idx)

    notes = {}
    for T in BIGSUM_LENGTHS:
        for s, x0 in BIGSUM_SCALES + (BIGSUM_SCALES_49 if T == 49 else ()):
            s = np.float32(s)
            assert smo.x0_of(s) == x0
            assert T > 208 or T * abs(x0) * 2 ** 15 < 2 ** 32           # the short entries' bound on the row sum
            qmax = 127
            E = smo.shiftexp(smo.phi_table(s)[::-1] - smo.phi_table(s)[qmax + 128], x0).astype(np.int64)   # E[dist], dist = 0 .. 255
            s_hi = (T - 3) * int(E[0])
            if s_hi < 1 << 24:
                notes[f"T{T}_x0{x0}"] = "no row reaches 2^24"
                continue
            # ---- class (a): every key within a few steps of the maximum; (b): near-flat with far keys, as drawn
            for bits in (8, 16):
                for qm in (127, 120, 112, 96, 64, 33, 0):                # natural scales: a maximum whose neighbours phi leaves whole
                    qa = (qm - rng.integers(0, 4, size=(64, T))).astype(np.int64)
                    qa[:, 0] = qm
                    if take(T, qa, s, bits, smo.CLASS_A, 2 if T == 49 else 1):
                        break
                qb = (qmax - rng.integers(0, 4, size=(256, T))).astype(np.int64)
                far = rng.random(size=qb.shape) < 0.135
                qb[far] = qmax - rng.integers(40, 256, size=int(far.sum()))
                qb[:, 0] = qmax
                take(T, qb, s, bits, smo.CLASS_B, 1)
            # ---- class (c), directed: for a factor f, a multiset whose exact sum lies between the float32 neighbours of 2^31 / f
            f_lo = max(2, int(np.ceil(2.0 ** 31 / s_hi)) + 1)
            found = {8: 0, 16: 0}
            fs = list(range(f_lo, 128))
            rng.shuffle(fs)
            # factors at which some near key's 8-bit output changes come first: they can give class (c) at 8 bits
            d8 = {}
            for f in fs:
                chg = np.flatnonzero((E[:24] * f >> 24) != (E[:24] * (f - 1) >> 24))
                if len(chg):
                    d8[f] = int(chg[0])
            fs.sort(key=lambda f: f not in d8)
            for f in fs:
                if found[16] >= 4 and (found[8] >= 2 or f not in d8):
                    continue
                if time.time() - t_start > 1500:
                    break
                bd = _bigsum_boundary(smo, f)
                if bd is None:
                    continue
                for attempt in range(6):
                    d = _bigsum_multiset(rng, E, T, bd[0], bd[1], d8.get(f) if attempt % 2 == 0 else None)
                    if d is None:
                        continue
                    q = qmax - np.stack([rng.permutation(d) for _ in range(192)])    # the key order changes torch's sum only
                    got = 0
                    if found[8] < 2 and f in d8:
                        got = take(T, q, s, 8, smo.CLASS_C, 1)
                        found[8] += got
                    if not got and found[16] < 4:
                        found[16] += take(T, q, s, 16, smo.CLASS_C, 1)
                    if found[16] >= 4 and (found[8] >= 2 or f not in d8):
                        break
            notes[f"T{T}_x0{x0}"] = f"class c: {found[16]} rows at 16 bits, {found[8]} at 8"
            print(f"[bigsum] T={T} x0={x0}: {notes[f'T{T}_x0{x0}']}  ({time.time() - t_start:.0f} s)", flush=True)

    # ---- the reference itself on every row; the restatement must agree with it, sum and output
    out = {}
    counts = {}
    for T in BIGSUM_LENGTHS:
        R = recs[T]
        q = np.stack([r[0] for r in R])
        sc = np.array([r[1] for r in R], np.float32)
        bits = np.array([r[2] for r in R], np.int32)
        cls = np.array([r[3] for r in R], np.uint8)
        ot = np.stack([r[4] for r in R])
        oe = np.stack([r[5] for r in R])
        ref = np.empty_like(ot)
        for s in np.unique(sc):
            for b in (8, 16):
                m = np.flatnonzero((sc == s) & (bits == b))
                if not len(m):
                    continue
                sm = rq.IVITIntSoftmax(output_bit=b)
                st = torch.tensor([s])
                x = (torch.from_numpy(q[m].astype(np.float32))[None, None] * st).float()
                ys, ss = sm(x, st)
                ref[m] = torch.round(ys / ss).numpy().reshape(len(m), T).astype(np.int32)
                xi = x / st
                ex, _ = sm.int_exp_shift(xi - xi.max(dim=-1, keepdim=True)[0], st)
                ef = smo.exponents(q[m], s)
                assert np.array_equal(ex.numpy().reshape(len(m), T), ef)
                St, Se, isum = smo.both_sums(ef)
                assert np.array_equal(ex.sum(dim=-1).numpy().reshape(-1), St), "torch's sum is not the restated order"
                assert np.all(isum >= 1 << 24)
        assert np.array_equal(ref, ot), "the reference's output is not the restatement's"
        for c in (smo.CLASS_A, smo.CLASS_B, smo.CLASS_C):
            for b in (8, 16):
                counts[f"T{T}_{smo.CLASS_NAMES[c]}{b}"] = int(((cls == c) & (bits == b)).sum())
        pow2 = np.isin(sc, [np.float32(0.25), np.float32(0.125), np.float32(0.0625)])
        if T >= 144:
            assert ((cls == smo.CLASS_C) & (bits == 16) & pow2).sum() >= 4 and ((cls == smo.CLASS_C) & (bits == 16) & ~pow2).sum() >= 4, T
            assert (cls == smo.CLASS_A).sum() >= 4 and (cls == smo.CLASS_B).sum() >= 4, T
        else:
            assert (cls == smo.CLASS_A).sum() >= 4, T
            if not (cls != smo.CLASS_A).any():
                notes[f"T{T}"] = "class (a) only: the search found no row here whose two sums differ"
        assert np.all(np.any(ref != oe, axis=1) == (cls == smo.CLASS_C))
        assert ref.min() >= 0 and ref.max() <= 32768 and np.abs(oe - ref).max() < 32768
        out[f"q_{T}"], out[f"s_{T}"], out[f"bits_{T}"], out[f"cls_{T}"] = q, sc, bits.astype(np.uint8), cls
        out[f"ref_{T}"] = ref.astype(np.uint16)                        # the reference's output
        out[f"exact_minus_ref_{T}"] = (oe - ref).astype(np.int16)       # the exact-sum-rounded-once candidate, as a difference
    n_c8 = sum(v for k, v in counts.items() if k.endswith("_c8"))
    assert n_c8 >= 4, n_c8
    out["lengths"] = np.array(BIGSUM_LENGTHS, np.int32)
    out["meta"] = np.array(json.dumps(dict(seed=20261020, scales=[[float(np.float32(s)), x0] for s, x0 in BIGSUM_SCALES],
                                           scales_49_only=[[float(np.float32(s)), x0] for s, x0 in BIGSUM_SCALES_49],
                                           classes=dict(a=0, b=1, c=2), counts=counts, notes=notes, torch=torch.__version__)))
    path = os.path.join(GOLD, "shiftmax_bigsum_kat.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 300 * 1024, os.path.getsize(path)
    print(f"shiftmax_bigsum_kat.npz written: {os.path.getsize(path)} bytes; {counts}")


LN16_RANGES = {0: 4.0, 1: 3.71}          # the QuantAct range behind the LayerNorm, per scale index (power-of-two, natural)


def _ln16_fix_sum(rng, q, tgt):
    """move the integer row sums of q [N, C] to tgt [N] by steps of +-1 on |delta| distinct random elements (|delta| <= C)"""
    delta = tgt - q.sum(axis=1)
    assert np.abs(delta).max() <= q.shape[1]
    rank = np.argsort(rng.random(q.shape), axis=1).argsort(axis=1)
    return q + np.sign(delta)[:, None] * (rank < np.abs(delta)[:, None])


def _ln16_v_row(rng, C, T, ulp, ok_value):
    """a row of +- pairs (mean 0, var = 2 sum a^2) whose variance rounds to the float32 T: -> int64 [C] or None"""
    x = int(T) // 2
    tol = 0 if ulp <= 2 else ulp // 4 - 1                    # |2 sum a^2 - T| < ulp / 2, no tie
    half = C // 2
    vals = []
    n0 = min(half - 14, max(1, -(-x // (30000 * 30000))))
    a0 = int(np.sqrt(x // n0))
    while a0 > 0 and not ok_value(a0):
        a0 -= 1
    if a0 > 32767:
        return None
    if a0 > 0:
        vals += [a0] * n0
        x -= n0 * a0 * a0
    while x > tol and len(vals) < half:
        a = min(int(np.sqrt(x)), 32767)
        while a * a > x:
            a -= 1
        while a > 1 and not ok_value(a):
            a -= 1
        vals.append(a)
        x -= a * a
    if abs(x) > tol:
        return None
    row = np.zeros(C, np.int64)
    row[:len(vals)] = vals
    row[half:half + len(vals)] = [-v for v in vals]
    return row


def gen_ln16_bigrows():
    """tests/golden/ln16_bigrows_kat.npz: IVITIntLayerNorm + an 8-bit QuantAct on 16-bit rows whose float32 sum reaches 2^24 (the
    mean, ivit_modules.py:37, then depends on the order of torch's CPU kernel), whose int32 squares wrap (:41), or whose variance
    lies where swin.hip's ln16_std10 decides between its shortcut and the literal Newton loop.  Stored per width C and scale: the
    int16 rows, gamma, beta, the output range, the REFERENCE's int8 output, a class per row (tests/ln16_order_ref.py) and per row
    the CRC32 of the two other candidates' outputs (exact sum rounded once; 64-bit squares).  Class (c) rows come from a seeded,
    directed search: rows whose integer sum is moved next to a .5 tie of the mean, kept where the two sums fall on either side."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ln16_order_ref as lno
    torch.set_num_threads(1)
    rng = np.random.default_rng(20261021)
    t_start = time.time()
    out, counts, notes = {}, {}, {}
    for C in lno.TILED_C + lno.OTHER_C:
        gamma = rng.uniform(0.5, 1.5, size=C).astype(np.float32)
        beta = rng.normal(0, 0.1, size=C).astype(np.float32)
        out[f"gamma_{C}"], out[f"beta_{C}"] = gamma, beta
        for si, s in enumerate(lno.SCALES):
            hi = LN16_RANGES[si]
            key = f"{C}_{si}"
            rows, kinds, vkind, edge = [], [], [], []

            def cls_of(q):
                return lno.classify(q, s, gamma, beta, -hi, hi)

            def keep(q, want, limit, vk=lno.V_NONE, ed=0):
                cls, _, _ = cls_of(q)
                idx = np.flatnonzero(cls == (lno.CLASS_A if want == lno.CLASS_V else want))[:limit]
                for i in idx:
                    rows.append(q[i].astype(np.int16)); kinds.append(want); vkind.append(vk); edge.append(ed)
                return len(idx)

            # ---- (a) control: centred rows, one of small amplitude
            qa = np.clip(np.rint(rng.normal(0, 3000, size=(8, C))), -32768, 32767).astype(np.int64)
            qa[1] = rng.integers(-5, 6, size=C)
            assert keep(qa, lno.CLASS_A, 2) == 2
            # ---- (b), (c): rows far from zero, either sign, their integer sum moved next to a .5 tie of the mean
            base_lo = max(8000, (1 << 24) // C + 200)
            nb, nc = 0, {1: 0, -1: 0}
            n_c, n_sign = (8, 3) if C in lno.TILED_C else (4, 2)      # (the wave-per-row kernels: one form, fewer rows); rows per sign at least
            for attempt in range(400):
                if nc[1] + nc[-1] >= n_c and min(nc.values()) >= n_sign:
                    break
                N = 4096
                sign = rng.choice([-1, 1], size=(N, 1))
                sigma = np.exp(rng.uniform(np.log(3), np.log(16), size=(N, 1)))
                base = rng.uniform(base_lo, 31500, size=(N, 1))
                q = np.rint(sign * base + sigma * rng.normal(size=(N, C))).astype(np.int64)
                k = np.floor(q.sum(axis=1) / C).astype(np.int64)
                q = _ln16_fix_sum(rng, q, C * k + C // 2 + rng.integers(-1, 2, size=N))
                q = q[(np.abs(q).max(axis=1) <= 32767)]
                xf = lno.xint_of(q, s)
                St, Se = lno.both_sums(xf)
                m = lno.mean_int_of(St, C) != lno.mean_int_of(Se, C)
                if nb < 2:
                    nb += keep(q[~m][:64], lno.CLASS_B, 2 - nb)
                for sg in (1, -1):
                    qs = q[m & (q[:, 0] * sg > 0)]
                    if len(qs) and nc[sg] < n_c - n_sign and nc[1] + nc[-1] < n_c:
                        nc[sg] += keep(qs, lno.CLASS_C, min(n_c - n_sign - nc[sg], n_c - nc[1] - nc[-1]))
            assert nb == 2 and nc[1] + nc[-1] == n_c and min(nc.values()) >= n_sign, (key, nb, nc)
            # ---- (w): a cluster around a mean of 14 000 or more, 1..4 elements at the opposite rail; the first two rows have
            #      max |d| = 46 341 exactly (class w) and 46 340 exactly (no wrap: stored with edge = 1, class a or b)
            nw = 0
            for attempt in range(200):
                if nw >= 9:
                    break
                sg = 1 if attempt % 2 == 0 else -1            # the sign of the cluster; the rail is the other one
                rail = -32768 if sg > 0 else 32767
                krail = int(np.trunc(lno.xint_of(np.array([rail]), s))[0])
                nr = 1 if nw < 2 else int(rng.integers(1, 5))
                if nw < 2:
                    want_d = lno.WRAP_FROM - nw                # 46 341, then 46 340
                    target = krail + want_d if sg > 0 else krail - want_d
                else:
                    target = sg * int(rng.integers(14000, 19000))
                sigma = 2500 + 700 * nr
                # (sixteen levels of the normal distribution, not its whole range: the rows compress)
                q = np.clip(np.rint(target + sigma * np.rint(rng.normal(size=(1, C)) * 3) / 3), -32768, 32767).astype(np.int64)
                q[0, rng.choice(C, size=nr, replace=False)] = rail
                # the mean: the rails are part of it
                for _ in range(3):
                    delta = C * target - int(q.sum())
                    cl = q[0] != rail
                    q[0, cl] = np.clip(q[0, cl] + delta // int(cl.sum()), -32767, 32766)
                delta = C * target - int(q.sum())
                if not 0 <= delta < int(cl.sum()):
                    continue
                q[0, np.flatnonzero(cl)[:delta]] += 1          # the integer sum is C * target exactly
                cls, cand, ref = cls_of(q)
                if nw == 1:
                    if ref["maxd"][0] == lno.WRAP_FROM - 1 and cls[0] in (lno.CLASS_A, lno.CLASS_B):
                        rows.append(q[0].astype(np.int16)); kinds.append(int(cls[0])); vkind.append(lno.V_NONE); edge.append(1)
                        nw += 1
                    continue
                if nw == 0 and ref["maxd"][0] != lno.WRAP_FROM:
                    continue
                if cls[0] != lno.CLASS_W or not np.any(cand[("torch", True)] != cand[("torch", False)]):
                    continue
                assert ref["var"][0] > 0
                nw += keep(q, lno.CLASS_W, 1)
            assert nw == 9, (key, nw)
            # ---- (v): +- pairs whose variance rounds into, or just outside, the band of ln16_std10, per binade; the 2^37 boundary
            k_ok = np.trunc(lno.xint_of(np.arange(32768), s)).astype(np.int64) == np.arange(32768)

            def ok_value(a):
                return bool(k_ok[a])

            reach = C // 2 * 2 * 32767 ** 2
            # (the wave-per-row kernels of C = 772 / 2048 always run the ten literal steps: four binades and the boundary there)
            for ex in (range(24, 42) if C in lno.TILED_C else lno.V_BINADES_OTHER_C):
                lo_sq, hi_sq = 2.0 ** ex * 1.05, min(2.0 ** (ex + 1) * 0.95, reach * 0.93)
                if lo_sq >= hi_sq:
                    notes[f"{key}_v{ex}"] = "out of reach of 16-bit +- pairs at this width"
                    continue
                got = {lno.V_INSIDE: 0, lno.V_OUTSIDE: 0}
                for attempt in range(40):
                    if got[lno.V_INSIDE] and got[lno.V_OUTSIDE]:
                        break
                    s1 = int(np.sqrt(rng.uniform(lo_sq, hi_sq)))
                    T = np.float32(s1 * s1)
                    if float(T) >= s1 * s1:
                        T = np.nextafter(T, np.float32(0))
                    for _ in range(12):                         # walk down from the square: in the band first, then out of it
                        slow = bool(lno.std10_rule(T)[0])
                        vk = lno.V_INSIDE if slow else lno.V_OUTSIDE
                        if not got[vk]:
                            row = _ln16_v_row(rng, C, int(T), 1 << (ex - 23), ok_value)
                            if row is not None:
                                chk = lno.layernorm(row[None], s, gamma, beta)
                                if np.float32(chk["var"][0]) == T and chk["mean_int"][0] == 0:
                                    got[vk] += keep(row[None], lno.CLASS_V, 1, vk)
                        if not slow:
                            break
                        T = np.nextafter(T, np.float32(0))
                assert got[lno.V_INSIDE] and got[lno.V_OUTSIDE], (key, ex, got)
            if reach > 2 ** 37:
                for T in (np.float32(2.0 ** 37), np.nextafter(np.float32(2.0 ** 37), np.float32(0))):
                    row = _ln16_v_row(rng, C, int(T), 1 << 13, ok_value)
                    assert row is not None and np.float32(lno.layernorm(row[None], s, gamma, beta)["var"][0]) == T
                    assert keep(row[None], lno.CLASS_V, 1, lno.V_BOUNDARY) == 1
            # ---- the reference itself on every row of the group
            q = np.stack(rows).astype(np.int64)
            kinds, vkind, edge = np.array(kinds, np.uint8), np.array(vkind, np.uint8), np.array(edge, np.uint8)
            ln = rq.IVITIntLayerNorm(C)
            ln.weight.data, ln.bias.data = torch.from_numpy(gamma), torch.from_numpy(beta)
            st = torch.tensor([s])
            x = (torch.from_numpy(q.astype(np.float32))[None] * st).float().contiguous()
            yl, sl = ln(x, st)
            assert bool(torch.isfinite(yl).all()), key
            qa_mod = rq.QuantAct()
            qa_mod.x_min.fill_(-hi)
            qa_mod.x_max.fill_(hi)
            qa_mod.fix()
            yq, sq = qa_mod(yl, sl)
            ref_out = torch.round(yq / sq).numpy().reshape(len(q), C).astype(np.int32)
            assert ref_out.min() >= -128 and ref_out.max() <= 127
            # the restatement must agree with it, and the classes hold what they say
            cls, cand, ref = cls_of(q)
            assert np.array_equal(cand[("torch", True)], ref_out), (key, "the reference's output is not the restatement's")
            assert np.array_equal((ref["y"] * ref["s_ln"]).astype(np.float32).view(np.int32), yl.numpy().reshape(len(q), C).view(np.int32)), key
            assert np.array_equal(np.where(kinds == lno.CLASS_V, lno.CLASS_A, kinds), cls), key
            xf = lno.xint_of(q, s)
            big = np.abs(xf.astype(np.float64).sum(axis=1)) >= 2.0 ** 24
            St, Se = lno.both_sums(xf)
            assert np.array_equal(x[0].div(st).sum(dim=-1).numpy(), St), "torch's sum is not the restated order"
            same_mean = lno.mean_int_of(St, C) == lno.mean_int_of(Se, C)
            d_exact = np.any(cand[("exact", True)] != ref_out, axis=1)
            d_nowrap = np.any(cand[("torch", False)] != ref_out, axis=1)
            a = np.isin(kinds, (lno.CLASS_A, lno.CLASS_V))
            assert not big[a].any() and (ref["maxd"][a] < lno.WRAP_FROM).all() and not d_exact[a].any() and not d_nowrap[a].any()
            b = kinds == lno.CLASS_B
            assert big[b].all() and same_mean[b].all() and not d_exact[b].any() and not d_nowrap[b].any()
            c = kinds == lno.CLASS_C
            assert big[c].all() and not same_mean[c].any() and d_exact[c].all() and not d_nowrap[c].any()
            assert (St[c] > 0).sum() >= n_sign and (St[c] < 0).sum() >= n_sign and c.sum() == n_c
            w = kinds == lno.CLASS_W
            assert (ref["maxd"][w] >= lno.WRAP_FROM).all() and (ref["var"][w] > 0).all() and d_nowrap[w].all() and not d_exact[w].any()
            assert w.sum() >= 8 and (ref["maxd"][w] == lno.WRAP_FROM).any() and (ref["maxd"][edge == 1] == lno.WRAP_FROM - 1).all()
            assert edge.sum() == 1 and (ref["var"] > 0).all()
            v = kinds == lno.CLASS_V
            slow = lno.std10_rule(ref["var"][v].astype(np.float32))[0]
            assert np.array_equal(slow[vkind[v] == lno.V_INSIDE], np.ones((vkind[v] == lno.V_INSIDE).sum(), bool))
            assert not slow[vkind[v] == lno.V_OUTSIDE].any() and (ref["mean_int"][v] == 0).all()
            out[f"q_{key}"], out[f"cls_{key}"], out[f"vkind_{key}"], out[f"edge_{key}"] = q.astype(np.int16), kinds, vkind, edge
            out[f"ref_{key}"] = ref_out.astype(np.int8)
            out[f"exact_crc_{key}"] = np.array([zlib.crc32(r.tobytes()) for r in cand[("exact", True)]], np.uint32)
            out[f"nowrap_crc_{key}"] = np.array([zlib.crc32(r.tobytes()) for r in cand[("torch", False)]], np.uint32)
            for kc in lno.CLASS_NAMES:
                counts[f"{key}_{lno.CLASS_NAMES[kc]}"] = int((kinds == kc).sum())
            print(f"[ln16_bigrows] C={C} s={float(s):.6g}: {len(q)} rows, "
                  f"{ {lno.CLASS_NAMES[kc]: int((kinds == kc).sum()) for kc in lno.CLASS_NAMES} }  ({time.time() - t_start:.0f} s)", flush=True)
    out["widths"] = np.array(lno.TILED_C + lno.OTHER_C, np.int32)
    out["scales"] = np.array(lno.SCALES, np.float32)
    out["ranges"] = np.array([LN16_RANGES[0], LN16_RANGES[1]], np.float32)
    out["meta"] = np.array(json.dumps(dict(seed=20261021, classes={v: k for k, v in lno.CLASS_NAMES.items()}, counts=counts, notes=notes,
                                           torch=torch.__version__)))
    path = os.path.join(GOLD, "ln16_bigrows_kat.npz")
    np.savez_compressed(path, **out)
    # (8 (c) and 8 (w) rows at six widths and two scales are about 190 000 elements whose int16 inputs and int8 outputs barely compress)
    assert os.path.getsize(path) < 640 * 1024, os.path.getsize(path)
    print(f"ln16_bigrows_kat.npz written: {os.path.getsize(path)} bytes")


def gen_schema():
    """state_dict keys and shapes of the reference's DeiT and Swin models (the on-disk checkpoint format)"""
    out = {}
    for factory in ("deit_tiny_patch16_224", "deit_small_patch16_224", "deit_base_patch16_224"):
        model = getattr(ref_models, factory)(pretrained=False, gelu_type="ivit", softmax_type="ivit",
                                             layernorm_type="ivit")
        out[factory] = {k: list(v.shape) for k, v in model.state_dict().items()}
    # the same DeiT with the I-BERT operators (the fork's default family): different buffers (shift, internal QuantAct)
    model = ref_models.deit_tiny_patch16_224(pretrained=False, gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
    out["deit_tiny_patch16_224@ibert"] = {k: list(v.shape) for k, v in model.state_dict().items()}
    sq = _import_swin()
    for factory in ("swin_tiny_patch4_window7_224",):
        out[factory] = {k: list(v.shape) for k, v in getattr(sq, factory)(pretrained=False).state_dict().items()}
    with open(os.path.join(GOLD, "state_dict_schema.json"), "w") as f:
        json.dump(out, f)
    print("state_dict_schema.json written:", {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    what = sys.argv[1:] or ["ops", "schema", "deit_tiny", "deit_small", "deit_base", "vit_base"]
    for w in what:
        if w == "ops":
            gen_ops()
        elif (w.endswith("_w16") or w.endswith("_w16all")) and "ibert" not in w:
            gen_w16(w)
        elif w == "compat_ops":
            gen_compat_ops()
        elif w == "ibert_ops":
            gen_ibert_ops()
        elif w == "calib_trace":
            gen_calib_trace()
        elif w == "schema":
            gen_schema()
        elif w == "shiftmax_bigsum":
            gen_shiftmax_bigsum()
        elif w == "ln16_bigrows":
            gen_ln16_bigrows()
        elif w in ("deit_tiny_ibert_natural", "deit_tiny_ibert_w16all"):
            gen_ibert_natural(w)
        elif w.endswith("_natural") and not w.startswith("swin"):
            gen_natural(w)
        elif w.startswith("swin"):
            gen_swin(w)
        else:
            gen_model(w)
