"""Writes the fixtures of IBERTIntLayerNorm(use_int_sqrt=True) -- layernorm_type 'ibert_use-int-sqrt_true' -- by running the REFERENCE
on the CPU.  The reference is imported unmodified through the harness of oracle/gen_golden.py (its shims and its path); the files
hold data only.

    python scripts/make_ibert_intsqrt_golden.py [kat] [ops] [deit_tiny_ibert_isqrt] [deit_tiny_ibert_isqrt_natural] [deit_tiny_ibert_isqrt_w16all]

  tests/golden/ibert_intsqrt_kat.npz   n (float32) and the reference's integer_sqrt(n): every float32 integer within 40 steps of
                                       2^1 .. 2^32, k^2 - 1 / k^2 / k^2 + 1 for a spread of k up to 65535, all integers below 4096, 20 000
                                       seeded log-uniform values, 0
  tests/golden/ibert_intsqrt_ops.npz   per case of tests/ibert_intsqrt_ref.CASES (inputs by seed): the CRC-32 of every output row of the
                                       reference's module (the vectors themselves would take 11 MB), and the two float32 row statistics
                                       mean_int / var_int in torch's reduction order.  The numpy restatement of tests/ibert_intsqrt_ref.py
                                       is held to the module's output here, element by element, before anything is written
  tests/golden/<tag>.npz               DeiT-T with the I-BERT operators and that LayerNorm, in the format of deit_tiny_ibert.npz /
                                       deit_tiny_ibert_natural.npz / deit_tiny_ibert_w16all.npz: own calibration, ranges, INT32 logits, top-1
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import gen_golden as gg  # noqa: E402  (imports the reference; torch.Tensor.cuda shim)
import ibert_intsqrt_ref as R  # noqa: E402

LN_TYPE = "ibert_use-int-sqrt_true"
f32 = np.float32


def gen_kat():
    vals = [np.zeros(1, f32), np.arange(4096, dtype=f32)]
    for k in range(1, 33):
        lo = hi = f32(2.0 ** k)
        for _ in range(40):
            vals.append(np.array([hi], f32))
            lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))
            vals.append(np.array([lo], f32))
    ks = np.unique(np.concatenate([np.arange(2, 300), np.rint(np.exp2(np.linspace(8, 16, 1500))), [4096, 46340, 46341, 65535]])).astype(np.int64)
    ks = ks[ks <= 65535]
    vals.append(np.concatenate([ks * ks - 1, ks * ks, ks * ks + 1]).astype(np.float64).astype(f32))
    vals.append(np.exp2(np.random.default_rng(20261018).uniform(0, 32, 20000)).astype(f32))
    n = np.unique(np.floor(np.concatenate(vals)))
    n = n[n < 2.0 ** 32].astype(f32)
    ln = gg.rq.IBERTIntLayerNorm(8, use_int_sqrt=True)
    out = ln.integer_sqrt(torch.from_numpy(n)).numpy().astype(np.int32)
    assert np.array_equal(out, R.integer_sqrt(n)), "the numpy restatement differs from the reference"
    isq = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    np.savez_compressed(os.path.join(gg.GOLD, "ibert_intsqrt_kat.npz"), n=n, isqrt=out,
                        meta=np.array(json.dumps(dict(torch=torch.__version__, above_floor_sqrt=int((out != isq).sum())))))
    print(f"ibert_intsqrt_kat.npz: {n.size} values, {int((out != isq).sum())} differ from floor(sqrt(n)); restatement bit-equal")


def gen_ops():
    out, meta = {}, {}
    for case in R.CASES:
        d, key = R.make_case(case), R.case_key(case)
        C, s = d["C"], torch.tensor([d["s_in"]])
        ln = gg.rq.IBERTIntLayerNorm(C, use_int_sqrt=True)
        ln.weight.data = torch.from_numpy(d["gamma"])
        ln.bias.data = torch.from_numpy(d["beta"])
        ln.shift.fill_(float(np.log2(d["shift_pow2"])))
        x = torch.from_numpy((d["q"].astype(f32) * d["s_in"]).astype(f32)).reshape(1, R.ROWS, C)
        y_open, _ = ln(x, s)                       # overflow handling on (var_int < 2^32: the shift stays)
        ln.fix()
        y, so = ln(x, s)
        assert torch.equal(y_open.view(torch.int32), y.view(torch.int32)) and float(ln.shift) == float(np.log2(d["shift_pow2"]))
        y = y.numpy().reshape(R.ROWS, C)
        # the row statistics with torch's own reductions (the operations of the module's forward on the same operand)
        xi = x / s
        mean_int = torch.round(xi.mean(axis=2, keepdim=True))
        ys = torch.floor((xi - mean_int) / 2 ** ln.shift)
        var_int = torch.sum(ys ** 2, axis=2, keepdim=True)
        mean_int, var_int = mean_int.numpy().reshape(R.ROWS, 1), var_int.numpy().reshape(R.ROWS, 1)
        bias_int, s_out = R.layernorm_constants(d["gamma"], d["beta"])
        assert np.array_equal(so.detach().numpy().reshape(-1), s_out)
        mine = R.layernorm(R.x_int_of(d["q"], d["s_in"]), bias_int, s_out, d["shift_pow2"], mean_int=mean_int, var_int=var_int)
        assert np.array_equal(mine.view(np.int32), y.view(np.int32)), f"{key}: the numpy restatement differs from the reference"
        if d["s_in"] == 2.0 ** round(np.log2(d["s_in"])):
            for row, T in d["targets"].items():      # (from 2^24 on the float32 sum may round on the way: near the value, not on it)
                assert float(var_int[row, 0]) == float(T) or T >= 2 ** 24, (key, row, T, float(var_int[row, 0]))
        plain = R.layernorm(R.x_int_of(d["q"], d["s_in"]), bias_int, s_out, d["shift_pow2"], mean_int=mean_int, var_int=var_int, int_sqrt=False)
        out[key + "/mean_int"], out[key + "/var_int"], out[key + "/row_crc32"] = mean_int[:, 0].copy(), var_int[:, 0].copy(), R.row_crcs(y)
        meta[key] = dict(rows_var_ge_2p24=int((var_int >= 2 ** 24).sum()),
                         targets_hit=int(sum(float(var_int[r, 0]) == float(T) for r, T in d["targets"].items())), targets=len(d["targets"]),
                         rows_differing_from_float_sqrt=int((mine.view(np.int32) != plain.view(np.int32)).any(axis=1).sum()))
        print(key, meta[key])
    out["meta"] = np.array(json.dumps(dict(torch=torch.__version__, cases=meta)))
    np.savez_compressed(os.path.join(gg.GOLD, "ibert_intsqrt_ops.npz"), **out)


def gen_model(tag):
    """deit_tiny_ibert_isqrt: the plan of deit_tiny_ibert (one calibration batch, ranges snapped to +-q 2^p); _natural / _w16all: the
    plan of deit_tiny_ibert_natural / deit_tiny_ibert_w16all (two batches, ranges as calibrated).  Four images each."""
    factory, wseed, iseed, nimg, cb = "deit_tiny_patch16_224", 11, 1001, 4, 4
    pow2 = tag == "deit_tiny_ibert_isqrt"
    cseeds = (101,) if pow2 else (101, 111)
    widths = gg.W16_ALL if tag.endswith("_w16all") else {}
    rq, synth = gg.rq, gg.synth
    model = getattr(gg.ref_models, factory)(pretrained=False, gelu_type="ibert", softmax_type="ibert", layernorm_type=LN_TYPE, **widths)
    lns = [m for m in model.modules() if isinstance(m, rq.IBERTIntLayerNorm)]
    assert len(lns) == 25 and all(m.use_int_sqrt for m in lns)
    fs = synth.make_float_state(factory, wseed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.eval()
    for cs in cseeds:
        model(torch.from_numpy(synth.make_images(cb, cs)))
    mods = dict(model.named_modules())
    if pow2:
        for name, mod in mods.items():
            if isinstance(mod, rq.QuantAct):
                mx = float(torch.max(-mod.x_min, mod.x_max))
                qmax = float(2 ** (mod.activation_bit - 1) - 1)
                p = int(np.ceil(np.log2(mx / qmax)))
                mod.x_max.fill_(qmax * 2.0 ** p)
                mod.x_min.fill_(-qmax * 2.0 ** p)
    ranges = {n: (f32(m.x_min.item()), f32(m.x_max.item())) for n, m in mods.items() if isinstance(m, rq.QuantAct)}
    shifts = {n: float(m.shift) for n, m in mods.items() if isinstance(m, rq.IBERTIntLayerNorm)}
    gg.ref_models.freeze_model(model)
    taps = {}

    def hook(name):
        def fn(mod, inp, outp):
            taps[name] = gg.to_int(outp[0], outp[1])
        return fn

    for name, mod in mods.items():
        if isinstance(mod, rq.QuantAct) and not name.endswith("int_softmax.act"):
            mod.register_forward_hook(hook(name))
    y = model(torch.from_numpy(synth.make_images(nimg, iseed)))
    s_head = (model.head.fc_scaling_factor * model.qact2.act_scaling_factor).float()
    names = sorted(taps)
    out = {
        "meta": np.array(json.dumps(dict(tag=tag, factory=factory, family="ibert", layernorm_type=LN_TYPE, weight_seed=wseed,
                                         calib_seeds=list(cseeds), calib_batch=cb, image_seed=iseed, n_images=nimg,
                                         qkv_gain=synth.QKV_GAIN, regime="pow2" if pow2 else "natural", ln_shifts=shifts,
                                         widths=widths, torch=torch.__version__))),
        "range_names": np.array(list(ranges)),
        "range_bits": np.array([int(mods[n].activation_bit) for n in ranges], np.int32),
        "x_min": np.array([v[0] for v in ranges.values()], f32),
        "x_max": np.array([v[1] for v in ranges.values()], f32),
        "logits_int32": torch.round(y / s_head).to(torch.int64).numpy().astype(np.int32),
        "logits_f32_bits": y.numpy().astype(f32).view(np.int32),
        "top1": y.argmax(dim=1).numpy().astype(np.int64), "head_scale": s_head.numpy().astype(f32),
        "tap_names": np.array(names), "tap_crc32": np.array([gg.crc(taps[n]) for n in names], np.uint32),
    }
    np.savez_compressed(os.path.join(gg.GOLD, f"{tag}.npz"), **out)
    print(f"[{tag}] wrote fixtures; LayerNorm shifts {sorted(set(shifts.values()))}; top1 = {out['top1'].tolist()}")


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    for what in sys.argv[1:] or ["kat", "ops", "deit_tiny_ibert_isqrt", "deit_tiny_ibert_isqrt_natural", "deit_tiny_ibert_isqrt_w16all"]:
        {"kat": gen_kat, "ops": gen_ops}.get(what, lambda: gen_model(what))()
