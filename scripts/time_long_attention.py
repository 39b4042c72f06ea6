"""Long-row attention: time per (query, key) score of ivit_attention_fused_i8_long against the 197-token kernel, and DeiT-B at 384 px
(577 tokens), batch 64: the engine's forward against the module path's.  Torch events time each case here; the numbers to quote come
from the kernel trace of one run:

    rocprofv3 --kernel-trace --stats -d prof -o run -- python scripts/time_long_attention.py [kernels] [model]
    python scripts/time_long_attention.py summary prof/run_results.db

`summary` reads the trace database and prints, per attention kernel form and token count, the dispatch durations and the time
per score (T is recovered from the launch's LDS size, B from the cases below; the model's launches are the natural-scale form).

    python scripts/time_long_attention.py --family ibert [kernels] [model]

times the I-BERT family instead: ivit_attention_fused_i8_ibert_long (table and band form) against ivit_attention_fused_i8_long at 577
and 1025 tokens, batch 64, and the forward of a depth-2 I-BERT model of DeiT-B's geometry (C = 768, 12 heads) at 384 / 16, batch 64,
through the module path (the fused engine does not take I-BERT models of more than 207 tokens).  Every figure is the median of
seven event-timed repeats after warm-up, with the smallest and largest repeat.

    python scripts/time_long_attention.py --softmax-bits 16

times ivit_attention_fused_i8_wide_long with 16-bit probabilities beside the 8-bit long-row kernel in the same run, on the same
operands: 577 and 785 tokens, batch 64, 12 heads, power-of-two scales and a natural scale (band table); the same seven repeats."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivit_amd  # noqa: E402,F401
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.prepare import dyadic  # noqa: E402

DEV = "cuda:0"
H, hd = 12, 64
rng = np.random.default_rng(0)
st = _lib.stream_ptr


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def attention(B, T):
    """us per launch: power-of-two scales (the float32 score requantisation), row-major output"""
    qkv = torch.from_numpy(np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)).to(DEV)
    out = torch.empty(B * T, H * hd, dtype=torch.int8, device=DEV)
    ms, es = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))
    mo, eo = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -3))
    name = "ivit_attention_fused_i8_long" if T > 207 else "ivit_attention_fused_i8_compat_band"
    return timeit(lambda: _lib.call(name, _lib.ptr(qkv), _lib.ptr(out), B, H, T, hd, int(ms[0]), int(es[0]), 0.25, int(mo[0]),
                                    int(eo[0]), None, None, 0, 0, st()))


def repeats(fn, n, reps=7):
    """(median, min, max) in us of `reps` event-timed windows of n calls each"""
    t = sorted(timeit(fn, n) for _ in range(reps))
    return t[reps // 2], t[0], t[-1]


def ibert_tables(s_at=0.25, hi=1.0):
    """the (row max, q) table of the I-BERT softmax at input scale s_at, internal QuantAct range [0, hi], and its band form"""
    from ivit_amd.prepare import shiftexp_band
    from ivit_amd.quantization_utils.ibert_modules import softmax_constants
    x0i, bi, ci, exp_sf, act_sf, ma, ea = softmax_constants(s_at, 0.0, hi)
    tab = torch.empty(65536, dtype=torch.float32, device=DEV)
    _lib.call("ivit_ibert_softmax_build_table", float(s_at), x0i, bi, ci, float(exp_sf), float(act_sf), ma, ea, _lib.ptr(tab), st())
    band, bw = shiftexp_band(tab.cpu().numpy().view(np.uint32).reshape(256, 256))
    return tab, (torch.from_numpy(band.view(np.float32)).to(DEV) if bw else None), bw


def ibert_attention(B, T):
    """us per launch (median, min, max) of ivit_attention_fused_i8_long (power-of-two form: exponents from LDS; natural-scale form:
    gathered from the global band table) and of the I-BERT entry, table and band form, on the same operands"""
    qkv = torch.from_numpy(np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)).to(DEV)
    out = torch.empty(B * T, H * hd, dtype=torch.int8, device=DEV)
    ms, es = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))
    mo, eo = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -3))
    tab, band, bw = ibert_tables()
    a = (_lib.ptr(qkv), _lib.ptr(out), B, H, T, hd, int(ms[0]), int(es[0]))
    from ivit_amd.prepare import shiftexp2d, shiftexp_band
    nb, nbw = shiftexp_band(shiftexp2d(np.float32(0.0437)))          # I-ViT at a natural scale: the same two gathers per score
    nband = torch.from_numpy(nb.view(np.int32)).to(DEV)
    res = {"ivit": repeats(lambda: _lib.call("ivit_attention_fused_i8_long", *a, 0.25, int(mo[0]), int(eo[0]), None, None, 0, 0, st()), 10),
           "ibert table": repeats(lambda: _lib.call("ivit_attention_fused_i8_ibert_long", *a, int(mo[0]), int(eo[0]), _lib.ptr(tab), None, 0,
                                                    0, st()), 10)}
    res[f"ivit band {nbw}"] = repeats(lambda: _lib.call("ivit_attention_fused_i8_long", *a, 0.0437, int(mo[0]), int(eo[0]), None,
                                                       _lib.ptr(nband), nbw, 0, st()), 10)
    if bw:
        res[f"ibert band {bw}"] = repeats(lambda: _lib.call("ivit_attention_fused_i8_ibert_long", *a, int(mo[0]), int(eo[0]), _lib.ptr(tab),
                                                            _lib.ptr(band), bw, 0, st()), 10)
    return res


def wide_attention(B, T, bits):
    """us per launch (median, min, max) of the 8-bit long-row kernel and of ivit_attention_fused_i8_wide_long with `bits`-wide
    probabilities on the same operands, at power-of-two scales and at a natural scale (band table); the output requantiser
    follows the width of the probabilities (2^-(bits-1) times the scale of V)"""
    from ivit_amd.prepare import shiftexp2d, shiftexp_band
    qkv = torch.from_numpy(np.clip(np.rint(rng.normal(0, 40, size=(3, B, H, T, hd))), -128, 127).astype(np.int8)).to(DEV)
    out = torch.empty(B * T, H * hd, dtype=torch.int8, device=DEV)
    ms, es = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -2))
    mo8, eo8 = dyadic(np.float32(2.0 ** -11), np.float32(2.0 ** -3))
    mow, eow = dyadic(np.float32(2.0 ** -(bits + 3)), np.float32(2.0 ** -3))
    nb, nbw = shiftexp_band(shiftexp2d(np.float32(0.0437)))
    nband = torch.from_numpy(nb.view(np.int32)).to(DEV)
    a = (_lib.ptr(qkv), _lib.ptr(out), B, H, T, hd, int(ms[0]), int(es[0]))
    res = {}
    for regime, s_at, band, bw in (("pow2", 0.25, None, 0), (f"band {nbw}", 0.0437, nband, nbw)):
        res[f"8 bit {regime}"] = repeats(lambda: _lib.call("ivit_attention_fused_i8_long", *a, s_at, int(mo8[0]), int(eo8[0]), None,
                                                           _lib.ptr(band), bw, 0, st()), 10)
        res[f"{bits} bit {regime}"] = repeats(lambda: _lib.call("ivit_attention_fused_i8_wide_long", *a, s_at, int(mow[0]), int(eow[0]),
                                                                None, _lib.ptr(band), bw, bits, 0, st()), 10)
    return res


def ibert_model():
    """forward of a frozen depth-2 I-BERT model, C = 768, 12 heads, 384 / 16, batch 64, as the reference calls it (module by module)"""
    from ivit_amd.quantization_utils import lazy
    torch.manual_seed(0)
    model = ivit_amd.VisionTransformer(img_size=384, patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                       num_classes=1000, gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert").to(DEV).eval()
    imgs = torch.from_numpy(np.concatenate([synth.make_images(32, 5 + i) for i in range(2)])).to(DEV)
    x = torch.nn.functional.interpolate(imgs, size=(384, 384), mode="bilinear", align_corners=False).float().contiguous()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        model(x[:8])
        ivit_amd.freeze_model(model)
        assert model.engine_unsupported_reason() is not None
        names = []
        orig = _lib.call
        _lib.call = lambda name, *args: (names.append(name), orig(name, *args))[1]
        try:
            model(x)
        finally:
            _lib.call = orig
        med, lo, hi = repeats(lambda: model(x), 3)
    attn = sorted({n for n in names if "attention" in n or "bgemm" in n or "softmax" in n})
    print(f"I-BERT C=768 depth 2, 384 px b64, module path: forward {med / 1e3:.2f} ms (min {lo / 1e3:.2f}, max {hi / 1e3:.2f}); "
          f"{len(names)} launches, attention through {attn}; int8-carrying path {'on' if lazy.ENABLED else 'off'}")


CASES = [(256, 197), (64, 209), (64, 577), (64, 785)]


def long_lds(T):
    """dynamic LDS of ivit_attention_fused_i8_long (its launcher): exponent tables, K image, V^T rows padded to 256 bytes"""
    nkt = (T + 15) // 16
    return 2048 + nkt * 1024 + 64 * (((nkt + 3) // 4 + 3) // 4) * 256


def summary(db):
    import sqlite3
    con = sqlite3.connect(db)
    by_lds = {long_lds(T): T for _, T in CASES if T > 207}
    rows = con.execute("select name, lds_size, count(*), avg(duration), min(duration) from kernels where name like '%attention%' "
                       "group by name, lds_size order by min(start)").fetchall()
    for name, lds, n, avg, mn in rows:
        form = name.split("(anonymous namespace)::")[1].rsplit("(", 1)[0]
        T = 197 if form.startswith("attention_kernel") else by_lds.get(lds)
        B = {197: 256}.get(T, 64)
        ps = mn * 1e3 / (B * H * T * T) if T else float("nan")
        print(f"{form:52s} T={T} B={B}: {n:3d} dispatches, mean {avg / 1e3:8.1f} us, min {mn / 1e3:8.1f} us, {ps:.3f} ps/score (min)")


argv = sys.argv[1:]
family = "ivit"
if "--family" in argv:
    i = argv.index("--family")
    family = argv[i + 1]
    del argv[i:i + 2]
    assert family in ("ivit", "ibert"), family
if "--softmax-bits" in argv:
    i = argv.index("--softmax-bits")
    sm_bits = int(argv[i + 1])
    assert sm_bits in (8, 16), sm_bits
    for B, T in [(64, 577), (64, 785)]:
        res = wide_attention(B, T, sm_bits)
        for k, (med, lo, hi) in res.items():
            base = res["8 bit " + k.split(" bit ")[1]][0]
            print(f"attention B={B} T={T:4d} {k:16s} {med:8.1f} us (min {lo:.1f}, max {hi:.1f})  {med * 1e6 / (B * H * T * T):.3f} ps/score  "
                  f"{med / base:.2f}x the 8-bit kernel")
    sys.exit(0)
which = argv or ["kernels", "model"]
if family == "ibert":
    if "kernels" in which:
        for B, T in [(64, 577), (64, 1025)]:
            res = ibert_attention(B, T)
            for k, (med, lo, hi) in res.items():
                print(f"attention B={B} T={T:4d} {k:14s} {med:8.1f} us (min {lo:.1f}, max {hi:.1f})  {med * 1e6 / (B * H * T * T):.3f} ps/score  "
                      f"{med / res['ivit'][0]:.2f}x ivit")
    if "model" in which:
        ibert_model()
    sys.exit(0)
if which[0] == "summary":
    summary(which[1])
    sys.exit(0)
if "kernels" in which:
    for B, T in CASES:
        us = attention(B, T)
        ps = us * 1e6 / (B * H * T * T)      # chip-wide: launch time over every (query, key) score of the batch
        print(f"attention B={B:3d} T={T:4d}  {us:8.1f} us  {ps:.3f} ps/score")

if "model" in which:
    from ivit_amd.quantization_utils import lazy
    fs = synth.make_float_state("deit_base_patch16_224", 31)
    fs["pos_embed"] = np.random.default_rng(1).normal(0, 0.02, size=(1, 577, 768)).astype(np.float32)
    model = ivit_amd.deit_base_patch16_224(img_size=384)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in fs.items()}, strict=False)
    model.to(DEV).eval()
    imgs = torch.from_numpy(np.concatenate([synth.make_images(32, 5 + i) for i in range(2)])).to(DEV)
    imgs = torch.nn.functional.interpolate(imgs, size=(384, 384), mode="bilinear", align_corners=False).contiguous()
    with torch.no_grad():
        model(imgs[:8])
        ivit_amd.freeze_model(model)
        assert model.engine_unsupported_reason() is None, model.engine_unsupported_reason()
        eng = model.engine(64)
        x = imgs.float().contiguous()
        t_eng = timeit(lambda: eng.forward(x), n=10)
        model.use_engine = False
        lazy.enable_everywhere(True)
        try:
            t_mod = timeit(lambda: model(x), n=3)
        finally:
            lazy.enable_everywhere(False)
    print(f"DeiT-B 384 px b64: engine forward {t_eng / 1e3:.2f} ms, module path {t_mod / 1e3:.2f} ms ({t_mod / t_eng:.1f}x)")
    # the engine's own attention launches (its exponent tables: natural scales here), on the workspace of the last forward
    ws, t_att = eng.ws, 0.0
    for blk in eng.blocks:
        a = blk["attn"]
        t_att += timeit(lambda: _lib.call("ivit_attention_fused_i8_long", _lib.ptr(ws["qkv"]), _lib.ptr(ws["ao"]), 64, eng.H, eng.T, 64,
                                          a["ms"][0], a["ms"][1], a["s_attn"], a["mo"][0], a["mo"][1], _lib.ptr(a["exp2d"]),
                                          _lib.ptr(a["band"]), a["band_w"], 1, st()), n=5)
    print(f"attention share of the engine forward: {t_att:.1f} us over {len(eng.blocks)} blocks = {t_att / t_eng * 100:.1f} % "
          f"(natural-scale launches: {sum(1 for b in eng.blocks if b['attn']['band_w'] or b['attn']['exp2d'] is not None)})")
