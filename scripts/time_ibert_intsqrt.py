"""IBERTIntLayerNorm use_int_sqrt on against off, on the MI355X (DESIGN.md section 4 / 5 quote this script's output):

  kernel   ivit_ibert_layernorm_i8 at the DeiT-B headline shape (50 432 rows x 768, 8-bit stream), microseconds per launch with and
           without IVIT_IBERT_LN_INT_SQRT on the same inputs, interleaved rounds; and ivit_ibert_layernorm_i16_i8_ex likewise
  model    DeiT-B, I-BERT operators, batch 256, graph replay: milliseconds per step with layernorm_type 'ibert_use-int-sqrt_true' and
           'ibert' (the model of `bench.py --operators ibert`: synthetic weights, ranges calibrated on one batch)
  rows     the share of LayerNorm rows that leave the fast kernel's decided path for the literal row (mean within the undecided
           band, V = 0, V >= 2^24), counted on the host from the kernel inputs and from the model's LayerNorm inputs of 8 images

    python scripts/time_ibert_intsqrt.py [kernel] [model]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib, synth  # noqa: E402
from ivit_amd.engine_common import IBERT_LN_INT_SQRT as FLAG  # noqa: E402
from ivit_amd.prepare import LayerNormParams  # noqa: E402

DEV = "cuda:0"
ISQRT = "ibert_use-int-sqrt_true"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def timeit(fn, n=30):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def ab(fns, rounds=7):
    """interleaved rounds -> per form (median, min, max) microseconds"""
    for f in fns.values():
        for _ in range(5):
            f()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            got[k].append(timeit(f))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def slow_rows(q, shift_pow2=1.0):
    """share of int8 rows that ibert_layernorm_i8_fast_kernel hands to the literal row before its element loop"""
    q = np.asarray(q, np.int64)
    C = q.shape[-1]
    m0 = (q.sum(-1).astype(np.float32) / np.float32(C)).astype(np.float32)
    band = np.abs((m0 - np.floor(m0)) - np.float32(0.5)) < np.float32(2.2e-3)
    V = (np.floor((q - np.rint(m0)[..., None]) / shift_pow2) ** 2).sum(-1)
    return dict(rows=int(band.size), mean_band=int(band.sum()), v_zero=int((V == 0).sum()), v_ge_2p24=int((V >= 2 ** 24).sum()),
                share=float((band | (V == 0) | (V >= 2 ** 24)).mean()))


def kernel():
    rows, C = 197 * 256, 768
    rng = np.random.default_rng(0)
    lp = LayerNormParams(rng.uniform(0.5, 1.5, size=C).astype(np.float32), rng.normal(0, 0.1, size=C).astype(np.float32), np.float32(2.0 ** -4))
    b, s, m, e = t(lp.bias_int), t(lp.s_ln), t(lp.m.view(np.int32)), t(lp.e)
    for sigma in (30, 60):
        q8 = np.clip(np.rint(rng.normal(0, sigma, size=(rows, C))), -128, 127).astype(np.int8)
        x, out = t(q8), torch.empty(rows, C, dtype=torch.int8, device=DEV)
        for s_in in (2.0 ** -4, 0.0371):
            fns = {name: (lambda fl=fl: _lib.call("ivit_ibert_layernorm_i8", _lib.ptr(x), C, rows, C, s_in, _lib.ptr(b), _lib.ptr(s), 1.0, _lib.ptr(m),
                                                  _lib.ptr(e), _lib.ptr(out), C, fl, _lib.stream_ptr())) for name, fl in (("float_sqrt", 0), ("int_sqrt", FLAG))}
            print(f"ivit_ibert_layernorm_i8 {rows} x {C} sigma {sigma} s_in {s_in:g}: us per launch (median, min, max)", ab(fns), "rows", slow_rows(q8), flush=True)
    q16 = np.clip(np.rint(rng.normal(0, 6000, size=(rows, C))), -32768, 32767).astype(np.int16)
    x, out = t(q16), torch.empty(rows, C, dtype=torch.int8, device=DEV)
    fns = {name: (lambda fl=fl: _lib.call("ivit_ibert_layernorm_i16_i8_ex", _lib.ptr(x), C, rows, C, 2.0 ** -9, _lib.ptr(b), _lib.ptr(s), 2.0, _lib.ptr(m),
                                          _lib.ptr(e), _lib.ptr(out), C, fl, _lib.stream_ptr())) for name, fl in (("float_sqrt", 0), ("int_sqrt", FLAG))}
    print(f"ivit_ibert_layernorm_i16_i8_ex {rows} x {C} s_in 2^-9 shift 1: us per launch (median, min, max)", ab(fns), flush=True)


def model():
    batch = 256
    engines = {}
    for name, ln_type in (("float_sqrt", "ibert"), ("int_sqrt", ISQRT)):
        mdl = ivit.deit_base_patch16_224(gelu_type="ibert", softmax_type="ibert", layernorm_type=ln_type)
        mdl.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_float_state("deit_base_patch16_224", 7).items()}, strict=False)
        mdl.to(DEV).eval()
        with torch.no_grad():
            mdl(torch.from_numpy(synth.make_images(8, 4242)).to(DEV))
        ivit.freeze_model(mdl)
        eng = mdl.engine(batch)
        assert eng.family == "ibert" and eng.int_sqrt == (name == "int_sqrt"), mdl.engine_unsupported_reason()
        engines[name] = (mdl, eng)
    images = torch.from_numpy(synth.make_images(batch, 5000)).to(DEV)
    fns = {name: (lambda eng=eng: eng.forward_graph(images)) for name, (_, eng) in engines.items()}
    res = ab(fns, rounds=5)
    print(f"DeiT-B I-BERT batch {batch} graph replay: ms per step (median, min, max)",
          {k: tuple(round(v / 1e3, 3) for v in r) for k, r in res.items()}, flush=True)
    eng = engines["int_sqrt"][1]
    taps = {}
    eng.forward(images[:8].contiguous(), taps)
    torch.cuda.synchronize()
    names = ["qact1"] + [f"blocks.{i}.qact{j}" for i in range(12) for j in (2, 4)]
    tot = dict(rows=0, mean_band=0, v_zero=0, v_ge_2p24=0, slow=0)
    for n in names:
        r = slow_rows(taps[n].cpu().numpy().reshape(-1, 768))
        for k in ("rows", "mean_band", "v_zero", "v_ge_2p24"):
            tot[k] += r[k]
        tot["slow"] += r["share"] * r["rows"]
    print("LayerNorm inputs of 8 images (25 LayerNorms):", {**tot, "share": tot["slow"] / tot["rows"]}, flush=True)


if __name__ == "__main__":
    for what in sys.argv[1:] or ["kernel", "model"]:
        {"kernel": kernel, "model": model}[what]()
