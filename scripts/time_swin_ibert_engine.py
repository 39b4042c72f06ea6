"""Swin-T at 224 px, batch 128, three ways in one process: the I-BERT operators through the fused engine
(swin_engine.engine_from_model: eager and graph replay), the same frozen model module by module (the integer-carrying path of
quantization_utils/lazy.py), and the I-ViT operators through the fused engine.  Device events, profiler off, median (smallest ..
largest) of seven windows after warm-up; the three are measured in turn, twice, so that a drift of the box shows:

    python scripts/time_swin_ibert_engine.py            # one JSON line

A kernel trace of the I-BERT engine alone (ten eager forwards after warm-up), in a run of its own:

    rocprofv3 --kernel-trace --stats -d prof -o swin_ibert -- python scripts/time_swin_ibert_engine.py profile

Numbers: DESIGN.md section 5 ("Swin with the I-BERT operators in the fused engine")."""
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402
from ivit_amd import _lib  # noqa: E402
from ivit_amd.swin_engine import engine_from_model  # noqa: E402

DEV = "cuda:0"
BATCH = 128
SWIN_T = dict(img_size=224, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), num_classes=1000)


def model(seed, **ops):
    """Swin-T with widened random weights, calibrated on the GPU (ranges as calibrated), frozen -- scripts/time_ibert_module_paths.py"""
    torch.manual_seed(seed)
    m = ivit.SwinTransformer(**SWIN_T, **ops).to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        c = torch.randn(2, 3, 224, 224, generator=g).to(DEV)
        m(c)
        m(c.flip(0) * 0.7)
    ivit.freeze_model(m)
    return m, torch.randn(BATCH, 3, 224, 224, generator=g).to(DEV)


def timed(fn, reps, windows=7):
    ts = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3))


def launches(fn):
    names, real = [], _lib.call
    try:
        _lib.call = lambda n, *a: (names.append(n), real(n, *a))[1]
        fn()
    finally:
        _lib.call = real
    return names


def main():
    warnings.simplefilter("ignore")
    ib = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
    m_ib, x = model(3, **ib)
    eng_ib = engine_from_model(m_ib, max_batch=BATCH)
    if sys.argv[1:2] == ["profile"]:
        for _ in range(3):
            eng_ib.forward(x)
        torch.cuda.synchronize()
        for _ in range(10):
            eng_ib.forward(x)
        torch.cuda.synchronize()
        return
    m_iv, x_iv = model(3)
    eng_iv = engine_from_model(m_iv, max_batch=BATCH)
    with torch.no_grad():
        m_ib.use_engine = m_iv.use_engine = False      # model(x): module by module, for both
        y_mod = m_ib(x)
        names = launches(lambda: eng_ib.forward(x))
        res = dict(model="swin_t_224", batch=BATCH, launches_per_forward=len(names),
                   ibert_engine_equals_module_path=bool(torch.equal(eng_ib.forward(x)[1], y_mod)),
                   ivit_engine_equals_module_path=bool(torch.equal(eng_iv.forward(x_iv)[1], m_iv(x_iv))),
                   fused_fc1_gelu_launches=names.count("ivit_gemm_i8_requant_lut_ex"), series=[])
        for f in (lambda: eng_ib.forward(x), lambda: eng_ib.forward_graph(x), lambda: eng_iv.forward(x_iv), lambda: eng_iv.forward_graph(x_iv),
                  lambda: m_ib(x)):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        for _ in range(2):
            res["series"].append(dict(ibert_engine_eager=timed(lambda: eng_ib.forward(x), 20),
                                      ibert_engine_graph=timed(lambda: eng_ib.forward_graph(x), 20),
                                      ibert_module_path=timed(lambda: m_ib(x), 3),
                                      ivit_engine_eager=timed(lambda: eng_iv.forward(x_iv), 20),
                                      ivit_engine_graph=timed(lambda: eng_iv.forward_graph(x_iv), 20)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
