"""Graph replay of the frozen module-by-module forward (graph.ModuleGraph.forward_graph) against the eager `model(x)`, for
configurations the fused engines decline (or, `use_engine = False`, are kept from).  One process, device events, profiler off: after
the capture, five repetitions of each side, alternating eager / replay; a repetition is the median of five forwards timed one by one.

    python scripts/time_module_graph.py [--out DIR] [config ...]      # one JSON line per configuration, and DIR/module_graph_<config>.json

The condition the numbers are read against: the slowest replay repetition is faster than the fastest eager repetition of the same
run.  `graph_pool_mib`: device memory the graph holds (its private pool keeps every intermediate of the forward): reserved memory
after the capture against before it, the allocator's cache emptied both times.  For a kernel trace of one side, in a run of its own
(eight forwards, set apart from the warm-up by a pause of 0.2 s in the kernels' timestamps):

    rocprofv3 --kernel-trace --stats -d prof -o run -- python scripts/time_module_graph.py --trace eager|replay swin_t_b128_ivit

Numbers: DESIGN.md section 5 ("Graph replay of the module path")."""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import ivit_amd as ivit  # noqa: E402

DEV = "cuda:0"
IBERT = dict(gelu_type="ibert", softmax_type="ibert", layernorm_type="ibert")
SWIN_T = dict(img_size=224, patch_size=4, window_size=7, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), num_classes=1000)
SWIN_B_384 = dict(img_size=384, patch_size=4, window_size=12, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), num_classes=1000)
W16 = dict(patch_embed_bw=16, pos_encoding_bw=8, block_input_bw=16, attention_out_bw=16, softmax_bw=8, mlp_out_bw=16, norm2_in_bw=16,
           att_block_out_bw=16)
# config -> (constructor, image size, batch, use_engine)
CONFIGS = {
    "swin_t_b128_ivit": (lambda: ivit.SwinTransformer(**SWIN_T), 224, 128, False),
    "swin_t_b128_ibert": (lambda: ivit.SwinTransformer(**SWIN_T, **IBERT), 224, 128, True),
    "swin_b_384_b64": (lambda: ivit.SwinTransformer(**SWIN_B_384), 384, 64, False),
    "deit_b_b256_gelu_ibert": (lambda: ivit.deit_base_patch16_224(gelu_type="ibert"), 224, 256, True),
    "deit_b_384_b64_w16": (lambda: ivit.VisionTransformer(img_size=384, patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4,
                                                          qkv_bias=True, **W16), 384, 64, True),
}


def build(make, img, seed=3):
    torch.manual_seed(seed)
    m = make().to(DEV).eval()
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for _, p in m.named_parameters():
            if p.dim() > 1:
                p.mul_(3.0)
        c = torch.randn(2, 3, img, img, generator=g).to(DEV)
        m(c)
        m(c.flip(0) * 0.7)
    ivit.freeze_model(m)
    return m, g


def repetition(fn, forwards=5):
    """median of `forwards` forwards, each between its own pair of events"""
    ts = []
    for _ in range(forwards):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(ts[len(ts) // 2], 3)


def measure(name, trace=None):
    make, img, B, use_engine = CONFIGS[name]
    m, g = build(make, img)
    m.use_engine = use_engine
    x = torch.randn(B, 3, img, img, generator=g).to(DEV)
    res = dict(config=name, batch=B, engine_declines=m.engine_unsupported_reason(), use_engine=use_engine)
    assert not m.takes_engine(x), "the configuration must run module by module"
    with torch.no_grad():
        y = m(x).clone()
        m(x)
        if trace == "eager":
            torch.cuda.synchronize()
            time.sleep(0.2)
            for _ in range(8):
                m(x)
            torch.cuda.synchronize()
            return None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_reserved()
        yg = m.forward_graph(x, resident=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        res["graph_pool_mib"] = round((torch.cuda.memory_reserved() - before) / 2 ** 20, 1)
        res["equal"] = bool(torch.equal(yg, y))
        if trace == "replay":
            torch.cuda.synchronize()
            time.sleep(0.2)
            for _ in range(8):
                m.forward_graph(x, resident=True)
            torch.cuda.synchronize()
            return None
        eager, replay = [], []
        for _ in range(5):
            # (eager first: for a model with a literal step its eager call moves published buffers, and the replay that follows
            # captures again -- outside the timed forwards, by one untimed call)
            eager.append(repetition(lambda: m(x)))
            m.forward_graph(x, resident=True)
            replay.append(repetition(lambda: m.forward_graph(x, resident=True)))
        m.graph_status()
    res.update(eager_ms=eager, replay_ms=replay, eager_median_ms=sorted(eager)[2], replay_median_ms=sorted(replay)[2],
               slowest_replay_below_fastest_eager=bool(max(replay) < min(eager)))
    m.drop_graphs()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"))
    ap.add_argument("--trace", choices=["eager", "replay"])
    ap.add_argument("configs", nargs="*", default=list(CONFIGS))
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    os.makedirs(args.out, exist_ok=True)
    for name in args.configs:
        res = measure(name, args.trace)
        if res is not None:
            print(json.dumps(res), flush=True)
            with open(os.path.join(args.out, f"module_graph_{name}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
