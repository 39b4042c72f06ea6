"""Writes tests/golden/qact_percentile_trace.npz: the reference's QuantAct in percentile mode (quant_modules.py:319-360), observed step
by step on the CPU.  The reference is imported unmodified, as oracle/gen_golden.py imports it; the file holds data only.

    python scripts/gen_percentile_trace.py --reference <checkout of the reference>

For p in {99.0, 99.99, 100.0} and act_range_momentum in {0.95, -1}: three successive running-stat forwards of seeded tensors (values
`integer * scale`, as a producer hands them over).  One case adds an `identity` operand, one runs in input mode (no incoming scale).
Per case: the inputs, (x_min, x_max) after every step and the scale every step returned.  tests/test_gpu_quantile.py sends the same
inputs through this package's QuantAct on the device and compares bits."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "qact_percentile_trace.npz")

# (percentile, momentum, shape, kind)
CASES = [
    (99.0, 0.95, (2, 37, 24), "plain"),
    (99.0, -1, (3, 7, 16), "identity"),
    (99.99, 0.95, (1, 50, 64), "identity"),
    (99.99, -1, (2, 3, 16, 16), "input"),
    (100.0, 0.95, (4, 33), "plain"),
    (100.0, -1, (1, 197, 12), "plain"),
]
STEPS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory of the reference (holds models/quantization_utils)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    # the reference's hard-coded .cuda() calls stay on the tensor's device (the shim of oracle/gen_golden.py)
    torch.Tensor.cuda = lambda self, device=None, *a, **k: self if device is None else self.to(device)
    sys.path.insert(0, args.reference)
    import models.quantization_utils as rq

    torch.set_num_threads(1)
    out, meta = {}, []
    for ci, (p, mo, shape, kind) in enumerate(CASES):
        rng = np.random.default_rng(7100 + ci)
        qa = rq.QuantAct(8, act_range_momentum=mo)
        qa.percentile = p
        pre = np.float32(2.0 ** -5)
        idpre = np.float32(2.0 ** -6)
        post, scales = [], []
        for s in range(STEPS):
            spread = (9.0, 14.0, 6.0)[s]                       # the range moves from step to step
            if kind == "input":
                x = (rng.standard_normal(shape) * spread / 10).astype(np.float32)
                x.reshape(-1)[rng.integers(0, x.size, 3)] *= 25      # a few outliers: what the percentile is for
                y, sc = qa(torch.from_numpy(x))
            else:
                z = np.rint(rng.standard_normal(shape) * spread)
                z.reshape(-1)[rng.integers(0, z.size, 3)] *= 20
                x = (z.astype(np.float32) * pre).astype(np.float32)
                if kind == "identity":
                    z2 = np.rint(rng.standard_normal(shape) * 2 * spread)
                    ident = (z2.astype(np.float32) * idpre).astype(np.float32)
                    out[f"c{ci}/id{s}"] = ident
                    y, sc = qa(torch.from_numpy(x), torch.tensor([pre]), identity=torch.from_numpy(ident),
                               identity_scaling_factor=torch.tensor([idpre]))
                else:
                    y, sc = qa(torch.from_numpy(x), torch.tensor([pre]))
            out[f"c{ci}/x{s}"] = x
            post.append([float(qa.x_min), float(qa.x_max)])
            scales.append(float(sc.reshape(-1)[0]))
        out[f"c{ci}/post"] = np.array(post, np.float32)
        out[f"c{ci}/scale"] = np.array(scales, np.float32)
        out[f"c{ci}/pre"] = np.array([pre, idpre], np.float32)
        meta.append(dict(case=f"c{ci}", percentile=p, momentum=mo, kind=kind, steps=STEPS))
        print(f"c{ci}: p={p} momentum={mo} {kind} {shape}: ranges {post}")
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
