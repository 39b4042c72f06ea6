#!/usr/bin/env python3
"""Headline benchmark: images/s of the integer-only DeiT-B forward (batch 256 per GPU, 224x224
synthetic images resident in HBM) on N MI355X, one process per GPU.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full] (N > 1: spawns its own N ranks)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = one forward of the whole hot path over one batch: input quantisation + im2col, patch-embed
GEMM, 12 blocks (LN, qkv GEMM, fused attention, proj GEMM + residual, LN, fc1 GEMM, ShiftGELU,
fc2 GEMM + residual), final LN, head GEMM, per-class scaling + arg-max; for N > 1 followed by the one
RCCL all-gather of the top-1 indices.  Images are independent, so ranks share nothing else (weak
scaling: 256 images per GPU).  Prints ONE JSON line on rank 0.

A plain run does what the headline figure needs and no more: set-up, phase 1, the outputs if --dump-outputs is given, the
JSON line (`roofline` is null, the keys of phases 3 and 4 are absent).  --full adds phases 2 to 4, which cost several times
what the plain run does.  Separate phases, in this order, so that nothing perturbs the number it does not belong to:
  1. the timed region: W warm-up + K steps, nothing but launches (HIP-graph replay of the forward reading the
     resident image tensor + the all-gather), bracketed by barrier + synchronize;
  2. --full: an instrumented pass (untimed): a few eager forwards with device-scope HIP events around every launch of the
     dominant kernel -> `roofline`;
  3. --full: extra keys of the same line, each with its own barrier-bracketed timed loop (never part of `value`):
     `natural_scales` -- the headline workload with activation ranges AS CALIBRATED (the regime of a real checkpoint), rank 0;
     `config4` -- BASELINE.json's config 4: ViT-B, GLOBAL batch 1024 split over the ranks with parallel.shard_bounds (strong
     scaling: 128 per rank at N = 8), all-gather of the top-1 per step;
  4. --full, rank 0, N = 1 only: the CPU oracle on a bounded sample -> `cpu_baseline`.
--dump-outputs DIR: right after phase 1, rank 0 writes what the last timed step returned (dump_outputs()).  Images and
weights are seeded, so two builds run with the same arguments can be compared array for array.
Each rank pins its host threads to the NUMA node of its GPU before anything touches the GPU (no exec, no re-launch).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MODEL_TAG = "deit_base"
BATCH = 256
CONFIG4_BATCH = 1024               # BASELINE.json configs[3]: ViT-B, batch 1024 sharded over the node's GPUs
MAC_PER_IMAGE = 17.5638e9          # SURVEY.md Appendix C (GEMM + attention + patch-embed + head)
INT8_PEAK_TOPS = 5033.0            # 256 CU x 4 SIMD x 1024 MAC/clk x 2.4 GHz x 2 ops (MI355X_MICROARCH.md)
# the reference's own PyTorch-CPU integer path as shipped, measured in the build container: it
# cannot travel to the GPU box, so the figure is carried as a constant next to the port timed on this host
REFERENCE_AS_IS = {"value": 1.5, "unit": "images/s", "cores": 8,
                   "sample": "reference models/vit_quant.py DeiT-B batch 32 on 8 vCPU Xeon 2.1 GHz, 21.0 s/batch (BASELINE.md)"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run everything that is not the headline figure: the instrumented pass "
                         "(`roofline`), the natural_scales and config4 keys, the CPU baseline.  Off by default: a plain run sets "
                         "up, warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the cpu_baseline key")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the natural_scales and config4 keys (profiling runs)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches in the timed region instead of HIP-graph replay")
    ap.add_argument("--probe-forwards", type=int, default=3, help="with --full: forwards of the instrumented pass (0 = skip)")
    ap.add_argument("--operators", choices=("ivit", "ibert"), default="ivit",
                    help="operator family of GELU / Softmax / LayerNorm: 'ivit' (the headline, BASELINE.json) or 'ibert' (the fork's "
                         "default family; ranges calibrated on the spot, as calibrated; no cpu_baseline)")
    ap.add_argument("--bitwidth", type=int, choices=(8, 16), default=8,
                    help="the reference's quant_train.py --bitwidth: 16 sets all eight width knobs of vit_quant.py:180-187 to 16 "
                         "(16-bit residual stream, softmax output, position embedding; GEMM operands stay int8).  Not the headline.")
    ap.add_argument("--natural-scales", action="store_true",
                    help="the same model with its activation ranges AS CALIBRATED (fixture deit_base_natural) instead of "
                         "power-of-two snapped: the regime of a real checkpoint, phi tables active (DESIGN.md section 2)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy: top1 (every rank's, "
                         "gathered) and rank 0's logits and logits_f (integers as float64, floats as float32; about 3 MB)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ---------------------------------------------------------------------------------------------- launcher
def launch(args, argv):
    """`python bench.py --gpus N` without a rendezvous in the environment: start N ranks of this same script (one per
    GPU) as CHILD processes and wait for them.  Runs before anything in this process touches the GPU (no torch import
    up to here), and never replaces a process image."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "8")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                code = p.poll()
                if code is None:
                    continue
                pending.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in pending:        # one rank died: the others would wait in a collective for ever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc if rc >= 0 else 1


# ---------------------------------------------------------------------------------------------- pieces
_T0 = time.perf_counter()


def progress(msg):
    """one line on STDERR (stdout carries the JSON line alone): a harness that watches for output does not take the quiet phases
    -- building engines, the CPU baseline's passes -- for a hang"""
    if os.environ.get("RANK", "0") == "0":
        sys.stderr.write(f"[bench.py +{time.perf_counter() - _T0:6.1f} s] {msg}\n")
        sys.stderr.flush()


def usable_cpus():
    """CPUs this process may actually use: its affinity mask, cut to the cgroup's CPU quota when there is one (a container with a
    16-CPU share on a 256-CPU host: 128 OpenMP threads over the NUMA node's mask only fight for the quota)"""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(int(parts[0]) / int(parts[1]))))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                        n = min(n, max(1, q // int(f.read().split()[0])))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def pmc_traffic(kernel_keys):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 --pmc summary (FETCH_SIZE /
    WRITE_SIZE passes, corrected as MI355X_MICROARCH.md prescribes; scripts/summarize_profiles.py)."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_summary.json")), reverse=True):
        try:
            pmc = json.load(open(path))["pmc"]
        except (KeyError, ValueError):
            continue
        for key in kernel_keys:
            v = pmc.get(key, {}).get("hbm_bytes_per_launch_corrected")
            if v is not None:
                return v, os.path.basename(path)
    return None, None


def cpu_baseline(fs, ranges, cfg):
    """The CPU oracle (port of the reference's integer algorithm, oracle/ivit_oracle.c) timed on this host's cores on a
    bounded sample of the same workload: 2 warm-up passes, median of ALWAYS 5 timed passes -- the sample size
    (32, 16, 8 or 4 images per pass) is chosen from the first warm-up so that the seven passes stay near half a minute, instead
    of cutting the pass count on a slow host.  It is a correctness port -- OpenMP over rows, a row-blocked int8 GEMM on
    16-bit dot products, everything else scalar -- not a tuned CPU path."""
    import numpy as np
    from ivit_amd import synth
    from oracle import oracle as orc
    om = orc.OracleViT(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"])
    cpus = usable_cpus()
    if cpus < orc.max_threads():
        orc.set_threads(cpus)
    progress(f"cpu_baseline: C oracle on {min(cpus, orc.max_threads())} thread(s); first warm-up (8 images)")
    n = 8
    t0 = time.perf_counter()
    om.forward(synth.make_images(n, 31337))
    first = time.perf_counter() - t0                 # includes first-touch costs: an upper estimate of a pass of 8 images
    n = 32 if first * 4 * 6 <= 30.0 else 16 if first * 2 * 6 <= 40.0 else 8 if first * 6 <= 40.0 else 4      # ~10-30 s of CPU work in all
    imgs = synth.make_images(n, 31337)
    times = []
    for i in range(6):                               # one more warm-up at the chosen size, then the five timed passes
        t0 = time.perf_counter()
        om.forward(imgs)
        times.append(time.perf_counter() - t0)
        progress(f"cpu_baseline: pass {i + 1} of 6 ({n} images) {times[-1]:.2f} s")
    timed = sorted(times[1:])
    med = timed[len(timed) // 2]
    threads = min(cpus, orc.max_threads())
    rows = n * 197
    return {"value": round(n / med, 3), "unit": "images/s", "cores": threads, "kind": "port",
            "sample": f"DeiT-B INT8, forwards of {n} images (224x224 synthetic; {rows} token rows over {threads} OpenMP threads = "
                      f"{rows / max(threads, 1):.0f} rows per thread): 2 warm-ups (8 images {first:.2f} s, {n} images {times[0]:.2f} s), median "
                      f"of {len(timed)} timed passes = {med:.2f} s (all: {', '.join(f'{t:.2f}' for t in times[1:])} s); a correctness "
                      "port of the integer algorithm (row-blocked int8 GEMM, otherwise scalar), not a tuned CPU path",
            "reference_as_is": REFERENCE_AS_IS}


def numa_cpus_of_gpu(local_rank, sysfs="/sys", allowed=None, why=None):
    """CPUs of the NUMA node the rank's GPU hangs off (sysfs; GPUs in PCI bus order = the order HIP enumerates them), or None.
    `why` (a list) receives the reason when there is no answer -- it goes into the JSON line, so that a box without the
    information says which piece is missing (round 3: the driver's box reported "no NUMA information" and nothing else).
    `sysfs` / `allowed`: test hooks (tests/test_host_logic.py builds a fake tree)."""
    import glob

    def no(reason):
        if why is not None:
            why.append(reason)
        return None
    try:
        devs = []
        for d in glob.glob(os.path.join(sysfs, "class/drm/card[0-9]*/device")):
            real = os.path.realpath(d)
            try:
                with open(os.path.join(real, "vendor")) as f:
                    if f.read().strip() != "0x1002":
                        continue
                with open(os.path.join(real, "class")) as f:
                    cls = f.read().strip()
            except OSError:
                continue      # not a PCI function (round 4: the driver's box lists /sys/devices/platform/amdgpu_xcp_NN partition nodes)
            if not (cls.startswith("0x03") or cls.startswith("0x12")):      # display controller / processing accelerator
                continue
            devs.append(real)
        if not devs:
            return no(f"no AMD GPU under {sysfs}/class/drm")
        devs = sorted(set(devs), key=os.path.basename)
        vis = os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES")
        if vis:
            order = [int(v) for v in vis.split(",") if v.strip().isdigit()]
            devs = [devs[i] for i in order if i < len(devs)]
        if local_rank >= len(devs):
            return no(f"rank {local_rank} but {len(devs)} GPU(s) in sysfs")
        with open(os.path.join(devs[local_rank], "numa_node")) as f:
            node = int(f.read().strip())
        if node < 0:
            return no(f"numa_node = {node} for {os.path.basename(devs[local_rank])} (single-node host or a VM without NUMA topology)")
        with open(os.path.join(sysfs, f"devices/system/node/node{node}/cpulist")) as f:
            cpus = set()
            for part in f.read().strip().split(","):
                a, _, b = part.partition("-")
                cpus.update(range(int(a), int(b or a) + 1))
        if allowed is None:
            allowed = os.sched_getaffinity(0)
        both = cpus & set(allowed)
        if not both:
            return no(f"node {node} has CPUs {min(cpus)}-{max(cpus)}, none of them in this process's affinity mask")
        return both
    except (OSError, ValueError) as e:
        return no(f"{type(e).__name__}: {e}")


def pin_to_numa(local_rank):
    """os.sched_setaffinity in this (child) process BEFORE anything touches the GPU; returns what was done, for the JSON line"""
    if os.environ.get("IVIT_BENCH_NO_PIN") == "1":
        return "off"
    why = []
    cpus = numa_cpus_of_gpu(local_rank, why=why)
    if not cpus:
        return "not pinned: " + (why[0] if why else "no NUMA information")
    try:
        os.sched_setaffinity(0, cpus)
    except OSError as e:
        return f"refused: {e}"
    return f"{len(cpus)} CPUs of the GPU's NUMA node"


def timed_steps(step, steps, warmup, sync, grouped, dev):
    """W warm-up + K timed calls of `step`, bracketed by barrier + synchronize on both sides; seconds, MAX over ranks"""
    import torch
    import torch.distributed as dist
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    dt = time.perf_counter() - t0
    if grouped:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt


class _StubEngine:
    """CPU stand-in used ONLY by the launcher test (IVIT_BENCH_STUB=1, tests/test_parallel_cpu.py): the rank launch,
    rendezvous, barrier / max-over-ranks timing, all-gather and the JSON line are the real code, the forward is not."""
    dev = "cpu"

    def __call__(self, images):
        import torch
        top1 = (images.reshape(images.shape[0], -1).sum(dim=1).round().to(torch.int64) % 1000).to(torch.int32)
        return None, None, top1

    forward = __call__

    def forward_graph(self, images, resident=False):
        return self(images)


class _KeepLast:
    """--dump-outputs: hands the timed path's forwards to `engine` and keeps what the last one returned (DataParallelTop1
    passes only the top-1 on)"""

    def __init__(self, engine):
        self.engine, self.last = engine, None

    def __call__(self, images):
        self.last = self.engine(images)
        return self.last

    def forward_graph(self, images, resident=False):
        self.last = self.engine.forward_graph(images, resident=resident)
        return self.last


def dump_outputs(path, top1, local):
    """DIR/<name>.npy of the last timed step: the gathered top-1 and this rank's (logits, logits_f).  float64 holds every int32
    exactly; float32 arrays stay float32."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    logits, logits_f, _ = local
    for name, t in (("top1", top1), ("logits", logits), ("logits_f", logits_f)):
        if t is None:      # the launcher test's stub engine computes the top-1 only
            continue
        a = t.detach().cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a.astype(np.float32 if a.dtype == np.float32 else np.float64))


def worker(args):
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    pinned = pin_to_numa(local_rank)      # first thing in the rank's process: before torch is imported, before any GPU call
    import torch
    import torch.distributed as dist
    from ivit_amd.parallel import DataParallelTop1, shard_bounds

    stub = os.environ.get("IVIT_BENCH_STUB") == "1"
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # a rendezvous in the environment (torch.distributed.run, or this script's own launcher) means the distributed path, also
    # for ONE rank: `python -m torch.distributed.run --nproc-per-node 1 bench.py` runs the same RCCL calls as N ranks do
    grouped = world > 1 or "WORLD_SIZE" in os.environ
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")

    # stdout carries ONE JSON line.  RCCL prints a version banner to file descriptor 1 when its communicator comes up (at
    # init_process_group with a device_id, or at the first collective): until the warm-up is over, fd 1 points at stderr.
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    if stub:
        dev, batch = "cpu", 8
        if grouped:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        eng = _StubEngine()
        if os.environ.get("IVIT_BENCH_STUB_FAIL_RANK") == str(rank):   # launcher test: a rank that dies after rendezvous
            os._exit(3)
        images = torch.randint(0, 50, (batch, 3, 4, 4), generator=torch.Generator().manual_seed(rank)).float()
        fs = ranges = cfg = None
    else:
        from ivit_amd import synth
        from ivit_amd.checkpoint import load_synthetic_model
        from ivit_amd.engine import IntViTEngine
        batch = BATCH
        torch.cuda.set_device(local_rank)
        dev = f"cuda:{local_rank}"
        if grouped:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
        if args.operators == "ibert" or args.bitwidth != 8:
            # no fixture for these at DeiT-B: build the module tree, calibrate its ranges on one small batch, freeze, and take
            # the fused engine the frozen model dispatches to (dispatch.py)
            import ivit_amd as ivit
            knobs = ("patch_embed_bw", "pos_encoding_bw", "block_input_bw", "attention_out_bw", "softmax_bw", "mlp_out_bw",
                     "norm2_in_bw", "att_block_out_bw")
            op = args.operators
            model = ivit.deit_base_patch16_224(gelu_type=op, softmax_type=op, layernorm_type=op, **{k: args.bitwidth for k in knobs})
            model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_float_state("deit_base_patch16_224", 7).items()},
                                  strict=False)
            model.to(dev).eval()
            with torch.no_grad():
                model(torch.from_numpy(synth.make_images(8, 4242)).to(dev))
            ivit.freeze_model(model)
            eng = model.engine(batch)
            assert eng.family == args.operators and eng.stream_bits == args.bitwidth, model.engine_unsupported_reason()
            fs = ranges = cfg = None
        else:
            fs, ranges, cfg, meta, _ = load_synthetic_model(MODEL_TAG + ("_natural" if args.natural_scales else ""))
            eng = IntViTEngine(fs, ranges, cfg["embed_dim"], cfg["depth"], cfg["num_heads"], device=dev, max_batch=batch)
        images = torch.from_numpy(synth.make_images(batch, 5000 + rank)).to(dev)  # resident in HBM
    keep = _KeepLast(eng) if args.dump_outputs else None
    dp = DataParallelTop1(eng if keep is None else keep, world, graph=not args.no_graph)

    def sync():
        if grouped:
            dist.barrier()
        if not stub:
            torch.cuda.synchronize()

    # ---- phase 1: the timed region
    progress(f"engine ready; {args.warmup} warm-up + {args.steps} timed steps")
    for _ in range(args.warmup):
        dp.step(images)
    if grouped:
        dp.step(images)          # at least one collective before fd 1 comes back, also with --warmup 0
    sync()
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        top1 = dp.step(images)
    sync()
    dt = time.perf_counter() - t0
    if grouped:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:      # before phase 2: its forwards write the same workspace
        dump_outputs(args.dump_outputs, top1, keep.last)
        progress(f"outputs of the last timed step written to {args.dump_outputs}")

    # ---- phase 2 (--full): dominant-kernel duration, outside the timed region
    progress(f"timed region done: {dt / args.steps * 1e3:.3f} ms per step" + ("; probing the dominant kernel" if args.full else ""))
    roof = None
    if args.full and rank == 0 and not stub and args.probe_forwards > 0:
        from ivit_amd.hiptime import KernelProbe
        eng.forward(images)
        torch.cuda.synchronize()
        probe = KernelProbe(select=lambda tag: tag == "gemm_resid")
        eng.probe = probe
        for _ in range(args.probe_forwards):
            eng.forward(images)
        torch.cuda.synchronize()
        eng.probe = None
        rows = probe.results()
        # an event pair costs a few microseconds of its own (marker packets between the kernels): the pair recorded around
        # nothing right after each launch measures that in the same queue state, and is subtracted
        # `achieved` / `frac` come from the RAW per-launch durations.  An event pair costs a few microseconds of its own (marker
        # packets between the kernels); the pair recorded around nothing right after each launch measures that in the same queue
        # state and is reported as a separate key -- subtracting it overshoots rocprofv3's kernel duration by ~2 us
        raw = [r[1] for r in rows]
        overhead = sum(r[3] for r in rows) / len(rows)
        ms = raw
        macs = [float(M) * N * K for _, _, (M, N, K), _ in rows]
        avg_ms = sum(ms) / len(ms)
        achieved = 2.0 * sum(macs) / (sum(ms) * 1e-3) / 1e12
        traffic, traffic_src = (None, None) if args.bitwidth != 8 else pmc_traffic(("gemm_i8_wreg_kernel<1, 4096, true>", "gemm_i8_wreg_kernel<1, 0, true>", "gemm_i8_wreg_kernel<1, 0>", "gemm_i8_wreg_kernel<1>", "gemm_i8_pers_kernel<1, 0>", "gemm_i8_pers_kernel<1>"))   # names as profiled
        roof = {"bound": "mfma", "kernel": "gemm_i8_wreg_kernel<EPI_RESID> (attn.proj + mlp.fc2, residual QuantAct fused)" if args.bitwidth == 8
                else "gemm_i8_wreg_kernel<EPI_RQ16_RES16> (attn.proj + mlp.fc2, 16-bit QuantAct + 16-bit residual QuantAct fused)",
                "achieved": round(achieved, 1), "peak": INT8_PEAK_TOPS, "unit": "TFLOP/s",
                "frac": round(achieved / INT8_PEAK_TOPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                "launches": len(ms), "avg_launch_ms": round(avg_ms, 4),
                "event_pair_overhead_ms": round(overhead, 4),
                "frac_minus_event_overhead": round(2.0 * sum(macs) / (max(sum(raw) - overhead * len(raw), 1e-9) * 1e-3) / 1e12 / INT8_PEAK_TOPS, 4),
                "algorithmic_ops_per_launch": 2.0 * sum(macs) / len(macs),
                "how": f"device-scope HIP events around each of the {len(ms)} launches in {args.probe_forwards} eager "
                       "forwards run after the timed region (raw durations; the cost of an empty event pair is `event_pair_overhead_ms`)"}
    if grouped:
        dist.barrier()

    # ---- phase 3 (--full): extra keys, each with its own timed loop (never part of `value`)
    headline = args.operators == "ivit" and args.bitwidth == 8 and not args.natural_scales
    natural = None
    config4 = None
    if args.full and stub and not args.no_extras:
        # launcher self-test: the config-4 code path (uneven shards, padded all-gather, timing) with the stub engine over gloo
        n4 = 33
        lo, hi = shard_bounds(n4, world, rank)
        images4 = torch.randint(0, 50, (hi - lo, 3, 4, 4), generator=torch.Generator().manual_seed(100 + rank)).float()
        dp4 = DataParallelTop1(_StubEngine(), world, graph=False, counts=[b - a for a, b in (shard_bounds(n4, world, r) for r in range(world))])
        got = dp4.step(images4)
        assert got.numel() == n4
        dt4 = timed_steps(lambda: dp4.step(images4), 3, 1, sync, grouped, dev)
        config4 = {"workload": f"launcher self-test: {n4} images over {world} rank(s)", "ms_per_step": round(dt4 / 3 * 1e3, 3),
                   "images_per_s": round(n4 * 3 / dt4, 1), "steps": 3, "per_rank_batch": hi - lo, "scaling": "strong"}
    if args.full and headline and not stub and not args.no_extras:
        del dp
        eng = None
        torch.cuda.empty_cache()
        k_extra = max(5, min(args.steps, 20))
        # (a) the headline workload with ranges as calibrated: rank 0 alone (the other ranks wait at the barrier below)
        progress("extras: the headline workload at natural scales")
        if rank == 0:
            fs_n, ranges_n, cfg_n, _, _ = load_synthetic_model(MODEL_TAG + "_natural")
            eng_n = IntViTEngine(fs_n, ranges_n, cfg_n["embed_dim"], cfg_n["depth"], cfg_n["num_heads"], device=dev, max_batch=batch)
            dt_n = timed_steps(lambda: eng_n.forward_graph(images, resident=True), k_extra, 3, torch.cuda.synchronize, False, dev)
            natural = {"ms_per_step": round(dt_n / k_extra * 1e3, 3), "value": round(batch * k_extra / dt_n, 1), "unit": "images/s",
                       "steps": k_extra, "n_gpus": 1,
                       "what": "the same workload with activation ranges as calibrated (fixture deit_base_natural: phi tables at all 61 sites)"}
            del eng_n
            torch.cuda.empty_cache()
        if grouped:
            dist.barrier()
        # (b) config 4: ViT-B, global batch 1024 split over the ranks (strong scaling)
        progress("extras: config 4 (ViT-B, global batch 1024)")
        lo, hi = shard_bounds(CONFIG4_BATCH, world, rank)
        fs4, ranges4, cfg4, _, _ = load_synthetic_model("vit_base")
        eng4 = IntViTEngine(fs4, ranges4, cfg4["embed_dim"], cfg4["depth"], cfg4["num_heads"], device=dev, max_batch=hi - lo)
        images4 = torch.from_numpy(synth.make_images(hi - lo, 7000 + rank)).to(dev)
        dp4 = DataParallelTop1(eng4, world, graph=not args.no_graph, counts=[b - a for a, b in (shard_bounds(CONFIG4_BATCH, world, r) for r in range(world))])
        dt4 = timed_steps(lambda: dp4.step(images4), k_extra, 2, sync, grouped, dev)
        config4 = {"workload": f"ViT-B INT8, global batch {CONFIG4_BATCH} split over {world} rank(s) (parallel.shard_bounds), all-gather of the top-1 per step",
                   "ms_per_step": round(dt4 / k_extra * 1e3, 3), "images_per_s": round(CONFIG4_BATCH * k_extra / dt4, 1), "steps": k_extra,
                   "per_rank_batch": hi - lo, "scaling": "strong"}
        del dp4, eng4

    if rank == 0:
        value = world * batch * args.steps / dt
        out = {"metric": "images/sec DeiT-B INT8 @batch256, 1→8 MI355X; % INT8 MFMA peak",
               "value": round(value, 1), "unit": "images/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "full": args.full, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "int8", "data": "synthetic",
               "config": {"workload": "DeiT-B INT8 integer-only forward, batch 256 per GPU, 224x224" if not stub
                          else "launcher self-test (stub engine, CPU, gloo)",
                          "global_batch": world * batch, "parallelism": f"dp{world}",
                          "launch": "eager" if args.no_graph else "hip-graph replay",
                          "bitwidth": args.bitwidth,
                          "activation_ranges": "as calibrated (natural scales)" if (args.natural_scales or args.operators == "ibert" or args.bitwidth != 8)
                          else "power-of-two",
                          "operators": "I-ViT (IVITIntLayerNorm, Shiftmax, ShiftGELU)" if args.operators == "ivit"
                          else "I-BERT (IBERTIntLayerNorm, IBERTIntSoftmax, IBERTIntGELU)"},
               "mfma_util_end_to_end": round(value / world * MAC_PER_IMAGE / 2.5166e15, 4),
               "roofline": roof, "host_affinity": pinned}
        if natural is not None:
            out["natural_scales"] = natural
        if config4 is not None:
            out["config4"] = config4
        if args.full and world == 1 and not stub and not args.no_cpu_baseline and args.operators == "ivit" and args.bitwidth == 8:
            out["cpu_baseline"] = cpu_baseline(fs, ranges, cfg)
        print(json.dumps(out, ensure_ascii=False), flush=True)
    if grouped:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch(args, argv)
    return worker(args)


if __name__ == "__main__":
    sys.exit(main())
