#!/usr/bin/env python3
"""Headline benchmark: sampled trajectories/sec of the RAMP energy-based diffusion sampler on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A "step" is ONE whole sampling job of the workload BASELINE.json quotes the metric on
(configs[1]: Maze2D static, B = 4096 trajectories, H = 48, S = 4, T = 25 DDPM reverse steps with
CFG (2 network rows per trajectory), 1k-point cloud, APF on for forward_t > 20): 25 x 8192 score-net
forward+backward evaluations, the sampler arithmetic, the final RCCL all-gather (N > 1).  Inputs
(weights, scene latent, noise, hard conditions) are resident in HBM when the timed region starts.
Weak scaling: every rank samples its own B trajectories; value = N*B*K / max-over-ranks time.

Without a torchrun environment `python bench.py --gpus N` (N > 1) starts its own N ranks (a parent that never touches the
GPU spawns one child per GPU with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set) and exits non-zero unless all N ran.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run does only what that line's headline needs: set-up,
the warm-up jobs, the K timed jobs, --dump-outputs.  --full adds everything else the benchmark measures, on rank 0 of a one-GPU run
after the timed region: `solution_quality` of the last batch, `guard_trip`, `roofline` (HIP-event timing of the dominant KERNEL,
ramp::ffx_kernel<fwd | bwd>, on its launch stream, priced against the fp16 matrix pipe it executes on; `class_frac` = the same
for the whole split-precision GEMM class), the bf16x6 and exact fp32-MFMA modes, configs 3 / 4 / 5 as `other_configs`, and
`cpu_baseline` (an eager PyTorch-CPU model of the same architecture, oracle/torch_cpu.py, pinned to the reference's
outputs, timed on this host's cores on a bounded sample; the numpy oracle's rate is reported beside it).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# reduced algorithmic FLOPs per sample-eval (fwd + bwd), 2-D S=4 H=48
FLOP_PER_ROW_EVAL = 1.324e9
PEAK_FP32_MFMA_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md, Peak FP32 (matrix)
PEAK_FP16_MFMA_TFLOPS = 2500.0         # same guide: Peak BF16/FP16 MFMA, dense
PEAK_HBM_TBS = 8.0                     # same guide: HBM3E peak (6.3 achievable)
FP16_PRODUCTS_PER_FP32 = 3             # fp16x3: h1h1' + h1h2' + h2h1' per fp32 product


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4096, help="trajectories per GPU (BASELINE configs[1])")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure everything beyond the headline (solution quality, guard trip, roofline, "
                         "bf16x6 / fp32 modes, configs 3 / 4 / 5, CPU baseline); a plain run reports the headline alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full without guard trip, roofline and the bf16x6 / fp32 modes")
    ap.add_argument("--max-rows", type=int, default=0, help="network rows per chunk of a score evaluation (0: all 2 B rows at once)")
    ap.add_argument("--no-calibration-reuse", action="store_true",
                    help="diagnostic: every job calibrates itself in its first evaluation (bf16x6) instead of using the context's canonical "
                         "calibration; jobs are self-contained either way")
    ap.add_argument("--cpu-sample", type=int, default=256, help="trajectories in the PyTorch-CPU baseline sample (halved "
                                                                  "until the projected chain time is <= 40 s)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --batch trajectories PER GPU (the driver's default); strong: --batch trajectories in TOTAL, sharded "
                         "contiguously over the ranks (ramp_amd.dist.shard_counts)")
    ap.add_argument("--preset", choices=["config5-strong"], default=None,
                    help="config5-strong = BASELINE configs[4] as ONE job: --config 5 --scaling strong --batch 65536 (65536 Maze3D "
                         "trajectories, H=64, T=50, 8000-pt cloud, sharded over the --gpus ranks, one RCCL all-gather)")
    ap.add_argument("--noise", choices=["philox", "torch"], default="philox",
                    help="philox: every job draws its N(0, I) inside its captured graph (Philox4x32-10, SURVEY 8(d)); torch: "
                         "torch.randn on the host stream + a copy into the job, like the reference")
    ap.add_argument("--no-other-configs", action="store_true", help="--full without the configs 3 / 4 / 5 sub-lines")
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 4, 5],
                    help="BASELINE.json config (1-based): 2 = headline Maze2D B=4096 H=48 T=25 (default); "
                         "3 = Maze3D B=4096 H=48 T=25 4k-pt cloud; 4 = Maze2D dynamic replanning B=8192 (10 high-level DDIM steps "
                         "+ 3 replans x 5, moving 1024-pt pursuer cloud, one hipGraph per replan); "
                         "5 = Maze3D B=8192/GPU H=64 T=50 8k-pt cloud")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (rank 0; float32, at most "
                         "64 MB: a larger output is replaced by a fixed seeded sample of its rows, DIR/<name>_rows.npy names them)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 64 * 10 ** 6      # --dump-outputs: bytes on disk, the .npy headers included


def dump_output(outdir, name, a):
    """Write the float32 array `a` as outdir/<name>.npy.  Above DUMP_LIMIT_BYTES it is cut to a fixed (seeded, sorted) sample of
    its leading-axis rows, whose indices go to outdir/<name>_rows.npy.  Returns {file name: shape}."""
    os.makedirs(outdir, exist_ok=True)
    a = np.ascontiguousarray(a, dtype=np.float32)
    written = {}
    if a.nbytes > DUMP_LIMIT_BYTES - 4096:
        k = (DUMP_LIMIT_BYTES - 4096) // (a.nbytes // a.shape[0] + 8)          # rows that fit beside their float64 indices
        rows = np.sort(np.random.default_rng(0).choice(a.shape[0], size=k, replace=False)).astype(np.float64)
        a = a[rows.astype(np.int64)]
        np.save(os.path.join(outdir, f"{name}_rows.npy"), rows)
        written[f"{name}_rows.npy"] = list(rows.shape)
    np.save(os.path.join(outdir, f"{name}.npy"), a)
    written[f"{name}.npy"] = list(a.shape)
    return written


WORKLOADS = {   # S, H, T, 3-D?, cloud (n_obstacles, n_points), use_apf
    2: dict(S=4, H=48, T=25, o3=False, cloud=(16, 64), apf=True),
    3: dict(S=6, H=48, T=25, o3=True, cloud=(20, 200), apf=False),
    5: dict(S=6, H=64, T=50, o3=True, cloud=(40, 200), apf=False),
    # dynamic planner: T = 100 schedule, 10 + 3 x 5 = 25 score-network steps per job
    4: dict(S=4, H=48, T=100, o3=False, cloud=(16, 64), apf=False, dynamic=True, evals=25, replans=3),
}
WL = WORKLOADS[2]


MAX_ROWS = None       # --max-rows: network rows per chunk (default: the whole batch, 2 B, in one chunk)
NOISE = "philox"      # --noise


def build_model(B, device, gemm_mode="default"):
    import torch
    from ramp_amd import synth
    from ramp_amd.models import GaussianDiffusionModel3d, StaticGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    sp = make_unet_spec(WL["S"], WL["H"], obstacle_3d=WL["o3"])
    sd = synth.make_unet_state_dict(sp, seed=0)
    unet = TemporalUnetInference(n_support_points=WL["H"], state_dim=WL["S"], unet_input_dim=32, dim_mults=(1, 2, 4, 8),
                                 obstacle_3d=WL["o3"], max_rows=MAX_ROWS or 2 * B, gemm_mode=gemm_mode)
    load_numpy_state_dict(unet, sd)
    if WL.get("dynamic"):
        from ramp_amd.models import DynamicGaussianDiffusionModel
        dm = DynamicGaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=WL["T"],
                                           predict_epsilon=True, use_graph=True)
        dm.apf_dynamic = dict(dm.apf_dynamic, points_per_obstacle=1024)      # pursuer cloud re-sampled to 1024 points per replan
        return dm.eval().to(device), sd
    cls = GaussianDiffusionModel3d if WL["o3"] else StaticGaussianDiffusionModel
    dm = cls(model=unet, variance_schedule="exponential", n_diffusion_steps=WL["T"], predict_epsilon=True,
             compose=False, use_apf=WL["apf"], sampler="ddpm", use_graph=True, noise_source=NOISE, noise_seed=1234)
    dm = dm.eval().to(device)
    return dm, sd


class StepEvents:
    """HIP events on the job's stream around the two halves of every timed step: [start, sampling job done, all-gather done].
    The all-gather's span starts when THIS rank's job is done, so it contains the wait for the slowest rank."""

    def __init__(self):
        self.ev = []

    def mark(self, k):
        import torch
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if k == 0:
            self.ev.append([e])
        else:
            self.ev[-1].append(e)

    def sums(self):
        job = sum(a.elapsed_time(b) for a, b, _ in self.ev) * 1e-3
        gather = sum(b.elapsed_time(c) for _, b, c in self.ev) * 1e-3
        return job, gather


def run_job(dm, B, cloud, hard_conds, world, n_total=None, want_local=False, events=None):
    """One step = one run_inference of this rank's B trajectories + the final all-gather to n_total (default B * world)."""
    import torch
    from ramp_amd import dist as rdist
    if events is not None:
        events.mark(0)
    if WL.get("dynamic"):
        # one job = the high-level plan (10 DDIM steps, one graph) + selection + WL["replans"] replans (5 DDIM steps each,
        # one graph per replan) against a freshly reset pursuit environment; the executed plan (H, S) is the product
        from ramp_amd import compat, synth
        import numpy as np
        np.random.seed(0)
        boxes = synth.make_boxes(WL["cloud"][0], 2, seed=42)
        ctx = {"dataset": compat.make_pursuit_env(boxes, np.full((len(boxes), 2), 0.26), [0.6, 0.55])}
        hc = {k: v.unsqueeze(0).expand(B, -1).contiguous() for k, v in hard_conds.items()}
        x, _chain, _obs, _start = dm.ddim_p_sample_loop((B, WL["H"], WL["S"]), hc, context=ctx, return_chain=False,
                                                        obstacle_pts=cloud, max_iteration=WL["replans"])
        if events is not None:
            events.mark(1); events.mark(2)
        return (x, x) if want_local else x
    x = dm.run_inference(None, hard_conds, n_samples=B, horizon=WL["H"], return_chain=False, traj_normalized=None,
                         obstacle_pts=cloud, sample_fn=None, guide=None, n_guide_steps=1, t_start_guide=7,
                         noise_std_extra_schedule_fn=lambda t: 0.5, n_diffusion_steps_without_noise=0)
    local = x
    if events is not None:
        events.mark(1)
    if world > 1:
        x = rdist.all_gather_trajectories(x.contiguous(), n_total if n_total is not None else B * world)
    if events is not None:
        events.mark(2)
    return (x, local) if want_local else x


def guard_trip_jobs(dm, B, cloud, hard_conds):
    """What leaving the fast path costs: the default job with torch noise whose 4th per-step draw is 3e4 x too large,
    so that evaluation 4 meets operands 2^14 above the maxima its predecessor recorded and the on-device range guard fires.  The job is
    discarded and repeated in fp16x3 with that evaluation calibrating (ramp_set_fallback(ctx, 2)).  Returns the wall time of such a job
    (detection + repeat; the second one, whose repeat graph exists) next to an untripped job drawn the same way."""
    import warnings
    import torch
    real = torch.randn_like
    calls = {"n": 0, "kick": False}

    def randn_like(x, **kw):
        calls["n"] += 1
        z = real(x, **kw)
        return z * 3.0e4 if (calls["kick"] and calls["n"] == 4) else z

    src = dm.noise_source
    dm.noise_source = "torch"
    torch.randn_like = randn_like
    out = {}
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r0, f0 = dm.range_reruns, dm.range_fallbacks
            for key, kick, reps in (("untripped_job_s", False, 2), ("guard_trip_first_job_s", True, 1), ("guard_trip_job_s", True, 2)):
                best = None
                for _ in range(reps):
                    calls["n"], calls["kick"] = 0, kick
                    torch.cuda.synchronize(); tq = time.perf_counter()
                    x = run_job(dm, B, cloud, hard_conds, 1)
                    torch.cuda.synchronize(); dq = time.perf_counter() - tq
                    best = dq if best is None else min(best, dq)
                    assert bool(torch.isfinite(x).all())
                out[key] = best
            out["ended_as"] = dm.last_job_mode
            out["fp16x3_repeats"] = dm.range_reruns - r0
            out["bf16x6_repeats"] = dm.range_fallbacks - f0
            out["ratio_to_untripped"] = out["guard_trip_job_s"] / out["untripped_job_s"]
            out["note"] = ("torch-noise jobs (the noise is drawn on the host stream and copied in, a few ms more than the Philox jobs that are timed "
                           "above); a tripped job = the flagged run + one read-back of the per-evaluation guard log + the same job again on the "
                           "fp16x3 kernels with the flagged evaluation as a calibrating (bf16x6, recording) one; rounds 2-5 repeated it entirely "
                           "on the bf16x6 kernels: 2.83 x")
    finally:
        torch.randn_like = real
        dm.noise_source = src
    return out


def profile_gemm(dm, B, cloud, hard_conds):
    """HIP-event timing of every kernel launch of ONE eager (non-graph) step on the launch stream."""
    import torch
    from ramp_amd import _lib
    lib = _lib.load()
    ctx = dm.model.ctx()
    dm.use_graph = False
    run_job(dm, B, cloud, hard_conds, 1)              # eager warm-up
    torch.cuda.synchronize()
    _lib.check(lib.ramp_profile(ctx, 1))
    run_job(dm, B, cloud, hard_conds, 1)
    ms = (C.c_double * 5)(); fl = (C.c_double * 5)(); cnt = (C.c_int64 * 5)()
    _lib.check(lib.ramp_profile_read(ctx, ms, fl, cnt))
    kms = (C.c_double * 9)(); kfl = (C.c_double * 9)(); kcnt = (C.c_int64 * 9)()
    _lib.check(lib.ramp_profile_read_kernels(ctx, 9, kms, kfl, kcnt))
    _lib.check(lib.ramp_profile(ctx, 0))
    dm.use_graph = True
    names = ["gemm_f32_mfma", "attention", "norm_rows", "small_convs", "sampler"]
    out = {n: {"ms": ms[i], "flops": fl[i], "launches": int(cnt[i])} for i, n in enumerate(names)}
    knames = ["ffx_fwd", "ffx_bwd", "tkl", "tklb", "ato", "abl", "tkc", "tkw", "other_gemm"]
    out["_kernels"] = {n: {"ms": kms[i], "flops": kfl[i], "launches": int(kcnt[i])} for i, n in enumerate(knames)}
    return out


PMC_FILE = next((f for f in ("profiles/r06_pmc_traffic.json", "profiles/r05_pmc_traffic.json")
                 if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), f))), "profiles/r06_pmc_traffic.json")
SUSTAINED_FP32EQ_TFLOPS = 510.0        # profiles/r02_power_clocks.txt, r03_power_clocks.txt: the bare fp16x3 MFMA + LDS-read loop sustains 491-530 TFLOP/s (fp32-
                                       # equivalent) at the 1.4 kW socket limit, i.e. 0.59-0.64 of the 833.3 nominal ceiling
STASH_BYTES_PER_ROW_EVAL = 4.0e6       # what ONE score evaluation must keep per network row for the input
                                       # gradient (conv outputs, norm statistics, per block-token z, qkv, z1, GEGLU stash)


def pmc_traffic(klass):
    """Per-launch HBM traffic of a kernel class from the committed PMC summary: counters need rocprofv3's own passes
    (FETCH_SIZE and WRITE_SIZE do not even fit one pass), so they cannot be collected inside this run.  Returns
    (bytes per launch or None, provenance string)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), PMC_FILE)
    try:
        with open(path) as fh:
            d = json.load(fh)
        return float(d[klass]["hbm_bytes_per_launch"]), f"{PMC_FILE} ({d.get('collected', 'separate rocprofv3 --pmc passes')})"
    except Exception:
        return None, "no PMC summary committed for this round"


def pmc_total():
    """HBM bytes of one whole score evaluation (all kernel classes) from the committed PMC summary, or None."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), PMC_FILE)
    try:
        with open(path) as fh:
            return float(json.load(fh)["total_hbm_bytes_per_evaluation"])
    except Exception:
        return None


def host_cores():
    """Physical cores this process may use (the GPU box hands each GPU a share of the host)."""
    try:
        avail = len(os.sched_getaffinity(0))
    except Exception:
        avail = os.cpu_count() or 1
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or avail
    except Exception:
        phys = avail
    quota = avail
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):      # container CPU share (cgroup v2 / v1)
        try:
            with open(path) as fh:
                parts = fh.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    quota = max(1, int(int(parts[0]) / int(parts[1])))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                        quota = max(1, q // int(fh.read()))
            break
        except Exception:
            continue
    env = os.environ.get("RAMP_CPU_BASELINE_THREADS")
    if env:
        return max(1, int(env))
    return max(1, min(avail, phys, quota))


def cpu_baseline(sd, cloud_np, n_traj):
    """(1) PyTorch-CPU eager model of the same architecture (oracle/torch_cpu.py; same ATen kernels and autograd energy
    gradient as the reference's CPU path, validated against the reference's outputs in tests/) on a bounded sample of
    the headline workload; (2) the numpy oracle on a smaller sample, for continuity with round 1."""
    import torch
    from oracle import ramp_oracle as O
    from oracle.torch_cpu import TorchCpuSampler, TorchCpuScoreNet
    from ramp_amd import synth
    cores = host_cores()
    net = TorchCpuScoreNet(sd, 4, 48)
    # a container may expose more cores than it may use: time one small evaluation per candidate thread count and keep
    # the fastest (over-subscription makes ATen's intra-op pool dramatically slower, not just flat)
    xs = torch.from_numpy(synth.make_noise((64, 48, 4), seed=6)); ts = torch.full((64,), 12, dtype=torch.long)
    ls = torch.zeros((64, 320))
    best = None
    for c in sorted({cores, min(cores, 64), min(cores, 32), min(cores, 16), min(cores, 8)}, reverse=True):
        torch.set_num_threads(c)
        net.score(xs[:8], ts[:8], ls[:8])
        t0 = time.time(); net.score(xs, ts, ls); tc = time.time() - t0
        if best is None or tc < best[0]:
            best = (tc, c)
    cores = best[1]
    torch.set_num_threads(cores)
    u = O.UNetOracle(sd, 4, 48, dtype=np.float32)
    lat = u.encode_scene(cloud_np)
    sched = O.make_schedule(25, np.float32)
    sm = TorchCpuSampler(net, sched, 2.0)
    hc = synth.default_hard_conds(4, 48)
    # size the sample: one score evaluation of 2 x n rows, then the whole chain if it projects to <= 40 s
    n = n_traj
    while True:
        x = torch.from_numpy(synth.make_noise((2 * n, 48, 4), seed=5))
        lt = torch.from_numpy(np.tile(lat[None], (2 * n, 1)).astype(np.float32))
        tt = torch.full((2 * n,), 12, dtype=torch.long)
        net.score(x[:8], tt[:8], lt[:8])                       # first-call overheads out of the estimate
        t0 = time.time(); net.score(x, tt, lt); te = time.time() - t0
        if te * 25 <= 40.0 or n <= 8:
            break
        n //= 2
    noise = synth.make_noise((26, n, 48, 4), seed=1234)
    t0 = time.time()
    sm.ddpm(noise, hc, lat, cloud=cloud_np.reshape(-1, 2), use_apf=True)
    dt = time.time() - t0
    out = {"value": n / dt, "unit": "trajectories/s", "cores": int(cores), "kind": "port",
           "sample": f"eager PyTorch-CPU model of the same architecture (oracle/torch_cpu.py, pinned to the reference's "
                     f"outputs), torch.set_num_threads({cores}), B={n} trajectories x 2 CFG rows, full T=25 DDPM chain + APF, "
                     f"fp32, {dt:.1f} s",
           "torch_version": torch.__version__}
    nn = 4
    sm2 = O.SamplerOracle(u, 25, 2.0, dtype=np.float32)
    t0 = time.time()
    sm2.ddpm(synth.make_noise((26, nn, 48, 4), seed=1234), hc, lat, cloud=cloud_np.reshape(-1, 2), use_apf=True)
    dn = time.time() - t0
    out["numpy_oracle"] = {"value": nn / dn, "unit": "trajectories/s", "sample": f"numpy restatement (the parity oracle), B={nn}, {dn:.1f} s"}
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no torchrun around us: this process becomes a GPU-free parent of args.gpus ranks (one per GPU, RCCL between them)
        from ramp_amd.dist import launch_local_ranks
        sys.exit(launch_local_ranks([os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
    import torch
    import torch.distributed as dist
    from ramp_amd import dist as rdist
    from ramp_amd import synth

    global WL, MAX_ROWS, NOISE
    if args.preset == "config5-strong":
        args.config, args.scaling, args.batch = 5, "strong", 65536
    WL = WORKLOADS[args.config]
    MAX_ROWS = args.max_rows or None
    NOISE = args.noise
    if args.config in (4, 5) and args.batch == 4096:
        args.batch = 8192
    rank, world, local = rdist.env_rank()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a {world}-rank run as "
                         f"{args.gpus} GPUs")
    if world > 1:
        if torch.cuda.device_count() < world:
            raise SystemExit(f"bench.py: {world} ranks but only {torch.cuda.device_count()} visible GPU(s)")
        torch.cuda.set_device(local)
        rdist.init_process_group("nccl")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the RAMP sampler has no CPU path")
    device = torch.device("cuda", local if world > 1 else 0)
    torch.cuda.set_device(device)
    strong = args.scaling == "strong"
    n_total = args.batch if strong else args.batch * world       # trajectories of the whole job
    B = rdist.shard_counts(n_total, world)[rank]                  # this rank's share (weak: --batch on every rank)
    if B == 0:
        raise SystemExit(f"bench.py: --scaling strong with --batch {args.batch} leaves rank {rank} of {world} without work")
    torch.manual_seed(1234 + rank)

    dm, sd = build_model(B, device)
    # noise_source 'philox': ONE stream for the whole job, addressed by global sample index -- the N ranks together draw exactly
    # what a single GPU running all n_total trajectories would draw (ramp_sample_params.philox_sample0 / philox_total)
    dm.noise_seed = 1234
    if hasattr(dm, "set_noise_shard"):
        dm.set_noise_shard(rdist.shard_range(n_total, rank, world)[0], n_total)
    if args.no_calibration_reuse:
        dm.model.set_calibration_reuse(False)
    cloud_np = synth.make_cloud(WL["cloud"][0], WL["cloud"][1], 3 if WL["o3"] else 2, seed=42)   # config 2: 16 x 64 = 1024 pts
    cloud = torch.from_numpy(cloud_np).to(device)
    hard_conds = {k: torch.from_numpy(v).to(device) for k, v in synth.default_hard_conds(WL["S"], WL["H"]).items()}

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    cold = {}
    if rank == 0 and world == 1 and args.config == 2:
        # SURVEY 8(d) "also report including them": what a FRESH context pays before its first trajectory -- weight upload +
        # packing (ramp_load_weight / ramp_finalize_weights), time table + scene encoding, then the first job (graph capture +
        # the context's canonical calibration evaluation); the steady job time is added below.  A plain run keeps this first job
        # too: it is what leaves graph capture and calibration out of the timed steps even at --warmup 0
        torch.cuda.synchronize(); tq = time.perf_counter()
        dm.model.ctx()
        torch.cuda.synchronize(); cold["weight_load_and_pack_s"] = time.perf_counter() - tq
        tq = time.perf_counter()
        dm.model.prepare_time_table(dm.n_diffusion_steps)
        dm._prepare_scene(cloud, B)
        torch.cuda.synchronize(); cold["time_table_and_scene_encode_s"] = time.perf_counter() - tq
        tq = time.perf_counter()
        run_job(dm, B, cloud, hard_conds, world, n_total)
        torch.cuda.synchronize(); cold["first_job_s"] = time.perf_counter() - tq
    for _ in range(args.warmup):
        run_job(dm, B, cloud, hard_conds, world, n_total)
    barrier()
    events = StepEvents()
    fallbacks0 = getattr(dm, "range_fallbacks", 0)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out, out_local = run_job(dm, B, cloud, hard_conds, world, n_total, want_local=True, events=events)
    barrier()
    dt = time.perf_counter() - t0
    dt_local = dt
    if world > 1:
        tt = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    job_s, gather_s = events.sums()
    rank_timing = rdist.rank_timing_report(job_s, gather_s, dt_local, device)      # (a collective: every rank calls it)
    if WL.get("dynamic"):
        assert out.shape == (WL["H"], WL["S"]) and bool(torch.isfinite(out).all())
        gather_check = {"world": dist.get_world_size() if world > 1 else 1, "note": "planner: the ranks' candidates are merged at "
                        "every selection (ramp_amd.dist.select_best_sharded), the product is one (H, S) plan"}
        if world > 1:      # every rank must hold the same executed plan
            ref = out.clone(); dist.broadcast(ref, src=0)
            gather_check["same_plan_on_every_rank"] = bool(torch.equal(ref, out))
            if not gather_check["same_plan_on_every_rank"]:
                raise SystemExit("bench.py: the ranks executed different plans")
    else:
        assert out.shape == (n_total, WL["H"], WL["S"]) and bool(torch.isfinite(out).all())
        # outside the timed region: a second REAL collective proves how many ranks the gathered block came from
        gather_check = rdist.verify_gather(out_local.contiguous(), out, n_total)
        if gather_check["world"] != args.gpus or not gather_check["checksum_ok"] or gather_check["ranks_seen"] != list(range(args.gpus)):
            raise SystemExit(f"bench.py: the all-gather does not show {args.gpus} ranks: {gather_check}")
    dumped = None
    if args.dump_outputs and rank == 0:
        # the last timed step's product as its caller receives it: the gathered (n_total, H, S) trajectories, or the planner's (H, S) plan
        name = "plan" if WL.get("dynamic") else "trajectories"
        dumped = dump_output(args.dump_outputs, name, out.detach().float().cpu().numpy())

    value = n_total * args.steps / dt
    ms_per_step = dt / args.steps * 1e3
    flop_row = {2: 1.324e9, 3: 1.323e9, 4: 1.324e9, 5: 1.773e9}[args.config]          # SURVEY.md §8(d), reduced count
    e2e_tflops_per_gpu = (n_total / world) * 2 * WL.get("evals", WL["T"]) * flop_row / (dt / args.steps) / 1e12

    result = {
        "metric": f"sampled trajectories/sec (H={WL['H']}, T={WL['T']})", "value": value, "unit": "trajectories/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32-emulated (2 x fp16 planes per operand, fp32 accumulate)", "data": "synthetic",
        "gemm_mode": "fp16x3 (default): every fp32 operand is scaled by a power of two and split into 2 fp16 planes (22 "
                     "significand bits), 3 fp16 MFMA products accumulated in fp32; the scales of an evaluation come from the operand "
                     "maxima its predecessor recorded -- for a job's first evaluation, from the context's canonical calibration (one "
                     "bf16x6 evaluation on fixed-seed Philox noise, run once, outside any job: ramp_set_calibration_reuse) -- under an "
                     "on-device range guard (fp32-level accuracy: the parity tests run in this mode); the bf16x6 and exact fp32-MFMA "
                     "modes are timed by --full",
        "jobs_self_contained": "every timed job is independent of the jobs before it (no carried-over maxima, no bf16x6 evaluation inside a "
                               "job); the context's one canonical calibration evaluation is inside cold_start.first_job_s",
        "canonical_calibration": not args.no_calibration_reuse,
        "full": args.full,
        "config": {"workload": {2: "BASELINE configs[1]: Maze2D static DDPM, B=4096 trajectories/GPU x 2 CFG rows, "
                                   "H=48, S=4, T=25, 1024-pt cloud, APF forward_t>20, hipGraph replay",
                                3: "BASELINE configs[2]: Maze3D DDPM (w=5.75), B=4096/GPU x 2 CFG rows, H=48, S=6, T=25, 4000-pt cloud",
                                4: "BASELINE configs[3]: Maze2D dynamic replanning, B=8192 candidates x 2 CFG rows, H=48, 25 score steps "
                                   "(10 high-level DDIM + 3 replans x 5), 1024-pt static + 1024-pt moving pursuer cloud, one hipGraph "
                                   "per replan, device-side APF / costs / selection",
                                5: "BASELINE configs[4]: Maze3D DDPM, B=8192/GPU x 2 CFG rows, H=64, S=6, T=50, 8000-pt cloud"}[args.config],
                   "trajectories_per_gpu": B, "horizon": WL["H"], "state_dim": WL["S"], "n_diffusion_steps": WL["T"],
                   "cloud_points": WL["cloud"][0] * WL["cloud"][1], "sharding": f"sample-batch x{world}, final all-gather only"},
        "e2e_algorithmic_tflops_per_gpu": e2e_tflops_per_gpu,
        "e2e_frac_of_fp16x3_ceiling": e2e_tflops_per_gpu * FP16_PRODUCTS_PER_FP32 / PEAK_FP16_MFMA_TFLOPS,
        "e2e_frac_of_fp32_mfma_peak": e2e_tflops_per_gpu / PEAK_FP32_MFMA_TFLOPS,
        "n_ranks_rccl": gather_check["world"], "gather_check": gather_check,
        "trajectories_total": n_total,
        "workspace_gb": dm.model.workspace_bytes() / 2 ** 30,
        "range_flag": getattr(dm, "range_fallbacks", 0) - fallbacks0,      # timed jobs the fp16x3 range guard sent to bf16x6 (0 expected)
        "noise": "philox4x32-10 + Box-Muller drawn inside every job's captured graph (ramp_sample_params.noise_mode 1)"
                 if NOISE == "philox" and not WL.get("dynamic") else "torch.randn on the host stream, copied into the job",
        # multi-GPU diagnosis: per-rank sampling-job time and the all-gather's own span, over the timed steps
        "rank_timing": rank_timing,
        "scaling_note": "weak: every rank samples --batch trajectories, so --gpus 1 of this mode IS the single-GPU BENCH workload; "
                        "strong: --batch trajectories in total over the ranks (preset config5-strong = BASELINE configs[4], 65536 "
                        "trajectories); value = trajectories of all ranks / max-over-ranks wall time either way",
    }
    if dumped is not None:
        result["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if cold:
        steady = dt / args.steps
        cold["steady_job_s"] = steady
        cold["note"] = ("fresh context on rank 0: weights uploaded and packed, time table + scene encoded, first job = graph capture "
                        "+ the canonical calibration evaluation + a steady job; value_incl_* = B / (weight load + scene encode + ONE steady "
                        "job), i.e. a cold start that replays an existing graph; value_first_job_* additionally pays capture + calibration")
        result["cold_start"] = cold
        result["value_incl_scene_encode_and_weight_load"] = B / (cold["weight_load_and_pack_s"] + cold["time_table_and_scene_encode_s"] + steady)
        result["value_first_job_incl_everything"] = B / (cold["weight_load_and_pack_s"] + cold["time_table_and_scene_encode_s"] + cold["first_job_s"])
    if args.full and rank == 0 and not WL["o3"] and not WL.get("dynamic"):
        # solution quality of the last timed batch, outside the timed region (on-device metrics);
        # the weights are random, so this only shows that the metric path runs at the benchmark's batch size
        from ramp_amd.metrics import Metrics
        boxes = synth.make_boxes(WL["cloud"][0], 2, seed=42)
        tq = time.perf_counter()
        mt = Metrics()
        loc = out[:B].contiguous()
        ci = mt.compute_collision_intensity(loc, boxes.astype(np.float32), np.full((len(boxes), 2), 0.26, np.float32))
        q = mt.trajectory_success_and_metrics(loc, ci, threshold=0.01)
        torch.cuda.synchronize()
        result["solution_quality"] = {k: q[k] for k in ("success", "collision_intensity", "path_length", "path_length_std",
                                                         "waypoint_variance", "n_free_trajectories")}
        result["solution_quality"]["metrics_ms"] = (time.perf_counter() - tq) * 1e3
        result["solution_quality"]["note"] = "random-init weights: not a planning-quality claim"

    if args.full and rank == 0 and world == 1 and args.config == 2 and not args.no_roofline:
        result["guard_trip"] = guard_trip_jobs(dm, B, cloud, hard_conds)
    if args.full and rank == 0 and world == 1 and not args.no_roofline and not WL.get("dynamic"):
        prof = profile_gemm(dm, B, cloud, hard_conds)
        kern = prof.pop("_kernels")
        g = prof["gemm_f32_mfma"]
        class_achieved = g["flops"] / (g["ms"] * 1e-3) / 1e12
        total_ms = sum(v["ms"] for v in prof.values())
        peak = PEAK_FP16_MFMA_TFLOPS / FP16_PRODUCTS_PER_FP32
        traffic, traffic_src = pmc_traffic("ffx")
        # THE DOMINANT KERNEL = ramp::ffx_kernel<fwd | bwd> (the token-owning fused feed-forward, ~48 % of all kernel time):
        # frac = (algorithmic FLOPs of ITS launches) / (ITS summed HIP-event time) / 833.3 -- fixed from round 5 on; the figure
        # of the whole split-precision GEMM class (rounds 1-4's `frac`) is `class_frac`
        fx_ms = kern["ffx_fwd"]["ms"] + kern["ffx_bwd"]["ms"]
        fx_fl = kern["ffx_fwd"]["flops"] + kern["ffx_bwd"]["flops"]
        fx_n = kern["ffx_fwd"]["launches"] + kern["ffx_bwd"]["launches"]
        achieved = fx_fl / (fx_ms * 1e-3) / 1e12 if fx_ms > 0 else 0.0
        avg_us = fx_ms * 1e3 / max(fx_n, 1)
        result["roofline"] = {
            "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
            # field history, so that round-over-round parsers do not mix definitions: rounds 1-4 `frac` = the whole split-precision
            # GEMM class (now `class_frac`); round 5 on `frac` = `frac_ffx` = the dominant kernel pair alone
            "frac_ffx": achieved / peak, "frac_definition": "dominant kernel pair (fused feed-forward) since round 5; rounds 1-4: class_frac",
            "traffic": traffic, "traffic_source": traffic_src,
            "hbm_frac": (traffic / (avg_us * 1e-6) / 1e12 / PEAK_HBM_TBS) if traffic else None,
            "kernel": "ramp::ffx16_kernel<BWD = false | true> + its half-tile twin ramp::ffx16h_kernel for the last round of the L = 6 level's launches "
                      "(ffx16.hip, v_mfma_f32_16x16x32_f16; ramp_launch_plan.mfma16 = 0: ramp::ffx_kernel, "
                      "ffx.hip, 32x32x16): LN3 -> FF1 -> GEGLU -> FF2 + residual and its input gradient as token-owning waves, all 16 transformer "
                      "blocks, forward and dX; 1.573 MFLOP (algorithmic, fp32) per token and direction",
            "peak_note": "achieved = ALGORITHMIC fp32 FLOPs of the ffx launches (tokens x 1.573 MFLOP) / their summed HIP-event time on the "
                         "launch stream; peak = the pipe the kernel executes on, fp16 dense MFMA 2500 TFLOP/s, divided by the 3 fp16 "
                         "products it spends per fp32 product (833.3); recompute from profiles/r06_kernel_stats.csv: "
                         "sum(tokens) x 1.573e6 / TotalDurationNs of the two ffx16_kernel rows + the two ffx16h_kernel rows",
            "executed_fp16_tflops": FP16_PRODUCTS_PER_FP32 * achieved,
            "frac_vs_fp32_matrix_peak": achieved / PEAK_FP32_MFMA_TFLOPS,
            "launches_per_step": fx_n, "avg_launch_us": avg_us,
            "algorithmic_gflop_per_launch": fx_fl / max(fx_n, 1) / 1e9,
            "share_of_kernel_time": fx_ms / total_ms,
            "by_kernel": {k: {"ms": round(v["ms"], 3), "launches": v["launches"],
                              "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["ms"] > 0 else None} for k, v in kern.items()},
            # the whole split-precision GEMM class (what rounds 1-4 reported as `frac`; its membership moved between rounds)
            "class_frac": class_achieved / peak, "class_achieved": class_achieved, "class_launches_per_step": g["launches"],
            "class_share_of_kernel_time": g["ms"] / total_ms,
            "class_kernels": "ffx + tkl / tklb (token-owning LN1 -> QKV, d(o), d(ln1)) + ato / abl (sample-owning attention blocks) + tkc / tkw "
                             "(k5 convolutions) + gemm_x6p*_kernel<*, NP=2> tile kernels + gemm_kernel<*> (exact fp32, N = 32 layers)",
            # the waste, visible in the line: what the design must move per step (every row's stash written once and read
            # once, 2 x 4.0 MB per network row and evaluation) against what the PMC counters saw it move
            "algorithmic_bytes_per_step": 2 * STASH_BYTES_PER_ROW_EVAL * (2 * B) * WL["T"],
            "traffic_bytes_per_step": (pmc_total() or 0.0) * WL["T"] * (2 * B / 8192.0) or None,
            "traffic_ratio": ((pmc_total() or 0.0) * (2 * B / 8192.0)) / (2 * STASH_BYTES_PER_ROW_EVAL * 2 * B) if pmc_total() else None,
            "sustained_ceiling_tflops": SUSTAINED_FP32EQ_TFLOPS,
            "frac_of_sustained": achieved / SUSTAINED_FP32EQ_TFLOPS,
            "class_note": "the GEMM class mixes fp16x3 launches (833.3 ceiling) with the exact-fp32 N = 32 layers (157.3 ceiling) and, in a "
                          "job that calibrates, bf16x6 launches: class_frac is a lower bound for the fp16x3 kernels; the fused tkw / tkc launches "
                          "carry their GroupNorm + Mish TIME inside the class while only the convolution FLOPs are counted (round 5 on), so the "
                          "class figure is deflated by that much and `norm_rows` shrank partly for accounting reasons",
            "kernel_time_ms_by_class": {k: round(v["ms"], 3) for k, v in prof.items()},
        }
    elif rank == 0:
        result["roofline"] = None
    if args.full and rank == 0 and world == 1 and not args.no_roofline and args.config == 2:
        # the same job with exact fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMMs, one step, for reference
        del dm
        torch.cuda.empty_cache()
        for key, mode in (("bf16x6_mode", "bf16x6"), ("fp32_mfma_mode", "fp32")):
            dm2, _ = build_model(B, device, gemm_mode=mode)
            run_job(dm2, B, cloud, hard_conds, 1)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            run_job(dm2, B, cloud, hard_conds, 1)
            torch.cuda.synchronize(); dt2 = time.perf_counter() - t1
            tf = B * 2 * 25 * FLOP_PER_ROW_EVAL / dt2 / 1e12
            result[key] = {"value": B / dt2, "unit": "trajectories/s", "ms_per_step": dt2 * 1e3,
                           "e2e_frac_of_its_roofline": tf * 6 / PEAK_FP16_MFMA_TFLOPS if mode == "bf16x6" else tf / PEAK_FP32_MFMA_TFLOPS}
            del dm2
            torch.cuda.empty_cache()
    if args.full and rank == 0 and world == 1 and args.config == 2 and not args.no_other_configs:
        # BASELINE configs[2], [3], [4] (one GPU's share) in the driver's own run: 1 warm-up + 2 timed jobs each
        try:
            del dm
        except NameError:
            pass
        torch.cuda.empty_cache()
        result["other_configs"] = {}
        for cfg in (3, 4, 5):
            WL = WORKLOADS[cfg]
            Bc = 4096 if cfg == 3 else 8192
            dmc, _ = build_model(Bc, device)
            cl = torch.from_numpy(synth.make_cloud(WL["cloud"][0], WL["cloud"][1], 3 if WL["o3"] else 2, seed=42)).to(device)
            hcc = {k: torch.from_numpy(v).to(device) for k, v in synth.default_hard_conds(WL["S"], WL["H"]).items()}
            run_job(dmc, Bc, cl, hcc, 1)
            f0 = getattr(dmc, "range_fallbacks", 0)
            torch.cuda.synchronize(); tq = time.perf_counter()
            for _ in range(2):
                oc = run_job(dmc, Bc, cl, hcc, 1)
            torch.cuda.synchronize(); dq = (time.perf_counter() - tq) / 2
            assert bool(torch.isfinite(oc).all())
            flop_c = {3: 1.323e9, 4: 1.324e9, 5: 1.773e9}[cfg]
            tf = Bc * 2 * WL.get("evals", WL["T"]) * flop_c / dq / 1e12
            result["other_configs"][f"config{cfg}"] = {
                "workload": {3: "Maze3D DDPM w=5.75, B=4096 x 2 CFG rows, H=48, S=6, T=25, 4000-pt cloud",
                             4: "Maze2D dynamic replanning, B=8192 candidates x 2 CFG rows, H=48, 10 high-level DDIM + 3 replans x 5 "
                                "score steps, 1024-pt static + 1024-pt moving pursuer cloud, one hipGraph per replan",
                             5: "one GPU's shard of Maze3D B=65536: B=8192 x 2 CFG rows, H=64, S=6, T=50, 8000-pt cloud"}[cfg],
                "value": Bc / dq, "unit": "trajectories/s" if cfg != 4 else "candidate trajectories/s", "ms_per_step": dq * 1e3,
                "steps": 2, "warmup": 1, "workspace_gb": dmc.model.workspace_bytes() / 2 ** 30,
                "range_flag": getattr(dmc, "range_fallbacks", 0) - f0,
                "e2e_algorithmic_tflops": tf, "e2e_frac_of_fp16x3_ceiling": tf * FP16_PRODUCTS_PER_FP32 / PEAK_FP16_MFMA_TFLOPS}
            del dmc, oc
            torch.cuda.empty_cache()
        WL = WORKLOADS[args.config]
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and args.config == 2:
        result["cpu_baseline"] = cpu_baseline(sd, cloud_np, args.cpu_sample)
    elif rank == 0:
        result["cpu_baseline"] = None
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
