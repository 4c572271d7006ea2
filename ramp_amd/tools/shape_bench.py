#!/usr/bin/env python3
"""Headline workload at each network shape the engine serves: B = 4096 trajectories, H = 48, T = 25 DDPM, CFG, APF, Philox noise,
graph replay (bench.py's configs[1] job) with the U-Net built at (1,2,4) / (1,2,4,8) x unet_input_dim 16 / 32 / 64.  For C0 = 64 the
same job also runs with the wide fused convolutions off (tkw_rows = 0).  One line per shape; output of record: profiles/network_shapes.txt.

    python ramp_amd/tools/shape_bench.py [--steps 3] [--warmup 1] [--batch 4096]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run(opt, c0, B, steps, warmup, plan):
    import torch
    from ramp_amd import synth
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.spec import UNET_DIM_MULTS, make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    S, H, T = 4, 48, 25
    dm_ = UNET_DIM_MULTS[opt]
    sd = synth.make_unet_state_dict(make_unet_spec(S, H, c0, dm_), seed=0)
    unet = TemporalUnetInference(n_support_points=H, state_dim=S, unet_input_dim=c0, dim_mults=dm_, max_rows=2 * B)
    load_numpy_state_dict(unet, sd)
    if plan:
        unet.set_launch_plan(**plan)
    dm = StaticGaussianDiffusionModel(model=unet, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True,
                                      compose=False, use_apf=True, sampler="ddpm", use_graph=True, noise_source="philox",
                                      noise_seed=1234).eval().to("cuda")
    cloud = torch.from_numpy(synth.make_cloud(16, 64, 2, seed=42)).cuda()
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}

    def job():
        return dm.run_inference(None, hc, n_samples=B, horizon=H, return_chain=False, traj_normalized=None, obstacle_pts=cloud,
                                sample_fn=None, noise_std_extra_schedule_fn=lambda t: 0.5, n_diffusion_steps_without_noise=0)
    for _ in range(1 + warmup):
        x = job()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        x = job()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    assert torch.isfinite(x).all()
    return dict(dim_mults=list(dm_), unet_input_dim=c0, plan=plan or "default", ms_per_job=round(dt * 1e3, 2),
                traj_per_s=round(B / dt, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--one", help=argparse.SUPPRESS)          # "opt,c0,tkw_off": one shape in this process
    a = ap.parse_args()
    if a.one:
        opt, c0, off = (int(v) for v in a.one.split(","))
        print(json.dumps(run(opt, c0, a.batch, a.steps, a.warmup, dict(tkw_rows=0) if off else None)), flush=True)
        return
    import torch
    print(f"# shape_bench: B={a.batch} H=48 T=25 DDPM CFG APF philox graph; steps={a.steps} warmup={a.warmup}; "
          f"{torch.cuda.get_device_name(0)}", flush=True)
    cases = [(opt, c0, 0) for opt in (0, 1) for c0 in (16, 32, 64)] + [(0, 64, 1), (1, 64, 1)]
    for opt, c0, off in cases:      # a fresh process per shape: one context's workspace at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{opt},{c0},{off}", "--steps", str(a.steps),
                            "--warmup", str(a.warmup), "--batch", str(a.batch)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(f"# dm{opt} c{c0} tkw_off={off}: exit {r.returncode}: {r.stderr.strip().splitlines()[-1:]}", flush=True)
            sys.exit(r.returncode)
        print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
