"""What resampling inside the job costs (resample= of run_inference*): T = 25 DDPM, Philox noise, hipGraph, B = 4096, Maze2D H = 48 with a
1024-point 2-D cloud (the headline shape), one group of 4096.

  (1) one event's parts against one score evaluation of the same job (plain job / 25): the cost of the batch (ramp_guide_cost through
      cost_guide_terms) and the resampling (ramp_resample_groups through systematic_resample: scan, search, row gather and copy back).
      Median of `reps` timed calls of the Python wrappers after `warm` untimed ones, synchronised wall time: the wrappers' copies of x and
      their table uploads and scratch allocations are inside, so the figures are upper bounds on the launches.
  (2) the 25-step job with an event every 5 steps (5 events, ESS gate 0.5) against the plain job, alternating, `reps` timed pairs.
      --ab PARENT_TREE: the plain job runs on the PARENT commit instead -- a checkout of it with its library built: every timed job is then
      a fresh child process of this script importing ramp_amd from one of the two trees, alternating on one box, and what is compared is
      the children's own in-process medians.

The network carries SYNTHETIC weights: this tool reports cost only and makes no claim about plan quality.  Appends to profiles/resample.txt.
usage: python ramp_amd/tools/resample_bench.py [reps] [warm] [--tag TAG] [--ab PARENT_TREE]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("RAMP_RESAMPLE_BENCH_TREE") or ROOT)      # (a child of --ab imports the package from the tree it is given)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import synth  # noqa: E402
from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

T, B, H, S, P = 25, 4096, 48, 4, 1024
STEER = dict(every=5, lambda_=2.0, ess_frac=0.5, radius=0.2, w_obs=1.0, w_smooth=0.5, w_acc=0.25)


def make():
    sd = synth.make_unet_state_dict(make_unet_spec(S, H, obstacle_3d=False), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=False, max_rows=2 * B + 256), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True,
                                        noise_source="philox").eval().to("cuda:0")


def inputs():
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    scene = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=1)).cuda()
    cloud = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (P, 2)).astype(np.float32)).cuda()
    return hc, scene, cloud


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def job_times(steered, reps, warm):
    """wall times of the 25-step job on this process's library; a steered job also reports how many (event, group) pairs resampled"""
    hc, scene, cloud = inputs()
    dm = make()
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=H)
    if steered:
        kw["resample"] = dict(STEER, cloud=cloud)
    run = lambda: dm.run_inference(None, hc, n_samples=B, obstacle_pts=scene, **kw)      # noqa: E731
    for _ in range(warm):
        run()
    ts = [once(run) for _ in range(reps)]
    moved = int((dm.last_resample["ancestors"].numpy() != np.arange(B)).any(axis=1).sum()) if steered else 0
    return ts, moved


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--ab", default=None, help="a checkout of the parent commit, library built: the plain job of (2) runs there")
    ap.add_argument("--child", default=None, help="internal: steered|plain, print the job's times as one JSON line")
    a = ap.parse_args()
    ab = None
    if a.ab is not None:      # the children first: this process has not touched the device yet, and holds no memory beside them
        pairs = []
        for _ in range(2):      # alternating child processes, one library each
            res = {}
            for what, tree in (("plain", os.path.abspath(a.ab)), ("steered", ROOT)):
                env = dict(os.environ, RAMP_RESAMPLE_BENCH_TREE=tree)
                env.pop("RAMP_HIP_LIB", None)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.reps), str(a.warm), "--child", what],
                                     env=env, capture_output=True, text=True, timeout=600, check=True).stdout
                res[what] = statistics.median(json.loads(out.strip().splitlines()[-1]))
            pairs.append(res)
        ab = (statistics.median(p["plain"] for p in pairs), statistics.median(p["steered"] for p in pairs))
    torch.cuda.set_device(0)
    if a.child:
        print(json.dumps(job_times(a.child == "steered", a.reps, a.warm)[0]), flush=True)
        return
    lines = [f"# resample_bench {a.tag}: B = {B} in one group, H = {H}, {P}-point cloud, T = {T}, DDPM, Philox noise, hipGraph; {a.reps} timed "
             f"after {a.warm} warm-up; device {torch.cuda.get_device_name(0)}; synthetic weights: cost only, no claim about plan quality"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    from ramp_amd.guide import cost_guide_terms
    from ramp_amd.resample import systematic_resample
    hc, scene, cloud = inputs()
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, H, S)).astype(np.float32)).cuda()
    logw = torch.from_numpy(rng.normal(0, 2, B)).cuda()
    u = torch.tensor([0.37], device="cuda")

    def med(fn):
        ts = [once(fn) for _ in range(a.warm + a.reps)]
        return statistics.median(ts[a.warm:])

    t_cost = med(lambda: cost_guide_terms(x, cloud, STEER["radius"]))
    t_res = med(lambda: systematic_resample(x, logw, [0, B], u, 2.0))
    t_copy = med(lambda: (x.clone(), logw.clone()))      # (what the wrapper of the resampling spends on its working copies)
    plain_ts, _ = job_times(False, a.reps, a.warm)
    plain = statistics.median(plain_ts)
    ev = plain / T
    say(f"(1) one event: cost of the batch {t_cost * 1e3:7.3f} ms, resampling (scan, search, gather, copy back; wrapper copies "
        f"{t_copy * 1e3:6.3f} ms inside) {t_res * 1e3:7.3f} ms; one score evaluation (plain job / {T}) {ev * 1e3:7.3f} ms -> "
        f"{t_cost / ev:.4f} + {t_res / ev:.4f} = {(t_cost + t_res) / ev:.4f} of an evaluation")
    if ab is None:
        st, moved = job_times(True, a.reps, a.warm)
        g = statistics.median(st)
        say(f"(2) plain job {plain * 1e3:8.1f} ms, job with an event every 5 steps ({moved} of 5 resampled) {g * 1e3:8.1f} ms: x {g / plain:.4f}, "
            f"{(g - plain) / 5 * 1e3:6.3f} ms per event (same library, one process)")
    else:
        p0, g = ab
        say(f"(2) plain job of the parent commit {p0 * 1e3:8.1f} ms, job with an event every 5 steps on this build {g * 1e3:8.1f} ms: x {g / p0:.4f}, "
            f"{(g - p0) / 5 * 1e3:6.3f} ms per event (alternating child processes)")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "resample.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
