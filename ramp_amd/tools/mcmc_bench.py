"""What Langevin refinement inside the job costs, and how often MALA accepts (mcmc= of run_inference*): Maze2D, H = 48, T = 25 DDPM,
Philox noise, hipGraph.

  (1) cost of one inner step against one evaluation of the same job: B = 4096 CFG (8192 network rows) and one composed configuration
      (K = 3 obstacle sets, B = 1024, 4096 rows), one inner step on every iteration (sum K = 25), ULA and MALA.  The plain job and the
      job with inner steps run ALTERNATELY, `reps` timed pairs after `warm` untimed ones; per pair
      (job with inner steps - plain job) / sum K is set against plain job / n_steps, and the median ratio is reported.
      An inner step is one evaluation plus the proposal and accept kernels (B H S floats each), the row energies and their combination
      (MALA); the expectation is a ratio within a few percent of 1.  The two kinds of job run on a model of their own each: a context keeps
      the graph of one job shape, so both replay their captured graphs.
  (2) acceptance rate of MALA by timestep for a few step_scale values, B = 512 CFG, one inner step on every iteration.

The networks here carry SYNTHETIC weights: this tool reports cost and acceptance only and makes no claim about plan quality.
Appends to profiles/mcmc_refine.txt.
usage: python ramp_amd/tools/mcmc_bench.py [reps] [warm] [--tag TAG]"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ramp_amd import synth  # noqa: E402
from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

S, H, T = 4, 48, 25


def make(max_rows):
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=max_rows), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True,
                                        noise_source="philox").eval().to("cuda:0")


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--tag", default="run")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=H)

    def cloud(seed):
        return torch.from_numpy(synth.make_cloud(6, 64, 2, seed=seed)).cuda()

    lines = [f"# mcmc_bench {a.tag}: H = {H}, T = {T}, DDPM, Philox noise, hipGraph (each kind of job on its own model: replays); {a.reps} timed alternating pairs after {a.warm} warm-up; "
             f"device {torch.cuda.get_device_name(0)}; synthetic weights: cost and acceptance only, no claim about plan quality"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    # A context keeps the captured graph of ONE job shape, and inner steps are part of the shape: the plain job and the job with inner steps run
    # on a model of their own each, so that every timed job REPLAYS its graph (on one model each would be captured again every time)
    dm_plain = make(8448)
    sets = [cloud(800 + k) for k in range(3)]
    jobs = {
        "CFG, B = 4096 (8192 rows)": lambda dm, mc: dm.run_inference(None, hc, n_samples=4096, obstacle_pts=cloud(1), mcmc=mc, **kw),
        "composed K = 3, B = 1024 (4096 rows)": lambda dm, mc: dm.run_inference_composed([sets], [hc], n_samples=1024, weights=1.0, mcmc=mc, **kw),
    }
    for name, job in jobs.items():
        for kind in ("ula", "mala"):
            mc = dict(kind=kind, steps=1, step_scale=0.05)
            dm_mc = make(8448)
            for _ in range(a.warm):
                job(dm_plain, None); job(dm_mc, mc)
            ratios, plain, refined = [], [], []
            for _ in range(a.reps):      # alternating: both see the same clocks and the same neighbours
                tp = once(lambda: job(dm_plain, None)); tm = once(lambda: job(dm_mc, mc))
                plain.append(tp); refined.append(tm)
                ratios.append(((tm - tp) / T) / (tp / T))
            del dm_mc
            say(f"(1) {name}, {kind.upper()}: plain job median {statistics.median(plain) * 1e3:8.1f} ms ({statistics.median(plain) / T * 1e3:6.2f} ms per "
                f"evaluation), with sum K = {T} inner steps {statistics.median(refined) * 1e3:8.1f} ms; inner step / evaluation: median "
                f"{statistics.median(ratios):.4f}  min {min(ratios):.4f}  max {max(ratios):.4f}")
    # (2) acceptance by timestep
    small = make(1088)
    for scale in (0.05, 0.5, 2.0):
        small.run_inference(None, hc, n_samples=512, obstacle_pts=cloud(1), mcmc=dict(kind="mala", steps=1, step_scale=scale), **kw)
        rate = small.last_mcmc["rate"]
        say(f"(2) MALA, step_scale {scale}: acceptance by timestep t = {T - 1} .. 0: " + " ".join(f"{r:.2f}" for r in rate))
    with open(os.path.join(ROOT, "profiles", "mcmc_refine.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
