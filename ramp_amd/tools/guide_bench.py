"""What cost-gradient guidance inside the job costs (cost_guide= of run_inference*): T = 25 DDPM, Philox noise, hipGraph, B = 4096.

  (1) one guide launch (ramp_guide_step) with 1 and with 4 iterations against one score evaluation of the same job (unguided job / 25):
      Maze2D H = 48 with a 1024-point 2-D cloud (the headline shape), and the 3-D sampler at H = 64 with a 4096-point 3-D cloud.
      Median of `reps` timed calls of the Python wrapper after `warm` untimed ones, synchronised wall time: the wrapper's copy of x and its
      table upload are inside, so the figure is an upper bound on the launch; (4 iterations - 1 iteration) / 3 is the cost of an iteration.
  (2) the guided 25-step job (2 guide iterations on every reverse step) against the unguided job, alternating, `reps` timed pairs.
      --ab PARENT_TREE: the unguided job runs on the PARENT commit instead -- a checkout of it with its library built (its Python binding
      too, not only RAMP_HIP_LIB as ramp_amd/tools/ab_libs.sh switches builds: this commit's binding refuses a library that lacks the new
      symbols): every timed job is then a fresh child process of this script importing ramp_amd from one of the two trees, alternating on
      one box, and what is compared is the children's own in-process medians.

The networks carry SYNTHETIC weights: this tool reports cost only and makes no claim about plan quality.  Appends to profiles/cost_guide.txt.
usage: python ramp_amd/tools/guide_bench.py [reps] [warm] [--tag TAG] [--ab PARENT_TREE]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("RAMP_GUIDE_BENCH_TREE") or ROOT)      # (a child of --ab imports the package from the tree it is given)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import synth  # noqa: E402
from ramp_amd.models import GaussianDiffusionModel3d, StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

T, B = 25, 4096
SHAPES = {"2d": dict(S=4, H=48, o3=False, P=1024, d=2), "3d": dict(S=6, H=64, o3=True, P=4096, d=3)}
GUIDE = dict(radius=0.2, step=2e-3, w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=4.0)


def make(shape):
    sh = SHAPES[shape]
    sd = synth.make_unet_state_dict(make_unet_spec(sh["S"], sh["H"], obstacle_3d=sh["o3"]), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=sh["H"], state_dim=sh["S"], obstacle_3d=sh["o3"], max_rows=2 * B + 256), sd)
    cls = GaussianDiffusionModel3d if sh["o3"] else StaticGaussianDiffusionModel
    return cls(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True, noise_source="philox").eval().to("cuda:0")


def inputs(shape):
    sh = SHAPES[shape]
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(sh["S"], sh["H"]).items()}
    scene = torch.from_numpy(synth.make_cloud(4, 30, 3, seed=41) if sh["o3"] else synth.make_cloud(6, 64, 2, seed=1)).cuda()
    gcloud = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (sh["P"], sh["d"])).astype(np.float32)).cuda()
    return hc, scene, gcloud


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def job_times(shape, guided, reps, warm):
    """wall times of the 25-step job on this process's library"""
    sh = SHAPES[shape]
    hc, scene, gcloud = inputs(shape)
    dm = make(shape)
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=sh["H"])
    if guided:
        kw["cost_guide"] = dict(GUIDE, cloud=gcloud)
    run = lambda: dm.run_inference(None, hc, n_samples=B, obstacle_pts=scene, **kw)      # noqa: E731
    for _ in range(warm):
        run()
    return [once(run) for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--ab", default=None, help="a checkout of the parent commit, library built: the unguided job of (2) runs there")
    ap.add_argument("--child", default=None, help="internal: SHAPE:guided|unguided, print the job's times as one JSON line")
    a = ap.parse_args()
    ab = {}
    if a.ab is not None:      # the children first: this process has not touched the device yet, and holds no memory beside them
        for shape in SHAPES:
            pairs = []
            for _ in range(2):      # alternating child processes, one library each
                res = {}
                for what, tree in (("unguided", os.path.abspath(a.ab)), ("guided", ROOT)):
                    env = dict(os.environ, RAMP_GUIDE_BENCH_TREE=tree)
                    env.pop("RAMP_HIP_LIB", None)
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.reps), str(a.warm), "--child", f"{shape}:{what}"],
                                         env=env, capture_output=True, text=True, timeout=600, check=True).stdout
                    res[what] = statistics.median(json.loads(out.strip().splitlines()[-1]))
                pairs.append(res)
            ab[shape] = (statistics.median(p["unguided"] for p in pairs), statistics.median(p["guided"] for p in pairs))
    torch.cuda.set_device(0)
    if a.child:
        shape, what = a.child.split(":")
        print(json.dumps(job_times(shape, what == "guided", a.reps, a.warm)), flush=True)
        return
    lines = [f"# guide_bench {a.tag}: B = {B}, T = {T}, DDPM, Philox noise, hipGraph; {a.reps} timed after {a.warm} warm-up; device "
             f"{torch.cuda.get_device_name(0)}; synthetic weights: cost only, no claim about plan quality"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    from ramp_amd.guide import cost_guide_step
    for shape, sh in SHAPES.items():
        hc, scene, gcloud = inputs(shape)
        x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (B, sh["H"], sh["S"])).astype(np.float32)).cuda()
        per = {}
        for n_iter in (1, 4):
            ts = []
            for k in range(a.warm + a.reps):
                t = once(lambda: cost_guide_step(x, gcloud, GUIDE["radius"], GUIDE["step"], w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=n_iter,
                                                 max_norm=4.0, hard_conds=hc))
                if k >= a.warm:
                    ts.append(t)
            per[n_iter] = statistics.median(ts)      # (the wrapper's copy of x and table upload included: an upper bound on the launch)
        plain = statistics.median(job_times(shape, False, a.reps, a.warm))
        say(f"(1) {shape}: H = {sh['H']}, {sh['P']}-point {sh['d']}-D cloud: guide launch 1 iteration {per[1] * 1e3:7.3f} ms, 4 iterations "
            f"{per[4] * 1e3:7.3f} ms ({(per[4] - per[1]) / 3 * 1e3:7.3f} ms per added iteration); one score evaluation (unguided job / {T}) {plain / T * 1e3:7.3f} ms -> {per[1] / (plain / T):.4f} / "
            f"{per[4] / (plain / T):.4f} of an evaluation")
        if a.ab is None:
            g = statistics.median(job_times(shape, True, a.reps, a.warm))
            say(f"(2) {shape}: unguided job {plain * 1e3:8.1f} ms, guided job (2 iterations on each of {T} steps) {g * 1e3:8.1f} ms: x {g / plain:.4f} "
                "(same library, one process)")
        else:
            u, g = ab[shape]
            say(f"(2) {shape}: unguided job of the parent commit {u * 1e3:8.1f} ms, guided job on this build {g * 1e3:8.1f} ms: x {g / u:.4f} "
                "(alternating child processes)")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cost_guide.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
