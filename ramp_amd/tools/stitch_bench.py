"""What stitched windows cost (run_inference_stitched): T = 25 DDPM, Philox noise, hipGraph, Maze2D H = 48, S = 4, C = 1024 chains of W = 4
windows with overlap O = 8 (L = 168 waypoints), B = C W = 4096 rows.

  (1) one stitch launch (ramp_stitch_windows: blend of C (W - 1) O S elements, two pins) against one score evaluation of the plain job of the
      same 4096 rows (plain job / 25).  Median of `reps` timed calls of the Python wrapper after `warm` untimed ones, synchronised wall time:
      the wrapper's copy of x and its table upload are inside, so the figure is an upper bound on the launch.
  (2) the stitched 25-step job against the plain job of the same 4096 rows, `reps` timed jobs each, and against run_inference_scenes with the
      one scene and the same rows: the stitched entry shares that entry's host path (scenes encoded and the row -> latent table set on
      every call, after which the context computes its canonical calibration anew: one bf16x6 evaluation), so the second ratio is what
      the stitch launches themselves add.
      --ab PARENT_TREE: the plain job runs on the PARENT commit instead -- a checkout of it with its library built (its Python binding too:
      this commit's binding refuses a library that lacks the new symbols): every timed job is then a fresh child process of this script
      importing ramp_amd from one of the two trees, alternating on one box, and what is compared is the children's own in-process medians.

The network carries SYNTHETIC weights: this tool reports cost only and makes no claim about plan quality.  Appends to profiles/stitch.txt.
usage: python ramp_amd/tools/stitch_bench.py [reps] [warm] [--tag TAG] [--ab PARENT_TREE]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("RAMP_STITCH_BENCH_TREE") or ROOT)      # (a child of --ab imports the package from the tree it is given)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import synth  # noqa: E402
from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

T, C_, W, H, O, S = 25, 1024, 4, 48, 8, 4
B = C_ * W


def make():
    sd = synth.make_unet_state_dict(make_unet_spec(S, H, obstacle_3d=False), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=False, max_rows=2 * B + 256), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True,
                                        noise_source="philox").eval().to("cuda:0")


def inputs():
    hc = synth.default_hard_conds(S, H)
    scene = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=1)).cuda()
    return {0: torch.from_numpy(hc[0]), H - 1: torch.from_numpy(hc[H - 1])}, {0: torch.from_numpy(hc[0]), -1: torch.from_numpy(hc[H - 1])}, scene


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def job_times(kind, reps, warm):
    """wall times of the 25-step job of 4096 rows on this process's library: 'plain' run_inference, 'scenes' run_inference_scenes with the one
    scene (the host path of the stitched entry: scenes encoded and the row -> latent table set on every call, which costs the context its
    kept canonical calibration), 'stitched' run_inference_stitched"""
    hc, pins, scene = inputs()
    dm = make()
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5)
    if kind == "stitched":
        run = lambda: dm.run_inference_stitched(scene, pins, W, O, n_samples=C_, blend='ramp', **kw)      # noqa: E731
    elif kind == "scenes":
        run = lambda: dm.run_inference_scenes([scene], [hc], n_samples=B, **kw)      # noqa: E731
    else:
        run = lambda: dm.run_inference(None, hc, n_samples=B, obstacle_pts=scene, horizon=H, **kw)      # noqa: E731
    for _ in range(warm):
        run()
    return [once(run) for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--ab", default=None, help="a checkout of the parent commit, library built: the plain job of (2) runs there")
    ap.add_argument("--child", default=None, help="internal: plain|stitched, print the job's times as one JSON line")
    a = ap.parse_args()
    ab = None
    if a.ab is not None:      # the children first: this process has not touched the device yet, and holds no memory beside them
        pairs = []
        for _ in range(2):      # alternating child processes, one library each
            res = {}
            for what, tree in (("plain", os.path.abspath(a.ab)), ("scenes", ROOT), ("stitched", ROOT)):
                env = dict(os.environ, RAMP_STITCH_BENCH_TREE=tree)
                env.pop("RAMP_HIP_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.reps), str(a.warm), "--child", what],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"the {what} child failed ({r.returncode}):\n{r.stderr[-3000:]}")
                res[what] = statistics.median(json.loads(r.stdout.strip().splitlines()[-1]))
            pairs.append(res)
        ab = tuple(statistics.median(p[k] for p in pairs) for k in ("plain", "scenes", "stitched"))
    torch.cuda.set_device(0)
    if a.child:
        print(json.dumps(job_times(a.child, a.reps, a.warm)), flush=True)
        return
    lines = [f"# stitch_bench {a.tag}: C = {C_}, W = {W}, H = {H}, O = {O}, S = {S} (L = {H + (W - 1) * (H - O)}, B = {B} rows), T = {T}, DDPM, Philox noise, "
             f"hipGraph; {a.reps} timed after {a.warm} warm-up; device {torch.cuda.get_device_name(0)}; synthetic weights: cost only, no claim about plan quality"]
    print(lines[0], flush=True)

    def say(text):
        lines.append(text)
        print(text, flush=True)

    from ramp_amd.stitch import stitch_windows
    _hc, pins, _scene = inputs()
    x = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (B, H, S)).astype(np.float32)).cuda()
    ts = []
    for k in range(a.warm + a.reps):
        t = once(lambda: stitch_windows(x, W, O, 'ramp', pins))
        if k >= a.warm:
            ts.append(t)
    one = statistics.median(ts)      # (the wrapper's copy of x and table upload included: an upper bound on the launch)
    plain = statistics.median(job_times("plain", a.reps, a.warm))
    say(f"(1) stitch launch ({C_ * (W - 1) * O * S} blended elements, 2 pins) {one * 1e3:7.3f} ms; one score evaluation (plain job of {B} rows / {T}) "
        f"{plain / T * 1e3:7.3f} ms -> {one / (plain / T):.4f} of an evaluation")
    if ab is None:
        sc = statistics.median(job_times("scenes", a.reps, a.warm))
        g = statistics.median(job_times("stitched", a.reps, a.warm))
        say(f"(2) plain job of {B} rows {plain * 1e3:8.1f} ms, stitched job {g * 1e3:8.1f} ms: x {g / plain:.4f}; many-scene entry with the one scene "
            f"{sc * 1e3:8.1f} ms: stitched x {g / sc:.4f} of it (same library, one process)")
    else:
        u, sc, g = ab
        say(f"(2) plain job of {B} rows on the parent commit {u * 1e3:8.1f} ms, stitched job on this build {g * 1e3:8.1f} ms: x {g / u:.4f}; "
            f"many-scene entry with the one scene on this build {sc * 1e3:8.1f} ms: stitched x {g / sc:.4f} of it (alternating child processes)")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "stitch.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
