"""What replanning many pursuit-evasion episodes in one job buys: E in {1, 8, 64} episodes of 35 candidates (the reference's n_samples,
scripts/inference/inference_dynamic.py), Maze2D, H = 48, high-level DDIM-10 plan + R replans of DDIM-5 each, synthetic weights and scenes,
torch noise, hipGraph.

  (a) the E episodes one after another through run_inference on one model (E planners of B = 35: the only way without
      run_inference_episodes) -- every episode re-encodes its scene and captures its graphs again;
  (b) the same E episodes as ONE run_inference_episodes job (B = 35 E).

Start and goal lie 2.26 apart and an episode executes one waypoint per replan, so no episode reaches its goal within R replans: both
sides run the high-level plan and R replans per episode (the count is printed).  The scenes are sparse, so that no episode should need
the eager from-scratch fallback of a replan without a collision-free candidate, which would show as a longer time.  Each line: median, min and max of `reps` timed
repetitions after `warm` untimed ones (wall clock around a synchronised run; side (a) at E = 64: at most 2 after 1), then the ratio of
the medians and its range over all pairs of repetitions.
Appends to profiles/multi_episode.txt (--out PATH: another file).
usage: python ramp_amd/tools/episodes_bench.py [reps] [warm] [--replans R] [--episodes 1,8,64] [--tag TAG] [--out PATH]"""
from __future__ import annotations

import os
import statistics
import sys
import time
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import synth  # noqa: E402
from ramp_amd.apf_dynamic import generate_box_points  # noqa: E402
from ramp_amd.models import DynamicGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

S, H, T, PER = 4, 48, 100, 35
# boxes away from the start -> goal diagonal, so that candidates stay collision-free
BOXES = np.array([[-0.3, 0.5], [0.4, -0.5], [-0.7, 0.7], [0.7, -0.7], [0.1, 0.8], [-0.8, 0.1]])
START, GOAL = [-0.8, -0.8, 0.0, 0.0], [0.8, 0.8, 0.0, 0.0]


class Sphere:
    """A one-sphere pursuer stepping 0.05 towards the mean evader position (the stand-in the parity tests drive the planner with)."""

    def __init__(self):
        self.centers = torch.tensor([[0.6, 0.55]], dtype=torch.float32)
        self.radii = torch.tensor([0.1], dtype=torch.float32)

    def update_centers(self, t, current_state):
        d = current_state.detach().cpu().float().mean(dim=0)[:2] - self.centers[0]
        n = float(torch.linalg.norm(d))
        self.centers = (self.centers[0] + (d * (0.05 / n) if n > 0.05 else d)).unsqueeze(0)


def make_episode(i):
    """(context, cloud) of synthetic episode i: six boxes, jittered per episode, and a pursuer of its own."""
    rng = np.random.RandomState(1000 + i)
    centres = BOXES + rng.uniform(-0.05, 0.05, BOXES.shape)
    boxes = NS(centers=torch.tensor(centres, dtype=torch.float32), sizes=torch.full((6, 2), 0.16))
    env = NS(obj_fixed_list=[NS(fields=[boxes])], obj_extra_list=[NS(fields=[Sphere()])])
    cloud = np.stack([generate_box_points(c, (0.16, 0.16), 64, rng=rng) for c in centres]).astype(np.float32)
    return {'dataset': NS(env=env)}, torch.from_numpy(cloud).cuda()


def make(max_rows):
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=max_rows), sd)
    return DynamicGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, use_graph=True).eval().to("cuda:0")


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    named = ("--replans", "--episodes", "--tag", "--out")
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in named]
    reps = int(args[0]) if len(args) > 0 else 5
    warm = int(args[1]) if len(args) > 1 else 2
    R = int(opt("--replans", "6"))
    sizes = [int(v) for v in opt("--episodes", "1,8,64").split(",")]
    tag = opt("--tag", "run")
    out = opt("--out", os.path.join(ROOT, "profiles", "multi_episode.txt"))
    torch.cuda.set_device(0)
    hard = {0: torch.tensor(START), H - 1: torch.tensor(GOAL)}
    small = make(2 * PER)
    lines = [f"# episodes_bench {tag}: episodes of {PER} candidates, H = {H}, DDIM-10 plan + {R} replans of DDIM-5, CFG, torch noise, hipGraph; "
             f"{reps} timed repetitions after {warm} warm-up; device {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    for E in sizes:
        big = make(2 * E * PER)
        replans = {"a": [], "b": []}

        def a():
            torch.manual_seed(1); np.random.seed(1)
            n = 0
            for i in range(E):
                ctx, cloud = make_episode(i)
                _chain, obs, _start = small.run_inference(context=ctx, hard_conds=hard, n_samples=PER, return_chain=True, obstacle_pts=cloud,
                                                          max_iteration=R)
                n += len(obs)
            replans["a"].append(n)

        def b():
            torch.manual_seed(1)
            made = [make_episode(i) for i in range(E)]
            res = big.run_inference_episodes([m[0] for m in made], [hard] * E, [m[1] for m in made], n_samples=PER,
                                             rngs=[np.random.RandomState(i) for i in range(E)], return_chain=True, max_iteration=R)
            replans["b"].append(sum(len(r[1]) for r in res))

        res = {}
        for name, fn, what in (("a", a, f"{E} run_inference planners of B = {PER}, one after another"),
                               ("b", b, f"ONE run_inference_episodes job of B = {E * PER}")):
            ts = timed(fn, min(reps, 2), 1) if (name == "a" and E >= 64) else timed(fn, reps, warm)
            res[name] = ts
            med = statistics.median(ts)
            lines.append(f"E = {E:3d} ({name}) {what}: median {med * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f}  max {max(ts) * 1e3:9.1f}  "
                         f"-> {replans[name][-1] / med:7.1f} episode-replans/s ({replans[name][-1]} replans of {E * R}, "
                         f"range fallbacks {small.range_fallbacks if name == 'a' else big.range_fallbacks})")
            print(lines[-1], flush=True)
        ratios = sorted(x / y for x in res["a"] for y in res["b"])
        lines.append(f"E = {E:3d} (a) / (b) = {statistics.median(res['a']) / statistics.median(res['b']):.2f}  "
                     f"(all pairs of repetitions: {ratios[0]:.2f} .. {ratios[-1]:.2f})")
        print(lines[-1], flush=True)
        del big
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
