"""What scoring a many-scene batch costs after the job: seeded synthetic batches of 64 scenes x 64 samples (the shape of scenes_bench.py)
and 256 scenes x 16 samples, H = 48, S = 4, three boxes per scene.

  (a) the per-scene loop of examples/inference_static.py::run_all_experiments before Metrics.evaluate_scenes existed: per scene a
      boolean-mask gather, compute_collision_intensity (two uploads, one launch) and trajectory_success_and_metrics (torch.where /
      any / mean / std with an .item() each, a second ramp_traj_metrics and the two waypoint-variance launches on the gathered rows);
  (b) Metrics.evaluate_scenes: all uploads, ramp_traj_metrics_scenes + ramp_scene_summary, one copy back.

(a) and (b) alternate in one process after warm-up; each figure is a host clock around work that ends synchronised, median and
min .. max of `reps` repetitions.  Both paths must agree: n_free exactly, intensity percentage 1e-4, path-length mean / std 1e-5,
waypoint variance 4e-6 relative (each path is within 2e-6 of the float64 oracle, tests/test_gpu_scenes_eval.py).  Kernel launches of
one call of each path are counted with torch.profiler where it records device events.
Appends to profiles/multi_scene_eval.txt.  usage: python ramp_amd/tools/scenes_eval_bench.py [reps] [warm] [--out FILE]"""
from __future__ import annotations

import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd.metrics import Metrics  # noqa: E402

H, S = 48, 4
SHAPES = ((64, 64), (256, 16))


def make(n_scenes, per, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    trajs = torch.from_numpy((g.standard_normal((n_scenes * per, H, S)) * 0.4).astype(np.float32)).cuda()
    centers = [torch.from_numpy(g.uniform(-1, 1, (3, 2)).astype(np.float32)) for _ in range(n_scenes)]
    sizes = [torch.from_numpy(g.uniform(0.1, 0.3, (3, 2)).astype(np.float32)) for _ in range(n_scenes)]
    traj_scene = torch.arange(n_scenes, dtype=torch.int32).repeat_interleave(per).cuda()
    return trajs, traj_scene, centers, sizes


def loop_path(M, trajs, traj_scene, centers, sizes):
    out = []
    for i in range(len(centers)):
        mine = trajs[traj_scene == i]
        ci = M.compute_collision_intensity(mine, centers[i], sizes[i])
        out.append(M.trajectory_success_and_metrics(mine, ci))
    return out


def count_kernels(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = sum(1 for n in names if "memcpy" in n.lower() or n.lower().startswith("copy"))
        return (len(names) - copies, copies) if names else None
    except Exception:                                    # the profiler is optional; the timing is not
        return None


def agree(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["n_free_trajectories"] == y["n_free_trajectories"] and x["success"] == y["success"], i
        assert abs(x["collision_intensity"] - y["collision_intensity"]) < 1e-4, i
        for k, tol in (("path_length", 1e-5), ("path_length_std", 1e-5)):
            if x[k] is None or math.isnan(x[k]):
                assert y[k] is None, (i, k)
            else:
                assert abs(x[k] - y[k]) < tol, (i, k, x[k], y[k])
        if x["waypoint_variance"] in (None, 0.0):
            assert y["waypoint_variance"] == x["waypoint_variance"], i
        else:
            assert abs(x["waypoint_variance"] - y["waypoint_variance"]) < 4e-6 * x["waypoint_variance"], i


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 20
    warm = int(args[1]) if len(args) > 1 else 3
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "multi_scene_eval.txt")
    torch.cuda.set_device(0)
    M = Metrics()
    lines = [f"# scenes_eval_bench: per-scene loop (a) vs Metrics.evaluate_scenes (b), H = {H}, S = {S}, 3 boxes per scene; (a) and (b) "
             f"alternate, {reps} timed repetitions after {warm} warm-up; device {torch.cuda.get_device_name(0)}"]
    for n_scenes, per in SHAPES:
        trajs, traj_scene, centers, sizes = make(n_scenes, per, seed=n_scenes)
        counts = [per] * n_scenes
        a = lambda: loop_path(M, trajs, traj_scene, centers, sizes)                     # noqa: E731
        b = lambda: M.evaluate_scenes(trajs, counts, centers, sizes)[0]                 # noqa: E731
        agree(a(), b())
        for _ in range(warm):
            a(); b()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(reps):
            for fn, ts in ((a, ta), (b, tb)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
        lines.append(f"{n_scenes} scenes x {per} samples (B = {n_scenes * per}):")
        for name, ts, fn in (("(a) per-scene loop   ", ta, a), ("(b) evaluate_scenes  ", tb, b)):
            k = count_kernels(fn)
            launches = "launches not counted" if k is None else f"{k[0]} kernel launches, {k[1]} copies"
            lines.append(f"  {name} median {statistics.median(ts) * 1e3:9.3f} ms  min {min(ts) * 1e3:9.3f}  max {max(ts) * 1e3:9.3f}   {launches}")
        ma, mb = statistics.median(ta), statistics.median(tb)
        lines.append(f"  (a) / (b) = {ma / mb:.1f}   (b) slower than (a) beyond the spread: {'YES' if min(tb) > max(ta) else 'no'}")
        assert not min(tb) > max(ta), "the one-pass path is slower than the per-scene loop"
    job = os.path.join(ROOT, "profiles", "multi_scene.txt")
    lines.append("share of a 64 x 64 job's wall time: " + ("see profiles/multi_scene.txt line (b) for the job's time"
                                                           if os.path.exists(job) else "job time not measured"))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
