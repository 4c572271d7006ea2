"""What encoding the scenes of a many-scene job costs: ONE ramp_encode_scenes call over N scenes against the loop of N
ramp_encode_scene calls (the per-scene path, untouched: the baseline), N in {1, 16, 64, 256}, for the reference's 6 x 64 2-D clouds
and 20 x 200 3-D clouds.

Both sides run in one process, alternating (loop, batched, loop, batched, ...) after `warm` untimed rounds; a timed window is a host
clock around `inner` repetitions that end in a device synchronise, `inner` chosen so that a window holds at least 64 scenes.  Per N:
median, min and max of the `reps` windows per side, the ratio of the medians and of all pairs of windows, and the run-to-run spread
((max - min) / median, the larger of the two sides).  The latents of both sides are compared bit for bit at every timed size.
Then the wall time of one run_inference_scenes job of 256 scenes x 16 samples (T = 25 DDPM + CFG + APF, Philox noise, hipGraph)
with its encoding share: the job's encode_scenes call timed alone, and what the per-scene loop took for the same scenes.
Appends to profiles/multi_scene_encode.txt.  usage: python ramp_amd/tools/encode_bench.py [reps] [warm] [--tag TAG] [--no-job]"""
from __future__ import annotations

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

COUNTS = (1, 16, 64, 256)
H, T = 48, 25


def make_unet(S, o3, max_rows):
    sd = synth.make_unet_state_dict(make_unet_spec(S, H, obstacle_3d=o3), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=o3, max_rows=max_rows), sd)
    return u.eval().to("cuda:0")


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def compare(u, clouds, reps, warm):
    """Alternating windows of the per-scene loop and the one batched call over `clouds`: (loop times, batched times)."""
    out = {}

    def loop():
        out["loop"] = torch.cat([u.encode_scene(c) for c in clouds])

    def batched():
        out["batched"] = u.encode_scenes(clouds)

    inner = max(1, 64 // len(clouds))
    for _ in range(warm):
        window(loop, inner); window(batched, inner)
    assert torch.equal(out["loop"], out["batched"]), "the batched latents differ from the per-scene loop's"
    tl, tb = [], []
    for _ in range(reps):
        tl.append(window(loop, inner)); tb.append(window(batched, inner))
    return tl, tb, u.last_encode_passes


def report(name, n, tl, tb, passes):
    ml, mb = statistics.median(tl), statistics.median(tb)
    spread = max((max(t) - min(t)) / statistics.median(t) for t in (tl, tb))
    pairs = sorted(b / l for b in tb for l in tl)
    verdict = "batched faster" if mb < ml else ("within the spread" if mb <= ml * (1 + spread) else "BATCHED SLOWER beyond the spread")
    return (f"{name} N = {n:3d}: loop median {ml * 1e3:9.3f} ms (min {min(tl) * 1e3:9.3f} max {max(tl) * 1e3:9.3f}) | batched median "
            f"{mb * 1e3:9.3f} ms (min {min(tb) * 1e3:9.3f} max {max(tb) * 1e3:9.3f}, {passes} pass{'es' if passes != 1 else ''}) | "
            f"batched / loop = {mb / ml:.3f} (all pairs {pairs[0]:.3f} .. {pairs[-1]:.3f}), loop / batched = {ml / mb:.2f}x, "
            f"spread {spread * 100:.1f} % -> {verdict}")


def job_share(reps, warm):
    """One run_inference_scenes job of 256 scenes x 16 samples: wall time, and the share of its encode_scenes call."""
    n, per, S = 256, 16, 4
    u = make_unet(S, False, 2 * n * per)
    dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_apf=True, use_graph=True,
                                      noise_source="philox").eval().to("cuda:0")
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    clouds = [torch.from_numpy(synth.make_cloud(6, 64, 2, seed=300 + i)).cuda() for i in range(n)]

    def job():
        dm.run_inference_scenes(clouds, [hc] * n, n_samples=per, horizon=H, noise_std_extra_schedule_fn=lambda t: 0.5)

    for _ in range(warm):
        job()
    torch.cuda.synchronize()
    tj = [window(job, 1) for _ in range(reps)]
    tl, tb, _ = compare(u, clouds, reps, 1)
    mj, ml, mb = statistics.median(tj), statistics.median(tl), statistics.median(tb)
    return [f"run_inference_scenes, {n} scenes (6 x 64) x {per} samples, B = {n * per}, T = {T} DDPM + CFG + APF, Philox, hipGraph: wall median "
            f"{mj * 1e3:9.1f} ms (min {min(tj) * 1e3:9.1f} max {max(tj) * 1e3:9.1f})",
            f"  its encode_scenes call alone: median {mb * 1e3:8.2f} ms = {mb / mj * 100:5.2f} % of the job; the per-scene loop over the same scenes: "
            f"median {ml * 1e3:8.2f} ms = {ml / (mj - mb + ml) * 100:5.2f} % of the job as it was (job - batched + loop = {(mj - mb + ml) * 1e3:9.1f} ms)"]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 7
    warm = int(args[1]) if len(args) > 1 else 2
    tag = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else "run"
    if not torch.cuda.is_available():
        raise SystemExit("encode_bench needs a HIP device: nothing is measured without one")
    torch.cuda.set_device(0)
    lines = [f"# encode_bench {tag}: ramp_encode_scenes (one call) vs the loop of ramp_encode_scene calls, alternating windows in one process; "
             f"{reps} timed windows per side after {warm} warm-up rounds; device {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)
    for name, S, o3, shape in (("2-D  6 x  64", 4, False, (6, 64, 2)), ("3-D 20 x 200", 6, True, (20, 200, 3))):
        u = make_unet(S, o3, 4)
        for n in COUNTS:
            clouds = [torch.from_numpy(synth.make_cloud(*shape, seed=500 + i)).cuda() for i in range(n)]
            lines.append(report(name, n, *compare(u, clouds, reps, warm)))
            print(lines[-1], flush=True)
        del u
    if "--no-job" not in sys.argv:
        lines += job_share(min(reps, 5), 2)
        print("\n".join(lines[-2:]), flush=True)
    with open(os.path.join(ROOT, "profiles", "multi_scene_encode.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
