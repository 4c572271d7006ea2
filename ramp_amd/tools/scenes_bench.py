"""What a job of many scenes costs: 64 scenes x 64 samples (B = 4096), Maze2D, H = 48, T = 25 DDPM + CFG + APF, Philox noise, hipGraph.

  (a) the 64 scenes one after another through run_inference (64 jobs of B = 64: one scene per job, the only way without
      run_inference_scenes) -- every job re-encodes its scene and drops graph and calibration;
  (b) the same work as ONE run_inference_scenes job;
  (c) a single-scene job of the same B = 4096 (the plan DESIGN.md section 4.1 describes).

Each line: median and spread of `reps` timed repetitions after `warm` untimed ones (wall clock around a synchronised job; line (a): at most 2
after 1).  Then the
per-kernel profile (ramp_profile_read_kernels, one eager job each) of (b) and (c), so that a (b) / (c) gap can be named by kernel.
Writes profiles/multi_scene.txt.  usage: python ramp_amd/tools/scenes_bench.py [reps] [warm] [--tag TAG]"""
from __future__ import annotations

import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ramp_amd import _lib, synth  # noqa: E402
from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402

S, H, T, N, PER = 4, 48, 25, 64, 64
KERNELS = ("ffx_fwd", "ffx_bwd", "tkl", "tklb", "ato", "abl", "tkc", "tkw", "other")


def make(max_rows, use_graph=True):
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=max_rows), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_apf=True,
                                        use_graph=use_graph, noise_source="philox").eval().to("cuda:0")


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


def kernel_profile(dm, fn):
    """Per-kernel (ms, launches) of one EAGER job (the profiler brackets launches with events; graphs carry none)."""
    lib = _lib.load()
    dm.use_graph = False
    fn(); fn()
    _lib.check(lib.ramp_profile(dm.model.ctx(), 1))
    fn()
    torch.cuda.synchronize()
    ms = (C.c_double * 9)(); fl = (C.c_double * 9)(); cnt = (C.c_int64 * 9)()
    _lib.check(lib.ramp_profile_read_kernels(dm.model.ctx(), 9, ms, fl, cnt))
    cms = (C.c_double * 5)(); cfl = (C.c_double * 5)(); ccnt = (C.c_int64 * 5)()
    _lib.check(lib.ramp_profile_read(dm.model.ctx(), cms, cfl, ccnt))
    _lib.check(lib.ramp_profile(dm.model.ctx(), 0))
    dm.use_graph = True
    return list(ms), list(cnt), list(cms), list(ccnt)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 5
    warm = int(args[1]) if len(args) > 1 else 2
    tag = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else "run"
    torch.cuda.set_device(0)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    clouds = [torch.from_numpy(synth.make_cloud(6 + (i % 11), 64, 2, seed=300 + i)).cuda() for i in range(N)]
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5)
    small, big = make(2 * PER), make(2 * N * PER)

    def a():
        for c in clouds:
            small.run_inference(None, hc, n_samples=PER, horizon=H, obstacle_pts=c, **kw)

    def b():
        big.run_inference_scenes(clouds, [hc] * N, n_samples=PER, horizon=H, **kw)

    def c():
        big.run_inference(None, hc, n_samples=N * PER, horizon=H, obstacle_pts=clouds[0], **kw)

    lines = [f"# scenes_bench {tag}: {N} scenes x {PER} samples, H = {H}, T = {T}, DDPM + CFG + APF, Philox noise, hipGraph; "
             f"{reps} timed repetitions after {warm} warm-up; device {torch.cuda.get_device_name(0)}"]
    res = {}
    for name, fn, what in (("a", a, f"{N} single-scene jobs of B = {PER}, one after another"), ("b", b, "ONE run_inference_scenes job"),
                           ("c", c, f"a single-scene job of B = {N * PER}")):
        if name == "a":
            print(lines[0], flush=True)
        ts = timed(fn, min(reps, 2), 1) if name == "a" else timed(fn, reps, warm)      # (a) is 64 jobs, each capturing its own graph: minutes per repetition
        res[name] = ts
        med = statistics.median(ts)
        lines.append(f"({name}) {what}: median {med * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f}  max {max(ts) * 1e3:9.1f}  "
                     f"-> {N * PER / med:8.0f} trajectories/s")
        print(lines[-1], flush=True)
    ma, mb, mc = (statistics.median(res[k]) for k in "abc")
    ratios = sorted(x / y for x in res["b"] for y in res["c"])
    lines.append(f"(a) / (b) = {ma / mb:.2f}    (b) / (c) = {mb / mc:.3f}  (all pairs of repetitions: {ratios[0]:.3f} .. {ratios[-1]:.3f})")
    pb, pc = kernel_profile(big, b), kernel_profile(big, c)
    lines.append("per-kernel profile of one eager job, ms (launches):   (b) many scenes | (c) one scene | (b) - (c)")
    for i, k in enumerate(KERNELS):
        lines.append(f"  {k:8s} {pb[0][i]:9.2f} ({pb[1][i]:5d}) | {pc[0][i]:9.2f} ({pc[1][i]:5d}) | {pb[0][i] - pc[0][i]:+8.2f}")
    for i, k in enumerate(("gemm", "attention", "rows", "small conv", "sampler")):
        lines.append(f"  cat {k:10s} {pb[2][i]:9.2f} ({pb[3][i]:5d}) | {pc[2][i]:9.2f} ({pc[3][i]:5d}) | {pb[2][i] - pc[2][i]:+8.2f}")
    text = "\n".join(lines) + "\n"
    print(text[text.index("(a) / (b)"):], flush=True)
    out = os.path.join(ROOT, "profiles", "multi_scene.txt")
    with open(out, "a", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
