"""What composed jobs cost (run_inference_composed): Maze2D, H = 48, T = 25 DDPM, Philox noise, hipGraph.

  (1) N in {1, 8, 64} two-set scenes of 6 x 64 points, 64 trajectories each: ONE run_inference_composed job against the loop of N
      run_inference(compose=True) jobs (one scene per job: every job re-encodes its scene and drops graph and calibration).
      `--part loop` times the loops only, so that a same-box A/B can run them on another build of the library (RAMP_HIP_LIB);
  (2) K = 3 (B = 1024, 4 rows per trajectory) and K = 7 (B = 512, 8 rows) against a CFG job of the same 4096 network rows (B = 2048);
  (3) padding: the ragged job of tests/test_gpu_compose.py -- set counts (2, 3, 1) and sample counts (3, 1, 2), cycled over 64 scenes,
      4 rows per trajectory -- against CFG jobs with its padded and its useful number of network rows; and the same with 16 x the samples.

Each line: median, min and max of `reps` timed repetitions after `warm` untimed ones (wall clock around a synchronised job; the N = 64
loop: one repetition).  Appends to profiles/compose_sets.txt.
usage: python ramp_amd/tools/compose_bench.py [reps] [warm] [--part all|loop] [--tag TAG]"""
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

S, H, T, PER = 4, 48, 25, 64


def make(max_rows, compose=False):
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=max_rows), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", compose=compose,
                                        use_graph=True, noise_source="philox").eval().to("cuda:0")


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--part", choices=["all", "loop"], default="all")
    ap.add_argument("--tag", default="run")
    a = ap.parse_args()
    reps, warm, part, tag = a.reps, a.warm, a.part, a.tag
    torch.cuda.set_device(0)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=H)

    def cloud(seed):
        return torch.from_numpy(synth.make_cloud(6, 64, 2, seed=seed)).cuda()

    lines = [f"# compose_bench {tag} ({part}): H = {H}, T = {T}, DDPM, Philox noise, hipGraph; {reps} timed repetitions after {warm} warm-up; "
             f"library {'alternate (RAMP_HIP_LIB)' if os.environ.get('RAMP_HIP_LIB') else 'in-tree'}; device {torch.cuda.get_device_name(0)}"]
    print(lines[0], flush=True)

    def line(what, ts, n_traj):
        med = statistics.median(ts)
        lines.append(f"{what}: median {med * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f}  max {max(ts) * 1e3:9.1f}  -> {n_traj / med:8.0f} trajectories/s")
        print(lines[-1], flush=True)
        return med

    # (1) many two-set scenes: one composed job against the loop of compose jobs
    pairs = [torch.stack([cloud(700 + 2 * i), cloud(701 + 2 * i)]) for i in range(64)]
    loop_dm = make(3 * PER, compose=True)
    for N in (1, 8, 64):
        def loop():
            for p in pairs[:N]:
                loop_dm.run_inference(None, hc, n_samples=PER, obstacle_pts=p, **kw)

        r, w = (1, 0) if N == 64 else (min(reps, 3), 1)
        once = " (ONE repetition, no warm-up: median = min = max is one sample)" if N == 64 else ""
        m_loop = line(f"(1) N = {N:2d}: loop of {N} run_inference(compose=True) jobs of B = {PER}{once}", timed(loop, r, w), N * PER)
        if part == "loop":
            continue
        dm = make(3 * N * PER)
        m_one = line(f"(1) N = {N:2d}: ONE run_inference_composed job, B = {N * PER}",
                     timed(lambda: dm.run_inference_composed(pairs[:N], [hc] * N, n_samples=PER, **kw), reps, warm), N * PER)
        lines.append(f"(1) N = {N:2d}: loop / one job = {m_loop / m_one:.2f}")
        print(lines[-1], flush=True)
        del dm
    if part != "loop":
        # (2) K = 3 and K = 7 against a CFG job of the same number of network rows
        dm = make(8448)
        m_cfg = line("(2) CFG job, B = 2048 (4096 rows)",
                     timed(lambda: dm.run_inference(None, hc, n_samples=2048, obstacle_pts=cloud(1), **kw), reps, warm), 2048)
        for K, B in ((3, 1024), (7, 512)):
            sets = [cloud(800 + k) for k in range(K)]
            m = line(f"(2) K = {K} composed job, B = {B} (4096 rows)",
                     timed(lambda: dm.run_inference_composed([sets], [hc], n_samples=B, weights=1.0, **kw), reps, warm), B)
            lines.append(f"(2) K = {K}: composed / CFG at equal rows = {m / m_cfg:.3f}")
            print(lines[-1], flush=True)
        # (3) padding cost of the ragged job
        for mult in (1, 16):
            ks = [(2, 3, 1)[i % 3] for i in range(64)]
            ns = [(3, 1, 2)[i % 3] * mult for i in range(64)]
            scenes = [[cloud(900 + 3 * i + k) for k in range(K)] for i, K in enumerate(ks)]
            B, useful = sum(ns), sum(n * (K + 1) for n, K in zip(ns, ks))
            padded = 4 * B
            m_r = line(f"(3) ragged job x{mult}: 64 scenes, B = {B}, {padded} rows of which {useful} useful",
                       timed(lambda: dm.run_inference_composed(scenes, [hc] * 64, n_samples=ns, **kw), reps, warm), B)
            m_p = line(f"(3) CFG job of {padded} rows",
                       timed(lambda: dm.run_inference(None, hc, n_samples=padded // 2, obstacle_pts=cloud(1), **kw), reps, warm), padded // 2)
            m_u = line(f"(3) CFG job of {useful} rows",
                       timed(lambda: dm.run_inference(None, hc, n_samples=useful // 2, obstacle_pts=cloud(1), **kw), reps, warm), useful // 2)
            lines.append(f"(3) x{mult}: ragged / CFG at the padded rows = {m_r / m_p:.3f}; at the useful rows = {m_r / m_u:.3f}; "
                         f"padded / useful rows = {padded / useful:.3f}")
            print(lines[-1], flush=True)
    with open(os.path.join(ROOT, "profiles", "compose_sets.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
