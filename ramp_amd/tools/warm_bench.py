"""What a warm start saves: the headline job (B = 4096, Maze2D, H = 48, T = 25 DDPM + CFG + APF, Philox noise, hipGraph) from uniform levels
that leave n' = 25, 13 and 6 of the 25 iterations, against the plain job of the same build on the same box (the plain job launches what the
parent commit launches: tests/test_gpu_sample_one_job.py holds it to the parent's bits and launch counts).  The expectation is n' / n.

Each line: median and spread of `reps` timed repetitions after `warm` untimed ones (wall clock around a synchronised job).  Then the cost of
one init and one hold launch, from the sampler category of the per-launch profile (ramp_profile_read, eager jobs): init = (warm job at
level T - 1) - (plain job); hold = ((half the rows at level 12, n_hold = 12) - (all rows at level T - 1)) / 12.
With synthetic weights there is no claim about plan quality.
Appends to profiles/warm_start.txt.  usage: python ramp_amd/tools/warm_bench.py [reps] [warm] [--tag TAG] [--out FILE]"""
from __future__ import annotations

import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import _lib, synth  # noqa: E402
from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.unet import load_numpy_state_dict  # noqa: E402
from ramp_amd.warm import straight_line_prior  # noqa: E402

S, H, T, B = 4, 48, 25, 4096
CAT_SAMPLER = 4


def make():
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=2 * B), sd)
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_apf=True,
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


def sampler_profile(dm, fn, runs=3):
    """(median ms, launches) of the sampler category over `runs` eager jobs (the profiler brackets launches with events; graphs carry none)."""
    lib = _lib.load()
    dm.use_graph = False
    fn(); fn()
    ms_all, cnt = [], 0
    for _ in range(runs):
        _lib.check(lib.ramp_profile(dm.model.ctx(), 1))
        fn()
        torch.cuda.synchronize()
        cms = (C.c_double * 5)(); cfl = (C.c_double * 5)(); ccnt = (C.c_int64 * 5)()
        _lib.check(lib.ramp_profile_read(dm.model.ctx(), cms, cfl, ccnt))
        _lib.check(lib.ramp_profile(dm.model.ctx(), 0))
        ms_all.append(cms[CAT_SAMPLER]); cnt = ccnt[CAT_SAMPLER]
    dm.use_graph = True
    return statistics.median(ms_all), cnt


def main():
    argv, named = sys.argv[1:], {}
    for k in ("--tag", "--out"):
        if k in argv:
            i = argv.index(k)
            named[k] = argv[i + 1]
            del argv[i:i + 2]
    reps = int(argv[0]) if len(argv) > 0 else 5
    warm = int(argv[1]) if len(argv) > 1 else 2
    tag = named.get("--tag", "run")
    torch.cuda.set_device(0)
    hc_np = synth.default_hard_conds(S, H)
    hc = {k: torch.from_numpy(v) for k, v in hc_np.items()}
    cloud = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=42)).cuda()
    line = straight_line_prior(hc_np[0], hc_np[H - 1], H)
    prior = torch.from_numpy((line[None] + 0.05 * np.random.default_rng(0).standard_normal((B, H, S))).astype(np.float32)).cuda()
    dm = make()
    kw = dict(n_samples=B, horizon=H, obstacle_pts=cloud, noise_std_extra_schedule_fn=lambda t: 0.5)

    def job(level=None):
        w = {} if level is None else dict(warm_start=dict(prior=prior, level=level))
        return lambda: dm.run_inference(None, hc, **kw, **w)

    lines = [f"# warm_bench {tag}: B = {B}, H = {H}, T = {T}, DDPM + CFG + APF, Philox noise, hipGraph; {reps} timed repetitions after "
             f"{warm} warm-up; device {torch.cuda.get_device_name(0)}; synthetic weights (no claim about plan quality)"]
    print(lines[0], flush=True)
    plain = timed(job(), reps, warm)
    mp = statistics.median(plain)
    lines.append(f"plain job, n = {T}:            median {mp * 1e3:9.1f} ms  min {min(plain) * 1e3:9.1f}  max {max(plain) * 1e3:9.1f}")
    print(lines[-1], flush=True)
    for level in (24, 12, 5):
        ts = timed(job(level), reps, warm)
        n1 = len(dm.last_warm["steps"])
        med = statistics.median(ts)
        lines.append(f"warm, level {level:2d}, n' = {n1:2d}:      median {med * 1e3:9.1f} ms  min {min(ts) * 1e3:9.1f}  max {max(ts) * 1e3:9.1f}   "
                     f"ratio to plain {med / mp:.3f}  (expected n'/n = {n1 / T:.3f})")
        print(lines[-1], flush=True)
    mixed = [24] * (B // 2) + [12] * (B - B // 2)
    ts = timed(job(mixed), reps, warm)
    med = statistics.median(ts)
    lines.append(f"mixed, half at 24, half at 12 (n_hold = 12, n' = 25): median {med * 1e3:9.1f} ms  ratio to plain {med / mp:.3f}  "
                 "(held rows are still evaluated: expected 1)")
    print(lines[-1], flush=True)
    (p_ms, p_n), (w_ms, w_n), (m_ms, m_n) = sampler_profile(dm, job()), sampler_profile(dm, job(24)), sampler_profile(dm, job(mixed))
    lines.append(f"sampler-category launches of one eager job, ms (launches): plain {p_ms:.3f} ({p_n}) | level 24 {w_ms:.3f} ({w_n}) | mixed {m_ms:.3f} ({m_n})")
    lines.append(f"one init launch: {w_ms - p_ms:+.4f} ms ({w_n - p_n} launch more than plain)   one hold launch: {(m_ms - w_ms) / max(1, m_n - w_n):+.4f} ms "
                 f"({m_n - w_n} launches more than level 24)")
    text = "\n".join(lines) + "\n"
    print("\n".join(lines[-2:]), flush=True)
    out = named.get("--out", os.path.join(ROOT, "profiles", "warm_start.txt"))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
