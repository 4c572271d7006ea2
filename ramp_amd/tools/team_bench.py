"""What teams of robots in one job cost (cost_guide=dict(..., team=dict(size=A, ...))): T = 25 DDPM, Philox noise, hipGraph, B = 4096 rows,
H = 48, a 1024-point 2-D cloud.

  (1) one launch of ramp_guide_step_team with 1 and with 2 iterations at team sizes A = 1, 2, 4, 8 (A = 1 launches the cloud guide's own
      kernel) against one launch of ramp_guide_step at equal rows and iteration count, and against one score evaluation (unguided job / 25).
      The C entries are timed directly on prepared tables (their own table upload and synchronisation are inside, for both); the rows are
      reset before every timed call.  The rows of a team lie on a ring inside radius_team, so that every pair is active.
  (2) one launch of ramp_team_clearance at the same shapes (swept, with the per-row arrays of the selection).
  (3) the 25-step job with two team iterations on every reverse step (A = 2, 4, 8) against the cloud-guided job of the same rows and against
      the unguided job.
      --ab PARENT_TREE: ramp_guide_step, the cloud-guided and the unguided job run on the PARENT commit -- a checkout of it with its library
      built -- in child processes of this script that alternate with this build's on one box; what is compared is the children's own medians.

The networks carry SYNTHETIC weights: this tool reports cost only and makes no claim about plan quality.  Appends to profiles/team_guide.txt.
usage: python ramp_amd/tools/team_bench.py [reps] [warm] [--tag TAG] [--ab PARENT_TREE]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("RAMP_TEAM_BENCH_TREE") or ROOT)      # (a child of --ab imports the package from the tree it is given)

T, B, H, S, P = 25, 4096, 48, 4, 1024
SIZES = (1, 2, 4, 8)
ITERS = (1, 2)
CLOUD_GUIDE = dict(radius=0.2, step=2e-3, w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=4.0)
TEAM = dict(radius=0.3, w=1.0)


def child(what):
    """Everything one process measures on the library of its tree: `what` = 'parent' (ramp_guide_step, cloud-guided and unguided job) or
    'this' (the same plus the team launches, the team clearance and the team jobs).  Returns a dict of medians in seconds."""
    import numpy as np
    import torch
    from ramp_amd import _lib, synth
    from ramp_amd.guide import cloud_table, fill_cost_guide
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    reps, warm = child.reps, child.warm
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    gcloud = torch.from_numpy(rng.uniform(-1, 1, (P, 2)).astype(np.float32)).cuda()
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    scene = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=1)).cuda()
    # rows in teams of 8 around common rough paths (any smaller team size divides them): every pair of a team inside radius_team
    x_np = rng.uniform(-1, 1, (B, H, S)).astype(np.float32)
    base = rng.uniform(-0.7, 0.7, (B // 8, 1, H, 2))
    ang = 2 * np.pi * np.arange(8) / 8
    ring = 0.1 * np.stack([np.cos(ang), np.sin(ang)], -1)[None, :, None, :]
    x_np[:, :, :2] = (base + ring + rng.uniform(-0.02, 0.02, (B // 8, 8, H, 2))).reshape(B, H, 2).astype(np.float32)
    x0 = torch.from_numpy(x_np).cuda()
    x = x0.clone()
    lib = _lib.load()

    def med(fn, reset=None):
        ts = []
        for k in range(warm + reps):
            if reset is not None:
                reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warm:
                ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    out = {}
    idx = (C.c_int32 * 2)(0, H - 1)
    val = torch.stack([v.cuda().unsqueeze(0).expand(B, -1) for v in hc.values()]).contiguous()
    pts, off, d = cloud_table([gcloud], "cuda")
    cg = fill_cost_guide(pts, off, d, dict(CLOUD_GUIDE))
    s = _lib.current_stream()
    for n_iter in ITERS:
        out[f"cloud_step_{n_iter}"] = med(lambda: _lib.check(lib.ramp_guide_step(_lib.ptr(x), B, H, S, C.byref(cg), None, n_iter, CLOUD_GUIDE["step"], 2,
                                                                                 C.cast(idx, _lib.c_i32p), _lib.ptr(val), s), "ramp_guide_step"),
                                          lambda: x.copy_(x0))
    if what == "this":
        from ramp_amd.team import fill_team_guide
        mask = torch.zeros(B, dtype=torch.int32, device="cuda")
        plen, smooth = torch.rand(B, device="cuda"), torch.rand(B, device="cuda")
        for A in SIZES:
            tg = fill_team_guide(dict(size=A, **TEAM))
            for n_iter in ITERS:
                out[f"team_step_{A}_{n_iter}"] = med(lambda: _lib.check(lib.ramp_guide_step_team(
                    _lib.ptr(x), B, H, S, C.byref(cg), C.byref(tg), None, n_iter, CLOUD_GUIDE["step"], 2, C.cast(idx, _lib.c_i32p), _lib.ptr(val), s),
                    "ramp_guide_step_team"), lambda: x.copy_(x0))
            f = [torch.empty(B // A, device="cuda") for _ in range(4)]
            i = [torch.empty(B // A, dtype=torch.int32, device="cuda") for _ in range(3)]
            out[f"clearance_{A}"] = med(lambda: _lib.check(lib.ramp_team_clearance(
                _lib.ptr(x0), B, H, S, 2, A, 0.1, 1, _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(smooth), _lib.ptr(f[0]), _lib.ptr(f[1]), _lib.ptr(i[0]),
                _lib.ptr(i[1]), _lib.ptr(i[2]), _lib.ptr(f[2]), _lib.ptr(f[3]), s), "ramp_team_clearance"))
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=2 * B + 256), sd)
    dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True,
                                      noise_source="philox").eval().to("cuda:0")
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=H)
    jobs = {"unguided_job": {}, "cloud_job": dict(cost_guide=dict(CLOUD_GUIDE, cloud=gcloud))}
    if what == "this":
        for A in SIZES[1:]:
            jobs[f"team_job_{A}"] = dict(cost_guide=dict(CLOUD_GUIDE, cloud=gcloud, team=dict(size=A, **TEAM)))
    for name, extra in jobs.items():
        out[name] = med(lambda: dm.run_inference(None, hc, n_samples=B, obstacle_pts=scene, **kw, **extra))
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("reps", type=int, nargs="?", default=5)
    ap.add_argument("warm", type=int, nargs="?", default=2)
    ap.add_argument("--tag", default="run")
    ap.add_argument("--ab", default=None, help="a checkout of the parent commit, library built: the cloud guide and the unguided job run there")
    ap.add_argument("--child", default=None, help="internal: parent|this, print the medians as one JSON line")
    a = ap.parse_args()
    child.reps, child.warm = a.reps, a.warm
    if a.child:
        print(json.dumps(child(a.child)), flush=True)
        return

    def spawn(what, tree):
        env = dict(os.environ, RAMP_TEAM_BENCH_TREE=tree)
        env.pop("RAMP_HIP_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.reps), str(a.warm), "--child", what], env=env,
                             capture_output=True, text=True, timeout=900, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])

    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    runs = {"parent": [], "this": []}
    for _ in range(2 if a.ab else 1):      # alternating child processes, one library each
        if a.ab:
            runs["parent"].append(spawn("parent", os.path.abspath(a.ab)))
        runs["this"].append(spawn("this", ROOT))
    m = lambda who, k: statistics.median(r[k] for r in runs[who])      # noqa: E731
    base = "parent" if a.ab else "this"
    whose = "parent commit" if a.ab else "this build"
    say(f"# team_bench {a.tag}: B = {B} rows, H = {H}, {P}-point cloud, T = {T}, DDPM, Philox noise, hipGraph; {a.reps} timed after {a.warm} warm-up per "
        f"process; device {runs['this'][0]['device']}; {'parent commit and this build in alternating child processes' if a.ab else 'one library'}; "
        "synthetic weights: cost only")
    ev = m(base, "unguided_job") / T
    for n_iter in ITERS:
        cs = m(base, f"cloud_step_{n_iter}")
        say(f"(1) {n_iter} iteration(s) in one launch: ramp_guide_step ({whose}) {cs * 1e3:7.3f} ms; one score evaluation (unguided job / {T}) {ev * 1e3:7.3f} ms")
        for A in SIZES:
            ts = m("this", f"team_step_{A}_{n_iter}")
            say(f"    ramp_guide_step_team, teams of {A}: {ts * 1e3:7.3f} ms = x {ts / cs:.3f} of ramp_guide_step, {ts / ev:.4f} of an evaluation")
    say("(2) ramp_team_clearance, swept, with the selection's per-row arrays: " +
        ", ".join(f"teams of {A} {m('this', f'clearance_{A}') * 1e3:.3f} ms" for A in SIZES))
    cj, uj = m(base, "cloud_job"), m(base, "unguided_job")
    for A in SIZES[1:]:
        tj = m("this", f"team_job_{A}")
        say(f"(3) job with the team guide, teams of {A} (2 iterations on each of {T} steps) {tj * 1e3:8.1f} ms; cloud-guided job ({whose}) "
            f"{cj * 1e3:8.1f} ms: x {tj / cj:.4f}; unguided job {uj * 1e3:8.1f} ms: x {tj / uj:.4f}")
    if a.ab:
        say(f"    this build's own cloud-guided job {m('this', 'cloud_job') * 1e3:8.1f} ms (x {m('this', 'cloud_job') / cj:.4f} of the parent's), unguided job "
            f"{m('this', 'unguided_job') * 1e3:8.1f} ms (x {m('this', 'unguided_job') / uj:.4f})")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "team_guide.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
