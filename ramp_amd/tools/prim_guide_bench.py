"""What the swept box and sphere terms of the cost guide cost (cost_guide=dict(boxes=, spheres=, ...)): T = 25 DDPM, Philox noise, hipGraph,
B = 4096.

  (1) one launch of ramp_guide_step_prims with 2 iterations at the headline guide shape (H = 48, D = 2, 64 boxes, n_sub 1 / 4 / 8) and at the
      3-D shape (H = 64, 64 boxes + 64 spheres, n_sub 1 / 4 / 8), against one launch of ramp_guide_step (the cloud guide of
      ramp_amd/tools/guide_bench.py: 1024 2-D / 4096 3-D points) at the same B, H and iteration count, and against one score evaluation
      (unguided job / 25).  The C entries are timed directly on prepared tables (their own table upload and synchronisation are inside, for
      both); the trajectories are reset before every timed call.
  (2) the 25-step job with the primitives-only guide (n_sub = 4, 2 iterations on every reverse step) against the cloud-guided job of the
      same rows and against the unguided job.
      --ab PARENT_TREE: ramp_guide_step, the cloud-guided and the unguided job run on the PARENT commit -- a checkout of it with its library
      built -- in child processes of this script that alternate with this build's on one box; what is compared is the children's own medians.

The networks carry SYNTHETIC weights: this tool reports cost only and makes no claim about plan quality.  Appends to profiles/prim_guide.txt.
usage: python ramp_amd/tools/prim_guide_bench.py [reps] [warm] [--tag TAG] [--ab PARENT_TREE]"""
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
sys.path.insert(0, os.environ.get("RAMP_PRIM_BENCH_TREE") or ROOT)      # (a child of --ab imports the package from the tree it is given)

T, B, N_ITER = 25, 4096, 2
SHAPES = {"2d": dict(S=4, H=48, o3=False, P=1024, d=2, boxes=64, spheres=0), "3d": dict(S=6, H=64, o3=True, P=4096, d=3, boxes=64, spheres=64)}
CLOUD_GUIDE = dict(radius=0.2, step=2e-3, w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=N_ITER, max_norm=4.0)
PRIM_GUIDE = dict(cloud=None, w_obs=0.0, w_smooth=0.5, w_acc=0.25, step=2e-3, n_steps=N_ITER, max_norm=4.0, margin=0.05, band=0.05)
SUBS = (1, 4, 8)


def child(shape, what):
    """Everything one process measures on the library of its tree: `what` = 'parent' (ramp_guide_step, cloud-guided and unguided job) or
    'this' (the same plus the primitive launches and the primitive-guided job).  Returns a dict of medians in seconds."""
    import numpy as np
    import torch
    from ramp_amd import _lib, synth
    from ramp_amd.guide import cloud_table, fill_cost_guide
    from ramp_amd.models import GaussianDiffusionModel3d, StaticGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    reps, warm = child.reps, child.warm
    sh = SHAPES[shape]
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    gcloud = torch.from_numpy(rng.uniform(-1, 1, (sh["P"], sh["d"])).astype(np.float32)).cuda()
    boxes = (torch.from_numpy(rng.uniform(-1, 1, (sh["boxes"], sh["d"])).astype(np.float32)).cuda(),
             torch.from_numpy(rng.uniform(0.1, 0.3, (sh["boxes"], sh["d"])).astype(np.float32)).cuda())
    spheres = None
    if sh["spheres"]:
        spheres = (torch.from_numpy(rng.uniform(-1, 1, (sh["spheres"], sh["d"])).astype(np.float32)).cuda(),
                   torch.from_numpy(rng.uniform(0.05, 0.15, sh["spheres"]).astype(np.float32)).cuda())
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(sh["S"], sh["H"]).items()}
    scene = torch.from_numpy(synth.make_cloud(4, 30, 3, seed=41) if sh["o3"] else synth.make_cloud(6, 64, 2, seed=1)).cuda()
    x0 = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (B, sh["H"], sh["S"])).astype(np.float32)).cuda()
    x = x0.clone()
    lib, s = _lib.load(), None

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
    idx = (C.c_int32 * 2)(0, sh["H"] - 1)
    val = torch.stack([v.cuda().unsqueeze(0).expand(B, -1) for v in hc.values()]).contiguous()
    pts, off, d = cloud_table([gcloud], "cuda")
    cg = fill_cost_guide(pts, off, d, dict(CLOUD_GUIDE))
    s = _lib.current_stream()
    out["cloud_step"] = med(lambda: _lib.check(lib.ramp_guide_step(_lib.ptr(x), B, sh["H"], sh["S"], C.byref(cg), None, N_ITER, CLOUD_GUIDE["step"], 2,
                                                                   C.cast(idx, _lib.c_i32p), _lib.ptr(val), s), "ramp_guide_step"), lambda: x.copy_(x0))
    if what == "this":
        from ramp_amd.guide import fill_prim_guide, prim_scalars, prim_table
        tab = prim_table(boxes, spheres, 1, sh["d"], "cuda")
        e_pts, e_off, _ = cloud_table([torch.zeros(0, sh["d"])], "cuda")
        cg0 = fill_cost_guide(e_pts, e_off, sh["d"], dict(w_smooth=0.5, w_acc=0.25, max_norm=4.0))
        for n_sub in SUBS:
            pg = fill_prim_guide(tab, prim_scalars(PRIM_GUIDE["margin"], PRIM_GUIDE["band"], 1.0, n_sub))
            out[f"prim_step_{n_sub}"] = med(lambda: _lib.check(lib.ramp_guide_step_prims(_lib.ptr(x), B, sh["H"], sh["S"], C.byref(cg0), C.byref(pg), None,
                                                                                         N_ITER, PRIM_GUIDE["step"], 2, C.cast(idx, _lib.c_i32p),
                                                                                         _lib.ptr(val), s), "ramp_guide_step_prims"), lambda: x.copy_(x0))
    sd = synth.make_unet_state_dict(make_unet_spec(sh["S"], sh["H"], obstacle_3d=sh["o3"]), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=sh["H"], state_dim=sh["S"], obstacle_3d=sh["o3"], max_rows=2 * B + 256), sd)
    cls = GaussianDiffusionModel3d if sh["o3"] else StaticGaussianDiffusionModel
    dm = cls(model=u, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=True, noise_source="philox").eval().to("cuda:0")
    kw = dict(noise_std_extra_schedule_fn=lambda t: 0.5, horizon=sh["H"])
    jobs = {"unguided_job": {}, "cloud_job": dict(cost_guide=dict(CLOUD_GUIDE, cloud=gcloud))}
    if what == "this":
        jobs["prim_job"] = dict(cost_guide=dict(PRIM_GUIDE, boxes=boxes, spheres=spheres, n_sub=4))
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
    ap.add_argument("--child", default=None, help="internal: SHAPE:parent|this, print the medians as one JSON line")
    a = ap.parse_args()
    child.reps, child.warm = a.reps, a.warm
    if a.child:
        shape, what = a.child.split(":")
        print(json.dumps(child(shape, what)), flush=True)
        return

    def spawn(shape, what, tree):
        env = dict(os.environ, RAMP_PRIM_BENCH_TREE=tree)
        env.pop("RAMP_HIP_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(a.reps), str(a.warm), "--child", f"{shape}:{what}"], env=env,
                             capture_output=True, text=True, timeout=900, check=True).stdout
        return json.loads(out.strip().splitlines()[-1])

    lines, dev = [], None

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for shape, sh in SHAPES.items():
        runs = {"parent": [], "this": []}
        for _ in range(2 if a.ab else 1):      # alternating child processes, one library each
            if a.ab:
                runs["parent"].append(spawn(shape, "parent", os.path.abspath(a.ab)))
            runs["this"].append(spawn(shape, "this", ROOT))
        dev = runs["this"][0]["device"]
        if not lines:
            say(f"# prim_guide_bench {a.tag}: B = {B}, T = {T}, DDPM, Philox noise, hipGraph; {a.reps} timed after {a.warm} warm-up per process; device "
                f"{dev}; {'parent commit and this build in alternating child processes' if a.ab else 'one library'}; synthetic weights: cost only")
        m = lambda who, k: statistics.median(r[k] for r in runs[who])      # noqa: E731
        base = "parent" if a.ab else "this"
        ev = m(base, "unguided_job") / T
        cs = m(base, "cloud_step")
        prims = f"{sh['boxes']} boxes" + (f" + {sh['spheres']} spheres" if sh["spheres"] else "")
        say(f"(1) {shape}: H = {sh['H']}, {N_ITER} iterations in one launch: ramp_guide_step ({sh['P']}-point cloud, {'parent commit' if a.ab else 'this build'}) "
            f"{cs * 1e3:7.3f} ms; one score evaluation (unguided job / {T}) {ev * 1e3:7.3f} ms")
        for n_sub in SUBS:
            ps = m("this", f"prim_step_{n_sub}")
            say(f"    ramp_guide_step_prims, {prims}, n_sub = {n_sub}: {ps * 1e3:7.3f} ms = x {ps / cs:.3f} of ramp_guide_step, {ps / ev:.4f} of an evaluation")
        pj, cj, uj = m("this", "prim_job"), m(base, "cloud_job"), m(base, "unguided_job")
        say(f"(2) {shape}: job with the primitive guide (n_sub = 4, {N_ITER} iterations on each of {T} steps) {pj * 1e3:8.1f} ms; cloud-guided job "
            f"({'parent commit' if a.ab else 'this build'}) {cj * 1e3:8.1f} ms: x {pj / cj:.4f}; unguided job {uj * 1e3:8.1f} ms: x {pj / uj:.4f}")
        if a.ab:
            say(f"    this build's own cloud-guided job {m('this', 'cloud_job') * 1e3:8.1f} ms (x {m('this', 'cloud_job') / cj:.4f} of the parent's), unguided job "
                f"{m('this', 'unguided_job') * 1e3:8.1f} ms (x {m('this', 'unguided_job') / uj:.4f})")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "prim_guide.txt"), "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
