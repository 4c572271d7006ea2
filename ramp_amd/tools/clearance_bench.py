"""What the swept collision check costs: ramp_traj_clearance with and without the segment work at the two shapes that matter,

  2-D   B = 4096, H = 48, S = 4, D = 2, 1024 cloud points, 6 boxes                  (the static planner's batch)
  3-D   B = 4096, H = 64, S = 6, D = 3, 4096 cloud points, 10 boxes + 10 spheres    (Maze3D)

beside ramp_traj_costs at the 2-D shape (the same waypoint work against the cloud, no segments, no boxes: the code the selection runs
today) and beside ONE score evaluation at B = 4096 x 2 rows, H = 48 (rowtime_bench.py's set-up), which is what a sampling job pays per
denoising step.

Every figure is per launch: `launches` back-to-back launches between two device events, `reps` such windows per side after `warm` warm-up
launches, the sides alternating window by window in one process; median and min .. max over the windows.  The score evaluation is timed
one call per window.  Appends to profiles/clearance.txt.
usage: python ramp_amd/tools/clearance_bench.py [--reps 15] [--launches 50] [--warm 5] [--no-score] [--out FILE]"""
from __future__ import annotations

import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ramp_amd import _lib, synth  # noqa: E402

B = 4096
SHAPES = {"2-D": dict(H=48, S=4, D=2, P=1024, boxes=6, spheres=0), "3-D": dict(H=64, S=6, D=3, P=4096, boxes=10, spheres=10)}


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def make_side(shape, swept):
    """A closure that launches ramp_traj_clearance once on a seeded batch of straight-ish trajectories across [-1, 1]^D."""
    H, S, D, P = shape["H"], shape["S"], shape["D"], shape["P"]
    rng = np.random.default_rng(11)
    w = np.linspace(0, 1, H, dtype=np.float32)[None, :, None]
    ends = rng.uniform(-0.9, 0.9, (2, B, 1, S)).astype(np.float32)
    x = ((1 - w) * ends[0] + w * ends[1] + 0.03 * rng.standard_normal((B, H, S)).astype(np.float32)).astype(np.float32)
    t = torch.from_numpy(x).cuda()
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()      # noqa: E731
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()        # noqa: E731
    keep = dict(t=t, bc=f32(rng.uniform(-0.8, 0.8, (shape["boxes"], D))), bs=f32(np.full((shape["boxes"], D), 0.26)),
                sc=f32(rng.uniform(-0.8, 0.8, (max(shape["spheres"], 1), D))), sr=f32(np.full(max(shape["spheres"], 1), 0.1)),
                cloud=f32(rng.uniform(-1, 1, (P, D))), first=i32([0, B]), bo=i32([0, shape["boxes"]]), so=i32([0, shape["spheres"]]),
                co=i32([0, P]), hits=torch.empty(2, B, dtype=torch.int32, device="cuda"), vals=torch.empty(4, B, device="cuda"))
    ob = _lib.RampObstacles()
    ob.point_dim, ob.n_scenes, ob.margin = D, 1, 0.0
    ob.box_centers, ob.box_sizes, ob.sphere_centers, ob.sphere_radii, ob.cloud = (keep[k].data_ptr() for k in ("bc", "bs", "sc", "sr", "cloud"))
    ob.box_offset, ob.sphere_offset, ob.cloud_offset = keep["bo"].data_ptr(), keep["so"].data_ptr(), keep["co"].data_ptr()
    ob.n_boxes_total, ob.n_spheres_total, ob.n_points_total = shape["boxes"], shape["spheres"], P
    lib, s = _lib.load(), _lib.current_stream()
    hits, vals = keep["hits"], keep["vals"]

    def launch():
        _lib.check(lib.ramp_traj_clearance(t.data_ptr(), B, H, S, C.byref(ob), keep["first"].data_ptr(), swept, hits[0].data_ptr(),
                                           hits[1].data_ptr(), vals[0].data_ptr(), vals[1].data_ptr(), vals[2].data_ptr(),
                                           vals[3].data_ptr(), s), "ramp_traj_clearance")
    launch.keep = (keep, ob)
    return launch


def make_costs(shape):
    H, S, P = shape["H"], shape["S"], shape["P"]
    side = make_side(shape, 0)
    keep, _ = side.keep
    mask = torch.empty(B, dtype=torch.int32, device="cuda")
    plen, smooth = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    lib, s = _lib.load(), _lib.current_stream()

    def launch():
        _lib.check(lib.ramp_traj_costs(keep["t"].data_ptr(), B, H, S, keep["cloud"].data_ptr(), P, 0.05, mask.data_ptr(), plen.data_ptr(),
                                       smooth.data_ptr(), s), "ramp_traj_costs")
    launch.keep = (keep, mask, plen, smooth)
    return launch


def make_score():
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    H, S, n_rp = 48, 4, 2
    m = TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=B * n_rp)
    load_numpy_state_dict(m, synth.make_unet_state_dict(make_unet_spec(S, H)))
    m = m.eval().to("cuda")
    lat = m.encode_scene(torch.from_numpy(synth.make_cloud(6, 64, 2, seed=3)).cuda())
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    x = torch.from_numpy(synth.make_noise((B, H, S), seed=21)).cuda()
    eps = torch.empty((B * n_rp, H, S), device="cuda")
    lib, s = _lib.load(), _lib.current_stream()

    def launch():
        _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(x), B, n_rp, 11, None, _lib.ptr(eps), s), "ramp_score")
    launch.keep = (m, x, eps)
    return launch


def window(fn, n):
    """Milliseconds per launch over n back-to-back launches between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    reps, launches, warm = int(opt("--reps", "15")), int(opt("--launches", "50")), int(opt("--warm", "5"))
    out = opt("--out", os.path.join(ROOT, "profiles", "clearance.txt"))
    sides = []
    for name, shape in SHAPES.items():
        what = f"{shape['P']} points, {shape['boxes']} boxes" + (f" + {shape['spheres']} spheres" if shape["spheres"] else "")
        sides.append((f"{name} H = {shape['H']} {what}: ramp_traj_clearance, waypoints only", make_side(shape, 0), launches))
        sides.append((f"{name} H = {shape['H']} {what}: ramp_traj_clearance, swept", make_side(shape, 1), launches))
        if name == "2-D":
            sides.append((f"{name} H = {shape['H']} {shape['P']} points: ramp_traj_costs (cloud mask, no segments, no boxes)", make_costs(shape), launches))
    if "--no-score" not in sys.argv:
        sides.append((f"one score evaluation, B = {B} x 2 rows, H = 48, S = 4", make_score(), 1))
    for _, fn, _n in sides:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _, _ in sides}
    for _ in range(reps):
        for name, fn, n in sides:
            got[name].append(window(fn, n))
    lines = [f"# clearance_bench: B = {B}; ms per launch, {launches} launches per window between device events, {reps} alternating windows "
             f"after {warm} warm-up launches (score: one call per window)"]
    med = {}
    for name, _, _ in sides:
        v = got[name]
        med[name] = statistics.median(v)
        lines.append(f"  {name:95s} median {med[name]:9.4f} ms   min {min(v):9.4f}   max {max(v):9.4f}")
    names = [n for n, _, _ in sides]
    for d in SHAPES:
        wp, sw = (next(n for n in names if n.startswith(d) and n.endswith(e)) for e in ("waypoints only", "swept"))
        lines.append(f"  {d}: swept / waypoints only = {med[sw] / med[wp]:.2f}")
    score = next((n for n in names if n.startswith("one score")), None)
    if score:
        for d in SHAPES:
            sw = next(n for n in names if n.startswith(d) and n.endswith("swept"))
            lines.append(f"  {d}: swept pass / one score evaluation = {med[sw] / med[score]:.4f}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as fh:
        fh.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
