"""What the cost guide costs inside a replan: one ramp_replan_guided call with the guide on the last DDIM step at 1, 2 and 4 iterations
against the unguided replan of THIS tree and of the PARENT commit, and the same for the many-episode job.

  single   config 4's replan: B = 8192 candidates x 2 CFG rows, H = 48, DDIM-5, 16 x 64-point clouds (1024 static guide points), n_mov = 64
  episodes episodes_bench.py's shapes: E episodes of 35 candidates (E = 8 and 64), 6 x 64-point clouds each, n_mov = 64

Every side runs in a child process of its own (a fresh context, its graphs captured in the warm-up), the sides alternate round by round on
one box, and a side's figure is the median over the rounds of each child's median replan time (wall clock around the call, which
synchronises its stream).  The parent's side needs a checkout of the parent commit with its library built (--parent TREE); it drives the
same set-up through ramp_replan / ramp_replan_episodes, the only entries it has.  Synthetic weights: no claim about plan quality.
Appends to profiles/replan_guide.txt (--out PATH: another file).
usage: python ramp_amd/tools/replan_guide_bench.py [--parent TREE] [--rounds 3] [--calls 20] [--episodes 8,64] [--tag TAG] [--out PATH]"""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S, H, T, PER = 4, 48, 100, 35
GUIDE = dict(radius=0.2, radius_mov=0.3, w_obs=1.0, w_mov=1.0, w_smooth=0.5, w_acc=0.0, max_norm=4.0)
STEP = 0.01


def opt(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


# ---------------------------------------------------------------------------------------------- a child: one side, one shape
def child(shape: str, n_iter: int, calls: int):
    """shape 'single' or 'episodesE'; n_iter < 0: the unguided entry (ramp_replan / ramp_replan_episodes).  Prints one JSON line."""
    import ctypes as C

    import numpy as np
    import torch

    from ramp_amd import _lib, synth
    from ramp_amd.apf_dynamic import generate_box_points, generate_sphere_points
    from ramp_amd.diffusion import _HostArrays
    from ramp_amd.models import DynamicGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.scenes import build_episode_tables
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict

    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    E = 1 if shape == "single" else int(shape[len("episodes"):])
    counts = [8192] if shape == "single" else [PER] * E
    B = sum(counts)
    sd = synth.make_unet_state_dict(make_unet_spec(S, H), seed=0)
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=2 * B), sd)
    dm = DynamicGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True, use_graph=True).eval().to(dev)
    m, lib = dm.model, _lib.load()
    rng = np.random.RandomState(7)
    n_box = 16 if shape == "single" else 6
    centres = [rng.uniform(-0.9, 0.9, (n_box, 2)) for _ in range(E)]
    clouds = [torch.from_numpy(np.stack([generate_box_points(c, (0.16, 0.16), 64, rng=rng) for c in cs]).astype(np.float32)).to(dev) for cs in centres]
    cost = [c.reshape(-1, 2).contiguous() for c in clouds]
    static = [torch.from_numpy(np.vstack([generate_box_points(c, (0.16, 0.16), 64, rng=rng) for c in cs[:4]])).to(dev) for cs in centres]
    start, goal = np.float32([-0.8, -0.8, 0, 0]), np.float32([0.8, 0.8, 0, 0])
    w = np.linspace(0, 1, H, dtype=np.float32)[:, None]
    plan = ((1 - w) * start[None] + w * goal[None]).astype(np.float32)
    x_clean = torch.from_numpy(np.tile(plan[None], (E, 1, 1))).to(dev).contiguous()
    hist = torch.zeros((E, H, S), device=dev)
    hist[:, :2] = x_clean[:, :2]
    n_hist, stepp = 2, 1
    centre = plan[stepp, :2].astype(np.float64) + [0.3, 0.2]
    dyn = np.stack([generate_sphere_points(centre, 0.1, 64, rng=rng) for _ in range(E)])
    extra = dyn.astype(np.float32)
    near = np.ones(E, np.int32)
    noise = torch.randn((B, H, S), device=dev, generator=torch.Generator(dev).manual_seed(3))
    hard = {0: torch.from_numpy(start).to(dev).repeat(B, 1), H - 1: torch.from_numpy(goal).to(dev).repeat(B, 1)}
    ts = [int(i) for i in dm.ddim_set_timesteps(dm.ddim_num_inference_steps_high)]
    low = ts[-dm.ddim_num_inference_steps_low:]
    m.prepare_time_table(dm.n_diffusion_steps)
    arrays = _HostArrays()
    res = _lib.RampReplanResult()
    best = torch.empty((E, H, S), device=dev)
    rg = None
    if n_iter >= 0:
        from ramp_amd.guide import cloud_table, fill_replan_guide
        pts, off, _d = cloud_table(cost, dev)
        mov = np.ascontiguousarray(dyn, np.float32)
        track = np.ascontiguousarray(np.tile((np.maximum(0, np.arange(H) - stepp)[:, None] * np.float32([[-0.01, -0.008]]))[None], (E, 1, 1)), np.float32)
        rg = fill_replan_guide(arrays.keep(pts), arrays.keep(off), arrays.keep(mov), arrays.keep(track), GUIDE)
        rg.n_guide, rg.step = arrays.i32([0] * (len(low) - 1) + [n_iter]), arrays.f32([STEP] * len(low))
    if shape == "single":
        dm._prepare_scene(clouds[0], B)
        p = dm._replan_params(B, low, hard, cost[0], 0.05, arrays)
        p.static_pts, p.n_static = _lib.ptr(static[0]), static[0].shape[0]
        st = _lib.RampReplanState()
        st.noise, st.x_clean, st.history = _lib.ptr(noise), _lib.ptr(x_clean[0]), _lib.ptr(hist[0])
        st.n_hist, st.stepp = n_hist, stepp
        st.dyn_pts_host, st.near, st.extra_pts_host = dyn[0].ctypes.data, 1, extra[0].ctypes.data
        st.pursuer[0], st.pursuer[1] = float(centre[0]), float(centre[1])
        if rg is None:
            call = lambda: lib.ramp_replan(m.ctx(), C.byref(p), C.byref(st), _lib.ptr(best), None, None, C.byref(res), _lib.current_stream())      # noqa: E731
        else:
            call = lambda: lib.ramp_replan_guided(m.ctx(), C.byref(p), C.byref(st), C.byref(rg), _lib.ptr(best), None, None, C.byref(res),      # noqa: E731
                                                  _lib.current_stream())
    else:
        tab = build_episode_tables(counts, [dm._row_pattern(n) for n in counts])
        latents = torch.cat([m.encode_scenes(clouds), torch.zeros(1, m.context_dim, device=dev)])
        m.set_scenes(latents, tab["row_variant"])
        cost_all, static_all = torch.cat(cost).contiguous(), torch.cat(static).contiguous()
        cost_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in cost])]).astype(np.int32)
        static_off = np.concatenate([[0], np.cumsum([s.shape[0] for s in static])]).astype(np.int32)
        p = dm._replan_params(B, low, hard, cost_all, 0.05, arrays)
        p.cost_cloud, p.n_cost = None, 0
        state = (_lib.RampEpisodeState * E)()
        for e in range(E):
            state[e].n_hist, state[e].stepp, state[e].active = n_hist, stepp, 1
            state[e].pursuer[0], state[e].pursuer[1] = float(centre[0]), float(centre[1])
        eb = _lib.RampEpisodeBatch()
        eb.n_episodes, eb.traj_first_host, eb.state_host = E, tab["traj_first"].ctypes.data_as(_lib.c_i32p), state
        eb.noise, eb.x_clean, eb.history = _lib.ptr(noise), _lib.ptr(x_clean), _lib.ptr(hist)
        eb.static_pts, eb.static_offset_host = _lib.ptr(static_all), static_off.ctypes.data_as(_lib.c_i32p)
        eb.cost_cloud, eb.cost_offset_host = _lib.ptr(cost_all), cost_off.ctypes.data_as(_lib.c_i32p)
        eb.dyn_pts_host, eb.near_host, eb.extra_pts_host = dyn.ctypes.data, near.ctypes.data_as(_lib.c_i32p), extra.ctypes.data
        results = np.zeros((E, 4), np.int32)
        rp = results.ctypes.data_as(_lib.c_i32p)
        if rg is None:
            call = lambda: lib.ramp_replan_episodes(m.ctx(), C.byref(p), C.byref(eb), _lib.ptr(best), None, None, rp, C.byref(res),      # noqa: E731
                                                    _lib.current_stream())
        else:
            call = lambda: lib.ramp_replan_episodes_guided(m.ctx(), C.byref(p), C.byref(eb), C.byref(rg), _lib.ptr(best), None, None, rp,      # noqa: E731
                                                           C.byref(res), _lib.current_stream())
    fell = 0
    for _ in range(4):                                       # both graphs (calibrating, steady) captured
        _lib.check(call(), "replan")
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        _lib.check(call(), "replan")
        times.append(time.perf_counter() - t0)
        fell += int(res.fell_back != 0)
    print(json.dumps(dict(shape=shape, n_iter=n_iter, B=B, median_ms=statistics.median(times) * 1e3, min_ms=min(times) * 1e3,
                          max_ms=max(times) * 1e3, fell_back=fell, n_free=int(res.n_free))), flush=True)


# ---------------------------------------------------------------------------------------------- the alternation
def main():
    if "--child" in sys.argv:
        return child(opt("--shape", "single"), int(opt("--iters", "-1")), int(opt("--calls", "20")))
    parent = opt("--parent", None)
    rounds, calls = int(opt("--rounds", "3")), opt("--calls", "20")
    shapes = ["single"] + [f"episodes{int(v)}" for v in opt("--episodes", "8,64").split(",") if v]
    tag = opt("--tag", "run")
    out = opt("--out", os.path.join(ROOT, "profiles", "replan_guide.txt"))
    sides = ([("parent, unguided", parent, -1)] if parent else []) + [("this tree, unguided", ROOT, -1)] + \
            [(f"this tree, {k} guide iteration{'s' if k > 1 else ''} on the last step", ROOT, k) for k in (1, 2, 4)]
    lines = [f"# replan_guide_bench {tag}: one replan (DDIM-5, CFG, hipGraph), median of {calls} calls per child, {rounds} alternating rounds; "
             f"parent tree: {'given' if parent else 'not given'}"]
    print(lines[0], flush=True)
    for shape in shapes:
        got = {name: [] for name, _, _ in sides}
        for _ in range(rounds):
            for name, tree, k in sides:
                env = dict(os.environ, PYTHONPATH=tree)
                env.pop("RAMP_HIP_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--iters", str(k), "--calls", calls],
                                   env=env, cwd=tree, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"child '{name}' on {shape} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                got[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        base = statistics.median(g["median_ms"] for g in got[sides[0][0]])
        for name, _, _ in sides:
            meds = [g["median_ms"] for g in got[name]]
            med = statistics.median(meds)
            lines.append(f"{shape:11s} B = {got[name][0]['B']:5d}  {name:55s} median {med:8.3f} ms  rounds {min(meds):8.3f} .. {max(meds):8.3f}  "
                         f"{med - base:+7.3f} ms ({med / base:.4f} x) vs {sides[0][0]}; range fallbacks {sum(g['fell_back'] for g in got[name])}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
