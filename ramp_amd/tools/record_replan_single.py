"""The single-episode replan entries (ramp_replan, ramp_replan_guided) pinned byte for byte: records tests/golden/replan_single_parent.npz.

Run once by hand on the GPU against the build whose results are to be kept (the commit before the single entry became the one-episode
job of the many-episode body); tests/test_gpu_replan_one_path.py replays the same sequences through ``replay`` and requires every stored
output bit for bit.  The fixture holds every input except the network weights (``in/...``: noise, history, x_clean, the scene, static,
pursuer, cost and extra clouds, hard conditions, the DDIM schedule, the guide's tables) and per call ``out/<sequence>/<call>/`` best, batch,
mask, record {n_free, rank, row, fell_back}, the launch count and, where guided, the tap.  The weights are the seeded synthetic ones
(ramp_amd/synth.py).  B = 6, H = 48, S = 4, DDIM-5 of T = 100: replan_chain.npz's shape, whose scene cloud and first plan are reused.

Sequences, each on a fresh context:
  a_graph, a_eager   three replans in a row (x_clean given, then twice the previous winner; near 0, 1, 0), use_graph 1 and 0
  b                  the first call with n_steps = 1 (always calibrates)
  c_none, c_two      the first call without hard conditions, and with two others (waypoints 5 and 20)
  d_guided, d_zero   guided: 3 iterations on the last step, n_mov = 64, tap; and a guide without an iteration
  e                  cost_thr so large that every candidate collides (`best` is not stored: nothing defines it there)
  f_graph, f_eager   sequence a on the bf16x6 kernels
  g                  a single call, a one-episode ramp_replan_episodes call on the same context, a single call with x_clean given; the
                     single calls are stored
usage: python ramp_amd/tools/record_replan_single.py [--out PATH]"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "replan_single_parent.npz")
B, H, S, T, N_DYN, N_EXTRA = 6, 48, 4, 100, 64, 64
GUIDE_SCALARS = dict(radius=0.2, radius_mov=0.3, w_obs=1.0, w_mov=1.0, w_smooth=0.5, w_acc=0.0, max_norm=4.0)
SEQUENCES = ("a_graph", "a_eager", "b", "c_none", "c_two", "d_guided", "d_zero", "e", "f_graph", "f_eager", "g")
# (n_hist, stepp, near) of the three calls of a sequence
CALLS = ((1, 0, 0), (2, 1, 1), (3, 2, 0))


def make_model(gemm_mode="default"):
    """A fresh context with the seeded synthetic weights, and the planner around it (for the scene and the time table only)."""
    import torch

    from ramp_amd import synth
    from ramp_amd.models import DynamicGaussianDiffusionModel, TemporalUnetInference
    from ramp_amd.spec import make_unet_spec
    from ramp_amd.unet import load_numpy_state_dict
    torch.cuda.set_device(0)
    sd = synth.make_unet_state_dict(make_unet_spec(S, H, obstacle_3d=False))
    u = load_numpy_state_dict(TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=False, max_rows=2 * B, gemm_mode=gemm_mode), sd)
    u = u.eval().to("cuda")
    dm = DynamicGaussianDiffusionModel(model=u, n_diffusion_steps=T, predict_epsilon=True).eval().to("cuda")
    u.prepare_time_table(T)
    return dm, u


def make_inputs() -> dict:
    """Every input of the sequences, as numpy arrays (seeded; the schedule from the planner's own tables)."""
    from ramp_amd.apf_dynamic import generate_box_points, generate_sphere_points
    g = np.load(os.path.join(ROOT, "tests", "golden", "replan_chain.npz"))
    rng = np.random.RandomState(11)
    inp = {}
    inp["scene_cloud"] = g["cloud"].astype(np.float32)                                  # (6, 64, 2): the scene the network sees
    inp["cost"] = np.ascontiguousarray(inp["scene_cloud"].reshape(-1, 2))               # (384, 2) float32
    centres = inp["scene_cloud"].mean(axis=1)[:4].astype(np.float64)
    inp["static"] = np.vstack([generate_box_points(c, (0.16, 0.16), 16, rng=rng) for c in centres]).astype(np.float64)      # (64, 2)
    inp["x_clean"] = g["cost0/best"].astype(np.float32)
    inp["history"] = np.zeros((H, S), np.float32)
    inp["history"][:3] = inp["x_clean"][:3]
    inp["noise"] = rng.standard_normal((3, B, H, S)).astype(np.float32)
    pursuer = np.stack([inp["x_clean"][stepp, :2].astype(np.float64) + off for (_, stepp, _), off in zip(CALLS, ([0.7, 0.7], [0.15, 0.1], [0.6, -0.5]))])
    inp["pursuer"] = pursuer.astype(np.float32)
    inp["dyn"] = np.stack([generate_sphere_points(c, 0.1, N_DYN, rng=rng) for c in pursuer]).astype(np.float64)
    inp["extra"] = np.stack([generate_sphere_points(c, 0.1, N_EXTRA, rng=rng) for c in pursuer]).astype(np.float32)
    inp["hard_idx"] = np.array([0, H - 1], np.int32)
    inp["hard_val"] = np.stack([np.tile(g["hard0"][None], (B, 1)), np.tile(g["hardN"][None], (B, 1))]).astype(np.float32)
    inp["hard_idx_two"] = np.array([5, 20], np.int32)
    inp["hard_val_two"] = rng.uniform(-0.5, 0.5, (2, B, S)).astype(np.float32)
    # the schedule: the low-level tail of the planner's DDIM steps
    dm, _ = make_model()
    ts = [int(i) for i in dm.ddim_set_timesteps(dm.ddim_num_inference_steps_high)]
    low = ts[-5:]
    inp["t"] = np.array(low, np.int32)
    for k, v in dm._ddim_coefficients(low, dm.ddim_num_inference_steps_high).items():
        inp[k] = np.array([float(x) for x in v], np.float32)
    inp["q"] = np.array([float(dm.sqrt_alphas_cumprod[low[0]]), float(dm.sqrt_one_minus_alphas_cumprod[low[0]])], np.float32)
    inp["w"] = np.array([float(dm.cfg_weight)], np.float64)
    inp["flags"] = np.array([int(bool(dm.clip_denoised)), int(not dm.predict_epsilon)], np.int32)      # clip_denoised, predict_x0
    # the guide: the cost cloud, the first call's pursuer cloud and a track that carries it along the plan, 0.06 beside it
    inp["guide_cloud"] = inp["cost"].copy()
    inp["guide_mov"] = inp["dyn"][:1].astype(np.float32)
    inp["guide_track"] = (inp["x_clean"][:, :2] - inp["pursuer"][0][None] + np.float32([0.05, 0.03])[None])[None].astype(np.float32)
    inp["guide_scalars"] = np.array([GUIDE_SCALARS[k] for k in sorted(GUIDE_SCALARS)], np.float32)
    inp["guide_step"] = np.full(5, 0.02, np.float32)
    return inp


class _Job:
    """One context and what its calls point at."""

    def __init__(self, inp, gemm_mode="default"):
        import torch

        from ramp_amd import _lib
        self.inp, self.lib, self._lib, self.torch = inp, _lib.load(), _lib, torch
        self.dm, self.m = make_model(gemm_mode)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.d = {k: dev(inp[k]) for k in ("scene_cloud", "cost", "static", "x_clean", "history", "noise", "hard_val", "hard_val_two", "guide_cloud")}
        self.dm._prepare_scene(self.d["scene_cloud"], B)
        self.keep = []

    def params(self, n_steps=5, hard="default", cost_thr=0.05, use_graph=1):
        from ramp_amd.diffusion import _HostArrays
        inp, _lib = self.inp, self._lib
        a = _HostArrays(); self.keep.append(a)
        p = _lib.RampReplanParams()
        p.B, p.n_rp, p.n_steps, p.w = B, 2, n_steps, float(inp["w"][0])
        p.clip_denoised, p.predict_x0 = int(inp["flags"][0]), int(inp["flags"][1])
        first = 5 - n_steps                                   # (a shorter job is the tail of the schedule: it still ends at t = 0)
        p.t = a.i32(inp["t"][first:])
        for k in ("sqrt_recip", "sqrt_recipm1", "sqrt_a_t", "sqrt_1m_a_t", "sqrt_a_prev", "dir_coef"):
            setattr(p, k, a.f32(inp[k][first:]))
        p.q_sqrt_a, p.q_sqrt_1m_a = float(inp["q"][0]), float(inp["q"][1])
        if hard == "default":
            p.n_hard, p.hard_idx_host, p.hard_val = 2, a.i32(inp["hard_idx"]), _lib.ptr(self.d["hard_val"])
        elif hard == "two":
            p.n_hard, p.hard_idx_host, p.hard_val = 2, a.i32(inp["hard_idx_two"]), _lib.ptr(self.d["hard_val_two"])
        else:
            p.n_hard = 0
        p.sm_window_last, p.sm_window_final, p.sm_dt, p.sm_max_vel = 3, 2, 0.1, 0.8
        p.thr_static, p.thr_pred, p.strength_static, p.strength_pred, p.window_static = 0.2, 0.5, 0.15, 0.15, 8
        p.static_pts, p.n_static, p.n_dyn = _lib.ptr(self.d["static"]), self.d["static"].shape[0], N_DYN
        p.cost_cloud, p.n_cost, p.n_extra = _lib.ptr(self.d["cost"]), self.d["cost"].shape[0], N_EXTRA
        p.cost_thr, p.w_smooth, p.w_len, p.use_graph = cost_thr, 0.1, 0.9, use_graph
        return p

    def guide(self, n_iter):
        """(ramp_replan_guide, tap tensor): n_iter iterations on the last step (0: a guide without an iteration, no tap)."""
        from ramp_amd.diffusion import _HostArrays
        from ramp_amd.guide import fill_replan_guide
        inp = self.inp
        a = _HostArrays(); self.keep.append(a)
        off = np.array([0, inp["guide_cloud"].shape[0]], np.int32)
        mov, track = np.ascontiguousarray(inp["guide_mov"]), np.ascontiguousarray(inp["guide_track"])
        self.keep += [off, mov, track]
        rg = fill_replan_guide(self.d["guide_cloud"], off, mov, track, dict(zip(sorted(GUIDE_SCALARS), (float(v) for v in inp["guide_scalars"]))))
        rg.n_guide, rg.step = a.i32([0, 0, 0, 0, n_iter]), a.f32(inp["guide_step"])
        tap = self.torch.full((2, B, H, S), float("nan"), device="cuda") if n_iter else None
        rg.tap_out = self._lib.ptr(tap)
        return rg, tap

    def single(self, p, k, x_clean=True, rg=None, tap=None) -> dict:
        """Call k of a sequence (its noise, record, pursuer) through ramp_replan, or ramp_replan_guided with a guide."""
        inp, _lib, torch = self.inp, self._lib, self.torch
        n_hist, stepp, near = CALLS[k]
        st = _lib.RampReplanState()
        st.noise, st.history = _lib.ptr(self.d["noise"][k]), _lib.ptr(self.d["history"])
        st.x_clean = _lib.ptr(self.d["x_clean"]) if x_clean else None
        st.n_hist, st.stepp, st.near = n_hist, stepp, near
        dyn, extra = np.ascontiguousarray(inp["dyn"][k]), np.ascontiguousarray(inp["extra"][k])
        st.dyn_pts_host, st.extra_pts_host = dyn.ctypes.data, extra.ctypes.data if near else None
        st.pursuer[0], st.pursuer[1] = float(inp["pursuer"][k][0]), float(inp["pursuer"][k][1])
        best, batch = torch.full((H, S), float("nan"), device="cuda"), torch.empty((B, H, S), device="cuda")
        mask, res = torch.empty(B, dtype=torch.int32, device="cuda"), _lib.RampReplanResult()
        ctx, s = self.m.ctx(), _lib.current_stream()
        if rg is None:
            _lib.check(self.lib.ramp_replan(ctx, C.byref(p), C.byref(st), _lib.ptr(best), _lib.ptr(batch), _lib.ptr(mask), C.byref(res), s), "ramp_replan")
        else:
            _lib.check(self.lib.ramp_replan_guided(ctx, C.byref(p), C.byref(st), C.byref(rg), _lib.ptr(best), _lib.ptr(batch), _lib.ptr(mask),
                                                   C.byref(res), s), "ramp_replan_guided")
        torch.cuda.synchronize()
        out = dict(best=best.cpu().numpy(), batch=batch.cpu().numpy(), mask=mask.cpu().numpy(),
                   record=np.array([res.n_free, res.best_rank, res.best_row, res.fell_back], np.int32),
                   launches=np.array([self.m.launch_count()], np.int64))
        if tap is not None:
            out["tap"] = tap.cpu().numpy()
        return out

    def one_episode(self, p, k):
        """Call k as a one-episode ramp_replan_episodes job (its row table installed first); nothing of it is stored."""
        from ramp_amd.scenes import build_episode_tables
        inp, _lib, torch = self.inp, self._lib, self.torch
        n_hist, stepp, near = CALLS[k]
        tab = build_episode_tables([B], [self.dm._row_pattern(B)])
        latents = torch.cat([self.m.encode_scene(self.d["scene_cloud"]), torch.zeros(1, self.m.context_dim, device="cuda")])
        self.m.set_scenes(latents, tab["row_variant"])
        state = (_lib.RampEpisodeState * 1)()
        state[0].n_hist, state[0].stepp, state[0].active = n_hist, stepp, 1
        state[0].pursuer[0], state[0].pursuer[1] = float(inp["pursuer"][k][0]), float(inp["pursuer"][k][1])
        first = np.array([0, B], np.int32)
        s_off, c_off = np.array([0, inp["static"].shape[0]], np.int32), np.array([0, inp["cost"].shape[0]], np.int32)
        near_a = np.array([near], np.int32)
        dyn, extra = np.ascontiguousarray(inp["dyn"][k]), np.ascontiguousarray(inp["extra"][k])
        eb = _lib.RampEpisodeBatch()
        eb.n_episodes, eb.traj_first_host, eb.state_host = 1, first.ctypes.data_as(_lib.c_i32p), state
        eb.noise, eb.x_clean, eb.history = _lib.ptr(self.d["noise"][k]), _lib.ptr(self.d["x_clean"]), _lib.ptr(self.d["history"])
        eb.static_pts, eb.static_offset_host = p.static_pts, s_off.ctypes.data_as(_lib.c_i32p)
        eb.cost_cloud, eb.cost_offset_host = p.cost_cloud, c_off.ctypes.data_as(_lib.c_i32p)
        eb.dyn_pts_host, eb.near_host, eb.extra_pts_host = dyn.ctypes.data, near_a.ctypes.data_as(_lib.c_i32p), extra.ctypes.data
        results, rr = np.zeros((1, 4), np.int32), _lib.RampReplanResult()
        _lib.check(self.lib.ramp_replan_episodes(self.m.ctx(), C.byref(p), C.byref(eb), None, None, None, results.ctypes.data_as(_lib.c_i32p),
                                                 C.byref(rr), _lib.current_stream()), "ramp_replan_episodes")
        torch.cuda.synchronize()


def run_sequence(inp, name) -> list:
    """The stored calls of one sequence on a fresh context: a list of dicts (best, batch, mask, record, launches[, tap])."""
    job = _Job(inp, "bf16x6" if name.startswith("f_") else "default")
    if name in ("a_graph", "a_eager", "f_graph", "f_eager"):
        p = job.params(use_graph=int(name.endswith("graph")))
        return [job.single(p, k, x_clean=k == 0) for k in range(3)]
    if name == "b":
        return [job.single(job.params(n_steps=1), 0)]
    if name in ("c_none", "c_two"):
        return [job.single(job.params(hard=name[2:]), 0)]
    if name in ("d_guided", "d_zero"):
        rg, tap = job.guide(3 if name == "d_guided" else 0)
        return [job.single(job.params(), 0, rg=rg, tap=tap)]
    if name == "e":
        return [job.single(job.params(cost_thr=10.0), 0)]
    assert name == "g"
    p = job.params()
    first = job.single(p, 0)
    job.one_episode(p, 1)
    return [first, job.single(p, 0)]


def replay(inp, sequences=SEQUENCES) -> dict:
    """{'<sequence>/<call>/<output>': array} of the listed sequences (with e/0/best, which the fixture leaves out)."""
    out = {}
    for name in sequences:
        for k, call in enumerate(run_sequence(inp, name)):
            out.update({f"{name}/{k}/{key}": v for key, v in call.items()})
    return out


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    inp = make_inputs()
    out = replay(inp)
    del out["e/0/best"]                                       # (every candidate collides: nothing defined `best` there)
    for k in sorted(out):
        if k.endswith("/record"):
            print(f"{k}: {out[k].tolist()}  launches {int(out[k[:-6] + 'launches'][0])}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **{f"in/{k}": v for k, v in inp.items()}, **{f"out/{k}": v for k, v in out.items()})
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} outputs of {len(SEQUENCES)} sequences")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
