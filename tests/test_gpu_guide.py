"""Cost-gradient guidance inside the sampling job, 2-D and 3-D: the kernel alone (``ramp_guide_step``), the cost terms (``ramp_guide_cost``),
the wiring into ``ramp_sample_guided`` (bit-exact against the kernel applied to the unguided job's output), "off is off", free-running guided
chains against float64, stale graphs and the refusals.

The truth is the float64 numpy restatement of the definition in include/ramp_hip.h written below (``guide_grad`` / ``guide_iterate`` /
``guide_terms``; ``GuideOracle`` inserts it into ``oracle.ramp_oracle.SamplerOracle``'s loops at the place the header gives).  The same code
in float32 is the yardstick: every bar that is not an exact statement is 4 x the float32 restatement's distance from the float64 one on the
test's own inputs, measured on the CPU inside the test, never what the HIP code gives.  The kernel rounds the five scalars and the step to
fp32 once; the tests hand over fp32-representable values, so both sides compute with the same numbers."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.diffusion import guide_tables
from ramp_amd.spec import UNET_DIM_MULTS
from util import NoiseInjector, dev

pytestmark = pytest.mark.gpu

TILE = 1024      # GUIDE_TILE of ramp_amd/csrc/args_sampler.h
F32 = lambda v: float(np.float32(v))      # noqa: E731
RADIUS = F32(0.35)


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def guide_terms(p, c, r):
    """(C_obs, C_smooth, C_acc), unweighted, of positions p (H, d) against cloud c (P, d): pair values in p's dtype, sums in float64."""
    dt = p.dtype.type
    obs = 0.0
    if len(c):
        dx = p.T[:, :, None] - c.T.astype(p.dtype)[:, None, :]
        u = np.maximum(dt(0), dt(r) - np.sqrt((dx * dx).sum(0)))
        obs = float((dt(0.5) * u * u).astype(np.float64).sum())
    dp = p[1:] - p[:-1]
    a = (p[2:] - dt(2) * p[1:-1]) + p[:-2]
    return np.array([obs, float((dt(0.5) * (dp * dp).sum(1)).astype(np.float64).sum()), float((dt(0.5) * (a * a).sum(1)).astype(np.float64).sum())])


def guide_grad(p, c, r, w_obs, w_smooth, w_acc):
    """dC/dp (H, d) in p's dtype; a pair at distance 0 contributes nothing.  The sum over points runs over a contiguous last axis (numpy's
    pairwise order), the stencils in the order the header's formulas are written."""
    dt = p.dtype.type
    gs = np.zeros_like(p)
    gs[:-1] = p[:-1] - p[1:]
    gs[1:] += p[1:] - p[:-1]
    a = np.zeros_like(p)
    a[1:-1] = (p[2:] - dt(2) * p[1:-1]) + p[:-2]
    ga = dt(-2) * a
    ga[:-1] += a[1:]
    ga[1:] += a[:-1]
    g = dt(w_smooth) * gs + dt(w_acc) * ga
    if len(c) and w_obs != 0:
        dx = p.T[:, :, None] - c.T.astype(p.dtype)[:, None, :]                    # (d, H, P)
        d = np.sqrt((dx * dx).sum(0))
        inside = (d < dt(r)) & (d > 0)
        f = np.where(inside, (dt(r) - d) / np.where(inside, d, dt(1)), dt(0)).astype(p.dtype)
        g = dt(w_obs) * (-(f[None] * dx).sum(-1).T) + g
    return g.astype(p.dtype)


def guide_iterate(x, clouds, traj_scene, pins, r, w_obs, w_smooth, w_acc, step, n_iter, max_norm, dtype, d=None, log=None):
    """n_iter guide iterations on trajectories x (B, H, S) -> new array of ``dtype``.  clouds: per scene (P, d); traj_scene (B,) or None;
    pins {waypoint: (S,) or (B, S)} (later entries win).  ``log`` collects (trajectory, iteration, s)."""
    out = np.array(x, dtype=dtype)
    dt = out.dtype.type
    B, H, S = out.shape
    d = d or clouds[0].shape[-1]
    for b in range(B):
        c = clouds[0 if traj_scene is None else int(traj_scene[b])].reshape(-1, d)
        p = out[b, :, :d].copy()
        free = np.ones(H, bool)
        for h, v in pins.items():
            v = np.asarray(v)
            p[h] = (v if v.ndim == 1 else v[b])[:d].astype(dtype)
            free[h] = False
        for it in range(n_iter):
            g = guide_grad(p, c, r, w_obs, w_smooth, w_acc)
            g[~free] = 0
            n = dt(np.sqrt((g.astype(np.float64) ** 2).sum()))
            s = min(dt(1), dt(max_norm) / n) if (max_norm > 0 and n > 0) else dt(1)
            if log is not None:
                log.append((b, it, float(s)))
            p[free] = (p - (dt(step) * dt(s)) * g)[free]
        out[b, free, :d] = p[free]
    return out


class GuideOracle(O.SamplerOracle):
    """SamplerOracle with the guide behind the posterior mean (DDPM) / x0 (DDIM), before the noise / the DDIM update and its hard
    conditioning.  ``guide`` = dict(cloud (P, d), tab = guide_tables(...) of the job) or None."""

    def __init__(self, *a, guide=None, **k):
        super().__init__(*a, **k)
        self.guide = guide

    def _guide(self, v, j, hard_conds):
        if self.guide is None or self.guide["tab"]["n_guide"][j] == 0:
            return v
        t = self.guide["tab"]
        return guide_iterate(v, [self.guide["cloud"]], None, hard_conds, t["radius"], t["w_obs"], t["w_smooth"], t["w_acc"],
                             np.float32(t["step"][j]), t["n_guide"][j], t["max_norm"], self.dt)

    def ddpm(self, noise, hard_conds, latent, noise_scale=0.5, **kw):
        s, dt = self.sched, self.dt
        x = O.apply_hard_conditioning(noise[0].astype(dt).copy(), hard_conds)
        chain = [x.copy()]
        for j, t in enumerate(reversed(range(self.T))):
            e = self.eps_cfg(x, t, latent)
            _, mean = self.x0_mean(x, e, t)
            mean = self._guide(mean, j, hard_conds)
            z = noise[1 + j].astype(dt) if t != 0 else np.zeros_like(x)
            std = np.exp(dt(0.5) * s["posterior_log_variance_clipped"][t])
            x = O.apply_hard_conditioning((mean + std * z * dt(noise_scale)).astype(dt), hard_conds)
            chain.append(x.copy())
        return np.stack(chain)

    def ddim(self, noise0, hard_conds, latent, K=5, **kw):
        s, dt = self.sched, self.dt
        x = O.apply_hard_conditioning(noise0.astype(dt).copy(), hard_conds)
        chain, ac = [x.copy()], s["alphas_cumprod"]
        for j, t in enumerate(O.ddim_timesteps(self.T, K)):
            prev = t - self.T // K
            a_t, a_prev = ac[t], (ac[prev] if prev >= 0 else dt(1.0))
            e = self.eps_cfg(x, int(t), latent)
            x0, _ = self.x0_mean(x, e, int(t))
            x0 = self._guide(x0, j, hard_conds)
            e2 = (x - np.sqrt(a_t) * x0) / np.sqrt(dt(1) - a_t)
            x = O.apply_hard_conditioning((np.sqrt(a_prev) * x0 + np.sqrt(dt(1) - a_prev) * e2).astype(dt), hard_conds)
            chain.append(x.copy())
        return np.stack(chain)


# ------------------------------------------------------------------------------------------------ inputs shared by the op tests
def uniform(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


PINS = {"ends": lambda H: [0, H - 1], "ends+3": lambda H: [0, 3, H - 1]}
WEIGHTS = {"all": (1.0, 0.5, 0.25), "obs": (1.0, 0.0, 0.0), "noobs": (0.0, 0.5, 0.25)}
# (small scene's P, large scene's P, H, S, d, n_iter, pins, weights): every value of the issue's lists, the tile size and its neighbours, an
# empty cloud, the obstacle sum alone and no obstacle term
OP_CASES = [(1, TILE, 8, 2, 2, 1, "ends", "all"), (63, TILE + 1, 48, 4, 2, 3, "ends+3", "all"), (64, 2500, 64, 6, 3, 3, "ends", "all"),
            (65, TILE - 1, 48, 6, 3, 1, "ends+3", "all"), (0, 2500, 48, 4, 2, 3, "ends", "all"), (65, TILE + 1, 64, 2, 2, 3, "ends+3", "obs"),
            (63, TILE, 8, 6, 3, 3, "ends", "noobs"), (64, TILE - 1, 64, 4, 2, 1, "ends", "all"), (1, 2500, 48, 6, 3, 3, "ends+3", "obs")]
OP_STEP = F32(2e-3)
_OP = {}


def op_case(case):
    """Inputs and both restatements of one op case, computed once: x (3, H, S), the two clouds, traj_scene (0, 1, 0), pins with random values,
    max_norm between the smallest and the largest first-iteration gradient norm (one trajectory clipped, another not)."""
    if case not in _OP:
        Ps, Pl, H, S, d, n_iter, pins, wk = case
        seed = 1000 + OP_CASES.index(case)
        x = uniform((3, H, S), seed)
        clouds = [uniform((Ps, d), seed + 100), uniform((Pl, d), seed + 200)]
        ts = np.array([0, 1, 0], np.int32)
        idx = PINS[pins](H)
        val = uniform((len(idx), 3, S), seed + 300)
        pd = {h: val[k] for k, h in enumerate(idx)}
        w = WEIGHTS[wk]
        norms = []
        for b in range(3):
            p = x[b, :, :d].astype(np.float64)
            for h in idx:
                p[h] = pd[h][b, :d]
            g = guide_grad(p, clouds[ts[b]].astype(np.float64), RADIUS, *w)
            g[idx] = 0
            norms.append(float(np.sqrt((g ** 2).sum())))
        max_norm = F32(np.sqrt(min(norms) * max(norms)))
        args = (clouds, ts, pd, RADIUS, w[0], w[1], w[2], OP_STEP, n_iter, max_norm)
        log = []
        y64 = guide_iterate(x, *args, np.float64, log=log)
        y32 = guide_iterate(x, *args, np.float32)
        _OP[case] = dict(x=x, clouds=clouds, ts=ts, idx=idx, val=val, w=w, max_norm=max_norm, y64=y64, y32=y32, log=log, norms=norms)
    return _OP[case]


def run_op(x, clouds, ts, idx, val, w, step, n_iter, max_norm, radius=RADIUS):
    from ramp_amd.guide import cost_guide_step
    hc = {h: dev(val[k]) for k, h in enumerate(idx)}
    y = cost_guide_step(dev(x), [dev(c) for c in clouds], radius, step, w_obs=w[0], w_smooth=w[1], w_acc=w[2], n_steps=n_iter, max_norm=max_norm,
                        hard_conds=hc, traj_scene=None if ts is None else dev(ts))
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: the op against float64
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "P%d-%d_H%d_S%d_d%d_it%d_%s_%s" % c)
def test_op_against_float64(case):
    """B = 3 trajectories in [-1, 1] over 2 scenes (0, 1, 0) with ragged uniform clouds, r = 0.35, step 2e-3, weights (1, 0.5, 0.25) (or the
    obstacle sum alone / no obstacle term), random pinned values, max_norm the geometric mean of the smallest and largest first gradient
    norm.  Bar: 4 x the float32 numpy restatement's largest distance from the float64 one on these inputs -- measured on the CPU here,
    2.8e-8 .. 8.2e-8 over the nine cases (printed) -- so 1.1e-7 .. 3.3e-7; the HIP sum over points runs in another
    order than numpy's and 4 x covers the order, no more."""
    c = op_case(case)
    s1 = [s for b, it, s in c["log"] if it == 0]
    assert min(s1) < 1.0 and max(s1) == 1.0, s1                    # one trajectory clipped, another not
    moved = float(np.abs(c["y64"] - c["x"]).max())
    d32 = float(np.abs(c["y32"] - c["y64"]).max())
    assert moved > 1e-3 and d32 > 0
    y = run_op(c["x"], c["clouds"], c["ts"], c["idx"], c["val"], c["w"], OP_STEP, case[5], c["max_norm"])
    err = float(np.abs(y - c["y64"]).max())
    print(f"guide op {case}: HIP {err:.2e}, float32 restatement {d32:.2e} (bar {4 * d32:.2e}); moved {moved:.2e}, first s {np.round(s1, 3).tolist()}")
    assert err <= 4 * d32


# ------------------------------------------------------------------------------------------------ 2: what must not move
@pytest.mark.parametrize("case", [OP_CASES[1], OP_CASES[2], OP_CASES[4]], ids=["2d", "3d", "empty"])
def test_what_must_not_move(case):
    """Pinned waypoints and channels >= d keep their bits; with w_smooth = w_acc = 0 and no cloud point within r nothing moves at all; a
    trajectory's result does not depend on the batch around it (alone = inside the batch of 3, bit for bit)."""
    c = op_case(case)
    Ps, Pl, H, S, d, n_iter, pins, wk = case
    y = run_op(c["x"], c["clouds"], c["ts"], c["idx"], c["val"], c["w"], OP_STEP, n_iter, c["max_norm"])
    xb, yb = c["x"].view(np.uint32), y.view(np.uint32)
    assert np.array_equal(yb[:, c["idx"]], xb[:, c["idx"]])
    assert np.array_equal(yb[:, :, d:], xb[:, :, d:])
    free = np.setdiff1d(np.arange(H), c["idx"])
    assert (yb[:, free, :d] != xb[:, free, :d]).mean() > 0.9      # (and the rest did move)
    far = [cl + np.float32(5.0) for cl in c["clouds"]]
    y0 = run_op(c["x"], far, c["ts"], c["idx"], c["val"], (1.0, 0.0, 0.0), OP_STEP, n_iter, c["max_norm"])
    assert np.array_equal(y0.view(np.uint32), xb)
    for b in range(3):
        alone = run_op(c["x"][b:b + 1], c["clouds"], c["ts"][b:b + 1], c["idx"], c["val"][:, b:b + 1], c["w"], OP_STEP, n_iter, c["max_norm"])
        assert np.array_equal(alone.view(np.uint32), yb[b:b + 1]), b
    # n_iter iterations in one launch = n_iter launches of one (the positions round to fp32 once per iteration either way)
    z = c["x"]
    for _ in range(n_iter):
        z = run_op(z, c["clouds"], c["ts"], c["idx"], c["val"], c["w"], OP_STEP, 1, c["max_norm"])
    assert np.array_equal(z.view(np.uint32), yb)


# ------------------------------------------------------------------------------------------------ 3: the cost terms
@pytest.mark.parametrize("S,d,H", [(4, 2, 48), (6, 3, 64), (2, 2, 8)])
def test_cost_terms_against_float64(S, d, H):
    """ramp_guide_cost on B = 3 trajectories over the clouds (65, 1025 points) and an all-empty table: relative 1e-6 on each term (fp64 sums
    over fp32 pair values).  The float32 restatement (fp32 pair values, fp64 sums) sits at 5e-9 .. 8.2e-8 on these inputs (printed, asserted
    below 2.5e-7)."""
    from ramp_amd.guide import cost_guide_terms
    x = uniform((3, H, S), 77 + H)
    clouds = [uniform((65, d), 78), uniform((1025, d), 79)]
    ts = np.array([0, 1, 0], np.int32)
    got = cost_guide_terms(dev(x), [dev(c) for c in clouds], RADIUS, traj_scene=dev(ts)).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3, 3)
    for b in range(3):
        want = guide_terms(x[b, :, :d].astype(np.float64), clouds[ts[b]].astype(np.float64), RADIUS)
        f32 = guide_terms(x[b, :, :d], clouds[ts[b]], RADIUS)
        assert (want > 0).all()
        print(f"cost terms S={S} d={d} H={H} b={b}: HIP {np.abs(got[b] / want - 1).max():.2e}, float32 restatement {np.abs(f32 / want - 1).max():.2e}")
        assert np.abs(f32 / want - 1).max() < 2.5e-7
        assert np.abs(got[b] / want - 1).max() < 1e-6
    empty = cost_guide_terms(dev(x), dev(np.zeros((0, d), np.float32)), RADIUS).cpu().numpy()
    assert (empty[:, 0] == 0).all() and np.array_equal(empty[:, 1:], got[:, 1:])


# ------------------------------------------------------------------------------------------------ the smallest network
def small_model(S=4, o3=False, T=25, sampler="ddpm", use_graph=True, noise_source="torch", noise_seed=0, schedule="exponential", use_apf=False):
    """UNET_DIM_MULTS[0], unet_input_dim 16, H = 8."""
    from ramp_amd import models
    from test_gpu_shapes import build_shape_unet
    u = build_shape_unet(S, 8, o3, 0, 16, max_rows=16)
    cls = models.GaussianDiffusionModel3d if o3 else models.StaticGaussianDiffusionModel
    return cls(model=u, variance_schedule=schedule, n_diffusion_steps=T, predict_epsilon=True, sampler=sampler, use_graph=use_graph,
               noise_source=noise_source, noise_seed=noise_seed, use_apf=use_apf).eval().to("cuda")


def hcn(S):
    return synth.default_hard_conds(S, 8)


def hct(S):
    return {k: torch.from_numpy(v) for k, v in hcn(S).items()}


def raw_params(dm, B, steps, arrays, ddim, hard=None, use_graph=1):
    p = _lib.RampSampleParams()
    p.B, p.n_rp, p.w0, p.w1 = B, 2, dm.cfg_weight, 0.0
    dm._fill_schedule(p, arrays, ddim, steps, [0.5] * len(steps), ddim_K=5)
    p.apply_apf = arrays.i32([0] * len(steps))
    p.clip_denoised, p.predict_x0, p.use_graph = 1, 0, use_graph
    if hard is not None:
        dm._fill_hard(p, arrays, hard, B)
    return p


def raw_guide(arrays, clouds, n_guide, step, w=(1.0, 0.5, 0.25), radius=RADIUS, max_norm=0.0):
    from ramp_amd.guide import cloud_table, fill_cost_guide
    pts, off, d = cloud_table(clouds, "cuda")
    cg = fill_cost_guide(arrays.keep(pts), arrays.keep(off), d, dict(radius=radius, w_obs=w[0], w_smooth=w[1], w_acc=w[2], max_norm=max_norm))
    cg.n_guide, cg.step = arrays.i32(n_guide), arrays.f32(step)
    return cg


# ------------------------------------------------------------------------------------------------ 4: wiring, bit-exact
WIRE_STEP = F32(5e-3)
WIRE_MAX = F32(2.0)


# (the 3-D sampler is always DDPM; the APF case is run once, on DDPM: DDIM re-pins x0 between the hook's passes)
WIRE_CASES = [(job, kind) for kind in ("ddpm", "ddim") for job in ("plain", "scenes", "composed", "ula")] + [("3d", "ddpm"), ("apf", "ddpm")]


@pytest.mark.parametrize("job,kind", WIRE_CASES)
def test_wiring_is_the_kernel_on_the_unguided_output(job, kind):
    """A one-iteration job, B = 4, injected noise whose step slot is zero: the guided job's output equals ramp_guide_step applied to the
    unguided job's output, bit for bit (the free waypoints of hard(mean) are the mean's; the kernel pins its own working copy).  DDPM at
    t = 12 (x = mean + std 0) and the last DDIM step (t = 0: sqrt_a_prev = 1, dir_coef = 0, so x = x0).  As a plain job, a 2-scene job with
    different clouds, a composed job, a ULA job with one inner step, the 3-D model with a (P, 3) cloud, and once with the APF on in the same
    iteration (order: APF, then guide; DDPM, no hard conditions, so that the unguided APF-free output is the mean the hook sees)."""
    from ramp_amd.apf import ObstacleField, avoidance
    from ramp_amd.diffusion import _HostArrays
    from ramp_amd.guide import cost_guide_step
    lib = _lib.load()
    o3 = job == "3d"
    S, d, B, H = (6, 3, 4, 8) if o3 else (4, 2, 4, 8)
    ddim = kind == "ddim"
    dm = small_model(S, o3, sampler=kind)
    steps = [0] if ddim else [12]
    arrays = _HostArrays()
    noise = synth.make_noise((2, B, H, S), seed=90)
    noise[1] = 0
    noise = dev(noise)
    hc = None if job == "apf" else {k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hct(S).items()}
    scene_cloud = synth.make_cloud(4, 30, 3, seed=41) if o3 else synth.make_cloud(6, 64, 2, seed=3)
    ctx, s = dm.model.ctx(), _lib.current_stream()
    dm.model.prepare_time_table(25)
    rows = batch = mp = z = None
    gclouds = [dev(uniform((300, d), 91))]
    ts = None
    if job in ("scenes", "composed"):
        if job == "scenes":
            sj, hcc, Bc = dm._prepare_scene_job([dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))], [hct(S)] * 2, [1, 3])
        else:
            sc = [[dev(synth.make_cloud(5, 64, 2, seed=31))], [dev(synth.make_cloud(4, 64, 2, seed=32 + k)) for k in range(2)]]
            sj, guid, hcc, Bc = dm._prepare_composed_job(sc, [hct(S)] * 2, [1, 3], None, None)
        assert Bc == B
        hc = hcc
        batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(sj["traj_scene"])
        ts = sj["traj_scene"]
        gclouds = [dev(uniform((70, d), 92)), dev(uniform((1100, d), 93))]
    else:
        dm._prepare_scene(dev(scene_cloud), B)
    p = raw_params(dm, B, steps, arrays, ddim, hard=hc)
    if job == "composed":
        p.n_rp, p.w0, p.w1 = guid["n_rp"], 0.0, 0.0
        rows = _lib.RampGuidanceRows(); rows.n_rp, rows.row_weight = guid["n_rp"], _lib.ptr(guid["row_weight"])
    if job == "ula":
        mp = _lib.RampMcmcParams(); mp.kind = 1
        mp.n_inner, mp.step_size, mp.sigma = arrays.i32([1]), arrays.f32([0.01]), arrays.f32([float(dm.sqrt_one_minus_alphas_cumprod[steps[0]])])
        z = dev(synth.make_noise((1, B, H, S), seed=94))
    apf_cloud = dev(uniform((400, 2), 95))
    if job == "apf":
        p.apply_apf = arrays.i32([1])
    cg = raw_guide(arrays, gclouds, [2], [WIRE_STEP], max_norm=WIRE_MAX)

    def run(guide, apf=False):
        out = torch.empty((B, H, S), device="cuda")
        if apf:
            dm._fill_apf(p, arrays, dict(window=5, threshold=0.25, strength=0.1, passes=1), apf_cloud)
        else:
            p.apf.cloud = None
        _lib.check(lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg) if guide else None, C.byref(mp) if mp is not None else None,
                                          C.byref(rows) if rows is not None else None, C.byref(batch) if batch is not None else None,
                                          _lib.ptr(noise), _lib.ptr(z), None, None, _lib.ptr(out), None, s), "ramp_sample_guided")
        torch.cuda.synchronize()
        return out

    plain = run(False)
    guided = run(True, apf=job == "apf")
    base = plain
    if job == "apf":
        base = avoidance(plain, ObstacleField(apf_cloud, distance_threshold=0.25), avoidance_window=5, avoidance_strength=0.1)
        assert not torch.equal(base, plain)                       # the hook did fire
        assert torch.equal(base, run(False, apf=True))            # and the job's hook is that kernel
    want = cost_guide_step(base, gclouds, RADIUS, WIRE_STEP, w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=WIRE_MAX,
                           hard_conds=hc, traj_scene=ts)
    moved = float((want - base).abs().max())
    print(f"wiring {job} {kind}: guide moved the output by {moved:.2e}")
    assert moved > 1e-3 and np.isfinite(guided.cpu().numpy()).all()
    assert torch.equal(guided, want)


# ------------------------------------------------------------------------------------------------ 5: off is off
def test_off_is_off_bit_for_bit():
    """cg == NULL and n_guide = 0 everywhere give ramp_sample_mcmc's chain; t_start = 0 gives the unguided Python call, with injected and
    with Philox noise."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = small_model()
    B, H, S, steps = 4, 8, 4, [24, 12, 1, 0]
    arrays = _HostArrays()
    noise = dev(synth.make_noise((len(steps) + 1, B, H, S), seed=8))
    dm.model.prepare_time_table(25)
    cloud = dev(synth.make_cloud(6, 64, 2, seed=3))
    dm._prepare_scene(cloud, B)
    p = raw_params(dm, B, steps, arrays, False, hard={k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hct(S).items()})
    ctx, s = dm.model.ctx(), _lib.current_stream()
    mp0 = _lib.RampMcmcParams()
    gcloud = dev(uniform((300, 2), 91))
    cg0 = raw_guide(arrays, [gcloud], [0] * 4, [WIRE_STEP] * 4)
    cg1 = raw_guide(arrays, [gcloud], [0, 1, 1, 1], [WIRE_STEP] * 4)
    chains = []
    for call in (lambda o: lib.ramp_sample_mcmc(ctx, C.byref(p), C.byref(mp0), None, None, _lib.ptr(noise), None, None, _lib.ptr(o), None, None, s),
                 lambda o: lib.ramp_sample_guided(ctx, C.byref(p), None, None, None, None, _lib.ptr(noise), None, None, _lib.ptr(o), None, None, s),
                 lambda o: lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg0), C.byref(mp0), None, None, _lib.ptr(noise), None, None, _lib.ptr(o),
                                                  None, None, s),
                 lambda o: lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg1), None, None, None, _lib.ptr(noise), None, None, _lib.ptr(o), None,
                                                  None, s)):
        o = torch.empty((len(steps) + 1, B, H, S), device="cuda")
        _lib.check(call(o), "job")
        torch.cuda.synchronize()
        chains.append(o)
    assert np.isfinite(chains[0].cpu().numpy()).all()
    assert torch.equal(chains[0], chains[1]) and torch.equal(chains[0], chains[2])
    assert torch.equal(chains[0][:2], chains[3][:2]) and not torch.equal(chains[0][2], chains[3][2])      # (and on is on, from iteration 1)
    # the Python keyword
    off = dict(cloud=gcloud, radius=RADIUS, step=WIRE_STEP, w_smooth=0.5, t_start=0)
    for src in ("torch", "philox"):
        res = []
        for kw in ({}, dict(cost_guide=off), dict(cost_guide=dict(off, t_start=float("inf")))):
            m = small_model(noise_source=src, noise_seed=5)
            torch.manual_seed(3)
            res.append(m.run_inference(None, hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=cloud,
                                       noise_std_extra_schedule_fn=lambda x: 0.5, **kw))
            assert m.last_job_mode is not None
        assert torch.equal(res[0], res[1]), src
        assert not torch.equal(res[0], res[2]), src


# ------------------------------------------------------------------------------------------------ 6: free-running chains against float64
CHAIN_GUIDE = dict(radius=RADIUS, step=F32(4e-3), w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=F32(4.0))
_CHAIN = {}


def chain_inputs(kind):
    T = 3 if kind == "ddpm" else 25
    n = (T + 1) if kind == "ddpm" else 1
    return T, synth.make_noise((n, 2, 8, 4), seed=600), uniform((500, 2), 601), synth.make_cloud(6, 64, 2, seed=3)


def chain_sched(T, kind):
    """the model's own schedule buffers (cosine for the 3-step DDPM job: the exponential schedule ends at beta = 1)."""
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    dm = StaticGaussianDiffusionModel(model=TemporalUnetInference(n_support_points=8, state_dim=4), n_diffusion_steps=T,
                                      variance_schedule="cosine" if kind == "ddpm" else "exponential", predict_epsilon=True, sampler=kind)
    names = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
             "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
             "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    return {k: getattr(dm, k).numpy() for k in names}, steps, dm.posterior_variance


def oracle_chains(kind):
    """float64 guided and unguided chains and the float32 guided chain of the free-running test, once per process (seconds on the CPU)."""
    if kind not in _CHAIN:
        from test_gpu_shapes import shape_weights
        T, noise, gcloud, scene = chain_inputs(kind)
        sched, steps, pv = chain_sched(T, kind)
        tab = guide_tables(dict(CHAIN_GUIDE, cloud=gcloud, t_start=steps[0]), steps, pv)
        assert tab["n_guide"] == [0] + [2] * (len(steps) - 1)
        out = {}
        for name, dtype, guide in (("g64", np.float64, True), ("u64", np.float64, False), ("g32", np.float32, True)):
            uo = O.UNetOracle(shape_weights(4, 8, False, 0, 16), 4, 8, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            so = GuideOracle(uo, T, 2.0, dtype=dtype, sched=sched, guide=dict(cloud=gcloud, tab=tab) if guide else None)
            lat = uo.encode_scene(scene)
            out[name] = so.ddpm(noise, hcn(4), lat) if kind == "ddpm" else so.ddim(noise[0], hcn(4), lat, K=5)
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """(bar, float32 oracle's distance, guided-vs-unguided distance of the final float64 states): what the inputs must satisfy."""
    c = oracle_chains(kind)
    bar = 1e-4 * float(np.abs(c["g64"]).max())
    return bar, float(np.abs(c["g32"] - c["g64"]).max()), float(np.abs(c["g64"][-1] - c["u64"][-1]).max())


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_guided_chain(kind):
    """A 3-iteration DDPM job (T = 3, cosine schedule) and the 5-step DDIM job (T = 25) at the smallest network, B = 2, guide on from the
    second iteration with n_steps = 2, through run_inference(cost_guide=): every state against the float64 oracle chain at the project's
    standing bar, 1e-4 of max |x|.  The inputs keep the float32 oracle within a quarter of that bar (checked here and in
    test_guide_host.py), and the float64 guided and unguided final states differ by >= 100 x the bar: the test cannot pass with the guide
    missing."""
    c = oracle_chains(kind)
    bar, d32, moved = chain_conditions(kind)
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    T, noise, gcloud, scene = chain_inputs(kind)
    dm = small_model(T=T, sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential")
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    with NoiseInjector(list(noise)):
        chain = dm.run_inference(None, hct(4), n_samples=2, horizon=8, return_chain=True, obstacle_pts=dev(scene),
                                 noise_std_extra_schedule_fn=lambda x: 0.5, cost_guide=dict(CHAIN_GUIDE, cloud=dev(gcloud), t_start=steps[0])
                                 ).cpu().numpy()
    assert chain.shape == c["g64"].shape
    err = float(np.abs(chain - c["g64"]).max())
    print(f"guided {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {d32:.2e}; guided vs unguided {moved:.2e}); mode {dm.last_job_mode}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 7: graph hygiene
def test_a_guided_job_never_replays_a_stale_graph():
    """Jobs of one shape back to back on one context with use_graph = 1: another step, then another radius, then another cloud of the same
    size -- each equals its own use_graph = 0 run bit for bit (and differs from its predecessor)."""
    B, H, S = 3, 8, 4
    noise = synth.make_noise((26, B, H, S), seed=5)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    cl_a, cl_b = dev(uniform((300, 2), 91)), dev(uniform((300, 2), 96))
    base = dict(radius=RADIUS, step=F32(4e-3), w_smooth=0.5, w_acc=0.25, n_steps=2, t_start=10, max_norm=F32(4.0))
    jobs = [dict(base, cloud=cl_a), dict(base, cloud=cl_a, step=F32(8e-3)), dict(base, cloud=cl_a, step=F32(8e-3), radius=F32(0.2)),
            dict(base, cloud=cl_b, step=F32(8e-3), radius=F32(0.2))]

    def run(dm, g):
        with NoiseInjector(list(noise)):
            return dm.run_inference(None, hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene,
                                    noise_std_extra_schedule_fn=lambda x: 0.5, cost_guide=g)

    graph, eager = small_model(use_graph=True), small_model(use_graph=False)
    prev = None
    for g in jobs:
        a, b = run(graph, g), run(eager, g)
        assert torch.equal(a, b)
        assert prev is None or not torch.equal(a, prev)
        prev = a
    assert torch.equal(run(graph, jobs[-1]), prev)      # (and a replay of the same job is the same job)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_of_the_job_entry_and_the_python_layer():
    """Every refusal of ramp_sample_guided is a host check made before anything launches: non-zero, the entry's name in ramp_last_error, the
    launch counter untouched, the output as it was.  cost_guide= on the dynamic planner and with a caller's sample_fn raises."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = small_model()
    B, H, S, steps = 2, 8, 4, [24, 12, 0]
    dm.model.prepare_time_table(25)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    dm._prepare_scene(scene, B)
    arrays = _HostArrays()
    noise = dev(synth.make_noise((4, B, H, S), seed=8))
    p = raw_params(dm, B, steps, arrays, False)
    ctx, s = dm.model.ctx(), _lib.current_stream()
    out = torch.full((B, H, S), 7.0, device="cuda")
    gcloud = dev(uniform((50, 2), 91))
    ts = dev(np.zeros(B, np.int32))

    def refused(cg, batch=None):
        n0 = dm.model.launch_count()
        rc = lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg), None, None, C.byref(batch) if batch is not None else None, _lib.ptr(noise),
                                    None, None, None, _lib.ptr(out), None, s)
        msg = lib.ramp_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "ramp_sample_guided" in msg, (rc, msg)
        assert dm.model.launch_count() == n0 and float(out.min()) == 7.0 and float(out.max()) == 7.0
        return msg

    def guide(**kw):
        cg = raw_guide(arrays, [kw.pop("cloud", gcloud)], kw.pop("n_guide", [1, 1, 1]), kw.pop("step", [0.01] * 3))
        for k, v in kw.items():
            setattr(cg, k, v)
        return cg

    assert "point_dim" in refused(guide(point_dim=1))
    assert "point_dim" in refused(guide(point_dim=4))
    assert "n_guide" in refused(guide(n_guide=[1, 17, 1]))
    assert "n_guide" in refused(guide(n_guide=[1, -1, 1]))
    for bad in (float("nan"), float("inf")):
        assert "step" in refused(guide(step=[0.01, bad, 0.01]))
        for k in ("radius", "w_obs", "w_smooth", "w_acc", "max_norm"):
            assert "finite" in refused(guide(**{k: bad}))
    assert "radius" in refused(guide(radius=0.0))
    assert "radius" in refused(guide(radius=-0.1))
    bad_off = (C.c_int32 * 2)(1, 50)
    assert "offsets" in refused(guide(cloud_offset_host=C.cast(bad_off, _lib.c_i32p)))
    two = raw_guide(arrays, [gcloud, gcloud], [1] * 3, [0.01] * 3)
    assert "n_scenes" in refused(two)
    dec = (C.c_int32 * 3)(0, 50, 20)
    two.cloud_offset_host = C.cast(dec, _lib.c_i32p)
    batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(ts)
    assert "non-decreasing" in refused(two, batch)
    batch3 = _lib.RampSceneBatch(); batch3.n_scenes, batch3.traj_scene = 3, _lib.ptr(ts)
    assert "n_scenes" in refused(raw_guide(arrays, [gcloud, gcloud], [1] * 3, [0.01] * 3), batch3)
    assert "cloud_points" in refused(guide(cloud_points=None))
    # radius <= 0 is fine without an obstacle term, an empty cloud is fine, and an unused step is still checked for finiteness only
    ok = guide(radius=0.0, w_obs=0.0, w_smooth=0.5, cloud=dev(np.zeros((0, 2), np.float32)))
    _lib.check(lib.ramp_sample_guided(ctx, C.byref(p), C.byref(ok), None, None, None, _lib.ptr(noise), None, None, None, _lib.ptr(out), None, s),
               "ramp_sample_guided")
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all() and float(out.max()) != 7.0
    # (point_dim > state_dim: test_guide_host.py, through ramp_guide_step on 2-wide states)
    # the wrapper refuses a cloud list of the wrong length
    g = dict(cloud=gcloud, radius=RADIUS, step=0.01)
    with pytest.raises(ValueError, match="entries for 1 scene"):
        dm.run_inference(None, hct(S), n_samples=1, obstacle_pts=scene, cost_guide=dict(clouds=[gcloud, gcloud], radius=RADIUS, step=0.01))
    from ramp_amd.models import DynamicGaussianDiffusionModel
    dyn = DynamicGaussianDiffusionModel(model=dm.model, n_diffusion_steps=25, predict_epsilon=True)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dyn.conditional_sample({}, cost_guide=g)

    def my_step(*a, **k):
        raise AssertionError("never called")
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            small_model(sampler=sampler).run_inference(None, hct(S), n_samples=1, obstacle_pts=scene, sample_fn=my_step, cost_guide=g)
