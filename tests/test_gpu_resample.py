"""Resampling trajectories by cost inside the sampling job (SMC steering): the kernels alone (``ramp_resample_groups``), the ESS gate, "off is
off", the wiring into ``ramp_sample_steered``, free-running steered chains against float64, the Philox uniforms, stale graphs and the refusals.

The truth is the float64 numpy restatement of the definition in include/ramp_hip.h written below (``resample_group`` / ``resample_event`` /
``replay_events``; ``SteeredOracle`` inserts it into the sampler oracle's loops at the places the header gives).  Ancestors are integers: they
are compared exactly, and only where the restatement itself is decided -- no threshold (i + u) / n closer to a prefix sum than the fp64 sums
can differ by their order (``64 n 2^-53``; in the free-running chains 4 x the shift the float32 restatement shows).  The inputs are chosen so
that this leaves nothing out, and that is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_guide as G
import test_gpu_mcmc as M
from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.diffusion import mcmc_tables, resample_tables
from ramp_amd.spec import UNET_DIM_MULTS
from util import NoiseInjector, dev, philox_normal

pytestmark = pytest.mark.gpu

F32 = G.F32
RADIUS = G.RADIUS
NINF = -np.inf


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def resample_group(logw, u, ess_frac):
    """Steps 3 and 4 for one group: (ancestors within the group, ESS, resampled?, margin, cum).  margin = the smallest distance of a threshold
    (i + u) / n from a prefix sum cum_0 .. cum_{n-2} (cum_{n-1} = 1 decides nothing: the count is capped at n - 1); inf where nothing resampled."""
    n = len(logw)
    lw = np.where(np.isfinite(logw), logw, NINF).astype(np.float64)
    ident = np.arange(n)
    if not lw.max() > NINF:
        return ident, 0.0, False, np.inf, None
    w = np.exp(lw - lw.max())
    W = w / w.sum()
    ess = 1.0 / float((W * W).sum())
    if not ess < ess_frac * n:
        return ident, ess, False, np.inf, None
    cum = np.cumsum(W)
    cum[-1] = 1.0
    thr = (np.arange(n, dtype=np.float64) + float(u)) / float(n)
    anc = np.minimum(n - 1, np.searchsorted(cum, thr, side="right"))
    margin = np.inf
    if n > 1:
        c = np.sort(cum[:-1])
        k = np.clip(np.searchsorted(c, thr), 1, len(c) - 1) if len(c) > 1 else np.zeros(n, int)
        margin = float(np.minimum(np.abs(c[k] - thr), np.abs(c[np.maximum(k - 1, 0)] - thr)).min())
    return anc, ess, True, margin, cum


def resample_event(x, logw, c_prev, gf, u, ess_frac):
    """Steps 3 and 4 over all groups on copies: (x, logw, c_prev, ancestors within the batch, ess (G,), smallest margin)."""
    x, logw = x.copy(), np.array(logw, np.float64)
    c_prev = None if c_prev is None else np.array(c_prev, np.float64)
    anc, ess, margin = np.arange(len(logw)), np.zeros(len(gf) - 1), np.inf
    for g, (a, b) in enumerate(zip(gf[:-1], gf[1:])):
        ag, ess[g], did, mg, _ = resample_group(logw[a:b], u[g], ess_frac)
        margin = min(margin, mg / (b - a))      # (relative to the group's size: the bar is 64 n 2^-53)
        anc[a:b] = a + ag
        if did:
            logw[a:b] = 0.0
    return x[anc], logw, (None if c_prev is None else c_prev[anc]), anc.astype(np.int32), ess, margin


def update_logw(logw, c_prev, c, lam):
    """Step 2: (logw, c_prev) after the event's costs c."""
    with np.errstate(invalid="ignore", over="ignore"):
        lw = logw + (-lam) * (c - c_prev)
    return np.where(np.isfinite(lw), lw, NINF), np.array(c, np.float64)


def replay_events(cost, gf, lam, u, ess_frac):
    """The events of a job from its own costs (n_events, B): (ancestors (n_events, B), ess (n_events, G), final logw, smallest margin)."""
    E, B = cost.shape
    logw, c_prev = np.zeros(B), np.zeros(B)
    ancs, esss, margin = [], [], np.inf
    for k in range(E):
        logw, c_prev = update_logw(logw, c_prev, cost[k], lam[k])
        _, logw, c_prev, a, e, mg = resample_event(np.zeros((B, 1)), logw, c_prev, gf, u[k], ess_frac)
        ancs.append(a); esss.append(e); margin = min(margin, mg)
    return np.array(ancs), np.array(esss), logw, margin


def weighted_cost(v, cloud, r, w):
    """c_b of trajectories v (B, H, S) against one cloud (P, d): the three terms in v's precision (sums fp64), the weighted sum in fp64."""
    d = cloud.shape[-1]
    t = np.array([G.guide_terms(v[b, :, :d], cloud.astype(v.dtype), r) for b in range(v.shape[0])])
    return w[0] * t[:, 0] + w[1] * t[:, 1] + w[2] * t[:, 2]


class SteeredOracle(M.McmcOracle):
    """The sampler oracle (with optional ULA inner steps) and the resampling events of ONE group: ``steer`` = dict(cloud (P, d), tab =
    resample_tables(...) of the job, u (n_events,)).  ``log`` receives per event (ancestors, ess, resampled?, margin, cum, logw)."""

    def __init__(self, *a, steer=None, **k):
        super().__init__(*a, **k)
        self.steer = steer

    def run(self, kind, noise, hard_conds, latent, mcmc=None, z=None, K_ddim=5, noise_scale=0.5, log=None):
        s, dt, st = self.sched, self.dt, self.steer
        ts = list(reversed(range(self.T))) if kind == "ddpm" else [int(t) for t in O.ddim_timesteps(self.T, K_ddim)]
        mt = mcmc_tables(mcmc, ts, s["alphas_cumprod"]) if mcmc is not None else None
        x = O.apply_hard_conditioning(noise[0].astype(dt).copy(), hard_conds)
        B = x.shape[0]
        logw, c_prev, ke, kk = np.zeros(B), np.zeros(B), 0, 0
        chain, ac = [x.copy()], s["alphas_cumprod"]
        w = None if st is None else (st["tab"]["w_obs"], st["tab"]["w_smooth"], st["tab"]["w_acc"])
        for j, t in enumerate(ts):
            e, E, _ = self.eps_energy(x, t, latent)
            if mt is not None and mt["n_inner"][j]:
                K = mt["n_inner"][j]
                x, e, E, _ = self.inner_steps(x, e, E, t, latent, "ula", K, np.float32(mt["step_size"][j]), np.float32(mt["sigma"][j]),
                                              z[kk:kk + K], None, hard_conds.keys())
                kk += K
            x0, mean = self.x0_mean(x, e, t)
            event = st is not None and st["tab"]["resample"][j]
            if event:
                c = weighted_cost(mean if kind == "ddpm" else x0, st["cloud"], st["tab"]["radius"], w)
                logw, c_prev = update_logw(logw, c_prev, c, st["tab"]["lambda"][j])
            if kind == "ddpm":
                zz = noise[1 + j].astype(dt) if t != 0 else np.zeros_like(x)
                std = np.exp(dt(0.5) * s["posterior_log_variance_clipped"][t])
                x = O.apply_hard_conditioning((mean + std * zz * dt(noise_scale)).astype(dt), hard_conds)
            else:
                prev = t - self.T // K_ddim
                a_t, a_prev = ac[t], (ac[prev] if prev >= 0 else dt(1.0))
                e2 = (x - np.sqrt(a_t) * x0) / np.sqrt(dt(1) - a_t)
                x = O.apply_hard_conditioning((np.sqrt(a_prev) * x0 + np.sqrt(dt(1) - a_prev) * e2).astype(dt), hard_conds)
            if event:
                lw_in = logw.copy()
                anc, ess, did, margin, cum = resample_group(logw, st["u"][ke], st["tab"]["ess_frac"])
                if did:
                    x, c_prev, logw = x[anc], c_prev[anc], np.zeros(B)
                if log is not None:
                    log.append(dict(anc=anc, ess=ess, did=did, margin=margin, cum=cum, logw=lw_in, cost=c))
                ke += 1
            chain.append(x.copy())
        return np.stack(chain)


def uniform(shape, seed):
    return G.uniform(shape, seed)


def u01(shape, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.98, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: the kernels alone
KERNEL_CASES = {"ragged": ([1, 2, 3, 64, 257, 1025], 11), "one4096": ([4096], 12)}
_KERNEL = {}


def kernel_case(name):
    """Inputs and the restatement's answer of one kernel case, once per process: x (B, 8, 4) uniform, log-weights N(0, 2^2), c_prev uniform."""
    if name not in _KERNEL:
        sizes, seed = KERNEL_CASES[name]
        gf = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        B = int(gf[-1])
        rng = np.random.default_rng(seed)
        x, logw, cp, u = uniform((B, 8, 4), seed), rng.normal(0.0, 2.0, B), rng.uniform(0.0, 3.0, B), u01((len(sizes),), seed + 1)
        want = resample_event(x, logw, cp, gf, u, 2.0)
        _KERNEL[name] = dict(gf=gf, B=B, x=x, logw=logw, cp=cp, u=u, want=want)
    return _KERNEL[name]


def kernel_precondition(name):
    """no threshold closer than 64 n 2^-53 to a prefix sum (the margin is kept relative to n): (margin / n, bar / n)."""
    return kernel_case(name)["want"][5], 64 * 2.0 ** -53


def run_kernel(x, logw, gf, u, ess_frac, cp=None):
    from ramp_amd.resample import systematic_resample
    out = systematic_resample(dev(x), torch.from_numpy(np.asarray(logw, np.float64)), gf, dev(u), ess_frac,
                              c_prev=None if cp is None else torch.from_numpy(np.asarray(cp, np.float64)))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_alone_against_the_restatement(name):
    """One call with groups of 1, 2, 3, 64, 257 and 1025 trajectories (less than a wave, a wave, a block plus one, four chunks plus one) and one
    call with a single group of 4096 (16 chunks), H S = 8 x 4, ess_frac 2 (every group resamples): the ancestors are exactly the float64
    restatement's, x is bit-equal to x[ancestors], c_prev is permuted alike, logw is reset, ESS agrees to 1e-12 relative.  Precondition,
    asserted on the restatement alone: no threshold lies closer than 64 n 2^-53 to a prefix sum."""
    c = kernel_case(name)
    margin, bar = kernel_precondition(name)
    print(f"resample kernel {name}: smallest margin / n {margin:.2e} (bar {bar:.2e})")
    assert margin > bar
    xw, lww, cpw, ancw, essw, _ = c["want"]
    x, lw, anc, ess, cp = run_kernel(c["x"], c["logw"], c["gf"], c["u"], 2.0, c["cp"])
    assert anc.dtype == np.int32 and np.array_equal(anc, ancw)
    assert (ancw != np.arange(c["B"])).mean() > 0.3 or name == "ragged"        # (it did resample)
    assert np.array_equal(x.view(np.uint32), c["x"][ancw].view(np.uint32))
    assert np.array_equal(cp, c["cp"][ancw]) and np.array_equal(lw, np.zeros(c["B"]))
    print(f"  ESS {ess[-1]:.6f} of {np.diff(c['gf'])[-1]}; relative ESS error {np.abs(ess / essw - 1).max():.2e}")
    assert np.abs(ess / essw - 1).max() <= 1e-12
    # without c_prev the same ancestors
    x2, _, anc2, _ = run_kernel(c["x"], c["logw"], c["gf"], c["u"], 2.0)
    assert np.array_equal(anc2, ancw) and np.array_equal(x2.view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2: the gate
def test_ess_gate_and_weights_of_zero():
    """ess_frac 0 never resamples (x, logw, c_prev keep their bits, ESS is still reported); ess_frac 2 always does; between them the gate follows
    ESS < ess_frac n per group.  A group whose log-weights are all -inf (or NaN: a non-finite log-weight is a weight of 0) is the identity with
    ESS 0; a NaN log-weight inside a live group is never an ancestor."""
    c = kernel_case("ragged")
    x, lw, anc, ess, cp = run_kernel(c["x"], c["logw"], c["gf"], c["u"], 0.0, c["cp"])
    assert np.array_equal(x.view(np.uint32), c["x"].view(np.uint32)) and np.array_equal(lw, c["logw"]) and np.array_equal(cp, c["cp"])
    assert np.array_equal(anc, np.arange(c["B"])) and np.abs(ess / c["want"][4] - 1).max() <= 1e-12
    # a threshold between the groups' ESS / n: some groups resample, some do not
    frac = c["want"][4] / np.diff(c["gf"])
    mid = float(np.sort(frac)[3] + np.sort(frac)[2]) / 2
    xw, lww, cpw, ancw, essw, _ = resample_event(c["x"], c["logw"], c["cp"], c["gf"], c["u"], mid)
    x, lw, anc, ess, cp = run_kernel(c["x"], c["logw"], c["gf"], c["u"], mid, c["cp"])
    did = [bool((lww[a:b] == 0).all()) for a, b in zip(c["gf"][:-1], c["gf"][1:])]
    assert 0 < sum(did) < len(did), did
    assert np.array_equal(anc, ancw) and np.array_equal(lw, lww) and np.array_equal(cp, cpw) and np.array_equal(x.view(np.uint32), xw.view(np.uint32))
    # weights of zero
    gf = np.array([0, 7, 12, 80], np.int32)
    logw = np.random.default_rng(5).normal(0, 2, 80)
    logw[0:7] = NINF
    logw[7:12] = [NINF, np.nan, NINF, np.nan, np.nan]
    logw[[20, 33, 34]] = [np.nan, NINF, np.inf]
    xx, u = uniform((80, 8, 4), 6), u01((3,), 7)
    xw, lww, _, ancw, essw, margin = resample_event(xx, logw, None, gf, u, 2.0)
    assert margin > 64 * 2.0 ** -53
    x, lw, anc, ess = run_kernel(xx, logw, gf, u, 2.0)
    assert ess[0] == 0.0 and ess[1] == 0.0 and abs(ess[2] / essw[2] - 1) <= 1e-12
    assert np.array_equal(anc[:12], np.arange(12)) and np.array_equal(x[:12].view(np.uint32), xx[:12].view(np.uint32))
    assert np.array_equal(lw[:12].view(np.uint64), logw[:12].view(np.uint64))      # nothing changes there
    assert np.array_equal(anc, ancw) and not set(anc[12:]) & {20, 33, 34} and np.array_equal(lw[12:], np.zeros(68))
    assert np.array_equal(x.view(np.uint32), xx[ancw].view(np.uint32))


# ------------------------------------------------------------------------------------------------ jobs through the raw ABI
STEPS = [24, 12, 1, 0]
W3 = (1.0, 0.5, 0.25)


def raw_cost(arrays, clouds, w=W3, radius=RADIUS):
    from ramp_amd.guide import cloud_table, fill_cost_guide
    pts, off, d = cloud_table(clouds, "cuda")
    return arrays.keep(fill_cost_guide(arrays.keep(pts), arrays.keep(off), d, dict(radius=radius, w_obs=w[0], w_smooth=w[1], w_acc=w[2])))


def raw_rs(arrays, gf, flags, lam, ess_frac, cost):
    rs = _lib.RampResampleParams()
    g = arrays.keep(np.ascontiguousarray(gf, dtype=np.int32))
    rs.n_groups, rs.group_first_host = len(g) - 1, g.ctypes.data_as(_lib.c_i32p)
    rs.resample = arrays.i32(flags) if flags is not None else None
    if lam is not None:
        rs.lambda_ = arrays.keep(np.ascontiguousarray(lam, dtype=np.float64)).ctypes.data_as(_lib.c_f64p)
    rs.ess_frac = ess_frac
    rs.cost = C.pointer(cost) if cost is not None else None
    return rs


class Job:
    """A small DDPM job (the smallest network, H = 8, S = 4, iterations t = 24, 12, 1, 0) of one of four kinds, through the raw ABI."""

    def __init__(self, kind="plain", use_graph=1, hard=True):
        from ramp_amd.diffusion import _HostArrays
        self.lib, self.kind = _lib.load(), kind
        self.dm = dm = G.small_model()
        self.arrays = arrays = _HostArrays()
        S, H = 4, 8
        dm.model.prepare_time_table(25)
        self.rows = self.batch = self.mp = self.z = self.mu = None
        self.counts = [6]
        hc = {k: v.cuda().unsqueeze(0).expand(6, -1).contiguous() for k, v in G.hct(S).items()} if hard else None
        if kind in ("scenes", "composed"):
            self.counts = [2, 4]
            if kind == "scenes":
                sj, hcc, B = dm._prepare_scene_job([dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))],
                                                   [G.hct(S)] * 2, self.counts)
            else:
                sc = [[dev(synth.make_cloud(5, 64, 2, seed=31))], [dev(synth.make_cloud(4, 64, 2, seed=32 + k)) for k in range(2)]]
                sj, guid, hcc, B = dm._prepare_composed_job(sc, [G.hct(S)] * 2, self.counts, None, None)
            hc = hcc if hard else None
            self.sj = sj
            self.batch = _lib.RampSceneBatch(); self.batch.n_scenes, self.batch.traj_scene = 2, _lib.ptr(sj["traj_scene"])
        else:
            dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), 6)
        self.B, self.H, self.S = 6, H, S
        self.gf = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.p = G.raw_params(dm, 6, STEPS, arrays, False, hard=hc, use_graph=use_graph)
        if kind == "composed":
            self.p.n_rp, self.p.w0, self.p.w1 = guid["n_rp"], 0.0, 0.0
            self.guid = guid
            self.rows = _lib.RampGuidanceRows(); self.rows.n_rp, self.rows.row_weight = guid["n_rp"], _lib.ptr(guid["row_weight"])
        if kind == "mala":
            self.mp = _lib.RampMcmcParams(); self.mp.kind = 2
            sig = [float(dm.sqrt_one_minus_alphas_cumprod[t]) for t in STEPS]
            self.mp.n_inner, self.mp.step_size, self.mp.sigma = arrays.i32([1, 0, 1, 0]), arrays.f32([1e-3 * s * s for s in sig]), arrays.f32(sig)
            self.z, self.mu = dev(synth.make_noise((2, 6, H, S), seed=94)), dev(u01((2, 6), 95))
        self.noise = dev(synth.make_noise((5, 6, H, S), seed=90))
        self.clouds = [dev(uniform((300, 2), 91))] if self.batch is None else [dev(uniform((70, 2), 92)), dev(uniform((400, 2), 93))]
        self.ctx, self.s = dm.model.ctx(), _lib.current_stream()

    def guided(self, cg=None):
        chain = torch.empty((5, self.B, self.H, self.S), device="cuda")
        _lib.check(self.lib.ramp_sample_guided(self.ctx, C.byref(self.p), C.byref(cg) if cg is not None else None,
                                               C.byref(self.mp) if self.mp is not None else None, C.byref(self.rows) if self.rows is not None else None,
                                               C.byref(self.batch) if self.batch is not None else None, _lib.ptr(self.noise), _lib.ptr(self.z),
                                               _lib.ptr(self.mu), _lib.ptr(chain), None, None, self.s), "ramp_sample_guided")
        torch.cuda.synchronize()
        return chain

    def steered_rc(self, rs, ru=None, n_events=0, noise="own", out=None):
        E, B, Gn = max(n_events, 1), self.B, len(self.gf) - 1
        r = dict(chain=torch.empty((5, B, self.H, self.S), device="cuda"), x=torch.empty((B, self.H, self.S), device="cuda") if out is None else out,
                 anc=torch.full((E, B), -1, device="cuda", dtype=torch.int32), ess=torch.full((E, Gn), -1.0, device="cuda", dtype=torch.float64),
                 cost=torch.full((E, B), -1.0, device="cuda", dtype=torch.float64), logw=torch.full((B,), -1.0, device="cuda", dtype=torch.float64))
        rc = self.lib.ramp_sample_steered(self.ctx, C.byref(self.p), C.byref(rs) if rs is not None else None, None,
                                          C.byref(self.mp) if self.mp is not None else None, C.byref(self.rows) if self.rows is not None else None,
                                          C.byref(self.batch) if self.batch is not None else None,
                                          _lib.ptr(self.noise) if isinstance(noise, str) else noise, _lib.ptr(self.z), _lib.ptr(self.mu), _lib.ptr(ru),
                                          _lib.ptr(r["chain"]), _lib.ptr(r["x"]), None, _lib.ptr(r["anc"]), _lib.ptr(r["ess"]), _lib.ptr(r["cost"]),
                                          _lib.ptr(r["logw"]), self.s)
        torch.cuda.synchronize()
        return rc, r

    def steered(self, rs, ru=None, n_events=0):
        rc, r = self.steered_rc(rs, ru, n_events)
        _lib.check(rc, "ramp_sample_steered")
        return r


# ------------------------------------------------------------------------------------------------ 3: off is off
@pytest.mark.parametrize("kind", ["plain", "scenes", "composed", "mala"])
def test_off_is_off_bit_for_bit(kind):
    """rs == NULL and a table with no flag set give ramp_sample_guided's chain bit for bit, as a plain job, a 2-scene job, a composed job and
    with MALA inner steps; and on is on: with flags set and ess_frac 2 the chain differs from the first event on."""
    job = Job(kind)
    base = job.guided()
    assert np.isfinite(base.cpu().numpy()).all()
    cost = raw_cost(job.arrays, job.clouds)
    assert torch.equal(job.steered(None)["chain"], base)
    assert torch.equal(job.steered(raw_rs(job.arrays, job.gf, [0] * 4, [1.0] * 4, 2.0, cost))["chain"], base)
    assert torch.equal(job.steered(raw_rs(job.arrays, job.gf, None, None, 2.0, None))["chain"], base)
    on = job.steered(raw_rs(job.arrays, job.gf, [0, 1, 1, 0], [50.0] * 4, 2.0, cost), dev(u01((2, len(job.gf) - 1), 3)), 2)
    assert torch.equal(on["chain"][:2], base[:2]) and not torch.equal(on["chain"][2], base[2])
    assert torch.equal(job.guided(), base)      # (and the plain job after a steered one is still the plain job)


# ------------------------------------------------------------------------------------------------ 4: wiring
def test_wiring_costs_and_log_weights():
    """A DDPM job without hard conditions, events on iterations 1 and 3 (the last: t = 0, so x_out is the posterior mean the cost saw),
    ess_frac 0: chain and x_out are bit-equal to the job without resampling; cost_out of the last event equals the weighted ramp_guide_cost of
    x_out bit for bit; logw_out equals -lambda_1 c_1 - lambda_3 (c_3 - c_1) to 1e-12; the ancestors are the identity and ESS is what the
    restatement gives for those log-weights.  Then lambda = 1e308 with ess_frac 2: every log-weight overflows to -inf at the first event and
    (inf - inf) is NaN at the second -- both count as -inf: ESS 0, identity, the chain of the job without resampling, no NaN in logw_out."""
    from ramp_amd.guide import cost_guide_terms
    job = Job("plain", hard=False)
    base = job.guided()
    cost = raw_cost(job.arrays, job.clouds)
    lam = [0.0, 3.0, 0.0, 7.0]
    r = job.steered(raw_rs(job.arrays, job.gf, [0, 1, 0, 1], lam, 0.0, cost), dev(u01((2, 1), 3)), 2)
    assert torch.equal(r["chain"], base) and torch.equal(r["x"], base[-1])
    t = cost_guide_terms(r["x"], job.clouds, RADIUS).cpu().numpy()
    c = r["cost"].cpu().numpy()
    want = W3[0] * t[:, 0] + W3[1] * t[:, 1] + W3[2] * t[:, 2]
    assert (want > 0).all() and np.array_equal(c[1].view(np.uint64), want.view(np.uint64))
    lw = -3.0 * c[0] + -7.0 * (c[1] - c[0])
    got = r["logw"].cpu().numpy()
    print(f"wiring: costs {c[1].round(4).tolist()}, logw error {np.abs(got - lw).max():.2e}")
    assert np.abs(got - lw).max() <= 1e-12 * np.abs(lw).max()
    ancw, essw, lww, _ = replay_events(c, job.gf, [3.0, 7.0], np.full((2, 1), 0.5), 0.0)
    assert np.array_equal(r["anc"].cpu().numpy(), ancw) and np.abs(r["ess"].cpu().numpy() / essw - 1).max() <= 1e-12
    # non-finite log-weights count as -inf
    big = raw_cost(job.arrays, job.clouds, w=(1000.0, 500.0, 250.0))
    r = job.steered(raw_rs(job.arrays, job.gf, [0, 1, 0, 1], [1e308] * 4, 2.0, big), dev(u01((2, 1), 3)), 2)
    cb = r["cost"].cpu().numpy()
    assert (cb[0] > 2.0).all() and len(set(np.sign(cb[1] - cb[0]))) == 2      # (1e308 c overflows; some costs rose, some fell: -inf + inf occurs)
    assert torch.equal(r["chain"], base)
    assert (r["ess"].cpu().numpy() == 0).all() and np.array_equal(r["anc"].cpu().numpy(), np.tile(np.arange(6), (2, 1)))
    assert (r["logw"].cpu().numpy() == NINF).all()


# ------------------------------------------------------------------------------------------------ 5: free-running steered chains against float64
CHAIN_SIZES = [5, 11]
CHAIN_STEER = {"ddpm": dict(flags=[0, 1, 1, 0], lambda_=40.0, ess_frac=2.0, radius=RADIUS, w_obs=1.0, w_smooth=0.5, w_acc=0.25),
               "ddim": dict(flags=[0, 1, 0, 1, 0], lambda_=40.0, ess_frac=0.95, radius=RADIUS, w_obs=1.0, w_smooth=0.5, w_acc=0.25)}
CHAIN_MCMC = dict(kind="ula", steps=1, step_scale=0.02)
CHAIN_SEED = {"ddpm": 700, "ddim": 710}
_CHAIN = {}


def chain_inputs(kind):
    T = 4 if kind == "ddpm" else 25
    seed = CHAIN_SEED[kind]
    n = (T + 1) if kind == "ddpm" else 1
    return dict(T=T, noise=synth.make_noise((n, 16, 8, 4), seed=seed), z=synth.make_noise((5, 16, 8, 4), seed=seed + 1),
                clouds=[uniform((200, 2), seed + 2), uniform((300, 2), seed + 3)], u=u01((2, 2), seed + 4),
                scenes=[synth.make_cloud(6, 64, 2, seed=3), synth.make_cloud(5, 64, 2, seed=31)])


def oracle_chains(kind):
    """float64 and float32 steered chains and the float64 chain without events, per scene (a group never sees another), once per process."""
    if kind not in _CHAIN:
        from test_gpu_shapes import shape_weights
        ci = chain_inputs(kind)
        sched, steps, _ = G.chain_sched(ci["T"], kind)
        tab = resample_tables(dict(CHAIN_STEER[kind], cloud=None), steps)
        out = dict(tab=tab, steps=steps)
        for name, dtype, steer in (("s64", np.float64, True), ("s32", np.float32, True), ("u64", np.float64, False)):
            uo = O.UNetOracle(shape_weights(4, 8, False, 0, 16), 4, 8, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            chains, logs = [], []
            for g, (a, b) in enumerate(zip([0, 5], [5, 16])):
                so = SteeredOracle(uo, ci["T"], 2.0, dtype=dtype, sched=sched,
                                   steer=dict(cloud=ci["clouds"][g], tab=tab, u=ci["u"][:, g]) if steer else None)
                log = []
                chains.append(so.run(kind, ci["noise"][:, a:b], G.hcn(4), uo.encode_scene(ci["scenes"][g]),
                                     mcmc=CHAIN_MCMC if kind == "ddim" else None, z=ci["z"][:, a:b], log=log))
                logs.append(log)
            out[name], out[name + "_log"] = np.concatenate(chains, axis=1), logs
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """What the inputs must satisfy, on the oracle alone.  Per (group, event): the float32 restatement takes the float64 one's decisions; the
    gate is decided (|ESS - ess_frac n| > 4 x the float32 shift of ESS) and so is every ancestor (margin > 4 x the float32 shift of the prefix
    sums).  Returns (events left out, events, resampling events, bar of the chain = 4 x float32 distance, steered-vs-unsteered distance)."""
    c = oracle_chains(kind)
    left_out, events, resampled = 0, 0, 0
    for g, n in enumerate(CHAIN_SIZES):
        for e64, e32 in zip(c["s64_log"][g], c["s32_log"][g]):
            events += 1
            resampled += e64["did"]
            ok = e64["did"] == e32["did"] and np.array_equal(e64["anc"], e32["anc"])
            ok = ok and abs(e64["ess"] - c["tab"]["ess_frac"] * n) > 4 * abs(e32["ess"] - e64["ess"])
            if ok and e64["did"]:
                ok = e64["margin"] > 4 * float(np.abs(e32["cum"] - e64["cum"]).max())
            left_out += not ok
    return left_out, events, resampled, 4 * float(np.abs(c["s32"] - c["s64"]).max()), float(np.abs(c["s64"][-1] - c["u64"][-1]).max())


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_steered_chain(kind):
    """Two scenes with groups of 5 and 11 in one job at the smallest network (H = 8, S = 4) through run_inference_scenes(resample=): a 4-step
    DDPM job (cosine schedule) with events on iterations 1 and 2, always resampling, and the 5-step DDIM job (T = 25) with one ULA step per
    iteration and events on iterations 1 and 3 behind an ESS gate of 0.95.  Every ancestor of every event equals the float64 oracle's -- the
    inputs leave no event out (asserted and printed: the float32 oracle decides alike and every margin exceeds 4 x its shift) -- and every
    state of the chain lies within 4 x the float32 oracle's own distance from the float64 one; every ESS within 4 x the float32 oracle's
    largest relative ESS distance over the chain's events (measured on the MI355X: DDPM chain 2.8e-4 against a bar of 1.1e-3; DDIM + ULA
    ESS 1.2e-5 relative against 5.8e-5)."""
    left_out, events, resampled, bar, moved = chain_conditions(kind)
    print(f"steered {kind}: {events} (group, event) pairs, {resampled} resample, {left_out} left out; chain bar {bar:.2e}; steered vs unsteered {moved:.2e}")
    assert left_out == 0 and resampled >= 2 and moved > 100 * bar
    c, ci = oracle_chains(kind), chain_inputs(kind)
    dm = G.small_model(T=ci["T"], sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential")
    kw = dict(resample=dict(CHAIN_STEER[kind], clouds=[dev(cl) for cl in ci["clouds"]], u=dev(ci["u"])))
    if kind == "ddim":
        kw["mcmc"] = dict(CHAIN_MCMC, noise=dev(ci["z"]))
    with NoiseInjector(list(ci["noise"])):
        chain, ts = dm.run_inference_scenes([dev(s) for s in ci["scenes"]], [G.hct(4)] * 2, n_samples=CHAIN_SIZES, return_chain=True,
                                            noise_std_extra_schedule_fn=lambda x: 0.5, **kw)
    chain = chain.cpu().numpy()
    lr = dm.last_resample
    assert lr["group_first"].tolist() == [0, 5, 16] and lr["events"] == [j for j, f in enumerate(c["tab"]["resample"]) if f]
    anc = lr["ancestors"].numpy()
    # the ESS bar: 4 x the float32 oracle's largest relative distance from the float64 one over the events of this chain (the aggregate the
    # chain's own bar uses; one event's own shift is a single sample and can be arbitrarily small)
    ess_bar = 4 * max(abs(e32["ess"] / e["ess"] - 1) for g in range(2) for e, e32 in zip(c["s64_log"][g], c["s32_log"][g]))
    for g, (a, b) in enumerate(zip([0, 5], [5, 16])):
        for k, (e, e32) in enumerate(zip(c["s64_log"][g], c["s32_log"][g])):
            assert np.array_equal(anc[k, a:b], a + e["anc"]), (g, k, anc[k, a:b], a + e["anc"])
            print(f"  group {g} event {k}: ESS {float(lr['ess'][k, g]):.6f}, float64 {e['ess']:.6f}, float32 {e32['ess']:.6f}; margin {e['margin']:.2e}")
            assert abs(float(lr["ess"][k, g]) / e["ess"] - 1) <= ess_bar, (g, k, ess_bar)
    err = float(np.abs(chain - c["s64"]).max())
    print(f"steered {kind} chain vs float64: {err:.2e} (bar {bar:.2e}); mode {dm.last_job_mode}")
    assert chain.shape == c["s64"].shape and err <= bar


# ------------------------------------------------------------------------------------------------ 6: Philox
def philox_u(seed, offset, n_steps, K, B, HS, n_events, n_groups):
    """The uniforms of (event k, group g) of a whole job: ((r >> 9) + 0.5) 2^-23, r = output 0 of group (n_steps + 1 + K) B HS / 4 + K B + k G + g."""
    g0 = (n_steps + 1 + K) * B * HS // 4 + K * B
    r = philox_normal(seed, offset + g0, 4 * n_events * n_groups)[1].reshape(-1, 4)[:, 0]
    return (((r >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)).reshape(n_events, n_groups)


def test_philox_uniforms_replicate_on_the_host():
    """noise_source='philox', two scenes (5 and 11), 25 DDPM steps with an event every 5: with u replicated on the host from (seed, offset) the
    restatement -- fed the job's own costs -- gives the job's ancestors, ESS and final log-weights, with and without MALA inner steps (the K T
    groups of MALA's uniforms are reserved either way).  The next job of the same model (a later offset) draws other uniforms."""
    scenes = [dev(synth.make_cloud(6, 64, 2, seed=3)), dev(synth.make_cloud(5, 64, 2, seed=31))]
    clouds = [dev(uniform((200, 2), 702)), dev(uniform((300, 2), 703))]
    rs = dict(every=5, lambda_=40.0, ess_frac=2.0, clouds=clouds, radius=RADIUS, w_smooth=0.5, w_acc=0.25)
    for mc in (None, dict(kind="mala", steps=[1 if j % 6 == 0 else 0 for j in range(25)], step_scale=0.02)):
        dm = G.small_model(noise_source="philox", noise_seed=77)
        seen = []
        for _ in range(2):
            dm.run_inference_scenes(scenes, [G.hct(4)] * 2, n_samples=CHAIN_SIZES, noise_std_extra_schedule_fn=lambda x: 0.5, resample=rs,
                                    **({} if mc is None else dict(mcmc=mc)))
            lr = dm.last_resample
            seed, offset, _ = dm.last_philox
            K = 0 if mc is None else sum(mc["steps"])
            u = philox_u(seed, offset, 25, K, 16, 32, 5, 2)
            assert ((u > 0) & (u < 1)).all()
            cost = lr["cost"].numpy()
            ancw, essw, lww, margin = replay_events(cost, lr["group_first"], [40.0] * 5, u, 2.0)
            print(f"philox (K = {K}, offset {offset}): u[0] {u[0].tolist()}, margin / n {margin:.2e}")
            assert margin > 64 * 2.0 ** -53
            assert np.array_equal(lr["ancestors"].numpy(), ancw)
            assert np.abs(lr["ess"].numpy() / essw - 1).max() <= 1e-12 and np.allclose(lr["logw"].numpy(), lww, rtol=0, atol=1e-12 * 40 * np.abs(cost).max())
            seen.append(u)
        assert not np.array_equal(seen[0], seen[1])


# ------------------------------------------------------------------------------------------------ 7: stale graphs
def test_a_steered_job_never_replays_a_stale_graph():
    """Jobs of one shape back to back on one context with use_graph = 1: another lambda, then other group boundaries with the same number of
    groups (11 + 5 instead of 5 + 11), then ess_frac 0 (never) instead of 2 (always) -- each equals its own use_graph = 0 run bit for bit, ancestors included."""
    scenes = [dev(synth.make_cloud(6, 64, 2, seed=3)), dev(synth.make_cloud(5, 64, 2, seed=31))]
    clouds = [dev(uniform((200, 2), 702)), dev(uniform((200, 2), 703))]
    noise = synth.make_noise((26, 16, 8, 4), seed=5)
    base = dict(every=5, lambda_=40.0, ess_frac=2.0, clouds=clouds, radius=RADIUS, w_smooth=0.5, w_acc=0.25, u=dev(u01((5, 2), 9)))
    jobs = [(base, [5, 11]), (dict(base, lambda_=10.0), [5, 11]), (dict(base, lambda_=10.0), [11, 5]), (dict(base, lambda_=10.0, ess_frac=0.0), [11, 5])]

    def run(dm, rs, counts):
        with NoiseInjector(list(noise)):
            chain, _ = dm.run_inference_scenes(scenes, [G.hct(4)] * 2, n_samples=counts, return_chain=True,
                                               noise_std_extra_schedule_fn=lambda x: 0.5, resample=rs)
        return chain, dm.last_resample

    graph, eager = G.small_model(use_graph=True), G.small_model(use_graph=False)
    prev = None
    for rs, counts in jobs:
        (a, la), (b, lb) = run(graph, rs, counts), run(eager, rs, counts)
        assert la["group_first"].tolist() == [0, counts[0], 16]
        assert torch.equal(a, b) and torch.equal(la["ancestors"], lb["ancestors"]) and torch.equal(la["logw"], lb["logw"])
        assert prev is None or not torch.equal(a, prev)
        assert (la["ancestors"].numpy() != np.arange(16)).any() == (rs["ess_frac"] > 0)
        for k in range(5):      # nothing crosses a group
            assert (la["ancestors"][k, :counts[0]] < counts[0]).all() and (la["ancestors"][k, counts[0]:] >= counts[0]).all()
        prev = a
    assert torch.equal(run(graph, *jobs[-1])[0], prev)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_through_the_raw_abi():
    """Every refusal of ramp_sample_steered is a host check made before anything launches: non-zero, the entry's name in ramp_last_error, the
    launch counter untouched, the output as it was."""
    job = Job("plain")
    cost = raw_cost(job.arrays, job.clouds)
    out = torch.full((6, 8, 4), 7.0, device="cuda")
    u = dev(u01((2, 1), 3))

    def refused(rs, ru=u, job=job, out=out):
        n0 = job.dm.model.launch_count()
        rc, _ = job.steered_rc(rs, ru, 2, out=out)
        msg = job.lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_sample_steered" in msg, (rc, msg)
        assert job.dm.model.launch_count() == n0 and float(out.min()) == 7.0 and float(out.max()) == 7.0
        return msg

    def rs(gf=job.gf, flags=(0, 1, 1, 0), lam=(1.0,) * 4, ess=0.5, cost=cost, **kw):
        r = raw_rs(job.arrays, gf, list(flags), list(lam), ess, cost)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    for gf in ([1, 6], [0, 5], [0, 7], [0, 3, 3, 6], [0, 4, 2, 6]):
        assert "group table" in refused(rs(gf=gf)), gf
    assert "group table" in refused(rs(n_groups=0)) and "group table" in refused(rs(group_first_host=None))
    for bad in (-0.1, 2.5, float("nan"), float("inf")):
        assert "ess_frac" in refused(rs(ess=bad))
    for bad in (float("nan"), float("inf")):
        assert "lambda" in refused(rs(lam=(1.0, 1.0, bad, 1.0)))
        assert "lambda" in refused(rs(lam=(bad, 1.0, 1.0, 1.0)))      # (checked on every iteration, flagged or not)
    assert "lambda" in refused(rs(lambda_=None))
    assert "resample_u" in refused(rs(), ru=None)
    assert "cost table" in refused(rs(cost=None))
    bad_cost = raw_cost(job.arrays, job.clouds, radius=0.0)
    assert "radius" in refused(rs(cost=bad_cost))
    bad_cost = raw_cost(job.arrays, job.clouds); bad_cost.point_dim = 4
    assert "point_dim" in refused(rs(cost=bad_cost))
    assert "n_scenes" in refused(rs(cost=raw_cost(job.arrays, job.clouds * 2)))
    assert "groups_total" in refused(rs(group0=1)) and "groups_total" in refused(rs(group0=1, groups_total=1))
    job.p.predict_x0 = 1
    assert "predict_x0" in refused(rs())
    job.p.predict_x0 = 0
    # more than 64 events: a 65-iteration table
    from ramp_amd.diffusion import _HostArrays
    arrays = _HostArrays()
    steps65 = [24 - (j % 25) for j in range(65)]
    p65 = G.raw_params(job.dm, 6, steps65, arrays, False)
    keep, job.p = job.p, p65
    many = raw_rs(arrays, job.gf, [1] * 65, [1.0] * 65, 0.5, cost)
    n0 = job.dm.model.launch_count()
    rc = job.lib.ramp_sample_steered(job.ctx, C.byref(p65), C.byref(many), None, None, None, None, _lib.ptr(dev(np.zeros((66, 6, 8, 4), np.float32))),
                                     None, None, _lib.ptr(dev(u01((65, 1), 4))), None, _lib.ptr(out), None, None, None, None, None, job.s)
    assert rc != 0 and "events" in job.lib.ramp_last_error().decode() and job.dm.model.launch_count() == n0
    job.p = keep
    # DDIM without inner steps; with a ULA table whose counts are all 0; fine with one inner step
    pd = G.raw_params(job.dm, 6, [20, 15, 10, 5, 0], arrays, True)
    job.p = pd
    job.noise = dev(synth.make_noise((1, 6, 8, 4), seed=90))
    r5 = raw_rs(arrays, job.gf, [0, 1, 1, 0, 0], [1.0] * 5, 0.5, cost)
    assert "DDIM" in refused(r5)
    sig = [float(job.dm.sqrt_one_minus_alphas_cumprod[t]) for t in (20, 15, 10, 5, 0)]
    job.mp = _lib.RampMcmcParams(); job.mp.kind = 1
    job.mp.n_inner, job.mp.step_size, job.mp.sigma = arrays.i32([0] * 5), arrays.f32([1e-3] * 5), arrays.f32(sig)
    job.z = dev(synth.make_noise((1, 6, 8, 4), seed=94))
    assert "DDIM" in refused(r5)
    job.mp.n_inner = arrays.i32([0, 1, 0, 0, 0])
    rc, r = job.steered_rc(r5, u, 2)
    assert rc == 0 and np.isfinite(r["x"].cpu().numpy()).all() and (r["anc"].cpu().numpy() >= 0).all()
    # the kernel-level entry
    lw = torch.zeros(6, dtype=torch.float64, device="cuda")
    for gf, ess in (([0, 5], 0.5), ([1, 6], 0.5), ([0, 6], 2.5), ([0, 6], float("nan"))):
        g = np.asarray(gf, np.int32)
        assert job.lib.ramp_resample_groups(_lib.ptr(out), 6, 8, 4, _lib.ptr(lw), None, g.ctypes.data_as(_lib.c_i32p), 1, _lib.ptr(u), ess, None,
                                            None, job.s) != 0
        assert "ramp_resample_groups" in job.lib.ramp_last_error().decode()
    assert float(out.min()) == 7.0


def test_python_refusals_on_the_device():
    """resample= with hard-condition values that differ inside a group, on a sharded job, on the DDIM loop without inner steps and with
    injected u next to Philox noise: each raises with a message before the job runs; last_resample of a job without events is empty."""
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    rs = dict(every=2, lambda_=1.0, cloud=dev(uniform((50, 2), 91)), radius=RADIUS)
    dm = G.small_model()
    hc = {k: v.unsqueeze(0).repeat(4, 1).cuda() for k, v in G.hct(4).items()}
    hc[next(iter(hc))][2, 0] += 0.5
    with pytest.raises(ValueError, match="differ inside a group"):
        dm.run_inference(None, hc, n_samples=4, obstacle_pts=scene, resample=rs)
    dm.set_noise_shard(0, 8)
    with pytest.raises(NotImplementedError, match="sharded"):
        dm.run_inference(None, G.hct(4), n_samples=4, obstacle_pts=scene, resample=rs)
    dm.set_noise_shard(None)
    with pytest.raises(NotImplementedError, match="DDIM"):
        G.small_model(sampler="ddim").run_inference(None, G.hct(4), n_samples=4, obstacle_pts=scene, resample=rs)
    with pytest.raises(ValueError, match="philox"):
        G.small_model(noise_source="philox").run_inference(None, G.hct(4), n_samples=4, obstacle_pts=scene, resample=dict(rs, u=torch.rand(12, 1)))
    out = dm.run_inference(None, G.hct(4), n_samples=4, obstacle_pts=scene, resample=dict(rs, t_start=0))
    assert np.isfinite(out.cpu().numpy()).all() and dm.last_resample["events"] == [] and dm.last_resample["ancestors"].shape == (0, 4)
    from ramp_amd.resample import lineage
    dm.run_inference(None, G.hct(4), n_samples=4, obstacle_pts=scene, resample=dict(rs, ess_frac=2.0, lambda_=50.0))
    lr = dm.last_resample
    assert lr["ancestors"].shape == (12, 4) and lr["ess"].shape == (12, 1) and lr["cost"].shape == (12, 4) and lr["logw"].shape == (4,)
    assert set(lineage(lr["ancestors"]).tolist()) <= set(range(4))
