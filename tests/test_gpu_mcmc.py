"""Per-trajectory energies and Langevin refinement (ULA / MALA) inside the sampling job: ``ramp_score_energy``, the combined energy of a
job's evaluation, the step kernels alone, one teacher-forced MALA iteration against the float64 oracle, a free-running ULA chain, kind 0,
many-scene and composed jobs, the Philox layout, stale graphs and the refusals of ``ramp_sample_mcmc``.

The truth is ``oracle.ramp_oracle`` in float64; the MALA rule is restated in numpy below (``McmcOracle``).  Every bar that is not an
exact statement comes from a CPU measurement of the float32 oracle against the float64 one on the inputs of the test (recorded in the
docstrings and in DESIGN.md section 2), never from what the HIP code gives."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.diffusion import mcmc_tables
from util import GOLDEN, NoiseInjector, build_unet, dev, weights

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the oracle
def score_and_f(uo, x, tt, lat):
    """(f, eps) of one oracle evaluation: ``score`` runs the forward pass itself, its output is kept."""
    keep = {}
    orig = uo.forward_no_energy

    def wrapped(*a, **k):
        r = orig(*a, **k)
        keep["f"] = r[0] if isinstance(r, tuple) else r
        return r

    uo.forward_no_energy = wrapped
    try:
        eps = uo.score(x, tt, lat)
    finally:
        del uo.forward_no_energy
    return keep["f"], eps


def row_energy(f):
    """E[r] = 1/2 sum f^2 in float64 of the values f holds."""
    f = np.asarray(f, np.float64)
    return 0.5 * (f.reshape(f.shape[0], -1) ** 2).sum(1)


class McmcOracle(O.SamplerOracle):
    """SamplerOracle with the guidance-combined energy next to the guidance-combined gradient, and the Langevin inner steps.  ``latent``
    (ctx,): CFG, rows [cond, uncond], weights (1 + w, -w); ``latent`` (K, ctx) with ``set_weights``: K obstacle sets, rows
    [c_0 .. c_{K-1}, u], weights (w_0 .. w_{K-1}, 1 - sum w) -- the weights that form e_comb, applied to the rows' energies in float64."""

    def __init__(self, *a, set_weights=None, **k):
        super().__init__(*a, **k)
        self.set_weights = None if set_weights is None else tuple(set_weights)

    def eps_energy(self, x, t, latent):
        B = x.shape[0]
        if self.set_weights is None:
            n, lat = 2, np.zeros((B, 2, latent.shape[-1]), self.dt)
            lat[:, 0] = latent
            wts = np.array([np.float32(1.0 + self.w), -np.float32(self.w)], np.float64)
        else:
            K = len(self.set_weights)
            n, lat = K + 1, np.zeros((B, K + 1, latent.shape[-1]), self.dt)
            lat[:, :K] = latent
            wts = np.array([np.float32(w) for w in self.set_weights] + [np.float32(1.0 - sum(self.set_weights))], np.float64)
        f, out = score_and_f(self.unet, np.repeat(x, n, axis=0), np.full((B * n,), t, np.int64), lat.reshape(B * n, -1))
        out = out.reshape(B, n, *x.shape[1:])
        if self.set_weights is None:
            w = self.dt(self.w)
            e = ((1 + w) * out[:, 0] - w * out[:, 1]).astype(self.dt)
        else:
            e = out[:, n - 1]
            for k, w in enumerate(self.set_weights):
                e = e + self.dt(w) * (out[:, k] - out[:, n - 1])
            e = e.astype(self.dt)
        E_rows = row_energy(f).reshape(B, n)
        return e, E_rows @ wts, E_rows

    def eps_cfg(self, x, t, latent):
        return self.eps_energy(x, t, latent)[0]

    def inner_steps(self, x, e, E, t, latent, kind, K, eta, sigma, z, u, pinned, log=None):
        """K inner steps from state x with cached (e, E): returns (x, e, E, flags (K, B)).  a = float32(eta / sigma), c = float32(sqrt(2 eta))
        are the proposal's parameters in every precision; log alpha is formed in float64 from the values the precision holds."""
        dt = self.dt
        a, cz = np.float32(np.float64(eta) / np.float64(sigma)), np.float32(np.sqrt(2.0 * np.float64(eta)))
        free = np.ones(x.shape[1], bool)
        free[list(pinned)] = False
        flags = []
        for k in range(K):
            xp = x.copy()
            xp[:, free] = ((x[:, free] - dt(a) * e[:, free]).astype(dt) + (dt(cz) * z[k][:, free].astype(dt)).astype(dt)).astype(dt)
            ep, Ep, _ = self.eps_energy(xp, t, latent)
            if kind == "ula":
                acc = np.ones(x.shape[0], bool)
                la = np.zeros(x.shape[0])
            else:
                x64, xp64, e64, ep64 = (np.asarray(v, np.float64)[:, free] for v in (x, xp, e, ep))
                rev = ((x64 - xp64 + np.float64(a) * ep64) ** 2).reshape(x.shape[0], -1).sum(1)
                fwd = ((xp64 - x64 + np.float64(a) * e64) ** 2).reshape(x.shape[0], -1).sum(1)
                la = -(Ep - E) / np.float64(sigma) - (rev - fwd) / (4.0 * np.float64(eta))
                acc = np.isfinite(Ep) & np.isfinite(la) & (np.log(np.asarray(u[k], np.float64)) < la)
            if log is not None:
                log.append(la)
            x = np.where(acc[:, None, None], xp, x)
            e = np.where(acc[:, None, None], ep, e)
            E = np.where(acc, Ep, E)
            flags.append(acc.astype(np.int32))
        return x, e, E, np.array(flags).reshape(K, x.shape[0])

    def ddpm_mcmc(self, noise, hard_conds, latent, mcmc, z, u, noise_scale=0.5, x_start=None, steps=None, log=None):
        """The DDPM loop with inner steps; ``steps`` restricts it to those loop iterations (teacher forcing from ``x_start``)."""
        s, dt = self.sched, self.dt
        ts = list(reversed(range(self.T)))
        tab = mcmc_tables(mcmc, ts if steps is None else [ts[j] for j in steps], s["alphas_cumprod"])
        kind = "ula" if tab["kind"] == 1 else "mala"
        x = O.apply_hard_conditioning((noise[0] if x_start is None else x_start).astype(dt).copy(), hard_conds)
        chain, flags, kk = [x.copy()], [], 0
        for i, j in enumerate(range(self.T) if steps is None else steps):
            t = ts[j]
            K, eta, sig = tab["n_inner"][i], np.float32(tab["step_size"][i]), np.float32(tab["sigma"][i])
            e, E, _ = self.eps_energy(x, t, latent)
            if K:
                x, e, E, fl = self.inner_steps(x, e, E, t, latent, kind, K, eta, sig, z[kk:kk + K], None if u is None else u[kk:kk + K],
                                               hard_conds.keys(), log)
                flags.append(fl)
                kk += K
            _, mean = self.x0_mean(x, e, t)
            zz = noise[1 + i].astype(dt) if t != 0 else np.zeros_like(x)
            std = np.exp(dt(0.5) * s["posterior_log_variance_clipped"][t])
            x = O.apply_hard_conditioning((mean + std * zz * dt(noise_scale)).astype(dt), hard_conds)
            chain.append(x.copy())
        return np.stack(chain), (np.concatenate(flags) if flags else np.zeros((0, x.shape[0]), np.int32))

    def ddim_mcmc(self, noise0, hard_conds, latent, mcmc, z, u, K_ddim, cloud=None, use_apf=False, apf_from=2):
        s, dt = self.sched, self.dt
        ts = [int(t) for t in O.ddim_timesteps(self.T, K_ddim)]
        tab = mcmc_tables(mcmc, ts, s["alphas_cumprod"])
        kind = "ula" if tab["kind"] == 1 else "mala"
        x = O.apply_hard_conditioning(noise0.astype(dt).copy(), hard_conds)
        chain, kk, ac = [x.copy()], 0, s["alphas_cumprod"]
        for j, t in enumerate(ts):
            K = tab["n_inner"][j]
            e, E, _ = self.eps_energy(x, t, latent)
            if K:
                x, e, E, _ = self.inner_steps(x, e, E, t, latent, kind, K, np.float32(tab["step_size"][j]), np.float32(tab["sigma"][j]),
                                              z[kk:kk + K], None if u is None else u[kk:kk + K], hard_conds.keys())
                kk += K
            prev = t - self.T // K_ddim
            a_t, a_prev = ac[t], (ac[prev] if prev >= 0 else dt(1.0))
            x0, _ = self.x0_mean(x, e, t)
            if use_apf and j >= apf_from:
                for _ in range(3):
                    x0 = O.apply_hard_conditioning(O.apf_avoidance(x0, cloud, 0.07, 0.1, 7).copy(), hard_conds)
            e2 = (x - np.sqrt(a_t) * x0) / np.sqrt(dt(1) - a_t)
            x = O.apply_hard_conditioning((np.sqrt(a_prev) * x0 + np.sqrt(dt(1) - a_prev) * e2).astype(dt), hard_conds)
            chain.append(x.copy())
        return np.stack(chain)


def _sched(T):
    return dict(np.load(f"{GOLDEN}/schedule_T{T}.npz"))


def _oracle(dtype, T=25, w=2.0, S=4, H=48, o3=False, set_weights=None):
    uo = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=dtype)
    return McmcOracle(uo, T, w, dtype=dtype, sched=_sched(T), set_weights=set_weights)


def _hcn(S=4, H=48):
    return synth.default_hard_conds(S, H)


def _hc(S=4, H=48):
    return {k: torch.from_numpy(v) for k, v in _hcn(S, H).items()}


def _static(T=25, use_apf=False, sampler="ddpm", use_graph=True, max_rows=64, gemm_mode="default", noise_source="torch", noise_seed=0):
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=max_rows, gemm_mode=gemm_mode)
    return StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True, compose=False,
                                        use_apf=use_apf, sampler=sampler, use_graph=use_graph, noise_source=noise_source,
                                        noise_seed=noise_seed).eval().to("cuda")


def _uniforms(shape, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.98, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: energy of one evaluation
ENERGY_SHAPES = [(2, 8, False), (4, 48, False), (16, 64, False), (6, 48, True)]
ENERGY_FIXTURES = [("2d_h48", 4, 48, False), ("3d_h48", 6, 48, True)]
# The bars: 4 x the float32 UNetOracle's relative energy error against float64 on the test's own inputs (worst row of every n_rp), measured on
# the CPU by write_goldens and kept in the fixture -- (2, 8) 1.80e-6, (4, 48) 4.32e-7, (16, 64) 1.07e-7, 3-D (6, 48) 2.57e-7


def energy_bar(key):
    return 4.0 * float(np.load(f"{GOLDEN}/mcmc_oracle64.npz")[key])


def energy_inputs(S, H, o3, n_rp, B=3):
    """x (B, H, S), the per-variant clouds (n_rp - 1 scenes and the unconditional row; n_rp = 1: one scene), t."""
    x = synth.make_noise((B, H, S), seed=300 + S + n_rp)
    n_sc = max(1, n_rp - 1)
    clouds = [synth.make_cloud(4, 30, 3, seed=40 + k) if o3 else synth.make_cloud(6, 64, 2, seed=40 + k) for k in range(n_sc)]
    return x, clouds, 11


def energy_rows_oracle(uo, x, clouds, n_rp, t):
    B = x.shape[0]
    lat = np.zeros((B, n_rp, uo.encode_scene(clouds[0]).shape[-1]), uo.dt)
    for k, c in enumerate(clouds):
        lat[:, k] = uo.encode_scene(c)
    f = uo.forward_no_energy(np.repeat(x, n_rp, axis=0), np.full((B * n_rp,), t, np.int64), lat.reshape(B * n_rp, -1))
    return row_energy(f)


def _score_energy(m, xd, B, n_rp, t, want=True):
    H, S = xd.shape[1], xd.shape[2]
    f = torch.empty((B * n_rp, H, S), device="cuda") if want else None
    eps = torch.empty((B * n_rp, H, S), device="cuda") if want else None
    E = torch.empty((B * n_rp,), device="cuda", dtype=torch.float64)
    _lib.check(_lib.load().ramp_score_energy(m.ctx(), _lib.ptr(xd), B, n_rp, t, _lib.ptr(f), _lib.ptr(eps), _lib.ptr(E), _lib.current_stream()),
               "ramp_score_energy")
    torch.cuda.synchronize()
    return f, eps, E


@pytest.mark.parametrize("S,H,o3", ENERGY_SHAPES)
def test_energy_of_one_evaluation(S, H, o3):
    """B = 3, n_rp in {1, 2, 4}: energies against 1/2 sum f^2 of the float64 oracle; f_out / eps_out bit-equal to ramp_score's; energies
    bit-equal with max_rows forcing two chunks.  Bar: 4 x the float32 CPU oracle's own relative energy error against float64 on these
    inputs (fixture energy/f32rel/*, measured on the CPU; the README puts the GPU's f error at about 1.4 x the float32 CPU's).  On a bf16x6
    context (no call-history-dependent scales: the chunked energies are bit-equal) and, same bar, on a context in the default fp16x3 mode (its
    second evaluation: the first one calibrates on the bf16x6 kernels)."""
    lib = _lib.load()
    u64 = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=np.float64)
    m = build_unet(S, H, o3, max_rows=64, gemm_mode="bf16x6")
    small = build_unet(S, H, o3, max_rows=8, gemm_mode="bf16x6")
    dflt = build_unet(S, H, o3, max_rows=64)
    for mm in (m, small, dflt):
        mm.prepare_time_table(25)
    bar = energy_bar(f"energy/f32rel/{S}_{H}_{int(o3)}")
    for n_rp in (1, 2, 4):
        x, clouds, t = energy_inputs(S, H, o3, n_rp)
        want = energy_rows_oracle(u64, x, clouds, n_rp, t)
        xd = dev(x)
        got = {}
        for mm in (m, small):
            lat = torch.cat([mm.encode_scene(dev(c)) for c in clouds] + ([torch.zeros(1, mm.context_dim, device="cuda")] if n_rp > 1 else []))
            mm.set_scene(lat, list(range(n_rp)))
            f, eps, E = _score_energy(mm, xd, 3, n_rp, t)
            f0 = torch.empty_like(f); e0 = torch.empty_like(eps)
            _lib.check(lib.ramp_score(mm.ctx(), _lib.ptr(xd), 3, n_rp, t, _lib.ptr(f0), _lib.ptr(e0), _lib.current_stream()), "ramp_score")
            torch.cuda.synchronize()
            assert torch.equal(f, f0) and torch.equal(eps, e0)
            got[mm] = E.cpu().numpy()
        err = float(np.abs(got[m] / want - 1.0).max())
        print(f"energy S={S} H={H} 3d={o3} n_rp={n_rp}: worst relative error {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        if 3 * n_rp > 8:       # (two chunks on the small context)
            assert np.array_equal(got[m], got[small])
        _, _, E2 = _score_energy(m, xd, 3, n_rp, t, want=False)      # no f_out: the context's scratch
        assert np.array_equal(E2.cpu().numpy(), got[m])
        lat = torch.cat([dflt.encode_scene(dev(c)) for c in clouds] + ([torch.zeros(1, dflt.context_dim, device="cuda")] if n_rp > 1 else []))
        dflt.set_scene(lat, list(range(n_rp)))
        _score_energy(dflt, xd, 3, n_rp, t)
        _, _, E3 = _score_energy(dflt, xd, 3, n_rp, t)
        assert dflt.score_mode() == "fp16x3"
        err3 = float(np.abs(E3.cpu().numpy() / want - 1.0).max())
        print(f"    the same in fp16x3: {err3:.2e}")
        assert err3 <= bar


@pytest.mark.parametrize("tag,S,H,o3", ENERGY_FIXTURES)
def test_energy_against_the_reference_fixture(tag, S, H, o3):
    """1/2 sum f^2 of the reference's own f (tests/golden/unet*_h48.npz) through the Python accessor.  Bar: 4 x the float32 oracle's relative
    energy error against float64 on THESE inputs (2-D 2.56e-7, 3-D 4.0e-8) plus the distance of the reference's own energies from float64
    (2.0e-7, 1.4e-7: the reference's f is a float32 evaluation itself, on the 3-D fixture 3.5 x as far from float64 as the numpy one) -- i.e. the
    HIP energy may be 4 x the float32 error from the truth, and the comparison is with something that far from it.  Both measured on the CPU by
    write_goldens (fixture energy/fixture/<tag>/f32rel, refrel)."""
    g = np.load(f"{GOLDEN}/unet{tag}.npz")
    m = build_unet(S, H, o3, max_rows=8, gemm_mode="bf16x6")
    N = g["x"].shape[0]
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    E = m.energy(dev(g["x"]), torch.from_numpy(g["t"]).cuda(), obstacle_pts=pts)
    assert E.dtype == torch.float64 and tuple(E.shape) == (N,)
    err = float(np.abs(E.cpu().numpy() / row_energy(g["f"]) - 1.0).max())
    bar = energy_bar(f"energy/fixture/{tag}/f32rel") + float(np.load(f"{GOLDEN}/mcmc_oracle64.npz")[f"energy/fixture/{tag}/refrel"])
    print(f"energy vs reference f, {tag}: {err:.2e} (bar {bar:.2e})")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 2: combined energy in a job's evaluation
def test_combined_energy_equals_the_weighted_row_energies():
    """CFG, the three-row compose and a row_weight table with a zero-weight padding row: E_comb[b] = sum_j w_j E[b n_rp + j] of
    ramp_score_energy's per-row energies to fp64 rounding (n_rp terms: (n_rp + 1) ulp of the largest term)."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    lib = _lib.load()
    B, t = 3, 9
    x = synth.make_noise((B, 48, 4), seed=61)
    xd = dev(x)
    # CFG and compose through model.energy
    for compose in (False, True):
        u = build_unet(4, 48, False, max_rows=64, gemm_mode="bf16x6")
        dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=25, predict_epsilon=True, compose=compose, sampler="ddpm").eval().to("cuda")
        pts = torch.stack([dev(synth.make_cloud(6, 64, 2, seed=3)), dev(synth.make_cloud(6, 64, 2, seed=4))]) if compose \
            else dev(synth.make_cloud(6, 64, 2, seed=3))
        Ec = dm.energy(xd, t, pts).cpu().numpy()
        n_rp = 3 if compose else 2
        _, _, E = _score_energy(u, xd, B, n_rp, t)
        E = E.cpu().numpy().reshape(B, n_rp)
        w = np.array(dm._comb_weights(), np.float64)
        want = (E * w).sum(1)
        tol = (n_rp + 1) * np.finfo(np.float64).eps * np.abs(E * w).max(1)
        print(f"combined energy compose={compose}: {np.abs(Ec - want).max():.2e} (tol {tol.min():.2e})")
        assert (np.abs(Ec - want) <= tol).all()
        if not compose:
            assert w.tolist() == [3.0, -2.0]
    # a weight table with a zero-weight padding row, n_rp = 4
    u = build_unet(4, 48, False, max_rows=64, gemm_mode="bf16x6")
    u.prepare_time_table(25)
    lat = torch.cat([u.encode_scene(dev(synth.make_cloud(6, 64, 2, seed=3 + k))) for k in range(2)] + [torch.zeros(1, u.context_dim, device="cuda")])
    u.set_scenes(lat, [0, 1, 2, 2] * B)
    rw = np.tile(np.array([[1.5, 2.5, 0.0, -3.0]], np.float32), (B, 1))
    rw[1] = [0.5, 0.0, 0.0, 0.5]
    _, _, E = _score_energy(u, xd, B, 4, t)
    out = torch.empty((B,), device="cuda", dtype=torch.float64)
    rwd = dev(rw)
    _lib.check(lib.ramp_combine_energy(_lib.ptr(E), B, 4, None, _lib.ptr(rwd), _lib.ptr(out), _lib.current_stream()), "ramp_combine_energy")
    torch.cuda.synchronize()
    E = E.cpu().numpy().reshape(B, 4)
    want = (E * rw.astype(np.float64)).sum(1)
    assert (np.abs(out.cpu().numpy() - want) <= 5 * np.finfo(np.float64).eps * np.abs(E * rw).max(1)).all()
    assert np.array_equal(E[:, 2], E[:, 3])       # the padding row reads the unconditional latent


# ------------------------------------------------------------------------------------------------ 3: the step kernels alone
def _propose(x, eps, z, a, cz, pinned, B, H, S):
    xp = torch.empty_like(x)
    pin = torch.tensor(list(pinned), dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_mcmc_propose(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(z), float(a), float(cz), _lib.ptr(pin), len(pinned),
                                             _lib.ptr(xp), B, H, S, _lib.current_stream()), "ramp_mcmc_propose")
    torch.cuda.synchronize()
    return xp


@pytest.mark.parametrize("S,H", [(2, 8), (4, 48)])
def test_step_kernels_alone(S, H):
    """B = 5, pinned waypoints {0, H - 1} and one interior one.  Proposal: (x - a eps) + c z is two fp32 products, a difference and a sum --
    against the exact (float64) value at most 1/2 ulp per operation: eps32 (|a eps| + |c z| + |x - a eps| + |x'|) / 2 covers the four
    roundings as they propagate; pinned waypoints are bit-equal to x.  log alpha against numpy float64 from crafted E, E', eps, eps' (fp64
    sums of <= 1024 terms: 1e-12 relative to the terms' magnitude); decisions exact wherever |log alpha - log u| exceeds that; a NaN E' rejects."""
    B = 5
    pinned = (0, H - 1, H // 2)
    rng = np.random.default_rng(S * 100 + H)
    x, eps, z, epsp = (rng.standard_normal((B, H, S)).astype(np.float32) for _ in range(4))
    sigma, eta = np.float32(0.8), np.float32(0.03)
    a, cz = np.float32(np.float64(eta) / np.float64(sigma)), np.float32(np.sqrt(2.0 * np.float64(eta)))
    xd, ed, zd = dev(x), dev(eps), dev(z)
    xp = _propose(xd, ed, zd, a, cz, pinned, B, H, S).cpu().numpy()
    free = np.ones(H, bool); free[list(pinned)] = False
    x64, e64, z64 = (v.astype(np.float64) for v in (x, eps, z))
    want = x64 - np.float64(a) * e64 + np.float64(cz) * z64
    e32 = np.finfo(np.float32).eps
    bar = 0.5 * e32 * (np.abs(np.float64(a) * e64) + np.abs(np.float64(cz) * z64) + np.abs(x64 - np.float64(a) * e64) + np.abs(want))
    assert (np.abs(xp[:, free] - want[:, free]) <= bar[:, free]).all()
    assert np.array_equal(xp[:, ~free], x[:, ~free])
    # log alpha and the decisions
    E = rng.uniform(5, 6, B); Ep = E + rng.uniform(-0.5, 0.5, B)
    rev = ((x64 - xp + np.float64(a) * epsp.astype(np.float64)) ** 2)[:, free].reshape(B, -1).sum(1)
    fwd = ((xp.astype(np.float64) - x64 + np.float64(a) * e64) ** 2)[:, free].reshape(B, -1).sum(1)
    la = -(Ep - E) / np.float64(sigma) - (rev - fwd) / (4.0 * np.float64(eta))
    u = np.exp(la + np.array([0.3, -0.3, 1e-3, -1e-3, 0.5])).clip(1e-6, 1 - 1e-6).astype(np.float32)
    Ep_nan = Ep.copy(); Ep_nan[1] = np.nan
    for kind, Eprop in ((2, Ep), (2, Ep_nan), (1, Ep)):
        xs, es, xpd, epd, ud = dev(x), dev(eps), dev(xp), dev(epsp), dev(u)      # (held: a temporary's block would be reused by the next one)
        Es, Eps = dev(E), dev(Eprop)
        flag = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        lad = torch.zeros((B,), dtype=torch.float64, device="cuda")
        pin = torch.tensor(list(pinned), dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().ramp_mcmc_accept(_lib.ptr(xs), _lib.ptr(xpd), _lib.ptr(es), _lib.ptr(epd), _lib.ptr(Es), _lib.ptr(Eps),
                                                _lib.ptr(ud), kind, float(a), float(sigma), float(eta), _lib.ptr(pin), len(pinned),
                                                _lib.ptr(flag), _lib.ptr(lad), B, H, S, _lib.current_stream()), "ramp_mcmc_accept")
        torch.cuda.synchronize()
        flag = flag.cpu().numpy()
        if kind == 1:
            assert flag.tolist() == [1] * B
        else:
            got_la = lad.cpu().numpy()
            ok = np.isfinite(Eprop)
            assert (np.abs(got_la[ok] - la[ok]) <= 1e-12 * (np.abs(E[ok]) / sigma + (rev[ok] + fwd[ok]) / (4 * eta))).all()
            want_flag = (np.log(u.astype(np.float64)) < la) & ok
            assert flag.tolist() == want_flag.astype(int).tolist(), (flag, want_flag)
            assert flag[ok].min() == 0 and flag[ok].max() == 1
        acc = flag.astype(bool)
        assert np.array_equal(xs.cpu().numpy(), np.where(acc[:, None, None], xp, x))
        assert np.array_equal(es.cpu().numpy(), np.where(acc[:, None, None], epsp, eps))
        if kind == 2:
            assert np.array_equal(Es.cpu().numpy()[acc], Eprop[acc]) and np.array_equal(Es.cpu().numpy()[~acc], E[~acc])


# ------------------------------------------------------------------------------------------------ 4: one teacher-forced MALA iteration
MALA_CASES = [(24, 0), (12, 12), (3, 21), (0, 24)]      # (network timestep t, loop iteration j of the T = 25 DDPM list)
MALA_STEP_SCALE = 2.0
# 4 x the largest |log alpha_float32 - log alpha_float64| of the oracle over these cases, K = 1 and 2 (1.20e-3, at t = 0; measured on the CPU
# by write_goldens, kept in the fixture as mala/dmax32)
MALA_DELTA = 4.8e-3


def mala_case_inputs(j, K, B=6):
    """State (B, H, S) of a DDPM chain at iteration j (the four rows of the plain chain fixture and its rows 2, 3 with the horizon reversed),
    the iteration's noise, the inner steps' normals and uniforms (K = 1 takes the first of K = 2's)."""
    g = np.load(f"{GOLDEN}/chain_ddpm_plain.npz")
    x = np.concatenate([g["chain"][j], g["chain"][j][2:4][:, ::-1].copy()])[:B]
    x = O.apply_hard_conditioning(x.copy(), _hcn())
    nz = synth.make_noise((B, 48, 4), seed=900 + j)
    z = synth.make_noise((2, B, 48, 4), seed=910 + j)[:K]
    u = _uniforms((2, B), 920 + j)[:K]
    return g, x, nz, z, u


def mala_oracle_case(dtype, t, j, K, scale):
    """(next state, flags (K, B), log alpha (K, B), log u (K, B)) of the oracle in ``dtype``."""
    g, x, nz, z, u = mala_case_inputs(j, K)
    so = _oracle(dtype)
    log = []
    chain, flags = so.ddpm_mcmc(np.stack([x, nz]), _hcn(), g["latent"], dict(kind="mala", steps=K, step_scale=scale), z, u, x_start=x,
                                steps=[j], log=log)
    return chain[1], flags, np.array(log), np.log(u.astype(np.float64))


@pytest.mark.parametrize("K", [1, 2])
def test_one_teacher_forced_mala_iteration(K):
    """CFG, B = 6, S = 4, H = 48, T = 25, iterations with t in {24, 12, 3, 0}, K inner steps (K = 2: an accepted proposal's cached eps / E feed the
    next inner step and the reverse step), step_scale 2.0, against the float64 oracle (tests/golden/mcmc_oracle64.npz, written by
    write_goldens below).  A decision is compared only where the float64 oracle has |log alpha - log u| >= MALA_DELTA = 4.8e-3 = 4 x 1.20e-3, the
    largest |log alpha_float32 - log alpha_float64| of the oracle over these cases; at most 10 % are left out, at least a quarter of the compared
    ones are accepted and a quarter rejected (the oracle alone: 13 of 24 accepted for K = 1, 23 of 48 for K = 2, none left out, smallest margin
    1.2e-1; test_mcmc_host.py checks it on the CPU); where all decisions of a trajectory agree, its next state meets the teacher-forced step
    bar of tests/test_gpu_sampler.py (1e-4)."""
    G = np.load(f"{GOLDEN}/mcmc_oracle64.npz")
    dm = _static(25, use_graph=True)
    n_cmp = n_acc = n_all = 0
    for t, j in MALA_CASES:
        g, x, nz, z, u = mala_case_inputs(j, K)
        want_x, want_f, la, lu = G[f"mala/K{K}/t{t}/x"], G[f"mala/K{K}/t{t}/flags"], G[f"mala/K{K}/t{t}/la"], np.log(u.astype(np.float64))
        mc = dict(kind="mala", steps=K, step_scale=MALA_STEP_SCALE, noise=dev(z), u=dev(u))
        hc = {k: v.cuda().unsqueeze(0).expand(6, -1) for k, v in _hc().items()}
        out, _ = dm._launch(6, torch.stack([dev(x), dev(nz)]), hc, dev(g["cloud"]), False, [t], [0], [0.5], None, False, mcmc=mc)
        got_f = dm.last_mcmc["accept"].numpy()
        assert got_f.shape == (K, 6)
        sure = np.abs(la - lu) >= MALA_DELTA
        agree = np.ones(6, bool)      # (a trajectory's later decisions are comparable only while its earlier ones were)
        for k in range(K):
            cmp_k = sure[k] & agree
            assert np.array_equal(got_f[k][cmp_k], want_f[k][cmp_k]), (t, k, got_f[k], want_f[k], la[k] - lu[k])
            n_cmp += int(cmp_k.sum()); n_acc += int(want_f[k][cmp_k].sum()); n_all += 6
            agree &= sure[k]
        err = float(np.abs(out.cpu().numpy()[agree] - want_x[agree]).max()) if agree.any() else 0.0
        print(f"MALA K={K} t={t}: flags {got_f.tolist()} smallest margin {np.abs(la - lu).min():.2e}, next state vs float64 {err:.2e}, "
              f"rate {dm.last_mcmc['rate']}")
        assert err < 1e-4
    assert n_cmp >= 0.9 * n_all
    assert n_acc >= 0.25 * n_cmp and (n_cmp - n_acc) >= 0.25 * n_cmp


# ------------------------------------------------------------------------------------------------ 4b: the in-job combined energy beyond CFG
COMP_KINDS = ("compose", "padded")


def comp_scenes(kind):
    """compose: the wrapper's own three-row job (two obstacle sets, rows [A, B, unconditional], weights (2, 2, -3)).  padded: a composed job of
    two scenes with 1 and 2 sets, n_samples (2, 3), three rows per trajectory -- scene 0's middle row is a zero-weight padding row."""
    if kind == "compose":
        return [[synth.make_cloud(6, 64, 2, seed=3), synth.make_cloud(6, 64, 2, seed=4)]], [6]
    return [[synth.make_cloud(5, 64, 2, seed=500)], [synth.make_cloud(4, 64, 2, seed=510), synth.make_cloud(5, 64, 2, seed=511)]], [2, 3]


def comp_oracle_case(dtype, kind, t, j):
    """One teacher-forced MALA iteration (K = 1) of such a job in ``dtype``: every scene's rows through McmcOracle(set_weights = 2 per set) on
    the scene's own latents (a padding row has weight 0: it adds nothing to gradient or energy).  (next state, flags (1, B), log alpha (1, B))."""
    scenes, ns = comp_scenes(kind)
    B = sum(ns)
    _, x, nz, z, u = mala_case_inputs(j, 1)
    xs, fl, las, b = [], [], [], 0
    for sets, n in zip(scenes, ns):
        so = _oracle(dtype, set_weights=(2.0,) * len(sets))
        lat = np.stack([so.unet.encode_scene(c) for c in sets])
        log = []
        sl = slice(b, b + n)
        chain, f = so.ddpm_mcmc(np.stack([x[sl], nz[sl]]), _hcn(), lat, dict(kind="mala", steps=1, step_scale=MALA_STEP_SCALE), z[:, sl], u[:, sl],
                                x_start=x[sl], steps=[j], log=log)
        xs.append(chain[1]); fl.append(f); las.append(np.array(log))
        b += n
    assert b == B
    return np.concatenate(xs), np.concatenate(fl, axis=1), np.concatenate(las, axis=1)


@pytest.mark.parametrize("kind", COMP_KINDS)
def test_in_job_combined_energy_of_compose_and_composed_jobs_in_two_chunks(kind):
    """The combined energy INSIDE a job's evaluation (score_all with the shared prefix, f of all rows in the context's scratch, the rows'
    energies at their chunk's offset, the weights from the job's scalars or from its row_weight table) where test 4 does not reach: the
    three-row compose job (B = 6, max_rows = 12: chunks of 4 and 2 trajectories) and a padded composed job (scenes of 1 and 2 sets, B = 2 + 3,
    max_rows = 9: chunks of 3 and 2, a zero-weight padding row), one teacher-forced MALA iteration (K = 1, step_scale 2.0) at t in
    {24, 12, 3, 0} against the float64 McmcOracle(set_weights=...) of the fixture.  log alpha is -(E' - E) / sigma - ..., so a wrong energy, weight
    or offset moves the decisions.  As in test 4: decisions compared where the float64 oracle has |log alpha - log u| >= delta = 4 x the largest
    |log alpha_float32 - log alpha_float64| of the oracle over these cases (fixture: comp/<kind>/dmax32), at most 10 % left out, both outcomes
    among the compared ones, and the next state of the trajectories compared held to 1e-4."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    G = np.load(f"{GOLDEN}/mcmc_oracle64.npz")
    delta = 4.0 * float(G[f"comp/{kind}/dmax32"])
    scenes, ns = comp_scenes(kind)
    B = sum(ns)
    if kind == "compose":
        u_ = build_unet(4, 48, False, max_rows=12)
        dm = StaticGaussianDiffusionModel(model=u_, n_diffusion_steps=25, predict_epsilon=True, compose=True, sampler="ddpm").eval().to("cuda")
        pts, job, guid = torch.stack([dev(c) for c in scenes[0]]), None, None
        hc = {k: v.cuda().unsqueeze(0).expand(B, -1) for k, v in _hc().items()}
    else:
        dm = _static(25, max_rows=9)
        job, guid, hc, Bc = dm._prepare_composed_job([[dev(c) for c in sets] for sets in scenes], [_hc() for _ in scenes], ns, None, None)
        assert Bc == B and guid["n_rp"] == 3 and guid["row_weight"].cpu().numpy().tolist() == [[2.0, 0.0, -1.0]] * 2 + [[2.0, 2.0, -3.0]] * 3
        pts = None
    n_cmp = n_acc = n_all = 0
    for t, j in MALA_CASES:
        _, x, nz, z, u = mala_case_inputs(j, 1)
        x, nz, z, u = x[:B], nz[:B], z[:, :B], u[:, :B]
        want_x, want_f, la = G[f"comp/{kind}/t{t}/x"], G[f"comp/{kind}/t{t}/flags"], G[f"comp/{kind}/t{t}/la"]
        mc = dict(kind="mala", steps=1, step_scale=MALA_STEP_SCALE, noise=dev(z), u=dev(u))
        out, _ = dm._launch(B, torch.stack([dev(x), dev(nz)]), hc, pts, False, [t], [0], [0.5], None, False, scene_job=job, guidance=guid, mcmc=mc)
        got_f = dm.last_mcmc["accept"].numpy()
        sure = (np.abs(la - np.log(u.astype(np.float64))) >= delta)[0]
        assert np.array_equal(got_f[0][sure], want_f[0][sure]), (kind, t, got_f, want_f, la)
        n_cmp += int(sure.sum()); n_acc += int(want_f[0][sure].sum()); n_all += B
        err = float(np.abs(out.cpu().numpy()[sure] - want_x[sure]).max()) if sure.any() else 0.0
        print(f"{kind} MALA t={t}: flags {got_f.tolist()} (oracle {want_f.tolist()}), next state vs float64 {err:.2e}, delta {delta:.2e}")
        assert err < 1e-4
    assert n_cmp >= 0.9 * n_all and 0 < n_acc < n_cmp


# ------------------------------------------------------------------------------------------------ 5: ULA free-running chains
ULA_SCALE = 0.02
# float32 oracle chain against the float64 one on these inputs, largest distance over all states (measured on the CPU by write_goldens, kept in
# the fixture as ula/<kind>/drift32)
ULA_F32_DRIFT = {"ddpm": 1.203e-05, "ddim": 0.1073}
ULA_MARGIN = 1e-4 / 3.5e-5      # test_ddpm_chain_free_running: 1e-4 allowed where the reference's own float32 drift from float64 is 3.5e-5


def ula_inputs(kind):
    g = np.load(f"{GOLDEN}/chain_ddpm_plain.npz")
    return g, synth.make_noise((25 if kind == "ddpm" else 5, 4, 48, 4), seed=1234)


def ula_oracle_chain(dtype, kind):
    g, z = ula_inputs(kind)
    mc = dict(kind="ula", steps=1, step_scale=ULA_SCALE)
    if kind == "ddpm":
        return _oracle(dtype, 25).ddpm_mcmc(g["noise"], _hcn(), g["latent"], mc, z, None)[0]
    return _oracle(dtype, 25).ddim_mcmc(g["noise"][0], _hcn(), g["latent"], mc, z, None, 5, cloud=g["cloud"].reshape(-1, 2), use_apf=True)


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_ula_free_running_chain(kind):
    """T = 25, B = 4, one ULA step on every iteration: the DDPM loop, and DDIM-5 with the three-pass APF hook (from step 2), against the float64
    oracle chain of the fixture (every state, largest distance, as the existing chain tests compare).  Bar: the existing free-running chain
    test allows 1e-4 where the reference's own float32 drift from float64 is 3.5e-5, a margin of 2.86; the same margin on the float32
    oracle's drift on THESE chains (ULA_F32_DRIFT, measured on the CPU): DDPM 1.20e-5 -> bar 3.4e-5.  DDIM with APF: the hook is discontinuous
    (a waypoint enters or leaves the 0.07 threshold), the float32 oracle itself ends 1.07e-1 from the float64 one (5.6e-5 before the hook's
    second firing) -> bar 3.1e-1: by the same rule, and a weak statement.  Hence a second one: states 0 .. 2, before the hook fires at all (the
    repository compares free-running APF chains only up to the first application of the hook), where two iterations with
    their ULA steps have run and the float32 oracle sits 4.3e-6 from float64 -> bar 1.2e-5 by the same margin."""
    G = np.load(f"{GOLDEN}/mcmc_oracle64.npz")
    g, z = ula_inputs(kind)
    dm = _static(25, use_apf=(kind == "ddim"), sampler=kind)
    mc = dict(kind="ula", steps=1, step_scale=ULA_SCALE, noise=dev(z))
    with NoiseInjector(list(g["noise"][:26 if kind == "ddpm" else 1])):
        chain = dm.run_inference(None, _hc(), n_samples=4, horizon=48, return_chain=True, obstacle_pts=dev(g["cloud"]),
                                 noise_std_extra_schedule_fn=lambda x: 0.5, mcmc=mc).cpu().numpy()
    truth = G[f"ula/{kind}/chain"]
    assert chain.shape == truth.shape
    err = float(np.abs(chain - truth).max())
    bar = ULA_MARGIN * ULA_F32_DRIFT[kind]
    per = np.abs(chain - truth).reshape(chain.shape[0], -1).max(1)
    print(f"ULA {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {float(G[f'ula/{kind}/drift32']):.2e}); states 0..3: {per[:4]}")
    assert dm.last_mcmc["accept"].numpy().min() == 1 and dm.last_mcmc["accept"].shape == (z.shape[0], 4)
    assert np.abs(chain - g["chain"]).max() > 1e-2 if kind == "ddpm" else True      # (the inner steps do move the chain)
    assert err <= bar
    if kind == "ddim":      # the states before the APF hook first fires (it fires from iteration 2, i.e. into state 3): the DDIM inner steps alone
        pre = float(G["ula/ddim/drift32_states"][:3].max())
        assert per[:3].max() <= ULA_MARGIN * pre, (per[:3], pre)


def energy_fixture_oracle(dtype, tag, S, H, o3):
    """The rows' energies of the reference fixture's inputs in ``dtype`` (2-D: odd rows unconditional, as the network's own forward has it)."""
    g = np.load(f"{GOLDEN}/unet{tag}.npz")
    uo = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=dtype)
    N = g["x"].shape[0]
    lat = np.tile(uo.encode_scene(g["cloud"])[None], (N, 1)).astype(dtype)
    if o3:
        lat[1] = 0
    else:
        lat[1::2] = 0
    return row_energy(uo.forward_no_energy(g["x"], g["t"], lat))


def write_goldens(path=f"{GOLDEN}/mcmc_oracle64.npz", parts=("energy", "mala", "comp", "ula")):
    """The float64 oracle's results for tests 4, 4b and 5 (minutes of CPU: computed once, kept as a fixture), with the float32 oracle's
    distances from float64 that EVERY measured bar of this file is derived from (tests 1, 4, 4b, 5).  ``python -m ramp_amd.tools.make_mcmc_goldens``
    calls this; ``parts`` recomputes only those groups and keeps the others as the file has them."""
    import os
    out = dict(np.load(path)) if os.path.exists(path) and set(parts) != {"energy", "mala", "comp", "ula"} else {}
    if "energy" in parts:
        for S, H, o3 in ENERGY_SHAPES:
            u64, u32 = (O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=d) for d in (np.float64, np.float32))
            worst = 0.0
            for n_rp in (1, 2, 4):
                x, clouds, t = energy_inputs(S, H, o3, n_rp)
                worst = max(worst, float(np.abs(energy_rows_oracle(u32, x, clouds, n_rp, t) / energy_rows_oracle(u64, x, clouds, n_rp, t) - 1).max()))
            out[f"energy/f32rel/{S}_{H}_{int(o3)}"] = np.float64(worst)
            print(f"energy ({S}, {H}, 3d={o3}): float32 oracle relative error {worst:.3e}")
        for tag, S, H, o3 in ENERGY_FIXTURES:
            e64, e32 = energy_fixture_oracle(np.float64, tag, S, H, o3), energy_fixture_oracle(np.float32, tag, S, H, o3)
            g = np.load(f"{GOLDEN}/unet{tag}.npz")
            out[f"energy/fixture/{tag}/f32rel"] = np.float64(np.abs(e32 / e64 - 1).max())
            out[f"energy/fixture/{tag}/refrel"] = np.float64(np.abs(row_energy(g["f"]) / e64 - 1).max())
            print(f"energy of fixture {tag}: float32 oracle {out[f'energy/fixture/{tag}/f32rel']:.3e}; the reference's own f against float64 "
                  f"{np.abs(row_energy(g['f']) / e64 - 1).max():.3e}")
    if "mala" in parts:
        dmax = 0.0
        for K in (1, 2):
            n = acc = 0
            margins = []
            for t, j in MALA_CASES:
                x64, f64, la64, lu = mala_oracle_case(np.float64, t, j, K, MALA_STEP_SCALE)
                x32, f32, la32, _ = mala_oracle_case(np.float32, t, j, K, MALA_STEP_SCALE)
                same = np.ones(6, bool)
                for k in range(K):
                    if same.any():
                        dmax = max(dmax, float(np.abs(la32[k] - la64[k])[same].max()))
                    same &= f32[k] == f64[k]
                out[f"mala/K{K}/t{t}/x"], out[f"mala/K{K}/t{t}/flags"], out[f"mala/K{K}/t{t}/la"] = x64, f64, la64
                margins.append(np.abs(la64 - lu).ravel()); n += f64.size; acc += int(f64.sum())
                print(f"MALA K={K} t={t}: flags {f64.tolist()}; float32 oracle: |d log alpha| {np.abs(la32 - la64).max():.2e}, next state {np.abs(x32 - x64).max():.2e}")
            print(f"MALA K={K}: {acc} of {n} accepted, smallest |log alpha - log u| {np.concatenate(margins).min():.2e}")
        out["mala/dmax32"] = np.float64(dmax)
        print(f"largest |log alpha_32 - log alpha_64| {dmax:.3e} -> delta {4 * dmax:.3e}")
    if "comp" in parts:
        for kind in COMP_KINDS:
            dmax, acc, n, margins = 0.0, 0, 0, []
            for t, j in MALA_CASES:
                x64, f64, la64 = comp_oracle_case(np.float64, kind, t, j)
                x32, f32, la32 = comp_oracle_case(np.float32, kind, t, j)
                dmax = max(dmax, float(np.abs(la32 - la64).max()))
                out[f"comp/{kind}/t{t}/x"], out[f"comp/{kind}/t{t}/flags"], out[f"comp/{kind}/t{t}/la"] = x64, f64, la64
                lu = np.log(mala_case_inputs(j, 1)[4][:, :f64.shape[1]].astype(np.float64))
                margins.append(np.abs(la64 - lu).ravel()); n += f64.size; acc += int(f64.sum())
                print(f"{kind} t={t}: flags {f64.tolist()} log alpha {np.round(la64, 3).tolist()}; float32 oracle: |d log alpha| {np.abs(la32 - la64).max():.2e}, "
                      f"next state {np.abs(x32 - x64).max():.2e}")
            out[f"comp/{kind}/dmax32"] = np.float64(dmax)
            m = np.concatenate(margins)
            print(f"{kind}: {acc} of {n} accepted, delta {4 * dmax:.3e}, {int((m < 4 * dmax).sum())} left out, smallest margin {m.min():.2e}")
    if "ula" in parts or "ula-ddim" in parts:
        for kind in (("ddpm", "ddim") if "ula" in parts else ("ddim",)):
            c64, c32 = ula_oracle_chain(np.float64, kind), ula_oracle_chain(np.float32, kind)
            per = np.abs(c32 - c64).reshape(c64.shape[0], -1).max(1)
            out[f"ula/{kind}/chain"] = c64
            out[f"ula/{kind}/drift32"] = np.float64(per.max())
            out[f"ula/{kind}/drift32_states"] = per
            print(f"ULA {kind}: float32 oracle drift {per.max():.3e}, per state {per}")
    np.savez_compressed(path, **out)
    return out


# ------------------------------------------------------------------------------------------------ 6: kind 0
def _raw_params(dm, B, steps, arrays, hard=True):
    """ramp_sample_params of a DDPM job through the model's own filler."""
    p = _lib.RampSampleParams()
    p.B, p.n_rp, p.w0, p.w1 = B, 2, dm.cfg_weight, 0.0
    dm._fill_schedule(p, arrays, False, steps, [0.5] * len(steps))
    p.apply_apf = arrays.i32([0] * len(steps))
    p.clip_denoised, p.predict_x0, p.use_graph = 1, 0, 1
    if hard:
        dm._fill_hard(p, arrays, {k: v.cuda().unsqueeze(0).expand(B, -1) for k, v in _hc().items()}, B)
    return p


def _mcmc_params(arrays, kind, n_inner, step, sigma):
    mp = _lib.RampMcmcParams()
    mp.kind = kind
    mp.n_inner, mp.step_size, mp.sigma = arrays.i32(n_inner), arrays.f32(step), arrays.f32(sigma)
    return mp


def test_kind_0_is_the_plain_job_bit_for_bit():
    """ramp_sample_mcmc with kind 0 against ramp_sample, ramp_sample_scenes and ramp_sample_composed on the same noise: equal chains."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = _static(25)
    B, steps = 3, [24, 23, 22, 1, 0]
    noise = dev(synth.make_noise((len(steps) + 1, B, 48, 4), seed=8))
    arrays = _HostArrays()
    mp0 = _mcmc_params(arrays, 0, [0] * len(steps), [0.0] * len(steps), [0.0] * len(steps))

    def chains(plain, mc):
        a = torch.empty((len(steps) + 1, B, 48, 4), device="cuda"); b = torch.empty_like(a)
        plain(a); mc(b)
        torch.cuda.synchronize()
        assert np.isfinite(a.cpu().numpy()).all() and float(a[-1].abs().max()) > 0
        return torch.equal(a, b)

    # plain
    dm.model.prepare_time_table(25)
    dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
    p = _raw_params(dm, B, steps, arrays)
    ctx = dm.model.ctx()
    s = _lib.current_stream()
    assert chains(lambda o: _lib.check(lib.ramp_sample(ctx, C.byref(p), _lib.ptr(noise), _lib.ptr(o), None, s)),
                  lambda o: _lib.check(lib.ramp_sample_mcmc(ctx, C.byref(p), C.byref(mp0), None, None, _lib.ptr(noise), None, None, _lib.ptr(o), None,
                                                            None, s)))
    # many scenes, composed: the tables of the Python layer, the raw entries
    scenes = [[dev(synth.make_cloud(5, 64, 2, seed=31))], [dev(synth.make_cloud(4, 64, 2, seed=32 + k)) for k in range(3)]]
    job, guid, hc, Bc = dm._prepare_composed_job(scenes, [_hc(), _hc()], [1, 2], None, None)
    assert Bc == B
    pc = _raw_params(dm, B, steps, arrays, hard=False)
    dm._fill_hard(pc, arrays, hc, B)
    pc.n_rp, pc.w0, pc.w1 = guid["n_rp"], 0.0, 0.0
    rows = _lib.RampGuidanceRows(); rows.n_rp, rows.row_weight = guid["n_rp"], _lib.ptr(guid["row_weight"])
    batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(job["traj_scene"])
    assert chains(lambda o: _lib.check(lib.ramp_sample_composed(ctx, C.byref(pc), C.byref(rows), C.byref(batch), _lib.ptr(noise), _lib.ptr(o), None, s)),
                  lambda o: _lib.check(lib.ramp_sample_mcmc(ctx, C.byref(pc), C.byref(mp0), C.byref(rows), C.byref(batch), _lib.ptr(noise), None, None,
                                                            _lib.ptr(o), None, None, s)))
    job2, hc2, B2 = dm._prepare_scene_job([dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))], [_hc(), _hc()], [1, 2])
    ps = _raw_params(dm, B, steps, arrays, hard=False)
    dm._fill_hard(ps, arrays, hc2, B)
    batch2 = _lib.RampSceneBatch(); batch2.n_scenes, batch2.traj_scene = 2, _lib.ptr(job2["traj_scene"])
    assert chains(lambda o: _lib.check(lib.ramp_sample_scenes(ctx, C.byref(ps), C.byref(batch2), _lib.ptr(noise), _lib.ptr(o), None, s)),
                  lambda o: _lib.check(lib.ramp_sample_mcmc(ctx, C.byref(ps), C.byref(mp0), None, C.byref(batch2), _lib.ptr(noise), None, None,
                                                            _lib.ptr(o), None, None, s)))


# ------------------------------------------------------------------------------------------------ 7: many-scene and composed jobs
def test_composed_many_scene_job_rows_follow_their_own_scene():
    """Two scenes with 1 and 3 obstacle sets, n_samples (2, 3), MALA with K = 1 on three iterations: every scene's trajectories against that
    scene's OWN composed job on the same draws, as the existing ragged-job test compares (1e-4 on the states: the jobs differ in rows per
    trajectory, hence in chunking and calibration, so bit equality is not the rule there), and its accept flags equal."""
    dm = _static(25, max_rows=24)
    scenes = [[dev(synth.make_cloud(5, 64, 2, seed=500))], [dev(synth.make_cloud(4 + k, 64, 2, seed=510 + k)) for k in range(3)]]
    ns = [2, 3]
    noise = synth.make_noise((26, 5, 48, 4), seed=78)
    K = [1 if j in (3, 12, 20) else 0 for j in range(25)]
    z = synth.make_noise((3, 5, 48, 4), seed=79)
    u = _uniforms((3, 5), 80)

    def run(sc, counts, sl):
        mc = dict(kind="mala", steps=K, step_scale=0.5, noise=dev(z[:, sl]), u=dev(u[:, sl]))
        with NoiseInjector(list(noise[:, sl])):
            chain, _ = dm.run_inference_composed(sc, [_hc() for _ in sc], n_samples=counts, return_chain=True, horizon=48,
                                                 noise_std_extra_schedule_fn=lambda x: 0.5, mcmc=mc)
        return chain.cpu().numpy(), dm.last_mcmc["accept"].numpy()

    mixed, fl = run(scenes, ns, slice(0, 5))
    assert fl.shape == (3, 5) and np.isfinite(mixed).all() and 0 < fl.sum() < fl.size, fl
    b = 0
    for i, n in enumerate(ns):
        own, ofl = run([scenes[i]], n, slice(b, b + n))
        d = float(np.abs(mixed[:, b:b + n] - own).max())
        print(f"composed MALA job, scene {i}: vs its own job {d:.2e}, flags {fl[:, b:b + n].tolist()} / {ofl.tolist()}")
        assert np.array_equal(fl[:, b:b + n], ofl)
        assert d < 1e-4
        b += n


# ------------------------------------------------------------------------------------------------ 8: Philox
def philox_mcmc_draws(seed, offset, n_steps, K, B, HS, sample0=0, total=None):
    """numpy replica of the documented layout (ramp_sample_mcmc in ramp_hip.h): the inner steps' normals (K, B, HS) and uniforms (K, B)."""
    total = total or B
    z_all, _ = util.philox_normal(seed, offset, (n_steps + 1 + K) * total * HS)
    z = z_all.reshape(n_steps + 1 + K, total, HS)[n_steps + 1:, sample0:sample0 + B]
    g0 = (n_steps + 1 + K) * total * HS // 4
    _, r = util.philox_normal(seed, offset + g0, 4 * K * total)
    r0 = r.reshape(K * total, 4)[:, 0].reshape(K, total)[:, sample0:sample0 + B]
    uu = ((r0 >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return z, uu, z_all.reshape(n_steps + 1 + K, total, HS)[:n_steps + 1, sample0:sample0 + B]


def test_philox_job_equals_the_injected_job_and_shards_reproduce_it():
    """noise_mode 1 against noise_mode 0 fed the numbers of the documented layout: the numpy replica gives the uniforms exactly and the
    normals within its allowance (2e-5); a free-running chain amplifies such differences, so the injected job is fed the device stream's own
    elements at the replica's positions and must then equal the Philox job bit for bit, flags included.  Two half-jobs with set_noise_shard
    reproduce the whole job's rows and flags bit for bit."""
    B = 4
    K = [1 if j in (2, 10) else 0 for j in range(25)]
    mc = dict(kind="mala", steps=K, step_scale=0.5)      # (proposals are rejected too: the flags and the chain then depend on the uniforms)
    cloud = dev(synth.make_cloud(6, 64, 2, seed=3))

    def run(dm, n, mcd, inject=None):
        kw = dict(n_samples=n, horizon=48, return_chain=True, obstacle_pts=cloud, noise_std_extra_schedule_fn=lambda x: 0.5, mcmc=mcd)
        if inject is None:
            chain = dm.run_inference(None, _hc(), **kw)
        else:
            with NoiseInjector(list(inject)):
                chain = dm.run_inference(None, _hc(), **kw)
        return chain.cpu().numpy(), dm.last_mcmc["accept"].numpy()

    dmp = _static(25, noise_source="philox", noise_seed=77)
    whole, wf = run(dmp, B, mc)
    seed, offset, _ = dmp.last_philox
    assert dmp._philox_offset == offset + (26 + 2) * B * 192 // 4 + 2 * B
    z, uu, main = philox_mcmc_draws(seed, offset, 25, 2, B, 192)
    # the device's own stream at the documented positions: within the replica's allowance for normals (2e-5: numpy's float32 log / sin / cos
    # against the device's, as the existing Philox test allows); the uniforms are a function of one word, hence exact
    dnz = torch.empty((26 + 2) * B * 192, device="cuda")
    _lib.check(_lib.load().ramp_philox_normal(_lib.ptr(dnz), dnz.numel(), seed, offset, None), "ramp_philox_normal")
    dnz = dnz.reshape(28, B, 48, 4)
    assert np.abs(dnz[26:].cpu().numpy().reshape(2, B, 192) - z).max() < 2e-5 and np.abs(dnz[:26].cpu().numpy().reshape(26, B, 192) - main).max() < 2e-5
    dmi = _static(25)
    inj, jf = run(dmi, B, dict(mc, noise=dnz[26:].contiguous(), u=dev(uu)), inject=dnz[:26])
    print(f"philox MALA job vs the same draws injected: {np.abs(whole - inj).max():.2e}; flags {wf.tolist()}")
    assert 0 < wf.sum() < wf.size, wf      # both outcomes: the uniforms at the documented positions decide
    assert np.array_equal(wf, jf)
    assert np.array_equal(whole, inj)
    # shards: in bf16x6 a row's arithmetic does not depend on the batch around it (no delayed scales recorded on the batch; the existing
    # sharded test claims 2e-4 for fp16x3 for that reason), so two half-jobs equal the whole job's rows and flags bit for bit.  A larger step
    # so that proposals are rejected too
    mcs = mc
    whole_b, wfb = run(_static(25, noise_source="philox", noise_seed=77, gemm_mode="bf16x6"), B, mcs)
    assert 0 < wfb.sum() < wfb.size, wfb
    for s0 in (0, 2):
        dms = _static(25, noise_source="philox", noise_seed=77, gemm_mode="bf16x6")
        dms.set_noise_shard(s0, B)
        part, pf = run(dms, 2, mcs)
        assert np.array_equal(pf, wfb[:, s0:s0 + 2]), (pf, wfb)
        assert np.array_equal(part, whole_b[:, s0:s0 + 2]), float(np.abs(part - whole_b[:, s0:s0 + 2]).max())


# ------------------------------------------------------------------------------------------------ 9: stale graphs
def test_a_job_never_replays_a_stale_graph():
    """Job A (step_scale 0.05) then job B (0.2) at the same shape on one context: B equals B on a fresh context; likewise after a changed
    n_inner list."""
    cloud = dev(synth.make_cloud(6, 64, 2, seed=3))
    noise = synth.make_noise((26, 3, 48, 4), seed=5)
    z = synth.make_noise((3, 3, 48, 4), seed=6)
    u = _uniforms((3, 3), 7)

    def run(dm, scale, K):
        n = int(sum(K))
        mc = dict(kind="mala", steps=K, step_scale=scale, noise=dev(z[:n]), u=dev(u[:n]))
        with NoiseInjector(list(noise)):
            c = dm.run_inference(None, _hc(), n_samples=3, horizon=48, return_chain=True, obstacle_pts=cloud,
                                 noise_std_extra_schedule_fn=lambda x: 0.5, mcmc=mc)
        return c.cpu().numpy(), dm.last_mcmc["accept"].numpy()

    K2 = [1 if j in (1, 3) else 0 for j in range(25)]
    K3 = [1 if j in (1, 2, 3) else 0 for j in range(25)]
    dm = _static(25)
    a, _ = run(dm, 0.05, K2)
    b, bf = run(dm, 0.2, K2)
    c, cf = run(dm, 0.2, K3)
    fresh_b, fbf = run(_static(25), 0.2, K2)
    fresh_c, fcf = run(_static(25), 0.2, K3)
    eager_b, ebf = run(_static(25, use_graph=False), 0.2, K2)      # use_graph=False shares the entry: the same bits without a capture
    assert np.array_equal(b, eager_b) and np.array_equal(bf, ebf)
    assert 0 < bf.sum() + cf.sum() < bf.size + cf.size, (bf, cf)      # both outcomes among the compared flags
    assert not np.array_equal(a, b)
    assert np.array_equal(b, fresh_b) and np.array_equal(bf, fbf)
    assert np.array_equal(c, fresh_c) and np.array_equal(cf, fcf)


# ------------------------------------------------------------------------------------------------ 10: refusals of the C entry
def test_refusals_through_the_raw_abi():
    """Every refusal of ramp_sample_mcmc is a host check made before anything launches: non-zero, the entry's name in ramp_last_error, the
    launch counter untouched and the output buffers as they were."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = _static(25)
    B, steps = 2, [24, 12, 0]
    dm.model.prepare_time_table(25)
    dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
    arrays = _HostArrays()
    noise = dev(synth.make_noise((4, B, 48, 4), seed=8))
    z = dev(synth.make_noise((3, B, 48, 4), seed=9)); u = dev(_uniforms((3, B), 10))
    sig = [float(dm.sqrt_one_minus_alphas_cumprod[t]) for t in steps]
    ctx, s = dm.model.ctx(), _lib.current_stream()
    out = torch.full((B, 48, 4), 7.0, device="cuda")
    rw = dev(np.ones((B, 3), np.float32))

    def refused(p, mp, g=None, zz=z, uu=u):
        n0 = dm.model.launch_count()
        rc = lib.ramp_sample_mcmc(ctx, C.byref(p), C.byref(mp), C.byref(g) if g is not None else None, None, _lib.ptr(noise), _lib.ptr(zz),
                                  _lib.ptr(uu), None, _lib.ptr(out), None, s)
        msg = lib.ramp_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "ramp_sample_mcmc" in msg, (rc, msg)
        assert dm.model.launch_count() == n0 and float(out.min()) == 7.0 and float(out.max()) == 7.0
        return msg

    ok = [1, 1, 1]
    p = _raw_params(dm, B, steps, arrays)
    px0 = _raw_params(dm, B, steps, arrays); px0.predict_x0 = 1
    assert "predict_x0" in refused(px0, _mcmc_params(arrays, 2, ok, [0.01] * 3, sig))
    assert "n_inner" in refused(p, _mcmc_params(arrays, 2, [1, 17, 1], [0.01] * 3, sig))
    assert "n_inner" in refused(p, _mcmc_params(arrays, 1, [1, -1, 1], [0.01] * 3, sig))
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        assert "step_size" in refused(p, _mcmc_params(arrays, 2, ok, [0.01, bad, 0.01], sig))
    assert "mcmc_noise" in refused(p, _mcmc_params(arrays, 1, ok, [0.01] * 3, sig), zz=None)
    assert "mcmc_u" in refused(p, _mcmc_params(arrays, 2, ok, [0.01] * 3, sig), uu=None)
    assert "kind" in refused(p, _mcmc_params(arrays, 3, ok, [0.01] * 3, sig))
    g = _lib.RampGuidanceRows(); g.n_rp, g.row_weight = 3, _lib.ptr(rw)
    assert "n_rp" in refused(p, _mcmc_params(arrays, 2, ok, [0.01] * 3, sig), g=g)
    # a step size that is not used (n_inner 0 there) is not looked at; and ULA needs no uniforms
    mp = _mcmc_params(arrays, 1, [1, 0, 1], [0.01, float("nan"), 0.01], sig)
    _lib.check(lib.ramp_sample_mcmc(ctx, C.byref(p), C.byref(mp), None, None, _lib.ptr(noise), _lib.ptr(z), None, None, _lib.ptr(out), None, s),
               "ramp_sample_mcmc")
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all() and float(out.max()) != 7.0


def test_python_refusals_on_the_device():
    """predict_epsilon=False through run_inference, and injected inner draws on a model that draws its own noise, are refused with a message
    (the dynamic planner, a custom sample_fn and the table checks: test_mcmc_host.py)."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=8)
    dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=25, predict_epsilon=False, sampler="ddpm").eval().to("cuda")
    with pytest.raises(NotImplementedError, match="predict_epsilon"):
        dm.run_inference(None, _hc(), n_samples=1, obstacle_pts=dev(synth.make_cloud(6, 64, 2, seed=3)), mcmc=dict(kind="ula", steps=1))
    dp = _static(25, noise_source="philox")
    with pytest.raises(ValueError, match="noise_source='philox'"):
        dp.run_inference(None, _hc(), n_samples=1, obstacle_pts=dev(synth.make_cloud(6, 64, 2, seed=3)),
                         mcmc=dict(kind="ula", steps=1, noise=torch.zeros(25, 1, 48, 4)))
