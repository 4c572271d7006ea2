"""The warm start inside the oracle's loops, and the inputs the free-running warm-start tests share (test_warm_host.py checks their
conditions on the CPU, test_gpu_warm.py runs the HIP job on them).

``WarmOracle`` is ``oracle.ramp_oracle.SamplerOracle`` with the start state and the hold of ``ramp_amd.warm`` at the places
include/ramp_hip.h gives: init, then hard conditioning, is chain block 0 and x_init; after every iteration's hard conditioning the rows that
have not started yet are x_init again."""
import numpy as np

from oracle import ramp_oracle as O
from ramp_amd import synth
from ramp_amd.spec import UNET_DIM_MULTS
from ramp_amd.warm import straight_line_prior, warm_hold_reference, warm_init_reference, warm_tables  # noqa: F401

SCHED_NAMES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
               "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_variance",
               "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


class WarmOracle(O.SamplerOracle):
    """``warm`` = dict(prior (B, H, S), J, j0 (B), t_row (B)) of ``warm_tables``, or None (the plain loops).  ``noise`` holds the blocks of
    the job's own iterations J .. n - 1 (block 0 the start draw)."""

    def _start(self, noise0, hard_conds, warm):
        dt, s = self.dt, self.sched
        if warm is None:
            x = noise0.astype(dt).copy()
        else:
            x = warm_init_reference(noise0, warm["prior"], warm["t_row"], s["sqrt_alphas_cumprod"], s["sqrt_one_minus_alphas_cumprod"], dtype=dt)
        return O.apply_hard_conditioning(x, hard_conds)

    @staticmethod
    def _hold(x, x_init, warm, j):
        return x if warm is None else warm_hold_reference(x, x_init, warm["j0"], j)

    def ddpm(self, noise, hard_conds, latent, warm=None, noise_scale=0.5, **kw):
        s, dt = self.sched, self.dt
        x = self._start(noise[0], hard_conds, warm)
        x_init, chain = x.copy(), [x.copy()]
        ts = list(reversed(range(self.T)))[(warm["J"] if warm else 0):]
        for j, t in enumerate(ts):
            e = self.eps_cfg(x, t, latent)
            _, mean = self.x0_mean(x, e, t)
            z = noise[1 + j].astype(dt) if t != 0 else np.zeros_like(x)
            std = np.exp(dt(0.5) * s["posterior_log_variance_clipped"][t])
            x = O.apply_hard_conditioning((mean + std * z * dt(noise_scale)).astype(dt), hard_conds)
            x = self._hold(x, x_init, warm, j)
            chain.append(x.copy())
        return np.stack(chain)

    def ddim(self, noise0, hard_conds, latent, warm=None, K=5, **kw):
        s, dt = self.sched, self.dt
        x = self._start(noise0, hard_conds, warm)
        x_init, chain, ac = x.copy(), [x.copy()], s["alphas_cumprod"]
        ts = list(O.ddim_timesteps(self.T, K))[(warm["J"] if warm else 0):]
        for j, t in enumerate(ts):
            prev = t - self.T // K
            a_t, a_prev = ac[t], (ac[prev] if prev >= 0 else dt(1.0))
            e = self.eps_cfg(x, int(t), latent)
            x0, _ = self.x0_mean(x, e, int(t))
            e2 = (x - np.sqrt(a_t) * x0) / np.sqrt(dt(1) - a_t)
            x = O.apply_hard_conditioning((np.sqrt(a_prev) * x0 + np.sqrt(dt(1) - a_prev) * e2).astype(dt), hard_conds)
            x = self._hold(x, x_init, warm, j)
            chain.append(x.copy())
        return np.stack(chain)


# ------------------------------------------------------------------------------------------------ the free-running jobs' inputs
CHAIN_LEVELS = {"ddim": [None, 12, 5], "ddpm": [None, 1, 0]}      # DDIM, T = 25, K = 5: j0 = [0, 2, 3]; DDPM, T = 3 cosine: j0 = [0, 1, 2]
CHAIN_J0 = {"ddim": [0, 2, 3], "ddpm": [0, 1, 2]}
NOISE_SEED = 700
_CHAIN = {}


def hcn(S=4):
    return synth.default_hard_conds(S, 8)


def chain_sched(kind):
    """(T, the model's own schedule buffers, its iteration list): cosine for the 3-step DDPM job (the exponential schedule ends at beta = 1)."""
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    T = 3 if kind == "ddpm" else 25
    dm = StaticGaussianDiffusionModel(model=TemporalUnetInference(n_support_points=8, state_dim=4), n_diffusion_steps=T,
                                      variance_schedule="cosine" if kind == "ddpm" else "exponential", predict_epsilon=True, sampler=kind)
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    return T, {k: getattr(dm, k).numpy() for k in SCHED_NAMES}, steps


def chain_inputs(kind, seed=NOISE_SEED):
    """noise (n + 1, 3, 8, 4), the scene cloud, the hard conditions at waypoints 0 and 7, and the prior: the line between them plus
    0.05 N(0, 1)."""
    T, sched, steps = chain_sched(kind)
    n = len(steps)
    hc = hcn(4)
    line = np.linspace(hc[0].astype(np.float64), hc[7].astype(np.float64), 8)
    prior = (line[None] + 0.05 * np.random.default_rng(1700).standard_normal((3, 8, 4))).astype(np.float32)
    return synth.make_noise((n + 1, 3, 8, 4), seed=seed), synth.make_cloud(6, 64, 2, seed=3), hc, prior


def oracle_chains(kind):
    """float64 warm and cold chains and the float32 warm chain of the free-running test, once per process (seconds on the CPU)."""
    if kind not in _CHAIN:
        from test_gpu_shapes import shape_weights
        T, sched, steps = chain_sched(kind)
        noise, scene, hc, prior = chain_inputs(kind)
        tab = warm_tables(CHAIN_LEVELS[kind], steps, T=T)
        assert tab["J"] == 0 and tab["j0"].tolist() == CHAIN_J0[kind], tab
        warm = dict(tab, prior=prior)
        out = {"tab": tab}
        for name, dtype, w in (("w64", np.float64, warm), ("c64", np.float64, None), ("w32", np.float32, warm)):
            uo = O.UNetOracle(shape_weights(4, 8, False, 0, 16), 4, 8, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            so = WarmOracle(uo, T, 2.0, dtype=dtype, sched=sched)
            lat = uo.encode_scene(scene)
            out[name] = so.ddpm(noise, hc, lat, warm=w) if kind == "ddpm" else so.ddim(noise[0], hc, lat, warm=w, K=5)
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """(bar, the float32 oracle's distance, the smallest distance over the rows WITH a prior between the warm and the cold float64 final
    state): what the inputs must satisfy."""
    c = oracle_chains(kind)
    bar = 1e-4 * float(np.abs(c["w64"]).max())
    rows = [b for b, lv in enumerate(CHAIN_LEVELS[kind]) if lv is not None]
    moved = min(float(np.abs(c["w64"][-1][b] - c["c64"][-1][b]).max()) for b in rows)
    return bar, float(np.abs(c["w32"] - c["w64"]).max()), moved
