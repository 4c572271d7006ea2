"""Host-side mirrors of the reference's diffusion wrappers over the HIP C ABI.

  StaticGaussianDiffusionModel   mpd/models/diffusion_models/diffusion_model_static.py:21-463
  GaussianDiffusionModel3d       mpd/models/diffusion_models/diffusion_model_3d.py:19-344

Same constructor kwargs, schedule buffers (computed with the same torch expressions, so they are
bitwise the reference's), ``run_inference`` / ``conditional_sample`` / ``warmup`` signatures and
return shapes.  The reverse-diffusion loop itself — score network, CFG combine, x0 clamp,
posterior / DDIM update, noise, hard conditioning, APF — runs inside ``ramp_sample`` (one
hipGraph for the whole loop); noise is drawn here with ``torch.randn`` / ``torch.randn_like``
in the reference's call order so that seeding / patching those functions behaves identically.

Quirks surfaced as kwargs with the reference's hard-coded values as defaults (SURVEY.md App. C,
Q5/Q6): ``sampler`` ('ddim' is the reference default, ``self.ddim = True``), ``cfg_weight``,
``apf_*``.  The 3-D wrapper is batched here: every sample gets its own cond/uncond pair (the
reference indexes rows 0/1 of the output and is only valid for n_samples == 1, Q2).
"""
from __future__ import annotations

import warnings

import ctypes as C
from copy import copy
from typing import Dict, Optional

import numpy as np
import torch
from torch import nn

from . import _lib
from .sample_functions import apply_hard_conditioning, ddpm_sample_fn, extract  # noqa: F401


def exponential_beta_schedule(n_diffusion_steps, beta_start=1e-4, beta_end=1.0):
    """helpers.py:40-46, same torch expression order."""
    x = torch.linspace(0, n_diffusion_steps, n_diffusion_steps)
    beta_start = torch.tensor(beta_start, dtype=torch.float32)
    beta_end = torch.tensor(beta_end, dtype=torch.float32)
    a = 1 / n_diffusion_steps * torch.log(beta_end / beta_start)
    return beta_start * torch.exp(a * x)


def cosine_beta_schedule(n_diffusion_steps, s=0.008, a_min=0, a_max=0.999):
    """helpers.py:26-37."""
    steps = n_diffusion_steps + 1
    x = np.linspace(0, steps, steps)
    ac = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = 1 - (ac[1:] / ac[:-1])
    return torch.tensor(np.clip(betas, a_min=a_min, a_max=a_max), dtype=torch.float32)


def make_timesteps(batch_size, i, device):
    return torch.full((batch_size,), i, device=device, dtype=torch.long)


class _HostArrays:
    """Owns what a params struct points at for the length of a job: the ctypes arrays it hands out, any tensor given to ``keep``."""

    def __init__(self):
        self._keep = []

    def keep(self, obj):
        self._keep.append(obj)
        return obj

    def f32(self, values):
        return C.cast(self.keep((C.c_float * len(values))(*[float(v) for v in values])), _lib.c_f32p)

    def i32(self, values):
        return C.cast(self.keep((C.c_int32 * len(values))(*[int(v) for v in values])), _lib.c_i32p)


DDIM_FIELDS = ('sqrt_recip', 'sqrt_recipm1', 'sqrt_a_t', 'sqrt_1m_a_t', 'sqrt_a_prev', 'dir_coef')


def mcmc_tables(mcmc: dict, steps, alphas_cumprod) -> dict:
    """The per-iteration tables of a Langevin refinement (``mcmc=`` of run_inference*; ramp_mcmc_params) for the job whose
    iterations evaluate the network timesteps ``steps`` (the DDPM or the DDIM list), host data only.

      kind        'ula' | 'mala'
      steps       K inner steps on every iteration, or one count per iteration (0 .. 16)
      step_scale  c: eta_t = c (1 - alphas_cumprod[t]), so a = eta / sigma_t = c sigma_t and the noise scale is sigma_t sqrt(2 c)
      step_size   None, or one eta per iteration (overrides step_scale)
      t_range     (lo, hi): only iterations with lo <= t <= hi refine (K_j = 0 outside)
      noise, u    optional injected draws, (sum K, B, H, S) normals and (sum K, B) uniforms in (0, 1), for a job whose loop noise is
                  injected too (``noise_source='torch'``); None: ``torch.randn`` / ``torch.rand`` behind the loop's own draws

    Returns ``{'kind': 1 | 2, 'n_inner': [...], 'step_size': [...], 'sigma': [...], 'total': sum K}``; sigma_t = sqrt(1 - alphas_cumprod[t])."""
    if not isinstance(mcmc, dict):
        raise TypeError("mcmc= takes a dict(kind=, steps=, step_scale= | step_size=, t_range=)")
    unknown = set(mcmc) - {'kind', 'steps', 'step_scale', 'step_size', 't_range', 'noise', 'u'}
    if unknown:
        raise ValueError(f"mcmc=: unknown keys {sorted(unknown)}")
    kind = mcmc.get('kind', 'mala')
    if kind not in _lib.MCMC_KINDS:
        raise ValueError(f"mcmc kind must be 'ula' or 'mala'; got {kind!r}")
    n = len(steps)
    ac = np.asarray(alphas_cumprod.detach().cpu().numpy() if torch.is_tensor(alphas_cumprod) else alphas_cumprod, dtype=np.float64)
    K = mcmc.get('steps', 1)
    K = [int(K)] * n if np.isscalar(K) else [int(k) for k in K]
    if len(K) != n:
        raise ValueError(f"mcmc steps: {len(K)} entries for {n} iterations")
    if 't_range' in mcmc and mcmc['t_range'] is not None:
        lo, hi = mcmc['t_range']
        K = [k if lo <= t <= hi else 0 for k, t in zip(K, steps)]
    if any(k < 0 or k > _lib.MCMC_MAX_INNER for k in K):
        raise ValueError(f"mcmc steps must lie in 0 .. {_lib.MCMC_MAX_INNER} per iteration")
    sigma = [float(np.sqrt(1.0 - ac[t])) for t in steps]
    if mcmc.get('step_size') is not None:
        eta = [float(e) for e in mcmc['step_size']]
        if len(eta) != n:
            raise ValueError(f"mcmc step_size: {len(eta)} entries for {n} iterations")
    else:
        c = float(mcmc.get('step_scale', 0.1))
        eta = [c * float(1.0 - ac[t]) for t in steps]
    for k, e in zip(K, eta):
        if k > 0 and not (np.isfinite(e) and e > 0):
            raise ValueError("mcmc step sizes must be positive and finite wherever inner steps run")
    return {'kind': _lib.MCMC_KINDS[kind], 'n_inner': K, 'step_size': eta, 'sigma': sigma, 'total': int(sum(K))}


GUIDE_PRIM_KEYS = {'boxes', 'spheres', 'margin', 'band', 'w_prim', 'n_sub'}      # the swept box and sphere terms (ramp_prim_guide)
GUIDE_KEYS = {'cloud', 'clouds', 'radius', 'w_obs', 'w_smooth', 'w_acc', 'step', 'n_steps', 't_start', 'max_norm', 'scale_by_variance',
              'team'} | GUIDE_PRIM_KEYS


def guide_has_prims(cost_guide) -> bool:
    """True when a ``cost_guide=`` dict carries any key of the swept box and sphere terms."""
    return isinstance(cost_guide, dict) and bool(GUIDE_PRIM_KEYS & set(cost_guide))


def guide_has_team(cost_guide) -> bool:
    """True when a ``cost_guide=`` dict carries the ``team=`` key (rows coupled in teams of robots, ramp_team_guide)."""
    return isinstance(cost_guide, dict) and cost_guide.get('team') is not None


def guide_tables(cost_guide: dict, steps, posterior_variance) -> dict:
    """The host tables of a job's cost-gradient guidance (``cost_guide=`` of run_inference*; ramp_cost_guide) for the job whose iterations
    evaluate the network timesteps ``steps`` (the DDPM or the DDIM list), host data only -- the clouds are not looked at here.

      cloud | clouds     the guide's obstacle points, (P, d) or (No, Np, d), d = 2 or 3; ``clouds``: one per scene of a scene / composed job
      radius             r of the obstacle term (required, > 0, unless w_obs = 0)
      w_obs, w_smooth, w_acc   weights of the three terms (default 1, 0, 0)
      step               step size (required), or one per iteration
      n_steps            guide iterations per loop iteration (default 1), or one count per iteration (0 .. 16)
      t_start            only iterations with t < t_start are guided (default inf: all)
      max_norm           clip of the trajectory's gradient norm, 0 = off (default)
      scale_by_variance  multiply the step of iteration j by posterior_variance[t_j] (default False)
      boxes, spheres     the swept primitive term (ramp_prim_guide): per scene a ``(centres, sizes)`` / ``(centres, radii)`` pair or None --
                         one entry for a plain job, the per-scene list ``clearance.trajectory_clearance`` takes for a scene / composed job;
                         ``cloud=None`` with ``w_obs=0`` is the primitives-only guide
      margin, band, w_prim, n_sub   the robot margin (default 0), the hinge's band (required with primitives), the term's weight (default 1)
                         and the samples per segment, 1 .. 8 (default 4)
      team               dict(size=A, radius=r_t, w=1.0): the rows of the job are teams of A robots that share a scene, row b agent b % A of
                         team b / A, coupled through the separation term of ``ramp_team_guide`` (``ramp_amd.team.team_scalars``)

    Returns ``{'n_guide': [...], 'step': [...], 'radius', 'w_obs', 'w_smooth', 'w_acc', 'max_norm', 'total': sum n_guide}`` and, with any
    of the primitive keys, ``'prim': {'margin', 'band', 'w_prim', 'n_sub'}``; with ``team=``, ``'team': {'size', 'radius', 'w'}``."""
    if not isinstance(cost_guide, dict):
        raise TypeError("cost_guide= takes a dict(cloud= | clouds=, radius=, step=, w_obs=, w_smooth=, w_acc=, n_steps=, t_start=, max_norm=, "
                        "scale_by_variance=)")
    unknown = set(cost_guide) - GUIDE_KEYS
    if unknown:
        raise ValueError(f"cost_guide=: unknown keys {sorted(unknown)}")
    if ('cloud' in cost_guide) == ('clouds' in cost_guide):
        raise ValueError("cost_guide=: exactly one of cloud= and clouds=")
    n = len(steps)
    out = {'radius': float(cost_guide.get('radius', 0.0)), 'w_obs': float(cost_guide.get('w_obs', 1.0)),
           'w_smooth': float(cost_guide.get('w_smooth', 0.0)), 'w_acc': float(cost_guide.get('w_acc', 0.0)),
           'max_norm': float(cost_guide.get('max_norm', 0.0))}
    if not all(np.isfinite(v) for v in out.values()):
        raise ValueError("cost_guide=: radius, w_obs, w_smooth, w_acc and max_norm must be finite")
    if out['w_obs'] != 0.0 and not out['radius'] > 0.0:
        raise ValueError("cost_guide=: radius must be positive where w_obs != 0")
    if 'step' not in cost_guide:
        raise ValueError("cost_guide=: step= is required")
    K = cost_guide.get('n_steps', 1)
    K = [int(K)] * n if np.isscalar(K) else [int(k) for k in K]
    if len(K) != n:
        raise ValueError(f"cost_guide n_steps: {len(K)} entries for {n} iterations")
    if any(k < 0 or k > _lib.GUIDE_MAX_STEPS for k in K):
        raise ValueError(f"cost_guide n_steps must lie in 0 .. {_lib.GUIDE_MAX_STEPS} per iteration")
    t_start = float(cost_guide.get('t_start', float('inf')))
    if np.isnan(t_start):
        raise ValueError("cost_guide=: t_start is NaN")
    K = [k if t < t_start else 0 for k, t in zip(K, steps)]
    st = cost_guide['step']
    st = [float(st)] * n if np.isscalar(st) else [float(v) for v in st]
    if len(st) != n:
        raise ValueError(f"cost_guide step: {len(st)} entries for {n} iterations")
    if cost_guide.get('scale_by_variance', False):
        pv = np.asarray(posterior_variance.detach().cpu().numpy() if torch.is_tensor(posterior_variance) else posterior_variance, dtype=np.float64)
        st = [v * float(pv[t]) for v, t in zip(st, steps)]
    if not all(np.isfinite(v) for v in st):
        raise ValueError("cost_guide=: step sizes must be finite")
    out.update(n_guide=K, step=st, total=int(sum(K)))
    if guide_has_prims(cost_guide):
        from .guide import prim_scalars
        if cost_guide.get('boxes') is None and cost_guide.get('spheres') is None:
            raise ValueError("cost_guide=: margin / band / w_prim / n_sub need boxes= or spheres=")
        out['prim'] = prim_scalars(cost_guide.get('margin', 0.0), cost_guide.get('band'), cost_guide.get('w_prim', 1.0), cost_guide.get('n_sub', 4))
    if guide_has_team(cost_guide):
        from .team import team_scalars
        if guide_has_prims(cost_guide):
            raise NotImplementedError("cost_guide=: team= with boxes= / spheres= is not served (ramp_sample_guided_prims takes no team)")
        out['team'] = team_scalars(cost_guide['team'])
    return out


RESAMPLE_KEYS = {'every', 'flags', 't_start', 'lambda_', 'ess_frac', 'cloud', 'clouds', 'radius', 'w_obs', 'w_smooth', 'w_acc', 'u'}


def resample_tables(resample: dict, steps) -> dict:
    """The host tables of a job's resampling events (``resample=`` of run_inference*; ramp_resample_params) for the job whose iterations
    evaluate the network timesteps ``steps``, host data only -- clouds and uniforms are not looked at here.

      every | flags      an event on every ``every``-th iteration (j + 1 a multiple of it), or one 0 / 1 flag per iteration
      t_start            only iterations with t < t_start hold an event (default inf: all)
      lambda_            the potential's inverse temperature (required), or one per iteration
      ess_frac           a group resamples when ESS < ess_frac * size, in [0, 2] (default 0.5; 0 never, above 1 always)
      cloud | clouds     the cost's obstacle points as in ``cost_guide=``; ``clouds``: one per scene of a scene / composed job
      radius, w_obs, w_smooth, w_acc   the cost c = w_obs C_obs + w_smooth C_smooth + w_acc C_acc (defaults 0, 1, 0, 0)
      u                  optional (n_events, n_groups) uniforms in (0, 1) of a job whose noise is injected

    Returns ``{'resample': [...], 'lambda': [...], 'ess_frac', 'radius', 'w_obs', 'w_smooth', 'w_acc', 'events': [j, ...]}``."""
    if not isinstance(resample, dict):
        raise TypeError("resample= takes a dict(every= | flags=, t_start=, lambda_=, ess_frac=, cloud= | clouds=, radius=, w_obs=, w_smooth=, "
                        "w_acc=, u=)")
    unknown = set(resample) - RESAMPLE_KEYS
    if unknown:
        raise ValueError(f"resample=: unknown keys {sorted(unknown)}")
    if ('cloud' in resample) == ('clouds' in resample):
        raise ValueError("resample=: exactly one of cloud= and clouds=")
    if ('every' in resample) == ('flags' in resample):
        raise ValueError("resample=: exactly one of every= and flags=")
    n = len(steps)
    out = {'radius': float(resample.get('radius', 0.0)), 'w_obs': float(resample.get('w_obs', 1.0)),
           'w_smooth': float(resample.get('w_smooth', 0.0)), 'w_acc': float(resample.get('w_acc', 0.0))}
    if not all(np.isfinite(v) for v in out.values()):
        raise ValueError("resample=: radius, w_obs, w_smooth and w_acc must be finite")
    if out['w_obs'] != 0.0 and not out['radius'] > 0.0:
        raise ValueError("resample=: radius must be positive where w_obs != 0")
    if 'every' in resample:
        every = int(resample['every'])
        if every < 1:
            raise ValueError("resample=: every must be at least 1")
        flags = [1 if (j + 1) % every == 0 else 0 for j in range(n)]
    else:
        flags = [1 if int(f) else 0 for f in resample['flags']]
        if len(flags) != n:
            raise ValueError(f"resample flags: {len(flags)} entries for {n} iterations")
    t_start = float(resample.get('t_start', float('inf')))
    if np.isnan(t_start):
        raise ValueError("resample=: t_start is NaN")
    flags = [f if t < t_start else 0 for f, t in zip(flags, steps)]
    if sum(flags) > _lib.RESAMPLE_MAX_EVENTS:
        raise ValueError(f"resample=: {sum(flags)} events, at most {_lib.RESAMPLE_MAX_EVENTS}")
    if 'lambda_' not in resample:
        raise ValueError("resample=: lambda_= is required")
    lam = resample['lambda_']
    lam = [float(lam)] * n if np.isscalar(lam) else [float(v) for v in lam]
    if len(lam) != n:
        raise ValueError(f"resample lambda_: {len(lam)} entries for {n} iterations")
    if not all(np.isfinite(v) for v in lam):
        raise ValueError("resample=: lambda_ must be finite")
    ess_frac = float(resample.get('ess_frac', 0.5))
    if not (np.isfinite(ess_frac) and 0.0 <= ess_frac <= 2.0):
        raise ValueError("resample=: ess_frac must lie in [0, 2]")
    out.update(resample=flags, ess_frac=ess_frac, events=[j for j, f in enumerate(flags) if f])
    out['lambda'] = lam
    return out


class _GaussianDiffusionBase(nn.Module):
    _default_cfg_weight = 2.0

    def __init__(self, model=None, variance_schedule='exponential', n_diffusion_steps=100, clip_denoised=True,
                 predict_epsilon=False, loss_type='l2', context_model=None, compose=False, use_apf=False,
                 training=False, sampler: Optional[str] = None, cfg_weight: Optional[float] = None,
                 compose_weights=None, use_graph: bool = True, fp16_fallback: bool = True, noise_source: str = "torch",
                 noise_seed: int = 0, **kwargs):
        super().__init__()
        self.model = model
        self.fp16_fallback = fp16_fallback      # fp16x3 range guard tripped -> repeat the job in bf16x6 (else raise)
        self.range_fallbacks = 0                # jobs / replans the fp16x3 range guard sent to the bf16x6 kernels so far
        self.range_reruns = 0                   # jobs the guard flagged and that were repeated in fp16x3 (the flagged evaluation calibrating)
        self.fp16_rerun = True                  # False: a flagged job goes straight to the bf16x6 repeat (rounds 2-5)
        self.last_job_mode = None               # arithmetic of the last sampling job's RESULT: 'fp16x3', 'fp16x3-rerun', 'bf16x6', 'fp32'
        # "torch": the reference's torch.randn / randn_like draws (sample_functions.py:36; what the parity runs patch);
        # "philox": the job draws its noise INSIDE the captured graph (ramp_sample_params.noise_mode 1), stream
        # (noise_seed, running offset) -- host-replicable through ramp_philox_normal / tests.util.philox_normal
        if noise_source not in ("torch", "philox"):
            raise ValueError("noise_source must be 'torch' or 'philox'")
        self.noise_source = noise_source
        self.noise_seed = int(noise_seed)
        self._philox_offset = 0                 # groups of four elements consumed so far
        # several GPUs: this wrapper's batch is samples [sample0, sample0 + B) of a job of `total` trajectories; a philox job then
        # draws exactly the elements the unsharded job draws for those samples (set_noise_shard; ramp_sample_params.philox_sample0)
        self._philox_shard = None
        self.last_resample = None               # after a job with resample=: {'ancestors': (n_events, B) int32, 'ess': (n_events, n_groups), 'cost': (n_events, B), 'logw': (B,), 'group_first', 'events'}
        self.last_warm = None                   # after a job with warm_start=: {'J', 'j0': (B,) int32, 't_row': (B,) int32 (-1: no prior), 'steps': the iterations the job ran}
        self.last_mcmc = None                   # after a job with mcmc=: {'accept': (sum K, B) int32, 'rate': per iteration, 'n_inner': per iteration}
        self.context_model = context_model
        self.n_diffusion_steps = n_diffusion_steps
        self.ddim_num_inference_steps = 8 if (compose and use_apf) else 5      # diffusion_model_static.py:40
        self.compose = compose
        self.APF = use_apf
        self.energy_mode = True
        self.training = training
        self.state_dim = self.model.state_dim
        self.use_graph = use_graph
        self.cfg_weight = self._default_cfg_weight if cfg_weight is None else float(cfg_weight)
        self.compose_weights = tuple(compose_weights) if compose_weights is not None else self._default_compose
        self.ddim = self._default_ddim if sampler is None else (sampler == 'ddim')
        # predict_epsilon=False is the reference constructor's default (diffusion_model_static.py:28): the guidance-combined
        # network output is then x0 itself (predict_start_from_noise, :109-118); the inference configs pass True (base_config.py:26)
        if variance_schedule == 'cosine':
            betas = cosine_beta_schedule(n_diffusion_steps, s=0.008, a_min=0, a_max=0.999)
        elif variance_schedule == 'exponential':
            betas = exponential_beta_schedule(n_diffusion_steps, beta_start=1e-4, beta_end=1.0)
        else:
            raise NotImplementedError
        alphas = 1. - betas
        alphas_cumprod = torch.cumprod(alphas, axis=0)
        alphas_cumprod_prev = torch.cat([torch.ones(1), alphas_cumprod[:-1]])
        self.clip_denoised = clip_denoised
        self.predict_epsilon = predict_epsilon
        # the denoising loss (loss / p_losses): 'l2' (the reference default) and 'l1' are served, helpers.py:71-100; anything else is
        # refused when a loss is asked for, not here -- the sampling configs pass whatever their training run used
        self.loss_type = loss_type
        self.register_buffer('betas', betas)
        self.register_buffer('alphas_cumprod', alphas_cumprod)
        self.register_buffer('alphas_cumprod_prev', alphas_cumprod_prev)
        self.register_buffer('sqrt_alphas_cumprod', torch.sqrt(alphas_cumprod))
        self.register_buffer('sqrt_one_minus_alphas_cumprod', torch.sqrt(1. - alphas_cumprod))
        self.register_buffer('log_one_minus_alphas_cumprod', torch.log(1. - alphas_cumprod))
        self.register_buffer('sqrt_recip_alphas_cumprod', torch.sqrt(1. / alphas_cumprod))
        self.register_buffer('sqrt_recipm1_alphas_cumprod', torch.sqrt(1. / alphas_cumprod - 1))
        posterior_variance = betas * (1. - alphas_cumprod_prev) / (1. - alphas_cumprod)
        self.register_buffer('posterior_variance', posterior_variance)
        self.register_buffer('posterior_log_variance_clipped', torch.log(torch.clamp(posterior_variance, min=1e-20)))
        self.register_buffer('posterior_mean_coef1', betas * np.sqrt(alphas_cumprod_prev) / (1. - alphas_cumprod))
        self.register_buffer('posterior_mean_coef2',
                             (1. - alphas_cumprod_prev) * np.sqrt(alphas) / (1. - alphas_cumprod))
        self.final_alpha_cumprod = torch.tensor([1.0, ])

    _default_ddim = True
    _default_compose = (2.0, 2.0)
    # APF constants hard-coded in the reference method bodies
    apf_ddpm = dict(threshold=0.07, strength=0.1, window=5, after=20)          # diffusion_model_static.py:176-184
    apf_ddim = dict(threshold=0.07, strength=0.1, window=7, start=2, passes=3)  # diffusion_model_static.py:298-319

    def set_noise_shard(self, sample0: Optional[int], total: Optional[int] = None):
        """noise_source='philox' on one shard of a larger job: this wrapper's n_samples trajectories are the global samples
        [sample0, sample0 + n_samples) of ``total``; every rank then draws what ONE GPU running all ``total`` samples with the
        same ``noise_seed`` would have drawn for them.  ``set_noise_shard(None)`` makes every call a whole job again."""
        self._philox_shard = None if sample0 is None else (int(sample0), int(total))

    # ------------------------------------------------------------------ helpers
    def _device(self):
        return self.betas.device

    # ------------------------------------------------------------------ the reference's public arithmetic helpers
    def predict_noise_from_start(self, x_t, t, x0):
        """diffusion_model_static.py:96-106."""
        if self.predict_epsilon:
            return x0
        return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t - x0) / \
            extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape)

    def predict_start_from_noise(self, x_t, t, noise):
        """diffusion_model_static.py:108-118."""
        if self.predict_epsilon:
            return (extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape) * x_t
                    - extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape) * noise)
        return noise

    def q_posterior(self, x_start, x_t, t):
        """diffusion_model_static.py:120-127."""
        posterior_mean = (extract(self.posterior_mean_coef1, t, x_t.shape) * x_start
                          + extract(self.posterior_mean_coef2, t, x_t.shape) * x_t)
        return (posterior_mean, extract(self.posterior_variance, t, x_t.shape),
                extract(self.posterior_log_variance_clipped, t, x_t.shape))

    def deep_repeat_tensor(self, x, t, traj_normalized, obstacle_pts, n_rp):
        """The reference's CFG batch doubling as tensors (diffusion_model_static.py:129-147: ``repeat_interleave``; the 3-D and
        dynamic classes override it with their blocked ``repeat``).  The HIP path never materialises these copies -- row r of
        the network reads trajectory r // n_rp -- the method exists for callers that hold it."""
        return (x.repeat_interleave(n_rp, dim=0), t.repeat_interleave(n_rp, dim=0),
                traj_normalized.repeat_interleave(n_rp, dim=0), obstacle_pts.repeat_interleave(x.shape[0] * n_rp, dim=0))

    def _n_rp(self) -> int:
        return 3 if self.compose else 2

    def _row_pattern(self, B):
        """network-row -> scene-variant pattern (variant 1 = unconditional); rows are [b*n_rp + v]."""
        return [0, 1]

    def invalidate_scene(self):
        """See ``TemporalUnetInference.invalidate_scene``: call after modifying a cloud tensor in a way autograd's version
        counter does not see."""
        self.model.invalidate_scene()

    def _prepare_scene(self, obstacle_pts: torch.Tensor, B=None):
        """Encode the distinct scene(s) once and hand the variants to the context.  A cloud is re-encoded when its content differs
        from the last one's (``unet.SceneCache``); writes that bypass the tensor's version counter need ``invalidate_scene()``."""
        m = self.model
        zero = torch.zeros(1, m.context_dim, device=self._device())
        if self.compose:
            assert obstacle_pts.dim() == 4 and obstacle_pts.shape[0] == 2, \
                "compose expects obstacle_pts of shape (2, n_obstacles, n_points, dim)"
            m.set_scene(torch.cat([m.encode_scene(obstacle_pts), zero]), [0, 1, 2])
        else:
            pattern = self._row_pattern(B)
            # the step-at-a-time callers (p_mean_variance, the replanning loop) pass the same cloud every step
            m.ctx()                          # (re)creates the context and clears the cache after a weight reload
            if obstacle_pts.device != self._device():        # a CPU-resident cloud is compared (and encoded) on the device
                obstacle_pts = obstacle_pts.to(self._device())
            # keyed on CONTENT: the cloud is a few KB, and a (data_ptr, _version) key of a temporary device copy is
            # recycled by the caching allocator for the next same-shaped cloud
            if m.scene_cache.holds(obstacle_pts, pattern):
                return
            m.set_scene(torch.cat([m.encode_scene(obstacle_pts), zero]), pattern)
            m.scene_cache.remember(obstacle_pts, pattern)
        m.cached_batch_size = None          # the compat forward() cache is keyed differently

    @staticmethod
    def _window_weights(window: int) -> torch.Tensor:
        # APFhelper.py:42-44, same torch expression
        return torch.exp(-0.5 * torch.square(torch.arange(-window, window + 1)) / (window / 2) ** 2).float()

    def _fill_hard(self, p, arrays: _HostArrays, hard_conds: Dict[int, torch.Tensor], B: int):
        """n_hard / hard_idx_host / hard_val of ramp_sample_params and ramp_replan_params."""
        H = self.model.n_support_points
        idx = [k if k >= 0 else H + k for k in hard_conds]
        p.n_hard = len(idx)
        if idx:
            vals = [hard_conds[k].to(self._device(), torch.float32) for k in hard_conds]
            val = torch.stack([v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v for v in vals]).contiguous()
            p.hard_idx_host, p.hard_val = arrays.i32(idx), _lib.ptr(arrays.keep(val))

    # ------------------------------------------------------------------ what goes into ramp_sample_params
    def _ddim_coefficients(self, steps, K) -> Dict[str, list]:
        """THE DDIM rule (diffusion_model_static.py:265-331 with eta = 0, use_clipped_model_output): per step t of ``steps``, with
        prev = t - T // K and alpha_prev = final_alpha_cumprod when prev < 0, the scalars of ``DDIM_FIELDS`` -- x0 from eps
        (sqrt_recip, sqrt_recipm1), eps' = (x - sqrt_a_t x0) / sqrt_1m_a_t, x <- sqrt_a_prev x0 + dir_coef eps'.  ``dir_coef`` keeps
        the reference's variance term; at eta = 0 it equals (1 - alpha_prev) ** 0.5 on every step in use (test_sampler_host.py)."""
        ac, sr, srm = (b.detach().cpu() for b in (self.alphas_cumprod, self.sqrt_recip_alphas_cumprod, self.sqrt_recipm1_alphas_cumprod))
        out = {k: [] for k in DDIM_FIELDS}
        for t in steps:
            prev = t - self.n_diffusion_steps // K
            a_t = ac[t]
            a_prev = ac[prev] if prev >= 0 else self.final_alpha_cumprod[0]
            variance = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev)
            std_dev_t = 0.0 * variance ** 0.5                                   # eta = 0
            out['sqrt_recip'].append(sr[t]); out['sqrt_recipm1'].append(srm[t])
            out['sqrt_a_t'].append(a_t ** 0.5); out['sqrt_1m_a_t'].append((1 - a_t) ** 0.5)
            out['sqrt_a_prev'].append(a_prev ** 0.5)
            out['dir_coef'].append((1 - a_prev - std_dev_t ** 2) ** 0.5)
        return out

    def _ddpm_steps(self, n_diffusion_steps_without_noise=0):
        """The DDPM loop's counter i = T - 1 .. -n_without_noise and the timestep it evaluates, max(i, 0) (sample_functions.py:25-27)."""
        raw = list(reversed(range(-n_diffusion_steps_without_noise, self.n_diffusion_steps)))
        return [max(i, 0) for i in raw], raw

    def _fill_schedule(self, p, arrays: _HostArrays, ddim: bool, steps, noise_scale=None, ddim_K: Optional[int] = None):
        """The per-step schedule tables of ramp_sample_params, from the schedule buffers exactly as the reference's extract() would
        (host data only: no device, no context).  DDPM fills coef1 / coef2 / stdv / use_noise / noise_scale, DDIM the DDIM rule's."""
        p.n_steps, p.ddim = len(steps), int(ddim)
        p.t = arrays.i32(steps)
        if ddim:
            for k, v in self._ddim_coefficients(steps, ddim_K or self.ddim_num_inference_steps).items():
                setattr(p, k, arrays.f32(v))
            return
        for field, buf in (('sqrt_recip', self.sqrt_recip_alphas_cumprod), ('sqrt_recipm1', self.sqrt_recipm1_alphas_cumprod),
                           ('coef1', self.posterior_mean_coef1), ('coef2', self.posterior_mean_coef2)):
            buf = buf.detach().cpu()
            setattr(p, field, arrays.f32([buf[t] for t in steps]))
        # model_std = exp(0.5 * posterior_log_variance_clipped[t])   (sample_functions.py:35-36)
        plv = self.posterior_log_variance_clipped.detach().cpu()
        p.stdv = arrays.f32([torch.exp(0.5 * plv[t]) for t in steps])
        p.use_noise = arrays.i32([0 if t == 0 else 1 for t in steps])
        p.noise_scale = arrays.f32(noise_scale)

    @staticmethod
    def _compose_apf_cloud(obstacle_pts):
        """compose: the APF field is the first six obstacles of scene A + the first four of scene B (static.py:306-310)."""
        return torch.cat([obstacle_pts[0], obstacle_pts[1][:4]], dim=0).reshape(-1, 2)

    def _fill_apf(self, p, arrays: _HostArrays, apf_cfg, obstacle_pts=None, batch=None, scene_job=None):
        """ramp_apf_params of the job; the points are one cloud (``obstacle_pts``) or, for a scene batch, its per-scene tables."""
        w = arrays.keep(self._window_weights(apf_cfg['window']).contiguous())
        p.apf.window = int(apf_cfg['window'])
        p.apf.window_weights_host = C.cast(w.data_ptr(), _lib.c_f32p)
        p.apf.threshold = float(apf_cfg['threshold'])
        p.apf.strength = float(apf_cfg['strength'])
        p.apf.passes = int(apf_cfg.get('passes', 1))
        if batch is not None:
            batch.cloud_points = _lib.ptr(scene_job['cloud_points'])
            batch.cloud_offset_host = scene_job['cloud_offset'].ctypes.data_as(_lib.c_i32p)
            return
        cloud = self._compose_apf_cloud(obstacle_pts) if self.compose else obstacle_pts.reshape(-1, 2)
        cloud = arrays.keep(cloud.to(self._device(), torch.float32).contiguous())
        p.apf.cloud = _lib.ptr(cloud)
        p.apf.n_points = cloud.shape[0]

    def _philox_block(self, B: int, n_steps: int, ddim: bool, n_inner: int = 0, n_resample: int = 0):
        """A job that draws its own noise takes the next (n_steps + 1 | 1) * total * H * S elements of the Philox stream: returns
        (seed, offset, sample0, total) for the params and advances the offset by the WHOLE job's block (every shard advances alike).
        ``n_inner`` > 0 (a job with Langevin steps): its draws sit behind the full (n_steps + 1)-block main block -- n_inner blocks of
        normals, then one group per uniform (ramp_sample_mcmc in ramp_hip.h) -- and the offset advances past them.  ``n_resample`` > 0 (a
        job with resampling events): that many groups more, one per (event, group), behind the inner steps' (ramp_resample_params)."""
        s0, tot = self._philox_shard if self._philox_shard is not None else (0, B)
        if not (0 <= s0 and s0 + B <= tot):
            raise ValueError(f"set_noise_shard: samples [{s0}, {s0 + B}) lie outside the job's {tot}")
        hs = self.model.n_support_points * self.state_dim
        n_el = (1 if ddim else n_steps + 1) * tot * hs
        offset = self._philox_offset
        self.last_philox = (self.noise_seed, offset, n_el)
        if n_inner or n_resample:
            self._philox_offset += (n_steps + 1 + n_inner) * tot * hs // 4 + n_inner * tot + n_resample
        else:
            self._philox_offset += (n_el + 3) // 4
        return self.noise_seed, offset, s0, tot

    def _mcmc_tables(self, mcmc: dict, steps) -> dict:
        """The host tables of the job's Langevin refinement (``mcmc_tables``), or the refusal -- before anything touches the device."""
        if not self.predict_epsilon:
            raise NotImplementedError("mcmc=: predict_epsilon=False makes the combined network output x0, not a score -- there is no "
                                      "density for the Langevin steps to correct")
        return mcmc_tables(mcmc, steps, self.alphas_cumprod)

    @staticmethod
    def _fill_mcmc(arrays: _HostArrays, tab: dict):
        """ramp_mcmc_params from the tables of ``mcmc_tables``."""
        mp = _lib.RampMcmcParams()
        mp.kind = tab['kind']
        mp.n_inner, mp.step_size, mp.sigma = arrays.i32(tab['n_inner']), arrays.f32(tab['step_size']), arrays.f32(tab['sigma'])
        return mp

    def _mcmc_draws(self, mcmc: dict, tab: dict, B: int, noise):
        """The inner steps' injected draws (z, u), behind the loop's own in call order; (None, None) for a job without an inner step or one
        that draws its own noise (``noise`` None), which takes none."""
        z_in, u_in = mcmc.get('noise'), mcmc.get('u')
        if noise is None and (z_in is not None or u_in is not None):
            raise ValueError("mcmc['noise'] / mcmc['u'] inject the inner steps' draws next to an injected loop noise; with "
                             "noise_source='philox' the job draws both itself -- leave them out")
        K, dev, H, S = tab['total'], self._device(), self.model.n_support_points, self.state_dim
        if noise is None or not K:
            return None, None
        z_in = torch.randn((K, B, H, S), device=dev) if z_in is None else z_in.to(dev, torch.float32).contiguous()
        if u_in is None:
            u_in = torch.rand((K, B), device=dev).clamp_(min=2.0 ** -24, max=1.0 - 2.0 ** -24)
        u_in = u_in.to(dev, torch.float32).contiguous()
        if tuple(z_in.shape) != (K, B, H, S) or tuple(u_in.shape) != (K, B):
            raise ValueError(f"mcmc noise / u must be ({K}, {B}, {H}, {S}) / ({K}, {B})")
        return z_in, u_in

    def _scene_clouds(self, name: str, opt: dict, scene_job: Optional[dict], arrays: Optional[_HostArrays] = None, d_empty: int = 2):
        """The per-scene clouds of a ``cost_guide=`` / ``resample=`` dict (``name`` in the messages): one for a plain job, one per scene for
        a scene / composed job (a single ``cloud`` then serves every scene).  A cloud that is None is an empty one, as wide as the other
        clouds' points (``d_empty`` without any).  Returns ``cloud_table``'s (points, offsets, d), kept in ``arrays`` -- without
        ``arrays`` (None, None, the width of the first cloud that is not None, or None): the list is checked and nothing is built."""
        from .guide import cloud_table
        n_scenes = scene_job['n_scenes'] if scene_job is not None else 1
        clouds = [opt['cloud']] * n_scenes if 'cloud' in opt else list(opt['clouds'])
        if len(clouds) != n_scenes:
            raise ValueError(f"{name} clouds: {len(clouds)} entries for {n_scenes} scene(s)")
        d_cloud = next((int(torch.as_tensor(c).shape[-1]) for c in clouds if c is not None), None)
        if arrays is None:
            return None, None, d_cloud
        clouds = [torch.zeros(0, d_cloud or d_empty) if c is None else c for c in clouds]
        points, off, d = cloud_table(clouds, self._device())
        if d > self.state_dim:
            raise ValueError(f"{name}: {d}-D points on {self.state_dim}-wide states")
        return arrays.keep(points), arrays.keep(off), d

    def _fill_guide(self, arrays: _HostArrays, tab: dict, cost_guide: dict, scene_job: Optional[dict], ptab: Optional[dict] = None):
        """ramp_cost_guide from the tables of ``guide_tables`` and the guide's clouds (``_scene_clouds``; without any, an empty cloud is as
        wide as the primitives' points).  ``ptab``: what ``_prim_tables`` returned."""
        from .guide import fill_cost_guide
        points, off, d = self._scene_clouds('cost_guide', cost_guide, scene_job, arrays, ptab['D'] if ptab is not None else 2)
        if ptab is not None and ptab['D'] != d:
            raise ValueError(f"cost_guide: {d}-D cloud points with {ptab['D']}-D boxes / spheres")
        cg = fill_cost_guide(points, off, d, tab)
        cg.n_guide, cg.step = arrays.i32(tab['n_guide']), arrays.f32(tab['step'])
        return cg

    def _prim_tables(self, arrays: _HostArrays, tab: dict, cost_guide: dict, scene_job: Optional[dict]):
        """The box and sphere tables (``ramp_amd.guide.prim_table``) of a guide whose dict carries the primitive keys, None otherwise."""
        if 'prim' not in tab:
            return None
        from .guide import prim_table
        n_scenes = scene_job['n_scenes'] if scene_job is not None else 1
        d_cloud = self._scene_clouds('cost_guide', cost_guide, scene_job)[2]
        return arrays.keep(prim_table(cost_guide.get('boxes'), cost_guide.get('spheres'), n_scenes, d_cloud, self._device()))

    def _fill_resample(self, arrays: _HostArrays, tab: dict, resample: dict, scene_job: Optional[dict], hard_conds, B: int):
        """ramp_resample_params from the tables of ``resample_tables``: one group for a plain job, one per scene for a scene / composed job,
        the cost's clouds like the guide's.  Returns (params, its cost table, the host group table)."""
        from .guide import fill_cost_guide
        n_scenes = scene_job['n_scenes'] if scene_job is not None else 1
        if scene_job is None:
            gf = np.array([0, B], dtype=np.int32)
        else:
            ts = scene_job['traj_scene'].cpu().numpy()
            if np.any(np.diff(ts) < 0):
                raise ValueError("resample=: a scene's trajectories must be adjacent, scenes in order")
            gf = np.concatenate([[0], np.cumsum(np.bincount(ts, minlength=n_scenes))]).astype(np.int32)
            if np.any(np.diff(gf) <= 0):
                raise ValueError("resample=: every scene needs at least one trajectory")
        for k, v in hard_conds.items():      # a resampled row keeps its place's pinned values: they must agree inside a group
            v = v.detach().cpu()
            if v.dim() == 2:
                for a, b in zip(gf[:-1], gf[1:]):
                    if not bool((v[a:b] == v[a:a + 1]).all()):
                        raise ValueError(f"resample=: the values of hard condition {k} differ inside a group (trajectories {a} .. {b - 1}): "
                                         "resampling moves whole rows between them")
        cost = arrays.keep(fill_cost_guide(*self._scene_clouds('resample', resample, scene_job, arrays), tab))
        rs = _lib.RampResampleParams()
        rs.n_groups, rs.group0, rs.groups_total = len(gf) - 1, 0, 0
        gf = arrays.keep(gf)
        rs.group_first_host = gf.ctypes.data_as(_lib.c_i32p)
        rs.resample = arrays.i32(tab['resample'])
        lam = arrays.keep(np.asarray(tab['lambda'], dtype=np.float64))
        rs.lambda_ = lam.ctypes.data_as(_lib.c_f64p)
        rs.ess_frac = tab['ess_frac']
        rs.cost = C.pointer(cost)
        return rs, cost, gf

    def _resample_draws(self, resample: dict, n_ev: int, G: int, noise):
        """The events' injected uniforms (n_ev, G); None for a job that draws its own noise (``noise`` None), which takes none."""
        ru = resample.get('u')
        if noise is None and ru is not None:
            raise ValueError("resample['u'] injects the events' uniforms next to an injected loop noise; with noise_source='philox' "
                             "the job draws them itself -- leave it out")
        if noise is None:
            return None
        if ru is None:
            ru = torch.rand((n_ev, G), device=self._device()).clamp_(min=2.0 ** -24, max=1.0 - 2.0 ** -24)
        ru = torch.as_tensor(ru).to(self._device(), torch.float32).contiguous()
        if tuple(ru.shape) != (n_ev, G):
            raise ValueError(f"resample u must be ({n_ev}, {G}); got {tuple(ru.shape)}")
        return ru

    @staticmethod
    def _refuse_prims_outside_the_guide(cost_guide, resample, stitch):
        """The swept primitive term lives in ``cost_guide=`` of plain, scene, composed and MCMC jobs only: host check, before any device call."""
        if guide_has_prims(resample):
            raise NotImplementedError("resample=: the potential takes no boxes= / spheres= (the swept primitive term belongs to cost_guide=)")
        if guide_has_prims(cost_guide) and (stitch is not None or resample is not None):
            raise NotImplementedError("cost_guide=: boxes= / spheres= (the swept primitive term) are not served on stitched windows or with "
                                      "resample= (ramp_sample_stitched and ramp_sample_steered take no primitives)")

    @staticmethod
    def _refuse_team_outside_the_guide(cost_guide, resample, stitch, counts=None):
        """Teams of robots live in ``cost_guide=`` of plain, scene, composed and MCMC jobs only, and every scene's rows must be whole teams
        (``counts``: the rows per scene, where the caller knows them): host checks, before any device call."""
        if not guide_has_team(cost_guide):
            return
        from .team import team_scalars
        A = team_scalars(cost_guide['team'])['size']
        if guide_has_prims(cost_guide):
            raise NotImplementedError("cost_guide=: team= with boxes= / spheres= is not served (ramp_sample_guided_prims takes no team)")
        if resample is not None:
            raise NotImplementedError("cost_guide=: team= with resample= is not served (a resampled row would leave its team)")
        if stitch is not None:
            raise NotImplementedError("cost_guide=: team= is not served on stitched windows (ramp_sample_stitched takes no team)")
        for i, n in enumerate(counts or []):
            if int(n) % A:
                raise ValueError(f"cost_guide team=: {int(n)} rows in scene {i} are no multiple of the team size {A} (n_samples counts rows)")

    def _run_guarded(self, job):
        """Run ``job`` under the fp16x3 range-guard policy: a flagged result is discarded and the same job (same noise) repeated, never
        a silently degraded answer.  First IN fp16x3 with the evaluation that raised the guard run as a calibrating one (range-free,
        its successor scaled from true maxima: ramp_set_fallback(ctx, 2)); if that repeat is flagged as well, all in bf16x6."""
        m, lib = self.model, _lib.load()

        def flagged():
            flag = C.c_int32(0)
            _lib.check(lib.ramp_range_status(m.ctx(), C.byref(flag), _lib.current_stream()), "ramp_range_status")
            return flag.value

        def again(mode):
            _lib.check(lib.ramp_set_fallback(m.ctx(), mode), "ramp_set_fallback")
            try:
                job()
                return flagged()
            finally:
                _lib.check(lib.ramp_set_fallback(m.ctx(), 0), "ramp_set_fallback")

        job()
        flag = flagged()
        self.last_job_mode = {0: "fp16x3", 1: "fp32", 2: "bf16x6", 3: "fp16x3"}[m.gemm_mode]      # (0: the library default)
        if not flag:
            return
        if not self.fp16_fallback:
            raise _lib.RampHipError("fp16x3 GEMM: an operand left the fp16 range between two score evaluations "
                                    f"(call site {flag - 1}); use gemm_mode='bf16x6'")
        ev, site = C.c_int32(-1), C.c_int32(-1)
        _lib.check(lib.ramp_range_trip(m.ctx(), C.byref(ev), C.byref(site)), "ramp_range_trip")
        again_flag = 1
        if ev.value >= 0 and self.fp16_rerun:
            warnings.warn(f"fp16x3 range guard tripped in evaluation {ev.value} (GEMM call site {site.value}): repeating the job "
                          "in fp16x3 with that evaluation calibrating")
            self.range_reruns += 1
            again_flag = again(2)
            self.last_job_mode = "fp16x3-rerun"
        if again_flag:
            warnings.warn(f"fp16x3 range guard tripped at GEMM call site {flag - 1}: repeating the job in bf16x6")
            self.range_fallbacks += 1
            again(1)
            self.last_job_mode = "bf16x6"

    def _warm_job(self, warm_start, B: int, steps_full, scene_job: Optional[dict] = None, stitch: Optional[dict] = None):
        """``warm_start=dict(prior=, level=, start=None)`` of run_inference* resolved for a job of ``B`` rows on the model's iteration list
        ``steps_full`` (``ramp_amd.warm`` states the definition): host checks only, before anything of the job touches the device.

          prior   normalised trajectories of the job's rows: (B, H, S), or (H, S) / (1, H, S) for all rows, or one entry per scene of a scene /
                  composed job (``warm.prior_rows``); rows without a level are not read.  None where no row has a level
          level   an int (every row), a (B,) sequence with None entries (no prior: the row starts from noise and runs the whole job), or one
                  entry per scene
          start   None, or the level the JOB starts at where it must not follow from these rows alone (a sharded caller passes the whole
                  job's value, so that every shard lays out the same noise block)

        Returns the resolved dict (``J``, ``j0``, ``t_row``, ``n_hold``, the device ``prior`` (B, H, S), ``sa`` / ``s1a`` / ``has``), or its
        argument where that is one already."""
        if warm_start is None or (isinstance(warm_start, dict) and warm_start.get('_resolved')):
            return warm_start
        from . import warm as W
        if not self._scenes_supported:
            raise NotImplementedError(f"warm_start=: {type(self).__name__} keeps its own replanning")
        if not isinstance(warm_start, dict):
            raise TypeError("warm_start= takes a dict(prior=, level=, start=None)")
        unknown = set(warm_start) - {'prior', 'level', 'start'}
        if unknown:
            raise ValueError(f"warm_start=: unknown keys {sorted(unknown)}")
        if 'level' not in warm_start:
            raise ValueError("warm_start=: level= is required")
        dev, H, S = self._device(), self.model.n_support_points, self.state_dim
        counts = [B]
        if scene_job is not None and stitch is None:      # a scene's rows are adjacent, scenes in order
            counts = np.bincount(scene_job['traj_scene'].cpu().numpy(), minlength=int(scene_job['n_scenes'])).tolist()
        levels = W.level_rows(warm_start['level'], counts)
        tab = W.warm_tables(levels, steps_full, warm_start.get('start'), T=self.n_diffusion_steps)
        has = tab['t_row'] >= 0
        prior = warm_start.get('prior')
        if prior is None:
            if has.any():
                raise ValueError("warm_start=: prior= is required where a row has a level")
            prior = torch.zeros((B, H, S), device=dev)
        else:
            if not (torch.is_tensor(prior) or (isinstance(prior, (list, tuple)) and len(prior) and torch.is_tensor(prior[0]))):
                prior = [np.asarray(v, np.float32) for v in prior] if isinstance(prior, (list, tuple)) else np.asarray(prior, np.float32)
            prior = W.prior_rows(prior, counts)
            prior = (prior if torch.is_tensor(prior) else torch.from_numpy(np.array(prior, np.float32))).to(dev, torch.float32).contiguous()
        if tuple(prior.shape) != (B, H, S):
            raise ValueError(f"warm_start=: the prior must hold ({B}, {H}, {S}) for the job's rows; got {tuple(prior.shape)}")
        if has.any() and not bool(torch.isfinite(prior[torch.from_numpy(has).to(dev)]).all()):
            raise ValueError("warm_start=: the prior is not finite")
        t_safe = np.where(has, tab['t_row'], 0)
        sa = self.sqrt_alphas_cumprod.detach().cpu().numpy().astype(np.float32)[t_safe]
        s1a = self.sqrt_one_minus_alphas_cumprod.detach().cpu().numpy().astype(np.float32)[t_safe]
        return dict(tab, _resolved=True, prior=prior, sa=sa, s1a=s1a, has=has.astype(np.int32), steps_full=[int(s) for s in steps_full])

    def _launch(self, B, noise, hard_conds, obstacle_pts, ddim: bool, steps, apply_apf, noise_scale, apf_cfg,
                return_chain: bool, ddim_K: Optional[int] = None, scene_job: Optional[dict] = None, guidance: Optional[dict] = None,
                mcmc: Optional[dict] = None, cost_guide: Optional[dict] = None, resample: Optional[dict] = None,
                stitch: Optional[dict] = None, warm_start: Optional[dict] = None):
        """One fused sampling job (``ramp_sample``).  ``scene_job``: what ``_prepare_scene_job`` returned -- a job of many scenes
        (``ramp_sample_scenes``); ``obstacle_pts`` is not read then.  ``guidance`` (with a ``scene_job``): a composed job
        (``ramp_sample_composed``) -- ``n_rp`` rows per trajectory and the device (B, n_rp) ``row_weight`` table of ``_prepare_composed_job``.
        ``mcmc``: Langevin refinement inside the job (``ramp_sample_mcmc``, the one entry for all three kinds of job; ``mcmc_tables``);
        the accept flags land in ``self.last_mcmc``.  ``cost_guide``: cost-gradient guidance inside the job (``ramp_sample_guided``, the
        same one entry with the guide added; ``guide_tables``).  ``resample``: resampling events inside the job (``ramp_sample_steered``;
        ``resample_tables``); ancestors, ESS, costs and final log-weights land in ``self.last_resample``.  ``stitch`` (with a ``scene_job``
        and empty ``hard_conds``): stitched windows (``ramp_sample_stitched``) -- the dict of ``run_inference_stitched``: ``n_windows``,
        ``overlap``, ``alpha`` (O) float32, ``pin_idx`` (n_pin) int32, ``pin_val`` device (n_pin, C, S) or None.  ``warm_start``: the rows start
        from given plans at levels of their own (``ramp_sample_warm``, the one entry for every job above; ``_warm_job`` / ``ramp_amd.warm``).
        ``steps`` / ``apply_apf`` / ``noise_scale`` are then still the model's FULL lists: the job runs their tail from iteration J, ``noise``
        holds that tail's blocks, and ``self.last_warm`` keeps ``J``, ``j0``, ``t_row`` and the job's ``steps``."""
        m = self.model
        # ---- refusals and the options' host tables, before anything touches the device
        if stitch is not None and (mcmc is not None or resample is not None or guidance is not None or hard_conds):
            raise NotImplementedError("stitched windows take no mcmc=, resample=, composed weights or hard conditions of their own")
        self._refuse_prims_outside_the_guide(cost_guide, resample, stitch)
        self._refuse_team_outside_the_guide(cost_guide, resample, stitch, [B])
        warm = self._warm_job(warm_start, B, steps, scene_job, stitch)
        rtab = resample_tables(resample, steps) if resample is not None else None      # (flags by iteration index: on the full list)
        if warm is not None:
            if warm['n_hold'] > 0:
                if resample is not None:
                    raise NotImplementedError("warm_start=: mixed levels with resample= are not served (a held row could become an ancestor)")
                if guide_has_team(cost_guide):
                    raise NotImplementedError("warm_start=: mixed levels with cost_guide team= are not served (a held agent would face moving team mates)")
                if stitch is not None:
                    raise NotImplementedError("warm_start=: mixed levels inside one stitched chain are not served (the windows of a chain start together)")
            J = warm['J']      # the job is the tail of the schedule: whatever indexes the full list was computed on it and loses J entries
            steps, apply_apf = list(steps)[J:], list(apply_apf)[J:]
            noise_scale = list(noise_scale)[J:] if noise_scale is not None else None
            if rtab is not None:
                rtab = dict(rtab, resample=rtab['resample'][J:], events=[j - J for j in rtab['events'] if j >= J])
                rtab['lambda'] = rtab['lambda'][J:]
            n_blocks = 1 if ddim else len(steps) + 1
            if noise is not None and noise.shape[0] != n_blocks:
                raise ValueError(f"warm_start=: the job runs {len(steps)} iterations and takes {n_blocks} noise blocks; got {noise.shape[0]}")
        if rtab is not None:
            if self._philox_shard is not None:
                raise NotImplementedError("resample=: a sharded job (set_noise_shard) cannot resample -- a group's trajectories would sit on "
                                          "several devices")
            if not self.predict_epsilon:
                raise NotImplementedError("resample=: predict_epsilon=False is not served")
            if ddim and not (mcmc is not None and mcmc_tables(mcmc, steps, self.alphas_cumprod)['total'] > 0):
                raise NotImplementedError("resample=: the DDIM loop (eta = 0) never separates duplicates -- add mcmc= inner steps or sample "
                                          "with sampler='ddpm'")
        tab = self._mcmc_tables(mcmc, steps) if mcmc is not None else None
        gtab = guide_tables(cost_guide, steps, self.posterior_variance) if cost_guide is not None else None
        dev = self._device()
        H, S = m.n_support_points, self.state_dim
        n_steps = len(steps)
        m.prepare_time_table(self.n_diffusion_steps)
        if scene_job is None:      # (run_inference_scenes: the scene table is already set, set_scenes)
            self._prepare_scene(obstacle_pts, B)
        # ---- the job's params; `arrays` keeps everything the C call reads referenced until it has returned
        p, arrays = _lib.RampSampleParams(), _HostArrays()
        p.B, p.n_rp = B, self._n_rp()
        p.w0, p.w1 = (float(w) for w in (self.compose_weights if self.compose else (self.cfg_weight, 0.0)))
        rows = None
        if guidance is not None:      # the weights are the table's; w0 / w1 are not read
            if scene_job is None:
                raise ValueError("a composed job needs its scene job (the row -> latent table comes from set_scenes)")
            p.n_rp, p.w0, p.w1 = int(guidance['n_rp']), 0.0, 0.0
            rows = _lib.RampGuidanceRows()
            rows.n_rp, rows.row_weight = p.n_rp, _lib.ptr(arrays.keep(guidance['row_weight']))
        self._fill_schedule(p, arrays, ddim, steps, noise_scale, ddim_K)
        p.apply_apf = arrays.i32(apply_apf)
        p.clip_denoised = int(bool(self.clip_denoised))
        p.predict_x0 = int(not self.predict_epsilon)
        self._fill_hard(p, arrays, hard_conds, B)
        batch = None
        if scene_job is not None:
            batch = _lib.RampSceneBatch()
            batch.n_scenes = scene_job['n_scenes']
            batch.traj_scene = _lib.ptr(scene_job['traj_scene'])
        if apf_cfg is not None and any(apply_apf):
            self._fill_apf(p, arrays, apf_cfg, obstacle_pts, batch, scene_job)
        p.use_graph = int(self.use_graph)
        chain = torch.empty((n_steps + 1, B, H, S), device=dev, dtype=torch.float32) if return_chain else None
        x_out = torch.empty((B, H, S), device=dev, dtype=torch.float32)
        # ---- the options: each one's struct, injected draws and outputs
        from .guide import fill_prim_guide
        from .team import fill_team_guide
        cg = pg = tg = None
        if gtab is not None:
            tg = fill_team_guide(gtab['team']) if gtab.get('team') is not None else None
            ptab = self._prim_tables(arrays, gtab, cost_guide, scene_job)
            cg = self._fill_guide(arrays, gtab, cost_guide, scene_job, ptab)
            pg = fill_prim_guide(ptab, gtab['prim']) if ptab is not None else None
        rs = ru = None
        r_out = (None, None, None, None)      # ancestors, ESS, costs, final log-weights
        n_ev = len(rtab['events']) if rtab is not None else 0
        if n_ev:
            rs, _cost, r_gf = self._fill_resample(arrays, rtab, resample, scene_job, hard_conds, B)
            r_out = (torch.empty((n_ev, B), device=dev, dtype=torch.int32), torch.empty((n_ev, rs.n_groups), device=dev, dtype=torch.float64),
                     torch.empty((n_ev, B), device=dev, dtype=torch.float64), torch.empty((B,), device=dev, dtype=torch.float64))
            ru = self._resample_draws(resample, n_ev, rs.n_groups, noise)
        mp = z_in = u_in = accept = None
        if tab is not None:
            mp = self._fill_mcmc(arrays, tab)
            accept = torch.zeros((tab['total'], B), device=dev, dtype=torch.int32)
            z_in, u_in = self._mcmc_draws(mcmc, tab, B, noise)
        from .stitch import fill_stitch
        st = fill_stitch(*(stitch[k] for k in ('n_windows', 'overlap', 'alpha', 'pin_idx', 'pin_val'))) if stitch is not None else None
        ws = None
        if warm is not None:
            ws = _lib.RampWarmStart()
            ws.prior, ws.n_hold = _lib.ptr(arrays.keep(warm['prior'])), warm['n_hold']
            ws.j0_host, ws.has_prior_host = arrays.i32(warm['j0']), arrays.i32(warm['has'])
            ws.sa_host, ws.s1a_host = arrays.f32(warm['sa']), arrays.f32(warm['s1a'])
        if noise is None:         # the job draws its own, the options' draws included
            p.noise_mode = 1
            p.philox_seed, p.philox_offset, p.philox_sample0, p.philox_total = self._philox_block(B, n_steps, ddim, tab['total'] if tab else 0,
                                                                                                     n_ev * rs.n_groups if n_ev else 0)
            if stitch is not None:      # (never a shard: the entry takes a whole job, spelled 0 / 0)
                p.philox_sample0, p.philox_total = 0, 0
        else:
            noise = noise.contiguous()

        # ---- the call: the job's options choose the entry and its leading structs; the rest is shared
        opt = lambda x: C.byref(x) if x is not None else None      # noqa: E731
        middle = (opt(mp), opt(rows), opt(batch), _lib.ptr(noise), _lib.ptr(z_in), _lib.ptr(u_in))
        plain = (_lib.ptr(noise), _lib.ptr(chain), _lib.ptr(x_out))
        outs = (_lib.ptr(chain), _lib.ptr(x_out), _lib.ptr(accept))
        if ws is not None:      # the one entry that takes every option
            entry = "ramp_sample_warm"
            args = ((C.byref(ws), opt(st), opt(rs), opt(cg), opt(pg), opt(tg)) + middle + (_lib.ptr(ru),) + outs + tuple(_lib.ptr(t) for t in r_out)
                    + (None,))
        elif st is not None:
            entry, args = "ramp_sample_stitched", (C.byref(st), opt(cg), opt(batch)) + plain + (None,)
        elif rs is not None:
            entry, args = "ramp_sample_steered", (C.byref(rs), opt(cg)) + middle + (_lib.ptr(ru),) + outs + tuple(_lib.ptr(t) for t in r_out)
        elif pg is not None:
            entry, args = "ramp_sample_guided_prims", (C.byref(cg), C.byref(pg)) + middle + outs
        elif tg is not None:
            entry, args = "ramp_sample_guided_team", (C.byref(cg), C.byref(tg)) + middle + outs
        elif cg is not None:
            entry, args = "ramp_sample_guided", (C.byref(cg),) + middle + outs
        elif mp is not None:
            entry, args = "ramp_sample_mcmc", middle + outs
        elif rows is not None:
            entry, args = "ramp_sample_composed", (C.byref(rows), C.byref(batch)) + plain
        elif batch is not None:
            entry, args = "ramp_sample_scenes", (C.byref(batch),) + plain
        else:
            entry, args = "ramp_sample", plain
        with torch.cuda.device(dev):
            fn = getattr(_lib.load(), entry)
            self._run_guarded(lambda: _lib.check(fn(m.ctx(), C.byref(p), *args, _lib.current_stream()), entry))
        # ---- results
        r_anc, r_ess, r_cost, r_logw = r_out
        if warm is not None:
            self.last_warm = {'J': warm['J'], 'j0': warm['j0'].copy(), 't_row': warm['t_row'].copy(), 'steps': list(steps)}
        if tab is not None:      # one copy back
            acc = accept.cpu()
            rate, k0 = [], 0
            held = torch.from_numpy(warm['j0']) if warm is not None and warm['n_hold'] > 0 else None
            for j, K in enumerate(tab['n_inner']):
                if held is not None and K:      # a held row's inner steps are undone by the hold: flag -1, left out of the rate
                    acc[k0:k0 + K, held > j] = -1
                live = acc[k0:k0 + K][acc[k0:k0 + K] >= 0] if K else None
                rate.append(float(live.float().mean()) if K and live.numel() else float('nan'))
                k0 += K
            self.last_mcmc = {'accept': acc, 'rate': rate, 'n_inner': list(tab['n_inner']), 'kind': tab['kind']}
        if rtab is not None:
            self.last_resample = {'ancestors': r_anc.cpu() if n_ev else torch.empty((0, B), dtype=torch.int32),
                                  'ess': r_ess.cpu() if n_ev else None, 'cost': r_cost.cpu() if n_ev else None,
                                  'logw': r_logw.cpu() if n_ev else torch.zeros((B,), dtype=torch.float64),
                                  'group_first': r_gf.copy() if n_ev else None, 'events': list(rtab['events'])}
        return x_out, chain

    # ------------------------------------------------------------------ loops (reference signatures)
    @staticmethod
    def _is_fused_ddpm_step(sample_fn) -> bool:
        """True for the two step functions the fused job implements: this package's ``ddpm_sample_fn`` and the reference's own
        (``mpd.models.diffusion_models.sample_functions.ddpm_sample_fn``, recognised by name and module so that a driver that
        still imports it from there keeps the fast path)."""
        if sample_fn is None or sample_fn is ddpm_sample_fn:      # (None = "the default": the reference would fail on the call)
            return True
        mod = getattr(sample_fn, '__module__', '') or ''
        return getattr(sample_fn, '__name__', None) == 'ddpm_sample_fn' and mod.startswith('mpd.') and mod.endswith('sample_functions')

    @torch.no_grad()
    def p_sample_loop(self, shape, hard_conds, context=None, return_chain=False, traj_normalized=None,
                      obstacle_pts=None, sample_fn=ddpm_sample_fn, n_diffusion_steps_without_noise=0,
                      noise_std_extra_schedule_fn=None, scene_job=None, guidance=None, mcmc=None, cost_guide=None, resample=None,
                      stitch=None, warm_start=None, **sample_kwargs):
        """diffusion_model_static.py:232-256 / diffusion_model_3d.py:185-218 (resample_steps = 1).  With the stock
        ``ddpm_sample_fn`` the whole loop is ONE fused job (``ramp_sample``: captured graph, noise and schedule tables on the
        device); any other ``sample_fn`` is honoured the way the reference honours it -- called once per step with the
        reference's arguments -- on the eager loop below."""
        if not self._is_fused_ddpm_step(sample_fn):
            if warm_start is not None:
                raise NotImplementedError("warm_start= runs inside the fused job only (ddpm_sample_fn): a caller-supplied sample_fn steps on its own")
            if mcmc is not None:
                raise NotImplementedError("mcmc= runs inside the fused job only (ddpm_sample_fn): a caller-supplied sample_fn steps on its own")
            if cost_guide is not None:
                raise NotImplementedError("cost_guide= runs inside the fused job only (ddpm_sample_fn): a caller-supplied sample_fn steps on its own")
            if resample is not None:
                raise NotImplementedError("resample= runs inside the fused job only (ddpm_sample_fn): a caller-supplied sample_fn steps on its own")
            if stitch is not None:
                raise NotImplementedError("run_inference_stitched runs the fused job only (ddpm_sample_fn): a caller-supplied sample_fn steps on its own")
            if scene_job is not None:
                raise NotImplementedError("run_inference_scenes runs the fused job only (ddpm_sample_fn): a custom sample_fn steps one "
                                          "scene's batch at a time -- use run_inference per scene")
            return self._p_sample_loop_stepwise(shape, hard_conds, context, return_chain, traj_normalized, obstacle_pts, sample_fn,
                                                n_diffusion_steps_without_noise, noise_std_extra_schedule_fn, sample_kwargs)
        device = self._device()
        B = shape[0]
        philox = self.noise_source == "philox"
        x = None if philox else torch.randn(shape, device=device)
        steps, raw = self._ddpm_steps(n_diffusion_steps_without_noise)
        warm = self._warm_job(warm_start, B, steps, scene_job, stitch)      # (a warm-started job draws its tail's blocks only)
        noises = [x] + ([] if philox else [torch.randn_like(x) for _ in steps[(warm['J'] if warm else 0):]])       # drawn every step, zeroed at t == 0
        if noise_std_extra_schedule_fn is None:
            scales = [1.0] * len(steps)
        else:       # the reference hands the schedule function t[0], a 0-d long tensor on the device (sample_functions.py:24, 41-44)
            ts = torch.tensor(raw, device=device, dtype=torch.long)
            scales = [float(noise_std_extra_schedule_fn(ts[j])) for j in range(len(raw))]
        # compose: ddpm_sample_fn calls p_mean_variance_compose, which has no APF hook (static.py:188-229)
        apf = [1 if (self.APF and self._supports_apf and not self.compose and guidance is None and j > self.apf_ddpm['after']) else 0
               for j in range(len(steps))]
        cfg = dict(self.apf_ddpm, passes=1) if any(apf) else None
        x_out, chain = self._launch(B, None if philox else torch.stack(noises), hard_conds, obstacle_pts, False, steps, apf, scales,
                                    cfg, return_chain, scene_job=scene_job, guidance=guidance, mcmc=mcmc, cost_guide=cost_guide,
                                    resample=resample, stitch=stitch, warm_start=warm)
        if return_chain:
            return x_out, chain.permute(1, 0, 2, 3)       # reference stacks along dim=1
        return x_out

    @torch.no_grad()
    def _p_sample_loop_stepwise(self, shape, hard_conds, context, return_chain, traj_normalized, obstacle_pts, sample_fn,
                                n_diffusion_steps_without_noise, noise_std_extra_schedule_fn, sample_kwargs):
        """The reference's loop, statement for statement, for a caller-supplied step function (diffusion_model_static.py:232-256):
        per step ``x, values = sample_fn(self, x, hard_conds, context, t, ...)`` with ``t`` a (B,) long tensor on the device, then
        ``apply_hard_conditioning``.  The step function reaches the HIP kernels through this class's single-step API
        (``p_mean_variance`` -> ``ramp_score`` + ``ramp_cfg_mean``, ``ramp_hard_cond``); noise comes from ``torch.randn`` whatever
        ``noise_source`` says (the step function draws its own)."""
        device = self._device()
        B = shape[0]
        pts = obstacle_pts if self.compose else obstacle_pts.unsqueeze(0)        # static.py:239-240
        x = torch.randn(shape, device=device)
        x = apply_hard_conditioning(x, hard_conds)
        chain = [x] if return_chain else None
        if noise_std_extra_schedule_fn is not None:      # one of the reference's **sample_kwargs
            sample_kwargs = dict(sample_kwargs, noise_std_extra_schedule_fn=noise_std_extra_schedule_fn)
        forward_t = 0
        for i in reversed(range(-n_diffusion_steps_without_noise, self.n_diffusion_steps)):
            t = make_timesteps(B, i, device)
            x, _values = sample_fn(self, x, hard_conds, context, t, traj_normalized=traj_normalized, obstacle_pts=pts,
                                   forward_t=forward_t, compose=self.compose, **sample_kwargs)
            x = apply_hard_conditioning(x.contiguous(), hard_conds)
            if return_chain:
                chain.append(x)
            forward_t += 1
        if return_chain:
            return x, torch.stack(chain, dim=1)
        return x

    def ddim_set_timesteps(self, num_inference_steps) -> np.ndarray:
        self.num_inference_steps = num_inference_steps
        step_ratio = self.n_diffusion_steps // self.num_inference_steps
        return (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)

    @torch.no_grad()
    def ddim_p_sample_loop(self, shape, hard_conds, context=None, return_chain=False, traj_normalized=None,
                           obstacle_pts=None, t_start_guide=float('inf'), guide=None, n_guide_steps=1, scene_job=None,
                           guidance=None, mcmc=None, cost_guide=None, resample=None, stitch=None, warm_start=None, **sample_kwargs):
        """diffusion_model_static.py:347-384 (eta = 0, use_clipped_model_output)."""
        device = self._device()
        B = shape[0]
        x = None if self.noise_source == "philox" else torch.randn(shape, device=device)
        steps = [int(i) for i in self.ddim_set_timesteps(self.ddim_num_inference_steps)]
        apf = [1 if (self.APF and self._supports_apf and j >= self.apf_ddim['start']) else 0 for j in range(len(steps))]
        cfg = dict(self.apf_ddim) if any(apf) else None
        x_out, chain = self._launch(B, None if x is None else x.unsqueeze(0), hard_conds, obstacle_pts, True, steps, apf, None, cfg,
                                    return_chain, scene_job=scene_job, guidance=guidance, mcmc=mcmc, cost_guide=cost_guide,
                                    resample=resample, stitch=stitch, warm_start=warm_start)
        if return_chain:
            return x_out, chain.permute(1, 0, 2, 3)
        return x_out

    @torch.no_grad()
    def conditional_sample(self, hard_conds, horizon=None, batch_size=1, ddim=False, traj_normalized=None,
                           obstacle_pts=None, **sample_kwargs):
        horizon = horizon or self.model.n_support_points
        shape = (batch_size, horizon, self.state_dim)
        self._refuse_prims_outside_the_guide(sample_kwargs.get('cost_guide'), sample_kwargs.get('resample'), sample_kwargs.get('stitch'))
        self._refuse_team_outside_the_guide(sample_kwargs.get('cost_guide'), sample_kwargs.get('resample'), sample_kwargs.get('stitch'), [batch_size])
        if self.ddim:
            for k in ('mcmc', 'cost_guide', 'resample', 'warm_start'):
                if sample_kwargs.get(k) is not None and not self._is_fused_ddpm_step(sample_kwargs.get('sample_fn')):
                    raise NotImplementedError(f"{k}= runs inside the fused job only: a caller-supplied sample_fn steps on its own")
            for k in ('sample_fn', 'n_diffusion_steps_without_noise', 'noise_std_extra_schedule_fn'):
                sample_kwargs.pop(k, None)      # silently ignored by the reference's DDIM loop
            return self.ddim_p_sample_loop(shape, hard_conds, traj_normalized=traj_normalized,
                                           obstacle_pts=obstacle_pts, **sample_kwargs)
        return self.p_sample_loop(shape, hard_conds, traj_normalized=traj_normalized, obstacle_pts=obstacle_pts,
                                  **sample_kwargs)

    def forward(self, cond, *args, **kwargs):
        raise NotImplementedError

    @torch.no_grad()
    def warmup(self, horizon=64, traj_normalized=None, obstacle_pts=None, batch_size=None, device='cuda'):
        """diffusion_model_static.py:405-433: one throw-away score evaluation (consumes one randn)."""
        shape = (batch_size, horizon, self.state_dim)
        x = torch.randn(shape, device=device)
        self.model.prepare_time_table(self.n_diffusion_steps)
        self._prepare_scene(obstacle_pts.to(self._device()))
        eps = torch.empty((batch_size * self._n_rp(), horizon, self.state_dim), device=self._device())
        with torch.cuda.device(self._device()):
            _lib.check(_lib.load().ramp_score(self.model.ctx(), _lib.ptr(x.contiguous()), batch_size, self._n_rp(), 1,
                                              None, _lib.ptr(eps), _lib.current_stream()), "ramp_score")

    @torch.no_grad()
    def run_inference(self, context=None, hard_conds=None, n_samples=1, return_chain=False, traj_normalized=None,
                      obstacle_pts=None, **diffusion_kwargs):
        """diffusion_model_static.py:437-463: returns (steps+1, B, H, S) if return_chain else (B, H, S)."""
        self._refuse_team_outside_the_guide(diffusion_kwargs.get('cost_guide'), diffusion_kwargs.get('resample'), None, [n_samples])
        hard_conds = copy(hard_conds)
        for k, v in hard_conds.items():
            hard_conds[k] = v.to(self._device()).unsqueeze(0).expand(n_samples, -1) if v.dim() == 1 else v
        for k in ('guide', 'n_guide_steps', 't_start_guide'):
            diffusion_kwargs.pop(k, None)           # accepted and unused by the reference samplers
        samples, chain = self.conditional_sample(hard_conds, context=context, batch_size=n_samples, ddim=False,
                                                 return_chain=True, traj_normalized=traj_normalized,
                                                 obstacle_pts=obstacle_pts.to(self._device()), **diffusion_kwargs)
        chain = chain.permute(1, 0, 2, 3)           # 'b diffsteps h d -> diffsteps b h d'
        if return_chain:
            return chain
        return chain[-1]

    def _concat_hard_conds(self, hard_conds, counts):
        """The scenes' hard-condition dicts as the job's one dict: per waypoint, (B, S) values, a scene's samples adjacent."""
        dev = self._device()
        hc = {}
        for k in hard_conds[0].keys():
            rows = []
            for h, n in zip(hard_conds, counts):
                v = h[k].to(dev, torch.float32)
                v = v.unsqueeze(0).expand(n, -1) if v.dim() == 1 else v
                if v.shape[0] != n:
                    raise ValueError(f"hard condition {k}: {v.shape[0]} rows for a scene of {n} samples")
                rows.append(v)
            hc[k] = torch.cat(rows).contiguous()
        return hc

    @torch.no_grad()
    def _prepare_scene_job(self, scenes, hard_conds, n_samples):
        """Encode all scenes in one call (``encode_scenes``), hand latents + row table to the context (``set_scenes``) and build what ``_launch`` needs for
        a multi-scene job: (job dict, concatenated hard conditions, B)."""
        from .scenes import build_scene_tables
        if not self._scenes_supported:
            raise NotImplementedError(f"{type(self).__name__} has no multi-scene job")
        dev = self._device()
        m = self.model
        use_cloud = bool(self.APF and self._supports_apf)
        sizes = [int(s.numel() // 2) if use_cloud else 1 for s in scenes]
        tab = build_scene_tables(sizes, n_samples, [list(h.keys()) for h in hard_conds], n_rp=self._n_rp(), compose=self.compose)
        counts = [int(c) for c in tab['counts']]
        B = int(sum(counts))
        hc = self._concat_hard_conds(hard_conds, counts)
        m.ctx()
        lat = torch.cat([m.encode_scenes([s.to(dev) for s in scenes]), torch.zeros(1, m.context_dim, device=dev)])
        m.set_scenes(lat, tab['row_variant'])
        job = {'n_scenes': len(scenes), 'traj_scene': torch.from_numpy(tab['traj_scene']).to(dev), 'cloud_offset': tab['cloud_offset'],
               'cloud_points': (torch.cat([s.reshape(-1, 2).to(dev, torch.float32) for s in scenes]).contiguous() if use_cloud else None)}
        return job, hc, B

    @torch.no_grad()
    def run_inference_scenes(self, scenes, hard_conds, n_samples=1, return_chain=False, **diffusion_kwargs):
        """Sample MANY scenes in ONE job: the loop over experiment directories of the reference's
        scripts/inference/inference_static.py (one ``run_inference`` per experiment) as one batch.

        scenes      list of ``obstacle_pts`` tensors (n_obstacles, n_points, dim), shapes may differ per scene
        hard_conds  list of one dict per scene, the same waypoint indices in every scene; values (S,) or (n_i, S)
        n_samples   trajectories per scene: an int, or one count per scene

        All scenes are encoded in one call (``ramp_encode_scenes``), the latents (one row per scene plus the shared all-zero
        unconditional row), the row -> latent table and the per-scene APF clouds go to the context, and ONE job runs.  Returns
        ``(result, traj_scene)``: what ``run_inference`` returns for the concatenated batch -- (steps + 1, B, H, S) if
        ``return_chain`` else (B, H, S), a scene's samples adjacent, scenes in order -- and the (B,) int32 scene of each
        trajectory.  A flagged job is repeated exactly as in ``run_inference``.  As in ``run_inference`` the sampler is the model's
        own (``sampler='ddpm'`` -> the fused DDPM job, the DDIM default -> ``ddim_p_sample_loop``; ``conditional_sample`` decides by
        the model's setting, not by its ``ddim`` argument) and ``guide`` / ``n_guide_steps`` / ``t_start_guide`` are accepted and
        unused.  Not supported: compose (``run_inference_composed`` is the composed many-scene job), the dynamic planner,
        a caller-supplied ``sample_fn``."""
        self._refuse_team_outside_the_guide(diffusion_kwargs.get('cost_guide'), diffusion_kwargs.get('resample'), None,
                                            [n_samples] * len(scenes) if np.isscalar(n_samples) else list(n_samples))
        job, hc, B = self._prepare_scene_job(scenes, hard_conds, n_samples)
        for k in ('guide', 'n_guide_steps', 't_start_guide'):
            diffusion_kwargs.pop(k, None)
        _samples, chain = self.conditional_sample(hc, batch_size=B, ddim=False, return_chain=True, obstacle_pts=None, scene_job=job,
                                                  **diffusion_kwargs)
        chain = chain.permute(1, 0, 2, 3)
        return (chain if return_chain else chain[-1]), job['traj_scene']

    @torch.no_grad()
    def run_inference_stitched(self, scenes, hard_conds, n_windows, overlap, n_samples=1, blend='ramp', return_chain=False,
                               return_windows=False, cost_guide=None, **diffusion_kwargs):
        """Plans LONGER than the network's horizon in one job: every one of the ``n_samples`` long trajectories of
        ``L = H + (n_windows - 1)(H - overlap)`` waypoints is ``n_windows`` overlapping windows of ``H`` waypoints in adjacent rows of the batch,
        made to agree on the waypoints they share after every reverse step (``ramp_sample_stitched``; include/ramp_hip.h states the stitch
        and its places in the job, ``ramp_amd.stitch`` its numpy reference).

        scenes      one ``obstacle_pts`` tensor for every window, or a list of ``n_windows`` tensors: window w is conditioned on (and, with
                    APF or ``cost_guide``, avoids the cloud of) its own scene
        hard_conds  ONE dict {long waypoint index: (S,) or (n_samples, S)}, negative indices counted from L -- typically {0: start, -1: goal}
        overlap     1 .. H / 2 shared waypoints of neighbouring windows (not read with one window)
        blend       'ramp' | 'mean' | 'left' (``stitch.blend_weights``) or the (overlap,) weights in [0, 1] themselves
        cost_guide  as in ``run_inference_scenes``, one cloud per window scene.  The job has no hard conditions of its own: the guide sees
                    the pinned values in its target and may move them; the stitch behind it restores them

        Returns (n_samples, L, S); with ``return_chain`` (steps + 1, n_samples, L, S); with ``return_windows`` a pair whose second entry is
        the (..., n_samples * n_windows, H, S) windows.  Sampler choice, Philox or torch noise, the repeat of a flagged job and ``guide`` /
        ``n_guide_steps`` / ``t_start_guide`` are ``run_inference_scenes``'.  Not supported (NotImplementedError): ``mcmc=``, ``resample=``,
        compose, a caller-supplied ``sample_fn``, a noise shard or multi-rank process group, the dynamic planner.  No claim is made about
        plan quality: the network's checkpoints were trained on single windows."""
        import torch.distributed as tdist
        from . import stitch as _st
        if not self._scenes_supported:
            raise NotImplementedError(f"{type(self).__name__} has no stitched job")
        if self.compose:
            raise NotImplementedError("run_inference_stitched: compose is not supported (composed weights with stitching are out of scope)")
        for k in ('mcmc', 'resample'):
            if diffusion_kwargs.get(k) is not None:
                raise NotImplementedError(f"run_inference_stitched: {k}= is not supported (its proposals / ancestors would have to be chain-wise)")
        if guide_has_prims(cost_guide):
            raise NotImplementedError("run_inference_stitched: cost_guide= takes no boxes= / spheres= here (ramp_sample_stitched takes no primitives)")
        if guide_has_team(cost_guide):
            raise NotImplementedError("run_inference_stitched: cost_guide= takes no team= here (ramp_sample_stitched takes no team)")
        if not self._is_fused_ddpm_step(diffusion_kwargs.get('sample_fn')):
            raise NotImplementedError("run_inference_stitched runs the fused job only: a caller-supplied sample_fn steps on its own")
        if self._philox_shard is not None:
            raise NotImplementedError("run_inference_stitched: a noise shard (set_noise_shard) is not supported -- the windows of a chain must sit in one shard")
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            raise NotImplementedError("run_inference_stitched under a multi-rank process group: sharding a stitched job is out of scope")
        dev, m = self._device(), self.model
        H, S, W, Cn = m.n_support_points, self.state_dim, int(n_windows), int(n_samples)
        scene_list = list(scenes) if isinstance(scenes, (list, tuple)) else [scenes]
        if isinstance(scenes, (list, tuple)) and len(scene_list) != W:
            raise ValueError(f"run_inference_stitched: {len(scene_list)} scenes for {W} windows; one tensor for all windows or one per window")
        use_cloud = bool(self.APF and self._supports_apf)
        tab = _st.build_stitch_tables(H, W, overlap, Cn, len(scene_list), list(hard_conds.keys()),
                                      [int(s.numel() // 2) for s in scene_list] if use_cloud else None)
        O = int(overlap) if W > 1 else 0
        sd = {'n_windows': W, 'overlap': O, 'alpha': _st.blend_table(blend, O),'pin_idx': tab['pin_idx'], 'pin_val': _st.pin_values(hard_conds, Cn, S, dev)}
        m.ctx()
        lat = torch.cat([m.encode_scenes([s.to(dev) for s in scene_list]), torch.zeros(1, m.context_dim, device=dev)])
        m.set_scenes(lat, tab['row_variant'])
        job = {'n_scenes': len(scene_list), 'traj_scene': torch.from_numpy(tab['traj_scene']).to(dev), 'cloud_offset': tab.get('cloud_offset'),
               'cloud_points': (torch.cat([s.reshape(-1, 2).to(dev, torch.float32) for s in scene_list]).contiguous() if use_cloud else None)}
        for k in ('guide', 'n_guide_steps', 't_start_guide'):
            diffusion_kwargs.pop(k, None)
        ws = diffusion_kwargs.pop('warm_start', None)
        if ws is not None:      # the prior is LONG, (C, L, S) or (L, S): cut into the windows' rows; the windows of a chain start together
            lv = ws.get('level') if isinstance(ws, dict) else None
            if not (lv is not None and np.isscalar(lv)):
                raise NotImplementedError("run_inference_stitched: warm_start= takes one level for the whole job (mixed levels inside one "
                                          "stitched chain are not served)")
            pl = ws.get('prior')
            pl = (pl.detach().cpu().numpy() if torch.is_tensor(pl) else np.asarray(pl)).astype(np.float32)
            pl = np.broadcast_to(pl[None], (Cn,) + pl.shape) if pl.ndim == 2 else pl
            if pl.ndim != 3 or pl.shape[0] != Cn or pl.shape[2] != S:
                raise ValueError(f"run_inference_stitched: the warm-start prior must be ({Cn}, L, {S}) or (L, {S}); got {tuple(pl.shape)}")
            diffusion_kwargs['warm_start'] = dict(ws, prior=_st.split_long(np.ascontiguousarray(pl), H, W, O))
        _samples, chain = self.conditional_sample({}, batch_size=tab['B'], ddim=False, return_chain=True, obstacle_pts=None, scene_job=job,
                                                  stitch=sd, cost_guide=cost_guide, **diffusion_kwargs)
        windows = chain.permute(1, 0, 2, 3)
        windows = (windows if return_chain else windows[-1]).contiguous()
        long = _st.assemble(windows, W, O)
        return (long, windows) if return_windows else long

    @torch.no_grad()
    def _prepare_composed_job(self, scenes, hard_conds, n_samples, weights=None, apf_clouds=None):
        """Encode all obstacle sets of all scenes in one call (``encode_scenes``), hand latents + row table to the context (``set_scenes``)
        and build what ``_launch`` needs for a composed job: (scene job dict, guidance dict, concatenated hard conditions, B)."""
        from .scenes import build_compose_tables
        dev = self._device()
        m = self.model
        sets = []
        for i, s in enumerate(scenes):
            one = list(s) if (torch.is_tensor(s) and s.dim() == 4) else ([s] if torch.is_tensor(s) else list(s))
            for c in one:
                if not torch.is_tensor(c) or c.dim() != 3:
                    raise ValueError(f"scene {i}: expected a (K, No, Np, D) tensor or a list of (No, Np, D) tensors")
            sets.append(one)
        if weights is None:
            weights = float(self._default_compose[0])
        tab = build_compose_tables([len(s) for s in sets], n_samples, [list(h.keys()) for h in hard_conds], weights)
        counts = [int(c) for c in tab['counts']]
        B = int(sum(counts))
        hc = self._concat_hard_conds(hard_conds, counts)
        use_cloud = bool(self.APF and self._supports_apf)
        cloud_points, cloud_offset = None, np.arange(len(sets) + 1, dtype=np.int32)
        if use_cloud:
            if apf_clouds is not None and len(apf_clouds) != len(sets):
                raise ValueError(f"apf_clouds has {len(apf_clouds)} entries for {len(sets)} scenes")
            # the field of scene i: the caller's cloud, or every point of every set of the scene
            per = [(apf_clouds[i].reshape(-1, 2) if apf_clouds is not None else torch.cat([c.reshape(-1, 2) for c in one]))
                   .to(dev, torch.float32) for i, one in enumerate(sets)]
            from .scenes import build_eval_tables
            cloud_offset = build_eval_tables(counts, cloud_sizes=[int(c.shape[0]) for c in per])['cloud_offset']
            cloud_points = torch.cat(per).contiguous()
        m.ctx()
        lat = torch.cat([m.encode_scenes([c.to(dev) for one in sets for c in one]), torch.zeros(1, m.context_dim, device=dev)])
        m.set_scenes(lat, tab['row_variant'])
        job = {'n_scenes': len(sets), 'traj_scene': torch.from_numpy(tab['traj_scene']).to(dev), 'cloud_offset': cloud_offset,
               'cloud_points': cloud_points}
        guidance = {'n_rp': int(tab['n_rp']), 'row_weight': torch.from_numpy(tab['row_weight']).to(dev).contiguous()}
        return job, guidance, hc, B

    @torch.no_grad()
    def run_inference_composed(self, scenes, hard_conds, n_samples=1, weights=None, apf_clouds=None, return_chain=False,
                               **diffusion_kwargs):
        """Compose ANY number of obstacle sets per trajectory, many scenes in ONE job: the reference's p_mean_variance_compose,
        e = u + sum_k w_k (c_k - u) (diffusion_model_static.py:188-229; diffusion_model_3d.py:163-182, whose three-set form is
        commented-out code at :165-174), with rows and weights as data.

        scenes      per scene a (K_i, No, Np, D) tensor or a list of K_i (No_k, Np_k, D) tensors: its obstacle sets, 1 <= K_i <= 7
        hard_conds  one dict per scene, the same waypoint indices in every scene; values (S,) or (n_i, S)
        n_samples   trajectories per scene: an int, or one count per scene
        weights     None (every set weighs ``_default_compose[0]``: 2 for the 2-D sampler, 5 for the 3-D one), one number, one list
                    of max K_i numbers, or one list per scene (``scenes.build_compose_tables``)
        apf_clouds  per scene the (.., 2) points of its APF field; None: every point of every set of the scene.  The reference's
                    "six obstacles of A plus four of B" rule is ``_compose_apf_cloud``: a caller who wants it passes it

        Every trajectory gets ``max K_i + 1`` network rows; a scene with fewer sets is padded with zero-weight rows that read the
        all-zero latent, and pays their compute.  All sets of all scenes are encoded in one ``encode_scenes`` call, one
        ``set_scenes`` call follows and ONE job (``ramp_sample_composed``) runs.  The sampler is the model's own, as in
        ``run_inference_scenes``: on the fused DDPM job no APF hook fires (the reference's compose path has none); the DDIM loop
        (``ddim_num_inference_steps`` as the constructor set it) applies the three-pass APF to x0 from ``apf_ddim['start']`` against
        each trajectory's own scene cloud when the wrapper was built with ``use_apf``.  The wrapper's ``compose`` flag plays no part.
        Returns ``(result, traj_scene)`` like ``run_inference_scenes``.  Refused with a message: a caller-supplied ``sample_fn``, the
        dynamic planner, a multi-rank process group."""
        import torch.distributed as tdist
        if not self._scenes_supported:
            raise NotImplementedError(f"run_inference_composed: {type(self).__name__} has no composed job (composition in the dynamic "
                                      "planner is out of scope)")
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            raise NotImplementedError("run_inference_composed under a multi-rank process group: sharding a composed job is out of scope")
        if not self._is_fused_ddpm_step(diffusion_kwargs.get('sample_fn')):
            raise NotImplementedError("run_inference_composed runs the fused job only (ddpm_sample_fn): a custom sample_fn steps one "
                                      "scene's batch at a time")
        self._refuse_team_outside_the_guide(diffusion_kwargs.get('cost_guide'), diffusion_kwargs.get('resample'), None,
                                            [n_samples] * len(scenes) if np.isscalar(n_samples) else list(n_samples))
        job, guidance, hc, B = self._prepare_composed_job(scenes, hard_conds, n_samples, weights, apf_clouds)
        for k in ('guide', 'n_guide_steps', 't_start_guide'):
            diffusion_kwargs.pop(k, None)
        _samples, chain = self.conditional_sample(hc, batch_size=B, ddim=False, return_chain=True, obstacle_pts=None, scene_job=job,
                                                  guidance=guidance, **diffusion_kwargs)
        chain = chain.permute(1, 0, 2, 3)
        return (chain if return_chain else chain[-1]), job['traj_scene']

    # ------------------------------------------------------------------ single-step compat API
    def _comb_weights(self):
        """The weights of the rows' gradients (and energies) in the guidance-combined ones, as the library forms them (fp32)."""
        n_rp = self._n_rp()
        w0, w1 = (self.compose_weights if self.compose else (self.cfg_weight, 0.0))
        if n_rp == 1:
            return [1.0]
        if n_rp == 2:
            return [float(np.float32(1.0 + w0)), -float(np.float32(w0))]
        return [float(np.float32(w0)), float(np.float32(w1)), float(np.float32(1.0 - w0 - w1))]

    @torch.no_grad()
    def energy(self, x, t, obstacle_pts) -> torch.Tensor:
        """The guidance-combined energy of each trajectory at timestep t, E[b] = sum_j w_j 1/2 ||f(row j of b)||^2 with the weights that
        form the combined gradient (CFG: (1 + w) E_cond - w E_uncond): the scalar whose gradient ``_x0_mean_eps`` combines.  (B,) float64
        (``ramp_score_energy`` + ``ramp_combine_energy``)."""
        dev = self._device()
        B = x.shape[0]
        ti = int(t.reshape(-1)[0]) if torch.is_tensor(t) else int(t)
        self.model.prepare_time_table(self.n_diffusion_steps)
        pts = obstacle_pts
        if not self.compose and pts.dim() == 4:
            pts = pts[0]
        self._prepare_scene(pts.to(dev), B)
        xx = x.detach().to(dev, torch.float32).contiguous()
        n_rp = self._n_rp()
        e_rows = torch.empty((B * n_rp,), device=dev, dtype=torch.float64)
        out = torch.empty((B,), device=dev, dtype=torch.float64)
        w = self._comb_weights()
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.ramp_score_energy(self.model.ctx(), _lib.ptr(xx), B, n_rp, ti, None, None, _lib.ptr(e_rows),
                                             _lib.current_stream()), "ramp_score_energy")
            _lib.check(lib.ramp_combine_energy(_lib.ptr(e_rows), B, n_rp, (C.c_float * n_rp)(*w), None, _lib.ptr(out),
                                               _lib.current_stream()), "ramp_combine_energy")
        return out

    def _x0_mean_eps(self, x, t, obstacle_pts):
        """``ramp_score`` + ``ramp_cfg_mean`` at timestep t: (x0, posterior mean, guidance-combined eps)."""
        dev = self._device()
        B = x.shape[0]
        ti = int(t.reshape(-1)[0])
        self.model.prepare_time_table(self.n_diffusion_steps)
        pts = obstacle_pts
        if not self.compose and pts.dim() == 4:
            pts = pts[0]                    # the loops replicate one cloud per row; one copy is encoded
        self._prepare_scene(pts.to(dev), B)
        xx = x.detach().to(dev, torch.float32).contiguous()
        n_rp = self._n_rp()
        eps = torch.empty((B * n_rp,) + tuple(x.shape[1:]), device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.ramp_score(self.model.ctx(), _lib.ptr(xx), B, n_rp, ti, None, _lib.ptr(eps),
                                      _lib.current_stream()), "ramp_score")
            x0 = torch.empty_like(xx); mean = torch.empty_like(xx); ec = torch.empty_like(xx)
            w0, w1 = (self.compose_weights if self.compose else (self.cfg_weight, 0.0))
            _lib.check(lib.ramp_cfg_mean(_lib.ptr(xx), _lib.ptr(eps), B, xx[0].numel(), n_rp, float(w0), float(w1),
                                         float(self.sqrt_recip_alphas_cumprod[ti]),
                                         float(self.sqrt_recipm1_alphas_cumprod[ti]),
                                         float(self.posterior_mean_coef1[ti]), float(self.posterior_mean_coef2[ti]),
                                         int(bool(self.clip_denoised)), int(not self.predict_epsilon),
                                         _lib.ptr(x0), _lib.ptr(mean), _lib.ptr(ec),
                                         _lib.current_stream()), "ramp_cfg_mean")
        return x0, mean, ec

    @torch.no_grad()
    def p_mean_variance(self, x, hard_conds, context, t, traj_normalized=None, obstacle_pts=None, forward_t=None,
                        compose=False):
        """One p_mean_variance on the HIP kernels (diffusion_model_static.py:149-186); obstacle_pts is the
        un-batched cloud as passed by the loops.  Returns what the reference returns for the current mode."""
        x0, mean, ec = self._x0_mean_eps(x, t, obstacle_pts)
        pv = extract(self.posterior_variance, t, x.shape)
        plv = extract(self.posterior_log_variance_clipped, t, x.shape)
        if self.ddim:
            return mean, pv, plv, x0, ec
        if (self.APF and self._supports_apf and not self.compose and forward_t is not None
                and forward_t > self.apf_ddpm['after']):
            from .apf import ObstacleField, avoidance
            pts = obstacle_pts[0] if obstacle_pts.dim() == 4 else obstacle_pts      # one copy of the cloud is the field
            field = ObstacleField(pts.reshape(-1, 2), distance_threshold=self.apf_ddpm['threshold'])
            mean = avoidance(mean, field, avoidance_window=self.apf_ddpm['window'],
                             avoidance_strength=self.apf_ddpm['strength'])
        return mean, pv, plv

    _supports_apf = True
    _scenes_supported = True           # run_inference_scenes (the static 2-D and 3-D samplers)

    @torch.no_grad()
    def p_mean_variance_compose(self, x, hard_conds, context, t, traj_normalized=None, obstacle_pts=None, forward_t=None,
                                compose=True):
        """diffusion_model_static.py:188-229 / diffusion_model_3d.py:163-182: the three-row (scene A, scene B, unconditional)
        evaluation; the reference's own ``ddpm_sample_fn`` calls it by this name (sample_functions.py:28).  Same kernels as
        ``p_mean_variance`` on a wrapper built with ``compose=True`` (no APF hook on this path in the reference)."""
        if not self.compose:
            raise ValueError("p_mean_variance_compose needs a wrapper constructed with compose=True (three rows per trajectory)")
        return self.p_mean_variance(x, hard_conds, context, t, traj_normalized=traj_normalized, obstacle_pts=obstacle_pts,
                                    forward_t=None, compose=True)

    def _ddim_finish(self, xx, x0, ti, K):
        """The deterministic DDIM update of one step from (x_t, x0), through the kernel-level entry point."""
        k = self._ddim_coefficients([ti], K)
        out = torch.empty_like(xx)
        B, H, S = xx.shape
        with torch.cuda.device(self._device()):
            _lib.check(_lib.load().ramp_ddim_finish(_lib.ptr(xx), _lib.ptr(x0), float(k['sqrt_a_t'][0]), float(k['sqrt_1m_a_t'][0]),
                                                    float(k['sqrt_a_prev'][0]), float(k['dir_coef'][0]), _lib.ptr(out), B, H, S,
                                                    _lib.current_stream()), "ramp_ddim_finish")
        return out

    @torch.no_grad()
    def ddim_p_sample(self, x, hard_conds, context, t, obstacle_pts, traj_normalized=None, forward_t=None, eta=0.0,
                      use_clipped_model_output=False):
        """One DDIM step of the static sampler (diffusion_model_static.py:259-333, eta = 0): x0 from the CFG / compose
        evaluation, the APF hook (three passes of window 7 with hard conditioning after each) when ``use_apf`` and
        ``forward_t >= 2``, then the deterministic update -- the step ``ramp_sample`` runs inside its captured loop, here one
        at a time through the kernel-level entry points."""
        assert use_clipped_model_output and eta == 0.0
        ti = int(t.reshape(-1)[0])
        x0 = self._x0_mean_eps(x, t, obstacle_pts)[0]
        xx = x.detach().to(self._device(), torch.float32).contiguous()
        c = self.apf_ddim
        if self.APF and self._supports_apf and forward_t is not None and forward_t >= c['start']:
            from .apf import ObstacleField, avoidance
            if self.compose:
                cloud = self._compose_apf_cloud(obstacle_pts)
            else:       # the loop hands over obstacle_pts.unsqueeze(0) (static.py:366); one copy of the cloud is the field
                cloud = (obstacle_pts[0] if obstacle_pts.dim() == 4 else obstacle_pts).reshape(-1, 2)
            field = ObstacleField(cloud, distance_threshold=c['threshold'])
            for _ in range(c['passes']):
                x0 = avoidance(x0, field, avoidance_window=c['window'], avoidance_strength=c['strength'])
                x0 = apply_hard_conditioning(x0, hard_conds)
        return self._ddim_finish(xx, x0.contiguous(), ti, self.ddim_num_inference_steps)


class StaticGaussianDiffusionModel(_GaussianDiffusionBase):
    """2-D sampler: CFG w = 2, compose w1 = w2 = 2, DDIM-5 by default, APF hook."""
    _default_cfg_weight = 2.0          # diffusion_model_static.py:163
    _default_compose = (2.0, 2.0)      # diffusion_model_static.py:205
    _default_ddim = True               # diffusion_model_static.py:41

    # ------------------------------------------------------------------ the denoising loss (evaluation only)
    def _rows_t(self, t, B: int) -> torch.Tensor:
        """t (B,) -> device int32, every entry checked against the schedule on the host (no kernel indexes with an unchecked value)."""
        tv = t.detach().reshape(-1).to("cpu", torch.int64)
        if tv.numel() != B:
            raise ValueError(f"`t` must hold one timestep per row ({B}); got {tv.numel()}")
        if int(tv.min()) < 0 or int(tv.max()) >= self.n_diffusion_steps:
            raise ValueError(f"timesteps must lie in [0, {self.n_diffusion_steps}); got [{int(tv.min())}, {int(tv.max())}]")
        return tv.to(self._device(), torch.int32)

    @torch.no_grad()
    def q_sample(self, x_start, t, noise=None, pin_endpoints: bool = False):
        """diffusion_model_static.py:467-476: sqrt(acp[t]) x_start + sqrt(1 - acp[t]) noise with one t per row, in one launch
        (ramp_q_sample_rows).  ``pin_endpoints`` also overwrites waypoints 0 and H - 1 with x_start's in that launch (p_losses, :483-484)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        dev = self._device()
        xs = x_start.detach().to(dev, torch.float32).contiguous()
        nz = noise.detach().to(dev, torch.float32).contiguous()
        B, H, S = xs.shape
        tr = self._rows_t(t, B)
        out = torch.empty_like(xs)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ramp_q_sample_rows(_lib.ptr(xs), _lib.ptr(nz), _lib.ptr(self.sqrt_alphas_cumprod),
                                                      _lib.ptr(self.sqrt_one_minus_alphas_cumprod), _lib.ptr(tr), self.n_diffusion_steps,
                                                      _lib.ptr(out), B, H, S, int(bool(pin_endpoints)), _lib.current_stream()),
                       "ramp_q_sample_rows")
        return out

    @torch.no_grad()
    def p_losses(self, x_start, context, t, hard_conds, obstacle_pts, noise=None):
        """diffusion_model_static.py:478-505 in eval mode: the denoising loss of the loaded network on x_start at one timestep per
        row.  Returns (loss, info) like the reference, loss a 0-d float32 tensor, info = {'x_noisy', 'x_recon'} (the reference's is
        empty).  ``noise=`` supplies the draw (the reference draws torch.randn_like itself)."""
        if self.training:
            raise NotImplementedError("p_losses in training mode: parameter gradients are out of scope here; call .eval() first")
        if self.loss_type not in ("l2", "l1"):
            raise NotImplementedError(f"loss_type {self.loss_type!r}: only 'l2' and 'l1' are served (helpers.py:91-100)")
        if noise is None:
            noise = torch.randn_like(x_start)
        dev = self._device()
        xs = x_start.detach().to(dev, torch.float32).contiguous()
        nz = noise.detach().to(dev, torch.float32).contiguous()
        B, H, S = xs.shape
        x_noisy = self.q_sample(xs, t, nz, pin_endpoints=True)
        if context is not None:
            context = self.context_model(context)
        x_recon = self.model(x_noisy, t, context, obstacle_pts=obstacle_pts).contiguous()
        target = nz if self.predict_epsilon else xs
        scratch = torch.empty(1024, device=dev, dtype=torch.float64)
        out = torch.empty(1, device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ramp_denoise_loss(_lib.ptr(x_recon), _lib.ptr(xs), _lib.ptr(target), B, H, S,
                                                     int(self.loss_type == "l1"), _lib.ptr(scratch), _lib.ptr(out),
                                                     _lib.current_stream()), "ramp_denoise_loss")
        return out[0].to(torch.float32), {"x_noisy": x_noisy, "x_recon": x_recon, "loss64": out[0]}

    def loss(self, x, context, *args, **kwargs):
        """diffusion_model_static.py:507-511: t = randint(0, T, (B,)) per row, then p_losses(x, context, t, hard_conds, obstacle_pts)."""
        t = torch.randint(0, self.n_diffusion_steps, (x.shape[0],), device=x.device).long()
        return self.p_losses(x, context, t, *args, **kwargs)


class GaussianDiffusionModel3d(_GaussianDiffusionBase):
    """3-D sampler: always DDPM, CFG w = 5.75, compose w1 = w2 = 5, no APF (diffusion_model_3d.py:147-218)."""
    _default_cfg_weight = 5.75         # diffusion_model_3d.py:150
    _default_compose = (5.0, 5.0)      # diffusion_model_3d.py:170-171
    _default_ddim = False
    _supports_apf = False

    def deep_repeat_tensor(self, x, t, traj_normalized, obstacle_pts, n_rp):
        """diffusion_model_3d.py:124-142: blocked ``repeat`` (rows [x_0..x_{B-1}] n_rp times), unlike the static class."""
        rep = lambda v: v.repeat((n_rp,) + (1,) * (v.dim() - 1))
        return rep(x), t.repeat((n_rp,)), rep(traj_normalized), rep(obstacle_pts)


def __getattr__(name):
    # the pursuit-evasion planner lives in diffusion_dynamic.py (which imports this module); re-exported from here on first use
    if name == 'DynamicGaussianDiffusionModel':
        from .diffusion_dynamic import DynamicGaussianDiffusionModel
        return DynamicGaussianDiffusionModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
