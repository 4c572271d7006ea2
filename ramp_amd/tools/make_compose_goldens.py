#!/usr/bin/env python3
"""Reference fixtures for composition over MORE THAN TWO obstacle sets (runs in the BUILD container only).

Like oracle/make_goldens.py it imports ``mpd.models`` from the reference checkout (``RAMP_REFERENCE``), loads the repo's own seeded
synthetic weights (ramp_amd/synth.py) into the reference ``TemporalUnetInference`` and writes DATA only: tests/golden/compose_sets.npz.

How the reference is driven.  Its samplers combine e = u + sum_k w_k (c_k - u) (p_mean_variance_compose, diffusion_model_static.py:188-229,
diffusion_model_3d.py:163-182; the three-set form is commented-out code at diffusion_model_3d.py:165-174), but its network hard-wires the
three-row mask (``scene_latents[2::3] = 0``, UnetInference.py:190-191).  So the sampler classes are subclassed here and
``p_mean_variance_compose`` overridden: the network is called with ``compose=False`` on its classifier-free-guidance layout -- rows
``[c_0, u, c_1, u, ...]`` per trajectory, where it zeroes the latent of every odd row (UnetInference.py:192-195) -- and the rows are combined
by the reference's formula, in its association order.  Everything else -- predict_start_from_noise, the clamp, q_posterior, ddpm_sample_fn,
ddim_p_sample, the loops -- is the reference's own code, and every chain comes out of the reference's own ``run_inference``.

  2d/   H = 48, T = 25, B = 3, K = 3; clouds make_cloud(6, 64, 2, seed in (1, 2, 7)); weights (1.5, 1.0, 1.5): sum |row weight| = 7, the
        amplification of the two-set (2, 2) fixture, and unequal so that a weight-order mistake shows
        clouds, weights, latents, pmv_x (make_noise(seed = 3)), pmv_t (9), pmv_ecomb, pmv_x0, pmv_mean    one p_mean_variance_compose
        ddpm_noise (make_noise((26, 3, 48, 4), seed = 2345)), ddpm_chain                                   free-running DDPM chain
  ddim/ the same scene and weights, T = 100, DDIM-5, no APF: noise (make_noise((1, 3, 48, 4), seed = 5433)), chain (6, 3, 48, 4)
  3d/   H = 48, T = 25, B = 2, K = 3; clouds make_cloud(5, 50, 3, seed in (44, 46, 48)); weights (2.5, 2.5, 5.0): sum |row weight| = 19 as the
        two-set (5, 5) fixture; clouds, weights, latents, noise (make_noise((26, 2, 48, 6), seed = 780)), chain stacked from n_samples = 1
        runs as gen_compose3d does

The check behind the bars of tests/test_gpu_compose.py: the reference's fp32 results against a float64 K-set oracle (oracle/ramp_oracle.py's
SamplerOracle with eps_cfg overridden; the reference's own fp32 schedule tables).  Printed by this script; every case must leave at least
3 x room under its bar, else its seeds change, not the bar:

    2-D, K = 3, weights (1.5, 1.0, 1.5)
      single evaluation, reference fp32 vs float64 oracle (e_comb, relative): 7.93e-06  (bar 5e-05, room 6.3 x)
      DDPM chain free-running, reference fp32 vs float64 oracle: 2.35e-05  (bar 2e-04, room 8.5 x)
      DDPM chain teacher-forced, worst step: 8.73e-06  (bar 1e-04, room 11.4 x)
    DDIM-5 of T = 100, the same scene
      DDIM chain free-running, reference fp32 vs float64 oracle: 9.60e-06  (bar 2e-04, room 20.8 x)
      DDIM chain teacher-forced, worst step: 8.30e-06  (bar 1e-04, room 12.0 x)
    3-D, K = 3, weights (2.5, 2.5, 5.0)
      DDPM chain teacher-forced, worst step: 3.02e-05  (bar 1e-04, room 3.3 x)

    python ramp_amd/tools/make_compose_goldens.py

Nothing on the product path and no GPU test imports this file.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import make_goldens as G  # noqa: E402  (puts RAMP_REFERENCE on sys.path and imports mpd.models)
from oracle import ramp_oracle as O  # noqa: E402
from ramp_amd import synth  # noqa: E402

W2D, W3D = (1.5, 1.0, 1.5), (2.5, 2.5, 5.0)
BARS = dict(single=5e-5, free=2e-4, step=1e-4)      # e_comb relative; free-running chain; one teacher-forced step


def composed(base, weights):
    """The reference sampler ``base`` with p_mean_variance_compose over len(weights) obstacle sets (see the module docstring)."""

    class Composed(base):
        set_weights = tuple(float(w) for w in weights)

        def p_mean_variance_compose(self, x, hard_conds, context, t, traj_normalized=None, obstacle_pts=None, forward_t=None, compose=True):
            n, K = x.shape[0], len(self.set_weights)
            assert obstacle_pts.shape[0] == K
            x2, t2 = x.repeat_interleave(2 * K, dim=0), t.repeat_interleave(2 * K, dim=0)
            pts2 = obstacle_pts.repeat_interleave(2, dim=0).repeat((n,) + (1,) * (obstacle_pts.dim() - 1))
            out = self.model(x2, t2, context, x_start=None, obstacle_pts=pts2, forward_t=forward_t, compose=False)
            out = out.view(n, 2 * K, *out.shape[1:])
            u = out[:, 1]                                   # every odd row is unconditional
            e_comb = u
            for k, w in enumerate(self.set_weights):        # u + w1 (c1 - u) + w2 (c2 - u) + ..., the reference's association order
                e_comb = e_comb + w * (out[:, 2 * k] - u)
            x_recon = self.predict_start_from_noise(x, t=t, noise=e_comb)
            x_recon.clamp_(-1., 1.)
            model_mean, posterior_variance, posterior_log_variance = self.q_posterior(x_start=x_recon, x_t=x, t=t)
            if getattr(self, "ddim", False):
                return model_mean, posterior_variance, posterior_log_variance, x_recon, e_comb
            return model_mean, posterior_variance, posterior_log_variance

    return Composed


class KSetOracle(O.SamplerOracle):
    """SamplerOracle over K obstacle sets: latents (K, ctx), e = u + sum_k w_k (c_k - u) (the same class lives in tests/test_gpu_compose.py)."""

    def __init__(self, *a, set_weights, **k):
        super().__init__(*a, **k)
        self.set_weights = tuple(set_weights)

    def eps_cfg(self, x, t, latents):
        B, K = x.shape[0], len(self.set_weights)
        lat = np.zeros((B, K + 1, latents.shape[1]), self.dt)
        lat[:, :K] = latents
        out = self.unet.score(np.repeat(x, K + 1, axis=0), np.full((B * (K + 1),), t, np.int64), lat.reshape(B * (K + 1), -1))
        out = out.reshape(B, K + 1, *x.shape[1:])
        e = out[:, K]
        for k, w in enumerate(self.set_weights):
            e = e + self.dt(w) * (out[:, k] - out[:, K])
        return e.astype(self.dt)


def run_kwargs(H, S, pts):
    return dict(horizon=H, return_chain=True, traj_normalized=torch.zeros(H, S), obstacle_pts=pts, sample_fn=G.ddpm_sample_fn, guide=None,
                n_guide_steps=1, t_start_guide=7, noise_std_extra_schedule_fn=lambda x: 0.5, n_diffusion_steps_without_noise=0)


def report(name, got, bar):
    room = bar / max(got, 1e-30)
    print(f"  {name}: {got:.2e}  (bar {bar:.0e}, room {room:.1f} x)")
    assert room >= 3.0, f"{name} leaves {room:.1f} x under its bar: change the seeds"


def gen_2d(arrs):
    S, H, B = 4, 48, 3
    m, sp, sd = G.build_unet(S, H, False)
    clouds = np.stack([synth.make_cloud(6, 64, 2, seed=s) for s in (1, 2, 7)])
    pts = torch.from_numpy(clouds)
    hcn = synth.default_hard_conds(S, H)
    hc = {k: torch.from_numpy(v) for k, v in hcn.items()}
    cls = composed(G.StaticGaussianDiffusionModel, W2D)
    m.reset_cache()
    lats = m.scene_encoder(pts).detach().numpy()
    m.reset_cache()
    uo = O.UNetOracle(sd, S, H, dtype=np.float64)
    lats64 = np.stack([uo.encode_scene(c) for c in clouds])
    golden = os.path.join(REPO, "tests", "golden")
    # (1) one p_mean_variance_compose
    dm = G.quiet(cls, model=m, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True, compose=True, use_apf=False)
    dm.eval(); dm.ddim = True
    x = synth.make_noise((B, H, S), seed=3)
    t = torch.full((B,), 9, dtype=torch.long)
    mean, _, _, x0, ec = dm.p_mean_variance_compose(torch.from_numpy(x.copy()), None, None, t, obstacle_pts=pts)
    m.reset_cache()
    so = KSetOracle(uo, 25, dtype=np.float64, sched=dict(np.load(f"{golden}/schedule_T25.npz")), set_weights=W2D)
    e64 = so.eps_cfg(x.astype(np.float64), 9, lats64)
    print("2-D, K = 3, weights", W2D)
    report("single evaluation, reference fp32 vs float64 oracle (e_comb, relative)",
           float(np.abs(ec.detach().numpy() - e64).max() / np.abs(e64).max()), BARS["single"])
    arrs.update({"2d/clouds": clouds, "2d/weights": np.asarray(W2D), "2d/latents": lats, "2d/pmv_x": x, "2d/pmv_t": 9,
                 "2d/pmv_mean": mean.detach().numpy(), "2d/pmv_x0": x0.detach().numpy(), "2d/pmv_ecomb": ec.detach().numpy()})
    # (2) the free-running DDPM chain
    dm = G.quiet(cls, model=m, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True, compose=True, use_apf=True)
    dm.eval(); dm.ddim = False
    noise = synth.make_noise((26, B, H, S), seed=2345)
    with G.NoiseInjector([torch.from_numpy(n) for n in noise]) as inj:
        chain = dm.run_inference(None, hc, n_samples=B, **run_kwargs(H, S, pts)).detach().numpy()
        assert inj.used == 26 and chain.shape == (26, B, H, S)
    m.reset_cache()
    free = so.ddpm(noise, hcn, lats64)
    tf = so.ddpm(noise, hcn, lats64, teacher=chain)
    report("DDPM chain free-running, reference fp32 vs float64 oracle", float(np.abs(chain - free).max()), BARS["free"])
    report("DDPM chain teacher-forced, worst step", float(np.abs(chain - tf).reshape(26, -1).max(1).max()), BARS["step"])
    arrs.update({"2d/ddpm_noise": noise, "2d/ddpm_chain": chain})
    # (3) DDIM-5 of T = 100, no APF
    dm = G.quiet(cls, model=m, variance_schedule="exponential", n_diffusion_steps=100, predict_epsilon=True, compose=True, use_apf=False)
    dm.eval()
    assert dm.ddim and dm.ddim_num_inference_steps == 5
    noise = synth.make_noise((1, B, H, S), seed=5433)
    with G.NoiseInjector([torch.from_numpy(n) for n in noise]) as inj:
        chain = dm.run_inference(None, hc, n_samples=B, **run_kwargs(H, S, pts)).detach().numpy()
        assert inj.used == 1 and chain.shape == (6, B, H, S)
    m.reset_cache()
    so100 = KSetOracle(uo, 100, dtype=np.float64, sched=dict(np.load(f"{golden}/schedule_T100.npz")), set_weights=W2D)
    print("DDIM-5 of T = 100, the same scene")
    report("DDIM chain free-running, reference fp32 vs float64 oracle", float(np.abs(chain - so100.ddim(noise[0], hcn, lats64, K=5)).max()), BARS["free"])
    report("DDIM chain teacher-forced, worst step",
           float(np.abs(chain - so100.ddim(noise[0], hcn, lats64, K=5, teacher=chain)).reshape(6, -1).max(1).max()), BARS["step"])
    arrs.update({"ddim/noise": noise, "ddim/chain": chain})


def gen_3d(arrs):
    S, H, T, B = 6, 48, 25, 2
    m, sp, sd = G.build_unet(S, H, True)
    clouds = np.stack([synth.make_cloud(5, 50, 3, seed=s) for s in (44, 46, 48)])
    pts = torch.from_numpy(clouds)
    noise = synth.make_noise((T + 1, B, H, S), seed=780)
    hcn = synth.default_hard_conds(S, H)
    cls = composed(G.GaussianDiffusionModel3d, W3D)
    chains = []
    for b in range(B):
        dm = G.quiet(cls, model=m, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True, compose=True, use_apf=False)
        dm.eval()
        m.reset_cache()
        hc = {k: torch.from_numpy(v) for k, v in hcn.items()}
        with G.NoiseInjector([torch.from_numpy(noise[j, b:b + 1]) for j in range(T + 1)]) as inj:
            chain = dm.run_inference(None, hc, n_samples=1, **run_kwargs(H, S, pts))
            assert inj.used == T + 1
        chains.append(chain.detach().numpy())
    m.reset_cache()
    chain = np.concatenate(chains, axis=1)
    lats = m.scene_encoder(pts).detach().numpy()
    m.reset_cache()
    uo = O.UNetOracle(sd, S, H, obstacle_3d=True, dtype=np.float64)
    lats64 = np.stack([uo.encode_scene(c) for c in clouds])
    so = KSetOracle(uo, T, dtype=np.float64, sched=dict(np.load(os.path.join(REPO, "tests", "golden", f"schedule_T{T}.npz"))), set_weights=W3D)
    tf = so.ddpm(noise, hcn, lats64, teacher=chain)
    print("3-D, K = 3, weights", W3D)
    report("DDPM chain teacher-forced, worst step", float(np.abs(chain - tf).reshape(T + 1, -1).max(1).max()), BARS["step"])
    arrs.update({"3d/clouds": clouds, "3d/weights": np.asarray(W3D), "3d/latents": lats, "3d/noise": noise, "3d/chain": chain, "3d/T": T})


if __name__ == "__main__":
    arrs = {}
    gen_2d(arrs)
    gen_3d(arrs)
    G.save("compose_sets.npz", **arrs)
