#!/usr/bin/env python3
"""Reference fixtures for per-row diffusion timesteps and the denoising loss (runs in the BUILD container only).

Like oracle/make_goldens.py it imports ``mpd.models`` from the reference checkout (``RAMP_REFERENCE``), loads the repo's own
seeded synthetic weights (ramp_amd/synth.py) into the reference ``TemporalUnetInference`` and writes DATA only:

  tests/golden/rowtime_cases.npz
    <tag>/x, t, cloud, latent, f, eps     one score evaluation with ONE TIMESTEP PER ROW (UnetInference.py:198 embeds `time` per row);
                                          t holds 0, T - 1 = 24 and a repeated value
        2d_h48   6 rows   the bench plan: narrow levels on tkc, wide ones on tkw
        3d_h64   6 rows   tkc<NG = 4> at L = 64
        2d_h40   8 rows   level lengths 40/20/10/5: every time bias through gn_fwd_kernel
    loss/x_start, t, noise, cloud, x_noisy, x_recon, loss_l2, loss_l1, predict_epsilon, T
                                          StaticGaussianDiffusionModel.p_losses (diffusion_model_static.py:478-505) in eval mode, 2-D,
                                          H = 48, T = 25, B = 6; `noise` is what the reference's torch.randn_like returned, x_noisy what
                                          it handed to the network, x_recon the network's output after the endpoint overwrite

    python ramp_amd/tools/make_rowtime_goldens.py

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
from ramp_amd import synth  # noqa: E402

T = 25
SCORE_CASES = (   # tag, S, H, 3-D, per-row t, seed
    ("2d_h48", 4, 48, False, [0, 24, 7, 7, 13, 1], 61),
    ("3d_h64", 6, 64, True, [24, 3, 3, 0, 17, 9], 62),
    ("2d_h40", 4, 40, False, [5, 0, 24, 11, 11, 2, 24, 19], 63),
)


def cloud_of(o3):
    return synth.make_cloud(5, 50, 3, seed=44) if o3 else synth.make_cloud(6, 64, 2, seed=42)


def gen_scores(arrs):
    for tag, S, H, o3, t_rows, seed in SCORE_CASES:
        m, sp, _ = G.build_unet(S, H, o3)
        n = len(t_rows)
        cloud = cloud_of(o3)
        x = torch.from_numpy(synth.make_noise((n, H, S), seed=seed))
        t = torch.tensor(t_rows, dtype=torch.long)
        pts = torch.from_numpy(cloud)[None].repeat(n, 1, 1, 1)
        m.reset_cache()
        latent = m.scene_encoder(pts[:1])[0].detach().numpy()
        m.reset_cache()
        eps = m(x, t, None, obstacle_pts=pts).detach()
        m.reset_cache()
        with torch.no_grad():
            f = m.forward_no_energy(x, t, obstacle_pts=pts)
        for k, v in dict(x=x.numpy(), t=t.numpy(), cloud=cloud, latent=latent, f=f.numpy(), eps=eps.numpy()).items():
            arrs[f"{tag}/{k}"] = v


def gen_loss(arrs):
    S, H, B = 4, 48, 6
    m, sp, _ = G.build_unet(S, H, False)
    cloud = cloud_of(False)
    pts = torch.from_numpy(cloud)[None].repeat(B, 1, 1, 1)
    x_start = torch.from_numpy(0.5 * synth.make_noise((B, H, S), seed=71))
    noise = synth.make_noise((B, H, S), seed=72)
    t = torch.tensor([0, 24, 7, 7, 13, 1], dtype=torch.long)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    seen = {}
    fwd = m.forward

    def spy(x, *a, **k):                       # what p_losses hands to the network, and the tensor it gets back (overwritten in place after)
        seen["x_noisy"] = x.detach().clone()
        seen["x_recon"] = fwd(x, *a, **k)
        return seen["x_recon"]

    out = {}
    for lt in ("l2", "l1"):
        dm = G.quiet(G.StaticGaussianDiffusionModel, model=m, variance_schedule="exponential", n_diffusion_steps=T,
                     predict_epsilon=True, loss_type=lt)
        dm.eval()
        assert not dm.training
        m.reset_cache()
        m.forward = spy
        try:
            # (under no_grad, as a held-out evaluation runs: with gradient recording on, the reference's own endpoint overwrite of the
            # network output -- one of two outputs of its autograd Function -- is refused by torch as an in-place write to a view)
            with torch.no_grad(), G.NoiseInjector([torch.from_numpy(noise)]) as inj:
                loss, _ = dm.p_losses(x_start.clone(), None, t, hc, pts)
                assert inj.used == 1
        finally:
            del m.forward
        out[lt] = (float(loss), seen["x_noisy"].numpy(), seen["x_recon"].detach().numpy())
    assert np.array_equal(out["l2"][1], out["l1"][1]) and np.array_equal(out["l2"][2], out["l1"][2])
    for k, v in dict(x_start=x_start.numpy(), t=t.numpy(), noise=noise, cloud=cloud, x_noisy=out["l2"][1], x_recon=out["l2"][2],
                     loss_l2=np.float64(out["l2"][0]), loss_l1=np.float64(out["l1"][0]), predict_epsilon=np.int32(1),
                     T=np.int32(T)).items():
        arrs[f"loss/{k}"] = v


if __name__ == "__main__":
    arrs = {}
    gen_scores(arrs)
    gen_loss(arrs)
    G.save("rowtime_cases.npz", **arrs)
