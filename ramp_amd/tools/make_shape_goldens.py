#!/usr/bin/env python3
"""Reference fixtures for the network shapes beyond the default (1,2,4,8) / unet_input_dim = 32 (runs in the BUILD container only).

Like oracle/make_goldens.py it imports ``mpd.models`` from the reference checkout (``RAMP_REFERENCE``), loads the repo's own
seeded synthetic weights (ramp_amd/synth.py) into the reference ``TemporalUnetInference`` built with ``dim_mults`` /
``unet_input_dim``, asserts that the key names and shapes agree with ramp_amd/spec.py, and writes DATA only to tests/golden/:

  unet_shape_state_dicts.json   the reference state_dict listing (name -> shape) of all six shapes at S = 4, H = 48
  unet2d_h48_dm0.npz            (1,2,4) / 32, 2-D, H = 48      one cond / uncond score evaluation (x, t, cloud, latent, temb, f,
  unet2d_h48_c16.npz            (1,2,4,8) / 16, 2-D, H = 48    eps) with the output / output-gradient taps of three modules
  unet2d_h48_c64.npz            (1,2,4,8) / 64, 2-D, H = 48
  unet3d_h64_dm0_c64.npz        (1,2,4) / 64, 3-D, H = 64
  chain_ddpm_dm0.npz            run_inference, 2-D, (1,2,4) / 32, H = 48, T = 25, DDPM, CFG, recorded noise (as chain_ddpm_plain.npz)

    python ramp_amd/tools/make_shape_goldens.py

Nothing on the product path and no GPU test imports this file.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

from oracle import make_goldens as G  # noqa: E402  (puts RAMP_REFERENCE on sys.path and imports mpd.models)
from ramp_amd import synth  # noqa: E402
from ramp_amd.spec import UNET_DIM_MULTS, make_unet_spec  # noqa: E402

SHAPES = [(opt, c0) for opt in (0, 1) for c0 in (16, 32, 64)]           # (unet_dim_mults_option, unet_input_dim)
SCORE_CASES = (   # tag, option, C0, S, H, 3-D, t, seed
    ("2d_h48_dm0", 0, 32, 4, 48, False, 7, 51),
    ("2d_h48_c16", 1, 16, 4, 48, False, 13, 52),
    ("2d_h48_c64", 1, 64, 4, 48, False, 19, 53),
    ("3d_h64_dm0_c64", 0, 64, 6, 64, True, 3, 54),
)


def shape_tag(opt, c0):
    return f"dm{opt}_c{c0}"


def build_unet(state_dim, horizon, obstacle_3d, opt, c0, seed=0):
    """The reference U-Net of that shape carrying synth weights; asserts the spec's key names and shapes."""
    dm = UNET_DIM_MULTS[opt]
    sp = make_unet_spec(state_dim, horizon, c0, dm, obstacle_3d)
    sd = synth.make_unet_state_dict(sp, seed=seed)
    m = G.quiet(G.TemporalUnetInference, n_support_points=horizon, state_dim=state_dim, unet_input_dim=c0,
                dim_mults=G.UNET_DIM_MULTS[opt], obstacle_3d=obstacle_3d)
    ref_sd = m.state_dict()
    assert set(ref_sd.keys()) == set(sd.keys()), "spec.py key name mismatch with reference"
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(sd[k].shape), (k, v.shape, sd[k].shape)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m, sp


def few_taps(sp):
    """The finest level's first block, the deepest block and the last up level's second block: the 16 / 512-channel ends."""
    return ["downs.0.0", "mid_block1", f"ups.{len(sp.ups) - 1}.1"]


def gen_listings():
    out = {}
    for opt, c0 in SHAPES:
        m, _ = build_unet(4, 48, False, opt, c0)
        out[shape_tag(opt, c0)] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    path = os.path.join(G.OUT, "unet_shape_state_dicts.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print(f"  wrote unet_shape_state_dicts.json: {os.path.getsize(path) / 1024:.1f} KiB")


def gen_scores():
    names = G.module_names
    try:
        for tag, opt, c0, S, H, o3, t_val, seed in SCORE_CASES:
            m, sp = build_unet(S, H, o3, opt, c0)
            G.module_names = few_taps
            cloud = synth.make_cloud(5, 50, 3, seed=44) if o3 else synth.make_cloud(6, 64, 2, seed=42)
            G.gen_unet(tag, m, sp, cloud, 2, t_val, seed=seed)
    finally:
        G.module_names = names


def gen_chain():
    m, sp = build_unet(4, 48, False, 0, 32)
    B, H, S, T = 4, 48, 4, 25
    cloud = synth.make_cloud(6, 64, 2, seed=42)
    m.reset_cache()
    latent = m.scene_encoder(torch.from_numpy(cloud)[None])[0].detach().numpy()
    noise = synth.make_noise((T + 1, B, H, S), seed=1234)
    chain, used = G.run_static(m, sp, T, B, cloud, noise, ddim=False, use_apf=False)
    assert used == T + 1 and chain.shape == (T + 1, B, H, S), (used, chain.shape)
    G.save("chain_ddpm_dm0.npz", chain=chain, noise=noise, cloud=cloud, latent=latent, T=T, n_without_noise=0, use_apf=False)


if __name__ == "__main__":
    gen_listings()
    gen_scores()
    gen_chain()
