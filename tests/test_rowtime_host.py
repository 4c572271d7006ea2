"""Per-row diffusion timesteps and the denoising loss, the host side: the new entry points in the header, the ctypes prototypes and the
library's export table; the oracle against the reference's per-row evaluations (tests/golden/rowtime_cases.npz, written by
ramp_amd/tools/make_rowtime_goldens.py); the loss restated in numpy against the reference's x_noisy and loss; the refusals that need
no device.  Runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib
from util import GOLDEN, rel, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ramp_score_rows", "ramp_op_groupnorm_rows", "ramp_op_tkw_rows", "ramp_q_sample_rows", "ramp_denoise_loss")
SCORE_CASES = [("2d_h48", 4, 48, False), ("3d_h64", 6, 64, True), ("2d_h40", 4, 40, False)]


@pytest.fixture(scope="module")
def cases():
    return np.load(f"{GOLDEN}/rowtime_cases.npz")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h"), encoding="utf-8").read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
        assert hasattr(lib, name), f"{name} not exported"
    # (ctx, x, B, n_rp, t_rows_host, f_out, eps_out, stream): ramp_score's with the scalar t replaced by a host int32 array
    res, args = _lib.PROTOTYPES["ramp_score_rows"]
    ref = list(_lib.PROTOTYPES["ramp_score"][1])
    ref[4] = _lib.c_i32p
    assert res is C.c_int and args == ref
    at = hdr.index("int ramp_score_rows(")
    doc = hdr[hdr.rindex("/*", 0, at):at]
    assert "UnetInference.py:198" in doc and "HOST" in doc and "before anything is launched" in doc


def test_fixture_covers_what_it_must(cases):
    """t holds 0, T - 1 and a repeated value in every score case; few rows."""
    for tag, S, H, o3 in SCORE_CASES:
        t = cases[f"{tag}/t"]
        assert 6 <= t.size <= 8 and cases[f"{tag}/x"].shape == (t.size, H, S)
        assert 0 in t and 24 in t and len(set(t.tolist())) < t.size, (tag, t)
    assert cases["loss/x_start"].shape == (6, 48, 4) and int(cases["loss/T"]) == 25


def _latents(cases, tag, o3, dtype):
    n = cases[f"{tag}/t"].size
    lats = np.tile(cases[f"{tag}/latent"][None].astype(dtype), (n, 1))
    if o3:
        lats[1] = 0                     # UnetInference.py:196-197
    else:
        lats[1::2] = 0                  # UnetInference.py:192-195
    return lats


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("tag,S,H,o3", SCORE_CASES)
def test_oracle_takes_per_row_timesteps_like_the_reference(cases, tag, S, H, o3, dtype):
    u = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=dtype)
    x, t = cases[f"{tag}/x"].astype(dtype), cases[f"{tag}/t"]
    lats = _latents(cases, tag, o3, dtype)
    ef = rel(u.forward_no_energy(x, t, lats), cases[f"{tag}/f"])
    ee = rel(u.score(x, t, lats), cases[f"{tag}/eps"])
    print(f"{tag} {np.dtype(dtype).name}: f {ef:.2e} eps {ee:.2e}")
    assert ef < 2e-5 and ee < 5e-5
    # and the per-row evaluation is not a uniform one in disguise: at one shared timestep the rows that carry another differ visibly
    shared = np.full_like(t, t[0])
    assert rel(u.forward_no_energy(x, shared, lats), cases[f"{tag}/f"]) > 1e-2


def test_loss_restated_in_numpy_reproduces_the_reference(cases):
    """diffusion_model_static.py:467-505 and helpers.py:71-100 in fp32 numpy on the fixture's own x_recon."""
    from ramp_amd.diffusion import exponential_beta_schedule
    g = {k.split("/")[1]: cases[k] for k in cases.files if k.startswith("loss/")}
    ac = torch.cumprod(1. - exponential_beta_schedule(int(g["T"])), axis=0)
    sa, s1a = torch.sqrt(ac).numpy(), torch.sqrt(1. - ac).numpy()
    t = g["t"]
    xn = sa[t][:, None, None] * g["x_start"] + s1a[t][:, None, None] * g["noise"]
    xn[:, 0] = g["x_start"][:, 0]; xn[:, -1] = g["x_start"][:, -1]
    assert xn.dtype == np.float32 and rel(xn, g["x_noisy"]) < 1e-6
    xr = g["x_recon"]
    assert np.array_equal(xr[:, 0], g["x_start"][:, 0]) and np.array_equal(xr[:, -1], g["x_start"][:, -1])
    target = g["noise"] if int(g["predict_epsilon"]) else g["x_start"]
    d = (xr - target).astype(np.float32)
    l2 = float(np.mean((d * d).astype(np.float64))); l1 = float(np.mean(np.abs(d).astype(np.float64)))
    # the reference's own mean is an fp32 reduction over 1152 non-negative terms: a few 2^-24 relative
    assert abs(l2 - float(g["loss_l2"])) < 1e-6 * l2 and abs(l1 - float(g["loss_l1"])) < 1e-6 * l1


def test_time_argument_refusals():
    from ramp_amd.unet import _split_time
    assert _split_time(7, 6) == (7, None)
    assert _split_time(torch.tensor([7]), 6) == (7, None)
    assert _split_time(torch.full((6,), 7), 6) == (7, None)
    t, rows = _split_time(torch.tensor([0, 24, 7, 7, 13, 1]), 6)
    assert t is None and rows.dtype == np.int32 and rows.tolist() == [0, 24, 7, 7, 13, 1]
    with pytest.raises(ValueError, match="one per row"):
        _split_time(torch.tensor([1, 2, 3]), 6)
    with pytest.raises(ValueError, match="one per row"):
        _split_time(torch.full((5,), 3), 6)
    with pytest.raises(ValueError, match="non-negative"):
        _split_time(torch.tensor([0, -1, 2, 3, 4, 5]), 6)
    with pytest.raises(ValueError, match="non-negative"):
        _split_time(-1, 6)


def _host_wrapper(loss_type="l2", training=False):
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    u = TemporalUnetInference(n_support_points=48, state_dim=4)
    dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=25, predict_epsilon=True, loss_type=loss_type)
    return dm.train() if training else dm.eval()


def test_loss_refusals_that_need_no_device():
    x = torch.zeros(6, 48, 4)
    t = torch.tensor([0, 24, 7, 7, 13, 1])
    with pytest.raises(NotImplementedError, match="l2smooth"):
        _host_wrapper("l2smooth").p_losses(x, None, t, {}, None)
    with pytest.raises(NotImplementedError, match="training"):
        _host_wrapper(training=True).p_losses(x, None, t, {}, None)
    dm = _host_wrapper()
    with pytest.raises(ValueError, match=r"\[0, 25\)"):
        dm.q_sample(x, torch.tensor([0, 25, 7, 7, 13, 1]), torch.zeros_like(x))
    with pytest.raises(ValueError, match=r"\[0, 25\)"):
        dm.q_sample(x, torch.tensor([0, -1, 7, 7, 13, 1]), torch.zeros_like(x))
    with pytest.raises(ValueError, match="one timestep per row"):
        dm.q_sample(x, torch.tensor([0, 1, 2]), torch.zeros_like(x))
