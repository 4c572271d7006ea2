"""The network shapes of the reference's configuration beyond the default: unet_dim_mults_option 0 = (1, 2, 4) and
unet_input_dim 16 / 64 (UnetInference.py:13-16, 40-56).  CPU only: ramp_create's shape rule, the spec against the reference's
state_dict listings and both CPU models against the reference's score evaluations (ramp_amd/tools/make_shape_goldens.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.spec import UNET_DIM_MULTS, make_unet_spec, unet_param_shapes

G = os.path.join(os.path.dirname(__file__), "golden")

ACCEPTED = [(nl, c0) for nl in (3, 4) for c0 in (16, 32, 64)]
REFUSED = [(2, 32), (5, 32), (4, 8), (4, 48), (3, 128), (4, 128)]
# tag, unet_dim_mults_option, unet_input_dim, S, H, 3-D
SCORE_CASES = [("2d_h48_dm0", 0, 32, 4, 48, False), ("2d_h48_c16", 1, 16, 4, 48, False),
               ("2d_h48_c64", 1, 64, 4, 48, False), ("3d_h64_dm0_c64", 0, 64, 6, 64, True)]


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


def shape_weights(S, H, o3, opt, c0):
    return synth.make_unet_state_dict(make_unet_spec(S, H, c0, UNET_DIM_MULTS[opt], o3))


def create(n_levels, c0, S=4, H=48):
    """ramp_create -> (rc, message); a context that was made is destroyed again."""
    lib = _lib.load()
    cfg = _lib.RampConfig(S, H, c0, n_levels, 320, 16, 0, 0)
    h = C.c_void_p()
    rc = lib.ramp_create(C.byref(cfg), C.byref(h))
    msg = lib.ramp_last_error().decode() if rc != 0 else ""
    if rc == 0:
        lib.ramp_destroy(h)
    return rc, msg


@pytest.mark.parametrize("n_levels,c0", ACCEPTED)
def test_ramp_create_accepts_the_reference_shapes(n_levels, c0):
    """Both depths x C0 in {16, 32, 64} pass the shape rule: on a host without a HIP device the only refusal left is the
    missing device; with one, the context is made."""
    rc, msg = create(n_levels, c0)
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc != 0 and "device" in msg.lower(), msg
        assert "network shape" not in msg


@pytest.mark.parametrize("n_levels,c0", REFUSED)
def test_ramp_create_refuses_other_shapes_naming_the_accepted_sets(n_levels, c0):
    rc, msg = create(n_levels, c0)
    assert rc != 0
    assert "network shape" in msg and "{3, 4}" in msg and "{16, 32, 64}" in msg, msg


@pytest.mark.parametrize("n_levels", [3, 4])
def test_horizon_rule_is_unchanged_for_both_depths(n_levels):
    """A multiple of 8 in [8, 64] at both depths: option 0's extra multiples of 4 stay refused."""
    for H, ok in ((8, True), (64, True), (44, False), (20, False), (72, False)):
        rc, msg = create(n_levels, 32, H=H)
        assert ("horizon" in msg) != ok, (H, msg)


def test_python_model_refuses_early_with_the_engine_wording():
    from ramp_amd.models import TemporalUnetInference
    for kw in (dict(dim_mults=(1, 2)), dict(dim_mults=(1, 2, 4, 8, 16)), dict(unet_input_dim=48), dict(unet_input_dim=128)):
        with pytest.raises(ValueError, match="network shape"):
            TemporalUnetInference(n_support_points=48, state_dim=4, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        TemporalUnetInference(n_support_points=44, state_dim=4, dim_mults=(1, 2, 4))
    for dm in UNET_DIM_MULTS.values():
        for c0 in (16, 32, 64):
            u = TemporalUnetInference(n_support_points=48, state_dim=4, dim_mults=dm, unet_input_dim=c0)
            assert u.spec.dims == [4] + [c0 * m for m in dm]


@pytest.mark.parametrize("opt,c0", [(o, c) for o in (0, 1) for c in (16, 32, 64)])
def test_spec_matches_the_reference_state_dict_listing(opt, c0):
    listing = json.load(open(f"{G}/unet_shape_state_dicts.json"))[f"dm{opt}_c{c0}"]
    ours = unet_param_shapes(make_unet_spec(4, 48, c0, UNET_DIM_MULTS[opt], False))
    assert {k: tuple(v) for k, v in listing} == {k: tuple(v) for k, v in ours.items()}


@pytest.mark.parametrize("tag,opt,c0,S,H,o3", SCORE_CASES)
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_oracle_reproduces_the_shape_fixtures(tag, opt, c0, S, H, o3, dt):
    g = np.load(f"{G}/unet{tag}.npz")
    u = O.UNetOracle(shape_weights(S, H, o3, opt, c0), S, H, unet_input_dim=c0, dim_mults=UNET_DIM_MULTS[opt],
                     obstacle_3d=o3, dtype=dt)
    assert rel(u.encode_scene(g["cloud"]), g["latent"]) < 5e-6
    N = g["x"].shape[0]
    lats = np.tile(g["latent"][None], (N, 1))
    lats[1::2] = 0
    assert rel(u.time_embedding(g["t"]), g["temb"]) < 2e-6
    taps, gt = {}, {}
    f = u.forward_no_energy(g["x"], g["t"], lats, taps=taps)
    eps = u.score(g["x"], g["t"], lats, grad_taps=gt)
    assert rel(f, g["f"]) < 1e-5
    assert rel(eps, g["eps"]) < 2e-5
    n_taps = 0
    for k in g.files:
        if k.startswith("out/"):
            assert rel(taps[k[4:]], g[k]) < 1e-5, k; n_taps += 1
        if k.startswith("gout/"):
            assert rel(gt[k[5:]], g[k]) < 2e-5, k; n_taps += 1
    assert n_taps == 6


@pytest.mark.parametrize("tag,opt,c0,S,H,o3", SCORE_CASES)
def test_torch_cpu_model_reproduces_the_shape_fixtures(tag, opt, c0, S, H, o3):
    from oracle.torch_cpu import TorchCpuScoreNet
    g = np.load(f"{G}/unet{tag}.npz")
    net = TorchCpuScoreNet(shape_weights(S, H, o3, opt, c0), S, H, n_levels=len(UNET_DIM_MULTS[opt]))
    N = g["x"].shape[0]
    lats = np.tile(g["latent"][None], (N, 1))
    lats[1::2] = 0
    x, t, lat = torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(lats)
    assert rel(net.f(x, t, lat).detach().numpy(), g["f"]) < 1e-5
    assert rel(net.score(x, t, lat).numpy(), g["eps"]) < 2e-5


def test_chain_fixture_of_option_0_is_a_reference_run():
    g = np.load(f"{G}/chain_ddpm_dm0.npz")
    assert g["chain"].shape == (26, 4, 48, 4) and g["noise"].shape == (26, 4, 48, 4) and int(g["T"]) == 25
    hc = synth.default_hard_conds(4, 48)
    for i, v in hc.items():
        assert np.array_equal(g["chain"][-1][:, i], np.broadcast_to(v, (4, 4)))


def _tw_lds(L, N, K):
    """tkw.hip tw_geometry restated: LDS bytes of a block (96-token tile + 2 zero rows per sample, K in chunks of <= 128 channels,
    halved until the tile and the 8 KB scratch fit 80 KB), or None where the kernel refuses the shape."""
    if L < 3 or 96 % L or N not in (128, 256, 512, 1024) or K < 32 or K > 1024 or K & (K - 1):
        return None
    rows = 96 + 2 * (96 // L + 1)
    KC = min(K, 128)
    while KC > 32 and rows * (4 * KC + 16) + 8192 > 80 * 1024:
        KC //= 2
    lds = rows * (4 * KC + 16) + 8192
    return lds if lds <= 80 * 1024 and K % KC == 0 else None


def test_tkw_wide_instantiations_fit_two_blocks_per_cu():
    """The tkw variants the unet_input_dim = 64 network adds: the 512-channel GroupNorm epilogue (tkw_kernel2<0, 2>) keeps 256 registers
    at most and parks no more than the 256-channel epilogue variant it mirrors (tkw_kernel2<0, 1>, unchanged); the geometry of the new
    (L, N, K) launches -- N = 512 forward, K = 1024 from two sources, N = 1024 input gradient, at every wide level length -- fits
    80 KB of LDS (two blocks per CU), and 2048-wide operands or outputs are refused."""
    import test_host_cpu as T
    notes = T._kernel_notes("tkw.o")
    new = [v for k, v in notes.items() if "tkw_kernel2ILi0ELi2E" in k]
    old = [v for k, v in notes.items() if "tkw_kernel2ILi0ELi1E" in k]
    assert len(new) == 1 and len(old) == 1, list(notes)
    assert new[0]["vgpr_count"] <= 256
    assert new[0]["vgpr_spill_count"] <= old[0]["vgpr_spill_count"], (new, old)
    assert new[0]["private_segment_fixed_size"] <= old[0]["private_segment_fixed_size"], (new, old)
    for L in (3, 4, 6, 8, 12):
        for N, K in ((512, 256), (512, 512), (256, 1024), (1024, 256), (1024, 512)):
            lds = _tw_lds(L, N, K)
            assert lds is not None and lds <= 80 * 1024, (L, N, K, lds)
    for N, K in ((2048, 256), (256, 2048)):
        assert _tw_lds(6, N, K) is None
