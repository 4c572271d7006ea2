"""The network shapes beyond the default on the GPU: unet_dim_mults_option 0 = (1, 2, 4) and unet_input_dim 16 / 64
(UnetInference.py:13-16, 40-56) against the reference's fixtures (ramp_amd/tools/make_shape_goldens.py) and the float64 oracle.
At C0 = 16 the 16-wide operands run on the narrow fp32 GEMM (gemm.hip, K % 32 != 0) and the 16-channel GroupNorm; at C0 = 64
with (1,2,4,8) the 512-channel GroupNorm; every other launch on the kernels of the default network."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.spec import UNET_DIM_MULTS, make_unet_spec
import util
from util import GOLDEN, NoiseInjector, dev, rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tag, unet_dim_mults_option, unet_input_dim, S, H, 3-D
SCORE_CASES = [("2d_h48_dm0", 0, 32, 4, 48, False), ("2d_h48_c16", 1, 16, 4, 48, False),
               ("2d_h48_c64", 1, 64, 4, 48, False), ("3d_h64_dm0_c64", 0, 64, 6, 64, True)]
_SD = {}


def shape_weights(S, H, o3, opt, c0):
    key = (S, o3, opt, c0)
    if key not in _SD:
        _SD[key] = synth.make_unet_state_dict(make_unet_spec(S, H, c0, UNET_DIM_MULTS[opt], o3))
    return _SD[key]


def build_shape_unet(S, H, o3, opt, c0, max_rows=8, debug=False, gemm_mode="default", launch_plan=None):
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.unet import load_numpy_state_dict
    m = TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=o3, unet_input_dim=c0, dim_mults=UNET_DIM_MULTS[opt],
                              max_rows=max_rows, debug_taps=debug, gemm_mode=gemm_mode, launch_plan=launch_plan)
    load_numpy_state_dict(m, shape_weights(S, H, o3, opt, c0))
    return m.eval().to("cuda")


@pytest.mark.parametrize("gemm_mode", ["fp32", "bf16x6", "fp16x3", "fp16x3-tkw"])
@pytest.mark.parametrize("tag,opt,c0,S,H,o3", SCORE_CASES)
def test_shape_score_against_reference_fixture(tag, opt, c0, S, H, o3, gemm_mode):
    """forward_no_energy, eps, the scene latent, the time embedding and the module taps of the reference at each new shape,
    with the bars of test_score_against_reference_fixture; in fp16x3 the compared evaluations are the ones after calibration."""
    g = np.load(f"{GOLDEN}/unet{tag}.npz")
    base, plan = util.split_mode(gemm_mode)
    m = build_shape_unet(S, H, o3, opt, c0, debug=True, gemm_mode=base, launch_plan=plan)
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    if base == "fp16x3":
        assert m.score_mode() == "bf16x6"
        f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    else:
        m.reset_cache()
    eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    if base == "fp16x3":
        assert m.score_mode() == "bf16x6"
        eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    assert m.score_mode() == base
    assert rel(m.cached_scene_latents[0].cpu().numpy(), g["latent"]) < 5e-6
    assert rel(m.time_embedding(int(g["t"][0])).cpu().numpy(), g["temb"][0]) < 5e-6
    assert rel(f, g["f"]) < 2e-5
    assert rel(eps, g["eps"]) < 5e-5
    n_taps = 0
    for k in g.files:
        if k.startswith("out/") or k.startswith("gout/"):
            kind, name = k.split("/")
            got = m.debug_read(kind, name, g[k].shape).cpu().numpy()
            assert rel(got, g[k]) < 5e-5, k
            n_taps += 1
    assert n_taps == 6
    print(f"{tag} {gemm_mode}: f {rel(f, g['f']):.2e} eps {rel(eps, g['eps']):.2e}")


_ORACLE64 = {}
BATCH_CASES = [(0, 32, H) for H in range(8, 65, 8)] + [(opt, c0, H) for opt in (0, 1) for c0 in (16, 64) for H in (8, 48, 64)]


@pytest.mark.parametrize("gemm_mode", ["fp16x3", "fp16x3-tkw"])
@pytest.mark.parametrize("opt,c0,H", BATCH_CASES)
def test_shape_score_batch_vs_oracle64(opt, c0, H, gemm_mode):
    """B = 7 trajectories x 2 variants through a context of 6 rows (chunks of 6, 6 and 2) against the float64 oracle, per row:
    option 0 at C0 = 32 at every accepted horizon, C0 = 16 and 64 at both depths at the horizon ends and the drivers' 48."""
    base, plan = util.split_mode(gemm_mode)
    S = 4
    m = build_shape_unet(S, H, False, opt, c0, max_rows=6, gemm_mode=base, launch_plan=plan)
    cloud = synth.make_cloud(6, 64, 2, seed=3)
    lat = m.encode_scene(dev(cloud))
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    B = 7
    x = synth.make_noise((B, H, S), seed=23)
    xd = dev(x)
    lats = np.tile(lat[0].cpu().numpy()[None], (2 * B, 1)); lats[1::2] = 0
    lib = _lib.load()
    eps = torch.empty((2 * B, H, S), device="cuda"); f = torch.empty_like(eps)
    _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xd), B, 2, 24, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()))
    assert m.score_mode() == "bf16x6"
    t = 11
    _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xd), B, 2, t, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()))
    assert m.score_mode() == "fp16x3"
    key = (opt, c0, H)
    if key not in _ORACLE64:      # (shared by the two launch plans)
        u = O.UNetOracle(shape_weights(S, H, False, opt, c0), S, H, unet_input_dim=c0, dim_mults=UNET_DIM_MULTS[opt], dtype=np.float64)
        x2, tt = np.repeat(x, 2, axis=0), np.full((2 * B,), t)
        _ORACLE64[key] = (u.forward_no_energy(x2, tt, lats), u.score(x2, tt, lats))
    f64, eps64 = _ORACLE64[key]
    fh, eh = f.cpu().numpy(), eps.cpu().numpy()
    row_f = [rel(fh[r], f64[r]) for r in range(2 * B)]
    row_e = [rel(eh[r], eps64[r]) for r in range(2 * B)]
    print(f"dm{opt} C0={c0} H={H} {gemm_mode}: f {rel(fh, f64):.2e} eps {rel(eh, eps64):.2e}, worst row f {max(row_f):.2e} eps {max(row_e):.2e}")
    assert rel(fh, f64) < 2e-5 and rel(eh, eps64) < 5e-5
    assert max(row_f) < 2e-5, row_f
    assert max(row_e) < 5e-5, row_e


def test_narrow_gemm_matches_float64():
    """The K = 16 reductions of a C0 = 16 network (ramp_op_gemm, exact fp32 path): a k = 5 convolution and its input gradient
    with partial segments, and a plain linear; the tile kernels require K % 32 == 0."""
    rng = np.random.default_rng(5)
    for (M, N, K, taps, s0, st, L) in ((96, 16, 16, 5, -2, 1, 48), (96, 64, 16, 5, 2, -1, 24), (72, 256, 16, 1, 0, 0, 1), (40, 32, 48, 5, -2, 1, 8)):
        A = rng.standard_normal((M, K)).astype(np.float32)
        W = rng.standard_normal((taps, N, K)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        resid = rng.standard_normal((M, N)).astype(np.float32)
        out = torch.empty((M, N), device="cuda")
        dA, dW, db, dr = dev(A), dev(W), dev(bias), dev(resid)
        _lib.op_gemm(dA, dW, db, dr, out, M, N, K, taps, s0, st, L, mode="fp32")
        ref = bias[None].astype(np.float64) + resid
        for tap in range(taps):
            sh = s0 + tap * st
            for m in range(M):
                l = m % L + sh
                if 0 <= l < L:
                    ref[m] += W[tap].astype(np.float64) @ A[m - m % L + l].astype(np.float64)
        assert rel(out.cpu().numpy(), ref) < 2e-6, (M, N, K, taps)


@pytest.mark.parametrize("graph", [True, False])
def test_ddpm_chain_of_option_0_against_the_reference(graph):
    """A free-running T = 25 DDPM chain (CFG) at (1,2,4) / 32 through ramp_sample, eagerly and from the captured graph,
    against the reference's run_inference on the same noise; the hard conditions hold exactly."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    g = np.load(f"{GOLDEN}/chain_ddpm_dm0.npz")
    u = build_shape_unet(4, 48, False, 0, 32, max_rows=64)
    dm = StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True,
                                      compose=False, use_apf=False, sampler="ddpm", use_graph=graph).eval().to("cuda")
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(4, 48).items()}
    with NoiseInjector(list(g["noise"])) as inj:
        chain = dm.run_inference(None, hc, n_samples=4, horizon=48, return_chain=True, traj_normalized=None,
                                 obstacle_pts=dev(g["cloud"]), sample_fn=None, guide=None, n_guide_steps=1, t_start_guide=7,
                                 noise_std_extra_schedule_fn=lambda x: 0.5, n_diffusion_steps_without_noise=0).cpu().numpy()
        used = inj.used
    assert used == g["noise"].shape[0] and chain.shape == g["chain"].shape
    err = np.abs(chain - g["chain"]).max()
    print(f"ddpm (1,2,4)/32 graph={graph}: max {err:.2e}")
    assert err < 1e-4
    for i, v in hc.items():
        assert np.array_equal(chain[:, :, i], np.broadcast_to(v.numpy(), chain[:, :, i].shape))


def test_philox_job_at_c0_64_replays_bit_for_bit():
    """noise_source='philox' at (1,2,4,8) / 64: the captured graph's replay gives what the eager job gives, bit for bit."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    H, S, T, B = 48, 4, 25, 6
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}
    cloud = dev(synth.make_cloud(6, 64, 2, seed=42))
    out = {}
    for graph in (True, False):
        u = build_shape_unet(S, H, False, 1, 64, max_rows=16)
        dm = StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True,
                                          use_apf=False, sampler="ddpm", use_graph=graph, noise_source="philox", noise_seed=91).eval().to("cuda")
        out[graph] = [dm.run_inference(None, hc, n_samples=B, horizon=H, obstacle_pts=cloud,
                                       noise_std_extra_schedule_fn=lambda x: 0.5).cpu().numpy() for _ in range(2)]
    for j in range(2):
        assert np.isfinite(out[True][j]).all() and np.abs(out[True][j]).max() < 10.0
        assert np.array_equal(out[True][j], out[False][j]), (j, np.abs(out[True][j] - out[False][j]).max())


def test_3d_job_at_option_0_c0_64_steps_like_the_float64_oracle():
    """A 3-D DDPM job at (1,2,4) / 64, H = 64 through GaussianDiffusionModel3d; every step compared, teacher-forced, with the float64
    oracle's step from the HIP chain's own previous state (CFG at w = 5.75 amplifies rounding too much for a free-running bar)."""
    from ramp_amd.models import GaussianDiffusionModel3d
    H, S, T, B, w = 64, 6, 25, 2, 5.75
    u = build_shape_unet(S, H, True, 0, 64, max_rows=8)
    dm = GaussianDiffusionModel3d(model=u, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True,
                                  compose=False, use_apf=False).eval().to("cuda")
    cloud = synth.make_cloud(5, 50, 3, seed=44)
    noise = synth.make_noise((T + 1, B, H, S), seed=61)
    hc_np = synth.default_hard_conds(S, H)
    hc = {k: torch.from_numpy(v) for k, v in hc_np.items()}
    with NoiseInjector(list(noise)) as inj:
        chain = dm.run_inference(None, hc, n_samples=B, horizon=H, return_chain=True, traj_normalized=None,
                                 obstacle_pts=dev(cloud), sample_fn=None, guide=None, n_guide_steps=1, t_start_guide=7,
                                 noise_std_extra_schedule_fn=lambda x: 0.5, n_diffusion_steps_without_noise=0).cpu().numpy()
        assert inj.used == T + 1
    assert chain.shape == (T + 1, B, H, S) and np.isfinite(chain).all()
    uo = O.UNetOracle(shape_weights(S, H, True, 0, 64), S, H, unet_input_dim=64, dim_mults=UNET_DIM_MULTS[0], obstacle_3d=True,
                      dtype=np.float64)
    sm = O.SamplerOracle(uo, T, w, dtype=np.float64, sched=dict(np.load(f"{GOLDEN}/schedule_T{T}.npz")))
    truth = sm.ddpm(noise, hc_np, uo.encode_scene(cloud), teacher=chain)
    err = np.array([np.abs(chain[j + 1] - truth[j + 1]).max() for j in range(T)])
    print(f"3-D (1,2,4)/64 H=64: worst teacher-forced step {err.max():.2e}")
    assert err.max() < 1e-4


def test_example_static_runs_at_option_0_c0_64(tmp_path):
    """examples/inference_static.py with --unet-dim-mults-option 0 --unet-input-dim 64 on a synthetic experiment of that shape."""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "inference_static.py"), "--make-synthetic", str(tmp_path), "--n-samples", "64",
           "--unet-dim-mults-option", "0", "--unet-input-dim", "64"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "{" in r.stdout.strip().splitlines()[-1]


# ---- tkw.hip at the widths of the unet_input_dim = 64, (1,2,4,8) network -----------------------------------------------------------
# (a) forward with the GroupNorm + Mish epilogue at C_out = 512 (downs.3.*, mid_block1/2: two passes of 256 channels, a 64-channel group
# per wave), (b) the two-source K = 1024 operand of ups.0.0 conv 1, (c) its N = 1024 input gradient split at 512 with the GroupNorm
# backward folded in.  The float64 references and bars are test_gpu_ops.py's; sample counts leave the last 96-token tile partly empty.
TKW_FWD_WIDE = [(3, 256, 512, 33, 0), (6, 512, 512, 21, 0), (12, 256, 512, 9, 0), (6, 256, 512, 13, 0), (6, 1024, 256, 21, 512),
                (3, 1024, 256, 33, 512), (12, 1024, 256, 9, 512)]
TKW_BWD_WIDE = [(6, 256, 1024, 21, 512), (4, 256, 1024, 33, 512), (12, 256, 1024, 9, 512), (6, 512, 512, 13, 0)]   # (L = 3: no GroupNorm-backward staging, tile kernels)


@pytest.mark.parametrize("L,K,N,R,K1", TKW_FWD_WIDE)
@pytest.mark.parametrize("extras", [0, 1, 2])
def test_tkw_wide_forward_vs_float64(L, K, N, R, K1, extras):
    import test_gpu_ops as OPS
    OPS.test_tkw_conv_groupnorm_mish_forward(L, K, N, R, K1, extras)


@pytest.mark.parametrize("L,K,N,R,N1", TKW_BWD_WIDE)
@pytest.mark.parametrize("extras", [0, 3])
def test_tkw_wide_input_gradient_vs_float64(L, K, N, R, N1, extras):
    import test_gpu_ops as OPS
    OPS.test_tkw_groupnorm_backward_conv_input_gradient(L, K, N, R, N1, extras)


def test_tkw_refuses_2048_wide_operands_and_outputs():
    import ctypes as C
    for K, N, epi in ((2048, 256, False), (256, 2048, False), (512, 1024, True)):
        M, L = 96, 6
        X = torch.randn(M, K, device="cuda"); W = torch.randn(5, N, K, device="cuda"); Y = torch.empty(M, N, device="cuda")
        Cs = torch.empty(M, N, device="cuda"); st = torch.empty(M // L, 8, 2, device="cuda")
        b = torch.zeros(N, device="cuda"); gam = torch.ones(N, device="cuda")
        amax, flag = C.c_float(0.0), C.c_int32(0)
        rc = _lib.load().ramp_op_tkw(_lib.ptr(X), None, 0, _lib.ptr(W), _lib.ptr(b), None, None, None, None, None, None,
                                     _lib.ptr(gam) if epi else None, _lib.ptr(b) if epi else None, None, M, L, N, K, 1, N, 1.0, _lib.ptr(Y), None,
                                     _lib.ptr(Cs) if epi else None, _lib.ptr(st) if epi else None, C.byref(amax), C.byref(flag), _lib.current_stream())
        assert rc != 0, (K, N, epi)
        assert "tkw" in _lib.load().ramp_last_error().decode()


_DISPATCH_PROBE = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import util
from test_gpu_shapes import build_shape_unet
from ramp_amd import _lib, synth
m = build_shape_unet(4, 48, False, 1, 64, max_rows=8, gemm_mode="fp16x3", launch_plan=util.PLANS["tkw"])
x = torch.from_numpy(synth.make_noise((2, 48, 4), seed=7)).cuda(); t = torch.tensor([5, 5]).cuda()
pts = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=42)).cuda()[None].repeat(2, 1, 1, 1)
m(x, t, None, obstacle_pts=pts); m(x, t, None, obstacle_pts=pts)
lib = _lib.load()
_lib.check(lib.ramp_profile(m.ctx(), 1))
m(x, t, None, obstacle_pts=pts)
import ctypes as C
ms = (C.c_double * 5)(); fl = (C.c_double * 5)(); cnt = (C.c_int64 * 5)()
_lib.check(lib.ramp_profile_read(m.ctx(), ms, fl, cnt))
assert m.score_mode() == "fp16x3"
"""


def test_wide_convolutions_of_the_c64_network_dispatch_to_tkw(tmp_path):
    """(1,2,4,8) / 64, H = 48, 2 rows, the bench's plan: the per-shape profile lines (RAMP_PROFILE_DUMP) of one fp16x3 evaluation.  Every
    k = 5 convolution of the coarsest level (L = H / 8 = 6 tokens, the smallest M) is a tkw line (taps code -7) and none is a tile-kernel line
    (taps 5).  Expected tkw launches there, from the spec: each of downs.3.0 (256 -> 512), downs.3.1, mid_block1, mid_block2 (512 -> 512)
    and ups.0.0 (cat 512 + 512 -> 256), ups.0.1 (256 -> 256) runs conv 1 and conv 2 forward (N = C_out, K = C_in resp. C_out) and their
    input gradients (N = C_in resp. C_out, K = C_out).  Launches a-c of the issue are (512, 256) / (512, 512) forward, (256, 1024) and (1024, 256)."""
    from collections import Counter
    probe = tmp_path / "probe.py"
    probe.write_text(_DISPATCH_PROBE)
    env = dict(os.environ, RAMP_PROFILE_DUMP="1")
    r = subprocess.run([sys.executable, str(probe), ROOT], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l.split()[2:7] for l in r.stderr.splitlines() if l.startswith("[ramp profile]") and l.split()[2].isdigit()]
    conv = [(int(M), int(N), int(K), int(taps), int(calls)) for M, N, K, taps, calls in lines if int(taps) in (5, -7)]
    Mc = min(c[0] for c in conv)                                       # the coarsest level: 2 rows x 6 tokens
    got = Counter()
    for M, N, K, taps, calls in conv:
        if M == Mc:
            got[(N, K, taps)] += calls
    want = Counter()
    for cin, cout in ((256, 512), (512, 512), (512, 512), (512, 512), (1024, 256), (256, 256)):
        want[(cout, cin, -7)] += 1; want[(cout, cout, -7)] += 1          # forward conv 1, conv 2
        want[(cin, cout, -7)] += 1; want[(cout, cout, -7)] += 1          # input gradients of conv 1, conv 2
    print("coarsest-level k = 5 launches (N, K, taps): calls", dict(got))
    assert got == want, (dict(got), dict(want))
