"""Per-row diffusion timesteps on the GPU: the three time-bias consumers against their uniform launches (bitwise), the network against
the reference's per-row evaluations and the float64 oracle, chunking, explicit scene tables, the denoising loss and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
import util
from util import GOLDEN, build_unet, dev, rel, weights

pytestmark = pytest.mark.gpu

S_ = _lib.current_stream
SCORE_CASES = [("2d_h48", 4, 48, False), ("3d_h64", 6, 64, True), ("2d_h40", 4, 40, False)]
T_LINES = 5


@pytest.fixture(scope="module")
def cases():
    return np.load(f"{GOLDEN}/rowtime_cases.npz")


def _table(C_, seed):
    """A time table of T_LINES lines whose layer sits at column 16 of a wider line, as a block's does inside the engine's table."""
    stride = C_ + 32
    tab = torch.from_numpy(np.random.default_rng(seed).standard_normal((T_LINES, stride)).astype(np.float32)).cuda()
    return tab, stride, 16


def _rows(n, all_equal=None):
    """n timesteps using three distinct lines, first and last line included, one repeated; or n copies of one."""
    if all_equal is not None:
        return np.full(n, all_equal, np.int32)
    return np.array([(T_LINES - 1, 0, 2, 2)[i % 4] for i in range(n)], np.int32)


def _line(tab, off, t):
    return tab.data_ptr() + 4 * (t * tab.shape[1] + off)


# ------------------------------------------------------------------------------------------------ 1. kernel level, bitwise
@pytest.mark.parametrize("C_,L", [(32, 5), (32, 48), (512, 5), (16, 5), (16, 48)])
def test_groupnorm_rows_equal_the_uniform_launch_bitwise(C_, L):
    """gn_fwd_kernel (C = 32, and WIDE at C = 512) and the 16-channel kernel the first block of a unet_input_dim = 16 network reaches:
    every sample of the per-row launch equals the same sample of a uniform launch at its timestep, output and statistics."""
    R = 3
    g = np.random.default_rng(C_ + L)
    x = dev(g.standard_normal((R, L, C_)).astype(np.float32)); res = dev(g.standard_normal((R, L, C_)).astype(np.float32))
    gam = dev(g.standard_normal(C_).astype(np.float32)); bet = dev(g.standard_normal(C_).astype(np.float32))
    tab, stride, off = _table(C_, 1)
    lib = _lib.load()

    def uniform(t):
        y = torch.full((R, L, C_), float("nan"), device="cuda"); st = torch.full((R, 8, 2), float("nan"), device="cuda")
        _lib.check(lib.ramp_op_groupnorm(_lib.ptr(x), _lib.ptr(gam), _lib.ptr(bet), _line(tab, off, t), _lib.ptr(res), _lib.ptr(y), _lib.ptr(st),
                                         R, L, C_, 1e-5, 1, S_()), "ramp_op_groupnorm")
        return y, st

    def rows(tr):
        y = torch.full((R, L, C_), float("nan"), device="cuda"); st = torch.full((R, 8, 2), float("nan"), device="cuda")
        d = dev(tr)
        _lib.check(lib.ramp_op_groupnorm_rows(_lib.ptr(x), _lib.ptr(gam), _lib.ptr(bet), _line(tab, off, 0), stride, _lib.ptr(d), _lib.ptr(res),
                                              _lib.ptr(y), _lib.ptr(st), R, L, C_, 1e-5, 1, S_()), "ramp_op_groupnorm_rows")
        return y, st

    tr = _rows(R)
    y, st = rows(tr)
    for t in sorted(set(tr.tolist())):
        yu, su = uniform(t)
        sel = torch.from_numpy(tr == t).cuda()
        assert torch.equal(y[sel], yu[sel]) and torch.equal(st[sel], su[sel]), t
    assert not torch.equal(y[0], uniform(int(tr[1]))[0][0])          # (the lines do differ)
    ye, se = rows(_rows(R, all_equal=3)); yu, su = uniform(3)
    assert torch.equal(ye, yu) and torch.equal(se, su)


def test_groupnorm_rows_keeps_the_kernel_row_limit():
    """C = 512 at L = 48 is beyond both launches alike (L * C <= 4096: 512 channels exist at the coarsest level only): an error, no launch."""
    R, L, C_ = 3, 48, 512
    x = torch.zeros(R, L, C_, device="cuda"); v = torch.zeros(C_, device="cuda")
    tab, stride, off = _table(C_, 1)
    d = dev(_rows(R))
    lib = _lib.load()
    assert lib.ramp_op_groupnorm(_lib.ptr(x), _lib.ptr(v), _lib.ptr(v), _line(tab, off, 0), None, _lib.ptr(x), None, R, L, C_, 1e-5, 1, S_()) != 0
    assert lib.ramp_op_groupnorm_rows(_lib.ptr(x), _lib.ptr(v), _lib.ptr(v), _line(tab, off, 0), stride, _lib.ptr(d), None, _lib.ptr(x), None,
                                      R, L, C_, 1e-5, 1, S_()) != 0


def _conv_gn_pair(L, N, K, R, seed):
    """The fused convolution + GroupNorm forward, uniform (ramp_op_tkw) and per row (ramp_op_tkw_rows), on the same input, weights and scale."""
    g = np.random.default_rng(seed)
    M = L * R
    X = g.standard_normal((M, K)).astype(np.float32)
    keep = dict(X=dev(X), W=dev((g.standard_normal((5, N, K)) / np.sqrt(5 * K)).astype(np.float32)), b=dev(g.standard_normal(N).astype(np.float32)),
                res=dev(g.standard_normal((M, N)).astype(np.float32)), gam=dev(g.standard_normal(N).astype(np.float32)),
                bet=dev(g.standard_normal(N).astype(np.float32)))
    tab, stride, off = _table(N, seed + 1)
    prev = float(np.abs(X).max()) * 0.8
    lib = _lib.load()

    def outs():
        return (torch.full((M, N), float("nan"), device="cuda"), torch.full((M, N), float("nan"), device="cuda"),
                torch.full((R, 8, 2), float("nan"), device="cuda"))

    def uniform(t):
        Y, Cs, st = outs()
        amax, flag = C.c_float(0.0), C.c_int32(0)
        _lib.check(lib.ramp_op_tkw(_lib.ptr(keep["X"]), None, 0, _lib.ptr(keep["W"]), _lib.ptr(keep["b"]), _lib.ptr(keep["res"]), None, None, None, None, None,
                                   _lib.ptr(keep["gam"]), _lib.ptr(keep["bet"]), _line(tab, off, t), M, L, N, K, 1, N, prev, _lib.ptr(Y), None, _lib.ptr(Cs),
                                   _lib.ptr(st), C.byref(amax), C.byref(flag), S_()), "ramp_op_tkw")
        assert flag.value == 0
        return Y.reshape(R, L, N), Cs.reshape(R, L, N), st

    def rows(tr):
        Y, Cs, st = outs()
        d = dev(tr)
        amax, flag = C.c_float(0.0), C.c_int32(0)
        _lib.check(lib.ramp_op_tkw_rows(_lib.ptr(keep["X"]), _lib.ptr(keep["W"]), _lib.ptr(keep["b"]), _lib.ptr(keep["res"]), _lib.ptr(keep["gam"]),
                                        _lib.ptr(keep["bet"]), _line(tab, off, 0), stride, _lib.ptr(d), M, L, N, K, prev, _lib.ptr(Y), _lib.ptr(Cs),
                                        _lib.ptr(st), C.byref(amax), C.byref(flag), S_()), "ramp_op_tkw_rows")
        assert flag.value == 0
        return Y.reshape(R, L, N), Cs.reshape(R, L, N), st

    return uniform, rows


def _check_rows_against_uniform(uniform, rows, R):
    tr = _rows(R)
    got = rows(tr)
    assert not any(torch.isnan(a).any() for a in got)
    for t in sorted(set(tr.tolist())):
        ref = uniform(t)
        sel = torch.from_numpy(tr == t).cuda()
        for a, b in zip(got, ref):
            assert torch.equal(a[sel], b[sel]), t
    assert not torch.equal(got[0][0], uniform(int(tr[1]))[0][0])
    for a, b in zip(rows(_rows(R, all_equal=1)), uniform(1)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("L", [8, 16, 32, 64])
def test_tkc_epilogue_rows_equal_the_uniform_launch_bitwise(L, N):
    """tkc.hip, sample-owning waves: L = 8 and 16 (48-token wave tiles, NG 3), 32 (NG 2) and 64 (NG 4, one sample per wave); 5 samples leave
    the last wave partly (or wholly) empty."""
    uniform, rows = _conv_gn_pair(L, N, 32, 5, 100 + L + N)
    _check_rows_against_uniform(uniform, rows, 5)


@pytest.mark.parametrize("N", [128, 256, 512])
@pytest.mark.parametrize("L,R", [(3, 33), (6, 5), (24, 3)])
def test_tkw_epilogue_rows_equal_the_uniform_launch_bitwise(L, R, N):
    """tkw.hip, sample-owning blocks of 96 tokens: L = 3 with 33 samples is two tiles, the second holding one sample; N = 128 (one 32-channel
    block per wave), 256, and 512 (EPI 2: two passes of 256)."""
    uniform, rows = _conv_gn_pair(L, N, 64, R, 200 + L + N)
    _check_rows_against_uniform(uniform, rows, R)


# ------------------------------------------------------------------------------------------------ 2. the network against the reference
@pytest.mark.parametrize("gemm_mode", ["fp16x3-tkw", "bf16x6", "fp32"])
@pytest.mark.parametrize("tag,S,H,o3", SCORE_CASES)
def test_network_with_per_row_timesteps_against_reference_fixture(cases, tag, S, H, o3, gemm_mode):
    """forward_no_energy and forward with the fixture's per-row t.  fp16x3: the compared evaluation is the one after calibration."""
    gemm_mode, plan = util.split_mode(gemm_mode)
    m = build_unet(S, H, o3, max_rows=8, gemm_mode=gemm_mode, launch_plan=plan)
    x = dev(cases[f"{tag}/x"]); t = torch.from_numpy(cases[f"{tag}/t"]).cuda()
    N = x.shape[0]
    pts = dev(cases[f"{tag}/cloud"])[None].repeat(N, 1, 1, 1)
    f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    if gemm_mode == "fp16x3":
        assert m.score_mode() == "bf16x6"
        f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    assert m.score_mode() == gemm_mode
    eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    if gemm_mode == "fp16x3":
        assert m.score_mode() == "bf16x6"
        eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    assert m.score_mode() == gemm_mode
    ef, ee = rel(f, cases[f"{tag}/f"]), rel(eps, cases[f"{tag}/eps"])
    print(f"{tag} {gemm_mode}: f {ef:.2e} eps {ee:.2e}")
    assert ef < 2e-5 and ee < 5e-5


# ------------------------------------------------------------------------------------------------ 3. chunking and row independence
def _score_rows(m, xd, B, n_rp, tr, want_f=True):
    H, S = xd.shape[1:]
    eps = torch.full((n_rp * B, H, S), float("nan"), device="cuda"); f = torch.full_like(eps, float("nan")) if want_f else None
    tr = np.ascontiguousarray(tr, np.int32)
    _lib.check(_lib.load().ramp_score_rows(m.ctx(), _lib.ptr(xd), B, n_rp, tr.ctypes.data_as(_lib.c_i32p), _lib.ptr(f), _lib.ptr(eps), S_()),
               "ramp_score_rows")
    return f, eps


def _score(m, xd, B, n_rp, t):
    H, S = xd.shape[1:]
    eps = torch.empty((n_rp * B, H, S), device="cuda"); f = torch.empty_like(eps)
    _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(xd), B, n_rp, int(t), _lib.ptr(f), _lib.ptr(eps), S_()), "ramp_score")
    return f, eps


def test_chunked_rows_vs_oracle64_and_vs_the_uniform_call():
    """B = 11 x n_rp = 2 through max_rows = 6 (four chunks, the table sliced per chunk), a random timestep per row: against the float64
    oracle; every row bitwise what ramp_score gives it at its t; an all-equal table bitwise ramp_score."""
    S, H, B = 4, 48, 11
    m = build_unet(S, H, False, max_rows=6, gemm_mode="bf16x6")
    u = O.UNetOracle(weights(S, H, False), S, H, obstacle_3d=False, dtype=np.float64)
    cloud = synth.make_cloud(6, 64, 2, seed=3)
    lat = m.encode_scene(dev(cloud))
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    x = synth.make_noise((B, H, S), seed=21); xd = dev(x)
    tr = np.random.default_rng(5).integers(0, 25, 2 * B).astype(np.int32)
    tr[3], tr[16] = 0, 24
    f, eps = _score_rows(m, xd, B, 2, tr)
    lats = np.tile(lat[0].cpu().numpy()[None], (2 * B, 1)); lats[1::2] = 0
    x2 = np.repeat(x, 2, axis=0)
    ef, ee = rel(f.cpu().numpy(), u.forward_no_energy(x2, tr, lats)), rel(eps.cpu().numpy(), u.score(x2, tr, lats))
    print(f"chunked per-row vs float64: f {ef:.2e} eps {ee:.2e}")
    assert ef < 2e-5 and ee < 5e-5
    for t in sorted(set(tr.tolist())):
        fu, eu = _score(m, xd, B, 2, t)
        sel = torch.from_numpy(tr == t).cuda()
        assert torch.equal(f[sel], fu[sel]) and torch.equal(eps[sel], eu[sel]), t
    fe, ee_ = _score_rows(m, xd, B, 2, np.full(2 * B, 11))
    fu, eu = _score(m, xd, B, 2, 11)
    assert torch.equal(fe, fu) and torch.equal(ee_, eu)


# ------------------------------------------------------------------------------------------------ 4. with an explicit scene table
def test_per_row_time_composes_with_per_row_latents():
    S, H, B = 4, 48, 3
    m = build_unet(S, H, False, max_rows=8, gemm_mode="bf16x6")
    u = O.UNetOracle(weights(S, H, False), S, H, obstacle_3d=False, dtype=np.float64)
    lat = torch.cat([m.encode_scene(dev(synth.make_cloud(6, 64, 2, seed=s))) for s in (3, 4, 5)])
    lat4 = torch.cat([lat, torch.zeros_like(lat[:1])])
    rv = np.array([0, 3, 1, 3, 2, 3], np.int32)          # trajectory b: [scene b, unconditional]
    m.set_scenes(lat4, rv)
    m.prepare_time_table(25)
    x = synth.make_noise((B, H, S), seed=33)
    tr = np.array([24, 7, 0, 7, 13, 2], np.int32)
    f, eps = _score_rows(m, dev(x), B, 2, tr)
    lats = lat4.cpu().numpy()[rv]
    x2 = np.repeat(x, 2, axis=0)
    ef, ee = rel(f.cpu().numpy(), u.forward_no_energy(x2, tr, lats)), rel(eps.cpu().numpy(), u.score(x2, tr, lats))
    print(f"scenes x per-row time vs float64: f {ef:.2e} eps {ee:.2e}")
    assert ef < 2e-5 and ee < 5e-5
    # neither table stands in for the other: with the latents shifted by one scene, or the times by one row, the result moves visibly
    assert rel(f.cpu().numpy(), u.forward_no_energy(x2, np.roll(tr, 1), lats)) > 1e-3
    assert rel(f.cpu().numpy(), u.forward_no_energy(x2, tr, lat4.cpu().numpy()[np.array([1, 3, 2, 3, 0, 3])])) > 1e-3


# ------------------------------------------------------------------------------------------------ 5. the denoising loss
def _loss_model(u, loss_type):
    from ramp_amd.models import StaticGaussianDiffusionModel
    return StaticGaussianDiffusionModel(model=u, n_diffusion_steps=25, predict_epsilon=True, loss_type=loss_type).eval().to("cuda")


def test_denoising_loss_against_the_reference(cases):
    g = {k.split("/")[1]: cases[k] for k in cases.files if k.startswith("loss/")}
    u = build_unet(4, 48, False, max_rows=8)
    B = g["x_start"].shape[0]
    pts = dev(g["cloud"])[None].repeat(B, 1, 1, 1)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(4, 48).items()}
    t = torch.from_numpy(g["t"]).cuda()
    target = g["noise"] if int(g["predict_epsilon"]) else g["x_start"]
    for lt in ("l2", "l1"):
        dm = _loss_model(u, lt)
        loss, info = dm.p_losses(dev(g["x_start"]), None, t, hc, pts, noise=dev(g["noise"]))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        en, er = rel(info["x_noisy"].cpu().numpy(), g["x_noisy"]), rel(info["x_recon"].cpu().numpy(), g["x_recon"])
        xr = info["x_recon"].cpu().numpy()
        d = (xr - target).astype(np.float32)
        host = float(np.mean(((d * d) if lt == "l2" else np.abs(d)).astype(np.float64)))
        e_red = abs(float(info["loss64"]) - host) / host
        e_ref = abs(float(loss) - float(g[f"loss_{lt}"])) / float(g[f"loss_{lt}"])
        print(f"{lt}: x_noisy {en:.2e} x_recon {er:.2e} reduction vs float64 host sum {e_red:.2e} loss vs reference {e_ref:.2e}")
        assert en < 1e-6 and er < 5e-5
        assert np.array_equal(xr[:, 0], g["x_start"][:, 0]) and np.array_equal(xr[:, -1], g["x_start"][:, -1])
        assert e_red < 1e-6
        assert e_ref < 1e-4
    # the plain q_sample leaves the endpoints noised (diffusion_model_static.py:467-476)
    q = dm.q_sample(dev(g["x_start"]), t, dev(g["noise"])).cpu().numpy()
    assert rel(q[:, 1:-1], g["x_noisy"][:, 1:-1]) < 1e-6 and not np.array_equal(q[1:, 0], g["x_start"][1:, 0])
    # loss(): its own randint draw
    own, _ = dm.loss(dev(g["x_start"]), None, hc, pts)
    assert own.dim() == 0 and bool(torch.isfinite(own))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_timestep_beyond_the_table_is_refused_before_any_launch():
    S, H, B = 4, 48, 3
    m = build_unet(S, H, False, max_rows=8, gemm_mode="bf16x6")
    lat = m.encode_scene(dev(synth.make_cloud(6, 64, 2, seed=3)))
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    xd = dev(synth.make_noise((B, H, S), seed=1))
    _score_rows(m, xd, B, 2, np.array([0, 24, 1, 2, 3, 4]))
    n0 = m.launch_count()
    assert n0 > 0
    for bad in (25, -1, 1 << 30):
        tr = np.array([0, 24, 1, bad, 3, 4], np.int32)
        eps = torch.full((2 * B, H, S), float("nan"), device="cuda")
        rc = _lib.load().ramp_score_rows(m.ctx(), _lib.ptr(xd), B, 2, tr.ctypes.data_as(_lib.c_i32p), None, _lib.ptr(eps), S_())
        assert rc != 0 and "outside the prepared time table" in _lib.load().ramp_last_error().decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(eps).all()) and m.launch_count() == n0


def test_loss_in_training_mode_raises():
    u = build_unet(4, 48, False, max_rows=8)
    dm = _loss_model(u, "l2").train()
    x = torch.zeros(2, 48, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="training"):
        dm.loss(x, None, {}, torch.zeros(2, 6, 64, 2, device="cuda"))
    with pytest.raises(NotImplementedError, match="l2smooth"):
        _loss_model(u, "l2smooth").loss(x, None, {}, torch.zeros(2, 6, 64, 2, device="cuda"))
