"""Composition over any number of obstacle sets per trajectory, many scenes per job (``run_inference_composed`` -> ``ramp_set_scenes`` +
``ramp_sample_composed``): single evaluations beyond three rows per trajectory, the guidance step on a weight table, the reference
fixtures of tests/golden/compose_sets.npz (ramp_amd/tools/make_compose_goldens.py), two sets through the new path against the existing
compose fixture, ragged many-scene jobs, chunking, launch plans, weights as data of a captured graph, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.scenes import build_compose_tables
from util import GOLDEN, NoiseInjector, build_unet, dev, rel, weights

pytestmark = pytest.mark.gpu


class KSetOracle(O.SamplerOracle):
    """SamplerOracle over K obstacle sets: ``latent`` is (K, ctx) and e = u + sum_k w_k (c_k - u), the reference's formula and association
    order (diffusion_model_static.py:214, diffusion_model_3d.py:173-174), rows [c_0 .. c_{K-1}, u] per trajectory."""

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


def _hcn(S, H=48):
    return synth.default_hard_conds(S, H)


def _hc(S, H=48):
    return {k: torch.from_numpy(v) for k, v in _hcn(S, H).items()}


def _static(T=25, use_apf=False, sampler="ddpm", use_graph=True, max_rows=24, compose=False, launch_plan=None, gemm_mode="default"):
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=max_rows, gemm_mode=gemm_mode, launch_plan=launch_plan)
    return StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=T, predict_epsilon=True, compose=compose,
                                        use_apf=use_apf, sampler=sampler, use_graph=use_graph).eval().to("cuda")


def _range_flag(u):
    flag = C.c_int32(-1)
    _lib.check(_lib.load().ramp_range_status(u.ctx(), C.byref(flag), _lib.current_stream()))
    return flag.value


def _composed(dm, scenes, counts, noise, weights=None, apf_clouds=None):
    """One composed job on injected noise: the chain (steps + 1, B, H, S) as numpy."""
    S = dm.state_dim
    with NoiseInjector(list(noise)) as inj:
        chain, ts = dm.run_inference_composed(scenes, [_hc(S) for _ in scenes], n_samples=counts, weights=weights, apf_clouds=apf_clouds,
                                              return_chain=True, horizon=48, noise_std_extra_schedule_fn=lambda x: 0.5)
        assert inj.used == len(noise)
    return chain.cpu().numpy(), ts.cpu().numpy()


def _one_step(dm, job, guidance, hc, B, x, noise, t, ddim=False, apf=0, K=None):
    """One step of the job's loop from state x (teacher forcing): the next state as numpy."""
    if ddim:
        out, _ = dm._launch(B, dev(x)[None], hc, None, True, [t], [apf], None, dict(dm.apf_ddim) if apf else None, False, ddim_K=K,
                            scene_job=job, guidance=guidance)
    else:
        out, _ = dm._launch(B, torch.stack([dev(x), dev(noise)]), hc, None, False, [t], [0], [0.5], None, False, scene_job=job,
                            guidance=guidance)
    return out.cpu().numpy()


def _eval_composed(dm, x, B, n_rp, t, row_weight):
    """ramp_score over the table in place + ramp_cfg_mean_rows: (eps rows, e_comb, x0, mean) as numpy."""
    lib = _lib.load()
    xd = dev(x)
    eps = torch.empty((B * n_rp,) + tuple(x.shape[1:]), device="cuda")
    x0 = torch.empty_like(xd); mean = torch.empty_like(xd); ec = torch.empty_like(xd)
    dm.model.prepare_time_table(dm.n_diffusion_steps)
    _lib.check(lib.ramp_score(dm.model.ctx(), _lib.ptr(xd), B, n_rp, t, None, _lib.ptr(eps), _lib.current_stream()), "ramp_score")
    _lib.check(lib.ramp_cfg_mean_rows(_lib.ptr(xd), _lib.ptr(eps), B, xd[0].numel(), n_rp, _lib.ptr(row_weight),
                                      float(dm.sqrt_recip_alphas_cumprod[t]), float(dm.sqrt_recipm1_alphas_cumprod[t]),
                                      float(dm.posterior_mean_coef1[t]), float(dm.posterior_mean_coef2[t]), 1, 0,
                                      _lib.ptr(x0), _lib.ptr(mean), _lib.ptr(ec), _lib.current_stream()), "ramp_cfg_mean_rows")
    torch.cuda.synchronize()
    return eps.cpu().numpy(), ec.cpu().numpy(), x0.cpu().numpy(), mean.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("n_rp", [4, 8])
def test_single_evaluation_beyond_three_rows(n_rp):
    """ramp_score with 4 and 8 rows per trajectory, B = 3, 2-D H = 48, per-row latents through set_scenes (every trajectory reads the sets
    in another order), against UNetOracle in float64 under the bars of tests/test_gpu_unet.py: f < 2e-5, eps < 5e-5.  Before
    RAMP_MAX_ROWS_PER_TRAJ the call answered "bad batch" from 4 rows on."""
    S, H, B, K = 4, 48, 3, n_rp - 1
    m = build_unet(S, H, False, max_rows=24)
    m.prepare_time_table(25)
    clouds = [synth.make_cloud(4 + (k % 3), 64, 2, seed=300 + k) for k in range(K)]
    lat = torch.cat([m.encode_scenes([dev(c) for c in clouds]), torch.zeros(1, m.context_dim, device="cuda")])
    rv = np.stack([np.concatenate([np.roll(np.arange(K), b), [K]]) for b in range(B)]).astype(np.int32)
    m.set_scenes(lat, rv.reshape(-1))
    x = synth.make_noise((B, H, S), seed=23)
    xd = dev(x)
    eps = torch.empty((B * n_rp, H, S), device="cuda"); f = torch.empty_like(eps)
    _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(xd), B, n_rp, 7, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()), "ramp_score")
    uo = O.UNetOracle(weights(S, H, False), S, H, dtype=np.float64)
    lat64 = np.concatenate([np.stack([uo.encode_scene(c) for c in clouds]), np.zeros((1, m.context_dim))])
    xr, tt, lr = np.repeat(x, n_rp, axis=0), np.full((B * n_rp,), 7), lat64[rv.reshape(-1)]
    ef, ee = rel(f.cpu().numpy(), uo.forward_no_energy(xr, tt, lr)), rel(eps.cpu().numpy(), uo.score(xr, tt, lr))
    print(f"ramp_score n_rp = {n_rp}: f {ef:.2e} eps {ee:.2e}")
    assert ef < 2e-5 and ee < 5e-5
    # and one timestep per row takes the same bound
    t_rows = (C.c_int32 * (B * n_rp))(*([7] * (B * n_rp)))
    eps2 = torch.empty_like(eps)
    _lib.check(_lib.load().ramp_score_rows(m.ctx(), _lib.ptr(xd), B, n_rp, t_rows, None, _lib.ptr(eps2), _lib.current_stream()), "ramp_score_rows")
    assert rel(eps2.cpu().numpy(), uo.score(xr, tt, lr)) < 5e-5
    bad = torch.empty((B * 9, H, S), device="cuda")
    assert _lib.load().ramp_score(m.ctx(), _lib.ptr(xd), B, 9, 7, None, _lib.ptr(bad), _lib.current_stream()) != 0


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("n_rp", [2, 4, 8])
def test_cfg_mean_rows_against_float64(n_rp):
    """ramp_cfg_mean_rows, B = 5, HS = 48 * 4: e_comb against the same sum in numpy float64 (< 1e-6 relative), x0 and the posterior mean
    behind it; with the CFG pair's weights (n_rp = 2) within 2e-6 of ramp_cfg_mean."""
    B, H, S = 5, 48, 4
    HS = H * S
    rng = np.random.default_rng(40 + n_rp)
    x = rng.standard_normal((B, H, S)).astype(np.float32)
    eps = rng.standard_normal((B * n_rp, H, S)).astype(np.float32)
    w = rng.uniform(-3, 3, (B, n_rp)).astype(np.float32)
    sr, srm, c1, c2 = np.float32(1.7), np.float32(1.3), np.float32(0.4), np.float32(0.6)
    lib = _lib.load()
    xd, ed = dev(x), dev(eps)

    def rows(wt, predict_x0=0, clip=1):
        x0 = torch.empty(B, H, S, device="cuda"); mean = torch.empty_like(x0); ec = torch.empty_like(x0)
        wd = dev(wt)
        _lib.check(lib.ramp_cfg_mean_rows(_lib.ptr(xd), _lib.ptr(ed), B, HS, n_rp, _lib.ptr(wd), sr, srm, c1, c2, clip, predict_x0,
                                          _lib.ptr(x0), _lib.ptr(mean), _lib.ptr(ec), _lib.current_stream()), "ramp_cfg_mean_rows")
        return ec.cpu().numpy(), x0.cpu().numpy(), mean.cpu().numpy()

    ec, x0, mean = rows(w, clip=0)
    e64 = (w.astype(np.float64)[:, :, None, None] * eps.astype(np.float64).reshape(B, n_rp, H, S)).sum(1)
    x64 = np.float64(sr) * x - np.float64(srm) * e64
    m64 = np.float64(c1) * x64 + np.float64(c2) * x
    print(f"cfg_mean_rows n_rp = {n_rp}: e_comb {rel(ec, e64):.2e} x0 {rel(x0, x64):.2e} mean {rel(mean, m64):.2e}")
    assert rel(ec, e64) < 1e-6
    # x0 and the mean each add three rounded operations to e_comb's error (unclamped, so that the maximum they are measured against is theirs)
    assert rel(x0, x64) < 2e-6 and rel(mean, m64) < 2e-6
    ecc, x0c, meanc = rows(w)                              # the clamp: on x0 itself, then the mean from the clamped value
    assert np.array_equal(ecc, ec) and np.array_equal(x0c, np.clip(x0, -1, 1))
    assert rel(meanc, np.float64(c1) * x0c + np.float64(c2) * x) < 1e-6
    ecp, x0p, _ = rows(w, predict_x0=1)
    assert np.array_equal(ecp, ec) and np.array_equal(x0p, np.clip(ec, -1, 1))
    # the existing job's weights through the table: CFG at w = 2 (n_rp = 2), two sets at (2, 2) (n_rp = 3 would be the compose job)
    k = n_rp - 1
    wt = build_compose_tables((k,), B, [[0]], 3.0 if k == 1 else 2.0)["row_weight"]
    ec_t, x0_t, mean_t = rows(wt)
    if n_rp == 2:
        x0r = torch.empty(B, H, S, device="cuda"); meanr = torch.empty_like(x0r); ecr = torch.empty_like(x0r)
        _lib.check(lib.ramp_cfg_mean(_lib.ptr(xd), _lib.ptr(ed), B, HS, 2, 2.0, 0.0, sr, srm, c1, c2, 1, 0, _lib.ptr(x0r), _lib.ptr(meanr),
                                     _lib.ptr(ecr), _lib.current_stream()), "ramp_cfg_mean")
        d = max(rel(ec_t, ecr.cpu().numpy()), rel(x0_t, x0r.cpu().numpy()), rel(mean_t, meanr.cpu().numpy()))
        print(f"cfg_mean_rows with the CFG weights vs ramp_cfg_mean: {d:.2e}")
        assert d < 2e-6


def test_cfg_mean_rows_with_two_set_weights_equals_cfg_mean():
    """The compose job's (2, 2) and (5, 5) through the table (n_rp = 3) within 2e-6 of ramp_cfg_mean's u + w1 (c1 - u) + w2 (c2 - u)."""
    B, H, S = 5, 48, 4
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, H, S)).astype(np.float32)
    eps = rng.standard_normal((B * 3, H, S)).astype(np.float32)
    lib = _lib.load()
    xd, ed = dev(x), dev(eps)
    for w in (2.0, 5.0):
        wd = dev(build_compose_tables((2,), B, [[0]], w)["row_weight"])
        out = [[torch.empty(B, H, S, device="cuda") for _ in range(3)] for _ in range(2)]
        _lib.check(lib.ramp_cfg_mean_rows(_lib.ptr(xd), _lib.ptr(ed), B, H * S, 3, _lib.ptr(wd), 1.7, 1.3, 0.4, 0.6, 1, 0,
                                          *[_lib.ptr(o) for o in out[0]], _lib.current_stream()), "ramp_cfg_mean_rows")
        _lib.check(lib.ramp_cfg_mean(_lib.ptr(xd), _lib.ptr(ed), B, H * S, 3, w, w, 1.7, 1.3, 0.4, 0.6, 1, 0,
                                     *[_lib.ptr(o) for o in out[1]], _lib.current_stream()), "ramp_cfg_mean")
        d = max(rel(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(*out))
        print(f"cfg_mean_rows vs cfg_mean, two sets at ({w}, {w}): {d:.2e}")
        assert d < 2e-6


# ------------------------------------------------------------------------------------------------ 3
def test_three_sets_2d_against_reference_fixture():
    """compose_sets.npz, 2-D, K = 3, weights (1.5, 1.0, 1.5), under the bars test_compose_static_against_reference_fixture uses: one
    evaluation (e_comb < 5e-5 relative, x0 and mean < 1e-4), the free-running DDPM chain (< 2e-4: the same sum of |row weight| as the
    (2, 2) case), every DDPM step teacher-forced (< 1e-4, or as close to the float64 K-set oracle as 3 x the reference's own distance), and
    the free-running DDIM-5 chain of T = 100 (< 2e-4, the DDPM chain's bar: the same amplification over fewer steps)."""
    g = np.load(f"{GOLDEN}/compose_sets.npz")
    clouds, w = dev(g["2d/clouds"]), [float(v) for v in g["2d/weights"]]
    dm = _static(25, use_apf=True, max_rows=12)
    job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3, w)
    assert B == 3 and guid["n_rp"] == 4
    assert rel(dm.model.cached_scene_latents[:3].cpu().numpy(), g["2d/latents"]) < 5e-6
    _, ec, x0, mean = _eval_composed(dm, g["2d/pmv_x"], 3, 4, int(g["2d/pmv_t"]), guid["row_weight"])
    print(f"K = 3 single evaluation: e_comb {rel(ec, g['2d/pmv_ecomb']):.2e} x0 {np.abs(x0 - g['2d/pmv_x0']).max():.2e} mean {np.abs(mean - g['2d/pmv_mean']).max():.2e}")
    assert rel(ec, g["2d/pmv_ecomb"]) < 5e-5
    assert np.abs(x0 - g["2d/pmv_x0"]).max() < 1e-4 and np.abs(mean - g["2d/pmv_mean"]).max() < 1e-4
    chain, ts = _composed(dm, [clouds], 3, g["2d/ddpm_noise"], w)
    ref = g["2d/ddpm_chain"]
    err = np.abs(chain - ref).reshape(26, -1).max(1)
    print(f"K = 3 ddpm free-running: final {err[-1]:.2e} max {err.max():.2e}")
    assert ts.tolist() == [0, 0, 0] and _range_flag(dm.model) == 0 and err.max() < 2e-4
    # every step from the reference's own previous state
    job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3, w)
    truth = None
    worst = 0.0
    for j in range(25):
        got = _one_step(dm, job, guid, hc, 3, ref[j], g["2d/ddpm_noise"][j + 1], 24 - j)
        e_ref = float(np.abs(got - ref[j + 1]).max())
        worst = max(worst, e_ref)
        if e_ref >= 1e-4:
            if truth is None:
                uo = O.UNetOracle(weights(4, 48, False), 4, 48, dtype=np.float64)
                so = KSetOracle(uo, 25, dtype=np.float64, sched=dict(np.load(f"{GOLDEN}/schedule_T25.npz")), set_weights=w)
                truth = so.ddpm(g["2d/ddpm_noise"], _hcn(4), np.stack([uo.encode_scene(c) for c in g["2d/clouds"]]), teacher=ref)
            e_truth, ref_truth = float(np.abs(got - truth[j + 1]).max()), float(np.abs(ref[j + 1] - truth[j + 1]).max())
            assert e_truth < 3 * ref_truth, (j, e_ref, e_truth, ref_truth)
    print(f"K = 3 ddpm teacher-forced worst vs reference {worst:.2e}")
    # DDIM-5 of T = 100, no APF
    dd = _static(100, use_apf=False, sampler="ddim", max_rows=12)
    assert dd.ddim and dd.ddim_num_inference_steps == 5
    chain, _ = _composed(dd, [clouds], 3, g["ddim/noise"], w)
    err = np.abs(chain - g["ddim/chain"]).max()
    print(f"K = 3 ddim-5 free-running max {err:.2e}")
    assert chain.shape == (6, 3, 48, 4) and err < 2e-4


def test_three_sets_3d_against_reference_fixture():
    """compose_sets.npz, 3-D, K = 3, weights (2.5, 2.5, 5.0) (sum of |row weight| 19, as the (5, 5) case): one batched B = 2 job against
    two independent n_samples = 1 reference runs, every step teacher-forced < 1e-4, or as close to the float64 K-set oracle as 3 x the
    reference's own distance from it."""
    from ramp_amd.models import GaussianDiffusionModel3d
    g = np.load(f"{GOLDEN}/compose_sets.npz")
    u = build_unet(6, 48, True, max_rows=12)
    dm = GaussianDiffusionModel3d(model=u, n_diffusion_steps=25, predict_epsilon=True, use_graph=False).eval().to("cuda")
    w = [float(v) for v in g["3d/weights"]]
    job, guid, hc, B = dm._prepare_composed_job([dev(g["3d/clouds"])], [_hc(6)], 2, w)
    assert rel(u.cached_scene_latents[:3].cpu().numpy(), g["3d/latents"]) < 5e-6
    ref, nz = g["3d/chain"], g["3d/noise"]
    truth = None
    worst = 0.0
    for j in range(25):
        got = _one_step(dm, job, guid, hc, 2, ref[j], nz[j + 1], 24 - j)
        e_ref = float(np.abs(got - ref[j + 1]).max())
        worst = max(worst, e_ref)
        if e_ref >= 1e-4:
            if truth is None:
                uo = O.UNetOracle(weights(6, 48, True), 6, 48, obstacle_3d=True, dtype=np.float64)
                so = KSetOracle(uo, 25, dtype=np.float64, sched=dict(np.load(f"{GOLDEN}/schedule_T25.npz")), set_weights=w)
                truth = so.ddpm(nz, _hcn(6), np.stack([uo.encode_scene(c) for c in g["3d/clouds"]]), teacher=ref)
            e_truth, ref_truth = float(np.abs(got - truth[j + 1]).max()), float(np.abs(ref[j + 1] - truth[j + 1]).max())
            assert e_truth < 3 * ref_truth, (j, e_ref, e_truth, ref_truth)
    print(f"3-D K = 3 teacher-forced worst vs reference {worst:.2e}")
    # the default weight of the 3-D sampler is 5
    assert dm._prepare_composed_job([dev(g["3d/clouds"])], [_hc(6)], 1)[1]["row_weight"].cpu().numpy().tolist() == [[5.0, 5.0, 5.0, -14.0]]


# ------------------------------------------------------------------------------------------------ 4
def test_two_sets_through_the_composed_job_meet_the_compose_fixture():
    """One scene, K = 2, default weights, apf_clouds the reference's six-plus-four rule: every assertion of
    test_compose_static_against_reference_fixture on compose_static.npz with that test's numbers -- the single step, the DDPM chain, the
    DDIM-8 + APF chain (free-running until the hook first fires, then teacher-forced with the float64 fallback)."""
    g = np.load(f"{GOLDEN}/compose_static.npz")
    clouds = dev(g["clouds"])
    hcn = _hcn(4)
    # (1) one evaluation
    dm = _static(25, use_apf=True, compose=True, max_rows=12)
    job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3)
    assert guid["row_weight"].cpu().numpy().tolist() == [[2.0, 2.0, -3.0]] * 3
    _, ec, x0, mean = _eval_composed(dm, g["pmv_x"], 3, 3, int(g["pmv_t"]), guid["row_weight"])
    assert rel(ec, g["pmv_ecomb"]) < 5e-5
    assert np.abs(x0 - g["pmv_x0"]).max() < 1e-4 and np.abs(mean - g["pmv_mean"]).max() < 1e-4
    # (2) DDPM T = 25, use_apf = True: no hook on the compose path
    union = dm._compose_apf_cloud(clouds)
    chain, _ = _composed(dm, [clouds], 3, g["ddpm_noise"], apf_clouds=[union])
    err = np.abs(chain - g["ddpm_chain"]).reshape(26, -1).max(1)
    print(f"two sets, composed job, ddpm free-running: final {err[-1]:.2e} max {err.max():.2e}")
    assert err.max() < 2e-4
    # (3) DDIM-8 + APF
    dm = _static(100, use_apf=True, sampler=None, compose=True, max_rows=12)
    assert dm.ddim and dm.ddim_num_inference_steps == 8
    chain, _ = _composed(dm, [clouds], 3, g["ddim_noise"], apf_clouds=[union])
    assert chain.shape == (9, 3, 48, 4)
    assert np.abs(chain[:3] - g["ddim_chain"][:3]).max() < 1e-4
    ref = g["ddim_chain"]
    steps = [int(i) for i in dm.ddim_set_timesteps(8)]
    uo = O.UNetOracle(weights(4, 48, False), 4, 48, dtype=np.float64)
    lats = np.stack([uo.encode_scene(g["clouds"][0]), uo.encode_scene(g["clouds"][1])])
    so = O.SamplerOracle(uo, 100, 2.0, dtype=np.float64, sched=dict(np.load(f"{GOLDEN}/schedule_T100.npz")), compose_w=(2.0, 2.0))
    truth = so.ddim(g["ddim_noise"][0], hcn, lats, cloud=np.concatenate([g["clouds"][0], g["clouds"][1][:4]]).reshape(-1, 2), use_apf=True,
                    K=8, teacher=ref)
    job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3, apf_clouds=[union])
    worst = 0.0
    for j, tt in enumerate(steps):
        got = _one_step(dm, job, guid, hc, 3, ref[j], None, tt, ddim=True, apf=1 if j >= dm.apf_ddim["start"] else 0)
        e_ref = float(np.abs(got - ref[j + 1]).max())
        e_truth, ref_truth = float(np.abs(got - truth[j + 1]).max()), float(np.abs(ref[j + 1] - truth[j + 1]).max())
        worst = max(worst, e_ref)
        assert e_ref < 1e-4 or e_truth < 3 * ref_truth, (j, e_ref, e_truth, ref_truth)
    print(f"two sets, composed job, ddim-8 + apf teacher-forced worst vs reference {worst:.2e}")


# ------------------------------------------------------------------------------------------------ 5
RAGGED = ((2, 3, 1), (3, 1, 2))


def _ragged_scenes():
    ks, _ = RAGGED
    return [[dev(synth.make_cloud(4 + ((i + k) % 3), 64, 2, seed=500 + 10 * i + k)) for k in range(K)] for i, K in enumerate(ks)]


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_ragged_job_rows_follow_their_own_scene(sampler):
    """set_counts (2, 3, 1), n_samples (3, 1, 2) in one job of 4 rows per trajectory (padding rows: zero latent, weight 0): every scene's
    rows against that scene's OWN composed job on the same noise rows, as test_2d_mixed_job_rows_follow_their_own_scene compares -- 1e-4
    over the states before the APF hook first fires (DDPM: states 0 .. 21 as there, and this path has no hook at all; DDIM-5 of T = 100
    with the three-pass APF from step 2: states 0 .. 2) -- and a scene's rows against another scene's sets are far off."""
    ks, ns = RAGGED
    scenes = _ragged_scenes()
    ddim = sampler == "ddim"
    dm = _static(100 if ddim else 25, use_apf=True, sampler=sampler, max_rows=24)
    noise = synth.make_noise((1 if ddim else 26, sum(ns), 48, 4), seed=77)
    mixed, ts = _composed(dm, scenes, list(ns), noise)
    assert ts.tolist() == [0, 0, 0, 1, 2, 2] and np.isfinite(mixed).all() and _range_flag(dm.model) == 0
    upto = 3 if ddim else 22
    b = 0
    for i, n in enumerate(ns):
        own, _ = _composed(dm, [scenes[i]], n, noise[:, b:b + n])
        d, d_all = np.abs(mixed[:upto, b:b + n] - own[:upto]).max(), np.abs(mixed[:, b:b + n] - own).max()
        print(f"ragged {sampler} job, scene {i} (K = {ks[i]}): states 0..{upto - 1} vs its own job {d:.2e}; whole chain {d_all:.2e}")
        assert d < 1e-4
        b += n
    wrong, _ = _composed(dm, [scenes[1]], ns[0], noise[:, :ns[0]])
    assert np.abs(mixed[:upto, :ns[0]] - wrong[:upto]).max() > 1e-3


def test_ragged_job_apf_step_reads_each_scenes_own_default_cloud():
    """The APF of a many-scene composed job with the default clouds (apf_clouds=None: every point of every set of the scene, routed through
    traj_scene and the cloud offsets): ONE DDIM step with the three-pass hook, teacher-forced -- the ragged job and each scene's own job
    start from the same state (state 3 of the scene's own chain, where the hook has fired once), so the push decisions see the same x0 to
    rounding -- each scene's rows within the 1e-4 of the free-running comparison above.  The hook is seen to act, and a job whose every
    trajectory avoids scene 1's cloud instead is far off."""
    ks, ns = RAGGED
    scenes = _ragged_scenes()
    dm = _static(100, use_apf=True, sampler="ddim", max_rows=24)
    noise = synth.make_noise((1, sum(ns), 48, 4), seed=77)
    t3 = int(dm.ddim_set_timesteps(5)[3])
    own_state, own_next, own_free, b = [], [], [], 0
    for i, n in enumerate(ns):
        chain, _ = _composed(dm, [scenes[i]], n, noise[:, b:b + n])
        job, guid, hc, _ = dm._prepare_composed_job([scenes[i]], [_hc(4)], n)
        own_state.append(chain[3])
        own_next.append(_one_step(dm, job, guid, hc, n, chain[3], None, t3, ddim=True, apf=1))
        own_free.append(_one_step(dm, job, guid, hc, n, chain[3], None, t3, ddim=True, apf=0))
        b += n
    x = np.concatenate(own_state)
    job, guid, hc, B = dm._prepare_composed_job(scenes, [_hc(4)] * 3, list(ns))
    mixed = _one_step(dm, job, guid, hc, B, x, None, t3, ddim=True, apf=1)
    b = 0
    for i, n in enumerate(ns):
        d, moved = float(np.abs(mixed[b:b + n] - own_next[i]).max()), float(np.abs(own_next[i] - own_free[i]).max())
        print(f"ragged job, one DDIM + APF step, scene {i} (K = {ks[i]}): vs its own job {d:.2e}; the hook moved the step by {moved:.2e}")
        assert d < 1e-4
        b += n
    assert max(float(np.abs(a - f).max()) for a, f in zip(own_next, own_free)) > 1e-3          # the hook acts in this step
    wrong_job = dict(job, traj_scene=torch.ones_like(job["traj_scene"]))                      # everybody avoids scene 1's cloud
    wrong = _one_step(dm, wrong_job, guid, hc, B, x, None, t3, ddim=True, apf=1)
    assert float(np.abs(wrong[:ns[0]] - own_next[0]).max()) > 1e-3


def test_ragged_single_evaluation_and_the_cfg_special_case():
    """One evaluation after the ragged job's set_scenes: each scene's set and unconditional rows equal the same rows evaluated under the
    scene's own table, to the 2e-5 of test_single_evaluation_after_set_scenes_equals_set_scene_per_scene; the padding rows equal the
    unconditional row.  And a scene with ONE set and weight 1 + w is classifier-free guidance at w: one step of its composed job lands
    within the same 2e-5 of the CFG job's."""
    ks, ns = RAGGED
    scenes = _ragged_scenes()
    dm = _static(25, max_rows=24)
    B = sum(ns)
    x = synth.make_noise((B, 48, 4), seed=78)
    job, guid, hc, _ = dm._prepare_composed_job(scenes, [_hc(4)] * 3, list(ns))
    eps, *_ = _eval_composed(dm, x, B, 4, 7, guid["row_weight"])
    eps = eps.reshape(B, 4, 48, 4)
    worst, b = 0.0, 0
    for i, (K, n) in enumerate(zip(ks, ns)):
        _, g1, _, _ = dm._prepare_composed_job([scenes[i]], [_hc(4)], n)
        own, *_ = _eval_composed(dm, x[b:b + n], n, K + 1, 7, g1["row_weight"])
        own = own.reshape(n, K + 1, 48, 4)
        worst = max(worst, float(np.abs(eps[b:b + n, :K] - own[:, :K]).max()), float(np.abs(eps[b:b + n, 3] - own[:, K]).max()))
        for k in range(K, 3):
            worst = max(worst, float(np.abs(eps[b:b + n, k] - eps[b:b + n, 3]).max()))
        b += n
    print(f"ragged job, one evaluation: rows vs the same rows under the scene's own table, max {worst:.2e}")
    assert worst < 2e-5
    # one set, weight 1 + w = CFG at w
    cloud = scenes[2][0]
    nz = synth.make_noise((2, 48, 4), seed=79)
    job, guid, hc, _ = dm._prepare_composed_job([[cloud]], [_hc(4)], 2, weights=1.0 + dm.cfg_weight)
    assert guid["n_rp"] == 2 and guid["row_weight"].cpu().numpy().tolist() == [[3.0, -2.0]] * 2
    a = _one_step(dm, job, guid, hc, 2, x[:2], nz, 9)
    hcb = {k: v.cuda().unsqueeze(0).expand(2, -1) for k, v in _hc(4).items()}
    c, _ = dm._launch(2, torch.stack([dev(x[:2]), dev(nz)]), hcb, cloud, False, [9], [0], [0.5], None, False)
    d = float(np.abs(a - c.cpu().numpy()).max())
    print(f"one set at 1 + w vs the CFG job at w, one step: {d:.2e}")
    assert d < 2e-5


# ------------------------------------------------------------------------------------------------ 6, 7
def _five_row_job(dm, B=7):
    """B scenes of one trajectory each over the same four sets, every scene with weights of its own: n_rp = 5."""
    sets = [dev(synth.make_cloud(5, 64, 2, seed=600 + k)) for k in range(4)]
    w = [[0.5 + 0.25 * i, 1.0, 1.5 - 0.1 * i, 0.75] for i in range(B)]
    return dm._prepare_composed_job([sets] * B, [_hc(4)] * B, 1, w)


def test_chunked_evaluation_offsets_the_weight_table():
    """max_rows = 16, n_rp = 5, B = 7: chunks of 3, 3 and 1 trajectories, every trajectory with other weights, so a chunk that read the
    table from its start would combine with the wrong ones.  One step against max_rows = 40 (one chunk): < 2e-5."""
    x, nz = synth.make_noise((7, 48, 4), seed=80), synth.make_noise((7, 48, 4), seed=81)
    out = {}
    for mr in (16, 40):
        dm = _static(25, max_rows=mr)
        job, guid, hc, B = _five_row_job(dm)
        assert B == 7 and guid["n_rp"] == 5
        out[mr] = _one_step(dm, job, guid, hc, 7, x, nz, 9)
        assert _range_flag(dm.model) == 0
    d = float(np.abs(out[16] - out[40]).max())
    print(f"n_rp = 5, B = 7: chunks of 3 + 3 + 1 vs one chunk, one step: {d:.2e}")
    assert d < 2e-5
    # the mutation this guards against is visible at this size: the first trajectory's weights for everyone
    dm = _static(25, max_rows=40)
    job, guid, hc, B = _five_row_job(dm)
    guid["row_weight"] = guid["row_weight"][:1].repeat(7, 1).contiguous()
    assert float(np.abs(_one_step(dm, job, guid, hc, 7, x, nz, 9)[3:] - out[40][3:]).max()) > 1e-3


def test_plans_shared_prefix_and_graph():
    """n_rp = 4: the shared prefix (weighted combine in the backward, one row into the guidance step) against row-by-row evaluation
    (ramp_cfg_mean_rows on four rows): one step < 2e-5.  The captured graph against eager launches: bitwise, whole DDPM chain."""
    g = np.load(f"{GOLDEN}/compose_sets.npz")
    clouds, w = dev(g["2d/clouds"]), [float(v) for v in g["2d/weights"]]
    out = {}
    for share in (1, 0):
        dm = _static(25, max_rows=12, launch_plan=dict(share_prefix=share))
        job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3, w)
        out[share] = _one_step(dm, job, guid, hc, 3, g["2d/ddpm_chain"][15], g["2d/ddpm_noise"][16], 9)
        e = float(np.abs(out[share] - g["2d/ddpm_chain"][16]).max())
        print(f"share_prefix = {share}: one step vs the reference {e:.2e}")
        assert e < 1e-4
    d = float(np.abs(out[1] - out[0]).max())
    print(f"n_rp = 4, shared prefix vs row by row, one step: {d:.2e}")
    assert d < 2e-5
    a, _ = _composed(_static(25, max_rows=12, use_graph=True), [clouds], 3, g["2d/ddpm_noise"], w)
    b, _ = _composed(_static(25, max_rows=12, use_graph=False), [clouds], 3, g["2d/ddpm_noise"], w)
    assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 8
def test_weights_are_data_of_the_captured_graph():
    """Two jobs of one shape with weights (1.5, 1.0, 1.5) and (0.5, 2.0, 1.0) on ONE scene table, graph on: the second replays the graph
    the first captured (no launch is made for it) and still gets its own weights -- each equals its eager run bitwise, and the two differ.
    A CFG job before and after is bit-equal to itself: jobs do not depend on what ran before."""
    g = np.load(f"{GOLDEN}/compose_sets.npz")
    clouds, noise = dev(g["2d/clouds"]), g["2d/ddpm_noise"]
    ga = np.load(f"{GOLDEN}/chain_ddpm_plain.npz")
    w_a, w_b = [1.5, 1.0, 1.5], [0.5, 2.0, 1.0]

    def cfg(dm):
        with NoiseInjector(list(ga["noise"][:, :3])):
            return dm.run_inference(None, _hc(4), n_samples=3, horizon=48, return_chain=True, obstacle_pts=dev(ga["cloud"]),
                                    noise_std_extra_schedule_fn=lambda x: 0.5).cpu().numpy()

    def pair(dm):
        """Both weight tables on one set_scenes table: (chain a, chain b, kernel launches the second job made)."""
        job, guid, hc, B = dm._prepare_composed_job([clouds], [_hc(4)], 3, w_a)
        guid_b = dict(guid, row_weight=dev(build_compose_tables((3,), 3, [[0, 47]], w_b)["row_weight"]))
        outs = []
        for gd in (guid, guid_b):
            with NoiseInjector(list(noise)):
                _, chain = dm.conditional_sample(hc, horizon=48, batch_size=B, return_chain=True, obstacle_pts=None, scene_job=job, guidance=gd,
                                                 noise_std_extra_schedule_fn=lambda x: 0.5)
            outs.append(chain.permute(1, 0, 2, 3).cpu().numpy())
            assert _range_flag(dm.model) == 0
        return outs[0], outs[1], dm.model.launch_count()

    dm = _static(25, max_rows=12, use_graph=True)
    c0 = cfg(dm)
    a, b, n_second = pair(dm)
    c1 = cfg(dm)
    ea, eb, n_eager = pair(_static(25, max_rows=12, use_graph=False))
    print(f"second job of the shape: {n_second} launches with the graph on, {n_eager} eager; the two jobs differ by {np.abs(a - b).max():.2e}")
    assert n_second == 0 and n_eager > 0                   # a replay of the first job's graph
    assert np.array_equal(a, ea) and np.array_equal(b, eb)
    assert np.abs(a - b).max() > 1e-3
    assert np.abs(a - g["2d/ddpm_chain"]).max() < 2e-4
    assert np.array_equal(c0, c1)
    # and in the other order, on a fresh context: a job's bits do not depend on which weights ran before it
    fresh = _static(25, max_rows=12, use_graph=True)
    job, guid, hc, B = fresh._prepare_composed_job([clouds], [_hc(4)], 3, w_b)
    with NoiseInjector(list(noise)):
        _, chain = fresh.conditional_sample(hc, horizon=48, batch_size=B, return_chain=True, obstacle_pts=None, scene_job=job, guidance=guid,
                                            noise_std_extra_schedule_fn=lambda x: 0.5)
    assert np.array_equal(chain.permute(1, 0, 2, 3).cpu().numpy(), b)


# ------------------------------------------------------------------------------------------------ 9
def test_refusals_through_the_raw_abi():
    """Every refusal of ramp_sample_composed is a host check that names the entry; nothing is launched."""
    lib = _lib.load()
    m = build_unet(4, 48, False, max_rows=16)
    m.prepare_time_table(25)
    lat = torch.cat([m.encode_scene(dev(synth.make_cloud(6, 64, 2, seed=1))), torch.zeros(1, m.context_dim, device="cuda")])
    p = _lib.RampSampleParams()
    p.B, p.n_rp, p.n_steps = 2, 4, 1
    w = torch.zeros(2, 4, device="cuda")
    noise = torch.zeros(2, 2, 48, 4, device="cuda")
    x = torch.zeros(2, 48, 4, device="cuda")

    def call(g, expect):
        n0 = m.launch_count()
        rc = lib.ramp_sample_composed(m.ctx(), C.byref(p), C.byref(g) if g is not None else None, None, _lib.ptr(noise), None, _lib.ptr(x),
                                      _lib.current_stream())
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_sample_composed" in msg and expect in msg, (rc, msg)
        assert m.launch_count() == n0

    def rows(n_rp, ptr=w):
        g = _lib.RampGuidanceRows()
        g.n_rp, g.row_weight = n_rp, _lib.ptr(ptr)
        return g

    m.set_scenes(lat, [0, 1, 1, 1] * 2)
    call(None, "null guidance")
    call(rows(4, None), "null row_weight")
    call(rows(1), "outside 2")
    call(rows(9), "outside 2")
    call(rows(3), "differs")
    m.set_scene(lat, [0, 1, 1, 1])
    call(rows(4), "none is in place")
    m.set_scenes(lat, [0, 1, 1, 1])
    call(rows(4), "shorter")
    # ramp_cfg_mean_rows: the same range of n_rp
    assert lib.ramp_cfg_mean_rows(_lib.ptr(x), _lib.ptr(noise), 2, 192, 9, _lib.ptr(w), 1.0, 1.0, 1.0, 1.0, 1, 0, _lib.ptr(x), None, None,
                                  _lib.current_stream()) != 0
    assert b"ramp_cfg_mean_rows" in lib.ramp_last_error()


def test_python_refusals(monkeypatch):
    """A caller-supplied sample_fn, the dynamic planner and a multi-rank process group are refused by name; so are bad tables."""
    from ramp_amd.models import DynamicGaussianDiffusionModel
    dm = _static(25, max_rows=12)
    clouds = [dev(synth.make_cloud(6, 64, 2, seed=s)) for s in (1, 2, 7)]

    def my_step(model, x, hard_conds, context, t, **kw):
        return x, None

    with pytest.raises(NotImplementedError, match="run_inference_composed"):
        dm.run_inference_composed([clouds], [_hc(4)], n_samples=2, horizon=48, sample_fn=my_step)
    with pytest.raises(ValueError, match="at most 8"):
        dm.run_inference_composed([clouds * 3], [_hc(4)], n_samples=1, horizon=48)
    with pytest.raises(ValueError, match="expected a"):
        dm.run_inference_composed([[clouds[0][0]]], [_hc(4)], n_samples=1, horizon=48)
    dyn = DynamicGaussianDiffusionModel(model=dm.model, n_diffusion_steps=100, predict_epsilon=True).eval().to("cuda")
    with pytest.raises(NotImplementedError, match="run_inference_composed.*dynamic"):
        dyn.run_inference_composed([clouds], [_hc(4)], n_samples=2, horizon=48)
    import torch.distributed as tdist
    monkeypatch.setattr(tdist, "is_available", lambda: True)
    monkeypatch.setattr(tdist, "is_initialized", lambda: True)
    monkeypatch.setattr(tdist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="multi-rank"):
        dm.run_inference_composed([clouds], [_hc(4)], n_samples=2, horizon=48)
