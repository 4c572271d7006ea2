"""Many scenes in one job, job level: ``run_inference_scenes`` on the reference fixtures already under tests/golden/ (two scenes
with clouds of different sizes in ONE job, each under the bars its single-scene test asserts), single evaluations after
``set_scenes`` against ``set_scene``, the kernels a many-scene job dispatches, and independence of what ran before."""
import ctypes as C

import numpy as np
import pytest
import torch

import util
from ramp_amd import _lib, synth
from util import GOLDEN, NoiseInjector, build_unet, dev

pytestmark = pytest.mark.gpu


def _range_flag(u):
    flag = C.c_int32(-1)
    _lib.check(_lib.load().ramp_range_status(u.ctx(), C.byref(flag), _lib.current_stream()))
    return flag.value


def _static(use_graph=True, max_rows=64, launch_plan=util.PLANS["tkw"], gemm_mode="fp16x3"):
    """2-D T = 25 DDPM sampler with the APF hook, on the bench's launch plan (every fused kernel forced onto the small job)."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=max_rows, gemm_mode=gemm_mode, launch_plan=launch_plan)
    return StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True, compose=False,
                                        use_apf=True, sampler="ddpm", use_graph=use_graph).eval().to("cuda")


def _hc(S, H):
    return {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}


def _run_scenes(dm, fixtures, counts=None):
    """One job over the fixtures' scenes, each scene on its fixture's noise; returns (chain (T + 1, B, H, S) numpy, traj_scene)."""
    S, H = dm.state_dim, dm.model.n_support_points
    noise = np.concatenate([g["noise"] for g in fixtures], axis=1)
    with NoiseInjector(list(noise)) as inj:
        chain, ts = dm.run_inference_scenes([dev(g["cloud"]) for g in fixtures], [_hc(S, H) for _ in fixtures],
                                            n_samples=counts or [g["noise"].shape[1] for g in fixtures], return_chain=True, horizon=H,
                                            noise_std_extra_schedule_fn=lambda x: 0.5, n_diffusion_steps_without_noise=0)
        assert inj.used == noise.shape[0]
    return chain.cpu().numpy(), ts.cpu().numpy()


def _teacher_forced_apf_steps(dm, fixtures, first):
    """The steps first .. 24 of a mixed job, each from the references' own previous states (the APF decisions are stiff): worst
    distance to the reference's next state per scene."""
    S, H = dm.state_dim, dm.model.n_support_points
    job, hc, B = dm._prepare_scene_job([dev(g["cloud"]) for g in fixtures], [_hc(S, H) for _ in fixtures], [g["noise"].shape[1] for g in fixtures])
    ref = np.concatenate([g["chain"] for g in fixtures], axis=1)
    nz = np.concatenate([g["noise"] for g in fixtures], axis=1)
    worst = np.zeros(len(fixtures))
    for j in range(first, 25):
        apf = [1 if j > dm.apf_ddpm["after"] else 0]
        x, _ = dm._launch(B, torch.stack([dev(ref[j]), dev(nz[j + 1])]), hc, None, False, [24 - j], apf, [0.5],
                          dict(dm.apf_ddpm, passes=1) if apf[0] else None, False, scene_job=job)
        err = np.abs(x.cpu().numpy() - ref[j + 1]).reshape(B, -1).max(1)
        b = 0
        for s, g in enumerate(fixtures):
            n = g["noise"].shape[1]
            worst[s] = max(worst[s], err[b:b + n].max()); b += n
    return worst


@pytest.mark.parametrize("order", ["AB", "BA"])
def test_2d_mixed_job_meets_both_scenes_bars(order):
    """Scene A (chain_ddpm_apf: 6 x 64 cloud, 4 rows) and scene B (chain_c2: 16 x 64 cloud, 4 rows) in ONE T = 25 DDPM + APF job on
    the bench's plan, and again with the scenes' rows swapped.  Bars: test_ddpm_apf_chain_teacher_forced's for A, the config-2
    full-size test's for B -- states 0 .. 21 (before the first APF application) free-running within 1e-4 of the reference, the APF
    steps teacher-forced within 1e-4 -- graph and eager bitwise equal, no range-guard trip."""
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")
    fx = [ga, gb] if order == "AB" else [gb, ga]
    assert fx[0]["cloud"].shape != fx[1]["cloud"].shape and int(ga["T"]) == int(gb["T"]) == 25
    dm = _static(use_graph=True)
    chain, ts = _run_scenes(dm, fx)
    assert _range_flag(dm.model) == 0 and dm.last_job_mode == "fp16x3"
    assert ts.tolist() == [0] * 4 + [1] * 4 and chain.shape == (26, 8, 48, 4)
    for s, g in enumerate(fx):
        err = np.abs(chain[:22, 4 * s:4 * s + 4] - g["chain"][:22]).max()
        print(f"2-D mixed job {order}, scene {s}: states 0..21 free-running max {err:.2e}")
        assert err < 1e-4
    eager = _static(use_graph=False)
    chain_e, _ = _run_scenes(eager, fx)
    assert _range_flag(eager.model) == 0
    assert np.array_equal(chain, chain_e)                       # graph and eager paths: the same bits
    worst = _teacher_forced_apf_steps(eager, fx, 21)
    print(f"2-D mixed job {order}: APF steps teacher-forced worst per scene {worst}")
    assert worst.max() < 1e-4
    hc = synth.default_hard_conds(4, 48)
    assert np.array_equal(chain[:, :, 0], np.broadcast_to(hc[0], chain[:, :, 0].shape))
    assert np.array_equal(chain[:, :, 47], np.broadcast_to(hc[47], chain[:, :, 47].shape))


def test_2d_mixed_job_rows_follow_their_own_scene():
    """Mutation check at job level: scene A's rows in the mixed job equal (to rounding) scene A sampled alone, and differ from
    scene A's rows sampled against scene B's cloud."""
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")
    dm = _static()
    mixed, _ = _run_scenes(dm, [ga, gb])
    with NoiseInjector(list(ga["noise"])):
        alone = dm.run_inference(None, _hc(4, 48), n_samples=4, horizon=48, return_chain=True, obstacle_pts=dev(ga["cloud"]),
                                 noise_std_extra_schedule_fn=lambda x: 0.5).cpu().numpy()
    with NoiseInjector(list(ga["noise"])):
        wrong = dm.run_inference(None, _hc(4, 48), n_samples=4, horizon=48, return_chain=True, obstacle_pts=dev(gb["cloud"]),
                                 noise_std_extra_schedule_fn=lambda x: 0.5).cpu().numpy()
    assert np.abs(mixed[:22, :4] - alone[:22]).max() < 1e-4
    assert np.abs(mixed[:22, :4] - wrong[:22]).max() > 1e-3


def test_3d_mixed_job_meets_both_scenes_bars():
    """chain3d_ddpm (5 x 50 cloud) and chain_c3 (20 x 200 cloud) -- the same T = 25 and w = 5.75 -- in one GaussianDiffusionModel3d
    job: every step teacher-forced within 1e-4 of the reference (test_chain3d_batched_equals_independent_reference_runs (a), the
    config-3 full-size test's per-step bar), the free-running chain within the config-3 bars of the reference (4.5e-4) and of the
    float64 truth (3 x the reference's own distance, 2.5e-4)."""
    from ramp_amd.models import GaussianDiffusionModel3d
    g1, g2 = np.load(f"{GOLDEN}/chain3d_ddpm.npz"), np.load(f"{GOLDEN}/chain_c3.npz")
    assert int(g1["T"]) == int(g2["T"]) == 25 and float(g1["w"]) == float(g2["w"]) == 5.75
    u = build_unet(6, 48, True, max_rows=16, gemm_mode="fp16x3", launch_plan=util.PLANS["tkw"])
    dm = GaussianDiffusionModel3d(model=u, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True, use_graph=True).eval().to("cuda")
    chain, ts = _run_scenes(dm, [g1, g2])
    assert _range_flag(u) == 0 and ts.tolist() == [0, 0, 1, 1]
    for s, (name, g) in enumerate((("chain3d_ddpm", g1), ("chain_c3", g2))):
        mine = chain[:, 2 * s:2 * s + 2]
        truth = util.oracle64_chain(name, 6, 48, 25, 5.75)
        e_ref = np.abs(g["chain"] - truth).max(); e_gpu = np.abs(mine - truth).max(); err = np.abs(mine - g["chain"]).max()
        print(f"3-D mixed job, {name}: free-running vs reference {err:.2e}; vs float64 truth: reference {e_ref:.2e}, HIP {e_gpu:.2e}")
        assert e_gpu < 3 * e_ref and e_gpu < 2.5e-4 and err < 4.5e-4
    # every step from the references' own previous states
    job, hc, B = dm._prepare_scene_job([dev(g1["cloud"]), dev(g2["cloud"])], [_hc(6, 48)] * 2, [2, 2])
    ref = np.concatenate([g1["chain"], g2["chain"]], axis=1); nz = np.concatenate([g1["noise"], g2["noise"]], axis=1)
    tf = []
    for j in range(25):
        x, _ = dm._launch(B, torch.stack([dev(ref[j]), dev(nz[j + 1])]), hc, None, False, [24 - j], [0], [0.5], None, False, scene_job=job)
        tf.append(float(np.abs(x.cpu().numpy() - ref[j + 1]).max()))
    print("3-D mixed job: teacher-forced per step " + " ".join(f"{e:.1e}" for e in tf))
    assert max(tf) < 1e-4, tf


def test_single_evaluation_after_set_scenes_equals_set_scene_per_scene():
    """ramp_score after set_scenes with N = 16 scenes: each scene's rows equal the same rows evaluated alone through set_scene, to
    the 2e-5 the sharding test asserts for "a shard's rows = the whole batch's rows"; a batch longer than the table is refused."""
    S, H, N, per = 4, 48, 16, 3
    m = build_unet(S, H, False, max_rows=2 * N * per)
    m.prepare_time_table(25)
    gen = torch.Generator(device="cpu").manual_seed(3)
    clouds = [dev(synth.make_cloud(4 + (i % 5), 64, 2, seed=100 + i)) for i in range(N)]
    lat = torch.cat([m.encode_scene(c) for c in clouds] + [torch.zeros(1, m.context_dim, device="cuda")])
    B = N * per
    scene = torch.randperm(N, generator=gen).repeat_interleave(per)            # a scene's rows adjacent, scenes in random order
    rv = torch.stack([scene, torch.full_like(scene, N)], dim=1).reshape(-1)
    x = torch.randn(B, H, S, generator=gen).cuda()
    lib = _lib.load()

    def score(xb, nb):
        eps = torch.empty(nb * 2, H, S, device="cuda")
        _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xb.contiguous()), nb, 2, 7, None, _lib.ptr(eps), _lib.current_stream()), "ramp_score")
        torch.cuda.synchronize()
        return eps

    m.set_scenes(lat, rv)
    whole = score(x, B)
    bad = torch.empty(2 * (B + 1), H, S, device="cuda")
    assert lib.ramp_score(m.ctx(), _lib.ptr(torch.zeros(B + 1, H, S, device="cuda")), B + 1, 2, 7, None, _lib.ptr(bad), _lib.current_stream()) != 0
    assert b"ramp_set_scenes" in lib.ramp_last_error()
    worst = 0.0
    for i in range(N):
        s = int(scene[i * per])
        m.set_scene(torch.stack([lat[s], lat[N]]), [0, 1])
        alone = score(x[i * per:(i + 1) * per], per)
        worst = max(worst, float((alone - whole[2 * i * per:2 * (i + 1) * per]).abs().max()))
    print(f"set_scenes N = 16: rows vs the same rows through set_scene, max {worst:.2e}")
    assert worst < 2e-5
    # and a wrong table is seen: every conditional row reading scene 0's latent moves the result
    m.set_scenes(lat, torch.stack([torch.zeros_like(scene), torch.full_like(scene, N)], dim=1).reshape(-1))
    assert float((score(x, B) - whole).abs().max()) > 1e-3

@pytest.mark.parametrize("plan", ["tkw", "m32"])
def test_single_evaluation_on_the_fused_plan_reads_each_rows_own_constant(plan):
    """The values of the global-memory row constant as the ENGINE calls it (rb_stride = blocks x 256, the per-block base, 17 variants):
    steady fp16x3 evaluations after set_scenes with N = 16 scenes on the bench's plan forced onto the small batch -- ato_kernel and
    tkl16_kernel ("tkw"), tkl_kernel ("m32": mfma16 = 0) -- against the same rows evaluated alone through set_scene (2 variants: the
    LDS-staged constant), scene by scene, in the sharding test's measure and to its 2e-5.  The fused kernels are seen to launch (per-kernel
    profile of score()'s two evaluations, like for like with one scene) and nothing takes the attention kernel's place; a table that points every row at scene 0 is seen."""
    S, H, N, per = 4, 48, 16, 3
    m = build_unet(S, H, False, max_rows=2 * N * per, gemm_mode="fp16x3", launch_plan=util.PLANS[plan])
    m.prepare_time_table(25)
    gen = torch.Generator(device="cpu").manual_seed(11)
    clouds = [dev(synth.make_cloud(4 + (i % 5), 64, 2, seed=400 + i)) for i in range(N)]
    lat = torch.cat([m.encode_scene(c) for c in clouds] + [torch.zeros(1, m.context_dim, device="cuda")])
    B = N * per
    scene = torch.randperm(N, generator=gen).repeat_interleave(per)
    rv = torch.stack([scene, torch.full_like(scene, N)], dim=1).reshape(-1)
    x = torch.randn(B, H, S, generator=gen).cuda()
    lib = _lib.load()

    def score(xb, nb):
        eps = torch.empty(nb * 2, H, S, device="cuda")
        xb = xb.contiguous()
        for _ in range(2):      # (the first evaluation after a scene change calibrates with the bf16x6 kernels: compare steady fp16x3 evaluations)
            _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xb), nb, 2, 7, None, _lib.ptr(eps), _lib.current_stream()), "ramp_score")
        torch.cuda.synchronize()
        assert m.score_mode() == "fp16x3"
        return eps

    m.set_scenes(lat, rv)
    score(x, B)
    _lib.check(lib.ramp_profile(m.ctx(), 1))
    whole = score(x, B)
    cnt = (C.c_int64 * 9)(); ms = (C.c_double * 9)(); fl = (C.c_double * 9)()
    _lib.check(lib.ramp_profile_read_kernels(m.ctx(), 9, ms, fl, cnt))
    ccnt = (C.c_int64 * 5)(); cms = (C.c_double * 5)(); cfl = (C.c_double * 5)()
    _lib.check(lib.ramp_profile_read(m.ctx(), cms, cfl, ccnt))
    _lib.check(lib.ramp_profile(m.ctx(), 0))
    print(f"{plan}: kernel launches of two evaluations with 17 variants {list(cnt)}, categories {list(ccnt)}")
    assert cnt[2] > 0 and cnt[4] > 0 and cnt[0] > 0, list(cnt)       # tkl / tkl16, ato, ffx launched ...
    m.set_scene(torch.stack([lat[0], lat[N]]), [0, 1])
    score(x, B)
    _lib.check(lib.ramp_profile(m.ctx(), 1))
    score(x, B)
    cnt1 = (C.c_int64 * 9)(); ccnt1 = (C.c_int64 * 5)()
    _lib.check(lib.ramp_profile_read_kernels(m.ctx(), 9, ms, fl, cnt1))
    _lib.check(lib.ramp_profile_read(m.ctx(), cms, cfl, ccnt1))
    _lib.check(lib.ramp_profile(m.ctx(), 0))
    assert list(cnt) == list(cnt1) and list(ccnt) == list(ccnt1), (list(cnt1), list(ccnt1))      # ... exactly as with one scene
    worst = worst_abs = 0.0
    for i in range(N):
        s = int(scene[i * per])
        m.set_scene(torch.stack([lat[s], lat[N]]), [0, 1])
        alone = score(x[i * per:(i + 1) * per], per).cpu().numpy()
        mine = whole[2 * i * per:2 * (i + 1) * per].cpu().numpy()
        worst = max(worst, util.rel(mine, alone)); worst_abs = max(worst_abs, float(np.abs(mine - alone).max()))
    print(f"{plan}: set_scenes N = 16 on the fused kernels, rows vs the same rows through set_scene: rel {worst:.2e}, abs {worst_abs:.2e}")
    assert worst < 2e-5
    m.set_scenes(lat, torch.stack([torch.zeros_like(scene), torch.full_like(scene, N)], dim=1).reshape(-1))
    assert util.rel(score(x, B).cpu().numpy(), whole.cpu().numpy()) > 1e-3


def _kernel_counts(m, x, B):
    """Per-kernel launch counts of one eager fp16x3 evaluation (after its calibration) + the per-category counts."""
    lib = _lib.load()
    H, S = x.shape[1], x.shape[2]
    eps = torch.empty(2 * B, H, S, device="cuda")
    go = lambda: _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(x), B, 2, 7, None, _lib.ptr(eps), _lib.current_stream()), "ramp_score")
    go(); go()
    _lib.check(lib.ramp_profile(m.ctx(), 1))
    go()
    ms = (C.c_double * 9)(); fl = (C.c_double * 9)(); cnt = (C.c_int64 * 9)()
    _lib.check(lib.ramp_profile_read_kernels(m.ctx(), 9, ms, fl, cnt))
    cms = (C.c_double * 5)(); cfl = (C.c_double * 5)(); ccnt = (C.c_int64 * 5)()
    _lib.check(lib.ramp_profile_read(m.ctx(), cms, cfl, ccnt))
    _lib.check(lib.ramp_profile(m.ctx(), 0))
    assert m.score_mode() == "fp16x3"
    return list(cnt), list(ccnt), eps


def test_many_scene_job_dispatches_the_single_scene_plan():
    """64 scenes x 32 samples = 4096 network rows on the library's default plan against a single-scene evaluation of the same B:
    the same launch counts per kernel family (ffx, tkl, ato present), the same number of attention-fallback launches (category 1)
    and of tile-GEMM launches (slot 8) -- the row constant in global memory keeps the job on the fused kernels.  And the values those
    launches produce (65 variants, many blocks per launch): sampled scenes' rows against the same rows evaluated alone through set_scene,
    in the sharding test's measure and to its 2e-5."""
    S, H, N, per = 4, 48, 64, 32
    B = N * per
    m = build_unet(S, H, False, max_rows=2 * B, gemm_mode="fp16x3")
    m.prepare_time_table(25)
    gen = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(B, H, S, generator=gen).cuda()
    clouds = [dev(synth.make_cloud(6, 64, 2, seed=200 + i)) for i in range(N)]
    lat = torch.cat([m.encode_scene(c) for c in clouds] + [torch.zeros(1, m.context_dim, device="cuda")])
    m.set_scene(torch.stack([lat[0], lat[N]]), [0, 1])
    single, single_cat, _ = _kernel_counts(m, x, B)
    scene = torch.arange(N).repeat_interleave(per)
    m.set_scenes(lat, torch.stack([scene, torch.full_like(scene, N)], dim=1).reshape(-1))
    many, many_cat, eps = _kernel_counts(m, x, B)
    print(f"kernel launches ffx_fwd ffx_bwd tkl tklb ato abl tkc tkw other: single scene {single}, 64 scenes {many}; categories {single_cat} / {many_cat}")
    assert many == single and many_cat == single_cat
    assert many[0] > 0 and many[1] > 0 and many[2] > 0 and many[4] > 0, many
    eps = eps.cpu().numpy()
    lib = _lib.load()
    worst = 0.0
    for s in (0, 1, 37, 63):
        m.set_scene(torch.stack([lat[s], lat[N]]), [0, 1])
        xs = x[s * per:(s + 1) * per].contiguous()
        alone = torch.empty(2 * per, H, S, device="cuda")
        for _ in range(2):      # (calibration, then a steady fp16x3 evaluation)
            _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xs), per, 2, 7, None, _lib.ptr(alone), _lib.current_stream()), "ramp_score")
        torch.cuda.synchronize()
        worst = max(worst, util.rel(eps[2 * s * per:2 * (s + 1) * per], alone.cpu().numpy()))
    print(f"64 scenes on the fused kernels, scenes 0 / 1 / 37 / 63 vs the same rows through set_scene: rel {worst:.2e}")
    assert worst < 2e-5


def test_jobs_do_not_depend_on_what_ran_before():
    """A multi-scene job gives the same bits on a fresh context and after a single-scene job; a single-scene job gives the same
    bits before and after a multi-scene job; no job trips the range guard."""
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")

    def single(dm):
        with NoiseInjector(list(ga["noise"])):
            c = dm.run_inference(None, _hc(4, 48), n_samples=4, horizon=48, return_chain=True, obstacle_pts=dev(ga["cloud"]),
                                 noise_std_extra_schedule_fn=lambda x: 0.5).cpu().numpy()
        assert _range_flag(dm.model) == 0
        return c

    fresh = _static()
    multi_fresh, _ = _run_scenes(fresh, [ga, gb])
    assert _range_flag(fresh.model) == 0
    dm = _static()
    s0 = single(dm)
    multi_after, _ = _run_scenes(dm, [ga, gb])
    assert _range_flag(dm.model) == 0
    s1 = single(dm)
    assert np.array_equal(multi_fresh, multi_after)
    assert np.array_equal(s0, s1)
    multi_again, _ = _run_scenes(dm, [ga, gb])
    assert np.array_equal(multi_again, multi_fresh)


def test_graphs_survive_buffer_growth():
    """test_gpu_sampler's test of the same name through ramp_sample_scenes, on one graph-mode and one eager context: (1) the
    two-scene job [A, B] with its chain, (2) the same job with no chain asked for, (3) the four-scene job [A, B, A, B] -- twice
    the trajectories, scenes and cloud points: the per-trajectory scene table, the cloud offsets, the cloud and every per-B
    buffer move -- (4) job 1 again.  Final states of 1, 2 and 4 bitwise equal; chains of 1 and 4 bitwise equal on both contexts,
    to each other and to a fresh context's; chain 4 within test_2d_mixed_job_meets_both_scenes_bars' free-running bar (states
    0 .. 21 of either scene within 1e-4 of its reference); no job trips the range guard.  A regression sequence over graph, eager
    and fresh contexts: every job here resets the scene table and has another graph key than its predecessor, so each captures
    afresh (test_gpu_sampler.py::test_replan_graphs_survive_buffer_growth is where a key outlives a move)."""
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")
    fx = [ga, gb]
    noise = np.concatenate([g["noise"] for g in fx], axis=1)

    def final_only(dm):
        job, hc, B = dm._prepare_scene_job([dev(g["cloud"]) for g in fx], [_hc(4, 48) for _ in fx], [4, 4])
        with NoiseInjector(list(noise)) as inj:
            x = dm.conditional_sample(hc, horizon=48, batch_size=B, return_chain=False, obstacle_pts=None, scene_job=job,
                                      noise_std_extra_schedule_fn=lambda x: 0.5)
            assert inj.used == noise.shape[0]
        return x.cpu().numpy()

    def sequence(dm):
        c1, _ = _run_scenes(dm, fx)
        x2 = final_only(dm)
        c3, ts3 = _run_scenes(dm, fx + fx)
        assert c3.shape == (26, 16, 48, 4) and ts3.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
        c4, _ = _run_scenes(dm, fx)
        assert _range_flag(dm.model) == 0
        assert np.array_equal(c1[-1], x2) and np.array_equal(c1[-1], c4[-1])
        return c1, c4

    g1, g4 = sequence(_static(use_graph=True))
    e1, e4 = sequence(_static(use_graph=False))
    fresh, _ = _run_scenes(_static(use_graph=True), fx)
    assert np.array_equal(g1, g4) and np.array_equal(e1, e4) and np.array_equal(g1, e1) and np.array_equal(g4, fresh)
    for s, g in enumerate(fx):
        err = np.abs(g4[:22, 4 * s:4 * s + 4] - g["chain"][:22]).max()
        print(f"two-scene job after a four-scene job moved the buffers, scene {s}: states 0..21 free-running max {err:.2e}")
        assert err < 1e-4


def test_custom_step_function_is_refused_with_a_message():
    """A caller-supplied sample_fn steps one scene's batch through the eager loop: a many-scene job refuses it by name."""
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")
    dm = _static()

    def my_step(model, x, hard_conds, context, t, **kw):
        return x, None

    with pytest.raises(NotImplementedError, match="run_inference_scenes"):
        dm.run_inference_scenes([dev(ga["cloud"]), dev(gb["cloud"])], [_hc(4, 48)] * 2, n_samples=2, horizon=48, sample_fn=my_step)


def test_ddim_configured_model_runs_the_scene_job_on_its_ddim_loop():
    """The sampler of a many-scene job is the model's own, as in run_inference (conditional_sample looks at the model's setting): a
    DDIM-5-of-100 model takes ddim_p_sample_loop with the scene job.  6 states come back; scene A's rows are what run_inference gives
    for scene A alone from the same x_T, to the 2e-4 by which two fp32-faithful evaluations of a free-running chain agree
    (test_sharded_philox_jobs_reproduce_the_unsharded_job); against scene B's cloud they are not.  APF off (its decisions are stiff)."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    ga, gb = np.load(f"{GOLDEN}/chain_ddpm_apf.npz"), np.load(f"{GOLDEN}/chain_c2.npz")
    u = build_unet(4, 48, False, max_rows=64, gemm_mode="fp16x3", launch_plan=util.PLANS["tkw"])
    dm = StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=100, predict_epsilon=True, compose=False,
                                      use_apf=False, use_graph=True).eval().to("cuda")
    assert dm.ddim
    xT = synth.make_noise((1, 8, 48, 4), seed=31)
    with NoiseInjector([xT[0]]) as inj:
        chain, ts = dm.run_inference_scenes([dev(ga["cloud"]), dev(gb["cloud"])], [_hc(4, 48)] * 2, n_samples=4, return_chain=True, horizon=48)
        assert inj.used == 1
    chain = chain.cpu().numpy()
    assert chain.shape == (6, 8, 48, 4) and np.isfinite(chain).all() and ts.tolist() == [0] * 4 + [1] * 4 and _range_flag(u) == 0
    outs = []
    for g in (ga, gb):
        with NoiseInjector([xT[0, :4]]):
            outs.append(dm.run_inference(None, _hc(4, 48), n_samples=4, horizon=48, return_chain=True, obstacle_pts=dev(g["cloud"])).cpu().numpy())
    d = np.abs(chain[:, :4] - outs[0]).max()
    print(f"DDIM scene job, scene A's rows vs scene A alone: {d:.2e}; vs the same x_T against scene B's cloud {np.abs(chain[:, :4] - outs[1]).max():.2e}")
    assert d < 2e-4
    assert np.abs(chain[:, :4] - outs[1]).max() > 1e-3
