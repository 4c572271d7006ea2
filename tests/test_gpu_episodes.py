"""Many pursuit-evasion episodes replanned in lock-step (run_inference_episodes -> ramp_sample_scenes + ramp_replan_episodes) against the
reference planner's recorded run (replan_chain.npz) and against the single-episode path (ramp_replan)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramp_amd import _lib
from ramp_amd.apf_dynamic import generate_box_points, generate_sphere_points
from ramp_amd.diffusion import _HostArrays
from ramp_amd.scenes import build_episode_tables
from test_gpu_sampler import assert_replan_as_accurate_as_the_reference
from util import FAKE_BOX_CENTRES, GOLDEN, NoiseInjector, build_unet, dev, make_fake_pursuit_env

pytestmark = pytest.mark.gpu


def make_dynamic(max_rows, use_graph=True):
    from ramp_amd.models import DynamicGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=max_rows)
    return DynamicGaussianDiffusionModel(model=u, n_diffusion_steps=100, predict_epsilon=True, use_graph=use_graph).eval().to("cuda")


def fixture_episode(g, log_env):
    """The episode of replan_chain.npz: its environment (own instance), hard conditions, cloud and numpy stream."""
    dataset, sphere = make_fake_pursuit_env(log=log_env)
    H = g["noise"].shape[2]
    hard = {0: torch.from_numpy(g["hard0"]), H - 1: torch.from_numpy(g["hardN"])}
    return {'dataset': dataset}, sphere, hard, dev(g["cloud"]), np.random.RandomState(23)


def assert_selections_match_the_fixture(g, entries, n_sel):
    """One episode's log entries (selection 0 = the high-level plan) against the reference run: selected index, free mask, cost-cloud size
    equal; the ranked batches under test_gpu_sampler's accuracy rule.  Returns the distances to the float64 twin."""
    assert len(entries) == n_sel
    e64, r64 = [], []
    for j, en in enumerate(entries):
        tr, free = en["batch"].cpu().numpy(), en["free"].cpu().numpy()
        ref_free, ref_idx = g[f"cost{j}/free"], int(g[f"cost{j}/idx"])
        if not (en["idx"] == ref_idx and np.array_equal(free, ref_free)):
            print(f"   selection {j}: idx {en['idx']} (reference {ref_idx}), free {free.astype(int)} (reference {ref_free.astype(int)}), "
                  f"max |batch - reference's| {float(np.abs(tr - g[f'cost{j}/trajs']).max()):.3e}")
        assert en["npts"] == int(g[f"cost{j}/npts"]), (j, en["npts"])
        assert en["idx"] == ref_idx and np.array_equal(free, ref_free), (j, en["idx"], free)
        e64.append(float(np.abs(tr - g[f"cost{j}/trajs64"]).max()))
        r64.append(float(np.abs(g[f"cost{j}/trajs"] - g[f"cost{j}/trajs64"]).max()))
    assert_replan_as_accurate_as_the_reference(e64, r64)
    return e64


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager-launch"])
def test_three_copies_of_the_reference_run_in_one_job(use_graph):
    """E = 3 episodes, each the reference planner's recorded episode (replan_chain.npz: 6 candidates, its cloud, start / goal, fake
    environment, numpy stream 23, its torch noise tiled over the episodes): every selection of every episode picks the reference's
    candidate with the reference's collision mask and cost-cloud size, every evader state handed to a pursuer and every pursuer's final
    position are the reference's, and every ranked batch is as close to the float64 twin as test_gpu_sampler asks of the one-episode
    planner.  max_iteration = n_iter: n_iter environment calls and 1 + n_iter selections per episode."""
    g = np.load(f"{GOLDEN}/replan_chain.npz")
    K = int(g["n_iter"]); B0, H, S = g["noise"].shape[1:]
    E = 3
    dm = make_dynamic(2 * E * B0, use_graph)
    logs = [[] for _ in range(E)]
    made = [fixture_episode(g, logs[e]) for e in range(E)]
    dm.replan_log = []
    with NoiseInjector([np.tile(n, (E, 1, 1)) for n in g["noise"]]) as inj:
        out = dm.run_inference_episodes([m[0] for m in made], [m[2] for m in made], [m[3] for m in made], n_samples=B0,
                                        rngs=[m[4] for m in made], return_chain=True, max_iteration=K)
    assert inj.used == 1 + K and len(out) == E and len(dm.replan_log) == E * (1 + K)
    assert dm.range_fallbacks == 0
    for e in range(E):
        print(f" episode {e}")
        assert_selections_match_the_fixture(g, [en for en in dm.replan_log if en["episode"] == e], 1 + K)
        assert len(logs[e]) == K
        for j, (t, st) in enumerate(logs[e]):
            assert t == int(g[f"env{j}/t"])
            assert st.shape == (B0, 2) and float(np.abs(st - g[f"env{j}/state"]).max()) < 1e-5, (e, j)
        assert np.abs(made[e][1].centers.numpy() - g["pursuer_final"]).max() < 1e-4
        chain, chain_obs, chain_start = out[e]
        assert chain.shape == (K + 1, 1, H, S) and len(chain_obs) == K and len(chain_start) == K + 1
        assert bool(torch.isfinite(chain).all())


def test_one_call_of_unequal_episodes_against_the_single_episode_path():
    """ramp_replan_episodes driven directly: E = 2 with 5 and 8 candidates (an odd and an even count: both reference_compat row patterns),
    different stepp (0, 3), n_hist (1, 4), goals, static APF clouds (256 and 96 points) and cost clouds (384 and 320 points).  The pursuer of
    episode 1 is within thr_pred of its evader and its sphere points join its cost cloud; the pursuer of episode 0 is far away.  So the rows that
    take the pursuer pass are rows 5 .. 12: they must read the SECOND block of pursuer points, blend towards THEIR goal (not row 0's, which
    is episode 0's) and collide with the second slot of extra points.  The reference is one ramp_replan call per episode with that episode's
    scene installed and the same noise rows.  Collision masks, result records and winners' rows are equal; the batches agree to the bar the
    project holds the same candidates to at different batch positions (1.5e-4, test_dynamic_replanning_reference_run_embedded_in_a_large_batch:
    the operand scales of the fp16x3 products and the wave tiles' summation orders depend on the batch a row sits in).  That bar pins the
    pursuer pass because the pass matters here: with episode 1's pursuer points moved out of reach the single path's batch changes by far more
    (asserted: > 1e-3; a hit pushes a waypoint by at least 0.15 exp(-0.5 / 0.2) = 0.012).
    Measured on an MI355X: batches 8.9e-7 (episode 0) and 4.0e-6 (episode 1) apart; out of reach, episode 1 moves by 0.47; DESIGN.md section 5."""
    g = np.load(f"{GOLDEN}/replan_chain.npz")
    H, S = 48, 4
    counts = [5, 8]
    E, B = len(counts), sum(counts)
    dm = make_dynamic(2 * B)
    m, lib, device = dm.model, _lib.load(), torch.device("cuda")
    rng = np.random.RandomState(5)
    clouds = [dev(g["cloud"]), dev(np.stack([generate_box_points(c, (0.16, 0.16), 64, rng=rng) for c in FAKE_BOX_CENTRES[:5]]).astype(np.float32))]
    cost = [c.reshape(-1, 2).contiguous() for c in clouds]
    static = [dev(np.vstack([generate_box_points(c, (0.16, 0.16), n, rng=rng) for c in FAKE_BOX_CENTRES[:k]])) for k, n in ((4, 64), (3, 32))]
    assert [c.shape[0] for c in cost] == [384, 320] and [s.shape[0] for s in static] == [256, 96] and static[0].dtype == torch.float64
    ends = [(g["hard0"], g["hardN"]), (np.float32([-0.8, 0.0, 0, 0]), np.float32([0.8, 0.1, 0, 0]))]
    stepp, n_hist = [0, 3], [1, 4]
    # the clean plans: the reference run's high-level plan (collision-free in its cloud), and a straight line at constant velocity
    w = np.linspace(0, 1, H, dtype=np.float32)[:, None]
    line = (1 - w) * ends[1][0][None] + w * ends[1][1][None]
    line[1:-1, 2:] = (ends[1][1][:2] - ends[1][0][:2]) / (0.1 * (H - 1))
    plans = [g["cost0/best"].astype(np.float32), line.astype(np.float32)]
    x_clean = dev(np.stack(plans))
    hist = torch.zeros((E, H, S), device=device)
    for e in range(E):
        hist[e, :n_hist[e]] = x_clean[e, :n_hist[e]]
    centres = [plans[0][stepp[0], :2].astype(np.float64) + [0.7, 0.7], plans[1][stepp[1], :2].astype(np.float64) + [0.15, 0.1]]
    near = np.array([0, 1], np.int32)                        # |(0.7, 0.7)| = 0.99 > thr_pred = 0.5; |(0.15, 0.1)| = 0.18 < 0.4 < thr_pred
    dyn = np.stack([generate_sphere_points(c, 0.1, 64, rng=rng) for c in centres])
    extra = np.stack([generate_sphere_points(c, 0.1, 64, rng=rng) for c in centres]).astype(np.float32)
    noise = torch.randn((B, H, S), device=device, generator=torch.Generator(device).manual_seed(10))
    hard_e = [{0: dev(a).repeat(n, 1), H - 1: dev(b).repeat(n, 1)} for (a, b), n in zip(ends, counts)]
    tab = build_episode_tables(counts, [dm._row_pattern(n) for n in counts])
    first = tab["traj_first"]
    ts = [int(i) for i in dm.ddim_set_timesteps(dm.ddim_num_inference_steps_high)]
    low = ts[-dm.ddim_num_inference_steps_low:]
    m.prepare_time_table(dm.n_diffusion_steps)

    # ---- the single-episode path, one call per episode
    def single(e, dyn_e):
        n = counts[e]
        dm._prepare_scene(clouds[e], n)
        arrays = _HostArrays()
        p = dm._replan_params(n, low, hard_e[e], cost[e], 0.05, arrays)
        p.static_pts, p.n_static = _lib.ptr(static[e]), static[e].shape[0]
        st = _lib.RampReplanState()
        nz = noise[first[e]:first[e + 1]].contiguous()
        st.noise, st.x_clean, st.history = _lib.ptr(nz), _lib.ptr(x_clean[e]), _lib.ptr(hist[e])
        st.n_hist, st.stepp = n_hist[e], stepp[e]
        d, x = np.ascontiguousarray(dyn_e), np.ascontiguousarray(extra[e])
        st.dyn_pts_host, st.near, st.extra_pts_host = d.ctypes.data, int(near[e]), x.ctypes.data if near[e] else None
        st.pursuer[0], st.pursuer[1] = float(np.float32(centres[e][0])), float(np.float32(centres[e][1]))
        best, batch, mask = torch.empty((H, S), device=device), torch.empty((n, H, S), device=device), torch.empty(n, dtype=torch.int32, device=device)
        res = _lib.RampReplanResult()
        _lib.check(lib.ramp_replan(m.ctx(), C.byref(p), C.byref(st), _lib.ptr(best), _lib.ptr(batch), _lib.ptr(mask), C.byref(res),
                                   _lib.current_stream()), "ramp_replan")
        assert res.fell_back == 0
        return best.cpu().numpy(), batch.cpu().numpy(), mask.cpu().numpy(), [res.n_free, res.best_rank, res.best_row]

    ref = [single(e, dyn[e]) for e in range(E)]
    m.scene_cache.clear(); m.invalidate_scene()
    out_of_reach = float(np.abs(single(1, dyn[1] + 10.0)[1] - ref[1][1]).max())
    print(f"   episode 1 with its pursuer points out of reach: the single path's batch moves by {out_of_reach:.3e}")
    assert out_of_reach > 1e-3

    # ---- the same two episodes as one job
    latents = torch.cat([m.encode_scene(c) for c in clouds] + [torch.zeros(1, m.context_dim, device=device)])
    m.set_scenes(latents, tab["row_variant"])
    hard = {k: torch.cat([h[k] for h in hard_e]).contiguous() for k in hard_e[0]}
    cost_all, static_all = torch.cat(cost).contiguous(), torch.cat(static).contiguous()
    cost_off = np.array([0, 384, 704], np.int32)
    static_off = np.array([0, 256, 352], np.int32)
    arrays = _HostArrays()
    p = dm._replan_params(B, low, hard, cost_all, 0.05, arrays)
    p.cost_cloud, p.n_cost = None, 0
    state = (_lib.RampEpisodeState * E)()
    for e in range(E):
        state[e].n_hist, state[e].stepp, state[e].active = n_hist[e], stepp[e], 1
        state[e].pursuer[0], state[e].pursuer[1] = float(np.float32(centres[e][0])), float(np.float32(centres[e][1]))
    eb = _lib.RampEpisodeBatch()
    eb.n_episodes, eb.traj_first_host, eb.state_host = E, first.ctypes.data_as(_lib.c_i32p), state
    eb.noise, eb.x_clean, eb.history = _lib.ptr(noise), _lib.ptr(x_clean), _lib.ptr(hist)
    eb.static_pts, eb.static_offset_host = _lib.ptr(static_all), static_off.ctypes.data_as(_lib.c_i32p)
    eb.cost_cloud, eb.cost_offset_host = _lib.ptr(cost_all), cost_off.ctypes.data_as(_lib.c_i32p)
    eb.dyn_pts_host, eb.near_host, eb.extra_pts_host = dyn.ctypes.data, near.ctypes.data_as(_lib.c_i32p), extra.ctypes.data
    best, batch, mask = torch.empty((E, H, S), device=device), torch.empty((B, H, S), device=device), torch.empty(B, dtype=torch.int32, device=device)
    results, rr = np.zeros((E, 4), np.int32), _lib.RampReplanResult()
    _lib.check(lib.ramp_replan_episodes(m.ctx(), C.byref(p), C.byref(eb), _lib.ptr(best), _lib.ptr(batch), _lib.ptr(mask),
                                        results.ctypes.data_as(_lib.c_i32p), C.byref(rr), _lib.current_stream()), "ramp_replan_episodes")
    assert rr.fell_back == 0
    best, batch, mask = best.cpu().numpy(), batch.cpu().numpy(), mask.cpu().numpy()
    assert np.isfinite(batch).all()
    dist = []
    for e in range(E):
        r_best, r_batch, r_mask, (n_free, rank, row) = ref[e]
        sl = slice(first[e], first[e + 1])
        dist.append(float(np.abs(batch[sl] - r_batch).max()))
        print(f"   episode {e}: free {n_free} of {counts[e]}, record {results[e].tolist()}, max |batch - single path's| {dist[-1]:.3e}")
        assert np.array_equal(mask[sl], r_mask), (e, mask[sl], r_mask)
        assert results[e].tolist() == [n_free, rank, row + first[e] if n_free else -1, 0], (e, results[e], ref[e][3])
        assert dist[-1] < 1.5e-4
        if n_free:
            assert float(np.abs(best[e] - r_best).max()) < 1.5e-4
            assert np.array_equal(best[e][0, 2:], [0, 0])
    assert rr.n_free == sum(r[3][0] for r in ref)


def test_an_episode_that_ends_early_keeps_its_rows_and_is_ignored():
    """Two episodes, max_iteration = 3.  Episode A starts in free space 0.14 from its goal (inside safe_threshold = 0.2), so by
    _Episode.reached it ends after exactly one replan whatever the network outputs; episode B is the reference run's.  A's chain has the
    length its own run_inference gives and does not grow afterwards, its later result records are {-1, -1, -1, 0}; B's selections still
    match the reference run; everything stays finite."""
    g = np.load(f"{GOLDEN}/replan_chain.npz")
    K = 3; B0, H, S = g["noise"].shape[1:]
    dm = make_dynamic(4 * B0)
    hard_a = {0: torch.tensor([0.05, -0.05, 0.0, 0.0]), H - 1: torch.tensor([0.15, 0.05, 0.0, 0.0])}
    cloud_a = dev(np.stack([generate_box_points(c, (0.16, 0.16), 64, rng=np.random.RandomState(3)) for c in FAKE_BOX_CENTRES]).astype(np.float32))
    gen = torch.Generator().manual_seed(4)
    noise_a = [torch.randn((B0, H, S), generator=gen).numpy() for _ in range(1 + K)]
    # A alone: how long its chain is
    with NoiseInjector(list(noise_a)):
        chain_alone, _obs, _start = dm.run_inference(context={'dataset': make_fake_pursuit_env()[0]}, hard_conds=hard_a, n_samples=B0,
                                                     return_chain=True, obstacle_pts=cloud_a, max_iteration=K)
    assert chain_alone.shape[0] == 2
    log_b = []
    ctx_b, sphere_b, hard_b, cloud_b, rng_b = fixture_episode(g, log_b)
    dm.replan_log = []
    with NoiseInjector([np.concatenate([na, nb]) for na, nb in zip(noise_a, g["noise"])]) as inj:
        out = dm.run_inference_episodes([{'dataset': make_fake_pursuit_env()[0]}, ctx_b], [hard_a, hard_b], [cloud_a, cloud_b], n_samples=B0,
                                        rngs=[np.random.RandomState(9), rng_b], return_chain=True, max_iteration=K)
    assert inj.used == 1 + K and dm.range_fallbacks == 0
    (chain_a, obs_a, start_a), (chain_b, obs_b, start_b) = out
    assert chain_a.shape == chain_alone.shape and len(obs_a) == 1 and len(start_a) == 2
    assert chain_b.shape == (K + 1, 1, H, S) and len(obs_b) == K
    log_a = [en for en in dm.replan_log if en["episode"] == 0]
    assert [en["active"] for en in log_a] == [True, True] + [False] * (K - 1) and log_a[1]["record"][0] >= 0
    for en in log_a[2:]:
        assert en["record"] == [-1, -1, -1, 0], en
    assert_selections_match_the_fixture(g, [en for en in dm.replan_log if en["episode"] == 1], 1 + K)
    assert len(log_b) == K
    for j, (t, st) in enumerate(log_b):
        assert t == int(g[f"env{j}/t"]) and float(np.abs(st - g[f"env{j}/state"]).max()) < 1e-5
    for t in (chain_a, chain_b):
        assert bool(torch.isfinite(t).all())
    last = chain_a[-1, 0].cpu().numpy()
    assert np.allclose(last[0, :2], [0.05, -0.05]) and np.allclose(last[-1], [0.15, 0.05, 0, 0])


class BatchNoise:
    """torch.randn / randn_like replaced for draws of ONE batch size by a prepared list (the job's own draws); every other draw -- the eager
    fallback's candidates -- comes from torch's generator."""

    def __init__(self, rows, arrays):
        self.rows, self.q, self.used = rows, [dev(a) for a in arrays], 0

    def __enter__(self):
        self._randn, self._randn_like = torch.randn, torch.randn_like

        def randn(*shape, **kw):
            shp = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape
            if shp[0] != self.rows:
                return self._randn(*shape, **kw)
            t = self.q[self.used]; self.used += 1
            assert tuple(t.shape) == shp
            return t.clone()

        torch.randn, torch.randn_like = randn, lambda x, **kw: randn(x.shape, device=x.device)
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self._randn, self._randn_like


def test_an_episode_without_a_free_candidate_falls_back_alone():
    """Two copies of the reference run's episode, max_iteration = 2.  Episode A's pursuer starts 0.15 from A's start, so after its first move
    its sphere (radius 0.1, 57 ring points 0.011 apart) passes through the pinned start state: the near-check adds those points to A's cost
    cloud and every candidate of A's first replan collides (threshold 0.05) -> record {0, -1, -1, 0}, and A re-plans from scratch on the eager
    path against its static cloud alone, like the one-episode planner.  That path installs A's scene; the job's table must be installed again
    and the plans handed over explicitly: episode B, untouched by all this, still takes the reference run's decisions."""
    g = np.load(f"{GOLDEN}/replan_chain.npz")
    K = 2; B0, H, S = g["noise"].shape[1:]
    dm = make_dynamic(4 * B0)
    log_b = []
    ctx_a, sphere_a, hard_a, cloud_a, rng_a = fixture_episode(g, None)
    ctx_b, sphere_b, hard_b, cloud_b, rng_b = fixture_episode(g, log_b)
    sphere_a.centers = torch.from_numpy(g["hard0"][:2] + np.float32([0.15, 0.0])).unsqueeze(0)
    dm.replan_log = []
    torch.manual_seed(3)
    with BatchNoise(2 * B0, [np.tile(n, (2, 1, 1)) for n in g["noise"]]) as inj:
        out = dm.run_inference_episodes([ctx_a, ctx_b], [hard_a, hard_b], [cloud_a, cloud_b], n_samples=B0, rngs=[rng_a, rng_b],
                                        return_chain=True, max_iteration=K)
    assert inj.used == 1 + K and dm.range_fallbacks == 0
    log_a = [en for en in dm.replan_log if en["episode"] == 0]
    assert len(log_a) == 1 + K
    assert log_a[1]["record"] == [0, -1, -1, 0] and not bool(log_a[1]["free"].any()), log_a[1]["record"]
    assert [en["npts"] for en in log_a[1:]] == [384 + 64] * K      # (the second replan may or may not find a free candidate: both paths are fine)
    (chain_a, obs_a, start_a), (chain_b, obs_b, start_b) = out
    assert chain_a.shape == chain_b.shape == (K + 1, 1, H, S) and bool(torch.isfinite(chain_a).all()) and bool(torch.isfinite(chain_b).all())
    cost_a = cloud_a.reshape(-1, 2)
    for plan in chain_a[1:, 0]:                              # what the fallback handed over: free of the static cloud, start / goal pinned
        assert float(torch.cdist(plan[:, :2], cost_a).min()) >= 0.05
        assert torch.equal(plan[0, :2].cpu(), torch.from_numpy(g["hard0"][:2])) and torch.equal(plan[-1].cpu(), torch.from_numpy(g["hardN"]))
    assert torch.equal(chain_a[2, 0, 1], chain_a[1, 0, 1])   # the state executed after replan 0 is pinned in replan 1's plan
    assert_selections_match_the_fixture(g, [en for en in dm.replan_log if en["episode"] == 1], 1 + K)
    for j, (t, st) in enumerate(log_b):
        assert t == int(g[f"env{j}/t"]) and float(np.abs(st - g[f"env{j}/state"]).max()) < 1e-5


def test_refusals_need_no_planning_run():
    g = np.load(f"{GOLDEN}/replan_chain.npz")
    dm = make_dynamic(16)
    ctxs = [{'dataset': make_fake_pursuit_env()[0]} for _ in range(2)]
    hard = {0: torch.from_numpy(g["hard0"]), 47: torch.from_numpy(g["hardN"])}
    cloud = dev(g["cloud"])
    with pytest.raises(ValueError, match="entries for 2 episodes"):
        dm.run_inference_episodes(ctxs, [hard], [cloud, cloud], n_samples=2)
    with pytest.raises(ValueError, match="entries for 2 episodes"):
        dm.run_inference_episodes(ctxs, [hard, hard], [cloud, cloud], n_samples=[2, 2, 2])
    with pytest.raises(ValueError, match="same waypoints"):
        dm.run_inference_episodes(ctxs, [hard, {0: hard[0], 24: hard[47]}], [cloud, cloud], n_samples=2)
    with pytest.raises(ValueError, match="max_rows"):
        dm.run_inference_episodes(ctxs, [hard, hard], [cloud, cloud], n_samples=6)      # 2 x 6 x 2 = 24 rows > 16
    with pytest.raises(NotImplementedError):                 # the static flow's many-scene entry stays closed to the dynamic planner
        dm.run_inference_scenes([cloud], [hard], n_samples=2)


def test_inference_dynamic_entry_runs_its_contexts_as_one_job(tmp_path):
    """examples/inference_dynamic.py --one-job: the script's own environment, context 0 three times as one many-episode job; every episode
    reports what a single run reports, in the same structure."""
    import examples.inference_dynamic as ex
    torch.manual_seed(5); np.random.seed(5)
    many, runner = ex.main(["--make-synthetic", str(tmp_path), "--n-samples", "8", "--max-replans", "2", "--one-job", "0,0,0"])
    assert len(many) == 3
    for m in many:
        assert m["n_replans"] == len(m["chain_obs"]) <= 2 and len(m["chain_start"]) == m["n_replans"] + 2
        assert np.allclose(m["chain_start"][0], [[-0.8, -0.8]])
