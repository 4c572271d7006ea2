"""Teams of robots in one job: the team guide kernel alone (``ramp_guide_step_team``), its cost terms (``ramp_guide_cost_team``), the exact
statements (no team is the cost guide, a team does not depend on the batch, a hand-computed step), the swept team check
(``ramp_team_clearance``), the wiring into ``ramp_sample_guided_team`` (bit-exact against the kernel applied to the unguided job's output),
free-running chains against float64, stale graphs, the selection of the best free team and the refusals.

The truth is the float64 numpy restatement of tests/team_ref.py; the same code in float32 is the yardstick: every bar that is not an exact
statement is 4 x the float32 restatement's distance from the float64 one on the test's own inputs, measured on the CPU (in team_ref, once
per case), never what the HIP code gives.  The kernels round the scalars to fp32 once; the tests hand over fp32-representable values."""
import ctypes as C

import numpy as np
import pytest
import torch

import team_ref as R
from ramp_amd import _lib, synth
from util import NoiseInjector, dev

pytestmark = pytest.mark.gpu

F32 = R.F32
ID = lambda c: "A%d_H%d_S%d_D%d_P%d_it%d_clip%d" % c      # noqa: E731


def run_step(x, A, clouds, ts, idx, val, k, step, n_iter, max_norm):
    from ramp_amd.team import team_guide_step
    hc = {h: dev(val[j]) for j, h in enumerate(idx)}
    y = team_guide_step(dev(x), [dev(c) for c in clouds], A, k["radius_team"], k["radius"], step, w_team=k["w_team"], w_obs=k["w_obs"],
                        w_smooth=k["w_smooth"], w_acc=k["w_acc"], n_steps=n_iter, max_norm=max_norm, hard_conds=hc,
                        traj_scene=None if ts is None else dev(ts))
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1: the step against float64
@pytest.mark.parametrize("case", R.STEP_CASES, ids=ID)
def test_step_against_float64(case):
    """Four teams of A (scenes 0, 1, 0 and one outside the table of two ragged uniform clouds), agents on a ring inside r_t = 0.3 around a
    rough common path, pins at both ends and mid-path with per-row values, weights (1, 1, 0.5, 0.25), step 2e-3, with the clip between the
    smallest and largest first gradient norm or without.  Bar: 4 x the float32 numpy restatement's largest distance from the float64 one on
    these inputs (measured on the CPU; test_team_host.py asserts the conditions: a pair inside r_t in every iteration, none below
    0.02 r_t, moved >= 100 bars).  The team outside the table, the pinned waypoints and the channels >= D keep their bits."""
    c, k = R.step_case(case), R.step_conditions(case)
    A, H, S, D, P, n_iter, clip = case
    assert k["d32"] > 0 and k["min_active"] > 0 and k["min_dist"] >= 0.02 * R.RADIUS_TEAM and k["moved"] >= 100 * k["bar"]
    y = run_step(c["x"], A, c["clouds"], c["ts"], c["idx"], c["val"], c["k"], R.STEP, n_iter, c["max_norm"])
    err = float(np.abs(y - c["y64"]).max())
    print(f"team step {case}: HIP {err:.2e}, float32 restatement {k['d32']:.2e} (bar {k['bar']:.2e}); moved {k['moved']:.2e}")
    xb, yb = c["x"].view(np.uint32), y.view(np.uint32)
    assert np.array_equal(yb[3 * A:], xb[3 * A:])                      # the team outside the table, as a whole
    assert np.array_equal(yb[:, c["idx"]], xb[:, c["idx"]])            # pinned waypoints
    assert np.array_equal(yb[:, :, D:], xb[:, :, D:])                  # channels >= D
    free = np.setdiff1d(np.arange(H), c["idx"])
    assert (yb[:3 * A][:, free, :D] != xb[:3 * A][:, free, :D]).mean() > 0.9
    assert err <= k["bar"]


# ------------------------------------------------------------------------------------------------ 2: the cost against float64
@pytest.mark.parametrize("case", [R.STEP_CASES[0], R.STEP_CASES[1], R.STEP_CASES[2], R.STEP_CASES[3]], ids=ID)
def test_cost_against_float64(case):
    """ramp_guide_cost_team on the step cases' rows as they are: column 3 against the float64 restatement under 4 x the float32 restatement's
    distance (relative to the row's value), columns 0 .. 2 ramp_guide_cost's bits, NaN rows for the team outside the table, and a team's
    C_team = half the sum of its rows' column 3."""
    from ramp_amd.guide import cost_guide_terms
    from ramp_amd.team import team_guide_terms
    c = R.step_case(case)
    A, H, S, D = case[:4]
    x, cl, ts = dev(c["x"]), [dev(v) for v in c["clouds"]], dev(c["ts"])
    got = team_guide_terms(x, cl, A, R.RADIUS_TEAM, R.RADIUS, traj_scene=ts).cpu().numpy()
    base = cost_guide_terms(x, cl, R.RADIUS, traj_scene=ts).cpu().numpy()
    assert got.shape == (4 * A, 4) and got.dtype == np.float64
    assert np.array_equal(got[:, :3].view(np.uint64), base.view(np.uint64))
    assert np.isnan(got[3 * A:]).all() and np.isfinite(got[:3 * A]).all()
    for t in range(3):
        P = c["x"][t * A:(t + 1) * A, :, :D]
        want, f32 = R.team_row_cost(P.astype(np.float64), R.RADIUS_TEAM), R.team_row_cost(P, R.RADIUS_TEAM)
        assert (want > 0).all()
        d32 = np.abs(f32 / want - 1).max()
        err = np.abs(got[t * A:(t + 1) * A, 3] / want - 1).max()
        print(f"team cost {case} team {t}: HIP {err:.2e}, float32 restatement {d32:.2e}")
        assert d32 > 0 and err <= 4 * d32
        tc = R.team_cost(P.astype(np.float64), R.RADIUS_TEAM)
        assert abs(got[t * A:(t + 1) * A, 3].sum() / 2 / tc - 1) <= 4 * d32
    # no table: teams of one, column 3 = 0, the other columns unchanged
    none = team_guide_terms(x, cl, None, 0.0, R.RADIUS, traj_scene=ts).cpu().numpy()
    assert np.array_equal(none[:3 * A, :3].view(np.uint64), base[:3 * A].view(np.uint64)) and (none[:3 * A, 3] == 0).all()


# ------------------------------------------------------------------------------------------------ 3: exact statements
@pytest.mark.parametrize("S,D", [(4, 2), (6, 3)])
def test_no_team_is_the_cost_guide_bit_for_bit(S, D):
    """team_size = 1, w_team = 0 and tg = NULL each give ramp_guide_step bit for bit, with a cloud past one tile, pins and the clip."""
    from ramp_amd.guide import cost_guide_step
    from ramp_amd.team import team_guide_step
    x = R.team_rows(3, 2, 47, S, D, 81)
    clouds = [dev(R.uniform((1100, D), 82)), dev(R.uniform((70, D), 83))]
    ts = dev(np.array([0, 0, 1, 1, 0, 0], np.int32))
    hc = {0: dev(R.uniform((6, S), 84)), -1: dev(R.uniform((6, S), 85))}
    kw = dict(w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=3, max_norm=F32(1.5), hard_conds=hc, traj_scene=ts)
    want = cost_guide_step(dev(x), clouds, R.RADIUS, R.STEP, **kw)
    assert not torch.equal(want, dev(x))
    for size, rt, wt in ((1, 0.3, 1.0), (2, 0.3, 0.0), (2, 0.0, 0.0), (None, 0.0, 0.0)):
        got = team_guide_step(dev(x), clouds, size, rt, R.RADIUS, R.STEP, w_team=wt, **kw)
        assert torch.equal(got, want), (size, rt, wt)
    on = team_guide_step(dev(x), clouds, 2, 0.3, R.RADIUS, R.STEP, w_team=1.0, **kw)
    assert not torch.equal(on, want)                                    # (and on is on)


@pytest.mark.parametrize("case", [R.STEP_CASES[1], R.STEP_CASES[7]], ids=ID)
def test_a_team_does_not_depend_on_the_batch(case):
    """Every team alone = inside the batch of four, bit for bit; n_iter iterations in one launch = n_iter launches of one."""
    c = R.step_case(case)
    A, H, S, D, P, n_iter, clip = case
    y = run_step(c["x"], A, c["clouds"], c["ts"], c["idx"], c["val"], c["k"], R.STEP, n_iter, c["max_norm"])
    for t in range(3):
        rows = slice(t * A, (t + 1) * A)
        alone = run_step(c["x"][rows], A, c["clouds"], c["ts"][rows], c["idx"], c["val"][:, rows], c["k"], R.STEP, n_iter, c["max_norm"])
        assert np.array_equal(alone.view(np.uint32), y[rows].view(np.uint32)), t
    z = c["x"]
    for _ in range(n_iter):
        z = run_step(z, A, c["clouds"], c["ts"], c["idx"], c["val"], c["k"], R.STEP, 1, c["max_norm"])
    assert np.array_equal(z.view(np.uint32), y.view(np.uint32))


def test_agents_of_a_team_in_different_scenes_read_their_own_clouds():
    """The hosts lay a team out in one scene; the kernel must still never read a stale cloud tile: teams whose agents alternate between two
    scenes with one-tile clouds of different spans (and one of equal size), against the float64 restatement under the 4 d32 bar."""
    A, H, S, D = 3, 8, 4, 2
    x = R.team_rows(2, A, H, S, D, 91)
    clouds = [R.uniform((70, D), 92), R.uniform((70, D), 93), R.uniform((300, D), 94)]
    ts = np.array([0, 1, 0, 2, 1, 2], np.int32)
    k = dict(R.WEIGHTS, radius=R.RADIUS, radius_team=R.RADIUS_TEAM)
    y64 = R.iterate(x, A, clouds, ts, {}, k, R.STEP, 3, 0.0, np.float64, D)
    y32 = R.iterate(x, A, clouds, ts, {}, k, R.STEP, 3, 0.0, np.float32, D)
    same = R.iterate(x, A, [clouds[0]] * 3, ts, {}, k, R.STEP, 3, 0.0, np.float64, D)
    d32 = float(np.abs(y32 - y64).max())
    assert d32 > 0 and np.abs(same - y64).max() >= 100 * 4 * d32          # a stale tile would show
    y = run_step(x, A, clouds, ts, [], np.zeros((0, 6, S), np.float32), k, R.STEP, 3, 0.0)
    err = float(np.abs(y - y64).max())
    print(f"mixed scenes: HIP {err:.2e}, float32 restatement {d32:.2e}")
    assert err <= 4 * d32


def test_two_agents_move_apart_by_the_hand_computed_amount():
    """Two agents at x = -0.1 and x = +0.1 on every waypoint, r_t = 0.3, step 0.01, w_team = 1 and nothing else, no clip: every free
    waypoint moves outwards by step * (r_t - d) / d * d_x in fp32, each operation rounded once -- the same bits."""
    f = np.float32
    x = np.zeros((2, 8, 4), f)
    x[0, :, 0], x[1, :, 0] = f(-0.1), f(0.1)
    x[:, :, 1] = f(0.25)
    rt, step = f(0.3), f(0.01)
    dx = f(-0.1) - f(0.1)
    d = np.sqrt(f(dx * dx) + f(0.0) * f(0.0))
    fac = f(f(rt - d) / d)
    g = f(f(0.0) - f(fac * dx))                      # agent 0: sum -= f dx
    new0 = f(f(-0.1) - f(step * g))
    assert new0 < f(-0.1) and abs(float(new0) - (-0.1 - 0.01 * 0.1 / 0.2 * 0.2)) < 1e-7
    from ramp_amd.team import team_guide_step
    y = team_guide_step(dev(x), dev(np.zeros((0, 2), f)), 2, float(rt), 0.0, float(step), w_team=1.0, w_obs=0.0).cpu().numpy()
    assert np.array_equal(y[0, :, 0].view(np.uint32), np.full(8, new0).view(np.uint32))
    assert np.array_equal(y[1, :, 0].view(np.uint32), np.full(8, -new0).view(np.uint32))
    assert np.array_equal(y[:, :, 1:].view(np.uint32), x[:, :, 1:].view(np.uint32))
    # at distance 0 the pair costs and does not push
    z = np.zeros((2, 8, 4), f)
    assert np.array_equal(team_guide_step(dev(z), dev(np.zeros((0, 2), f)), 2, float(rt), 0.0, float(step), w_obs=0.0).cpu().numpy(), z)


# ------------------------------------------------------------------------------------------------ 4: the team check
def run_clear(x, A, min_sep, D, **kw):
    from ramp_amd.team import team_clearance
    r = team_clearance(dev(x), A, min_sep, point_dim=D, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("case", R.CLEAR_CASES, ids=lambda c: "A%d_H%d_S%d_D%d_sep%g" % c)
def test_clearance_against_float64(case):
    """Three teams per case: separations under 4 x the float32 restatement's distance from the float64 one (an exact match is asked where the
    yardstick is zero: a minimum of correctly rounded values), counts exact (every float64 distance keeps a relative gap >= 1e-4 from
    min_sep; asserted in team_ref's case and test_team_host.py), sep_seg <= sep_wp."""
    A, H, S, D, min_sep = case
    c = R.clear_case(case)
    assert min(c["gap"]) >= 1e-4
    got = run_clear(c["x"], A, min_sep, D)
    for t in range(3):
        w64, s64, nw, ns = c["r64"][t]
        w32, s32 = c["r32"][t][:2]
        print(f"team clearance {case} team {t}: sep_wp HIP {abs(got['sep_wp'][t] - w64):.2e} (float32 {abs(w32 - w64):.2e}), "
              f"sep_seg HIP {abs(got['sep_seg'][t] - s64):.2e} (float32 {abs(s32 - s64):.2e}); conflicts {nw} / {ns}")
        assert abs(got["sep_wp"][t] - w64) <= 4 * abs(w32 - w64) or got["sep_wp"][t] == np.float32(w32)
        assert abs(got["sep_seg"][t] - s64) <= 4 * max(abs(s32 - s64), abs(w32 - w64)) or got["sep_seg"][t] == np.float32(s32)
        assert (got["wp_conflicts"][t], got["seg_conflicts"][t]) == (nw, ns)
        assert got["sep_seg"][t] <= got["sep_wp"][t]
        assert got["team_mask"][t] == int(ns > 0) and got["team_len"][t] == 0 and got["team_smooth"][t] == 0
    by_wp = run_clear(c["x"], A, min_sep, D, swept=False)
    assert np.array_equal(by_wp["team_mask"], (by_wp["wp_conflicts"] > 0).astype(np.int32))


def test_clearance_designed_cases():
    """Two agents that swap places through a point: sep_wp > min_sep while sep_seg < min_sep -- the swept check sees what the waypoints miss.
    Parallel motion (|e| = 0): every separation is the constant offset.  A NaN row: NaN separations, all counts at their maximum, never
    free.  Teams of one: +inf and zero counts.  The member sums in agent order."""
    x, m = R.swap_case()
    g = run_clear(x, 2, m, 2)
    assert g["sep_wp"][0] > m > g["sep_seg"][0] and (g["wp_conflicts"][0], g["seg_conflicts"][0]) == (0, 1)
    assert g["sep_wp"][0] == np.float32(R.clearance(x[:, :, :2], m)[0]) and g["team_mask"][0] == 1
    assert run_clear(x, 2, m, 2, swept=False)["team_mask"][0] == 0
    p, mp = R.parallel_case()
    g = run_clear(p, 2, mp, 2)
    assert g["sep_wp"][0] == g["sep_seg"][0] == np.float32(0.25) and (g["wp_conflicts"][0], g["seg_conflicts"][0], g["team_mask"][0]) == (0, 0, 0)
    both = np.concatenate([p, p, x]).copy()
    both[2, 3, 1] = np.nan
    ln, sm = R.uniform((6,), 7) + 2, R.uniform((6,), 8) + 2
    g = run_clear(both, 2, mp, 2, row_mask=np.array([0, 1, 0, 0, 0, 0]), row_len=ln, row_smooth=sm)
    assert np.isnan(g["sep_wp"][1]) and np.isnan(g["sep_seg"][1]) and (g["wp_conflicts"][1], g["seg_conflicts"][1]) == (8, 7)
    assert g["team_mask"].tolist() == [1, 1, 1]                          # a member's mask, the NaN row, the swap's conflict
    assert np.array_equal(g["team_len"], np.array([np.float32(0) + ln[0] + ln[1], np.float32(0) + ln[2] + ln[3], np.float32(0) + ln[4] + ln[5]]))
    assert np.array_equal(g["team_smooth"], np.array([sm[0] + sm[1], sm[2] + sm[3], sm[4] + sm[5]], np.float32))
    one = run_clear(both, 1, mp, 2)
    ok = [0, 1, 3, 4, 5]
    assert np.isinf(one["sep_wp"][ok]).all() and np.isinf(one["sep_seg"][ok]).all() and not one["wp_conflicts"].any() and not one["seg_conflicts"].any()
    assert np.isnan(one["sep_wp"][2]) and one["team_mask"].tolist() == [0, 0, 1, 0, 0, 0]
    # 3-D, three agents of which two swap along z
    x3 = np.zeros((3, 8, 6), np.float32)
    x3[0, :, 2], x3[1, :, 2] = x[0, :, 0], x[1, :, 0]
    x3[2, :, 0] = 0.5
    g = run_clear(x3, 3, m, 3)
    assert (g["wp_conflicts"][0], g["seg_conflicts"][0]) == (0, 1) and g["sep_wp"][0] > m > g["sep_seg"][0]


# ------------------------------------------------------------------------------------------------ 5: wiring, bit-exact
WIRE_STEP = F32(5e-3)
WIRE_MAX = F32(2.0)
WIRE_RT = F32(1.0)


def crossing_endpoints(S):
    """(starts (2, S), goals (2, S)) of two agents whose straight lines cross in the middle."""
    s, g = np.zeros((2, S), np.float32), np.zeros((2, S), np.float32)
    s[0, :2], g[0, :2] = (-0.8, -0.8), (0.8, 0.8)
    s[1, :2], g[1, :2] = (-0.8, 0.8), (0.8, -0.8)
    return s, g


def raw_team(size=2, radius=WIRE_RT, w=1.0):
    tg = _lib.RampTeamGuide()
    tg.team_size, tg.radius_team, tg.w_team = size, float(radius), float(w)
    return tg


@pytest.mark.parametrize("job,kind", [(j, k) for k in ("ddpm", "ddim") for j in ("plain", "scenes")])
def test_wiring_is_the_kernel_on_the_unguided_output(job, kind):
    """A one-iteration job, B = 4 (two teams of two with crossing per-row endpoints), injected noise whose step slot is zero: the team job's
    output equals ramp_guide_step_team applied to the unguided job's output, bit for bit.  DDPM at t = 12 and the last DDIM step, as a
    plain job and as a 2-scene job (one team per scene, different clouds).  The team term moved it by > 1e-3; tg = NULL, teams of one and
    w_team = 0 are ramp_sample_guided bit for bit, with the same number of launches."""
    import test_gpu_guide as G
    from ramp_amd.diffusion import _HostArrays
    from ramp_amd.guide import cost_guide_step
    from ramp_amd.team import team_guide_step, team_hard_conds
    lib = _lib.load()
    S, d, B, H = 4, 2, 4, 8
    ddim = kind == "ddim"
    dm = G.small_model(S, False, sampler=kind, use_graph=False)
    steps = [0] if ddim else [12]
    arrays = _HostArrays()
    noise = synth.make_noise((2, B, H, S), seed=90)
    noise[1] = 0
    noise = dev(noise)
    s0, g0 = crossing_endpoints(S)
    ctx, s = dm.model.ctx(), _lib.current_stream()
    dm.model.prepare_time_table(25)
    batch, ts = None, None
    if job == "scenes":
        hcs = [team_hard_conds(s0, g0, 1), team_hard_conds(s0 * 0.5, g0 * 0.5, 1)]
        hcs = [{0: h[0], H - 1: h[-1]} for h in hcs]
        sj, hc, Bc = dm._prepare_scene_job([dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))], hcs, [2, 2])
        assert Bc == B
        batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(sj["traj_scene"])
        ts = sj["traj_scene"]
        gclouds = [dev(G.uniform((70, d), 92)), dev(G.uniform((1100, d), 93))]
    else:
        t = team_hard_conds(s0, g0, 2)
        hc = {0: t[0].cuda(), H - 1: t[-1].cuda()}
        dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
        gclouds = [dev(G.uniform((300, d), 91))]
    p = G.raw_params(dm, B, steps, arrays, ddim, hard=hc, use_graph=0)
    cg = G.raw_guide(arrays, gclouds, [2], [WIRE_STEP], max_norm=WIRE_MAX)

    def run(guide, tg=None, entry="team"):
        out = torch.empty((B, H, S), device="cuda")
        if entry == "team":
            rc = lib.ramp_sample_guided_team(ctx, C.byref(p), C.byref(cg) if guide else None, C.byref(tg) if tg is not None else None, None, None,
                                             C.byref(batch) if batch is not None else None, _lib.ptr(noise), None, None, None, _lib.ptr(out), None, s)
        else:
            rc = lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg) if guide else None, None, None,
                                        C.byref(batch) if batch is not None else None, _lib.ptr(noise), None, None, None, _lib.ptr(out), None, s)
        _lib.check(rc, "job")
        torch.cuda.synchronize()
        return out, dm.model.launch_count()

    plain, _ = run(False)
    cloud_only, n_cloud = run(True, entry="guided")
    kw = dict(w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=WIRE_MAX, hard_conds=hc, traj_scene=ts)
    assert torch.equal(cloud_only, cost_guide_step(plain, gclouds, G.RADIUS, WIRE_STEP, **kw))
    for tg in (None, raw_team(size=1), raw_team(w=0.0), raw_team(w=0.0, radius=0.0)):
        off, n_off = run(True, tg)
        assert torch.equal(off, cloud_only) and n_off == n_cloud
    team, n_team = run(True, raw_team())
    want = team_guide_step(plain, gclouds, 2, WIRE_RT, G.RADIUS, WIRE_STEP, w_team=1.0, **kw)
    moved = float((want - cloud_only).abs().max())
    print(f"team wiring {job} {kind}: the team term moved the output by {moved:.2e}")
    assert moved > 1e-3 and np.isfinite(team.cpu().numpy()).all()
    assert torch.equal(team, want) and n_team == n_cloud


# ------------------------------------------------------------------------------------------------ 7: graph hygiene
def test_a_team_job_never_replays_a_stale_graph():
    """Jobs of one shape back to back on one context with use_graph = 1: another radius_team, another w_team, another team size, then other
    start / goal values with the same sizes -- each equals its own use_graph = 0 run bit for bit and differs from its predecessor."""
    import test_gpu_guide as G
    from ramp_amd.team import team_hard_conds
    B, H, S = 4, 8, 4
    noise = synth.make_noise((26, B, H, S), seed=5)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    cloud = dev(G.uniform((300, 2), 91))
    base = dict(cloud=cloud, radius=G.RADIUS, step=F32(4e-3), w_smooth=0.5, w_acc=0.25, n_steps=2, t_start=10, max_norm=F32(4.0))
    s0, g0 = crossing_endpoints(S)
    s4, g4 = np.concatenate([s0, s0 * 0.5]), np.concatenate([g0, g0 * 0.5])
    hc2 = team_hard_conds(s0, g0, 2)
    jobs = [(dict(base, team=dict(size=2, radius=F32(0.6))), hc2),
            (dict(base, team=dict(size=2, radius=F32(0.9))), hc2),
            (dict(base, team=dict(size=2, radius=F32(0.9), w=0.5)), hc2),
            (dict(base, team=dict(size=4, radius=F32(0.9), w=0.5)), hc2),
            (dict(base, team=dict(size=4, radius=F32(0.9), w=0.5)), team_hard_conds(s4, g4, 1))]

    def run(dm, g, hc):
        with NoiseInjector(list(noise)):
            return dm.run_inference(None, hc, n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene,
                                    noise_std_extra_schedule_fn=lambda x: 0.5, cost_guide=g)

    graph, eager = G.small_model(use_graph=True), G.small_model(use_graph=False)
    prev = None
    for g, hc in jobs:
        a, b = run(graph, g, hc), run(eager, g, hc)
        assert torch.equal(a, b)
        assert prev is None or not torch.equal(a, prev)
        prev = a
    assert torch.equal(run(graph, *jobs[-1]), prev)      # (and a replay of the same job is the same job)
    # the keyword off: the cloud guide's job, bit for bit
    no_team = {k: v for k, v in jobs[0][0].items() if k != "team"}
    assert torch.equal(run(graph, dict(no_team, team=dict(size=2, radius=F32(0.6), w=0.0)), hc2), run(eager, no_team, hc2))


# ------------------------------------------------------------------------------------------------ 8: selection
def selection_design():
    """Six teams of two in two scenes (rows 0 .. 5 | 6 .. 11), H = 8, S = 4, min_sep = 0.05.  Scene 0: teams 0 and 2 free, team 1 with a
    colliding member.  Scene 1: team 3 with a colliding member, teams 4 and 5 with a swap conflict the waypoints miss -- no free team.  The
    expected team-level arrays and selection, from the numpy rule."""
    sw, m = R.swap_case()
    x = np.concatenate([R.team_rows(4, 2, 8, 4, 2, 61, ring=0.3, jitter=0.02), sw, sw + np.float32(0.125)])
    row_mask = np.array([0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0], np.int32)
    row_len, row_smooth = R.uniform((12,), 62) + 2, R.uniform((12,), 63) + 2
    conflicts = [R.clearance(x[2 * t:2 * t + 2, :, :2].astype(np.float64), m)[3] for t in range(6)]
    mask = [int(row_mask[2 * t] or row_mask[2 * t + 1] or conflicts[t] > 0) for t in range(6)]
    tl = np.array([np.float32(row_len[2 * t]) + np.float32(row_len[2 * t + 1]) for t in range(6)], np.float32)
    tsm = np.array([np.float32(row_smooth[2 * t]) + np.float32(row_smooth[2 * t + 1]) for t in range(6)], np.float32)
    first = np.array([0, 3, 6], np.int32)
    return dict(x=x, min_sep=m, row_mask=row_mask, row_len=row_len, row_smooth=row_smooth, mask=mask, team_len=tl, team_smooth=tsm, first=first,
                want=R.select_teams(first, mask, tl, tsm, 0.1, 0.9))


def test_selection_of_the_best_free_team():
    from ramp_amd.cost import select_best_teams_scenes
    d = selection_design()
    assert d["mask"] == [0, 1, 0, 1, 1, 1]
    g = run_clear(d["x"], 2, d["min_sep"], 2, row_mask=d["row_mask"], row_len=d["row_len"], row_smooth=d["row_smooth"])
    assert g["team_mask"].tolist() == d["mask"] and np.array_equal(g["team_len"], d["team_len"]) and np.array_equal(g["team_smooth"], d["team_smooth"])
    x = dev(d["x"])
    best, res = select_best_teams_scenes(x, 2, d["first"], dev(g["team_mask"]), dev(g["team_len"]), dev(g["team_smooth"]), 0.1, 0.9)
    torch.cuda.synchronize()
    best, res = best.cpu().numpy(), res.cpu().numpy()
    assert best.shape == (2, 2, 8, 4)
    n_free, idx, team = d["want"][0]
    assert res[0].tolist() == [n_free, idx, team, 0] and n_free == 2 and team in (0, 2)
    assert np.array_equal(best[0].view(np.uint32), d["x"][2 * team:2 * team + 2].view(np.uint32))
    assert res[1].tolist() == [0, -1, -1, 0] and np.isnan(best[1]).all()
    # by waypoints alone the swaps pass: scene 1 then has free teams
    gw = run_clear(d["x"], 2, d["min_sep"], 2, swept=False, row_mask=d["row_mask"], row_len=d["row_len"], row_smooth=d["row_smooth"])
    _, res_w = select_best_teams_scenes(x.reshape(6, 2, 8, 4), 2, d["first"], dev(gw["team_mask"]), dev(gw["team_len"]), dev(gw["team_smooth"]))
    assert res_w.cpu().numpy()[1].tolist()[0] == 2


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_of_every_entry():
    """Every refusal is a host check made before anything launches: non-zero, the entry's name in ramp_last_error, the launch counter
    untouched, the output as it was."""
    import test_gpu_guide as G
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = G.small_model()
    B, H, S, steps = 4, 8, 4, [24, 12, 0]
    dm.model.prepare_time_table(25)
    dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
    arrays = _HostArrays()
    noise = dev(synth.make_noise((4, B, H, S), seed=8))
    p = G.raw_params(dm, B, steps, arrays, False)
    ctx, s = dm.model.ctx(), _lib.current_stream()
    out = torch.full((B, H, S), 7.0, device="cuda")
    gcloud = dev(G.uniform((50, 2), 91))
    cg = G.raw_guide(arrays, [gcloud], [1, 1, 1], [0.01] * 3)

    def untouched():
        torch.cuda.synchronize()
        return float(out.min()) == 7.0 and float(out.max()) == 7.0

    def job(tg, guide=cg):
        n0 = dm.model.launch_count()
        rc = lib.ramp_sample_guided_team(ctx, C.byref(p), C.byref(guide) if guide is not None else None, C.byref(tg), None, None, None, _lib.ptr(noise),
                                         None, None, None, _lib.ptr(out), None, s)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_sample_guided_team" in msg, (rc, msg)
        assert dm.model.launch_count() == n0 and untouched()
        return msg

    assert "cost guide" in job(raw_team(), guide=None)
    for n in (0, 9, -1):
        assert "team_size" in job(raw_team(size=n))
    assert "multiple of team_size" in job(raw_team(size=3))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "radius_team" in job(raw_team(radius=bad))
    for bad in (float("nan"), float("inf")):
        assert "w_team" in job(raw_team(w=bad))
    bad_cg = G.raw_guide(arrays, [gcloud], [1, 17, 1], [0.01] * 3)
    assert "n_guide" in job(raw_team(), guide=bad_cg)                     # what ramp_sample_guided refuses, with the new name
    p.noise_mode, p.philox_sample0, p.philox_total = 1, 1, 8
    assert "whole teams" in job(raw_team())
    p.noise_mode, p.philox_sample0, p.philox_total = 0, 0, 0

    def op(fn, *a):
        rc = fn(*a)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and untouched(), (rc, msg)
        return msg

    terms = torch.full((B, 4), 7.0, device="cuda", dtype=torch.float64)
    sep = torch.full((2,), 7.0, device="cuda")
    for tg, word in ((raw_team(size=3), "multiple"), (raw_team(size=9), "team_size"), (raw_team(radius=0.0), "radius_team"), (raw_team(w=float("nan")), "w_team")):
        assert word in op(lib.ramp_guide_step_team, _lib.ptr(out), B, H, S, C.byref(cg), C.byref(tg), None, 1, 0.01, 0, None, None, s)
        assert word in op(lib.ramp_guide_cost_team, _lib.ptr(out), B, H, S, C.byref(cg), C.byref(tg), None, _lib.ptr(terms), s)
    assert "ramp_guide_step_team" in op(lib.ramp_guide_step_team, _lib.ptr(out), B, H, S, None, C.byref(raw_team()), None, 1, 0.01, 0, None, None, s)
    for a in ((B, 1, S, 2, 2, 0.1), (B, H, S, 4, 2, 0.1), (B, H, S, 2, 3, 0.1), (B, H, S, 2, 2, -0.1), (B, H, S, 2, 2, float("nan"))):
        assert "ramp_team_clearance" in op(lib.ramp_team_clearance, _lib.ptr(out), *a, 1, None, None, None, _lib.ptr(sep), *([None] * 6), s)
    torch.cuda.synchronize()
    assert float(terms.min()) == 7.0 and float(sep.max()) == 7.0 and float(sep.min()) == 7.0


# ------------------------------------------------------------------------------------------------ 6: free-running chains against float64
# radius_team and step chosen on the CPU (team_ref / the oracle, never the HIP output) so that both conditions of the test hold: the float32
# oracle within a quarter of the bar (5.8e-5 / 1.5e-6 of 6.1e-5) and team-guided vs cloud-only-guided >= 100 bars apart (134 / 127)
CHAIN_GUIDE = dict(radius=R.RADIUS, step=F32(8e-3), w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=F32(4.0))
CHAIN_TEAM = dict(size=2, radius=F32(2.0), w=1.0)
_CHAIN = {}


def chain_hard_conds():
    """{0: (2, 4), 7: (2, 4)} numpy: one team of two whose straight lines cross (per-row endpoints, not the shared default ones)."""
    s, g = crossing_endpoints(4)
    return {0: s, 7: g}


def team_oracle_class():
    import test_gpu_guide as G

    class TeamOracle(G.GuideOracle):
        """GuideOracle with the team iteration of team_ref in the guide's place; ``guide`` carries ``team`` (or None: the cloud guide alone)."""

        def _guide(self, v, j, hard_conds):
            if self.guide is None or self.guide["tab"]["n_guide"][j] == 0:
                return v
            t, team = self.guide["tab"], self.guide.get("team")
            k = dict(radius=t["radius"], w_obs=t["w_obs"], w_smooth=t["w_smooth"], w_acc=t["w_acc"], radius_team=team["radius"] if team else 0.0,
                     w_team=team["w"] if team else 0.0)
            return R.iterate(v, team["size"] if team else 1, [self.guide["cloud"]], None, hard_conds, k, np.float32(t["step"][j]), t["n_guide"][j],
                             t["max_norm"], self.dt, 2)

    return TeamOracle


def oracle_chains(kind):
    """float64 team-guided and cloud-only-guided chains and the float32 team-guided chain, once per process (seconds on the CPU)."""
    if kind not in _CHAIN:
        import test_gpu_guide as G
        from oracle import ramp_oracle as O
        from ramp_amd.diffusion import guide_tables
        from ramp_amd.spec import UNET_DIM_MULTS
        from test_gpu_shapes import shape_weights
        T, noise, gcloud, scene = G.chain_inputs(kind)
        sched, steps, pv = G.chain_sched(T, kind)
        tab = guide_tables(dict(CHAIN_GUIDE, cloud=gcloud, t_start=steps[0], team=CHAIN_TEAM), steps, pv)
        assert tab["n_guide"] == [0] + [2] * (len(steps) - 1) and tab["team"]["size"] == 2
        cls = team_oracle_class()
        out = {}
        for name, dtype, team in (("t64", np.float64, True), ("c64", np.float64, False), ("t32", np.float32, True)):
            uo = O.UNetOracle(shape_weights(4, 8, False, 0, 16), 4, 8, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            so = cls(uo, T, 2.0, dtype=dtype, sched=sched, guide=dict(cloud=gcloud, tab=tab, team=tab["team"] if team else None))
            lat = uo.encode_scene(scene)
            out[name] = so.ddpm(noise, chain_hard_conds(), lat) if kind == "ddpm" else so.ddim(noise[0], chain_hard_conds(), lat, K=5)
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """(bar, float32 oracle's distance, team-guided vs cloud-only-guided distance of the final float64 states)."""
    c = oracle_chains(kind)
    bar = 1e-4 * float(np.abs(c["t64"]).max())
    return bar, float(np.abs(c["t32"] - c["t64"]).max()), float(np.abs(c["t64"][-1] - c["c64"][-1]).max())


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_team_chain(kind):
    """A 3-iteration DDPM job (T = 3, cosine schedule) and the 5-step DDIM job (T = 25) at the smallest network, one team of two (B = 2) with
    per-row endpoints whose straight lines cross, the team guide on from the second iteration with n_steps = 2, through
    run_inference(cost_guide=dict(..., team=)): every state against the float64 oracle chain at the project's standing bar, 1e-4 of max |x|.
    The inputs keep the float32 oracle within a quarter of that bar, and the float64 team-guided and cloud-only-guided final states differ
    by >= 100 x the bar (checked here and in test_team_host.py): the test cannot pass with the team term missing."""
    import test_gpu_guide as G
    c = oracle_chains(kind)
    bar, d32, moved = chain_conditions(kind)
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    T, noise, gcloud, scene = G.chain_inputs(kind)
    dm = G.small_model(T=T, sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential")
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    hc = {k: torch.from_numpy(v) for k, v in chain_hard_conds().items()}
    with NoiseInjector(list(noise)):
        chain = dm.run_inference(None, hc, n_samples=2, horizon=8, return_chain=True, obstacle_pts=dev(scene),
                                 noise_std_extra_schedule_fn=lambda x: 0.5,
                                 cost_guide=dict(CHAIN_GUIDE, cloud=dev(gcloud), t_start=steps[0], team=CHAIN_TEAM)).cpu().numpy()
    assert chain.shape == c["t64"].shape
    err = float(np.abs(chain - c["t64"]).max())
    print(f"team {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {d32:.2e}; team vs cloud-only {moved:.2e}); mode {dm.last_job_mode}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 10: the example
def test_static_example_plans_for_teams(tmp_path, capsys):
    """examples/inference_static.py --agents 2 --team-sep d on a synthetic experiment: one JSON line per scene with the free teams and the
    winner's swept separation for the job with the team term and for the job without it; the smallest swept separation over the scene's
    teams is larger with the term.  (Synthetic weights: no claim about plan quality.)"""
    import json
    import examples.inference_static as ex
    out, runner = ex.main(["--make-synthetic", str(tmp_path), "--n-samples", "6", "--sampler", "ddpm", "--n-diffusion-steps", "25",
                           "--n-steps-without-noise", "0", "--agents", "2", "--team-sep", "0.3"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(out) == len(lines) == 1 and lines[0]["agents"] == 2 and abs(lines[0]["team_radius"] - 0.45) < 1e-12
    m = out[0]
    on, off = m["with_team_term"], m["without_team_term"]
    print(f"example: with the team term {on}, without {off}")
    assert on["n_teams"] == off["n_teams"] == 6 and set(on) == {"n_teams", "free_teams", "winner", "winner_sep_seg", "min_sep_seg"}
    assert on["min_sep_seg"] > off["min_sep_seg"]
    assert runner.last_trajectories.shape == (6, 2, 48, 4) and m["best_team"].shape == (2, 48, 4)
    s, g = ex.StaticInference.team_endpoints(torch.tensor([-0.8, -0.8]), torch.tensor([0.8, 0.8]), 2)
    assert torch.allclose((s + g) / 2, torch.zeros(2, 2), atol=1e-6) and torch.allclose(s[1], torch.tensor([0.8, -0.8]), atol=1e-6)
    with pytest.raises(SystemExit):
        ex.main(["--make-synthetic", str(tmp_path), "--agents", "9"])
