"""The context-free planner kernels (sampler.hip, metrics.hip) through the C ABI, at the shapes, ties and thresholds where they can
break: the second cloud tile, the shuffle and tile tie-breaks, strided tails, grid-stride loops, windows of 0 and 64, H = 2 and
128, point counts that are no multiple of 64.  References and case tables: tests/planner_ref.py (tests/test_planner_ref_host.py
proves on the CPU that every designed tie is exact and every random case keeps its margins).

Out of scope: rows with non-finite waypoints in the costs and the selection -- the kernel's fminf / fmaxf drop a NaN where the
reference's min() / max() keep it, so the two legitimately differ there."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib
import planner_ref as R
from util import build_unet, dev, rel, weights

pytestmark = pytest.mark.gpu

APF_BAR = 5e-7


def S():
    return _lib.current_stream()


def cpu(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. ramp_apf
def call_apf(traj, cloud, thr, window, passes=1, strength=R.APF_STRENGTH, n_points=None):
    """ramp_apf on a copy of traj with the window weights of ramp_amd.apf; returns (rc, the array afterwards)."""
    from ramp_amd.apf import window_weights
    t, cl = dev(traj), dev(cloud)
    w = window_weights(window).contiguous()
    p = _lib.RampApfParams()
    p.cloud = _lib.ptr(cl); p.n_points = cloud.shape[0] if n_points is None else n_points
    p.window = window; p.window_weights_host = C.cast(w.data_ptr(), _lib.c_f32p)
    p.threshold = thr; p.strength = strength; p.passes = passes
    B, H, Sd = traj.shape
    rc = _lib.load().ramp_apf(_lib.ptr(t), B, H, Sd, C.byref(p), S())
    return rc, cpu(t)


@pytest.mark.parametrize("name", list(R.APF_RANDOM))
def test_apf_shapes(name):
    """H = 2 .. 128, S = 2 .. 16, P = 1 .. 2500 (one point, 63, and one past one and two tiles), windows 0, 64 and wider than
    H, two passes: max |diff| < 5e-7 against the oracle; columns >= 2 keep their bits.  With window 0 the reference's weight is
    0 / 0: the waypoints that are hit are NaN on both sides, and on no other."""
    c = R.apf_random_case(name)
    rc, out = call_apf(c["traj"], c["cloud"], c["thr"], c["window"], c["passes"])
    assert rc == 0
    err = R.maxdiff_nan_equal(out, c["ref"])
    print(f"apf {name}: max |diff| {err:.2e}, NaN {int(np.isnan(out).sum())}")
    assert err < APF_BAR
    assert np.array_equal(out[..., 2:], c["traj"][..., 2:])


@pytest.mark.parametrize("name", list(R.TIE_PAIRS))
def test_apf_nearest_point_ties(name):
    """Three points at exactly the same distance of one waypoint; the two of lowest index in the same lane, in different lanes, in
    the next tile, on both sides of the tile edge.  The lowest index wins: the push is along -x and y keeps its bits."""
    c = R.tie_case(name)
    ref = R.apf_ref(c["traj"], c["cloud"], c["thr"], R.APF_STRENGTH, c["window"])
    rc, out = call_apf(c["traj"], c["cloud"], c["thr"], c["window"])
    assert rc == 0
    assert out[0, R.TIE_H0, 0] < c["traj"][0, R.TIE_H0, 0] and np.array_equal(out[..., 1:], c["traj"][..., 1:])
    assert np.abs(out - ref).max() < APF_BAR


def test_apf_threshold_and_degenerate_cases():
    """d = thr exactly is a miss, thr one ulp larger a hit; a waypoint exactly on a point has direction 0 and stays."""
    for kind in ("miss", "hit", "on_point"):
        c = R.apf_threshold_case(kind)
        ref = R.apf_ref(c["traj"], c["cloud"], c["thr"], R.APF_STRENGTH, c["window"])
        rc, out = call_apf(c["traj"], c["cloud"], c["thr"], c["window"])
        assert rc == 0
        if kind == "hit":
            assert (out != c["traj"]).any() and np.abs(out - ref).max() < APF_BAR, kind
        else:
            assert np.array_equal(out, c["traj"]), kind
        assert np.array_equal(out[..., 2:], c["traj"][..., 2:])


def test_apf_refusals_leave_the_array_untouched():
    g = R.rng(1)
    cloud = g.uniform(-1, 1, size=(8, 2)).astype(np.float32)
    for H, window, n_points in ((129, 5, None), (48, 65, None), (48, 5, 0)):
        traj = g.uniform(-1, 1, size=(2, H, 2)).astype(np.float32)
        rc, out = call_apf(traj, cloud, 2.0, window, n_points=n_points)
        assert rc != 0 and np.array_equal(out, traj), (H, window, n_points)
    rc, out = call_apf(traj, cloud, 2.0, 5)                         # the same call, accepted, moves every waypoint
    assert rc == 0 and (out != traj).any(-1).all()


# ------------------------------------------------------------------------------------------------ 2. ramp_apf_dynamic
def call_dyn(traj, points, thr_query, thr_force, strength, window, affected=0, goal=None, enable=None):
    """ramp_apf_dynamic, called directly, on a copy of traj; window None = the pursuer pass (-1)."""
    t, p = dev(traj), dev(np.asarray(points, np.float64))
    gl = None if goal is None else dev(goal)
    en = None if enable is None else dev(np.asarray(enable, np.int32))
    B, H, Sd = traj.shape
    _lib.check(_lib.load().ramp_apf_dynamic(_lib.ptr(t), B, H, Sd, _lib.ptr(p), points.shape[0], thr_query, thr_force, strength,
                                            -1 if window is None else window, affected, _lib.ptr(gl), _lib.ptr(en), S()),
               "ramp_apf_dynamic")
    return cpu(t)


@pytest.mark.parametrize("name", list(R.DYN_STATIC))
def test_apf_dynamic_static_pass(name):
    """The static pass at P = 64 .. 3000 (1025 and 3000: a second and third tile), H = 8, 48, 128, windows 0, 3, 5 and wider than
    H, thr_query != thr_force; window 0 and a cloud out of reach leave every bit as it is."""
    c = R.dyn_static_case(name)
    out = call_dyn(c["traj"], c["points"], c["thr_query"], c["thr_force"], R.DYN_STRENGTH, c["window"])
    err = float(np.abs(out - c["ref"]).max())
    print(f"apf_dynamic {name}: max |diff| {err:.2e}")
    assert err < APF_BAR
    assert np.array_equal(out[..., 2:], c["traj"][..., 2:])
    if c["noop"]:
        assert np.array_equal(out, c["traj"])


@pytest.mark.parametrize("kind", ["last", "twin"])
def test_apf_dynamic_designed_static_cases(kind):
    """last: the closest waypoint is H - 1 and [ci - w, min(H - 1, ci + w)) leaves it where it is; twin: two waypoints are equally
    closest and the first is ci."""
    c = R.dyn_designed_case(kind)
    out = call_dyn(c["traj"], c["points"], c["thr_query"], c["thr_force"], R.DYN_STRENGTH, c["window"])
    assert np.abs(out - c["ref"]).max() < APF_BAR
    assert np.array_equal(out != c["traj"], c["ref"] != c["traj"])
    moved = (out[0] != c["traj"][0]).any(-1).tolist()
    assert moved == ([False] * 5 + [True, True, False] if kind == "last" else [False, False, True] + [False] * 5)


@pytest.mark.parametrize("P,affected,with_goal", R.DYN_PURSUER_CASES)
def test_apf_dynamic_pursuer_pass(P, affected, with_goal):
    """window = -1: affected = 0, 5, H and H + 10, with a goal (one waypoint equals its xy: goal direction 0) and without, and a
    cloud of 1025 points.  Waypoints from `affected` on keep their bits."""
    c = R.dyn_pursuer_case(P, affected, with_goal)
    out = call_dyn(c["traj"], c["points"], c["thr_query"], c["thr_force"], c["strength"], None, affected, goal=c["goal"])
    assert np.abs(out - c["ref"]).max() < APF_BAR
    nq = min(affected, c["H"])
    assert np.array_equal(out[:, nq:], c["traj"][:, nq:]) and np.array_equal(out[..., 2:], c["traj"][..., 2:])
    assert (out[:, :nq] != c["traj"][:, :nq]).any() == (nq > 0)


def test_apf_dynamic_enable_mask():
    """enable = [1, 0, 1, 0, 1]: disabled rows keep their bits, enabled rows have the bits of the same call on those rows alone."""
    c = R.dyn_enable_case()
    args = (c["points"], c["thr_query"], c["thr_force"], R.DYN_STRENGTH, c["window"])
    out = call_dyn(c["traj"], *args, enable=R.DYN_ENABLE)
    on = np.array(R.DYN_ENABLE, bool)
    assert np.array_equal(out[~on], c["traj"][~on])
    assert np.array_equal(out[on], call_dyn(np.ascontiguousarray(c["traj"][on]), *args))
    assert np.abs(out - c["ref"]).max() < APF_BAR and (out[on] != c["traj"][on]).any(axis=(1, 2)).all()


@pytest.mark.parametrize("name", list(R.TIE_PAIRS))
def test_apf_dynamic_nearest_point_ties(name):
    """The ties of test_apf_nearest_point_ties for this kernel's own copy of the search (float64 points, static pass)."""
    c = R.tie_case(name, "float64")
    ref = R.apf_dynamic_ref(c["traj"], c["cloud"], c["thr"], c["thr"], R.DYN_STRENGTH, c["window"])
    out = call_dyn(c["traj"], c["cloud"], c["thr"], c["thr"], R.DYN_STRENGTH, c["window"])
    assert out[0, R.TIE_H0, 0] < c["traj"][0, R.TIE_H0, 0] and np.array_equal(out[..., 1:], c["traj"][..., 1:])
    assert np.abs(out - ref).max() < APF_BAR


# ------------------------------------------------------------------------------------------------ 3. ramp_traj_costs
def call_costs(traj, cloud, thr):
    t, cl = dev(traj), dev(cloud)
    B, H, Sd = traj.shape
    mask = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    plen = torch.full((B,), float("nan"), device="cuda"); smooth = torch.full((B,), float("nan"), device="cuda")
    _lib.check(_lib.load().ramp_traj_costs(_lib.ptr(t), B, H, Sd, _lib.ptr(cl), cloud.shape[0], thr, _lib.ptr(mask), _lib.ptr(plen),
                                           _lib.ptr(smooth), S()), "ramp_traj_costs")
    return cpu(mask), cpu(plen), cpu(smooth)


def check_lengths(tag, got_plen, got_smooth, c, H):
    """Within (H + 4) 2^-24 relative of float64; exactly 0 where float64 is 0."""
    bar = R.cost_bar(H)
    for what, got, ref in (("path length", got_plen, c["plen"]), ("smoothness", got_smooth, c["smooth"])):
        zero = ref == 0
        err = float((np.abs(got.astype(np.float64) - ref)[~zero] / ref[~zero]).max()) if (~zero).any() else 0.0
        print(f"{tag} {what}: max rel {err:.2e} (bar {bar:.2e}), {int(zero.sum())} exact zeros")
        assert err <= bar and (got[zero] == 0).all(), (tag, what)


def check_costs(tag, c):
    mask, plen, smooth = call_costs(c["traj"], c["cloud"], c["thr"])
    assert set(mask.tolist()) <= {0, 1} and np.array_equal(mask.astype(bool), c["mask"]), tag
    check_lengths(tag, plen, smooth, c, c["H"])
    return mask


@pytest.mark.parametrize("name", list(R.COST_RANDOM))
def test_traj_costs_shapes(name):
    """H = 2 .. 128, S = 2 (smoothness exactly 0) .. 16, P = 1, 1023, 1025, 2500: the mask equals the float32 oracle's, lengths
    within the float32 bound of the float64 value."""
    check_costs(name, R.cost_random_case(name))


def test_traj_costs_designed_cases():
    """One colliding (waypoint, point) pair: the last point of the last tile, the first of the second tile with waypoint H - 1,
    point 0 with waypoint 0; a point at exactly thr is no collision, one float32 ulp more is."""
    for name in R.COST_DESIGNED:
        c = R.cost_designed_case(name)
        assert np.nonzero(check_costs(name, c))[0].tolist() == [c["row"]]
    assert not check_costs("at thr", R.cost_threshold_case(False)).any()
    assert np.nonzero(check_costs("one ulp over thr", R.cost_threshold_case(True)))[0].tolist() == [3]


# ------------------------------------------------------------------------------------------------ 4. selection
def call_select_from_costs(c):
    m, p, s = dev(c["mask"]), dev(c["plen"]), dev(c["smooth"])
    res = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_select_from_costs(_lib.ptr(m), _lib.ptr(p), _lib.ptr(s), c["B"], c["w_s"], c["w_l"], _lib.ptr(res), S()),
               "ramp_select_from_costs")
    return tuple(int(v) for v in res.cpu()[:3])


def call_select_best(c, traj, cloud, thr):
    t, cl = dev(traj), dev(cloud)
    B, H, Sd = traj.shape
    mask = torch.empty(B, dtype=torch.int32, device="cuda"); plen = torch.empty(B, device="cuda"); smooth = torch.empty(B, device="cuda")
    best = torch.full((H, Sd), 77.0, device="cuda"); res = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_select_best(_lib.ptr(t), B, H, Sd, _lib.ptr(cl), cloud.shape[0], thr, c["w_s"], c["w_l"], _lib.ptr(mask),
                                            _lib.ptr(plen), _lib.ptr(smooth), _lib.ptr(best), _lib.ptr(res), S()), "ramp_select_best")
    return tuple(int(v) for v in res.cpu()[:3]), cpu(best), (t, mask, plen, smooth)


def expect(c):
    return R.select_ref(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])


@pytest.mark.parametrize("name", list(R.SELECT_RANDOM))
def test_select_from_costs_batch_sizes(name):
    """B = 1, 2, 63, 1023, 1024, 1025, 3000 (up to three trips of the 1024-thread loop), random scalars and mask; the winner in
    the last row of B = 1025 and in row 1024 of B = 3000."""
    c = R.select_random_case(name)
    assert call_select_from_costs(c) == expect(c)


@pytest.mark.parametrize("name", list(R.SELECT_TIES))
def test_select_ties_go_to_the_lowest_row(name):
    """An exactly equal minimum total in two rows of one thread, of two lanes, of two waves, and with the lower row in the later
    wave: the lowest row wins."""
    c = R.select_tie_case(name)
    got = call_select_from_costs(c)
    assert got == expect(c) and got[2] == min(c["rows"])


@pytest.mark.parametrize("kind", R.SELECT_DEGENERATE)
def test_select_degenerate_batches(kind):
    """A zero range (all free rows equal, or equal in one of the two costs) makes every total 0 / 0 and the first free row wins,
    also when it is not row 0; one free row wins; no free row gives {0, -1, -1}."""
    c = R.select_degenerate_case(kind)
    assert call_select_from_costs(c) == expect(c)
    assert expect(c) == {"one_free": (1, 0, 1234), "none_free": (0, -1, -1)}.get(kind, (int((c["mask"] == 0).sum()), 0, 3))


def test_select_best_on_a_batch_with_exact_costs():
    """ramp_select_best on B = 2100 trajectories whose costs are a tie case's arrays exactly: the kernel's arrays equal them, the
    result is select_ref's and `best` is the winner with [0, 2:] = 0.  Without a free row: {0, -1, -1}, `best` keeps its contents
    and select_best_sharded returns None."""
    from ramp_amd import dist as rdist
    c = R.select_tie_case("other_wave")
    traj, cloud, thr = R.select_batch(c)
    got, best, (t, mask, plen, smooth) = call_select_best(c, traj, cloud, thr)
    free = c["mask"] == 0
    assert np.array_equal(cpu(mask), c["mask"])
    assert np.array_equal(cpu(plen)[free], c["plen"][free]) and np.array_equal(cpu(smooth)[free], c["smooth"][free])
    assert got == expect(c) and got[2] == min(c["rows"])
    want = traj[got[2]].copy(); want[0, 2:] = 0
    assert np.array_equal(best, want) and (traj[got[2], 0, 2:] != 0).all()
    sh, n_free, row = rdist.select_best_sharded(t, mask, plen, smooth, c["w_s"], c["w_l"])
    assert (n_free, row) == (got[0], got[2]) and np.array_equal(cpu(sh), want)
    traj, cloud, thr = R.select_batch(c, all_collide=True)
    got, best, (t, mask, plen, smooth) = call_select_best(c, traj, cloud, thr)
    assert got == (0, -1, -1) and cpu(mask).all() and (best == 77.0).all()
    assert rdist.select_best_sharded(t, mask, plen, smooth, c["w_s"], c["w_l"]) == (None, 0, -1)


# ------------------------------------------------------------------------------------------------ 5. metrics
@pytest.mark.parametrize("H", R.METRIC_H)
def test_traj_metrics_shapes(H):
    """H = 2, 48, 65, 128 (H > 64: the strided lane loop) x S = 2, 6 x 0, 1, 5 boxes, with waypoints exactly on a lower and an upper
    box face (inside): the intensity equals the oracle's, lengths keep the bound of ramp_traj_costs (FMA contraction and the lane /
    tree order of the sums stay inside it)."""
    lib = _lib.load()
    for Sd in R.METRIC_S:
        for n_boxes in R.METRIC_BOXES:
            c = R.metric_case(H, Sd, n_boxes)
            t = dev(c["traj"])
            ce, sz = (dev(c["centers"]), dev(c["sizes"])) if n_boxes else (None, None)
            out = [torch.full((R.METRIC_B,), float("nan"), device="cuda") for _ in range(3)]
            _lib.check(lib.ramp_traj_metrics(_lib.ptr(t), R.METRIC_B, H, Sd, _lib.ptr(ce), _lib.ptr(sz), n_boxes, _lib.ptr(out[0]),
                                             _lib.ptr(out[1]), _lib.ptr(out[2]), S()), "ramp_traj_metrics")
            tag = f"metrics H={H} S={Sd} boxes={n_boxes}"
            assert np.array_equal(cpu(out[0]), c["intensity"]), tag
            check_lengths(tag, cpu(out[1]), cpu(out[2]), c, H)


def call_variance(traj):
    B, H, Sd = traj.shape
    t = dev(traj)
    scratch = torch.empty(2 * H * ((B + 255) // 256), dtype=torch.float64, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    rc = _lib.load().ramp_waypoint_variance(_lib.ptr(t), B, H, Sd, _lib.ptr(scratch), _lib.ptr(out), S())
    return rc, float(out.cpu()[0])


@pytest.mark.parametrize("B", R.VARIANCE_B)
def test_waypoint_variance_at_the_tile_edges(B):
    """B = 2 and B around the 256-row tile (255, 256, 257, 513), H = 4, against the float64 oracle at 2e-6 relative."""
    c = R.variance_case(B)
    rc, got = call_variance(c["traj"])
    err = abs(got - c["ref"]) / c["ref"]
    print(f"waypoint variance B={B}: rel {err:.2e}")
    assert rc == 0 and err < 2e-6


def test_waypoint_variance_refuses_one_row():
    rc, got = call_variance(R.variance_case(2)["traj"][:1])
    assert rc != 0 and np.isnan(got)


# ------------------------------------------------------------------------------------------------ 6. elementwise steps
CANARY = -12345.0


def call_cfg(c, case, null=None, n_rp=None):
    x, e = dev(c["x"]), dev(c["eps"])
    outs = {k: torch.full(c["x"].shape, CANARY, device="cuda") for k in ("x0", "mean", "ecomb")}
    p = {k: (None if k == null else _lib.ptr(v)) for k, v in outs.items()}
    co = R.CFG_COEF
    rc = _lib.load().ramp_cfg_mean(_lib.ptr(x), _lib.ptr(e), case["B"], case["HS"], case["n_rp"] if n_rp is None else n_rp, R.CFG_W0,
                                   R.CFG_W1, co["sqrt_recip"], co["sqrt_recipm1"], co["coef1"], co["coef2"], case["clip"],
                                   case["predict_x0"], p["x0"], p["mean"], p["ecomb"], S())
    return rc, {k: cpu(v) for k, v in outs.items()}


@pytest.mark.parametrize("case", R.CFG_CASES, ids=lambda c: "rp{n_rp}_x0{predict_x0}_clip{clip}_B{B}".format(**c))
def test_cfg_mean_forms(case):
    """n_rp = 1, 2, 3 (w1 != 0) x predict_x0 x clip at HS = 6, and one batch just above 8192 * 256 elements (the grid-stride loop):
    bitwise the float32 restatement.  Each output NULL in turn: it is not written, the other two are written in full."""
    c = R.cfg_case(**case)
    for null in (None, "x0", "mean", "ecomb") if case["B"] < 1000 else (None,):
        rc, out = call_cfg(c, case, null)
        assert rc == 0
        for k in ("x0", "mean", "ecomb"):
            if k == null:
                assert (out[k] == CANARY).all(), (null, k)
            else:
                assert np.array_equal(out[k], c[k]), (null, k)


def test_cfg_mean_refuses_four_rows():
    case = dict(n_rp=3, predict_x0=0, clip=1, B=37, HS=R.CFG_HS)
    rc, out = call_cfg(R.cfg_case(**case), case, n_rp=4)
    assert rc != 0 and all((v == CANARY).all() for v in out.values())


@pytest.mark.parametrize("shape", R.DDIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("t", [24, 0])
def test_ddim_finish(shape, t):
    """B H S = 10, 960 and just above 8192 * 256, schedule values of a 25-step DDIM at t = 24 and t = 0: bitwise the float32
    restatement; x and x0 keep their bits.  The output differs from both inputs at t = 24; at t = 0 the previous alpha is 1, so
    the step is 1 x0 + 0 mo and the output is x0 itself."""
    g = R.rng(sum(shape) + t)
    x, x0 = g.standard_normal(shape, dtype=np.float32), np.clip(g.standard_normal(shape, dtype=np.float32), -1, 1)
    co = R.ddim_coefficients(t)
    ref = R.ddim_finish_ref(x, x0, *co)
    dx, dx0 = dev(x), dev(x0)
    out = torch.full(shape, CANARY, device="cuda")
    _lib.check(_lib.load().ramp_ddim_finish(_lib.ptr(dx), _lib.ptr(dx0), *co, _lib.ptr(out), *shape, S()), "ramp_ddim_finish")
    out = cpu(out)
    assert np.array_equal(out, ref)
    assert (out != x).any() and (out != x0).any() == (t != 0) and (out != CANARY).all()
    assert np.array_equal(cpu(dx), x) and np.array_equal(cpu(dx0), x0)


def call_hard_cond(x, idx, val):
    dx, dv = dev(x), dev(val)
    idx = np.ascontiguousarray(idx, np.int32)
    B, H, Sd = x.shape
    rc = _lib.load().ramp_hard_cond(_lib.ptr(dx), B, H, Sd, len(idx), idx.ctypes.data_as(_lib.c_i32p), _lib.ptr(dv), S())
    return rc, cpu(dx)


@pytest.mark.parametrize("n", R.HARD_N)
def test_hard_cond(n):
    """n = 1, 3 (an index twice), 256 (every index several times), per-row values (n, B, S): the last duplicate wins, every other
    element keeps its bits."""
    c = R.hard_cond_case(n)
    rc, out = call_hard_cond(c["x"], c["idx"], c["val"])
    assert rc == 0 and np.array_equal(out, c["ref"])
    rest = np.ones(48, bool); rest[c["idx"]] = False
    assert np.array_equal(out[:, rest], c["x"][:, rest])


def test_hard_cond_refusals_leave_x_untouched():
    c = R.hard_cond_case(3)
    for idx in ([0, 48, 1], [0, -1, 1]):
        rc, out = call_hard_cond(c["x"], idx, c["val"])
        assert rc != 0 and np.array_equal(out, c["x"]), idx
    idx = np.arange(257) % 48
    rc, out = call_hard_cond(c["x"], idx, R.rng(2).standard_normal((257, 5, 4), dtype=np.float32))
    assert rc != 0 and np.array_equal(out, c["x"])


# ------------------------------------------------------------------------------------------------ 7. time table
def test_time_table_at_every_timestep():
    """time_embedding(t) of a 100-step table (the dynamic model's schedule: the largest sin / cos arguments) against the float64
    oracle for every t, at the bar the fixtures' single t is held to; t = 100 is outside the table and refused."""
    m = build_unet(4, 48, False, max_rows=4)
    m.prepare_time_table(100)
    ref = O.UNetOracle(weights(4, 48, False), 4, 48, dtype=np.float64).time_embedding(np.arange(100))
    worst = 0.0
    for t in range(100):
        err = rel(cpu(m.time_embedding(t)), ref[t])
        worst = max(worst, err)
        assert err < 5e-6, (t, err)
    print(f"time table: worst rel {worst:.2e}")
    out = torch.full((32,), CANARY, device="cuda")
    rc = _lib.load().ramp_time_embedding(m.ctx(), 100, _lib.ptr(out), S())
    assert rc != 0 and (cpu(out) == CANARY).all()
