"""The references and case tables of tests/planner_ref.py, on the CPU: every reference reproduces the reference fixtures under
tests/golden at the bars those fixtures are already held to, and every case of the tables that tests/test_gpu_planner_kernels.py
runs meets the conditions that make a bitwise or 5e-7 comparison meaningful -- designed ties are exact ties in float64, designed
threshold cases are exactly representable, random cases keep their margins, and every case does something."""
import os

import numpy as np
import pytest

from oracle import ramp_oracle as O
import planner_ref as R

G = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


def check_margins(xy, pts, thr):
    """No nearest distance within THR_MARGIN of thr, no second-nearest point within TIE_MARGIN (relative) of the nearest."""
    d1, d2, _, n_tied = R.nearest_two(xy.reshape(-1, 2), pts)
    assert np.abs(d1 - thr).min() > R.THR_MARGIN
    assert (n_tied == 1).all() and ((d2 - d1) > R.TIE_MARGIN * d1).all()
    return d1


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", ["rand", "line", "nohit", "ends", "big"])
def test_apf_reference_reproduces_the_fixture(name):
    g = np.load(f"{G}/apf_cases.npz")
    thr, strength, win = g[name + "/params"]
    out = R.apf_ref(g[name + "/traj"], g[name + "/cloud"], float(thr), float(strength), int(win))
    assert np.abs(out - g[name + "/out"]).max() < 5e-7
    assert np.array_equal(out[..., 2:], g[name + "/traj"][..., 2:])
    if name == "nohit":
        assert np.array_equal(out, g[name + "/traj"])


def test_dynamic_apf_reference_reproduces_the_fixture():
    g = np.load(f"{G}/dynamic_cases.npz")
    thr_s, thr_p, st_s, st_p, w_s, _ = g["apf/params"]
    tr = g["apf/traj"]
    o1 = R.apf_dynamic_ref(tr, g["apf/static_points"], thr_s, thr_s, st_s, int(w_s))
    o2 = R.apf_dynamic_ref(tr, g["apf/dynamic_points"], thr_p, thr_s, st_p, None, affected=48, goal=g["apf/goal"])
    assert np.abs(o1 - g["apf/out_static"]).max() < 2e-7 and np.abs(o2 - g["apf/out_dynamic"]).max() < 2e-7
    en = [1, 0, 1, 0]
    o3 = R.apf_dynamic_ref(tr, g["apf/static_points"], thr_s, thr_s, st_s, int(w_s), enable=en)
    assert np.array_equal(o3[1::2], tr[1::2]) and np.array_equal(o3[0::2], o1[0::2])
    assert np.array_equal(R.apf_dynamic_ref(tr, g["apf/dynamic_points"], thr_p, thr_s, st_p, None, affected=0), tr)


def test_cost_and_selection_references_reproduce_the_fixture():
    g = np.load(f"{G}/cost_cases.npz")
    for thr in (0.02, 0.05, 0.1):
        mask, plen, smooth = R.costs_ref(g["trajs"], g["cloud"], thr)
        assert np.array_equal(mask, g[f"mask_{thr}"])
    assert rel(plen, g["path_length"]) < 1e-6 and rel(smooth, g["smoothness"]) < 1e-6
    mask = R.costs_ref(g["trajs"], g["cloud"], 0.05)[0]
    assert np.array_equal(~mask, g["free_mask"])
    for pl, sm in ((plen.astype(np.float32), smooth.astype(np.float32)), (g["path_length"], g["smoothness"])):
        n_free, rank, row = R.select_ref(mask, pl, sm, 0.1, 0.9)
        assert n_free == int(g["free_mask"].sum()) and rank == int(g["best_index"])
        assert row == int(np.nonzero(g["free_mask"])[0][rank])
        assert np.array_equal(g["trajs"][row], g["best"])
        assert rel(R.select_totals(mask, pl, sm, 0.1, 0.9), g["total_costs"]) < 1e-5


def test_metric_references_reproduce_the_fixture():
    g = np.load(f"{G}/metrics_cases.npz")
    tr = g["traj"]
    plen, smooth = R.lengths_ref(tr)
    assert np.array_equal(O.collision_intensity(tr, g["centers"], g["sizes"]), g["intensity"])
    assert np.abs(plen - g["path_length"]).max() < 2e-6
    assert np.abs(smooth - g["smoothness"]).max() < 2e-5
    assert abs(O.waypoint_variance(tr) - float(g["variance_all"])) < 1e-5 * float(g["variance_all"])


# ------------------------------------------------------------------------------------------------ static APF
@pytest.mark.parametrize("name", list(R.APF_RANDOM))
def test_apf_random_cases_keep_their_margins_and_move(name):
    c = R.apf_random_case(name)
    assert len(c["stages"]) == c["passes"] + 1
    for inp in c["stages"][:-1]:                                   # the input of every pass
        assert np.isfinite(inp).all() and np.abs(inp[..., :2]).max() <= 1.0 + 2 * R.APF_STRENGTH
        d1 = check_margins(inp[..., :2], c["cloud"], c["thr"])
        assert (d1 < c["thr"]).any()
    assert (c["ref"] != c["traj"]).any()                           # (a NaN counts as moved)
    assert np.array_equal(c["ref"][..., 2:], c["traj"][..., 2:])
    # window 0: the reference's weight is 0 / 0, so the waypoints that are hit, and only they, are NaN
    d1 = R.nearest_two(c["traj"][..., :2].reshape(-1, 2), c["cloud"])[0].reshape(c["traj"].shape[:2])
    assert np.array_equal(np.isnan(c["ref"][..., 0]), (d1 < c["thr"]) & (c["window"] == 0))


def check_tie(c, ref):
    """The designed tie of tie_case is exact in float64, it is the nearest distance of waypoint TIE_H0, no other waypoint is
    hit, and the reference takes the lowest index: a push along -x, y stays 0."""
    xy = c["traj"][0, :, :2]
    q = xy[R.TIE_H0].astype(np.float64)
    d2 = ((q[None] - c["cloud"].astype(np.float64)) ** 2).sum(-1)
    tied = np.nonzero(d2 == d2.min())[0]
    assert tied.tolist() == [c["i"], c["j"], R.TIE_P - 1] and d2.min() == 1 / 256 and np.sqrt(d2.min()) < c["thr"]
    assert np.sort(d2)[3] > 0.25                                   # the rest of the cloud is far away
    d1, _, idx, n_tied = R.nearest_two(xy, c["cloud"])
    others = np.arange(R.TIE_H) != R.TIE_H0
    assert idx[R.TIE_H0] == c["i"] and n_tied[R.TIE_H0] == 3 and (d1[others] > c["thr"] + R.THR_MARGIN).all()
    assert ref[0, R.TIE_H0, 0] < 0 and ref[0, R.TIE_H0, 1] == 0
    assert np.array_equal(ref[..., 2:], c["traj"][..., 2:])


@pytest.mark.parametrize("name", list(R.TIE_PAIRS))
def test_apf_ties_are_exact_and_the_winner_shows(name):
    c = R.tie_case(name)
    ref = R.apf_ref(c["traj"], c["cloud"], c["thr"], R.APF_STRENGTH, c["window"])
    check_tie(c, ref)
    swapped = c["cloud"].copy()
    swapped[[c["i"], c["j"]]] = swapped[[c["j"], c["i"]]]
    alt = R.apf_ref(c["traj"], swapped, c["thr"], R.APF_STRENGTH, c["window"])
    assert alt[0, R.TIE_H0, 1] < 0 and alt[0, R.TIE_H0, 0] == 0    # had the other point won, the push would be along -y
    # the same cloud as float64 points, for the dynamic kernel's own copy of the search (static pass around the only hit)
    c64 = R.tie_case(name, "float64")
    assert c64["cloud"].dtype == np.float64 and np.array_equal(c64["traj"], c["traj"])
    check_tie(c64, R.apf_dynamic_ref(c64["traj"], c64["cloud"], c64["thr"], c64["thr"], R.DYN_STRENGTH, c64["window"]))


@pytest.mark.parametrize("kind", ["miss", "hit", "on_point"])
def test_apf_threshold_cases_are_exactly_representable(kind):
    c = R.apf_threshold_case(kind)
    d1, d2, idx, _ = R.nearest_two(c["traj"][0, :, :2], c["cloud"])
    assert d1[3] == c["d"] and idx[3] == 7 and d2[3] > 0.5        # d is exact: sqrt(1/64) = 1/8, or 0
    assert (np.delete(d1, 3) > c["thr"] + R.THR_MARGIN).all()
    ref = R.apf_ref(c["traj"], c["cloud"], c["thr"], R.APF_STRENGTH, c["window"])
    if kind == "miss":
        assert c["thr"] == 1 / 8 == d1[3] and np.array_equal(ref, c["traj"])
    elif kind == "hit":
        assert c["thr"] > 1 / 8 and c["thr"] - 1 / 8 < 1e-16 and (ref[0, :, 0] != c["traj"][0, :, 0]).sum() == 5
    else:
        assert d1[3] < c["thr"] and np.array_equal(ref, c["traj"])    # hit with direction 0


# ------------------------------------------------------------------------------------------------ dynamic APF
def check_dyn_rows(traj, points, thr_query, nq):
    """Margins of the rows' first nq waypoints, and a closest waypoint that no other hit waypoint ties with."""
    for b in range(traj.shape[0]):
        if nq == 0:
            continue
        d1 = check_margins(traj[b, :nq, :2], points, thr_query)
        hits = np.sort(d1[d1 < thr_query])
        if len(hits) > 1:
            assert hits[1] - hits[0] > R.TIE_MARGIN * hits[0]


@pytest.mark.parametrize("name", list(R.DYN_STATIC))
def test_dynamic_static_cases_keep_their_margins_and_move(name):
    c = R.dyn_static_case(name)
    check_dyn_rows(c["traj"], c["points"], c["thr_query"], c["H"])
    moved = (c["ref"] != c["traj"]).any(axis=(1, 2))
    assert not moved.any() if c["noop"] else moved.all()
    assert np.array_equal(c["ref"][..., 2:], c["traj"][..., 2:])
    d1 = R.nearest_two(c["traj"][..., :2].reshape(-1, 2), c["points"])[0]
    assert (d1 < c["thr_query"]).any() == (name != "nohit")       # window 0 is a no-op although waypoints are hit


def test_dynamic_designed_cases():
    c = R.dyn_designed_case("last")
    d1 = check_margins(c["traj"][0, :, :2], c["points"], c["thr_query"])
    assert d1.argmin() == 7 and (d1 < c["thr_query"]).tolist() == [False] * 5 + [True] * 3
    moved = (c["ref"][0] != c["traj"][0]).any(-1)
    assert moved.tolist() == [False] * 5 + [True, True, False]    # [ci - w, min(H - 1, ci + w)): the closest one itself stays
    c = R.dyn_designed_case("twin")
    d1, _, _, n_tied = R.nearest_two(c["traj"][0, :, :2], c["points"])
    assert d1[2] == d1[6] == 1 / 16 and (np.delete(d1, [2, 6]) > c["thr_query"] + R.THR_MARGIN).all() and (n_tied == 1).all()
    moved = (c["ref"][0] != c["traj"][0]).any(-1)
    assert moved.tolist() == [False, False, True] + [False] * 5   # the first of the two is ci


@pytest.mark.parametrize("P,affected,with_goal", R.DYN_PURSUER_CASES)
def test_dynamic_pursuer_cases_keep_their_margins_and_move(P, affected, with_goal):
    c = R.dyn_pursuer_case(P, affected, with_goal)
    nq = min(affected, c["H"])
    check_dyn_rows(c["traj"], c["points"], c["thr_query"], nq)
    moved = (c["ref"] != c["traj"]).any(-1)
    assert not moved[:, nq:].any()
    assert moved[:, :nq].any(axis=1).all() if nq else not moved.any()
    assert np.array_equal(c["ref"][..., 2:], c["traj"][..., 2:])
    traj, _, goal = R.dyn_pursuer_inputs(P)
    assert np.array_equal(traj[1, 2, :2], goal[:2])                # the waypoint that equals the goal's xy ...
    if nq > 2:
        assert moved[1, 2]                                         # ... is pushed, with or without a goal
    if with_goal and nq:
        other = R.dyn_pursuer_case(P, affected, False)["ref"]
        assert (c["ref"] != other).any() and np.abs(c["ref"][1, 2] - other[1, 2]).max() < 1e-6      # goal direction 0: the blend only renormalises


def test_dynamic_enable_case():
    c = R.dyn_enable_case()
    check_dyn_rows(c["traj"], c["points"], c["thr_query"], c["H"])
    moved = (c["ref"] != c["traj"]).any(axis=(1, 2))
    assert moved.tolist() == [bool(e) for e in R.DYN_ENABLE]


# ------------------------------------------------------------------------------------------------ costs
@pytest.mark.parametrize("name", list(R.COST_RANDOM))
def test_cost_random_cases(name):
    c = R.cost_random_case(name)
    assert 0 < c["mask"].sum() < c["mask"].size                    # both values
    d1 = R.nearest_two(c["traj"][..., :2].reshape(-1, 2), c["cloud"])[0]
    assert np.abs(d1 - c["thr"]).min() > R.THR_MARGIN
    assert np.array_equal((d1.reshape(6, -1) < c["thr"]).any(1), c["mask"])
    assert (c["plen"] > 0).all() and ((c["smooth"] == 0).all() if c["S"] == 2 else (c["smooth"] > 0).all())


@pytest.mark.parametrize("name", list(R.COST_DESIGNED))
def test_cost_designed_cases_have_one_colliding_pair(name):
    c = R.cost_designed_case(name)
    xy = c["traj"][..., :2].astype(np.float64).reshape(-1, 1, 2)
    under = np.sqrt(((xy - c["cloud"].astype(np.float64)[None]) ** 2).sum(-1)) < c["thr"] + R.THR_MARGIN
    assert np.argwhere(under).tolist() == [[c["row"] * 48 + c["h"], c["p"]]]
    assert np.nonzero(c["mask"])[0].tolist() == [c["row"]]


def test_cost_threshold_cases_are_exactly_representable():
    miss, hit = R.cost_threshold_case(False), R.cost_threshold_case(True)
    d = np.sqrt(((miss["traj"][3, 20, :2] - miss["cloud"][1024]) ** 2).sum(dtype=np.float32))
    assert d.dtype == np.float32 and d == np.float32(miss["thr"]) == 0.125 and np.float32(hit["thr"]) == hit["thr"] > 0.125
    assert not miss["mask"].any() and np.nonzero(hit["mask"])[0].tolist() == [3]
    d1 = R.nearest_two(miss["traj"][..., :2].reshape(-1, 2), miss["cloud"])[0]
    assert np.sort(d1)[0] == 0.125 and (np.sort(d1)[1:] > 0.25).all()      # every other waypoint is far from every point


# ------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("name", list(R.SELECT_RANDOM))
def test_selection_random_cases_keep_their_margin(name):
    c = R.select_random_case(name)
    B = c["B"]
    assert c["mask"].shape == c["plen"].shape == c["smooth"].shape == (B,) and np.isfinite(c["plen"]).all() and np.isfinite(c["smooth"]).all()
    n_free, rank, row = R.select_ref(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])
    assert n_free == int((c["mask"] == 0).sum()) >= 1 and c["mask"][row] == 0 and rank == int((c["mask"][:row] == 0).sum())
    if B >= 63:
        assert 0 < c["mask"].sum() < B
    if B == 1:
        assert (n_free, rank, row) == (1, 0, 0)
        return
    t64 = R.select_totals(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"], dtype=np.float64)
    assert np.isfinite(t64).all() and np.diff(np.sort(t64)).min() > R.TOTAL_MARGIN
    assert int(np.nonzero(c["mask"] == 0)[0][t64.argmin()]) == row
    if c["winner"] is not None:
        assert row == c["winner"]


def test_selection_random_cases_cover_the_rows_the_issue_names():
    assert R.select_random_case("b1025_last")["winner"] == 1025 - 1 and R.select_random_case("b3000_r1024")["winner"] == 1024
    assert sorted(c["B"] for c in R.SELECT_RANDOM.values()) == [1, 2, 63, 1023, 1024, 1025, 3000, 3000]


@pytest.mark.parametrize("name", list(R.SELECT_TIES))
def test_selection_ties_are_exact(name):
    c = R.select_tie_case(name)
    r1, r2 = c["rows"]
    free = np.nonzero(c["mask"] == 0)[0]
    t32 = R.select_totals(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])
    t64 = R.select_totals(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"], dtype=np.float64)
    assert t32.dtype == np.float32 and np.array_equal(t32.astype(np.float64), t64)        # float32 arithmetic is exact here
    at = {int(r): float(t) for r, t in zip(free, t64)}
    assert at[r1] == at[r2] == 0.125 and min(t for r, t in at.items() if r not in (r1, r2)) >= 0.25
    assert (c["plen"][r1], c["smooth"][r1]) != (c["plen"][r2], c["smooth"][r2])
    assert R.select_ref(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])[2] == min(r1, r2)
    # placement: same thread (rows 1024 apart), other lane of one wave, other wave, the lower row in the later wave
    tid = (r1 % 1024, r2 % 1024)
    assert {"same_thread": tid[0] == tid[1], "other_lane": tid[0] // 64 == tid[1] // 64 and tid[0] != tid[1],
            "other_wave": tid[0] // 64 != tid[1] // 64, "lower_row_in_later_wave": tid[0] // 64 > tid[1] // 64}[name]


@pytest.mark.parametrize("kind", R.SELECT_DEGENERATE)
def test_selection_degenerate_cases(kind):
    c = R.select_degenerate_case(kind)
    got = R.select_ref(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])
    n_free = int((c["mask"] == 0).sum())
    if kind == "none_free":
        assert got == (0, -1, -1)
    elif kind == "one_free":
        assert got == (1, 0, 1234)
    else:
        assert n_free > 100 and got == (n_free, 0, 3)               # 0 / 0: the first free row, which is not row 0
        assert np.isnan(R.select_totals(c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"])).all()
        pl, sm = c["plen"][c["mask"] == 0], c["smooth"][c["mask"] == 0]
        assert (np.ptp(pl) == 0) == (kind != "smooth_equal") and (np.ptp(sm) == 0) == (kind != "plen_equal")
        assert np.ptp(c["plen"][:4]) > 0 and np.ptp(c["smooth"][:4]) > 0     # the colliding rows in front carry other values


def test_selection_batch_reproduces_its_arrays():
    """The trajectory batch ramp_select_best runs on has exactly the case's costs, in float32 and in float64."""
    c = R.select_tie_case("other_wave")
    traj, cloud, thr = R.select_batch(c)
    mask, plen, smooth = R.costs_ref(traj, cloud, thr)
    free = c["mask"] == 0
    assert np.array_equal(mask, ~free) and 0 < free.sum() < c["B"]
    assert np.array_equal(plen[free], c["plen"][free].astype(np.float64)) and np.array_equal(smooth[free], c["smooth"][free].astype(np.float64))
    assert np.array_equal(O.path_length(traj)[free], c["plen"][free]) and np.array_equal(O.smoothness(traj)[free], c["smooth"][free])
    assert (traj[:, 0, 2:] != 0).all()                              # so that best[0, 2:] = 0 shows
    assert R.costs_ref(*R.select_batch(c, all_collide=True))[0].all()


# ------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("H", R.METRIC_H)
@pytest.mark.parametrize("S", R.METRIC_S)
@pytest.mark.parametrize("n_boxes", R.METRIC_BOXES)
def test_metric_cases(H, S, n_boxes):
    c = R.metric_case(H, S, n_boxes)
    for a in (c["traj"], c["centers"], c["sizes"]):
        assert a.dtype == np.float32
    lo, hi = c["centers"] - c["sizes"] / 2, c["centers"] + c["sizes"] / 2
    assert np.array_equal(lo.astype(np.float64), c["centers"].astype(np.float64) - c["sizes"].astype(np.float64) / 2)   # exact faces
    assert (c["intensity"] == 0).all() if n_boxes == 0 else (c["intensity"][:3] > 0).all()
    assert len(c["planted"]) == (3 if n_boxes else 0)
    for b, h, axis, sign in c["planted"]:
        face = (hi if sign > 0 else lo)[0, axis]
        assert c["traj"][b, h, axis] == face
        out = c["traj"].copy()                                     # one ulp outwards and the waypoint no longer counts
        out[b, h, axis] = np.nextafter(face, np.float32(sign * 2))
        assert O.collision_intensity(out, c["centers"], c["sizes"])[b] == np.float32((c["intensity"][b] * H - 1) / H)
    assert (c["plen"] > 0).all() and ((c["smooth"] == 0).all() if S == 2 else (c["smooth"] > 0).all())


def test_variance_cases():
    assert R.VARIANCE_B == (2, 255, 256, 257, 513)
    for B in R.VARIANCE_B:
        c = R.variance_case(B)
        assert c["traj"].shape == (B, 4, 4) and c["ref"] > 0


# ------------------------------------------------------------------------------------------------ elementwise steps
@pytest.mark.parametrize("case", R.CFG_CASES, ids=lambda c: "rp{n_rp}_x0{predict_x0}_clip{clip}_B{B}".format(**c))
def test_cfg_cases(case):
    c = R.cfg_case(**case)
    n = case["B"] * case["HS"]
    assert case["HS"] % 4 != 0 and c["x0"].shape == (case["B"], case["HS"])
    assert (n > 8192 * 256 and n - 8192 * 256 < 256) or n < 8192 * 256
    if case["clip"]:
        assert (np.abs(c["x0"]) == 1).sum() > 10 and (np.abs(c["x0"]) < 1).sum() > 10       # the clamp bites, and not everywhere
    else:
        assert np.abs(c["x0"]).max() > 1
    args = dict(case); args.pop("B"); args.pop("HS")
    if case["n_rp"] == 3:                                          # both weights count
        for w0, w1 in ((R.CFG_W0, 0.0), (0.0, R.CFG_W1)):
            assert (R.cfg_mean_ref(c["x"], c["eps"], 3, w0, w1, clip=0, predict_x0=1, **R.CFG_COEF)[0] != c["ecomb"]).any()
    assert (c["mean"] != c["x0"]).any() and (c["ecomb"] != c["eps"][:, -1]).any() == (case["n_rp"] > 1)
    assert (c["x0"] is c["ecomb"]) == bool(case["predict_x0"] and not case["clip"])


def test_ddim_and_hard_cond_cases():
    for t in (24, 0):
        co = R.ddim_coefficients(t)
        assert np.isfinite(co).all() and co[1] > 0 and all(np.float32(v) == v for v in co)
    assert R.ddim_coefficients(0)[2:] == (1.0, 0.0) and R.ddim_coefficients(24)[3] > 0.5
    assert [b * h * s for b, h, s in R.DDIM_SHAPES][:2] == [10, 5 * 48 * 4] and 0 < np.prod(R.DDIM_SHAPES[2]) - 8192 * 256 < 256
    for n in R.HARD_N:
        c = R.hard_cond_case(n)
        hit = np.zeros(48, bool); hit[c["idx"]] = True
        assert np.array_equal(c["ref"][:, ~hit], c["x"][:, ~hit]) and (c["ref"][:, hit] != c["x"][:, hit]).all()
        last = {int(h): k for k, h in enumerate(c["idx"])}
        for h, k in last.items():
            assert np.array_equal(c["ref"][:, h], c["val"][k])
        assert (len(last) < n) == (n > 1)                          # n = 3 and n = 256 repeat indices
    c = R.hard_cond_case(3)
    assert c["idx"].tolist() == [0, 17, 0] and not np.array_equal(c["val"][0], c["val"][2])
