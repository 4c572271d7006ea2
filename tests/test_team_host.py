"""Teams of robots in one job, host side: the numpy restatement of tests/team_ref.py against finite differences and dense sampling, the
conditions the GPU tests ask of their inputs, ``team_hard_conds`` layouts, struct layout, the declared / bound / exported symbols and every
refusal that needs no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import team_ref as R
from ramp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("A,H,D", [(2, 8, 2), (3, 5, 3), (8, 6, 3)])
def test_team_grad_is_the_gradient_of_team_cost(A, H, D):
    """team_grad in float64 against central differences of team_cost (h = 1e-6) at positions with pairs inside and outside r_t and none at
    the kink d = r_t or at d = 0: 1e-6 relative to the largest gradient entry."""
    P = R.team_rows(1, A, H, D, D, 77 + A, ring=0.12, jitter=0.06)[:, :, :D].astype(np.float64)
    r = 0.25
    d = R.pair_distances(P)
    assert (d < r).any() and (d > r).any() and np.abs(d - r).min() > 1e-4 and d.min() > 1e-3
    g = R.team_grad(P, r)
    num = np.zeros_like(P)
    h = 1e-6
    for i in np.ndindex(*P.shape):
        Pp, Pm = P.copy(), P.copy()
        Pp[i] += h
        Pm[i] -= h
        num[i] = (R.team_cost(Pp, r) - R.team_cost(Pm, r)) / (2 * h)
    assert np.abs(g).max() > 0.01
    assert np.abs(g - num).max() <= 1e-6 * np.abs(g).max()
    # a team's C_team is half the sum of its rows' shares; a pair at distance 0 costs and does not push
    assert abs(R.team_row_cost(P, r).sum() / 2 - R.team_cost(P, r)) <= 1e-12 * R.team_cost(P, r)
    Z = np.zeros((2, 3, D))
    assert R.team_cost(Z, r) == 3 * 0.5 * r * r and not R.team_grad(Z, r).any()


def test_closed_form_closest_approach_against_dense_samples():
    """The closed-form segment distance of every pair against 2001 samples per segment of the two synchronous motions: never above the
    sampled minimum, and within the grid's resolution of it (half a grid step times the relative speed |e|)."""
    rng = np.random.default_rng(5)
    P = rng.uniform(-1, 1, size=(4, 9, 3))
    P[3] = P[2] + np.array([0.3, 0.0, 0.0])                     # a pair in parallel motion: |e| = 0
    ds = R.segment_distances(P)
    t = np.linspace(0.0, 1.0, 2001)
    k = 0
    for a in range(4):
        for o in range(a + 1, 4):
            dd = P[a] - P[o]
            for h in range(8):
                e = dd[h + 1] - dd[h]
                dense = np.sqrt(((dd[h][None] + t[:, None] * e[None]) ** 2).sum(1)).min()
                assert ds[k, h] <= dense * (1 + 1e-15) + 1e-300
                assert dense - ds[k, h] <= 0.5 * (t[1] - t[0]) * np.sqrt((e ** 2).sum()) + 1e-15
            k += 1
    assert np.abs(ds[5] - 0.3).max() < 1e-12
    dw = R.pair_distances(P)
    assert (ds <= np.minimum(dw[:, :-1], dw[:, 1:])).all()      # sep_seg <= sep_wp always


def test_designed_clearance_cases():
    x, m = R.swap_case()
    w, s, nw, ns = R.clearance(x[:, :, :2].astype(np.float64), m)
    assert w > m > s and nw == 0 and ns == 1 and abs(w - 0.1) < 1e-6 and s < 1e-6
    x, m = R.parallel_case()
    assert R.clearance(x[:, :, :2], m) == (0.25, 0.25, 0, 0)
    bad = x.copy()
    bad[1, 3, 1] = np.nan
    w, s, nw, ns = R.clearance(bad[:, :, :2], m)
    assert np.isnan(w) and np.isnan(s) and (nw, ns) == (8, 7)
    assert R.clearance(x[:1, :, :2], m) == (float("inf"), float("inf"), 0, 0)


# ------------------------------------------------------------------------------------------------ what the GPU inputs must satisfy
def test_the_lists_of_the_issue_are_covered():
    v = list(zip(*R.STEP_CASES))
    assert set(v[0]) == {2, 3, 8} and set(v[1]) == {8, 47, 128} and set(zip(v[2], v[3])) == {(4, 2), (6, 3)}
    assert set(v[4]) == {0, 70, 1100} and set(v[5]) == {1, 3} and set(v[6]) == {True, False}
    assert (8, 128, 6, 3) in {c[:4] for c in R.STEP_CASES}      # the LDS maximum


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: "A%d_H%d_S%d_D%d_P%d_it%d_clip%d" % c)
def test_step_inputs_satisfy_their_conditions(case):
    """What tests/test_gpu_team.py asks of its step inputs, on the float64 restatement: some pair inside r_t in every iteration of every
    team, no pair distance ever below 0.02 r_t, the state moved by at least 100 bars, the yardstick is no zero; with the clip one agent is
    clipped and another is not; the team outside the table, the pinned waypoints and the channels >= D stay."""
    c, k = R.step_case(case), R.step_conditions(case)
    A, H, S, D, P, n_iter, clip = case
    print(f"{case}: bar {k['bar']:.2e}, moved {k['moved']:.2e}, smallest pair distance {k['min_dist']:.3f} (r_t {R.RADIUS_TEAM}), "
          f"fewest pairs inside r_t {k['min_active']}")
    assert k["d32"] > 0 and k["min_active"] > 0 and k["min_dist"] >= 0.02 * R.RADIUS_TEAM and k["moved"] >= 100 * k["bar"]
    if clip:
        assert min(k["s_first"]) < 1.0 and max(k["s_first"]) == 1.0
    for y in (c["y64"], c["y32"]):
        assert np.array_equal(y[3 * A:], c["x"][3 * A:].astype(y.dtype))
        assert np.array_equal(y[:, c["idx"]], c["x"][:, c["idx"]].astype(y.dtype)) and np.array_equal(y[:, :, D:], c["x"][:, :, D:].astype(y.dtype))
    # the team term is what moved it: without it the float64 result lies at least 100 bars away
    off = R.iterate(c["x"], A, c["clouds"], c["ts"], c["pins"], dict(c["k"], w_team=0.0), R.STEP, n_iter, c["max_norm"], np.float64, D)
    assert np.abs(off - c["y64"]).max() >= 100 * k["bar"]


@pytest.mark.parametrize("case", R.CLEAR_CASES, ids=lambda c: "A%d_H%d_S%d_D%d_sep%g" % c)
def test_clearance_inputs_satisfy_their_conditions(case):
    """Every float64 distance keeps a relative gap >= 1e-4 from min_sep (so the counts are exact), and min_sep separates: some team has
    conflicts, and not every item conflicts."""
    c = R.clear_case(case)
    A, H = case[0], case[1]
    assert min(c["gap"]) >= 1e-4
    assert [r[2:] for r in c["r32"]] == [r[2:] for r in c["r64"]]
    n_pairs = A * (A - 1) // 2
    assert any(r[3] > 0 for r in c["r64"]) and all(r[2] < n_pairs * H for r in c["r64"])


def test_wiring_and_selection_inputs():
    """The crossing endpoints of the wiring and chain tests do cross, and the selection's designed arrays have a scene without a free team."""
    import test_gpu_team as T
    s, g = T.crossing_endpoints(4)
    a0, a1 = (s[0, :2], g[0, :2]), (s[1, :2], g[1, :2])
    # the straight lines cross at their midpoints
    assert np.allclose((a0[0] + a0[1]) / 2, (a1[0] + a1[1]) / 2)
    d = T.selection_design()
    assert d["want"][1] == (0, -1, -1) and d["want"][0][0] >= 2


def test_free_running_chain_inputs_satisfy_their_conditions():
    """What tests/test_gpu_team.py::test_free_running_team_chain asks of its inputs, checked on the CPU: the float32 oracle stays within a
    quarter of the bar (1e-4 of max |x|) and the float64 team-guided and cloud-only-guided final states lie at least 100 bars apart."""
    import test_gpu_team as T
    for kind in ("ddpm", "ddim"):
        bar, d32, moved = T.chain_conditions(kind)
        print(f"{kind}: bar {bar:.3e}, float32 oracle {d32:.3e}, team vs cloud-only {moved:.3e}")
        assert d32 <= bar / 4 and moved >= 100 * bar


# ------------------------------------------------------------------------------------------------ the Python layer
def test_team_hard_conds_layouts():
    from ramp_amd.team import team_hard_conds
    s = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    g = -s
    hc = team_hard_conds(s, g, 2)
    assert set(hc) == {0, -1} and hc[0].shape == (6, 4) and hc[0].is_contiguous()
    for k in range(2):
        for a in range(3):
            assert torch.equal(hc[0][k * 3 + a], s[a]) and torch.equal(hc[-1][k * 3 + a], g[a])
    assert team_hard_conds(s.numpy(), g.numpy(), 1)[0].dtype == torch.float32
    for bad in (lambda: team_hard_conds(s, g[:2], 1), lambda: team_hard_conds(s[0], g[0], 1), lambda: team_hard_conds(s, g, 0),
                lambda: team_hard_conds(torch.zeros(9, 4), torch.zeros(9, 4), 1)):
        with pytest.raises(ValueError):
            bad()


def make(T=25, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    kw.setdefault("predict_epsilon", True)
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=48, state_dim=4), n_diffusion_steps=T, **kw)


TEAM = dict(size=2, radius=0.3, w=1.0)
GUIDE = dict(cloud=torch.zeros(4, 2), radius=0.3, step=0.01, team=TEAM)


def test_guide_tables_take_the_team_key():
    from ramp_amd.diffusion import guide_tables
    from ramp_amd.team import fill_team_guide
    dm = make(sampler="ddpm")
    steps = dm._ddpm_steps()[0]
    tab = guide_tables(GUIDE, steps, dm.posterior_variance)
    assert tab["team"] == dict(size=2, radius=0.3, w=1.0)
    assert guide_tables(dict(GUIDE, team=dict(size=3, radius=0.2)), steps, dm.posterior_variance)["team"]["w"] == 1.0
    assert "team" not in guide_tables({k: v for k, v in GUIDE.items() if k != "team"}, steps, dm.posterior_variance)
    tg = fill_team_guide(tab["team"])
    assert (tg.team_size, tg.radius_team, tg.w_team) == (2, 0.3, 1.0)


@pytest.mark.parametrize("team, exc, msg", [
    (dict(radius=0.3), ValueError, "size= is required"),
    (dict(size=0, radius=0.3), ValueError, "size must be"),
    (dict(size=9, radius=0.3), ValueError, "size must be"),
    (dict(size=2.5, radius=0.3), ValueError, "size must be"),
    (dict(size=2), ValueError, "radius must be positive"),
    (dict(size=2, radius=-0.1), ValueError, "radius must be positive"),
    (dict(size=2, radius=float("nan")), ValueError, "radius must be positive"),
    (dict(size=2, radius=float("inf")), ValueError, "radius must be positive"),
    (dict(size=2, radius=0.3, w=float("nan")), ValueError, "w must be finite"),
    (dict(size=2, radius=0.3, weight=1.0), ValueError, "unknown keys"),
    ((2, 0.3), TypeError, "takes a dict"),
])
def test_bad_team_keys_are_refused_with_a_message(team, exc, msg):
    from ramp_amd.diffusion import guide_tables
    dm = make(sampler="ddpm")
    with pytest.raises(exc, match=msg):
        guide_tables(dict(GUIDE, team=team), dm._ddpm_steps()[0], dm.posterior_variance)


def test_python_refusals_before_anything_touches_a_device():
    """team= with boxes= / spheres=, resample=, stitched windows, a caller's sample_fn and the dynamic model raise NotImplementedError with a
    one-line reason; rows that are no multiple of the team size raise ValueError; all before any device call (the models here have none)."""
    dm = make(sampler="ddpm")
    box = (torch.zeros(1, 2), torch.full((1, 2), 0.4))
    with pytest.raises(NotImplementedError, match="boxes= / spheres="):
        dm.conditional_sample({}, batch_size=2, cost_guide=dict(GUIDE, boxes=box, band=0.02))
    with pytest.raises(NotImplementedError, match="resample="):
        dm.conditional_sample({}, batch_size=2, cost_guide=GUIDE, resample=dict(every=1, lambda_=1.0, cloud=torch.zeros(4, 2), radius=0.3))
    with pytest.raises(NotImplementedError, match="stitched"):
        dm.conditional_sample({}, batch_size=2, cost_guide=GUIDE, stitch=dict(n_windows=2))
    with pytest.raises(NotImplementedError, match="run_inference_stitched"):
        dm.run_inference_stitched(torch.zeros(4, 2), {}, 2, 4, cost_guide=GUIDE)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        make(cls="DynamicGaussianDiffusionModel").conditional_sample({}, cost_guide=GUIDE)
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            make(sampler=sampler).conditional_sample({}, batch_size=2, sample_fn=lambda *a, **k: None, cost_guide=GUIDE)
    # n_samples counts rows: a multiple of the team size, per scene
    with pytest.raises(ValueError, match="no multiple of the team size 2"):
        dm.run_inference(None, {}, n_samples=3, obstacle_pts=torch.zeros(4, 2), cost_guide=GUIDE)
    with pytest.raises(ValueError, match="scene 1"):
        dm.run_inference_scenes([torch.zeros(1, 4, 2)] * 2, [{}, {}], n_samples=[2, 3], cost_guide=dict({k: v for k, v in GUIDE.items() if k != "cloud"}, clouds=[torch.zeros(4, 2)] * 2))
    with pytest.raises(ValueError, match="scene 0"):
        dm.run_inference_composed([[torch.zeros(1, 4, 2)]], [{}], n_samples=5, cost_guide=GUIDE)
    from ramp_amd.team import run_inference_teams, team_clearance
    with pytest.raises(ValueError, match="needs team="):
        run_inference_teams(dm, [torch.zeros(1, 4, 2)], [torch.zeros(2, 4)], [torch.zeros(2, 4)], 1, dict(cloud=torch.zeros(4, 2), radius=0.3, step=0.01))
    with pytest.raises(ValueError, match="start states for teams of 2"):
        run_inference_teams(dm, [torch.zeros(1, 4, 2)], [torch.zeros(3, 4)], [torch.zeros(3, 4)], 1, dict({k: v for k, v in GUIDE.items() if k != "cloud"}, clouds=[torch.zeros(4, 2)]))
    with pytest.raises(_lib.RampHipError, match="HIP device"):
        team_clearance(torch.zeros(2, 8, 4), 2, 0.1)


# ------------------------------------------------------------------------------------------------ the C side
def test_team_guide_layout_matches_the_header():
    cls = _lib.RampTeamGuide
    body = 'printf("%zu", sizeof(ramp_team_guide));' + "".join(f'printf(" %zu", offsetof(ramp_team_guide, {f}));' for f, _ in cls._fields_)
    src = ('#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body +
           'printf(" %zu %d\\n", sizeof(ramp_cost_guide), RAMP_TEAM_MAX);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got[:-2] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert got[-2] == C.sizeof(_lib.RampCostGuide) == 80 and got[-1] == _lib.TEAM_MAX == 8


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_guided_team", 14), ("ramp_guide_step_team", 13), ("ramp_guide_cost_team", 9), ("ramp_team_clearance", 19)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_guided_team"][1][3] == C.POINTER(_lib.RampTeamGuide)
    for name, n in (("ramp_sample_guided", 13), ("ramp_sample_guided_prims", 14), ("ramp_sample_steered", 19), ("ramp_sample_stitched", 10)):
        assert len(_lib.PROTOTYPES[name][1]) == n      # untouched
    assert "take no team" in hdr
    from ramp_amd import build
    for f in ("guide_team.hip", "team.hip"):
        assert f in build.SOURCES and build.EXTRA_FLAGS[f] == ["-ffp-contract=off"]
    assert any(p.endswith("guide_core.h") for p in build.source_deps(os.path.join(build.CSRC, "guide_team.hip")))


def make_tables(keep, **kw):
    """A well-formed (ramp_cost_guide, ramp_team_guide) pair on pointers that no refused call dereferences (the host table is real)."""
    off = (C.c_int32 * 2)(0, 5)
    keep.append(off)
    cg = _lib.RampCostGuide()
    cg.point_dim, cg.n_scenes, cg.cloud_points, cg.cloud_offset_host = 2, 1, 0x1000, C.cast(off, _lib.c_i32p)
    cg.radius, cg.w_obs = 0.3, 1.0
    tg = _lib.RampTeamGuide()
    tg.team_size, tg.radius_team, tg.w_team = 2, 0.3, 1.0
    for k, v in kw.items():
        setattr(cg if k.startswith("cg_") else tg, k[3:] if k.startswith("cg_") else k, v)
    return cg, tg


def test_host_refusals_of_the_entries():
    """Every refusal of the issue's section 2 is a host check made before any device call: non-zero, the entry's name in ramp_last_error.
    (The device pointers are never dereferenced: every call here is refused.)"""
    lib = _lib.load()
    keep = []

    def step(t, B=4, H=8, S=4, n_iter=1, step=0.01, cg=True):
        rc = lib.ramp_guide_step_team(0x1000, B, H, S, C.byref(t[0]) if cg else None, C.byref(t[1]), None, n_iter, step, 0, None, None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_step_team" in msg, (rc, msg)
        return msg

    def cost(t, B=4, H=8, S=4, cg=True):
        rc = lib.ramp_guide_cost_team(0x1000, B, H, S, C.byref(t[0]) if cg else None, C.byref(t[1]), None, 0x1000, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_cost_team" in msg, (rc, msg)
        return msg

    for fn in (step, cost):
        assert "cost guide" in fn(make_tables(keep), cg=False)                              # tg without cg
        for n in (0, 9, -1):
            assert "team_size" in fn(make_tables(keep, team_size=n))
        assert "multiple of team_size" in fn(make_tables(keep, team_size=3))                # B = 4
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert "radius_team" in fn(make_tables(keep, radius_team=bad))
        for bad in (float("nan"), float("inf")):
            assert "w_team" in fn(make_tables(keep, w_team=bad))
        assert "up to 128" in fn(make_tables(keep), H=129)
        assert "point_dim" in fn(make_tables(keep, cg_point_dim=1)) and "point_dim" in fn(make_tables(keep, cg_point_dim=3), S=2)
        # the cost guide's own refusals speak with the new entry's name
        assert "radius" in fn(make_tables(keep, cg_radius=0.0)) and "finite" in fn(make_tables(keep, cg_w_acc=float("nan")))
    assert "n_iter" in step(make_tables(keep), n_iter=17) and "step" in step(make_tables(keep), step=float("nan"))
    # what is allowed: no radius where the term is off (the next check speaks)
    assert "n_iter" in step(make_tables(keep, radius_team=0.0, w_team=0.0), n_iter=17)

    def clear(B=4, H=8, S=4, D=2, A=2, min_sep=0.1, traj=0x1000):
        rc = lib.ramp_team_clearance(traj, B, H, S, D, A, min_sep, 1, *([None] * 11))
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_team_clearance" in msg, (rc, msg)
        return msg

    assert "null" in clear(traj=None) and "bad dims" in clear(B=0)
    assert "2 .. 128" in clear(H=1) and "2 .. 128" in clear(H=129)
    assert "point_dim" in clear(D=1) and "point_dim" in clear(D=4) and "point_dim" in clear(D=3, S=2)
    assert "team_size" in clear(A=0) and "team_size" in clear(A=9) and "multiple of team_size" in clear(A=3)
    assert "min_sep" in clear(min_sep=-0.1) and "min_sep" in clear(min_sep=float("nan"))
    # the job entry: without a context
    assert lib.ramp_sample_guided_team(*([None] * 14)) != 0
    assert "ramp_sample_guided_team" in lib.ramp_last_error().decode()
