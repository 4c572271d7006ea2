"""Host side of the swept box and sphere terms of the cost guide (``cost_guide=dict(boxes=, spheres=, ...)`` -> ``ramp_sample_guided_prims``):
the restatement's gradient (tests/prim_guide_ref.py) against central differences of its own cost, the designed cases of the issue, the
conditions the GPU test asks of its inputs, struct layout, the declared / bound / exported symbols and every refusal that needs no device.
No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import clearance_ref as CR
import prim_guide_ref as R
from ramp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the definition
def fd_scene(rng, D):
    boxes = (rng.uniform(-0.5, 0.5, (3, D)).astype(np.float32), rng.uniform(0.2, 0.5, (3, D)).astype(np.float32))
    spheres = (rng.uniform(-0.5, 0.5, (2, D)).astype(np.float32), rng.uniform(0.1, 0.25, 2).astype(np.float32))
    return dict(boxes=boxes, spheres=spheres, cloud=rng.uniform(-1, 1, (40, D)).astype(np.float32))


@pytest.mark.parametrize("n_sub", [1, 3, 8])
@pytest.mark.parametrize("D", [2, 3])
def test_gradient_is_the_costs_own_derivative(D, n_sub):
    """The restatement's gradient equals central differences (h = 1e-6) of its own four-term cost in float64, boxes + spheres + a cloud, to
    1e-8 of the largest component (a prototype measured 2e-11 absolute).  The path is drawn until its samples lie outside, in the band of and
    inside some primitive and stay 1e-3 away from every kink -- phi = band, the medial axes of the boxes, the spheres' centres -- which is
    checked here."""
    H, margin, band = 9, 0.04, 0.06
    k = dict(margin=margin, band=band, n_sub=n_sub, w_prim=1.0, w_obs=0.7, radius=0.3, w_smooth=0.5, w_acc=0.25)
    rng = np.random.default_rng(100 * D + n_sub)
    for attempt in range(2000):
        scene = fd_scene(rng, D)
        p = np.cumsum(rng.uniform(-0.25, 0.25, (H, D)), 0) + rng.uniform(-0.3, 0.3, D)
        low = R.sample_terms(R.samples(p, n_sub), scene, margin, band)[2]
        zones = (low > band).any() and ((low > 0) & (low < band)).any() and (low < 0).any()
        if zones and min(R.kink_distance(p, scene, margin, band, n_sub)) > 1e-3:
            break
    else:
        raise AssertionError("no path found")
    assert min(R.kink_distance(p, scene, margin, band, n_sub)) > 1e-3
    g = R.total_grad(p, scene, k)
    assert g.dtype == np.float64 and float(np.abs(R.prim_grad(p, scene, margin, band, n_sub)).max()) > 0
    eps, worst = 1e-6, 0.0
    for h in range(H):
        for d in range(D):
            q1, q2 = p.copy(), p.copy()
            q1[h, d] += eps; q2[h, d] -= eps
            fd = (R.exact_cost(q1, scene, k) - R.exact_cost(q2, scene, k)) / (q1[h, d] - q2[h, d])
            worst = max(worst, abs(fd - g[h, d]))
    scale = float(np.abs(g).max())
    print(f"D={D} n_sub={n_sub}: worst |fd - g| {worst:.2e}, scale {scale:.2e}")
    assert worst < 1e-8 * scale, (worst, scale)
    # one iteration: free waypoints move by -step s g, pinned ones and the other channels stay, a scene outside the table leaves the row alone
    x = np.zeros((1, H, D + 1)); x[0, :, :D] = p; x[0, :, D] = 7.0
    pins = {0: x[0, 0], H - 1: x[0, H - 1]}
    gz = g.copy(); gz[[0, H - 1]] = 0
    nrm = float(np.sqrt((gz ** 2).sum()))
    for max_norm, s in ((0.0, 1.0), (0.5 * nrm, 0.5)):
        y = R.iterate(x, [scene], None, pins, k, 1e-3, 1, max_norm, np.float64, D)
        assert np.allclose(y[0, :, :D], p - 1e-3 * s * gz, rtol=0, atol=1e-15) and (y[0, :, D] == 7.0).all()
    assert np.array_equal(R.iterate(x, [scene], [1], pins, k, 1e-3, 1, 0.0, np.float64, D), x)


def test_samples_and_hand_back():
    """m = 0 is the waypoint itself, bit for bit; (H - 1) n + 1 samples; the hand-back weights of a segment's samples add up to the samples'
    gradients (sum_h g_prim[h] = sum_u g_u in float64 to rounding)."""
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, (7, 3)).astype(np.float32)
    p[2, 0] = -0.0
    for n in (1, 2, 8):
        u = R.samples(p, n)
        assert u.shape == (6 * n + 1, 3) and np.array_equal(u[0::n].view(np.uint32), p.view(np.uint32))
        gu = rng.uniform(-1, 1, (6 * n + 1, 3))
        assert np.allclose(R.hand_back(gu, 7, n).sum(0), gu.sum(0), rtol=0, atol=1e-13)
    assert 127 * 8 + 1 == 1017


def test_box_and_sphere_signed_distances():
    """phi and its gradient in the regions of the definition: outside a face, outside a corner, inside (nearest face; lowest axis on a tie,
    sign(0) = +1), a sphere and its centre; phi <= 0 is 'inside the widened box' of the clearance restatement."""
    c, half = np.zeros(2), np.array([0.25, 0.5])
    u = np.array([[0.5, 0.0], [0.55, 0.9], [0.1, 0.0], [-0.125, -0.375], [0.0, 0.45], [0.0, 0.0], [-0.3, -0.1]])
    phi, g = R.box_phi(u, c, half)
    assert np.allclose(phi, [0.25, 0.5, -0.15, -0.125, -0.05, -0.25, 0.05]) and phi[3] == -0.125
    assert np.allclose(g, [[1, 0], [0.6, 0.8], [1, 0], [-1, 0], [0, 1], [1, 0], [-1, 0]])
    lo, hi = CR.box_bounds(c[None], 2 * half[None], 0.0)
    assert np.array_equal(phi <= 0, CR.wp_in_box(u, lo[0], hi[0]))
    phi, g = R.sphere_phi(np.array([[0.3, 0.4], [0.0, 0.0]]), np.zeros(2), 0.2)
    assert np.allclose(phi, [0.3, -0.2]) and np.allclose(g, [[0.6, 0.8], [0.0, 0.0]])


# ------------------------------------------------------------------------------------------------ the designed cases
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("D", [2, 3])
def test_designed_box_case(D, dtype):
    """Box of sides 0.4 at the origin, margin 0.05, band 0.02, the straight line (-0.71, 0.29) -> (0.29, -0.71) over 8 waypoints: no waypoint
    is hit, segment 3-4 cuts the corner, the smallest waypoint phi (0.0314) is above the band.  n_sub = 1 therefore leaves the trajectory
    bit-unchanged and the swept hit in place; n_sub = 8 clears it in 16 iterations (min phi along the path 0.0136)."""
    m = R.DESIGN["margin"]
    x, y1, scene = R.design_run("box", D, 1, dtype)
    r0 = CR.ref_scene(x, D, scene["boxes"], None, None, m)
    assert r0["wp_hit"].sum() == 0 and r0["seg_hit"].sum() == 1 and r0["seg_hit"][0, 3]
    assert abs(R.min_phi(x[0, :, :D], scene, m, 1) - 0.0314) < 5e-5 and R.min_phi(x[0, :, :D], scene, m, 1) > R.DESIGN["band"]
    assert np.array_equal(np.asarray(y1, np.float32).view(np.uint32), x.view(np.uint32))
    x, y8, scene = R.design_run("box", D, 8, dtype)
    r8 = CR.ref_scene(np.asarray(y8, np.float32), D, scene["boxes"], None, None, m)
    assert r8["wp_hit"].sum() == 0 and r8["seg_hit"].sum() == 0
    assert abs(R.min_phi(y8[0, :, :D], scene, m, 64) - 0.0136) < 5e-5
    assert np.array_equal(np.asarray(y8, np.float32)[0, [0, -1]], x[0, [0, -1]]) and (np.asarray(y8)[0, :, D:] == 7.0).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_designed_sphere_case(dtype):
    """Sphere of radius 0.2 at the origin, the line (-0.665, 0.335) -> (0.335, -0.665): the path's min phi is -0.0167 where the waypoints' is
    +0.0043.  n_sub = 1 pushes the waypoints out of the band and leaves a swept hit (min phi -0.0022); n_sub = 8 clears the path (+0.046)."""
    m = R.DESIGN["margin"]
    x, y1, scene = R.design_run("sphere", 2, 1, dtype)
    r0 = CR.ref_scene(x, 2, None, scene["spheres"], None, m)
    assert r0["wp_hit"].sum() == 0 and r0["seg_hit"].sum() == 1
    assert abs(R.min_phi(x[0, :, :2], scene, m, 64) + 0.0167) < 5e-5 and abs(R.min_phi(x[0, :, :2], scene, m, 1) - 0.0043) < 5e-5
    r1 = CR.ref_scene(np.asarray(y1, np.float32), 2, None, scene["spheres"], None, m)
    assert r1["seg_hit"].sum() == 1 and abs(R.min_phi(y1[0, :, :2], scene, m, 64) + 0.0022) < 5e-5
    x, y8, scene = R.design_run("sphere", 2, 8, dtype)
    r8 = CR.ref_scene(np.asarray(y8, np.float32), 2, None, scene["spheres"], None, m)
    assert r8["seg_hit"].sum() == 0 and abs(R.min_phi(y8[0, :, :2], scene, m, 64) - 0.046) < 5e-4


def test_exact_cases_do_what_they_claim():
    """The exact cases of the GPU test, in float32 and float64: a sample at a sphere's centre adds cost and moves nothing; a sample inside a
    box on an axis tie moves along the lowest axis only, with the sign of its offset (+ at offset 0)."""
    for name, c in R.exact_cases().items():
        for dtype in (np.float32, np.float64):
            y = R.iterate(c["x"], [c["scene"]], None, {}, c["k"], c["step"], 1, 0.0, dtype, c["D"])
            moved = np.asarray(y, np.float64) - c["x"]
            assert np.array_equal(moved != 0, c["moves"]), (name, dtype, moved)
            assert (np.sign(moved[c["moves"]]) == c["sign"]).all(), (name, moved)
            assert R.prim_cost(c["x"][0, :, :c["D"]].astype(dtype), c["scene"], c["k"]["margin"], c["k"]["band"], c["k"]["n_sub"]) > 0


@pytest.mark.parametrize("case", R.OP_CASES, ids=lambda c: "H%d_S%d_d%d_n%d_b%d_s%d_it%d_clip%d_band%g" % c)
def test_op_case_inputs_satisfy_their_conditions(case):
    """What tests/test_gpu_prim_guide.py asks of its op inputs, on the CPU: no sample of an input path within 1e-4 of phi = band, of a tie
    inside a box or of a sphere's centre; the primitive term pushes (a non-zero gradient); the float32 restatement differs from the float64
    one (the yardstick is no zero); with clip one trajectory is clipped and another is not; the trajectory outside the table stays."""
    c = R.op_case(case)
    d32 = float(np.abs(c["y32"] - c["y64"]).max())
    print(f"{case}: kink distance {c['kink']:.2e}, float32 restatement {d32:.2e}, first |g| {np.round(c['norms'], 3).tolist()}, prim |g| {c['prim_g']:.2e}")
    assert c["kink"] > 1e-4 and c["prim_g"] > 0 and d32 > 0
    s1 = [s for b, it, s, n in c["log"] if it == 0 and c["ts"][b] == 0]
    if case[7]:
        assert min(s1) < 1.0 and max(s1) == 1.0, s1
    assert np.array_equal(c["y64"][3], c["x"][3].astype(np.float64)) and np.array_equal(c["y32"][3], c["x"][3])
    assert np.array_equal(c["y32"][:, c["idx"]], c["x"][:, c["idx"]]) and np.array_equal(c["y32"][:, :, c["D"]:], c["x"][:, :, c["D"]:])


def test_the_lists_of_the_issue_are_covered():
    vals = list(zip(*R.OP_CASES))
    assert set(vals[0]) == {8, 128} and set(zip(vals[1], vals[2])) == {(4, 2), (6, 3)} and set(vals[3]) == {1, 2, 8}
    assert {1, 64, 65} <= set(vals[4]) and {1, 64, 65} <= set(vals[5]) and set(vals[6]) == {1, 16} and set(vals[7]) == {True, False}
    assert 0.0 in vals[8]


def test_free_running_chain_inputs_satisfy_their_conditions():
    """What tests/test_gpu_prim_guide.py::test_free_running_guided_chain asks of its inputs, checked on the CPU: the float32 oracle stays
    within a quarter of the bar (1e-4 of max |x|) and the float64 guided and unguided final states lie at least 100 bars apart."""
    import test_gpu_prim_guide as P
    for kind in ("ddpm", "ddim"):
        bar, d32, moved = P.chain_conditions(kind)
        print(f"{kind}: bar {bar:.3e}, float32 oracle {d32:.3e}, guided vs unguided {moved:.3e}")
        assert d32 <= bar / 4 and moved >= 100 * bar


# ------------------------------------------------------------------------------------------------ the C side
def test_prim_guide_layout_matches_the_header():
    """The ctypes mirror of ramp_prim_guide has the size and field offsets the C compiler gives it; ramp_cost_guide keeps its 80 bytes."""
    cls = _lib.RampPrimGuide
    body = 'printf("%zu", sizeof(ramp_prim_guide));' + "".join(f'printf(" %zu", offsetof(ramp_prim_guide, {f}));' for f, _ in cls._fields_)
    src = ('#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body +
           'printf(" %zu %d\\n", sizeof(ramp_cost_guide), RAMP_PRIM_GUIDE_MAX_SUB);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got[:-2] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert got[-2] == C.sizeof(_lib.RampCostGuide) == 80 and got[-1] == _lib.PRIM_GUIDE_MAX_SUB == 8


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_guided_prims", 14), ("ramp_guide_step_prims", 13), ("ramp_guide_cost_prims", 9)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_guided_prims"][1][2] == C.POINTER(_lib.RampCostGuide)
    assert _lib.PROTOTYPES["ramp_sample_guided_prims"][1][3] == C.POINTER(_lib.RampPrimGuide)
    assert len(_lib.PROTOTYPES["ramp_sample_guided"][1]) == 13 and len(_lib.PROTOTYPES["ramp_sample_steered"][1]) == 19      # untouched
    assert "take no primitives" in hdr
    from ramp_amd import build
    assert "guide_prims.hip" in build.SOURCES and build.EXTRA_FLAGS["guide_prims.hip"] == ["-ffp-contract=off"]


def make_tables(keep, **kw):
    """A well-formed (ramp_cost_guide, ramp_prim_guide) pair on pointers that no refused call dereferences (the host tables are real)."""
    off, boff, soff = (C.c_int32 * 2)(0, 5), (C.c_int32 * 2)(0, 3), (C.c_int32 * 2)(0, 2)
    keep += [off, boff, soff]
    cg = _lib.RampCostGuide()
    cg.point_dim, cg.n_scenes, cg.cloud_points, cg.cloud_offset_host = 2, 1, 0x1000, C.cast(off, _lib.c_i32p)
    cg.radius, cg.w_obs = 0.3, 1.0
    pg = _lib.RampPrimGuide()
    pg.point_dim, pg.n_scenes = 2, 1
    pg.box_centers = pg.box_sizes = pg.sphere_centers = pg.sphere_radii = 0x1000
    pg.box_offset_host, pg.sphere_offset_host = C.cast(boff, _lib.c_i32p), C.cast(soff, _lib.c_i32p)
    pg.margin, pg.band, pg.w_prim, pg.n_sub = 0.05, 0.02, 1.0, 4
    for k, v in kw.items():
        setattr(cg if k.startswith("cg_") else pg, k[3:] if k.startswith("cg_") else k, v)
    return cg, pg


def test_host_refusals_of_the_three_entries():
    """Every refusal of section 2 of the issue is a host check made before any device call: non-zero, the entry's name in ramp_last_error.
    (The device pointers are never dereferenced: every call here is refused.)"""
    lib = _lib.load()
    keep = []

    def step(t, H=8, S=4, n_iter=1, step=0.01):
        cg, pg = t
        rc = lib.ramp_guide_step_prims(0x1000, 2, H, S, C.byref(cg), C.byref(pg), None, n_iter, step, 0, None, None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_step_prims" in msg, (rc, msg)
        return msg

    def cost(t, H=8, S=4):
        cg, pg = t
        rc = lib.ramp_guide_cost_prims(0x1000, 2, H, S, C.byref(cg), C.byref(pg), None, 0x1000, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_cost_prims" in msg, (rc, msg)
        return msg

    i32 = lambda *v: C.cast((C.c_int32 * len(v))(*v), _lib.c_i32p)      # noqa: E731
    for fn in (step, cost):
        assert "point_dim" in fn(make_tables(keep, point_dim=1)) and "point_dim" in fn(make_tables(keep, point_dim=4))
        assert "point_dim" in fn(make_tables(keep, point_dim=3, cg_point_dim=3), S=2)                  # > state_dim
        assert "differs from the cost guide" in fn(make_tables(keep, point_dim=3))                     # the guide's is 2
        for n in (0, 9, -1):
            assert "n_sub" in fn(make_tables(keep, n_sub=n))
        assert "up to 128" in fn(make_tables(keep), H=129)
        for k in ("margin", "band"):
            for bad in (-0.01, float("nan"), float("inf")):
                assert "margin and band" in fn(make_tables(keep, **{k: bad}))
        assert "w_prim" in fn(make_tables(keep, w_prim=float("nan"))) and "w_prim" in fn(make_tables(keep, w_prim=float("inf")))
        assert "offsets" in fn(make_tables(keep, box_offset_host=i32(1, 3))) and "offsets" in fn(make_tables(keep, sphere_offset_host=i32(1, 2)))
        assert "offsets" in fn(make_tables(keep, box_offset_host=None)) and "offsets" in fn(make_tables(keep, sphere_offset_host=None))
        two = dict(n_scenes=2, cg_n_scenes=2, cg_cloud_offset_host=i32(0, 5, 5))
        assert "non-decreasing" in fn(make_tables(keep, box_offset_host=i32(0, 3, 2), sphere_offset_host=i32(0, 0, 2), **two))
        assert "non-decreasing" in fn(make_tables(keep, box_offset_host=i32(0, 0, 3), sphere_offset_host=i32(0, 2, 1), **two))
        for arr in ("box_centers", "box_sizes", "sphere_centers", "sphere_radii"):
            assert arr.split("_")[0] in fn(make_tables(keep, **{arr: None}))
        assert "n_scenes" in fn(make_tables(keep, n_scenes=2, box_offset_host=i32(0, 3, 3), sphere_offset_host=i32(0, 2, 2)))
        assert "n_scenes" in fn(make_tables(keep, n_scenes=0))
        # the cost guide's own refusals speak with the new entry's name
        assert "radius" in fn(make_tables(keep, cg_radius=0.0)) and "finite" in fn(make_tables(keep, cg_w_acc=float("nan")))
    assert "n_iter" in step(make_tables(keep), n_iter=17) and "step" in step(make_tables(keep), step=float("nan"))
    # what is allowed: a scene without either kind, an empty table with NULL arrays (the next check speaks)
    ok = make_tables(keep, box_offset_host=i32(0, 0), sphere_offset_host=i32(0, 0), box_centers=None, box_sizes=None, sphere_centers=None,
                     sphere_radii=None)
    assert "n_iter" in step(ok, n_iter=17)
    # the job entry: without a context, and a table without its cost guide is refused by name once there is one (GPU test)
    assert lib.ramp_sample_guided_prims(*([None] * 14)) != 0
    assert "ramp_sample_guided_prims" in lib.ramp_last_error().decode()


# ------------------------------------------------------------------------------------------------ the Python layer
def make(T=25, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    kw.setdefault("predict_epsilon", True)
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=48, state_dim=4), n_diffusion_steps=T, **kw)


BOX = (torch.zeros(1, 2), torch.full((1, 2), 0.4))
SPH = (torch.zeros(2, 2), torch.tensor([0.1, 0.2]))


def test_tables_defaults_and_the_primitives_only_guide():
    """The new keys of cost_guide=: defaults margin 0, w_prim 1, n_sub 4; band required; cloud=None with w_obs=0 builds its tables (an empty
    cloud of the primitives' dimension); the existing keys and defaults stay."""
    from ramp_amd.diffusion import _HostArrays, guide_tables
    from ramp_amd.guide import fill_prim_guide
    dm = make(sampler="ddpm")
    steps = dm._ddpm_steps()[0]
    g = dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, step=0.5)
    tab = guide_tables(g, steps, dm.posterior_variance)
    assert tab["prim"] == dict(margin=0.0, band=0.02, w_prim=1.0, n_sub=4) and tab["w_obs"] == 0.0 and tab["total"] == 25
    assert "prim" not in guide_tables(dict(cloud=None, radius=0.3, step=0.01), steps, dm.posterior_variance)
    arrays = _HostArrays()
    dm._device = lambda: torch.device("cpu")      # (tables only: nothing here touches a device)
    ptab = dm._prim_tables(arrays, tab, g, None)
    cg = dm._fill_guide(arrays, tab, g, None, ptab)
    pg = fill_prim_guide(ptab, tab["prim"])
    assert (cg.point_dim, cg.n_scenes, cg.w_obs) == (2, 1, 0.0) and [cg.cloud_offset_host[i] for i in range(2)] == [0, 0] and not cg.cloud_points
    assert (pg.point_dim, pg.n_scenes, pg.n_sub, pg.band, pg.w_prim, pg.margin) == (2, 1, 4, 0.02, 1.0, 0.0)
    assert [pg.box_offset_host[i] for i in range(2)] == [0, 1] and [pg.sphere_offset_host[i] for i in range(2)] == [0, 0]
    assert pg.box_centers and pg.box_sizes and not pg.sphere_centers and not pg.sphere_radii
    # a scene job: per-scene lists, a scene may lack either kind; a 3-D table
    g2 = dict(clouds=[None, torch.zeros(3, 2)], w_obs=0, boxes=[BOX, None], spheres=[None, SPH], band=0.0, margin=0.05, w_prim=2.0, n_sub=8, step=0.5)
    tab2 = guide_tables(g2, steps, dm.posterior_variance)
    ptab2 = dm._prim_tables(arrays, tab2, g2, dict(n_scenes=2))
    cg2 = dm._fill_guide(arrays, tab2, g2, dict(n_scenes=2), ptab2)
    assert ptab2["box_offset"].tolist() == [0, 1, 1] and ptab2["sphere_offset"].tolist() == [0, 0, 2] and ptab2["box_offset"].dtype == np.int32
    assert [cg2.cloud_offset_host[i] for i in range(3)] == [0, 0, 3] and tab2["prim"] == dict(margin=0.05, band=0.0, w_prim=2.0, n_sub=8)
    from ramp_amd.guide import prim_table
    t3 = prim_table((torch.zeros(2, 3), torch.tensor([0.25, 0.5])), None, 1, None, "cpu")      # (n,) sizes: cubes, as the clearance takes them
    assert t3["D"] == 3 and t3["box_sizes"].tolist() == [[0.25] * 3, [0.5] * 3] and t3["n_spheres"] == 0 and t3["sphere_centers"] is None
    # cloud=None without primitives is an empty 2-D cloud now
    g0 = dict(cloud=None, w_obs=0.0, w_smooth=1.0, step=0.01)
    cg0 = dm._fill_guide(arrays, guide_tables(g0, steps, dm.posterior_variance), g0, None)
    assert cg0.point_dim == 2 and cg0.cloud_offset_host[1] == 0


@pytest.mark.parametrize("g, exc, msg", [
    (dict(cloud=None, w_obs=0, boxes=BOX, step=0.5), ValueError, "band= is required"),
    (dict(cloud=None, w_obs=0, band=0.02, step=0.5), ValueError, "need boxes= or spheres="),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=-0.01, step=0.5), ValueError, "margin and band"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=float("nan"), step=0.5), ValueError, "margin and band"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, margin=-1.0, step=0.5), ValueError, "margin and band"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, margin=float("inf"), step=0.5), ValueError, "margin and band"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, w_prim=float("nan"), step=0.5), ValueError, "w_prim"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, n_sub=0, step=0.5), ValueError, "n_sub"),
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, n_sub=9, step=0.5), ValueError, "n_sub"),
    (dict(cloud=None, boxes=BOX, band=0.02, step=0.5), ValueError, "radius must be positive"),      # the existing refusal stays: w_obs defaults to 1
    (dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, step=0.5, prims=1), ValueError, "unknown keys"),
])
def test_bad_primitive_keys_are_refused_with_a_message(g, exc, msg):
    from ramp_amd.diffusion import guide_tables
    dm = make(sampler="ddpm")
    with pytest.raises(exc, match=msg):
        guide_tables(g, dm._ddpm_steps()[0], dm.posterior_variance)


def test_bad_primitive_tables_are_refused_with_a_message():
    from ramp_amd.guide import prim_table
    for boxes, spheres, n, d, msg in (
            ([BOX, BOX], None, 1, None, "2 entries for 1 scene"),
            (None, [SPH], 2, None, "1 entries for 2 scene"),
            ((torch.zeros(2, 2), torch.zeros(3, 2)), None, 1, None, "2 box centres but 3 box sizes"),
            (None, (torch.zeros(2, 2), torch.zeros(3)), 1, None, "2 sphere centres but 3 radii"),
            (BOX, None, 1, 3, "box centres must be"),
            ((torch.zeros(1, 4), torch.zeros(1, 4)), None, 1, None, "2-D or 3-D"),
            ((torch.zeros(1, 2), torch.full((1, 2), -0.1)), None, 1, None, "must not be negative"),
            ((torch.full((1, 2), float("nan")), torch.ones(1, 2)), None, 1, None, "non-finite"),
            (None, None, 1, None, "cannot be inferred")):
        with pytest.raises(ValueError, match=msg):
            prim_table(boxes, spheres, n, d, "cpu")


def test_python_refusals_before_anything_touches_a_device():
    """run_inference_stitched, the resample= potential and the dynamic model raise NotImplementedError when handed the new keys."""
    g = dict(cloud=None, w_obs=0, boxes=BOX, band=0.02, step=0.5)
    dm = make(sampler="ddpm")
    with pytest.raises(NotImplementedError, match="run_inference_stitched"):
        dm.run_inference_stitched(torch.zeros(4, 2), {}, 2, 4, cost_guide=g)
    with pytest.raises(NotImplementedError, match="resample="):
        dm.conditional_sample({}, resample=dict(every=1, lambda_=1.0, cloud=None, w_obs=0, boxes=BOX, band=0.02))
    with pytest.raises(NotImplementedError, match="resample="):
        dm.conditional_sample({}, cost_guide=g, resample=dict(every=1, lambda_=1.0, cloud=torch.zeros(4, 2), radius=0.3))
    with pytest.raises(NotImplementedError, match="stitched"):
        dm.conditional_sample({}, cost_guide=g, stitch=dict(n_windows=2))
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        make(cls="DynamicGaussianDiffusionModel").conditional_sample({}, cost_guide=g)
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            make(sampler=sampler).conditional_sample({}, sample_fn=lambda *a, **k: None, cost_guide=g)
    from ramp_amd.guide import prim_guide_step
    with pytest.raises(ValueError, match="band"):
        prim_guide_step(torch.zeros(1, 8, 4), BOX, band=-1.0, step=0.5)
    with pytest.raises(ValueError, match="n_sub"):
        prim_guide_step(torch.zeros(1, 8, 4), BOX, band=0.02, step=0.5, n_sub=9)
