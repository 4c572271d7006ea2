"""Host side of the swept collision checks (``ramp_traj_clearance`` and the layers over it): the float64 restatement of the definitions
(tests/clearance_ref.py) against brute-force sampling of every segment, the classes of case the shared scene generator must hold, the
struct layout, the declared / bound / exported symbols, every refusal that needs no device and the table builder.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import clearance_ref as R
from ramp_amd import _lib
from ramp_amd.scenes import build_clearance_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = len(R.CASE_TABLE)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("idx", range(N_CASES))
def test_restatement_agrees_with_sampling_and_no_decision_is_marginal(idx):
    """Every segment sampled at a spacing <= 2e-5: the minimum of max_d(|x_d - c_d| - half_d) resp. |x - c| - r over the samples has the
    sign the slab / clamp decision says, per primitive, and lies at least MARGIN from 0 (so fp32 and float64 cannot differ)."""
    case = R.make_case(idx)
    D = case["D"]
    for sc in case["scenes"]:
        fns = R.primitive_fns(sc["boxes"], sc["spheres"])
        if not fns:
            continue
        seg, wp = R.sampled_minima(sc["traj"], D, fns)
        assert np.abs(seg).min() >= R.MARGIN and np.abs(wp).min() >= R.MARGIN
        p = sc["traj"].astype(np.float64)[..., :D]
        a, b = p[:, :-1], p[:, 1:]
        j = 0
        if sc["boxes"] is not None:
            lo, hi = R.box_bounds(sc["boxes"][0], sc["boxes"][1], 0.0)
            for k in range(lo.shape[0]):
                assert np.array_equal(R.wp_in_box(p, lo[k], hi[k]), wp[..., j] <= 0)
                assert np.array_equal(R.seg_hits_box(a, b, lo[k], hi[k]), seg[..., j] <= 0)
                j += 1
        if sc["spheres"] is not None:
            c, r = sc["spheres"][0].astype(np.float64), sc["spheres"][1].astype(np.float64)
            for k in range(c.shape[0]):
                assert np.array_equal(np.sqrt(((p - c[k]) ** 2).sum(-1)) <= r[k], wp[..., j] <= 0)
                assert np.array_equal(R.seg_point_dist(a, b, c[k]) <= r[k], seg[..., j] <= 0)
                j += 1


@pytest.mark.parametrize("idx", [1, 2, 3])
def test_swept_clearance_lies_within_half_a_spacing_below_the_sampled_minimum(idx):
    case = R.make_case(idx)
    D = case["D"]
    sc = case["scenes"][0]
    cloud = sc["cloud"][:6]
    ref = R.ref_scene(sc["traj"], D, cloud=cloud)
    fns = [(lambda x, q=q.astype(np.float64): np.sqrt(((x - q) ** 2).sum(-1))) for q in cloud]
    seg, wp = R.sampled_minima(sc["traj"], D, fns)
    m = seg.min(axis=(1, 2))
    assert (ref["clear_seg"] <= m + 1e-15).all() and (ref["clear_seg"] >= m - R.SPACING / 2).all()
    assert np.allclose(ref["clear_wp"], wp.min(axis=(1, 2)), rtol=0, atol=1e-15)
    assert (ref["clear_seg"] <= ref["clear_wp"]).all()


def test_generated_set_holds_every_class():
    seen = dict(free=False, wp_hit=False, box_tunnel=False, sphere_tunnel=False, zero_length=False, zero_in=False, zero_out=False)
    for idx in range(N_CASES):
        case = R.make_case(idx)
        D = case["D"]
        for sc in case["scenes"]:
            ref = R.ref_scene(sc["traj"], D, sc["boxes"], sc["spheres"])
            wp, sg = ref["wp_hit"], ref["seg_hit"]
            seen["free"] |= bool((~wp.any(-1) & ~sg.any(-1)).any())
            seen["wp_hit"] |= bool(wp.any())
            quiet = ~(wp[:, :-1] | wp[:, 1:])                # neither endpoint inside any primitive
            p = sc["traj"].astype(np.float64)[..., :D]
            a, b = p[:, :-1], p[:, 1:]
            seen["zero_length"] |= bool((a == b).all(-1).any())
            if sc["boxes"] is not None:
                lo, hi = R.box_bounds(sc["boxes"][0], sc["boxes"][1], 0.0)
                for k in range(lo.shape[0]):
                    seen["box_tunnel"] |= bool((R.seg_hits_box(a, b, lo[k], hi[k]) & quiet).any())
                    zero, inside = (a == b) & ~(a == b).all(-1, keepdims=True), (a >= lo[k]) & (a <= hi[k])
                    seen["zero_in"] |= bool((zero & inside).any())
                    seen["zero_out"] |= bool((zero & ~inside).any())
            if sc["spheres"] is not None:
                c, r = sc["spheres"][0].astype(np.float64), sc["spheres"][1].astype(np.float64)
                for k in range(c.shape[0]):
                    seen["sphere_tunnel"] |= bool(((R.seg_point_dist(a, b, c[k]) <= r[k]) & quiet).any())
    assert all(seen.values()), seen


def test_case_table_covers_the_test_table():
    t = np.array(R.CASE_TABLE)
    assert set(t[:, 0]) == {2, 3, 65, 128} and {(s, d) for s, d in t[:, 1:3]} == {(4, 2), (6, 3), (3, 3)}
    assert set(t[:, 3]) == {0, 1, 3} and set(t[:, 4]) == {0, 2} and set(t[:, 5]) == {0, 1, 1023, 1025} and set(t[:, 6]) == {1, 3}
    case = R.make_case(3)
    assert case["counts"] == [2, 1, 2] and case["scenes"][1]["boxes"] is None and case["traj"].shape == (R.B, 3, 4)
    assert np.abs(case["traj"][..., :2]).max() <= 1.0


# ------------------------------------------------------------------------------------------------ the C side
def test_obstacles_layout_matches_the_header():
    """The ctypes mirror of ramp_obstacles has the size and field offsets the C compiler gives it (the method of
    test_replan_guide_layout_matches_the_header)."""
    cls = _lib.RampObstacles
    body = 'printf("%zu", sizeof(ramp_obstacles));' + "".join(f'printf(" %zu", offsetof(ramp_obstacles, {f}));' for f, _ in cls._fields_)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf("\\n");return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert C.sizeof(cls) == 88


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_traj_clearance", 14), ("ramp_select_scored_scenes", 14), ("ramp_scene_summary_nd", 14)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_traj_clearance"][1][4] == C.POINTER(_lib.RampObstacles)
    assert len(_lib.PROTOTYPES["ramp_scene_summary"][1]) == 13          # the existing entry keeps its signature
    from ramp_amd import build
    assert "clearance.hip" in build.SOURCES and build.EXTRA_FLAGS["clearance.hip"] == ["-ffp-contract=off"]


def make_obstacles(**kw):
    """A well-formed ramp_obstacles on pointers that no refused call dereferences."""
    ob = _lib.RampObstacles()
    ob.point_dim, ob.n_scenes = 3, 1
    ob.box_centers = ob.box_sizes = ob.sphere_centers = ob.sphere_radii = ob.cloud = 0x1000
    ob.box_offset = ob.sphere_offset = ob.cloud_offset = 0x1000
    ob.n_boxes_total, ob.n_spheres_total, ob.n_points_total, ob.margin = 2, 2, 8, 0.0
    for k, v in kw.items():
        setattr(ob, k, v)
    return ob


def refused(lib, ob, B=4, H=8, S=6, traj=0x1000, first=0x1000):
    """The call is refused on the host: non-zero, the entry's name in ramp_last_error.  Returns the message."""
    rc = lib.ramp_traj_clearance(traj, B, H, S, C.byref(ob) if ob is not None else None, first, 1, 0x1000, 0x1000, 0x1000, 0x1000,
                                 0x1000, 0x1000, None)
    msg = lib.ramp_last_error().decode()
    assert rc != 0 and "ramp_traj_clearance" in msg, (rc, msg)
    return msg


def check_every_refusal(lib):
    """Every refusal of ramp_traj_clearance (shared with the GPU test: there the same calls must launch nothing either)."""
    for d in (1, 4, 0, -1):
        assert "point_dim" in refused(lib, make_obstacles(point_dim=d))
    assert "point_dim" in refused(lib, make_obstacles(point_dim=3), S=2)
    for H in (1, 0, -3, 129):
        assert "horizon" in refused(lib, make_obstacles(), H=H)
    assert "margin" in refused(lib, make_obstacles(margin=-1e-6)) and "margin" in refused(lib, make_obstacles(margin=float("nan")))
    for k in ("box_offset", "sphere_offset", "cloud_offset"):
        assert "missing table" in refused(lib, make_obstacles(**{k: None}))
    assert "missing table" in refused(lib, make_obstacles(), first=None)
    assert "null boxes" in refused(lib, make_obstacles(box_centers=None)) and "null boxes" in refused(lib, make_obstacles(box_sizes=None))
    assert "null spheres" in refused(lib, make_obstacles(sphere_centers=None))
    assert "null spheres" in refused(lib, make_obstacles(sphere_radii=None))
    assert "null cloud" in refused(lib, make_obstacles(cloud=None))
    assert "negative total" in refused(lib, make_obstacles(n_points_total=-1))
    assert "n_scenes" in refused(lib, make_obstacles(n_scenes=0)) and "n_scenes" in refused(lib, make_obstacles(n_scenes=5))
    refused(lib, None)
    refused(lib, make_obstacles(), traj=None)
    refused(lib, make_obstacles(), B=0)
    # the other two entries name themselves too
    assert lib.ramp_select_scored_scenes(0x1000, 4, 8, 6, None, 1, 0x1000, 0x1000, 0x1000, 0.1, 0.9, 0x1000, 0x1000, None) != 0
    assert "ramp_select_scored_scenes" in lib.ramp_last_error().decode()
    assert lib.ramp_select_scored_scenes(0x1000, 4, 8, 6, 0x1000, 1, None, 0x1000, 0x1000, 0.1, 0.9, 0x1000, 0x1000, None) != 0
    assert "ramp_select_scored_scenes" in lib.ramp_last_error().decode()
    for pd, S in ((1, 6), (4, 6), (3, 2)):
        assert lib.ramp_scene_summary_nd(0x1000, 4, 8, S, pd, 0x1000, 1, 0x1000, 0x1000, 0.01, 0x1000, 0x1000, 0x1000, None) != 0
        assert "ramp_scene_summary_nd" in lib.ramp_last_error().decode() and "point_dim" in lib.ramp_last_error().decode()


def test_host_refusals():
    check_every_refusal(_lib.load())


def test_what_is_allowed_is_not_refused_for_a_missing_array():
    """Totals of 0 go with NULL arrays: only the missing table speaks (the call is still refused, so nothing is dereferenced)."""
    ob = make_obstacles(box_centers=None, box_sizes=None, sphere_centers=None, sphere_radii=None, cloud=None, n_boxes_total=0,
                        n_spheres_total=0, n_points_total=0, cloud_offset=None)
    assert "missing table" in refused(_lib.load(), ob)


# ------------------------------------------------------------------------------------------------ tables
def test_table_builder():
    t = build_clearance_tables([2, 1, 2], box_counts=[3, 0, 1], sphere_counts=[0, 0, 2], cloud_sizes=[5, 7, 0])
    assert all(v.dtype == np.int32 for v in t.values())
    assert t["traj_first"].tolist() == [0, 2, 3, 5] and t["box_offset"].tolist() == [0, 3, 3, 4]
    assert t["sphere_offset"].tolist() == [0, 0, 0, 2] and t["cloud_offset"].tolist() == [0, 5, 12, 12]
    t = build_clearance_tables([4])
    assert t["traj_first"].tolist() == [0, 4] and t["box_offset"].tolist() == t["sphere_offset"].tolist() == t["cloud_offset"].tolist() == [0, 0]
    with pytest.raises(ValueError, match="no scenes"):
        build_clearance_tables([])
    with pytest.raises(ValueError, match="trajectory counts"):
        build_clearance_tables([2, 0])
    with pytest.raises(ValueError, match="box counts has 1 entries"):
        build_clearance_tables([2, 1], box_counts=[1])
    with pytest.raises(ValueError, match="sphere counts"):
        build_clearance_tables([2, 1], sphere_counts=[1, -1])
    with pytest.raises(ValueError, match="32-bit"):
        build_clearance_tables([1, 1], cloud_sizes=[2 ** 30, 2 ** 30])
