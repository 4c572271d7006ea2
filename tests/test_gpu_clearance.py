"""ramp_traj_clearance, ramp_select_scored_scenes, ramp_scene_summary_nd and the Python layers over them (trajectory_clearance, Metrics3d,
select_best_clear_scenes, examples/inference3d.py --evaluate) on the device, against the float64 restatement of the definitions
(tests/clearance_ref.py, itself checked against brute-force sampling in test_clearance_host.py) on the scenes of the shared generator, and
against the existing 2-D entry points where the two must agree bit for bit."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import clearance_ref as R
from ramp_amd import _lib, cost
from ramp_amd.clearance import trajectory_clearance
from ramp_amd.metrics import Metrics, Metrics3d
from test_clearance_host import make_obstacles
from util import GOLDEN, dev

pytestmark = pytest.mark.gpu
N_CASES = len(R.CASE_TABLE)


def S():
    return _lib.current_stream()


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def _lists(case):
    sc = case["scenes"]
    return [s["boxes"] for s in sc], [s["spheres"] for s in sc], [s["cloud"] for s in sc]


@functools.lru_cache(maxsize=None)
def computed(idx):
    """Case idx of the generator on the device: (case, float64 reference, Clearance with segments, Clearance without), computed once."""
    case = R.make_case(idx)
    boxes, spheres, clouds = _lists(case)
    t = dev(case["traj"])
    got = trajectory_clearance(t, boxes, spheres, clouds, case["counts"], point_dim=case["D"])
    wp_only = trajectory_clearance(t, boxes, spheres, clouds, case["counts"], point_dim=case["D"], swept=False)
    torch.cuda.synchronize()
    return case, R.ref_case(case), got, wp_only


def _np(x):
    return x.cpu().numpy()


def _absdiff(got, want):
    """max |got - want| with +inf == +inf counting as 0 (a scene without cloud points)."""
    got, want = _np(got).astype(np.float64), np.asarray(want, np.float64)
    same_inf = np.isinf(got) & np.isinf(want) & (got > 0) & (want > 0)
    return float(np.abs(np.where(same_inf, 0.0, got) - np.where(same_inf, 0.0, want)).max())


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("idx", range(N_CASES))
def test_against_the_float64_restatement(idx):
    """Hit counts exactly; clearances within 1e-5 (coordinates in [-1, 1], some twenty fp32 roundings: about 5e-6); path length /
    smoothness within 2e-6 / 2e-5, the bars of metrics_cases.npz.  Invariants: clear_seg <= clear_wp, a one-segment trajectory's segment
    count is never below either endpoint's flag, and without segments the waypoint outputs keep their bits."""
    case, ref, got, wp_only = computed(idx)
    e = dict(clear_wp=_absdiff(got.clearance, ref["clear_wp"]), clear_seg=_absdiff(got.swept_clearance, ref["clear_seg"]),
             path_len=_absdiff(got.path_length, ref["path_len"]), smooth=_absdiff(got.smoothness, ref["smooth"]))
    print(f"case {idx} {R.CASE_TABLE[idx]}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert np.array_equal(_np(got.wp_hits), ref["wp_hits"]), (_np(got.wp_hits), ref["wp_hits"])
    assert np.array_equal(_np(got.seg_hits), ref["seg_hits"]), (_np(got.seg_hits), ref["seg_hits"])
    assert e["clear_wp"] <= 1e-5 and e["clear_seg"] <= 1e-5, e
    assert e["path_len"] <= 2e-6 and e["smooth"] <= 2e-5, e
    assert bool((got.swept_clearance <= got.clearance).all())
    H = case["H"]
    if H == 2:
        assert bool((got.seg_hits >= got.wp_hits.clamp(max=1)).all())
    assert bool((got.seg_hits * 2 >= got.wp_hits).all())              # every hit waypoint ends a hit segment, a segment has two ends
    assert np.array_equal(_np(got.intensity), ref["wp_hits"].astype(np.float32) / np.float32(H))          # correctly rounded quotients
    assert np.array_equal(_np(got.swept_intensity), ref["seg_hits"].astype(np.float32) / np.float32(H - 1))
    assert wp_only.seg_hits is None and wp_only.swept_clearance is None
    for a, b in ((got.wp_hits, wp_only.wp_hits), (got.clearance, wp_only.clearance), (got.path_length, wp_only.path_length),
                 (got.smoothness, wp_only.smoothness)):
        assert torch.equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="swept=False"):
        wp_only.free()
    free = got.free()
    assert free.dtype == torch.bool and np.array_equal(_np(free), ref["seg_hits"] / (H - 1) <= 0.01)


def raw(t, D, first, n_scenes, prims, swept=1, margin=0.0, outs=None):
    """ramp_traj_clearance through the raw ABI.  prims: dict of device tensors / totals; outs: six tensors or None entries."""
    B, H, Sd = t.shape
    ob = _lib.RampObstacles()
    ob.point_dim, ob.n_scenes, ob.margin = D, n_scenes, margin
    for k in ("box_centers", "box_sizes", "sphere_centers", "sphere_radii", "cloud", "box_offset", "sphere_offset", "cloud_offset"):
        setattr(ob, k, _lib.ptr(prims.get(k)))
    ob.n_boxes_total, ob.n_spheres_total, ob.n_points_total = prims.get("nb", 0), prims.get("ns", 0), prims.get("np", 0)
    return _lib.load().ramp_traj_clearance(_lib.ptr(t), B, H, Sd, C.byref(ob), _lib.ptr(first), swept, *[_lib.ptr(o) for o in outs], S())


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def test_null_outputs_and_unswept_leaves_the_segment_outputs_untouched():
    case, ref, got, _ = computed(1)
    sc = case["scenes"][0]
    t = dev(case["traj"])
    B = t.shape[0]
    prims = dict(box_centers=dev(sc["boxes"][0]), box_sizes=dev(sc["boxes"][1]), sphere_centers=dev(sc["spheres"][0]),
                 sphere_radii=dev(sc["spheres"][1]), cloud=dev(sc["cloud"]), box_offset=_i32([0, 3]), sphere_offset=_i32([0, 2]),
                 cloud_offset=_i32([0, 1]), nb=3, ns=2, np=1)
    first = _i32([0, B])
    seg = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    cseg = torch.full((B,), -7.0, device="cuda")
    wp = torch.empty(B, dtype=torch.int32, device="cuda")
    assert raw(t, 3, first, 1, prims, swept=0, outs=[wp, seg, None, cseg, None, None]) == 0
    torch.cuda.synchronize()
    assert bool((seg == -7).all()) and bool((cseg == -7.0).all()) and torch.equal(wp, got.wp_hits)
    assert raw(t, 3, first, 1, prims, swept=1, outs=[None, seg, None, None, None, None]) == 0
    assert torch.equal(seg, got.seg_hits)
    assert raw(t, 3, first, 1, prims, swept=1, outs=[None] * 6) == 0
    torch.cuda.synchronize()


def test_margin_widens_boxes_and_spheres():
    """A waypoint 0.05 outside a box face and one 0.05 outside a sphere: free at margin 0 and 0.04, hit at margin 0.06; a segment passing
    0.05 beside a box edge likewise."""
    box = (np.array([[0.0, 0.0, 0.0]], np.float32), np.array([[0.4, 0.4, 0.4]], np.float32))
    sph = (np.array([[0.6, 0.6, 0.6]], np.float32), np.array([0.1], np.float32))
    t = np.zeros((3, 2, 3), np.float32)
    t[0] = [[0.25, 0.0, 0.0], [0.9, 0.9, -0.9]]                       # waypoint 0.05 off the box's +x face
    t[1] = [[0.6, 0.75, 0.6], [0.9, 0.9, -0.9]]                       # waypoint 0.05 off the sphere
    t[2] = [[0.25, -0.9, 0.1], [0.25, 0.9, 0.1]]                      # segment parallel to the +x face, 0.05 off it
    for margin, want_wp, want_seg in ((0.0, [0, 0, 0], [0, 0, 0]), (0.04, [0, 0, 0], [0, 0, 0]), (0.06, [1, 1, 0], [1, 1, 1])):
        r = trajectory_clearance(dev(t), box, sph, margin=margin)
        assert _np(r.wp_hits).tolist() == want_wp and _np(r.seg_hits).tolist() == want_seg, margin


# ------------------------------------------------------------------------------------------------ tunnelling
def tunnel_batch():
    """Four 2-D trajectories of H = 6 against one box of side 0.3 at the origin: row 0 is the shortest and smoothest but one of its
    segments crosses the box between two waypoints; rows 1-3 go round it, each longer and rougher than the one before."""
    H = 6
    t = np.zeros((4, H, 4), np.float32)
    x = np.linspace(-0.8, 0.8, H).astype(np.float32)                  # +-0.16 either side of the box: no waypoint inside (half side 0.15)
    t[0, :, 0] = x
    for i, y in enumerate((0.5, 0.6, 0.7)):
        t[1 + i, :, 0] = x
        t[1 + i, 1:-1, 1] = y
    for i in range(4):
        t[i, ::2, 2] = 0.01 * (i + 1)                                 # smoothness grows with the row
    box = (np.array([[0.0, 0.0]], np.float32), np.array([[0.3, 0.3]], np.float32))
    return t, box


def test_tunnelling_is_seen_by_the_swept_test_only():
    t, box = tunnel_batch()
    H = t.shape[1]
    d = dev(t)
    assert float(Metrics.compute_collision_intensity(d, box[0], box[1])[0]) == 0.0          # the existing kernel: waypoints only
    r = trajectory_clearance(d, box)
    assert _np(r.wp_hits).tolist() == [0, 0, 0, 0] and _np(r.seg_hits).tolist() == [1, 0, 0, 0]
    assert float(r.swept_intensity[0]) == np.float32(1) / np.float32(H - 1) and float(r.intensity[0]) == 0.0
    assert _np(r.free()).tolist() == [False, True, True, True] and _np(r.free(swept=False)).tolist() == [True] * 4
    best, n_free, idx, row, free = cost.select_best_clear_scenes(d, [4], boxes=box, swept=True)
    assert int(row[0]) == 1 and int(idx[0]) == 0 and int(n_free[0]) == 3 and _np(free).tolist() == [False, True, True, True]
    assert torch.equal(best[0], d[1])
    best, n_free, idx, row, free = cost.select_best_clear_scenes(d, [4], boxes=box, swept=False)
    assert int(row[0]) == 0 and int(n_free[0]) == 4 and torch.equal(best[0], d[0])


# ------------------------------------------------------------------------------------------------ agreement with what exists (D = 2)
def test_agrees_with_the_existing_2d_entry_points():
    g = np.load(f"{GOLDEN}/cost_cases.npz")
    t, cloud = dev(g["trajs"]), g["cloud"].reshape(-1, 2)
    r = trajectory_clearance(t, clouds=torch.from_numpy(cloud), swept=False)
    for thr in (0.02, 0.05, 0.1):
        mask, plen, smooth = cost._costs(t, torch.from_numpy(cloud), thr)
        assert torch.equal(r.clearance < thr, mask) and np.array_equal(_np(mask), g[f"mask_{thr}"]), thr
        assert torch.equal(bits(r.path_length), bits(plen)) and torch.equal(bits(r.smoothness), bits(smooth))
    # the selection, two scenes of five rows each, the fixture's cloud and a shifted copy
    clouds = [cloud, cloud + np.float32(0.07)]
    for thr in (0.02, 0.05, 0.1):
        want = cost.compute_trajectory_costs_scenes(t, [5, 5], clouds, collision_threshold=thr)
        got = cost.select_best_clear_scenes(t, [5, 5], clouds=clouds, swept=False, collision_threshold=thr)
        for a, b in zip(got, want):                                       # winner (NaN block included), n_free, rank, row, mask
            assert a.dtype == b.dtype and (torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b)), thr
    # boxes: the intensity of ramp_traj_metrics, exactly, and the reference fixture's bars
    m = np.load(f"{GOLDEN}/metrics_cases.npz")
    tm = dev(m["traj"])
    rb = trajectory_clearance(tm, (m["centers"], m["sizes"]), swept=False)
    assert torch.equal(bits(rb.intensity), bits(Metrics.compute_collision_intensity(tm, m["centers"], m["sizes"])))
    assert np.array_equal(_np(rb.intensity), m["intensity"])
    assert np.abs(_np(rb.path_length) - m["path_length"]).max() < 2e-6 and np.abs(_np(rb.smoothness) - m["smoothness"]).max() < 2e-5
    assert bool(torch.isinf(rb.clearance).all())


# ------------------------------------------------------------------------------------------------ ramp_scene_summary_nd
def summary(t, first, intensity, path_len, thr, point_dim=None):
    B, H, Sd = t.shape
    n = first.numel() - 1
    scratch = torch.full((2 * H * ((B + 255) // 256 + n) + n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rec = torch.empty(n, 6, dtype=torch.float64, device="cuda")
    mask = torch.empty(B, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    if point_dim is None:
        _lib.check(lib.ramp_scene_summary(_lib.ptr(t), B, H, Sd, _lib.ptr(first), n, _lib.ptr(intensity), _lib.ptr(path_len), thr,
                                          _lib.ptr(scratch), _lib.ptr(rec), _lib.ptr(mask), S()), "ramp_scene_summary")
    else:
        _lib.check(lib.ramp_scene_summary_nd(_lib.ptr(t), B, H, Sd, point_dim, _lib.ptr(first), n, _lib.ptr(intensity), _lib.ptr(path_len),
                                             thr, _lib.ptr(scratch), _lib.ptr(rec), _lib.ptr(mask), S()), "ramp_scene_summary_nd")
    return rec, mask


def test_scene_summary_nd():
    """point_dim = 2 is ramp_scene_summary bit for bit; point_dim = 3 against a float64 cdist / var over the free rows at the 2-D test's
    1e-5 relative bar.  Three scenes of 300 (more than one 256-row tile), 2 and 7 rows; some rows are not free."""
    rng = np.random.default_rng(7)
    counts, H, Sd = [300, 2, 7], 5, 6
    B = sum(counts)
    x = (rng.standard_normal((B, H, Sd)) * 0.4).astype(np.float32)
    inten = np.where(rng.uniform(size=B) < 0.3, 0.25, 0.0).astype(np.float32)
    inten[300:306] = 0.0
    plen = rng.uniform(1, 2, B).astype(np.float32)
    t, first = dev(x), _i32(np.concatenate([[0], np.cumsum(counts)]))
    rec2, m2 = summary(t, first, dev(inten), dev(plen), 0.01)
    nd2, mn2 = summary(t, first, dev(inten), dev(plen), 0.01, point_dim=2)
    assert torch.equal(bits(rec2), bits(nd2)) and torch.equal(m2, mn2)
    rec3, m3 = summary(t, first, dev(inten), dev(plen), 0.01, point_dim=3)
    assert torch.equal(m3, m2) and torch.equal(bits(rec3[:, :5]), bits(rec2[:, :5]))
    b = 0
    for i, n in enumerate(counts):
        rows = np.arange(b, b + n)[inten[b:b + n] <= 0.01]
        p = x[rows][..., :3].astype(np.float64)
        want = 0.0
        for h in range(H):
            d = np.triu(np.sqrt(((p[:, None, h] - p[None, :, h]) ** 2).sum(-1)), 1)
            want += d.reshape(-1).var(ddof=1)
        got = float(rec3[i, 5])
        assert abs(got - want) < 1e-5 * want, (i, got, want)
        assert abs(float(rec2[i, 5]) - want) > 1e-3 * want               # and the third coordinate matters
        b += n
    v = Metrics3d.compute_variance_waypoints(t[:300])
    p = x[:300, :, :3].astype(np.float64)
    want = sum(np.triu(np.sqrt(((p[:, None, h] - p[None, :, h]) ** 2).sum(-1)), 1).reshape(-1).var(ddof=1) for h in range(H))
    assert abs(float(v) - want) < 1e-5 * want


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("idx", [3, 4, 7])
def test_a_scene_alone_and_inside_the_batch_gives_the_same_bits(idx):
    case, _, got, _ = computed(idx)
    b = 0
    for sc, n in zip(case["scenes"], case["counts"]):
        alone = trajectory_clearance(dev(sc["traj"]), sc["boxes"], sc["spheres"], sc["cloud"], point_dim=case["D"])
        for name in ("wp_hits", "seg_hits", "clearance", "swept_clearance", "path_length", "smoothness"):
            assert torch.equal(bits(getattr(alone, name)), bits(getattr(got, name)[b:b + n])), name
        b += n


def test_metrics3d_and_selection_over_scenes():
    """Metrics3d.evaluate_scenes on the three-scene 3-D case: the keys of Metrics.evaluate_scenes plus the swept intensity, per-scene values
    from the per-row results; select_best_clear_scenes picks a free row of every scene that has one."""
    case, ref, got, _ = computed(4)
    assert case["D"] == 3
    boxes, spheres, _ = _lists(case)
    t = dev(case["traj"])
    H = case["H"]
    per, free = Metrics3d.evaluate_scenes(t, case["counts"], boxes, spheres, threshold=0.01, swept=True)
    want_free = ref["seg_hits"] / (H - 1) <= 0.01
    assert np.array_equal(_np(free), want_free)
    b = 0
    for i, n in enumerate(case["counts"]):
        m, rows = per[i], slice(b, b + n)
        assert set(m) == {"success", "collision_intensity", "swept_collision_intensity", "path_length", "path_length_std",
                          "waypoint_variance", "n_free_trajectories"}
        assert m["n_free_trajectories"] == int(want_free[rows].sum()) and m["success"] == int(want_free[rows].any()) and m.rows == rows
        assert abs(m["collision_intensity"] - 100 * (ref["wp_hits"][rows] / H).mean()) < 1e-4
        assert abs(m["swept_collision_intensity"] - 100 * (ref["seg_hits"][rows] / (H - 1)).mean()) < 1e-4
        if want_free[rows].any():
            assert abs(m["path_length"] - ref["path_len"][rows][want_free[rows]].mean()) < 1e-5
        else:
            assert m["path_length"] is None
        b += n
    per_wp, free_wp = Metrics3d.evaluate_scenes(t, case["counts"], boxes, spheres, swept=False)
    assert np.array_equal(_np(free_wp), ref["wp_hits"] / H <= 0.01) and per_wp[0]["swept_collision_intensity"] is None
    ci = Metrics3d.compute_collision_intensity(dev(case["scenes"][0]["traj"]), *boxes[0], *spheres[0], swept=True)
    assert torch.equal(ci, got.swept_intensity[:case["counts"][0]])
    assert np.abs(_np(Metrics3d.compute_path_length(t)) - ref["path_len"]).max() < 2e-6
    assert np.abs(_np(Metrics3d.compute_smoothness(t)) - ref["smooth"]).max() < 2e-5
    best, n_free, idx, row, fm = cost.select_best_clear_scenes(t, case["counts"], boxes=boxes, spheres=spheres, point_dim=3, swept=True,
                                                               intensity_threshold=0.0)
    wf = ref["seg_hits"] == 0
    assert np.array_equal(_np(fm), wf)
    b = 0
    for i, n in enumerate(case["counts"]):
        k = int(wf[b:b + n].sum())
        assert int(n_free[i]) == k
        if k:
            assert b <= int(row[i]) < b + n and wf[int(row[i])] and torch.equal(best[i], t[int(row[i])])
        else:
            assert int(row[i]) == -1 and bool(torch.isnan(best[i]).all())
        b += n


# ------------------------------------------------------------------------------------------------ non-finite rows, refusals
def test_a_non_finite_row_is_never_free():
    case, ref, got, _ = computed(4)
    boxes, spheres, clouds = _lists(case)
    x = case["traj"].copy()
    H = case["H"]
    x[1, 7, 2] = np.nan
    x[3, H - 1, 0] = np.inf
    t = dev(x)
    r = trajectory_clearance(t, boxes, spheres, clouds, case["counts"], point_dim=3)
    for b in (1, 3):
        assert int(r.wp_hits[b]) == H and int(r.seg_hits[b]) == H - 1
        assert bool(torch.isnan(r.clearance[b])) and bool(torch.isnan(r.swept_clearance[b]))
        assert not bool(r.free(threshold=2.0)[b]) and not bool(r.free(threshold=2.0, swept=False)[b])
    for b in (0, 2, 4):                                                   # the other rows keep their bits
        for name in ("wp_hits", "seg_hits", "clearance", "swept_clearance", "path_length", "smoothness"):
            assert torch.equal(bits(getattr(r, name)[b]), bits(getattr(got, name)[b])), name
    for swept in (True, False):
        best, n_free, idx, row, free = cost.select_best_clear_scenes(t, case["counts"], clouds, boxes, spheres, point_dim=3, swept=swept,
                                                                     intensity_threshold=2.0, collision_threshold=-1.0)
        assert not bool(free[1]) and not bool(free[3]) and 1 not in _np(row).tolist() and 3 not in _np(row).tolist()
        assert _np(n_free).tolist() == [1, 1, 1]                          # thresholds that pass every finite row: only the two are out


def test_refusals_launch_nothing():
    """Every refusal through the raw ABI on real device arrays: non-zero, the entry named, and the outputs keep their sentinel."""
    lib = _lib.load()
    t = torch.zeros(4, 8, 6, device="cuda")
    buf = torch.zeros(64, device="cuda")
    tab = _i32([0, 4])
    outs_i = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    outs_f = torch.full((4, 4), -7.0, device="cuda")
    p, q = buf.data_ptr(), tab.data_ptr()
    real = dict(box_centers=p, box_sizes=p, sphere_centers=p, sphere_radii=p, cloud=p, box_offset=q, sphere_offset=q, cloud_offset=q)

    def refused(kw, H=8, Sd=6, first=q, what=""):
        ob = make_obstacles(**{**real, **kw})
        rc = lib.ramp_traj_clearance(t.data_ptr(), 4, H, Sd, C.byref(ob), first, 1, outs_i[0].data_ptr(), outs_i[1].data_ptr(),
                                     outs_f[0].data_ptr(), outs_f[1].data_ptr(), outs_f[2].data_ptr(), outs_f[3].data_ptr(), S())
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_traj_clearance" in msg and what in msg, (kw, rc, msg)

    for d in (1, 4):
        refused(dict(point_dim=d), what="point_dim")
    refused(dict(point_dim=3), Sd=2, what="point_dim")
    refused({}, H=1, what="horizon"); refused({}, H=129, what="horizon")
    refused(dict(margin=-0.5), what="margin")
    for k in ("box_offset", "sphere_offset", "cloud_offset"):
        refused({k: None}, what="missing table")
    refused({}, first=None, what="missing table")
    refused(dict(box_sizes=None), what="null boxes"); refused(dict(sphere_radii=None), what="null spheres"); refused(dict(cloud=None), what="null cloud")
    torch.cuda.synchronize()
    assert bool((outs_i == -7).all()) and bool((outs_f == -7.0).all())
    with pytest.raises(ValueError, match="point_dim"):
        trajectory_clearance(t, clouds=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="same number of scenes"):
        trajectory_clearance(t, boxes=[None, None], clouds=[torch.zeros(3, 3)], counts=[2, 2])
    with pytest.raises(_lib.RampHipError, match="no CPU path"):
        trajectory_clearance(t.cpu(), clouds=torch.zeros(3, 3))
    with pytest.raises(_lib.RampHipError, match="horizon"):
        trajectory_clearance(torch.zeros(2, 129, 6, device="cuda"), clouds=torch.zeros(3, 3))


# ------------------------------------------------------------------------------------------------ the example
def test_example_evaluates_the_3d_batch(tmp_path, capsys):
    import examples.inference3d as ex
    out, chain = ex.main(["--make-synthetic", str(tmp_path), "--n-samples", "3", "--n-diffusion-steps", "5", "--evaluate"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and "evaluation" in lines[1] and "evaluation" not in lines[0]
    ev = out["evaluation"]
    assert set(ev) >= {"success", "collision_intensity", "swept_collision_intensity", "n_free_trajectories", "best_row"}
    assert ev["success"] in (0, 1) and 0.0 <= ev["collision_intensity"] <= 100.0 and 0.0 <= ev["swept_collision_intensity"] <= 100.0
    assert ev["n_free_selected"] == ev["n_free_trajectories"] and ev["success"] == int(ev["n_free_trajectories"] > 0)
    assert (ev["best_row"] == -1) == (ev["n_free_selected"] == 0) and -1 <= ev["best_row"] < 3
