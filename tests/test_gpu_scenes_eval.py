"""Per-scene evaluation and selection of a many-scene batch in one pass (ramp_traj_metrics_scenes, ramp_scene_summary,
ramp_traj_costs_scenes, ramp_select_best_scenes and their Python mirrors) against the one-scene entry points run scene by scene and
against the numpy oracle, on the batch of tests/test_scenes_eval_host.py (whose coverage that CPU test asserts)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, cost
from ramp_amd.metrics import Metrics
from ramp_amd.scenes import build_eval_tables
from test_scenes_eval_host import (COST_THRESHOLD, FREE_THRESHOLD, SCENE_BIG, SCENE_NO_BOX, SCENE_NO_FREE, SCENE_ONE_FREE,
                                   SCENE_TWO_FREE, make_eval_batch)
from util import GOLDEN, dev

pytestmark = pytest.mark.gpu
W_S, W_L = 0.1, 0.9


def S():
    return _lib.current_stream()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _cat(parts):
    return dev(np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in parts] + [np.zeros((1, 2), np.float32)]))


def metrics_scenes(t, first, centers, sizes, box_off, n_boxes):
    B, H, Sd = t.shape
    out = torch.empty(3, B, device="cuda")
    _lib.check(_lib.load().ramp_traj_metrics_scenes(_lib.ptr(t), B, H, Sd, _lib.ptr(first), first.numel() - 1, _lib.ptr(centers),
                                                    _lib.ptr(sizes), _lib.ptr(box_off), n_boxes, out[0].data_ptr(),
                                                    out[1].data_ptr(), out[2].data_ptr(), S()), "ramp_traj_metrics_scenes")
    return out


def summary_scenes(t, first, intensity, path_len, thr=FREE_THRESHOLD):
    B, H, Sd = t.shape
    n = first.numel() - 1
    scratch = torch.full((2 * H * ((B + 255) // 256 + n) + n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rec = torch.empty(n, 6, dtype=torch.float64, device="cuda")
    mask = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_scene_summary(_lib.ptr(t), B, H, Sd, _lib.ptr(first), n, _lib.ptr(intensity), _lib.ptr(path_len),
                                              thr, _lib.ptr(scratch), _lib.ptr(rec), _lib.ptr(mask), S()), "ramp_scene_summary")
    return rec, mask


def costs_scenes(t, first, cloud, cloud_off, n_points, thr=COST_THRESHOLD):
    B, H, Sd = t.shape
    mask = torch.empty(B, dtype=torch.int32, device="cuda"); plen = torch.empty(B, device="cuda"); sm = torch.empty(B, device="cuda")
    _lib.check(_lib.load().ramp_traj_costs_scenes(_lib.ptr(t), B, H, Sd, _lib.ptr(first), first.numel() - 1, _lib.ptr(cloud),
                                                  _lib.ptr(cloud_off), n_points, thr, _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(sm),
                                                  S()), "ramp_traj_costs_scenes")
    return mask, plen, sm


def select_scenes(t, first, cloud, cloud_off, n_points, thr=COST_THRESHOLD):
    B, H, Sd = t.shape
    n = first.numel() - 1
    mask = torch.empty(B, dtype=torch.int32, device="cuda"); plen = torch.empty(B, device="cuda"); sm = torch.empty(B, device="cuda")
    best = torch.zeros(n, H, Sd, device="cuda"); res = torch.full((n, 4), 77, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_select_best_scenes(_lib.ptr(t), B, H, Sd, _lib.ptr(first), n, _lib.ptr(cloud), _lib.ptr(cloud_off),
                                                   n_points, thr, W_S, W_L, _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(sm),
                                                   _lib.ptr(best), _lib.ptr(res), S()), "ramp_select_best_scenes")
    return res, best, mask


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


@functools.lru_cache(maxsize=None)
def batch(H=48, Sd=4):
    """The evaluation batch on the device with its tables and the results of the four many-scene entry points, computed once."""
    b = make_eval_batch(H, Sd)
    tab = build_eval_tables(b["counts"], [c.shape[0] for c in b["centers"]], [c.shape[0] for c in b["clouds"]])
    d = dict(b)
    d["t"] = dev(b["traj"])
    d["first"], d["box_off"], d["cloud_off"] = _i32(tab["traj_first"]), _i32(tab["box_offset"]), _i32(tab["cloud_offset"])
    d["n_boxes"], d["n_points"] = int(tab["box_offset"][-1]), int(tab["cloud_offset"][-1])
    d["c"], d["s"], d["cloud"] = _cat(b["centers"]), _cat(b["sizes"]), _cat(b["clouds"])     # (+ one unused row: never empty)
    d["per"] = metrics_scenes(d["t"], d["first"], d["c"], d["s"], d["box_off"], d["n_boxes"])
    d["rec"], d["free"] = summary_scenes(d["t"], d["first"], d["per"][0], d["per"][1])
    d["costs"] = costs_scenes(d["t"], d["first"], d["cloud"], d["cloud_off"], d["n_points"])
    d["sel"] = select_scenes(d["t"], d["first"], d["cloud"], d["cloud_off"], d["n_points"])
    torch.cuda.synchronize()
    return d


def one_scene(d, i):
    """Scene i of the batch as a batch of its own: (trajectories, tables, boxes, cloud)."""
    r = d["rows"][i]
    n = r.stop - r.start
    nb, npnt = d["centers"][i].shape[0], d["clouds"][i].shape[0]
    return (d["t"][r].contiguous(), _i32([0, n]), _cat([d["centers"][i]]), _cat([d["sizes"][i]]), _i32([0, nb]), nb,
            _cat([d["clouds"][i]]), _i32([0, npnt]), npnt)


@pytest.mark.parametrize("H,Sd", [(48, 4), (8, 6)])
def test_segmented_metrics_are_the_one_scene_kernel_per_scene(H, Sd):
    """Every scene's slice of (intensity, path length, smoothness) is bit for bit ramp_traj_metrics on that slice with that scene's
    boxes, and the intensity is exactly the oracle's."""
    d = batch(H, Sd)
    for i, r in enumerate(d["rows"]):
        n, nb = r.stop - r.start, d["centers"][i].shape[0]
        want = torch.empty(3, n, device="cuda")
        tt, c, s = d["t"][r].contiguous(), _cat([d["centers"][i]]), _cat([d["sizes"][i]])
        _lib.check(_lib.load().ramp_traj_metrics(_lib.ptr(tt), n, H, Sd, _lib.ptr(c), _lib.ptr(s), nb, want[0].data_ptr(),
                                                 want[1].data_ptr(), want[2].data_ptr(), S()))
        assert torch.equal(d["per"][:, r], want), i
        assert np.abs(d["per"][0, r].cpu().numpy() - O.collision_intensity(d["traj"][r], d["centers"][i], d["sizes"][i])).max() == 0, i
    assert float(d["per"][0, d["rows"][SCENE_NO_BOX]].abs().max()) == 0.0 and float(d["per"][0, d["rows"][SCENE_NO_FREE]].min()) == 1.0


@pytest.mark.parametrize("H,Sd", [(48, 4), (8, 6)])
def test_segmented_costs_are_the_one_cloud_kernel_per_scene(H, Sd):
    d = batch(H, Sd)
    mask, plen, sm = d["costs"]
    for i, r in enumerate(d["rows"]):
        n = r.stop - r.start
        tt, cl = d["t"][r].contiguous(), dev(d["clouds"][i])
        m1 = torch.empty(n, dtype=torch.int32, device="cuda"); p1 = torch.empty(n, device="cuda"); s1 = torch.empty(n, device="cuda")
        _lib.check(_lib.load().ramp_traj_costs(_lib.ptr(tt), n, H, Sd, _lib.ptr(cl), cl.shape[0], COST_THRESHOLD, _lib.ptr(m1),
                                               _lib.ptr(p1), _lib.ptr(s1), S()))
        assert torch.equal(mask[r], m1) and torch.equal(plen[r], p1) and torch.equal(sm[r], s1), i
        assert np.array_equal(m1.cpu().numpy() != 0, O.collision_mask(d["traj"][r], d["clouds"][i], COST_THRESHOLD)), i


@pytest.mark.parametrize("H,Sd", [(48, 4), (8, 6)])
def test_segmented_selection_is_select_best_per_scene(H, Sd):
    """{n_free, rank, row - first} is ramp_select_best's on the slice alone, the rank the oracle's argmin, `best` the winning row
    itself (no zeroed velocities); a scene without a free row gives {0, -1, -1, 0} and a NaN block."""
    d = batch(H, Sd)
    res, best, mask = d["sel"]
    assert torch.equal(mask, d["costs"][0])
    res_h, none = res.cpu().numpy(), 0
    for i, r in enumerate(d["rows"]):
        n = r.stop - r.start
        tt, cl = d["t"][r].contiguous(), dev(d["clouds"][i])
        m1 = torch.empty(n, dtype=torch.int32, device="cuda"); p1 = torch.empty(n, device="cuda"); s1 = torch.empty(n, device="cuda")
        b1 = torch.empty(H, Sd, device="cuda"); r1 = torch.zeros(4, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().ramp_select_best(_lib.ptr(tt), n, H, Sd, _lib.ptr(cl), cl.shape[0], COST_THRESHOLD, W_S, W_L,
                                                _lib.ptr(m1), _lib.ptr(p1), _lib.ptr(s1), _lib.ptr(b1), _lib.ptr(r1), S()))
        nf, rank, row, _ = (int(v) for v in r1.cpu())
        want_rank = O.trajectory_costs(d["traj"][r], d["clouds"][i], COST_THRESHOLD, W_S, W_L)[0]
        if nf == 0:
            none += 1
            assert want_rank is None and res_h[i].tolist() == [0, -1, -1, 0], i
            assert bool(torch.isnan(best[i]).all()), i
        else:
            assert res_h[i].tolist() == [nf, rank, row + r.start, 0], i
            assert rank == want_rank, i
            assert torch.equal(best[i], d["t"][row + r.start]), i
    assert none >= 1


def _close(got, want, tol):
    """None where the one-scene call gives None or NaN (a NaN becomes None in evaluate_scenes), else within tol."""
    if want is None or np.isnan(want):
        return got is None
    return got is not None and abs(got - want) < tol


def test_scene_summaries_match_the_one_scene_metrics_and_the_oracle():
    """Metrics.evaluate_scenes per scene vs compute_collision_intensity + trajectory_success_and_metrics on the slice (bars of
    test_metrics_against_reference_fixture_and_oracle: 1e-4 on the intensity percentage, 1e-5 on the path-length mean and std) and
    the waypoint variance within 2e-6 relative of the float64 oracle on the free rows."""
    d = batch()
    M = Metrics()
    got, free = M.evaluate_scenes(d["t"], d["counts"], d["centers"], d["sizes"], threshold=FREE_THRESHOLD)
    assert free.dtype == torch.bool and torch.equal(free, d["per"][0] <= FREE_THRESHOLD) and torch.equal(free, d["free"].bool())
    worst = 0.0
    for i, r in enumerate(d["rows"]):
        tt = d["t"][r]
        ci = M.compute_collision_intensity(tt, d["centers"][i], d["sizes"][i])
        want = M.trajectory_success_and_metrics(tt, ci, threshold=FREE_THRESHOLD)
        g = got[i]
        assert g["success"] == want["success"] and g["n_free_trajectories"] == want["n_free_trajectories"], i
        assert abs(g["collision_intensity"] - want["collision_intensity"]) < 1e-4, i
        assert _close(g["path_length"], want["path_length"], 1e-5), (i, g["path_length"], want["path_length"])
        assert _close(g["path_length_std"], want["path_length_std"], 1e-5), (i, g["path_length_std"], want["path_length_std"])
        assert torch.equal(g["free_trajectories"], want["free_trajectories"]) and g.rows == r, i
        nf = want["n_free_trajectories"]
        if nf == 0:
            assert g["waypoint_variance"] is None and want["waypoint_variance"] is None and g["path_length"] is None, i
        elif nf == 1:
            assert g["waypoint_variance"] == 0.0 and want["waypoint_variance"] == 0.0 and g["path_length_std"] is None, i
        else:
            ref = O.waypoint_variance(d["traj"][r][free[r].cpu().numpy()])
            worst = max(worst, abs(g["waypoint_variance"] - ref) / ref)
            assert abs(g["waypoint_variance"] - ref) < 2e-6 * ref, (i, g["waypoint_variance"], ref)
            assert abs(g["waypoint_variance"] - want["waypoint_variance"]) < 4e-6 * ref, i     # both within 2e-6 of the oracle
    print(f"waypoint variance vs the float64 oracle, worst scene: {worst:.2e} relative")
    nf = [g["n_free_trajectories"] for g in got]
    assert nf[SCENE_NO_FREE] == 0 and nf[SCENE_ONE_FREE] == 1 and nf[SCENE_TWO_FREE] == 2 and nf[SCENE_BIG] > 256 and nf[SCENE_NO_BOX] == 4


def test_one_scene_batch_against_the_reference_fixture():
    """tests/golden/metrics_cases.npz (the reference's Metrics outputs) as a batch of one scene, with that fixture's bars."""
    g = np.load(f"{GOLDEN}/metrics_cases.npz")
    t = dev(g["traj"])
    got, free = Metrics.evaluate_scenes(t, [t.shape[0]], [g["centers"]], [g["sizes"]], threshold=0.01)
    res = got[0]
    assert res["success"] == int(g["success"]) and res["n_free_trajectories"] == int(g["n_free"]) == int(free.sum())
    assert abs(res["collision_intensity"] - float(g["collision_intensity_pct"])) < 1e-4
    assert abs(res["path_length"] - float(g["free_path_length"])) < 1e-5
    assert abs(res["path_length_std"] - float(g["free_path_length_std"])) < 1e-5
    assert abs(res["waypoint_variance"] - float(g["free_variance"])) < 1e-5 * float(g["free_variance"])
    allfree, _ = Metrics.evaluate_scenes(t, [t.shape[0]], [np.zeros((0, 2))], [np.zeros((0, 2))])
    assert abs(allfree[0]["waypoint_variance"] - float(g["variance_all"])) < 1e-5 * float(g["variance_all"])


def test_a_scene_alone_and_inside_the_batch_gives_the_same_bits_and_runs_repeat():
    d = batch()
    for i in (0, 1, 2, SCENE_BIG, 4, 5, SCENE_NO_FREE, SCENE_ONE_FREE, SCENE_TWO_FREE, SCENE_NO_BOX, 40, 75):
        tt, first, c, s, boff, nb, cl, coff, npnt = one_scene(d, i)
        per = metrics_scenes(tt, first, c, s, boff, nb)
        rec, mask = summary_scenes(tt, first, per[0], per[1])
        assert torch.equal(bits(rec[0]), bits(d["rec"][i])), (i, rec[0].tolist(), d["rec"][i].tolist())
        assert torch.equal(mask, d["free"][d["rows"][i]]), i
        res, best, _ = select_scenes(tt, first, cl, coff, npnt)
        want = d["sel"][0][i].clone()
        if int(want[2]) >= 0:
            want[2] -= d["rows"][i].start
        assert torch.equal(res[0], want) and torch.equal(bits(best[0]), bits(d["sel"][1][i])), i
    again = metrics_scenes(d["t"], d["first"], d["c"], d["s"], d["box_off"], d["n_boxes"])
    rec2, free2 = summary_scenes(d["t"], d["first"], again[0], again[1])
    sel2 = select_scenes(d["t"], d["first"], d["cloud"], d["cloud_off"], d["n_points"])
    assert torch.equal(bits(again), bits(d["per"])) and torch.equal(bits(rec2), bits(d["rec"])) and torch.equal(free2, d["free"])
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(sel2, d["sel"]))


def test_the_tables_are_read():
    """Handing scene k the boxes / the cloud of its neighbour, or moving one scene boundary by a row, changes the results."""
    d = batch()
    nbx = [c.shape[0] for c in d["centers"]]; npt = [c.shape[0] for c in d["clouds"]]
    rolled = build_eval_tables(d["counts"], nbx[1:] + nbx[:1], npt[1:] + npt[:1])      # same totals, spans moved by one scene
    per = metrics_scenes(d["t"], d["first"], d["c"], d["s"], _i32(rolled["box_offset"]), d["n_boxes"])
    assert not torch.equal(per[0], d["per"][0]) and torch.equal(per[1:], d["per"][1:])
    mask = costs_scenes(d["t"], d["first"], d["cloud"], _i32(rolled["cloud_offset"]), d["n_points"])[0]
    assert not torch.equal(mask, d["costs"][0])
    res = select_scenes(d["t"], d["first"], d["cloud"], _i32(rolled["cloud_offset"]), d["n_points"])[0]
    assert not torch.equal(res, d["sel"][0])
    # the first row of the scene under the all-covering box joins its neighbour: its intensity drops below 1, both records move
    first = d["first"].clone(); first[SCENE_NO_FREE] += 1
    per = metrics_scenes(d["t"], first, d["c"], d["s"], d["box_off"], d["n_boxes"])
    row = d["rows"][SCENE_NO_FREE].start
    assert float(per[0, row]) < 1.0 and float(d["per"][0, row]) == 1.0
    rec, _ = summary_scenes(d["t"], first, d["per"][0], d["per"][1])
    assert rec[SCENE_NO_FREE - 1, 0] == d["rec"][SCENE_NO_FREE - 1, 0] + 1 and rec[SCENE_NO_FREE, 0] == d["rec"][SCENE_NO_FREE, 0] - 1
    # a boundary row whose collision mask differs between the two neighbouring clouds (from the oracle)
    for k in range(1, d["n_scenes"]):
        r0 = d["rows"][k].start
        one = d["traj"][r0:r0 + 1]
        if O.collision_mask(one, d["clouds"][k], COST_THRESHOLD)[0] != O.collision_mask(one, d["clouds"][k - 1], COST_THRESHOLD)[0]:
            break
    else:
        raise AssertionError("no boundary row tells the two neighbouring clouds apart")
    first = d["first"].clone(); first[k] += 1
    mask = costs_scenes(d["t"], first, d["cloud"], d["cloud_off"], d["n_points"])[0]
    assert int(mask[r0]) != int(d["costs"][0][r0])
    res = select_scenes(d["t"], first, d["cloud"], d["cloud_off"], d["n_points"])[0]
    assert not torch.equal(res[k - 1:k + 1], d["sel"][0][k - 1:k + 1])


def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [n for n in names if "memcpy" in n.lower() or n.lower().startswith("copy")]
    d2h = [n for n in copies if "dtoh" in n.lower() or "devicetohost" in n.lower()]
    kernels = [n for n in names if n not in copies and "memset" not in n.lower()]
    return kernels, copies, d2h


def test_launches_do_not_grow_with_the_scenes_and_one_copy_comes_back():
    """evaluate_scenes on the 76-scene batch issues the kernel launches of a 3-scene batch and one device-to-host copy."""
    d = batch()
    M = Metrics()
    small = (d["t"][:8].contiguous(), d["counts"][:3], d["centers"][:3], d["sizes"][:3])
    big = (d["t"], d["counts"], d["centers"], d["sizes"])
    M.evaluate_scenes(*small); M.evaluate_scenes(*big)                     # warm: allocations and lazy module loads
    k3, c3, h3 = _device_events(lambda: M.evaluate_scenes(*small))
    k76, c76, h76 = _device_events(lambda: M.evaluate_scenes(*big))
    print(f"3 scenes: {len(k3)} kernels {sorted(set(k3))}, copies {c3}; 76 scenes: {len(k76)} kernels, copies {c76}")
    assert len(k76) == len(k3) and len(k3) >= 4
    assert len(h76) == 1 and len(h3) == 1 and len(c76) == len(c3)


def test_python_mirror_of_the_selection_and_its_refusals():
    d = batch()
    best, n_free, idx, row, free = cost.compute_trajectory_costs_scenes(d["t"], d["counts"], d["clouds"], W_S, W_L, COST_THRESHOLD)
    res, want_best, mask = d["sel"]
    assert torch.equal(n_free, res[:, 0]) and torch.equal(idx, res[:, 1]) and torch.equal(row, res[:, 2])
    assert torch.equal(bits(best), bits(want_best)) and torch.equal(free, mask == 0) and free.dtype == torch.bool
    traj_scene = torch.repeat_interleave(torch.arange(d["n_scenes"]), torch.tensor(d["counts"]))
    again = cost.compute_trajectory_costs_scenes(d["t"], traj_scene, d["clouds"], W_S, W_L, COST_THRESHOLD)
    assert torch.equal(again[3], row)
    with pytest.raises(ValueError, match="2-D"):
        cost.compute_trajectory_costs_scenes(d["t"][:2], [2], [np.zeros((5, 3), np.float32)])
    lib, t, f = _lib.load(), d["t"], d["first"]
    o = torch.empty(3, 8, device="cuda")
    for args, msg in (((_lib.ptr(t), 8, 48, 4, None, 2), "null scene table"), ((_lib.ptr(t), 8, 48, 4, _lib.ptr(f), 0), "n_scenes"),
                      ((_lib.ptr(t), 8, 48, 1, _lib.ptr(f), 2), "S >= 2"), ((_lib.ptr(t), 0, 48, 4, _lib.ptr(f), 2), "B <= 0")):
        rc = lib.ramp_traj_metrics_scenes(*args, None, None, _lib.ptr(d["box_off"]), 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), S())
        assert rc != 0 and msg in lib.ramp_last_error().decode(), msg
    m = torch.empty(8, dtype=torch.int32, device="cuda")
    rc = lib.ramp_traj_costs_scenes(_lib.ptr(t), 8, 129, 4, _lib.ptr(f), 2, _lib.ptr(d["cloud"]), _lib.ptr(d["cloud_off"]), 5, 0.05,
                                    _lib.ptr(m), o[0].data_ptr(), o[1].data_ptr(), S())
    assert rc != 0 and "limit" in lib.ramp_last_error().decode()


def test_example_scores_every_directory_in_one_pass(tmp_path):
    """run_all_experiments on a 3-directory synthetic tree: its per-env metrics are those of the per-scene Metrics calls on the same
    trajectories (bars of the summary test), best_trajectory of env 0 is cost.compute_trajectory_costs on that env's rows."""
    import examples.inference_static as ex
    from ramp_amd import compat
    from test_gpu_scenes_example import _add_experiment
    cfg = ex.StaticConfig()
    cfg.n_diffusion_steps = 25
    ex.make_synthetic_experiment(str(tmp_path), cfg)
    _add_experiment(str(tmp_path), cfg.dataset_subdir, "1", 9, 7, [-0.7, 0.6], [0.7, -0.6])
    _add_experiment(str(tmp_path), cfg.dataset_subdir, "2", 4, 8, [0.5, -0.8], [-0.5, 0.8])
    per_env, runner = ex.main(["--dataset-path", str(tmp_path / "data"), "--trained-models-dir", str(tmp_path / "models"),
                               "--n-samples", "4", "--sampler", "ddpm", "--n-diffusion-steps", "25", "--n-steps-without-noise", "0",
                               "--all-envs"])
    x, M = runner.last_trajectories, Metrics()
    assert len(per_env) == 3 and x.shape == (12, 48, 4)
    for i, m in enumerate(per_env):
        data = compat.load_environment_dir(os.path.join(str(tmp_path), "data", cfg.dataset_subdir, str(i)))
        mine = x[4 * i:4 * i + 4]
        want = M.trajectory_success_and_metrics(mine, M.compute_collision_intensity(mine, data["box_centers"], data["box_sizes"]))
        assert m["env"] == i and m["success"] == want["success"] and m["n_free_trajectories"] == want["n_free_trajectories"]
        assert abs(m["collision_intensity"] - want["collision_intensity"]) < 1e-4
        assert _close(m["path_length"], want["path_length"], 1e-5) and _close(m["path_length_std"], want["path_length_std"], 1e-5)
        if want["waypoint_variance"] in (None, 0.0):
            assert m["waypoint_variance"] == want["waypoint_variance"]
        else:
            ref = O.waypoint_variance(want["free_trajectories"].cpu().numpy())
            assert abs(m["waypoint_variance"] - ref) < 2e-6 * ref
        assert torch.equal(m["free_trajectories"], want["free_trajectories"])
        if i == 0:
            best = cost.compute_trajectory_costs(mine, data["obstacle_points"])[0]
            assert torch.equal(m["best_trajectory"], best)
