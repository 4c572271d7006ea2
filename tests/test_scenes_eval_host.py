"""Per-scene evaluation of a many-scene batch, the host side: the table builder ``build_eval_tables``, its refusals, the new entry
points in the header and the ctypes prototypes, and the evaluation batch the GPU tests (test_gpu_scenes_eval.py) run on -- whose
coverage is asserted HERE from the float64-capable numpy oracle alone, so that no GPU test can pass on a degenerate batch.
Runs without a GPU."""
import os
import re

import numpy as np
import pytest

from oracle import ramp_oracle as O
from ramp_amd import _lib
from ramp_amd.scenes import build_eval_tables, scene_counts, scene_slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ramp_traj_metrics_scenes", "ramp_scene_summary", "ramp_traj_costs_scenes", "ramp_select_best_scenes")

COUNTS = [1, 2, 5, 300, 3, 64] + [4] * 70           # B = 655: a scene larger than a 256-row tile that starts mid-tile (row 8),
FREE_THRESHOLD = 0.01                               # 256 adjacent rows holding more than 60 scenes, a one-trajectory scene
COST_THRESHOLD = 0.05
# scenes built on purpose (the rest draw 0..6 random boxes): index -> what the construction guarantees
SCENE_BIG, SCENE_NO_FREE, SCENE_ONE_FREE, SCENE_TWO_FREE, SCENE_NO_BOX = 3, 6, 7, 8, 9


def make_eval_batch(H=48, S=4, seed=2024):
    """The evaluation batch: seeded standard_normal * 0.4 trajectories (B, H, S) in the layout of a many-scene job, per-scene
    boxes (0 to 6 each) and per-scene 2-D cost clouds (1 to 1100 points, crossing the cost kernel's 1024-point tile).
    Returns a dict of numpy arrays / lists; deterministic."""
    g = np.random.Generator(np.random.PCG64(seed))
    counts = list(COUNTS)
    n_scenes, B = len(counts), sum(counts)
    rows = scene_slices(counts)
    traj = (g.standard_normal((B, H, S)) * 0.4).astype(np.float32)
    centers, sizes = [], []
    for i in range(n_scenes):
        nb = i % 7                                                          # 0 .. 6 boxes
        centers.append(g.uniform(-1.0, 1.0, (nb, 2)).astype(np.float32))
        sizes.append(g.uniform(0.1, 0.4, (nb, 2)).astype(np.float32))
    everything = (np.zeros((1, 2), np.float32), np.full((1, 2), 20.0, np.float32))        # covers [-10, 10]^2
    far = np.float32(50.0)                                                  # rows shifted here are inside no box
    # one trajectory, boxes it cannot reach: n_free == n_traj == 1 (std NaN, variance 0)
    centers[0], sizes[0] = np.full((2, 2), 5.0, np.float32), np.full((2, 2), 0.5, np.float32)
    # 300 rows, 5 small boxes in a corner few samples reach; 20 rows moved INTO the corner: n_free > 256 but < n_traj
    centers[SCENE_BIG] = (np.array([1.5, 1.5], np.float32) + g.uniform(-0.05, 0.05, (5, 2))).astype(np.float32)
    sizes[SCENE_BIG] = np.full((5, 2), 0.3, np.float32)
    r = rows[SCENE_BIG]
    traj[r.start + 40:r.start + 60, :, :2] += np.float32(1.5)
    centers[SCENE_NO_FREE], sizes[SCENE_NO_FREE] = everything
    centers[SCENE_ONE_FREE], sizes[SCENE_ONE_FREE] = everything
    traj[rows[SCENE_ONE_FREE].start + 2, :, :2] += far
    centers[SCENE_TWO_FREE], sizes[SCENE_TWO_FREE] = everything
    traj[rows[SCENE_TWO_FREE].start + 1, :, :2] += far
    traj[rows[SCENE_TWO_FREE].start + 3, :, :2] += far
    centers[SCENE_NO_BOX], sizes[SCENE_NO_BOX] = np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    # cost clouds
    small = [1, 2, 3, 5, 8, 13, 30, 60]
    clouds = [g.uniform(-1.2, 1.2, (small[i % 8], 2)).astype(np.float32) for i in range(n_scenes)]
    clouds[0] = np.full((1, 2), 3.0, np.float32)                            # one point, out of reach
    # 1100 points: the first 1090 out of reach, the last 10 (all beyond the first 1024-point tile) among the trajectories
    clouds[SCENE_BIG] = np.concatenate([g.uniform(4.0, 5.0, (1090, 2)), g.uniform(-0.3, 0.3, (10, 2))]).astype(np.float32)
    clouds[5] = g.uniform(-1.2, 1.2, (3, 2)).astype(np.float32)            # 64 rows against 3 points: several free rows
    return {"traj": traj, "counts": counts, "rows": rows, "centers": centers, "sizes": sizes, "clouds": clouds,
            "n_scenes": n_scenes, "B": B}


def test_offsets_of_trajectories_boxes_and_clouds():
    t = build_eval_tables([2, 1, 3], [4, 0, 2], [10, 1, 1100])
    assert t["traj_first"].tolist() == [0, 2, 3, 6]
    assert t["box_offset"].tolist() == [0, 4, 4, 6]                         # a scene without boxes repeats the offset
    assert t["cloud_offset"].tolist() == [0, 10, 11, 1111]
    assert all(t[k].dtype == np.int32 and t[k].shape == (4,) for k in t)
    assert sorted(build_eval_tables([2, 1])) == ["traj_first"]              # tables only for what was given
    assert sorted(build_eval_tables([2, 1], cloud_sizes=[3, 4])) == ["cloud_offset", "traj_first"]


def test_refusals():
    with pytest.raises(ValueError, match="no scenes"):
        build_eval_tables([], [], [])
    with pytest.raises(ValueError, match="scene 1"):
        build_eval_tables([2, 0, 1], [1, 1, 1], [1, 1, 1])                  # an empty scene
    with pytest.raises(ValueError, match="scene 0"):
        build_eval_tables([-1], [1], [1])
    with pytest.raises(ValueError, match="box counts has 2 entries for 3 scenes"):
        build_eval_tables([2, 1, 3], [1, 1], [1, 1, 1])
    with pytest.raises(ValueError, match="cost cloud sizes has 4 entries for 3 scenes"):
        build_eval_tables([2, 1, 3], [1, 1, 1], [1, 1, 1, 1])
    with pytest.raises(ValueError, match="scene 2"):
        build_eval_tables([2, 1, 3], [1, 1, -1], [1, 1, 1])
    with pytest.raises(ValueError, match="32-bit"):
        build_eval_tables([2 ** 30, 2 ** 30])
    with pytest.raises(ValueError, match="32-bit"):
        build_eval_tables([1, 1], [2 ** 30, 2 ** 30])
    with pytest.raises(ValueError, match="32-bit"):
        build_eval_tables([1, 1], None, [2 ** 30, 2 ** 30])
    assert build_eval_tables([2 ** 30, 2 ** 30 - 1])["traj_first"][-1] == 2 ** 31 - 1


def test_box_offsets_may_repeat_cloud_offsets_may_not():
    assert build_eval_tables([1, 1, 1], [0, 0, 0])["box_offset"].tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="scene 1"):
        build_eval_tables([1, 1, 1], None, [5, 0, 5])


def test_counts_from_counts_or_from_the_scene_of_each_trajectory():
    assert scene_counts([2, 1, 3], 3, 6) == [2, 1, 3]
    assert scene_counts(np.array([0, 0, 1, 2, 2, 2]), 3, 6) == [2, 1, 3]
    assert scene_counts([0, 1, 2], 3, 3) == [1, 1, 1]                       # B == n_scenes: [0, 1, 2] cannot be counts (a zero)
    assert scene_counts([1, 1, 1], 3, 3) == [1, 1, 1]
    with pytest.raises(ValueError, match="ascending"):
        scene_counts([0, 1, 0, 1], 2, 4)
    with pytest.raises(ValueError, match="ascending"):
        scene_counts([0, 0, 2, 2], 2, 4)
    with pytest.raises(ValueError, match="got 5 entries"):
        scene_counts([1, 1, 1, 1, 1], 2, 4)


def test_new_entry_points_are_declared_and_prototyped():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
    assert "2 * H * W + n_scenes + 1 doubles" in hdr                        # the documented scratch size of ramp_scene_summary


@pytest.mark.parametrize("H,S", [(48, 4), (8, 6)])
def test_evaluation_batch_has_the_coverage_the_gpu_tests_rely_on(H, S):
    """From the oracle alone: the free sets (intensity <= 0.01) and the collision-free sets (cost threshold 0.05) of the batch hit
    every case the device code branches on."""
    b = make_eval_batch(H, S)
    assert b["B"] == 655 and b["n_scenes"] == 76 and b["traj"].shape == (655, H, S) and b["traj"].dtype == np.float32
    assert b["rows"][SCENE_BIG] == slice(8, 308)                            # larger than a tile, starts mid-tile, spans two
    assert sum(1 for r in b["rows"] if r.start >= 375 and r.stop <= 375 + 256) > 60    # 256 adjacent rows hold > 60 scenes
    assert sorted({c.shape[0] for c in b["centers"]}) == [0, 1, 2, 3, 4, 5, 6]
    n_free, n_traj = [], []
    for i, r in enumerate(b["rows"]):
        ci = O.collision_intensity(b["traj"][r], b["centers"][i], b["sizes"][i])
        n_free.append(int((ci <= FREE_THRESHOLD).sum())); n_traj.append(r.stop - r.start)
    assert n_free[SCENE_NO_FREE] == 0 and n_free[SCENE_ONE_FREE] == 1 and n_free[SCENE_TWO_FREE] == 2
    assert 256 < n_free[SCENE_BIG] < 300
    assert b["centers"][SCENE_NO_BOX].shape[0] == 0 and n_free[SCENE_NO_BOX] == n_traj[SCENE_NO_BOX] == 4
    assert n_traj[0] == 1 and n_free[0] == 1
    assert sum(1 for f, n in zip(n_free, n_traj) if 0 < f < n) >= 10        # plenty of mixed scenes
    sizes = [c.shape[0] for c in b["clouds"]]
    assert min(sizes) == 1 and max(sizes) == 1100 and sizes[SCENE_BIG] > 1024
    free = [~O.collision_mask(b["traj"][r], b["clouds"][i], COST_THRESHOLD) for i, r in enumerate(b["rows"])]
    nf = [int(f.sum()) for f in free]
    assert 0 in nf and 1 in nf and sum(1 for v in nf if v >= 2) >= 10
    # the big scene's collisions come from points beyond the first 1024-point tile only
    first_tile = O.collision_mask(b["traj"][b["rows"][SCENE_BIG]], b["clouds"][SCENE_BIG][:1024], COST_THRESHOLD)
    assert not first_tile.any() and 0 < nf[SCENE_BIG] < 300
    # the selection is decided somewhere: a scene with several free rows whose winner is not its first free row
    ranks = [O.trajectory_costs(b["traj"][r], b["clouds"][i], COST_THRESHOLD)[0] for i, r in enumerate(b["rows"])]
    assert any(k is not None and k > 0 for k in ranks) and any(k is None for k in ranks)
