"""Mirror of mpd/models/diffusion_models/cost.py on the HIP kernel (distance reduction on the GPU,
normalisation / argmin over B scalars in torch)."""
from __future__ import annotations

import torch

import numpy as np

from . import _lib
from .scenes import build_eval_tables, scene_counts


def _costs(trajs, obstacle_points, thr):
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("trajectory costs: tensors must live on a HIP device (no CPU path)")
    t = trajs.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    cloud = obstacle_points.reshape(-1, 2).to(t.device, torch.float32).contiguous()
    mask = torch.empty(B, dtype=torch.int32, device=t.device)
    plen = torch.empty(B, device=t.device)
    smooth = torch.empty(B, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().ramp_traj_costs(_lib.ptr(t), B, H, S, _lib.ptr(cloud), cloud.shape[0], float(thr),
                                               _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(smooth),
                                               _lib.current_stream()), "ramp_traj_costs")
    return mask.bool(), plen, smooth


def compute_collision_with_pointcloud(trajs, obstacle_points, collision_threshold=0.0, safety_margin=0.05):
    """cost.py:25-54."""
    return _costs(trajs, obstacle_points, collision_threshold)[0]


def compute_path_length(trajs):
    """cost.py:3-7."""
    return _costs(trajs, torch.full((1, 2), 1e9, device=trajs.device), 0.0)[1]


def compute_smoothness(trajs):
    """cost.py:19-24."""
    return _costs(trajs, torch.full((1, 2), 1e9, device=trajs.device), 0.0)[2]


def compute_trajectory_costs(trajs, obstacle_points, smoothness_weight=.1, path_length_weight=.9,
                             collision_threshold=0.0, normalize=True):
    """cost.py:56-88: (best_trajectory, best_cost, total_costs, collision_free_mask, best_index)."""
    coll, plen, smooth = _costs(trajs, obstacle_points, collision_threshold)
    free = ~coll
    if not free.any():
        return None, None, None, free, None
    pl, sm = plen[free], smooth[free]
    if normalize:
        pl = (pl - pl.min()) / (pl.max() - pl.min())
        sm = (sm - sm.min()) / (sm.max() - sm.min())
    total = smoothness_weight * sm + path_length_weight * pl
    best = torch.argmin(total)
    return trajs[free][best], total[best], total, free, best


def compute_trajectory_costs_scenes(trajs, counts_or_traj_scene, clouds, smoothness_weight=.1, path_length_weight=.9,
                                    collision_threshold=0.0):
    """``compute_trajectory_costs`` (cost.py:56-88, normalize=True) for every scene of a many-scene batch at once
    (ramp_select_best_scenes: two launches whatever the number of scenes): scene i's trajectories are scored against
    ``clouds[i]`` alone ((..., 2) points, 2-D like cost.py).

    Returns device tensors, without a host sync: ``best`` (n_scenes, H, S) the winner of each scene (NaN where no trajectory is
    collision-free), ``n_free`` (n_scenes) int32, ``best_index`` (n_scenes) the winner's index among the scene's collision-free
    trajectories (what the reference's argmin returns; -1 for none), ``best_row`` (n_scenes) its row in the batch (-1 for none) and
    the (B) bool ``collision_free_mask``."""
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("trajectory costs: tensors must live on a HIP device (no CPU path)")
    t = trajs.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    n_scenes = len(clouds)
    pts = []
    for i, c in enumerate(clouds):
        c = torch.as_tensor(c)
        if c.dim() < 1 or c.shape[-1] != 2:
            raise ValueError(f"scene {i}: cost clouds are 2-D point sets (..., 2); got shape {tuple(c.shape)}")
        pts.append(c.detach().reshape(-1, 2).to(torch.float32))
    counts = scene_counts(counts_or_traj_scene, n_scenes, B)
    tab = build_eval_tables(counts, cloud_sizes=[p.shape[0] for p in pts])
    dev = t.device
    cloud = torch.cat([p.to(dev) for p in pts]).contiguous()
    tables = torch.from_numpy(np.concatenate([tab["traj_first"], tab["cloud_offset"]])).to(dev)
    mask = torch.empty(B, dtype=torch.int32, device=dev)
    plen = torch.empty(B, device=dev)
    smooth = torch.empty(B, device=dev)
    best = torch.empty(n_scenes, H, S, device=dev)
    res = torch.empty(n_scenes, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_select_best_scenes(
            _lib.ptr(t), B, H, S, tables.data_ptr(), n_scenes, _lib.ptr(cloud), tables[n_scenes + 1:].data_ptr(), cloud.shape[0],
            float(collision_threshold), float(smoothness_weight), float(path_length_weight), _lib.ptr(mask), _lib.ptr(plen),
            _lib.ptr(smooth), _lib.ptr(best), _lib.ptr(res), _lib.current_stream()), "ramp_select_best_scenes")
    return best, res[:, 0], res[:, 1], res[:, 2], ~mask.bool()


def select_best_clear_scenes(trajs, counts_or_traj_scene, clouds=None, boxes=None, spheres=None, *, point_dim=None, margin=0.0, swept=True,
                             collision_threshold=0.0, intensity_threshold=0.0, smoothness_weight=.1, path_length_weight=.9):
    """``compute_trajectory_costs_scenes`` with the collision test of ``trajectory_clearance``: 2-D or 3-D, against cost clouds, boxes
    and spheres (each one entry or a list per scene, as ``trajectory_clearance`` takes them), on the segments between the waypoints
    too (``swept``).  A row is colliding iff its (swept) cloud clearance ``< collision_threshold`` or its (swept) primitive intensity
    ``> intensity_threshold``; a row with a non-finite position always is.  Selection: ramp_select_scored_scenes, the rule of
    ``compute_trajectory_costs`` per scene.

    Returns the tuple of ``compute_trajectory_costs_scenes`` -- ``best`` (n_scenes, H, S), ``n_free``, ``best_index``, ``best_row``,
    ``collision_free_mask`` (B) -- all device tensors, without a host sync.  With 2-D clouds alone, ``swept=False`` and the same
    thresholds it is ``compute_trajectory_costs_scenes`` bit for bit."""
    from .clearance import _per_scene, trajectory_clearance
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("trajectory costs: tensors must live on a HIP device (no CPU path)")
    t = trajs.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    lists = [v for v in (_per_scene("clouds", clouds, False), _per_scene("boxes", boxes, True), _per_scene("spheres", spheres, True))
             if v is not None]
    n_scenes = len(lists[0]) if lists else 1
    counts = scene_counts(counts_or_traj_scene, n_scenes, B)
    r = trajectory_clearance(t, boxes, spheres, clouds, counts, point_dim=point_dim, margin=margin, swept=swept)
    mask = r.colliding(intensity_threshold, collision_threshold, swept).to(torch.int32)
    dev = t.device
    first = r.traj_first
    best = torch.empty(n_scenes, H, S, device=dev)
    res = torch.empty(n_scenes, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_select_scored_scenes(
            _lib.ptr(t), B, H, S, first.data_ptr(), n_scenes, _lib.ptr(mask), _lib.ptr(r.path_length), _lib.ptr(r.smoothness),
            float(smoothness_weight), float(path_length_weight), _lib.ptr(best), _lib.ptr(res), _lib.current_stream()),
            "ramp_select_scored_scenes")
    return best, res[:, 0], res[:, 1], res[:, 2], ~mask.bool()
