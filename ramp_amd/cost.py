"""Mirror of mpd/models/diffusion_models/cost.py on the HIP kernel (distance reduction on the GPU,
normalisation / argmin over B scalars in torch)."""
from __future__ import annotations

from typing import NamedTuple

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


DIVERSE_MAX_K = 16                      # RAMP_DIVERSE_MAX_K
DIVERSE_METRICS = {"mean": 0, "max": 1}


class DiverseSelection(NamedTuple):
    """What the diverse selections return, all device tensors: ``best`` (n_scenes, k, H, S) the representatives (NaN in the slots
    nothing fills), ``rows`` (n_scenes, k) their rows in the batch (-1 padded), ``n_free`` / ``n_selected`` (n_scenes) int32,
    ``mode_of`` (B) the slot of every row (-1: colliding, or no distance that is not NaN), ``separation`` (B) its distance to that
    slot's representative (NaN where ``mode_of`` is -1), ``mode_count`` (n_scenes, k) rows per slot, ``collision_free_mask`` (B) bool."""
    best: torch.Tensor
    rows: torch.Tensor
    n_free: torch.Tensor
    n_selected: torch.Tensor
    mode_of: torch.Tensor
    separation: torch.Tensor
    mode_count: torch.Tensor
    collision_free_mask: torch.Tensor


def _diverse_params(k, min_sep, metric):
    """(k, min_sep, metric code) or a ValueError, before any device work."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= DIVERSE_MAX_K:
        raise ValueError(f"k must be an integer 1 .. {DIVERSE_MAX_K}; got {k!r}")
    if isinstance(min_sep, bool) or not isinstance(min_sep, (int, float, np.integer, np.floating)) or not float(min_sep) >= 0.0:
        raise ValueError(f"min_sep must be a number that is not negative (and not NaN); got {min_sep!r}")
    if not isinstance(metric, str) or metric not in DIVERSE_METRICS:
        raise ValueError(f"metric must be one of {sorted(DIVERSE_METRICS)}; got {metric!r}")
    return int(k), float(min_sep), DIVERSE_METRICS[metric]


def _select_diverse(t, first, n_scenes, mask, plen, smooth, w_s, w_l, k, min_sep, code, D):
    """ramp_select_diverse_scenes on device tensors that are already float32 / int32 and contiguous."""
    B, H, S = t.shape
    dev = t.device
    best = torch.empty(n_scenes, k, H, S, device=dev)
    rows = torch.empty(n_scenes, k, dtype=torch.int32, device=dev)
    res = torch.empty(n_scenes, 4, dtype=torch.int32, device=dev)
    mode_of = torch.empty(B, dtype=torch.int32, device=dev)
    sep = torch.empty(B, device=dev)
    count = torch.empty(n_scenes, k, dtype=torch.int32, device=dev)
    scratch = torch.empty(2 * B + n_scenes, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_select_diverse_scenes(
            _lib.ptr(t), B, H, S, D, first.data_ptr(), n_scenes, _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(smooth), float(w_s), float(w_l),
            k, min_sep, code, _lib.ptr(best), _lib.ptr(rows), _lib.ptr(res), _lib.ptr(mode_of), _lib.ptr(sep), _lib.ptr(count),
            _lib.ptr(scratch), _lib.current_stream()), "ramp_select_diverse_scenes")
    return DiverseSelection(best, rows, res[:, 0], res[:, 1], mode_of, sep, count, mask == 0)


def select_diverse_scored_scenes(trajs, traj_first, mask, path_length, smoothness, *, k, min_sep, metric="mean", point_dim=2,
                                 smoothness_weight=.1, path_length_weight=.9):
    """The ``k`` cheapest collision-free trajectories of every scene that are pairwise at least ``min_sep`` apart, and the one of
    them every other free row is nearest to, on per-row arrays the caller already holds (ramp_select_diverse_scenes, whose
    definition is in include/ramp_hip.h; 2 k + 1 launches whatever the number of scenes, no host sync).

    trajs (B, H, S) device tensor, 1 <= H <= 128; ``traj_first`` (n_scenes + 1) the first row of each scene, non-decreasing (a device
    int32 tensor is used as it is); ``mask`` (B), non-zero = colliding; ``path_length`` / ``smoothness`` (B), e.g. from
    ``trajectory_clearance``.  ``metric``: 'mean' or 'max' of the waypoint distances over the first ``point_dim`` (2 or 3) state
    entries.  Column 0 is what ramp_select_scored_scenes picks.  Returns a ``DiverseSelection``."""
    k, min_sep, code = _diverse_params(k, min_sep, metric)
    if int(point_dim) not in (2, 3) or int(point_dim) > trajs.shape[-1]:
        raise ValueError(f"point_dim must be 2 or 3 and at most the state width {trajs.shape[-1]}; got {point_dim}")
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("diverse selection: tensors must live on a HIP device (no CPU path)")
    t = trajs.detach().to(torch.float32).contiguous()
    dev = t.device
    first = torch.as_tensor(traj_first).to(dev, torch.int32).contiguous()
    if first.dim() != 1 or first.numel() < 2:
        raise ValueError("traj_first must hold n_scenes + 1 >= 2 entries")
    m = torch.as_tensor(mask).to(dev)
    m = (m != 0).to(torch.int32).contiguous()
    plen = torch.as_tensor(path_length).to(dev, torch.float32).contiguous()
    smooth = torch.as_tensor(smoothness).to(dev, torch.float32).contiguous()
    if not (m.numel() == plen.numel() == smooth.numel() == t.shape[0]):
        raise ValueError(f"mask, path_length and smoothness must hold one entry per trajectory ({t.shape[0]})")
    return _select_diverse(t, first, first.numel() - 1, m, plen, smooth, smoothness_weight, path_length_weight, k, min_sep, code,
                           int(point_dim))


def select_diverse_clear_scenes(trajs, counts_or_traj_scene, clouds=None, boxes=None, spheres=None, *, k, min_sep, metric="mean",
                                point_dim=None, margin=0.0, swept=True, collision_threshold=0.0, intensity_threshold=0.0,
                                smoothness_weight=.1, path_length_weight=.9):
    """``select_best_clear_scenes`` with ``k`` plans per scene instead of one: the same ``trajectory_clearance`` scoring and the same
    collision rule, then the selection of ``select_diverse_scored_scenes`` (distances over the ``point_dim`` position entries the
    clearance uses).  ``k=1`` is ``select_best_clear_scenes``.  Returns a ``DiverseSelection``, all device tensors, without a host sync."""
    from .clearance import _per_scene, trajectory_clearance
    k, min_sep, code = _diverse_params(k, min_sep, metric)
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("diverse selection: tensors must live on a HIP device (no CPU path)")
    t = trajs.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    lists = [v for v in (_per_scene("clouds", clouds, False), _per_scene("boxes", boxes, True), _per_scene("spheres", spheres, True))
             if v is not None]
    n_scenes = len(lists[0]) if lists else 1
    counts = scene_counts(counts_or_traj_scene, n_scenes, B)
    r = trajectory_clearance(t, boxes, spheres, clouds, counts, point_dim=point_dim, margin=margin, swept=swept)
    mask = r.colliding(intensity_threshold, collision_threshold, swept).to(torch.int32)
    return _select_diverse(t, r.traj_first, n_scenes, mask, r.path_length, r.smoothness, smoothness_weight, path_length_weight, k,
                           min_sep, code, r.point_dim)


def diverse_reference(traj, traj_first, mask, plen, smooth, w_s, w_l, k, min_sep, metric, point_dim):
    """The numpy statement of ramp_select_diverse_scenes (include/ramp_hip.h), for tests; the product never calls it.  Totals in
    float32 exactly as the kernels form them, distances in float64 on the float32 inputs, ``min_sep`` as the float32 the call receives;
    ``metric`` 0 / 'mean' or 1 / 'max'.  Returns a dict of numpy arrays: ``best`` (n_scenes, k, H, S), ``rows`` (n_scenes, k),
    ``result`` (n_scenes, 4), ``mode_of`` (B), ``sep`` (B) float64, ``mode_count`` (n_scenes, k), and ``dist`` -- per scene the
    (n_selected, rows of the scene) float64 distances of every row to every representative (what a test checks its margins on)."""
    F = np.float32
    x = np.asarray(traj, F)
    B, H, S = x.shape
    D = int(point_dim)
    p = x[:, :, :D].astype(np.float64)
    tf = np.asarray(traj_first, np.int64)
    n_scenes = len(tf) - 1
    mask = np.asarray(mask) != 0
    code = DIVERSE_METRICS.get(metric, metric)
    ms = float(F(min_sep))
    best = np.full((n_scenes, k, H, S), np.nan, F)
    rows = np.full((n_scenes, k), -1, np.int32)
    result = np.zeros((n_scenes, 4), np.int32)
    mode_of = np.full(B, -1, np.int32)
    sep = np.full(B, np.nan)
    mode_count = np.zeros((n_scenes, k), np.int32)
    dist = []

    def d_to(rep, lo, hi):
        n = np.sqrt(((p[lo:hi] - p[rep]) ** 2).sum(-1))                   # (rows, H)
        return n.max(-1) if code == 1 else n.sum(-1) / H

    for s in range(n_scenes):
        lo = int(min(max(tf[s], 0), B)); hi = int(min(max(tf[s + 1], lo), B))
        free = np.nonzero(~mask[lo:hi])[0]
        result[s] = (len(free), 0, -1, 0)
        ds = []
        if len(free):
            pl, sm = np.asarray(plen, F)[lo:hi][free], np.asarray(smooth, F)[lo:hi][free]
            with np.errstate(divide="ignore", invalid="ignore"):
                pl = (pl - pl.min()) / (pl.max() - pl.min())
                sm = (sm - sm.min()) / (sm.max() - sm.min())
                tot = F(w_s) * sm + F(w_l) * pl
            assert tot.dtype == np.float32
            nan = np.isnan(tot)
            order = free[np.lexsort((free, np.where(nan, F(0), tot), ~nan))]    # NaN totals first, then the total, then the row
            alive = np.zeros(hi - lo, bool); alive[free] = True
            near = np.full(hi - lo, np.nan); slot = np.full(hi - lo, -1, np.int32)
            reps = []
            for b in order:
                if len(reps) == k:
                    break
                if not alive[b]:
                    continue
                j = len(reps)
                reps.append(b); alive[b] = False
                with np.errstate(invalid="ignore"):
                    d = d_to(lo + b, lo, hi)
                    ds.append(d)
                    alive &= d >= ms                                             # a NaN distance suppresses
                    closer = ~np.isnan(d) & ((slot < 0) | (d < near)) & ~mask[lo:hi]
                is_rep = np.zeros(hi - lo, bool); is_rep[reps[:-1]] = True
                closer &= ~is_rep
                slot[closer] = j; near[closer] = d[closer]
                slot[b] = j; near[b] = d[b]                                      # a representative belongs to its own slot
            rows[s, :len(reps)] = lo + np.asarray(reps, np.int32)
            best[s, :len(reps)] = x[lo + np.asarray(reps)]
            result[s, 1], result[s, 2] = len(reps), rows[s, 0]
            mode_of[lo:hi] = slot; sep[lo:hi] = near
            mode_count[s] = np.bincount(slot[slot >= 0], minlength=k)[:k]
        dist.append(np.asarray(ds, np.float64).reshape(len(ds), hi - lo))
    return dict(best=best, rows=rows, result=result, mode_of=mode_of, sep=sep, mode_count=mode_count, dist=dist)


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


def select_best_teams_scenes(x, size, team_first, team_mask, team_len, team_smooth, w_smooth=.1, w_len=.9):
    """The best conflict-free TEAM of every scene (``ramp_amd.team``): ``x`` (B, H, S) rows in team layout or (B / size, size, H, S),
    ``team_first`` (n_scenes + 1) the first team of each scene (``traj_first / size``), and the team-level arrays of
    ``team.team_clearance`` -- ``team_mask`` (1 = a member collides or the team has a conflict), ``team_len``, ``team_smooth``.  The
    selection is ramp_select_scored_scenes on the trajectories viewed as (B / size, size * H, S): a team's rows are adjacent.

    Returns ``(winners, result)``: (n_scenes, size, H, S), NaN for a scene without a free team, and the int32 (n_scenes, 4) table
    ``{n_free, winner's index among the scene's free teams, winner's team in the batch, 0}`` (``{0, -1, -1, 0}`` for none) -- device
    tensors, without a host sync."""
    if x.device.type != "cuda":
        raise _lib.RampHipError("team selection: tensors must live on a HIP device (no CPU path)")
    size = int(size)
    t = x.detach().to(torch.float32).contiguous()
    if t.dim() == 4:
        t = t.reshape(-1, t.shape[-2], t.shape[-1])
    B, H, S = t.shape
    if size < 1 or B % size:
        raise ValueError(f"team selection: {B} rows are no multiple of the team size {size}")
    n = B // size
    dev = t.device
    first = torch.as_tensor(team_first).to(dev, torch.int32).contiguous()
    if first.dim() != 1 or first.numel() < 2:
        raise ValueError("team_first must hold n_scenes + 1 >= 2 entries")
    n_scenes = first.numel() - 1
    m = (torch.as_tensor(team_mask).to(dev) != 0).to(torch.int32).contiguous()
    plen = torch.as_tensor(team_len).to(dev, torch.float32).contiguous()
    smooth = torch.as_tensor(team_smooth).to(dev, torch.float32).contiguous()
    if not (m.numel() == plen.numel() == smooth.numel() == n):
        raise ValueError(f"team_mask, team_len and team_smooth must hold one entry per team ({n})")
    best = torch.empty(n_scenes, size * H, S, device=dev)
    res = torch.empty(n_scenes, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_select_scored_scenes(
            _lib.ptr(t), n, size * H, S, first.data_ptr(), n_scenes, _lib.ptr(m), _lib.ptr(plen), _lib.ptr(smooth), float(w_smooth),
            float(w_len), _lib.ptr(best), _lib.ptr(res), _lib.current_stream()), "ramp_select_scored_scenes")
    return best.reshape(n_scenes, size, H, S), res
