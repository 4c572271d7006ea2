"""Mirror of scripts/inference/core/metrics.py (Metrics / DynamicMetrics) on the HIP kernels: the per-trajectory
reductions and the O(B^2 H) pairwise waypoint variance run on the device (ramp_traj_metrics / ramp_waypoint_variance);
the selection logic around them is the reference's."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .scenes import build_eval_tables, scene_counts


def _dev_traj(trajs: torch.Tensor) -> torch.Tensor:
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("metrics: tensors must live on a HIP device (no CPU path)")
    assert trajs.ndim == 3
    return trajs.detach().to(torch.float32).contiguous()


def _per_traj(trajs, centers=None, sizes=None):
    t = _dev_traj(trajs)
    B, H, S = t.shape
    out = torch.empty(3, B, device=t.device)
    nb = 0 if centers is None else centers.shape[0]
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().ramp_traj_metrics(_lib.ptr(t), B, H, S, _lib.ptr(centers), _lib.ptr(sizes), nb,
                                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 _lib.current_stream()), "ramp_traj_metrics")
    return out


class SceneMetrics(dict):
    """One scene's dict of ``Metrics.evaluate_scenes``: the keys of ``trajectory_success_and_metrics``.  ``free_trajectories`` is
    gathered from the batch's free mask (a boolean-mask gather, i.e. a host sync) only when it is first read, so that
    evaluating many scenes costs no per-scene sync; ``rows`` is the scene's slice of the batch."""

    def __init__(self, values, trajs, free_mask, rows):
        super().__init__(values)
        self._trajs, self._free_mask, self.rows = trajs, free_mask, rows

    def __missing__(self, key):
        if key != 'free_trajectories':
            raise KeyError(key)
        self[key] = self._trajs[self.rows][self._free_mask[self.rows]]
        return self[key]


class Metrics:
    """metrics.py:5-126."""

    @staticmethod
    def compute_variance_waypoints(trajs, eps=1e-8):
        t = _dev_traj(trajs)
        B, H, S = t.shape
        if B < 2:
            return torch.tensor(float("nan"), device=t.device)
        scratch = torch.empty(2 * H * ((B + 255) // 256), dtype=torch.float64, device=t.device)
        out = torch.empty(1, dtype=torch.float64, device=t.device)
        with torch.cuda.device(t.device):
            _lib.check(_lib.load().ramp_waypoint_variance(_lib.ptr(t), B, H, S, _lib.ptr(scratch), _lib.ptr(out),
                                                          _lib.current_stream()), "ramp_waypoint_variance")
        return out[0].to(torch.float32)

    @staticmethod
    def compute_smoothness(trajs: torch.Tensor, trajs_vel: Optional[torch.Tensor] = None) -> torch.Tensor:
        if trajs_vel is not None:                      # velocities given separately: pad two position columns
            assert trajs_vel.ndim == 3
            trajs = torch.cat([torch.zeros_like(trajs_vel[..., :2]), trajs_vel], dim=-1)
        return _per_traj(trajs)[2]

    @staticmethod
    def compute_path_length(trajectories: torch.Tensor) -> torch.Tensor:
        assert trajectories.ndim == 3
        if len(trajectories) == 0:
            return torch.tensor(0.0, device=trajectories.device)
        return _per_traj(trajectories)[1]

    @staticmethod
    def compute_collision_intensity(trajs: torch.Tensor, box_centers, box_sizes) -> torch.Tensor:
        dev = trajs.device
        c = torch.as_tensor(box_centers, dtype=torch.float32, device=dev)
        s = torch.as_tensor(box_sizes, dtype=torch.float32, device=dev)
        if s.dim() == 1:
            s = s.unsqueeze(-1).repeat(1, 2)
        return _per_traj(trajs, c.reshape(-1, 2)[:, :2].contiguous(), s.reshape(-1, 2).contiguous())[0]

    def trajectory_success_and_metrics(self, trajs_final: torch.Tensor, collision_intensities: torch.Tensor,
                                       threshold: float = 0.01) -> Dict[str, Any]:
        ok = collision_intensities <= threshold
        free = trajs_final[torch.where(ok)[0]]
        n_free = len(free)
        m = {'success': 1 if bool(torch.any(ok)) else 0,
             'collision_intensity': collision_intensities.mean().item() * 100,
             'path_length': None, 'path_length_std': None, 'waypoint_variance': None,
             'free_trajectories': free, 'n_free_trajectories': n_free}
        if n_free > 0:
            pl = self.compute_path_length(free)
            m['path_length'] = pl.mean().item()
            m['path_length_std'] = pl.std().item()
            if n_free == 1:
                m['waypoint_variance'] = 0.0
            else:
                v = float(self.compute_variance_waypoints(free))
                m['waypoint_variance'] = v if not np.isnan(v) else None
        return m


    @staticmethod
    def evaluate_scenes(trajs: torch.Tensor, counts_or_traj_scene, box_centers_list, box_sizes_list, threshold: float = 0.01):
        """``compute_collision_intensity`` + ``trajectory_success_and_metrics`` for every scene of a many-scene batch
        (``run_inference_scenes``: a scene's trajectories adjacent, scenes in order) in one pass: the loop over experiments of
        scripts/inference/inference_static.py around metrics.py:21-126.

        counts_or_traj_scene  trajectories per scene, or the (B) ``traj_scene`` array (a device one costs a copy: pass counts)
        box_centers_list / box_sizes_list  per scene, what ``compute_collision_intensity`` takes ((n, 2) centres, (n, 2) or (n) sizes;
                                           a scene may have no box)

        Returns ``(per_scene, free_mask)``: one dict per scene with the keys and value conventions of
        ``trajectory_success_and_metrics`` (None where the reference gives None, collision intensity in percent), and the (B) bool
        device mask ``intensity <= threshold``.  ``free_trajectories`` is gathered lazily, when a caller reads it (SceneMetrics);
        ``.rows`` of each dict is the scene's slice of the batch.
        All uploads happen first (boxes, one int32 table); then ramp_traj_metrics_scenes + ramp_scene_summary, four kernels
        whatever the number of scenes; the call ends in its only device-to-host copy, the (n_scenes, 6) records."""
        t = _dev_traj(trajs)
        B, H, S = t.shape
        n_scenes = len(box_centers_list)
        if len(box_sizes_list) != n_scenes:
            raise ValueError(f"{n_scenes} box-centre entries but {len(box_sizes_list)} box-size entries")
        counts = scene_counts(counts_or_traj_scene, n_scenes, B)
        cs, ss = [], []
        for c, z in zip(box_centers_list, box_sizes_list):
            c = torch.as_tensor(c, dtype=torch.float32).detach().cpu().reshape(-1, 2)
            z = torch.as_tensor(z, dtype=torch.float32).detach().cpu()
            if z.dim() == 1:
                z = z.unsqueeze(-1).repeat(1, 2)
            z = z.reshape(-1, 2)
            if z.shape[0] != c.shape[0]:
                raise ValueError(f"scene {len(cs)}: {c.shape[0]} box centres but {z.shape[0]} box sizes")
            cs.append(c); ss.append(z)
        tab = build_eval_tables(counts, box_counts=[c.shape[0] for c in cs])
        n_boxes = int(tab["box_offset"][-1])
        dev = t.device
        boxes = torch.cat([torch.cat(cs), torch.cat(ss)]).contiguous().to(dev)         # (2 n_boxes, 2): centres then sizes
        tables = torch.from_numpy(np.concatenate([tab["traj_first"], tab["box_offset"]])).to(dev)
        per = torch.empty(3, B, device=dev)
        W = (B + 255) // 256 + n_scenes
        scratch = torch.empty(2 * H * W + n_scenes + 1, dtype=torch.float64, device=dev)
        summary = torch.empty(n_scenes, 6, dtype=torch.float64, device=dev)
        mask = torch.empty(B, dtype=torch.int32, device=dev)
        first, box_off = tables[:n_scenes + 1], tables[n_scenes + 1:]
        with torch.cuda.device(dev):
            lib = _lib.load()
            _lib.check(lib.ramp_traj_metrics_scenes(_lib.ptr(t), B, H, S, first.data_ptr(), n_scenes,
                                                    boxes.data_ptr() if n_boxes else None,
                                                    boxes[n_boxes:].data_ptr() if n_boxes else None, box_off.data_ptr(), n_boxes,
                                                    per[0].data_ptr(), per[1].data_ptr(), per[2].data_ptr(),
                                                    _lib.current_stream()), "ramp_traj_metrics_scenes")
            _lib.check(lib.ramp_scene_summary(_lib.ptr(t), B, H, S, first.data_ptr(), n_scenes, per[0].data_ptr(),
                                              per[1].data_ptr(), float(threshold), _lib.ptr(scratch), _lib.ptr(summary),
                                              _lib.ptr(mask), _lib.current_stream()), "ramp_scene_summary")
        free_mask = mask.bool()
        rec = summary.cpu().numpy()                                                     # the one device-to-host copy
        out, b = [], 0
        for i in range(n_scenes):
            n_traj, n_free, ci, pl, sd, var = rec[i]
            out.append(SceneMetrics({'success': 1 if n_free > 0 else 0, 'collision_intensity': float(ci) * 100,
                                     'path_length': None if np.isnan(pl) else float(pl),
                                     'path_length_std': None if np.isnan(sd) else float(sd),
                                     'waypoint_variance': None if np.isnan(var) else float(var),
                                     'n_free_trajectories': int(n_free)}, trajs, free_mask, slice(b, b + counts[i])))
            b += counts[i]
        return out, free_mask


class Metrics3d(Metrics):
    """``Metrics`` over D = 3 positions (the first three state entries), with spheres beside the boxes and an optional swept
    (segment) test: the evaluation of the Maze3D experiments, whose boxes and spheres the reference's inference3d.py only plots.
    ``trajectory_success_and_metrics`` is inherited and runs on the 3-D path length and waypoint variance below."""

    @staticmethod
    def compute_collision_intensity(trajs, box_centers, box_sizes, sphere_centers=None, sphere_radii=None, swept=False, margin=0.0):
        """Fraction of the waypoints (``swept``: of the segments) of each trajectory that meet any box or sphere widened by ``margin``."""
        from .clearance import trajectory_clearance
        boxes = None if box_centers is None else (torch.as_tensor(box_centers), torch.as_tensor(box_sizes))
        spheres = None if sphere_centers is None else (torch.as_tensor(sphere_centers), torch.as_tensor(sphere_radii))
        r = trajectory_clearance(trajs, boxes, spheres, point_dim=3, margin=margin, swept=swept)
        return r.swept_intensity if swept else r.intensity

    @staticmethod
    def compute_path_length(trajectories):
        from .clearance import trajectory_clearance
        assert trajectories.ndim == 3
        if len(trajectories) == 0:
            return torch.tensor(0.0, device=trajectories.device)
        return trajectory_clearance(trajectories, point_dim=3, swept=False).path_length

    @staticmethod
    def compute_smoothness(trajs, trajs_vel=None):
        from .clearance import trajectory_clearance
        if trajs_vel is not None:                      # velocities given separately: pad three position columns
            assert trajs_vel.ndim == 3
            trajs = torch.cat([torch.zeros_like(trajs_vel[..., :1]).repeat(1, 1, 3), trajs_vel], dim=-1)
        return trajectory_clearance(trajs, point_dim=3, swept=False).smoothness

    @staticmethod
    def compute_variance_waypoints(trajs, eps=1e-8):
        """``Metrics.compute_variance_waypoints`` with the pairwise distance over three coordinates (ramp_scene_summary_nd on one
        scene whose rows are all free)."""
        t = _dev_traj(trajs)
        B, H, S = t.shape
        if B < 2:
            return torch.tensor(float("nan"), device=t.device)
        first = torch.tensor([0, B], dtype=torch.int32).to(t.device)
        zeros = torch.zeros(2, B, device=t.device)
        scratch = torch.empty(2 * H * ((B + 255) // 256 + 1) + 2, dtype=torch.float64, device=t.device)
        summary = torch.empty(1, 6, dtype=torch.float64, device=t.device)
        mask = torch.empty(B, dtype=torch.int32, device=t.device)
        with torch.cuda.device(t.device):
            _lib.check(_lib.load().ramp_scene_summary_nd(_lib.ptr(t), B, H, S, 3, first.data_ptr(), 1, zeros[0].data_ptr(),
                                                         zeros[1].data_ptr(), 0.0, _lib.ptr(scratch), _lib.ptr(summary), _lib.ptr(mask),
                                                         _lib.current_stream()), "ramp_scene_summary_nd")
        return summary[0, 5].to(torch.float32)

    @staticmethod
    def evaluate_scenes(trajs, counts_or_traj_scene, boxes_list, spheres_list=None, threshold: float = 0.01, swept: bool = True,
                        margin: float = 0.0):
        """``Metrics.evaluate_scenes`` for 3-D scenes of boxes and spheres: scene i's trajectories meet ``boxes_list[i]`` =
        ``(centers (n, 3), sizes (n, 3) or (n,))`` and ``spheres_list[i]`` = ``(centers (m, 3), radii (m,))`` (either may be None).
        ``swept``: a trajectory is free when the fraction of its SEGMENTS that meet a primitive is ``<= threshold``; otherwise the
        fraction of its waypoints, the reference's rule.

        Returns what ``Metrics.evaluate_scenes`` returns -- the same keys, ``SceneMetrics`` and (B) bool device free mask --, with
        ``collision_intensity`` the waypoint intensity in percent and one more key, ``swept_collision_intensity`` (percent; None with
        ``swept=False``).  Uploads first, then ramp_traj_clearance + ramp_scene_summary_nd; the call ends in its only
        device-to-host copy, the (n_scenes, 7) records."""
        from .clearance import trajectory_clearance
        t = _dev_traj(trajs)
        B, H, S = t.shape
        n_scenes = len(boxes_list)
        if spheres_list is not None and len(spheres_list) != n_scenes:
            raise ValueError(f"{n_scenes} box entries but {len(spheres_list)} sphere entries")
        counts = scene_counts(counts_or_traj_scene, n_scenes, B)
        dev = t.device
        r = trajectory_clearance(t, list(boxes_list), None if spheres_list is None else list(spheres_list), counts=counts,
                                 point_dim=3, margin=margin, swept=swept)
        first = r.traj_first
        decide = (r.swept_intensity if swept else r.intensity).contiguous()
        W = (B + 255) // 256 + n_scenes
        scratch = torch.empty(2 * H * W + n_scenes + 1, dtype=torch.float64, device=dev)
        summary = torch.empty(n_scenes, 6, dtype=torch.float64, device=dev)
        mask = torch.empty(B, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ramp_scene_summary_nd(_lib.ptr(t), B, H, S, 3, first.data_ptr(), n_scenes, _lib.ptr(decide),
                                                         _lib.ptr(r.path_length), float(threshold), _lib.ptr(scratch), _lib.ptr(summary),
                                                         _lib.ptr(mask), _lib.current_stream()), "ramp_scene_summary_nd")
        # the per-scene mean of the waypoint intensity (the record's own mean is of the deciding intensity): differences of a running sum
        run = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), r.intensity.to(torch.float64).cumsum(0)])
        idx = first.long()
        wp_mean = (run[idx[1:]] - run[idx[:-1]]) / (idx[1:] - idx[:-1]).to(torch.float64)
        free_mask = mask.bool()
        rec = torch.cat([summary, wp_mean[:, None]], dim=1).cpu().numpy()               # the one device-to-host copy
        out, b = [], 0
        for i in range(n_scenes):
            n_traj, n_free, ci, pl, sd, var, wp = rec[i]
            out.append(SceneMetrics({'success': 1 if n_free > 0 else 0, 'collision_intensity': float(wp) * 100,
                                     'swept_collision_intensity': float(ci) * 100 if swept else None,
                                     'path_length': None if np.isnan(pl) else float(pl),
                                     'path_length_std': None if np.isnan(sd) else float(sd),
                                     'waypoint_variance': None if np.isnan(var) else float(var),
                                     'n_free_trajectories': int(n_free)}, trajs, free_mask, slice(b, b + counts[i])))
            b += counts[i]
        return out, free_mask


class DynamicMetrics(Metrics):
    """metrics.py:128-170: host-side bookkeeping over the executed states of one pursuit-evasion episode."""

    def calculate_single_episode_metrics(self, chain_start: List, chain_obs: List, start_state_pos, goal_state_pos,
                                         goal_safe_threshold: float, static_collision: bool,
                                         pursuer_radius: float) -> Dict[str, Any]:
        goal = goal_state_pos.cpu().numpy() if torch.is_tensor(goal_state_pos) else goal_state_pos
        thr = pursuer_radius + 0.02
        capture = False
        for i in range(len(chain_obs)):
            if i + 2 >= len(chain_start):
                break
            if np.linalg.norm(chain_start[i + 2] - chain_obs[i]) <= thr:
                capture = True
                break
        captured = static_collision or capture
        reached = (np.linalg.norm(chain_start[-1] - goal) <= goal_safe_threshold) and not captured
        plen = 0
        for i in range(len(chain_start) - 1):
            plen += np.linalg.norm(chain_start[i + 1] - chain_start[i])
        return {'static_collision': static_collision, 'pursuer_capture': capture, 'captured': captured,
                'goal_reached': reached, 'path_length': plen if not captured else None,
                'score': 0.5 * float(reached) + 0.5 * float(not captured)}
