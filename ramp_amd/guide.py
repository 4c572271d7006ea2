"""Cost-gradient guidance on the HIP kernels: thin wrappers of ``ramp_guide_step`` / ``ramp_guide_cost`` and the cloud table that
``ramp_cost_guide`` carries (include/ramp_hip.h states the cost and one guide iteration).  Inside a sampling job the same kernel runs through
``cost_guide=`` of ``run_inference*`` (``ramp_amd.diffusion.guide_tables``, ``ramp_sample_guided``)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib

GUIDE_SCALARS = ('radius', 'w_obs', 'w_smooth', 'w_acc', 'max_norm')


def cloud_table(clouds: Sequence[torch.Tensor], device) -> tuple:
    """The scenes' clouds, each (P, d) or (No, Np, d) with the same d in {2, 3} (a scene may be empty), as ``ramp_cost_guide`` wants them:
    (device (sum P, d) float32 points or None when all are empty, host int32 (n_scenes + 1) offsets, d)."""
    if len(clouds) == 0:
        raise ValueError("cost guide: at least one cloud (an empty one is a (0, d) tensor)")
    flat = []
    for i, c in enumerate(clouds):
        c = torch.as_tensor(c)
        if c.dim() < 2 or c.shape[-1] not in (2, 3):
            raise ValueError(f"cost guide: cloud {i} must be (P, d) or (No, Np, d) with d = 2 or 3; got {tuple(c.shape)}")
        flat.append(c.reshape(-1, c.shape[-1]))
    d = int(flat[0].shape[1])
    if any(int(c.shape[1]) != d for c in flat):
        raise ValueError("cost guide: every cloud needs the same point dimension")
    off = np.zeros(len(flat) + 1, dtype=np.int32)
    off[1:] = np.cumsum([int(c.shape[0]) for c in flat])
    points = torch.cat([c.to(device, torch.float32) for c in flat]).contiguous() if off[-1] else None
    return points, off, d


def fill_cost_guide(points, offsets: np.ndarray, d: int, scalars: Dict[str, float]) -> _lib.RampCostGuide:
    """``ramp_cost_guide`` without its per-iteration tables; the caller keeps ``points`` and ``offsets`` alive for the call."""
    cg = _lib.RampCostGuide()
    cg.point_dim, cg.n_scenes = d, len(offsets) - 1
    cg.cloud_points = _lib.ptr(points)
    cg.cloud_offset_host = offsets.ctypes.data_as(_lib.c_i32p)
    for k in GUIDE_SCALARS:
        setattr(cg, k, float(scalars.get(k, 0.0)))
    return cg


def _as_clouds(cloud_or_clouds) -> list:
    return list(cloud_or_clouds) if isinstance(cloud_or_clouds, (list, tuple)) else [cloud_or_clouds]


def _scene_table(traj_scene, B: int, n_scenes: int, device) -> Optional[torch.Tensor]:
    if traj_scene is None:
        if n_scenes != 1:
            raise ValueError(f"{n_scenes} clouds need traj_scene, the (B,) scene of each trajectory")
        return None
    ts = torch.as_tensor(traj_scene).to(device, torch.int32).contiguous()
    if tuple(ts.shape) != (B,):
        raise ValueError(f"traj_scene must be ({B},); got {tuple(ts.shape)}")
    return ts


@torch.no_grad()
def cost_guide_step(x: torch.Tensor, cloud_or_clouds: Union[torch.Tensor, Sequence[torch.Tensor]], radius: float, step: float, w_obs: float = 1.0,
                    w_smooth: float = 0.0, w_acc: float = 0.0, n_steps: int = 1, max_norm: float = 0.0,
                    hard_conds: Optional[Dict[int, torch.Tensor]] = None, traj_scene=None) -> torch.Tensor:
    """``n_steps`` guide iterations (one launch, ``ramp_guide_step``) on a copy of the (B, H, S) trajectories ``x``.  ``cloud_or_clouds``: one
    cloud, or one per scene with ``traj_scene`` (B,) naming each trajectory's; ``hard_conds`` {waypoint: (S,) or (B, S)}: the pinned waypoints
    (negative indices count from the end, later entries win)."""
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    points, off, d = cloud_table(_as_clouds(cloud_or_clouds), dev)
    cg = fill_cost_guide(points, off, d, dict(radius=radius, w_obs=w_obs, w_smooth=w_smooth, w_acc=w_acc, max_norm=max_norm))
    ts = _scene_table(traj_scene, B, cg.n_scenes, dev)
    idx, val = None, None
    hard_conds = hard_conds or {}
    if hard_conds:
        idx = (C.c_int32 * len(hard_conds))(*[int(k) if k >= 0 else H + int(k) for k in hard_conds])
        vals = [torch.as_tensor(v).to(dev, torch.float32) for v in hard_conds.values()]
        val = torch.stack([v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v for v in vals]).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_step(_lib.ptr(out), B, H, S, C.byref(cg), _lib.ptr(ts), int(n_steps), float(step), len(hard_conds),
                                               C.cast(idx, _lib.c_i32p) if idx is not None else None, _lib.ptr(val), _lib.current_stream()),
                   "ramp_guide_step")
    return out


@torch.no_grad()
def cost_guide_terms(x: torch.Tensor, cloud_or_clouds: Union[torch.Tensor, Sequence[torch.Tensor]], radius: float, traj_scene=None) -> torch.Tensor:
    """(B, 3) float64 = the unweighted (C_obs, C_smooth, C_acc) of each trajectory (``ramp_guide_cost``), for ranking and diagnostics."""
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    B, H, S = xx.shape
    points, off, d = cloud_table(_as_clouds(cloud_or_clouds), dev)
    cg = fill_cost_guide(points, off, d, dict(radius=radius))
    ts = _scene_table(traj_scene, B, cg.n_scenes, dev)
    out = torch.empty((B, 3), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_cost(_lib.ptr(xx), B, H, S, C.byref(cg), _lib.ptr(ts), _lib.ptr(out), _lib.current_stream()),
                   "ramp_guide_cost")
    return out
