"""Teams of robots in one job, on the HIP kernels (``ramp_team_guide`` and ``ramp_team_clearance`` in include/ramp_hip.h state the team term,
the Jacobi iteration and the swept check).

Several robots that share a scene are sampled in ONE batch with the single-robot model: row ``b`` of the job is agent ``b % A`` of team
``b // A``, a team's rows are adjacent and belong to one scene.  The rows know about each other only through the separation term of the
cost guide (``cost_guide=dict(..., team=dict(size=A, radius=r, w=1.0))`` of ``run_inference*``); afterwards ``team_clearance`` checks every
team for conflicts between its members, waypoints and the synchronous segments between them, and
``ramp_amd.cost.select_best_teams_scenes`` picks the best conflict-free team of every scene.

  team_hard_conds        the per-row start / goal conditions of ``n_teams`` teams in team layout
  run_inference_teams    ``run_inference_scenes`` for teams: ``(n_teams_total, A, H, S)`` and the ``team_first`` table
  team_guide_step / team_guide_terms   the kernels alone, the counterparts of ``guide.cost_guide_step`` / ``guide.cost_guide_terms``
  team_clearance         separations, conflict counts and the team-level arrays the selection reads

No claim is made about plan quality: the guide moves what the network proposes, it trains nothing."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .guide import _as_clouds, _scene_table, cloud_table, fill_cost_guide

TEAM_KEYS = {'size', 'radius', 'w'}


def team_scalars(team: dict) -> dict:
    """``team=dict(size=A, radius=r_t, w=1.0)`` of ``cost_guide=``, validated on the host: ``{'size', 'radius', 'w'}``."""
    if not isinstance(team, dict):
        raise TypeError("team= takes a dict(size=, radius=, w=)")
    unknown = set(team) - TEAM_KEYS
    if unknown:
        raise ValueError(f"team=: unknown keys {sorted(unknown)}")
    if 'size' not in team:
        raise ValueError("team=: size= is required")
    size = int(team['size'])
    if size != team['size'] or not 1 <= size <= _lib.TEAM_MAX:
        raise ValueError(f"team=: size must be an integer in 1 .. {_lib.TEAM_MAX}; got {team['size']}")
    w = float(team.get('w', 1.0))
    if not np.isfinite(w):
        raise ValueError("team=: w must be finite")
    radius = float(team.get('radius', 0.0))
    if w != 0.0 and not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("team=: radius must be positive and finite where w != 0")
    return {'size': size, 'radius': radius, 'w': w}


def fill_team_guide(tab: dict) -> _lib.RampTeamGuide:
    """``ramp_team_guide`` from the table of ``team_scalars``."""
    tg = _lib.RampTeamGuide()
    tg.team_size, tg.radius_team, tg.w_team = int(tab['size']), float(tab['radius']), float(tab['w'])
    return tg


def team_hard_conds(starts, goals, n_teams: int) -> Dict[int, torch.Tensor]:
    """``{0: (n_teams * A, S), -1: (n_teams * A, S)}``: the agents' start states ``starts`` (A, S) and goal states ``goals`` (A, S) repeated
    for ``n_teams`` teams in team layout (row ``k * A + a`` is agent ``a`` of team ``k``)."""
    starts, goals = torch.as_tensor(starts, dtype=torch.float32), torch.as_tensor(goals, dtype=torch.float32)
    if starts.dim() != 2 or starts.shape != goals.shape:
        raise ValueError(f"team_hard_conds: starts and goals must both be (A, S); got {tuple(starts.shape)} and {tuple(goals.shape)}")
    if not 1 <= starts.shape[0] <= _lib.TEAM_MAX:
        raise ValueError(f"team_hard_conds: 1 .. {_lib.TEAM_MAX} agents; got {starts.shape[0]}")
    if int(n_teams) < 1:
        raise ValueError("team_hard_conds: at least one team")
    return {0: starts.repeat(int(n_teams), 1).contiguous(), -1: goals.repeat(int(n_teams), 1).contiguous()}


def _hard_arrays(hard_conds, B: int, H: int, dev):
    idx, val = None, None
    if hard_conds:
        idx = (C.c_int32 * len(hard_conds))(*[int(k) if k >= 0 else H + int(k) for k in hard_conds])
        vals = [torch.as_tensor(v).to(dev, torch.float32) for v in hard_conds.values()]
        val = torch.stack([v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v for v in vals]).contiguous()
    return idx, val


@torch.no_grad()
def team_guide_step(x: torch.Tensor, cloud_or_clouds: Union[torch.Tensor, Sequence[torch.Tensor]], size: int, radius_team: float, radius: float,
                    step: float, w_team: float = 1.0, w_obs: float = 1.0, w_smooth: float = 0.0, w_acc: float = 0.0, n_steps: int = 1,
                    max_norm: float = 0.0, hard_conds: Optional[Dict[int, torch.Tensor]] = None, traj_scene=None) -> torch.Tensor:
    """``n_steps`` Jacobi iterations of the guide with the team term (one launch, ``ramp_guide_step_team``) on a copy of the (B, H, S) rows
    ``x`` in team layout, teams of ``size``.  The other arguments are ``guide.cost_guide_step``'s; ``size=None`` hands over no team table."""
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    points, off, d = cloud_table(_as_clouds(cloud_or_clouds), dev)
    cg = fill_cost_guide(points, off, d, dict(radius=radius, w_obs=w_obs, w_smooth=w_smooth, w_acc=w_acc, max_norm=max_norm))
    tg = None if size is None else fill_team_guide(dict(size=size, radius=radius_team, w=w_team))
    ts = _scene_table(traj_scene, B, cg.n_scenes, dev)
    hard_conds = hard_conds or {}
    idx, val = _hard_arrays(hard_conds, B, H, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_step_team(_lib.ptr(out), B, H, S, C.byref(cg), C.byref(tg) if tg is not None else None, _lib.ptr(ts),
                                                    int(n_steps), float(step), len(hard_conds),
                                                    C.cast(idx, _lib.c_i32p) if idx is not None else None, _lib.ptr(val), _lib.current_stream()),
                   "ramp_guide_step_team")
    return out


@torch.no_grad()
def team_guide_terms(x: torch.Tensor, cloud_or_clouds: Union[torch.Tensor, Sequence[torch.Tensor]], size: int, radius_team: float, radius: float,
                     traj_scene=None) -> torch.Tensor:
    """(B, 4) float64 = the unweighted (C_obs, C_smooth, C_acc, the row's share of C_team) of each row (``ramp_guide_cost_team``); a team's
    C_team is half the sum of its rows' last column."""
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    B, H, S = xx.shape
    points, off, d = cloud_table(_as_clouds(cloud_or_clouds), dev)
    cg = fill_cost_guide(points, off, d, dict(radius=radius))
    tg = None if size is None else fill_team_guide(dict(size=size, radius=radius_team, w=1.0))
    ts = _scene_table(traj_scene, B, cg.n_scenes, dev)
    out = torch.empty((B, 4), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_cost_team(_lib.ptr(xx), B, H, S, C.byref(cg), C.byref(tg) if tg is not None else None, _lib.ptr(ts),
                                                    _lib.ptr(out), _lib.current_stream()), "ramp_guide_cost_team")
    return out


@torch.no_grad()
def team_clearance(x: torch.Tensor, size: int, min_sep: float, point_dim: int = 2, swept: bool = True, row_mask=None, row_len=None,
                   row_smooth=None) -> dict:
    """The joint check of the teams of ``size`` in the (B, H, S) rows ``x`` (``ramp_team_clearance``, one launch, no host sync): a dict of
    device tensors over the B / size teams -- ``sep_wp``, ``sep_seg`` (float32), ``wp_conflicts``, ``seg_conflicts`` (int32) and the
    team-level arrays of the selection, ``team_mask`` (int32; 1 = a member collides or the team has a conflict, by segments with ``swept``,
    by waypoints without), ``team_len``, ``team_smooth`` (the members' ``row_len`` / ``row_smooth`` added in agent order; zeros without)."""
    if x.device.type != "cuda":
        raise _lib.RampHipError("team clearance: tensors must live on a HIP device (no CPU path)")
    t = x.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    size = int(size)
    if not 1 <= size <= _lib.TEAM_MAX or B % size:
        raise ValueError(f"team clearance: team size must lie in 1 .. {_lib.TEAM_MAX} and divide the {B} rows; got {size}")
    dev = t.device
    n = B // size

    def row(v, dtype, name):
        if v is None:
            return None
        v = torch.as_tensor(v).to(dev)
        v = (v != 0).to(torch.int32) if dtype is torch.int32 else v.to(dtype)
        if tuple(v.shape) != (B,):
            raise ValueError(f"team clearance: {name} must be ({B},); got {tuple(v.shape)}")
        return v.contiguous()

    rm, rl, rs = row(row_mask, torch.int32, "row_mask"), row(row_len, torch.float32, "row_len"), row(row_smooth, torch.float32, "row_smooth")
    f = [torch.empty(n, device=dev, dtype=torch.float32) for _ in range(4)]
    i = [torch.empty(n, device=dev, dtype=torch.int32) for _ in range(3)]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_team_clearance(_lib.ptr(t), B, H, S, int(point_dim), size, float(min_sep), int(bool(swept)), _lib.ptr(rm),
                                                   _lib.ptr(rl), _lib.ptr(rs), _lib.ptr(f[0]), _lib.ptr(f[1]), _lib.ptr(i[0]), _lib.ptr(i[1]),
                                                   _lib.ptr(i[2]), _lib.ptr(f[2]), _lib.ptr(f[3]), _lib.current_stream()), "ramp_team_clearance")
    return {'sep_wp': f[0], 'sep_seg': f[1], 'wp_conflicts': i[0], 'seg_conflicts': i[1], 'team_mask': i[2], 'team_len': f[2], 'team_smooth': f[3]}


@torch.no_grad()
def run_inference_teams(dm, scenes, starts, goals, n_teams, cost_guide: dict, **kw):
    """Teams of robots in many scenes as ONE job, built on ``dm.run_inference_scenes``: ``starts[i]`` / ``goals[i]`` are scene i's (A, S) start
    and goal states, ``n_teams`` an int or one count per scene, ``cost_guide`` carries ``team=dict(size=A, ...)`` and one cloud per scene.
    Returns ``(teams, team_first)``: the plans as (sum n_teams, A, H, S) -- (steps + 1, sum n_teams, A, H, S) with ``return_chain`` -- and the
    host int32 (n_scenes + 1) table of every scene's first team."""
    from .diffusion import guide_has_team
    if not guide_has_team(cost_guide):
        raise ValueError("run_inference_teams: cost_guide= needs team=dict(size=, radius=, w=)")
    A = team_scalars(cost_guide['team'])['size']
    n_scenes = len(scenes)
    counts = [int(n_teams)] * n_scenes if np.isscalar(n_teams) else [int(n) for n in n_teams]
    if len(counts) != n_scenes or len(starts) != n_scenes or len(goals) != n_scenes:
        raise ValueError(f"run_inference_teams: {n_scenes} scenes need as many starts, goals and team counts")
    hcs = []
    for i in range(n_scenes):
        hc = team_hard_conds(starts[i], goals[i], counts[i])
        if hc[0].shape[0] != counts[i] * A:
            raise ValueError(f"run_inference_teams: scene {i} has {hc[0].shape[0] // counts[i]} start states for teams of {A}")
        hcs.append(hc)
    res, _traj_scene = dm.run_inference_scenes(scenes, hcs, n_samples=[n * A for n in counts], cost_guide=cost_guide, **kw)
    team_first = np.zeros(n_scenes + 1, dtype=np.int32)
    team_first[1:] = np.cumsum(counts)
    H, S = res.shape[-2:]
    return res.reshape(*res.shape[:-3], int(team_first[-1]), A, H, S), team_first
