"""Cost-gradient guidance on the HIP kernels: thin wrappers of ``ramp_guide_step`` / ``ramp_guide_cost`` and the cloud table that
``ramp_cost_guide`` carries (include/ramp_hip.h states the cost and one guide iteration).  Inside a sampling job the same kernel runs through
``cost_guide=`` of ``run_inference*`` (``ramp_amd.diffusion.guide_tables``, ``ramp_sample_guided``).

The swept box and sphere terms that travel with that guide (``ramp_prim_guide``: a signed-distance hinge at ``n_sub`` samples per segment,
against the primitives ``ramp_amd.clearance`` evaluates): ``prim_table`` builds their device arrays and host offsets, ``prim_guide_step`` /
``prim_guide_terms`` wrap ``ramp_guide_step_prims`` / ``ramp_guide_cost_prims``; inside a job they are the ``boxes=`` / ``spheres=`` keys of
``cost_guide=`` (``ramp_sample_guided_prims``).

The replanning jobs have a guide of their own (``ramp_replan_guide``: a moving-cloud term with a per-waypoint track, per-episode pins):
``moving_guide_step`` / ``moving_guide_terms`` wrap its kernel-level entries, ``replan_guide_tables`` and ``predict_track`` are the host side of
``replan_guide=`` of the dynamic model's entry points."""
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


# ---------------------------------------------------------------------------------------------- swept box and sphere terms
PRIM_KEYS = ('boxes', 'spheres', 'margin', 'band', 'w_prim', 'n_sub')


def prim_table(boxes, spheres, n_scenes: int, point_dim: Optional[int], device) -> dict:
    """The scenes' boxes and spheres as ``ramp_prim_guide`` wants them.  ``boxes``: per scene a ``(centres (n, D), sizes (n, D) or (n,))`` pair
    or None, a single pair for one scene, or None; ``spheres`` likewise with ``(centres (n, D), radii (n,))`` -- the lists
    ``clearance.trajectory_clearance`` takes.  Returns ``{'D', 'n_scenes', 'box_centers', 'box_sizes', 'sphere_centers', 'sphere_radii'`` (device
    float32 or None when the table is empty), ``'box_offset', 'sphere_offset'`` (host int32 (n_scenes + 1)), ``'n_boxes', 'n_spheres'}``."""
    from .clearance import _f32, _per_scene
    bl, sl = _per_scene("boxes", boxes, True), _per_scene("spheres", spheres, True)
    for what, v in (("boxes", bl), ("spheres", sl)):
        if v is not None and len(v) != n_scenes:
            raise ValueError(f"cost guide {what}: {len(v)} entries for {n_scenes} scene(s)")
    D = point_dim
    for v in (bl, sl):
        e = next((e for e in (v or []) if e is not None), None)
        if e is not None and D is None:
            D = int(torch.as_tensor(e[0]).shape[-1])
    if D is None:
        raise ValueError("cost guide: point_dim cannot be inferred (no cloud, boxes or spheres were given)")
    D = int(D)
    if D not in (2, 3):
        raise ValueError(f"cost guide: primitives must be 2-D or 3-D; got {D}")
    bc, bs, sc, sr = [], [], [], []
    nb, ns = [0] * n_scenes, [0] * n_scenes
    for i in range(n_scenes):
        if bl is not None and bl[i] is not None:
            c, z = _f32(bl[i][0]), _f32(bl[i][1])
            if c.dim() < 1 or c.shape[-1] != D:
                raise ValueError(f"scene {i}: box centres must be (n, {D}); got shape {tuple(c.shape)}")
            c = c.reshape(-1, D)
            if z.dim() == 1:
                z = z.unsqueeze(-1).repeat(1, D)
            z = z.reshape(-1, D)
            if z.shape[0] != c.shape[0]:
                raise ValueError(f"scene {i}: {c.shape[0]} box centres but {z.shape[0]} box sizes")
            bc.append(c); bs.append(z); nb[i] = int(c.shape[0])
        if sl is not None and sl[i] is not None:
            c, r = _f32(sl[i][0]), _f32(sl[i][1]).reshape(-1)
            if c.dim() < 1 or c.shape[-1] != D:
                raise ValueError(f"scene {i}: sphere centres must be (n, {D}); got shape {tuple(c.shape)}")
            c = c.reshape(-1, D)
            if r.shape[0] != c.shape[0]:
                raise ValueError(f"scene {i}: {c.shape[0]} sphere centres but {r.shape[0]} radii")
            sc.append(c); sr.append(r); ns[i] = int(c.shape[0])
    for what, parts in (("box centres", bc), ("box sizes", bs), ("sphere centres", sc), ("sphere radii", sr)):
        if any(not bool(torch.isfinite(p).all()) for p in parts):
            raise ValueError(f"cost guide: non-finite {what}")
    if any(bool((p < 0).any()) for p in bs + sr):
        raise ValueError("cost guide: box sizes and sphere radii must not be negative")
    boff, soff = np.zeros(n_scenes + 1, np.int32), np.zeros(n_scenes + 1, np.int32)
    boff[1:], soff[1:] = np.cumsum(nb), np.cumsum(ns)

    def cat(parts):
        return torch.cat([p.to(device) for p in parts]).contiguous() if parts and sum(int(p.shape[0]) for p in parts) else None
    return dict(D=D, n_scenes=n_scenes, box_centers=cat(bc), box_sizes=cat(bs), sphere_centers=cat(sc), sphere_radii=cat(sr),
                box_offset=boff, sphere_offset=soff, n_boxes=int(boff[-1]), n_spheres=int(soff[-1]))


def prim_scalars(margin=0.0, band=None, w_prim=1.0, n_sub=4) -> dict:
    """margin, band, w_prim and n_sub of a primitive term, checked as the C entries check them."""
    if band is None:
        raise ValueError("cost guide: band= is required with boxes= / spheres=")
    out = dict(margin=float(margin), band=float(band), w_prim=float(w_prim), n_sub=int(n_sub))
    if not (np.isfinite(out['margin']) and out['margin'] >= 0 and np.isfinite(out['band']) and out['band'] >= 0):
        raise ValueError("cost guide: margin and band must be finite and not negative")
    if not np.isfinite(out['w_prim']):
        raise ValueError("cost guide: w_prim must be finite")
    if not 1 <= out['n_sub'] <= _lib.PRIM_GUIDE_MAX_SUB:
        raise ValueError(f"cost guide: n_sub outside 1 .. {_lib.PRIM_GUIDE_MAX_SUB}")
    return out


def fill_prim_guide(tab: dict, scalars: dict) -> _lib.RampPrimGuide:
    """``ramp_prim_guide`` from ``prim_table`` and ``prim_scalars``; the caller keeps ``tab`` alive for the call."""
    pg = _lib.RampPrimGuide()
    pg.point_dim, pg.n_scenes = tab['D'], tab['n_scenes']
    pg.box_centers, pg.box_sizes = _lib.ptr(tab['box_centers']), _lib.ptr(tab['box_sizes'])
    pg.sphere_centers, pg.sphere_radii = _lib.ptr(tab['sphere_centers']), _lib.ptr(tab['sphere_radii'])
    pg.box_offset_host = tab['box_offset'].ctypes.data_as(_lib.c_i32p)
    pg.sphere_offset_host = tab['sphere_offset'].ctypes.data_as(_lib.c_i32p)
    pg.margin, pg.band, pg.w_prim, pg.n_sub = scalars['margin'], scalars['band'], scalars['w_prim'], scalars['n_sub']
    return pg


def _prim_setup(x, cloud_or_clouds, boxes, spheres, radius, scalars, cost_scalars, traj_scene):
    """The two structs of a kernel-level call on x (B, H, S): clouds None = an empty cloud per scene of the primitive lists."""
    from .clearance import _per_scene
    dev = x.device
    B, H, S = x.shape
    lists = [v for v in (_per_scene("boxes", boxes, True), _per_scene("spheres", spheres, True)) if v is not None]
    n_scenes = len(_as_clouds(cloud_or_clouds)) if cloud_or_clouds is not None else (len(lists[0]) if lists else 1)
    d = None if cloud_or_clouds is None else int(torch.as_tensor(_as_clouds(cloud_or_clouds)[0]).shape[-1])
    tab = prim_table(boxes, spheres, n_scenes, d, dev)
    clouds = _as_clouds(cloud_or_clouds) if cloud_or_clouds is not None else [torch.zeros(0, tab['D'])] * n_scenes
    points, off, d = cloud_table(clouds, dev)
    if d != tab['D']:
        raise ValueError(f"cost guide: {d}-D cloud points with {tab['D']}-D primitives")
    cg = fill_cost_guide(points, off, d, dict(cost_scalars, radius=radius))
    pg = fill_prim_guide(tab, scalars)
    ts = _scene_table(traj_scene, B, cg.n_scenes, dev)
    return cg, pg, ts, (points, off, tab)


@torch.no_grad()
def prim_guide_step(x: torch.Tensor, boxes=None, spheres=None, *, band: float, step: float, margin: float = 0.0, w_prim: float = 1.0,
                    n_sub: int = 4, cloud_or_clouds=None, radius: float = 0.0, w_obs: float = 0.0, w_smooth: float = 0.0, w_acc: float = 0.0,
                    n_steps: int = 1, max_norm: float = 0.0, hard_conds: Optional[Dict[int, torch.Tensor]] = None, traj_scene=None) -> torch.Tensor:
    """``n_steps`` guide iterations with the swept box and sphere terms (one launch, ``ramp_guide_step_prims``) on a copy of the (B, H, S)
    trajectories ``x``.  ``boxes`` / ``spheres``: a ``(centres, sizes)`` / ``(centres, radii)`` pair, or one per scene (None = the scene has
    none) with ``traj_scene`` (B,); ``cloud_or_clouds``, ``radius`` and ``w_obs`` add ``cost_guide_step``'s cloud term (default: none);
    ``hard_conds`` as there."""
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    cg, pg, ts, keep = _prim_setup(out, cloud_or_clouds, boxes, spheres, radius, prim_scalars(margin, band, w_prim, n_sub),
                                   dict(w_obs=w_obs, w_smooth=w_smooth, w_acc=w_acc, max_norm=max_norm), traj_scene)
    idx, val = None, None
    hard_conds = hard_conds or {}
    if hard_conds:
        idx = (C.c_int32 * len(hard_conds))(*[int(k) if k >= 0 else H + int(k) for k in hard_conds])
        vals = [torch.as_tensor(v).to(dev, torch.float32) for v in hard_conds.values()]
        val = torch.stack([v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v for v in vals]).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_step_prims(_lib.ptr(out), B, H, S, C.byref(cg), C.byref(pg), _lib.ptr(ts), int(n_steps), float(step),
                                                     len(hard_conds), C.cast(idx, _lib.c_i32p) if idx is not None else None, _lib.ptr(val),
                                                     _lib.current_stream()), "ramp_guide_step_prims")
    return out


@torch.no_grad()
def prim_guide_terms(x: torch.Tensor, boxes=None, spheres=None, *, band: float, margin: float = 0.0, n_sub: int = 4, cloud_or_clouds=None,
                     radius: float = 0.0, traj_scene=None) -> torch.Tensor:
    """(B, 4) float64 = the unweighted (C_obs, C_smooth, C_acc, C_prim) of each trajectory (``ramp_guide_cost_prims``)."""
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    B, H, S = xx.shape
    cg, pg, ts, keep = _prim_setup(xx, cloud_or_clouds, boxes, spheres, radius, prim_scalars(margin, band, 1.0, n_sub), {}, traj_scene)
    out = torch.empty((B, 4), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_cost_prims(_lib.ptr(xx), B, H, S, C.byref(cg), C.byref(pg), _lib.ptr(ts), _lib.ptr(out),
                                                     _lib.current_stream()), "ramp_guide_cost_prims")
    return out


# ---------------------------------------------------------------------------------------------- the replanning jobs' guide
REPLAN_GUIDE_SCALARS = ('radius', 'radius_mov', 'w_obs', 'w_mov', 'w_smooth', 'w_acc', 'max_norm')
REPLAN_GUIDE_KEYS = ('radius', 'step', 'radius_moving', 'w_obs', 'w_moving', 'w_smooth', 'w_acc', 'max_norm', 'n_steps', 't_start', 'cloud', 'predict')
PREDICTORS = ('hold', 'constant_velocity')


def replan_guide_tables(g, low_steps: Sequence[int]) -> dict:
    """``replan_guide=`` checked and expanded over the low-level DDIM steps ``low_steps`` of a replan: the seven scalars, ``n_guide`` /
    ``step`` per DDIM step (``n_steps`` iterations on the steps with ``t < t_start``; the default ``t_start = 1`` guides the last step only),
    ``total``, ``predict`` and ``cloud``."""
    if not isinstance(g, dict):
        raise TypeError(f"replan_guide= takes a dict; got {type(g).__name__}")
    unknown = sorted(set(g) - set(REPLAN_GUIDE_KEYS))
    if unknown:
        raise ValueError(f"replan_guide=: unknown keys {unknown}; known: {list(REPLAN_GUIDE_KEYS)}")
    for k in ('radius', 'step'):
        if g.get(k) is None:
            raise ValueError(f"replan_guide=: {k}= is required")
    tab = dict(radius=float(g['radius']), radius_mov=float(g.get('radius_moving', g['radius'])), w_obs=float(g.get('w_obs', 1.0)),
               w_mov=float(g.get('w_moving', 1.0)), w_smooth=float(g.get('w_smooth', 0.0)), w_acc=float(g.get('w_acc', 0.0)),
               max_norm=float(g.get('max_norm', 0.0)))
    step, n_steps, t_start = float(g['step']), int(g.get('n_steps', 1)), float(g.get('t_start', 1))
    if not all(np.isfinite(v) for v in tab.values()) or not np.isfinite(step):
        raise ValueError("replan_guide=: the scalars and step must be finite")
    if (tab['w_obs'] != 0 and tab['radius'] <= 0) or (tab['w_mov'] != 0 and tab['radius_mov'] <= 0):
        raise ValueError("replan_guide=: radius (radius_moving) must be positive where w_obs (w_moving) is not 0")
    if not 0 <= n_steps <= _lib.GUIDE_MAX_STEPS:
        raise ValueError(f"replan_guide=: n_steps outside 0 .. {_lib.GUIDE_MAX_STEPS}")
    if np.isnan(t_start):
        raise ValueError("replan_guide=: t_start must not be NaN")
    predict = g.get('predict', 'constant_velocity')
    if not callable(predict) and predict not in PREDICTORS:
        raise ValueError(f"replan_guide=: unknown predict {predict!r}; known: {list(PREDICTORS)} or a callable")
    tab['n_guide'] = [n_steps if t < t_start else 0 for t in low_steps]
    tab['step'] = [step] * len(low_steps)
    tab['total'] = sum(tab['n_guide'])
    tab['predict'], tab['cloud'] = predict, g.get('cloud')
    return tab


def predict_track(predict, centre_now, centre_prev, plan_xy, stepp: int) -> np.ndarray:
    """The track (H, 2) float32 of a moving cloud: its displacement at waypoint h of the plan ``plan_xy`` (H, 2) whose waypoint ``stepp`` is now.
    'hold': zeros.  'constant_velocity': max(0, h - stepp) (centre_now - centre_prev), zeros without a previous centre (an episode's first
    replan).  A callable ``(centre_now, centre_prev or None, plan_xy, stepp) -> (H, 2)``.  Draws no random numbers."""
    H = int(np.asarray(plan_xy).shape[0])
    if callable(predict):
        tr = np.asarray(predict(centre_now, centre_prev, plan_xy, stepp))
        if tr.shape != (H, 2):
            raise ValueError(f"replan_guide=: predict returned shape {tuple(tr.shape)}; wanted ({H}, 2)")
        if not np.isfinite(tr).all():
            raise ValueError("replan_guide=: predict returned non-finite displacements")
        return np.ascontiguousarray(tr, np.float32)
    if predict == 'hold' or (predict == 'constant_velocity' and centre_prev is None):
        return np.zeros((H, 2), np.float32)
    if predict != 'constant_velocity':
        raise ValueError(f"replan_guide=: unknown predict {predict!r}; known: {list(PREDICTORS)} or a callable")
    v = np.asarray(centre_now, np.float64)[:2] - np.asarray(centre_prev, np.float64)[:2]
    ahead = np.maximum(0, np.arange(H) - int(stepp)).astype(np.float64)
    return np.ascontiguousarray(ahead[:, None] * v[None, :], np.float32)


def fill_replan_guide(points, offsets: np.ndarray, moving: Optional[np.ndarray], track: Optional[np.ndarray],
                      scalars: Dict[str, float]) -> _lib.RampReplanGuide:
    """``ramp_replan_guide`` without its per-step tables and tap: ``points`` device (sum P, 2) or None, ``offsets`` host int32
    (n_scenes + 1), ``moving`` host float32 (n_scenes, n_mov, 2) or None, ``track`` host float32 (n_scenes, H, 2) or None; the caller keeps all
    four alive for the call."""
    rg = _lib.RampReplanGuide()
    rg.n_scenes = len(offsets) - 1
    rg.n_mov = 0 if moving is None else int(moving.shape[1])
    rg.cloud_points = _lib.ptr(points)
    rg.cloud_offset_host = offsets.ctypes.data_as(_lib.c_i32p)
    if rg.n_mov:
        assert moving.dtype == np.float32 and track.dtype == np.float32 and moving.flags.c_contiguous and track.flags.c_contiguous
        assert moving.shape[0] == rg.n_scenes and track.shape[0] == rg.n_scenes
        rg.mov_points_host = moving.ctypes.data_as(_lib.c_f32p)
        rg.mov_track_host = track.ctypes.data_as(_lib.c_f32p)
    for k in REPLAN_GUIDE_SCALARS:
        setattr(rg, k, float(scalars.get(k, 0.0)))
    return rg


def _moving_tables(clouds, moving, track, H: int, dev):
    points, off, d = cloud_table(clouds, dev)
    if d != 2:
        raise ValueError("moving guide: the replanning jobs are 2-D; every cloud must be (P, 2)")
    n_scenes = len(off) - 1
    mv = tr = None
    if moving is not None:
        mv = np.ascontiguousarray(torch.as_tensor(moving).detach().cpu().numpy(), np.float32)
        mv = mv[None] if mv.ndim == 2 else mv
        if mv.ndim != 3 or mv.shape[0] != n_scenes or mv.shape[2] != 2:
            raise ValueError(f"moving guide: moving must be ({n_scenes}, M, 2); got {tuple(mv.shape)}")
        if mv.shape[1] == 0:
            mv = None
    if mv is not None:
        tr = np.zeros((n_scenes, H, 2), np.float32) if track is None else np.ascontiguousarray(torch.as_tensor(track).detach().cpu().numpy(), np.float32)
        tr = tr[None] if tr.ndim == 2 else tr
        if tr.shape != (n_scenes, H, 2):
            raise ValueError(f"moving guide: track must be ({n_scenes}, {H}, 2); got {tuple(tr.shape)}")
    return points, off, mv, tr


@torch.no_grad()
def moving_guide_step(x: torch.Tensor, cloud_or_clouds, moving, track, radius: float, step: float, radius_moving: Optional[float] = None,
                      w_obs: float = 1.0, w_moving: float = 1.0, w_smooth: float = 0.0, w_acc: float = 0.0, n_steps: int = 1,
                      max_norm: float = 0.0, hard_conds: Optional[Dict[int, torch.Tensor]] = None, traj_scene=None, pin_first=None) -> torch.Tensor:
    """``n_steps`` iterations of the replans' guide (one launch, ``ramp_guide_step_moving``) on a copy of the (B, H, S) rows ``x``.
    ``cloud_or_clouds``: one static (P, 2) cloud or one per scene with ``traj_scene`` (B,); ``moving`` (n_scenes, M, 2) (or (M, 2) for one
    scene, None = no moving term) the moving clouds now, ``track`` (n_scenes, H, 2) their displacement per waypoint (None = zeros).
    ``pin_first`` (B,) int: waypoints below it and waypoint H - 1 are pinned, with those of ``hard_conds`` (whose values win in the working
    copy; later entries win)."""
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    points, off, mv, tr = _moving_tables(_as_clouds(cloud_or_clouds), moving, track, H, dev)
    rg = fill_replan_guide(points, off, mv, tr, dict(radius=radius, radius_mov=radius if radius_moving is None else radius_moving, w_obs=w_obs,
                                                     w_mov=w_moving, w_smooth=w_smooth, w_acc=w_acc, max_norm=max_norm))
    ts = _scene_table(traj_scene, B, rg.n_scenes, dev)
    pf = None
    if pin_first is not None:
        pf = torch.as_tensor(pin_first).to(dev, torch.int32).contiguous()
        if tuple(pf.shape) != (B,):
            raise ValueError(f"pin_first must be ({B},); got {tuple(pf.shape)}")
    idx, val = None, None
    hard_conds = hard_conds or {}
    if hard_conds:
        idx = (C.c_int32 * len(hard_conds))(*[int(k) if k >= 0 else H + int(k) for k in hard_conds])
        vals = [torch.as_tensor(v).to(dev, torch.float32) for v in hard_conds.values()]
        val = torch.stack([v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v for v in vals]).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_step_moving(_lib.ptr(out), B, H, S, C.byref(rg), _lib.ptr(ts), _lib.ptr(pf), int(n_steps), float(step),
                                                      len(hard_conds), C.cast(idx, _lib.c_i32p) if idx is not None else None, _lib.ptr(val),
                                                      _lib.current_stream()), "ramp_guide_step_moving")
    return out


@torch.no_grad()
def moving_guide_terms(x: torch.Tensor, cloud_or_clouds, moving, track, radius: float, radius_moving: Optional[float] = None,
                       traj_scene=None) -> torch.Tensor:
    """(B, 4) float64 = the unweighted (C_obs, C_mov, C_smooth, C_acc) of each row (``ramp_guide_cost_moving``)."""
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    B, H, S = xx.shape
    points, off, mv, tr = _moving_tables(_as_clouds(cloud_or_clouds), moving, track, H, dev)
    rg = fill_replan_guide(points, off, mv, tr, dict(radius=radius, radius_mov=radius if radius_moving is None else radius_moving))
    ts = _scene_table(traj_scene, B, rg.n_scenes, dev)
    out = torch.empty((B, 4), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_guide_cost_moving(_lib.ptr(xx), B, H, S, C.byref(rg), _lib.ptr(ts), _lib.ptr(out), _lib.current_stream()),
                   "ramp_guide_cost_moving")
    return out
