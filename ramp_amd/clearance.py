"""Swept collision checks and clearances of a batch of trajectories, 2-D or 3-D, on the HIP kernel (``ramp_traj_clearance``):
waypoints AND the segments between them against the boxes, spheres and cloud points of each trajectory's own scene.  The reference
tests waypoints only (metrics.py:49-82, cost.py:25-54); the definitions are those of include/ramp_hip.h."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .scenes import build_clearance_tables, scene_counts


def _is_array(v) -> bool:
    return hasattr(v, "shape")


def _per_scene(what, v, pair: bool):
    """None, one entry or a list of per-scene entries -> list of per-scene entries (None = the scene has none)."""
    if v is None:
        return None
    if pair:
        if len(v) == 2 and _is_array(v[0]) and _is_array(v[1]):
            return [v]
    elif _is_array(v):
        return [v]
    out = list(v)
    for i, e in enumerate(out):
        if e is not None and pair and not (len(e) == 2 and _is_array(e[0]) and _is_array(e[1])):
            raise ValueError(f"{what}: scene {i} must be a pair of arrays or None")
        if e is not None and not pair and not _is_array(e):
            raise ValueError(f"{what}: scene {i} must be an array or None")
    return out


def _f32(v):
    return torch.as_tensor(v).detach().to(torch.float32)


class Clearance:
    """What ``trajectory_clearance`` returns: device tensors of (B) entries, nothing copied to the host.

    ``wp_hits`` / ``seg_hits`` int32 counts of waypoints / segments that meet a box or sphere, ``clearance`` / ``swept_clearance`` the
    distance of the waypoints / segments to the nearest cloud point (+inf without a cloud), ``path_length``, ``smoothness``;
    ``seg_hits`` and ``swept_clearance`` are None when the call skipped the segment work (``swept=False``)."""

    def __init__(self, H, wp_hits, seg_hits, clearance, swept_clearance, path_length, smoothness, traj_first=None, point_dim=None):
        self.H, self.wp_hits, self.seg_hits = H, wp_hits, seg_hits
        self.point_dim = point_dim                            # the position entries the call used (2 or 3)
        self.traj_first = traj_first                          # device int32 (n_scenes + 1): first row of each scene
        self.clearance, self.swept_clearance, self.path_length, self.smoothness = clearance, swept_clearance, path_length, smoothness

    @staticmethod
    def _fraction(hits, n):
        # a tensor / tensor division: dividing by a Python number multiplies by its rounded reciprocal, one ulp off ramp_traj_metrics's
        # hits / (float)H for some counts (10 / 48)
        h = hits.to(torch.float32)
        return h / torch.full_like(h, float(n))

    @property
    def intensity(self):
        return self._fraction(self.wp_hits, self.H)

    @property
    def swept_intensity(self):
        if self.seg_hits is None:
            raise ValueError("the segment work was skipped (swept=False): there is no swept intensity")
        return self._fraction(self.seg_hits, self.H - 1)

    def colliding(self, intensity_threshold=0.0, cloud_threshold=0.0, swept=True):
        """(B) bool: primitive intensity ``> intensity_threshold`` or cloud clearance ``< cloud_threshold`` (strict, cost.py:45-49); a
        row with a non-finite position (NaN clearance) always collides."""
        inten = self.swept_intensity if swept else self.intensity
        clear = self.swept_clearance if swept else self.clearance
        return (inten > intensity_threshold) | (clear < cloud_threshold) | torch.isnan(clear)

    def free(self, threshold=0.01, cloud_threshold=0.0, swept=True):
        """(B) bool: intensity ``<= threshold`` (Metrics' rule) and clearance not below ``cloud_threshold``."""
        return ~self.colliding(threshold, cloud_threshold, swept)


def trajectory_clearance(trajs, boxes=None, spheres=None, clouds=None, counts=None, *, point_dim=None, margin=0.0, swept=True):
    """Waypoint and swept (segment) collision counts, cloud clearances, path length and smoothness of every trajectory, in one launch.

    trajs    (B, H, S) device tensor, 2 <= H <= 128; positions are the first ``point_dim`` state entries
    boxes    ``(centers, sizes)`` or a list of such pairs, one per scene (None = the scene has no box); centers (n, D), sizes (n, D)
             or (n,) full side lengths, as ``Metrics.compute_collision_intensity`` takes them
    spheres  ``(centers, radii)`` or a list per scene; clouds: (..., D) points or a list per scene
             (single entries must be tensors or numpy arrays, so that a pair is told from a list of scenes)
    counts   trajectories per scene or the (B) scene of each trajectory, as in ``scene_counts``; default: one scene
    point_dim  2 or 3; default: the last axis of what was given
    margin   the robot's radius: boxes and spheres grow by it
    swept    False skips the segment work

    All uploads come first -- one concatenated primitive buffer and one int32 table buffer (primitives that already live on the
    device are concatenated there instead) -- then one launch.  Returns a ``Clearance`` of device tensors, without a host sync."""
    if trajs.device.type != "cuda":
        raise _lib.RampHipError("trajectory clearance: tensors must live on a HIP device (no CPU path)")
    if trajs.ndim != 3:
        raise ValueError(f"trajs must be (B, H, S); got shape {tuple(trajs.shape)}")
    t = trajs.detach().to(torch.float32).contiguous()
    B, H, S = t.shape
    bl, sl, cl = _per_scene("boxes", boxes, True), _per_scene("spheres", spheres, True), _per_scene("clouds", clouds, False)
    given = [len(v) for v in (bl, sl, cl) if v is not None]
    n_scenes = given[0] if given else 1
    if not given:
        counts = None                                         # no primitive anywhere: the scenes make no difference
    if any(n != n_scenes for n in given):
        raise ValueError(f"boxes, spheres and clouds must list the same number of scenes; got {given}")
    if point_dim is None:
        for v, last in ((bl, lambda e: e[0]), (sl, lambda e: e[0]), (cl, lambda e: e)):
            e = next((e for e in (v or []) if e is not None), None)
            if e is not None and point_dim is None:
                point_dim = int(last(e).shape[-1])
        if point_dim is None:
            raise ValueError("point_dim cannot be inferred: no boxes, spheres or clouds were given")
    D = int(point_dim)
    if D not in (2, 3) or D > S:
        raise ValueError(f"point_dim must be 2 or 3 and at most the state width {S}; got {D}")
    cnt = scene_counts([B] if counts is None else counts, n_scenes, B)

    bc, bs, sc, sr, pts = [], [], [], [], []
    nb, ns, npts = [0] * n_scenes, [0] * n_scenes, [0] * n_scenes
    for i in range(n_scenes):
        if bl is not None and bl[i] is not None:
            c, z = _f32(bl[i][0]).reshape(-1, D), _f32(bl[i][1])
            if z.dim() == 1:
                z = z.unsqueeze(-1).repeat(1, D)
            z = z.reshape(-1, D)
            if z.shape[0] != c.shape[0]:
                raise ValueError(f"scene {i}: {c.shape[0]} box centres but {z.shape[0]} box sizes")
            bc.append(c); bs.append(z); nb[i] = c.shape[0]
        if sl is not None and sl[i] is not None:
            c, r = _f32(sl[i][0]).reshape(-1, D), _f32(sl[i][1]).reshape(-1)
            if r.shape[0] != c.shape[0]:
                raise ValueError(f"scene {i}: {c.shape[0]} sphere centres but {r.shape[0]} radii")
            sc.append(c); sr.append(r); ns[i] = c.shape[0]
        if cl is not None and cl[i] is not None:
            p = _f32(cl[i])
            if p.dim() < 1 or p.shape[-1] != D:
                raise ValueError(f"scene {i}: cloud points must be (..., {D}); got shape {tuple(p.shape)}")
            p = p.reshape(-1, D)
            pts.append(p); npts[i] = p.shape[0]
    tab = build_clearance_tables(cnt, nb, ns, npts)
    dev = t.device
    pieces = [p.reshape(-1) for p in bc + bs + sc + sr + pts]
    if not pieces:
        prim = torch.zeros(1, device=dev)
    elif all(p.device.type == "cpu" for p in pieces):
        prim = torch.cat(pieces).to(dev)                      # one upload
    else:
        prim = torch.cat([p.to(dev) for p in pieces])
    tables = torch.from_numpy(np.concatenate([tab["traj_first"], tab["box_offset"], tab["sphere_offset"], tab["cloud_offset"]])).to(dev)
    NB, NS, NP = sum(nb), sum(ns), sum(npts)
    o_bs, o_sc, o_sr, o_pt = NB * D, 2 * NB * D, 2 * NB * D + NS * D, 2 * NB * D + NS * D + NS
    n1 = n_scenes + 1
    ob = _lib.RampObstacles()
    ob.point_dim, ob.n_scenes = D, n_scenes
    ob.box_centers = prim.data_ptr() if NB else None
    ob.box_sizes = prim[o_bs:].data_ptr() if NB else None
    ob.sphere_centers = prim[o_sc:].data_ptr() if NS else None
    ob.sphere_radii = prim[o_sr:].data_ptr() if NS else None
    ob.cloud = prim[o_pt:].data_ptr() if NP else None
    ob.box_offset, ob.sphere_offset, ob.cloud_offset = tables[n1:].data_ptr(), tables[2 * n1:].data_ptr(), tables[3 * n1:].data_ptr()
    ob.n_boxes_total, ob.n_spheres_total, ob.n_points_total, ob.margin = NB, NS, NP, float(margin)
    hits = torch.empty(2, B, dtype=torch.int32, device=dev)
    vals = torch.empty(4, B, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_traj_clearance(
            _lib.ptr(t), B, H, S, C.byref(ob), tables.data_ptr(), 1 if swept else 0, hits[0].data_ptr(),
            hits[1].data_ptr() if swept else None, vals[0].data_ptr(), vals[1].data_ptr() if swept else None, vals[2].data_ptr(),
            vals[3].data_ptr(), _lib.current_stream()), "ramp_traj_clearance")
    return Clearance(H, hits[0], hits[1] if swept else None, vals[0], vals[1] if swept else None, vals[2], vals[3], tables[:n1], D)
