"""The swept box and sphere terms of the cost guide (ramp_prim_guide in include/ramp_hip.h) restated in numpy, generic in dtype: float64 is
the truth, the same code in float32 the yardstick of tests/test_gpu_prim_guide.py.  Every product and sum is written in the header's order
(primitives one after the other: boxes, then spheres, in table order; the hand-back sample after sample), so the float32 run rounds where the
kernel rounds.  Also the designed cases of the issue and the case tables the host and GPU tests share.  numpy only.

A scene is a dict ``boxes (centres (k, D), sizes (k, D)) or None, spheres (centres (m, D), radii (m,)) or None, cloud (P, D) or None``."""
import numpy as np

F32 = lambda v: float(np.float32(v))      # noqa: E731


# ------------------------------------------------------------------------------------------------ the definition
def samples(p, n):
    """u ((H - 1) n + 1, D) of positions p (H, D): u[h n + m] = p_h + (m / n) (p_{h+1} - p_h); m = 0 and the last sample are waypoints."""
    dt = p.dtype.type
    H, D = p.shape
    u = np.empty(((H - 1) * n + 1, D), p.dtype)
    u[0::n] = p
    for m in range(1, n):
        t = dt(m) / dt(n)
        u[m::n] = p[:-1] + t * (p[1:] - p[:-1])
    return u


def box_phi(u, c, half):
    """phi (N,) and grad phi (N, D) of one box (centre c, widened half sides) at the samples u (N, D)."""
    dt = u.dtype.type
    e = u - c
    q = np.abs(e) - half
    sgn = np.where(e < 0, dt(-1), dt(1))
    out = (q > 0).any(1)
    mx = np.maximum(q, dt(0))
    s2 = mx[:, 0] * mx[:, 0]
    for d in range(1, u.shape[1]):
        s2 = s2 + mx[:, d] * mx[:, d]
    phi_out = np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        g_out = (sgn * mx) / phi_out[:, None]
    k = q.argmax(1)                                           # the lowest axis that attains the maximum
    g_in = np.zeros_like(u)
    g_in[np.arange(len(u)), k] = sgn[np.arange(len(u)), k]
    return np.where(out, phi_out, q.max(1)), np.where(out[:, None], g_out, g_in)


def sphere_phi(u, c, R):
    """phi (N,) and grad phi (N, D) of one sphere (centre c, widened radius R); zero gradient at the centre."""
    e = u - c
    d2 = e[:, 0] * e[:, 0]
    for d in range(1, u.shape[1]):
        d2 = d2 + e[:, d] * e[:, d]
    dist = np.sqrt(d2)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(dist[:, None] > 0, e / dist[:, None], u.dtype.type(0))
    return dist - R, g


def sample_terms(u, scene, margin, band):
    """g_u (N, D) = - sum_k (band - phi_k) grad phi_k and the float64 sum of the values 1/2 (band - phi_k)^2, over the primitives with
    phi_k < band: boxes, then spheres, in table order.  Also the smallest phi per sample (N,) (+inf without a primitive)."""
    dt = u.dtype.type
    g = np.zeros_like(u)
    cost = 0.0
    low = np.full(len(u), np.inf)
    prims = []
    if scene.get("boxes") is not None:
        c, s = scene["boxes"]
        prims += [("b", c[k].astype(u.dtype), s[k].astype(u.dtype) / dt(2) + dt(margin)) for k in range(len(c))]
    if scene.get("spheres") is not None:
        c, r = scene["spheres"]
        prims += [("s", c[k].astype(u.dtype), r[k].astype(u.dtype) + dt(margin)) for k in range(len(c))]
    for kind, c, ext in prims:
        phi, gr = box_phi(u, c, ext) if kind == "b" else sphere_phi(u, c, ext)
        on = phi < dt(band)
        w = np.where(on, dt(band) - phi, dt(0))
        g = np.where(on[:, None], g - w[:, None] * gr, g)
        cost += float((dt(0.5) * (w * w)).astype(np.float64).sum())
        low = np.minimum(low, phi.astype(np.float64))
    return g, cost, low


def hand_back(gu, H, n):
    """g_prim (H, D) from the samples' gradients gu ((H - 1) n + 1, D), in the header's order."""
    dt = gu.dtype.type
    seg = gu[:-1].reshape(H - 1, n, -1)
    gp = np.empty((H, gu.shape[1]), gu.dtype)
    gp[:-1] = seg[:, 0]
    gp[-1] = gu[-1]
    for m in range(1, n):
        gp[:-1] = gp[:-1] + (dt(1) - dt(m) / dt(n)) * seg[:, m]
    for m in range(1, n):
        gp[1:] = gp[1:] + (dt(m) / dt(n)) * seg[:, m]
    return gp


def n_prims(scene):
    return sum(len(scene[k][0]) for k in ("boxes", "spheres") if scene.get(k) is not None)


def prim_grad(p, scene, margin, band, n):
    """d C_prim / d p (H, D) in p's dtype."""
    return hand_back(sample_terms(samples(p, n), scene, margin, band)[0], len(p), n)


def prim_cost(p, scene, margin, band, n):
    """C_prim of positions p (H, D): values in p's dtype, the sum in float64."""
    return sample_terms(samples(p, n), scene, margin, band)[1]


def min_phi(p, scene, margin, n):
    """The smallest phi over the n-per-segment samples of the path p (H, D), float64."""
    return float(sample_terms(samples(np.asarray(p, np.float64), n), scene, margin, 0.0)[2].min())


def cloud_grad(p, c, r):
    """d/dp sum_j 1/2 max(0, r - |p_h - c_j|)^2 (H, D) in p's dtype; a pair at distance 0 contributes nothing."""
    dt = p.dtype.type
    dx = p.T[:, :, None] - c.T.astype(p.dtype)[:, None, :]
    d = np.sqrt((dx * dx).sum(0))
    inside = (d < dt(r)) & (d > 0)
    f = np.where(inside, (dt(r) - d) / np.where(inside, d, dt(1)), dt(0)).astype(p.dtype)
    return (-(f[None] * dx).sum(-1).T).astype(p.dtype)


def stencil_grad(p, w_smooth, w_acc):
    """w_smooth g_smooth + w_acc g_acc of ramp_cost_guide (H, D) in p's dtype."""
    dt = p.dtype.type
    gs = np.zeros_like(p)
    gs[:-1] = p[:-1] - p[1:]
    gs[1:] += p[1:] - p[:-1]
    a = np.zeros_like(p)
    a[1:-1] = (p[2:] - dt(2) * p[1:-1]) + p[:-2]
    ga = dt(-2) * a
    ga[:-1] += a[1:]
    ga[1:] += a[:-1]
    return dt(w_smooth) * gs + dt(w_acc) * ga


def total_grad(p, scene, k):
    """g = w_obs g_obs + (w_prim g_prim + (w_smooth g_s + w_acc g_a)); a term that is switched off or empty is not added at all."""
    dt = p.dtype.type
    g = stencil_grad(p, k.get("w_smooth", 0.0), k.get("w_acc", 0.0))
    if k.get("w_prim", 1.0) != 0 and n_prims(scene):
        g = dt(k.get("w_prim", 1.0)) * prim_grad(p, scene, k["margin"], k["band"], k["n_sub"]) + g
    cloud = scene.get("cloud")
    if cloud is not None and len(cloud) and k.get("w_obs", 0.0) != 0:
        g = dt(k["w_obs"]) * cloud_grad(p, cloud, k["radius"]) + g
    return g.astype(p.dtype)


def iterate(x, scenes, traj_scene, pins, k, step, n_iter, max_norm, dtype, D, log=None):
    """n_iter guide iterations on trajectories x (B, H, S) -> new array of ``dtype``.  scenes: list of scene dicts; traj_scene (B,) or None (a
    trajectory whose scene is outside the list stays); pins {waypoint: (S,) or (B, S)} (later entries win); k: margin, band, n_sub, w_prim and
    optionally radius, w_obs, w_smooth, w_acc.  ``log`` collects (trajectory, iteration, s, |g|)."""
    out = np.array(x, dtype=dtype)
    dt = out.dtype.type
    B, H, S = out.shape
    for b in range(B):
        sc = 0 if traj_scene is None else int(traj_scene[b])
        if not 0 <= sc < len(scenes):
            continue
        p = out[b, :, :D].copy()
        free = np.ones(H, bool)
        for h, v in pins.items():
            v = np.asarray(v)
            p[h] = (v if v.ndim == 1 else v[b])[:D].astype(dtype)
            free[h] = False
        for it in range(n_iter):
            g = total_grad(p, scenes[sc], k)
            g[~free] = 0
            nrm = dt(np.sqrt((g.astype(np.float64) ** 2).sum()))
            s = min(dt(1), dt(max_norm) / nrm) if (max_norm > 0 and nrm > 0) else dt(1)
            if log is not None:
                log.append((b, it, float(s), float(nrm)))
            p[free] = (p - (dt(step) * dt(s)) * g)[free]
        out[b, free, :D] = p[free]
    return out


def exact_cost(p, scene, k):
    """C of positions p (H, D) in float64 (w_obs C_obs + w_prim C_prim + w_smooth C_smooth + w_acc C_acc), for difference quotients."""
    c = k.get("w_prim", 1.0) * prim_cost(p, scene, k["margin"], k["band"], k["n_sub"])
    cloud = scene.get("cloud")
    if cloud is not None and len(cloud) and k.get("w_obs", 0.0) != 0:
        u = np.maximum(0.0, k["radius"] - np.sqrt(((p[:, None, :] - cloud[None].astype(np.float64)) ** 2).sum(-1)))
        c += k["w_obs"] * float((0.5 * u * u).sum())
    c += k.get("w_smooth", 0.0) * float((0.5 * ((p[1:] - p[:-1]) ** 2).sum(1)).sum())
    c += k.get("w_acc", 0.0) * float((0.5 * ((p[2:] - 2 * p[1:-1] + p[:-2]) ** 2).sum(1)).sum())
    return c


def kink_distance(p, scene, margin, band, n):
    """How far the samples of the path p (H, D) stay from the term's kinks, float64: (|phi - band| over all pairs, the gap between the largest
    and the second largest q_d of a sample inside a box -- the medial axes --, the distance to a sphere's centre); inf where there is none."""
    u = samples(np.asarray(p, np.float64), n)
    d_band = d_tie = d_centre = np.inf
    if scene.get("boxes") is not None:
        for c, s in zip(*scene["boxes"]):
            half = np.float64(s) / 2 + margin
            q = np.abs(u - np.float64(c)) - half
            phi = box_phi(u, np.float64(c), half)[0]
            d_band = min(d_band, float(np.abs(phi - band).min()))
            near = phi < band + 1e-3                                # a tie matters only where the pair contributes (or nearly does)
            near &= (q <= 1e-4).all(1)                              # ... and where the sample is inside the box (or nearly)
            qs = np.sort(q[near], axis=1)
            if len(qs):      # (and sign(0) on the axis that takes the gradient)
                e_k = np.abs(u[near] - np.float64(c))[np.arange(len(qs)), q[near].argmax(1)]
                d_tie = min(d_tie, float((qs[:, -1] - qs[:, -2]).min()), float(e_k.min()))
    if scene.get("spheres") is not None:
        for c, r in zip(*scene["spheres"]):
            dist = np.sqrt(((u - np.float64(c)) ** 2).sum(1))
            d_band = min(d_band, float(np.abs(dist - (np.float64(r) + margin) - band).min()))
            d_centre = min(d_centre, float(dist.min()))
    return d_band, d_tie, d_centre


# ------------------------------------------------------------------------------------------------ the designed cases of the issue
DESIGN = dict(H=8, margin=F32(0.05), band=F32(0.02), w_prim=1.0, step=0.5, n_iter=16)


def design_case(kind, D):
    """The straight line and the scene of a designed case: 'box' -- centre 0, sides 0.4, line (-0.71, 0.29) -> (0.29, -0.71) --, 'sphere' --
    radius 0.2 at the origin, line (-0.665, 0.335) -> (0.335, -0.665); in 3-D a constant third coordinate 0.05 (and a cubic box).  Returns
    x (1, H, D + 2) float32 (the other channels 7) and the scene."""
    a, b = ((-0.71, 0.29), (0.29, -0.71)) if kind == "box" else ((-0.665, 0.335), (0.335, -0.665))
    H = DESIGN["H"]
    t = np.linspace(0.0, 1.0, H)[:, None]
    xy = (1 - t) * np.float64(a) + t * np.float64(b)
    p = xy if D == 2 else np.concatenate([xy, np.full((H, 1), 0.05)], 1)
    x = np.full((1, H, D + 2), 7.0, np.float32)
    x[0, :, :D] = p
    if kind == "box":
        scene = dict(boxes=(np.zeros((1, D), np.float32), np.full((1, D), 0.4, np.float32)), spheres=None, cloud=None)
    else:
        scene = dict(boxes=None, spheres=(np.zeros((1, D), np.float32), np.float32([0.2])), cloud=None)
    return x, scene


def design_run(kind, D, n_sub, dtype):
    """The designed case after its 16 iterations (endpoints pinned, step 0.5, no clip): (x before, x after, scene)."""
    x, scene = design_case(kind, D)
    H = DESIGN["H"]
    pins = {0: x[0, 0], H - 1: x[0, H - 1]}
    k = dict(margin=DESIGN["margin"], band=DESIGN["band"], w_prim=DESIGN["w_prim"], n_sub=n_sub)
    return x, iterate(x, [scene], None, pins, k, DESIGN["step"], DESIGN["n_iter"], 0.0, dtype, D), scene


# ------------------------------------------------------------------------------------------------ the exact cases
def exact_cases():
    """Inputs whose arithmetic is exact in float32 (dyadic numbers), one iteration, no pins, w_prim alone.  name -> dict x (1, 4, D + 1), scene,
    k, step, D, moves (1, 4, D + 1) bool: the entries that change, sign: the direction they move in.
      centre_wp   a waypoint exactly at a sphere's centre (n_sub = 1): cost, no gradient -- nothing moves
      centre_mid  the midpoint of segment 0 exactly at the centre (n_sub = 2), the waypoints outside the band: nothing moves
      tie_pos / tie_neg   a waypoint inside a box with q_0 == q_1 (> q_2): axis 0 alone moves, away from the centre
      sign_zero   a waypoint inside a box at offset 0 along the axis of its nearest face: sign(0) = +1, it moves in +x"""
    out = {}
    for D in (2, 3):
        pad = [0.0] * (D - 2)
        far = [[-1.0, 0.5] + pad, [1.0, 0.5] + pad, [2.0, 0.5] + pad]

        def traj(wps):
            x = np.full((1, 4, D + 1), 7.0, np.float32)
            x[0, :, :D] = np.float32(wps)
            return x
        k1 = dict(margin=F32(0.03125), band=F32(0.0625), w_prim=1.0, n_sub=1)
        sph = dict(boxes=None, spheres=(np.zeros((1, D), np.float32), np.float32([0.125])), cloud=None)
        none = np.zeros((1, 4, D + 1), bool)
        out[f"centre_wp_{D}d"] = dict(x=traj([far[0], [0.0, 0.0] + pad, far[1], far[2]]), scene=sph, k=k1, moves=none, sign=1)
        out[f"centre_mid_{D}d"] = dict(x=traj([[-0.25, 0.0] + pad, [0.25, 0.0] + pad, [0.75, 0.0] + pad, [1.25, 0.0] + pad]), scene=sph,
                                       k=dict(k1, n_sub=2), moves=none, sign=1)
        one = none.copy(); one[0, 1, 0] = True
        cube = dict(boxes=(np.zeros((1, D), np.float32), np.float32([[0.5, 0.5] + [1.0] * (D - 2)])), spheres=None, cloud=None)
        out[f"tie_pos_{D}d"] = dict(x=traj([far[0], [0.125, 0.125] + pad, far[1], far[2]]), scene=cube, k=k1, moves=one, sign=1)
        out[f"tie_neg_{D}d"] = dict(x=traj([far[0], [-0.125, 0.125] + pad, far[1], far[2]]), scene=cube, k=k1, moves=one, sign=-1)
        slab = dict(boxes=(np.zeros((1, D), np.float32), np.float32([[0.125, 1.0] + [1.0] * (D - 2)])), spheres=None, cloud=None)
        out[f"sign_zero_{D}d"] = dict(x=traj([[-1.0, 1.5] + pad, [0.0, 0.0] + pad, [1.0, 1.5] + pad, [2.0, 1.5] + pad]), scene=slab, k=k1, moves=one,
                                      sign=1)
    for c in out.values():
        c.update(step=0.5, D=c["x"].shape[2] - 1)
    return out


# ------------------------------------------------------------------------------------------------ the op cases shared by host and GPU tests
# (H, S, D, n_sub, boxes, spheres, n_iter, clip, band): every value of the issue's lists -- H 8 / 128, (S, D) (4, 2) / (6, 3), n_sub 1 / 2 / 8,
# 1 / 64 / 65 primitives of each kind (the LDS chunk border), 1 / 16 iterations, clip on / off, band = 0
OP_CASES = [
    (8, 4, 2, 1, 1, 1, 1, False, 0.05),
    (8, 6, 3, 2, 64, 64, 16, True, 0.05),
    (8, 4, 2, 8, 65, 65, 16, False, 0.05),
    (128, 6, 3, 8, 1, 65, 1, True, 0.05),
    (128, 4, 2, 2, 65, 1, 16, True, 0.05),
    (128, 4, 2, 1, 64, 0, 1, False, 0.05),
    (128, 6, 3, 8, 0, 64, 1, False, 0.0),
    (8, 6, 3, 8, 65, 64, 16, False, 0.0),
]
OP_B = 5
OP_MARGIN = F32(0.03)
OP_STEP = F32(0.05)
OP_SCENES = [0, 1, 0, 2, 0]      # scene 1 has no primitive, scene index 2 is outside the table: that trajectory is left untouched
_OP = {}


def op_case(case):
    """Inputs and both restatements of one op case, computed once.  B = 5 smooth random paths in [-1, 1]^D over two scenes (the second one
    without primitives) and one scene index outside the table; pins at both ends and in the middle, with values of their own; weights
    w_prim = 1, w_smooth = 0.5, w_acc = 0.25, no cloud; with clip, max_norm is the geometric mean of the smallest and largest first gradient
    norm of the trajectories that have primitives.  The primitives are redrawn until no sample of an input path lies within 1e-4 of
    phi = band, of a box's medial axis or of a sphere's centre (kink_distance)."""
    if case in _OP:
        return _OP[case]
    H, S, D, n, nb, ns, n_iter, clip, band = case
    band = F32(band)
    rng = np.random.default_rng(4000 + OP_CASES.index(case))
    x = np.zeros((OP_B, H, S), np.float32)
    for b in range(OP_B):      # a clipped random walk: neighbouring waypoints 0.05 .. 0.4 apart, so that segments matter
        p = [rng.uniform(-0.8, 0.8, D)]
        for _ in range(H - 1):
            p.append(np.clip(p[-1] + rng.uniform(-1, 1, D) * min(0.4, 3.0 / H), -1, 1))
        x[b, :, :D] = np.asarray(p)
    x[:, :, D:] = rng.uniform(-1, 1, (OP_B, H, S - D))
    idx = [0, H // 2, H - 1]
    val = rng.uniform(-0.8, 0.8, (len(idx), OP_B, S)).astype(np.float32)
    val[1] = x[:, H // 2] + rng.uniform(-0.02, 0.02, (OP_B, S)).astype(np.float32)      # (the middle pin stays near the path)
    pins = {h: val[i] for i, h in enumerate(idx)}
    k = dict(margin=OP_MARGIN, band=band, w_prim=1.0, n_sub=n, w_smooth=0.5, w_acc=0.25)

    def working(b):
        p = x[b, :, :D].astype(np.float64)
        for h in idx:
            p[h] = pins[h][b, :D]
        return p
    for attempt in range(200):
        boxes = (rng.uniform(-0.8, 0.8, (nb, D)).astype(np.float32), rng.uniform(0.05, 0.3, (nb, D)).astype(np.float32)) if nb else None
        spheres = (rng.uniform(-0.8, 0.8, (ns, D)).astype(np.float32), rng.uniform(0.03, 0.15, ns).astype(np.float32)) if ns else None
        scene = dict(boxes=boxes, spheres=spheres, cloud=None)
        kd = [kink_distance(working(b), scene, OP_MARGIN, band, n) for b in range(OP_B) if OP_SCENES[b] == 0]
        if min(min(v) for v in kd) > 1e-4:
            break
    else:
        raise RuntimeError("no primitive draw keeps the samples clear of the kinks")
    scenes = [scene, dict(boxes=None, spheres=None, cloud=None)]
    ts = np.array(OP_SCENES, np.int32)
    norms, prim_g = [], 0.0
    for b in range(OP_B):
        if OP_SCENES[b] == 0:
            g = total_grad(working(b), scene, k)
            g[idx] = 0
            norms.append(float(np.sqrt((g ** 2).sum())))
            prim_g = max(prim_g, float(np.abs(prim_grad(working(b), scene, OP_MARGIN, band, n)).max()))
    max_norm = F32(np.sqrt(min(norms) * max(norms))) if clip else 0.0
    log = []
    y64 = iterate(x, scenes, ts, pins, k, OP_STEP, n_iter, max_norm, np.float64, D, log=log)
    y32 = iterate(x, scenes, ts, pins, k, OP_STEP, n_iter, max_norm, np.float32, D)
    _OP[case] = dict(x=x, scenes=scenes, ts=ts, idx=idx, val=val, pins=pins, k=k, max_norm=max_norm, y64=y64, y32=y32, log=log, norms=norms,
                     kink=min(min(v) for v in kd), prim_g=prim_g, D=D, n_iter=n_iter)
    return _OP[case]
