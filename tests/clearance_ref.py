"""The definitions of ramp_traj_clearance (include/ramp_hip.h) restated in float64 numpy, a brute-force sampler that checks the
restatement against something independent of it, and the scene generator the host and GPU tests share.  numpy only.

Conventions: a scene is a dict ``traj (n, H, S) float32, boxes (centers (k, D), sizes (k, D)) or None, spheres (centers (m, D), radii (m))
or None, cloud (p, D) or None``; every function takes float32 inputs and computes in float64."""
import numpy as np

SPACING = 2e-5          # sample spacing of the brute-force check
MARGIN = 1e-3           # no (waypoint or segment, primitive) decision of a generated scene sits closer than this to its boundary


# ------------------------------------------------------------------------------------------------ the restatement
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def box_bounds(centers, sizes, margin):
    c, s = _f64(centers), _f64(sizes)
    return c - s / 2 - margin, c + s / 2 + margin


def wp_in_box(p, lo, hi):
    """p (..., D) -> (...) bool, inclusive on both sides."""
    return ((p >= lo) & (p <= hi)).all(-1)


def seg_hits_box(a, b, lo, hi):
    """Slab clipping of t in [0, 1]: a, b (..., D) -> (...) bool.  An axis with zero direction passes iff the start is in the slab."""
    d = b - a
    zero = d == 0
    inside = (a >= lo) & (a <= hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = (lo - a) / d, (hi - a) / d
    tn = np.where(zero, -np.inf, np.minimum(u, v))
    tf = np.where(zero, np.inf, np.maximum(u, v))
    ok = np.where(zero, inside, True).all(-1)
    t0 = np.maximum(0.0, tn.max(-1))
    t1 = np.minimum(1.0, tf.min(-1))
    return ok & (t0 <= t1)


def seg_point_dist(a, b, q):
    """Distance from q to the closed segment [a, b]: t = clamp((q - a).(b - a) / |b - a|^2, 0, 1), t = 0 for a zero-length segment."""
    d = b - a
    l2 = (d * d).sum(-1)
    w = q - a
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(l2 > 0, np.clip((w * d).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0), 0.0)
    r = w - t[..., None] * d
    return np.sqrt((r * r).sum(-1))


def ref_scene(traj, D, boxes=None, spheres=None, cloud=None, margin=0.0):
    """One scene.  Returns wp_hit (n, H) bool, seg_hit (n, H - 1) bool, clear_wp, clear_seg, path_len, smooth (n) float64."""
    x = _f64(traj)
    n, H, S = x.shape
    p = x[..., :D]
    a, b = p[:, :-1], p[:, 1:]
    wp = np.zeros((n, H), bool)
    sg = np.zeros((n, H - 1), bool)
    if boxes is not None:
        lo, hi = box_bounds(boxes[0], boxes[1], margin)
        for k in range(lo.shape[0]):
            wp |= wp_in_box(p, lo[k], hi[k])
            sg |= seg_hits_box(a, b, lo[k], hi[k])
    if spheres is not None:
        c, r = _f64(spheres[0]), _f64(spheres[1]) + margin
        for k in range(c.shape[0]):
            wp |= np.sqrt(((p - c[k]) ** 2).sum(-1)) <= r[k]
            sg |= seg_point_dist(a, b, c[k]) <= r[k]
    sg |= wp[:, :-1] | wp[:, 1:]
    cw = np.full(n, np.inf)
    cs = np.full(n, np.inf)
    if cloud is not None and len(cloud):
        q = _f64(cloud)
        for i in range(n):
            cw[i] = np.sqrt(((p[i][:, None, :] - q[None]) ** 2).sum(-1)).min()
            cs[i] = min(seg_point_dist(a[i][:, None, :], b[i][:, None, :], q[None]).min(), cw[i])
    plen = np.sqrt(((b - a) ** 2).sum(-1)).sum(-1)
    smooth = np.sqrt(((x[:, 1:, D:] - x[:, :-1, D:]) ** 2).sum(-1)).sum(-1)
    return dict(wp_hit=wp, seg_hit=sg, clear_wp=cw, clear_seg=cs, path_len=plen, smooth=smooth)


def ref_case(case, margin=0.0):
    """All scenes of a generated case, rows in batch order: wp_hits / seg_hits (B) int, clear_wp, clear_seg, path_len, smooth (B)."""
    parts = [ref_scene(s["traj"], case["D"], s["boxes"], s["spheres"], s["cloud"], margin) for s in case["scenes"]]
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("clear_wp", "clear_seg", "path_len", "smooth")}
    out["wp_hits"] = np.concatenate([p["wp_hit"].sum(-1) for p in parts])
    out["seg_hits"] = np.concatenate([p["seg_hit"].sum(-1) for p in parts])
    return out


# ------------------------------------------------------------------------------------------------ brute force
def box_fn(x, c, half):
    """max_d (|x_d - c_d| - half_d): <= 0 exactly on the closed box."""
    return (np.abs(x - c) - half).max(-1)


def sphere_fn(x, c, r):
    return np.sqrt(((x - c) ** 2).sum(-1)) - r


def segment_samples(a, b, spacing=SPACING):
    """Points of the closed segment [a, b] at a spacing <= `spacing`, both ends included."""
    n = int(np.ceil(np.sqrt(((b - a) ** 2).sum()) / spacing)) + 1
    t = np.linspace(0.0, 1.0, max(n, 2))[:, None]
    return a + t * (b - a)


def sampled_minima(traj, D, fns, spacing=SPACING):
    """For one scene: the minimum of every function of `fns` (each maps (m, D) points to (m) values) over the samples of every segment
    (n, H - 1, len(fns)) and its value at every waypoint (n, H, len(fns))."""
    p = _f64(traj)[..., :D]
    n, H, _ = p.shape
    seg = np.empty((n, H - 1, len(fns)))
    wp = np.empty((n, H, len(fns)))
    for i in range(n):
        for j, f in enumerate(fns):
            wp[i, :, j] = f(p[i])
        for h in range(H - 1):
            x = segment_samples(p[i, h], p[i, h + 1], spacing)
            for j, f in enumerate(fns):
                seg[i, h, j] = f(x).min()
    return seg, wp


def primitive_fns(boxes, spheres, margin=0.0):
    fns = []
    if boxes is not None:
        c, s = _f64(boxes[0]), _f64(boxes[1])
        fns += [(lambda x, c=c[k], h=s[k] / 2 + margin: box_fn(x, c, h)) for k in range(c.shape[0])]
    if spheres is not None:
        c, r = _f64(spheres[0]), _f64(spheres[1])
        fns += [(lambda x, c=c[k], r=r[k] + margin: sphere_fn(x, c, r)) for k in range(c.shape[0])]
    return fns


# ------------------------------------------------------------------------------------------------ the generator
def _walk(rng, p0, n, D, step):
    """n more waypoints from p0: uniform draws for short trajectories (long segments), a clipped random walk for long ones."""
    out, p = [], p0
    for _ in range(n):
        if step >= 1.0:
            p = rng.uniform(-1, 1, D)
        else:
            p = np.clip(p + rng.uniform(-step, step, D), -1, 1)
        out.append(p)
    return out


def _draw_traj(rng, kind, H, S, D, boxes, spheres):
    """One trajectory (H, S).  kind: 'random', or a planted first segment -- 'box_cross' through box 0 along an axis (two zero direction
    components inside their slabs, both waypoints outside the box), 'box_beside' the same segment moved out of a slab (a zero component
    outside it), 'sphere_cross' through sphere 0 along a diagonal, 'zero' a zero-length segment -- or 'inside', a start at the centre of the
    last box (sphere), so that a run of waypoints is hit before the walk leaves it."""
    # long trajectories walk in steps of at most 3 / H per axis, so that their path length stays below 4 (a trajectory crosses a world of
    # side 2; metrics_cases.npz: at most 5.2 at H = 48): the per-segment lengths are added serially in fp32, each add rounds to half an ulp of
    # the running sum, and over 127 adds that is about sqrt(127 / 3) half-ulps -- 1.6e-6 while the sum stays in 2 .. 4, 3.1e-6 in 4 .. 8
    # (measured at a path length of 8: 2.4e-6) -- against the absolute bar of 2e-6 that fixture carries.
    step = min(1.0, 3.0 / H)
    p0 = rng.uniform(-1, 1, D)
    pts = [p0]
    if kind == "zero":
        pts.append(p0.copy())
    elif kind == "inside":
        pts = [np.float64(boxes[0][-1] if boxes is not None else spheres[0][-1])]
    elif kind in ("box_cross", "box_beside"):
        c, half = np.float64(boxes[0][0]), np.float64(boxes[1][0]) / 2
        a, b = c.copy(), c.copy()
        a[0] -= 0.4; b[0] += 0.4
        if kind == "box_beside":
            a[1] = b[1] = c[1] + half[1] + 0.15
        pts = [a, b]
    elif kind == "sphere_cross":
        c = np.float64(spheres[0][0])
        u = np.ones(D) / np.sqrt(D)
        pts = [c - 0.4 * u, c + 0.4 * u]
    pts = pts[:H] + _walk(rng, pts[-1], H - len(pts), D, step)
    x = np.zeros((H, S), np.float32)
    x[:, :D] = np.asarray(pts)
    # the state entries behind the position are velocities: half the forward difference of the positions (0 at the last waypoint), as a
    # trajectory's are, not noise.  Smoothness then stays within the magnitude it has in metrics_cases.npz (20 .. 30), which is what that
    # fixture's absolute bar of 2e-5 presumes: a serial fp32 sum of 127 terms that reaches 180 (independent uniform entries at H = 128,
    # measured: 6.0e-5 off) carries up to 127 half-ulps of 128 .. 256, 7.6e-6 each, whatever the kernel.
    v = np.zeros((H, D))
    v[:-1] = 0.5 * np.diff(np.asarray(pts), axis=0)
    x[:, D:] = v[:, :S - D]
    return x


def _violations(traj, D, boxes, spheres, samples_cache, which=None):
    """Per primitive (boxes first, then spheres): does any sampled (waypoint or segment, primitive) minimum lie within MARGIN of 0?
    `which`: the primitives to look at (the others are reported clear)."""
    fns = primitive_fns(boxes, spheres)
    if not fns:
        return np.zeros(0, bool)
    if "x" not in samples_cache:
        p = _f64(traj)[..., :D]
        samples_cache["x"] = [segment_samples(p[i, h], p[i, h + 1]) for i in range(p.shape[0]) for h in range(p.shape[1] - 1)]
    bad = np.zeros(len(fns), bool)
    for j, f in enumerate(fns):
        if which is not None and not which[j]:
            continue
        for x in samples_cache["x"]:
            v = f(x)
            if abs(v.min()) < MARGIN or abs(v[0]) < MARGIN or abs(v[-1]) < MARGIN:
                bad[j] = True
                break
    return bad


def make_scene(rng, n, H, S, D, n_boxes, n_spheres, n_points):
    """One scene of n trajectories in [-1, 1]^D.  The first row is random, the others plant a box crossing, a sphere crossing, a zero-length
    segment, a segment beside a slab and a start inside a primitive, as far as rows and primitives allow.  Then every primitive whose decision on some waypoint or
    segment lies within MARGIN of its boundary (by sampling) gets a new size, until none does."""
    boxes = spheres = None
    if n_boxes:
        boxes = (rng.uniform(-0.6, 0.6, (n_boxes, D)).astype(np.float32), rng.uniform(0.2, 0.4, (n_boxes, D)).astype(np.float32))
    if n_spheres:
        spheres = (rng.uniform(-0.6, 0.6, (n_spheres, D)).astype(np.float32), rng.uniform(0.08, 0.2, n_spheres).astype(np.float32))
    kinds = ["random"] + (["box_cross"] if n_boxes else []) + (["sphere_cross"] if n_spheres else []) + ["zero"] + \
        (["box_beside"] if n_boxes else []) + (["inside"] if n_boxes or n_spheres else [])
    traj = np.stack([_draw_traj(rng, kinds[i] if i < len(kinds) else "random", H, S, D, boxes, spheres) for i in range(n)])
    cache, bad = {}, None
    for _ in range(200):
        bad = _violations(traj, D, boxes, spheres, cache, bad)       # (a primitive found clear stays clear: only the redrawn ones change)
        if not bad.any():
            break
        for j in np.nonzero(bad)[0]:
            if j < n_boxes:
                boxes[1][j] = rng.uniform(0.2, 0.4, D).astype(np.float32)
            else:
                spheres[1][j - n_boxes] = np.float32(rng.uniform(0.08, 0.2))
    else:
        raise RuntimeError("the generator found no primitive sizes clear of every decision boundary")
    cloud = rng.uniform(-1, 1, (n_points, D)).astype(np.float32) if n_points else None
    return dict(traj=traj, boxes=boxes, spheres=spheres, cloud=cloud)


# (H, S, D, boxes, spheres, cloud points, scenes): every value of the test table appears, every (S, D) with every kind of primitive
CASE_TABLE = [
    (2, 4, 2, 1, 0, 0, 1),
    (2, 6, 3, 3, 2, 1, 1),
    (3, 3, 3, 1, 2, 1023, 1),
    (3, 4, 2, 3, 2, 1025, 3),
    (65, 6, 3, 3, 2, 1025, 3),
    (65, 4, 2, 0, 2, 1, 1),
    (128, 3, 3, 3, 0, 1023, 1),
    (128, 6, 3, 1, 2, 1025, 3),
    (128, 4, 2, 3, 2, 0, 1),
    (3, 6, 3, 0, 0, 1025, 1),
]
B = 5
SCENE_COUNTS = (2, 1, 2)        # three scenes with unequal counts; the middle one has no boxes

_cases = {}


def make_case(idx):
    """Case idx of CASE_TABLE (cached): dict H, S, D, counts, scenes (list of scene dicts), traj (B, H, S)."""
    if idx in _cases:
        return _cases[idx]
    H, S, D, nb, ns, npts, n_scenes = CASE_TABLE[idx]
    rng = np.random.default_rng(1000 + idx)
    counts = SCENE_COUNTS if n_scenes == 3 else (B,)
    scenes = []
    for i, n in enumerate(counts):
        scenes.append(make_scene(rng, n, H, S, D, 0 if (n_scenes == 3 and i == 1) else nb, ns, npts + (i if npts > 1 else 0)))
    case = dict(H=H, S=S, D=D, counts=list(counts), scenes=scenes, traj=np.concatenate([s["traj"] for s in scenes]))
    _cases[idx] = case
    return case
