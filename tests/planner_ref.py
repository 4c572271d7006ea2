"""Plain numpy references of the planner kernels (ramp_amd/csrc/sampler.hip, metrics.hip) and the case tables that
tests/test_planner_ref_host.py proves on the CPU and tests/test_gpu_planner_kernels.py runs on the device.  numpy only.

References: the oracle's brute-force float64 APF (lowest index on a distance tie), the float32 collision mask, float64 path length
and smoothness, the selection rule of cost.py:56-88 in float32, and the elementwise steps restated in the kernels' documented
float32 order.  Case builders are cached: a case and its reference are computed once per process and must not be modified."""
import functools

import numpy as np

from oracle import ramp_oracle as O

U32 = 2.0 ** -24
F = np.float32

# margins every random case keeps (test_planner_ref_host.py checks them; a seed that misses one is replaced, never skipped)
THR_MARGIN = 1e-6          # no nearest distance this close to its threshold
TIE_MARGIN = 1e-12         # no second-nearest point this close (relative) to the nearest, unless the tie is designed
TOTAL_MARGIN = 1e-5        # no two free totals of a selection case this close, unless designed equal


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def maxdiff_nan_equal(a, b):
    """max |a - b| over the entries where both are finite; inf if the NaN patterns differ."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return np.inf
    d = np.abs(a - b)[~na]
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------------ references
def nearest_two(q, pts):
    """q (N, 2), pts (P, 2): float64 distance to the nearest point, to the second nearest (inf when P = 1), the nearest's index
    (lowest on a tie) and the number of points at exactly the nearest squared distance."""
    q, p = np.asarray(q, np.float64), np.asarray(pts, np.float64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    idx = d2.argmin(1)
    best = d2[np.arange(len(q)), idx]
    n_tied = (d2 == best[:, None]).sum(1)
    if p.shape[0] > 1:
        second = np.partition(d2, 1, axis=1)[:, 1]
    else:
        second = np.full(len(q), np.inf)
    return np.sqrt(best), np.sqrt(second), idx, n_tied


def apf_ref(traj, cloud, thr, strength, window, passes=1):
    """oracle.apf_avoidance as it is, `passes` times.  window = 0: the reference's only weight is exp(-0 / 0) = NaN, so a waypoint
    that is hit becomes NaN -- on the device too (the weights are an input of the kernel)."""
    out = traj.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(passes):
            out = O.apf_avoidance(out.copy(), cloud, thr, strength, window)
    return out


def apf_dynamic_ref(traj, points, thr_query, thr_force, strength, window, affected=None, goal=None, enable=None):
    """oracle.apf_dynamic_avoidance as it is on every enabled row of traj (B, H, S) with one cloud and one goal for all.
    window None = the pursuer pass.  A pursuer pass over no waypoint (affected <= 0) pushes nothing: the oracle's argmin has
    nothing to look at there, so the row is returned as it is."""
    out = traj.copy()
    B, H, _ = traj.shape
    for b in range(B):
        if enable is not None and not enable[b]:
            continue
        if window is None and min(H if affected is None else affected, H) <= 0:
            continue
        out[b] = O.apf_dynamic_avoidance(traj[b], points, thr_query, thr_force, strength, window, affected=affected, goal=goal)
    return out


def costs_ref(traj, cloud, thr):
    """mask: oracle.collision_mask in float32 (the kernel rounds every product and sum once, in the same order, so the comparison
    is exact); path length and smoothness: float64 arithmetic on the same float32 inputs."""
    traj = np.asarray(traj, np.float32)
    mask = O.collision_mask(traj, np.asarray(cloud, np.float32), float(thr))
    return (mask,) + lengths_ref(traj)


def lengths_ref(traj):
    """(path length, smoothness) per row: sums of |xy_{h+1} - xy_h| and |v_{h+1} - v_h| (columns 2 and up) in float64."""
    x = np.asarray(traj, np.float32).astype(np.float64)
    plen = np.sqrt((np.diff(x[:, :, :2], axis=1) ** 2).sum(-1)).sum(-1)
    smooth = np.sqrt((np.diff(x[:, :, 2:], axis=1) ** 2).sum(-1)).sum(-1)
    return plen, smooth


def cost_bar(H):
    """Relative bar of a float32 path length / smoothness against float64: about 3 roundings per segment and a float32 sum of
    H - 1 non-negative terms, (H - 2) u at most, whatever the order."""
    return (H + 4) * U32


def select_totals(mask, plen, smooth, w_s, w_l, dtype=np.float32):
    """The totals of cost.py:56-88 over the free rows, in `dtype`: min-max normalisation, w_s sm + w_l pl."""
    free = ~np.asarray(mask, bool)
    pl, sm = np.asarray(plen, dtype)[free], np.asarray(smooth, dtype)[free]
    with np.errstate(divide="ignore", invalid="ignore"):
        pl = (pl - pl.min()) / (pl.max() - pl.min())
        sm = (sm - sm.min()) / (sm.max() - sm.min())
        return dtype(w_s) * sm + dtype(w_l) * pl


def select_ref(mask, plen, smooth, w_s, w_l):
    """(n_free, rank of the winner among the free rows, its row); (0, -1, -1) without a free row.  np.argmin ranks the first NaN
    first, like torch.argmin and select_block."""
    free = ~np.asarray(mask, bool)
    n_free = int(free.sum())
    if n_free == 0:
        return 0, -1, -1
    rank = int(np.argmin(select_totals(mask, plen, smooth, w_s, w_l)))
    return n_free, rank, int(np.nonzero(free)[0][rank])


def cfg_mean_ref(x, eps, n_rp, w0, w1, sqrt_recip, sqrt_recipm1, coef1, coef2, clip, predict_x0):
    """cfg_mean_kernel in float32 numpy, one rounding per product and sum: x (B, HS), eps (B, n_rp, HS) -> (e_comb, x0, mean)."""
    x, e = np.asarray(x, F), np.asarray(eps, F)
    if n_rp == 2:
        ec = F(1.0 + w0) * e[:, 0] - F(w0) * e[:, 1]
    elif n_rp == 3:
        u = e[:, 2]
        ec = (u + F(w0) * (e[:, 0] - u)) + F(w1) * (e[:, 1] - u)
    else:
        ec = e[:, 0].copy()
    x0 = ec if predict_x0 else F(sqrt_recip) * x - F(sqrt_recipm1) * ec
    if clip:
        x0 = np.minimum(np.maximum(x0, F(-1)), F(1))
    mean = F(coef1) * x0 + F(coef2) * x
    assert ec.dtype == x0.dtype == mean.dtype == np.float32
    return ec, x0, mean


def ddim_finish_ref(x, x0, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, dir_coef):
    """ddim_finish_kernel: mo = (x - sqrt(a_t) x0) / sqrt(1 - a_t); out = sqrt(a_prev) x0 + dir mo, float32."""
    x, x0 = np.asarray(x, F), np.asarray(x0, F)
    mo = (x - F(sqrt_a_t) * x0) / F(sqrt_1m_a_t)
    out = F(sqrt_a_prev) * x0 + F(dir_coef) * mo
    assert out.dtype == np.float32
    return out


def hard_cond_ref(x, idx, val):
    """x (B, H, S), idx (n), val (n, B, S): x[:, idx[k]] = val[k] in order, so a later duplicate wins."""
    out = x.copy()
    for k, h in enumerate(idx):
        out[:, h, :] = val[k]
    return out


# ------------------------------------------------------------------------------------------------ static APF cases
# (H, S, P, window, thr, passes, seed); B = 3, coordinates in [-1, 1], strength 0.1
APF_RANDOM = {
    "h2_p1_w0":      dict(H=2, S=2, P=1, window=0, thr=1.0, passes=1, seed=1),
    "h48_p63_x2":    dict(H=48, S=4, P=63, window=5, thr=0.2, passes=2, seed=2),
    "h48_p1025":     dict(H=48, S=4, P=1025, window=5, thr=0.07, passes=1, seed=3),
    "h64_p2049_w64": dict(H=64, S=6, P=2049, window=64, thr=0.07, passes=1, seed=4),
    "h128_p2500":    dict(H=128, S=16, P=2500, window=7, thr=0.07, passes=1, seed=5),
    "h7_p300_w10":   dict(H=7, S=3, P=300, window=10, thr=0.1, passes=1, seed=6),       # window wider than H
}
APF_STRENGTH = 0.1
TIE_PAIRS = {"same_lane": (5, 69), "other_lane": (5, 70), "next_tile": (5, 1029), "tile_edge": (1023, 1024)}
TIE_P, TIE_H, TIE_H0 = 1100, 7, 3


@functools.lru_cache(maxsize=None)
def apf_random_case(name):
    c = APF_RANDOM[name]
    g = rng(1000 + c["seed"])
    traj = g.uniform(-1, 1, size=(3, c["H"], c["S"])).astype(F)
    cloud = g.uniform(-1, 1, size=(c["P"], 2)).astype(F)
    # the input of every pass, for the margin checks; the last entry is the reference result
    stages = [traj]
    for _ in range(c["passes"]):
        stages.append(apf_ref(stages[-1], cloud, c["thr"], APF_STRENGTH, c["window"]))
    return dict(c, traj=traj, cloud=cloud, stages=stages, ref=stages[-1])


def _far_cloud(g, P, dtype):
    """P points in [-1, -0.75]^2: farther than 0.7 from every designed waypoint (those have y >= 0)."""
    return g.uniform(-1.0, -0.75, size=(P, 2)).astype(dtype)


def _line(g, H, S, h0, x0, y0, step):
    """A straight trajectory along x with waypoint h0 at (x0, y0); the other columns random."""
    t = g.uniform(-1, 1, size=(1, H, S)).astype(F)
    t[0, :, 0] = x0 + (np.arange(H) - h0) * step
    t[0, :, 1] = y0
    return t


@functools.lru_cache(maxsize=None)
def tie_case(name, dtype_name="float32"):
    """Waypoint TIE_H0 of a straight trajectory sits at the origin; points i < j of the pair at (1/16, 0) and (0, 1/16) and the
    last point at (-1/16, 0) are at exactly the same distance, the rest of the cloud is far away.  The lowest index must win:
    the waypoint is pushed along -x and its y stays 0."""
    dt = np.dtype(dtype_name).type
    i, j = TIE_PAIRS[name]
    g = rng(2000 + i + j)
    cloud = _far_cloud(g, TIE_P, dt)
    cloud[i] = (1 / 16, 0); cloud[j] = (0, 1 / 16); cloud[TIE_P - 1] = (-1 / 16, 0)
    traj = _line(g, TIE_H, 3, TIE_H0, 0.0, 0.0, 0.25)
    return dict(traj=traj, cloud=cloud, i=i, j=j, thr=1 / 8, window=2)


@functools.lru_cache(maxsize=None)
def apf_threshold_case(kind):
    """miss: a point at exactly d = 1/8 of the waypoint at the origin with thr = 1/8 ('<' is strict); hit: thr one ulp larger;
    on_point: a waypoint exactly on a point (d = 0: direction 0, nothing moves)."""
    g = rng(3000 + len(kind))
    cloud = _far_cloud(g, 200, F)
    if kind == "on_point":
        traj = _line(g, 7, 3, 3, 0.25, 0.5, 0.25)
        cloud[7] = (0.25, 0.5)
        thr = 1 / 8
    else:
        traj = _line(g, 7, 3, 3, 0.0, 0.0, 0.5)
        cloud[7] = (1 / 8, 0)
        thr = 1 / 8 if kind == "miss" else float(np.nextafter(1 / 8, 1))
    return dict(traj=traj, cloud=cloud, thr=thr, window=2, d=0.0 if kind == "on_point" else 1 / 8)


# ------------------------------------------------------------------------------------------------ dynamic APF cases
DYN_STRENGTH = 0.1
DYN_STATIC = {       # static pass, B = 3, points float64 in [-1, 1]
    "h48_p256":        dict(H=48, S=4, P=256, window=5, thr_query=0.1, thr_force=0.1, seed=1, noop=False),
    "h48_p1025_thr":   dict(H=48, S=4, P=1025, window=5, thr_query=0.15, thr_force=0.1, seed=2, noop=False),   # thr_query != thr_force
    "h128_p3000":      dict(H=128, S=6, P=3000, window=3, thr_query=0.05, thr_force=0.05, seed=3, noop=False),
    "h8_p64_w0":       dict(H=8, S=2, P=64, window=0, thr_query=0.2, thr_force=0.1, seed=4, noop=True),          # [ci, ci) is empty
    "h8_p64_w20":      dict(H=8, S=4, P=64, window=20, thr_query=0.2, thr_force=0.1, seed=5, noop=False),        # window wider than H
    "nohit":           dict(H=48, S=4, P=256, window=5, thr_query=1e-3, thr_force=0.1, seed=6, noop=True),       # nothing within thr_query
}
DYN_AFFECTED = (0, 5, 48, 58)
DYN_PURSUER = dict(H=48, S=4, thr_query=0.2, thr_force=0.1, strength=0.3)


@functools.lru_cache(maxsize=None)
def dyn_static_case(name):
    c = DYN_STATIC[name]
    g = rng(4000 + c["seed"])
    traj = g.uniform(-1, 1, size=(3, c["H"], c["S"])).astype(F)
    points = g.uniform(-1, 1, size=(c["P"], 2))
    ref = apf_dynamic_ref(traj, points, c["thr_query"], c["thr_force"], DYN_STRENGTH, c["window"])
    return dict(c, traj=traj, points=points, ref=ref)


@functools.lru_cache(maxsize=None)
def dyn_designed_case(kind):
    """last: the closest waypoint is H - 1, the reference pushes [ci - w, min(H - 1, ci + w)) and so leaves it where it is;
    twin: waypoints 2 and 6 are equally closest (d = 1/16 exactly), the first is ci, and with window 1 only {1, 2} can move."""
    g = rng(5000 + len(kind))
    H = 8
    points = _far_cloud(g, 64, np.float64)
    traj = g.uniform(-1, 1, size=(1, H, 4)).astype(F)
    traj[0, :, 0] = (-0.75 + 0.25 * np.arange(H)).astype(F)
    traj[0, :, 1] = 0.5
    if kind == "last":
        for k, (h, d) in enumerate(((7, 0.03), (6, 0.05), (5, 0.08))):
            points[k] = traj[0, h, :2].astype(np.float64) + (0.0, d)
        window = 2
    else:
        traj[0, :, 1] = 0.875
        traj[0, 2, :2] = (0.0, 0.0); points[0] = (1 / 16, 0.0)
        traj[0, 6, :2] = (0.5, 0.5); points[1] = (0.5 + 1 / 16, 0.5)
        window = 1
    ref = apf_dynamic_ref(traj, points, 0.1, 0.1, DYN_STRENGTH, window)
    return dict(traj=traj, points=points, thr_query=0.1, thr_force=0.1, window=window, ref=ref)


@functools.lru_cache(maxsize=None)
def dyn_pursuer_inputs(P):
    """B = 3 rows; waypoint 2 of row 1 equals the goal's xy (goal direction 0) and has a point 0.05 away, so it is pushed."""
    c = DYN_PURSUER
    g = rng(6000 + P)
    traj = g.uniform(-1, 1, size=(3, c["H"], c["S"])).astype(F)
    points = g.uniform(-1, 1, size=(P, 2))
    goal = g.uniform(-1, 1, size=c["S"]).astype(F)
    traj[1, 2, :2] = goal[:2]
    points[0] = goal[:2].astype(np.float64) + (0.05, 0.0)
    return traj, points, goal


@functools.lru_cache(maxsize=None)
def dyn_pursuer_case(P, affected, with_goal):
    c = DYN_PURSUER
    traj, points, goal = dyn_pursuer_inputs(P)
    ref = apf_dynamic_ref(traj, points, c["thr_query"], c["thr_force"], c["strength"], None, affected=affected,
                          goal=goal if with_goal else None)
    return dict(c, traj=traj, points=points, goal=goal if with_goal else None, affected=affected, ref=ref)


DYN_PURSUER_CASES = [(64, a, wg) for a in DYN_AFFECTED for wg in (True, False)] + [(1025, 48, True)]
DYN_ENABLE = (1, 0, 1, 0, 1)


@functools.lru_cache(maxsize=None)
def dyn_enable_case():
    c = DYN_STATIC["h48_p256"]
    g = rng(7000)
    traj = g.uniform(-1, 1, size=(5, c["H"], c["S"])).astype(F)
    points = g.uniform(-1, 1, size=(c["P"], 2))
    ref = apf_dynamic_ref(traj, points, c["thr_query"], c["thr_force"], DYN_STRENGTH, c["window"], enable=DYN_ENABLE)
    return dict(c, traj=traj, points=points, ref=ref)


# ------------------------------------------------------------------------------------------------ cost cases
# B = 6, waypoints and points uniform in [-1, 1]; thr small enough that some rows stay free
COST_RANDOM = {
    "h2_p1":      dict(H=2, S=2, P=1, thr=0.8, seed=1),
    "h48_p1023":  dict(H=48, S=4, P=1023, thr=0.004, seed=2),
    "h48_p1025":  dict(H=48, S=4, P=1025, thr=0.004, seed=3),
    "h128_p2500": dict(H=128, S=16, P=2500, thr=0.002, seed=4),
    "h64_s2":     dict(H=64, S=2, P=384, thr=0.006, seed=5),                # S = 2: smoothness is exactly 0
}
# the only colliding (row, waypoint, point); P = 2000 = one full tile and a partial one
COST_DESIGNED = {
    "last_of_last_tile":    dict(row=2, h=17, p=1999),
    "first_of_second_tile": dict(row=4, h=47, p=1024),                      # and the only colliding waypoint is H - 1
    "first_point_h0":       dict(row=0, h=0, p=0),
}
COST_DESIGNED_THR = 0.05


@functools.lru_cache(maxsize=None)
def cost_random_case(name):
    c = COST_RANDOM[name]
    g = rng(8000 + c["seed"])
    traj = g.uniform(-1, 1, size=(6, c["H"], c["S"])).astype(F)
    cloud = g.uniform(-1, 1, size=(c["P"], 2)).astype(F)
    mask, plen, smooth = costs_ref(traj, cloud, c["thr"])
    return dict(c, traj=traj, cloud=cloud, mask=mask, plen=plen, smooth=smooth)


@functools.lru_cache(maxsize=None)
def cost_designed_case(name):
    c = COST_DESIGNED[name]
    g = rng(9000 + c["p"])
    traj = g.uniform(0, 1, size=(6, 48, 4)).astype(F)
    cloud = _far_cloud(g, 2000, F)
    traj[c["row"], c["h"], :2] = (-0.5, 0.5)                       # a quadrant of its own
    cloud[c["p"]] = (-0.5 + 0.01, 0.5)
    mask, plen, smooth = costs_ref(traj, cloud, COST_DESIGNED_THR)
    return dict(c, H=48, thr=COST_DESIGNED_THR, traj=traj, cloud=cloud, mask=mask, plen=plen, smooth=smooth)


@functools.lru_cache(maxsize=None)
def cost_threshold_case(hit):
    """One point at exactly thr = 1/8 of one waypoint: no collision ('<' is strict); with thr one float32 ulp larger: a collision."""
    g = rng(9500)
    traj = g.uniform(0, 1, size=(6, 48, 4)).astype(F)
    traj[3, 20, :2] = (-0.5, 0.5)                                  # a quadrant of its own
    cloud = _far_cloud(g, 1025, F)
    cloud[1024] = (-0.5 + 1 / 8, 0.5)
    thr = float(np.nextafter(F(1 / 8), F(1))) if hit else 1 / 8
    mask, plen, smooth = costs_ref(traj, cloud, thr)
    return dict(H=48, thr=thr, traj=traj, cloud=cloud, mask=mask, plen=plen, smooth=smooth)


# ------------------------------------------------------------------------------------------------ selection cases
PL_LO, PL_RNG, SM_LO, SM_RNG = 1.0, 8.0, 2.0, 32.0       # ranges are powers of two
SELECT_RANDOM = {    # B, seed, planted winner row (None: wherever the random minimum falls)
    "b1": dict(B=1, seed=1, winner=None), "b2": dict(B=2, seed=2, winner=None), "b63": dict(B=63, seed=3, winner=None),
    "b1023": dict(B=1023, seed=4, winner=None), "b1024": dict(B=1024, seed=5, winner=None),
    "b1025_last": dict(B=1025, seed=6, winner=1024),      # the winner is the last row: the second trip of thread 0
    "b3000_r1024": dict(B=3000, seed=7, winner=1024), "b3000": dict(B=3000, seed=8, winner=None),
}
W_S, W_L = 0.1, 0.9
TIE_W_S, TIE_W_L = 0.25, 0.75
# rows of the equal minimum total: the lower must win wherever the reduction meets the other
SELECT_TIES = {"same_thread": (7, 1031), "other_lane": (7, 12), "other_wave": (7, 200), "lower_row_in_later_wave": (70, 1029)}


@functools.lru_cache(maxsize=None)
def select_random_case(name):
    """Random finite scalars and a random mask.  Two free rows pin the ranges ((lo, hi) and (hi, lo)); every other row is drawn
    uniformly and drawn again while its total lies within 2 TOTAL_MARGIN of a total already there, so that no float32 rounding
    can change the order of two rows."""
    c = SELECT_RANDOM[name]
    B, g = c["B"], rng(10000 + c["seed"])
    mask = (g.random(B) < 0.4).astype(np.int32)
    plen = np.empty(B, F); smooth = np.empty(B, F)
    if B == 1:
        mask[0] = 0; plen[0] = 3.0; smooth[0] = 5.0
        return dict(c, mask=mask, plen=plen, smooth=smooth, w_s=W_S, w_l=W_L)
    rows = [r for r in range(B) if r != c["winner"]]
    a, b = (int(v) for v in g.choice(rows, 2, replace=False))
    fixed = {a: (PL_LO, SM_LO + SM_RNG), b: (PL_LO + PL_RNG, SM_LO)}
    floor = 0.0
    if c["winner"] is not None:
        fixed[c["winner"]] = (PL_LO + PL_RNG / 128, SM_LO + SM_RNG / 128)        # total 1 / 128
        floor = 0.05
    taken = set()

    def total(p, s):
        return W_S * (float(F(s)) - SM_LO) / SM_RNG + W_L * (float(F(p)) - PL_LO) / PL_RNG

    for r, (p, s) in fixed.items():
        mask[r] = 0; plen[r] = p; smooth[r] = s
        taken.add(int(total(p, s) / (2 * TOTAL_MARGIN)))
    for r in range(B):
        if r in fixed:
            continue
        while True:
            p, s = g.uniform(PL_LO, PL_LO + PL_RNG), g.uniform(SM_LO, SM_LO + SM_RNG)
            t = total(p, s)
            k = int(t / (2 * TOTAL_MARGIN))
            if t >= floor and not ({k - 1, k, k + 1} & taken):
                break
        taken.add(k); plen[r] = p; smooth[r] = s
    return dict(c, mask=mask, plen=plen, smooth=smooth, w_s=W_S, w_l=W_L)


def _exact_background(B, g):
    """Multiples of 1/8 with totals >= 0.375 under TIE_W_S / TIE_W_L, and the two free rows 0 and 1 that pin the ranges."""
    mask = (g.random(B) < 0.3).astype(np.int32)
    plen = (PL_LO + PL_RNG / 2 + g.integers(0, 33, B) / 8).astype(F)           # 5 .. 9
    smooth = (SM_LO + g.integers(0, 257, B) / 8).astype(F)                    # 2 .. 34
    mask[:2] = 0
    plen[0], smooth[0] = PL_LO, SM_LO + SM_RNG                                 # total 0.25
    plen[1], smooth[1] = PL_LO + PL_RNG, SM_LO                                 # total 0.75
    return mask, plen, smooth


@functools.lru_cache(maxsize=None)
def select_tie_case(name):
    """Two free rows with the total 1/8, reached by different (length, smoothness) pairs; every value is a multiple of 1/8, the
    ranges are powers of two and the weights 1/4 and 3/4, so the float32 arithmetic is exact on both sides."""
    r1, r2 = SELECT_TIES[name]
    B = 2100
    mask, plen, smooth = _exact_background(B, rng(11000 + r1 + r2))
    mask[[r1, r2]] = 0
    plen[r1], smooth[r1] = 2.0, 6.0            # 3/4 * 1/8 + 1/4 * 1/8
    plen[r2], smooth[r2] = 1.5, 12.0           # 3/4 * 1/16 + 1/4 * 5/16
    return dict(B=B, mask=mask, plen=plen, smooth=smooth, w_s=TIE_W_S, w_l=TIE_W_L, rows=(r1, r2))


@functools.lru_cache(maxsize=None)
def select_degenerate_case(kind):
    """all_equal / plen_equal / smooth_equal: a zero range gives 0 / 0 = NaN totals and the first free row wins, which is row 3
    (rows 0 .. 2 collide and carry other values); one_free: only row 1234 is free; none_free: no row is."""
    g = rng(12000 + len(kind))
    if kind in ("one_free", "none_free"):
        B = 1500
        mask = np.ones(B, np.int32)
        plen = g.uniform(1, 9, B).astype(F); smooth = g.uniform(2, 34, B).astype(F)
        if kind == "one_free":
            mask[1234] = 0
    else:
        B = 1100
        mask = (g.random(B) < 0.3).astype(np.int32)
        mask[:3] = 1; mask[3] = 0
        plen = g.uniform(1, 9, B).astype(F); smooth = g.uniform(2, 34, B).astype(F)
        free = mask == 0
        if kind in ("all_equal", "plen_equal"):
            plen[free] = 3.0
        if kind in ("all_equal", "smooth_equal"):
            smooth[free] = 5.0
    return dict(B=B, mask=mask, plen=plen, smooth=smooth, w_s=W_S, w_l=W_L)


SELECT_DEGENERATE = ("all_equal", "plen_equal", "smooth_equal", "one_free", "none_free")


def select_batch(case, all_collide=False):
    """A trajectory batch (B, 3, 4) and a one-point cloud whose costs are the case's arrays exactly: row b runs from the origin
    along x by plen[b] and stays there, its third column steps by smooth[b]; a colliding row starts on the cloud's point."""
    B = case["B"]
    mask = np.ones(B, np.int32) if all_collide else case["mask"]
    traj = np.zeros((B, 3, 4), F)
    traj[:, 1:, 0] = case["plen"][:, None]
    traj[:, 0, 2] = 1.0
    traj[:, 1:, 2] = 1.0 + case["smooth"][:, None]
    traj[:, :, 3] = 0.5
    traj[:, :, 1] = np.where(mask != 0, 100.0, 0.0)[:, None]
    return traj, np.array([[0.0, 100.0]], F), 0.5


# ------------------------------------------------------------------------------------------------ metrics cases
METRIC_H, METRIC_S, METRIC_BOXES = (2, 48, 65, 128), (2, 6), (0, 1, 5)
METRIC_B = 5
# float32-exact, disjoint boxes (centres and sizes are multiples of 1/8)
BOX_CENTERS = np.array([[0.0, 0.0], [-0.5, -0.5], [0.5, -0.5], [-0.5, 0.5], [0.5, 0.5]], F)
BOX_SIZES = np.array([[0.25, 0.375], [0.375, 0.25], [0.25, 0.25], [0.375, 0.375], [0.25, 0.125]], F)
VARIANCE_B = (2, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def metric_case(H, S, n_boxes):
    """Random waypoints in [-1, 1]; with boxes, three waypoints sit exactly on a face of box 0: row 0 on the lower x face, row 1
    on the upper x face, row 2 on the upper y face.  `planted` lists them with the outward direction."""
    g = rng(13000 + 100 * H + 10 * S + n_boxes)
    traj = g.uniform(-1, 1, size=(METRIC_B, H, S)).astype(F)
    centers, sizes = BOX_CENTERS[:n_boxes].copy(), BOX_SIZES[:n_boxes].copy()
    planted = []
    if n_boxes:
        c, s = centers[0], sizes[0]
        traj[0, 0, :2] = (c[0] - s[0] / 2, c[1]); planted.append((0, 0, 0, -1))
        traj[1, H - 1, :2] = (c[0] + s[0] / 2, c[1] + s[1] / 4); planted.append((1, H - 1, 0, +1))
        traj[2, H // 2, :2] = (c[0], c[1] + s[1] / 2); planted.append((2, H // 2, 1, +1))
    intensity = O.collision_intensity(traj, centers, sizes)
    plen, smooth = lengths_ref(traj)
    return dict(traj=traj, centers=centers, sizes=sizes, planted=planted, intensity=intensity, plen=plen, smooth=smooth)


@functools.lru_cache(maxsize=None)
def variance_case(B):
    traj = (rng(14000 + B).standard_normal((B, 4, 4)) * 0.4).astype(F)
    return dict(traj=traj, ref=O.waypoint_variance(traj))


# ------------------------------------------------------------------------------------------------ elementwise cases
CFG_COEF = dict(sqrt_recip=1.7, sqrt_recipm1=2.9, coef1=0.3, coef2=0.69)
CFG_W0, CFG_W1 = 2.0, 1.5
CFG_BIG_B, CFG_HS = 349526 + 1, 6                     # B * HS just above 8192 * 256: the grid-stride loop takes a second trip
CFG_CASES = [dict(n_rp=n, predict_x0=p, clip=c, B=37, HS=CFG_HS) for n in (1, 2, 3) for p in (0, 1) for c in (0, 1)] + \
            [dict(n_rp=2, predict_x0=0, clip=1, B=CFG_BIG_B, HS=CFG_HS)]


@functools.lru_cache(maxsize=None)
def cfg_case(n_rp, predict_x0, clip, B, HS):
    g = rng(15000 + 100 * n_rp + 10 * predict_x0 + clip + B)
    x = g.standard_normal((B, HS), dtype=F)
    eps = g.standard_normal((B, n_rp, HS), dtype=F) * F(0.6)
    ec, x0, mean = cfg_mean_ref(x, eps, n_rp, CFG_W0, CFG_W1, clip=clip, predict_x0=predict_x0, **CFG_COEF)
    return dict(x=x, eps=eps, ecomb=ec, x0=x0, mean=mean)


DDIM_SHAPES = ((1, 5, 2), (5, 48, 4), (8739, 48, 5))   # B H S = 10, 960 and 2097360 > 8192 * 256


def ddim_coefficients(t, T=25):
    """(sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)) of a T-step DDIM at timestep t, from the oracle's schedule."""
    ac = O.make_schedule(T)["alphas_cumprod"]
    a_t = ac[t]
    a_prev = ac[t - 1] if t > 0 else F(1.0)
    return tuple(float(v) for v in (np.sqrt(a_t), np.sqrt(F(1) - a_t), np.sqrt(a_prev), np.sqrt(F(1) - a_prev)))


HARD_N = (1, 3, 256)


@functools.lru_cache(maxsize=None)
def hard_cond_case(n):
    """B = 5, H = 48, S = 4; n = 3 repeats an index, n = 256 repeats every one several times."""
    g = rng(16000 + n)
    x = g.standard_normal((5, 48, 4), dtype=F)
    idx = {1: [47], 3: [0, 17, 0]}.get(n)
    idx = np.array(idx if idx is not None else g.integers(0, 48, n), np.int32)
    val = g.standard_normal((n, 5, 4), dtype=F)
    return dict(x=x, idx=idx, val=val, ref=hard_cond_ref(x, idx, val))
