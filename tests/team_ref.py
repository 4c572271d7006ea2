"""Teams of robots in one job (ramp_team_guide / ramp_team_clearance in include/ramp_hip.h) restated in numpy, generic in dtype: float64 is
the truth, the same code in float32 the yardstick of tests/test_gpu_team.py.  Every product and sum is written in the header's order
(teammates in ascending a', skipping a, added serially; squares added in coordinate order), so the float32 run rounds where the kernel
rounds.  Also the case tables and the inputs the host and GPU tests share, each computed once.  numpy only.

Layout: row b of a (B, H, S) batch is agent b % A of team b // A."""
import numpy as np

from prim_guide_ref import cloud_grad, stencil_grad

F32 = lambda v: float(np.float32(v))      # noqa: E731


# ------------------------------------------------------------------------------------------------ the definition
def _dist(dx):
    d2 = dx[..., 0] * dx[..., 0]
    for c in range(1, dx.shape[-1]):
        d2 = d2 + dx[..., c] * dx[..., c]
    return np.sqrt(d2)


def pair_distances(P):
    """|p_{a,h} - p_{a',h}| for every pair a < a' (pairs in the order (0,1), (0,2), .., (1,2), ..) -> (n_pairs, H) in P's dtype."""
    A = P.shape[0]
    out = [_dist(P[a] - P[o]) for a in range(A) for o in range(a + 1, A)]
    return np.stack(out) if out else np.zeros((0, P.shape[1]), P.dtype)


def team_cost(P, r):
    """C_team of the positions P (A, H, D): sum over pairs a < a' and waypoints of 1/2 max(0, r - d)^2, values in P's dtype, float64 sum."""
    dt = P.dtype.type
    u = np.maximum(dt(0), dt(r) - pair_distances(P))
    return float((dt(0.5) * (u * u)).astype(np.float64).sum())


def team_row_cost(P, r):
    """Per agent a, sum_{a' != a} sum_h 1/2 (r - d)^2 over the pairs with d < r (column 3 of ramp_guide_cost_team): (A,) float64."""
    dt = P.dtype.type
    A = P.shape[0]
    out = np.zeros(A)
    for a in range(A):
        for o in range(A):
            if o == a:
                continue
            u = np.maximum(dt(0), dt(r) - _dist(P[a] - P[o]))
            out[a] += float((dt(0.5) * (u * u)).astype(np.float64).sum())
    return out


def team_grad(P, r):
    """dC_team/dp (A, H, D) in P's dtype: guide_pair_force's arithmetic, the teammate's waypoint in the place of a cloud point; teammates in
    ascending a', skipping a, added serially.  A pair at distance 0 contributes nothing."""
    dt = P.dtype.type
    A = P.shape[0]
    g = np.zeros_like(P)
    for a in range(A):
        for o in range(A):
            if o == a:
                continue
            dx = P[a] - P[o]
            d = _dist(dx)
            inside = (d < dt(r)) & (d > 0)
            f = np.where(inside, (dt(r) - d) / np.where(inside, d, dt(1)), dt(0)).astype(P.dtype)
            g[a] = g[a] - f[:, None] * dx
    return g


def iterate(x, A, clouds, traj_scene, pins, k, step, n_iter, max_norm, dtype, D, log=None):
    """n_iter Jacobi iterations on the rows x (B, H, S) in team layout -> new array of ``dtype``.  clouds: per scene (P, D); traj_scene (B,) or
    None (a team with a row whose scene is outside the list stays as a whole); pins {waypoint: (S,) or (B, S)} (later entries win);
    k: radius, radius_team, w_obs, w_team, w_smooth, w_acc.  ``log`` collects, per team and iteration (and once more behind the last one,
    iteration n_iter), (team, iteration, smallest pair distance, pairs inside radius_team) and, per agent step, (team, iteration, agent, s)."""
    out = np.array(x, dtype=dtype)
    dt = out.dtype.type
    B, H, S = out.shape
    team_on = A > 1 and k.get("w_team", 0.0) != 0
    for t in range(B // A):
        rows = list(range(t * A, (t + 1) * A))
        scs = [0 if traj_scene is None else int(traj_scene[b]) for b in rows]
        if any(not 0 <= s < len(clouds) for s in scs):
            continue
        P = out[rows][:, :, :D].copy()
        free = np.ones((A, H), bool)
        for h, v in pins.items():
            v = np.asarray(v)
            for a, b in enumerate(rows):
                P[a, h] = (v if v.ndim == 1 else v[b])[:D].astype(dtype)
                free[a, h] = False
        for it in range(n_iter + 1):
            if log is not None and A > 1:
                d = pair_distances(P)
                log.append(("pairs", t, it, float(d.min()), int((d < k["radius_team"]).sum())))
            if it == n_iter:
                break
            gt = team_grad(P, k["radius_team"]) if team_on else None
            new = P.copy()
            for a in range(A):
                g = stencil_grad(P[a], k.get("w_smooth", 0.0), k.get("w_acc", 0.0))
                if team_on:
                    g = dt(k["w_team"]) * gt[a] + g
                c = np.asarray(clouds[scs[a]]).reshape(-1, D)
                if len(c) and k.get("w_obs", 0.0) != 0:
                    g = dt(k["w_obs"]) * cloud_grad(P[a], c, k["radius"]) + g
                g = g.astype(dtype)
                g[~free[a]] = 0
                nrm = dt(np.sqrt((g.astype(np.float64) ** 2).sum()))
                s = min(dt(1), dt(max_norm) / nrm) if (max_norm > 0 and nrm > 0) else dt(1)
                if log is not None:
                    log.append(("step", t, it, a, float(s), float(nrm)))
                new[a][free[a]] = (P[a] - (dt(step) * dt(s)) * g)[free[a]]
            P = new
        for a, b in enumerate(rows):
            out[b, free[a], :D] = P[a][free[a]]
    return out


def segment_distances(P):
    """The closed-form closest approach of every pair a < a' on every synchronous segment: (n_pairs, H - 1) in P's dtype.  D0, D1 the
    differences at both ends, e = D1 - D0, t = clamp(-(D0 . e) / |e|^2, 0, 1) (0 when |e|^2 == 0), |D0 + t e| min-ed with |D0| and |D1|."""
    dt = P.dtype.type
    A, H, D = P.shape
    out = []
    for a in range(A):
        for o in range(a + 1, A):
            dd = P[a] - P[o]
            d0, d1 = dd[:-1], dd[1:]
            e = d1 - d0
            e2 = e[:, 0] * e[:, 0]
            dot = d0[:, 0] * e[:, 0]
            for c in range(1, D):
                e2 = e2 + e[:, c] * e[:, c]
                dot = dot + d0[:, c] * e[:, c]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = np.where(e2 > 0, np.clip(-dot / np.where(e2 > 0, e2, dt(1)), dt(0), dt(1)), dt(0)).astype(P.dtype)
            v = d0 + t[:, None] * e
            out.append(np.minimum(np.minimum(_dist(v), _dist(d0)), _dist(d1)))
    return np.stack(out) if out else np.zeros((0, H - 1), P.dtype)


def clearance(P, min_sep):
    """(sep_wp, sep_seg, wp_conflicts, seg_conflicts) of one team P (A, H, D) in P's dtype: NaN separations and all counts at their maximum
    with a non-finite coordinate, +inf and zero counts for A == 1."""
    A, H, D = P.shape
    n_pairs = A * (A - 1) // 2
    if not np.isfinite(P).all():
        return float("nan"), float("nan"), n_pairs * H, n_pairs * (H - 1)
    if A == 1:
        return float("inf"), float("inf"), 0, 0
    dw, ds = pair_distances(P), segment_distances(P)
    m = P.dtype.type(min_sep)
    return float(dw.min()), float(min(ds.min(), dw.min())), int((dw < m).sum()), int((ds < m).sum())


def select_teams(team_first, mask, plen, smooth, w_s, w_l):
    """The rule of ramp_select_scored_scenes on team-level arrays, in float32 like the kernel: per scene (n_free, index among the free teams,
    team in the batch) -- (0, -1, -1) without a free team; min-max normalised length and smoothness over the scene's free teams."""
    out = []
    f = np.float32
    for s in range(len(team_first) - 1):
        lo, hi = int(team_first[s]), int(team_first[s + 1])
        free = [i for i in range(lo, hi) if not mask[i]]
        if not free:
            out.append((0, -1, -1))
            continue
        pl, sm = np.array([plen[i] for i in free], f), np.array([smooth[i] for i in free], f)
        with np.errstate(divide="ignore", invalid="ignore"):
            tot = f(w_s) * ((sm - sm.min()) / (sm.max() - sm.min())) + f(w_l) * ((pl - pl.min()) / (pl.max() - pl.min()))
        j = int(np.argmin(tot))      # (a NaN total -- 0 / 0 when the free teams tie -- ranks first, as in torch.argmin)
        out.append((len(free), j, free[j]))
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by the tests
RADIUS = F32(0.35)          # the cloud term's radius
RADIUS_TEAM = F32(0.3)      # r_t
STEP = F32(2e-3)
WEIGHTS = dict(w_obs=1.0, w_team=1.0, w_smooth=0.5, w_acc=0.25)
OUTSIDE = 7                 # the scene index of the fourth team: outside the table of two scenes
# (A, H, S, D, P, n_iter, clip): every value of A in {2, 3, 8}, H in {8, 47, 128}, (S, D) in {(4, 2), (6, 3)}, P in {0, 70, 1100} (1100 is
# past one tile of 1024 points), n_iter in {1, 3}, the clip on and off; (8, 128, 6, 3) is the LDS maximum
STEP_CASES = [(2, 8, 4, 2, 70, 1, True), (3, 47, 6, 3, 1100, 3, False), (8, 128, 6, 3, 1100, 3, True), (8, 47, 4, 2, 0, 3, False),
              (2, 128, 4, 2, 1100, 3, True), (3, 8, 6, 3, 70, 1, False), (2, 47, 6, 3, 0, 1, True), (8, 8, 4, 2, 70, 3, True)]
_STEP = {}


def team_rows(n_teams, A, H, S, D, seed, ring=0.1, jitter=0.02):
    """(n_teams * A, H, S) float32 rows in team layout: every team follows a rough common path (uniform in [-0.7, 0.7] per waypoint), agent a
    displaced to its place on a ring of radius ``ring`` around it plus a jitter of +-``jitter`` per coordinate: neighbours on the ring are
    2 ring sin(pi / A) apart, so pairs sit inside r_t = 0.3 and never closer than that minus 2 sqrt(D) jitter.  Channels >= D are uniform."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=(n_teams * A, H, S)).astype(np.float32)
    for t in range(n_teams):
        base = rng.uniform(-0.7, 0.7, size=(H, D))
        for a in range(A):
            off = np.zeros(D)
            off[0], off[1] = ring * np.cos(2 * np.pi * a / A), ring * np.sin(2 * np.pi * a / A)
            x[t * A + a, :, :D] = (base + off + rng.uniform(-jitter, jitter, size=(H, D))).astype(np.float32)
    return x


def uniform(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def step_case(case):
    """Inputs and both restatements of one step case, computed once: four teams (scenes 0, 1, 0 and one outside the table), two clouds of P
    and (P + 1) // 2 points, pins at both ends and mid-path with per-row values (the row's own position moved by +-0.01), max_norm the
    geometric mean of the smallest and largest first-iteration gradient norm of an agent (clip on) or 0."""
    if case not in _STEP:
        A, H, S, D, P, n_iter, clip = case
        seed = 4000 + 10 * STEP_CASES.index(case)
        x = team_rows(4, A, H, S, D, seed)
        B = 4 * A
        clouds = [uniform((P, D), seed + 1), uniform(((P + 1) // 2, D), seed + 2)]
        ts = np.repeat(np.array([0, 1, 0, OUTSIDE], np.int32), A)
        idx = [0, H // 2, H - 1]
        val = (x[:, idx].transpose(1, 0, 2) + np.random.default_rng(seed + 3).uniform(-0.01, 0.01, size=(3, B, S))).astype(np.float32)
        pins = {h: val[j] for j, h in enumerate(idx)}
        k = dict(WEIGHTS, radius=RADIUS, radius_team=RADIUS_TEAM)
        max_norm = 0.0
        if clip:
            probe = []
            iterate(x, A, clouds, ts, pins, k, STEP, 1, 0.0, np.float64, D, log=probe)
            norms = [e[5] for e in probe if e[0] == "step"]
            max_norm = F32(np.sqrt(min(norms) * max(norms)))
        log = []
        y64 = iterate(x, A, clouds, ts, pins, k, STEP, n_iter, max_norm, np.float64, D, log=log)
        y32 = iterate(x, A, clouds, ts, pins, k, STEP, n_iter, max_norm, np.float32, D)
        _STEP[case] = dict(x=x, clouds=clouds, ts=ts, idx=idx, val=val, pins=pins, k=k, max_norm=max_norm, y64=y64, y32=y32, log=log)
    return _STEP[case]


def step_conditions(case):
    """What the inputs of a step case must satisfy, from the float64 restatement: (bar = 4 d32, moved, the smallest pair distance over all
    iterations, the fewest pairs inside r_t in any iteration of any team, the first-iteration scale factors)."""
    c = step_case(case)
    pairs = [e for e in c["log"] if e[0] == "pairs"]
    d32 = float(np.abs(c["y32"] - c["y64"]).max())
    return dict(bar=4 * d32, d32=d32, moved=float(np.abs(c["y64"] - c["x"]).max()), min_dist=min(e[3] for e in pairs),
                min_active=min(e[4] for e in pairs), s_first=[e[4] for e in c["log"] if e[0] == "step" and e[2] == 0])


# the clearance cases: (A, H, S, D, min_sep); three teams each, the agents on a ring of radius 0.1 with a jitter of 0.04, so that the pair
# distances straddle min_sep
CLEAR_CASES = [(2, 8, 4, 2, F32(0.2)), (3, 47, 6, 3, F32(0.175)), (8, 128, 6, 3, F32(0.08)), (8, 47, 4, 2, F32(0.1)), (2, 128, 4, 2, F32(0.19))]
_CLEAR = {}


def clear_case(case):
    """Rows of a clearance case and, per team, the float64 and float32 restatements and the smallest relative gap |d / min_sep - 1| of any
    waypoint or segment distance (float64): the counts are exact where that gap is >= 1e-4."""
    if case not in _CLEAR:
        A, H, S, D, min_sep = case
        x = team_rows(3, A, H, S, D, 5000 + CLEAR_CASES.index(case), ring=0.1, jitter=0.04)
        r64, r32, gap = [], [], []
        for t in range(3):
            P = x[t * A:(t + 1) * A, :, :D]
            r64.append(clearance(P.astype(np.float64), min_sep))
            r32.append(clearance(P, min_sep))
            d = np.concatenate([pair_distances(P.astype(np.float64)).ravel(), segment_distances(P.astype(np.float64)).ravel()])
            gap.append(float(np.abs(d / float(min_sep) - 1).min()))
        _CLEAR[case] = dict(x=x, r64=r64, r32=r32, gap=gap)
    return _CLEAR[case]


def swap_case(S=4):
    """Two agents that swap places through a point between two waypoints: agent 0 runs along y = 0 from x = -0.35 to x = +0.35 in 8 steps of
    0.1, agent 1 the other way, so that they pass through each other in the middle of segment 3 -> 4.  The closest waypoints are 0.1 apart
    (x = -0.05 against x = +0.05), the segment distance there is 0.  With min_sep = 0.05: sep_wp > min_sep, sep_seg < min_sep."""
    xs = (np.arange(8) * 0.1 - 0.35).astype(np.float32)
    x = np.zeros((2, 8, S), np.float32)
    x[0, :, 0], x[1, :, 0] = xs, -xs
    return x, F32(0.05)


def parallel_case(S=4):
    """Two agents in parallel motion 0.25 apart (|e| = 0 on every segment): every separation is 0.25 exactly, nothing conflicts at 0.2."""
    xs = (np.arange(8) * 0.125 - 0.5).astype(np.float32)
    x = np.zeros((2, 8, S), np.float32)
    x[0, :, 0], x[1, :, 0] = xs, xs
    x[1, :, 1] = 0.25
    return x, F32(0.2)
