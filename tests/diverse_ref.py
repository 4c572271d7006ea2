"""Cases of the diverse selection (ramp_select_diverse_scenes) and the conditions they keep, shared by tests/test_diverse_host.py (which
proves the conditions and the properties of ``cost.diverse_reference`` on the CPU) and tests/test_gpu_diverse.py (which runs the cases on
the device).  numpy only.  Case builders are cached: a case and its reference are computed once per process and must not be modified.

Every input is a float32 array, so the float64 reference reads the values the kernels read.  Conditions (checked, never skipped: a seed
that misses one is replaced):
  * no two free totals of a scene closer than planner_ref.TOTAL_MARGIN, unless designed equal;
  * no distance of a free row to a representative within DIST_MARGIN (relative) of min_sep, unless the case is designed to sit on it;
  * the two smallest distances of a free row to the representatives not within DIST_MARGIN (relative) of each other: the fp32 distance
    is within SEP_BAR of the float64 one, so with this margin both pick the same nearest slot."""
import functools

import numpy as np

import planner_ref as P
from ramp_amd.cost import diverse_reference

F = np.float32
DIST_MARGIN = 1e-5
# about 7 fp32 roundings in d^2 (D = 3: three differences, three squares, two sums, one of each shared), halved by the root, one for the
# root and one for the final rounding of the mean
SEP_BAR = 8 * 2.0 ** -24
W_S, W_L = P.W_S, P.W_L
SHAPES = ((2, 2, 2), (8, 4, 2), (48, 4, 2), (64, 6, 3), (128, 16, 3))
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 3000)        # wave and block-stride boundaries of the pick, the sizes SELECT_RANDOM uses


def scored(n, g, p_hit=0.3):
    """mask, path lengths and smoothnesses of n rows, planner_ref.select_random_case's way: two free rows pin the ranges, every other
    row is drawn again while its total lies within 2 TOTAL_MARGIN of one already there."""
    mask = (g.random(n) < p_hit).astype(np.int32)
    plen = np.empty(n, F); smooth = np.empty(n, F)
    if n == 1:
        return np.zeros(1, np.int32), np.full(1, 3.0, F), np.full(1, 5.0, F)
    a, b = (int(v) for v in g.choice(n, 2, replace=False))
    fixed = {a: (P.PL_LO, P.SM_LO + P.SM_RNG), b: (P.PL_LO + P.PL_RNG, P.SM_LO)}

    def total(p, s):
        return W_S * (float(F(s)) - P.SM_LO) / P.SM_RNG + W_L * (float(F(p)) - P.PL_LO) / P.PL_RNG

    taken = set()
    for r, (p, s) in fixed.items():
        mask[r] = 0; plen[r] = p; smooth[r] = s
        taken.add(int(total(p, s) / (2 * P.TOTAL_MARGIN)))
    for r in range(n):
        if r in fixed:
            continue
        while True:
            p, s = g.uniform(P.PL_LO, P.PL_LO + P.PL_RNG), g.uniform(P.SM_LO, P.SM_LO + P.SM_RNG)
            k = int(total(p, s) / (2 * P.TOTAL_MARGIN))
            if not ({k - 1, k, k + 1} & taken):
                break
        taken.add(k); plen[r] = p; smooth[r] = s
    return mask, plen, smooth


def profile(H):
    """A detour's shape over the horizon, nowhere zero (so H = 2 separates rows too)."""
    return np.sin(np.pi * (np.arange(H) + 0.5) / H)


def detours(n, H, S, D, g, amp=None, jitter=0.02):
    """n rows from start to goal along x with a sinusoidal detour of amplitude amp[b] in y (and amp2[b] / 2 in z), every coordinate jittered
    by at most `jitter`; the other state entries random.  Distances between rows spread continuously with the amplitudes."""
    t = g.uniform(-1, 1, size=(n, H, S)).astype(F)
    amp = g.uniform(-1, 1, n) if amp is None else np.asarray(amp, np.float64)
    t[:, :, 0] = (np.linspace(-1, 1, H)[None, :] + g.uniform(-jitter, jitter, (n, H))).astype(F)
    t[:, :, 1] = (amp[:, None] * profile(H)[None, :] + g.uniform(-jitter, jitter, (n, H))).astype(F)
    if D == 3:
        t[:, :, 2] = (0.5 * g.uniform(-1, 1, n)[:, None] * profile(H)[None, :] + g.uniform(-jitter, jitter, (n, H))).astype(F)
    return t


def assemble(scenes):
    """[(traj, mask, plen, smooth)] -> one batch with its table; an entry of 0 rows is an empty scene."""
    first = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in scenes])]).astype(np.int32)
    return dict(traj=np.ascontiguousarray(np.concatenate([s[0] for s in scenes])), first=first,
                mask=np.concatenate([s[1] for s in scenes]).astype(np.int32), plen=np.concatenate([s[2] for s in scenes]).astype(F),
                smooth=np.concatenate([s[3] for s in scenes]).astype(F))


def random_scene(n, H, S, D, g, kind="random"):
    t = detours(n, H, S, D, g)
    if n == 0:
        return t, np.zeros(0, np.int32), np.zeros(0, F), np.zeros(0, F)
    mask, plen, smooth = scored(n, g)
    if kind == "none_free":
        mask[:] = 1
    elif kind == "one_free":
        mask[:] = 1; mask[n // 2] = 0
    elif kind == "tight":                                # every row but two within a narrow band: fewer than K separable rows
        amp = g.uniform(-0.02, 0.02, n); amp[n // 3] = 0.9; amp[2 * n // 3] = -0.7
        t = detours(n, H, S, D, g, amp=amp, jitter=0.005)
    return t, mask, plen, smooth


RAGGED_SIZES = tuple((n, "random") for n in SIZES) + ((0, "random"), (40, "none_free"), (70, "one_free"), (300, "tight"))
SMALL_SIZES = ((65, "random"), (0, "random"), (1025, "random"), (3, "none_free"), (5, "one_free"), (200, "tight"))
# seeds for which every condition above holds (test_diverse_host.py checks them)
RAGGED_SEED = 2
SMALL_SEED = {(2, 2, 2): 1, (8, 4, 2): 1, (48, 4, 2): 1, (64, 6, 3): 2, (128, 16, 3): 2}
MIN_SEP = {"mean": 0.25, "max": 0.375}


@functools.lru_cache(maxsize=None)
def ragged_case():
    """Every size of SIZES, an empty scene, one without a free row, one with a single free row and one with fewer than K separable rows, in
    one batch at (H, S, D) = (48, 4, 2)."""
    g = P.rng(20000 + RAGGED_SEED)
    return dict(assemble([random_scene(n, 48, 4, 2, g, kind) for n, kind in RAGGED_SIZES]), H=48, S=4, D=2)


@functools.lru_cache(maxsize=None)
def small_case(H, S, D):
    g = P.rng(21000 + 100 * H + SMALL_SEED[(H, S, D)])
    return dict(assemble([random_scene(n, H, S, D, g, kind) for n, kind in SMALL_SIZES]), H=H, S=S, D=D)


@functools.lru_cache(maxsize=None)
def reference(case_fn, args, k, min_sep, metric):
    c = case_fn(*args)
    return diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], W_S, W_L, k, min_sep, metric, c["D"])


def scene_slice(c, s):
    """Scene s of a batch as a batch of its own."""
    lo, hi = int(c["first"][s]), int(c["first"][s + 1])
    return dict(traj=np.ascontiguousarray(c["traj"][lo:hi]), first=np.array([0, hi - lo], np.int32), mask=c["mask"][lo:hi],
                plen=c["plen"][lo:hi], smooth=c["smooth"][lo:hi], H=c["H"], S=c["S"], D=c["D"]), lo, hi


# ------------------------------------------------------------------------------------------------ the conditions
def totals_gap(c, w_s=W_S, w_l=W_L):
    """The smallest gap between two free float32 totals of one scene (inf when no scene has two; NaN totals are left out)."""
    gap = np.inf
    for s in range(len(c["first"]) - 1):
        lo, hi = int(c["first"][s]), int(c["first"][s + 1])
        if (c["mask"][lo:hi] == 0).sum() >= 2:
            t = np.sort(P.select_totals(c["mask"][lo:hi], c["plen"][lo:hi], c["smooth"][lo:hi], w_s, w_l).astype(np.float64))
            t = t[~np.isnan(t)]
            if t.size >= 2:
                gap = min(gap, float(np.diff(t).min()))
    return gap


def distance_margins(c, ref, min_sep):
    """(smallest relative |d - min_sep| / min_sep over free rows and the representatives that are not the row itself, smallest relative gap
    between the two smallest distances of one free row to the representatives); inf where there is nothing to compare."""
    ms = float(F(min_sep))
    at_sep, between = np.inf, np.inf
    for s, d in enumerate(ref["dist"]):
        lo, hi = int(c["first"][s]), int(c["first"][s + 1])
        if d.shape[0] == 0:
            continue
        free = c["mask"][lo:hi] == 0
        d = d[:, free].copy()
        reps = ref["rows"][s][ref["rows"][s] >= 0] - lo
        idx = np.nonzero(free)[0]
        for j, r in enumerate(reps):
            d[j, idx == r] = np.nan                       # a representative's distance to itself decides nothing
        with np.errstate(invalid="ignore"):
            if ms > 0 and np.isfinite(d).any():
                at_sep = min(at_sep, float(np.nanmin(np.abs(d - ms)) / ms))
            if d.shape[0] >= 2:
                srt = np.sort(d, axis=0)                  # NaN last
                gaps = (srt[1] - srt[0]) / np.maximum(srt[1], 1e-300)      # only the two nearest can swap
                if np.isfinite(gaps).any():
                    between = min(between, float(np.nanmin(gaps)))
    return at_sep, between


def conditions_hold(c, ref, min_sep, designed_totals=False, designed_sep=False, designed_between=False):
    at_sep, between = distance_margins(c, ref, min_sep)
    return ((designed_totals or totals_gap(c) >= P.TOTAL_MARGIN) and (designed_sep or at_sep > DIST_MARGIN)
            and (designed_between or between > DIST_MARGIN))


# ------------------------------------------------------------------------------------------------ designed cases
PLANTED_M, PLANTED_N = 5, 1030
PLANTED_AMP = (-0.8, -0.4, 0.0, 0.4, 0.8)
PLANTED_EPS = 0.03              # within a bundle: every coordinate jittered by <= 0.01, so two rows differ by <= 0.02 sqrt(2) < 0.03 per waypoint
PLANTED_SEP = 0.125             # eps < min_sep < delta in both metrics: mean |0.4 sin| - eps > 0.22


@functools.lru_cache(maxsize=None)
def planted_case():
    """M bundles of sinusoidal detours of different amplitude and sign round a central obstacle, rows interleaved (bundle = row mod M)."""
    g = P.rng(22000)
    n = PLANTED_N
    amp = np.asarray(PLANTED_AMP)[np.arange(n) % PLANTED_M]
    t = detours(n, 48, 4, 2, g, amp=amp, jitter=0.01)
    mask, plen, smooth = scored(n, g, p_hit=0.2)
    return dict(assemble([(t, mask, plen, smooth)]), H=48, S=4, D=2, bundle=np.arange(n) % PLANTED_M)


@functools.lru_cache(maxsize=None)
def tie_case(name):
    """planner_ref.select_tie_case: two free rows share the smallest total exactly (weights TIE_W_S / TIE_W_L)."""
    c = P.select_tie_case(name)
    t = detours(c["B"], 8, 4, 2, P.rng(23000 + sum(c["rows"])))
    return dict(assemble([(t, c["mask"], c["plen"], c["smooth"])]), H=8, S=4, D=2, rows=c["rows"], w_s=c["w_s"], w_l=c["w_l"])


@functools.lru_cache(maxsize=None)
def all_tie_case():
    """planner_ref.select_degenerate_case('all_equal'): every free total is 0 / 0, the order is the rows'."""
    c = P.select_degenerate_case("all_equal")
    t = detours(c["B"], 8, 4, 2, P.rng(23500))
    return dict(assemble([(t, c["mask"], c["plen"], c["smooth"])]), H=8, S=4, D=2)


@functools.lru_cache(maxsize=None)
def threshold_case(H, D):
    """Row 1 is the cheapest; row 4 is row 1 displaced by exactly 0.25 in the last position coordinate at every waypoint (coordinates are
    multiples of 1/8: d = 0.25 exactly in both metrics); the other rows are far from both."""
    g = P.rng(24000 + H + D)
    n, S = 6, D + 2
    t = (g.integers(-8, 9, size=(n, H, S)) / 8).astype(F)
    t[:, :, 0] += F(4.0) * np.arange(n, dtype=F)[:, None]          # rows 4 apart in x
    t[4] = t[1]; t[4, :, D - 1] += F(0.25)
    mask = np.zeros(n, np.int32); mask[0] = 1
    plen = np.array([1, 1, 5, 9, 2, 6], F); smooth = np.array([2, 2, 34, 10, 4, 20], F)
    return dict(assemble([(t, mask, plen, smooth)]), H=H, S=S, D=D)


REPLAY_K, REPLAY_SEP = 8, 0.125


@functools.lru_cache(maxsize=None)
def replay_case():
    """What replaces small_case(48, 4, 2) in its buffers before a captured call is replayed: its rows in reverse and the costs of another batch."""
    a, b = small_case(48, 4, 2), small_case(8, 4, 2)
    return dict(a, traj=np.ascontiguousarray(a["traj"][::-1]), mask=b["mask"], plen=b["plen"], smooth=b["smooth"])


def nan_rows(metric):
    """Rows of scene 0 of small_case(48, 4, 2) that get NaN positions: (a colliding row, a free row that is not first in the order, the row
    that is)."""
    c = small_case(48, 4, 2)
    winner = int(reference(small_case, (48, 4, 2), 16, MIN_SEP[metric], metric)["rows"][0, 0])
    hit = int(np.nonzero(c["mask"][:65] != 0)[0][0])
    other = int(np.nonzero((c["mask"][:65] == 0) & (np.arange(65) != winner))[0][0])
    return hit, other, winner


def with_nan_row(c, row, free):
    """The batch with NaN positions in `row`, which is made free or colliding."""
    out = dict(c, traj=c["traj"].copy(), mask=c["mask"].copy())
    out["traj"][row, :, :c["D"]] = np.nan
    out["mask"][row] = 0 if free else 1
    return out
