"""Host side of the diverse selection (``ramp_select_diverse_scenes`` and the Python layers over it): the symbol, every refusal that needs
no device, the properties of the numpy statement ``cost.diverse_reference`` on random and designed inputs, and the conditions the cases of
tests/test_gpu_diverse.py need of their inputs (tests/diverse_ref.py).  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import diverse_ref as R
import planner_ref as P
from ramp_amd import _lib, cost

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ramp_select_diverse_scenes"
K_MAX = 16


# ------------------------------------------------------------------------------------------------ the C side
def test_symbol_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    assert re.search(rf"\bint {NAME}\s*\(", hdr), "not declared"
    assert NAME in _lib.PROTOTYPES and len(_lib.PROTOTYPES[NAME][1]) == 23
    assert hasattr(_lib.load(), NAME), "not exported"
    assert re.search(r"#define RAMP_DIVERSE_MAX_K 16\b", hdr) and cost.DIVERSE_MAX_K == K_MAX
    assert "2 * B + n_scenes 32-bit words" in hdr                        # the documented scratch size
    assert len(_lib.PROTOTYPES["ramp_select_scored_scenes"][1]) == 14    # the existing entry keeps its signature


P_ = 0x1000       # a pointer no refused call dereferences
GOOD = dict(traj=P_, B=4, H=8, S=6, point_dim=3, traj_first=P_, n_scenes=1, mask=P_, path_len=P_, smooth=P_, w_smooth=0.1, w_len=0.9, K=4,
            min_sep=0.25, metric=0, best_out=P_, rows_out=P_, result_dev=P_, mode_of=P_, sep_out=P_, mode_count=P_, scratch=P_, stream=None)


def refused(lib, **kw):
    """The call is refused on the host: non-zero, the entry's name in ramp_last_error.  Returns the message."""
    rc = getattr(lib, NAME)(*{**GOOD, **kw}.values())
    msg = lib.ramp_last_error().decode()
    assert rc != 0 and NAME in msg, (kw, rc, msg)
    return msg


def check_every_refusal(lib, **real):
    """Every refusal of the entry (shared with the GPU test: there the same calls, on real arrays, must launch nothing either)."""
    for K in (0, -1, K_MAX + 1):
        assert "K must be" in refused(lib, **real, K=K)
    for ms in (-1e-6, -math.inf, math.nan):
        assert "min_sep" in refused(lib, **real, min_sep=ms)
    for m in (-1, 2):
        assert "metric" in refused(lib, **real, metric=m)
    for d in (1, 4, 0):
        assert "point_dim" in refused(lib, **real, point_dim=d)
    assert "point_dim" in refused(lib, **real, point_dim=3, S=2)
    for H in (0, -3, 129):
        assert "horizon" in refused(lib, **real, H=H)
    assert "B must not" in refused(lib, **real, B=-1) and "n_scenes" in refused(lib, **real, n_scenes=0)
    for k in ("traj", "traj_first", "mask", "path_len", "smooth", "best_out", "rows_out", "result_dev", "mode_of", "sep_out", "mode_count",
              "scratch"):
        assert "null" in refused(lib, **{**real, k: None})


def test_host_refusals():
    check_every_refusal(_lib.load())


def test_python_refusals_come_before_any_device_work():
    t = torch.zeros(4, 8, 4)                 # a CPU tensor: a ValueError must come first, the CPU refusal after it
    arrays = (torch.tensor([0, 4]), torch.zeros(4), torch.ones(4), torch.ones(4))
    for fn, args in ((cost.select_diverse_clear_scenes, ([4],)), (cost.select_diverse_scored_scenes, arrays)):
        for k in (0, -1, K_MAX + 1, 2.0, None, True):
            with pytest.raises(ValueError, match="k must be"):
                fn(t, *args, k=k, min_sep=0.1)
        for ms in (-0.1, float("nan"), None, "0.1"):
            with pytest.raises(ValueError, match="min_sep"):
                fn(t, *args, k=2, min_sep=ms)
        for m in ("median", 0, None):
            with pytest.raises(ValueError, match="metric"):
                fn(t, *args, k=2, min_sep=0.1, metric=m)
        with pytest.raises(_lib.RampHipError, match="no CPU path"):
            fn(t, *args, k=2, min_sep=0.1)
    with pytest.raises(ValueError, match="point_dim"):
        cost.select_diverse_scored_scenes(t, *arrays, k=2, min_sep=0.1, point_dim=5)


# ------------------------------------------------------------------------------------------------ the numpy statement
def order_of(mask, plen, smooth, w_s=R.W_S, w_l=R.W_L):
    """The free rows in the order of the definition, from planner_ref's totals: NaN totals first by row, then (total, row)."""
    free = np.nonzero(np.asarray(mask) == 0)[0]
    if free.size == 0:
        return []
    tot = P.select_totals(mask, plen, smooth, w_s, w_l)
    return [int(free[i]) for i in sorted(range(free.size), key=lambda i: (0, 0.0, free[i]) if np.isnan(tot[i]) else (1, float(tot[i]), free[i]))]


def distances(c, rows, reps, metric):
    """(len(reps), len(rows)) float64 distances of the definition."""
    p = c["traj"][:, :, :c["D"]].astype(np.float64)
    n = np.sqrt(((p[rows][None] - p[reps][:, None]) ** 2).sum(-1))
    return n.max(-1) if metric == "max" else n.sum(-1) / n.shape[-1]


def check_properties(c, ref, k, min_sep, metric, w_s=R.W_S, w_l=R.W_L):
    """What the definition promises, checked on a reference result without using its own bookkeeping."""
    ms = float(np.float32(min_sep))
    for s in range(len(c["first"]) - 1):
        lo, hi = int(c["first"][s]), int(c["first"][s + 1])
        mask, plen, smooth = c["mask"][lo:hi], c["plen"][lo:hi], c["smooth"][lo:hi]
        order = [lo + b for b in order_of(mask, plen, smooth, w_s, w_l)]
        reps = [int(r) for r in ref["rows"][s] if r >= 0]
        n_free = len(order)
        assert ref["result"][s].tolist() == [n_free, len(reps), reps[0] if reps else -1, 0]
        assert (ref["rows"][s][len(reps):] == -1).all() and np.isnan(ref["best"][s, len(reps):]).all()
        assert (ref["mode_of"][lo:hi][mask != 0] == -1).all() and np.isnan(ref["sep"][lo:hi][mask != 0]).all()
        # slot 0 is the existing selection's row
        assert (reps[0] if reps else -1) == (lo + P.select_ref(mask, plen, smooth, w_s, w_l)[2] if n_free else -1)
        if not reps:
            assert n_free == 0 and not ref["mode_count"][s].any()
            continue
        assert np.array_equal(ref["best"][s, :len(reps)], c["traj"][reps], equal_nan=True)
        d = distances(c, np.asarray(order), reps, metric)                  # (reps, free rows in the order)
        pos = [order.index(r) for r in reps]
        # in the order, pairwise apart
        assert pos == sorted(pos) and len(set(reps)) == len(reps)
        for i in range(len(reps)):
            assert (d[:i, pos[i]] >= ms).all()
        # maximal: every free row that is not selected and precedes the point where selection stopped is within min_sep of (or has a NaN
        # distance to) a representative before it
        stop = pos[-1] if len(reps) == k else len(order)
        before = np.asarray(pos)[:, None] < np.arange(len(order))[None, :]
        with np.errstate(invalid="ignore"):
            suppressed = (before & ~(d >= ms)).any(0)
        unselected = np.ones(len(order), bool); unselected[pos] = False
        assert suppressed[:stop][unselected[:stop]].all(), s
        if ms == 0.0 and not np.isnan(d).any():
            assert reps == order[:k]
        # modes: the nearest representative, the lowest slot on a tie; a representative has its own slot
        mode, sep = ref["mode_of"][order], ref["sep"][order]
        lost = np.isnan(d).all(0) & unselected
        assert (mode[lost] == -1).all() and np.isnan(sep[lost]).all()
        rest = unselected & ~lost
        assert np.array_equal(mode[rest], np.nanargmin(d[:, rest], axis=0)) and np.allclose(sep[rest], np.nanmin(d[:, rest], axis=0), rtol=1e-14, atol=0)
        assert mode[pos].tolist() == list(range(len(reps)))
        assert np.array_equal(ref["mode_count"][s], np.bincount(mode[mode >= 0], minlength=k))
        if np.isfinite(d).all():
            assert int(ref["mode_count"][s].sum()) == n_free


@pytest.mark.parametrize("metric", ["mean", "max"])
@pytest.mark.parametrize("k", [1, 2, 16])
def test_reference_properties_on_the_small_batches(k, metric):
    for shape in ((2, 2, 2), (8, 4, 2), (64, 6, 3)):
        c = R.small_case(*shape)
        for ms in (R.MIN_SEP[metric], 0.0):
            check_properties(c, R.reference(R.small_case, shape, k, ms, metric), k, ms, metric)


def test_reference_properties_on_designed_inputs():
    c = R.planted_case()
    check_properties(c, R.reference(R.planted_case, (), 16, R.PLANTED_SEP, "mean"), 16, R.PLANTED_SEP, "mean")
    for name in P.SELECT_TIES:
        c = R.tie_case(name)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"], 2, 0.0, "mean", 2)
        check_properties(c, ref, 2, 0.0, "mean", c["w_s"], c["w_l"])
        assert ref["rows"][0].tolist() == list(c["rows"])                  # the lower row first
    c = R.all_tie_case()
    ref = R.reference(R.all_tie_case, (), 16, 0.0, "max")
    check_properties(c, ref, 16, 0.0, "max")
    assert ref["rows"][0].tolist() == np.nonzero(c["mask"] == 0)[0][:16].tolist() and ref["rows"][0][0] == 3
    c = R.threshold_case(7, 3)
    for ms, want in ((0.25, [1, 4, 2, 5, 3]), (float(np.nextafter(np.float32(0.25), np.float32(1))), [1, 2, 5, 3])):
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 16, ms, "mean", 3)
        check_properties(c, ref, 16, ms, "mean")
        assert ref["rows"][0][:len(want)].tolist() == want and ref["sep"][4] == (0.0 if len(want) == 5 else 0.25)
    # a free row with NaN positions: first in the order it is the only representative and nothing else has a mode; elsewhere it is suppressed
    base = R.small_case(8, 4, 2)
    first_row = int(R.reference(R.small_case, (8, 4, 2), 1, 0.0, "mean")["rows"][0, 0])
    for row in (first_row, first_row + 1 if first_row + 1 < 65 else first_row - 1):
        c = R.with_nan_row(base, row, free=True)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 4, 0.25, "mean", 2)
        check_properties(c, ref, 4, 0.25, "mean")
        if ref["rows"][0, 0] == row:
            assert ref["result"][0, 1] == 1 and ref["mode_count"][0].tolist() == [1, 0, 0, 0]
        else:
            assert row not in ref["rows"][0] and ref["mode_of"][row] == -1 and np.isnan(ref["sep"][row])


# ------------------------------------------------------------------------------------------------ the conditions of the GPU cases
def test_planted_bundles_are_tight_and_apart():
    c = R.planted_case()
    p = c["traj"][:, :, :2].astype(np.float64)
    for metric in ("mean", "max"):
        red = (lambda n: n.max(-1)) if metric == "max" else (lambda n: n.mean(-1))
        for m in range(R.PLANTED_M):
            rows = np.nonzero(c["bundle"] == m)[0]
            n = np.sqrt(((p[rows][:, None] - p[rows][None, :64]) ** 2).sum(-1))
            assert red(n).max() <= R.PLANTED_EPS < R.PLANTED_SEP
            other = np.nonzero(c["bundle"] != m)[0][:64]
            assert red(np.sqrt(((p[rows][:, None] - p[other][None]) ** 2).sum(-1))).min() >= 0.22 > R.PLANTED_SEP


@pytest.mark.parametrize("metric", ["mean", "max"])
def test_gpu_cases_keep_their_conditions(metric):
    """K = 16 walks the longest greedy path: the paths of K = 1 and 2 are its beginnings."""
    ms = R.MIN_SEP[metric]
    assert R.conditions_hold(R.ragged_case(), R.reference(R.ragged_case, (), 16, ms, metric), ms)
    for shape in R.SHAPES:
        assert R.conditions_hold(R.small_case(*shape), R.reference(R.small_case, shape, 16, ms, metric), ms), shape
    assert R.conditions_hold(R.planted_case(), R.reference(R.planted_case, (), 16, R.PLANTED_SEP, metric), R.PLANTED_SEP)
    for H, D in ((7, 3), (48, 2)):
        c = R.threshold_case(H, D)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 16, 0.25, metric, D)
        at_sep, between = R.distance_margins(c, ref, 0.25)
        assert at_sep == 0.0 and R.conditions_hold(c, ref, 0.25, designed_sep=True)     # it sits on min_sep, by design
        d = ref["dist"][0][:, 1:]
        assert ((d == 0.0) | (d == 0.25) | (d > 1.0)).all()                             # and every other distance is far from it
    for shape in R.SHAPES:                                                              # min_sep = 0: only the nearest slot can go wrong
        assert R.conditions_hold(R.small_case(*shape), R.reference(R.small_case, shape, 3, 0.0, metric), 0.0), shape
    base = R.small_case(48, 4, 2)
    hit, other, winner = R.nan_rows(metric)
    assert base["mask"][hit] != 0 and base["mask"][other] == 0 and base["mask"][winner] == 0 and len({hit, other, winner}) == 3
    for row, free in ((hit, False), (other, True), (winner, True)):
        c = R.with_nan_row(base, row, free)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 16, ms, metric, 2)
        assert R.conditions_hold(c, ref, ms), (row, free)


def test_designed_gpu_cases_keep_their_conditions():
    for name in P.SELECT_TIES:
        c = R.tie_case(name)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"], 2, 0.0, "mean", 2)
        assert R.conditions_hold(c, ref, 0.0, designed_totals=True), name
    for ms in (0.0, 0.25):
        assert R.conditions_hold(R.all_tie_case(), R.reference(R.all_tie_case, (), 16, ms, "max"), ms, designed_totals=True), ms
    old, new = R.small_case(48, 4, 2), R.replay_case()
    assert R.conditions_hold(old, R.reference(R.small_case, (48, 4, 2), R.REPLAY_K, R.REPLAY_SEP, "mean"), R.REPLAY_SEP)
    ref = R.reference(R.replay_case, (), R.REPLAY_K, R.REPLAY_SEP, "mean")
    assert R.conditions_hold(new, ref, R.REPLAY_SEP)
    assert not np.array_equal(ref["rows"], R.reference(R.small_case, (48, 4, 2), R.REPLAY_K, R.REPLAY_SEP, "mean")["rows"])
    c = R.ragged_case()                                        # the scenes run alone walk the paths they walk inside the batch
    assert R.conditions_hold(c, R.reference(R.ragged_case, (), 16, 0.25, "mean"), 0.25)
