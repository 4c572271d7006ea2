"""ramp_select_diverse_scenes and the Python layers over it on the device, against the float64 numpy statement ``cost.diverse_reference``
on the cases of tests/diverse_ref.py (whose input conditions tests/test_diverse_host.py proves on the CPU; each test here asserts the ones
it needs again before it compares): integers equal, ``best_out`` bit for bit, ``sep_out`` within diverse_ref.SEP_BAR."""
import functools
import json

import numpy as np
import pytest
import torch

import diverse_ref as R
import planner_ref as P
from ramp_amd import _lib, cost
from test_diverse_host import check_every_refusal
from util import dev

pytestmark = pytest.mark.gpu
CODE = {"mean": 0, "max": 1}


class Call:
    """The buffers of one raw call, filled with sentinels; ``launch`` enqueues it on the current stream."""

    def __init__(self, c, k):
        self.c, self.k = c, k
        self.B, self.n = c["traj"].shape[0], len(c["first"]) - 1
        self.t, self.first, self.mask = dev(c["traj"]), dev(c["first"]), dev(c["mask"])
        self.plen, self.smooth = dev(c["plen"]), dev(c["smooth"])
        H, S = c["H"], c["S"]
        self.best = torch.full((self.n, k, H, S), -7.0, device="cuda")
        self.rows = torch.full((self.n, k), -7, dtype=torch.int32, device="cuda")
        self.res = torch.full((self.n, 4), -7, dtype=torch.int32, device="cuda")
        self.mode = torch.full((max(self.B, 1),), -7, dtype=torch.int32, device="cuda")
        self.sep = torch.full((max(self.B, 1),), -7.0, device="cuda")
        self.count = torch.full((self.n, k), -7, dtype=torch.int32, device="cuda")
        self.scratch = torch.full((2 * self.B + self.n,), -7, dtype=torch.int32, device="cuda")

    def launch(self, min_sep, metric, w_s=R.W_S, w_l=R.W_L):
        c = self.c
        _lib.check(_lib.load().ramp_select_diverse_scenes(
            self.t.data_ptr(), self.B, c["H"], c["S"], c["D"], self.first.data_ptr(), self.n, self.mask.data_ptr(), self.plen.data_ptr(),
            self.smooth.data_ptr(), w_s, w_l, self.k, min_sep, CODE[metric], self.best.data_ptr(), self.rows.data_ptr(), self.res.data_ptr(),
            self.mode.data_ptr(), self.sep.data_ptr(), self.count.data_ptr(), self.scratch.data_ptr(), _lib.current_stream()),
            "ramp_select_diverse_scenes")

    def outputs(self):
        torch.cuda.synchronize()
        return dict(best=self.best.cpu().numpy(), rows=self.rows.cpu().numpy(), result=self.res.cpu().numpy(),
                    mode_of=self.mode.cpu().numpy()[:self.B], sep=self.sep.cpu().numpy()[:self.B], mode_count=self.count.cpu().numpy())


def run(c, k, min_sep, metric, w_s=R.W_S, w_l=R.W_L):
    call = Call(c, k)
    call.launch(min_sep, metric, w_s, w_l)
    return call.outputs()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def compare(c, got, ref, what=""):
    """Integers equal, best_out the gathered rows bit for bit with NaN in the unfilled slots, sep_out within SEP_BAR of float64."""
    for name in ("rows", "result", "mode_of", "mode_count"):
        assert np.array_equal(got[name], ref[name]), (what, name, np.nonzero(got[name] != ref[name]))
    filled = ref["rows"] >= 0
    assert same_bits(got["best"][filled], c["traj"][ref["rows"][filled]]), what
    assert np.isnan(got["best"][~filled]).all(), what
    nan = np.isnan(ref["sep"])
    assert np.array_equal(np.isnan(got["sep"]), nan), what
    err = np.abs(got["sep"][~nan].astype(np.float64) - ref["sep"][~nan])
    worst = float((err / np.maximum(ref["sep"][~nan], 1e-300))[ref["sep"][~nan] > 0].max(initial=0.0))
    print(f"{what}: sep_out relative error {worst / 2.0 ** -24:.2f} x 2^-24 (bar 8)")
    assert (err <= R.SEP_BAR * ref["sep"][~nan]).all(), (what, worst)


# ------------------------------------------------------------------------------------------------ against the float64 statement
@pytest.mark.parametrize("metric", ["mean", "max"])
@pytest.mark.parametrize("k", [1, 2, 16])
def test_ragged_batch_against_float64(k, metric):
    """Scenes of 1, 2, 63, 64, 65, 1023, 1024, 1025 and 3000 rows, an empty one, one without a free row, one with a single free row and
    one with fewer than K separable rows, in one call."""
    c, ms = R.ragged_case(), R.MIN_SEP[metric]
    assert R.conditions_hold(c, R.reference(R.ragged_case, (), 16, ms, metric), ms)
    ref = R.reference(R.ragged_case, (), k, ms, metric)
    sizes = np.diff(c["first"]).tolist()
    assert sizes[:9] == list(R.SIZES) and sizes[9] == 0 and ref["result"][10].tolist() == [0, 0, -1, 0] and ref["result"][11, 0] == 1
    assert k < 16 or (ref["result"][:, 1] < 16).all()                          # nobody has 16 separable rows
    compare(c, run(c, k, ms, metric), ref, f"ragged k={k} {metric}")


@pytest.mark.parametrize("metric", ["mean", "max"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "h%d_s%d_d%d" % s)
def test_every_shape_against_float64(shape, metric):
    c, ms = R.small_case(*shape), R.MIN_SEP[metric]
    for k in (16, 2):
        ref = R.reference(R.small_case, shape, k, ms, metric)
        assert R.conditions_hold(c, R.reference(R.small_case, shape, 16, ms, metric), ms)
        compare(c, run(c, k, ms, metric), ref, f"{shape} k={k} {metric}")
    ref = R.reference(R.small_case, shape, 3, 0.0, metric)                      # min_sep = 0: the first rows of the order
    assert R.conditions_hold(c, ref, 0.0)
    compare(c, run(c, 3, 0.0, metric), ref, f"{shape} min_sep=0 {metric}")


# ------------------------------------------------------------------------------------------------ designed cases
@pytest.mark.parametrize("metric", ["mean", "max"])
def test_planted_modes_are_found_one_representative_each(metric):
    c = R.planted_case()
    ref = R.reference(R.planted_case, (), 16, R.PLANTED_SEP, metric)
    assert R.conditions_hold(c, ref, R.PLANTED_SEP)
    got = run(c, 16, R.PLANTED_SEP, metric)
    compare(c, got, ref, f"planted {metric}")
    reps = got["rows"][0][got["rows"][0] >= 0]
    free = c["mask"] == 0
    assert len(reps) == R.PLANTED_M and sorted(c["bundle"][reps]) == list(range(R.PLANTED_M))
    tot = P.select_totals(c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L)
    rank = {int(r): i for i, r in enumerate(np.nonzero(free)[0])}
    assert [tot[rank[int(r)]] for r in reps] == sorted(tot[rank[int(r)]] for r in reps)             # in cost order
    slot_of_bundle = {int(c["bundle"][r]): j for j, r in enumerate(reps)}
    assert np.array_equal(got["mode_of"][free], [slot_of_bundle[int(m)] for m in c["bundle"][free]])
    assert got["mode_count"][0, :R.PLANTED_M].tolist() == [int((free & (c["bundle"] == c["bundle"][r])).sum()) for r in reps]
    assert (got["sep"][free] <= R.PLANTED_EPS).all() and (got["mode_count"][0, R.PLANTED_M:] == 0).all()


@pytest.mark.parametrize("name", list(P.SELECT_TIES))
def test_equal_totals_take_the_lower_row_first(name):
    c = R.tie_case(name)
    got = run(c, 2, 0.0, "mean", c["w_s"], c["w_l"])
    ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], c["w_s"], c["w_l"], 2, 0.0, "mean", 2)
    assert R.conditions_hold(c, ref, 0.0, designed_totals=True)
    assert got["rows"][0].tolist() == list(c["rows"]) and c["rows"][0] < c["rows"][1]
    compare(c, got, ref, f"tie {name}")


@pytest.mark.parametrize("min_sep", [0.0, 0.25])
def test_an_all_tie_scene_is_selected_in_row_order(min_sep):
    c = R.all_tie_case()
    assert np.isnan(P.select_totals(c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L)).all()
    ref = R.reference(R.all_tie_case, (), 16, min_sep, "max")
    assert R.conditions_hold(c, ref, min_sep, designed_totals=True)
    got = run(c, 16, min_sep, "max")
    compare(c, got, ref, f"all-tie {min_sep}")
    reps = got["rows"][0][got["rows"][0] >= 0]
    assert reps[0] == 3 and (np.diff(reps) > 0).all()
    if min_sep == 0.0:
        assert reps.tolist() == np.nonzero(c["mask"] == 0)[0][:16].tolist()


@pytest.mark.parametrize("metric", ["mean", "max"])
@pytest.mark.parametrize("H,D", [(7, 3), (48, 2)])
def test_a_row_exactly_min_sep_away_is_kept_and_one_ulp_closer_is_not(H, D, metric):
    c = R.threshold_case(H, D)
    above = float(np.nextafter(np.float32(0.25), np.float32(1)))
    for ms, want in ((0.25, [1, 4, 2, 5, 3]), (above, [1, 2, 5, 3])):
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 16, ms, metric, D)
        assert R.conditions_hold(c, ref, ms, designed_sep=True) and ref["dist"][0][0, 4] == 0.25
        got = run(c, 16, ms, metric)
        compare(c, got, ref, f"threshold {ms!r} {metric}")
        assert got["rows"][0][:len(want)].tolist() == want and got["result"][0, 1] == len(want)
    assert got["mode_of"][4] == 0 and got["sep"][4] == 0.25


# ------------------------------------------------------------------------------------------------ the existing selection
def test_slot_0_is_the_existing_selection():
    """Column 0 of rows_out / best_out equals ramp_select_scored_scenes on the same arrays, exactly, and the n_free agree."""
    for c in (R.ragged_case(), R.small_case(64, 6, 3), R.all_tie_case()):
        call = Call(c, 4)
        call.launch(0.25, "mean")
        best = torch.full((call.n, c["H"], c["S"]), -7.0, device="cuda")
        res = torch.full((call.n, 4), -7, dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().ramp_select_scored_scenes(
            call.t.data_ptr(), call.B, c["H"], c["S"], call.first.data_ptr(), call.n, call.mask.data_ptr(), call.plen.data_ptr(),
            call.smooth.data_ptr(), R.W_S, R.W_L, best.data_ptr(), res.data_ptr(), _lib.current_stream()), "ramp_select_scored_scenes")
        got = call.outputs()
        res, best = res.cpu().numpy(), best.cpu().numpy()
        assert np.array_equal(got["rows"][:, 0], res[:, 2]) and np.array_equal(got["result"][:, 0], res[:, 0])
        assert np.array_equal(got["result"][:, 2], res[:, 2]) and same_bits(got["best"][:, 0], best)


def test_python_layers_agree_with_the_single_selection():
    """select_diverse_clear_scenes(k=1) is select_best_clear_scenes; with k = 4 its column 0 still is, and select_diverse_scored_scenes on
    the clearance's own arrays gives the same result."""
    from ramp_amd.clearance import trajectory_clearance
    c = R.small_case(64, 6, 3)
    counts = [n for n in np.diff(c["first"]).tolist() if n]
    t = dev(c["traj"])
    spheres = [(torch.tensor([[0.0, 0.3 * (-1) ** i, 0.0]]), torch.tensor([0.2])) for i in range(len(counts))]
    kw = dict(spheres=spheres, point_dim=3, swept=True)
    best, n_free, _, row, free = cost.select_best_clear_scenes(t, counts, **kw)
    one = cost.select_diverse_clear_scenes(t, counts, k=1, min_sep=0.25, **kw)
    four = cost.select_diverse_clear_scenes(t, counts, k=4, min_sep=0.25, metric="max", **kw)
    assert 0 < int(free.sum()) < t.shape[0]
    for sel in (one, four):
        assert torch.equal(sel.rows[:, 0], row) and torch.equal(sel.n_free, n_free) and torch.equal(sel.collision_free_mask, free)
        assert same_bits(sel.best[:, 0].cpu().numpy(), best.cpu().numpy())
        assert torch.equal(sel.n_selected, (sel.rows >= 0).sum(1).to(torch.int32))
        assert bool((sel.mode_of[~free] == -1).all()) and torch.equal(sel.mode_count.sum(1).to(torch.int32), n_free)
    assert one.best.shape == (len(counts), 1, 64, 6) and four.rows.shape == (len(counts), 4) and int(four.n_selected.max()) > 1
    r = trajectory_clearance(t, None, spheres, None, counts, point_dim=3)
    again = cost.select_diverse_scored_scenes(t, r.traj_first, r.colliding(0.0, 0.0, True), r.path_length, r.smoothness, k=4, min_sep=0.25,
                                              metric="max", point_dim=3)
    for a, b in zip(again, four):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------ independence, NaN rows, capture
@functools.lru_cache(maxsize=None)
def whole_ragged():
    return run(R.ragged_case(), 16, 0.25, "mean")


@pytest.mark.parametrize("scene", [2, 7, 8, 12], ids=["63_rows", "1025_rows", "3000_rows", "tight"])
def test_a_scene_alone_and_inside_the_batch_give_the_same_bits(scene):
    c = R.ragged_case()
    assert R.conditions_hold(c, R.reference(R.ragged_case, (), 16, 0.25, "mean"), 0.25)
    whole = whole_ragged()
    alone_c, lo, hi = R.scene_slice(c, scene)
    alone = run(alone_c, 16, 0.25, "mean")
    rows = alone["rows"][0]
    assert np.array_equal(np.where(rows >= 0, rows + lo, -1), whole["rows"][scene])
    assert alone["result"][0, :2].tolist() == whole["result"][scene, :2].tolist()
    assert np.array_equal(alone["mode_of"], whole["mode_of"][lo:hi]) and np.array_equal(alone["mode_count"][0], whole["mode_count"][scene])
    assert same_bits(alone["best"][0], whole["best"][scene]) and same_bits(alone["sep"], whole["sep"][lo:hi])


@pytest.mark.parametrize("metric", ["mean", "max"])
def test_rows_with_nan_positions(metric):
    """A colliding row with NaN positions disturbs nothing; a free one is suppressed and has no mode, or, first in the order, is the only
    representative of its scene and nothing else there has a mode."""
    base, ms = R.small_case(48, 4, 2), R.MIN_SEP[metric]
    plain = run(base, 16, ms, metric)
    masked_row, other, winner = R.nan_rows(metric)
    assert winner == plain["rows"][0, 0]
    c = R.with_nan_row(base, masked_row, free=False)
    got = run(c, 16, ms, metric)
    for name in plain:
        assert same_bits(got[name], plain[name]), name
    for row in (other, winner):
        c = R.with_nan_row(base, row, free=True)
        ref = cost.diverse_reference(c["traj"], c["first"], c["mask"], c["plen"], c["smooth"], R.W_S, R.W_L, 16, ms, metric, 2)
        assert R.conditions_hold(c, ref, ms)
        got = run(c, 16, ms, metric)
        compare(c, got, ref, f"NaN row {row} {metric}")
        if row == winner:
            assert got["rows"][0].tolist() == [winner] + [-1] * 15 and got["mode_count"][0].tolist() == [1] + [0] * 15
            assert (np.delete(got["mode_of"][:65], winner) == -1).all() and np.isnan(got["sep"][winner])
        else:
            assert row not in got["rows"][0] and got["mode_of"][row] == -1 and np.isnan(got["sep"][row])
    assert np.array_equal(got["rows"][2], plain["rows"][2])                    # the other scenes are as they were


def test_captured_once_and_replayed_on_new_trajectories():
    """One capture in a single-stream graph; the replay after the trajectories, mask and costs in the same buffers were replaced matches the
    reference of the new contents."""
    a, new, ms = R.small_case(48, 4, 2), R.replay_case(), R.REPLAY_SEP
    ref_old, ref_new = R.reference(R.small_case, (48, 4, 2), R.REPLAY_K, ms, "mean"), R.reference(R.replay_case, (), R.REPLAY_K, ms, "mean")
    assert R.conditions_hold(new, ref_new, ms) and R.conditions_hold(a, ref_old, ms) and not np.array_equal(ref_new["rows"], ref_old["rows"])
    call = Call(a, R.REPLAY_K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.launch(ms, "mean")                                                 # (code objects loaded before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call.launch(ms, "mean")
    graph.replay()
    compare(a, call.outputs(), ref_old, "captured")
    call.t.copy_(dev(new["traj"])); call.mask.copy_(dev(new["mask"])); call.plen.copy_(dev(new["plen"])); call.smooth.copy_(dev(new["smooth"]))
    graph.replay()
    compare(new, call.outputs(), ref_new, "replayed")


def test_refusals_launch_nothing():
    c = R.small_case(8, 4, 2)
    call = Call(c, 4)
    real = dict(traj=call.t.data_ptr(), traj_first=call.first.data_ptr(), mask=call.mask.data_ptr(), path_len=call.plen.data_ptr(),
                smooth=call.smooth.data_ptr(), best_out=call.best.data_ptr(), rows_out=call.rows.data_ptr(), result_dev=call.res.data_ptr(),
                mode_of=call.mode.data_ptr(), sep_out=call.sep.data_ptr(), mode_count=call.count.data_ptr(), scratch=call.scratch.data_ptr(),
                stream=_lib.current_stream())
    check_every_refusal(_lib.load(), **real)
    torch.cuda.synchronize()
    for x in (call.best, call.rows, call.res, call.mode, call.sep, call.count, call.scratch):
        assert bool((x == -7).all())
    with pytest.raises(_lib.RampHipError, match="horizon"):
        cost.select_diverse_scored_scenes(torch.zeros(2, 129, 4, device="cuda"), [0, 2], torch.zeros(2), torch.ones(2), torch.ones(2), k=2,
                                          min_sep=0.1)


# ------------------------------------------------------------------------------------------------ the examples
def test_static_example_stores_the_alternatives_next_to_the_best(tmp_path, capsys):
    import examples.inference_static as ex
    common = ["--make-synthetic", str(tmp_path), "--all-envs", "--n-samples", "6", "--sampler", "ddpm", "--n-diffusion-steps", "25",
              "--n-steps-without-noise", "0"]
    plain, _ = ex.main(common)
    keys_plain = [json.loads(l).keys() for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    with_alt, runner = ex.main(common + ["--alternatives", "3", "--min-sep", "0.0"])
    keys_alt = [json.loads(l).keys() for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    new = {"alternative_trajectories", "alternative_rows", "mode_count", "n_alternatives"}
    assert len(plain) == len(with_alt) == 1 and not new & set(plain[0]) and set(with_alt[0]) == set(plain[0]) | new
    assert [set(k) for k in keys_alt] == [set(k) | {"n_alternatives"} for k in keys_plain]
    m = with_alt[0]
    assert m["alternative_trajectories"].shape == (3, 48, 4) and m["n_alternatives"] == 3 and int(m["mode_count"].sum()) == 6
    assert torch.equal(m["alternative_trajectories"][0], m["best_trajectory"])
    assert torch.equal(m["alternative_trajectories"], runner.last_trajectories[m["alternative_rows"].long()])


def test_3d_example_reports_the_alternatives(tmp_path, capsys):
    import examples.inference3d as ex
    common = ["--make-synthetic", str(tmp_path), "--n-samples", "6", "--n-diffusion-steps", "5", "--evaluate"]
    plain, _ = ex.main(common)
    out, _ = ex.main(common + ["--alternatives", "4", "--min-sep", "0.05"])
    capsys.readouterr()
    ev = out["evaluation"]
    assert set(ev) == set(plain["evaluation"]) | {"alternative_rows", "mode_count"}
    assert len(ev["alternative_rows"]) == len(ev["mode_count"]) == 4 and ev["alternative_rows"][0] == ev["best_row"]
    assert sum(ev["mode_count"]) == ev["n_free_selected"] and all((r >= 0) == (c > 0) for r, c in zip(ev["alternative_rows"], ev["mode_count"]))
    with pytest.raises(SystemExit):
        ex.main(["--make-synthetic", str(tmp_path), "--alternatives", "2"])
