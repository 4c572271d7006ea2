"""The single-episode replan (ramp_replan, ramp_replan_guided) against results recorded from the commit before it became the one-episode
job of the many-episode body: tests/golden/replan_single_parent.npz, written by ramp_amd/tools/record_replan_single.py, whose ``replay``
runs the same sequences here.  Every stored output -- best, batch, mask, the record with its fell_back word, the launch count and, where
guided, the tap -- must come back bit for bit: nothing in the arithmetic was meant to change, so there is no tolerance.

One exception, stated in include/ramp_hip.h at ramp_replan: without a collision-free candidate (n_free = 0) `best` used to be whatever the
buffer held and is now the plan the replan started from.  The fixture stores no `best` for the one call where the two differ (sequence e);
the new rule is checked there instead."""
import numpy as np
import pytest

from ramp_amd.tools import record_replan_single as R
from util import GOLDEN

pytestmark = pytest.mark.gpu

_FIX = {}


def fixture():
    if not _FIX:
        g = np.load(f"{GOLDEN}/replan_single_parent.npz")
        _FIX["in"] = {k[3:]: g[k] for k in g.files if k.startswith("in/")}
        _FIX["out"] = {k[4:]: g[k] for k in g.files if k.startswith("out/")}
    return _FIX["in"], _FIX["out"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_the_fixture_leaves_no_case_out():
    """Every sequence of the recorder is stored, with every output of every call (`best` is absent from sequence e only); the sequences
    cover a calibrating, a carried and a previous-winner call with both values of `near`, and a call without a free candidate."""
    inp, out = fixture()
    calls = {"a_graph": 3, "a_eager": 3, "b": 1, "c_none": 1, "c_two": 1, "d_guided": 1, "d_zero": 1, "e": 1, "f_graph": 3, "f_eager": 3, "g": 2}
    assert set(calls) == set(R.SEQUENCES)
    want = set()
    for name, n in calls.items():
        for k in range(n):
            want |= {f"{name}/{k}/{key}" for key in ("best", "batch", "mask", "record", "launches")}
    want.remove("e/0/best")
    want.add("d_guided/0/tap")
    assert set(out) == want
    assert [c[2] for c in R.CALLS] == [0, 1, 0]
    assert out["e/0/record"][0] == 0 and out["e/0/mask"].all()
    assert out["a_graph/0/record"][0] > 0
    assert np.isfinite(out["d_guided/0/tap"]).all() and float(np.abs(out["d_guided/0/tap"][1] - out["d_guided/0/tap"][0]).max()) > 1e-3


@pytest.mark.parametrize("name", R.SEQUENCES)
def test_single_replan_is_the_recorded_one_bit_for_bit(name):
    inp, out = fixture()
    got = R.replay(inp, [name])
    stored = {k: v for k, v in out.items() if k.startswith(name + "/")}
    assert set(got) - {"e/0/best"} == set(stored)
    for key in sorted(stored):
        call = key.rsplit("/", 1)[0]
        assert got[key].dtype == stored[key].dtype and got[key].shape == stored[key].shape, key
        assert np.array_equal(bits(got[key]), bits(stored[key])), (key, got[call + "/record"].tolist(), stored[call + "/record"].tolist())


def test_without_a_free_candidate_best_is_the_plan_the_replan_started_from():
    """The rule stated at ramp_replan in include/ramp_hip.h (the many-episode entry's): sequence e, where every candidate collides, hands
    back x_clean as given.  (Before, `best` held whatever the buffer held, which is why the fixture stores none for this call.  Calls 1 of
    sequences a and f also find no free candidate, but start from the previous winner, which is what the buffer held before as well:
    their `best` is stored and compared above.)"""
    inp, out = fixture()
    got = R.replay(inp, ["e"])
    assert got["e/0/record"].tolist() == [0, -1, -1, 0]
    assert np.array_equal(bits(got["e/0/best"]), bits(inp["x_clean"]))
    for name in ("a_graph", "a_eager", "f_graph", "f_eager"):
        assert out[f"{name}/1/record"][0] == 0 and np.array_equal(bits(out[f"{name}/1/best"]), bits(out[f"{name}/0/best"]))


def test_a_single_call_after_an_episode_call_calibrates():
    """Sequence g's third call (a single call behind a one-episode ramp_replan_episodes call on the same context, same inputs as its
    first) equals the first, calibrating call: the carried operand maxima of the other entry are not reused."""
    _, out = fixture()
    for key in ("best", "batch", "mask", "record", "launches"):
        assert np.array_equal(bits(out[f"g/1/{key}"]), bits(out[f"g/0/{key}"])), key
