"""The nine sampling entries (ramp_sample .. ramp_sample_stitched) against results recorded from the commit before they were put behind one
job descriptor: tests/golden/sample_jobs_parent.npz, written by ramp_amd/tools/record_sample_jobs.py, whose ``replay`` runs the same walks
here.  Every stored output -- x, the chain, the accept flags, ancestors / ESS / costs / log-weights, the assembled long trajectories and the
launch count -- must come back bit for bit: nothing in the arithmetic was meant to change, so there is no tolerance.

A walk runs its jobs on ONE context, every job twice in a row (the capture, then the replay of its graph), neighbours differing in one
field of the graph key: a field lost from the key replays the previous job's graph, a staging copy lost or misplaced leaves the previous
job's table in the buffer, and either shows as different bits."""
import numpy as np
import pytest

from ramp_amd.tools import record_sample_jobs as R
from util import GOLDEN

_FIX = {}


def fixture():
    if not _FIX:
        g = np.load(f"{GOLDEN}/sample_jobs_parent.npz")
        _FIX["in"] = {k[3:]: g[k] for k in g.files if k.startswith("in/")}
        _FIX["out"] = {k[4:]: g[k] for k in g.files if k.startswith("out/")}
    return _FIX["in"], _FIX["out"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def wanted_keys():
    want = set()
    for wname, (jobs, _, _) in R.WALKS.items():
        for i, name in enumerate(jobs):
            kind, opt = R.JOBS[name]
            keys = ["x", "chain", "launches"] + (["accept"] if "mcmc" in opt else []) + (["long"] if kind == "stitched" else [])
            keys += ["ancestors", "ess", "cost", "logw"] if opt.get("resample") else []
            want |= {f"{wname}/{i:02d}_{name}/{run}/{key}" for run in range(2) for key in keys}
    return want


def test_the_fixture_leaves_no_case_out():
    """Every job of every walk is stored, both runs, with every output the job has; the graph walk is the nineteen jobs in their order and
    ends on its first job; the second walk runs the same jobs without graphs, the third a subset on the bf16x6 kernels.  The stored jobs did
    something: the options moved the result, every event resampled, inner steps were accepted and refused."""
    _, out = fixture()
    assert set(out) == wanted_keys()
    assert R.WALK == ("ddpm", "ddim", "scenes_apf", "composed", "ula", "composed_mala", "guided", "guided_w_obs", "prims", "prims_margin", "team",
                      "team_radius", "steered", "stitched", "stitched_pin", "philox", "philox_mala", "philox_steered", "ddpm")
    assert R.WALKS["graph"] == (R.WALK, 1, "default") and R.WALKS["eager"] == (R.WALK, 0, "default")
    assert R.WALKS["bf16x6"] == (("ddpm", "guided", "steered", "stitched"), 1, "bf16x6")
    x = lambda job: out[f"graph/{R.WALK.index(job):02d}_{job}/1/x"]      # noqa: E731
    for a, b in (("ddpm", "ddim"), ("ddpm", "ula"), ("ddpm", "guided"), ("guided", "guided_w_obs"), ("guided", "prims"), ("prims", "prims_margin"),
                 ("guided", "team"), ("team", "team_radius"), ("composed", "composed_mala"), ("stitched", "stitched_pin"), ("philox", "philox_mala"),
                 ("philox", "philox_steered")):
        assert np.isfinite(x(a)).all() and np.isfinite(x(b)).all() and not np.array_equal(x(a), x(b)), (a, b)
    for job in ("steered", "philox_steered"):
        anc = out[f"graph/{R.WALK.index(job):02d}_{job}/1/ancestors"]
        assert anc.shape == (2, R.B) and (anc != np.arange(R.B)[None]).any()
    acc = out[f"graph/{R.WALK.index('composed_mala'):02d}_composed_mala/1/accept"]
    assert acc.shape == (3, R.B) and set(np.unique(acc)) <= {0, 1}
    long = out[f"graph/{R.WALK.index('stitched'):02d}_stitched/1/long"]
    assert long.shape == (R.CHAINS, 20, R.S) and np.isfinite(long).all()


@pytest.mark.parametrize("walk", ["graph", "eager"])
def test_a_job_does_not_depend_on_what_ran_before_it(walk):
    """The canonical calibration's promise, in the fixture: the last job of the walk is its first again, seventeen other jobs later, and
    gives the same bits, launch for launch."""
    _, out = fixture()
    last = len(R.WALK) - 1
    for run in range(2):
        for key in ("x", "chain", "launches"):
            assert np.array_equal(bits(out[f"{walk}/{last:02d}_ddpm/{run}/{key}"]), bits(out[f"{walk}/00_ddpm/{run}/{key}"])), (run, key)


@pytest.mark.gpu
@pytest.mark.parametrize("walk", list(R.WALKS))
def test_every_job_of_the_walk_is_the_recorded_one_bit_for_bit(walk):
    inp, out = fixture()
    got = R.replay(inp, [walk])
    stored = {k: v for k, v in out.items() if k.startswith(walk + "/")}
    assert set(got) == set(stored)
    for key in sorted(stored):
        assert got[key].dtype == stored[key].dtype and got[key].shape == stored[key].shape, key
        assert np.array_equal(bits(got[key]), bits(stored[key])), key
