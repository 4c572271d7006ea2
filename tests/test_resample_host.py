"""Host side of the resampling events (``resample=`` -> ``ramp_sample_steered``): struct layout, the declared / bound / exported symbols,
``resample_tables``, the refusals that need no device, ``lineage``, the restatement's own property (systematic resampling gives every
trajectory floor(n W) or ceil(n W) children) and the conditions the GPU tests ask of their inputs.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import test_gpu_resample as R
from ramp_amd import _lib
from ramp_amd.diffusion import _HostArrays, resample_tables
from ramp_amd.resample import group_table, lineage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S = 48, 4


def make(T, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    kw.setdefault("predict_epsilon", True)
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=H, state_dim=S), n_diffusion_steps=T, **kw)


# ------------------------------------------------------------------------------------------------ the C side
def test_resample_params_layout_matches_the_header():
    cls = _lib.RampResampleParams
    names = [f if f != "lambda_" else "lambda" for f, _ in cls._fields_]
    body = 'printf("%zu", sizeof(ramp_resample_params));' + "".join(f'printf(" %zu", offsetof(ramp_resample_params, {f}));' for f in names)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf(" %d\\n", RAMP_RESAMPLE_MAX_EVENTS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got[:-1] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert got[-1] == _lib.RESAMPLE_MAX_EVENTS == 64
    assert C.sizeof(cls) == 56


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_steered", 19), ("ramp_resample_groups", 13)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_steered"][1][2] == C.POINTER(_lib.RampResampleParams)
    assert _lib.PROTOTYPES["ramp_sample_steered"][1][3] == C.POINTER(_lib.RampCostGuide)
    from ramp_amd import build
    assert "resample.hip" in build.SOURCES and build.EXTRA_FLAGS["resample.hip"] == ["-ffp-contract=off"]
    assert os.path.exists(os.path.join(ROOT, "ramp_amd", "csrc", "args_resample.h"))


def test_host_refusals_of_the_entries():
    """ramp_resample_groups refuses on the host before any device call (the pointers are never dereferenced), and the job entry needs its
    context and parameters."""
    lib = _lib.load()

    def groups(gf, n_groups, ess, B=6, Hh=8, Ss=4, x=0x1000, lw=0x1000, u=0x1000):
        g = None if gf is None else np.asarray(gf, np.int32).ctypes.data_as(_lib.c_i32p)
        rc = lib.ramp_resample_groups(x, B, Hh, Ss, lw, None, g, n_groups, u, ess, None, None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_resample_groups" in msg, (rc, msg)
        return msg

    for gf, n in (([1, 6], 1), ([0, 5], 1), ([0, 7], 1), ([0, 3, 3, 6], 3), ([0, 4, 2, 6], 3), (None, 1), ([0, 6], 0)):
        assert "group table" in groups(gf, n, 0.5), gf
    for bad in (-0.1, 2.0000001, float("nan"), float("inf")):
        assert "ess_frac" in groups([0, 6], 1, bad)
    assert "multiple of 4" in groups([0, 6], 1, 0.5, Hh=3, Ss=2)
    assert "null" in groups([0, 6], 1, 0.5, x=None) and "null" in groups([0, 6], 1, 0.5, lw=None) and "null" in groups([0, 6], 1, 0.5, u=None)
    assert lib.ramp_sample_steered(*([None] * 19)) != 0
    assert "ramp_sample_steered" in lib.ramp_last_error().decode()


# ------------------------------------------------------------------------------------------------ resample_tables
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_tables(sampler):
    T = 25 if sampler == "ddpm" else 100
    dm = make(T, sampler=sampler)
    steps = dm._ddpm_steps()[0] if sampler == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    n = len(steps)
    base = dict(cloud=None, radius=0.3, lambda_=2.0)
    tab = resample_tables(dict(base, every=2), steps)
    assert tab["resample"] == [1 if (j + 1) % 2 == 0 else 0 for j in range(n)] and tab["events"] == list(range(1, n, 2))
    assert tab["lambda"] == [2.0] * n and tab["ess_frac"] == 0.5
    assert (tab["radius"], tab["w_obs"], tab["w_smooth"], tab["w_acc"]) == (0.3, 1.0, 0.0, 0.0)
    assert resample_tables(dict(base, every=1), steps)["resample"] == [1] * n
    # t_start: t == t_start is off, t_start - 1 is on
    ts = steps[2]
    assert resample_tables(dict(base, every=1, t_start=ts), steps)["resample"] == [1 if t < ts else 0 for t in steps]
    assert resample_tables(dict(base, every=1, t_start=0), steps)["events"] == []
    # explicit flags and per-step lambda
    flags, lam = [j % 2 for j in range(n)], [0.5 * j for j in range(n)]
    tab = resample_tables(dict(base, flags=[3 * f for f in flags], lambda_=lam, ess_frac=2.0, w_obs=0.0, w_smooth=1.0, w_acc=0.25, radius=0.0), steps)
    assert tab["resample"] == flags and tab["lambda"] == lam and tab["ess_frac"] == 2.0 and tab["w_obs"] == 0.0
    # through the model, on the CPU: one group for a plain job, one per scene otherwise
    arrays = _HostArrays()
    hc = {0: torch.zeros(S), H - 1: torch.ones(7, S)}
    rs, cost, gf = dm._fill_resample(arrays, tab, dict(cloud=torch.zeros(9, 2)), None, hc, 7)
    assert (rs.n_groups, rs.group0, rs.groups_total, rs.ess_frac) == (1, 0, 0, 2.0) and gf.tolist() == [0, 7]
    assert [rs.resample[j] for j in range(n)] == flags and [rs.lambda_[j] for j in range(n)] == lam
    assert (rs.cost.contents.point_dim, rs.cost.contents.n_scenes, rs.cost.contents.w_smooth) == (2, 1, 1.0)
    job = dict(n_scenes=3, traj_scene=torch.tensor([0, 0, 1, 2, 2, 2, 2], dtype=torch.int32))
    rs, cost, gf = dm._fill_resample(arrays, tab, dict(clouds=[torch.zeros(2, 3), torch.zeros(0, 3), torch.zeros(4, 3)]), job, {}, 7)
    assert rs.n_groups == 3 and gf.tolist() == [0, 2, 3, 7] and [rs.group_first_host[i] for i in range(4)] == [0, 2, 3, 7]
    assert rs.cost.contents.point_dim == 3 and [rs.cost.contents.cloud_offset_host[i] for i in range(4)] == [0, 2, 2, 6]


@pytest.mark.parametrize("r, exc, msg", [
    ("every", TypeError, "takes a dict"),
    (dict(cloud=None, radius=0.3, lambda_=1.0, every=1, lam=1), ValueError, "unknown keys"),
    (dict(radius=0.3, lambda_=1.0, every=1), ValueError, "exactly one of cloud= and clouds="),
    (dict(cloud=None, clouds=[], radius=0.3, lambda_=1.0, every=1), ValueError, "exactly one of cloud= and clouds="),
    (dict(cloud=None, radius=0.3, lambda_=1.0), ValueError, "exactly one of every= and flags="),
    (dict(cloud=None, radius=0.3, lambda_=1.0, every=1, flags=[1] * 25), ValueError, "exactly one of every= and flags="),
    (dict(cloud=None, radius=0.3, lambda_=1.0, every=0), ValueError, "at least 1"),
    (dict(cloud=None, radius=0.3, lambda_=1.0, flags=[1, 0]), ValueError, "2 entries for 25"),
    (dict(cloud=None, radius=0.3, every=1), ValueError, "lambda_= is required"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=float("nan")), ValueError, "lambda_ must be finite"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=[1.0] * 24 + [float("inf")]), ValueError, "lambda_ must be finite"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=[1.0, 2.0]), ValueError, "2 entries for 25"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=1.0, ess_frac=2.5), ValueError, "ess_frac"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=1.0, ess_frac=-0.1), ValueError, "ess_frac"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=1.0, ess_frac=float("nan")), ValueError, "ess_frac"),
    (dict(cloud=None, every=1, lambda_=1.0), ValueError, "radius must be positive"),
    (dict(cloud=None, radius=float("nan"), every=1, lambda_=1.0), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, w_acc=float("inf"), every=1, lambda_=1.0), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, every=1, lambda_=1.0, t_start=float("nan")), ValueError, "t_start"),
])
def test_bad_tables_are_refused_with_a_message(r, exc, msg):
    dm = make(25, sampler="ddpm")
    with pytest.raises(exc, match=msg):
        resample_tables(r, dm._ddpm_steps()[0])


def test_more_than_64_events_are_refused():
    with pytest.raises(ValueError, match="at most 64"):
        resample_tables(dict(cloud=None, radius=0.3, every=1, lambda_=1.0), list(range(99, -1, -1)))
    assert len(resample_tables(dict(cloud=None, radius=0.3, every=2, lambda_=1.0), list(range(99, -1, -1)))["events"]) == 50


# ------------------------------------------------------------------------------------------------ the Python refusals
def test_python_refusals_before_anything_touches_a_device():
    r = dict(cloud=torch.zeros(4, 2), radius=0.3, lambda_=1.0, every=5)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        make(25, cls="DynamicGaussianDiffusionModel").conditional_sample({}, resample=r)

    def my_step(*a, **k):
        raise AssertionError("never called")
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            make(25, sampler=sampler).conditional_sample({}, sample_fn=my_step, resample=r)
    # a sharded job, and the DDIM loop without inner steps
    dm = make(25, sampler="ddpm", noise_source="philox")
    dm.set_noise_shard(0, 8)
    with pytest.raises(NotImplementedError, match="sharded"):
        dm.conditional_sample({}, batch_size=4, resample=r)
    with pytest.raises(NotImplementedError, match="DDIM"):
        make(25, sampler="ddim").conditional_sample({}, batch_size=4, resample=r)
    with pytest.raises(NotImplementedError, match="predict_epsilon"):
        make(25, sampler="ddpm", predict_epsilon=False).conditional_sample({}, batch_size=4, resample=r)
    # hard-condition values that differ inside a group (host compare), and a scene without a trajectory
    dm = make(25, sampler="ddpm")
    tab = resample_tables(r, dm._ddpm_steps()[0])
    same, other = torch.ones(6, S), torch.ones(6, S)
    other[4, 1] = 2.0
    arrays = _HostArrays()
    with pytest.raises(ValueError, match="differ inside a group"):
        dm._fill_resample(arrays, tab, r, None, {0: same, H - 1: other}, 6)
    two = dict(n_scenes=2, traj_scene=torch.tensor([0, 0, 0, 0, 1, 1], dtype=torch.int32))
    rr = dict(r, clouds=[torch.zeros(4, 2)] * 2); rr.pop("cloud")
    with pytest.raises(ValueError, match="trajectories 4 .. 5"):      # (rows 4 and 5 are a group of their own now, and still differ)
        dm._fill_resample(arrays, tab, rr, two, {0: same, H - 1: other}, 6)
    other[5, 1] = 2.0
    rs, _, gf = dm._fill_resample(arrays, tab, rr, two, {0: same, H - 1: other}, 6)      # (differing BETWEEN groups is fine)
    assert gf.tolist() == [0, 4, 6]
    with pytest.raises(ValueError, match="entries for 2 scene"):
        dm._fill_resample(arrays, tab, dict(rr, clouds=[torch.zeros(4, 2)] * 3), two, {}, 6)
    with pytest.raises(ValueError, match="at least one trajectory"):
        dm._fill_resample(arrays, tab, rr, dict(n_scenes=2, traj_scene=torch.zeros(6, dtype=torch.int32)), {}, 6)
    with pytest.raises(ValueError, match="group table"):
        group_table([0, 3, 3, 6], 6)


# ------------------------------------------------------------------------------------------------ lineage, and the restatement's own property
def test_lineage():
    assert lineage(np.zeros((0, 5), np.int32)).tolist() == [0, 1, 2, 3, 4]
    a = np.array([[0, 0, 2, 3], [1, 1, 3, 3], [0, 2, 2, 3]], np.int32)
    # event 0 puts old 0 into rows 0, 1; event 1 then rows (1, 1, 3, 3); event 2 rows (0, 2, 2, 3)
    want = []
    for i in range(4):
        k = i
        for e in (2, 1, 0):
            k = a[e][k]
        want.append(int(k))
    assert lineage(a).tolist() == want == [0, 3, 3, 3]
    assert lineage(torch.from_numpy(a)).tolist() == want
    x = np.arange(4) * 10.0
    y = x.copy()
    for e in range(3):
        y = y[a[e]]
    assert np.array_equal(y, x[lineage(a)])
    with pytest.raises(ValueError):
        lineage(np.array([[0, 4]]))
    with pytest.raises(ValueError):
        lineage(np.zeros(3, np.int32))


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257, 1025, 4096])
def test_systematic_resampling_gives_floor_or_ceil_children(n):
    """The restatement's own property, 20 seeds per size: trajectory k has floor(n W_k) or ceil(n W_k) children (counted with a slack of one
    part in 1e9 of n W for the rounding of the prefix sums), the ancestors are non-decreasing and their count is n; weights of zero have none."""
    for seed in range(20):
        rng = np.random.default_rng(1000 * n + seed)
        logw = rng.normal(0, 2, n)
        if n > 3:
            logw[rng.integers(0, n, 2)] = -np.inf
        u = np.float32(rng.uniform(0.02, 0.98))
        anc, ess, did, margin, cum = R.resample_group(logw, u, 2.0)
        assert did and anc.min() >= 0 and anc.max() < n and (np.diff(anc) >= 0).all()
        w = np.exp(logw - logw.max())
        nW = n * w / w.sum()
        counts = np.bincount(anc, minlength=n)
        assert counts.sum() == n
        assert (counts >= np.floor(nW * (1 - 1e-9))).all() and (counts <= np.ceil(nW * (1 + 1e-9))).all()
        assert (counts[~np.isfinite(logw)] == 0).all()
        assert 1.0 <= ess <= n * (1 + 1e-12)
    # never: ess_frac 0; all weights zero: identity with ESS 0
    assert not R.resample_group(logw, u, 0.0)[2]
    a, e, did, _, _ = R.resample_group(np.full(n, -np.inf), u, 2.0)
    assert e == 0.0 and not did and a.tolist() == list(range(n))


def test_difference_potential_telescopes():
    """With constant lambda and no resampling the log-weight after any number of events is -lambda c of the last one."""
    rng = np.random.default_rng(3)
    cost = rng.uniform(0, 2, (4, 9))
    anc, ess, logw, _ = R.replay_events(cost, np.array([0, 4, 9]), [1.5] * 4, np.full((4, 2), 0.5), 0.0)
    assert np.allclose(logw, -1.5 * cost[-1], rtol=0, atol=1e-14) and (anc == np.arange(9)).all()
    # a non-finite cost is a weight of zero from then on
    cost[1, 2] = np.nan
    _, ess, logw, _ = R.replay_events(cost, np.array([0, 4, 9]), [1.5] * 4, np.full((4, 2), 0.5), 0.0)
    assert logw[2] == -np.inf and np.isfinite(np.delete(logw, 2)).all() and np.isfinite(ess).all()


# ------------------------------------------------------------------------------------------------ what the GPU tests ask of their inputs
@pytest.mark.parametrize("name", list(R.KERNEL_CASES))
def test_kernel_inputs_satisfy_their_precondition(name):
    margin, bar = R.kernel_precondition(name)
    print(f"{name}: smallest margin / n {margin:.3e}, bar {bar:.3e}")
    assert margin > bar


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_chain_inputs_satisfy_their_conditions(kind):
    """What tests/test_gpu_resample.py::test_free_running_steered_chain asks of its inputs, on the oracle alone: no (group, event) is left out,
    at least two of them resample, and steering moves the final float64 states by more than 100 x the chain's bar."""
    left_out, events, resampled, bar, moved = R.chain_conditions(kind)
    print(f"{kind}: {events} (group, event) pairs, {resampled} resample, {left_out} left out; bar {bar:.3e}; steered vs unsteered {moved:.3e}")
    assert left_out == 0 and resampled >= 2 and moved > 100 * bar
