"""Host side of the cost-gradient guidance (``cost_guide=`` -> ``ramp_sample_guided``): the definition's gradient against finite
differences of its own cost, the per-iteration tables, struct layout, the declared / bound / exported symbols, the refusals that need no
device, and the conditions the free-running GPU test asks of its inputs.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import test_gpu_guide as G
from ramp_amd import _lib
from ramp_amd.diffusion import guide_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S = 48, 4


def make(T, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    kw.setdefault("predict_epsilon", True)
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=H, state_dim=S), n_diffusion_steps=T, **kw)


# ------------------------------------------------------------------------------------------------ the definition
def exact_cost(p, c, r, w):
    """C of positions p (H, d) in float64, its terms added exactly (math.fsum): the difference quotient then sees no summation noise."""
    terms = []
    if len(c):
        u = np.maximum(0.0, r - np.sqrt(((p[:, None, :] - c[None, :, :]) ** 2).sum(-1)))
        terms += (w[0] * 0.5 * u * u).ravel().tolist()
    terms += (w[1] * 0.5 * ((p[1:] - p[:-1]) ** 2).sum(1)).tolist()
    terms += (w[2] * 0.5 * ((p[2:] - 2 * p[1:-1] + p[:-2]) ** 2).sum(1)).tolist()
    return math.fsum(terms)


@pytest.mark.parametrize("pinned", [(0, 7), (0, 4, 7)], ids=["ends", "interior"])
@pytest.mark.parametrize("P", [0, 1, 65, 1025])
@pytest.mark.parametrize("d", [2, 3])
def test_gradient_is_the_costs_own_derivative(d, P, pinned):
    """The restatement's gradient (tests/test_gpu_guide.py) equals central finite differences of its own cost in float64 to < 1e-8 of
    the largest component, with the pinned waypoints held at their conditioned values; guide_terms is that cost's three terms."""
    Hh, r, w = 8, 0.35, (1.0, 0.5, 0.25)
    rng = np.random.default_rng(10 * d + P)
    p = rng.uniform(-1, 1, (Hh, d))
    c = rng.uniform(-1, 1, (P, d)) if P != 1 else p[2:3] + 0.1      # (one point: within r of a free waypoint)
    for h in pinned:
        p[h] = rng.uniform(-1, 1, d)
    g = G.guide_grad(p, c, r, *w)
    assert g.dtype == np.float64
    t = G.guide_terms(p, c, r)
    assert abs(float(np.dot(w, t)) - exact_cost(p, c, r, w)) <= 1e-12 * max(1.0, exact_cost(p, c, r, w))
    eps, worst = 1e-6, 0.0
    for h in range(Hh):
        for k in range(d):
            if h in pinned:
                continue
            q1, q2 = p.copy(), p.copy()
            q1[h, k] += eps; q2[h, k] -= eps
            fd = (exact_cost(q1, c, r, w) - exact_cost(q2, c, r, w)) / (q1[h, k] - q2[h, k])
            worst = max(worst, abs(fd - g[h, k]))
    scale = float(np.abs(g).max())
    assert scale > 0 and worst < 1e-8 * scale, (worst, scale)
    # one iteration moves the free waypoints by -step s g and leaves the pinned ones and the other channels alone
    x = np.zeros((1, Hh, d + 1)); x[0, :, :d] = p; x[0, :, d] = 7.0
    pins = {h: np.append(p[h], 0.0) for h in pinned}
    gz = g.copy(); gz[list(pinned)] = 0
    n = float(np.sqrt((gz ** 2).sum()))
    for max_norm in (0.0, 0.5 * n):
        y = G.guide_iterate(x, [c if P else np.zeros((0, d))], None, pins, r, *w, 1e-3, 1, max_norm, np.float64, d=d)
        s = 1.0 if max_norm == 0 else 0.5
        assert np.allclose(y[0, :, :d], p - 1e-3 * s * gz, rtol=0, atol=1e-15) and (y[0, :, d] == 7.0).all()


# ------------------------------------------------------------------------------------------------ guide_tables
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_tables_t_start_variance_and_sequences(sampler):
    T = 25 if sampler == "ddpm" else 100
    dm = make(T, sampler=sampler)
    steps = dm._ddpm_steps()[0] if sampler == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    n = len(steps)
    base = dict(cloud=None, radius=0.3, step=0.01)
    tab = guide_tables(base, steps, dm.posterior_variance)
    assert tab["n_guide"] == [1] * n and tab["step"] == [0.01] * n and tab["total"] == n      # defaults: n_steps 1, t_start inf
    assert (tab["radius"], tab["w_obs"], tab["w_smooth"], tab["w_acc"], tab["max_norm"]) == (0.3, 1.0, 0.0, 0.0, 0.0)
    # the boundary: t == t_start is off, t_start - 1 is on
    ts = steps[2]
    tab = guide_tables(dict(base, n_steps=3, t_start=ts), steps, dm.posterior_variance)
    assert tab["n_guide"] == [3 if t < ts else 0 for t in steps] and tab["n_guide"][2] == 0 and tab["n_guide"][3] == 3
    assert guide_tables(dict(base, t_start=0), steps, dm.posterior_variance)["total"] == 0
    assert guide_tables(dict(base, t_start=1), steps, dm.posterior_variance)["n_guide"] == [1 if t == 0 else 0 for t in steps]
    # scale_by_variance against the schedule buffer
    pv = dm.posterior_variance.double().numpy()
    tab = guide_tables(dict(base, step=2.0, scale_by_variance=True), steps, dm.posterior_variance)
    assert np.allclose(tab["step"], 2.0 * pv[steps], rtol=1e-15, atol=0)
    # per-iteration sequences
    Ks, st = [j % 4 for j in range(n)], [0.001 * (j + 1) for j in range(n)]
    tab = guide_tables(dict(base, n_steps=Ks, step=st, scale_by_variance=True, t_start=steps[1]), steps, dm.posterior_variance)
    assert tab["n_guide"] == [0, 0] + Ks[2:] and np.allclose(tab["step"], np.array(st) * pv[steps], rtol=1e-15, atol=0)
    # through the model: the same tables as ramp_cost_guide, one (P, 2) cloud and a (No, Np, 3) one
    from ramp_amd.diffusion import _HostArrays
    arrays = _HostArrays()
    cg = dm._fill_guide(arrays, tab, dict(cloud=torch.zeros(7, 2)), None)
    assert (cg.point_dim, cg.n_scenes, cg.radius, cg.w_obs) == (2, 1, 0.3, 1.0) and [cg.cloud_offset_host[i] for i in range(2)] == [0, 7]
    assert [cg.n_guide[j] for j in range(n)] == tab["n_guide"] and [cg.step[j] for j in range(n)] == [np.float32(v) for v in tab["step"]]
    cg = dm._fill_guide(arrays, tab, dict(clouds=[torch.zeros(2, 5, 3), torch.zeros(0, 3)]), dict(n_scenes=2))
    assert cg.point_dim == 3 and [cg.cloud_offset_host[i] for i in range(3)] == [0, 10, 10]


@pytest.mark.parametrize("g, exc, msg", [
    ("guide", TypeError, "takes a dict"),
    (dict(cloud=None, radius=0.3, step=0.01, stepsize=1), ValueError, "unknown keys"),
    (dict(cloud=None, radius=0.3, step=0.01, guide=1), ValueError, "unknown keys"),
    (dict(radius=0.3, step=0.01), ValueError, "exactly one of cloud= and clouds="),
    (dict(cloud=None, clouds=[], radius=0.3, step=0.01), ValueError, "exactly one of cloud= and clouds="),
    (dict(cloud=None, radius=0.3), ValueError, "step= is required"),
    (dict(cloud=None, step=0.01), ValueError, "radius must be positive"),
    (dict(cloud=None, radius=0.0, step=0.01), ValueError, "radius must be positive"),
    (dict(cloud=None, radius=-1.0, step=0.01), ValueError, "radius must be positive"),
    (dict(cloud=None, radius=float("nan"), step=0.01), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, step=0.01, w_obs=float("inf")), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, step=0.01, w_smooth=float("nan")), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, step=0.01, w_acc=float("nan")), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, step=0.01, max_norm=float("inf")), ValueError, "must be finite"),
    (dict(cloud=None, radius=0.3, step=float("nan")), ValueError, "step sizes must be finite"),
    (dict(cloud=None, radius=0.3, step=[0.01] * 24 + [float("inf")]), ValueError, "step sizes must be finite"),
    (dict(cloud=None, radius=0.3, step=[0.01, 0.02]), ValueError, "2 entries for 25"),
    (dict(cloud=None, radius=0.3, step=0.01, n_steps=[1, 2, 3]), ValueError, "3 entries for 25"),
    (dict(cloud=None, radius=0.3, step=0.01, n_steps=17), ValueError, "0 .. 16"),
    (dict(cloud=None, radius=0.3, step=0.01, n_steps=-1), ValueError, "0 .. 16"),
    (dict(cloud=None, radius=0.3, step=0.01, t_start=float("nan")), ValueError, "t_start"),
])
def test_bad_tables_are_refused_with_a_message(g, exc, msg):
    dm = make(25, sampler="ddpm")
    with pytest.raises(exc, match=msg):
        guide_tables(g, dm._ddpm_steps()[0], dm.posterior_variance)


def test_radius_is_not_needed_without_an_obstacle_term():
    dm = make(25, sampler="ddpm")
    assert guide_tables(dict(cloud=None, w_obs=0.0, w_smooth=1.0, step=0.01), dm._ddpm_steps()[0], dm.posterior_variance)["total"] == 25


def test_python_refusals_before_anything_touches_a_device():
    g = dict(cloud=torch.zeros(4, 2), radius=0.3, step=0.01)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        make(25, cls="DynamicGaussianDiffusionModel").conditional_sample({}, cost_guide=g)

    def my_step(*a, **k):
        raise AssertionError("never called")
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            make(25, sampler=sampler).conditional_sample({}, sample_fn=my_step, cost_guide=g)
    # the cloud table
    from ramp_amd.guide import cloud_table
    with pytest.raises(ValueError, match="d = 2 or 3"):
        cloud_table([torch.zeros(4, 4)], "cpu")
    with pytest.raises(ValueError, match="same point dimension"):
        cloud_table([torch.zeros(4, 2), torch.zeros(4, 3)], "cpu")
    pts, off, d = cloud_table([torch.zeros(0, 3), torch.ones(2, 2, 3)], "cpu")
    assert d == 3 and off.tolist() == [0, 0, 4] and off.dtype == np.int32 and tuple(pts.shape) == (4, 3)
    assert cloud_table([torch.zeros(0, 2)], "cpu")[0] is None


# ------------------------------------------------------------------------------------------------ the C side
def test_cost_guide_layout_matches_the_header():
    """The ctypes mirror of ramp_cost_guide has the size and field offsets the C compiler gives it (the method of
    test_struct_layout_matches_header); RAMP_GUIDE_MAX_STEPS is 16 on both sides."""
    cls = _lib.RampCostGuide
    body = 'printf("%zu", sizeof(ramp_cost_guide));' + "".join(f'printf(" %zu", offsetof(ramp_cost_guide, {f}));' for f, _ in cls._fields_)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf(" %d\\n", RAMP_GUIDE_MAX_STEPS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got[:-1] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert got[-1] == _lib.GUIDE_MAX_STEPS == 16
    assert C.sizeof(cls) == 80


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_guided", 13), ("ramp_guide_step", 12), ("ramp_guide_cost", 8)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_guided"][1][2] == C.POINTER(_lib.RampCostGuide)
    assert _lib.PROTOTYPES["ramp_sample_guided"][1][3] == C.POINTER(_lib.RampMcmcParams)
    from ramp_amd import build
    assert "guide.hip" in build.SOURCES and build.EXTRA_FLAGS["guide.hip"] == ["-ffp-contract=off"]


def test_host_refusals_of_the_kernel_level_entries():
    """ramp_guide_step / ramp_guide_cost refuse on the host before any device call: non-zero, the entry's name in ramp_last_error.  (The
    pointers are never dereferenced: every call here is refused.)"""
    lib = _lib.load()
    off = (C.c_int32 * 2)(0, 5)

    def guide(**kw):
        cg = _lib.RampCostGuide()
        cg.point_dim, cg.n_scenes, cg.cloud_points, cg.cloud_offset_host = 2, 1, 0x1000, C.cast(off, _lib.c_i32p)
        cg.radius, cg.w_obs = 0.3, 1.0
        for k, v in kw.items():
            setattr(cg, k, v)
        return cg

    def step(cg, S=4, n_iter=1, step=0.01, n_hard=0, idx=None):
        rc = lib.ramp_guide_step(0x1000, 2, 8, S, C.byref(cg), None, n_iter, step, n_hard, idx, 0x1000 if n_hard else None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_step" in msg, (rc, msg)
        return msg

    def cost(cg, S=4):
        rc = lib.ramp_guide_cost(0x1000, 2, 8, S, C.byref(cg), None, 0x1000, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_cost" in msg, (rc, msg)
        return msg

    for fn in (step, cost):
        assert "point_dim" in fn(guide(point_dim=1))
        assert "point_dim" in fn(guide(point_dim=4))
        assert "point_dim" in fn(guide(point_dim=3), S=2)                      # > state_dim
        for k in ("radius", "w_obs", "w_smooth", "w_acc", "max_norm"):
            assert "finite" in fn(guide(**{k: float("nan")})) and "finite" in fn(guide(**{k: float("inf")}))
        assert "radius" in fn(guide(radius=0.0)) and "radius" in fn(guide(radius=-1.0))
        assert "offsets" in fn(guide(cloud_offset_host=C.cast((C.c_int32 * 2)(1, 5), _lib.c_i32p)))
        assert "non-decreasing" in fn(guide(n_scenes=2, cloud_offset_host=C.cast((C.c_int32 * 3)(0, 5, 3), _lib.c_i32p)))
        assert "cloud_points" in fn(guide(cloud_points=None))
        assert "at least one scene" in fn(guide(n_scenes=0))
    assert "n_iter" in step(guide(), n_iter=17) and "n_iter" in step(guide(), n_iter=-1)
    assert "step" in step(guide(), step=float("nan")) and "step" in step(guide(), step=float("inf"))
    assert "hard" in step(guide(), n_hard=1, idx=C.cast((C.c_int32 * 1)(8), _lib.c_i32p))
    assert lib.ramp_guide_step(0x1000, 2, 129, 4, C.byref(guide()), None, 1, 0.01, 0, None, None, None) != 0
    assert "H up to 128" in lib.ramp_last_error().decode()
    # the job entry without a context
    assert lib.ramp_sample_guided(None, None, None, None, None, None, None, None, None, None, None, None, None) != 0
    assert "ramp_sample_guided" in lib.ramp_last_error().decode()


def test_free_running_chain_inputs_satisfy_their_conditions():
    """What tests/test_gpu_guide.py::test_free_running_guided_chain asks of its inputs, checked on the CPU: the float32 oracle stays within a
    quarter of the bar (1e-4 of max |x|) and the float64 guided and unguided final states differ by at least 100 x the bar.  Measured:
    DDPM (T = 3) bar 2.45e-4, float32 oracle 3.97e-5, guided vs unguided 8.6e-2; DDIM-5 bar 2.45e-4, 1.5e-6, 4.9e-2."""
    for kind in ("ddpm", "ddim"):
        bar, d32, moved = G.chain_conditions(kind)
        print(f"{kind}: bar {bar:.3e}, float32 oracle {d32:.3e}, guided vs unguided {moved:.3e}")
        assert d32 <= bar / 4 and moved >= 100 * bar
