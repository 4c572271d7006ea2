"""Host side of the cost guidance inside the replanning jobs (``replan_guide=`` -> ``ramp_replan_guided`` / ``ramp_replan_episodes_guided``):
the numpy restatement of the definition in include/ramp_hip.h (``moving_grad`` / ``moving_iterate`` / ``moving_terms``: test_gpu_guide.py's
restatement extended by the moving term and the per-row pins; tests/test_gpu_replan_guide.py measures the kernels against it), its gradient
against finite differences of its own cost, the predictors, struct layout, the declared / bound / exported symbols and every refusal that
needs no device.  No GPU."""
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
from ramp_amd.guide import predict_track, replan_guide_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the definition, in numpy
def pair_grad(q, c, r):
    """d/dq sum_j 1/2 max(0, r - |q_h - c_j|)^2 (H, 2) in q's dtype; a pair at distance 0 contributes nothing."""
    dt = q.dtype.type
    dx = q.T[:, :, None] - c.T.astype(q.dtype)[:, None, :]                    # (2, H, P)
    d = np.sqrt((dx * dx).sum(0))
    inside = (d < dt(r)) & (d > 0)
    f = np.where(inside, (dt(r) - d) / np.where(inside, d, dt(1)), dt(0)).astype(q.dtype)
    return (-(f[None] * dx).sum(-1).T).astype(q.dtype)


def pair_cost(q, c, r):
    dt = q.dtype.type
    dx = q.T[:, :, None] - c.T.astype(q.dtype)[:, None, :]
    u = np.maximum(dt(0), dt(r) - np.sqrt((dx * dx).sum(0)))
    return float((dt(0.5) * u * u).astype(np.float64).sum())


def moving_terms(p, c, m, delta, r, r_mov):
    """(C_obs, C_mov, C_smooth, C_acc), unweighted, of positions p (H, 2): pair values in p's dtype, sums in float64."""
    t = G.guide_terms(p, c, r)
    mov = pair_cost(p - delta.astype(p.dtype), m, r_mov) if len(m) else 0.0
    return np.array([t[0], mov, t[1], t[2]])


def moving_grad(p, c, m, delta, r, r_mov, w_obs, w_mov, w_smooth, w_acc):
    """dC/dp (H, 2) in p's dtype: g = w_obs g_obs + (w_mov g_mov + (w_smooth g_smooth + w_acc g_acc)), the header's order; the moving pair's
    difference is (p - delta) - m."""
    dt = p.dtype.type
    g = G.guide_grad(p, np.zeros((0, 2), p.dtype), r, 0.0, w_smooth, w_acc)
    if len(m) and w_mov != 0:
        g = dt(w_mov) * pair_grad(p - delta.astype(p.dtype), m, r_mov) + g
    if len(c) and w_obs != 0:
        g = dt(w_obs) * pair_grad(p, c, r) + g
    return g.astype(p.dtype)


def pinned_copy(xb, b, pin_first, hard, dtype):
    """The working copy (H, 2) of row xb (H, S) and its free mask: waypoints < pin_first, waypoint H - 1 and the waypoints of ``hard`` (a list
    of (waypoint, (B, S) values), later entries win) are pinned; a pinned waypoint the list names takes its value, another keeps its own."""
    H = xb.shape[0]
    p = xb[:, :2].astype(dtype).copy()
    free = np.ones(H, bool)
    free[:max(0, min(H, int(pin_first)))] = False
    free[H - 1] = False
    for h, v in hard:
        p[h] = np.asarray(v)[b, :2].astype(dtype)
        free[h] = False
    return p, free


def moving_iterate(x, clouds, moving, tracks, traj_scene, pin_first, hard, r, r_mov, w_obs, w_mov, w_smooth, w_acc, step, n_iter, max_norm, dtype,
                   log=None):
    """n_iter iterations of the replans' guide on rows x (B, H, S) -> new array of ``dtype``.  clouds: per scene (P, 2); moving (n_scenes, M, 2);
    tracks (n_scenes, H, 2); traj_scene (B,) (a row whose scene is outside the table stays); pin_first (B,); hard as in ``pinned_copy``.
    ``log`` collects (row, iteration, s, |g|)."""
    out = np.array(x, dtype=dtype)
    dt = out.dtype.type
    B, H, S = out.shape
    for b in range(B):
        e = int(traj_scene[b])
        if not 0 <= e < len(clouds):
            continue
        c, m, delta = clouds[e].reshape(-1, 2), moving[e].reshape(-1, 2), tracks[e].astype(dtype)
        p, free = pinned_copy(out[b], b, pin_first[b], hard, dtype)
        for it in range(n_iter):
            g = moving_grad(p, c, m, delta, r, r_mov, w_obs, w_mov, w_smooth, w_acc)
            g[~free] = 0
            n = dt(np.sqrt((g.astype(np.float64) ** 2).sum()))
            s = min(dt(1), dt(max_norm) / n) if (max_norm > 0 and n > 0) else dt(1)
            if log is not None:
                log.append((b, it, float(s), float(n)))
            p[free] = (p - (dt(step) * dt(s)) * g)[free]
        out[b, free, :2] = p[free]
    return out


def exact_cost(p, c, m, delta, r, r_mov, w):
    """C of positions p (H, 2) in float64, its terms added exactly (math.fsum)."""
    terms = []
    for q, cl, rr, ww in ((p, c, r, w[0]), (p - delta, m, r_mov, w[1])):
        if len(cl):
            u = np.maximum(0.0, rr - np.sqrt(((q[:, None, :] - cl[None, :, :]) ** 2).sum(-1)))
            terms += (ww * 0.5 * u * u).ravel().tolist()
    terms += (w[2] * 0.5 * ((p[1:] - p[:-1]) ** 2).sum(1)).tolist()
    terms += (w[3] * 0.5 * ((p[2:] - 2 * p[1:-1] + p[:-2]) ** 2).sum(1)).tolist()
    return math.fsum(terms)


@pytest.mark.parametrize("P,M", [(0, 0), (65, 0), (0, 64), (65, 64), (1025, 1024)])
def test_gradient_is_the_costs_own_derivative(P, M):
    """The restatement's gradient agrees with central finite differences of its own four-term cost at 20 random free coordinates (float64,
    h = 1e-6, relative 1e-5 of the largest component); pinned waypoints get zero gradient in an iteration; moving_terms is that cost's terms."""
    Hh, r, r_mov, w = 12, 0.35, 0.3, (1.0, 0.75, 0.5, 0.25)
    rng = np.random.default_rng(100 + P + M)
    p = rng.uniform(-1, 1, (Hh, 2))
    c, m, delta = rng.uniform(-1, 1, (P, 2)), rng.uniform(-1, 1, (M, 2)), rng.uniform(-0.3, 0.3, (Hh, 2))
    g = moving_grad(p, c, m, delta, r, r_mov, *w)
    assert g.dtype == np.float64
    t = moving_terms(p, c, m, delta, r, r_mov)
    want = exact_cost(p, c, m, delta, r, r_mov, w)
    assert abs(float(np.dot(w, t)) - want) <= 1e-12 * max(1.0, want)
    pin_first, hard = 3, [(6, np.tile(rng.uniform(-1, 1, (1, 4)), (1, 1)))]
    x = np.zeros((1, Hh, 4)); x[0, :, :2] = p; x[0, :, 2:] = 7.0
    pw, free = pinned_copy(x[0], 0, pin_first, hard, np.float64)
    assert sorted(np.nonzero(~free)[0].tolist()) == [0, 1, 2, 6, Hh - 1]
    gw = moving_grad(pw, c, m, delta, r, r_mov, *w)
    scale = float(np.abs(gw).max())
    coords = [(h, k) for h in np.nonzero(free)[0] for k in range(2)]
    picks = [coords[i] for i in rng.choice(len(coords), 20, replace=len(coords) < 20)]
    eps, worst = 1e-6, 0.0
    for h, k in picks:
        q1, q2 = pw.copy(), pw.copy()
        q1[h, k] += eps; q2[h, k] -= eps
        fd = (exact_cost(q1, c, m, delta, r, r_mov, w) - exact_cost(q2, c, m, delta, r, r_mov, w)) / (q1[h, k] - q2[h, k])
        worst = max(worst, abs(fd - gw[h, k]))
    assert scale > 0 and worst <= 1e-5 * scale, (worst, scale)
    # one iteration: the free waypoints move by -step g, the pinned ones (zero gradient) and the other channels stay
    y = moving_iterate(x, [c], m[None], delta[None], [0], [pin_first], hard, r, r_mov, *w, 1e-3, 1, 0.0, np.float64)
    gz = gw.copy(); gz[~free] = 0
    assert np.allclose(y[0, free, :2], (pw - 1e-3 * gz)[free], rtol=0, atol=1e-15)
    assert np.array_equal(y[0, ~free], x[0, ~free]) and (y[0, :, 2:] == 7.0).all()
    # a row whose scene is outside the table stays
    assert np.array_equal(moving_iterate(x, [c], m[None], delta[None], [1], [pin_first], hard, r, r_mov, *w, 1e-3, 1, 0.0, np.float64), x)


def test_without_a_moving_term_it_is_the_static_guides_restatement():
    rng = np.random.default_rng(5)
    p, c = rng.uniform(-1, 1, (9, 2)).astype(np.float32), rng.uniform(-1, 1, (70, 2)).astype(np.float32)
    none = np.zeros((0, 2), np.float32)
    a = moving_grad(p, c, none, np.zeros((9, 2), np.float32), 0.35, 0.35, 1.0, 1.0, 0.5, 0.25)
    assert np.array_equal(a, G.guide_grad(p, c, 0.35, 1.0, 0.5, 0.25))
    assert np.array_equal(moving_terms(p, c, none, np.zeros((9, 2)), 0.35, 0.35)[[0, 2, 3]], G.guide_terms(p, c, 0.35))


# ------------------------------------------------------------------------------------------------ the predictors and the dict
def test_predictors():
    H = 6
    plan = np.zeros((H, 2))
    assert np.array_equal(predict_track('hold', [1.0, 2.0], [0.5, 0.5], plan, 2), np.zeros((H, 2), np.float32))
    assert predict_track('hold', [1.0, 2.0], None, plan, 0).dtype == np.float32
    cv = predict_track('constant_velocity', [1.0, 2.0], [0.75, 2.5], plan, 2)
    want = np.float32([[0, 0], [0, 0], [0, 0], [0.25, -0.5], [0.5, -1.0], [0.75, -1.5]])
    assert cv.dtype == np.float32 and np.array_equal(cv, want)
    assert np.array_equal(predict_track('constant_velocity', [1.0, 2.0], None, plan, 2), np.zeros((H, 2), np.float32))      # an episode's first replan
    seen = []

    def mine(now, prev, plan_xy, stepp):
        seen.append((tuple(now), prev, plan_xy.shape, stepp))
        return np.full((H, 2), 0.125)
    assert np.array_equal(predict_track(mine, [1.0, 2.0], None, plan, 4), np.full((H, 2), 0.125, np.float32))
    assert seen == [((1.0, 2.0), None, (H, 2), 4)]
    with pytest.raises(ValueError, match="predict returned shape"):
        predict_track(lambda *a: np.zeros((H, 3)), [0, 0], None, plan, 0)
    with pytest.raises(ValueError, match="predict returned shape"):
        predict_track(lambda *a: np.zeros((H - 1, 2)), [0, 0], None, plan, 0)
    with pytest.raises(ValueError, match="non-finite"):
        predict_track(lambda *a: np.full((H, 2), np.nan), [0, 0], None, plan, 0)
    # the predictors draw no random numbers
    st = np.random.get_state()[1].copy()
    predict_track('constant_velocity', [1.0, 2.0], [0.0, 0.0], plan, 1)
    assert np.array_equal(np.random.get_state()[1], st)


def test_tables_defaults_and_t_start():
    low = [40, 30, 20, 10, 0]
    tab = replan_guide_tables(dict(radius=0.3, step=0.01), low)
    assert tab['n_guide'] == [0, 0, 0, 0, 1] and tab['step'] == [0.01] * 5 and tab['total'] == 1      # the default guides the last step only
    assert (tab['radius'], tab['radius_mov'], tab['w_obs'], tab['w_mov'], tab['w_smooth'], tab['w_acc'], tab['max_norm']) == (0.3, 0.3, 1.0, 1.0, 0.0, 0.0, 0.0)
    assert tab['predict'] == 'constant_velocity' and tab['cloud'] is None
    tab = replan_guide_tables(dict(radius=0.3, step=0.01, radius_moving=0.2, n_steps=4, t_start=21, w_moving=2.0), low)
    assert tab['n_guide'] == [0, 0, 4, 4, 4] and tab['radius_mov'] == 0.2 and tab['w_mov'] == 2.0
    assert replan_guide_tables(dict(radius=0.3, step=0.01, t_start=0), low)['total'] == 0
    assert replan_guide_tables(dict(radius=0.3, step=0.01, t_start=float('inf')), low)['n_guide'] == [1] * 5


@pytest.mark.parametrize("g, exc, msg", [
    ("guide", TypeError, "takes a dict"),
    (dict(radius=0.3, step=0.01, predict='ballistic'), ValueError, "unknown predict"),
    (dict(step=0.01), ValueError, "radius= is required"),
    (dict(radius=0.3), ValueError, "step= is required"),
    (dict(radius=0.3, step=0.01, stepsize=1), ValueError, "unknown keys"),
    (dict(radius=0.0, step=0.01), ValueError, "must be positive"),
    (dict(radius=0.3, step=0.01, radius_moving=-1.0), ValueError, "must be positive"),
    (dict(radius=float("nan"), step=0.01), ValueError, "must be finite"),
    (dict(radius=0.3, step=float("inf")), ValueError, "must be finite"),
    (dict(radius=0.3, step=0.01, n_steps=17), ValueError, "0 .. 16"),
    (dict(radius=0.3, step=0.01, t_start=float("nan")), ValueError, "t_start"),
])
def test_python_refusals_of_the_dict(g, exc, msg):
    with pytest.raises(exc, match=msg):
        replan_guide_tables(g, [40, 30, 20, 10, 0])


def test_python_refusals_through_the_model():
    """The dict is checked before anything touches a device -- here by the helper the planners call first -- and cost_guide= / mcmc= /
    resample= on the dynamic model keep raising."""
    from ramp_amd import models
    from ramp_amd.diffusion import _HostArrays
    dm = models.DynamicGaussianDiffusionModel(model=models.TemporalUnetInference(n_support_points=48, state_dim=4), n_diffusion_steps=100,
                                              predict_epsilon=True)
    for g, msg in ((dict(radius=0.3, step=0.01, predict='ballistic'), "unknown predict"), (dict(step=0.01), "radius= is required"),
                   (dict(radius=0.3), "step= is required")):
        with pytest.raises(ValueError, match=msg):
            dm._replan_guide_setup(g, [40, 30, 20, 10, 0], [torch.zeros(4, 2)], _HostArrays())
    assert dm._replan_guide_setup(dict(radius=0.3, step=0.01, t_start=0), [40, 30, 20, 10, 0], [torch.zeros(4, 2)], _HostArrays()) is None
    g = dict(cloud=torch.zeros(4, 2), radius=0.3, step=0.01)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dm.conditional_sample({}, cost_guide=g)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dm.conditional_sample({}, mcmc=dict(kind='ula'))
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dm.conditional_sample({}, resample=dict())
    import inspect
    for fn in (dm.ddim_p_sample_loop, dm.run_inference_episodes):
        assert "replan_guide" in inspect.signature(fn).parameters


# ------------------------------------------------------------------------------------------------ the C side
def test_replan_guide_layout_matches_the_header():
    """The ctypes mirror of ramp_replan_guide has the size and field offsets the C compiler gives it (the method of
    test_struct_layout_matches_header)."""
    cls = _lib.RampReplanGuide
    body = 'printf("%zu", sizeof(ramp_replan_guide));' + "".join(f'printf(" %zu", offsetof(ramp_replan_guide, {f}));' for f, _ in cls._fields_)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf("\\n");return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert C.sizeof(cls) == 120


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_replan_guided", 9), ("ramp_replan_episodes_guided", 10), ("ramp_guide_step_moving", 13), ("ramp_guide_cost_moving", 8)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_replan_guided"][1][3] == C.POINTER(_lib.RampReplanGuide)
    assert _lib.PROTOTYPES["ramp_replan_episodes_guided"][1][3] == C.POINTER(_lib.RampReplanGuide)
    assert "take no guide" not in hdr
    from ramp_amd import build
    assert "guide_replan.hip" in build.SOURCES and build.EXTRA_FLAGS["guide_replan.hip"] == ["-ffp-contract=off"]


def make_guide(keep, **kw):
    """A well-formed ramp_replan_guide on pointers that no refused call dereferences (the host tables are real)."""
    off = (C.c_int32 * 2)(0, 5)
    mov, trk = (C.c_float * 8)(), (C.c_float * 16)()
    n_guide, step = (C.c_int32 * 5)(0, 0, 0, 0, 1), (C.c_float * 5)(*[0.01] * 5)
    keep += [off, mov, trk, n_guide, step]
    rg = _lib.RampReplanGuide()
    rg.n_scenes, rg.n_mov, rg.cloud_points, rg.cloud_offset_host = 1, 4, 0x1000, C.cast(off, _lib.c_i32p)
    rg.mov_points_host, rg.mov_track_host = C.cast(mov, _lib.c_f32p), C.cast(trk, _lib.c_f32p)
    rg.radius, rg.radius_mov, rg.w_obs, rg.w_mov = 0.3, 0.3, 1.0, 1.0
    rg.n_guide, rg.step = C.cast(n_guide, _lib.c_i32p), C.cast(step, _lib.c_f32p)
    for k, v in kw.items():
        setattr(rg, k, v)
    return rg


def test_host_refusals_of_the_kernel_level_entries():
    """ramp_guide_step_moving / ramp_guide_cost_moving refuse on the host before any device call: non-zero, the entry's name in
    ramp_last_error.  (The device pointers are never dereferenced: every call here is refused.)"""
    lib = _lib.load()
    keep = []

    def step(rg, H=8, S=4, n_iter=1, step=0.01, n_hard=0, idx=None):
        rc = lib.ramp_guide_step_moving(0x1000, 2, H, S, C.byref(rg), None, None, n_iter, step, n_hard, idx, 0x1000 if n_hard else None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_step_moving" in msg, (rc, msg)
        return msg

    def cost(rg, H=8, S=4):
        rc = lib.ramp_guide_cost_moving(0x1000, 2, H, S, C.byref(rg), None, 0x1000, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_guide_cost_moving" in msg, (rc, msg)
        return msg

    for fn in (step, cost):
        assert "n_mov" in fn(make_guide(keep, n_mov=-1)) and "n_mov" in fn(make_guide(keep, n_mov=1025))
        assert "n_scenes" in fn(make_guide(keep, n_scenes=0))
        assert "offsets" in fn(make_guide(keep, cloud_offset_host=C.cast((C.c_int32 * 2)(1, 5), _lib.c_i32p)))
        assert "offsets" in fn(make_guide(keep, cloud_offset_host=None))
        assert "non-decreasing" in fn(make_guide(keep, n_scenes=2, cloud_offset_host=C.cast((C.c_int32 * 3)(0, 5, 3), _lib.c_i32p)))
        for k in ("radius", "radius_mov", "w_obs", "w_mov", "w_smooth", "w_acc", "max_norm"):
            assert "finite" in fn(make_guide(keep, **{k: float("nan")})) and "finite" in fn(make_guide(keep, **{k: float("inf")}))
        assert "radius must be positive" in fn(make_guide(keep, radius=0.0)) and "radius must be positive" in fn(make_guide(keep, radius=-1.0))
        assert "radius_mov must be positive" in fn(make_guide(keep, radius_mov=0.0))
        assert "cloud_points" in fn(make_guide(keep, cloud_points=None))
        assert "moving points" in fn(make_guide(keep, mov_points_host=None)) and "moving points" in fn(make_guide(keep, mov_track_host=None))
        assert "up to 128" in fn(make_guide(keep), H=129)
        assert "state_dim" in fn(make_guide(keep), S=1)
    assert "n_iter" in step(make_guide(keep), n_iter=17) and "n_iter" in step(make_guide(keep), n_iter=-1)
    assert "step" in step(make_guide(keep), step=float("nan")) and "step" in step(make_guide(keep), step=float("inf"))
    assert "hard" in step(make_guide(keep), n_hard=1, idx=C.cast((C.c_int32 * 1)(8), _lib.c_i32p))
    assert "hard" in step(make_guide(keep), n_hard=1, idx=None)
    assert lib.ramp_guide_cost_moving(0x1000, 2, 8, 4, C.byref(make_guide(keep)), None, None, None) != 0      # no output array
    assert "ramp_guide_cost_moving" in lib.ramp_last_error().decode()
    # what is allowed: radius_mov <= 0 without a moving term is no refusal of its own (the next check speaks)
    assert "n_iter" in step(make_guide(keep, radius_mov=0.0, w_mov=0.0), n_iter=17)
    assert "n_iter" in step(make_guide(keep, radius_mov=0.0, n_mov=0), n_iter=17)
    # the job entries without a context
    for name, n in (("ramp_replan_guided", 9), ("ramp_replan_episodes_guided", 10)):
        args = [None] * n
        args[3] = C.byref(make_guide(keep))
        assert getattr(lib, name)(*args) != 0
        assert name in lib.ramp_last_error().decode()
