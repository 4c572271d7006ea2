"""Warm-started jobs, host side: the tables of ``ramp_amd.warm`` on hand-worked cases, the numpy references, the prior helpers, the ctypes
mirror of ``ramp_warm_start``, the Python layer's host refusals and the conditions the free-running GPU test's inputs must satisfy."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import warm_ref as R
from ramp_amd import _lib
from ramp_amd.warm import (level_rows, prior_rows, straight_line_prior, warm_hold_reference, warm_init_reference, warm_tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DDIM5 = [20, 15, 10, 5, 0]      # ddim_set_timesteps(5) at T = 25


# ------------------------------------------------------------------------------------------------ warm_tables
def test_tables_ddim_level_between_two_timesteps():
    """T = 25, K = 5: level 12 lies between 15 and 10 -> the row starts at t = 10, iteration 2; the job starts there too."""
    t = warm_tables([12], DDIM5, T=25)
    assert t["J"] == 2 and t["j0"].tolist() == [0] and t["t_row"].tolist() == [10] and t["n_hold"] == 0
    assert t["j0"].dtype == np.int32 and t["t_row"].dtype == np.int32


def test_tables_level_zero_and_level_top():
    """level 0: the last iteration alone (n' = 1).  level T - 1 = 24: the largest timestep not above it is 20, iteration 0 -- the whole
    DDIM job; on DDPM (T = 25) it is iteration 0 at t = 24."""
    t = warm_tables([0, 0], DDIM5, T=25)
    assert t["J"] == 4 and t["j0"].tolist() == [0, 0] and t["t_row"].tolist() == [0, 0] and t["n_hold"] == 0
    t = warm_tables([24], DDIM5, T=25)
    assert t["J"] == 0 and t["t_row"].tolist() == [20]
    ddpm = list(range(24, -1, -1))
    t = warm_tables([24, 0, 7], ddpm, T=25)
    assert t["J"] == 0 and t["j0"].tolist() == [0, 24, 17] and t["t_row"].tolist() == [24, 0, 7] and t["n_hold"] == 24


def test_tables_mixed_levels_of_the_gpu_tests():
    t = warm_tables([None, 12, 5], DDIM5, T=25)
    assert t["J"] == 0 and t["j0"].tolist() == [0, 2, 3] and t["t_row"].tolist() == [-1, 10, 5] and t["n_hold"] == 3
    t = warm_tables([None, 1, 0], [2, 1, 0], T=3)
    assert t["J"] == 0 and t["j0"].tolist() == [0, 1, 2] and t["t_row"].tolist() == [-1, 1, 0] and t["n_hold"] == 2
    t = warm_tables([12, 5], DDIM5, T=25)      # no None row: the job starts at the earliest row
    assert t["J"] == 2 and t["j0"].tolist() == [0, 1] and t["n_hold"] == 1


def test_tables_with_steps_without_noise():
    """n_diffusion_steps_without_noise = 2 at T = 3: the list is [2, 1, 0, 0, 0]; level 0 starts at the FIRST 0 (iteration 2) and runs all three."""
    steps = [max(i, 0) for i in reversed(range(-2, 3))]
    assert steps == [2, 1, 0, 0, 0]
    t = warm_tables([0], steps, T=3)
    assert t["J"] == 2 and t["j0"].tolist() == [0] and t["t_row"].tolist() == [0]
    t = warm_tables([1, 0], steps, T=3)
    assert t["J"] == 1 and t["j0"].tolist() == [0, 1] and t["n_hold"] == 1


def test_tables_start_override():
    """start= fixes J whatever this shard's rows are: start 20 -> J = 0 and the rows hold; start 12 -> J = 2.  A start below a row's is an error."""
    t = warm_tables([5, 12], DDIM5, start=20, T=25)
    assert t["J"] == 0 and t["j0"].tolist() == [3, 2] and t["n_hold"] == 3
    t = warm_tables([5, 12], DDIM5, start=12, T=25)
    assert t["J"] == 2 and t["j0"].tolist() == [1, 0]
    with pytest.raises(ValueError, match="start"):
        warm_tables([5, 12], DDIM5, start=5, T=25)
    with pytest.raises(ValueError, match="start"):
        warm_tables([None, 5], DDIM5, start=12, T=25)


def test_tables_refuse_bad_levels():
    for bad in ([25], [-1], [3.5]):
        with pytest.raises(ValueError):
            warm_tables(bad, DDIM5, T=25)
    with pytest.raises(ValueError):
        warm_tables([], DDIM5, T=25)
    with pytest.raises(ValueError):
        warm_tables([3], [20, 15, 10], T=25)      # a list that does not end at 0


# ------------------------------------------------------------------------------------------------ the references
def test_init_and_hold_references():
    rng = np.random.default_rng(0)
    noise = rng.standard_normal((3, 8, 4)).astype(np.float32)
    noise[0, 0, 0] = -0.0
    prior = rng.standard_normal((3, 8, 4)).astype(np.float32)
    prior[0] = np.nan      # a row without a prior is never read
    sa, s1a = np.linspace(1, 0.1, 25).astype(np.float32), np.linspace(0.05, 0.99, 25).astype(np.float32)
    x = warm_init_reference(noise, prior, [-1, 10, 0], sa, s1a)
    assert x.dtype == np.float32 and np.array_equal(x[0].view(np.uint32), noise[0].view(np.uint32))
    want = (sa[10] * prior[1]).astype(np.float32) + (s1a[10] * noise[1]).astype(np.float32)
    assert np.array_equal(x[1], want)
    x64 = warm_init_reference(noise, np.nan_to_num(prior), [-1, 10, 0], sa, s1a, dtype=np.float64)
    assert x64.dtype == np.float64 and np.abs(x64[1:] - x[1:]).max() < 1e-6
    cur = rng.standard_normal((3, 8, 4)).astype(np.float32)
    held = warm_hold_reference(cur, x, [0, 2, 3], 2)
    assert np.array_equal(held[:2], cur[:2]) and np.array_equal(held[2], x[2]) and held is not cur
    assert np.array_equal(warm_hold_reference(cur, x, [0, 2, 3], 3), cur)


def test_straight_line_prior_and_prior_rows():
    a, b = np.array([-0.8, -0.8, 0, 0], np.float32), np.array([0.8, 0.4, 0, 0], np.float32)
    p = straight_line_prior(a, b, 9)
    assert p.shape == (9, 4) and p.dtype == np.float32
    assert np.allclose(p[:, 0], np.linspace(-0.8, 0.8, 9)) and np.allclose(p[:, 1], np.linspace(-0.8, 0.4, 9))
    assert np.allclose(p[:, 2], 1.6 / 8) and np.allclose(p[:, 3], 1.2 / 8)      # velocity channels: the constant finite difference
    assert np.allclose(np.diff(p[:, :2], axis=0), p[:-1, 2:])
    p6 = straight_line_prior(np.arange(5.0), np.arange(5.0) + 1, 5, n_pos=2)      # a fifth channel is interpolated
    assert np.allclose(p6[:, 4], np.linspace(4, 5, 5)) and np.allclose(p6[:, 2:4], 0.25)
    one = np.arange(32, dtype=np.float32).reshape(8, 4)
    assert prior_rows(one, [2, 3]).shape == (5, 8, 4) and np.array_equal(prior_rows(one[None], [2, 3])[4], one)
    per = np.stack([one, one + 100])
    rows = prior_rows(per, [2, 3])
    assert rows.shape == (5, 8, 4) and np.array_equal(rows[1], one) and np.array_equal(rows[2], one + 100)
    rows = prior_rows([one, np.stack([one + 1, one + 2, one + 3])], [2, 3])
    assert np.array_equal(rows[0], one) and np.array_equal(rows[4], one + 3)
    full = np.zeros((5, 8, 4), np.float32)
    assert prior_rows(full, [2, 3]) is not None and prior_rows(full, [2, 3]).shape == (5, 8, 4)
    t = prior_rows(torch.from_numpy(per), [1, 2])
    assert torch.is_tensor(t) and tuple(t.shape) == (3, 8, 4) and torch.equal(t[2], torch.from_numpy(one + 100))
    with pytest.raises(ValueError):
        prior_rows(np.zeros((4, 8, 4), np.float32), [2, 3])
    assert level_rows(7, [2, 1]) == [7, 7, 7] and level_rows([None, 3], [2, 1]) == [None, None, 3]
    assert level_rows([1, None, 3], [2, 1]) == [1, None, 3]
    with pytest.raises(ValueError):
        level_rows([1, 2, 3, 4], [2, 1])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_warm_start_layout_matches_header():
    """The ctypes mirror of ramp_warm_start has the size and the field offsets the C compiler gives the header's struct."""
    cls = _lib.RampWarmStart
    body = 'printf("%zu", sizeof(ramp_warm_start));' + "".join(f'printf(" %zu", offsetof(ramp_warm_start, {f}));' for f, _ in cls._fields_)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf("\\n");return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert C.sizeof(cls) == 48


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_warm", 24), ("ramp_warm_init", 10), ("ramp_warm_hold", 9)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_warm"][1][2] == C.POINTER(_lib.RampWarmStart)
    from ramp_amd import build
    assert "warm.hip" in build.SOURCES and build.EXTRA_FLAGS["warm.hip"] == ["-ffp-contract=off"]


def test_host_refusals_of_the_ops():
    """ramp_warm_init / ramp_warm_hold refuse on the host before any device call (the pointers are never dereferenced)."""
    lib = _lib.load()
    f, i = (C.c_float * 4)(), (C.c_int32 * 4)()
    fp, ip = C.cast(f, _lib.c_f32p), C.cast(i, _lib.c_i32p)
    for call, who in ((lambda: lib.ramp_warm_init(0x1000, 0x1000, None, fp, fp, ip, 2, 8, 4, None), "ramp_warm_init"),
                      (lambda: lib.ramp_warm_init(0x1000, 0x1000, 0x1000, fp, fp, ip, 2, 3, 3, None), "ramp_warm_init"),
                      (lambda: lib.ramp_warm_init(0x1000, 0x1000, 0x1000, fp, fp, ip, 0, 8, 4, None), "ramp_warm_init"),
                      (lambda: lib.ramp_warm_hold(0x1000, None, None, ip, 0, 2, 8, 4, None), "ramp_warm_hold"),
                      (lambda: lib.ramp_warm_hold(0x1000, None, 0x1000, ip, 0, 2, 3, 3, None), "ramp_warm_hold")):
        rc = call()
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and who in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ the Python layer's host checks
def host_model(sampler="ddim"):
    from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
    return StaticGaussianDiffusionModel(model=TemporalUnetInference(n_support_points=8, state_dim=4), n_diffusion_steps=25,
                                        predict_epsilon=True, sampler=sampler)


def test_warm_job_resolves_and_refuses_on_the_host():
    dm = host_model()
    prior = np.zeros((3, 8, 4), np.float32)
    w = dm._warm_job(dict(prior=prior, level=[None, 12, 5]), 3, DDIM5)
    assert w["J"] == 0 and w["j0"].tolist() == [0, 2, 3] and w["has"].tolist() == [0, 1, 1] and tuple(w["prior"].shape) == (3, 8, 4)
    assert np.array_equal(w["sa"][1:], dm.sqrt_alphas_cumprod.numpy()[[10, 5]])
    assert np.array_equal(w["s1a"][1:], dm.sqrt_one_minus_alphas_cumprod.numpy()[[10, 5]])
    assert dm._warm_job(w, 3, DDIM5) is w and dm._warm_job(None, 3, DDIM5) is None
    w = dm._warm_job(dict(prior=prior[0], level=7), 3, DDIM5)      # (H, S) for all rows, one level
    assert w["J"] == 3 and w["n_hold"] == 0 and tuple(w["prior"].shape) == (3, 8, 4)
    for bad in (dict(prior=prior, level=25), dict(prior=prior, level=[-1, 0, 0]), dict(prior=prior, level=[1, 2]),
                dict(prior=prior[:2], level=3), dict(prior=np.zeros((3, 8, 6), np.float32), level=3),
                dict(prior=np.full((3, 8, 4), np.nan, np.float32), level=3), dict(prior=np.full((3, 8, 4), np.inf, np.float32), level=[None, None, 0]),
                dict(prior=prior, level=[5, 12, 12], start=5), dict(prior=prior, level=3, speed=1), dict(prior=prior), dict(level=3)):
        with pytest.raises(ValueError):
            dm._warm_job(bad, 3, DDIM5)
    nan_free_row = np.zeros((3, 8, 4), np.float32)
    nan_free_row[0] = np.nan      # a non-finite prior of a row WITHOUT a level is never read
    assert dm._warm_job(dict(prior=nan_free_row, level=[None, 7, 7]), 3, DDIM5)["n_hold"] == 3
    with pytest.raises(TypeError):
        dm._warm_job([prior, 3], 3, DDIM5)


def test_dynamic_model_and_custom_step_functions_refuse():
    from ramp_amd.models import DynamicGaussianDiffusionModel, TemporalUnetInference
    dyn = DynamicGaussianDiffusionModel(model=TemporalUnetInference(n_support_points=8, state_dim=4), n_diffusion_steps=25, predict_epsilon=True)
    with pytest.raises(NotImplementedError, match="warm_start"):
        dyn.conditional_sample({}, batch_size=1, warm_start=dict(prior=np.zeros((8, 4), np.float32), level=3))
    with pytest.raises(NotImplementedError, match="warm_start"):
        dyn._warm_job(dict(prior=np.zeros((8, 4), np.float32), level=3), 1, DDIM5)
    ws = dict(prior=np.zeros((8, 4), np.float32), level=3)
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="warm_start"):
            host_model(sampler).conditional_sample({}, batch_size=1, sample_fn=lambda *a, **k: None, warm_start=ws)


# ------------------------------------------------------------------------------------------------ the free-running test's inputs
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_free_running_inputs_satisfy_their_conditions(kind):
    """The jobs of test_gpu_warm.py's free-running test, on the CPU: the float32 oracle stays within a quarter of the bar (1e-4 of max |x|
    of the float64 chain), the float64 final states of the rows with a prior differ from the cold chain of the same noise by >= 100 x the
    bar, and in the float64 chain the held rows equal x_init in every block up to j0."""
    bar, d32, moved = R.chain_conditions(kind)
    print(f"warm {kind}: bar {bar:.2e}, float32 oracle {d32:.2e}, warm vs cold {moved:.2e}")
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    c = R.oracle_chains(kind)
    for b, j0 in enumerate(R.CHAIN_J0[kind]):
        for j in range(j0 + 1):
            assert np.array_equal(c["w64"][j][b], c["w64"][0][b]), (b, j)
        assert not np.array_equal(c["w64"][j0 + 1][b], c["w64"][0][b]), b
    assert np.array_equal(c["w64"][:, 0], c["c64"][:, 0])      # the row without a prior is the cold chain's
