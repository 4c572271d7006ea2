"""Host side of the stitched windows (``run_inference_stitched`` -> ``ramp_sample_stitched``): layout and table builders with their
refusals, the properties of the numpy statement of the definition, struct layout, the declared / bound / exported symbols, the refusals that
need no device, and the conditions the free-running GPU test asks of its inputs.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import test_gpu_stitch as G
from ramp_amd import _lib
from ramp_amd import stitch as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def uniform(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------ layout and tables
def test_layout_and_its_refusals():
    assert ST.stitch_layout(48, 4, 8) == (40, 168)
    assert ST.stitch_layout(8, 2, 1) == (7, 15) and ST.stitch_layout(8, 3, 4) == (4, 16) and ST.stitch_layout(64, 3, 32) == (32, 128)
    assert ST.stitch_layout(8, 1, 0) == (8, 8) and ST.stitch_layout(8, 1, 99) == (8, 8)      # one window reads no overlap
    for H, W, O in ((8, 2, 0), (8, 2, 5), (8, 3, -1), (48, 2, 25)):
        with pytest.raises(ValueError, match="overlap"):
            ST.stitch_layout(H, W, O)
    with pytest.raises(ValueError, match="n_windows"):
        ST.stitch_layout(8, 0, 2)
    # every long waypoint lies in one or two windows; head and tail of a window are disjoint
    for H, W, O in ((8, 3, 4), (8, 2, 1), (48, 4, 8)):
        st, L = ST.stitch_layout(H, W, O)
        cover = np.zeros(L, int)
        for w in range(W):
            cover[w * st:w * st + H] += 1
        assert cover.min() == 1 and cover.max() == 2 and (cover == 2).sum() == (W - 1) * O and O <= st


def test_blend_weights():
    assert ST.blend_weights(4, 'mean').tolist() == [0.5] * 4 and ST.blend_weights(3, 'left').tolist() == [0.0] * 3
    r = ST.blend_weights(4, 'ramp')
    assert r.dtype == np.float32 and np.array_equal(r, (np.arange(1, 5) / 5.0).astype(np.float32))
    assert ST.blend_weights(0, 'ramp').size == 0
    with pytest.raises(ValueError, match="blend"):
        ST.blend_weights(4, 'cubic')


def test_tables_for_one_scene_and_for_one_per_window():
    t = ST.build_stitch_tables(8, 3, 2, 2, 1, [0, -1, 6, -20])
    assert (t["stride"], t["L"], t["B"]) == (6, 20, 6)
    assert t["traj_scene"].tolist() == [0] * 6 and t["traj_scene"].dtype == np.int32
    assert t["row_variant"].tolist() == [0, 1] * 6 and t["row_variant"].dtype == np.int32      # (the odd row: the shared zero latent)
    assert t["pin_idx"].tolist() == [0, 19, 6, 0] and t["pin_idx"].dtype == np.int32             # negative indices count from L
    t = ST.build_stitch_tables(8, 3, 2, 2, 3, [], cloud_sizes=[10, 3, 7])
    assert t["traj_scene"].tolist() == [0, 1, 2, 0, 1, 2]                                        # row c W + w reads scene w
    assert t["row_variant"].tolist() == [0, 3, 1, 3, 2, 3, 0, 3, 1, 3, 2, 3]
    assert t["cloud_offset"].tolist() == [0, 10, 13, 20] and t["pin_idx"].size == 0
    for bad, msg in ((dict(n_scenes=2), "scenes for 3 windows"), (dict(n_chains=0), "chains"), (dict(pin_keys=[20]), "outside the long trajectory"),
                     (dict(pin_keys=[-21]), "outside the long trajectory"), (dict(overlap=5), "overlap"), (dict(overlap=0), "overlap"),
                     (dict(cloud_sizes=[1, 2]), "cloud sizes"), (dict(pin_keys=list(range(20)) * 4), "at most 64")):
        kw = dict(H=8, n_windows=3, overlap=2, n_chains=2, n_scenes=1)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            ST.build_stitch_tables(**kw)


# ------------------------------------------------------------------------------------------------ the definition's properties
CASES = [(1, 1, 0), (1, 2, 1), (2, 2, 4), (2, 3, 2), (3, 3, 4)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("Cn,W,O", CASES)
def test_reference_properties(Cn, W, O, dtype):
    """stitch_reference is idempotent, leaves its input alone, makes the overlaps bit-equal, writes the pins over the blend (later pins win)
    and touches nothing else; W = 1 is hard conditioning; assemble(split_long(x)) == x and split_long(assemble(stitched)) == stitched."""
    H, S = 8, 4
    st, L = ST.stitch_layout(H, W, O)
    x = uniform((Cn * W, H, S), 7 + Cn + W + O).astype(dtype)
    x0 = x.copy()
    keys = [k for k in (0, 3, st, L - 1, -L) if -L <= k < L]
    vals = uniform((len(keys), Cn, S), 9).astype(dtype)
    pins = {k: vals[i] for i, k in enumerate(keys)}
    for kind in ST.BLEND_KINDS:
        y = ST.stitch_reference(x, W, O, ST.blend_weights(O, kind), pins)
        assert y.dtype == dtype and np.array_equal(x, x0)
        assert np.array_equal(ST.stitch_reference(y, W, O, ST.blend_weights(O, kind), pins), y)
        v = y.reshape(Cn, W, H, S)
        if W > 1:
            assert np.array_equal(v[:, :-1, st:], v[:, 1:, :O])
            assert np.array_equal(v[:, 0, st], pins[st]) and np.array_equal(v[:, 1, 0], pins[st])
        assert np.array_equal(v[:, 0, 0], pins[-L]) and np.array_equal(v[:, W - 1, H - 1], pins[L - 1])
        mask = G.touched_mask(Cn, W, O, S, ST.pin_indices(keys, L))
        assert np.array_equal(y[~mask], x[~mask])
        long = ST.assemble_reference(y, W, O)
        assert long.shape == (Cn, L, S) and np.array_equal(ST.split_long(long, H, W, O), y)
    # the blend itself, element by element, in the array's own precision
    if W > 1:
        a = ST.blend_weights(O, 'ramp')
        y = ST.stitch_reference(x, W, O, a, None).reshape(Cn, W, H, S)
        xv = x.reshape(Cn, W, H, S)
        for k in range(O):
            l, q = xv[0, 0, st + k, 1], xv[0, 1, k, 1]
            assert y[0, 0, st + k, 1] == dtype(l + dtype(dtype(a[k]) * dtype(q - l))) == y[0, 1, k, 1]
        left = ST.stitch_reference(x, W, O, ST.blend_weights(O, 'left'), None).reshape(Cn, W, H, S)
        assert np.array_equal(left[:, 1:, :O], xv[:, :-1, st:]) and np.array_equal(left[:, :-1, st:], xv[:, :-1, st:])
    else:
        from oracle.ramp_oracle import apply_hard_conditioning
        hc = {0: vals[0], 3: vals[1], H - 1: vals[2]}
        assert np.array_equal(ST.stitch_reference(x, 1, 0, [], hc), apply_hard_conditioning(x.copy(), hc))
    z = uniform((Cn, L, S), 11).astype(dtype)
    assert np.array_equal(ST.assemble_reference(ST.split_long(z, H, W, O), W, O), z)
    with pytest.raises(ValueError, match="waypoints"):
        ST.split_long(z[:, :-1], H, W, O)


def test_equal_inputs_come_back_bit_for_bit():
    """q == l returns l itself, whatever alpha: the closing stitch of an iteration only pins."""
    x = uniform((2, 8, 4), 3)
    x[1, :2] = x[0, 6:]
    x[0, 6, 0] = x[1, 0, 0] = np.float32(1e-40)      # a subnormal
    for kind in ST.BLEND_KINDS:
        assert np.array_equal(ST.stitch_reference(x, 2, 2, ST.blend_weights(2, kind), None).view(np.uint32), x.view(np.uint32))


def test_reference_refusals():
    x = uniform((4, 8, 4), 1)
    with pytest.raises(ValueError, match="multiple"):
        ST.stitch_reference(x, 3, 2, ST.blend_weights(2), None)
    with pytest.raises(ValueError, match="blend weights"):
        ST.stitch_reference(x, 2, 2, [0.5], None)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ST.stitch_reference(x, 2, 2, [0.5, bad], None)
    with pytest.raises(ValueError, match="float32 or float64"):
        ST.stitch_reference(x.astype(np.float16), 2, 2, [0.5, 0.5], None)


# ------------------------------------------------------------------------------------------------ the C side
def test_stitch_layout_matches_the_header():
    cls = _lib.RampStitch
    body = 'printf("%zu", sizeof(ramp_stitch));' + "".join(f'printf(" %zu", offsetof(ramp_stitch, {f}));' for f, _ in cls._fields_)
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + body + 'printf(" %d\\n", RAMP_STITCH_MAX_PINS);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).decode().split()]
    assert got[:-1] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_], got
    assert got[-1] == _lib.STITCH_MAX_PINS == 64


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_stitched", 10), ("ramp_stitch_windows", 7), ("ramp_stitch_assemble", 8)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_stitched"][1][2] == C.POINTER(_lib.RampStitch)
    assert _lib.PROTOTYPES["ramp_sample_stitched"][1][3] == C.POINTER(_lib.RampCostGuide)
    from ramp_amd import build
    assert "stitch.hip" in build.SOURCES and build.EXTRA_FLAGS["stitch.hip"] == ["-ffp-contract=off"]


def test_host_refusals_of_the_kernel_level_entries():
    """ramp_stitch_windows / ramp_stitch_assemble refuse on the host before any device call: non-zero, the entry's name in ramp_last_error.
    (The pointers are never dereferenced: every call here is refused.)"""
    lib = _lib.load()
    alpha = (C.c_float * 2)(0.5, 0.5)
    idx = (C.c_int32 * 2)(0, 13)

    def table(**kw):
        st = _lib.RampStitch()
        st.n_windows, st.overlap, st.alpha_host, st.n_pin = 2, 2, C.cast(alpha, _lib.c_f32p), 2
        st.pin_idx_host, st.pin_val = C.cast(idx, _lib.c_i32p), 0x1000
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def windows(st, Cn=2, W=2, H=8, S=4, x=0x1000):
        rc = lib.ramp_stitch_windows(x, Cn, W, H, S, C.byref(st) if st is not None else None, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_stitch_windows" in msg, (rc, msg)
        return msg

    assert "null" in windows(None) and "null" in windows(table(), x=None)
    assert "bad dims" in windows(table(), Cn=0) and "bad dims" in windows(table(), S=0)
    assert "bad dims" in windows(table(), W=0)
    assert "differs" in windows(table(), W=3)
    for bad in (0, 5, -1):
        assert "overlap" in windows(table(overlap=bad))
    for bad in (-0.5, 1.5, float("nan"), float("inf")):
        assert "alpha" in windows(table(alpha_host=C.cast((C.c_float * 2)(0.5, bad), _lib.c_f32p)))
    assert "alpha" in windows(table(alpha_host=None))
    assert "n_pin" in windows(table(n_pin=65)) and "n_pin" in windows(table(n_pin=-1))
    assert "pin table" in windows(table(pin_val=None)) and "pin table" in windows(table(pin_idx_host=None))
    for bad in (14, -1):
        assert "pin index" in windows(table(pin_idx_host=C.cast((C.c_int32 * 2)(0, bad), _lib.c_i32p)))

    def assemble(Cn=2, W=2, H=8, S=4, O=2, x=0x1000, out=0x1000):
        rc = lib.ramp_stitch_assemble(x, Cn, W, H, S, O, out, None)
        msg = lib.ramp_last_error().decode()
        assert rc != 0 and "ramp_stitch_assemble" in msg, (rc, msg)
        return msg

    assert "null" in assemble(x=None) and "null" in assemble(out=None)
    assert "bad dims" in assemble(W=0) and "bad dims" in assemble(H=0)
    assert "overlap" in assemble(O=0) and "overlap" in assemble(O=5)
    # the job entry without a context
    assert lib.ramp_sample_stitched(None, None, None, None, None, None, None, None, None, None) != 0
    assert "ramp_sample_stitched" in lib.ramp_last_error().decode()


def test_python_refusals_before_anything_touches_a_device():
    from ramp_amd import models

    def make(cls="StaticGaussianDiffusionModel", **kw):
        return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=8, state_dim=4), n_diffusion_steps=25,
                                    predict_epsilon=True, **kw)

    scene, hc = torch.zeros(2, 4, 2), {0: torch.zeros(4), -1: torch.zeros(4)}
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        make("DynamicGaussianDiffusionModel").run_inference_stitched(scene, hc, 2, 2)
    with pytest.raises(NotImplementedError, match="compose"):
        make(compose=True).run_inference_stitched(scene, hc, 2, 2)
    with pytest.raises(NotImplementedError, match="mcmc"):
        make().run_inference_stitched(scene, hc, 2, 2, mcmc=dict(kind='ula'))
    with pytest.raises(NotImplementedError, match="resample"):
        make().run_inference_stitched(scene, hc, 2, 2, resample=dict(every=1))

    def my_step(*a, **k):
        raise AssertionError("never called")
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            make(sampler=sampler).run_inference_stitched(scene, hc, 2, 2, sample_fn=my_step)
    dm = make()
    dm.set_noise_shard(0, 8)
    with pytest.raises(NotImplementedError, match="shard"):
        dm.run_inference_stitched(scene, hc, 2, 2)
    dm.set_noise_shard(None)
    for kw, msg in ((dict(overlap=5), "overlap"), (dict(overlap=0), "overlap"), (dict(n_windows=0), "n_windows"), (dict(blend='cubic'), "blend"),
                    (dict(blend=[0.5]), "blend weights"), (dict(blend=[0.5, 2.0]), r"\[0, 1\]"), (dict(hard_conds={14: hc[0]}), "outside the long trajectory"),
                    (dict(scenes=[scene] * 3), "scenes for 2 windows"), (dict(hard_conds={0: torch.zeros(3, 4)}), r"must be \(4,\) or \(1, 4\)")):
        a = dict(scenes=scene, hard_conds=hc, n_windows=2, overlap=2)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            dm.run_inference_stitched(**a)


# ------------------------------------------------------------------------------------------------ the free-running test's inputs
def test_free_running_chain_inputs_satisfy_their_conditions():
    """What tests/test_gpu_stitch.py::test_free_running_stitched_chain asks of its inputs (C = 1, W = 2, O = 2), checked on the CPU for the
    DDPM and the DDIM job: the float32 StitchOracle chain stays within a quarter of the bar (1e-4 of max |x|) of the float64 one, and the
    float64 stitched final state differs from the float64 chain of the same rows and noise without stitching by at least 100 x the bar."""
    for kind in ("ddpm", "ddim"):
        bar, d32, moved = G.chain_conditions(kind)
        print(f"{kind}: bar {bar:.3e}, float32 oracle {d32:.3e}, stitched vs unstitched {moved:.3e}")
        assert d32 <= bar / 4 and moved >= 100 * bar
        c = G.oracle_chains(kind)
        v = c["s64"].reshape(c["s64"].shape[0], 1, 2, 8, 4)
        assert np.array_equal(v[:, :, 0, 6:], v[:, :, 1, :2])      # every state of the oracle chain is consistent
