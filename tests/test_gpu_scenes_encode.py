"""All scenes of a batch through the scene encoder in one call (``ramp_encode_scenes`` / ``TemporalUnetInference.encode_scenes``):
the reference's latents inside a batch, and the contract that makes the switch-over of the many-scene jobs safe -- every row has the
BITS that ``ramp_encode_scene`` gives for that scene alone, whatever else is in the batch, in whatever order, under whatever pass
budget, and whatever ran before."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramp_amd import _lib, synth
from ramp_amd.scenes import build_encode_tables
from util import GOLDEN, build_unet, dev, rel

pytestmark = pytest.mark.gpu

# the smallest shapes (No, Np) that cover: a partial query tile and a partial key tile next to another scene's tokens, a scene shorter
# than one 64-token tile, an exact tile, several tiles, differing points per obstacle, one-token attention.  In this (shuffled) order
# the 2-D scenes hold 384, 7, 150, 64, 128, 1024, 65 points: tests/test_scenes_encode_host.py plans the same sizes.
SHAPES_2D = [(6, 64), (1, 7), (3, 50), (1, 64), (2, 64), (16, 64), (5, 13)]
SHAPES_3D = [(5, 50), (1, 1), (20, 200), (2, 1), (3, 64), (1, 5)]


@pytest.fixture(scope="module")
def m2():
    return build_unet(4, 48, False, max_rows=4)


@pytest.fixture(scope="module")
def m3():
    return build_unet(6, 48, True, max_rows=4)


def _clouds(shapes, D, seed0):
    return [dev(synth.make_cloud(no, n, D, seed=seed0 + i)) for i, (no, n) in enumerate(shapes)]


@pytest.fixture(scope="module")
def batch2(m2):
    """(clouds, per-scene latents from ramp_encode_scene alone): computed once, shared, never modified."""
    clouds = _clouds(SHAPES_2D, 2, 700)
    return clouds, [m2.encode_scene(c).clone() for c in clouds]


@pytest.fixture(scope="module")
def batch3(m3):
    clouds = _clouds(SHAPES_3D, 3, 800)
    return clouds, [m3.encode_scene(c).clone() for c in clouds]


def _raw(m, clouds, out, max_points=0, tables=None, n_scenes=None, point_dim=None):
    """ramp_encode_scenes through the raw ABI into `out`; returns (rc, passes, message)."""
    D = clouds[0].shape[2]
    pts = torch.cat([c.reshape(-1, D) for c in clouds]).contiguous()
    tab = tables or build_encode_tables([(c.shape[0], c.shape[1]) for c in clouds])
    of = np.ascontiguousarray(tab["obstacle_first"], dtype=np.int32)
    sf = np.ascontiguousarray(tab["scene_first"], dtype=np.int32)
    n_passes = C.c_int32(-1)
    lib = _lib.load()
    rc = lib.ramp_encode_scenes(m.ctx(), _lib.ptr(pts), of.ctypes.data_as(_lib.c_i32p), sf.ctypes.data_as(_lib.c_i32p),
                                len(clouds) if n_scenes is None else n_scenes, D if point_dim is None else point_dim, max_points,
                                _lib.ptr(out), C.byref(n_passes), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, n_passes.value, (lib.ramp_last_error() or b"").decode()


def test_reference_fixtures_inside_one_batch(m2, m3):
    g = np.load(f"{GOLDEN}/scene_latents.npz")
    lat = m2.encode_scenes([dev(g["cloud2d_6x64"]), dev(g["cloud2d_16x64"]), dev(g["cloud2d_6x64"][::-1].copy())]).cpu().numpy()
    assert lat.shape == (3, 320) and m2.last_encode_passes == 1
    e0, e1 = rel(lat[0], g["lat2d_6x64"]), rel(lat[1], g["lat2d_16x64"])
    print(f"2-D batch vs reference latents: 6x64 {e0:.2e}, 16x64 {e1:.2e}")
    assert e0 < 5e-6 and e1 < 5e-6
    assert not np.array_equal(lat[0], lat[2])                       # the position encodings see the obstacle order
    lat = m3.encode_scenes([dev(g["cloud3d_5x50"]), dev(g["cloud3d_20x200"])]).cpu().numpy()
    e0, e1 = rel(lat[0], g["lat3d_5x50"]), rel(lat[1], g["lat3d_20x200"])
    print(f"3-D batch vs reference latents: 5x50 {e0:.2e}, 20x200 {e1:.2e}")
    assert lat.shape == (2, 256) and e0 < 5e-6 and e1 < 5e-6


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_same_bits_alone_and_inside_the_batch(which, request):
    m = request.getfixturevalue("m2" if which == "2d" else "m3")
    clouds, alone = request.getfixturevalue("batch2" if which == "2d" else "batch3")
    lat = m.encode_scenes(clouds)
    assert lat.shape == (len(clouds), m.context_dim) and m.last_encode_passes == 1 and bool(torch.isfinite(lat).all())
    for i, a in enumerate(alone):
        assert torch.equal(lat[i:i + 1], a), (which, i, tuple(clouds[i].shape), float((lat[i] - a[0]).abs().max()))
    # the 4-D form of encode_scene is the same call
    if which == "2d":
        four = torch.stack([clouds[0], clouds[0].flip(0)])
        assert torch.equal(m.encode_scene(four), torch.cat([alone[0], m.encode_scene(clouds[0].flip(0))]))


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_order_and_duplicates(which, request):
    m = request.getfixturevalue("m2" if which == "2d" else "m3")
    clouds, alone = request.getfixturevalue("batch2" if which == "2d" else "batch3")
    perm = [4, 0, 6, 2, 5, 1, 3] if which == "2d" else [2, 5, 0, 3, 1, 4]
    lat = m.encode_scenes([clouds[i] for i in perm])
    assert torch.equal(lat, torch.cat([alone[i] for i in perm]))
    twice = m.encode_scenes([clouds[2], clouds[1], clouds[2]])
    assert torch.equal(twice[0], twice[2]) and torch.equal(twice, torch.cat([alone[2], alone[1], alone[2]]))


def test_pass_budget_changes_the_passes_not_the_bits(m2, m3, batch2, batch3):
    clouds, alone = batch2
    one = m2.encode_scenes(clouds)
    assert m2.last_encode_passes == 1
    split = m2.encode_scenes(clouds, max_points=200)
    assert m2.last_encode_passes == 5                 # [384] [7 150] [64 128] [1024: over the budget, alone] [65]
    assert torch.equal(split, one) and torch.equal(one, torch.cat(alone))
    assert torch.equal(m2.encode_scenes(clouds, max_points=1), one) and m2.last_encode_passes == len(clouds)
    clouds, alone = batch3                            # points: 250, 1, 4000, 2, 192, 5
    split = m3.encode_scenes(clouds, max_points=256)
    assert m3.last_encode_passes == 3                 # [250 1] [4000] [2 192 5]
    assert torch.equal(split, torch.cat(alone))


def test_nothing_else_is_written_and_scratch_growth_is_harmless():
    """A fresh context, so that the scratch buffer really grows between the calls."""
    m = build_unet(4, 48, False, max_rows=4)
    small = _clouds([(1, 7), (2, 20)], 2, 900)
    large = _clouds([(16, 64), (6, 64), (3, 50)], 2, 910)
    single = small[1]
    lat_single = m.encode_scene(single).clone()                     # the smallest scratch first
    out = torch.full((len(small) + 3, 320), float("nan"), device="cuda")
    rc, passes, msg = _raw(m, small, out)
    assert rc == 0 and passes == 1, msg
    assert bool(torch.isfinite(out[:2]).all()) and bool(torch.isnan(out[2:]).all())          # rows beyond n_scenes untouched
    lat_small = out[:2].clone()
    assert torch.equal(lat_small[1:2], lat_single)
    lat_large = m.encode_scenes(large)                              # grows the scratch and the table buffer
    assert torch.equal(m.encode_scenes(small), lat_small)
    assert torch.equal(m.encode_scene(single), lat_single)
    assert torch.equal(m.encode_scenes(large), lat_large)
    # the middle of a larger buffer: rows before and after stay as they were
    out = torch.full((5, 320), float("nan"), device="cuda")
    rc, _, msg = _raw(m, small, out[2:])
    assert rc == 0, msg
    assert bool(torch.isnan(out[:2]).all()) and bool(torch.isnan(out[4:]).all()) and torch.equal(out[2:4], lat_small)


def test_refusals_through_the_raw_abi(m2, batch2):
    """Host-side argument checks that run before any launch: the output buffer keeps its NaNs."""
    clouds = batch2[0][:3]                                          # (6, 64) (1, 7) (3, 50)
    good = build_encode_tables([(c.shape[0], c.shape[1]) for c in clouds])
    out = torch.full((3, 320), float("nan"), device="cuda")

    def refused(**kw):
        rc, _, msg = _raw(m2, clouds, out, **kw)
        assert rc != 0 and "ramp_encode_scenes" in msg, (rc, msg)
        assert bool(torch.isnan(out).all())
        return msg

    refused(n_scenes=0)
    sf = good["scene_first"].copy(); sf[1], sf[2] = sf[2], sf[1]
    assert "scene 1" in refused(tables=dict(good, scene_first=sf))                      # a non-monotonic scene table
    of = good["obstacle_first"].copy(); of[8] = of[9]
    assert "scene 2" in refused(tables=dict(good, obstacle_first=of))                   # an empty obstacle
    of = good["obstacle_first"].copy(); of[8] += 1
    msg = refused(tables=dict(good, obstacle_first=of))                                 # obstacles of 51 and 49 points in scene 2
    assert "scene 2" in msg and "51" in msg
    sf = good["scene_first"].copy(); sf[0] = 1
    refused(tables=dict(good, scene_first=sf))
    refused(point_dim=3)
    refused(max_points=-5)
    rc, passes, msg = _raw(m2, clouds, out)                                             # and the same arguments, unbroken, pass
    assert rc == 0 and passes == 1 and bool(torch.isfinite(out).all()), msg


def test_run_inference_scenes_equals_the_job_on_per_scene_latents():
    """End to end: a Philox-noise job over three ragged scenes, and the same job with the scenes' latents built by the per-scene
    ``encode_scene`` loop and handed over through ``set_scenes`` (the parent's path, rebuilt here): the same bits."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=8)
    dm = StaticGaussianDiffusionModel(model=u, variance_schedule="exponential", n_diffusion_steps=25, predict_epsilon=True,
                                      use_apf=True, sampler="ddpm", noise_source="philox", noise_seed=21).eval().to("cuda")
    scenes = _clouds([(6, 64), (2, 20), (3, 50)], 2, 950)
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(4, 48).items()}

    def job():
        dm._philox_offset = 0
        x, ts = dm.run_inference_scenes(scenes, [hc] * 3, n_samples=1, horizon=48, noise_std_extra_schedule_fn=lambda t: 0.5)
        return x.clone(), ts.cpu().tolist()

    batched, ts = job()
    assert ts == [0, 1, 2] and batched.shape == (3, 48, 4) and bool(torch.isfinite(batched).all()) and u.last_encode_passes == 1
    calls = []

    def per_scene_loop(clouds, max_points=None):
        calls.append(len(clouds))
        return torch.cat([u.encode_scene(c) for c in clouds])

    u.encode_scenes = per_scene_loop
    try:
        looped, _ = job()
    finally:
        del u.encode_scenes
    assert calls == [3]
    assert torch.equal(batched, looped)
    assert float((batched[0] - batched[1]).abs().max()) > 1e-3          # the scenes' rows do differ
