"""The scene encoders' kernels (scene.hip) against float64 at ragged and edge shapes: the three stages that look across tokens one
launch at a time through the ramp_op_scene_* entries (attention, column reduce, 2-D prep; single-scene and segmented forms), and the
whole encoders against oracle.ramp_oracle's float64 encoders.  References, case tables and bars: tests/scene_ref.py (checked on the
CPU by tests/test_scene_ref_host.py); a bar is max(b0, 4 x the float32 CPU evaluation's error), never derived from a kernel's output.

Every measured error is printed with its floor and bar; with RAMP_ACCURACY_LOG set the same lines are appended to that file
(profiles/scene_encoder_accuracy.txt is one such run).

One input is NOT an accuracy case (scene_ref.identical_inexact_cloud): an obstacle of identical points at coordinates float32 cannot
represent.  The float32 mean is an ulp off the point, the normalisation divides by 1e-8, and the float32 oracle itself is 2.3e-2 away
from float64; only a finite latent is asserted there."""
import os

import numpy as np
import pytest
import torch

import scene_ref as R
from ramp_amd import _lib
from util import GOLDEN, build_unet, dev, rel

pytestmark = pytest.mark.gpu

NAN = float("nan")


def record(what, err, floor, bar_):
    line = f"{what:44s} err {err:.3e}  floor {floor:.3e}  bar {bar_:.3e}  err/bar {err / bar_:.3f}"
    print(line)
    path = os.environ.get("RAMP_ACCURACY_LOG")
    if path:
        with open(path, "a", encoding="utf-8") as fh:
            fh.write(line + "\n")
    return err < bar_


def call(name, *args):
    """(rc, message) of a ramp_op_scene_* entry on the current stream, synchronised."""
    lib = _lib.load()
    rc = getattr(lib, name)(*args, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, (lib.ramp_last_error() or b"").decode() if rc else ""


def ok(name, *args):
    rc, msg = call(name, *args)
    assert rc == 0, (name, rc, msg)


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def attention(qkv, T, dh):
    """o (T, E) of ramp_op_scene_attention on a device qkv; the three rows behind T of the NaN-filled output must stay NaN."""
    o = nans(T + 3, R.HEADS * dh)
    ok("ramp_op_scene_attention", _lib.ptr(qkv), _lib.ptr(o), T, R.HEADS, dh, dh ** -0.5)
    assert bool(torch.isnan(o[T:]).all()), "rows beyond T were written"
    return o[:T]


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("dh", R.DHS)
def test_attention_against_float64(dh, regime):
    good = True
    for T in R.lengths_of(regime):
        c = R.attention_case(regime, T, dh)
        got = attention(dev(c["qkv"]), T, dh).cpu().numpy()
        assert np.isfinite(got).all(), (regime, T, dh)
        if regime == "zero_v":
            assert not got.any(), (T, dh)                                   # exact zeros
            continue
        b = R.bar(R.B0["attention"], c["floor"])
        good &= record(f"attention {regime} T={T} dh={dh}", rel(got, c["o"]), c["floor"], b)
        if regime == "flat":                                                # q = 0: the column mean of v, for every query
            mean = np.tile(c["qkv"][:, 2 * R.HEADS * dh:].astype(np.float64).mean(0), (T, 1))
            assert rel(got, mean) < b, (T, dh, rel(got, mean), b)
    assert good


@pytest.mark.parametrize("regime", ["gauss", "sharp", "late_max", "equal_large"])
@pytest.mark.parametrize("dh", R.DHS)
def test_segmented_attention_on_the_ragged_table(dh, regime):
    """Scenes of 7, 150, 64, 1 and 65 rows in one launch: each against float64, and bit for bit the single kernel on that scene alone."""
    cat, parts = R.ragged_attention_case(regime, dh)
    tiles = R.attention_tiles(R.RAGGED)
    qkv = dev(cat)
    n = cat.shape[0]
    o = nans(n + 2, R.HEADS * dh)
    ok("ramp_op_scene_attention_seg", _lib.ptr(qkv), _lib.ptr(o), _lib.ptr(i32(tiles)), len(tiles), R.HEADS, dh, dh ** -0.5)
    assert bool(torch.isnan(o[n:]).all()) and bool(torch.isfinite(o[:n]).all())
    good, base = True, 0
    for c in parts:
        T = c["T"]
        mine = o[base:base + T]
        good &= record(f"attention_seg {regime} scene T={T} dh={dh}", rel(mine.cpu().numpy(), c["o"]), c["floor"],
                       R.bar(R.B0["attention"], c["floor"]))
        alone = attention(qkv[base:base + T].clone(), T, dh)
        assert torch.equal(mine, alone), (regime, T, dh, float((mine - alone).abs().max()))
        base += T
    assert good


# ---- column reduce --------------------------------------------------------------------------------------------------------------------
def colreduce(x, n_seg, seglen, mode):
    C = x.shape[1]
    out = nans(n_seg + 1, C)
    ok("ramp_op_scene_colreduce", _lib.ptr(x), _lib.ptr(out), n_seg, seglen, C, mode)
    assert bool(torch.isnan(out[n_seg:]).all())
    return out[:n_seg]


def colreduce_seg(x, first, mode, ldo=None):
    C = x.shape[1]
    ldo = ldo or C
    n_seg = len(first) - 1
    out = nans(n_seg + 1, ldo)
    ok("ramp_op_scene_colreduce_seg", _lib.ptr(x), _lib.ptr(out), _lib.ptr(i32(first)), n_seg, C, ldo, mode)
    assert bool(torch.isnan(out[n_seg:]).all()) and bool(torch.isnan(out[:, C:]).all()), "the gap columns / rows beyond n_seg were written"
    return out[:n_seg, :C]


@pytest.mark.parametrize("mode", [0, 1], ids=["mean", "max"])
def test_colreduce_against_float64(mode):
    good = True
    for seglen, C, n_seg in R.COLREDUCE_SWEEP:
        first = R.csr([seglen] * n_seg)
        for kind in ("gauss", "negative", "ties"):
            x = R.make_colreduce_case(kind, seglen * n_seg, C, seglen + C + n_seg)
            xd = dev(x)
            got = colreduce(xd, n_seg, seglen, mode)
            assert torch.equal(colreduce_seg(xd, first, mode), got), (seglen, C, n_seg, kind)          # the segmented form: the same bits
            ref = R.colreduce_ref64(x, first, mode)
            if mode:
                assert np.array_equal(got.cpu().numpy().astype(np.float64), ref), (seglen, C, n_seg, kind)   # a maximum involves no rounding
            else:
                fl = rel(R.colreduce_fp32(x, first, 0), ref)
                good &= record(f"colreduce mean {kind} {n_seg}x{seglen}x{C}", rel(got.cpu().numpy(), ref), fl, R.stage_bar(fl))
    assert good


def test_colreduce_max_of_negative_columns_and_ties():
    for seglen in (1, 65):
        x = R.make_colreduce_case("negative", 3 * seglen, 256, 5)
        got = colreduce(dev(x), 3, seglen, 1).cpu().numpy()
        assert np.array_equal(got, x.reshape(3, seglen, 256).max(1)) and float(got.max()) < -0.5        # not the 0 a wrong start value gives
    x = R.make_colreduce_case("ties", 3 * 65, 64, 6)
    got = colreduce(dev(x), 3, 65, 1).cpu().numpy()
    assert np.array_equal(got, x.reshape(3, 65, 64).max(1)) and bool((got == 1.0).all())


@pytest.mark.parametrize("C", [64, 256])
def test_colreduce_segmented_ragged_with_a_row_stride(C):
    """Segments of 1, 65, 2, 1000 and 64 rows into rows of stride C + 32: against float64, the gap columns stay NaN, and every segment has
    the bits of the single form on it alone."""
    first = R.csr(R.COLREDUCE_RAGGED)
    x = R.make_colreduce_case("gauss", int(first[-1]), C, 7 + C)
    xd = dev(x)
    good = True
    for mode in (0, 1):
        got = colreduce_seg(xd, first, mode, ldo=C + 32)
        ref = R.colreduce_ref64(x, first, mode)
        if mode:
            assert np.array_equal(got.cpu().numpy().astype(np.float64), ref)
        else:
            fl = rel(R.colreduce_fp32(x, first, 0), ref)
            good &= record(f"colreduce_seg mean ragged C={C} ldo={C + 32}", rel(got.cpu().numpy(), ref), fl, R.stage_bar(fl))
        for s, n in enumerate(R.COLREDUCE_RAGGED):
            alone = colreduce(xd[first[s]:first[s + 1]].clone(), 1, n, mode)
            assert torch.equal(got[s:s + 1], alone), (C, mode, s)
    assert good


# ---- 2-D prep -------------------------------------------------------------------------------------------------------------------------
def prep(cloud):
    No, Np = cloud.shape[0], cloud.shape[1]
    c, m = nans(No + 1, 2), nans(No + 1)
    ok("ramp_op_scene_enc2d_prep", _lib.ptr(cloud), No, Np, _lib.ptr(c), _lib.ptr(m))
    assert bool(torch.isnan(c[No:]).all()) and bool(torch.isnan(m[No:]).all())
    return c[:No], m[:No]


def prep_seg(points, obstacle_first):
    No = len(obstacle_first) - 1
    c, m = nans(No + 1, 2), nans(No + 1)
    ok("ramp_op_scene_enc2d_prep_seg", _lib.ptr(points), _lib.ptr(i32(obstacle_first)), No, _lib.ptr(c), _lib.ptr(m))
    assert bool(torch.isnan(c[No:]).all()) and bool(torch.isnan(m[No:]).all())
    return c[:No], m[:No]


def check_prep(what, cloud):
    cd = dev(cloud)
    c, m = prep(cd)
    No, Np = cloud.shape[:2]
    cs, ms = prep_seg(cd.reshape(-1, 2), np.arange(No + 1) * Np)
    assert torch.equal(cs, c) and torch.equal(ms, m), what                  # the segmented form: the same bits
    ref = R.prep_ref64(cloud)
    fc, fm = R.prep_errors(R.prep_fp32(cloud), ref, cloud)
    ec, em = R.prep_errors((c.cpu().numpy(), m.cpu().numpy()), ref, cloud)
    good = record(f"prep centre {what}", ec, fc, R.stage_bar(fc))
    return record(f"prep maxd {what}", em, fm, R.stage_bar(fm)) and good, (c, m)


def test_prep_against_float64():
    good, singles = True, []
    for No, Np in R.PREP_SWEEP:
        cloud = R.make_prep_case(No, Np)
        g, (c, m) = check_prep(f"{No}x{Np}", cloud)
        good &= g
        singles.append((cloud, c, m))
        if Np == 1:                                                         # the centre is the point and maxd is 0, exactly
            assert np.array_equal(c.cpu().numpy(), cloud[:, 0]) and not bool(m.any())
    assert good
    # all of them as one ragged table: obstacles of 1 .. 130 points side by side, the bits of the single calls
    of = R.csr([cl.shape[1] for cl, _, _ in singles for _ in range(cl.shape[0])])
    c, m = prep_seg(dev(np.concatenate([cl.reshape(-1, 2) for cl, _, _ in singles])), of)
    assert torch.equal(c, torch.cat([s[1] for s in singles])) and torch.equal(m, torch.cat([s[2] for s in singles]))


def test_prep_identical_points_and_tied_maxima():
    c, m = prep(dev(R.IDENTICAL_EXACT))                                     # 16 x (0.375, -0.625): sum and mean are exact in float32
    assert float(m[0]) == 0.0 and np.array_equal(c.cpu().numpy(), R.IDENTICAL_EXACT[:, 0])
    for no, n in ((5, 64), (3, 50)):                                        # points snapped onto box faces: the maximum is tied across lanes
        g, _ = check_prep(f"boxes {no}x{n}", R.latent_cloud(False, no, n))
        assert g


# ---- whole encoders -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    """(3-D?, sharp weights?) -> model, built once per module."""
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.unet import load_numpy_state_dict
    made = {}

    def get(o3, sharp=False):
        if (o3, sharp) not in made:
            if sharp:
                m = TemporalUnetInference(n_support_points=48, state_dim=6 if o3 else 4, obstacle_3d=o3, max_rows=4)
                made[(o3, sharp)] = load_numpy_state_dict(m, R.state_dict(o3, True)).eval().to("cuda")
            else:
                made[(o3, sharp)] = build_unet(6 if o3 else 4, 48, o3, max_rows=4)
        return made[(o3, sharp)]
    return get


@pytest.mark.parametrize("name", list(R.LATENT_CASES))
def test_latent_against_the_float64_oracle(name, models):
    c = R.latent_case(name)
    lat = models(c["o3"], c["sharp"]).encode_scene(dev(c["cloud"])).cpu().numpy()
    assert lat.shape == (1,) + c["lat"].shape and np.isfinite(lat).all()
    assert record(f"latent {name}", rel(lat[0], c["lat"]), c["floor"], R.bar(R.LATENT_B0, c["floor"]))


def test_identical_inexact_points_give_a_finite_latent(models):
    """No accuracy case (see the module docstring): float32 itself is 2.3e-2 from float64 on this input."""
    lat = models(False).encode_scene(dev(R.identical_inexact_cloud()))
    assert lat.shape == (1, 320) and bool(torch.isfinite(lat).all())


def test_reference_fixtures_keep_their_bar(models):
    """The reference's own latents, at the four original shapes and at the edge shapes, at the existing 5e-6."""
    good = True
    for file, names in (("scene_latents.npz", ["2d_6x64", "2d_16x64", "3d_5x50", "3d_20x200"]),
                        ("scene_latents_edges.npz", ["2d_1x7", "2d_5x13", "2d_1x65", "3d_1x1", "3d_65x2"])):
        g = np.load(f"{GOLDEN}/{file}")
        for n in names:
            lat = models(n.startswith("3d")).encode_scene(dev(g["cloud" + n])).cpu().numpy()[0]
            e = rel(lat, g["lat" + n])
            print(f"latent {n} vs the reference's: {e:.3e}")
            good &= e < 5e-6
    assert good


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_grid_stride_loops_take_a_second_sweep_inside_one_pass(which, models):
    """The elementwise kernels sweep 4096 blocks x 256 elements at a time.  2-D: five copies of the 16x64 cloud and the other 2-D shapes
    in ONE pass are 5987 tokens, whose (T, 256) activations need a second sweep; 3-D: (21, 200), (20, 200) and the small shapes are 8910
    points x 256 channels, three sweeps.  Every row has the bits of encode_scene alone, whose accuracy the tests above pin."""
    o3 = which == "3d"
    m = models(o3)
    if o3:
        shapes = [(21, 200), (20, 200)] + [s for s in R.LATENT_3D if s[1] != 200]
    else:
        shapes = [(16, 64)] * 5 + [s for s in R.LATENT_2D if s != (16, 64)]
    clouds = [dev(R.latent_cloud(o3, no, n)) for no, n in shapes]
    points = sum(no * n for no, n in shapes)
    assert points == (8910 if o3 else 5987) and points > 4096              # T x 256 elements against 4096 blocks x 256
    lat = m.encode_scenes(clouds, max_points=16384)
    assert m.last_encode_passes == 1 and lat.shape == (len(clouds), m.context_dim) and bool(torch.isfinite(lat).all())
    alone = {}
    for i, (sh, c) in enumerate(zip(shapes, clouds)):
        if sh not in alone:
            alone[sh] = m.encode_scene(c).clone()
        assert torch.equal(lat[i:i + 1], alone[sh]), (which, i, sh, float((lat[i] - alone[sh][0]).abs().max()))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_new_entries_refuse_bad_arguments_before_any_launch():
    x = torch.zeros(64, 3 * 64, device="cuda")
    o = nans(64, 64)
    tab = i32([0, 64, 0])
    first = i32([0, 32, 64])
    p, q, t, f = _lib.ptr(x), _lib.ptr(o), _lib.ptr(tab), _lib.ptr(first)
    bad = {
        "ramp_op_scene_attention": [(None, q, 64, 4, 16, 0.25), (p, None, 64, 4, 16, 0.25), (p, q, 0, 4, 16, 0.25), (p, q, -3, 4, 16, 0.25),
                                    (p, q, 64, 0, 16, 0.25), (p, q, 64, 4, 32, 0.25), (p, q, 64, 4, 0, 0.25)],
        "ramp_op_scene_attention_seg": [(None, q, t, 1, 4, 16, 0.25), (p, None, t, 1, 4, 16, 0.25), (p, q, None, 1, 4, 16, 0.25),
                                        (p, q, t, 0, 4, 16, 0.25), (p, q, t, 1, 0, 16, 0.25), (p, q, t, 1, 4, 48, 0.25)],
        "ramp_op_scene_colreduce": [(None, q, 1, 64, 64, 0), (p, None, 1, 64, 64, 0), (p, q, 0, 64, 64, 0), (p, q, 1, 0, 64, 1),
                                    (p, q, 1, 64, -1, 0), (p, q, 1, 64, 64, 2)],
        "ramp_op_scene_colreduce_seg": [(None, q, f, 2, 64, 64, 0), (p, None, f, 2, 64, 64, 0), (p, q, None, 2, 64, 64, 0),
                                        (p, q, f, 0, 64, 64, 0), (p, q, f, 2, 0, 64, 0), (p, q, f, 2, 64, 32, 1), (p, q, f, 2, 64, 64, -1)],
        "ramp_op_scene_enc2d_prep": [(None, 2, 32, q, q), (p, 2, 32, None, q), (p, 2, 32, q, None), (p, 0, 32, q, q), (p, 2, 0, q, q)],
        "ramp_op_scene_enc2d_prep_seg": [(None, f, 2, q, q), (p, None, 2, q, q), (p, f, 2, None, q), (p, f, 2, q, None), (p, f, 0, q, q)],
    }
    for name, cases in bad.items():
        for args in cases:
            rc, msg = call(name, *args)
            assert rc != 0 and name + ":" in msg, (name, args, rc, msg)
            assert bool(torch.isnan(o).all()), (name, args)
    ok("ramp_op_scene_attention", p, q, 64, 4, 16, 0.25)                    # and an unbroken call passes: zeros in, zeros out
    assert not bool(o.any())
