"""The references and case tables of tests/scene_ref.py, checked on the CPU: the three restatements on inputs small enough to compute
by hand, the properties the attention regimes promise (in float64, never against a kernel), the float32 floor of every stage case, and
for every whole-encoder case the condition on its inputs -- the float32 oracle within LATENT_F32_CAP of the float64 one -- with
tests/torch_scene_encoders.py as the second opinion at the new shapes."""
import os

import numpy as np
import pytest
import torch

import scene_ref as R
from util import GOLDEN


# ---- the restatements on hand-computable inputs ---------------------------------------------------------------------------------------
def test_attention_restatement_by_hand():
    dh, E = 16, 64
    qkv = np.zeros((2, 3 * E), np.float32)
    qkv[:, 2 * E:] = np.arange(2 * E, dtype=np.float32).reshape(2, E)
    o = R.attn_ref64(qkv, dh)                                   # q = 0: both probabilities 1/2
    assert np.array_equal(o, np.tile(qkv[:, 2 * E:].astype(np.float64).mean(0), (2, 1)))
    # head 1 only: q . k = 4 ln 3 for key 0, 0 for key 1 -> logits ln 3, 0 -> P = (3/4, 1/4)
    qkv[0, dh] = 4.0; qkv[0, E + dh] = np.log(3.0); qkv[1, dh] = 4.0
    o = R.attn_ref64(qkv, dh)
    v = qkv[:, 2 * E:].astype(np.float64)
    p0 = np.exp(np.float64(np.float32(np.log(3.0)))) / (1.0 + np.exp(np.float64(np.float32(np.log(3.0)))))
    assert np.allclose(o[0, dh:2 * dh], p0 * v[0, dh:2 * dh] + (1 - p0) * v[1, dh:2 * dh], rtol=1e-14) and abs(p0 - 0.75) < 1e-7
    assert np.array_equal(o[:, :dh], np.tile(v[:, :dh].mean(0), (2, 1)))           # the other heads stay flat
    assert R.rel(R.attn_fp32(qkv, dh), o) < 1e-6
    one = R.make_attention_case("gauss", 1, 64)                 # one token attends to itself
    assert np.array_equal(R.attn_ref64(one, 64), one[:, 512:].astype(np.float64))


def test_attention_tiles_by_hand():
    t = R.attention_tiles(R.RAGGED)                             # 7 | 150 | 64 | 1 | 65 rows from 0, 7, 157, 221, 222
    assert t.dtype == np.int32
    assert t.tolist() == [[0, 7, 0], [7, 150, 0], [7, 150, 64], [7, 150, 128], [157, 64, 0], [221, 1, 0], [222, 65, 0], [222, 65, 64]]


def test_colreduce_restatement_by_hand():
    x = np.array([[1, -8], [3, -2], [-10, -4], [5, -6], [7, -7]], np.float32)
    first = R.csr([1, 3, 1])
    assert first.tolist() == [0, 1, 4, 5]
    for f in (R.colreduce_ref64, R.colreduce_fp32):
        assert np.array_equal(f(x, first, 1), [[1, -8], [5, -2], [7, -7]])          # an all-negative column keeps its true maximum
        assert np.array_equal(f(x, first, 0)[[0, 2]], [[1, -8], [7, -7]])           # seglen 1: the row itself
    assert np.allclose(R.colreduce_ref64(x, first, 0)[1], [-2.0 / 3.0, -4.0], rtol=1e-15, atol=0)
    assert np.allclose(R.colreduce_fp32(x, first, 0)[1], [-2.0 / 3.0, -4.0], rtol=2e-7, atol=0)
    assert R.colreduce_fp32(x, first, 0).dtype == np.float32 and R.colreduce_ref64(x, first, 0).dtype == np.float64


def test_prep_restatement_by_hand():
    cloud = np.array([[[0, 0], [2, 0], [0, 4], [2, 4]], [[1, 1], [1, 1], [1, 1], [1, 1]]], np.float32)
    for f in (R.prep_ref64, R.prep_fp32):
        c, m = f(cloud)
        assert np.array_equal(c, [[1, 2], [1, 1]]) and np.array_equal(m, [2, 0])
    c, m = R.prep_fp32(R.IDENTICAL_EXACT)                        # exactly representable identical points: maxd is exactly 0
    assert np.array_equal(c, R.IDENTICAL_EXACT[:, 0]) and m[0] == 0.0
    one = R.make_prep_case(5, 1)                                 # Np = 1: the centre is the point
    assert np.array_equal(R.prep_fp32(one)[0], one[:, 0]) and not R.prep_fp32(one)[1].any()


# ---- the regimes' properties (float64) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", R.DHS)
def test_regime_properties(dh):
    for T in R.LENGTHS:
        if T >= 16:
            mp = float(R.probs_ref64(R.attention_case("sharp", T, dh)["qkv"], dh).max(-1).mean())
            assert mp >= R.SHARP_MEAN_MAX_P, ("sharp", T, dh, mp)
        for regime, last in (("late_max", True), ("early_max", False)):
            s = R.logits_ref64(R.attention_case(regime, T, dh)["qkv"], dh)
            d = np.diff(s, axis=-1)
            assert T == 1 or bool(((d > 0.2) if last else (d < -0.2)).all()), (regime, T, dh)       # the running maximum moves at every key
            assert bool((s.argmax(-1) == (T - 1 if last else 0)).all())
            if last and T > R.TILE:
                assert (T - 1) // R.TILE == (T + R.TILE - 1) // R.TILE - 1                           # ... and lands in the last tile
        s = R.logits_ref64(R.attention_case("equal_large", T, dh)["qkv"], dh)
        assert 45.0 < float(s.min()) and float(s.max()) < 75.0
        assert float((s.max(-1) - s.min(-1)).max()) < 1e-3                  # equal to float32 input rounding; the kernels see them exactly equal
        c = R.attention_case("flat", T, dh)
        assert np.allclose(c["o"], np.tile(c["qkv"][:, 2 * R.HEADS * dh:].astype(np.float64).mean(0), (T, 1)), rtol=1e-13, atol=1e-15)
        assert not R.attention_case("zero_v", T, dh)["o"].any() and not R.attention_case("zero_v", T, dh)["o32"].any()
    for T in R.lengths_of("onehot_across_tiles"):
        assert T > R.TILE
        p = R.probs_ref64(R.attention_case("onehot_across_tiles", T, dh)["qkv"], dh)
        win = p.argmax(-1)                                                  # (4, T)
        assert bool((win == R.onehot_target(T)[None]).all())
        assert bool((win // R.TILE != np.arange(T)[None] // R.TILE).all()), (T, dh)
        assert float(p.max(-1).min()) > 0.9


# ---- float32 floors of the stage cases ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", R.DHS)
def test_attention_floors(dh):
    for regime in R.REGIMES:
        for T in R.lengths_of(regime):
            c = R.attention_case(regime, T, dh)
            assert np.isfinite(c["o"]).all() and np.isfinite(c["o32"]).all()
            assert np.isfinite(c["floor"]) and c["floor"] < R.FLOOR_CAP, (regime, T, dh, c["floor"])
            assert R.bar(R.B0["attention"], c["floor"]) <= 4 * R.FLOOR_CAP


def test_colreduce_and_prep_floors():
    for seglen, C, n_seg in R.COLREDUCE_SWEEP:
        first = R.csr([seglen] * n_seg)
        for kind in ("gauss", "negative", "ties"):
            x = R.make_colreduce_case(kind, seglen * n_seg, C, seglen + C + n_seg)
            assert np.array_equal(R.colreduce_fp32(x, first, 1), R.colreduce_ref64(x, first, 1))     # a maximum involves no rounding
            fl = R.rel(R.colreduce_fp32(x, first, 0), R.colreduce_ref64(x, first, 0))
            assert np.isfinite(fl) and fl < R.FLOOR_CAP, (seglen, C, n_seg, kind, fl)
            if kind == "negative":
                assert float(R.colreduce_ref64(x, first, 1).max()) < -0.5
            if kind == "ties" and seglen >= 63:
                top = R.colreduce_ref64(x, first, 1)
                assert bool(((x[:seglen].astype(np.float64) == top[0]).sum(0) >= 2).all())          # every column's maximum is tied
    for No, Np in R.PREP_SWEEP:
        cloud = R.make_prep_case(No, Np)
        fc, fm = R.prep_errors(R.prep_fp32(cloud), R.prep_ref64(cloud), cloud)
        assert fc < R.FLOOR_CAP and fm < R.FLOOR_CAP, (No, Np, fc, fm)
    boxes = R.latent_cloud(False, 5, 64)                                    # make_cloud snaps points onto faces: the maximum is tied
    c, m = R.prep_ref64(boxes)
    assert bool(((np.abs(boxes.astype(np.float64) - c[:, None]).max(-1) > m[:, None] - 1e-6).sum(1) >= 2).all())


# ---- whole-encoder cases: the condition on the inputs, and the second opinion ------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_models():
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.unet import load_numpy_state_dict
    out = {}

    def get(o3, sharp):
        if (o3, sharp) not in out:
            m = TemporalUnetInference(n_support_points=48, state_dim=6 if o3 else 4, obstacle_3d=o3)
            out[(o3, sharp)] = load_numpy_state_dict(m, R.state_dict(o3, sharp)).eval()
        return out[(o3, sharp)]
    return get


@pytest.mark.parametrize("name", list(R.LATENT_CASES))
def test_latent_case_is_well_conditioned_in_float32(name, torch_models):
    """rel(oracle float32, oracle float64) < LATENT_F32_CAP = half the latent bar: a condition on the case, so that the bar
    max(5e-6, 4 floor) of the GPU test stays within 2 x the project's 5e-6.  The torch restatement in float32 meets the same cap."""
    import torch_scene_encoders as tse
    c = R.latent_case(name)
    assert np.isfinite(c["lat"]).all() and c["lat"].shape == ((256,) if c["o3"] else (320,))
    print(f"{name}: rel(oracle float32, float64) = {c['floor']:.2e}")
    assert c["floor"] < R.LATENT_F32_CAP, (name, c["floor"])
    enc = torch_models(c["o3"], c["sharp"]).scene_encoder
    with torch.no_grad():
        lat = (tse.encode_3d if c["o3"] else tse.encode_2d)(enc, torch.from_numpy(np.array(c["cloud"]))[None])[0].numpy()
    e = R.rel(lat, c["lat"])
    print(f"{name}: rel(torch float32, float64) = {e:.2e}")
    assert e < R.LATENT_F32_CAP, (name, e)


def test_sharp_weights_sharpen_and_the_excluded_input_is_ill_conditioned():
    sd, sharp = R.state_dict(False), R.state_dict(False, True)
    k = "scene_encoder.set_transformers.1.2.attn.qkv.weight"
    assert np.array_equal(sharp[k], sd[k] * np.float32(R.SHARP_GAIN)) and sharp is not sd
    assert all(np.array_equal(sharp[n], sd[n]) for n in sd if not n.endswith(".attn.qkv.weight"))
    assert not np.array_equal(R.latent_case("2d_sharp_3x43")["lat"], R.latent_case("2d_3x43")["lat"])
    # the tiny obstacle is well conditioned whatever the order of the centre's sum (a kernel adds in another order than numpy)
    l64 = R.latent_case("2d_tiny_obstacle")["lat"]
    for seed in range(4):
        cloud = R._tiny_obstacle(np.random.default_rng(seed).permutation(43))
        e = R.rel(R.oracle(False, False, np.float32).encode_scene(cloud), l64)           # (a set encoder: float64 does not see the order)
        assert R.rel(R.oracle(False, False, np.float64).encode_scene(cloud), l64) < 1e-12 and e < R.LATENT_F32_CAP, (seed, e)
    # the excluded input: float32 itself is far from float64 there (an ulp of the mean over 1e-8), which is why it is no accuracy case
    cloud = R.identical_inexact_cloud()
    assert np.array_equal(cloud[1], np.tile(cloud[1, :1], (16, 1)))
    l64 = R.oracle(False, False, np.float64).encode_scene(cloud)
    l32 = R.oracle(False, False, np.float32).encode_scene(cloud)
    assert np.isfinite(l32).all() and R.rel(l32, l64) > 100 * R.LATENT_F32_CAP


# ---- the reference's own latents at the edge shapes --------------------------------------------------------------------------------------
def test_oracle_against_reference_fixtures_at_edge_shapes():
    path = os.path.join(GOLDEN, "scene_latents_edges.npz")
    g = np.load(path)
    names = ["2d_1x7", "2d_5x13", "2d_1x65", "3d_1x1", "3d_65x2"]
    assert sorted(k[3:] for k in g.files if k.startswith("lat")) == sorted(names)
    for n in names:
        c = R.latent_case(n)
        assert np.array_equal(g["cloud" + n], c["cloud"])                   # the fixture was captured on this very cloud
        e32, e64 = R.rel(c["lat32"], g["lat" + n]), R.rel(c["lat"], g["lat" + n])
        print(f"{n}: oracle float32 vs reference {e32:.2e}, float64 vs reference {e64:.2e}")
        assert e32 < 5e-6 and e64 < 5e-6, (n, e32, e64)
