"""Host side of the composed job (any number of obstacle sets per trajectory, many scenes per job): the tables of
``build_compose_tables``, its refusals, the struct layout and the declared / bound / exported symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ramp_amd import _lib
from ramp_amd.scenes import MAX_ROWS_PER_TRAJ, build_compose_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HK = [[0, 47]]


def test_layout_padding_and_weights_of_a_ragged_job():
    """set_counts (2, 3, 1), n_samples (3, 1, 2): latents in job order [s0k0 s0k1 | s1k0 s1k1 s1k2 | s2k0 | zero], n_rp = 4, padding rows read
    the zero latent (index 6) with weight 0, the last row of every trajectory is the unconditional one."""
    w = [[1.5, 1.0], [1.5, 1.0, 1.5], [3.0]]
    t = build_compose_tables((2, 3, 1), (3, 1, 2), HK * 3, w)
    assert t["n_rp"] == 4
    assert t["traj_scene"].dtype == np.int32 and t["traj_scene"].tolist() == [0, 0, 0, 1, 2, 2]
    assert t["counts"].tolist() == [3, 1, 2] and t["first"].tolist() == [0, 3, 4] and t["set_first"].tolist() == [0, 2, 5, 6]
    rv = t["row_variant"]
    assert rv.dtype == np.int32 and rv.shape == (24,) and rv.flags.c_contiguous
    assert rv.reshape(6, 4).tolist() == [[0, 1, 6, 6]] * 3 + [[2, 3, 4, 6]] + [[5, 6, 6, 6]] * 2
    rw = t["row_weight"]
    assert rw.dtype == np.float32 and rw.shape == (6, 4) and rw.flags.c_contiguous
    assert rw.tolist() == [[1.5, 1.0, 0.0, -1.5]] * 3 + [[1.5, 1.0, 1.5, -3.0]] + [[3.0, 0.0, 0.0, -2.0]] * 2
    assert np.allclose(rw.sum(1), 1.0)                      # e = u + sum_k w_k (c_k - u): the row weights sum to one
    # the other forms of `weights`
    one = build_compose_tables((2, 3, 1), 1, HK * 3, 2.0)["row_weight"]
    assert one.tolist() == [[2.0, 2.0, 0.0, -3.0], [2.0, 2.0, 2.0, -5.0], [2.0, 0.0, 0.0, -1.0]]
    flat = build_compose_tables((2, 3, 1), 1, HK * 3, [1.5, 1.0, 0.5])["row_weight"]
    assert flat.tolist() == [[1.5, 1.0, 0.0, -1.5], [1.5, 1.0, 0.5, -2.0], [1.5, 0.0, 0.0, -0.5]]
    none = build_compose_tables((2, 1), 1, HK * 2)["row_weight"]
    assert none.tolist() == [[1.0, 1.0, -1.0], [1.0, 0.0, 0.0]]
    # seven sets: the most the engine takes
    t7 = build_compose_tables((7,), 2, HK, 0.5)
    assert t7["n_rp"] == MAX_ROWS_PER_TRAJ == 8 and t7["row_variant"].reshape(2, 8).tolist() == [list(range(8))] * 2
    assert t7["row_weight"][0].tolist() == [0.5] * 7 + [-2.5]


@pytest.mark.parametrize("w", [(2.0, 2.0), (5.0, 5.0), (0.3, 0.1)])
def test_two_sets_get_the_weights_of_the_existing_compose_job(w):
    """The engine's two-set job weighs its rows (float(w1), float(w2), float(1.0 - w1 - w2)), the difference taken in double
    (engine.hip, comb_weights); one set with 1 + w is classifier-free guidance at w: (float(1 + w), float(-w))."""
    rw = build_compose_tables((2,), 1, HK, list(w))["row_weight"][0]
    assert rw.tolist() == [np.float32(w[0]), np.float32(w[1]), np.float32(1.0 - w[0] - w[1])]
    cfg = build_compose_tables((1,), 1, HK, 1.0 + w[0])["row_weight"][0]
    assert cfg.tolist() == [np.float32(1.0 + w[0]), np.float32(-w[0])]


@pytest.mark.parametrize("kw, msg", [
    (dict(set_counts=(), n_samples=1, hard_keys=[]), "no scenes"),
    (dict(set_counts=(2, 0), n_samples=1, hard_keys=HK * 2), "at least one"),
    (dict(set_counts=(8,), n_samples=1, hard_keys=HK), "at most 8"),
    (dict(set_counts=(2, 3), n_samples=1, hard_keys=HK * 2, weights=[1.0, 2.0]), "one weight per set"),
    (dict(set_counts=(2, 3), n_samples=1, hard_keys=HK * 2, weights=[[1.0, 2.0], [1.0, 2.0]]), "2 weights for 3 obstacle sets"),
    (dict(set_counts=(2, 3), n_samples=1, hard_keys=HK * 2, weights=[[1.0, 2.0]]), "1 lists for 2 scenes"),
    (dict(set_counts=(2,), n_samples=1, hard_keys=HK, weights=[1.0, float("nan")]), "finite"),
    (dict(set_counts=(2,), n_samples=1, hard_keys=HK, weights=float("inf")), "finite"),
    (dict(set_counts=(2,), n_samples=1, hard_keys=HK, weights=[1e39, 1.0]), "finite"),
    (dict(set_counts=(2, 2), n_samples=1, hard_keys=[[0, 47], [0, 46]]), "same waypoints"),
    (dict(set_counts=(2, 2), n_samples=1, hard_keys=HK), "hard_conds has 1 entries"),
    (dict(set_counts=(2, 2), n_samples=(1, 0), hard_keys=HK * 2), "at least one"),
    (dict(set_counts=(2, 2), n_samples=-3, hard_keys=HK * 2), "at least one"),
    (dict(set_counts=(2, 2), n_samples=(1,), hard_keys=HK * 2), "n_samples has 1 entries"),
])
def test_refusals_carry_a_message(kw, msg):
    with pytest.raises(ValueError, match=msg):
        build_compose_tables(**kw)


def test_guidance_rows_layout_matches_the_header():
    """{int32 n_rp, int32 reserved, pointer}: 16 bytes; RAMP_MAX_ROWS_PER_TRAJ is 8 in the header, the binding and the tables."""
    assert C.sizeof(_lib.RampGuidanceRows) == 16
    assert _lib.RampGuidanceRows.n_rp.offset == 0 and _lib.RampGuidanceRows.reserved.offset == 4 and _lib.RampGuidanceRows.row_weight.offset == 8
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    body = re.search(r"typedef struct ramp_guidance_rows \{(.*?)\} ramp_guidance_rows;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\*?\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.RampGuidanceRows._fields_]
    assert int(re.search(r"#define RAMP_MAX_ROWS_PER_TRAJ (\d+)", hdr).group(1)) == _lib.MAX_ROWS_PER_TRAJ == MAX_ROWS_PER_TRAJ == 8


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_composed", 8), ("ramp_cfg_mean_rows", 16)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_composed"][1][2] == C.POINTER(_lib.RampGuidanceRows)


def test_model_classes_expose_the_composed_entry():
    from ramp_amd.models import DynamicGaussianDiffusionModel, GaussianDiffusionModel3d, StaticGaussianDiffusionModel
    assert callable(StaticGaussianDiffusionModel.run_inference_composed) and callable(GaussianDiffusionModel3d.run_inference_composed)
    assert StaticGaussianDiffusionModel._default_compose[0] == 2.0 and GaussianDiffusionModel3d._default_compose[0] == 5.0
    assert not DynamicGaussianDiffusionModel._scenes_supported      # run_inference_composed refuses the dynamic planner by this flag
