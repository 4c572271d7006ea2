"""Many scenes in one job, the host side: the table builder of ``run_inference_scenes`` against hand-written expectations,
its refusals, and the new entry points in the header and the ctypes prototypes.  Runs without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ramp_amd import _lib
from ramp_amd.scenes import build_scene_tables, scene_slices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ramp_set_scenes", "ramp_sample_scenes", "ramp_apf_scenes")


def test_tables_for_ragged_samples_and_clouds_of_different_sizes():
    """Three scenes with 2 / 1 / 3 samples and clouds of 6 x 64, 16 x 64 and 5 points."""
    t = build_scene_tables([384, 1024, 5], [2, 1, 3], [[0, 47]] * 3)
    assert t["traj_scene"].tolist() == [0, 0, 1, 2, 2, 2]
    # rows [conditional, unconditional] per trajectory: the scene's latent, then the shared zero latent (index n_scenes = 3)
    assert t["row_variant"].tolist() == [0, 3, 0, 3, 1, 3, 2, 3, 2, 3, 2, 3]
    assert t["cloud_offset"].tolist() == [0, 384, 1408, 1413]
    assert t["counts"].tolist() == [2, 1, 3] and t["first"].tolist() == [0, 2, 3]
    assert all(t[k].dtype == np.int32 for k in t)
    assert scene_slices(t["counts"]) == [slice(0, 2), slice(2, 3), slice(3, 6)]


def test_one_count_serves_every_scene():
    t = build_scene_tables([10, 20], 4, [[0, -1], [0, -1]])
    assert t["traj_scene"].tolist() == [0] * 4 + [1] * 4
    assert t["row_variant"].tolist() == [0, 2] * 4 + [1, 2] * 4
    assert t["cloud_offset"].tolist() == [0, 10, 30]


def test_1024_scenes_need_1025_variants():
    t = build_scene_tables([64] * 1024, 4, [[0, 47]] * 1024)
    assert t["row_variant"].max() == 1024 and t["row_variant"].size == 2 * 4096
    assert np.array_equal(t["row_variant"][0::2], np.repeat(np.arange(1024), 4))
    assert t["cloud_offset"][-1] == 64 * 1024


@pytest.mark.parametrize("args,what", [
    (([], 1, []), "no scenes"),
    (([384, 0], 1, [[0], [0]]), "empty cloud"),
    (([384, 1024], [2], [[0], [0]]), "n_samples has 1 entries"),
    (([384, 1024], [2, 0], [[0], [0]]), "at least one"),
    (([384, 1024], 2, [[0, 47], [0, 46]]), "same waypoints"),
    (([384, 1024], 2, [[0, 47], [47, 0]]), "same waypoints"),
    (([384, 1024], 2, [[0, 47]]), "hard_conds has 1 entries"),
])
def test_refusals(args, what):
    with pytest.raises(ValueError, match=what):
        build_scene_tables(*args)


def test_compose_is_refused():
    with pytest.raises(ValueError, match="compose"):
        build_scene_tables([384], 1, [[0]], compose=True)
    with pytest.raises(ValueError, match="n_rp"):
        build_scene_tables([384], 1, [[0]], n_rp=3)


def test_new_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h"), encoding="utf-8").read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.PROTOTYPES, name
    # every new declaration names the reference call it stands for
    for name in NEW_SYMBOLS:
        at = hdr.index("int %s(" % name)
        doc = hdr[hdr.rindex(";\n/*", 0, at) if name != "ramp_set_scenes" else hdr.rindex("\n\n/*", 0, at):at]      # the comment block in front of it
        assert "inference_static.py" in doc and len(doc) < 2500, name
    assert "typedef struct ramp_scene_batch" in hdr
    # prototypes: (ctx, latents, n_variants, row_variant_host, n_rows, stream)
    res, args = _lib.PROTOTYPES["ramp_set_scenes"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int32, _lib.c_i32p, C.c_int32, C.c_void_p]
    res, args = _lib.PROTOTYPES["ramp_sample_scenes"]
    assert args[1] == C.POINTER(_lib.RampSampleParams) and args[2] == C.POINTER(_lib.RampSceneBatch) and len(args) == 7
    res, args = _lib.PROTOTYPES["ramp_apf_scenes"]
    assert args[4] == C.POINTER(_lib.RampApfParams) and args[5] == C.POINTER(_lib.RampSceneBatch) and len(args) == 7


def test_scene_batch_layout_matches_the_header():
    """{int32 n_scenes, int32 reserved, 3 pointers}: 32 bytes; the existing parameter structs keep their size."""
    assert C.sizeof(_lib.RampSceneBatch) == 32
    assert _lib.RampSceneBatch.traj_scene.offset == 8 and _lib.RampSceneBatch.cloud_offset_host.offset == 24
    assert C.sizeof(_lib.RampApfParams) == 48
    assert _lib.RampSampleParams.apf.offset + 48 <= _lib.RampSampleParams.use_graph.offset


def test_model_classes_expose_the_multi_scene_entry():
    from ramp_amd.models import DynamicGaussianDiffusionModel, GaussianDiffusionModel3d, StaticGaussianDiffusionModel, TemporalUnetInference
    assert callable(StaticGaussianDiffusionModel.run_inference_scenes) and StaticGaussianDiffusionModel._scenes_supported
    assert callable(GaussianDiffusionModel3d.run_inference_scenes) and GaussianDiffusionModel3d._scenes_supported
    assert not DynamicGaussianDiffusionModel._scenes_supported
    assert callable(TemporalUnetInference.set_scenes)
