"""Encoding many scenes in one call, without a device: the CSR tables (``build_encode_tables``), the declaration and binding of
``ramp_encode_scenes``, the pass planner (csrc/encode_plan.h, driven from a stand-alone sanitized program) and the two job paths
that hand all their scenes to ``encode_scenes`` at once."""
import contextlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import util
from ramp_amd import _lib
from ramp_amd.scenes import build_encode_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S = 48, 4


# ---------------------------------------------------------------------------------------------------------------- tables
def test_build_encode_tables_ragged():
    tab = build_encode_tables([(6, 64), (1, 7), (3, 50)])
    assert tab["scene_first"].dtype == tab["obstacle_first"].dtype == np.int32
    assert tab["scene_first"].tolist() == [0, 6, 7, 10]
    assert tab["obstacle_first"].tolist() == [0, 64, 128, 192, 256, 320, 384, 391, 441, 491, 541]
    one = build_encode_tables([(1, 1)])
    assert one["scene_first"].tolist() == [0, 1] and one["obstacle_first"].tolist() == [0, 1]
    # numpy integers and torch.Size entries are what callers pass
    assert build_encode_tables([torch.zeros(2, 3, 2).shape[:2], (np.int64(1), np.int32(5))])["obstacle_first"].tolist() == [0, 3, 6, 11]


@pytest.mark.parametrize("shapes,named", [
    ([], None),                                   # no scene
    ([(6, 64), (0, 7)], "scene 1"),               # an empty scene
    ([(6, 64), (2, 5), (3, 0)], "scene 2"),       # empty obstacles
    ([(6, 64), (-1, 4)], "scene 1"),
    ([(1, 8), (2, 2 ** 30)], "scene 1"),          # totals beyond 32-bit offsets
    ([(6, 64), (3, 50, 2)], "scene 1"),           # not (n_obstacles, n_points)
])
def test_build_encode_tables_refusals(shapes, named):
    with pytest.raises(ValueError) as e:
        build_encode_tables(shapes)
    if named:
        assert named in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_entry_is_declared_bound_and_wrapped():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    m = re.search(r"int\s+ramp_encode_scenes\s*\(([^;]*)\)\s*;", hdr)
    assert m, "ramp_encode_scenes is not declared in include/ramp_hip.h"
    assert len(m.group(1).split(",")) == 10
    assert re.search(r"#define\s+RAMP_ENCODE_DEFAULT_MAX_POINTS\s+32768\b", hdr)
    res, args = _lib.PROTOTYPES["ramp_encode_scenes"]
    assert len(args) == 10 and args[2] is _lib.c_i32p and args[3] is _lib.c_i32p and args[8] is _lib.c_i32p
    from ramp_amd.models import TemporalUnetInference
    assert callable(getattr(TemporalUnetInference, "encode_scenes"))
    plan_h = open(os.path.join(ROOT, "ramp_amd", "csrc", "encode_plan.h")).read()
    assert not re.search(r'#include\s+[<"][^>"]*hip', plan_h), "the planner header must not include anything from HIP"
    assert re.search(r"ENCODE_DEFAULT_MAX_POINTS\s*=\s*32768\b", plan_h)


# ---------------------------------------------------------------------------------------------------------------- planner
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/encode_plan_probe.cpp against csrc/encode_plan.h under AddressSanitizer + UBSan: a plain program with its own main."""
    exe = str(tmp_path_factory.mktemp("encode_plan") / "encode_plan_probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "ramp_amd", "csrc"), os.path.join(ROOT, "tests", "encode_plan_probe.cpp"), "-o", exe])

    def run(max_points, scene_first, obstacle_first, n_scenes=None):
        n = len(scene_first) - 1 if n_scenes is None else n_scenes
        r = subprocess.run([exe, str(max_points), str(n)] + [str(v) for v in scene_first] + ["--"] + [str(v) for v in obstacle_first],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]            # a sanitizer report ends the program with a non-zero status
        lines = r.stdout.strip().splitlines()
        if lines[0].startswith("refused: "):
            return lines[0][len("refused: "):]
        assert lines[0] == f"ok {len(lines) - 1}"
        return [tuple(int(v) for v in l.split()) for l in lines[1:]]
    return run


def _tables_for_points(points_per_scene, n_points=None):
    """Scenes of the given point totals; a scene of P points is P / n obstacles of n points (n = 64 where it divides, else P)."""
    shapes = []
    for P in points_per_scene:
        n = n_points or (64 if P % 64 == 0 else P)
        shapes.append((P // n, n))
    tab = build_encode_tables(shapes)
    return shapes, tab["scene_first"].tolist(), tab["obstacle_first"].tolist()


def _check_plan(passes, shapes, budget):
    """Every pass is at most `budget` points or a single scene, greedy (the next scene would not have fitted), order kept, all
    scenes covered once, and the ranges / tile counts are the scenes' own."""
    pts = [no * n for no, n in shapes]
    s = o = p = 0
    for k, (s0, s1, o0, o1, p0, p1, pt, ot) in enumerate(passes):
        assert (s0, o0, p0) == (s, o, p) and s1 > s0
        assert o1 - o0 == sum(no for no, _ in shapes[s0:s1]) and p1 - p0 == sum(pts[s0:s1])
        assert p1 - p0 <= budget or s1 - s0 == 1
        if s1 < len(shapes):
            assert p1 - p0 + pts[s1] > budget, "a pass stopped although the next scene fitted"
        assert pt == sum(-(-P // 64) for P in pts[s0:s1]) and ot == sum(-(-no // 64) for no, _ in shapes[s0:s1])
        s, o, p = s1, o1, p1
    assert s == len(shapes)


def test_planner_budget_200(probe):
    shapes, sf, of = _tables_for_points([384, 7, 150, 64, 128, 1024, 13])
    passes = probe(200, sf, of)
    assert [(a[0], a[1]) for a in passes] == [(0, 1), (1, 3), (3, 5), (5, 6), (6, 7)]          # [384] [7 150] [64 128] [1024] [13]
    assert [a[6] for a in passes] == [6, 1 + 3, 1 + 2, 16, 1] and [a[7] for a in passes] == [1, 2, 2, 1, 1]
    _check_plan(passes, shapes, 200)
    # the batch tests/test_gpu_scenes_encode.py encodes with max_points = 200: the same five passes
    shapes, sf, of = _tables_for_points([384, 7, 150, 64, 128, 1024, 65])
    passes = probe(200, sf, of)
    assert len(passes) == 5 and passes[3][:2] == (5, 6) and passes[3][5] - passes[3][4] == 1024
    _check_plan(passes, shapes, 200)


def test_planner_default_budget_single_scene_and_exact_fit(probe):
    shapes, sf, of = _tables_for_points([384, 7, 150, 64, 128, 1024, 13])
    assert probe(0, sf, of) == [(0, 7, 0, sf[-1], 0, of[-1], 6 + 1 + 3 + 1 + 2 + 16 + 1, 7)]              # 0 = default: one pass
    shapes, sf, of = _tables_for_points([32768, 64, 32704])
    passes = probe(0, sf, of)                                                                          # the default is 32768 points
    assert [(a[0], a[1]) for a in passes] == [(0, 1), (1, 3)]
    _check_plan(passes, shapes, 32768)
    assert probe(0, [0, 3], [0, 50, 100, 150]) == [(0, 1, 0, 3, 0, 150, 3, 1)]
    assert probe(1, [0, 3], [0, 50, 100, 150]) == [(0, 1, 0, 3, 0, 150, 3, 1)]                           # a scene over the budget: its own pass
    shapes, sf, of = _tables_for_points([100, 100, 100, 100])
    assert [(a[0], a[1]) for a in probe(200, sf, of)] == [(0, 2), (2, 4)]                               # exactly the budget fits
    # many obstacles in one scene: more than one obstacle tile
    shapes, sf, of = _tables_for_points([130, 3], n_points=1)
    assert probe(0, sf, of) == [(0, 2, 0, 133, 0, 133, 3 + 1, 3 + 1)]


@pytest.mark.parametrize("args,word", [
    ((0, [0], [0], 0), "n_scenes"),                                   # no scene
    ((0, [1, 2], [0, 4, 8]), "scene_first must start at 0"),
    ((0, [0, 2], [3, 4, 8]), "obstacle_first must start at 0"),
    ((0, [0, 2, 2], [0, 4, 8]), "scene 1"),                           # an empty scene
    ((0, [0, 2, 1], [0, 4, 8]), "scene 1"),                           # not monotonic
    ((0, [0, 1, 3], [0, 4, 4, 8]), "scene 1"),                        # an empty obstacle
    ((0, [0, 1, 3], [0, 4, 9, 8]), "scene 1"),                        # obstacle table not monotonic
    ((0, [0, 1, 3], [0, 4, 9, 13]), "scene 1"),                       # obstacles of 5 and 4 points in one scene
    ((-1, [0, 1], [0, 4]), "max_points"),
])
def test_planner_refusals(probe, args, word):
    got = probe(*args)
    assert isinstance(got, str) and word in got, got


# ---------------------------------------------------------------------------------------------------------------- job paths
class _Lib:
    """The C ABI answers 'ok' to everything and keeps the names it was asked for."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


@pytest.fixture
def stub(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    return lib


def _counted(u):
    """Count the calls of u.encode_scenes / u.encode_scene without replacing what they do."""
    n = dict(scenes=0, scene=0)
    many, one = u.encode_scenes, u.encode_scene

    def encode_scenes(clouds, max_points=None):
        n["scenes"] += 1
        n["clouds"] = len(clouds)
        return many(clouds, max_points)

    def encode_scene(cloud):
        n["scene"] += 1
        return one(cloud)

    u.ctx, u.encode_scenes, u.encode_scene = (lambda: None), encode_scenes, encode_scene
    return n


def _hc():
    from ramp_amd import synth
    return {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(S, H).items()}


def test_prepare_scene_job_encodes_all_scenes_in_one_call(stub):
    from ramp_amd import models
    dm = models.StaticGaussianDiffusionModel(model=models.TemporalUnetInference(n_support_points=H, state_dim=S), n_diffusion_steps=25,
                                             predict_epsilon=True, sampler="ddpm", use_apf=True)
    n = _counted(dm.model)
    scenes = [torch.rand(6, 64, 2), torch.rand(1, 7, 2), torch.rand(3, 50, 2)]
    job, hc, B = dm._prepare_scene_job(scenes, [_hc() for _ in scenes], [2, 1, 3])
    assert B == 6 and job["n_scenes"] == 3
    assert (n["scenes"], n["clouds"], n["scene"]) == (1, 3, 0)
    assert stub.calls.count("ramp_encode_scenes") == 1 and "ramp_encode_scene" not in stub.calls
    assert stub.calls.index("ramp_encode_scenes") < stub.calls.index("ramp_set_scenes")
    assert dm.model.cached_scene_latents.shape == (4, dm.model.context_dim)            # three scenes + the unconditional row


def test_run_inference_episodes_encodes_all_episodes_in_one_call(stub):
    """Up to the point where the job's scene table is installed (what follows needs a device): one encode_scenes call over the
    episodes' clouds, no per-scene call."""
    from ramp_amd import models
    dm = models.DynamicGaussianDiffusionModel(model=models.TemporalUnetInference(n_support_points=H, state_dim=S, max_rows=64),
                                              n_diffusion_steps=100, predict_epsilon=True)
    u = dm.model
    n = _counted(u)

    class Installed(Exception):
        pass

    def set_scenes(latents, row_variant):
        n["latents"] = tuple(latents.shape)
        raise Installed()

    u.set_scenes = set_scenes
    clouds = [torch.rand(6, 64, 2), torch.rand(4, 30, 2)]
    contexts = [{"dataset": util.make_fake_pursuit_env()[0]} for _ in clouds]
    with pytest.raises(Installed):
        dm.run_inference_episodes(contexts, [_hc() for _ in clouds], clouds, n_samples=[3, 2])
    assert (n["scenes"], n["clouds"], n["scene"]) == (1, 2, 0) and n["latents"] == (3, u.context_dim)
    assert stub.calls.count("ramp_encode_scenes") == 1 and "ramp_encode_scene" not in stub.calls


def test_encode_scene_4d_is_one_batched_call_and_3d_stays_single(stub):
    from ramp_amd import models
    u = models.TemporalUnetInference(n_support_points=H, state_dim=S)
    u.ctx = lambda: None
    assert u.encode_scene(torch.rand(2, 6, 64, 2)).shape == (2, u.context_dim)
    assert stub.calls == ["ramp_encode_scenes"]
    assert u.encode_scene(torch.rand(6, 64, 2)).shape == (1, u.context_dim)
    assert stub.calls == ["ramp_encode_scenes", "ramp_encode_scene"]
    with pytest.raises(ValueError, match="scene 1"):
        u.encode_scenes([torch.rand(6, 64, 2), torch.rand(6, 64, 3)])
    with pytest.raises(ValueError, match="scene 0"):
        u.encode_scenes([torch.rand(64, 2)])
