"""CPU-only checks of the many-episode replanning job's host side: the episode tables, the per-episode random streams of the
pursuit-evasion clouds, and the layout of the new C structs."""
import ctypes as C
import os

import numpy as np
import pytest

from ramp_amd import _lib
from ramp_amd.apf_dynamic import generate_box_points, generate_sphere_points
from ramp_amd.scenes import build_episode_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVEN, ODD, CFG = [0, 0, 1, 1], [0, 1, 1, 0], [0, 1]      # DynamicGaussianDiffusionModel._row_pattern: even / odd count, 'intended'


def test_episode_tables_reference_compat_pairs_rows_by_the_episodes_own_count():
    """Counts [6, 5, 1]: an even, an odd and a one-candidate episode.  Every episode's rows carry the pattern of ITS count from ITS first
    row -- the odd pattern of episode 1 starts at network row 12, not wherever a pattern over the whole batch would be by then."""
    t = build_episode_tables([6, 5, 1], [EVEN, ODD, ODD])
    assert t["traj_first"].dtype == np.int32 and t["traj_first"].tolist() == [0, 6, 11, 12]
    assert t["row_episode"].dtype == np.int32 and t["row_episode"].tolist() == [0] * 6 + [1] * 5 + [2]
    rv = t["row_variant"]
    assert rv.dtype == np.int32 and rv.shape == (24,)
    E = 3                                                   # the shared all-zero latent
    assert rv[:12].tolist() == [0, 0, E, E] * 3
    assert rv[12:22].tolist() == [1, E, E, 1, 1, E, E, 1, 1, E]
    assert rv[22:].tolist() == [2, E]
    # an episode's slice is what a single-episode job of that count reads (pattern cycled from row 0), with its own latent index
    for e, (n, pat) in enumerate([(6, EVEN), (5, ODD), (1, ODD)]):
        own = [e if pat[r % len(pat)] == 0 else E for r in range(2 * n)]
        assert rv[2 * t["traj_first"][e]:2 * t["traj_first"][e + 1]].tolist() == own


def test_episode_tables_intended_guidance_is_cond_uncond_like_the_scene_tables():
    from ramp_amd.scenes import build_scene_tables
    t = build_episode_tables([6, 5, 1], [CFG] * 3)
    ref = build_scene_tables([1, 1, 1], [6, 5, 1], [[0, 47]] * 3)
    assert np.array_equal(t["row_variant"], ref["row_variant"])
    assert np.array_equal(t["row_episode"], ref["traj_scene"])


def test_episode_tables_refuse_bad_input():
    with pytest.raises(ValueError):
        build_episode_tables([], [])
    with pytest.raises(ValueError):
        build_episode_tables([6, 0], [EVEN, EVEN])
    with pytest.raises(ValueError):
        build_episode_tables([6, -1], [EVEN, ODD])
    with pytest.raises(ValueError):
        build_episode_tables([6, 5], [EVEN])
    with pytest.raises(ValueError):
        build_episode_tables([6], [[]])
    with pytest.raises(ValueError):
        build_episode_tables([6], [[0, 2]])


@pytest.mark.parametrize("draw", [lambda **kw: generate_sphere_points(np.array([0.3, -0.2]), 0.1, 64, **kw),
                                  lambda **kw: generate_box_points((0.1, 0.55), (0.16, 0.16), 64, **kw)], ids=["sphere", "box"])
def test_cloud_generators_draw_from_the_stream_they_are_given(draw):
    """rng = RandomState(7) gives, bit for bit, what the global stream gives after seed(7); without rng the global stream is used as before."""
    np.random.seed(7)
    want = draw()
    state = np.random.get_state()[1].copy()
    got = draw(rng=np.random.RandomState(7))
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(np.random.get_state()[1], state), "a private stream must leave the global one alone"
    np.random.seed(7)
    assert np.array_equal(draw(), want)
    assert not np.array_equal(draw(rng=np.random.RandomState(8)), want)


def test_episode_struct_layout_matches_header():
    """The ctypes mirrors of ramp_episode_state / ramp_episode_batch have the sizes and field offsets the C compiler gives them; the
    state record is 32 bytes, the device record's size."""
    import subprocess, tempfile
    pairs = [("ramp_episode_state", _lib.RampEpisodeState), ("ramp_episode_batch", _lib.RampEpisodeBatch)]
    body = []
    for cname, cls in pairs:
        body.append(f'printf("%zu", sizeof({cname}));')
        for fname, _ in cls._fields_:
            body.append(f'printf(" %zu", offsetof({cname}, {fname}));')
        body.append('printf("\\n");')
    src = '#include "ramp_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){' + "".join(body) + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        lines = subprocess.check_output([os.path.join(d, "s")]).decode().strip().splitlines()
    for (cname, cls), line in zip(pairs, lines):
        got = [int(v) for v in line.split()]
        want = [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
        assert got == want, (cname, got, want)
    assert C.sizeof(_lib.RampEpisodeState) == 32
