"""Host-side tables of a job that samples MANY scenes at once (``run_inference_scenes`` -> ``ramp_set_scenes`` +
``ramp_sample_scenes``): the loop over experiment directories of the reference's ``scripts/inference/inference_static.py``
turned into one batch.  Pure numpy, no device: everything here is testable without a GPU."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from ._lib import MAX_ROWS_PER_TRAJ      # RAMP_MAX_ROWS_PER_TRAJ (include/ramp_hip.h); the binding module imports no device code until load()


def build_scene_tables(cloud_sizes: Sequence[int], n_samples: Union[int, Sequence[int]],
                       hard_keys: Sequence[Sequence[int]], n_rp: int = 2, compose: bool = False) -> Dict[str, np.ndarray]:
    """Tables of one multi-scene job.

    cloud_sizes  APF points of each scene's cloud (n_obstacles * n_points), one entry per scene; may differ per scene
    n_samples    trajectories per scene: one int for all, or one count per scene
    hard_keys    per scene, the waypoint indices of its hard-condition dict: every scene must condition the same waypoints
                 in the same order (the job has ONE hard-condition layout, ``hard_val (n_hard, B, S)``)
    n_rp         network rows per trajectory (2: classifier-free guidance)

    Returns int32 arrays: ``traj_scene`` (B) scene of each trajectory, scenes in order, a scene's samples adjacent;
    ``row_variant`` (B * n_rp) latent of each network row -- row ``b * n_rp`` reads its scene's latent ``traj_scene[b]``, row
    ``b * n_rp + 1`` the shared unconditional all-zero latent, index ``n_scenes`` -- ; ``cloud_offset`` (n_scenes + 1) first
    point of each scene in the concatenated cloud; ``counts`` (n_scenes); ``first`` (n_scenes) first trajectory of each scene.
    """
    if compose:
        raise ValueError("a multi-scene job does not support compose=True (three latent variants per scene): out of scope")
    if n_rp != 2:
        raise ValueError("a multi-scene job runs classifier-free guidance rows only (n_rp = 2)")
    n_scenes = len(cloud_sizes)
    if n_scenes == 0:
        raise ValueError("no scenes given")
    sizes = [int(s) for s in cloud_sizes]
    for i, s in enumerate(sizes):
        if s <= 0:
            raise ValueError(f"scene {i} has an empty cloud")
    if isinstance(n_samples, (int, np.integer)):
        counts = [int(n_samples)] * n_scenes
    else:
        counts = [int(c) for c in n_samples]
        if len(counts) != n_scenes:
            raise ValueError(f"n_samples has {len(counts)} entries for {n_scenes} scenes")
    for i, c in enumerate(counts):
        if c <= 0:
            raise ValueError(f"scene {i} asks for {c} samples; every scene needs at least one")
    if len(hard_keys) != n_scenes:
        raise ValueError(f"hard_conds has {len(hard_keys)} entries for {n_scenes} scenes")
    k0 = [int(k) for k in hard_keys[0]]
    for i, ks in enumerate(hard_keys):
        if [int(k) for k in ks] != k0:
            raise ValueError(f"scene {i} conditions waypoints {list(ks)}, scene 0 {k0}: every scene of a job must condition "
                             "the same waypoints in the same order")
    traj_scene = np.repeat(np.arange(n_scenes, dtype=np.int32), counts)
    row_variant = np.empty(traj_scene.size * 2, dtype=np.int32)
    row_variant[0::2] = traj_scene
    row_variant[1::2] = n_scenes
    cloud_offset = np.zeros(n_scenes + 1, dtype=np.int64)
    np.cumsum(sizes, out=cloud_offset[1:])
    if cloud_offset[-1] >= 2 ** 31:
        raise ValueError("the concatenated cloud does not fit 32-bit offsets")
    first = np.zeros(n_scenes, dtype=np.int64)
    first[1:] = np.cumsum(counts)[:-1]
    return {"traj_scene": traj_scene, "row_variant": row_variant, "cloud_offset": cloud_offset.astype(np.int32),
            "counts": np.asarray(counts, dtype=np.int32), "first": first.astype(np.int32)}




def _set_weights(weights, set_counts: Sequence[int]) -> List[List[float]]:
    """The per-scene, per-set guidance weights of ``build_compose_tables`` as doubles."""
    n_scenes, k_max = len(set_counts), max(set_counts)
    if weights is None:
        return [[1.0] * k for k in set_counts]
    if isinstance(weights, (int, float, np.integer, np.floating)):
        return [[float(weights)] * k for k in set_counts]
    ws = list(weights)
    if ws and all(isinstance(w, (int, float, np.integer, np.floating)) for w in ws):
        if len(ws) != k_max:
            raise ValueError(f"weights has {len(ws)} entries; a flat list holds one weight per set, {k_max} (the largest set count) -- "
                             "or give one list per scene")
        return [[float(w) for w in ws[:k]] for k in set_counts]
    if len(ws) != n_scenes:
        raise ValueError(f"weights has {len(ws)} lists for {n_scenes} scenes")
    out = []
    for i, (w, k) in enumerate(zip(ws, set_counts)):
        w = [float(v) for v in np.asarray(w, dtype=np.float64).reshape(-1)]
        if len(w) != k:
            raise ValueError(f"scene {i}: {len(w)} weights for {k} obstacle sets")
        out.append(w)
    return out


def build_compose_tables(set_counts: Sequence[int], n_samples: Union[int, Sequence[int]], hard_keys: Sequence[Sequence[int]],
                         weights=None) -> Dict[str, np.ndarray]:
    """Tables of one COMPOSED job (``run_inference_composed`` -> ``ramp_set_scenes`` + ``ramp_sample_composed``): every scene is a
    composition of ``K_i`` obstacle sets, e = u + sum_k w_k (c_k - u) (the reference's p_mean_variance_compose,
    diffusion_model_static.py:188-229 and diffusion_model_3d.py:163-182, for any number of sets), and many scenes share the job.

    set_counts   obstacle sets of each scene, ``K_i >= 1``; every trajectory gets ``n_rp = max K_i + 1 <= 8`` network rows
    n_samples    trajectories per scene: one int for all, or one count per scene
    hard_keys    per scene, the waypoint indices of its hard-condition dict: the same in every scene, in the same order
    weights      None (every set weighs 1), one number for every set, one list of ``max K_i`` numbers (set k of every scene gets
                 entry k) or one list per scene of ``K_i`` numbers

    The latents are expected in job order -- all sets of scene 0, all sets of scene 1, ... -- followed by ONE all-zero row at index
    ``sum K_i``.  Row ``b * n_rp + k`` of trajectory b (scene i) reads set k of its scene for ``k < K_i``; row ``b * n_rp + n_rp - 1``
    is the unconditional row; the rows in between are PADDING: they read the zero latent and weigh 0.  Padding is how scenes with
    different set counts share a job, and its cost is those rows' compute: a scene with K sets in a job of n_rp rows per trajectory
    pays for ``n_rp - 1 - K`` rows whose result is discarded.
    Weight of set k: ``float32(w_k)``; of the unconditional row: ``float32(1 - w_0 - w_1 - ...)`` with the difference taken in double,
    left to right -- the rule of the engine's two-set job, so two sets with (w1, w2) get exactly that job's weights, and one set with
    ``1 + w`` the weights of classifier-free guidance at w.

    Returns ``traj_scene`` (B) int32, ``row_variant`` (B * n_rp) int32, ``row_weight`` (B, n_rp) float32, ``counts`` (n_scenes) int32,
    ``first`` (n_scenes) int32 first trajectory of each scene, ``set_first`` (n_scenes + 1) int32 first latent of each scene, and
    ``n_rp`` (int)."""
    n_scenes = len(set_counts)
    if n_scenes == 0:
        raise ValueError("no scenes given")
    ks = [int(k) for k in set_counts]
    for i, k in enumerate(ks):
        if k < 1:
            raise ValueError(f"scene {i} has {k} obstacle sets; every scene needs at least one")
    n_rp = max(ks) + 1
    if n_rp > MAX_ROWS_PER_TRAJ:
        raise ValueError(f"a scene has {max(ks)} obstacle sets: {n_rp} network rows per trajectory, the engine takes at most {MAX_ROWS_PER_TRAJ} "
                         f"({MAX_ROWS_PER_TRAJ - 1} sets)")
    if isinstance(n_samples, (int, np.integer)):
        counts = [int(n_samples)] * n_scenes
    else:
        counts = [int(c) for c in n_samples]
        if len(counts) != n_scenes:
            raise ValueError(f"n_samples has {len(counts)} entries for {n_scenes} scenes")
    for i, c in enumerate(counts):
        if c <= 0:
            raise ValueError(f"scene {i} asks for {c} samples; every scene needs at least one")
    if len(hard_keys) != n_scenes:
        raise ValueError(f"hard_conds has {len(hard_keys)} entries for {n_scenes} scenes")
    k0 = [int(k) for k in hard_keys[0]]
    for i, hk in enumerate(hard_keys):
        if [int(k) for k in hk] != k0:
            raise ValueError(f"scene {i} conditions waypoints {list(hk)}, scene 0 {k0}: every scene of a job must condition "
                             "the same waypoints in the same order")
    ws = _set_weights(weights, ks)
    for i, w in enumerate(ws):
        with np.errstate(over="ignore"):
            finite = np.isfinite(np.asarray(w, dtype=np.float64)).all() and np.isfinite(np.asarray(w, dtype=np.float64).astype(np.float32)).all()
        if not finite:
            raise ValueError(f"scene {i}: weights must be finite, got {w}")
    B = int(sum(counts))
    if B * n_rp >= 2 ** 24:
        raise ValueError("the job's network rows exceed the engine's row table (2^24)")
    set_first = np.zeros(n_scenes + 1, dtype=np.int64)
    np.cumsum(ks, out=set_first[1:])
    zero = int(set_first[-1])
    traj_scene = np.repeat(np.arange(n_scenes, dtype=np.int32), counts)
    variant = np.full((n_scenes, n_rp), zero, dtype=np.int32)
    weight = np.zeros((n_scenes, n_rp), dtype=np.float32)
    for i, (k, w) in enumerate(zip(ks, ws)):
        variant[i, :k] = set_first[i] + np.arange(k)
        weight[i, :k] = np.asarray(w, dtype=np.float64).astype(np.float32)      # (finite: checked above)
        u = 1.0
        for v in w:
            u -= v
        weight[i, n_rp - 1] = np.float32(u)
    if not np.isfinite(weight).all():
        raise ValueError("weights must be finite: the unconditional row's weight 1 - sum_k w_k leaves the float32 range")
    first = np.zeros(n_scenes, dtype=np.int64)
    first[1:] = np.cumsum(counts)[:-1]
    return {"traj_scene": traj_scene, "row_variant": np.ascontiguousarray(variant[traj_scene].reshape(-1)),
            "row_weight": np.ascontiguousarray(weight[traj_scene]), "counts": np.asarray(counts, dtype=np.int32),
            "first": first.astype(np.int32), "set_first": set_first.astype(np.int32), "n_rp": n_rp}


def scene_slices(counts: Sequence[int]) -> List[slice]:
    """The rows of each scene in the job's batch (what ``build_scene_tables`` laid out)."""
    out, b = [], 0
    for c in counts:
        out.append(slice(b, b + int(c)))
        b += int(c)
    return out


def _offsets(what: str, sizes: Sequence[int], n_scenes: int, allow_empty: bool) -> np.ndarray:
    vals = [int(v) for v in sizes]
    if len(vals) != n_scenes:
        raise ValueError(f"{what} has {len(vals)} entries for {n_scenes} scenes")
    for i, v in enumerate(vals):
        if v < 0 or (v == 0 and not allow_empty):
            raise ValueError(f"scene {i}: {what} is {v}" + ("" if allow_empty else "; every scene needs at least one"))
    off = np.zeros(n_scenes + 1, dtype=np.int64)
    np.cumsum(vals, out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError(f"the concatenated {what} do not fit 32-bit offsets")
    return off.astype(np.int32)


def build_eval_tables(counts: Sequence[int], box_counts: Optional[Sequence[int]] = None,
                      cloud_sizes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """Tables of the per-scene evaluation of a many-scene batch (``ramp_traj_metrics_scenes``, ``ramp_scene_summary``,
    ``ramp_traj_costs_scenes``, ``ramp_select_best_scenes``), for the layout ``build_scene_tables`` produces: a scene's
    trajectories adjacent, scenes in order.

    counts       trajectories of each scene, at least one each
    box_counts   boxes of each scene (0 allowed: such a scene has collision intensity 0), or None
    cloud_sizes  points of each scene's cost cloud, at least one each, or None

    Returns int32 arrays of ``n_scenes + 1`` entries: ``traj_first`` (strictly increasing, ``[-1] = B``) and, for what was given,
    ``box_offset`` (may repeat a value) and ``cloud_offset`` (strictly increasing) into the boxes / clouds concatenated over scenes.
    """
    n_scenes = len(counts)
    if n_scenes == 0:
        raise ValueError("no scenes given")
    out = {"traj_first": _offsets("trajectory counts", counts, n_scenes, allow_empty=False)}
    if box_counts is not None:
        out["box_offset"] = _offsets("box counts", box_counts, n_scenes, allow_empty=True)
    if cloud_sizes is not None:
        out["cloud_offset"] = _offsets("cost cloud sizes", cloud_sizes, n_scenes, allow_empty=False)
    return out


def build_clearance_tables(counts: Sequence[int], box_counts: Optional[Sequence[int]] = None,
                           sphere_counts: Optional[Sequence[int]] = None,
                           cloud_sizes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """Tables of ``ramp_traj_clearance`` (``trajectory_clearance``) for the layout ``build_scene_tables`` produces: a scene's
    trajectories adjacent, scenes in order.

    counts         trajectories of each scene, at least one each
    box_counts / sphere_counts / cloud_sizes  boxes, spheres and cloud points of each scene, or None = none in any scene; 0 is
                   allowed everywhere: a scene may lack any kind of primitive

    Returns int32 arrays of ``n_scenes + 1`` entries: ``traj_first`` (strictly increasing, ``[-1] = B``) and ``box_offset``,
    ``sphere_offset``, ``cloud_offset`` (each may repeat a value) into the primitives concatenated over scenes."""
    n_scenes = len(counts)
    if n_scenes == 0:
        raise ValueError("no scenes given")
    out = {"traj_first": _offsets("trajectory counts", counts, n_scenes, allow_empty=False)}
    for key, what, vals in (("box_offset", "box counts", box_counts), ("sphere_offset", "sphere counts", sphere_counts),
                            ("cloud_offset", "cloud sizes", cloud_sizes)):
        out[key] = _offsets(what, [0] * n_scenes if vals is None else vals, n_scenes, allow_empty=True)
    return out


def build_encode_tables(shapes: Sequence[Sequence[int]]) -> Dict[str, np.ndarray]:
    """CSR tables of a ragged batch of scenes for the scene encoder (``TemporalUnetInference.encode_scenes`` ->
    ``ramp_encode_scenes``), the clouds concatenated point by point in scene order.

    shapes   per scene ``(n_obstacles, n_points)``: the leading dimensions of its ``(No, Np, D)`` cloud; scenes may differ in both,
             inside one scene every obstacle has ``n_points`` points

    Returns int32 arrays: ``scene_first`` (n_scenes + 1) first obstacle of each scene and ``obstacle_first`` (n_obstacles + 1) first
    point of each obstacle, both from 0 and strictly increasing.  Refused, as the C ABI refuses them: no scene, a scene without an
    obstacle or with empty obstacles, totals beyond 32-bit offsets."""
    n_scenes = len(shapes)
    if n_scenes == 0:
        raise ValueError("no scenes given")
    counts, sizes, total = [], [], 0
    for i, sh in enumerate(shapes):
        if len(sh) != 2:
            raise ValueError(f"scene {i}: expected (n_obstacles, n_points), got {tuple(sh)}")
        no, npts = int(sh[0]), int(sh[1])
        if no <= 0:
            raise ValueError(f"scene {i} has no obstacle (n_obstacles = {no})")
        if npts <= 0:
            raise ValueError(f"scene {i} has empty obstacles (n_points = {npts})")
        total += no * npts
        if total >= 2 ** 31:
            raise ValueError(f"scene {i}: the concatenated clouds do not fit 32-bit offsets")
        counts.append(no)
        sizes.append(npts)
    scene_first = np.zeros(n_scenes + 1, dtype=np.int64)
    np.cumsum(counts, out=scene_first[1:])
    obstacle_first = np.zeros(int(scene_first[-1]) + 1, dtype=np.int64)
    np.cumsum(np.repeat(np.asarray(sizes, dtype=np.int64), counts), out=obstacle_first[1:])
    return {"scene_first": scene_first.astype(np.int32), "obstacle_first": obstacle_first.astype(np.int32)}


def build_episode_tables(counts: Sequence[int], row_patterns: Sequence[Sequence[int]]) -> Dict[str, np.ndarray]:
    """Tables of one many-episode replanning job (``run_inference_episodes`` -> ``ramp_set_scenes`` + ``ramp_replan_episodes``): the
    loop over contexts and experiments of the reference's ``scripts/inference/inference_dynamic.py`` turned into one batch.

    counts        candidate trajectories of each episode, at least one each; an episode's rows are adjacent, episodes in order
    row_patterns  per episode, the network-row -> variant pattern (0 = the episode's own latent, 1 = unconditional) its
                  single-episode job would hand to ``set_scene``, applied cyclically FROM THE EPISODE'S FIRST ROW: ``[0, 1]`` for true
                  classifier-free guidance, and for the reference's row pairing ``[0, 0, 1, 1]`` (even count) or ``[0, 1, 1, 0]`` (odd
                  count) by the parity of the episode's OWN count -- so an episode's rows read what they read in a job of their own

    Returns int32 arrays: ``traj_first`` (E + 1) first row of each episode, ``[-1] = B``; ``row_episode`` (B) episode of each
    trajectory; ``row_variant`` (2 B) latent of each network row, episode e's own latent at index e and the shared all-zero one
    at index E."""
    E = len(counts)
    if E == 0:
        raise ValueError("no episodes given")
    if len(row_patterns) != E:
        raise ValueError(f"row_patterns has {len(row_patterns)} entries for {E} episodes")
    traj_first = _offsets("candidate counts", counts, E, allow_empty=False)
    if 2 * int(traj_first[-1]) >= 2 ** 31:
        raise ValueError("the job's network rows do not fit 32-bit offsets")
    row_episode = np.repeat(np.arange(E, dtype=np.int32), np.diff(traj_first))
    row_variant = np.empty(2 * row_episode.size, dtype=np.int32)
    for e, pat in enumerate(row_patterns):
        pat = np.asarray([int(v) for v in pat], dtype=np.int64)
        if pat.size == 0 or bool(((pat != 0) & (pat != 1)).any()):
            raise ValueError(f"episode {e}: a row pattern is a non-empty sequence of 0 (conditional) and 1 (unconditional), got {pat.tolist()}")
        r0, r1 = 2 * int(traj_first[e]), 2 * int(traj_first[e + 1])
        row_variant[r0:r1] = np.where(np.resize(pat, r1 - r0) == 0, e, E)
    return {"traj_first": traj_first, "row_episode": row_episode, "row_variant": row_variant}


def scene_counts(counts_or_traj_scene, n_scenes: int, B: int) -> List[int]:
    """Per-scene trajectory counts from either the counts themselves (``n_scenes`` positive entries summing to ``B``) or the
    ``traj_scene`` (B) array of ``build_scene_tables`` (scenes in order, a scene's rows adjacent).  A device ``traj_scene`` is copied
    to the host: pass counts where that copy matters."""
    v = counts_or_traj_scene
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    v = np.asarray(v).astype(np.int64).reshape(-1)
    if v.size == n_scenes and int(v.sum()) == B and bool((v > 0).all()):
        return [int(c) for c in v]
    if v.size != B:
        raise ValueError(f"expected {n_scenes} per-scene counts summing to {B}, or the scene of each of the {B} trajectories; "
                         f"got {v.size} entries")
    if v.size and (v.min() < 0 or v.max() >= n_scenes or bool((np.diff(v) < 0).any())):
        raise ValueError("traj_scene must hold scene indices in [0, n_scenes) in ascending order (a scene's trajectories adjacent)")
    return [int(c) for c in np.bincount(v, minlength=n_scenes)]
