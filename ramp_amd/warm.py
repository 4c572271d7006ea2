"""Warm-started sampling jobs: every row of a job starts from a given plan, noised to a level of its own, and runs only the tail of the
schedule (``warm_start=`` of ``run_inference*``; ``ramp_sample_warm`` / ``ramp_warm_start`` in include/ramp_hip.h).  This module is the
definition, in numpy, and the host tables of the job; the HIP kernels (csrc/warm.hip) are tested against it bit for bit.

Definition.  ``steps_full`` is the model's own iteration list (``_ddpm_steps(n_without_noise)[0]`` for DDPM, ``ddim_set_timesteps(K)`` for
DDIM), ``t_j = max(steps_full[j], 0)``, ``n = len(steps_full)``.

row levels   row b has a level l_b: None (no prior) or an integer in [0, T - 1].  ``j0_full(b)`` = 0 for None, else min{j : t_j <= l_b}
             (the last timestep is 0, so it exists): the row starts at the schedule's largest timestep not above what the caller asked for.
job start    J = min_b j0_full(b); ``start=`` overrides it with J = min{j : t_j <= start} and no row may start before it.  The job runs the
             iterations J .. n - 1 (n' = n - J evaluations) and ``j0[b] = j0_full(b) - J``.  Its noise block is (n' + 1, B, H, S) for DDPM,
             (1, B, H, S) for DDIM; block 0 is the start draw.  A None row forces J = 0.
start state  a None row: x_init[b] = noise[0][b], the same bits.  Otherwise, in float32,
                 x_init[b] = (sqrt_alphas_cumprod[t] * prior[b]) + (sqrt_one_minus_alphas_cumprod[t] * noise[0][b]),   t = t_{J + j0[b]},
             each product and the sum rounded once (``warm_init_reference``).  Then what the plain job applies to x_T: the hard conditioning,
             or the stitch of a stitched job.  The result is chain block 0 and is kept as x_init.
hold         after iteration j of the job (reverse step, hooks, hard conditioning or stitch, chain write) every row with j0[b] > j is put
             back to x_init[b], in the state and in chain block j + 1 (``warm_hold_reference``).  The network still evaluates such a row; the
             evaluation is wasted on it and harmless, and no hook result survives on it.
indexing     whatever indexes ``steps_full`` keeps doing so: the APF switches, the ``noise_std_extra_schedule_fn`` scales and the resampling
             flags are computed on the full list and lose their first J entries; tables keyed by timestep are built from the tail."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def _first_at_or_below(t, level: int) -> int:
    """min{j : t_j <= level}; t ends at 0 and level >= 0, so it exists."""
    for j, tj in enumerate(t):
        if tj <= level:
            return j
    raise ValueError(f"warm start: no timestep of the schedule is <= {level} (the list must end at 0)")


def warm_tables(levels: Sequence[Optional[int]], steps_full, start: Optional[int] = None, T: Optional[int] = None) -> dict:
    """The host tables of a warm-started job.  ``levels``: one entry per row, None or an int in [0, T - 1] (``T``: the model's
    n_diffusion_steps; without it only ``>= 0`` is checked).  Returns ``J`` (first iteration of ``steps_full`` the job runs), ``j0`` (B) int32
    (the row's first own iteration, counted from J), ``t_row`` (B) int32 (the timestep the row is noised to; -1 for a None row) and
    ``n_hold = max j0`` (the number of iterations with a hold launch)."""
    t = [max(int(s), 0) for s in steps_full]
    if not t or t[-1] != 0:
        raise ValueError("warm start: the iteration list must end at timestep 0")
    if len(levels) == 0:
        raise ValueError("warm start: no rows")
    full = []
    for b, lv in enumerate(levels):
        if lv is None:
            full.append(0)
            continue
        if isinstance(lv, (float, np.floating)) and float(lv) != int(lv):
            raise ValueError(f"warm start: level {lv!r} of row {b} is not an integer")
        lv = int(lv)
        if lv < 0 or (T is not None and lv > T - 1):
            raise ValueError(f"warm start: level {lv} of row {b} lies outside [0, {'T - 1' if T is None else T - 1}]")
        full.append(_first_at_or_below(t, lv))
    if start is None:
        J = min(full)
    else:
        start = int(start)
        if start < 0 or (T is not None and start > T - 1):
            raise ValueError(f"warm start: start={start} lies outside [0, {'T - 1' if T is None else T - 1}]")
        J = _first_at_or_below(t, start)
        for b, (lv, f) in enumerate(zip(levels, full)):
            if f < J:
                raise ValueError(f"warm start: start={start} (iteration {J}) lies below the start of row {b} "
                                 f"({'no prior' if lv is None else f'level {int(lv)}'}: iteration {f})")
    j0 = np.asarray([f - J for f in full], np.int32)
    t_row = np.asarray([-1 if lv is None else t[f] for lv, f in zip(levels, full)], np.int32)
    return {'J': int(J), 'j0': j0, 't_row': t_row, 'n_hold': int(j0.max())}


def warm_init_reference(noise0, prior, t_row, sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, dtype=np.float32):
    """x_init (B, H, S) BEFORE the hard conditioning / stitch: a row with t_row[b] < 0 is noise0[b] itself; every other row
    (sa[t] * prior[b]) + (s1a[t] * noise0[b]) in ``dtype`` -- two products and one sum, each rounded once, no fused multiply-add."""
    dt = np.dtype(dtype).type
    noise0 = np.asarray(noise0)
    out = noise0.astype(dtype).copy()
    sa, s1a = np.asarray(sqrt_alphas_cumprod).astype(dtype), np.asarray(sqrt_one_minus_alphas_cumprod).astype(dtype)
    for b, t in enumerate(np.asarray(t_row)):
        if t < 0:
            continue
        a = (dt(sa[t]) * np.asarray(prior[b]).astype(dtype)).astype(dtype)
        c = (dt(s1a[t]) * noise0[b].astype(dtype)).astype(dtype)
        out[b] = (a + c).astype(dtype)
    return out


def warm_hold_reference(x, x_init, j0, j: int):
    """The hold behind iteration j: rows with j0[b] > j are x_init[b] again (a copy; the other rows keep their bits)."""
    out = np.array(x, copy=True)
    held = np.asarray(j0) > j
    out[held] = np.asarray(x_init)[held]
    return out


def straight_line_prior(start_state, goal_state, H: int, n_pos: Optional[int] = None):
    """The straight line from ``start_state`` to ``goal_state`` (S,) over H waypoints as a (H, S) float32 prior: positions (the first
    ``n_pos`` channels, default S // 2) interpolated; the next ``n_pos`` channels (velocities) the constant finite difference of the
    positions, (goal - start) / (H - 1); whatever channels remain interpolated like the positions."""
    a, b = np.asarray(start_state, np.float64).reshape(-1), np.asarray(goal_state, np.float64).reshape(-1)
    if a.shape != b.shape or H < 2:
        raise ValueError("straight_line_prior: start and goal must be (S,) alike and H >= 2")
    S = a.shape[0]
    d = S // 2 if n_pos is None else int(n_pos)
    if not 0 < d <= S:
        raise ValueError("straight_line_prior: n_pos outside 1 .. S")
    w = np.linspace(0.0, 1.0, H)[:, None]
    out = a[None] + w * (b - a)[None]
    nv = min(d, S - d)
    if nv:
        out[:, d:d + nv] = ((b[:nv] - a[:nv]) / (H - 1))[None]
    return out.astype(np.float32)


def prior_rows(prior, counts):
    """Broadcast a prior to the job's rows (B, H, S), B = sum(counts): ``prior`` is (H, S) or (1, H, S) (every row the same plan), one
    entry per scene -- (n_scenes, H, S), or a list of (H, S) / (counts[i], H, S) arrays -- or already (B, H, S).  numpy in, numpy out;
    torch tensors in, a torch tensor out."""
    counts = [int(c) for c in counts]
    B, n_sc = sum(counts), len(counts)
    is_torch = hasattr(prior, 'detach') or (isinstance(prior, (list, tuple)) and len(prior) and hasattr(prior[0], 'detach'))
    if is_torch:
        import torch
        as_arr, cat, rep = (lambda v: v), torch.cat, (lambda v, n: v.unsqueeze(0).expand(n, -1, -1) if v.dim() == 2 else v)
        ndim = lambda v: v.dim()      # noqa: E731
    else:
        as_arr, cat = (lambda v: np.asarray(v, np.float32)), np.concatenate
        rep = lambda v, n: np.broadcast_to(v[None], (n,) + v.shape) if v.ndim == 2 else v      # noqa: E731
        ndim = lambda v: v.ndim      # noqa: E731
    if isinstance(prior, (list, tuple)):
        if len(prior) != n_sc:
            raise ValueError(f"prior_rows: {len(prior)} priors for {n_sc} scenes")
        parts = []
        for i, (v, n) in enumerate(zip(prior, counts)):
            v = rep(as_arr(v), n)
            if ndim(v) != 3 or v.shape[0] != n:
                raise ValueError(f"prior_rows: the prior of scene {i} must be (H, S) or ({n}, H, S)")
            parts.append(v)
        return cat(parts)
    v = as_arr(prior)
    if ndim(v) == 2:
        return rep(v, B)
    if ndim(v) != 3:
        raise ValueError("prior_rows: a prior is (H, S), (1, H, S), one entry per scene or one per row")
    if v.shape[0] == B and (n_sc == B or v.shape[0] != n_sc):
        return v
    if v.shape[0] == 1:
        return rep(v[0], B)
    if v.shape[0] == n_sc:
        return cat([rep(v[i], n) for i, n in enumerate(counts)])
    raise ValueError(f"prior_rows: {v.shape[0]} priors for {n_sc} scenes / {B} rows")


def level_rows(level, counts):
    """The ``level=`` argument as one entry per row: an int or None (all rows), one entry per row, or one per scene."""
    counts = [int(c) for c in counts]
    B = sum(counts)
    if level is None or np.isscalar(level):
        return [level] * B
    lv = [None if v is None else v for v in (level.tolist() if hasattr(level, 'tolist') else list(level))]
    if len(lv) == B:
        return lv
    if len(lv) == len(counts):
        return [v for v, n in zip(lv, counts) for _ in range(n)]
    raise ValueError(f"warm start: {len(lv)} levels for {len(counts)} scenes / {B} rows")
