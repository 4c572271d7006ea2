"""Resampling trajectories by weight on the HIP kernels: a thin wrapper of ``ramp_resample_groups`` (steps 3 and 4 of a resampling event as
include/ramp_hip.h states them: normalised weights and ESS per group, the gate, systematic resampling, the row gather) and the lineage of a
steered job.  Inside a sampling job the same kernels run through ``resample=`` of ``run_inference*`` (``ramp_amd.diffusion.resample_tables``,
``ramp_sample_steered``)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def group_table(group_first: Sequence[int], B: int) -> np.ndarray:
    """The host int32 (n_groups + 1) table of contiguous groups, checked: [0] = 0, strictly increasing, [-1] = B."""
    gf = np.ascontiguousarray(np.asarray(group_first, dtype=np.int64).reshape(-1))
    if gf.size < 2 or gf[0] != 0 or gf[-1] != B or np.any(np.diff(gf) <= 0):
        raise ValueError(f"group table must start at 0, increase strictly and end at B = {B}; got {gf.tolist()}")
    return gf.astype(np.int32)


@torch.no_grad()
def systematic_resample(x: torch.Tensor, logw: torch.Tensor, group_first: Sequence[int], u, ess_frac: float = 2.0,
                        c_prev: Optional[torch.Tensor] = None):
    """One resampling of the (B, H, S) trajectories ``x`` within the contiguous groups ``group_first`` (n_groups + 1 entries from 0 to B) by
    the log-weights ``logw`` (B,), one uniform ``u[g]`` in (0, 1) per group; a group resamples when its ESS < ``ess_frac`` * size (0 never,
    above 1 always).  Works on copies.  Returns ``(x, logw, ancestors, ess)`` -- and ``c_prev`` permuted alike as a fifth entry when given:
    x[i] = the old x[ancestors[i]], logw 0 in every group that resampled, ancestors (B,) int32 within the batch, ess (n_groups,) float64."""
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    gf = group_table(group_first, B)
    G = len(gf) - 1
    if not (np.isfinite(ess_frac) and 0.0 <= ess_frac <= 2.0):
        raise ValueError("ess_frac must lie in [0, 2]")
    lw = torch.as_tensor(logw).detach().to(dev, torch.float64).contiguous().clone()
    uu = torch.as_tensor(u).detach().to(dev, torch.float32).reshape(-1).contiguous()
    if tuple(lw.shape) != (B,) or tuple(uu.shape) != (G,):
        raise ValueError(f"logw must be ({B},) and u ({G},); got {tuple(lw.shape)} and {tuple(uu.shape)}")
    cp = None if c_prev is None else torch.as_tensor(c_prev).detach().to(dev, torch.float64).contiguous().clone()
    if cp is not None and tuple(cp.shape) != (B,):
        raise ValueError(f"c_prev must be ({B},)")
    anc = torch.empty((B,), device=dev, dtype=torch.int32)
    ess = torch.empty((G,), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_resample_groups(_lib.ptr(out), B, H, S, _lib.ptr(lw), _lib.ptr(cp), gf.ctypes.data_as(_lib.c_i32p), G,
                                                    _lib.ptr(uu), float(ess_frac), _lib.ptr(anc), _lib.ptr(ess), _lib.current_stream()),
                   "ramp_resample_groups")
    return (out, lw, anc, ess) if cp is None else (out, lw, anc, ess, cp)


def lineage(ancestors) -> np.ndarray:
    """For each final trajectory of a steered job its index at the start of the job: ``ancestors`` is the (n_events, B) table of the job
    (``last_resample['ancestors']``), event k having put the old row ancestors[k, i] into row i.  (B,) int64; no event: the identity."""
    a = np.asarray(ancestors.cpu() if torch.is_tensor(ancestors) else ancestors)
    if a.ndim != 2:
        raise ValueError(f"ancestors must be (n_events, B); got {a.shape}")
    B = a.shape[1]
    if a.size and (a.min() < 0 or a.max() >= B):
        raise ValueError("ancestor index outside the batch")
    idx = np.arange(B, dtype=np.int64)
    for k in range(a.shape[0] - 1, -1, -1):
        idx = a[k].astype(np.int64)[idx]
    return idx
