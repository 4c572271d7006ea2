"""Plans longer than the network's horizon: a long trajectory of ``L`` waypoints as ``W`` overlapping windows of ``H`` waypoints in adjacent
rows of one batch, made to agree on the waypoints they share (``run_inference_stitched`` -> ``ramp_set_scenes`` + ``ramp_sample_stitched``;
include/ramp_hip.h states the layout, the stitch and its places in the job).

The table helpers and the references are pure numpy, no device: everything but ``stitch_windows`` / ``assemble`` is testable without a GPU."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib      # the binding module imports no device code until load()

BLEND_KINDS = ('mean', 'ramp', 'left')


def stitch_layout(H: int, W: int, O: int) -> Tuple[int, int]:
    """``(stride, L)`` of ``W`` windows of ``H`` waypoints that overlap by ``O``: stride ``H - O``, ``L = H + (W - 1) stride``.  ``W = 1`` reads
    no overlap: ``(H, H)``."""
    H, W, O = int(H), int(W), int(O)
    if H < 1:
        raise ValueError(f"stitch: H = {H}")
    if W < 1:
        raise ValueError(f"stitch: n_windows = {W}; at least 1")
    if W == 1:
        return H, H
    if not 1 <= O <= H // 2:
        raise ValueError(f"stitch: overlap {O} outside 1 .. H / 2 = {H // 2}")
    return H - O, H + (W - 1) * (H - O)


def blend_weights(O: int, kind: str = 'ramp') -> np.ndarray:
    """The (O,) float32 weights alpha_k of the right window in the blend ``l + alpha_k (r - l)``: 'mean' 1/2, 'ramp' (k + 1) / (O + 1) (the left
    window fades out towards its end), 'left' 0 (the left window's values)."""
    if kind not in BLEND_KINDS:
        raise ValueError(f"stitch: unknown blend {kind!r}; known: {list(BLEND_KINDS)}")
    O = int(O)
    if O < 0:
        raise ValueError(f"stitch: overlap {O}")
    if kind == 'mean':
        return np.full(O, 0.5, dtype=np.float32)
    if kind == 'left':
        return np.zeros(O, dtype=np.float32)
    return ((np.arange(O, dtype=np.float64) + 1.0) / (O + 1.0)).astype(np.float32)


def _alpha(alpha, O: int) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(alpha, dtype=np.float32).reshape(-1))
    if a.size != O:
        raise ValueError(f"stitch: {a.size} blend weights for an overlap of {O}")
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError("stitch: blend weights must be finite and lie in [0, 1]")
    return a


def blend_table(blend: Union[str, Sequence[float]], O: int) -> np.ndarray:
    """``blend=`` of the entry points as (O,) float32 weights: a kind of ``blend_weights`` or the weights themselves, checked."""
    return blend_weights(O, blend) if isinstance(blend, str) else _alpha(blend, O)


def pin_indices(keys: Sequence[int], L: int) -> list:
    """Long waypoint indices of a hard-condition dict's keys: negative ones count from ``L``."""
    out = []
    for k in keys:
        i = int(k) if int(k) >= 0 else L + int(k)
        if not 0 <= i < L:
            raise ValueError(f"stitch: waypoint {k} outside the long trajectory of {L} waypoints")
        out.append(i)
    if len(out) > _lib.STITCH_MAX_PINS:
        raise ValueError(f"stitch: {len(out)} pinned waypoints; at most {_lib.STITCH_MAX_PINS}")
    return out


def build_stitch_tables(H: int, n_windows: int, overlap: int, n_chains: int, n_scenes: int, pin_keys: Sequence[int] = (),
                        cloud_sizes: Optional[Sequence[int]] = None) -> Dict[str, np.ndarray]:
    """Tables of one stitched job of ``n_chains`` chains: row ``c W + w`` is window ``w`` of chain ``c``.

    n_scenes     1 (every window reads the one scene's latent) or ``n_windows`` (window w reads scene w's)
    pin_keys     long waypoint indices of the hard conditions, negative ones counted from L
    cloud_sizes  points of each scene's APF cloud, or None

    Returns ``traj_scene`` (B) int32 scene of each row; ``row_variant`` (2 B) int32 -- row ``2 r`` reads its scene's latent, the odd row the shared
    all-zero latent at index ``n_scenes`` --; ``pin_idx`` (n_pin) int32; ``cloud_offset`` (n_scenes + 1) int32 (with ``cloud_sizes``); ``stride``, ``L``
    and ``B`` (ints)."""
    st, L = stitch_layout(H, n_windows, overlap)
    W, Cn, ns = int(n_windows), int(n_chains), int(n_scenes)
    if Cn < 1:
        raise ValueError(f"stitch: {Cn} chains; at least one")
    if ns not in (1, W):
        raise ValueError(f"stitch: {ns} scenes for {W} windows; one scene for all windows or one per window")
    win_scene = np.arange(W, dtype=np.int32) if ns == W else np.zeros(W, dtype=np.int32)
    traj_scene = np.ascontiguousarray(np.tile(win_scene, Cn))
    row_variant = np.empty(2 * traj_scene.size, dtype=np.int32)
    row_variant[0::2] = traj_scene
    row_variant[1::2] = ns
    out = {"traj_scene": traj_scene, "row_variant": row_variant, "pin_idx": np.asarray(pin_indices(pin_keys, L), dtype=np.int32),
           "stride": st, "L": L, "B": Cn * W}
    if cloud_sizes is not None:
        sizes = [int(s) for s in cloud_sizes]
        if len(sizes) != ns or any(s <= 0 for s in sizes):
            raise ValueError(f"stitch: cloud sizes {sizes} for {ns} scene(s); every scene needs at least one point")
        off = np.zeros(ns + 1, dtype=np.int64)
        np.cumsum(sizes, out=off[1:])
        out["cloud_offset"] = off.astype(np.int32)
    return out


def stitch_reference(a: np.ndarray, W: int, O: int, alpha, pins: Optional[Dict[int, np.ndarray]] = None) -> np.ndarray:
    """The definition, in the dtype of ``a`` (float32 or float64), on a copy of ``a`` (C W, H, S): the blend ``m = l + alpha_k (q - l)`` of every
    overlap element, difference, product and sum rounded once each (``q == l`` returns ``l``), then the pins {long waypoint: (S,) or (C, S)} in
    order, written into every window that covers them."""
    a = np.array(a, copy=True)
    if a.dtype not in (np.float32, np.float64) or a.ndim != 3:
        raise ValueError("stitch_reference: a (C W, H, S) float32 or float64 array")
    B, H, S = a.shape
    st, L = stitch_layout(H, W, O)
    if B % W:
        raise ValueError(f"stitch_reference: {B} rows are no multiple of {W} windows")
    Cn = B // W
    v = a.reshape(Cn, W, H, S)
    if W > 1:
        al = _alpha(alpha, O).astype(a.dtype)[None, None, :, None]
        l, q = v[:, :-1, st:, :].copy(), v[:, 1:, :O, :].copy()
        m = np.where(q == l, l, l + al * (q - l))
        v[:, :-1, st:, :] = m
        v[:, 1:, :O, :] = m
    for k, val in (pins or {}).items():
        i = pin_indices([k], L)[0]
        val = np.broadcast_to(np.asarray(val, dtype=a.dtype), (Cn, S))
        for w in range(W):
            if 0 <= i - w * st < H:
                v[:, w, i - w * st, :] = val
    return a


def assemble_reference(a: np.ndarray, W: int, O: int) -> np.ndarray:
    """(C, L, S) from the windows ``a`` (C W, H, S): every long waypoint from the window with the smallest ``w`` that covers it."""
    B, H, S = a.shape
    st, L = stitch_layout(H, W, O)
    v = a.reshape(B // W, W, H, S)
    out = np.empty((B // W, L, S), dtype=a.dtype)
    for w in reversed(range(W)):
        out[:, w * st:w * st + H, :] = v[:, w]
    return out


def split_long(x: np.ndarray, H: int, W: int, O: int) -> np.ndarray:
    """The windows (C W, H, S) of the long trajectories ``x`` (C, L, S): the inverse of ``assemble_reference`` on stitched windows."""
    st, L = stitch_layout(H, W, O)
    Cn, Lx, S = x.shape
    if Lx != L:
        raise ValueError(f"split_long: {Lx} waypoints; {W} windows of {H} with overlap {O} hold {L}")
    out = np.empty((Cn, W, H, S), dtype=x.dtype)
    for w in range(W):
        out[:, w] = x[:, w * st:w * st + H, :]
    return out.reshape(Cn * W, H, S)


# ---------------------------------------------------------------------------------------------- the device
def fill_stitch(n_windows: int, overlap: int, alpha: np.ndarray, pin_idx: np.ndarray, pin_val) -> _lib.RampStitch:
    """``ramp_stitch`` from host tables (``alpha`` float32 (O), ``pin_idx`` int32 (n_pin)) and the device (n_pin, C, S) ``pin_val`` tensor or None;
    the caller keeps all three alive for the call."""
    st = _lib.RampStitch()
    st.n_windows, st.overlap, st.n_pin = int(n_windows), int(overlap), int(len(pin_idx))
    if alpha is not None and len(alpha):
        assert alpha.dtype == np.float32 and alpha.flags.c_contiguous
        st.alpha_host = alpha.ctypes.data_as(_lib.c_f32p)
    if st.n_pin:
        assert pin_idx.dtype == np.int32 and pin_idx.flags.c_contiguous
        st.pin_idx_host = pin_idx.ctypes.data_as(_lib.c_i32p)
        st.pin_val = _lib.ptr(pin_val)
    return st


def pin_values(pins: Dict[int, object], n_chains: int, S: int, device):
    """The device (n_pin, C, S) float32 tensor of a hard-condition dict's values ((S,) or (C, S) each), or None without pins."""
    import torch
    if not pins:
        return None
    vals = []
    for k, v in pins.items():
        v = torch.as_tensor(v).to(device, torch.float32)
        v = v.unsqueeze(0).expand(n_chains, -1) if v.dim() == 1 else v
        if tuple(v.shape) != (n_chains, S):
            raise ValueError(f"stitch: the value of waypoint {k} must be ({S},) or ({n_chains}, {S}); got {tuple(v.shape)}")
        vals.append(v)
    return torch.stack(vals).contiguous()


def stitch_windows(x, n_windows: int, overlap: int, blend: Union[str, Sequence[float]] = 'ramp', pins: Optional[Dict[int, object]] = None):
    """The stitch (one launch, ``ramp_stitch_windows``) on a copy of the (C W, H, S) windows ``x``: ``blend`` a kind of ``blend_weights`` or
    the (O,) weights themselves, ``pins`` {long waypoint: (S,) or (C, S)} (negative indices count from L, later entries win)."""
    import torch
    dev = x.device
    out = x.detach().to(torch.float32).contiguous().clone()
    B, H, S = out.shape
    W = int(n_windows)
    st_, L = stitch_layout(H, W, overlap)
    if B % W:
        raise ValueError(f"stitch: {B} rows are no multiple of {W} windows")
    O = int(overlap) if W > 1 else 0
    alpha = blend_table(blend, O)
    idx = np.asarray(pin_indices(list((pins or {}).keys()), L), dtype=np.int32)
    val = pin_values(pins or {}, B // W, S, dev)
    st = fill_stitch(W, O, alpha, idx, val)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_stitch_windows(_lib.ptr(out), B // W, W, H, S, C.byref(st), _lib.current_stream()), "ramp_stitch_windows")
    return out


def assemble(x, n_windows: int, overlap: int):
    """(..., C, L, S) from the windows ``x`` (..., C W, H, S) on the device (``ramp_stitch_assemble``); leading dimensions (a chain's steps) are
    batched."""
    import torch
    dev = x.device
    xx = x.detach().to(torch.float32).contiguous()
    *lead, B, H, S = xx.shape
    W = int(n_windows)
    _st, L = stitch_layout(H, W, overlap)
    if B % W:
        raise ValueError(f"stitch: {B} rows are no multiple of {W} windows")
    n_lead = int(np.prod(lead)) if lead else 1
    out = torch.empty((*lead, B // W, L, S), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().ramp_stitch_assemble(_lib.ptr(xx), n_lead * (B // W), W, H, S, int(overlap) if W > 1 else 0, _lib.ptr(out),
                                                    _lib.current_stream()), "ramp_stitch_assemble")
    return out
