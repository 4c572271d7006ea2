"""Stitched windows (plans longer than the network's horizon): the kernel alone (``ramp_stitch_windows`` / ``ramp_stitch_assemble``) against the
numpy statement of the definition (``ramp_amd.stitch.stitch_reference``) bit for bit, the wiring into ``ramp_sample_stitched``, "one window is
the plain job", the consistency invariant of every chain block, free-running chains against float64, stale graphs and the refusals.

``StitchOracle`` inserts the reference into ``oracle.ramp_oracle.SamplerOracle``'s loops at the three places include/ramp_hip.h gives: the noise
blocks (alpha = 0, no pins), the start, and in every iteration the posterior mean (DDPM) / x0 (DDIM) and the updated state."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd import stitch as ST
from ramp_amd.spec import UNET_DIM_MULTS
from test_gpu_guide import F32, RADIUS, chain_sched, hcn, raw_guide, raw_params, small_model, uniform
from util import NoiseInjector, dev

pytestmark = pytest.mark.gpu

H = 8


# ------------------------------------------------------------------------------------------------ the job, in numpy
class StitchOracle(O.SamplerOracle):
    """SamplerOracle on stitched windows: ``stitch`` = dict(W, O, alpha (O), pins {long waypoint: (S,) or (C, S)}).  Every noise block is
    stitched with alpha = 0 and no pins; the start, the posterior mean / x0 and the updated state are stitched with the job's table.  The
    loops apply no hard conditions of their own."""

    def __init__(self, *a, stitch=None, **k):
        super().__init__(*a, **k)
        self.stitch = stitch

    def _st(self, v):
        s = self.stitch
        return ST.stitch_reference(v.astype(self.dt), s["W"], s["O"], s["alpha"], s["pins"])

    def _noise(self, z):
        s = self.stitch
        return ST.stitch_reference(z.astype(self.dt), s["W"], s["O"], np.zeros(s["O"] if s["W"] > 1 else 0, np.float32), None)

    def ddpm(self, noise, hard_conds, latent, noise_scale=0.5, **kw):
        assert not hard_conds
        s, dt = self.sched, self.dt
        x = self._st(self._noise(noise[0]))
        chain = [x.copy()]
        for j, t in enumerate(reversed(range(self.T))):
            e = self.eps_cfg(x, t, latent)
            _, mean = self.x0_mean(x, e, t)
            mean = self._st(mean)
            z = self._noise(noise[1 + j]) if t != 0 else np.zeros_like(x)
            std = np.exp(dt(0.5) * s["posterior_log_variance_clipped"][t])
            x = self._st((mean + std * z * dt(noise_scale)).astype(dt))
            chain.append(x.copy())
        return np.stack(chain)

    def ddim(self, noise0, hard_conds, latent, K=5, **kw):
        assert not hard_conds
        s, dt = self.sched, self.dt
        x = self._st(self._noise(noise0))
        chain, ac = [x.copy()], s["alphas_cumprod"]
        for j, t in enumerate(O.ddim_timesteps(self.T, K)):
            prev = t - self.T // K
            a_t, a_prev = ac[t], (ac[prev] if prev >= 0 else dt(1.0))
            e = self.eps_cfg(x, int(t), latent)
            x0, _ = self.x0_mean(x, e, int(t))
            x0 = self._st(x0)
            e2 = (x - np.sqrt(a_t) * x0) / np.sqrt(dt(1) - a_t)
            x = self._st((np.sqrt(a_prev) * x0 + np.sqrt(dt(1) - a_prev) * e2).astype(dt))
            chain.append(x.copy())
        return np.stack(chain)


# ------------------------------------------------------------------------------------------------ 1: the op against the definition
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def touched_mask(Cn, W, O, S, pin_idx):
    """True where the stitch may write: both locations of every overlap element and every window location of a pinned waypoint."""
    st, L = ST.stitch_layout(H, W, O)
    m = np.zeros((Cn, W, H, S), bool)
    if W > 1:
        m[:, :-1, st:] = True
        m[:, 1:, :O] = True
    for i in pin_idx:
        for w in range(W):
            if 0 <= i - w * st < H:
                m[:, w, i - w * st] = True
    return m.reshape(Cn * W, H, S)


@pytest.mark.parametrize("S", [4, 6])
@pytest.mark.parametrize("Cn,W,Ov", [(1, 1, 0), (1, 2, 1), (2, 2, 4), (2, 3, 2), (3, 3, 4)])
def test_op_is_the_definition_bit_for_bit(Cn, W, Ov, S):
    """ramp_stitch_windows against stitch_reference in float32 on uniform windows, every blend kind, pins {0, L - 1} and {0, 3, st, L - 1} (st
    lies in an overlap: the pin wins over the blend there; with one window st = L is left out) and once a waypoint named twice (the later
    value wins); every byte outside overlaps and pins keeps its bits; a second stitch changes nothing; ramp_stitch_assemble against
    assemble_reference on raw and on stitched windows."""
    st, L = ST.stitch_layout(H, W, Ov)
    x = uniform((Cn * W, H, S), 10 * Cn + W + Ov + S)
    pin_sets = [[0, L - 1], [k for k in (0, 3, st, L - 1) if k < L], [0, L - 1, -L]]
    for blend in ST.BLEND_KINDS:
        alpha = ST.blend_weights(Ov, blend)
        for n, keys in enumerate(pin_sets):
            vals = uniform((len(keys), Cn, S), 500 + n)
            pins = {k: vals[i] for i, k in enumerate(keys)}
            want = ST.stitch_reference(x, W, Ov, alpha, pins)
            got = ST.stitch_windows(dev(x), W, Ov, blend, {k: dev(v) for k, v in pins.items()}).cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (blend, keys)
            mask = touched_mask(Cn, W, Ov, S, ST.pin_indices(keys, L))
            assert np.array_equal(bits(got)[~mask], bits(x)[~mask])
            assert (bits(got)[mask] != bits(x)[mask]).any()
            if st in keys:      # the pin, not the blend, on both windows of the overlap waypoint
                v = got.reshape(Cn, W, H, S)
                assert np.array_equal(v[:, 0, st], pins[st]) and np.array_equal(v[:, 1, 0], pins[st])
            if -L in keys:
                assert np.array_equal(got.reshape(Cn, W, H, S)[:, 0, 0], pins[-L])
            again = ST.stitch_windows(dev(got), W, Ov, blend, {k: dev(v) for k, v in pins.items()}).cpu().numpy()
            assert np.array_equal(bits(again), bits(got))
            for a in (x, got):
                long = ST.assemble(dev(a), W, Ov).cpu().numpy()
                assert long.shape == (Cn, L, S) and np.array_equal(bits(long), bits(ST.assemble_reference(a, W, Ov)))
    # no pins: the blend alone; one window and no pins: nothing at all
    got = ST.stitch_windows(dev(x), W, Ov, 'ramp', None).cpu().numpy()
    assert np.array_equal(bits(got), bits(ST.stitch_reference(x, W, Ov, ST.blend_weights(Ov, 'ramp'), None)))
    if W == 1:
        assert np.array_equal(bits(got), bits(x))


# ------------------------------------------------------------------------------------------------ jobs through the C entry
def scene_clouds(o3, n):
    return [dev(synth.make_cloud(4, 30, 3, seed=41 + k) if o3 else synth.make_cloud(5 + k, 64, 2, seed=31 + k)) for k in range(n)]


def prepare(dm, scenes, Cn, W, Ov, pin_keys=()):
    """Latents and the row -> latent table of a stitched job in the context; returns the tables and the scene batch (no APF clouds)."""
    m = dm.model
    m.prepare_time_table(dm.n_diffusion_steps)
    tab = ST.build_stitch_tables(H, W, Ov, Cn, len(scenes), pin_keys)
    m.ctx()
    lat = torch.cat([m.encode_scenes(scenes), torch.zeros(1, m.context_dim, device="cuda")])
    m.set_scenes(lat, tab["row_variant"])
    ts = dev(tab["traj_scene"])
    batch = _lib.RampSceneBatch()
    batch.n_scenes, batch.traj_scene = len(scenes), _lib.ptr(ts)
    return tab, batch, ts


def run_stitched(dm, p, st, batch, noise, n_steps, cg=None, chain=True, want_long=None):
    """ramp_sample_stitched -> (chain or None, x_out, long_out or None)."""
    B, S = p.B, dm.state_dim
    ch = torch.empty((n_steps + 1, B, H, S), device="cuda") if chain else None
    out = torch.empty((B, H, S), device="cuda")
    long = torch.empty(want_long, device="cuda") if want_long else None
    _lib.check(_lib.load().ramp_sample_stitched(dm.model.ctx(), C.byref(p), C.byref(st) if st is not None else None,
                                                C.byref(cg) if cg is not None else None, C.byref(batch) if batch is not None else None,
                                                _lib.ptr(noise), _lib.ptr(ch), _lib.ptr(out), _lib.ptr(long), _lib.current_stream()),
               "ramp_sample_stitched")
    torch.cuda.synchronize()
    return ch, out, long


def stitch_table(keep, W, Ov, blend, pins, Cn, S):
    """ramp_stitch from a blend kind (or weights) and pins {long waypoint: numpy (S,) or (C, S)}; ``keep`` holds what it points at."""
    L = ST.stitch_layout(H, W, Ov)[1]
    O_ = Ov if W > 1 else 0
    alpha = ST.blend_weights(O_, blend) if isinstance(blend, str) else np.ascontiguousarray(blend, np.float32)
    idx = np.asarray(ST.pin_indices(list(pins.keys()), L), np.int32)
    val = ST.pin_values({k: torch.from_numpy(np.asarray(v)) for k, v in pins.items()}, Cn, S, "cuda")
    keep += [alpha, idx, val]
    return ST.fill_stitch(W, O_, alpha, idx, val)


# ------------------------------------------------------------------------------------------------ 2: wiring, bit-exact
@pytest.mark.parametrize("job,kind", [("2d", "ddpm"), ("2d", "ddim"), ("3d", "ddpm"), ("scenes", "ddpm"), ("scenes", "ddim")])
def test_wiring_is_the_stitch_on_the_plain_output(job, kind):
    """A one-iteration job, C = 2, W = 2, O = 2 (DDPM at t = 12 with the step's noise slot zeroed: x = mean; the last DDIM step: x = x0): the
    stitched job's x_out equals stitch_reference applied to the output of the plain job of the same rows -- no hard conditions, and as its
    noise the stitched job's own x_T (the caller's noise[0] stitched with alpha = 0, then pinned), so that both evaluate the network on the
    same state.  The stitched job is handed the RAW noise: its own noise stitch is part of what is checked.  2-D, 3-D, and with one scene per
    window."""
    from ramp_amd.diffusion import _HostArrays
    o3 = job == "3d"
    S, Cn, W, Ov = (6 if o3 else 4), 2, 2, 2
    B = Cn * W
    st_, L = ST.stitch_layout(H, W, Ov)
    ddim = kind == "ddim"
    dm = small_model(S, o3, sampler=kind)
    steps = [0] if ddim else [12]
    arrays, keep = _HostArrays(), []
    raw = synth.make_noise((2, B, H, S), seed=190)
    raw[1] = 0
    pins = {0: uniform((Cn, S), 191), st_: uniform((S,), 192), -1: uniform((Cn, S), 193)}
    alpha = ST.blend_weights(Ov, 'ramp')
    tab, batch, _ts = prepare(dm, scene_clouds(o3, W if job == "scenes" else 1), Cn, W, Ov)
    p = raw_params(dm, B, steps, arrays, ddim)
    pre = raw.copy()
    pre[0] = ST.stitch_reference(ST.stitch_reference(raw[0], W, Ov, np.zeros(Ov, np.float32), None), W, Ov, alpha, pins)
    assert not np.array_equal(pre[0], raw[0])
    _, plain, _ = run_stitched(dm, p, None, batch, dev(pre), 1, chain=False)
    noise = dev(raw)
    _, got, _ = run_stitched(dm, p, stitch_table(keep, W, Ov, 'ramp', pins, Cn, S), batch, noise, 1, chain=False)
    want = ST.stitch_reference(plain.cpu().numpy(), W, Ov, alpha, pins)
    moved = float(np.abs(want - plain.cpu().numpy()).max())
    print(f"wiring {job} {kind}: the stitch moved the plain output by {moved:.2e}")
    assert moved > 1e-3 and np.isfinite(want).all()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(noise.cpu().numpy()), bits(raw))      # the caller's array is never written


# ------------------------------------------------------------------------------------------------ 3: one window is the plain job
@pytest.mark.parametrize("src", ["injected", "philox"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_one_window_is_the_plain_job(kind, src):
    """W = 1 with pins {0, H - 1}: the whole chain of ramp_sample_stitched equals ramp_sample_guided with those hard conditions, bit for bit;
    st == NULL equals ramp_sample_guided the same way."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    S, B = 4, 3
    ddim = kind == "ddim"
    dm = small_model(S, sampler=kind)
    steps = [int(i) for i in dm.ddim_set_timesteps(5)] if ddim else [24, 12, 1, 0]
    n = len(steps)
    arrays, keep = _HostArrays(), []
    tab, batch, _ts = prepare(dm, scene_clouds(False, 1), B, 1, 0)
    hard = {k: torch.from_numpy(v).cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hcn(S).items()}
    noise = None if src == "philox" else dev(synth.make_noise((1 if ddim else n + 1, B, H, S), seed=8))

    def params(with_hard):
        p = raw_params(dm, B, steps, arrays, ddim, hard=hard if with_hard else None)
        if src == "philox":
            p.noise_mode, p.philox_seed, p.philox_offset = 1, 77, 12
        return p

    def guided(p):
        ch = torch.empty((n + 1, B, H, S), device="cuda")
        _lib.check(lib.ramp_sample_guided(dm.model.ctx(), C.byref(p), None, None, None, C.byref(batch), _lib.ptr(noise), None, None, _lib.ptr(ch),
                                          None, None, _lib.current_stream()), "ramp_sample_guided")
        torch.cuda.synchronize()
        return ch

    want = guided(params(True))
    assert np.isfinite(want.cpu().numpy()).all()
    st = stitch_table(keep, 1, 0, 'ramp', {0: hcn(S)[0], -1: hcn(S)[H - 1]}, B, S)
    got, _, _ = run_stitched(dm, params(False), st, batch, noise, n)
    assert torch.equal(got, want)
    null, _, _ = run_stitched(dm, params(True), None, batch, noise, n)
    assert torch.equal(null, want)
    assert not torch.equal(guided(params(False)), want)      # (the pins are what made them equal)


# ------------------------------------------------------------------------------------------------ 4: the consistency invariant
@pytest.mark.parametrize("hook,kind", [("guide", "ddpm"), ("guide", "ddim"), ("apf", "ddpm"), ("apf", "ddim")])
def test_every_chain_block_is_consistent(hook, kind):
    """A 4-iteration job, C = 2, W = 3, O = 4, one scene per window, with the cost guide resp. the APF (2-D) on iteration 2: in every chain
    block the tail of window w and the head of window w + 1 are bit-equal and the pinned waypoints hold their values; long_out is the assemble
    of x_out; the caller's noise array keeps its bits; and the hook did move the job (the same job without it differs from iteration 2 on)."""
    from ramp_amd.diffusion import _HostArrays
    S, Cn, W, Ov = 4, 2, 3, 4
    B = Cn * W
    st_, L = ST.stitch_layout(H, W, Ov)
    ddim = kind == "ddim"
    dm = small_model(S, sampler=kind, use_apf=hook == "apf")
    steps = [20, 15, 5, 0] if ddim else [24, 12, 1, 0]
    n = len(steps)
    arrays, keep = _HostArrays(), []
    scenes = scene_clouds(False, W)
    tab, batch, ts = prepare(dm, scenes, Cn, W, Ov)
    raw = synth.make_noise((1 if ddim else n + 1, B, H, S), seed=290)
    noise = dev(raw)
    pins = {0: uniform((Cn, S), 291), st_ + 1: uniform((Cn, S), 292), 2: uniform((S,), 294), -1: uniform((S,), 293)}      # (st + 1: in two windows)
    st = stitch_table(keep, W, Ov, 'mean', pins, Cn, S)
    gclouds = [dev(uniform((200 + 50 * k, 2), 295 + k)) for k in range(W)]

    def job(on):
        p = raw_params(dm, B, steps, arrays, ddim)
        cg = None
        if hook == "guide":
            cg = raw_guide(arrays, gclouds, [0, 0, 2 if on else 0, 0], [F32(5e-3)] * n, max_norm=F32(2.0))
        elif on:
            sizes = [int(s.numel() // 2) for s in scenes]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
            pts = torch.cat([s.reshape(-1, 2) for s in scenes]).contiguous()
            keep.extend([off, pts])
            p.apply_apf = arrays.i32([0, 0, 1, 0])
            dm._fill_apf(p, arrays, dict(window=5, threshold=0.5, strength=0.1, passes=2), None, batch, dict(cloud_points=pts, cloud_offset=off))
        else:
            batch.cloud_points = None
        return run_stitched(dm, p, st, batch, noise, n, cg=cg, want_long=(Cn, L, S))

    chain, x_out, long = job(True)
    ch = chain.cpu().numpy()
    assert np.isfinite(ch).all()
    v = ch.reshape(n + 1, Cn, W, H, S)
    assert np.array_equal(bits(v[:, :, :-1, st_:]), bits(v[:, :, 1:, :Ov]))
    for k, val in pins.items():
        i = ST.pin_indices([k], L)[0]
        for w in range(W):
            if 0 <= i - w * st_ < H:
                assert np.array_equal(v[:, :, w, i - w * st_], np.broadcast_to(val, (n + 1, Cn, S))), (k, w)
    assert torch.equal(chain[-1], x_out)
    assert np.array_equal(bits(long.cpu().numpy()), bits(ST.assemble_reference(x_out.cpu().numpy(), W, Ov)))
    assert torch.equal(ST.assemble(x_out, W, Ov), long)
    assert np.array_equal(bits(noise.cpu().numpy()), bits(raw))
    off_chain, _, _ = job(False)
    assert torch.equal(off_chain[:3], chain[:3]) and not torch.equal(off_chain[3], chain[3])


# ------------------------------------------------------------------------------------------------ 5: free-running chains against float64
CHAIN = dict(W=2, O=2)
_CHAIN = {}


def chain_inputs(kind):
    T = 3 if kind == "ddpm" else 25
    n = (T + 1) if kind == "ddpm" else 1
    hc = hcn(4)
    # (the seed: of 600 .. 611, five keep the float32 DDPM oracle within a quarter of the bar -- 600, 601, 603, 604, 608 -- and 608 by the widest
    # margin: bar 2.70e-4, float32 oracle 9.1e-6 (DDPM) / 6.4e-6 (DDIM), stitched vs unstitched 1.9; on the others the 3-step chain amplifies
    # float32 rounding past it, up to 1.8e-3)
    return T, synth.make_noise((n, 2, H, 4), seed=608), synth.make_cloud(6, 64, 2, seed=3), {0: hc[0], -1: hc[H - 1]}


def oracle_chains(kind):
    """float64 stitched and unstitched chains and the float32 stitched chain of the free-running test, once per process (CPU seconds)."""
    if kind not in _CHAIN:
        from test_gpu_shapes import shape_weights
        T, noise, scene, pins = chain_inputs(kind)
        sched, _steps, _pv = chain_sched(T, kind)
        out = {}
        for name, dtype, on in (("s64", np.float64, True), ("u64", np.float64, False), ("s32", np.float32, True)):
            uo = O.UNetOracle(shape_weights(4, H, False, 0, 16), 4, H, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            table = dict(CHAIN, alpha=ST.blend_weights(CHAIN["O"], 'ramp'), pins=pins)
            so = StitchOracle(uo, T, 2.0, dtype=dtype, sched=sched, stitch=table) if on else O.SamplerOracle(uo, T, 2.0, dtype=dtype, sched=sched)
            lat = uo.encode_scene(scene)
            out[name] = so.ddpm(noise, {}, lat) if kind == "ddpm" else so.ddim(noise[0], {}, lat, K=5)
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """(bar, float32 oracle's distance, stitched-vs-unstitched distance of the final float64 states): what the inputs must satisfy."""
    c = oracle_chains(kind)
    bar = 1e-4 * float(np.abs(c["s64"]).max())
    return bar, float(np.abs(c["s32"] - c["s64"]).max()), float(np.abs(c["s64"][-1] - c["u64"][-1]).max())


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_stitched_chain(kind):
    """The 3-iteration DDPM job (T = 3, cosine schedule) and the 5-step DDIM job (T = 25) of the guide's chain test at the smallest network, one
    chain of W = 2 windows with O = 2 (L = 14), pins {0: start, -1: goal}, through run_inference_stitched: every state of the windows against the
    float64 StitchOracle chain at the project's standing bar, 1e-4 of max |x|.  The inputs keep the float32 oracle within a quarter of that
    bar (checked here and in test_stitch_host.py), and the float64 final state differs from the unstitched chain of the same rows and noise by
    >= 100 x the bar: the test cannot pass with the stitch missing."""
    c = oracle_chains(kind)
    bar, d32, moved = chain_conditions(kind)
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    T, noise, scene, pins = chain_inputs(kind)
    dm = small_model(T=T, sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential")
    with NoiseInjector(list(noise)):
        long, windows = dm.run_inference_stitched(dev(scene), {k: torch.from_numpy(v) for k, v in pins.items()}, CHAIN["W"], CHAIN["O"], n_samples=1,
                                                  blend='ramp', return_chain=True, return_windows=True, noise_std_extra_schedule_fn=lambda x: 0.5)
    windows, long = windows.cpu().numpy(), long.cpu().numpy()
    assert windows.shape == c["s64"].shape and long.shape == (windows.shape[0], 1, 14, 4)
    err = float(np.abs(windows - c["s64"]).max())
    print(f"stitched {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {d32:.2e}; stitched vs unstitched {moved:.2e}); mode {dm.last_job_mode}")
    assert err <= bar
    for j in range(long.shape[0]):
        assert np.array_equal(bits(long[j]), bits(ST.assemble_reference(windows[j], CHAIN["W"], CHAIN["O"])))
    assert np.array_equal(long[-1, 0, 0], pins[0]) and np.array_equal(long[-1, 0, -1], pins[-1])


# ------------------------------------------------------------------------------------------------ 6: graph hygiene
def test_a_stitched_job_never_replays_a_stale_graph():
    """Jobs of one shape back to back on one context with use_graph = 1: another blend table, then other pin values, then another overlap --
    each equals its own use_graph = 0 run bit for bit (and differs from its predecessor)."""
    S, Cn, W = 4, 2, 2
    noise = synth.make_noise((26, Cn * W, H, S), seed=5)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    hc = hcn(S)
    pa = {0: torch.from_numpy(hc[0]), -1: torch.from_numpy(hc[H - 1])}
    pb = {0: torch.from_numpy(hc[0] * np.float32(0.5)), -1: torch.from_numpy(hc[H - 1])}
    jobs = [(2, 'ramp', pa), (2, 'mean', pa), (2, 'mean', pb), (3, 'mean', pb)]

    def run(dm, Ov, blend, pins):
        with NoiseInjector(list(noise)):
            return dm.run_inference_stitched(scene, pins, W, Ov, n_samples=Cn, blend=blend, return_chain=True, return_windows=True,
                                             noise_std_extra_schedule_fn=lambda x: 0.5)[1]

    graph, eager = small_model(sampler="ddpm", use_graph=True), small_model(sampler="ddpm", use_graph=False)
    prev = None
    for j in jobs:
        a, b = run(graph, *j), run(eager, *j)
        assert torch.equal(a, b), j[:2]
        assert prev is None or not torch.equal(a, prev)
        prev = a
    assert torch.equal(run(graph, *jobs[-1]), prev)      # (and a replay of the same job is the same job)


def test_philox_noise_through_the_python_layer():
    """noise_source='philox': the job draws its own noise and stitches it in the context's buffer -- graph and eager runs of the same seed agree
    bit for bit, the windows agree on their overlaps, and the next job (the stream has advanced) is another draw."""
    S, Cn, W, Ov = 4, 2, 2, 2
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    hc = hcn(S)
    pins = {0: torch.from_numpy(hc[0]), -1: torch.from_numpy(hc[H - 1])}
    res = []
    for use_graph in (True, False):
        dm = small_model(T=3, sampler="ddpm", schedule="cosine", use_graph=use_graph, noise_source="philox", noise_seed=5)
        res.append([dm.run_inference_stitched(scene, pins, W, Ov, n_samples=Cn, return_chain=True, return_windows=True,
                                              noise_std_extra_schedule_fn=lambda x: 0.5)[1] for _ in range(2)])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and not torch.equal(res[0][0], res[0][1])
    v = res[0][0].cpu().numpy().reshape(4, Cn, W, H, S)
    assert np.isfinite(v).all() and np.array_equal(bits(v[:, :, 0, H - Ov:]), bits(v[:, :, 1, :Ov]))


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_of_the_job_entry_and_the_python_layer():
    """Every refusal of ramp_sample_stitched is a host check made before anything launches: non-zero, the entry's name in ramp_last_error, the
    launch counter untouched, the output as it was.  The Python layer's NotImplementedError / ValueError list."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    S, Cn, W, Ov = 4, 2, 2, 2
    B = Cn * W
    dm = small_model(S)
    steps = [24, 12, 0]
    arrays, keep = _HostArrays(), []
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    tab, batch, ts = prepare(dm, [scene], Cn, W, Ov)
    noise = dev(synth.make_noise((4, B, H, S), seed=8))
    out = torch.full((B, H, S), 7.0, device="cuda")
    hard = {0: torch.zeros(B, S, device="cuda")}
    pins = {0: uniform((S,), 1), -1: uniform((S,), 2)}

    def refused(st, p=None, cg=None):
        p = p if p is not None else raw_params(dm, B, steps, arrays, False)
        n0 = dm.model.launch_count()
        rc = lib.ramp_sample_stitched(dm.model.ctx(), C.byref(p), C.byref(st), C.byref(cg) if cg is not None else None, C.byref(batch),
                                      _lib.ptr(noise), None, _lib.ptr(out), None, _lib.current_stream())
        msg = lib.ramp_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "ramp_sample_stitched" in msg, (rc, msg)
        assert dm.model.launch_count() == n0 and float(out.min()) == 7.0 and float(out.max()) == 7.0
        return msg

    def table(**kw):
        st = stitch_table(keep, kw.pop("W", W), kw.pop("Ov", Ov), kw.pop("blend", 'ramp'), kw.pop("pins", pins), Cn, S)
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    assert "n_windows" in refused(table(n_windows=0))
    assert "multiple" in refused(table(n_windows=3, overlap=2))
    for bad in (0, 5, -1):
        assert "overlap" in refused(table(overlap=bad))
    for bad in (-0.25, 1.5, float("nan"), float("inf")):
        assert "alpha" in refused(table(blend=[0.5, bad]))
    assert "alpha" in refused(table(alpha_host=None))
    assert "n_pin" in refused(table(n_pin=65)) and "n_pin" in refused(table(n_pin=-1))
    for bad in (14, -1):      # L = 14
        assert "pin index" in refused(table(pin_idx_host=C.cast((C.c_int32 * 2)(0, bad), _lib.c_i32p)))
    assert "pin table" in refused(table(pin_val=None)) and "pin table" in refused(table(pin_idx_host=None))
    assert "n_hard" in refused(table(), p=raw_params(dm, B, steps, arrays, False, hard=hard))
    sharded = raw_params(dm, B, steps, arrays, False)
    sharded.noise_mode, sharded.philox_total = 1, 2 * B
    assert "shard" in refused(table(), p=sharded)
    # what ramp_sample_guided refuses, under this entry's name
    gcloud = dev(uniform((50, 2), 91))
    assert "n_guide" in refused(table(), cg=raw_guide(arrays, [gcloud], [1, 17, 1], [0.01] * 3))
    assert "n_scenes" in refused(table(), cg=raw_guide(arrays, [gcloud, gcloud], [1] * 3, [0.01] * 3))
    assert lib.ramp_sample_stitched(None, None, None, None, None, None, None, None, None, None) != 0
    assert "ramp_sample_stitched" in lib.ramp_last_error().decode()
    # ... and the accepted table does run
    _, ok, _ = run_stitched(dm, raw_params(dm, B, steps, arrays, False), table(), batch, noise, 3, chain=False)
    assert np.isfinite(ok.cpu().numpy()).all()
    # the kernel-level entries
    x = torch.zeros((B, H, S), device="cuda")
    assert lib.ramp_stitch_windows(_lib.ptr(x), Cn, W, H, S, C.byref(table(overlap=5)), None) != 0
    assert "ramp_stitch_windows" in lib.ramp_last_error().decode() and "overlap" in lib.ramp_last_error().decode()
    assert lib.ramp_stitch_windows(_lib.ptr(x), Cn, 3, H, S, C.byref(table()), None) != 0 and "ramp_stitch_windows" in lib.ramp_last_error().decode()
    assert lib.ramp_stitch_assemble(_lib.ptr(x), Cn, W, H, S, 5, _lib.ptr(x), None) != 0 and "ramp_stitch_assemble" in lib.ramp_last_error().decode()
    assert lib.ramp_stitch_assemble(_lib.ptr(x), Cn, W, H, S, Ov, None, None) != 0 and "ramp_stitch_assemble" in lib.ramp_last_error().decode()
    # the Python layer
    tp = {k: torch.from_numpy(v) for k, v in pins.items()}
    with pytest.raises(ValueError, match="overlap"):
        dm.run_inference_stitched(scene, tp, 2, 5)
    with pytest.raises(ValueError, match="scenes for 2 windows"):
        dm.run_inference_stitched([scene] * 3, tp, 2, 2)
    with pytest.raises(ValueError, match="outside the long trajectory"):
        dm.run_inference_stitched(scene, {14: tp[0]}, 2, 2)
    with pytest.raises(ValueError, match="blend"):
        dm.run_inference_stitched(scene, tp, 2, 2, blend='cubic')
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        dm.run_inference_stitched(scene, tp, 2, 2, blend=[0.5, 1.5])
    with pytest.raises(NotImplementedError, match="mcmc"):
        dm.run_inference_stitched(scene, tp, 2, 2, mcmc=dict(kind='ula'))
    with pytest.raises(NotImplementedError, match="resample"):
        dm.run_inference_stitched(scene, tp, 2, 2, resample=dict(every=1))

    def my_step(*a, **k):
        raise AssertionError("never called")
    for sampler in ("ddpm", "ddim"):
        with pytest.raises(NotImplementedError, match="sample_fn"):
            small_model(sampler=sampler).run_inference_stitched(scene, tp, 2, 2, sample_fn=my_step)
    dm.set_noise_shard(0, 8)
    with pytest.raises(NotImplementedError, match="shard"):
        dm.run_inference_stitched(scene, tp, 2, 2)
    dm.set_noise_shard(None)
    from ramp_amd.models import DynamicGaussianDiffusionModel
    dyn = DynamicGaussianDiffusionModel(model=dm.model, n_diffusion_steps=25, predict_epsilon=True)
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dyn.run_inference_stitched(scene, tp, 2, 2)
    cmp_ = small_model()
    cmp_.compose = True
    with pytest.raises(NotImplementedError, match="compose"):
        cmp_.run_inference_stitched(scene, tp, 2, 2)
