"""Warm-started sampling jobs on the device: the two kernels against the numpy definition (``ramp_amd.warm``) bit for bit, "no prior is the
plain job", "a uniform level is the plain machinery on the tail of the schedule", mixed levels (held rows, hooks, hard conditions), free-running
chains against float64 (``warm_ref.WarmOracle``), stale graphs, and the Python layer with its refusals.

Everything runs on the smallest network (unet_input_dim 16, dim_mults (1, 2, 4), H = 8).  Only the free-running test carries a tolerance, the
project's standing 1e-4 of max |x| of the float64 chain; test_warm_host.py checks on the CPU that its inputs keep the float32 oracle within a
quarter of that bar and move the warm rows by >= 100 x the bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import warm_ref as R
from ramp_amd import _lib, synth
from ramp_amd.diffusion import _HostArrays, guide_tables
from ramp_amd.warm import straight_line_prior, warm_hold_reference, warm_init_reference, warm_tables
from test_gpu_guide import RADIUS, hcn, hct, raw_guide, raw_params, small_model, uniform
from util import NoiseInjector, dev

pytestmark = pytest.mark.gpu

F32 = lambda v: float(np.float32(v))      # noqa: E731
H = 8


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).view(np.uint32)


def sched_of(dm):
    return dm.sqrt_alphas_cumprod.cpu().numpy(), dm.sqrt_one_minus_alphas_cumprod.cpu().numpy()


def hard_np(x, hc):
    x = x.copy()
    for k, v in hc.items():
        x[:, k] = v
    return x


def x_init_np(dm, noise0, prior, t_row, hc):
    sa, s1a = sched_of(dm)
    return hard_np(warm_init_reference(noise0, prior, t_row, sa, s1a), hc)


def raw_ws(arrays, dm, prior, tab):
    """ramp_warm_start from ``warm_tables`` and a numpy (B, H, S) prior."""
    sa, s1a = sched_of(dm)
    has = tab["t_row"] >= 0
    t = np.where(has, tab["t_row"], 0)
    ws = _lib.RampWarmStart()
    ws.prior, ws.n_hold = _lib.ptr(arrays.keep(dev(prior))), int(tab["n_hold"])
    ws.j0_host, ws.has_prior_host = arrays.i32(tab["j0"]), arrays.i32(has)
    ws.sa_host, ws.s1a_host = arrays.f32(sa[t]), arrays.f32(s1a[t])
    return ws


def warm_entry(dm, p, ws, noise, B, S, cg=None, batch=None, rs=None, tg=None, st=None):
    """ramp_sample_warm with the options the tests use -> (chain, x)."""
    lib = _lib.load()
    opt = lambda v: C.byref(v) if v is not None else None      # noqa: E731
    chain = torch.empty((p.n_steps + 1, B, H, S), device="cuda")
    x = torch.empty((B, H, S), device="cuda")
    rc = lib.ramp_sample_warm(dm.model.ctx(), C.byref(p), opt(ws), opt(st), opt(rs), opt(cg), None, opt(tg), None, None, opt(batch), _lib.ptr(noise),
                              None, None, None, _lib.ptr(chain), _lib.ptr(x), None, None, None, None, None, None, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, chain, x


def line_prior(B, S, seed=1700):
    hc = hcn(S)
    line = straight_line_prior(hc[0], hc[H - 1], H)
    return (line[None] + 0.05 * np.random.default_rng(seed).standard_normal((B, H, S))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: the ops are the definition
@pytest.mark.parametrize("B,Hh,S", [(1, 8, 4), (5, 8, 6), (3, 48, 4)])
def test_ops_are_the_definition_bit_for_bit(B, Hh, S):
    """ramp_warm_init / ramp_warm_hold against warm_init_reference / warm_hold_reference: rows with and without a prior, levels at both ends
    of the schedule (t = 0 and t = T - 1) and in between, j below, at and above j0, with and without a chain block; the rows in front of and
    behind the arrays (guard rows of one buffer) and every row the hold does not name keep their bytes, and so do noise, prior and x_init."""
    lib = _lib.load()
    T, sched, _ = R.chain_sched("ddim")
    sa, s1a = sched["sqrt_alphas_cumprod"], sched["sqrt_one_minus_alphas_cumprod"]
    rng = np.random.default_rng(100 + B)
    noise, prior = rng.standard_normal((B, Hh, S)).astype(np.float32), rng.standard_normal((B, Hh, S)).astype(np.float32)
    noise[0, 0, 0] = -0.0
    f32p, i32p = (lambda a: a.ctypes.data_as(_lib.c_f32p)), (lambda a: a.ctypes.data_as(_lib.c_i32p))
    for rot in range(2):
        t_row = np.array(([-1, 0, T - 1, 10, -1] if rot == 0 else [T - 1, -1, 0, 5, 10])[:B], np.int32)
        prior_in = prior.copy()
        prior_in[t_row < 0] = np.nan                      # a row without a prior is never read
        has = np.ascontiguousarray((t_row >= 0).astype(np.int32))
        ts = np.where(t_row >= 0, t_row, 0)
        sar, s1ar = np.ascontiguousarray(sa[ts]), np.ascontiguousarray(s1a[ts])
        want = warm_init_reference(noise, prior_in, t_row, sa, s1a)
        buf = torch.full((B + 2, Hh, S), 7.25, device="cuda")
        dn, dp = dev(noise), dev(prior_in)
        _lib.check(lib.ramp_warm_init(_lib.ptr(buf[1:B + 1]), _lib.ptr(dn), _lib.ptr(dp), f32p(sar), f32p(s1ar), i32p(has), B, Hh, S,
                                      _lib.current_stream()), "ramp_warm_init")
        got = buf.cpu().numpy()
        assert np.array_equal(bits(got[1:B + 1]), bits(want)), rot
        assert (got[0] == 7.25).all() and (got[-1] == 7.25).all()
        assert np.array_equal(bits(dn), bits(noise)) and np.array_equal(bits(dp), bits(prior_in))
        inplace = dev(noise)                               # x may be noise0 itself
        _lib.check(lib.ramp_warm_init(_lib.ptr(inplace), _lib.ptr(inplace), _lib.ptr(dp), f32p(sar), f32p(s1ar), i32p(has), B, Hh, S,
                                      _lib.current_stream()), "ramp_warm_init")
        assert np.array_equal(bits(inplace), bits(want))
    # the hold
    x_init = rng.standard_normal((B, Hh, S)).astype(np.float32)
    cur, blk = rng.standard_normal((B, Hh, S)).astype(np.float32), rng.standard_normal((B, Hh, S)).astype(np.float32)
    j0 = np.ascontiguousarray(np.array([0, 2, 3, 1, 0][:B] if B > 1 else [2], np.int32))
    for j in range(4):
        for with_chain in (True, False):
            xb, cb = torch.full((B + 2, Hh, S), 7.25, device="cuda"), torch.full((B + 2, Hh, S), -3.5, device="cuda")
            xb[1:B + 1], cb[1:B + 1] = dev(cur), dev(blk)
            di = dev(x_init)
            _lib.check(lib.ramp_warm_hold(_lib.ptr(xb[1:B + 1]), _lib.ptr(cb[1:B + 1]) if with_chain else None, _lib.ptr(di), i32p(j0), j, B, Hh, S,
                                          _lib.current_stream()), "ramp_warm_hold")
            gx, gc = xb.cpu().numpy(), cb.cpu().numpy()
            assert np.array_equal(bits(gx[1:B + 1]), bits(warm_hold_reference(cur, x_init, j0, j))), (j, with_chain)
            assert np.array_equal(bits(gc[1:B + 1]), bits(warm_hold_reference(blk, x_init, j0, j) if with_chain else blk)), (j, with_chain)
            assert (gx[0] == 7.25).all() and (gx[-1] == 7.25).all() and (gc[0] == -3.5).all() and (gc[-1] == -3.5).all()
            assert np.array_equal(bits(di), bits(x_init))
    assert (j0 > 0).any()


# ------------------------------------------------------------------------------------------------ 2: no prior is the plain job
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_a_job_of_rows_without_a_prior_is_the_plain_job(kind):
    """Every level None: x and the chain are the plain entry's bit for bit -- through the C entry (injected noise) and through
    run_inference(warm_start=) with torch and with Philox noise."""
    lib = _lib.load()
    B, S = 3, 4
    ddim = kind == "ddim"
    dm = small_model(sampler=kind)
    steps = [20, 15, 10, 5, 0] if ddim else [24, 12, 1, 0]
    arrays = _HostArrays()
    noise = dev(synth.make_noise((1 if ddim else len(steps) + 1, B, H, S), seed=8))
    dm.model.prepare_time_table(25)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    dm._prepare_scene(scene, B)
    p = raw_params(dm, B, steps, arrays, ddim, hard={k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hct(S).items()})
    tab = warm_tables([None] * B, steps, T=25)
    ws = raw_ws(arrays, dm, np.full((B, H, S), np.nan, np.float32), tab)
    chain0, x0 = torch.empty((len(steps) + 1, B, H, S), device="cuda"), torch.empty((B, H, S), device="cuda")
    _lib.check(lib.ramp_sample(dm.model.ctx(), C.byref(p), _lib.ptr(noise), _lib.ptr(chain0), _lib.ptr(x0), _lib.current_stream()), "ramp_sample")
    torch.cuda.synchronize()
    for w in (ws, None):      # (and ws == NULL is the plain entry too)
        rc, chain1, x1 = warm_entry(dm, p, w, noise, B, S)
        _lib.check(rc, "ramp_sample_warm")
        assert np.isfinite(chain0.cpu().numpy()).all()
        assert torch.equal(chain0, chain1) and torch.equal(x0, x1) and torch.equal(chain1[-1], x1)
    for src in ("torch", "philox"):
        res = []
        for kw in ({}, dict(warm_start=dict(prior=None, level=None)), dict(warm_start=dict(prior=torch.zeros(B, H, S), level=[None] * B))):
            m = small_model(sampler=kind, noise_source=src, noise_seed=5)
            torch.manual_seed(3)
            res.append(m.run_inference(None, hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene,
                                       noise_std_extra_schedule_fn=lambda t: 0.5, **kw))
        assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), src
        assert m.last_warm["J"] == 0 and m.last_warm["j0"].tolist() == [0] * B and m.last_warm["t_row"].tolist() == [-1] * B


# ------------------------------------------------------------------------------------------------ 3: a uniform level is the tail of the plain job
UNIFORM_CASES = ["ddpm", "ddim", "scenes_apf", "guided", "3d"]


@pytest.mark.parametrize("case", UNIFORM_CASES)
def test_a_uniform_level_is_the_plain_machinery_on_the_tail(case):
    """run_inference*(warm_start=dict(prior, level)) under injected noise equals, bit for bit, the plain C entry run through raw params on
    steps_full[J:] with noise[0] replaced by warm_init_reference's array -- chain and final state.  What indexes the FULL list: the DDPM
    noise scales (a schedule function that depends on t: the tail's scales are f(t_J ..), not f(t_0 ..)) and the APF switch of the
    many-scene job (level 7 at T = 25 gives J = 17; ``j > 20`` fires on the job's iterations 4 .. 7 -- under job-local indexing it would
    never fire, and the test checks that the flags change the bits).  The guide's table is keyed by timestep (t < 6)."""
    lib = _lib.load()
    o3, ddim = case == "3d", case == "ddim"
    S, B = (6, 3) if o3 else (4, 3)
    dm = small_model(S, o3, sampler="ddim" if ddim else "ddpm", use_apf=case == "scenes_apf")
    level = 12 if ddim else 7
    steps_full = [int(i) for i in dm.ddim_set_timesteps(5)] if ddim else dm._ddpm_steps()[0]
    tab = warm_tables([level] * B, steps_full, T=25)
    J = tab["J"]
    assert (J, tab["n_hold"]) == ((2, 0) if ddim else (17, 0))
    tail = steps_full[J:]
    n1 = len(tail)
    prior = line_prior(B, S)
    noise = synth.make_noise((1 if ddim else n1 + 1, B, H, S), seed=31)
    scale_fn = lambda t: 0.3 + 0.02 * float(t)      # noqa: E731
    scales_tail = [F32(scale_fn(t)) for t in tail]
    scene = synth.make_cloud(4, 30, 3, seed=41) if o3 else synth.make_cloud(6, 64, 2, seed=3)
    hc_np = hcn(S)
    gcloud = uniform((300, 2), 91)
    guide = dict(cloud=dev(gcloud), radius=RADIUS, step=F32(4e-3), w_smooth=0.5, w_acc=0.25, n_steps=2, t_start=6, max_norm=F32(4.0))
    kw = dict(return_chain=True, noise_std_extra_schedule_fn=scale_fn, warm_start=dict(prior=prior, level=level))
    scenes = [dev(synth.make_cloud(5, 64, 2, seed=31)), dev(np.concatenate([synth.make_cloud(4, 64, 2, seed=32),
                                                                             line_prior(1, 4)[0][None, :, :2].repeat(4, 0)], 1))]
    if case == "scenes_apf":
        dm.apf_ddpm = dict(dm.apf_ddpm, threshold=0.3)
    # ---- the warm job, through the Python layer
    with NoiseInjector(list(noise)):
        if case == "scenes_apf":
            got, _ts = dm.run_inference_scenes(scenes, [hct(S)] * 2, n_samples=[1, 2], **kw)
        else:
            got = dm.run_inference(None, hct(S), n_samples=B, horizon=H, obstacle_pts=dev(scene), **(dict(kw, cost_guide=guide) if case == "guided" else kw))
    assert got.shape == (n1 + 1, B, H, S) and dm.last_warm["J"] == J and dm.last_warm["steps"] == tail
    # ---- the plain entry on the tail, from the reference's start state
    arrays = _HostArrays()
    ref_noise = noise.copy()
    sa, s1a = sched_of(dm)
    ref_noise[0] = warm_init_reference(noise[0], prior, tab["t_row"], sa, s1a)
    ref_noise = dev(ref_noise)
    batch = None
    if case == "scenes_apf":
        sj, hcc, Bc = dm._prepare_scene_job(scenes, [hct(S)] * 2, [1, 2])
        assert Bc == B
        batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(sj["traj_scene"])
        hard = hcc
    else:
        dm._prepare_scene(dev(scene), B)
        hard = {k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hct(S).items()}
    p = raw_params(dm, B, tail, arrays, ddim, hard=hard)
    if not ddim:
        p.noise_scale = arrays.f32(scales_tail)
    ctx, s = dm.model.ctx(), _lib.current_stream()

    def plain(apf_flags=None):
        chain, x = torch.empty((n1 + 1, B, H, S), device="cuda"), torch.empty((B, H, S), device="cuda")
        if case == "scenes_apf":
            p.apply_apf = arrays.i32(apf_flags)
            if any(apf_flags):
                dm._fill_apf(p, arrays, dict(dm.apf_ddpm, passes=1), None, batch, sj)
            else:
                batch.cloud_points, batch.cloud_offset_host = None, None
            rc = lib.ramp_sample_scenes(ctx, C.byref(p), C.byref(batch), _lib.ptr(ref_noise), _lib.ptr(chain), _lib.ptr(x), s)
        elif case == "guided":
            gt = guide_tables(dict(guide, cloud=gcloud), tail, dm.posterior_variance)
            assert gt["n_guide"] == [0, 0] + [2] * 6
            cg = raw_guide(arrays, [dev(gcloud)], gt["n_guide"], gt["step"], w=(1.0, 0.5, 0.25), max_norm=F32(4.0))
            rc = lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg), None, None, None, _lib.ptr(ref_noise), None, None, _lib.ptr(chain), _lib.ptr(x),
                                        None, s)
        else:
            rc = lib.ramp_sample(ctx, C.byref(p), _lib.ptr(ref_noise), _lib.ptr(chain), _lib.ptr(x), s)
        _lib.check(rc, "plain entry")
        torch.cuda.synchronize()
        return chain, x

    if case == "scenes_apf":
        full_flags = [1 if j > 20 else 0 for j in range(25)][J:]
        assert full_flags == [0, 0, 0, 0, 1, 1, 1, 1]
        want, x = plain(full_flags)
        off, _ = plain([0] * n1)                 # job-local indexing (j > 20 never fires in 8 iterations) would give this
        assert not torch.equal(want[5], off[5]) and torch.equal(want[:5], off[:5])
    else:
        want, x = plain()
    assert np.isfinite(want.cpu().numpy()).all() and torch.equal(want[-1], x)
    assert np.array_equal(bits(want[0]), bits(x_init_np(dm, noise[0], prior, tab["t_row"], hc_np)))
    assert torch.equal(got, want)
    if not ddim and case != "scenes_apf":      # the scales of the tail, not those of the list's head: the head's give other bits
        p.noise_scale = arrays.f32([F32(scale_fn(t)) for t in steps_full[:n1]])
        head, _ = plain()
        assert not torch.equal(head, want)


# ------------------------------------------------------------------------------------------------ 4: mixed levels
def mixed_model(kind, **kw):
    return small_model(T=3 if kind == "ddpm" else 25, sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential", **kw)


@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_mixed_levels_hold_rows_until_their_level(kind):
    """B = 3, levels [None, 12, 5] (DDIM, K = 5: j0 = [0, 2, 3]) / [None, 1, 0] (DDPM, T = 3 cosine: j0 = [0, 1, 2]), a cost guide on EVERY
    iteration: chain block 0 is the numpy x_init; a held row equals it bit for bit in every block up to j0 (the guide ran on it and left
    nothing) and has moved in block j0 + 1; the hard-conditioned waypoints hold in every block; chain[-1] is x_out; the row without a prior
    starts where the cold job's row does, and the rows with one end elsewhere."""
    S, B = 4, 3
    noise, scene, hc_np, prior = R.chain_inputs(kind)
    dm = mixed_model(kind)
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    tab = warm_tables(R.CHAIN_LEVELS[kind], steps, T=dm.n_diffusion_steps)
    guide = dict(cloud=dev(uniform((300, 2), 91)), radius=RADIUS, step=F32(4e-3), w_smooth=0.5, w_acc=0.25, n_steps=2, max_norm=F32(4.0))
    hc = {k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in hct(S).items()}
    draws = list(noise) if kind == "ddpm" else [noise[0]]

    def run(**kw):
        with NoiseInjector(draws):
            x, chain = dm.conditional_sample(hc, batch_size=B, return_chain=True, obstacle_pts=dev(scene), noise_std_extra_schedule_fn=lambda t: 0.5,
                                             cost_guide=guide, **kw)
        return x, chain.permute(1, 0, 2, 3).contiguous()

    x, chain = run(warm_start=dict(prior=prior, level=R.CHAIN_LEVELS[kind]))
    _, cold = run()
    assert chain.shape == (len(steps) + 1, B, H, S) and np.isfinite(chain.cpu().numpy()).all()
    assert dm.last_warm["j0"].tolist() == R.CHAIN_J0[kind] and dm.last_warm["J"] == 0
    x_init = x_init_np(dm, noise[0], prior, tab["t_row"], hc_np)
    assert np.array_equal(bits(chain[0]), bits(x_init))
    for b, j0 in enumerate(R.CHAIN_J0[kind]):
        for j in range(j0 + 1):
            assert np.array_equal(bits(chain[j, b]), bits(x_init[b])), (b, j)
        assert not torch.equal(chain[j0 + 1, b], chain[0, b]), b
    for k, v in hc_np.items():
        assert np.array_equal(bits(chain[:, :, k]), bits(np.broadcast_to(v, (len(steps) + 1, B, S)).copy())), k
    assert torch.equal(chain[-1], x)
    assert torch.equal(chain[0, 0], cold[0, 0]) and not torch.equal(chain[-1, 1:], cold[-1, 1:])


# ------------------------------------------------------------------------------------------------ 5: free-running chains against float64
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
def test_free_running_warm_chain(kind):
    """The jobs of test 4 without the guide through run_inference(warm_start=, return_chain=True) under NoiseInjector: every state against
    the float64 WarmOracle chain at the project's standing bar, 1e-4 of max |x|.  The inputs keep the float32 oracle within a quarter of
    that bar and the float64 warm and cold final states of the rows with a prior differ by >= 100 x the bar (checked here and in
    test_warm_host.py): the test cannot pass with the init or the hold missing."""
    c = R.oracle_chains(kind)
    bar, d32, moved = R.chain_conditions(kind)
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    noise, scene, hc_np, prior = R.chain_inputs(kind)
    dm = mixed_model(kind)
    with NoiseInjector(list(noise) if kind == "ddpm" else [noise[0]]):
        chain = dm.run_inference(None, hct(4), n_samples=3, horizon=H, return_chain=True, obstacle_pts=dev(scene),
                                 noise_std_extra_schedule_fn=lambda t: 0.5, warm_start=dict(prior=prior, level=R.CHAIN_LEVELS[kind])).cpu().numpy()
    assert chain.shape == c["w64"].shape
    err = float(np.abs(chain - c["w64"]).max())
    print(f"warm {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {d32:.2e}; warm vs cold {moved:.2e}); mode {dm.last_job_mode}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 6: no stale graph, launch counts
def test_a_warm_job_never_replays_a_stale_graph():
    """On one context with graphs: a warm job, the same with other levels at equal n_hold (one graph: levels are data), a job with another J,
    a plain job, the first again -- each equals its eager run bit for bit and differs from its predecessor.  The launch count of a job
    follows n_hold alone: mixed minus uniform-at-the-same-J is n_hold launches, and B = 3 and B = 5 launch alike."""
    S = 4
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    noise0 = synth.make_noise((1, 5, H, S), seed=44)
    prior = line_prior(5, S)
    jobs = [dict(level=[None, 12, 5]), dict(level=[7, None, 12]), dict(level=12), None, dict(level=[None, 12, 5])]

    def run(dm, w, B=3):
        kw = {} if w is None else dict(warm_start=dict(w, prior=prior[:B]))
        with NoiseInjector([noise0[0, :B]]):
            out = dm.run_inference(None, hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene, **kw)
        n = C.c_int64(0)
        _lib.check(_lib.load().ramp_launch_count(dm.model.ctx(), C.byref(n)), "ramp_launch_count")
        return out, n.value

    graph, eager = small_model(sampler="ddim", use_graph=True), small_model(sampler="ddim", use_graph=False)
    outs, counts = [], []
    for w in jobs:
        (a, na), (b, nb) = run(graph, w), run(eager, w)
        assert torch.equal(a, b), w
        assert not outs or a.shape != outs[-1].shape or not torch.equal(a, outs[-1])
        outs.append(a); counts.append(nb)      # (a replayed graph launches nothing anew: the eager context counts)
    assert torch.equal(outs[0], outs[-1]) and counts[0] == counts[-1] == counts[1]      # n_hold 3 both times
    assert [o.shape[0] for o in outs] == [6, 6, 4, 6, 6]
    _, uniform20 = run(eager, dict(level=20))      # J = 0, n_hold = 0
    assert counts[0] - uniform20 == 3
    _, five = run(eager, dict(level=[None, 12, 5, 5, 12]), B=5)
    assert five == counts[0]


# ------------------------------------------------------------------------------------------------ 7: the Python layer
def test_philox_noise_and_last_warm():
    """A warm job that draws its own noise takes (n' + 1) blocks of the Philox stream; last_warm holds J, j0, t_row and the job's steps."""
    dm = small_model(noise_source="philox", noise_seed=9)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    prior = line_prior(3, 4)
    chain = dm.run_inference(None, hct(4), n_samples=3, horizon=H, return_chain=True, obstacle_pts=scene,
                             warm_start=dict(prior=prior, level=[5, 3, 5])).cpu().numpy()
    assert chain.shape == (7, 3, H, 4) and np.isfinite(chain).all()
    assert dm.last_philox[2] == 7 * 3 * H * 4
    lw = dm.last_warm
    assert lw["J"] == 19 and lw["j0"].tolist() == [0, 2, 0] and lw["t_row"].tolist() == [5, 3, 5] and lw["steps"] == [5, 4, 3, 2, 1, 0]
    assert np.array_equal(chain[1, 1], chain[0, 1]) and np.array_equal(chain[2, 1], chain[0, 1]) and not np.array_equal(chain[3, 1], chain[0, 1])
    again = small_model(noise_source="philox", noise_seed=9).run_inference(None, hct(4), n_samples=3, horizon=H, return_chain=True, obstacle_pts=scene,
                                                                            warm_start=dict(prior=prior, level=[5, 3, 5])).cpu().numpy()
    assert np.array_equal(again, chain)


def test_per_scene_levels_and_a_long_prior():
    """run_inference_scenes with one level per scene: the held scene's rows keep x_init until their level.  run_inference_stitched with a long
    prior at a uniform level: the windows agree on their overlaps, bit for bit, in every chain block."""
    S = 4
    dm = small_model(sampler="ddim")
    scenes = [dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))]
    line = line_prior(1, S)[0]
    with NoiseInjector([synth.make_noise((3, H, S), seed=45)]):
        chain, ts = dm.run_inference_scenes(scenes, [hct(S)] * 2, n_samples=[1, 2], return_chain=True,
                                            warm_start=dict(prior=[line, line + np.float32(0.01)], level=[None, 5]))
    assert ts.tolist() == [0, 1, 1] and dm.last_warm["j0"].tolist() == [0, 3, 3] and chain.shape == (6, 3, H, S)
    for b in (1, 2):
        for j in range(4):
            assert torch.equal(chain[j, b], chain[0, b]), (b, j)
        assert not torch.equal(chain[4, b], chain[0, b])
    assert not torch.equal(chain[1, 0], chain[0, 0])
    # stitched: W = 3 windows of 8 with overlap 2 -> L = 20
    W, O, Cn = 3, 2, 2
    hc = hcn(S)
    long_line = straight_line_prior(hc[0], hc[H - 1], 20)
    long_prior = (long_line[None] + 0.05 * np.random.default_rng(3).standard_normal((Cn, 20, S))).astype(np.float32)
    with NoiseInjector([synth.make_noise((Cn * W, H, S), seed=46)]):
        long, windows = dm.run_inference_stitched(dev(synth.make_cloud(6, 64, 2, seed=3)), {0: torch.from_numpy(hc[0]), -1: torch.from_numpy(hc[H - 1])}, W, O,
                                                  n_samples=Cn, return_chain=True, return_windows=True, warm_start=dict(prior=long_prior, level=12))
    assert dm.last_warm["J"] == 2 and windows.shape == (4, Cn * W, H, S) and long.shape == (4, Cn, 20, S)
    assert np.isfinite(windows.cpu().numpy()).all()
    for c in range(Cn):
        for w in range(W - 1):
            assert torch.equal(windows[:, c * W + w, H - O:], windows[:, c * W + w + 1, :O]), (c, w)
    with pytest.raises(NotImplementedError, match="stitched"):
        dm.run_inference_stitched(dev(synth.make_cloud(6, 64, 2, seed=3)), {0: torch.from_numpy(hc[0])}, W, O, n_samples=Cn,
                                  warm_start=dict(prior=long_prior, level=[12, 5]))


def test_refusals_of_the_entry_and_the_python_layer():
    """NotImplementedError: mixed levels with resample= and with team=, a caller-supplied sample_fn.  ValueError: a level outside [0, T - 1], a
    non-finite prior, a wrong shape, start= below a row's start.  The C entry refuses malformed tables by name, before any launch."""
    S, B = 4, 4
    dm = small_model()
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    prior = line_prior(B, S)
    gcloud = dev(uniform((300, 2), 91))
    call = lambda **kw: dm.run_inference(None, hct(S), n_samples=B, horizon=H, obstacle_pts=scene, **kw)      # noqa: E731
    mixed = dict(prior=prior, level=[None, 5, 5, 3])
    with pytest.raises(NotImplementedError, match="resample"):
        call(warm_start=mixed, resample=dict(every=2, lambda_=1.0, cloud=gcloud, radius=RADIUS))
    with pytest.raises(NotImplementedError, match="team"):
        call(warm_start=mixed, cost_guide=dict(cloud=gcloud, radius=RADIUS, step=F32(4e-3), team=dict(size=2, radius=0.2)))
    with pytest.raises(NotImplementedError, match="sample_fn"):
        call(warm_start=mixed, sample_fn=lambda *a, **k: None)
    for bad in (dict(prior=prior, level=25), dict(prior=prior, level=[0, 1, 2, -1]), dict(prior=np.full((B, H, S), np.nan, np.float32), level=3),
                dict(prior=prior[:3], level=3), dict(prior=prior[:, :4], level=3), dict(prior=prior, level=[5, 5, 12, 12], start=5)):
        with pytest.raises(ValueError):
            call(warm_start=bad)
    # the C entry
    arrays = _HostArrays()
    steps = [24, 12, 1, 0]
    dm.model.prepare_time_table(25)
    dm._prepare_scene(scene, B)
    p = raw_params(dm, B, steps, arrays, False)
    noise = dev(synth.make_noise((5, B, H, S), seed=8))
    good = warm_tables([None, 12, 12, 1], steps, T=25)
    assert good["j0"].tolist() == [0, 1, 1, 2]

    def refused(tab, prior_np=prior, **kw):
        ws = raw_ws(arrays, dm, prior_np, tab)
        for k, v in kw.items():
            setattr(ws, k, v)
        rc, _, _ = warm_entry(dm, p, ws, noise, B, S)
        msg = _lib.load().ramp_last_error().decode()
        assert rc != 0 and "ramp_sample_warm" in msg, (rc, msg)
        return msg

    assert "n_hold" in refused(good, n_hold=1)
    assert "n_hold" in refused(good, n_hold=3)
    assert "n_hold" in refused(dict(good, j0=np.array([0, 4, 4, 4], np.int32), n_hold=4))
    assert "without a prior" in refused(dict(good, j0=np.array([2, 1, 1, 2], np.int32)))
    assert "null" in refused(good, prior=None)
    assert "null" in refused(good, j0_host=None)
    rc, chain, x = warm_entry(dm, p, raw_ws(arrays, dm, prior, good), noise, B, S)      # (and the well-formed table runs)
    _lib.check(rc, "ramp_sample_warm")
    assert np.isfinite(chain.cpu().numpy()).all() and torch.equal(chain[-1], x)


def test_mixed_levels_with_inner_steps_and_composed_rows():
    """The other served mixed-level combinations.  mcmc= (ULA, one inner step per iteration): a held row's inner steps are undone by the hold --
    its accept flags are -1 on the iterations before its start and left out of the rate -- and it keeps x_init until then.  A composed job
    with one level per scene: the held scene's rows keep x_init."""
    S, B = 4, 3
    dm = small_model(sampler="ddim")
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    prior = line_prior(B, S)
    with NoiseInjector([synth.make_noise((B, H, S), seed=47)]):
        chain = dm.run_inference(None, hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene,
                                 mcmc=dict(kind="ula", steps=1, step_scale=0.05, noise=dev(synth.make_noise((5, B, H, S), seed=48))),
                                 warm_start=dict(prior=prior, level=[None, 12, 5]))
    acc = dm.last_mcmc["accept"].numpy()
    assert acc.shape == (5, B) and (acc[:, 0] == 1).all()
    assert acc[:, 1].tolist() == [-1, -1, 1, 1, 1] and acc[:, 2].tolist() == [-1, -1, -1, 1, 1]
    assert dm.last_mcmc["rate"] == [1.0] * 5
    for b, j0 in enumerate([0, 2, 3]):
        for j in range(j0 + 1):
            assert torch.equal(chain[j, b], chain[0, b]), (b, j)
        assert not torch.equal(chain[j0 + 1, b], chain[0, b]), b
    sets = [[dev(synth.make_cloud(5, 64, 2, seed=31))], [dev(synth.make_cloud(4, 64, 2, seed=32 + k)) for k in range(2)]]
    with NoiseInjector([synth.make_noise((B, H, S), seed=49)]):
        chain, ts = dm.run_inference_composed(sets, [hct(S)] * 2, n_samples=[1, 2], return_chain=True,
                                              warm_start=dict(prior=prior[0], level=[20, 5]))
    assert dm.last_warm["J"] == 0 and dm.last_warm["j0"].tolist() == [0, 3, 3] and chain.shape == (6, B, H, S)
    assert np.isfinite(chain.cpu().numpy()).all() and not torch.equal(chain[1, 0], chain[0, 0])
    for b in (1, 2):
        assert all(torch.equal(chain[j, b], chain[0, b]) for j in range(4)) and not torch.equal(chain[4, b], chain[0, b])


def test_the_examples_take_a_warm_start(tmp_path):
    """examples/inference_static.py --warm-start line --warm-level 8 (T = 25 DDPM, smallest network): the job runs the 9 iterations from t = 8
    -- 10 chain states -- alone and with --all-envs, and ends on the hard conditions."""
    import examples.inference_static as ex
    cfg = ex.StaticConfig()
    cfg.n_diffusion_steps, cfg.unet_input_dim, cfg.unet_dim_mults_option = 25, 16, 0
    ex.make_synthetic_experiment(str(tmp_path), cfg)
    common = ["--dataset-path", str(tmp_path / "data"), "--trained-models-dir", str(tmp_path / "models"), "--n-samples", "4", "--sampler", "ddpm",
              "--n-diffusion-steps", "25", "--n-steps-without-noise", "0", "--unet-input-dim", "16", "--unet-dim-mults-option", "0",
              "--warm-start", "line", "--warm-level", "8"]
    metrics, runner = ex.main(common + ["--env", "0"])
    assert metrics["n_chain_states"] == 10 and runner.model.last_warm["J"] == 16
    x = runner.last_trajectories
    assert x.shape == (4, 48, 4) and bool(torch.isfinite(x).all())
    assert torch.equal(x[:, 0, :2], torch.tensor([-0.8, -0.8], device="cuda").expand(4, -1))
    per_env, runner = ex.main(common + ["--all-envs"])
    assert len(per_env) == 1 and runner.model.last_warm["steps"] == list(range(8, -1, -1))
    assert runner.last_trajectories.shape == (4, 48, 4) and bool(torch.isfinite(runner.last_trajectories).all())
