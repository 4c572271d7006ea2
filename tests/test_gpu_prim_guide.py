"""The swept box and sphere terms of the cost guide on the device: the kernels alone (``ramp_guide_step_prims``, ``ramp_guide_cost_prims``)
against the numpy restatement of tests/prim_guide_ref.py, the designed cases fed to ``ramp_traj_clearance`` (the guide closes the gap between
what it pushes on and what is counted), the exact statements, the wiring into ``ramp_sample_guided_prims``, a free-running chain against the
float64 oracle, stale graphs, the Python entry and the refusals.

float64 is the truth and the same restatement in float32 the yardstick: every bar that is not an exact statement is 4 x the float32
restatement's distance from the float64 one on the test's own inputs, measured on the CPU inside the test, never from the HIP output.  The
kernel rounds margin, band, w_prim and the step to fp32 once; the tests hand over fp32-representable values."""
import ctypes as C

import numpy as np
import pytest
import torch

import prim_guide_ref as R
import test_gpu_guide as G
from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from ramp_amd.diffusion import guide_tables
from ramp_amd.spec import UNET_DIM_MULTS
from util import NoiseInjector, dev

pytestmark = pytest.mark.gpu

F32 = R.F32


def t_pair(pair):
    return None if pair is None else (dev(pair[0]), dev(pair[1]))


def run_step(x, scenes, ts, pins, k, step, n_iter, max_norm, radius=0.0):
    """ramp_guide_step_prims through ramp_amd.guide.prim_guide_step on the restatement's inputs."""
    from ramp_amd.guide import prim_guide_step
    one = len(scenes) == 1 and ts is None
    boxes = [t_pair(s.get("boxes")) for s in scenes]
    spheres = [t_pair(s.get("spheres")) for s in scenes]
    clouds = [s.get("cloud") for s in scenes]
    cl = None
    if any(c is not None for c in clouds):
        d = next(c.shape[1] for c in clouds if c is not None)
        cl = [dev(c if c is not None else np.zeros((0, d), np.float32)) for c in clouds]
    y = prim_guide_step(dev(x), boxes[0] if one else boxes, spheres[0] if one else spheres, band=k["band"], step=step, margin=k["margin"],
                        w_prim=k.get("w_prim", 1.0), n_sub=k["n_sub"], cloud_or_clouds=cl, radius=k.get("radius", radius), w_obs=k.get("w_obs", 0.0),
                        w_smooth=k.get("w_smooth", 0.0), w_acc=k.get("w_acc", 0.0), n_steps=n_iter, max_norm=max_norm,
                        hard_conds={h: dev(np.ascontiguousarray(v)) for h, v in pins.items()}, traj_scene=None if ts is None else dev(ts))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run_terms(x, scenes, ts, k, radius=0.0):
    from ramp_amd.guide import prim_guide_terms
    one = len(scenes) == 1 and ts is None
    boxes = [t_pair(s.get("boxes")) for s in scenes]
    spheres = [t_pair(s.get("spheres")) for s in scenes]
    out = prim_guide_terms(dev(x), boxes[0] if one else boxes, spheres[0] if one else spheres, band=k["band"], margin=k["margin"], n_sub=k["n_sub"],
                           traj_scene=None if ts is None else dev(ts), radius=radius)
    torch.cuda.synchronize()
    return out.cpu().numpy()


CASE_ID = lambda c: "H%d_S%d_d%d_n%d_b%d_s%d_it%d_clip%d_band%g" % c      # noqa: E731


# ------------------------------------------------------------------------------------------------ 1: the kernels against float64
@pytest.mark.parametrize("case", R.OP_CASES, ids=CASE_ID)
def test_step_against_float64(case):
    """B = 5 paths over two scenes (the second without primitives) and one scene index outside the table, pins at both ends and in the
    middle with values of their own, w_prim 1, w_smooth 0.5, w_acc 0.25, margin 0.03, step 0.05.  Bar: 4 x the float32 restatement's
    largest distance from the float64 one on these inputs (2.8e-8 .. 1.3e-7 over the cases, printed).  The row outside the table, the
    pinned waypoints and the channels >= D keep their bits."""
    c = R.op_case(case)
    d32 = float(np.abs(c["y32"] - c["y64"]).max())
    assert d32 > 0 and c["prim_g"] > 0 and c["kink"] > 1e-4
    y = run_step(c["x"], c["scenes"], c["ts"], c["pins"], c["k"], R.OP_STEP, c["n_iter"], c["max_norm"])
    err = float(np.abs(y - c["y64"]).max())
    print(f"prim guide step {case}: HIP {err:.2e}, float32 restatement {d32:.2e} (bar {4 * d32:.2e}); moved {np.abs(c['y64'] - c['x']).max():.2e}; "
          f"HIP vs the float32 restatement {np.abs(y - c['y32']).max():.2e}")
    assert err <= 4 * d32
    xb, yb = c["x"].view(np.uint32), y.view(np.uint32)
    assert np.array_equal(yb[3], xb[3])
    assert np.array_equal(yb[:, c["idx"]], xb[:, c["idx"]]) and np.array_equal(yb[:, :, c["D"]:], xb[:, :, c["D"]:])


@pytest.mark.parametrize("case", R.OP_CASES, ids=CASE_ID)
def test_cost_against_float64(case):
    """ramp_guide_cost_prims on the same inputs: C_prim (column 3) against the float64 restatement, bar 4 x the float32 restatement's largest
    distance over the rows; columns 0 .. 2 are ramp_guide_cost's bits; NaN for the row outside the table."""
    from ramp_amd.guide import cost_guide_terms
    c = R.op_case(case)
    D, k = c["D"], c["k"]
    got = run_terms(c["x"], c["scenes"], c["ts"], k)
    assert got.shape == (R.OP_B, 4) and got.dtype == np.float64 and np.isnan(got[3]).all()
    rows = [b for b in range(R.OP_B) if b != 3]
    want = np.array([R.prim_cost(c["x"][b, :, :D].astype(np.float64), c["scenes"][c["ts"][b]], k["margin"], k["band"], k["n_sub"]) for b in rows])
    f32 = np.array([R.prim_cost(c["x"][b, :, :D], c["scenes"][c["ts"][b]], k["margin"], k["band"], k["n_sub"]) for b in rows])
    d32, err = float(np.abs(f32 - want).max()), float(np.abs(got[rows, 3] - want).max())
    print(f"prim guide cost {case}: HIP {err:.2e}, float32 restatement {d32:.2e} (bar {4 * d32:.2e}); C_prim {np.round(want, 5).tolist()}; "
          f"HIP vs the float32 restatement {np.abs(got[rows, 3] - f32).max():.2e}")
    assert want.max() > 0 and (want[[1]] == 0).all() and (got[1, 3] == 0)      # (scene 1 has no primitive)
    assert err <= 4 * d32
    empty = [dev(np.zeros((0, D), np.float32))] * 2
    base = cost_guide_terms(dev(c["x"]), empty, 0.3, traj_scene=dev(c["ts"])).cpu().numpy()
    assert np.array_equal(got[:, :3].view(np.uint64), base.view(np.uint64))


def test_cost_columns_with_a_cloud_are_the_cost_guides_bits():
    """With a cloud in the table columns 0 .. 2 equal ramp_guide_cost's, bit for bit (2-D and 3-D, a cloud past one tile)."""
    from ramp_amd.guide import cost_guide_terms, prim_guide_terms
    for S, D in ((4, 2), (6, 3)):
        x = G.uniform((3, 48, S), 50 + D)
        cloud = dev(G.uniform((1100, D), 51))
        box = (dev(np.zeros((1, D), np.float32)), dev(np.full((1, D), 0.5, np.float32)))
        got = prim_guide_terms(dev(x), box, None, band=F32(0.05), cloud_or_clouds=cloud, radius=G.RADIUS).cpu().numpy()
        base = cost_guide_terms(dev(x), cloud, G.RADIUS).cpu().numpy()
        assert (base > 0).all() and got[:, 3].max() > 0
        assert np.array_equal(got[:, :3].view(np.uint64), base.view(np.uint64))


# ------------------------------------------------------------------------------------------------ 2: the exact statements
@pytest.mark.parametrize("S,D", [(4, 2), (6, 3)])
def test_without_primitives_it_is_the_cost_guide_bit_for_bit(S, D):
    """No primitive in the scene, an empty table, or w_prim = 0: ramp_guide_step's output, bit for bit, with a real cloud term, stencils,
    pins and a clip; and a trajectory's result is the same bits alone and inside its batch."""
    from ramp_amd.guide import cost_guide_step
    H = 48
    x = G.uniform((4, H, S), 60 + D)
    clouds = [G.uniform((300, D), 61), G.uniform((1100, D), 62)]
    ts = np.array([0, 1, 1, 0], np.int32)
    idx = [0, 7, H - 1]
    val = G.uniform((3, 4, S), 63)
    pins = {h: val[i] for i, h in enumerate(idx)}
    w = dict(w_obs=1.0, w_smooth=0.5, w_acc=0.25, radius=G.RADIUS)
    base = cost_guide_step(dev(x), [dev(c) for c in clouds], G.RADIUS, F32(2e-3), w_obs=1.0, w_smooth=0.5, w_acc=0.25, n_steps=3, max_norm=F32(2.0),
                           hard_conds={h: dev(v) for h, v in pins.items()}, traj_scene=dev(ts)).cpu().numpy()
    assert float(np.abs(base - x).max()) > 1e-3
    rng = np.random.default_rng(64)
    boxes = (rng.uniform(-0.8, 0.8, (70, D)).astype(np.float32), rng.uniform(0.1, 0.4, (70, D)).astype(np.float32))
    k = dict(margin=F32(0.03), band=F32(0.05), n_sub=4, **w)
    none = [dict(boxes=None, spheres=None, cloud=clouds[0]), dict(boxes=None, spheres=None, cloud=clouds[1])]
    some = [dict(boxes=boxes, spheres=None, cloud=clouds[0]), dict(boxes=None, spheres=None, cloud=clouds[1])]
    y_none = run_step(x, none, ts, pins, dict(k, w_prim=1.0), F32(2e-3), 3, F32(2.0))
    y_zero = run_step(x, some, ts, pins, dict(k, w_prim=0.0), F32(2e-3), 3, F32(2.0))
    y_some = run_step(x, some, ts, pins, dict(k, w_prim=1.0), F32(2e-3), 3, F32(2.0))
    assert np.array_equal(y_none.view(np.uint32), base.view(np.uint32)) and np.array_equal(y_zero.view(np.uint32), base.view(np.uint32))
    # scene 1 has no primitive: its rows are the cost guide's even inside the primitive kernel; scene 0's rows differ
    assert np.array_equal(y_some[[1, 2]].view(np.uint32), base[[1, 2]].view(np.uint32))
    assert not np.array_equal(y_some[0], base[0]) and not np.array_equal(y_some[3], base[3])
    for b in range(4):
        alone = run_step(x[b:b + 1], some, ts[b:b + 1], {h: v[b:b + 1] for h, v in pins.items()}, dict(k, w_prim=1.0), F32(2e-3), 3, F32(2.0))
        assert np.array_equal(alone.view(np.uint32), y_some[b:b + 1].view(np.uint32)), b


@pytest.mark.parametrize("name", sorted(R.exact_cases()))
def test_exact_cases(name):
    """A sample exactly at a sphere's centre (a waypoint, and the midpoint of a segment): cost, no gradient, the trajectory keeps its bits.  A
    sample inside a box on an axis tie: the lowest axis alone moves, away from the centre, by exactly the float32 restatement's amount;
    sign(0) = +1."""
    c = R.exact_cases()[name]
    y = run_step(c["x"], [c["scene"]], None, {}, c["k"], c["step"], 1, 0.0)
    want = R.iterate(c["x"], [c["scene"]], None, {}, c["k"], c["step"], 1, 0.0, np.float32, c["D"])
    assert np.array_equal((y != c["x"]), c["moves"]) and np.array_equal(y.view(np.uint32), want.view(np.uint32))
    cost = run_terms(c["x"], [c["scene"]], None, c["k"])
    ref = R.prim_cost(c["x"][0, :, :c["D"]], c["scene"], c["k"]["margin"], c["k"]["band"], c["k"]["n_sub"])
    assert ref > 0 and cost[0, 3] == ref


# ------------------------------------------------------------------------------------------------ 3: the guide closes the gap
@pytest.mark.parametrize("kind,D", [("box", 2), ("box", 3), ("sphere", 2)])
def test_designed_cases_through_the_clearance_kernel(kind, D):
    """The issue's designed cases: the kernel's output goes to ramp_traj_clearance with the same margin.  At the start no waypoint is hit and
    one segment is.  n_sub = 1 (the guide sees waypoints only) leaves that swept hit: 1 -> 1 (the box case bit-unchanged).  n_sub = 8 clears
    it in 16 iterations: 1 -> 0.  Both outputs also agree with the float64 restatement at 4 x the float32 one's distance."""
    from ramp_amd.clearance import trajectory_clearance
    m = R.DESIGN["margin"]

    def hits(traj, scene):
        cl = trajectory_clearance(dev(np.ascontiguousarray(traj)), t_pair(scene["boxes"]), t_pair(scene["spheres"]), point_dim=D, margin=m)
        return int(cl.wp_hits.cpu()[0]), int(cl.seg_hits.cpu()[0])

    for n_sub, seg_after in ((1, 1), (8, 0)):
        x, y64, scene = R.design_run(kind, D, n_sub, np.float64)
        y32 = R.design_run(kind, D, n_sub, np.float32)[1]
        H = R.DESIGN["H"]
        k = dict(margin=m, band=R.DESIGN["band"], w_prim=R.DESIGN["w_prim"], n_sub=n_sub)
        y = run_step(x, [scene], None, {0: x[0, 0], H - 1: x[0, H - 1]}, k, R.DESIGN["step"], R.DESIGN["n_iter"], 0.0)
        assert hits(x, scene) == (0, 1)
        assert hits(y, scene) == (0, seg_after), (kind, D, n_sub)
        d32, err = float(np.abs(y32 - y64).max()), float(np.abs(y - y64).max())
        print(f"designed {kind} {D}-D n_sub={n_sub}: seg_hits 1 -> {seg_after}; HIP {err:.2e}, float32 restatement {d32:.2e}; min phi along the path "
              f"{R.min_phi(y[0, :, :D], scene, m, 64):+.4f}")
        assert err <= 4 * d32
        if kind == "box" and n_sub == 1:
            assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
        else:
            assert float(np.abs(y - x).max()) > 1e-3


# ------------------------------------------------------------------------------------------------ the smallest network
def raw_prims(arrays, boxes, spheres, n_scenes, D, margin, band, w_prim=1.0, n_sub=4):
    from ramp_amd.guide import fill_prim_guide, prim_scalars, prim_table
    tab = arrays.keep(prim_table(boxes, spheres, n_scenes, D, "cuda"))
    return fill_prim_guide(tab, prim_scalars(margin, band, w_prim, n_sub))


def wire_prims(D, seed):
    rng = np.random.default_rng(seed)
    boxes = (rng.uniform(-0.9, 0.9, (40, D)).astype(np.float32), rng.uniform(0.2, 0.5, (40, D)).astype(np.float32))
    spheres = (rng.uniform(-0.9, 0.9, (30, D)).astype(np.float32), rng.uniform(0.1, 0.25, 30).astype(np.float32))
    return boxes, spheres


WIRE_K = dict(margin=F32(0.05), band=F32(0.1), n_sub=4, w_prim=1.0)


# ------------------------------------------------------------------------------------------------ 4: wiring, bit-exact
@pytest.mark.parametrize("job,kind", [(j, s) for s in ("ddpm", "ddim") for j in ("plain", "scenes")])
def test_wiring_is_the_kernel_on_the_unguided_output(job, kind):
    """A one-iteration job, B = 4, injected noise whose step slot is zero (test_gpu_guide.py's construction): ramp_sample_guided_prims equals
    ramp_guide_step_prims applied to the unguided job's output, bit for bit, as a plain job and as a 2-scene job whose second scene has
    spheres only; with pg == NULL it is ramp_sample_guided, bit for bit."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    S, D, B, H = 4, 2, 4, 8
    ddim = kind == "ddim"
    dm = G.small_model(S, False, sampler=kind)
    steps = [0] if ddim else [12]
    arrays = _HostArrays()
    noise = synth.make_noise((2, B, H, S), seed=90)
    noise[1] = 0
    noise = dev(noise)
    hc = {k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in G.hct(S).items()}
    ctx, s = dm.model.ctx(), _lib.current_stream()
    dm.model.prepare_time_table(25)
    batch = ts = None
    bx, sp = wire_prims(D, 70)
    gclouds = [dev(G.uniform((300, D), 91))]
    scenes = [dict(boxes=bx, spheres=sp, cloud=gclouds[0].cpu().numpy())]
    if job == "scenes":
        sj, hc, Bc = dm._prepare_scene_job([dev(synth.make_cloud(5, 64, 2, seed=31)), dev(synth.make_cloud(4, 64, 2, seed=32))], [G.hct(S)] * 2, [1, 3])
        assert Bc == B
        batch = _lib.RampSceneBatch(); batch.n_scenes, batch.traj_scene = 2, _lib.ptr(sj["traj_scene"])
        ts = sj["traj_scene"].cpu().numpy()
        gclouds = [dev(G.uniform((70, D), 92)), dev(G.uniform((1100, D), 93))]
        scenes = [dict(boxes=bx, spheres=None, cloud=gclouds[0].cpu().numpy()), dict(boxes=None, spheres=wire_prims(D, 71)[1], cloud=gclouds[1].cpu().numpy())]
    else:
        dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
    p = G.raw_params(dm, B, steps, arrays, ddim, hard=hc)
    cg = G.raw_guide(arrays, gclouds, [2], [G.WIRE_STEP], max_norm=G.WIRE_MAX)
    pg = raw_prims(arrays, [t_pair(sc["boxes"]) for sc in scenes], [t_pair(sc["spheres"]) for sc in scenes], len(scenes), D, WIRE_K["margin"],
                   WIRE_K["band"], n_sub=WIRE_K["n_sub"])

    def run(entry):
        out = torch.empty((B, H, S), device="cuda")
        bt = C.byref(batch) if batch is not None else None
        if entry == "prims" or entry == "prims-null":
            rc = lib.ramp_sample_guided_prims(ctx, C.byref(p), C.byref(cg), C.byref(pg) if entry == "prims" else None, None, None, bt, _lib.ptr(noise),
                                              None, None, None, _lib.ptr(out), None, s)
        else:
            rc = lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg) if entry == "guided" else None, None, None, bt, _lib.ptr(noise), None, None, None,
                                        _lib.ptr(out), None, s)
        _lib.check(rc, entry)
        torch.cuda.synchronize()
        return out

    plain, guided, null, prims = run("plain"), run("guided"), run("prims-null"), run("prims")
    assert torch.equal(null, guided) and not torch.equal(guided, plain)
    k = dict(WIRE_K, w_obs=1.0, w_smooth=0.5, w_acc=0.25, radius=G.RADIUS)
    want = run_step(plain.cpu().numpy(), scenes, ts, {h: v.cpu().numpy() for h, v in hc.items()}, k, G.WIRE_STEP, 2, G.WIRE_MAX)
    moved = float(np.abs(want - guided.cpu().numpy()).max())
    print(f"wiring {job} {kind}: the primitive term moved the guided output by {moved:.2e}")
    assert moved > 1e-3 and np.isfinite(want).all()
    assert np.array_equal(prims.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5: a free-running chain against float64
CHAIN_SCENE = dict(boxes=(np.float32([[-0.35, 0.3], [0.4, -0.35], [0.05, 0.6]]), np.float32([[0.5, 0.4], [0.45, 0.5], [0.4, 0.3]])),
                   spheres=(np.float32([[0.3, 0.35], [-0.4, -0.3]]), np.float32([0.25, 0.3])), cloud=None)
CHAIN_K = dict(margin=F32(0.05), band=F32(0.1), n_sub=4, w_prim=1.0)
CHAIN_GUIDE = dict(cloud=None, w_obs=0.0, step=F32(0.25), n_steps=2, max_norm=F32(4.0))
_CHAIN = {}


class PrimOracle(G.GuideOracle):
    """GuideOracle with the primitive term in the guide's place (the header's: behind the posterior mean / x0, before the update)."""

    def _guide(self, v, j, hard_conds):
        if self.guide is None or self.guide["tab"]["n_guide"][j] == 0:
            return v
        t = self.guide["tab"]
        k = dict(CHAIN_K, w_obs=t["w_obs"], w_smooth=t["w_smooth"], w_acc=t["w_acc"], radius=t["radius"])
        return R.iterate(v, [CHAIN_SCENE], None, hard_conds, k, np.float32(t["step"][j]), t["n_guide"][j], t["max_norm"], self.dt, 2)


def chain_guide():
    return dict(CHAIN_GUIDE, boxes=t_pair_cpu(CHAIN_SCENE["boxes"]), spheres=t_pair_cpu(CHAIN_SCENE["spheres"]), margin=CHAIN_K["margin"],
                band=CHAIN_K["band"], n_sub=CHAIN_K["n_sub"])


def t_pair_cpu(pair):
    return (torch.from_numpy(pair[0]), torch.from_numpy(pair[1]))


def oracle_chains(kind):
    """float64 guided and unguided chains and the float32 guided chain, once per process (seconds on the CPU)."""
    if kind not in _CHAIN:
        from test_gpu_shapes import shape_weights
        T, noise, _, scene = G.chain_inputs(kind)
        sched, steps, pv = G.chain_sched(T, kind)
        tab = guide_tables(dict(chain_guide(), t_start=steps[0]), steps, pv)
        assert tab["n_guide"] == [0] + [2] * (len(steps) - 1) and tab["prim"]["n_sub"] == 4
        out = {}
        for name, dtype, guide in (("g64", np.float64, True), ("u64", np.float64, False), ("g32", np.float32, True)):
            uo = O.UNetOracle(shape_weights(4, 8, False, 0, 16), 4, 8, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0], dtype=dtype)
            so = PrimOracle(uo, T, 2.0, dtype=dtype, sched=sched, guide=dict(cloud=None, tab=tab) if guide else None)
            lat = uo.encode_scene(scene)
            out[name] = so.ddpm(noise, G.hcn(4), lat) if kind == "ddpm" else so.ddim(noise[0], G.hcn(4), lat, K=5)
        _CHAIN[kind] = out
    return _CHAIN[kind]


def chain_conditions(kind):
    """(bar, float32 oracle's distance, guided-vs-unguided distance of the final float64 states): what the inputs must satisfy."""
    c = oracle_chains(kind)
    bar = 1e-4 * float(np.abs(c["g64"]).max())
    return bar, float(np.abs(c["g32"] - c["g64"]).max()), float(np.abs(c["g64"][-1] - c["u64"][-1]).max())


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_free_running_guided_chain(kind):
    """test_gpu_guide.py's free-running jobs (3-iteration DDPM, 5-step DDIM, the smallest network, B = 2) with the primitives-only guide
    -- cost_guide=dict(cloud=None, w_obs=0, boxes=, spheres=, band=, ...), on from the second iteration, two iterations each -- through
    run_inference: every state against the float64 oracle chain at the project's standing bar, 1e-4 of max |x|.  The inputs keep the float32
    oracle within a quarter of that bar, and the guided and unguided float64 final states lie >= 100 bars apart (both asserted here and in
    test_prim_guide_host.py): the test cannot pass with the term missing."""
    c = oracle_chains(kind)
    bar, d32, moved = chain_conditions(kind)
    assert d32 <= bar / 4 and moved >= 100 * bar, (bar, d32, moved)
    T, noise, _, scene = G.chain_inputs(kind)
    dm = G.small_model(T=T, sampler=kind, schedule="cosine" if kind == "ddpm" else "exponential")
    steps = dm._ddpm_steps()[0] if kind == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    with NoiseInjector(list(noise)):
        chain = dm.run_inference(None, G.hct(4), n_samples=2, horizon=8, return_chain=True, obstacle_pts=dev(scene),
                                 noise_std_extra_schedule_fn=lambda x: 0.5, cost_guide=dict(chain_guide(), t_start=steps[0])).cpu().numpy()
    assert chain.shape == c["g64"].shape
    err = float(np.abs(chain - c["g64"]).max())
    print(f"prim-guided {kind} chain vs float64: {err:.2e} (bar {bar:.2e}; float32 oracle {d32:.2e}; guided vs unguided {moved:.2e}); mode {dm.last_job_mode}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ 6: graph hygiene and the Python entry
def test_a_job_with_primitives_never_replays_a_stale_graph():
    """Jobs of one shape back to back on one context with use_graph = 1: other centres with the same counts (replayed, and honoured), another
    band, another n_sub, then other counts -- each equals its own use_graph = 0 run bit for bit and differs from its predecessor."""
    B, H, S = 3, 8, 4
    noise = synth.make_noise((26, B, H, S), seed=5)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    (bx_a, sp_a), (bx_b, sp_b) = wire_prims(2, 80), wire_prims(2, 81)
    base = dict(cloud=None, w_obs=0.0, w_smooth=0.5, step=F32(0.05), n_steps=2, t_start=10, max_norm=F32(4.0), margin=F32(0.05), band=F32(0.1), n_sub=4)
    jobs = [dict(base, boxes=t_pair(bx_a), spheres=t_pair(sp_a)), dict(base, boxes=t_pair(bx_b), spheres=t_pair(sp_b)),
            dict(base, boxes=t_pair(bx_b), spheres=t_pair(sp_b), band=F32(0.05)), dict(base, boxes=t_pair(bx_b), spheres=t_pair(sp_b), band=F32(0.05), n_sub=8),
            dict(base, boxes=t_pair((bx_b[0][:7], bx_b[1][:7])), spheres=t_pair(sp_b), band=F32(0.05), n_sub=8),
            dict(base, boxes=t_pair((bx_b[0][:7], bx_b[1][:7])), spheres=None, band=F32(0.05), n_sub=8)]

    def run(dm, g):
        with NoiseInjector(list(noise)):
            return dm.run_inference(None, G.hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene,
                                    noise_std_extra_schedule_fn=lambda x: 0.5, cost_guide=g)

    graph, eager = G.small_model(use_graph=True), G.small_model(use_graph=False)
    prev = None
    for g in jobs:
        a, b = run(graph, g), run(eager, g)
        assert torch.equal(a, b)
        assert prev is None or not torch.equal(a, prev)
        prev = a
    assert torch.equal(run(graph, jobs[-1]), prev)      # (and a replay of the same job is the same job)


def test_the_python_entry_reaches_the_c_entrys_bits():
    """run_inference(cost_guide=dict(cloud=None, w_obs=0, boxes=, band=, step=)) equals ramp_sample_guided_prims called with the same tables,
    schedule and noise, bit for bit (T = 25 DDPM, B = 3, the whole chain)."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    B, H, S = 3, 8, 4
    dm = G.small_model()
    steps = dm._ddpm_steps()[0]
    noise = synth.make_noise((len(steps) + 1, B, H, S), seed=5)
    scene = dev(synth.make_cloud(6, 64, 2, seed=3))
    bx, _ = wire_prims(2, 80)
    g = dict(cloud=None, w_obs=0, boxes=t_pair(bx), band=F32(0.1), step=F32(0.05))
    with NoiseInjector(list(noise)):
        py = dm.run_inference(None, G.hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene, noise_std_extra_schedule_fn=lambda x: 0.5,
                              cost_guide=g)
    with NoiseInjector(list(noise)):
        off = dm.run_inference(None, G.hct(S), n_samples=B, horizon=H, return_chain=True, obstacle_pts=scene, noise_std_extra_schedule_fn=lambda x: 0.5)
    assert not torch.equal(py, off)
    arrays = _HostArrays()
    tab = guide_tables(g, steps, dm.posterior_variance)
    assert tab["n_guide"] == [1] * len(steps) and tab["prim"] == dict(margin=0.0, band=F32(0.1), w_prim=1.0, n_sub=4)
    p = G.raw_params(dm, B, steps, arrays, False, hard={k: v.cuda().unsqueeze(0).expand(B, -1).contiguous() for k, v in G.hct(S).items()})
    cg = G.raw_guide(arrays, [dev(np.zeros((0, 2), np.float32))], tab["n_guide"], tab["step"], w=(0.0, 0.0, 0.0), radius=0.0)
    pg = raw_prims(arrays, t_pair(bx), None, 1, 2, 0.0, F32(0.1))
    out = torch.empty((len(steps) + 1, B, H, S), device="cuda")
    _lib.check(lib.ramp_sample_guided_prims(dm.model.ctx(), C.byref(p), C.byref(cg), C.byref(pg), None, None, None, _lib.ptr(dev(noise)), None, None,
                                            _lib.ptr(out), None, None, _lib.current_stream()), "ramp_sample_guided_prims")
    torch.cuda.synchronize()
    assert torch.equal(out, py)


def test_example_guides_against_its_own_obstacles(tmp_path):
    """examples/inference3d.py --guide-obstacles on injected noise (T = 25, 3 samples): without the flag the run is what it was (the same
    bits twice); with it the chain keeps those bits up to the first guided reverse step (t < t_start_guide = 2: the last two), leaves them
    there, and ends with less than half the C_prim against the experiment's own boxes and spheres."""
    import examples.inference3d as ex
    from ramp_amd.guide import prim_guide_terms
    argv = ["--make-synthetic", str(tmp_path), "--n-samples", "3"]
    noise = synth.make_noise((26, 3, 48, 6), seed=12)
    chains = []
    for extra in ([], [], ["--guide-obstacles"]):
        with NoiseInjector(list(noise)):
            chains.append(ex.main(argv + extra)[1])
    assert bool(torch.isfinite(chains[0]).all()) and torch.equal(chains[0], chains[1])
    assert torch.equal(chains[2][:24], chains[0][:24]) and not torch.equal(chains[2][24], chains[0][24])
    data = ex.Dataset3dView(str(tmp_path / "data" / ex.Config3d.dataset_subdir / "0"), ex.Config3d())
    g = ex.obstacle_guide(data.item, data.normalizer)
    cost = [float(prim_guide_terms(c[-1], g["boxes"], g["spheres"], band=g["band"], margin=g["margin"], n_sub=g["n_sub"])[:, 3].sum())
            for c in (chains[0], chains[2])]
    print(f"example: C_prim of the final batch {cost[0]:.4f} without the guide, {cost[1]:.4f} with it")
    assert cost[0] > 0 and cost[1] < 0.5 * cost[0]


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_of_the_job_entry():
    """Every refusal of ramp_sample_guided_prims is a host check made before anything launches: non-zero, the entry's name in
    ramp_last_error, the launch counter untouched, the output as it was."""
    from ramp_amd.diffusion import _HostArrays
    lib = _lib.load()
    dm = G.small_model()
    B, H, S, steps = 2, 8, 4, [24, 12, 0]
    dm.model.prepare_time_table(25)
    dm._prepare_scene(dev(synth.make_cloud(6, 64, 2, seed=3)), B)
    arrays = _HostArrays()
    noise = dev(synth.make_noise((4, B, H, S), seed=8))
    p = G.raw_params(dm, B, steps, arrays, False)
    ctx, s = dm.model.ctx(), _lib.current_stream()
    out = torch.full((B, H, S), 7.0, device="cuda")
    bx, sp = wire_prims(2, 80)
    cg = G.raw_guide(arrays, [dev(G.uniform((50, 2), 91))], [1, 1, 1], [0.01] * 3)
    ts = dev(np.zeros(B, np.int32))

    def refused(pg, guide=cg, batch=None):
        n0 = dm.model.launch_count()
        rc = lib.ramp_sample_guided_prims(ctx, C.byref(p), C.byref(guide) if guide is not None else None, C.byref(pg), None, None,
                                          C.byref(batch) if batch is not None else None, _lib.ptr(noise), None, None, None, _lib.ptr(out), None, s)
        msg = lib.ramp_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and "ramp_sample_guided_prims" in msg, (rc, msg)
        assert dm.model.launch_count() == n0 and float(out.min()) == 7.0 and float(out.max()) == 7.0
        return msg

    def prims(D=2, n_scenes=1, **kw):
        b3 = (np.zeros((2, D), np.float32), np.ones((2, D), np.float32))
        pg = raw_prims(arrays, [t_pair(b3 if D == 3 else bx)] * n_scenes, [t_pair(sp) if D == 2 else None] * n_scenes, n_scenes, D, 0.05, 0.02)
        for k, v in kw.items():
            setattr(pg, k, v)
        return pg

    assert "cost guide" in refused(prims(), guide=None)
    assert "point_dim" in refused(prims(point_dim=1)) and "differs from the cost guide" in refused(prims(D=3))
    assert "n_sub" in refused(prims(n_sub=0)) and "n_sub" in refused(prims(n_sub=9))
    for k in ("margin", "band"):
        for bad in (-0.01, float("nan"), float("inf")):
            assert "margin and band" in refused(prims(**{k: bad}))
    assert "w_prim" in refused(prims(w_prim=float("nan")))
    assert "offsets" in refused(prims(box_offset_host=None))
    assert "offsets" in refused(prims(sphere_offset_host=C.cast(arrays.keep((C.c_int32 * 2)(1, 30)), _lib.c_i32p)))
    assert "box" in refused(prims(box_sizes=None)) and "sphere" in refused(prims(sphere_centers=None))
    assert "n_scenes" in refused(prims(n_scenes=2))                                  # the guide has one scene
    two = G.raw_guide(arrays, [dev(G.uniform((50, 2), 91))] * 2, [1, 1, 1], [0.01] * 3)
    assert "n_scenes" in refused(prims(n_scenes=2), guide=two)                        # ... and the job has no scene batch
    batch3 = _lib.RampSceneBatch(); batch3.n_scenes, batch3.traj_scene = 3, _lib.ptr(ts)
    assert "n_scenes" in refused(prims(n_scenes=2), guide=two, batch=batch3)
    assert "radius" in refused(prims(), guide=G.raw_guide(arrays, [dev(G.uniform((50, 2), 91))], [1, 1, 1], [0.01] * 3, radius=0.0))
    # what is allowed: an empty table is ramp_sample_guided itself
    none = raw_prims(arrays, None, None, 1, 2, 0.05, 0.02)
    _lib.check(lib.ramp_sample_guided_prims(ctx, C.byref(p), C.byref(cg), C.byref(none), None, None, None, _lib.ptr(noise), None, None, None,
                                            _lib.ptr(out), None, s), "ramp_sample_guided_prims")
    ref = torch.empty_like(out)
    _lib.check(lib.ramp_sample_guided(ctx, C.byref(p), C.byref(cg), None, None, None, _lib.ptr(noise), None, None, None, _lib.ptr(ref), None, s),
               "ramp_sample_guided")
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and float(out.max()) != 7.0
    # the Python layer: stitched windows and the potential take no primitives
    g = dict(cloud=None, w_obs=0, boxes=t_pair(bx), band=0.02, step=0.5)
    with pytest.raises(NotImplementedError, match="run_inference_stitched"):
        dm.run_inference_stitched(dev(synth.make_cloud(6, 64, 2, seed=3)), {}, 2, 2, cost_guide=g)
    with pytest.raises(NotImplementedError, match="resample="):
        dm.run_inference(None, G.hct(S), n_samples=1, obstacle_pts=dev(synth.make_cloud(6, 64, 2, seed=3)), cost_guide=g,
                         resample=dict(every=1, lambda_=1.0, cloud=None, w_obs=0.0, w_smooth=1.0))
