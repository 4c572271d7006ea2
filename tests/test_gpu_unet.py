"""Score-network parity on the GPU: HIP forward / energy-gradient vs fixtures captured from the reference
and vs the float64 oracle."""
import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import synth
import util
from util import GOLDEN, build_unet, dev, rel, weights

pytestmark = pytest.mark.gpu

CASES = [("2d_h48", 4, 48, False), ("3d_h48", 6, 48, True), ("3d_h64", 6, 64, True), ("2d_h40", 4, 40, False)]
# every other horizon ramp_create accepts (a multiple of 8 in [8, 64]) and the ends of its state-width range [2, 16]:
# level lengths 8/4/2/1, 16/8/4/2, 24/12/6/3, 32/16/8/4, 56/28/14/7 and 64/32/16/8 (oracle/make_goldens.py horizons)
HORIZON_CASES = [("2d_h8", 4, 8, False), ("3d_h16", 6, 16, True), ("2d_h24", 4, 24, False), ("s3_h32", 3, 32, False),
                 ("s2_h56", 2, 56, False), ("s16_h64", 16, 64, False)]
CASES += HORIZON_CASES


@pytest.mark.parametrize("gemm_mode", ["fp16x3", "fp16x3-fusedff", "fp16x3-ffx", "fp16x3-tok", "fp16x3-atk", "fp16x3-tkc", "fp16x3-tkw", "fp16x3-m32", "bf16x6", "fp32"])
@pytest.mark.parametrize("tag,S,H,o3", CASES)
def test_score_against_reference_fixture(tag, S, H, o3, gemm_mode):
    """forward_no_energy, eps and every per-module output / output-gradient tap of the reference
    (UnetInference.py:157-224), through the reference-style forward(x, time, context, obstacle_pts=...), in every
    arithmetic mode.  fp16x3 (the default, and what the bench times): the first evaluation after a scene change
    calibrates the delayed operand scales on the bf16x6 kernels, so the compared evaluations are the ones after it
    (checked through ramp_score_mode).  "fp16x3-fusedff" forces the one-launch FF1 -> GEGLU -> FF2 kernel and "fp16x3-ffx" the
    token-owning fused feed-forward pair (forward + backward, LayerNorm-3 folded in; ffx.hip) onto these small launches
    through the launch plan (ramp_set_launch_plan); by default they only take the large ones (the full-size tests);
    "fp16x3-tok" adds the token-owning LN1 -> QKV / out-projection / d(o) kernel (tkl.hip), "fp16x3-atk" the self-attention fused with
    its output projection (atk.hip: sample-owning waves; levels whose token count divides 48 or 32, the others keep the pair) =
    "fp16x3-tkc" also the narrow k = 5 convolutions on sample-owning waves (tkc.hip), "fp16x3-tkw" also the wide ones with their GroupNorm +
    Mish (forward) / GroupNorm backward (input gradient) fused (tkw.hip: sample-owning blocks, level lengths dividing 96) = the bench's plan."""
    g = np.load(f"{GOLDEN}/unet{tag}.npz")
    gemm_mode, plan = util.split_mode(gemm_mode)
    m = build_unet(S, H, o3, max_rows=8, debug=True, gemm_mode=gemm_mode, launch_plan=plan)
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    if gemm_mode == "fp16x3":
        assert m.score_mode() == "bf16x6"                      # calibration evaluation
        f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
        assert m.score_mode() == "fp16x3"
    else:
        assert m.score_mode() == gemm_mode
        m.reset_cache()
    eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    if gemm_mode == "fp16x3":
        assert m.score_mode() == "bf16x6"                      # first input-gradient pass: its call sites calibrate
        eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    assert m.score_mode() == gemm_mode
    # tolerance stated by BASELINE.json: 1e-4 relative fp32; measured headroom is ~30x
    assert rel(m.cached_scene_latents[0].cpu().numpy(), g["latent"]) < 5e-6
    # the time embedding itself (TimeEncoder, layers.py:233-259), not only its effect through the residual blocks
    assert rel(m.time_embedding(int(g["t"][0])).cpu().numpy(), g["temb"][0]) < 5e-6
    assert rel(f, g["f"]) < 2e-5
    assert rel(eps, g["eps"]) < 5e-5
    worst = 0.0
    for k in g.files:
        if k.startswith("out/") or k.startswith("gout/"):
            kind, name = k.split("/")
            got = m.debug_read(kind, name, g[k].shape).cpu().numpy()
            worst = max(worst, rel(got, g[k]))
            assert rel(got, g[k]) < 5e-5, k
    print(f"{tag} {gemm_mode}: f {rel(f, g['f']):.2e} eps {rel(eps, g['eps']):.2e} worst tap {worst:.2e}")


def test_score_fp16x3_recalibrates_when_the_operand_range_moves():
    """ramp_score in fp16x3 mode keeps its calibration from call to call; an input 2^14 larger than the one the scales
    were recorded on trips the on-device guard, and the call repeats itself with the bf16x6 kernels: the caller gets the
    bf16x6 answer bitwise, never a flagged one, and the next call is fp16x3 again."""
    g = np.load(f"{GOLDEN}/unet2d_h48.npz")
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    m = build_unet(4, 48, False, max_rows=8, gemm_mode="fp16x3")
    ref = build_unet(4, 48, False, max_rows=8, gemm_mode="bf16x6")
    m(x, t, None, obstacle_pts=pts); m(x, t, None, obstacle_pts=pts)
    assert m.score_mode() == "fp16x3"
    big = x * 16384.0
    got = m(big, t, None, obstacle_pts=pts)
    assert m.score_mode() == "bf16x6"
    assert torch.equal(got, ref(big, t, None, obstacle_pts=pts))
    again = m(big, t, None, obstacle_pts=pts)
    assert m.score_mode() == "fp16x3"
    assert rel(again.cpu().numpy(), got.cpu().numpy()) < 5e-5


def test_scene_cache_is_keyed_on_content():
    """Two different CPU clouds of equal shape back to back (compat.load_environment_dir returns CPU tensors): the
    temporary device copy of the second one lands in the allocator block the first one freed, so a cache keyed on
    (data_ptr, _version) would silently plan against the previous obstacle map."""
    from ramp_amd.models import StaticGaussianDiffusionModel
    u = build_unet(4, 48, False, max_rows=8)
    dm = StaticGaussianDiffusionModel(model=u, n_diffusion_steps=25, predict_epsilon=True, sampler="ddpm").eval().to("cuda")
    hc = {k: torch.from_numpy(v) for k, v in synth.default_hard_conds(4, 48).items()}
    lats = []
    for seed in (3, 4, 3):
        cloud = torch.from_numpy(synth.make_cloud(6, 64, 2, seed=seed))          # CPU tensor, as the loader returns
        dm.run_inference(None, hc, n_samples=2, obstacle_pts=cloud, noise_std_extra_schedule_fn=lambda x: 0.5)
        lats.append(u.cached_scene_latents[0].clone())
    assert not torch.equal(lats[0], lats[1])
    assert torch.equal(lats[0], lats[2])
    n0 = u.launch_count()
    dm.run_inference(None, hc, n_samples=2, obstacle_pts=torch.from_numpy(synth.make_cloud(6, 64, 2, seed=3)),
                     noise_std_extra_schedule_fn=lambda x: 0.5)                  # same content: no re-encode
    assert torch.equal(u.cached_scene_latents[0], lats[0])
    u.reset_cache()
    assert u.scene_cache.key is None


@pytest.mark.parametrize("S,H,o3", [(4, 48, False), (6, 64, True)])
def test_score_chunked_batch_vs_oracle64(S, H, o3):
    """B = 11 trajectories x 2 variants through a context whose capacity (6 rows) forces 4 chunks, at three
    timesteps; compared with the float64 oracle.  Also: rows are independent (a sub-batch reproduces bitwise)."""
    from ramp_amd import _lib
    m = build_unet(S, H, o3, max_rows=6, gemm_mode="bf16x6")   # bitwise row independence: no call-history-dependent scales
    u = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=np.float64)
    cloud = synth.make_cloud(6, 64, 2, seed=3) if not o3 else synth.make_cloud(4, 30, 3, seed=3)
    lat = m.encode_scene(dev(cloud))
    assert rel(lat[0].cpu().numpy(), u.encode_scene(cloud)) < 5e-6
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    B = 11
    x = synth.make_noise((B, H, S), seed=21)
    xd = dev(x)
    for t in (0, 11, 24):
        eps = torch.empty((2 * B, H, S), device="cuda"); f = torch.empty_like(eps)
        _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(xd), B, 2, t, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()))
        lats = np.tile(lat[0].cpu().numpy()[None], (2 * B, 1)); lats[1::2] = 0
        x2 = np.repeat(x, 2, axis=0)
        tt = np.full((2 * B,), t)
        assert rel(f.cpu().numpy(), u.forward_no_energy(x2, tt, lats)) < 2e-5
        assert rel(eps.cpu().numpy(), u.score(x2, tt, lats)) < 5e-5
    sub = torch.empty((2 * 3, H, S), device="cuda")
    _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(xd[4:7].contiguous()), 3, 2, 24, None, _lib.ptr(sub), _lib.current_stream()))
    assert torch.equal(sub, eps[8:14])


# Which sample-owning kernels the bench's plan (fp16x3-tkw) dispatches at each new horizon, from their predicates and the layer
# widths of spec.py (levels H, H/2, H/4, H/8; attention inner width 256 everywhere; k = 5 convolutions with C_in, C_out in {32, 64}
# at H and H/2, 64 x 64 at H/4 (ups.1), 128 .. 512 wide at H/4 and H/8; the input gradients swap N and K).
#   ato / abl: ato_applicable (atk.hip) -- some level length divides 48 or 32;
#   tkc: tkc_applicable (tkc.hip) -- a narrow level of length L >= 8 dividing 48 or 32, or 64 (not 64 x 64 channels);
#   tkw: tkw_applicable (tkw.hip) -- a wide level with L >= 3 and 96 % L == 0 (the input gradient also needs tw_pro_variant);
#   tklb: use_tklb -- the d(ln1) of a level abl does not take (ato_applicable false there).
# Slot order of ramp_profile_read_kernels: 0 ffx forward, 1 ffx backward, 2 tkl, 3 tklb, 4 ato, 5 abl, 6 tkc, 7 tkw.
DISPATCH = {   # H: (ato, abl, tkc, tkw, tklb)
    8: (True, True, True, False, False),    # 8 | 48; tkc at L = 8; no wide level has L >= 3 (H/4 = 2, H/8 = 1), and ups.2's conv-1 input
                                            # gradient (N = 128, K = 32, L = 4) fails tw_pro_variant (4 % 8 staged rows); 8/4/2/1 all take abl
    16: (True, True, True, True, False),    # 16 | 48; tkc at 16 and 8; tkw at L = 4 (96 % 4 == 0); 16/8/4/2 all take abl
    24: (True, True, True, True, False),    # every level divides 48 (abl everywhere, no tklb); tkc at 24 and 12; tkw at 6 and 3
    32: (True, True, True, True, False),    # 32 | 32; tkc at 32, 16 and 8; tkw at 8 and 4; 32/16/8/4 all take abl
    56: (False, False, False, False, True),  # 56/28/14/7: no level divides 48, 32 or 96 -- everything on the generic kernels
    64: (True, True, True, True, True),     # ato from L = 32 down; tkc at 64 (NG = 4) and 32; tkw at 16 and 8; L = 64 keeps tklb
}


# The exact launches of that evaluation per horizon: the nine counts of ramp_profile_read_kernels (slot 8: every other launch of the GEMM
# class) and ramp_launch_count.  Integers decided on the host by the routing predicates of engine.hip (struct Run), read off the commit before
# the routing refactor on an MI355X: a change of either is a change of routing, and of the call-site numbering the delayed scaling rests on.
DISPATCH_COUNTS = {   # H: ((ffx_fwd, ffx_bwd, tkl, tklb, ato, abl, tkc, tkw, other), launch_count)
    8: ((16, 16, 32, 0, 16, 16, 8, 0, 118), 299),
    16: ((16, 16, 32, 0, 16, 16, 22, 9, 95), 276),
    24: ((16, 16, 32, 0, 16, 16, 22, 19, 85), 266),
    32: ((16, 16, 32, 0, 16, 16, 28, 32, 66), 247),
    56: ((16, 16, 48, 16, 0, 0, 0, 0, 126), 339),
    64: ((16, 16, 34, 2, 14, 14, 28, 33, 65), 250),
}


def _profiled_eval(m, x, t, pts):
    """One eager evaluation under the per-launch profiler: (eps, the nine launch counts of ramp_profile_read_kernels, launch_count())."""
    import ctypes as C
    from ramp_amd import _lib
    lib = _lib.load()
    _lib.check(lib.ramp_profile(m.ctx(), 1))
    eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
    ms = (C.c_double * 9)(); fl = (C.c_double * 9)(); cnt = (C.c_int64 * 9)()
    _lib.check(lib.ramp_profile_read_kernels(m.ctx(), 9, ms, fl, cnt))
    _lib.check(lib.ramp_profile(m.ctx(), 0))
    return eps, tuple(cnt), m.launch_count()


@pytest.mark.parametrize("tag,S,H,o3", HORIZON_CASES)
def test_fused_plan_dispatches_what_the_predicates_admit(tag, S, H, o3):
    """The bench's launch plan on one eager fp16x3 evaluation (after its calibration): the profiled kernel slots that are
    non-zero are exactly the ones the predicates admit at this horizon (DISPATCH), so the fixture parity in fp16x3-tkw mode
    really exercised the sample-owning kernels where they apply, and the fallback path where they do not; and the launches
    are exactly the recorded ones (DISPATCH_COUNTS)."""
    g = np.load(f"{GOLDEN}/unet{tag}.npz")
    m = build_unet(S, H, o3, max_rows=8, gemm_mode="fp16x3", launch_plan=util.PLANS["tkw"])
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    m(x, t, None, obstacle_pts=pts); m(x, t, None, obstacle_pts=pts)      # forward and input-gradient call sites calibrated
    eps, counts, launches = _profiled_eval(m, x, t, pts)
    assert m.score_mode() == "fp16x3"
    print(f"{tag}: kernel launches ffx_fwd ffx_bwd tkl tklb ato abl tkc tkw other = {counts}, launch_count {launches}")
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0, counts
    want = dict(zip(("ato", "abl", "tkc", "tkw", "tklb"), DISPATCH[H]))
    got = dict(ato=counts[4] > 0, abl=counts[5] > 0, tkc=counts[6] > 0, tkw=counts[7] > 0, tklb=counts[3] > 0)
    assert got == want, (H, counts)
    assert (counts, launches) == DISPATCH_COUNTS[H], (H, counts, launches)
    assert rel(eps, g["eps"]) < 5e-5


# The same pair for every launch plan of util.PLANS, bf16x6 and fp32 on the 2d_h48 fixture: of the third evaluation (fp16x3 modes: the
# steady one) and, in the fp16x3 modes, of the first -- the calibration evaluation, on the bf16x6 kernels except for the narrow k = 5
# convolutions, which tkc.hip takes there too so that the call sites number alike.  Recorded like DISPATCH_COUNTS.
ROUTING_MODES = [f"fp16x3-{k}" if k else "fp16x3" for k in util.PLANS] + ["bf16x6", "fp32"]
ROUTING_COUNTS = {   # mode: (third evaluation, first evaluation or None), each ((nine counts), launch_count)
    "fp16x3": (((0, 0, 0, 0, 0, 0, 0, 0, 254), 435), ((0, 0, 0, 0, 0, 0, 0, 0, 254), 435)),
    "fp16x3-fusedff": (((0, 0, 0, 0, 0, 0, 0, 0, 238), 419), ((0, 0, 0, 0, 0, 0, 0, 0, 254), 435)),
    "fp16x3-ffx": (((16, 16, 0, 0, 0, 0, 0, 0, 190), 371), ((0, 0, 0, 0, 0, 0, 0, 0, 254), 435)),
    "fp16x3-tok": (((16, 16, 48, 16, 0, 0, 0, 0, 126), 339), ((0, 0, 0, 0, 0, 0, 0, 0, 254), 435)),
    "fp16x3-atk": (((16, 16, 32, 0, 16, 16, 0, 0, 126), 307), ((0, 0, 0, 0, 0, 0, 0, 0, 254), 435)),
    "fp16x3-tkc": (((16, 16, 32, 0, 16, 16, 28, 0, 98), 279), ((0, 0, 0, 0, 0, 0, 28, 0, 226), 407)),
    "fp16x3-tkw": (((16, 16, 32, 0, 16, 16, 28, 33, 65), 246), ((0, 0, 0, 0, 0, 0, 28, 0, 226), 407)),
    "fp16x3-m32": (((16, 16, 32, 0, 16, 16, 28, 33, 65), 246), ((0, 0, 0, 0, 0, 0, 28, 0, 226), 407)),
    "bf16x6": (((0, 0, 0, 0, 0, 0, 0, 0, 254), 435), None),
    "fp32": (((0, 0, 0, 0, 0, 0, 0, 0, 254), 435), None),
}


@pytest.mark.parametrize("mode", ROUTING_MODES)
def test_routing_of_every_launch_plan_and_phase(mode):
    """Which kernel serves each product of a score evaluation -- and with it the order in which GEMM call sites are taken -- is pinned
    for every launch plan in every phase it reaches: the launches of the calibration evaluation (fp16x3 modes) and of the third one
    equal the recorded ones (ROUTING_COUNTS)."""
    g = np.load(f"{GOLDEN}/unet2d_h48.npz")
    base, _, plan = mode.partition("-")
    m = build_unet(4, 48, False, max_rows=8, gemm_mode=base, launch_plan=util.PLANS[plan] if base == "fp16x3" else None)
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    m.prepare_time_table(int(g["t"][0]) + 1); m.cache_scene_encoding(pts)      # (the scene encoder's launches stay out of the first profile)
    first = None
    if base == "fp16x3":
        first = _profiled_eval(m, x, t, pts)[1:]
        assert m.score_mode() == "bf16x6"                      # calibration evaluation
    else:
        m(x, t, None, obstacle_pts=pts)
    m(x, t, None, obstacle_pts=pts)
    eps, counts, launches = _profiled_eval(m, x, t, pts)
    assert m.score_mode() == base
    print(f"{mode}: third evaluation {counts} launch_count {launches}; first {first}")
    assert ((counts, launches), first) == ROUTING_COUNTS[mode], (mode, counts, launches, first)
    assert rel(eps, g["eps"]) < 5e-5


_ORACLE64 = {}


def _oracle64_batch(S, H, o3, x2, lats):
    """float64 oracle (f, eps) of the per-horizon batch at t = 0 and 24, computed once per shape."""
    key = (S, H, o3)
    if key not in _ORACLE64:
        u = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=np.float64)
        out = {}
        for t in (0, 24):
            tt = np.full((x2.shape[0],), t)
            out[t] = (u.forward_no_energy(x2, tt, lats), u.score(x2, tt, lats))
        _ORACLE64[key] = out
    return _ORACLE64[key]


@pytest.mark.parametrize("gemm_mode", ["fp16x3", "fp16x3-tkw"])
@pytest.mark.parametrize("tag,S,H,o3", HORIZON_CASES)
def test_score_batch_at_every_horizon_vs_oracle64(tag, S, H, o3, gemm_mode):
    """B = 7 trajectories x 2 variants (14 rows) through a context of 6 rows (chunks of 6, 6 and 2 rows) at every new horizon and
    state width, against the float64 oracle, per ROW as well as over the batch: a max-normalised error over the whole batch cannot
    see one wrong sample in a partial tile or a short last chunk."""
    from ramp_amd import _lib
    base, plan = util.split_mode(gemm_mode)
    m = build_unet(S, H, o3, max_rows=6, gemm_mode=base, launch_plan=plan)
    cloud = synth.make_cloud(6, 64, 2, seed=3) if not o3 else synth.make_cloud(4, 30, 3, seed=3)
    lat = m.encode_scene(dev(cloud))
    m.set_scene(torch.cat([lat, torch.zeros_like(lat)]), [0, 1])
    m.prepare_time_table(25)
    B = 7
    x = synth.make_noise((B, H, S), seed=22)
    xd = dev(x)
    lats = np.tile(lat[0].cpu().numpy()[None], (2 * B, 1)); lats[1::2] = 0
    ref = _oracle64_batch(S, H, o3, np.repeat(x, 2, axis=0), lats)
    lib = _lib.load()
    eps = torch.empty((2 * B, H, S), device="cuda"); f = torch.empty_like(eps)
    _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xd), B, 2, 24, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()))
    assert m.score_mode() == "bf16x6"                          # calibration evaluation
    for t in (0, 24):
        _lib.check(lib.ramp_score(m.ctx(), _lib.ptr(xd), B, 2, t, _lib.ptr(f), _lib.ptr(eps), _lib.current_stream()))
        assert m.score_mode() == "fp16x3"
        f64, eps64 = ref[t]
        fh, eh = f.cpu().numpy(), eps.cpu().numpy()
        assert rel(fh, f64) < 2e-5 and rel(eh, eps64) < 5e-5, t
        row_f = [rel(fh[r], f64[r]) for r in range(2 * B)]
        row_e = [rel(eh[r], eps64[r]) for r in range(2 * B)]
        print(f"{tag} {gemm_mode} t={t}: f {rel(fh, f64):.2e} eps {rel(eh, eps64):.2e}, worst row f {max(row_f):.2e} eps {max(row_e):.2e}")
        assert max(row_f) < 2e-5, (t, row_f)
        assert max(row_e) < 5e-5, (t, row_e)


def test_missing_weights_and_bad_args_fail_loudly():
    from ramp_amd import _lib
    from ramp_amd.models import TemporalUnetInference
    m = TemporalUnetInference(n_support_points=48, state_dim=4).to("cuda")
    with pytest.raises(RuntimeError):
        m.ctx()
    m = build_unet(4, 48, False, max_rows=4)
    with pytest.raises(_lib.RampHipError):     # scene not set
        x = torch.zeros(1, 48, 4, device="cuda"); e = torch.empty(2, 48, 4, device="cuda")
        m.prepare_time_table(5)
        _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(x), 1, 2, 0, None, _lib.ptr(e), None))
    with pytest.raises(_lib.RampHipError):     # timestep outside the table
        lat = torch.zeros(2, 320, device="cuda"); m.set_scene(lat, [0, 1])
        _lib.check(_lib.load().ramp_score(m.ctx(), _lib.ptr(x), 1, 2, 7, None, _lib.ptr(e), None))


def test_scene_encoders_hip_against_reference_fixture():
    """ramp_encode_scene (HIP) vs the reference's scene latents: 2-D 6x64 and 16x64 clouds, 3-D 5x50 and 20x200."""
    g = np.load(f"{GOLDEN}/scene_latents.npz")
    m2 = build_unet(4, 48, False, max_rows=4)
    m3 = build_unet(6, 48, True, max_rows=4)
    for k in ("2d_6x64", "2d_16x64"):
        lat = m2.encode_scene(dev(g["cloud" + k]))[0].cpu().numpy()
        assert lat.shape == (320,) and rel(lat, g["lat" + k]) < 5e-6, k
    for k in ("3d_5x50", "3d_20x200"):
        lat = m3.encode_scene(dev(g["cloud" + k]))[0].cpu().numpy()
        assert lat.shape == (256,) and rel(lat, g["lat" + k]) < 5e-6, k
    two = m2.encode_scene(dev(np.stack([g["cloud2d_6x64"], g["cloud2d_6x64"][::-1].copy()])))
    assert two.shape == (2, 320) and rel(two[0].cpu().numpy(), g["lat2d_6x64"]) < 5e-6


def test_two_contexts_with_different_launch_plans_in_one_process():
    """The launch plan is per-context state set through the ABI (ramp_set_launch_plan), not process-wide environment:
    two contexts in one process run different kernels for the same feed-forward pairs -- the tile GEMMs with stand-alone
    LayerNorms in one, the token-owning fused forward + backward kernels (ffx.hip) in the other -- and agree with each
    other and with the reference fixture; switching a live context's plan takes effect at the next evaluation."""
    g = np.load(f"{GOLDEN}/unet2d_h48.npz")
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    a = build_unet(4, 48, False, max_rows=8, gemm_mode="fp16x3", launch_plan=dict(ff_fused_rows=0, ffx_rows=0))
    b = build_unet(4, 48, False, max_rows=8, gemm_mode="fp16x3", launch_plan=dict(ff_fused_rows=0, ffx_rows=1))
    assert a.get_launch_plan()["ffx_rows"] == 0 and b.get_launch_plan()["ffx_rows"] == 1
    out = {}
    for name, m in (("tiles", a), ("ffx", b)):
        m(x, t, None, obstacle_pts=pts); m(x, t, None, obstacle_pts=pts)      # forward + backward call sites calibrated
        out[name] = m(x, t, None, obstacle_pts=pts).cpu().numpy()
        assert m.score_mode() == "fp16x3"
        assert rel(out[name], g["eps"]) < 5e-5, name
    assert not np.array_equal(out["tiles"], out["ffx"])                  # different kernels, different summation orders
    assert rel(out["tiles"], out["ffx"]) < 2e-5
    a(x, t, None, obstacle_pts=pts); per_eval_tiles = a.launch_count()   # (kernel launches of the last call)
    a.set_launch_plan(ffx_rows=1)                                         # live switch: recalibrates, then the fused kernels
    a(x, t, None, obstacle_pts=pts); a(x, t, None, obstacle_pts=pts)
    got = a(x, t, None, obstacle_pts=pts).cpu().numpy()
    per_eval_ffx = a.launch_count()
    assert a.score_mode() == "fp16x3" and np.array_equal(got, out["ffx"])
    # 8 transformers x 2 blocks: LN + FF1 + FF2 (3 launches) -> 1 forward, d(hg) + FF1-dX + LN-backward (3) -> 1 backward
    assert per_eval_tiles - per_eval_ffx == 16 * 4, (per_eval_tiles, per_eval_ffx)


@pytest.mark.parametrize("gemm_mode", ["fp16x3-tkw", "bf16x6", "fp32"])
def test_score_with_outlier_channel_weights(gemm_mode):
    """Trained-transformer statistics: 8 output channels of every attn1.to_out and ff.net.2 scaled by 2^9
    (synth.add_outlier_channels), so the residual stream of every transformer carries a few channels two to three orders of
    magnitude above the rest -- where one power-of-two scale per operand tensor with a 2^8 full-precision window is most
    exposed.  Fixture: the imported reference with the same weights (unet2d_h48_outlier.npz).  The fp16x3 plan the bench runs
    must either stay inside the bar without tripping its range guard, or trip it and return the bf16x6 answer (ramp_score
    repeats a flagged evaluation at once); it may never return a silently degraded result."""
    g = np.load(f"{GOLDEN}/unet2d_h48_outlier.npz")
    gemm_mode, plan = util.split_mode(gemm_mode) if "-" in gemm_mode else (gemm_mode, None)
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.unet import load_numpy_state_dict
    sd = synth.add_outlier_channels(weights(4, 48, False))
    m = TemporalUnetInference(n_support_points=48, state_dim=4, max_rows=8, debug_taps=True, gemm_mode=gemm_mode, launch_plan=plan)
    m = load_numpy_state_dict(m, sd).eval().to("cuda")
    N = g["x"].shape[0]
    x = dev(g["x"]); t = torch.from_numpy(g["t"]).cuda()
    pts = dev(g["cloud"])[None].repeat(N, 1, 1, 1)
    modes = []
    for _ in range(3):
        eps = m(x, t, None, obstacle_pts=pts).cpu().numpy()
        modes.append(m.score_mode())
    f = m.forward_no_energy(x, t, obstacle_pts=pts).cpu().numpy()
    worst = 0.0
    for k in g.files:
        if k.startswith("out/") or k.startswith("gout/"):
            kind, name = k.split("/")
            worst = max(worst, rel(m.debug_read(kind, name, g[k].shape).cpu().numpy(), g[k]))
    print(f"outlier weights {gemm_mode}: evaluations ran as {modes}; f {rel(f, g['f']):.2e} eps {rel(eps, g['eps']):.2e} worst tap {worst:.2e}")
    assert rel(f, g["f"]) < 2e-5 and rel(eps, g["eps"]) < 5e-5 and worst < 5e-5
