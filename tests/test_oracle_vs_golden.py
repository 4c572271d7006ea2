"""Pin the CPU oracle (oracle/ramp_oracle.py) against fixtures captured from the reference itself
(oracle/make_goldens.py -> tests/golden/*.npz).  CPU only."""
import os

import numpy as np
import pytest

from oracle import ramp_oracle as O
from ramp_amd import synth
from ramp_amd.spec import make_unet_spec

G = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


_SD = {}


def weights(S, H, o3):
    key = (S, o3)
    if key not in _SD:
        _SD[key] = synth.make_unet_state_dict(make_unet_spec(S, H, obstacle_3d=o3))
    return _SD[key]


@pytest.mark.parametrize("T", [25, 50, 100])
def test_schedule(T):
    g = np.load(f"{G}/schedule_T{T}.npz")
    s = O.make_schedule(T)
    assert set(s) == set(g.files)
    for k in g.files:
        # tables built from 1 - alphas_cumprod at small t are cancellation-limited in float32:
        # two correct float32 evaluations differ by ~1e-4 relative (measured 1.8e-4 at T=100)
        tol = 3e-4 if k in ("sqrt_one_minus_alphas_cumprod", "log_one_minus_alphas_cumprod",
                             "sqrt_recipm1_alphas_cumprod", "posterior_variance",
                             "posterior_log_variance_clipped", "posterior_mean_coef1",
                             "posterior_mean_coef2") else 2e-6
        assert rel(s[k], g[k]) < tol, k


@pytest.mark.parametrize("tag,S,H,o3", [("2d_h48", 4, 48, False), ("3d_h48", 6, 48, True), ("3d_h64", 6, 64, True), ("2d_h40", 4, 40, False),
                                        # every other horizon the engine accepts and the ends of its state-width range
                                        ("2d_h8", 4, 8, False), ("3d_h16", 6, 16, True), ("2d_h24", 4, 24, False),
                                        ("s3_h32", 3, 32, False), ("s2_h56", 2, 56, False), ("s16_h64", 16, 64, False)])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_unet_forward_and_score(tag, S, H, o3, dt):
    g = np.load(f"{G}/unet{tag}.npz")
    u = O.UNetOracle(weights(S, H, o3), S, H, obstacle_3d=o3, dtype=dt)
    assert rel(u.encode_scene(g["cloud"]), g["latent"]) < 5e-6
    N = g["x"].shape[0]
    lats = np.tile(g["latent"][None], (N, 1))
    lats[1::2] = 0          # odd rows unconditional (UnetInference.py:192-197)
    assert rel(u.time_embedding(g["t"]), g["temb"]) < 2e-6
    taps, gt = {}, {}
    f = u.forward_no_energy(g["x"], g["t"], lats, taps=taps)
    eps = u.score(g["x"], g["t"], lats, grad_taps=gt)
    assert rel(f, g["f"]) < 1e-5
    assert rel(eps, g["eps"]) < 2e-5
    for k in g.files:
        if k.startswith("out/"):
            assert rel(taps[k[4:]], g[k]) < 1e-5, k
        if k.startswith("gout/"):
            assert rel(gt[k[5:]], g[k]) < 2e-5, k


def test_scene_latents():
    g = np.load(f"{G}/scene_latents.npz")
    u2 = O.UNetOracle(weights(4, 48, False), 4, 48)
    u3 = O.UNetOracle(weights(6, 48, True), 6, 48, obstacle_3d=True)
    for k in ("2d_6x64", "2d_16x64"):
        assert rel(u2.encode_scene(g["cloud" + k]), g["lat" + k]) < 5e-6
    for k in ("3d_5x50", "3d_20x200"):
        assert rel(u3.encode_scene(g["cloud" + k]), g["lat" + k]) < 5e-6


@pytest.mark.parametrize("name", ["rand", "line", "nohit", "ends", "big"])
def test_apf_cases(name):
    g = np.load(f"{G}/apf_cases.npz")
    thr, strength, win = g[name + "/params"]
    out = O.apf_avoidance(g[name + "/traj"].copy(), g[name + "/cloud"], float(thr), float(strength), int(win))
    assert np.abs(out - g[name + "/out"]).max() < 5e-7
    if name == "nohit":
        assert np.array_equal(out, g[name + "/traj"])
    else:
        assert (out != g[name + "/traj"]).sum() > 0
    assert np.array_equal(out[..., 2:], g[name + "/traj"][..., 2:])     # velocities untouched


def test_cost_cases():
    g = np.load(f"{G}/cost_cases.npz")
    for thr in (0.02, 0.05, 0.1):
        m = g[f"mask_{thr}"]
        assert 0 < m.sum() < m.size
        assert np.array_equal(O.collision_mask(g["trajs"], g["cloud"], thr), m)
    assert rel(O.path_length(g["trajs"]), g["path_length"]) < 1e-6
    assert rel(O.smoothness(g["trajs"]), g["smoothness"]) < 1e-6
    best, total, free = O.trajectory_costs(g["trajs"], g["cloud"], 0.05)
    assert np.array_equal(free, g["free_mask"])
    assert best == int(g["best_index"])
    assert rel(total, g["total_costs"]) < 1e-5


def _ddpm(tag, dt, teacher):
    g = np.load(f"{G}/chain_ddpm_{tag}.npz")
    sched = dict(np.load(f"{G}/schedule_T25.npz"))
    u = O.UNetOracle(weights(4, 48, False), 4, 48, dtype=dt)
    sm = O.SamplerOracle(u, 25, 2.0, dtype=dt, sched=sched)
    ch = sm.ddpm(g["noise"], synth.default_hard_conds(4, 48), g["latent"], cloud=g["cloud"].reshape(-1, 2),
                 use_apf=bool(g["use_apf"]), n_without_noise=int(g["n_without_noise"]),
                 teacher=g["chain"] if teacher else None)
    return ch, g["chain"]


def test_chain_ddpm_free_running():
    """Whole T=25 chain from x_T with injected noise; the reference's own fp32-vs-fp64 drift is 3.5e-5."""
    ch, ref = _ddpm("plain", np.float32, False)
    assert ch.shape == ref.shape == (26, 4, 48, 4)
    assert np.abs(ch - ref).max() < 1e-4


def test_chain_ddpm_extra_steps():
    ch, ref = _ddpm("extra2", np.float32, False)
    assert ch.shape == ref.shape == (28, 4, 48, 4)
    assert np.abs(ch - ref).max() < 1e-4


def test_chain_ddpm_apf_teacher_forced():
    """APF is discontinuous (hit / nearest-point decisions) and stiff (d dir / d x ~ 1/d), so a free-running
    chain amplifies 1e-5 drift; per-step parity is therefore checked with teacher forcing, and the
    free-running chain only on the steps before the first APF application."""
    ch, ref = _ddpm("apf", np.float32, True)
    assert np.abs(ch - ref).max() < 1e-4
    plain = np.load(f"{G}/chain_ddpm_plain.npz")["chain"]
    assert np.abs(ref[-1] - plain[-1]).max() > 1e-3          # the APF actually fired in the golden
    assert np.array_equal(ref[:22], plain[:22])               # and only for forward_t > 20


@pytest.mark.parametrize("tag", ["plain", "apf"])
def test_chain_ddim(tag):
    g = np.load(f"{G}/chain_ddim_{tag}.npz")
    sched = dict(np.load(f"{G}/schedule_T100.npz"))
    u = O.UNetOracle(weights(4, 48, False), 4, 48)
    sm = O.SamplerOracle(u, 100, 2.0, sched=sched)
    ch = sm.ddim(g["noise"][0], synth.default_hard_conds(4, 48), g["latent"], cloud=g["cloud"].reshape(-1, 2),
                 use_apf=bool(g["use_apf"]), teacher=g["chain"] if tag == "apf" else None)
    assert ch.shape == g["chain"].shape == (6, 4, 48, 4)
    assert np.abs(ch - g["chain"]).max() < 1e-4


def test_chain3d_ddpm():
    """3-D sampler (w = 5.75): B independent n_samples=1 reference runs stacked."""
    g = np.load(f"{G}/chain3d_ddpm.npz")
    sched = dict(np.load(f"{G}/schedule_T25.npz"))
    u = O.UNetOracle(weights(6, 48, True), 6, 48, obstacle_3d=True)
    sm = O.SamplerOracle(u, 25, float(g["w"]), sched=sched)
    ch = sm.ddpm(g["noise"], synth.default_hard_conds(6, 48), g["latent"])
    assert ch.shape == g["chain"].shape
    assert np.abs(ch - g["chain"]).max() < 2e-4


def test_chain3d_h64_t50():
    """BASELINE config 5's shape (3-D, H = 64, T = 50): w = 5.75 amplifies rounding ~12x per step and T = 50 doubles the
    length, so the free-running fp32 restatement is compared at 5e-4 and every step teacher-forced at 1e-4."""
    g = np.load(f"{G}/chain3d_h64_t50.npz")
    sched = dict(np.load(f"{G}/schedule_T50.npz"))
    u = O.UNetOracle(weights(6, 64, True), 6, 64, obstacle_3d=True)
    assert rel(u.encode_scene(g["cloud"]), g["latent"]) < 5e-6
    sm = O.SamplerOracle(u, 50, float(g["w"]), sched=sched)
    hc = synth.default_hard_conds(6, 64)
    ch = sm.ddpm(g["noise"], hc, g["latent"], teacher=g["chain"])
    assert ch.shape == g["chain"].shape == (51, 2, 64, 6)
    assert np.abs(ch - g["chain"]).max() < 1e-4
    free = sm.ddpm(g["noise"], hc, g["latent"])
    print("config-5 chain, free-running oracle32 vs reference:", np.abs(free - g["chain"]).max())
    assert np.abs(free - g["chain"]).max() < 5e-4


def test_compose_static():
    """compose=True on the static wrapper: the single p_mean_variance_compose, the DDPM chain (no APF hook on that path
    although use_apf=True) and the DDIM-8 + APF chain on the union cloud (diffusion_model_static.py:188-229, 298-319)."""
    g = np.load(f"{G}/compose_static.npz")
    u = O.UNetOracle(weights(4, 48, False), 4, 48)
    lats = np.stack([u.encode_scene(g["clouds"][0]), u.encode_scene(g["clouds"][1])])
    hc = synth.default_hard_conds(4, 48)
    sm = O.SamplerOracle(u, 25, 2.0, sched=dict(np.load(f"{G}/schedule_T25.npz")), compose_w=(2.0, 2.0))
    e = sm.eps_compose(g["pmv_x"], int(g["pmv_t"]), lats)
    assert rel(e, g["pmv_ecomb"]) < 2e-5
    x0, mean = sm.x0_mean(g["pmv_x"], g["pmv_ecomb"], int(g["pmv_t"]))
    assert np.abs(x0 - g["pmv_x0"]).max() < 1e-6 and np.abs(mean - g["pmv_mean"]).max() < 1e-6
    ch = sm.ddpm(g["ddpm_noise"], hc, lats, use_apf=False)
    assert ch.shape == g["ddpm_chain"].shape == (26, 3, 48, 4)
    assert np.abs(ch - g["ddpm_chain"]).max() < 2e-4                 # w1 + w2 = 4: ~2x the CFG chain's amplification
    sm100 = O.SamplerOracle(u, 100, 2.0, sched=dict(np.load(f"{G}/schedule_T100.npz")), compose_w=(2.0, 2.0))
    union = np.concatenate([g["clouds"][0], g["clouds"][1][:4]]).reshape(-1, 2)
    ch = sm100.ddim(g["ddim_noise"][0], hc, lats, cloud=union, use_apf=True, K=8, teacher=g["ddim_chain"])
    assert ch.shape == g["ddim_chain"].shape == (9, 3, 48, 4)
    assert np.abs(ch - g["ddim_chain"]).max() < 1e-4
    plain = sm100.ddim(g["ddim_noise"][0], hc, lats, use_apf=False, K=8, teacher=g["ddim_chain"])
    assert np.abs(plain[3:] - g["ddim_chain"][3:]).max() > 1e-4      # the APF hook did fire in the fixture (forward_t >= 2)


def test_compose_3d():
    """3-D compose (w1 = w2 = 5; diffusion_model_3d.py:163-182), B independent n_samples=1 reference runs stacked."""
    g = np.load(f"{G}/compose_3d.npz")
    u = O.UNetOracle(weights(6, 48, True), 6, 48, obstacle_3d=True)
    lats = np.stack([u.encode_scene(c) for c in g["clouds"]])
    assert rel(lats, g["latents"]) < 5e-6
    sm = O.SamplerOracle(u, 25, 5.75, sched=dict(np.load(f"{G}/schedule_T25.npz")), compose_w=(float(g["w1"]), float(g["w2"])))
    hc = synth.default_hard_conds(6, 48)
    ch = sm.ddpm(g["noise"], hc, g["latents"], teacher=g["chain"])
    assert ch.shape == g["chain"].shape == (26, 2, 48, 6)
    assert np.abs(ch - g["chain"]).max() < 1e-4


def test_torch_cpu_baseline_score_and_chain():
    """bench.py's PyTorch-CPU eager baseline (oracle/torch_cpu.py: the same architecture and loop written in this repo,
    ATen fp32 kernels, autograd energy gradient) against the reference's own outputs: forward / eps of unet2d_h48.npz and
    the free-running T = 25 DDPM chain."""
    import torch
    from oracle.torch_cpu import TorchCpuSampler, TorchCpuScoreNet
    g = np.load(f"{G}/unet2d_h48.npz")
    net = TorchCpuScoreNet(weights(4, 48, False), 4, 48)
    N = g["x"].shape[0]
    lat = np.tile(g["latent"][None], (N, 1)).astype(np.float32); lat[1::2] = 0
    x, t, lt = torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(lat)
    with torch.no_grad():
        f = net.f(x, t, lt).numpy()
    assert rel(f, g["f"]) < 2e-5
    assert rel(net.score(x, t, lt).numpy(), g["eps"]) < 5e-5
    c = np.load(f"{G}/chain_ddpm_plain.npz")
    sm = TorchCpuSampler(net, dict(np.load(f"{G}/schedule_T25.npz")), 2.0)
    ch = sm.ddpm(c["noise"], synth.default_hard_conds(4, 48), c["latent"])
    assert ch.shape == c["chain"].shape and np.abs(ch - c["chain"]).max() < 1e-4


def test_dynamic_cases():
    """Dynamic (pursuit-evasion) wrapper pieces: CFG with the reference's blocked row layout (quirk Q1) for even
    and odd batch sizes, the per-trajectory static / pursuer APF, and the velocity smoothing."""
    g = np.load(f"{G}/dynamic_cases.npz")
    sched = dict(np.load(f"{G}/schedule_T100.npz"))
    u = O.UNetOracle(weights(4, 48, False), 4, 48)
    sm = O.SamplerOracle(u, 100, 2.5, sched=sched)
    lat = u.encode_scene(g["cloud"])
    for B in (4, 3):
        e = sm.eps_cfg_dynamic_compat(g[f"pmv{B}/x"], 40, lat)
        assert rel(e, g[f"pmv{B}/ecomb"]) < 2e-5
        x0, mean = sm.x0_mean(g[f"pmv{B}/x"], g[f"pmv{B}/ecomb"], 40)
        assert np.abs(x0 - g[f"pmv{B}/x0"]).max() < 1e-6 and np.abs(mean - g[f"pmv{B}/mean"]).max() < 1e-6
    thr_s, thr_p, st_s, st_p, w_s, w_p = g["apf/params"]
    tr = g["apf/traj"]
    for b in range(tr.shape[0]):
        o1 = O.apf_dynamic_avoidance(tr[b], g["apf/static_points"], thr_s, thr_s, st_s, int(w_s))
        o2 = O.apf_dynamic_avoidance(tr[b], g["apf/dynamic_points"], thr_p, thr_s, st_p, None, affected=48, goal=g["apf/goal"])
        assert np.abs(o1 - g["apf/out_static"][b]).max() < 2e-7
        assert np.abs(o2 - g["apf/out_dynamic"][b]).max() < 2e-7
    assert (g["apf/out_static"] != tr).sum() > 20 and (g["apf/out_dynamic"] != tr).sum() > 20
    assert np.array_equal(g["apf/out_static"][3], tr[3]) and np.array_equal(g["apf/out_dynamic"][3], tr[3])
    assert np.abs(O.sm_smooth(g["sm/s1"], g["sm/s2"]) - g["sm/out"]).max() < 1e-6


def test_metrics_against_reference_fixture():
    """collision intensity / path length / smoothness / waypoint variance vs the reference's Metrics class."""
    g = np.load(f"{G}/metrics_cases.npz")
    tr = g["traj"]
    assert np.array_equal(O.collision_intensity(tr, g["centers"], g["sizes"]), g["intensity"])
    assert np.abs(O.path_length(tr) - g["path_length"]).max() < 2e-6
    assert np.abs(O.smoothness(tr) - g["smoothness"]).max() < 2e-5
    # the reference evaluates cdist + var in fp32: 1e-5 relative is its own rounding level
    assert abs(O.waypoint_variance(tr) - float(g["variance_all"])) < 1e-5 * float(g["variance_all"])
    free = tr[g["intensity"] <= 0.01]
    assert len(free) == int(g["n_free"])
    assert abs(O.waypoint_variance(free) - float(g["free_variance"])) < 1e-5 * float(g["free_variance"])
