"""Host side of the Langevin refinement (``mcmc=`` -> ``ramp_sample_mcmc``) and of the energy accessors: the eta / K tables, the evaluation
count, the Philox layout replicated in numpy, the Python-level refusals, struct layout and the declared / bound / exported symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import util
from ramp_amd import _lib
from ramp_amd.diffusion import mcmc_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, S = 48, 4


def make(T, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    kw.setdefault("predict_epsilon", True)
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=H, state_dim=S), n_diffusion_steps=T, **kw)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_tables_from_step_scale_t_range_and_explicit_lists(sampler):
    """eta_t = c (1 - abar_t), sigma_t = sqrt(1 - abar_t), so a = eta / sigma = c sigma and the noise scale sqrt(2 eta) = sigma sqrt(2 c); t_range
    zeroes K outside lo <= t <= hi; explicit lists override; a job runs n_steps + sum K evaluations."""
    T = 25 if sampler == "ddpm" else 100
    dm = make(T, sampler=sampler)
    steps = dm._ddpm_steps()[0] if sampler == "ddpm" else [int(i) for i in dm.ddim_set_timesteps(5)]
    ac = dm.alphas_cumprod.double().numpy()
    n = len(steps)
    assert n == (25 if sampler == "ddpm" else 5)
    tab = mcmc_tables(dict(kind="mala", steps=2, step_scale=0.05), steps, dm.alphas_cumprod)
    assert tab["kind"] == 2 and tab["n_inner"] == [2] * n and tab["total"] == 2 * n
    assert np.allclose(tab["sigma"], np.sqrt(1 - ac[steps]), rtol=1e-12) and np.allclose(tab["step_size"], 0.05 * (1 - ac[steps]), rtol=1e-12)
    eta, sig = np.array(tab["step_size"]), np.array(tab["sigma"])
    assert np.allclose(eta / sig, 0.05 * sig, rtol=1e-12) and np.allclose(np.sqrt(2 * eta), sig * np.sqrt(2 * 0.05), rtol=1e-12)
    lo, hi = steps[-2], steps[1]
    tr = mcmc_tables(dict(kind="ula", steps=3, step_scale=0.1, t_range=(lo, hi)), steps, dm.alphas_cumprod)
    assert tr["kind"] == 1 and tr["n_inner"] == [3 if lo <= t <= hi else 0 for t in steps] and tr["n_inner"][0] == 0 and tr["n_inner"][-1] == 0
    assert n + tr["total"] == n + 3 * (n - 2)      # the job's evaluation count
    Ks = [(j % 3) for j in range(n)]
    etas = [0.01 * (j + 1) for j in range(n)]
    ex = mcmc_tables(dict(kind="mala", steps=Ks, step_size=etas, step_scale=123.0), steps, dm.alphas_cumprod)
    assert ex["n_inner"] == Ks and ex["step_size"] == etas and ex["total"] == sum(Ks)
    # through the model: the same tables, as ramp_mcmc_params
    from ramp_amd.diffusion import _HostArrays
    arrays = _HostArrays()
    mp = dm._fill_mcmc(arrays, dm._mcmc_tables(dict(kind="mala", steps=Ks, step_size=etas), steps))
    assert mp.kind == 2 and [mp.n_inner[j] for j in range(n)] == Ks
    assert [mp.step_size[j] for j in range(n)] == [np.float32(e) for e in etas]
    assert [mp.sigma[j] for j in range(n)] == [np.float32(v) for v in ex["sigma"]]
    # the default kind is MALA, the default step_scale 0.1
    d = mcmc_tables(dict(steps=1), steps, dm.alphas_cumprod)
    assert d["kind"] == 2 and np.allclose(d["step_size"], 0.1 * (1 - ac[steps]))


@pytest.mark.parametrize("mc, msg", [
    (dict(kind="hmc", steps=1), "'ula' or 'mala'"),
    (dict(kind="ula", steps=17), "0 .. 16"),
    (dict(kind="ula", steps=-1), "0 .. 16"),
    (dict(kind="ula", steps=[1, 2]), "2 entries for 25"),
    (dict(kind="ula", steps=1, step_size=[0.1]), "1 entries for 25"),
    (dict(kind="ula", steps=1, step_scale=0.0), "positive and finite"),
    (dict(kind="ula", steps=1, step_scale=float("nan")), "positive and finite"),
    (dict(kind="ula", steps=1, step_size=[float("inf")] * 25), "positive and finite"),
    (dict(kind="ula", steps=1, stepsize=0.1), "unknown keys"),
])
def test_bad_tables_are_refused_with_a_message(mc, msg):
    dm = make(25, sampler="ddpm")
    with pytest.raises(ValueError, match=msg):
        mcmc_tables(mc, dm._ddpm_steps()[0], dm.alphas_cumprod)
    with pytest.raises(TypeError):
        mcmc_tables("mala", dm._ddpm_steps()[0], dm.alphas_cumprod)
    # a step size that is not used (K = 0 there) is not looked at
    ok = mcmc_tables(dict(kind="ula", steps=[0] + [1] * 24, step_size=[float("nan")] + [0.1] * 24), dm._ddpm_steps()[0], dm.alphas_cumprod)
    assert ok["total"] == 24


def test_python_refusals_before_anything_touches_a_device():
    mc = dict(kind="mala", steps=1)
    # DynamicGaussianDiffusionModel
    dyn = make(25, cls="DynamicGaussianDiffusionModel")
    with pytest.raises(NotImplementedError, match="DynamicGaussianDiffusionModel"):
        dyn.conditional_sample({}, mcmc=mc)
    # a caller-supplied sample_fn, on both samplers
    def my_step(*a, **k):
        raise AssertionError("never called")
    with pytest.raises(NotImplementedError, match="sample_fn"):
        make(25, sampler="ddpm").conditional_sample({}, sample_fn=my_step, mcmc=mc)
    with pytest.raises(NotImplementedError, match="sample_fn"):
        make(25, sampler="ddim").conditional_sample({}, sample_fn=my_step, mcmc=mc)
    # predict_epsilon=False: no score, no density to correct
    with pytest.raises(NotImplementedError, match="predict_epsilon"):
        make(25, sampler="ddpm", predict_epsilon=False)._launch(1, None, {}, None, False, [24], [0], [1.0], None, False, mcmc=mc)
    # without mcmc= nothing new is asked of a model
    assert make(25).last_mcmc is None


def _words(seed, offset, n_groups):
    return util.philox_normal(seed, offset, 4 * n_groups)[1].reshape(n_groups, 4)


def test_philox_layout_replicated_in_numpy():
    """The documented layout (ramp_sample_mcmc in include/ramp_hip.h): the main block keeps its elements, the normals of inner step k sit in
    block n_steps + 1 + k, the uniform of (k, global sample g) is word 0 of group (n_steps + 1 + K) T HS / 4 + k T + g; a shard addresses by the
    global sample index, so two halves draw what the whole job draws; the wrapper's offset accounting matches."""
    seed, offset, n_steps, K, T, HS = 77, 1000, 25, 3, 4, H * S
    plain, _ = util.philox_normal(seed, offset, (n_steps + 1) * T * HS)
    whole, _ = util.philox_normal(seed, offset, (n_steps + 1 + K) * T * HS)
    assert np.array_equal(whole[:plain.size], plain)                       # the main block is what a job without inner steps draws
    blocks = whole.reshape(n_steps + 1 + K, T, HS)
    g0 = (n_steps + 1 + K) * T * HS // 4
    w = _words(seed, offset + g0, K * T)[:, 0].reshape(K, T)
    u = ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert ((u > 0) & (u < 1)).all() and u.dtype == np.float32
    for s0, B in ((0, 2), (2, 2), (1, 3)):
        # element ((n_steps + 1 + k) T + s0 + b) HS + e of the stream, whatever the shard
        for k in range(K):
            for b in range(B):
                first = ((n_steps + 1 + k) * T + s0 + b) * HS
                z, _ = util.philox_normal(seed, offset + first // 4, HS)
                assert np.array_equal(z, blocks[n_steps + 1 + k, s0 + b])
                assert _words(seed, offset + g0 + k * T + s0 + b, 1)[0, 0] == w[k, s0 + b]
    # the wrapper's accounting: a job with inner steps advances past its normals and uniforms, a plain job as ever
    dm = make(25, sampler="ddpm", noise_source="philox", noise_seed=seed)
    dm._philox_offset = offset
    assert dm._philox_block(T, n_steps, False, K) == (seed, offset, 0, T)
    assert dm._philox_offset == offset + g0 + K * T
    dm._philox_offset = offset
    dm._philox_block(T, n_steps, False)
    assert dm._philox_offset == offset + (n_steps + 1) * T * HS // 4
    dm.set_noise_shard(2, T)
    dm._philox_offset = offset
    assert dm._philox_block(2, n_steps, False, K) == (seed, offset, 2, T) and dm._philox_offset == offset + g0 + K * T


def test_mcmc_params_layout_matches_the_header():
    """{int32 kind, int32 reserved, three pointers}: 32 bytes, fields in the header's order; RAMP_MCMC_MAX_INNER is 16 on both sides."""
    assert C.sizeof(_lib.RampMcmcParams) == 32
    assert [getattr(_lib.RampMcmcParams, f).offset for f, _ in _lib.RampMcmcParams._fields_] == [0, 4, 8, 16, 24]
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    body = re.search(r"typedef struct ramp_mcmc_params \{(.*?)\} ramp_mcmc_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\*?\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.RampMcmcParams._fields_]
    assert int(re.search(r"#define RAMP_MCMC_MAX_INNER (\d+)", hdr).group(1)) == _lib.MCMC_MAX_INNER == 16
    assert _lib.MCMC_KINDS == {"ula": 1, "mala": 2}


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    lib = _lib.load()
    for name, n_args in (("ramp_sample_mcmc", 12), ("ramp_score_energy", 9), ("ramp_row_energy", 5), ("ramp_combine_energy", 7),
                         ("ramp_mcmc_propose", 12), ("ramp_mcmc_accept", 19)):
        assert re.search(rf"\bint {name}\s*\(", hdr), f"{name} not declared"
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == n_args, name
        assert hasattr(lib, name), f"{name} not exported"
    assert _lib.PROTOTYPES["ramp_sample_mcmc"][1][2] == C.POINTER(_lib.RampMcmcParams)
    assert _lib.PROTOTYPES["ramp_sample_mcmc"][1][3] == C.POINTER(_lib.RampGuidanceRows)
    assert _lib.PROTOTYPES["ramp_sample_mcmc"][1][4] == C.POINTER(_lib.RampSceneBatch)


def test_model_classes_expose_the_accessors():
    from ramp_amd.models import GaussianDiffusionModel3d, StaticGaussianDiffusionModel, TemporalUnetInference
    assert callable(TemporalUnetInference.energy) and callable(StaticGaussianDiffusionModel.energy) and callable(GaussianDiffusionModel3d.energy)
    assert make(25, cfg_weight=2.0)._comb_weights() == [3.0, -2.0]
    assert make(25, compose=True, compose_weights=(2.0, 1.5))._comb_weights() == [2.0, 1.5, -2.5]
    with pytest.raises(ValueError, match="one timestep for all rows"):
        TemporalUnetInference(n_support_points=H, state_dim=S).energy(torch.zeros(2, H, S), torch.tensor([1, 2]), obstacle_pts=torch.zeros(2, 1, 4, 2))


def test_oracle_fixture_is_the_oracles_and_satisfies_the_mala_conditions():
    """tests/golden/mcmc_oracle64.npz (ramp_amd/tools/make_mcmc_goldens.py): one entry recomputed with the float64 oracle of
    tests/test_gpu_mcmc.py; the oracle ALONE satisfies what test 4 asks of the compared decisions -- at most 10 % within MALA_DELTA of the
    threshold, at least a quarter accepted and a quarter rejected -- and MALA_DELTA, ULA_F32_DRIFT are the fixture's measured values."""
    import test_gpu_mcmc as G
    fx = np.load(os.path.join(ROOT, "tests", "golden", "mcmc_oracle64.npz"))
    x, flags, la, lu = G.mala_oracle_case(np.float64, 0, 24, 1, G.MALA_STEP_SCALE)
    assert np.array_equal(flags, fx["mala/K1/t0/flags"]) and np.allclose(la, fx["mala/K1/t0/la"], rtol=0, atol=1e-9)
    assert np.abs(x - fx["mala/K1/t0/x"]).max() < 1e-12
    assert 4 * float(fx["mala/dmax32"]) <= G.MALA_DELTA <= 4.1 * float(fx["mala/dmax32"])
    for K in (1, 2):
        n = acc = out = 0
        for t, j in G.MALA_CASES:
            _, _, _, _, u = G.mala_case_inputs(j, K)
            la, f = fx[f"mala/K{K}/t{t}/la"], fx[f"mala/K{K}/t{t}/flags"]
            sure = np.abs(la - np.log(u.astype(np.float64))) >= G.MALA_DELTA
            n += f.size; out += int((~sure).sum()); acc += int(f[sure].sum())
        assert out <= 0.1 * n and acc >= 0.25 * (n - out) and (n - out - acc) >= 0.25 * (n - out), (K, n, out, acc)
    for kind in ("ddpm", "ddim"):
        d = float(fx[f"ula/{kind}/drift32"])
        assert d <= G.ULA_F32_DRIFT[kind] <= 1.01 * d, (kind, d)
        assert fx[f"ula/{kind}/chain"].shape == ((26 if kind == "ddpm" else 6), 4, 48, 4) and fx[f"ula/{kind}/chain"].dtype == np.float64
    # test 4b's cases: the oracle alone leaves out at most 10 % and has both outcomes among the rest
    for kind in G.COMP_KINDS:
        delta, n, out, acc = 4.0 * float(fx[f"comp/{kind}/dmax32"]), 0, 0, 0
        for t, j in G.MALA_CASES:
            la, f = fx[f"comp/{kind}/t{t}/la"], fx[f"comp/{kind}/t{t}/flags"]
            u = G.mala_case_inputs(j, 1)[4][:, :f.shape[1]]
            sure = np.abs(la - np.log(u.astype(np.float64))) >= delta
            n += f.size; out += int((~sure).sum()); acc += int(f[sure].sum())
        assert 0 < delta < 1e-2 and out <= 0.1 * n and 0 < acc < n - out, (kind, delta, n, out, acc)
    # every measured bar of test 1 is in the fixture
    for key in ["energy/f32rel/2_8_0", "energy/f32rel/4_48_0", "energy/f32rel/16_64_0", "energy/f32rel/6_48_1", "energy/fixture/2d_h48/f32rel",
                "energy/fixture/3d_h48/f32rel", "energy/fixture/2d_h48/refrel", "energy/fixture/3d_h48/refrel"]:
        assert 0 < float(fx[key]) < 1e-5, key
    assert fx["ula/ddim/drift32_states"].shape == (6,)
