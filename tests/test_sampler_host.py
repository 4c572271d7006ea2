"""The samplers' host layer without a device: the one DDIM rule, the schedule / APF fillers of ramp_sample_params, the Philox
block accounting and the content-keyed scene cache (ramp_amd/diffusion.py, ramp_amd/unet.py)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from ramp_amd import _lib
from ramp_amd.diffusion import DDIM_FIELDS, _HostArrays

H, S = 48, 4
DDPM_FIELDS = ("coef1", "coef2", "stdv", "use_noise", "noise_scale")


def make(T, cls="StaticGaussianDiffusionModel", **kw):
    from ramp_amd import models
    return getattr(models, cls)(model=models.TemporalUnetInference(n_support_points=H, state_dim=S), n_diffusion_steps=T,
                                predict_epsilon=True, **kw)


def bits(values):
    """float32 cast of a list of Python / 0-d tensor scalars, as its bit pattern."""
    return np.array([float(v) for v in values], np.float32).view(np.int32)


def host(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n,)).copy()


def reference_ddim_step(dm, t, K):
    """diffusion_model_static.py:259-333 for one step with eta = 0 and use_clipped_model_output, in the reference's names, on the
    wrapper's own buffers."""
    eta = 0.0
    prev_timestep = t - dm.n_diffusion_steps // K
    alpha_prod_t = dm.alphas_cumprod[t]
    alpha_prod_t_prev = dm.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else dm.final_alpha_cumprod[0]
    beta_prod_t = 1 - alpha_prod_t
    variance = (1 - alpha_prod_t_prev) / (1 - alpha_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)
    std_dev_t = eta * variance ** (0.5)
    return dict(sqrt_recip=dm.sqrt_recip_alphas_cumprod[t], sqrt_recipm1=dm.sqrt_recipm1_alphas_cumprod[t],      # x0 from eps, :109-118
                sqrt_a_t=alpha_prod_t ** (0.5), sqrt_1m_a_t=beta_prod_t ** (0.5),                                # :325
                sqrt_a_prev=alpha_prod_t_prev ** (0.5), dir_coef=(1 - alpha_prod_t_prev - std_dev_t ** 2) ** (0.5)     # :328-331
                ), prev_timestep, alpha_prod_t_prev


@pytest.mark.parametrize("T,K,tail", [(25, 5, None), (25, 8, None), (100, 10, None), (100, 10, 5)])
def test_ddim_rule_is_the_references_and_dir_coef_needs_no_variance_term(T, K, tail):
    """The six per-step coefficients equal the reference's expressions bitwise (as float32); and on every step in use the
    eta = 0 variance term changes nothing: dir_coef == (1 - alpha_prev) ** 0.5 bitwise, the form three removed copies used."""
    dm = make(T)
    steps = [int(i) for i in dm.ddim_set_timesteps(K)]
    if tail:
        steps = steps[-tail:]          # the planner's low-level tail of the high-level schedule
    got = dm._ddim_coefficients(steps, K)
    assert tuple(got) == DDIM_FIELDS and all(len(v) == len(steps) for v in got.values())
    ref = [reference_ddim_step(dm, t, K) for t in steps]
    for k in DDIM_FIELDS:
        assert np.array_equal(bits(got[k]), bits([r[0][k] for r in ref])), k
    assert np.array_equal(bits(got["dir_coef"]), bits([(1 - r[2]) ** 0.5 for r in ref]))
    assert np.isfinite(np.array([[float(v) for v in got[k]] for k in DDIM_FIELDS])).all()
    if (T, K) == (25, 5):
        assert any(r[1] < 0 for r in ref)          # the final_alpha_cumprod case
    # the same lists are what the DDIM job is fed, and nothing of the DDPM tables
    p, arrays = _lib.RampSampleParams(), _HostArrays()
    dm._fill_schedule(p, arrays, True, steps, None, K)
    assert (p.n_steps, p.ddim) == (len(steps), 1) and list(host(p.t, len(steps))) == steps
    for k in DDIM_FIELDS:
        assert np.array_equal(host(getattr(p, k), len(steps)).view(np.int32), bits(got[k])), k
    assert not any(bool(getattr(p, k)) for k in DDPM_FIELDS)


def test_ddpm_schedule_tables():
    T, extra = 25, 2
    dm = make(T, sampler="ddpm")
    steps, raw = dm._ddpm_steps(extra)
    assert raw == list(range(T - 1, -extra - 1, -1)) and steps == [max(i, 0) for i in raw] and steps[-3:] == [0, 0, 0]
    n = len(steps)
    scale = [0.5 + 0.01 * j for j in range(n)]
    p, arrays = _lib.RampSampleParams(), _HostArrays()
    dm._fill_schedule(p, arrays, False, steps, scale)
    assert (p.n_steps, p.ddim) == (n, 0)
    t = host(p.t, n)
    assert list(t) == steps
    assert np.array_equal(host(p.use_noise, n), (t != 0).astype(np.int32))
    assert np.array_equal(host(p.stdv, n).view(np.int32), bits([torch.exp(0.5 * dm.posterior_log_variance_clipped[i]) for i in steps]))
    for field, buf in (("coef1", dm.posterior_mean_coef1), ("coef2", dm.posterior_mean_coef2),
                       ("sqrt_recip", dm.sqrt_recip_alphas_cumprod), ("sqrt_recipm1", dm.sqrt_recipm1_alphas_cumprod)):
        assert np.array_equal(host(getattr(p, field), n).view(np.int32), bits([buf[i] for i in steps])), field
    assert np.array_equal(host(p.noise_scale, n).view(np.int32), bits(scale))
    assert not any(bool(getattr(p, k)) for k in DDIM_FIELDS[2:])          # the DDIM-only fields stay NULL


def test_apf_filler_one_cloud_and_scene_batch():
    dm = make(25, sampler="ddpm", use_apf=True)
    cloud = torch.rand(6, 64, 2)
    for cfg, passes in ((dict(dm.apf_ddpm), 1), (dict(dm.apf_ddim), 3)):       # `passes` absent -> 1
        one, arrays = _lib.RampSampleParams(), _HostArrays()
        dm._fill_apf(one, arrays, cfg, cloud)
        many, batch = _lib.RampSampleParams(), _lib.RampSceneBatch()
        job = dict(cloud_points=torch.rand(6 * 64 + 3 * 64, 2), cloud_offset=np.array([0, 384, 576], np.int32))
        dm._fill_apf(many, arrays, cfg, None, batch, job)
        for p in (one, many):
            a = p.apf
            assert (a.window, a.threshold, a.strength, a.passes) == (cfg["window"], cfg["threshold"], cfg["strength"], passes)
            assert np.array_equal(host(a.window_weights_host, 2 * a.window + 1), dm._window_weights(cfg["window"]).numpy())
        assert one.apf.n_points == 6 * 64 and one.apf.cloud and not batch.traj_scene
        assert not many.apf.cloud and batch.cloud_points == job["cloud_points"].data_ptr()
        assert list(host(batch.cloud_offset_host, 3)) == [0, 384, 576]
    # compose: the field is scene A's six obstacles + scene B's first four
    dc = make(100, compose=True, use_apf=True)
    two = torch.rand(2, 6, 64, 2)
    p, arrays = _lib.RampSampleParams(), _HostArrays()
    dc._fill_apf(p, arrays, dict(dc.apf_ddim), two)
    assert p.apf.n_points == (6 + 4) * 64
    pts = host(C.cast(p.apf.cloud, _lib.c_f32p), 2 * p.apf.n_points).reshape(-1, 2)
    assert np.array_equal(pts, torch.cat([two[0], two[1][:4]]).reshape(-1, 2).numpy())
    assert torch.equal(dc._compose_apf_cloud(two), torch.from_numpy(pts))


def test_philox_block_accounting():
    B, T = 4, 25
    block = lambda n_noise, total: (n_noise * total * H * S + 3) // 4
    dm = make(T, sampler="ddpm", noise_source="philox", noise_seed=9)
    assert dm._philox_block(B, T, False) == (9, 0, 0, B) and dm.last_philox == (9, 0, (T + 1) * B * H * S)
    off = block(T + 1, B)
    assert dm._philox_offset == off
    assert dm._philox_block(B, T, False) == (9, off, 0, B) and dm._philox_offset == 2 * off
    assert dm._philox_block(B, 5, True) == (9, 2 * off, 0, B)               # DDIM: x_T only
    assert dm.last_philox == (9, 2 * off, B * H * S) and dm._philox_offset == 2 * off + block(1, B)
    # shards of a job of 8: every shard advances by the WHOLE job's block
    for s0 in (0, 4):
        sh = make(T, sampler="ddpm", noise_source="philox", noise_seed=9)
        sh.set_noise_shard(s0, 8)
        assert sh._philox_block(B, T, False) == (9, 0, s0, 8) and sh._philox_offset == block(T + 1, 8)
        assert sh.last_philox == (9, 0, (T + 1) * 8 * H * S)
        assert sh._philox_block(B, T, False) == (9, block(T + 1, 8), s0, 8) and sh._philox_offset == 2 * block(T + 1, 8)
    for s0, total in ((6, 8), (-1, 8), (0, 3)):
        before = (dm._philox_offset, dm.last_philox)
        dm.set_noise_shard(s0, total)
        with pytest.raises(ValueError):
            dm._philox_block(B, T, False)
        assert (dm._philox_offset, dm.last_philox) == before


@pytest.fixture
def no_device(monkeypatch):
    """The C ABI answers 'ok' to everything and there is no HIP device to select: set_scene / set_scenes run on CPU tensors."""
    class Lib:
        def __getattr__(self, name):
            return lambda *args: 0
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    monkeypatch.setattr(_lib, "current_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())


def test_scene_cache(no_device, monkeypatch):
    dm = make(100, cls="DynamicGaussianDiffusionModel")          # (its row pattern depends on the batch's parity)
    u = dm.model
    n = dict(encode=0, equal=0)
    real_equal = torch.equal

    def encode(cloud):
        n["encode"] += 1
        return torch.zeros(1, u.context_dim)

    def equal(a, b):
        n["equal"] += 1
        return real_equal(a, b)

    u.ctx, u.encode_scene = (lambda: None), encode
    monkeypatch.setattr(torch, "equal", equal)
    forgotten = lambda: all(v is None for v in vars(u.scene_cache).values())

    def prepare(cloud, B=4):
        before = dict(n)
        dm._prepare_scene(cloud, B)
        return n["encode"] - before["encode"], n["equal"] - before["equal"]

    cloud = torch.rand(6, 64, 2)
    assert forgotten() and prepare(cloud) == (1, 0)
    assert prepare(cloud) == (0, 0)                                  # same object, same _version: no comparison at all
    assert prepare(cloud.clone()) == (0, 1)                          # equal content in a new object
    other = torch.rand(6, 64, 2)
    assert prepare(other) == (1, 1)                                  # different content
    assert prepare(other) == (0, 0)
    other.add_(1.0)
    assert prepare(other) == (1, 1)                                  # modified in place: _version moved
    assert prepare(other.double())[0] == 1                           # same values, another dtype
    assert prepare(other.double(), B=4)[0] == 0 and prepare(other.double(), B=3)[0] == 1      # another row pattern
    same = other.double()
    assert prepare(same, B=3) == (0, 1) and prepare(same, B=3) == (0, 0)
    u.scene_cache.clear()
    assert forgotten() and prepare(same, B=3) == (1, 0)
    lat = torch.zeros(2, u.context_dim)
    for forget in (lambda: u.set_scene(lat, [0, 1]), lambda: u.set_scenes(lat, [0, 1, 0, 1]), u.reset_cache, u.invalidate_scene,
                   dm.invalidate_scene):
        assert prepare(same, B=3) == (0, 0) and not forgotten()
        forget()
        assert forgotten()                                           # nothing of the last cloud survives, its identity included
        assert prepare(same, B=3) == (1, 0)
