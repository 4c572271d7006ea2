"""Many scenes in one job, kernel level: the row constant of the fused kernels with more variants than their LDS table holds
(ramp_op_ato / ramp_op_tkl / ramp_op_tkl16, n_var in {5, 9, 65, 1025}, a random row -> variant table) against float64, and the
per-scene APF (ramp_apf_scenes) bit for bit against ramp_apf run once per cloud.  Shapes and bars are those of the n_var = 3
cases in tests/test_gpu_ops.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from ramp_amd import _lib
from util import GOLDEN, dev, rel

pytestmark = pytest.mark.gpu

N_VARS = [5, 9, 65, 1025]


def _p(t):
    return _lib.ptr(t) if t is not None else None


def _random_rowvar(n_rows, n_var, gen):
    """A random (not cyclic) table that uses the first and the last variant."""
    rv = torch.randint(0, n_var, (n_rows,), generator=gen).to(torch.int32)
    rv[0], rv[-1] = n_var - 1, 0
    return rv.cuda()


@pytest.mark.parametrize("n_var", N_VARS)
@pytest.mark.parametrize("M", [293, 70000])
@pytest.mark.parametrize("entry", ["ramp_op_tkl16", "ramp_op_tkl"])
def test_tkl_row_constant_with_many_variants_against_float64(M, n_var, entry):
    """The attention output projection's epilogue (bias + residual + row constant, N = 256) of test_tkl_token_owning_linear_against_float64's
    epi = 3 cases -- M = 293 and 70000, neither a multiple of the 128-token tile, L = 6 -- with the constants read from global memory:
    the same 3e-6 bar against float64, the recorded maximum exact, a stale maximum trips the guard, and a table that points every
    row at variant 0 is seen (mutation)."""
    gen = torch.Generator(device="cpu").manual_seed(M + 256 + n_var)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    L, N = 6, 256
    X, W = r(M, 256, sc=1.3) + 0.2, r(N, 256, sc=1 / 16)
    bias, resid, rowbias = r(N, sc=0.3), r(M, N), r(n_var, N, sc=0.5)
    rowvar = _random_rowvar((M + L - 1) // L, n_var, gen)
    xd = X.double()
    ref = (xd @ W.double().T + bias.double() + resid.double() + rowbias.double()[rowvar.long()[torch.arange(M, device="cuda") // L]]).cpu().numpy()
    xmax = xd.abs().max().item()
    Y = torch.empty(M, N, device="cuda")
    out, flag = C.c_float(0), C.c_int32(0)

    def go(prev, rv=rowvar):
        Y.fill_(float("nan"))
        _lib.check(getattr(_lib.load(), entry)(_p(X), _p(W), _p(bias), _p(resid), _p(rowbias), _p(rv), n_var, L, None, None,
                                               M, N, prev, _p(Y), C.byref(out), C.byref(flag), None), entry)
        return rel(Y.double().cpu().numpy(), ref)

    e = go(0.0)
    print(f"{entry} M={M} n_var={n_var}: {e:.2e}")
    assert e < 3e-6 and flag.value == 0, (e, flag.value)
    assert abs(out.value - xmax) <= 1e-6 * xmax, (out.value, xmax)
    e2 = go(out.value)
    assert e2 < 3e-6 and flag.value == 0, (e2, flag.value)
    go(xmax / 4096.0)                                         # operand 2^12 larger than the scale assumes
    assert flag.value == 1, flag.value
    e0 = go(0.0, torch.zeros_like(rowvar))                   # mutation: every row reads variant 0
    assert e0 > 1e-2, e0


def _attention_block_float64(qkv, Wo, bias, resid, rowbias, rowvar, L):
    """resid + to_out(softmax(q k^T / 8) v) + bias + per-row-variant constant in float64 (layers_attention_mini.py:101-127, 132)."""
    M = qkv.shape[0]
    x = qkv.double().reshape(M // L, L, 3, 4, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)      # (R, 4, L, 64)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(M, 256)
    y = resid.double() + o @ Wo.double().T + bias.double()
    y = y + rowbias.double()[rowvar.long()[torch.arange(M, device=qkv.device) // L]]
    return y, o


@pytest.mark.parametrize("n_var", N_VARS)
@pytest.mark.parametrize("L,R", [(48, 4), (24, 7), (12, 33), (6, 131), (16, 5), (32, 3), (4, 9), (3, 50), (1, 100)])
def test_ato_row_constant_with_many_variants_against_float64(L, R, n_var):
    """test_ato_attention_with_output_projection_against_float64's cases that carry the row constant (the same L set, the same sample
    counts that leave the last wave / block partly empty), with n_var > 4: the same bars."""
    M = R * L
    gen = torch.Generator(device="cpu").manual_seed(1000 * L + R + n_var)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    qkv = r(M, 768, sc=1.5)
    qkv[:, 512:] = qkv[:, 512:] * 0.3 + 0.1
    Wo, bias, resid = r(256, 256, sc=1 / 16), r(256, sc=0.3), r(M, 256)
    rowbias = r(n_var, 256, sc=0.5)
    rowvar = _random_rowvar(R, n_var, gen)
    ref, o = _attention_block_float64(qkv, Wo, bias, resid, rowbias, rowvar, L)
    ref = ref.cpu().numpy(); omax = o.abs().max().item()
    Y = torch.empty(M, 256, device="cuda")
    out, flag = C.c_float(0), C.c_int32(0)

    def go(prev, rv=rowvar):
        Y.fill_(float("nan"))
        _lib.check(_lib.load().ramp_op_ato(_p(qkv), _p(Wo), _p(bias), _p(resid), _p(rowbias), _p(rv), n_var, L, M, prev, _p(Y), C.byref(out),
                                           C.byref(flag), None), "ramp_op_ato")
        return rel(Y.double().cpu().numpy(), ref)

    e = go(0.0)
    print(f"ato L={L} R={R} n_var={n_var}: {e:.2e}")
    assert e < 3e-6 and flag.value == 0, (e, flag.value)
    assert abs(out.value - omax) <= 2e-6 * omax, (out.value, omax)
    e2 = go(out.value)
    assert e2 < 3e-6 and flag.value == 0, (e2, flag.value)
    go(omax / 4096.0)
    assert flag.value == 1, flag.value
    e0 = go(0.0, torch.zeros_like(rowvar))                   # mutation: every row reads variant 0
    assert e0 > 1e-2, e0


def test_many_variants_give_the_bits_of_the_lds_table():
    """The same constants through the LDS-staged epilogue (n_var = 4) and through global memory (the same four rows declared as
    n_var = 5): the sums are formed in the same order, so the outputs are bitwise equal."""
    gen = torch.Generator(device="cpu").manual_seed(7)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    L, R = 6, 131
    M = L * R
    rowbias = r(5, 256, sc=0.5)
    rowvar = torch.randint(0, 4, (R,), generator=gen).to(torch.int32).cuda()
    out, flag = C.c_float(0), C.c_int32(0)
    X, W, bias, resid = r(M, 256), r(256, 256, sc=1 / 16), r(256, sc=0.3), r(M, 256)
    for entry in ("ramp_op_tkl16", "ramp_op_tkl"):
        ys = []
        for n_var in (4, 5):
            Y = torch.empty(M, 256, device="cuda")
            _lib.check(getattr(_lib.load(), entry)(_p(X), _p(W), _p(bias), _p(resid), _p(rowbias), _p(rowvar), n_var, L, None, None, M, 256, 0.0,
                                                   _p(Y), C.byref(out), C.byref(flag), None), entry)
            ys.append(Y)
        assert torch.equal(ys[0], ys[1]), entry
    qkv = r(M, 768, sc=1.5)
    ys = []
    for n_var in (4, 5):
        Y = torch.empty(M, 256, device="cuda")
        _lib.check(_lib.load().ramp_op_ato(_p(qkv), _p(W), _p(bias), _p(resid), _p(rowbias), _p(rowvar), n_var, L, M, 0.0, _p(Y), C.byref(out),
                                           C.byref(flag), None), "ramp_op_ato")
        ys.append(Y)
    assert torch.equal(ys[0], ys[1])


# ---- per-scene APF ---------------------------------------------------------------------------------------------------------------
def _apf(traj, cloud, thr, strength, win):
    """ramp_apf in place on a copy (one cloud for all rows)."""
    out = traj.clone()
    w = torch.exp(-0.5 * torch.square(torch.arange(-win, win + 1)) / (win / 2) ** 2).float().contiguous()
    p = _lib.RampApfParams(); p.cloud = _lib.ptr(cloud); p.n_points = cloud.shape[0]; p.window = win
    p.window_weights_host = C.cast(w.data_ptr(), _lib.c_f32p); p.threshold = thr; p.strength = strength; p.passes = 1
    _lib.check(_lib.load().ramp_apf(_lib.ptr(out), out.shape[0], out.shape[1], out.shape[2], C.byref(p), None), "ramp_apf")
    torch.cuda.synchronize()
    return out


def _apf_scenes(traj, clouds, traj_scene, thr, strength, win):
    out = traj.clone()
    w = torch.exp(-0.5 * torch.square(torch.arange(-win, win + 1)) / (win / 2) ** 2).float().contiguous()
    p = _lib.RampApfParams(); p.window = win
    p.window_weights_host = C.cast(w.data_ptr(), _lib.c_f32p); p.threshold = thr; p.strength = strength; p.passes = 1
    pts = torch.cat(clouds).contiguous()
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
    ts = torch.as_tensor(traj_scene, dtype=torch.int32).cuda()
    b = _lib.RampSceneBatch(); b.n_scenes = len(clouds); b.traj_scene = _lib.ptr(ts); b.cloud_points = _lib.ptr(pts)
    b.cloud_offset_host = off.ctypes.data_as(_lib.c_i32p)
    _lib.check(_lib.load().ramp_apf_scenes(_lib.ptr(out), out.shape[0], out.shape[1], out.shape[2], C.byref(p), C.byref(b), None), "ramp_apf_scenes")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["rand", "line", "ends", "big"])
def test_apf_scenes_is_bitwise_the_single_cloud_kernel_per_cloud(name):
    """The trajectories of an apf_cases.npz case against three clouds of different sizes -- the case's own, its first third, and a
    2500-point cloud that spans three LDS tiles -- the scenes interleaved row by row: every row must carry the bits ramp_apf gives
    for that row's cloud alone, and the rows of the case's own cloud the fixture's output within the existing 5e-7 bar."""
    from ramp_amd import synth
    g = np.load(f"{GOLDEN}/apf_cases.npz")
    thr, strength, win = (float(v) for v in g[name + "/params"])
    win = int(win)
    base = g[name + "/traj"]
    traj = dev(np.concatenate([base, base, base]).astype(np.float32))
    own = dev(g[name + "/cloud"].reshape(-1, 2).astype(np.float32))
    clouds = [own, own[: max(1, own.shape[0] // 3)].contiguous(), dev(synth.make_cloud(25, 100, 2, seed=9).reshape(-1, 2).astype(np.float32))]
    assert len({c.shape[0] for c in clouds}) == 3
    B = traj.shape[0]
    scene = np.arange(B) % 3
    out = _apf_scenes(traj, clouds, scene, thr, strength, win)
    moved = 0
    for s, c in enumerate(clouds):
        rows = np.nonzero(scene == s)[0]
        single = _apf(traj[rows].contiguous(), c, thr, strength, win)
        assert torch.equal(out[rows], single), (name, s)
        moved += int((single != traj[rows]).any())
    assert moved >= 1                                          # the comparison is not between untouched trajectories
    nb = base.shape[0]
    own_rows = np.nonzero(scene == 0)[0]
    ref = np.concatenate([g[name + "/out"]] * 3)[own_rows]
    assert np.abs(out[own_rows].cpu().numpy() - ref).max() < 5e-7
    assert torch.equal(out[..., 2:], traj[..., 2:]) and nb > 0


def test_apf_scenes_refuses_bad_tables():
    traj = torch.zeros(2, 8, 4, device="cuda")
    w = torch.ones(3).contiguous()
    p = _lib.RampApfParams(); p.window = 1; p.window_weights_host = C.cast(w.data_ptr(), _lib.c_f32p); p.threshold = 0.1; p.strength = 0.1; p.passes = 1
    pts = torch.zeros(4, 2, device="cuda"); ts = torch.zeros(2, dtype=torch.int32, device="cuda")
    b = _lib.RampSceneBatch(); b.n_scenes = 2; b.traj_scene = _lib.ptr(ts); b.cloud_points = _lib.ptr(pts)
    off = np.array([0, 4, 4], dtype=np.int32)                  # scene 1 is empty
    b.cloud_offset_host = off.ctypes.data_as(_lib.c_i32p)
    assert _lib.load().ramp_apf_scenes(_lib.ptr(traj), 2, 8, 4, C.byref(p), C.byref(b), None) != 0
    assert b"at least one cloud point" in _lib.load().ramp_last_error()
    off[:] = [0, 2, 4]
    p.cloud = _lib.ptr(pts)                                    # apf.cloud must be NULL
    assert _lib.load().ramp_apf_scenes(_lib.ptr(traj), 2, 8, 4, C.byref(p), C.byref(b), None) != 0
