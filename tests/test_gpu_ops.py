"""Kernel-level parity: each HIP kernel (through the C ABI) against the oracle's function of the same name,
and against the reference fixtures where they exist (APF, costs)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ramp_oracle as O
from ramp_amd import _lib
from util import GOLDEN, dev, rel

pytestmark = pytest.mark.gpu


def S():
    return _lib.current_stream()


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@pytest.mark.parametrize("M,N,K,taps,L", [
    (96, 256, 256, 1, 1), (1000, 768, 256, 1, 1), (333, 2048, 256, 1, 1), (257, 256, 1024, 1, 1),
    (48 * 5, 32, 32, 5, 48), (24 * 7, 64, 32, 5, 24), (6 * 11, 128, 512, 5, 6), (12 * 9, 64, 128, 5, 12),
    (130, 32, 256, 1, 1), (64 * 3, 32, 32, 5, 64), (777, 160, 64, 1, 1), (12 * 50, 512, 64, 3, 12), (129, 768, 2048, 1, 1),
    (48 * 20, 256, 128, 5, 48), (1000, 128, 32, 1, 1),
    # "same" k = 5 convolutions on samples shorter than the kernel and at odd lengths (the level lengths of H = 8, 16, 24, 32, 56):
    # a tap that is not masked at a sample edge reads the neighbouring sample
    (1 * 37, 64, 64, 5, 1), (2 * 29, 128, 64, 5, 2), (3 * 21, 256, 128, 5, 3), (4 * 19, 64, 32, 5, 4), (7 * 13, 256, 256, 5, 7),
    (56 * 3, 32, 32, 5, 56),
])
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "bf16x6-lds", "fp16x3"])
def test_gemm_taps(M, N, K, taps, L, backward, mode):
    """C = sum_tap shift(A) W_tap^T + bias + resid vs float64 numpy within fp32 rounding, on every GEMM kernel: the
    exact-fp32 MFMA mode, the pipelined bf16x6 mode (fragment-packed weights), its LDS-staged predecessor and the
    fp16x3 mode the bench times (unscaled operand here; shapes a split kernel does not cover run fp32)."""
    g = rng(M + N + K)
    A = g.standard_normal((M, K), dtype=np.float32)
    W = (g.standard_normal((taps, N, K), dtype=np.float32) / np.sqrt(K * taps)).astype(np.float32)
    bias = g.standard_normal(N, dtype=np.float32)
    resid = g.standard_normal((M, N), dtype=np.float32)
    shift0, step = ((taps // 2, -1) if backward else (-(taps // 2), 1)) if taps > 1 else (0, 0)
    ref = np.zeros((M, N))
    A3 = A.reshape(M // L, L, K).astype(np.float64)
    for j in range(taps):
        sh = shift0 + j * step
        Ash = np.zeros_like(A3)
        if sh >= 0:
            Ash[:, :L - sh] = A3[:, sh:]
        else:
            Ash[:, -sh:] = A3[:, :L + sh]
        ref += Ash.reshape(M, K) @ W[j].astype(np.float64).T
    ref += bias + resid
    out = torch.empty((M, N), device="cuda")
    dA, dW, db, dr = dev(A), dev(W), dev(bias), dev(resid)
    _, flag = _lib.op_gemm(dA, dW, db, dr, out, M, N, K, taps, shift0, step, L, mode=mode)
    assert flag == 0
    assert rel(out.cpu().numpy(), ref) < 3e-6


@pytest.mark.parametrize("M,N,K,resid", [(70000, 768, 256, False), (66000, 1024, 256, False), (200000, 256, 768, False),
                                         (200000, 256, 256, True)])
def test_gemm_fp16x3_launch_rules_at_scale(M, N, K, resid):
    """The fp16x3 launch rules that only many-tile launches reach (launch_x6, gemm.hip): a bias-only linear with at least
    3072 tiles of 64 x 256 runs the three-blocks-per-CU kernel built with only that epilogue; with a residual it stays on
    the two-block kernel.  Same bar as the small shapes, against float64 on the device; the launch repeats bit for bit."""
    gen = torch.Generator(device="cuda"); gen.manual_seed(M + N + K)
    A = torch.randn(M, K, device="cuda", generator=gen)
    W = torch.randn(1, N, K, device="cuda", generator=gen) / np.sqrt(K)
    bias = torch.randn(N, device="cuda", generator=gen)
    R = torch.randn(M, N, device="cuda", generator=gen) if resid else None
    out = torch.empty(M, N, device="cuda"); out2 = torch.empty(M, N, device="cuda")
    _, flag = _lib.op_gemm(A, W, bias, R, out, M, N, K, 1, 0, 0, 1, mode="fp16x3")
    _lib.op_gemm(A, W, bias, R, out2, M, N, K, 1, 0, 0, 1, mode="fp16x3")
    assert flag == 0 and torch.equal(out, out2)
    worst = 0.0
    for r0 in range(0, M, 50000):                              # float64 reference in row blocks
        ref = A[r0:r0 + 50000].double() @ W[0].double().T + bias.double()
        if resid:
            ref += R[r0:r0 + 50000].double()
        worst = max(worst, float((out[r0:r0 + 50000].double() - ref).abs().max() / ref.abs().max()))
    assert worst < 3e-6, worst


@pytest.mark.parametrize("R,L,C", [(3, 48, 32), (5, 24, 64), (2, 12, 128), (7, 6, 256), (2, 64, 32), (3, 8, 256), (2, 24, 32),
                                   (5, 1, 256), (3, 2, 128), (4, 7, 256)])
@pytest.mark.parametrize("mish", [0, 1])
def test_groupnorm_fwd_bwd(R, L, C, mish):
    g = rng(R * L + C + mish)
    x = (g.standard_normal((R, L, C)) * 1.5 + 0.3).astype(np.float32)
    gam = (1 + 0.1 * g.standard_normal(C)).astype(np.float32); bet = (0.1 * g.standard_normal(C)).astype(np.float32)
    tb = g.standard_normal(C).astype(np.float32); res = g.standard_normal((R, L, C)).astype(np.float32)
    dy = g.standard_normal((R, L, C)).astype(np.float32)
    eps = 1e-6 if not mish else 1e-5
    n, cache = O.groupnorm_fwd(x.astype(np.float64), gam, bet, 8, eps)
    y_ref = (O.mish(n) if mish else n) + tb + res
    dn = dy * (O.mish_grad(n) if mish else 1.0)
    dx_ref = O.groupnorm_bwd(dn, gam.astype(np.float64), cache) + res
    y = torch.empty((R, L, C), device="cuda"); st = torch.empty((R, 8, 2), device="cuda"); dx = torch.empty_like(y)
    lib = _lib.load()
    d = {k: dev(v) for k, v in dict(x=x, gam=gam, bet=bet, tb=tb, res=res, dy=dy).items()}
    _lib.check(lib.ramp_op_groupnorm(_lib.ptr(d["x"]), _lib.ptr(d["gam"]), _lib.ptr(d["bet"]), _lib.ptr(d["tb"]),
                                     _lib.ptr(d["res"]), _lib.ptr(y), _lib.ptr(st), R, L, C, eps, mish, S()))
    _lib.check(lib.ramp_op_groupnorm_bwd(_lib.ptr(d["dy"]), _lib.ptr(d["x"]), _lib.ptr(st), _lib.ptr(d["gam"]),
                                         _lib.ptr(d["bet"]), _lib.ptr(d["res"]), _lib.ptr(dx), R, L, C, mish, S()))
    assert rel(y.cpu().numpy(), y_ref) < 3e-6
    assert rel(dx.cpu().numpy(), dx_ref) < 5e-6


# every GroupNorm kernel: the C = 16 kernel (two groups per float4), the 32 .. 256 kernel and its C = 512 variant (a wave holds 4 of
# the 8 groups) at their L * C <= 4096 limit and below
GN_SHAPES = ([(16, L) for L in (8, 16, 24, 40, 48, 56, 64, 256)] + [(512, L) for L in (1, 2, 3, 5, 6, 7, 8)] +
             [(C, 4096 // C) for C in (32, 64, 128, 256)])
GN_R = 5                     # rows = blocks
U32 = 2.0 ** -24


def gn_input(g, R, L, C, cond):
    x = g.standard_normal((R, L, C)) * 1.5 + 0.3
    if cond == "offset":         # |mean| / std = 2000: a one-pass variance (E x^2 - mean^2) loses all of it in fp32
        x = 100.0 + 0.05 * g.standard_normal((R, L, C))
    elif cond.startswith("eps"):  # even groups near-constant (variance 1e-7 << eps): rstd is set by eps
        xg = x.reshape(R, L, 8, C // 8)
        xg[:, :, 0::2] = 3e-4 * g.standard_normal(xg[:, :, 0::2].shape)
    elif cond == "outlier":      # group 3 ten times its neighbours in spread and offset: leakage across groups shows
        xg = x.reshape(R, L, 8, C // 8)
        xg[:, :, 3] = xg[:, :, 3] * 10.0 + 5.0
    return x.astype(np.float32)


@pytest.mark.parametrize("cond", ["normal", "offset", "eps1e-5", "eps1e-6", "outlier"])
def test_groupnorm_every_width_and_epilogue(cond):
    """GroupNorm forward (+ time bias, + residual, Mish on / off) and its input gradient (+ add on / off) at every width the
    network uses, against float64, with the per-group statistics compared too.  Bars: 3e-6 forward, 5e-6 backward, 2e-6 for
    (mean, rstd); where |mean| * rstd = kappa is large (the offset inputs) the output bars are 8 u kappa, the rounding of the
    fp32 mean itself, while the statistics keep 2e-6."""
    eps = 1e-6 if cond == "eps1e-6" else 1e-5
    lib = _lib.load()
    worst = {"y": (0.0, None), "dx": (0.0, None), "mean": (0.0, None), "rstd": (0.0, None)}
    for C, L in GN_SHAPES:
        R = GN_R
        g = rng(C * 1000 + L + len(cond))
        x = gn_input(g, R, L, C, cond)
        gam = (1 + 0.1 * g.standard_normal(C)).astype(np.float32); bet = (0.1 * g.standard_normal(C)).astype(np.float32)
        tb = g.standard_normal(C).astype(np.float32); res = g.standard_normal((R, L, C)).astype(np.float32)
        dy = g.standard_normal((R, L, C)).astype(np.float32); add = g.standard_normal((R, L, C)).astype(np.float32)
        x64 = x.astype(np.float64)
        n, cache = O.groupnorm_fwd(x64, gam, bet, 8, eps)
        mean_ref = x64.reshape(R, L, 8, C // 8).mean(axis=(1, 3))
        rstd_ref = cache[1].reshape(R, 8)
        kappa = float((np.abs(mean_ref) * rstd_ref).max())
        bar_y, bar_dx = max(3e-6, 8 * U32 * kappa), max(5e-6, 8 * U32 * kappa)
        d = {k: dev(v) for k, v in dict(x=x, gam=gam, bet=bet, tb=tb, res=res, dy=dy, add=add).items()}
        y = torch.empty((R, L, C), device="cuda"); dx = torch.empty_like(y)
        for mish in (0, 1):
            act = O.mish(n) if mish else n
            dn = dy * (O.mish_grad(n) if mish else 1.0)
            dx0 = O.groupnorm_bwd(dn, gam.astype(np.float64), cache)
            for use_tb in (False, True):
                for use_res in (False, True):
                    st = torch.full((R, 8, 2), float("nan"), device="cuda")
                    _lib.check(lib.ramp_op_groupnorm(_lib.ptr(d["x"]), _lib.ptr(d["gam"]), _lib.ptr(d["bet"]),
                                                     _lib.ptr(d["tb"]) if use_tb else None, _lib.ptr(d["res"]) if use_res else None,
                                                     _lib.ptr(y), _lib.ptr(st), R, L, C, eps, mish, S()))
                    y_ref = act + (tb if use_tb else 0.0) + (res if use_res else 0.0)
                    sth = st.cpu().numpy()
                    tag = (C, L, mish, use_tb, use_res)
                    for key, got, ref, bar in (("y", y.cpu().numpy(), y_ref, bar_y), ("mean", sth[..., 0], mean_ref, 2e-6),
                                               ("rstd", sth[..., 1], rstd_ref, 2e-6)):
                        err = rel(got, ref)
                        worst[key] = max(worst[key], (err, tag), key=lambda t: t[0])
                        assert err < bar, (key, tag, err, bar)
                    for use_add in (False, True):
                        _lib.check(lib.ramp_op_groupnorm_bwd(_lib.ptr(d["dy"]), _lib.ptr(d["x"]), _lib.ptr(st), _lib.ptr(d["gam"]),
                                                             _lib.ptr(d["bet"]), _lib.ptr(d["add"]) if use_add else None,
                                                             _lib.ptr(dx), R, L, C, mish, S()))
                        err = rel(dx.cpu().numpy(), dx0 + (add if use_add else 0.0))
                        worst["dx"] = max(worst["dx"], (err, tag + (use_add,)), key=lambda t: t[0])
                        assert err < bar_dx, ("dx", tag, use_add, err, bar_dx)
    print(f"groupnorm {cond}: " + ", ".join(f"{k} {v[0]:.2e} at {v[1]}" for k, v in worst.items()))


@pytest.mark.parametrize("C,L", [(8, 4), (48, 4), (1024, 1), (512, 9), (16, 257)])
def test_groupnorm_refuses_unsupported_widths(C, L):
    """Widths without a kernel and rows past L * C = 4096 are refused, forward and backward, with a message naming the limit."""
    R = 2
    lib = _lib.load()
    t = {k: torch.zeros(R * L * C, device="cuda") for k in ("x", "y", "dy", "dx")}
    p = {k: torch.ones(C, device="cuda") for k in ("gam", "bet")}
    st = torch.zeros(R * 16, device="cuda")
    want = "L*C <= 4096" if C in (16, 512) else "C in {16,32,64,128,256,512}"
    rc = lib.ramp_op_groupnorm(_lib.ptr(t["x"]), _lib.ptr(p["gam"]), _lib.ptr(p["bet"]), None, None, _lib.ptr(t["y"]), _lib.ptr(st),
                               R, L, C, 1e-5, 1, S())
    assert rc != 0 and want in lib.ramp_last_error().decode()
    rc = lib.ramp_op_groupnorm_bwd(_lib.ptr(t["dy"]), _lib.ptr(t["x"]), _lib.ptr(st), _lib.ptr(p["gam"]), _lib.ptr(p["bet"]), None,
                                   _lib.ptr(t["dx"]), R, L, C, 1, S())
    assert rc != 0 and want in lib.ramp_last_error().decode()
    assert not t["y"].any() and not t["dx"].any()


@pytest.mark.parametrize("n_tok", [1, 5, 4097])
def test_layernorm_fwd_bwd(n_tok):
    g = rng(n_tok)
    x = (g.standard_normal((n_tok, 256)) * 2 + 0.5).astype(np.float32)
    gam = (1 + 0.1 * g.standard_normal(256)).astype(np.float32); bet = (0.1 * g.standard_normal(256)).astype(np.float32)
    dy = g.standard_normal((n_tok, 256)).astype(np.float32); add = g.standard_normal((n_tok, 256)).astype(np.float32)
    y_ref, cache = O.layernorm_fwd(x.astype(np.float64), gam, bet)
    dx_ref = O.layernorm_bwd(dy.astype(np.float64), gam, cache) + add
    y = torch.empty((n_tok, 256), device="cuda"); dx = torch.empty_like(y)
    lib = _lib.load()
    d = {k: dev(v) for k, v in dict(x=x, gam=gam, bet=bet, dy=dy, add=add).items()}
    _lib.check(lib.ramp_op_layernorm(_lib.ptr(d["x"]), _lib.ptr(d["gam"]), _lib.ptr(d["bet"]), _lib.ptr(y), n_tok, S()))
    _lib.check(lib.ramp_op_layernorm_bwd(_lib.ptr(d["dy"]), _lib.ptr(d["x"]), _lib.ptr(d["gam"]), _lib.ptr(d["add"]),
                                         _lib.ptr(dx), n_tok, S()))
    assert rel(y.cpu().numpy(), y_ref) < 2e-6
    assert rel(dx.cpu().numpy(), dx_ref) < 3e-6


def test_geglu_fwd_bwd():
    g = rng(3)
    n_tok, F = 37, 1024
    ag = (g.standard_normal((n_tok, 2 * F)) * 2).astype(np.float32)
    dh = g.standard_normal((n_tok, F)).astype(np.float32)
    a, gg = ag[:, :F].astype(np.float64), ag[:, F:].astype(np.float64)
    hg_ref = a * O.gelu(gg)
    dag_ref = np.concatenate([dh * O.gelu(gg), dh * a * O.gelu_grad(gg)], axis=-1)
    hg = torch.empty((n_tok, F), device="cuda"); dag = torch.empty((n_tok, 2 * F), device="cuda")
    lib = _lib.load(); dag_in = dev(ag); ddh = dev(dh)
    _lib.check(lib.ramp_op_geglu(_lib.ptr(dag_in), _lib.ptr(hg), n_tok, F, S()))
    _lib.check(lib.ramp_op_geglu_bwd(_lib.ptr(ddh), _lib.ptr(dag_in), _lib.ptr(dag), n_tok, F, S()))
    assert rel(hg.cpu().numpy(), hg_ref) < 2e-6
    assert rel(dag.cpu().numpy(), dag_ref) < 2e-6


# the level lengths H, H/2, H/4, H/8 of every horizon ramp_create accepts: all of RAMP_ATTN_LENGTHS (attention.hip; the CPU suite
# checks the two lists agree)
ATTN_LENGTHS = sorted({H >> k for H in range(8, 65, 8) for k in range(4)})


@pytest.mark.parametrize("L", ATTN_LENGTHS)
@pytest.mark.parametrize("R", [1, 7])
def test_attention_fwd_bwd(L, R):
    """4 x 64 softmax attention within each row of L tokens, forward and (dq, dk, dv), at every length a horizon produces."""
    g = rng(L * 10 + R)
    qkv = g.standard_normal((R, L, 768)).astype(np.float32)
    do = g.standard_normal((R, L, 256)).astype(np.float32)
    q, k, v = (qkv[..., i * 256:(i + 1) * 256].astype(np.float64).reshape(R, L, 4, 64).transpose(0, 2, 1, 3) for i in range(3))
    P = O.softmax_last((q @ k.transpose(0, 1, 3, 2)) * 0.125)
    o_ref = (P @ v).transpose(0, 2, 1, 3).reshape(R, L, 256)
    d_o = do.astype(np.float64).reshape(R, L, 4, 64).transpose(0, 2, 1, 3)
    dv = P.transpose(0, 1, 3, 2) @ d_o
    dP = d_o @ v.transpose(0, 1, 3, 2)
    dS = P * (dP - (dP * P).sum(-1, keepdims=True))
    dq = dS @ k * 0.125; dk = dS.transpose(0, 1, 3, 2) @ q * 0.125
    dqkv_ref = np.concatenate([u.transpose(0, 2, 1, 3).reshape(R, L, 256) for u in (dq, dk, dv)], axis=-1)
    o = torch.empty((R, L, 256), device="cuda"); dqkv = torch.empty((R, L, 768), device="cuda")
    lib = _lib.load(); dq_in = dev(qkv); ddo = dev(do)
    _lib.check(lib.ramp_op_attention(_lib.ptr(dq_in), _lib.ptr(o), R, L, S()))
    _lib.check(lib.ramp_op_attention_bwd(_lib.ptr(dq_in), _lib.ptr(ddo), _lib.ptr(dqkv), R, L, S()))
    assert rel(o.cpu().numpy(), o_ref) < 3e-6
    assert rel(dqkv.cpu().numpy(), dqkv_ref) < 5e-6


@pytest.mark.parametrize("name", ["rand", "line", "nohit", "ends", "big"])
def test_apf_against_reference_fixture(name):
    """avoidance() in/out pairs captured from the reference (APFhelper.py:37-104)."""
    from ramp_amd.apf import ObstacleField, avoidance
    g = np.load(f"{GOLDEN}/apf_cases.npz")
    thr, strength, win = g[name + "/params"]
    traj = dev(g[name + "/traj"])
    out = avoidance(traj, ObstacleField(g[name + "/cloud"], distance_threshold=float(thr)),
                    avoidance_window=int(win), avoidance_strength=float(strength)).cpu().numpy()
    assert np.array_equal(traj.cpu().numpy(), g[name + "/traj"])        # input untouched (returns a copy)
    assert np.abs(out - g[name + "/out"]).max() < 5e-7
    assert np.array_equal(out[..., 2:], g[name + "/traj"][..., 2:])
    if name == "nohit":
        assert np.array_equal(out, g[name + "/traj"])


def test_apf_large_cloud_and_oracle():
    """8k-point cloud (streams through LDS in 8 tiles), B=64, H=64, S=6 vs the oracle."""
    from ramp_amd.apf import ObstacleField, avoidance
    from ramp_amd import synth
    g = rng(11)
    cloud = synth.make_cloud(40, 200, 2, seed=5).reshape(-1, 2)
    traj = g.uniform(-1, 1, size=(64, 64, 6)).astype(np.float32)
    ref = O.apf_avoidance(traj.copy(), cloud, 0.07, 0.1, 7)
    out = avoidance(dev(traj), ObstacleField(cloud, 0.07), avoidance_window=7, avoidance_strength=0.1).cpu().numpy()
    assert (ref != traj).sum() > 100
    assert np.abs(out - ref).max() < 5e-7


def test_costs_against_reference_fixture():
    from ramp_amd import cost
    g = np.load(f"{GOLDEN}/cost_cases.npz")
    tr, cl = dev(g["trajs"]), dev(g["cloud"])
    for thr in (0.02, 0.05, 0.1):
        assert np.array_equal(cost.compute_collision_with_pointcloud(tr, cl, thr).cpu().numpy(), g[f"mask_{thr}"])
    assert rel(cost.compute_path_length(tr).cpu().numpy(), g["path_length"]) < 1e-6
    assert rel(cost.compute_smoothness(tr).cpu().numpy(), g["smoothness"]) < 1e-6
    best, best_cost, total, free, idx = cost.compute_trajectory_costs(tr, cl, collision_threshold=0.05)
    assert np.array_equal(free.cpu().numpy(), g["free_mask"]) and int(idx) == int(g["best_index"])
    assert rel(total.cpu().numpy(), g["total_costs"]) < 1e-5
    assert np.array_equal(best.cpu().numpy(), g["best"])


def test_selection_from_gathered_costs_matches_the_unsharded_selection():
    """Multi-GPU planning merges the ranks' candidates through their per-candidate scalars (ramp_select_from_costs, used by
    ramp_amd.dist.select_best_sharded): on the reference fixture's batch the selection from the (mask, length, smoothness)
    arrays -- whole, and cut into two uneven shards re-joined the way the all-gather joins them -- picks the reference's
    winner (cost.py:56-88), like the one-GPU selection does."""
    from ramp_amd import dist as rdist
    g = np.load(f"{GOLDEN}/cost_cases.npz")
    tr, cl = dev(g["trajs"]), dev(g["cloud"]).reshape(-1, 2).contiguous()
    B, H, Sd = tr.shape
    mask = torch.empty(B, dtype=torch.int32, device="cuda"); plen = torch.empty(B, device="cuda"); smooth = torch.empty(B, device="cuda")
    best = torch.empty((H, Sd), device="cuda"); res = torch.zeros(4, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ramp_select_best(_lib.ptr(tr), B, H, Sd, _lib.ptr(cl), cl.shape[0], 0.05, 0.1, 0.9, _lib.ptr(mask),
                                            _lib.ptr(plen), _lib.ptr(smooth), _lib.ptr(best), _lib.ptr(res), S()))
    n_free, rank, row, _ = (int(v) for v in res.cpu())
    assert rank == int(g["best_index"]) and n_free == int(g["free_mask"].sum())
    got, nf, grow = rdist.select_best_sharded(tr, mask, plen, smooth, 0.1, 0.9)          # one rank: the gathered arrays ARE the local ones
    assert nf == n_free and grow == row and torch.equal(got, best)
    cut = B // 3                                                                          # two shards, joined in rank order
    m2 = torch.cat([mask[:cut], mask[cut:]]); p2 = torch.cat([plen[:cut], plen[cut:]]); s2 = torch.cat([smooth[:cut], smooth[cut:]])
    assert rdist._select_hip(m2.contiguous(), p2.contiguous(), s2.contiguous(), 0.1, 0.9) == (n_free, rank, row)
    none, nf0, _ = rdist.select_best_sharded(tr, torch.ones_like(mask), plen, smooth, 0.1, 0.9)
    assert none is None and nf0 == 0


def test_hard_conditioning_and_cfg_mean():
    from ramp_amd.sample_functions import apply_hard_conditioning
    g = rng(5)
    x = g.standard_normal((5, 48, 4)).astype(np.float32)
    start = g.standard_normal(4).astype(np.float32); goal = g.standard_normal((5, 4)).astype(np.float32)
    xd = dev(x)
    apply_hard_conditioning(xd, {0: torch.from_numpy(start), 47: torch.from_numpy(goal), -2: torch.from_numpy(start)})
    want = x.copy(); want[:, 0] = start; want[:, 47] = goal; want[:, 46] = start
    assert np.array_equal(xd.cpu().numpy(), want)
    # CFG combine / x0 / clamp / posterior mean: bitwise vs the same float32 expression order in numpy
    eps = g.standard_normal((10, 48, 4)).astype(np.float32) * 3
    A, Bc, c1, c2, w = np.float32(1.7), np.float32(2.9), np.float32(0.3), np.float32(0.69), 2.0
    e = np.float32(1 + w) * eps[0::2] - np.float32(w) * eps[1::2]
    x0 = np.clip(A * x - Bc * e, -1, 1).astype(np.float32)
    mean = c1 * x0 + c2 * x
    o0 = torch.empty((5, 48, 4), device="cuda"); om = torch.empty_like(o0); oe = torch.empty_like(o0)
    de, dx = dev(eps), dev(x)
    _lib.check(_lib.load().ramp_cfg_mean(_lib.ptr(dx), _lib.ptr(de), 5, 192, 2, w, 0.0, A, Bc, c1, c2, 1, 0,
                                         _lib.ptr(o0), _lib.ptr(om), _lib.ptr(oe), S()))
    assert np.array_equal(oe.cpu().numpy(), e) and np.array_equal(o0.cpu().numpy(), x0)
    assert np.array_equal(om.cpu().numpy(), mean)
    assert (np.abs(x0) == 1).sum() > 10          # the clamp was exercised


def test_metrics_against_reference_fixture_and_oracle():
    """ramp_traj_metrics / ramp_waypoint_variance (through ramp_amd.metrics.Metrics) vs the reference's Metrics
    outputs, and at a batch size where the pairwise pass spans several tiles vs the float64 oracle."""
    from ramp_amd.metrics import Metrics
    g = np.load(f"{GOLDEN}/metrics_cases.npz")
    M = Metrics()
    t = dev(g["traj"])
    ci = M.compute_collision_intensity(t, g["centers"], g["sizes"])
    assert np.array_equal(ci.cpu().numpy(), g["intensity"])
    assert np.abs(M.compute_path_length(t).cpu().numpy() - g["path_length"]).max() < 2e-6
    assert np.abs(M.compute_smoothness(t).cpu().numpy() - g["smoothness"]).max() < 2e-5
    assert abs(float(M.compute_variance_waypoints(t)) - float(g["variance_all"])) < 1e-5 * float(g["variance_all"])
    res = M.trajectory_success_and_metrics(t, ci, threshold=0.01)
    assert res["success"] == int(g["success"]) and res["n_free_trajectories"] == int(g["n_free"])
    assert abs(res["collision_intensity"] - float(g["collision_intensity_pct"])) < 1e-4
    assert abs(res["path_length"] - float(g["free_path_length"])) < 1e-5
    assert abs(res["path_length_std"] - float(g["free_path_length_std"])) < 1e-5
    assert abs(res["waypoint_variance"] - float(g["free_variance"])) < 1e-5 * float(g["free_variance"])
    big = rng(5).standard_normal((700, 48, 4)).astype(np.float32) * 0.4
    assert abs(float(M.compute_variance_waypoints(dev(big))) - O.waypoint_variance(big)) < 2e-6 * O.waypoint_variance(big)
    assert np.abs(M.compute_collision_intensity(dev(big), g["centers"], g["sizes"]).cpu().numpy()
                  - O.collision_intensity(big, g["centers"], g["sizes"])).max() == 0


def test_fp16x3_scaling_and_range_guard():
    """fp16x3 GEMM with the delayed operand scale: a stale maximum 2^7 too large or 2^8 too small changes nothing
    (powers of two are undone exactly; fp16 keeps 2^-24 of the maximum normal), one that would push the scaled
    operand past the fp16 range raises the guard flag instead of returning infinities silently."""
    g = rng(9)
    M, N, K = 512, 256, 256
    A = g.standard_normal((M, K), dtype=np.float32); W = (g.standard_normal((1, N, K), dtype=np.float32) * 0.05).astype(np.float32)
    ref = A.astype(np.float64) @ W[0].astype(np.float64).T
    dA, dW = dev(A), dev(W)
    amax = float(np.abs(A).max())
    for stale in (5.0, 600.0, 0.02):
        out = torch.empty((M, N), device="cuda")
        rec, flag = _lib.op_gemm(dA, dW, None, None, out, M, N, K, 1, 0, 0, 1, mode="fp16x3", a_absmax_prev=stale)
        assert flag == 0 and rec == amax                     # the launch records the true maximum for its successor
        assert rel(out.cpu().numpy(), ref) < 2e-6
    for stale in (0.0001, 200000.0):     # scale 2^19: 4 sigma * 2^19 >> 65504; scale 2^-12: the largest element < 2^-3
        out = torch.empty((M, N), device="cuda")
        _, flag = _lib.op_gemm(dA, dW, None, None, out, M, N, K, 1, 0, 0, 1, mode="fp16x3", a_absmax_prev=stale)
        assert flag != 0


def _dyn_range_operand(kind, M, K, g):
    """Operands with a wide dynamic range inside ONE tensor -- what a per-tensor power-of-two scale handles worst."""
    A = g.standard_normal((M, K)).astype(np.float32)
    if kind == "loguniform":            # magnitudes log-uniform over 2^-12 .. 2^12
        A = (np.sign(A) * np.exp2(g.uniform(-12, 12, size=(M, K)))).astype(np.float32)
    elif kind == "outlier_cols":        # a few channels 2^10 larger than the rest (transformer outlier features)
        A[:, g.choice(K, 4, replace=False)] *= 1024.0
    elif kind == "tiny_rows":           # most rows 2^-14 of the largest
        A[g.random(M) < 0.9] *= 2.0 ** -14
    elif kind == "outlier_elem":        # one huge element
        A[3, 5] = 3.0e4
    return A


@pytest.mark.parametrize("kind", ["gauss", "loguniform", "outlier_cols", "tiny_rows", "outlier_elem"])
@pytest.mark.parametrize("wkind", ["gauss", "tiny_rows"])
def test_fp16x3_dynamic_range_sweep(kind, wkind):
    """The timed default arithmetic (two scaled fp16 planes per operand = 22 significand bits, ONE power-of-two scale per
    tensor) against the exact-fp32 MFMA kernel and float64 on operands whose magnitudes spread over 2^+-12 inside one
    tensor.  Two contracts, both asserted:
      (1) norm-wise (the measure of every parity bar in this repo, max |err| / max |ref|): fp16x3 is within 2x of the
          exact-fp32 kernel's own error -- or the range guard fires;
      (2) element-wise: |err(m,n)| <= 2 x the fp32 kernel's row-wise error + 2^-28 max|A| sum_k |w_nk|
          + 2^-33 max|W| sum_k |a_mk|: elements below 2^-9 of their tensor's maximum keep an ABSOLUTE accuracy of
          2^-30 of that maximum instead of fp32's relative 2^-24 (the price of a per-tensor scale).
    A stale maximum (operand grew 2^11-fold since it was recorded) must raise the guard."""
    g = rng(sum(map(ord, kind + wkind)))
    M, N, K = 640, 256, 512
    A = _dyn_range_operand(kind, M, K, g)
    W = (g.standard_normal((1, N, K)) / np.sqrt(K)).astype(np.float32)
    if wkind == "tiny_rows":
        W[0, g.random(N) < 0.5] *= 2.0 ** -10
    ref = A.astype(np.float64) @ W[0].astype(np.float64).T
    dA, dW = dev(A), dev(W)
    o32 = torch.empty((M, N), device="cuda"); o16 = torch.empty((M, N), device="cuda")
    _lib.op_gemm(dA, dW, None, None, o32, M, N, K, 1, 0, 0, 1, mode="fp32")
    amax = float(np.abs(A).max())
    _, flag = _lib.op_gemm(dA, dW, None, None, o16, M, N, K, 1, 0, 0, 1, mode="fp16x3", a_absmax_prev=amax)
    r32 = o32.cpu().numpy()
    absA, absW = np.abs(A).astype(np.float64), np.abs(W[0]).astype(np.float64)
    rowscale = absA @ absW.T                                    # what fp32 summation noise of an element scales with
    row32 = np.abs(r32 - ref).max(axis=1, keepdims=True)
    if flag:
        # The guard is evaluated per wave on the rows that wave staged: it fires as soon as ONE wave's rows all sit
        # below 2^-8 of the tensor maximum (they would lose bits), not only when the whole tensor moved.  That is the
        # "or the range guard fires" branch of the contract: the product then repeats the job on the bf16x6 kernels,
        # which must meet the element-wise fp32 bar on these operands (within 4x of the fp32 kernel's own row-wise error: max-over-a-row statistics of two ~2^-24 roundings).
        assert kind in ("tiny_rows", "outlier_elem", "outlier_cols", "loguniform"), "the guard must not fire on a Gaussian operand"
        _lib.op_gemm(dA, dW, None, None, o16, M, N, K, 1, 0, 0, 1, mode="bf16x6")
        e = np.abs(o16.cpu().numpy() - ref) / (4.0 * np.maximum(row32, 2.0 ** -24 * rowscale))
        print(f"{kind}/{wkind}: guard fired (site flag {flag}); bf16x6 fallback element-wise err/bound {e.max():.3f}")
        assert e.max() <= 1.0
        return
    r16 = o16.cpu().numpy()
    assert np.isfinite(r16).all()
    n32, n16 = rel(r32, ref), rel(r16, ref)
    assert n16 <= 2.0 * max(n32, 2.0 ** -24), (n16, n32)
    floor = 2.0 ** -28 * amax * absW.sum(axis=1)[None, :] + 2.0 ** -33 * float(absW.max()) * absA.sum(axis=1)[:, None]
    bound = 2.0 * np.maximum(row32, 2.0 ** -24 * rowscale) + floor
    excess = np.abs(r16 - ref) / bound
    print(f"{kind}/{wkind}: norm-wise fp32 {n32:.2e} fp16x3 {n16:.2e}; element-wise worst err/bound {excess.max():.3f}")
    assert excess.max() <= 1.0
    _, flag = _lib.op_gemm(dA, dW, None, None, o16, M, N, K, 1, 0, 0, 1, mode="fp16x3", a_absmax_prev=amax / 2048.0)
    assert flag != 0


# ffx16's tiling by M on a 256-CU device (launch_ffx16): 128, 293, 4173 -> half tiles only (at most CUs / 2 tiles: a wave owns 16 tokens, ffx16h_kernel);
# 20000 -> full tiles only (157); 33000 -> 256 full tiles + the last round's 2 tiles as 4 half tiles, the very last one partly past M
@pytest.mark.parametrize("M", [128, 293, 4173, 20000, 33000])
@pytest.mark.parametrize("entry", ["ramp_op_ffx16", "ramp_op_ffx"])
def test_ffx_fused_feed_forward_against_float64_autograd(M, entry):
    """The token-owning fused feed-forward kernels through the C ABI -- ramp_op_ffx16: the v_mfma_f32_16x16x32_f16 pair the
    product runs (ffx16.hip, round 6); ramp_op_ffx: the 32x32x16 pair (ffx.hip, ramp_launch_plan.mfma16 = 0) -- forward
    z2 = z1 + W2 (a gelu(g)) + b2, [a | g] = W1 LN(z1) + b1 (layers_attention_mini.py:38-45, 147) and its input gradient
    dz1 = dz + J^T dz (LayerNorm backward included), against float64 torch autograd; M not a multiple of the 128-token
    tile; the operand maxima each launch records are the true ones, and scaling from them leaves the result unchanged to
    rounding; a stale maximum (operand 2^12 larger than assumed) raises the range flag."""
    import ctypes as C
    from ramp_amd import _lib
    gen = torch.Generator(device="cpu").manual_seed(M)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    z1, dz = r(M, 256, sc=1.3), r(M, 256, sc=0.7)
    W1, b1, W2, b2 = r(2048, 256, sc=1 / 16), r(2048, sc=0.1), r(256, 1024, sc=1 / 32), r(256, sc=0.1)
    g, b = 1 + r(256, sc=0.1), r(256, sc=0.1)
    zz = z1.double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(zz, (256,), g.double(), b.double(), 1e-5)
    ag = y @ W1.double().T + b1.double()
    hg = ag[:, :1024] * torch.nn.functional.gelu(ag[:, 1024:])
    z2r = zz + hg @ W2.double().T + b2.double()
    (dz1r,) = torch.autograd.grad(z2r, zz, dz.double())
    z2r = z2r.detach()
    true_max = [y.detach().abs().max().item(), hg.detach().abs().max().item(), dz.abs().max().item()]
    z2, dz1 = torch.empty_like(z1), torch.empty_like(z1)
    out, flag = (C.c_float * 4)(), C.c_int32(0)

    def go(prev):
        _lib.check(getattr(_lib.load(), entry)(_lib.ptr(z1), _lib.ptr(dz), _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2), _lib.ptr(b2),
                                               _lib.ptr(g), _lib.ptr(b), M, (C.c_float * 4)(*prev), _lib.ptr(z2), _lib.ptr(dz1), out,
                                               C.byref(flag), None), entry)
        return rel(z2.double().cpu().numpy(), z2r.cpu().numpy()), rel(dz1.double().cpu().numpy(), dz1r.cpu().numpy())

    e = go([0.0, 0.0, 0.0, 0.0])                              # unscaled operands (the first, calibrating use of a call site)
    assert max(e) < 3e-6 and flag.value == 0, (e, flag.value)
    rec = list(out)
    assert all(abs(rec[i] - true_max[i]) <= 1e-6 * true_max[i] for i in range(3)), (rec, true_max)
    e2 = go(rec)                                              # delayed scaling from the recorded maxima
    assert max(e2) < 3e-6 and flag.value == 0, (e2, flag.value)
    go([rec[0] / 4096.0, rec[1], rec[2], rec[3]])             # LN output 2^12 larger than the scale assumes: overflow guard
    assert flag.value == 1, flag.value


@pytest.mark.parametrize("M,N,ln,epi", [(128, 768, True, 0), (293, 256, False, 3), (4173, 768, True, 0), (4173, 256, False, 0),
                                         (4173, 256, False, 1), (70000, 256, False, 3), (1000, 32, False, 1), (1000, 96, False, 1)])
@pytest.mark.parametrize("entry", ["ramp_op_tkl16", "ramp_op_tkl"])
def test_tkl_token_owning_linear_against_float64(M, N, ln, epi, entry):
    """The token-owning K = 256 linear through the C ABI -- ramp_op_tkl16: the v_mfma_f32_16x16x32_f16 kernel the product runs (tkl16.hip,
    round 6); ramp_op_tkl: the 32x32x16 kernel (tkl.hip, ramp_launch_plan.mfma16 = 0) -- LayerNorm(256) folded into the operand (LN1 -> QKV, layers_attention_mini.py:132), bias + residual +
    per-row-variant constant (the attention output projection with the block's cross-attention constant, :133-135), odd
    numbers of 32-feature blocks and M not a multiple of the 128-token tile, against float64; the recorded operand maximum is
    the true one and scaling from it leaves the result unchanged to rounding; a stale maximum raises the range flag."""
    import ctypes as C
    from ramp_amd import _lib
    gen = torch.Generator(device="cpu").manual_seed(M + N)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    L, n_var = 6, 3
    X, W = r(M, 256, sc=1.3) + 0.2, r(N, 256, sc=1 / 16)
    bias = r(N, sc=0.3) if epi else None
    resid = r(M, N) if epi & 1 else None
    rowbias = r(n_var, N, sc=0.5) if epi & 2 else None
    rowvar = (torch.arange((M + L - 1) // L, device="cuda") % n_var).to(torch.int32) if epi & 2 else None
    g, b = (1 + r(256, sc=0.1), r(256, sc=0.1)) if ln else (None, None)
    xd = X.double()
    if ln:
        xd = torch.nn.functional.layer_norm(xd, (256,), g.double(), b.double(), 1e-5)
    ref = xd @ W.double().T
    if bias is not None:
        ref = ref + bias.double()
    if resid is not None:
        ref = ref + resid.double()
    if rowbias is not None:
        ref = ref + rowbias.double()[rowvar.long()[torch.arange(M, device="cuda") // L]]
    xmax = xd.abs().max().item()
    Y = torch.empty(M, N, device="cuda")
    out, flag = C.c_float(0), C.c_int32(0)
    p = lambda t_: _lib.ptr(t_) if t_ is not None else None

    def go(prev):
        Y.fill_(float("nan"))
        _lib.check(getattr(_lib.load(), entry)(p(X), p(W), p(bias), p(resid), p(rowbias), p(rowvar), n_var if epi & 2 else 0, L, p(g), p(b),
                                               M, N, prev, p(Y), C.byref(out), C.byref(flag), None), entry)
        return rel(Y.double().cpu().numpy(), ref.cpu().numpy())

    e = go(0.0)
    assert e < 3e-6 and flag.value == 0, (e, flag.value)
    assert abs(out.value - xmax) <= 1e-6 * xmax, (out.value, xmax)
    e2 = go(out.value)
    assert e2 < 3e-6 and flag.value == 0, (e2, flag.value)
    go(xmax / 4096.0)                                         # operand 2^12 larger than the scale assumes
    assert flag.value == 1, flag.value


@pytest.mark.parametrize("M", [128, 293, 4173])
def test_tklb_dln1_with_layernorm_backward_against_float64_autograd(M):
    """d(ln1) = d(qkv) Wqkv^T with the LayerNorm-1 backward in its epilogue (tkl.hip tklb_kernel through ramp_op_tklb): the
    input gradient of qkv = Wqkv LN1(z) (layers_attention_mini.py:132) plus the gradient that bypasses the block, against
    float64 autograd; M not a multiple of the tile; recorded operand maximum exact, scaling from it leaves the result
    unchanged to rounding, a stale maximum raises the range flag."""
    import ctypes as C
    from ramp_amd import _lib
    gen = torch.Generator(device="cpu").manual_seed(M)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    z, dqkv, add = r(M, 256, sc=1.3) + 0.2, r(M, 768, sc=0.7), r(M, 256)
    Wqkv = r(768, 256, sc=1 / 16)                                  # qkv = LN(z) Wqkv^T
    g, b = 1 + r(256, sc=0.1), r(256, sc=0.1)
    zz = z.double().requires_grad_(True)
    qkv = torch.nn.functional.layer_norm(zz, (256,), g.double(), b.double(), 1e-5) @ Wqkv.double().T
    (dz,) = torch.autograd.grad(qkv, zz, dqkv.double())
    ref = (dz + add.double()).cpu().numpy()
    Wt = Wqkv.T.contiguous()                                       # (256, 768): the operand the kernel takes
    out = torch.empty(M, 256, device="cuda")
    amax, flag = C.c_float(0), C.c_int32(0)

    def go(prev):
        out.fill_(float("nan"))
        _lib.check(_lib.load().ramp_op_tklb(_lib.ptr(dqkv), _lib.ptr(Wt), _lib.ptr(z), _lib.ptr(g), _lib.ptr(add), M, prev, _lib.ptr(out),
                                            C.byref(amax), C.byref(flag), None), "ramp_op_tklb")
        return rel(out.double().cpu().numpy(), ref)

    e = go(0.0)
    assert e < 3e-6 and flag.value == 0, (e, flag.value)
    true_max = dqkv.abs().max().item()
    assert abs(amax.value - true_max) <= 1e-6 * true_max
    e2 = go(amax.value)
    assert e2 < 3e-6 and flag.value == 0, (e2, flag.value)
    go(true_max / 4096.0)
    assert flag.value == 1, flag.value


@pytest.mark.parametrize("L,R", [(48, 4), (48, 9), (24, 7), (12, 33), (6, 131), (16, 5), (32, 3), (8, 40), (4, 9), (3, 50), (1, 100), (48, 1024)])
def test_atb_attention_backward_against_float64_autograd(L, R):
    """d(q, k, v) of softmax(q k^T / 8) v on sample-owning waves (atk.hip atb_kernel through ramp_op_atb: 16 x 16 fp16x3 MFMAs, operands turned
    in registers by selection MFMAs, no LDS) against float64 autograd (CrossAttention.forward, layers_attention_mini.py:101-127): every level
    length dividing 48 or 32, sample counts that leave the last wave / block partly empty."""
    from ramp_amd import _lib
    M = R * L
    gen = torch.Generator(device="cpu").manual_seed(77 * L + R)
    qkv = (torch.randn(M, 768, generator=gen) * 1.3).cuda()
    qkv[:, 512:] = qkv[:, 512:] * 0.4 + 0.1
    dout = torch.randn(M, 256, generator=gen).cuda()
    x = qkv.double().clone().requires_grad_(True)
    y = x.reshape(R, L, 3, 4, 64)
    q, k, v = y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2), y[:, :, 2].transpose(1, 2)
    o = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(M, 256)
    (ref,) = torch.autograd.grad(o, x, dout.double())
    got = torch.full((M, 768), float("nan"), device="cuda")
    _lib.check(_lib.load().ramp_op_atb(_lib.ptr(qkv), _lib.ptr(dout), _lib.ptr(got), M, L, None), "ramp_op_atb")
    ref = ref.cpu().numpy(); got = got.cpu().numpy()
    for name, sl in (("dq", slice(0, 256)), ("dk", slice(256, 512)), ("dv", slice(512, 768))):
        e = rel(got[:, sl], ref[:, sl])
        assert e < 3e-6, (name, e)


@pytest.mark.parametrize("L,R", [(48, 4), (48, 9), (24, 7), (12, 33), (6, 131), (16, 5), (32, 3), (8, 40), (4, 9), (3, 50), (1, 100), (48, 1024)])
def test_abl_attention_backward_with_ln1_backward_against_float64_autograd(L, R):
    """The backward of `attn1(norm1(x)) + x` from d(o) to the block input in ONE launch (atl.hip abl_kernel through ramp_op_abl: attention
    backward on sample-owning waves, its gradient tiles projected through Wqkv^T into resident accumulators, LayerNorm backward in the
    epilogue; d(qkv) never reaches memory) against float64 autograd of LayerNorm -> QKV -> softmax attention (layers_attention_mini.py:
    101-127, 132): every level length dividing 48 or 32, sample counts that leave the last wave / block partly empty; the recorded operand
    maximum is max |d(qkv)|, scaling from it leaves the result unchanged to rounding, a stale maximum raises the range flag."""
    import ctypes as C
    from ramp_amd import _lib
    M = R * L
    gen = torch.Generator(device="cpu").manual_seed(91 * L + R)
    z = (torch.randn(M, 256, generator=gen) * 1.5 + 0.3)
    ln_g = 1.0 + 0.2 * torch.randn(256, generator=gen)
    ln_b = 0.1 * torch.randn(256, generator=gen)
    Wqkv = torch.randn(768, 256, generator=gen) / 16.0            # forward weight (768, 256); the kernel takes its transpose (256, 768)
    dout = torch.randn(M, 256, generator=gen)
    add = torch.randn(M, 256, generator=gen)
    zd = z.double().clone().requires_grad_(True)
    ln = torch.nn.functional.layer_norm(zd, (256,), ln_g.double(), ln_b.double(), 1e-5)
    qkv64 = ln @ Wqkv.double().t()
    qkv64.retain_grad()
    y = qkv64.reshape(R, L, 3, 4, 64)
    q, k, v = y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2), y[:, :, 2].transpose(1, 2)
    o = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(M, 256)
    o.backward(dout.double())
    ref = (zd.grad + add.double()).numpy()
    true_max = float(qkv64.grad.abs().max())
    qkv = qkv64.detach().float().cuda()
    Wb = Wqkv.t().contiguous().cuda()
    dout_d, z_d, g_d, add_d = dout.cuda(), z.cuda(), ln_g.cuda(), add.cuda()
    lib = _lib.load()

    def run(prev):
        got = torch.full((M, 256), float("nan"), device="cuda")
        amax, flag = C.c_float(0), C.c_int32(0)
        _lib.check(lib.ramp_op_abl(_lib.ptr(qkv), _lib.ptr(dout_d), _lib.ptr(Wb), _lib.ptr(z_d), _lib.ptr(g_d), _lib.ptr(add_d),
                                   M, L, prev, _lib.ptr(got), C.byref(amax), C.byref(flag), None), "ramp_op_abl")
        return got.cpu().numpy(), amax.value, flag.value

    got0, amax0, flag0 = run(0.0)
    assert flag0 == 0 or true_max < 0.125 or true_max >= 60000, flag0
    assert abs(amax0 - true_max) <= 2e-5 * true_max, (amax0, true_max)
    got1, amax1, flag1 = run(amax0)
    assert flag1 == 0
    for got in (got0, got1):
        e = rel(got, ref)
        assert e < 4e-6, e
    _, _, flag2 = run(amax0 / 4096.0)                             # a stale maximum: the operand leaves the fp16 planes' range
    assert flag2 == 1


def test_abl_per_sample_accuracy_under_a_magnitude_spread():
    """The documented trade-off of one power-of-two scale per operand TENSOR, measured per sample: the sample-owning kernels
    judge "operand shrank" on the block's maximum, so a trajectory whose gradients are 2^10 below its batch neighbours' raises no flag; its
    d(qkv) tiles then sit 2^10 below the scale's target and keep 11 + 1 significand bits instead of 22 -- an ABSOLUTE accuracy of 2^-30 of the
    tensor's maximum, i.e. ~2^-20 relative to that sample's own.  ramp_op_abl, L = 48, 8 samples, sample 5's d(o) scaled by 2^-10: every
    sample's error relative to ITS OWN largest gradient, the quiet sample's next to the others'."""
    import ctypes as C
    from ramp_amd import _lib
    L, R = 48, 8
    M = R * L
    gen = torch.Generator(device="cpu").manual_seed(4711)
    z = (torch.randn(M, 256, generator=gen) * 1.5 + 0.3)
    ln_g = 1.0 + 0.2 * torch.randn(256, generator=gen)
    ln_b = 0.1 * torch.randn(256, generator=gen)
    Wqkv = torch.randn(768, 256, generator=gen) / 16.0
    dout = torch.randn(M, 256, generator=gen)
    dout[5 * L:6 * L] *= 2.0 ** -10
    zd = z.double().clone().requires_grad_(True)
    ln = torch.nn.functional.layer_norm(zd, (256,), ln_g.double(), ln_b.double(), 1e-5)
    qkv64 = ln @ Wqkv.double().t()
    y = qkv64.reshape(R, L, 3, 4, 64)
    q, k, v = y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2), y[:, :, 2].transpose(1, 2)
    o = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(M, 256)
    o.backward(dout.double())
    ref = zd.grad.numpy().reshape(R, L * 256)
    got = torch.full((M, 256), float("nan"), device="cuda")
    amax, flag = C.c_float(0), C.c_int32(0)
    add = torch.zeros(M, 256, device="cuda")
    lib = _lib.load()
    keep = (qkv64.detach().float().cuda(), dout.cuda(), Wqkv.t().contiguous().cuda(), z.cuda(), ln_g.cuda(), add)      # (alive across the launches)
    args = tuple(_lib.ptr(t_) for t_ in keep)
    _lib.check(lib.ramp_op_abl(*args, M, L, 0.0, _lib.ptr(got), C.byref(amax), C.byref(flag), None), "ramp_op_abl")
    _lib.check(lib.ramp_op_abl(*args, M, L, amax.value, _lib.ptr(got), C.byref(amax), C.byref(flag), None), "ramp_op_abl")      # scaled from the tensor maximum
    assert flag.value == 0                                         # no guard trip: the block's maximum is in range
    out = got.cpu().numpy().astype(np.float64).reshape(R, L * 256)
    per = np.abs(out - ref).max(1) / np.abs(ref).max(1)
    print("abl, per-sample error relative to the sample's own largest gradient: " + " ".join(f"{e:.1e}" for e in per) + "  (sample 5: d(o) x 2^-10)")
    others = np.delete(per, 5)
    assert others.max() < 4e-6                                     # fp32 rounding, as everywhere
    assert per[5] < 2.0 ** -17, per[5]                             # 2^-30 of the tensor maximum = 2^-20 of its own, with head room for the accumulation


@pytest.mark.parametrize("L,R,N,K,extras", [(48, 3, 32, 32, True), (48, 9, 64, 64, True), (24, 7, 64, 32, False), (24, 8, 32, 64, True), (12, 33, 64, 64, True),
                                            (16, 5, 64, 64, False), (32, 3, 32, 32, True), (8, 41, 64, 64, True), (48, 4096, 32, 32, True),
                                            # round 6: L = 64 (the finest level of the H = 64 configurations): a wave owns ONE sample (tkc_kernel<NG = 4>)
                                            (64, 5, 32, 32, True), (64, 3, 32, 64, True), (64, 9, 64, 32, False), (64, 2048, 32, 32, True)])
@pytest.mark.parametrize("backward", [False, True])
def test_tkc_narrow_convolution_against_float64(L, R, N, K, extras, backward):
    """The k = 5 convolutions with C_in, C_out in {32, 64} on sample-owning waves (tkc.hip, ramp_op_gemm_mode 5): Conv1d(padding 2) inside
    every sample of L tokens (layers.py:280-297) and its input gradient (taps reversed), with bias + residual, against float64; sample counts
    that leave the last wave / block partly empty; the recorded operand maximum is the true one, scaling from it leaves the result unchanged
    to rounding, a stale maximum raises the range flag."""
    M = L * R
    g = rng(L * 1000 + R + N + K + backward)
    A = (g.standard_normal((M, K), dtype=np.float32) * 1.7 + 0.1).astype(np.float32)
    W = (g.standard_normal((5, N, K), dtype=np.float32) / np.sqrt(5 * K)).astype(np.float32)
    bias = g.standard_normal(N, dtype=np.float32) if extras else None
    resid = g.standard_normal((M, N), dtype=np.float32) if extras else None
    shift0, step = (2, -1) if backward else (-2, 1)
    ref = np.zeros((M, N))
    A3 = A.reshape(R, L, K).astype(np.float64)
    for j in range(5):
        sh = shift0 + j * step
        Ash = np.zeros_like(A3)
        if sh >= 0:
            Ash[:, :L - sh] = A3[:, sh:]
        else:
            Ash[:, -sh:] = A3[:, :L + sh]
        ref += Ash.reshape(M, K) @ W[j].astype(np.float64).T
    if extras:
        ref += bias + resid
    out = torch.full((M, N), float("nan"), device="cuda")
    dA, dW = dev(A), dev(W)
    db, dr = (dev(bias), dev(resid)) if extras else (None, None)
    amax, flag = _lib.op_gemm(dA, dW, db, dr, out, M, N, K, 5, shift0, step, L, mode="fp16x3-tkc")
    e = rel(out.cpu().numpy(), ref)
    assert e < 3e-6 and flag == 0, (e, flag)
    true_max = float(np.abs(A).max())
    assert abs(amax - true_max) <= 1e-6 * true_max
    out.fill_(float("nan"))
    _, flag = _lib.op_gemm(dA, dW, db, dr, out, M, N, K, 5, shift0, step, L, mode="fp16x3-tkc", a_absmax_prev=amax)
    assert rel(out.cpu().numpy(), ref) < 3e-6 and flag == 0
    _, flag = _lib.op_gemm(dA, dW, db, dr, out, M, N, K, 5, shift0, step, L, mode="fp16x3-tkc", a_absmax_prev=true_max / 4096.0)
    assert flag == 1


def _attention_block_float64(qkv, Wo, bias, resid, rowbias, rowvar, L):
    """resid + to_out(softmax(q k^T / 8) v) + bias + per-row-variant constant in float64 (layers_attention_mini.py:101-127, 132)."""
    M = qkv.shape[0]
    x = qkv.double().reshape(M // L, L, 3, 4, 64)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)      # (R, 4, L, 64)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    o = (p @ v).transpose(1, 2).reshape(M, 256)
    y = resid.double() + o @ Wo.double().T
    if bias is not None:
        y = y + bias.double()
    if rowbias is not None:
        y = y + rowbias.double()[rowvar.long()[torch.arange(M, device=qkv.device) // L]]
    return y, o


@pytest.mark.parametrize("L,R,rb", [(48, 4, True), (48, 9, False), (24, 7, True), (12, 33, True), (6, 131, True), (6, 64, False),
                                    (16, 5, True), (32, 3, True), (8, 40, False), (4, 9, True), (3, 50, True), (2, 7, False), (1, 100, True)])
def test_ato_attention_with_output_projection_against_float64(L, R, rb):
    """Self-attention fused with its output projection (atk.hip through ramp_op_ato: sample-owning waves, every product on the
    16 x 16 fp16 MFMAs in the fp16x3 split) against float64: every level length that divides 48 or 32, sample counts that leave
    the last wave / block partly or wholly empty, with and without the per-row-variant constant; the recorded operand maximum
    is the attention output's true one, scaling from it leaves the result unchanged to rounding, a stale maximum raises the
    range flag."""
    import ctypes as C
    from ramp_amd import _lib
    M = R * L
    gen = torch.Generator(device="cpu").manual_seed(1000 * L + R)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=gen) * sc).cuda()
    qkv = r(M, 768, sc=1.5)
    qkv[:, 512:] = qkv[:, 512:] * 0.3 + 0.1
    Wo, bias, resid = r(256, 256, sc=1 / 16), r(256, sc=0.3), r(M, 256)
    n_var = 3
    rowbias = r(n_var, 256, sc=0.5) if rb else None
    rowvar = (torch.arange(R, device="cuda") % n_var).to(torch.int32) if rb else None
    ref, o = _attention_block_float64(qkv, Wo, bias, resid, rowbias, rowvar, L)
    ref = ref.cpu().numpy(); omax = o.abs().max().item()
    Y = torch.empty(M, 256, device="cuda")
    out, flag = C.c_float(0), C.c_int32(0)
    p = lambda t_: _lib.ptr(t_) if t_ is not None else None

    def go(prev):
        Y.fill_(float("nan"))
        _lib.check(_lib.load().ramp_op_ato(p(qkv), p(Wo), p(bias), p(resid), p(rowbias), p(rowvar), n_var if rb else 0, L, M, prev, p(Y), C.byref(out),
                                           C.byref(flag), None), "ramp_op_ato")
        return rel(Y.double().cpu().numpy(), ref)

    e = go(0.0)
    print(f"ato L={L} R={R}: {e:.2e}")
    assert e < 3e-6 and flag.value == 0, (e, flag.value)
    assert abs(out.value - omax) <= 2e-6 * omax, (out.value, omax)
    e2 = go(out.value)
    assert e2 < 3e-6 and flag.value == 0, (e2, flag.value)
    go(omax / 4096.0)
    assert flag.value == 1, flag.value


STRESS_CASES = [   # name, M, N, K, taps, L, mode (ramp_bench_gemm), flags, compare with the exact-fp32 kernel?
    ("fp16x3 bias-only 768x256 (QKV; third resident block)", 393216, 768, 256, 1, 1, 3, 1, True),
    ("fp16x3 residual 256x256 (out-proj, 64x256 tile)", 393216, 256, 256, 1, 1, 3, 3, True),
    ("fp16x3 1024x256 (d(hg))", 393216, 1024, 256, 1, 1, 3, 1, True),
    ("fp16x3 256x768 (d(ln1))", 393216, 256, 768, 1, 1, 3, 1, True),
    ("fp16x3 A-multiplier 256x2048 (FF1 dX)", 393216, 256, 2048, 1, 1, 3, 8, False),   # (no exact-fp32 twin of the fused operand)
    ("fp16x3 GEGLU-forward epilogue 2048x256", 393216, 2048, 256, 1, 1, 3, 1 | 4, False),
    ("fp16x3 5-tap convolution 64x64, L=48", 393216, 64, 64, 5, 48, 3, 1, True),
    ("fp16x3 5-tap convolution 128x128, L=24", 196608, 128, 128, 5, 24, 3, 1, True),
    ("bf16x6 residual 256x256", 393216, 256, 256, 1, 1, 1, 3, True),
    ("fused FF1->GEGLU->FF2 forward (ff_fwd_kernel)", 393216, 2048, 256, 1, 1, 5, 0, False),
    ("token-owning fused feed-forward, forward (ffx)", 393216, 2048, 256, 1, 1, 6, 0, False),
    ("token-owning fused feed-forward, backward (ffx)", 393216, 2048, 256, 1, 1, 7, 0, False),
    ("token-owning fused feed-forward on 16x16x32 MFMAs, forward (ffx16)", 393216, 2048, 256, 1, 1, 6, 1 << 16, False),
    ("token-owning fused feed-forward on 16x16x32 MFMAs, backward (ffx16)", 393216, 2048, 256, 1, 1, 7, 1 << 16, False),
    ("token-owning fused feed-forward, HALF tiles only, forward (ffx16h)", 393216, 2048, 256, 1, 1, 6, (1 << 16) | (2 << 17), False),
    ("token-owning fused feed-forward, HALF tiles only, backward (ffx16h)", 393216, 2048, 256, 1, 1, 7, (1 << 16) | (2 << 17), False),
    ("token-owning fused feed-forward, 256 full + 256 half tiles, forward (ffx16 + ffx16h)", 49152, 2048, 256, 1, 1, 6, 1 << 16, False),
    ("token-owning fused feed-forward, 256 full + 256 half tiles, backward (ffx16 + ffx16h)", 49152, 2048, 256, 1, 1, 7, 1 << 16, False),
    ("token-owning LN1 -> QKV (tkl)", 393216, 768, 256, 1, 1, 8, 1, False),
    ("token-owning LN1 -> QKV on 16x16x32 MFMAs (tkl16)", 393216, 768, 256, 1, 1, 8, 1 | (1 << 16), False),
    ("token-owning d(o) on 16x16x32 MFMAs (tkl16)", 393216, 256, 256, 1, 1, 8, 1 << 16, False),
    ("token-owning out-projection with bias and residual (tkl)", 393216, 256, 256, 1, 1, 8, 2, False),
    ("token-owning d(ln1) with LayerNorm-1 backward (tklb)", 393216, 256, 768, 1, 1, 9, 0, False),
    ("self-attention fused with the out-projection, L = 48 (atk)", 393216, 256, 256, 1, 48, 10, 1, False),
    ("self-attention fused with the out-projection, L = 6 (atk)", 49152, 256, 256, 1, 6, 10, 1, False),
    ("sample-owning 5-tap convolution 64x64 with bias and residual, L = 24 (tkc)", 196608, 64, 64, 5, 24, 12, 3, False),
    ("sample-owning 5-tap convolution 32x32 input gradient, L = 48 (tkc)", 393216, 32, 32, 5, 48, 12, 4, False),
    ("sample-owning 5-tap convolution 64x64 with GroupNorm + Mish and residual, L = 24 (tkc)", 196608, 64, 64, 5, 24, 12, 2 | 8, False),
    ("sample-owning 5-tap convolution 32x32 input gradient with GroupNorm backward, L = 48 (tkc)", 393216, 32, 32, 5, 48, 12, 4 | 16 | 2, False),
    ("sample-owning 5-tap convolution 32x32 with GroupNorm + Mish and residual, L = 64 (tkc)", 524288, 32, 32, 5, 64, 12, 2 | 8, False),
    ("sample-owning 5-tap convolution 64->32 input gradient with GroupNorm backward, L = 64 (tkc)", 524288, 64, 32, 5, 64, 12, 4 | 16 | 2, False),
    ("attention backward on sample-owning waves, L = 24 (atb)", 196608, 256, 256, 1, 24, 13, 0, False),
    ("attention backward + d(ln1) + LayerNorm-1 backward in one launch, L = 48 (abl)", 393216, 256, 768, 1, 48, 15, 0, False),
    ("attention backward + d(ln1) + LayerNorm-1 backward in one launch, L = 12 (abl)", 98304, 256, 768, 1, 12, 15, 0, False),
    ("attention backward + d(ln1) + LayerNorm-1 backward, k fetched twice (round-4 twin), L = 48 (abl)", 393216, 256, 768, 1, 48, 15, 1 << 16, False),
    ("wide 5-tap convolution 256x256 + GroupNorm + Mish + residual, L = 6 (tkw)", 49152, 256, 256, 5, 6, 17, 1 | 8, False),
    ("wide 5-tap convolution 128x128 input gradient with GroupNorm backward, L = 12 (tkw)", 98304, 128, 128, 5, 12, 17, 2 | 4 | 8, False),
    ("wide 5-tap convolution 256x256 input gradient with GroupNorm backward, L = 6 (tkw)", 49152, 256, 256, 5, 6, 17, 2 | 4, False),
]


@pytest.mark.parametrize("name,M,N,K,taps,L,mode,flags,vs_fp32", STRESS_CASES, ids=[c[0].split(" (")[0].replace(" ", "-") for c in STRESS_CASES])
def test_gemm_variants_are_bitwise_stable_under_stress(name, M, N, K, taps, L, mode, flags, vs_fp32):
    """Every shipped GEMM variant at full size, 300 back-to-back launches on the same operands: each launch's output is
    compared BIT FOR BIT with the first one's on the device (hand-pipelined loaders with register stages across tile
    boundaries, LDS rings filled by DMA, wave-private epilogues: a latent ordering hazard shows up as a sporadic stale
    operand row, i.e. a handful of differing words in one launch out of many), and the first output sits within fp32
    rounding of the exact-fp32 MFMA kernel's on the same operands."""
    import ctypes as C
    mism, err = C.c_int64(-1), C.c_float(-2.0)
    _lib.check_tools(_lib.load_tools().ramp_stress_gemm(M, N, K, taps, L, mode, flags, 300, C.byref(mism), C.byref(err) if vs_fp32 else None, None),
               "ramp_stress_gemm")
    print(f"{name}: 300 launches, {mism.value} differing words" + (f", first launch vs exact fp32: {err.value:.2e}" if vs_fp32 else ""))
    assert mism.value == 0, name
    if vs_fp32:
        assert 0.0 <= err.value < 5e-6, (name, err.value)


SOAK_CASES = [   # name, M, N, K, taps, L, mode (ramp_bench_gemm), flags
    ("abl L=48", 393216, 256, 768, 1, 48, 15, 0), ("abl L=6", 49152, 256, 768, 1, 6, 15, 0), ("ato L=48", 393216, 256, 256, 1, 48, 10, 1),
    ("atb L=24", 196608, 256, 256, 1, 24, 13, 0), ("ffx forward", 393216, 2048, 256, 1, 1, 6, 0), ("ffx backward", 393216, 2048, 256, 1, 1, 7, 0),
    ("tkl LN1->QKV", 393216, 768, 256, 1, 1, 8, 1), ("tklb", 196608, 256, 768, 1, 1, 9, 0),
    ("ffx16 forward", 393216, 2048, 256, 1, 1, 6, 1 << 16), ("ffx16 backward", 393216, 2048, 256, 1, 1, 7, 1 << 16),
    ("tkl16 LN1->QKV", 393216, 768, 256, 1, 1, 8, 1 | (1 << 16)),
    ("ffx16h forward", 196608, 2048, 256, 1, 1, 6, (1 << 16) | (2 << 17)), ("ffx16h backward", 196608, 2048, 256, 1, 1, 7, (1 << 16) | (2 << 17)),
]


@pytest.mark.parametrize("name,M,N,K,taps,L,mode,flags", SOAK_CASES, ids=[c[0].replace(" ", "-") for c in SOAK_CASES])
def test_soak_2000_launches_bitwise(name, M, N, K, taps, L, mode, flags):
    """The kernels whose correctness rests on inline-asm LDS-DMA rings with hand-counted ``s_waitcnt vmcnt(N)`` (ffx, tkl / tklb,
    ato / atb, abl): 2000 back-to-back launches per kernel on the same operands, every output compared bit for bit with the first
    launch's on the device (ramp_stress_gemm).  ramp_amd/tools/soak.py as a test, so that the schedules are exercised on every box
    the suite runs on, not only the builder's (engineering 12)."""
    import ctypes as C
    mism = C.c_int64(-1)
    _lib.check_tools(_lib.load_tools().ramp_stress_gemm(M, N, K, taps, L, mode, flags, 2000, C.byref(mism), None, None), "ramp_stress_gemm")
    print(f"{name}: 2000 launches, {mism.value} differing words")
    assert mism.value == 0, name


def _conv5_f64(A, W, L, direction):
    """sum_tap shift(A, direction * (tap - 2)) W[tap]^T with zero padding per sample of L tokens; A (M, K), W (5, N, K) float64."""
    M, K = A.shape
    A3 = A.reshape(M // L, L, K)
    out = np.zeros((M, W.shape[1]))
    for j in range(5):
        sh = direction * (j - 2)
        Ash = np.zeros_like(A3)
        if sh >= 0:
            Ash[:, :L - sh] = A3[:, sh:]
        else:
            Ash[:, -sh:] = A3[:, :L + sh]
        out += Ash.reshape(M, K) @ W[j].T
    return out


def _mish64(x):
    return x * np.tanh(np.logaddexp(0.0, x))


def _mish_grad64(x):
    sp = np.logaddexp(0.0, x); th = np.tanh(sp)
    return th + x * (1.0 / (1.0 + np.exp(-x))) * (1.0 - th * th)


TKW_FWD = [   # L, K, N, samples, K1 (operand split) -- Conv1dBlock of the coarse levels: conv k5 -> GroupNorm(8) -> Mish (+ time bias / residual)
    (6, 256, 256, 37, 0), (12, 128, 128, 19, 0), (6, 128, 256, 16, 0), (12, 64, 128, 8, 0), (6, 512, 128, 21, 256), (8, 256, 256, 13, 0),
    (16, 128, 128, 7, 0), (3, 256, 256, 33, 0), (24, 64, 128, 5, 0), (48, 32, 128, 3, 0), (6, 256, 128, 16, 128),
    # the narrow levels: the same fusion on sample-owning waves (tkc.hip), wave tiles of 48 and of 32 tokens, partly empty last tiles
    (48, 32, 32, 7, 0), (24, 32, 64, 9, 0), (24, 64, 64, 11, 0), (48, 64, 32, 3, 0), (16, 32, 32, 5, 0), (8, 64, 64, 13, 0), (12, 64, 64, 9, 0),
    (32, 32, 64, 3, 0), (48, 64, 64, 300, 0),
    # round 6: L = 64, one sample per wave
    (64, 32, 32, 5, 0), (64, 64, 32, 3, 0), (64, 32, 32, 700, 0),
]


@pytest.mark.parametrize("L,K,N,R,K1", TKW_FWD)
@pytest.mark.parametrize("extras", [0, 1, 2])
def test_tkw_conv_groupnorm_mish_forward(L, K, N, R, K1, extras):
    """tkw.hip, forward: C = conv5(X) + bias (the stash), its GroupNorm(8) statistics, Y = mish(GN(C) gamma + beta) [+ time bias]
    [+ residual] in ONE launch of sample-owning blocks, against float64 (layers.py:280-297, 327-361): every coarse-level shape, the
    concatenated two-source operand of the up blocks, sample counts that leave the last tile partly empty; operand scaled from a
    recorded maximum, the recorded maximum exact; extras 0: GroupNorm + Mish only, 1: + time bias (first Conv1dBlock), 2: + residual
    (second)."""
    g = rng(L * 1000 + K + N + extras)
    M = L * R
    X = (g.standard_normal((M, K)) * 1.3).astype(np.float32)
    W = (g.standard_normal((5, N, K)) / np.sqrt(5 * K)).astype(np.float32)
    bias = g.standard_normal(N).astype(np.float32) * 0.3
    gam = (1 + 0.2 * g.standard_normal(N)).astype(np.float32); bet = (0.2 * g.standard_normal(N)).astype(np.float32)
    tb = g.standard_normal(N).astype(np.float32) if extras == 1 else None
    res = g.standard_normal((M, N)).astype(np.float32) if extras == 2 else None
    c = _conv5_f64(X.astype(np.float64), W.astype(np.float64), L, 1) + bias
    cg = c.reshape(R, L, 8, N // 8)
    mean = cg.mean(axis=(1, 3)); var = cg.var(axis=(1, 3)); rstd = 1.0 / np.sqrt(var + 1e-5)
    nrm = ((cg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(M, N) * gam + bet
    y = _mish64(nrm) + (tb if tb is not None else 0.0) + (res if res is not None else 0.0)
    if K1:
        xa, xb = dev(np.ascontiguousarray(X[:, :K1])), dev(np.ascontiguousarray(X[:, K1:]))
    else:
        xa, xb = dev(X), None
    Y = torch.full((M, N), float("nan"), device="cuda"); Cs = torch.full((M, N), float("nan"), device="cuda")
    st = torch.full((R, 8, 2), float("nan"), device="cuda")
    amax, flag = C.c_float(0.0), C.c_int32(0)
    prev = float(np.abs(X).max()) * 0.8
    dW, db, dg, dbt = dev(W), dev(bias), dev(gam), dev(bet)          # (kept alive: a temporary's memory is recycled by the next allocation)
    dres = dev(res) if res is not None else None; dtb = dev(tb) if tb is not None else None
    _lib.check(_lib.load().ramp_op_tkw(_lib.ptr(xa), _lib.ptr(xb), K1, _lib.ptr(dW), _lib.ptr(db), _lib.ptr(dres), None, None, None, None, None,
                                       _lib.ptr(dg), _lib.ptr(dbt), _lib.ptr(dtb), M, L, N, K, 1, N, prev, _lib.ptr(Y), None, _lib.ptr(Cs), _lib.ptr(st),
                                       C.byref(amax), C.byref(flag), S()), "ramp_op_tkw")
    assert flag.value == 0 and amax.value == float(np.abs(X).max())
    ec, ey = rel(Cs.cpu().numpy(), c), rel(Y.cpu().numpy(), y)
    es = max(rel(st[:, :, 0].cpu().numpy(), mean), rel(st[:, :, 1].cpu().numpy(), rstd))
    print(f"tkw fwd L={L} {K}->{N} rows={R} extras={extras}: stash {ec:.2e} stats {es:.2e} y {ey:.2e}")
    assert ec < 3e-6 and es < 3e-6 and ey < 5e-6


def test_tkw_refuses_operand_widths_that_are_not_powers_of_two():
    """the kernel's tap / chunk indexing shifts and masks by K / 32 and KC / 32, so K = 96 (a multiple of 32 that used to pass
    the geometry check) indexed taps up to 7 and read past the weight planes; K = 384 broke the GroupNorm-backward group reduction.  The
    network never has such widths (channels are 32 x 2^k); through ramp_op_tkw they must be an error return, not a silent wrong result."""
    for K, N in ((96, 128), (384, 256), (160, 128)):
        M, L = 96, 6
        X = torch.randn(M, K, device="cuda"); W = torch.randn(5, N, K, device="cuda"); Y = torch.empty(M, N, device="cuda")
        Cs = torch.empty(M, N, device="cuda"); st = torch.empty(M // L, 8, 2, device="cuda")
        b = torch.zeros(N, device="cuda"); gam = torch.ones(N, device="cuda")
        amax, flag = C.c_float(0.0), C.c_int32(0)
        rc = _lib.load().ramp_op_tkw(_lib.ptr(X), None, 0, _lib.ptr(W), _lib.ptr(b), None, None, None, None, None, None,
                                     _lib.ptr(gam), _lib.ptr(b), None, M, L, N, K, 1, N, 1.0, _lib.ptr(Y), None, _lib.ptr(Cs), _lib.ptr(st),
                                     C.byref(amax), C.byref(flag), S())
        assert rc != 0, (K, N)
        assert "tkw" in _lib.load().ramp_last_error().decode()


TKW_BWD = [   # L, K (= C_out of the forward layer), N (= C_in), samples, N1 (output split)
    (6, 256, 256, 37, 0), (12, 128, 128, 19, 0), (6, 256, 128, 16, 0), (6, 128, 512, 21, 256), (12, 64, 256, 9, 128), (8, 256, 256, 13, 0),
    (16, 128, 128, 7, 0), (4, 256, 256, 33, 0), (24, 64, 128, 5, 0), (12, 256, 256, 9, 0), (48, 32, 128, 3, 0),
    # the narrow levels (tkc.hip)
    (48, 32, 32, 7, 0), (24, 64, 32, 9, 0), (24, 64, 64, 11, 0), (48, 32, 64, 3, 0), (16, 32, 32, 5, 0), (8, 64, 64, 13, 0), (12, 64, 64, 9, 0),
    (32, 64, 32, 3, 0), (48, 64, 64, 300, 0),
    # round 6: L = 64, one sample per wave
    (64, 32, 32, 5, 0), (64, 32, 64, 3, 0), (64, 32, 32, 700, 0),
]


@pytest.mark.parametrize("L,K,N,R,N1", TKW_BWD)
@pytest.mark.parametrize("extras", [0, 3])
def test_tkw_groupnorm_backward_conv_input_gradient(L, K, N, R, N1, extras):
    """tkw.hip, input gradient: Y = conv5^T( GNbwd( dY (.) mish'(gamma x^ + beta) gamma ; x^ ) ) [+ resid + resid2] in ONE launch -- the
    GroupNorm + Mish backward is the operand staging of the convolution -- against float64, incl. the split output of the up blocks'
    first convolution (the skip gradient) and the recorded maximum of the operand the kernel never materialises."""
    g = rng(L * 1000 + K + N + extras + 7)
    M = L * R
    dy = g.standard_normal((M, K)).astype(np.float32)
    cst = (g.standard_normal((M, K)) * 1.5 + 0.3).astype(np.float32)
    gam = (1 + 0.2 * g.standard_normal(K)).astype(np.float32); bet = (0.2 * g.standard_normal(K)).astype(np.float32)
    W = (g.standard_normal((5, N, K)) / np.sqrt(5 * K)).astype(np.float32)
    r1 = g.standard_normal((M, N)).astype(np.float32) if extras & 1 else None
    r2 = g.standard_normal((M, N)).astype(np.float32) if (extras & 2 and not N1) else None
    cg = cst.astype(np.float64).reshape(R, L, 8, K // 8)
    mean = cg.mean(axis=(1, 3)); rstd = 1.0 / np.sqrt(cg.var(axis=(1, 3)) + 1e-5)
    stats = np.stack([mean, rstd], axis=-1).astype(np.float32)
    m32, r32 = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)          # what the kernel reads
    h = (cg - m32[:, None, :, None]) * r32[:, None, :, None]
    gg = gam.astype(np.float64).reshape(8, K // 8); bb = bet.astype(np.float64).reshape(8, K // 8)
    d = dy.astype(np.float64).reshape(R, L, 8, K // 8) * _mish_grad64(h * gg + bb) * gg
    m1 = d.mean(axis=(1, 3), keepdims=True); m2 = (d * h).mean(axis=(1, 3), keepdims=True)
    dc = ((d - m1 - h * m2) * r32[:, None, :, None]).reshape(M, K)
    y = _conv5_f64(dc, W.astype(np.float64), L, -1) + (r1 if r1 is not None else 0.0) + (r2 if r2 is not None else 0.0)
    Ya = torch.full((M, N1 or N), float("nan"), device="cuda")
    Yb = torch.full((M, N - N1), float("nan"), device="cuda") if N1 else None
    amax, flag = C.c_float(0.0), C.c_int32(0)
    prev = float(np.abs(dc).max()) * 1.3
    ddy, dW, dc_, dst, dg, dbt = dev(dy), dev(W), dev(cst), dev(stats), dev(gam), dev(bet)      # (kept alive)
    dr1 = dev(r1) if r1 is not None else None; dr2 = dev(r2) if r2 is not None else None
    _lib.check(_lib.load().ramp_op_tkw(_lib.ptr(ddy), None, 0, _lib.ptr(dW), None, _lib.ptr(dr1), _lib.ptr(dr2), _lib.ptr(dc_), _lib.ptr(dst), _lib.ptr(dg), _lib.ptr(dbt),
                                       None, None, None, M, L, N, K, -1, N1 or N, prev, _lib.ptr(Ya), _lib.ptr(Yb) if N1 else None, None, None,
                                       C.byref(amax), C.byref(flag), S()), "ramp_op_tkw")
    got = Ya.cpu().numpy() if not N1 else np.concatenate([Ya.cpu().numpy(), Yb.cpu().numpy()], axis=1)
    e = rel(got, y)
    print(f"tkw bwd L={L} {K}->{N} rows={R} extras={extras}: {e:.2e}; recorded max {amax.value:.4f} (float64 {np.abs(dc).max():.4f})")
    assert flag.value == 0 and abs(amax.value - np.abs(dc).max()) < 2e-5 * np.abs(dc).max()
    assert e < 5e-6
    # a stale maximum (the operand grew 2^12-fold since it was recorded) raises the range flag instead of overflowing silently
    _lib.check(_lib.load().ramp_op_tkw(_lib.ptr(ddy), None, 0, _lib.ptr(dW), None, None, None, _lib.ptr(dc_), _lib.ptr(dst), _lib.ptr(dg),
                                       _lib.ptr(dbt), None, None, None, M, L, N, K, -1, N1 or N, prev / 4096.0, _lib.ptr(Ya), _lib.ptr(Yb) if N1 else None, None, None,
                                       C.byref(amax), C.byref(flag), S()), "ramp_op_tkw")
    assert flag.value == 1
