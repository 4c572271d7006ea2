"""Float64 statements of the plain-C++ kernels at the two ends of the score network and where the shared prefix fans out
(ramp_amd/csrc/rowops.hip: conv_in forward / backward, conv_out, expand_rows, combine_rows, cross_bias, the time table's per-block
lines), written from the reference's definitions -- Conv1d(S, C0, 5, padding=2) and the 1x1 residual Conv1d of the first
ResidualTemporalBlock, the final Conv1d(C0, S, 1), attn2 with a single context token (softmax over one key == 1, so
to_out(to_v(context))), cond_mlp = Linear(SiLU(temb)) -- in torch's weight layouts, not from the kernels.

Every linear operation also returns its ABSOLUTE COMPANION: the same formula on |operands|.  It is what the a-priori rounding bound of
a fp32 evaluation multiplies: any evaluation of sum_i a_i b_i (+ c) in fp32, in any order, with or without FMA contraction, lies within
gamma_N * (sum_i |a_i| |b_i| (+ |c|)) of the exact value, gamma_N = N u / (1 - N u), u = 2^-24, N the number of roundings on the longest
path.  A two-stage result chains the companions: |W2| (|W1| |x| + |b1|) + |b2|.

Also here, because the host test and the GPU test must agree on them: the operand regimes, the case tables and the packing of the
torch-layout weights into the layouts the kernels read."""
import itertools

import numpy as np

U = 2.0 ** -24
REGIMES = ("gauss", "offset", "spread")


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the rounding lengths N of the bound, per output (number of fp32 roundings on the longest path) -------------------------------
def n_conv_in_fwd(S): return 5 * S + 1          # 5 S products summed, + bias
def n_conv_in_bwd(C0): return 6 * C0 + 1        # 5 C0 + C0 products summed
def n_conv_out_f(C0): return C0 + 1             # C0 products summed, + bias
def n_conv_out_da(C0, S): return C0 + 1 + S     # the rounded f, then S products summed
def n_cross_bias(ctx_dim): return ctx_dim + 256 + 1
def n_combine(n_rp): return 2 * n_rp


def f64(*a):
    return [np.asarray(v, np.float64) for v in a]


# ---- first conv block input: Conv1d(S, C0, 5, padding=2) and the 1x1 residual Conv1d, rows shared across n_rp --------------------
def _conv_in_fwd(x, W5, b5, W1, b1):
    B, H, S = x.shape
    xp = np.pad(x, ((0, 0), (2, 2), (0, 0)))
    c1 = np.zeros((B, H, W5.shape[0]))
    for j in range(5):                                  # y[l] = sum_j W[:, :, j] x[l + j - 2], zero outside [0, H)
        c1 += np.einsum("bls,cs->blc", xp[:, j:j + H], W5[:, :, j])
    return c1 + b5, np.einsum("bls,cs->blc", x, W1[:, :, 0]) + b1


def conv_in_fwd(x, W5, b5, W1, b1, n_rp):
    """x (B, H, S); W5 (C0, S, 5), b5 (C0); W1 (C0, S, 1), b1 (C0).  Network row r reads trajectory r // n_rp.
    Returns (c1, res, c1_abs, res_abs), each (B n_rp, H, C0)."""
    x, W5, b5, W1, b1 = f64(x, W5, b5, W1, b1)
    c1, res = _conv_in_fwd(x, W5, b5, W1, b1)
    c1a, resa = _conv_in_fwd(np.abs(x), np.abs(W5), np.abs(b5), np.abs(W1), np.abs(b1))
    return tuple(np.repeat(v, n_rp, axis=0) for v in (c1, res, c1a, resa))


def _conv_in_bwd(dc1, dy, W5, W1):
    R, H, C0 = dc1.shape
    dp = np.pad(dc1, ((0, 0), (2, 2), (0, 0)))
    eps = np.einsum("rlc,cs->rls", dy, W1[:, :, 0])
    for j in range(5):                                  # the adjoint of y[l] += W_j x[l + j - 2]: dx[m] += W_j^T dy[m - j + 2]
        eps += np.einsum("rlc,cs->rls", dp[:, 4 - j:4 - j + H], W5[:, :, j])
    return eps


def conv_in_bwd(dc1, dy, W5, W1):
    """Input gradient of the pair above per network row: dc1, dy (R, H, C0) -> eps (R, H, S).  Returns (eps, eps_abs)."""
    dc1, dy, W5, W1 = f64(dc1, dy, W5, W1)
    return _conv_in_bwd(dc1, dy, W5, W1), _conv_in_bwd(np.abs(dc1), np.abs(dy), np.abs(W5), np.abs(W1))


# ---- last conv: Conv1d(C0, S, 1), and the seed of the energy gradient (E = 0.5 sum f^2, dE/df = f, dE/da = f Wf) ------------------
def conv_out(a, Wf, bf):
    """a (n_tok, C0); Wf (S, C0, 1), bf (S).  Returns (f, da, f_abs, da_abs): f (n_tok, S), da (n_tok, C0)."""
    a, Wf, bf = f64(a, Wf, bf)
    W = Wf[:, :, 0]
    f = a @ W.T + bf
    fa = np.abs(a) @ np.abs(W).T + np.abs(bf)
    return f, f @ W, fa, fa @ np.abs(W)


# ---- rows leaving / re-entering the shared prefix ---------------------------------------------------------------------------------------
def expand_rows(x, n_rp, rowbias=None, rowvar=None, row0=0):
    """x (B, L, C) float32 -> (B n_rp, L, C) float32: row r is trajectory r // n_rp, plus -- one float32 addition -- the constant
    rowbias[rowvar[row0 + r]] of rowbias (n_var, C) on every token.  Exact in float32, so stated in float32."""
    out = np.repeat(np.asarray(x, np.float32), n_rp, axis=0)
    if rowbias is not None:
        R = out.shape[0]
        out = out + np.asarray(rowbias, np.float32)[np.asarray(rowvar)[row0:row0 + R]][:, None, :]
    return out


def combine_rows(x, w):
    """x (B n_rp, L, C), w (n_rp) or per trajectory (B, n_rp) -> out[b] = sum_j w[b, j] x[b n_rp + j].  Returns (out, out_abs)."""
    x, w = f64(x, w)
    n_rp = w.shape[-1]
    B = x.shape[0] // n_rp
    w = np.broadcast_to(w, (B, n_rp))
    xr = x.reshape(B, n_rp, *x.shape[1:])
    return np.einsum("bj,bjlc->blc", w, xr), np.einsum("bj,bjlc->blc", np.abs(w), np.abs(xr))


# ---- attn2 with a single context token, per variant and block -------------------------------------------------------------------------
def cross_bias(lat, wv, wo, bo):
    """lat (n_var, ctx_dim); per block to_v.weight wv[k] (256, ctx_dim), to_out.0.weight wo[k] (256, 256), to_out.0.bias bo[k] (256).
    Returns (out, out_abs), (n_var, n_blk, 256)."""
    lat = np.asarray(lat, np.float64)
    out = np.stack([(lat @ v.T) @ o.T + b for v, o, b in zip(*map(lambda t: f64(*t), (wv, wo, bo)))], axis=1)
    oa = np.stack([(np.abs(lat) @ np.abs(v).T) @ np.abs(o).T + np.abs(b) for v, o, b in zip(*map(lambda t: f64(*t), (wv, wo, bo)))], axis=1)
    return out, oa


# ---- the time table's per-block lines --------------------------------------------------------------------------------------------------
def cond_line(temb, W, b):
    """cond_mlp of one ResidualTemporalBlock on the time embedding temb (T, 32): Linear(SiLU(temb)), W (cout, 32), b (cout)."""
    temb, W, b = f64(temb, W, b)
    return (temb / (1.0 + np.exp(-temb))) @ W.T + b


def cond_line_f32(temb32, W, b):
    """The same in float32 numpy with sequential sums, from a float32 time embedding: the rounding a fp32 evaluation of the line carries
    on top of its input's."""
    t = np.asarray(temb32, np.float32)
    st = (t / (np.float32(1) + np.exp(-t))).astype(np.float32)
    W = np.asarray(W, np.float32)
    acc = np.zeros((t.shape[0], W.shape[0]), np.float32)
    for k in range(32):
        acc = acc + st[:, k:k + 1] * W[None, :, k]
    return acc + np.asarray(b, np.float32)


TIME_BAR = 5e-6         # the project's bar for temb (test_time_table_at_every_timestep)
TIME_NETS = ((4, 48, False), (7, 48, True))
TIME_T = 100


def rtb_names(sd):
    return sorted({k[:-len(".cond_mlp.1.weight")] for k in sd if k.endswith(".cond_mlp.1.weight")})


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def time_line_bars(sd, temb64):
    """{block: (bar, restatement's worst rel over t)}: TIME_BAR, unless the float32 restatement of the block's line (from the float64
    temb rounded to float32) comes within 2x of it; then 4x the restatement's error (the margin is for libm differences between numpy
    and the device)."""
    bars = {}
    t32 = temb64.astype(np.float32)
    for name in rtb_names(sd):
        W, b = sd[name + ".cond_mlp.1.weight"], sd[name + ".cond_mlp.1.bias"]
        ref, got = cond_line(temb64, W, b), cond_line_f32(t32, W, b)
        e = max(_rel(got[t], ref[t]) for t in range(ref.shape[0]))
        bars[name] = (4.0 * e if e > TIME_BAR / 2 else TIME_BAR, e)
    return bars


# ---- operand regimes --------------------------------------------------------------------------------------------------------------------
def rng(*key):
    return np.random.default_rng([sum(map(ord, str(k))) * 131 + i for i, k in enumerate(key)])


def data(g, shape, regime):
    """Activations / gradients: Gaussian; offset (mean 3); a per-row magnitude spread of e^+-6 (rows = the leading axis)."""
    a = g.standard_normal(shape)
    if regime == "offset":
        a += 3.0
    elif regime == "spread":
        a *= np.exp(g.uniform(-6.0, 6.0, size=(shape[0],) + (1,) * (len(shape) - 1)))
    return a.astype(np.float32)


def weight(g, shape, fan_in, regime):
    """Weights at the usual 1 / sqrt(fan_in) scale; the offset regime shifts them too (coherent sums: no cancellation to hide behind),
    the spread regime scales every output channel (the leading axis) by e^+-2."""
    w = g.standard_normal(shape)
    if regime == "offset":
        w += 3.0
    elif regime == "spread":
        w *= np.exp(g.uniform(-2.0, 2.0, size=(shape[0],) + (1,) * (len(shape) - 1)))
    return (w / np.sqrt(fan_in)).astype(np.float32)


# ---- packing into the layouts the kernels read -------------------------------------------------------------------------------------------
def pack_w5(W5): return np.ascontiguousarray(np.transpose(W5, (2, 1, 0)))       # (C0, S, 5) -> [5][S][C0]
def pack_w1(W1): return np.ascontiguousarray(W1[:, :, 0].T)                      # (C0, S, 1) -> [S][C0]
def pack_wf(Wf): return np.ascontiguousarray(Wf[:, :, 0])                        # (S, C0, 1) -> [S][C0]


# ---- case tables --------------------------------------------------------------------------------------------------------------------------
CONV_C0 = (16, 32, 64)
CONV_IN_S = (2, 3, 4, 7, 16)
CONV_IN_H = (1, 2, 5, 48, 64)
CONV_IN_B = (1, 3, 7)
CONV_IN_NRP = (1, 2, 3, 8)


def conv_in_cases():
    """Every (C0, S, H) once, the trajectory count B, n_rp and the regime cycling so that every pair of factor values meets; R = n_rp B
    network rows forward and backward (R in {1, 3, 7} where n_rp = 1).  H < 5: every tap partly out of range; H C0 and H S below, at
    (H S = 64 x 4) and not a multiple of the 256-thread block.  Last: the largest LDS the
    launchers admit (H = 64, S = 16, C0 = 64) in all three regimes."""
    out = []
    for (ic, C0), (i_s, S), (ih, H) in itertools.product(enumerate(CONV_C0), enumerate(CONV_IN_S), enumerate(CONV_IN_H)):
        out.append(dict(C0=C0, S=S, H=H, B=CONV_IN_B[(ic + i_s + ih) % 3], n_rp=CONV_IN_NRP[(ic + 2 * i_s + 3 * ih) % 4],
                        regime=REGIMES[(ic + i_s + 2 * ih) % 3]))
    for regime in REGIMES:
        out.append(dict(C0=64, S=16, H=64, B=3, n_rp=1, regime=regime))
    return out


def conv_in_operands(c):
    g = rng("conv_in", *sorted(c.items()))
    C0, S, H, B, R, rg = c["C0"], c["S"], c["H"], c["B"], c["B"] * c["n_rp"], c["regime"]
    return dict(x=data(g, (B, H, S), rg), W5=weight(g, (C0, S, 5), 5 * S, rg), b5=weight(g, (C0,), 1, rg),
                W1=weight(g, (C0, S, 1), S, rg), b1=weight(g, (C0,), 1, rg),
                dc1=data(g, (R, H, C0), rg), dy=data(g, (R, H, C0), rg))


CONV_OUT_S = (2, 3, 16)
CONV_OUT_NTOK = (1, 255, 256, 257, 700)


def conv_out_cases():
    out = []
    for (ic, C0), (i_s, S), (it, n_tok) in itertools.product(enumerate(CONV_C0), enumerate(CONV_OUT_S), enumerate(CONV_OUT_NTOK)):
        out.append(dict(C0=C0, S=S, n_tok=n_tok, regime=REGIMES[(ic + i_s + it) % 3]))
    return out


def conv_out_operands(c):
    g = rng("conv_out", *sorted(c.items()))
    return dict(a=data(g, (c["n_tok"], c["C0"]), c["regime"]), Wf=weight(g, (c["S"], c["C0"], 1), c["C0"], c["regime"]),
                bf=weight(g, (c["S"],), 1, c["regime"]))


GRID_ROUND = 16384 * 256        # float4 elements one round of the row kernels' grid covers


def expand_cases():
    """n_rp x with / without the row constant x L (w % c4 wraps where L > 1); the constant's table has 9 variants, a line stride above C
    (12 blocks x 256, the engine's n_blocks_total x 256) and is entered at row0 = 5 of a longer row -> variant table.  Last: just above
    one round of the grid."""
    out = []
    for (i, n_rp), (j, L), bias in itertools.product(enumerate((1, 2, 3, 8)), enumerate((1, 3, 48)), (False, True)):
        out.append(dict(n_rp=n_rp, L=L, C=(256, 64, 32)[(i + j) % 3], B=(1, 3, 7)[(i + 2 * j) % 3], bias=bias, row0=5 if bias else 0))
    out.append(dict(n_rp=3, L=1, C=256, B=65538 // 3, bias=True, row0=5))
    assert out[-1]["B"] * 3 * 256 // 4 > GRID_ROUND
    return out


EXPAND_NVAR, EXPAND_STRIDE, EXPAND_OFF = 9, 12 * 256, 2 * 256      # the launch enters every line at its block's 256 floats (here block 2)


def expand_slice(o, c):
    """The (n_var, C) constants a launch with rowbias + EXPAND_OFF reads from the (n_var, EXPAND_STRIDE) table; None without one."""
    return o["rowbias"][:, EXPAND_OFF:EXPAND_OFF + c["C"]] if c["bias"] else None


def expand_operands(c):
    g = rng("expand", *sorted(c.items()))
    R = c["B"] * c["n_rp"]
    o = dict(x=g.standard_normal((c["B"], c["L"], c["C"]), dtype=np.float32))
    if c["bias"]:
        o["rowbias"] = g.standard_normal((EXPAND_NVAR, EXPAND_STRIDE), dtype=np.float32)
        o["rowvar"] = g.integers(0, EXPAND_NVAR, size=c["row0"] + R + 11).astype(np.int32)
    return o


def combine_cases():
    """combine_rows (host weights) at n_rp 1, 2, 3 and combine_rows_weighted (per-row device weights, entered at a chunk's first
    trajectory b0 = 4) at n_rp 2, 5, 8, in the three regimes; one case each just above one round of the grid."""
    out = []
    for weighted, nrps in ((False, (1, 2, 3)), (True, (2, 5, 8))):
        for (i, n_rp), (j, rg) in itertools.product(enumerate(nrps), enumerate(REGIMES)):
            out.append(dict(weighted=weighted, n_rp=n_rp, regime=rg, B=(1, 3, 7)[(i + j) % 3], L=(1, 3, 48)[(i + 2 * j) % 3],
                            C=(256, 64, 32)[(2 * i + j) % 3]))
        out.append(dict(weighted=weighted, n_rp=2, regime="gauss", B=65537, L=1, C=256))
        assert out[-1]["B"] * 256 // 4 > GRID_ROUND
    return out


COMBINE_B0 = 4


def combine_operands(c):
    g = rng("combine", *sorted(c.items()))
    o = dict(x=data(g, (c["B"] * c["n_rp"], c["L"], c["C"]), c["regime"]))
    if c["weighted"]:       # the whole job's weights; the chunk's start at trajectory COMBINE_B0
        o["w_all"] = data(g, (COMBINE_B0 + c["B"], c["n_rp"]), "offset" if c["regime"] == "offset" else "gauss")
        o["w"] = o["w_all"][COMBINE_B0:]
    else:
        o["w"] = data(g, (c["n_rp"],), "offset" if c["regime"] == "offset" else "gauss")
    return o


def cross_bias_cases():
    out = []
    for (i, ctx), (j, n_var), (k, n_blk) in itertools.product(enumerate((1, 31, 32, 512)), enumerate((1, 4, 9)), enumerate((1, 2, 12))):
        out.append(dict(ctx_dim=ctx, n_var=n_var, n_blk=n_blk, regime=REGIMES[(i + j + k) % 3]))
    return out


def cross_bias_operands(c):
    g = rng("cross_bias", *sorted(c.items()))
    rg, nb, ctx = c["regime"], c["n_blk"], c["ctx_dim"]
    return dict(lat=data(g, (c["n_var"], ctx), rg), wv=[weight(g, (256, ctx), ctx, rg) for _ in range(nb)],
                wo=[weight(g, (256, 256), 256, rg) for _ in range(nb)], bo=[weight(g, (256,), 1, rg) for _ in range(nb)])
