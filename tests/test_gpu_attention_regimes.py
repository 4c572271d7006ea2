"""The four attention kernels (attention.hip, atk.hip, atb.hip, atl.hip through ramp_op_attention / _bwd, ramp_op_ato, ramp_op_atb,
ramp_op_abl) at sharp, flat and unevenly scaled softmax: the regimes of attention_ref.py (test_attention_ref_host.py proves them on the
CPU) against float64, with bars max(b0, 4 x the float32 evaluation's error on the same case), exact zeros / exact power-of-two scaling
where the arithmetic promises them, per head and per sample where one scale serves several, and the score network with sharpened
attention weights.  Out of scope: non-finite inputs, operand maxima below ~2^-100 (attention_ref.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as A
import util
from oracle import ramp_oracle as O
from ramp_amd import _lib, synth
from util import GOLDEN, weights

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _t(a):
    return torch.tensor(np.asarray(a))                            # (a copy: the shared case arrays are read-only)


def dev(a):
    return _t(a).cuda()


def _report(entry, c, rows):
    """rows: (block, measured, floor, bar); printed before anything is asserted."""
    print(f"{entry} {c['regime']} L={c['L']} R={c['R']}: " + "  ".join(f"{n} {e:.2e} (fp32 {f:.1e}, bar {b:.1e})" for n, e, f, b in rows))


def _check(rows, what):
    for n, e, f, b in rows:
        assert e < b, (what, n, e, f, b)


def _uniform_rows(c, o, bar):
    """equal_large / flat_*: within a sample all rows of o agree, and equal the float64 mean of v, to the bar."""
    L, R = c["L"], c["R"]
    v = np.asarray(c["qkv"][:, 512:], np.float64).reshape(R, L, 256)
    mean = np.repeat(v.mean(1, keepdims=True), L, axis=1)
    got = np.asarray(o, np.float64).reshape(R, L, 256)
    top = np.abs(mean).max()
    assert np.abs(got - got[:, :1]).max() < bar * top and np.abs(got - mean).max() < bar * top


# ---- the plain kernels (attention.hip): every length, the ones the fused kernels refuse included ---------------------------------------
def _plain(qkv, dout, L):
    R = qkv.shape[0] // L
    lib = _lib.load()
    o = torch.full((R * L, 256), NAN, device="cuda"); dqkv = torch.full((R * L, 768), NAN, device="cuda")
    q_d, d_d = dev(qkv), dev(dout)
    _lib.check(lib.ramp_op_attention(_lib.ptr(q_d), _lib.ptr(o), R, L, _lib.current_stream()))
    _lib.check(lib.ramp_op_attention_bwd(_lib.ptr(q_d), _lib.ptr(d_d), _lib.ptr(dqkv), R, L, _lib.current_stream()))
    return o.cpu().numpy(), dqkv.cpu().numpy()


def _grad_rows(c, got, b0):
    e = A.grad_errors(c["regime"], got, c["dqkv"], c["qkv"], c["dout"])
    return [(n, e[n], c["floor"][n], A.bar(b0, c["floor"][n])) for n in ("dq", "dk", "dv")]


def _head_rows(c, o, dqkv, b0_o, b0_g):
    rows = []
    if o is not None:
        rows += [(f"o/h{h}", e, f, A.bar(b0_o, f)) for h, (e, f) in enumerate(zip(A.head_errors(o, c["o"]), c["floor"]["heads_o"]))]
    if dqkv is not None:
        for n, s in A.BLOCKS:
            rows += [(f"{n}/h{h}", e, f, A.bar(b0_g, f)) for h, (e, f) in enumerate(zip(A.head_errors(dqkv[:, s], c["dqkv"][:, s]), c["floor"]["heads"][n]))]
    return rows


@pytest.mark.parametrize("L,R", A.PLAIN_SHAPES)
@pytest.mark.parametrize("regime", A.ACCURACY_REGIMES)
def test_plain_attention_in_every_regime(regime, L, R):
    """attention.hip forward and backward: o, d(q), d(k), d(v) per block against float64 (saturated regimes: d(q), d(k) on their natural
    scale), per head in loud_head, uniform rows where all logits are equal; nothing NaN."""
    c = A.case(regime, L, R)
    o, dqkv = _plain(c["qkv"], c["dout"], L)
    rows = [("o", A.rel(o, c["o"]), c["floor"]["o"], A.bar(A.B0["attention"], c["floor"]["o"]))] + _grad_rows(c, dqkv, A.B0["attention_bwd"])
    if regime == "loud_head":
        rows += _head_rows(c, o, dqkv, A.B0["attention"], A.B0["attention_bwd"])
    _report("attention", c, rows)
    assert np.isfinite(o).all() and np.isfinite(dqkv).all()
    _check(rows, "attention")
    if regime in ("equal_large", "flat_q0", "flat_k0"):
        _uniform_rows(c, o, rows[0][3])


# ---- atk.hip through ramp_op_ato -------------------------------------------------------------------------------------------------------
_ATO_W = {}


def _ato_operands(L, R, extras):
    """Wo = N(0, 1) / 16 and, with `extras`, bias, residual and a per-row-variant constant (3 variants); zeros otherwise."""
    key = (L, R, extras)
    if key not in _ATO_W:
        g = torch.Generator(device="cpu").manual_seed(5000 + 100 * L + R)
        M = R * L
        Wo = torch.randn(256, 256, generator=g) / 16.0
        if extras:
            bias, resid, rowbias = torch.randn(256, generator=g) * 0.3, torch.randn(M, 256, generator=g), torch.randn(3, 256, generator=g) * 0.5
        else:
            bias, resid, rowbias = torch.zeros(256), torch.zeros(M, 256), torch.zeros(3, 256)
        _ATO_W[key] = (Wo, bias, resid, rowbias, (torch.arange(R) % 3).to(torch.int32))
    return _ATO_W[key]


def _ato_block(o, ops, L, dtype):
    Wo, bias, resid, rowbias, rowvar = ops
    o = _t(o).to(dtype)
    return (resid.to(dtype) + o @ Wo.to(dtype).T + bias.to(dtype) + rowbias.to(dtype)[rowvar.long().repeat_interleave(L)]).numpy()


def _ato(qkv, ops, L, prev, rb=True):
    Wo, bias, resid, rowbias, rowvar = (t.cuda() for t in ops)
    M = qkv.shape[0]
    Y = torch.full((M, 256), NAN, device="cuda")
    out, flag = C.c_float(-1.0), C.c_int32(-1)
    q_d = dev(qkv)
    _lib.check(_lib.load().ramp_op_ato(_lib.ptr(q_d), _lib.ptr(Wo), _lib.ptr(bias), _lib.ptr(resid), _lib.ptr(rowbias) if rb else None,
                                       _lib.ptr(rowvar) if rb else None, 3 if rb else 0, L, M, prev, _lib.ptr(Y), C.byref(out), C.byref(flag), None), "ramp_op_ato")
    return Y.cpu().numpy(), out.value, flag.value


@pytest.mark.parametrize("L,R", A.FUSED_SHAPES)
@pytest.mark.parametrize("regime", A.ACCURACY_REGIMES)
def test_ato_in_every_regime(regime, L, R):
    """ramp_op_ato with bias, residual and row constant on: y against the float64 block, unscaled (prev = 0) and scaled from the recorded
    maximum; the recorded maximum is max |o|; where all logits are equal, y is the projection of the sample's mean v."""
    c = A.case(regime, L, R)
    ops = _ato_operands(L, R, True)
    y64 = _ato_block(c["o"], ops, L, torch.float64)
    floor = A.rel(_ato_block(c["o32"], ops, L, torch.float32), y64)
    b = A.bar(A.B0["ato"], floor)
    omax = np.abs(c["o"]).max()
    y0, amax0, flag0 = _ato(c["qkv"], ops, L, 0.0)
    y1, amax1, flag1 = _ato(c["qkv"], ops, L, amax0)
    rows = [("y", A.rel(y0, y64), floor, b), ("y, scaled", A.rel(y1, y64), floor, b)]
    _report("ato", c, rows)
    assert np.isfinite(y0).all() and np.isfinite(y1).all()
    _check(rows, "ato")
    assert abs(amax0 - omax) <= b * omax and abs(amax1 - omax) <= b * omax, (amax0, amax1, omax)
    assert flag1 == 0 and (flag0 == 0 or omax < 0.125), (flag0, flag1)
    if regime in ("equal_large", "flat_q0", "flat_k0"):
        v = np.asarray(c["qkv"][:, 512:], np.float64).reshape(R, L, 256)
        mean = np.repeat(v.mean(1, keepdims=True), L, axis=1).reshape(R * L, 256)
        assert A.rel(y1, _ato_block(mean, ops, L, torch.float64)) < b


def test_ato_per_head_accuracy_with_heads_of_different_magnitude():
    """loud_head through ramp_op_ato with Wo = identity / 16 (exact in the weight planes) and nothing added, so y = o / 16 column by column:
    every head, the one with v at 2^-8 of the others included, relative to ITS OWN maximum and held to the same bar -- the operand scales sq,
    sk, sv are per head; only the split of o for the projection shares one scale (from the recorded maximum), and 2^-8 of it still keeps
    2^-30 / 2^-8 = 2^-22 of the head's own."""
    for L, R in A.FUSED_SHAPES:
        c = A.case("loud_head", L, R)
        ops = (torch.eye(256) / 16.0, torch.zeros(256), torch.zeros(R * L, 256), torch.zeros(3, 256), torch.zeros(R, dtype=torch.int32))
        _, amax, _ = _ato(c["qkv"], ops, L, 0.0, rb=False)
        y, _, flag = _ato(c["qkv"], ops, L, amax, rb=False)
        e = A.head_errors(y * 16.0, c["o"])
        bars = [A.bar(A.B0["ato"], f) for f in c["floor"]["heads_o"]]
        print(f"ato loud_head L={L} R={R}: per head " + " ".join(f"{x:.2e}" for x in e) + "  bars " + " ".join(f"{x:.1e}" for x in bars))
        assert flag == 0
        for h in range(4):
            assert e[h] < bars[h], (L, R, h, e[h])


# ---- atb.hip through ramp_op_atb -------------------------------------------------------------------------------------------------------
def _atb(qkv, dout, L):
    M = qkv.shape[0]
    got = torch.full((M, 768), NAN, device="cuda")
    q_d, d_d = dev(qkv), dev(dout)
    _lib.check(_lib.load().ramp_op_atb(_lib.ptr(q_d), _lib.ptr(d_d), _lib.ptr(got), M, L, None), "ramp_op_atb")
    return got.cpu().numpy()


@pytest.mark.parametrize("L,R", A.FUSED_SHAPES)
@pytest.mark.parametrize("regime", A.ACCURACY_REGIMES)
def test_atb_in_every_regime(regime, L, R):
    c = A.case(regime, L, R)
    got = _atb(c["qkv"], c["dout"], L)
    rows = _grad_rows(c, got, A.B0["atb"])
    if regime == "loud_head":
        rows += _head_rows(c, None, got, 0.0, A.B0["atb"])
    _report("atb", c, rows)
    assert np.isfinite(got).all()
    _check(rows, "atb")


# ---- atl.hip through ramp_op_abl: qkv out of the real prologue LayerNorm -> Wqkv ---------------------------------------------------------
ABL_REGIMES = A.ACCURACY_REGIMES + ["zero_v", "zero_dout", "quiet_sample"]
_ABL = {}


def _abl_case(regime, L, R):
    """The construction of test_abl_attention_backward_with_ln1_backward_against_float64_autograd with the regime's gains on the q, k, v rows
    of Wqkv (q, k, v = LayerNorm(z) W^T have unit scale at gain 1); references by float64 and float32 autograd.
    equal_large is the one regime no gain produces: keys that are equal within a sample need equal z rows, which make q and v equal too --
    then d(P) is constant along the keys, the true dS is 0 everywhere and what is measured is whether a float32 sum of L equal terms happens to
    be exact (the kernel and torch's float32 both gave 2e-6 .. 5e-6 at L = 48, 32, 6, 3 and 2e-8 .. 5e-8 where the sum is exact, torch at L = 32
    and the kernel at L = 16).  The kernel takes qkv as an operand of its own, so that regime feeds it attention_ref's qkv and d(o) directly
    next to an unrelated z and W, and the reference chains float64 attention backward -> Wqkv^T -> LayerNorm backward."""
    key = (regime, L, R)
    if key in _ABL:
        return _ABL[key]
    M = R * L
    g = torch.Generator(device="cpu").manual_seed(7000 + A.case_seed(regime, L, R))
    z = torch.randn(M, 256, generator=g) * 1.5 + 0.3
    ln_g = 1.0 + 0.2 * torch.randn(256, generator=g)
    ln_b = 0.1 * torch.randn(256, generator=g)
    W = torch.randn(768, 256, generator=g) / 16.0
    dout = torch.randn(M, 256, generator=g)
    add = torch.randn(M, 256, generator=g)
    noise = torch.randn(256, 256, generator=g) / 16.0
    Wq, Wk, Wv = W[:256], W[256:512], W[512:]
    Wv *= 0.4
    given = None
    if regime in ("sharp3", "sharp6"):
        gain = 3.0 if regime == "sharp3" else 6.0
        Wq *= gain; Wk *= gain
    elif regime == "onehot":
        Wq *= 2.0; Wk.copy_(8.0 * Wq + 0.01 * noise)
    elif regime == "equal_large":
        given = A.case(regime, L, R)
        dout = _t(given["dout"]).clone()
    elif regime == "flat_q0":
        Wq.zero_(); Wk *= 1.3
    elif regime == "flat_k0":
        Wk.zero_(); Wq *= 1.3
    elif regime == "loud_head":
        Wq *= 0.4; Wk *= 0.4; Wq[128:192] *= 16.0; Wk[128:192] *= 16.0; Wv[0:64] *= 2.0 ** -8
    else:
        Wq *= 1.3; Wk *= 1.3
        if regime == "zero_v":
            Wv.zero_()
        elif regime == "zero_dout":
            dout.zero_()
        elif regime == "quiet_sample":
            dout[(R // 2) * L:(R // 2 + 1) * L] *= A.QUIET_SHIFT
            add.zero_()                                           # (the quiet sample's gradient is read off the output itself)

    def run(dtype):
        zd = z.to(dtype).clone().requires_grad_(True)
        ln = torch.nn.functional.layer_norm(zd, (256,), ln_g.to(dtype), ln_b.to(dtype), 1e-5)
        if given is not None:
            dqkv = _t(given["dqkv"] if dtype == torch.float64 else given["dqkv32"])
            ln.backward(dqkv @ W.to(dtype))
            return zd.grad.numpy(), _t(given["qkv"]), float(dqkv.abs().max())
        qkv = ln @ W.to(dtype).t()
        qkv.retain_grad()
        y = qkv.reshape(R, L, 3, 4, 64)
        q, k, v = y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2), y[:, :, 2].transpose(1, 2)
        o = (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(M, 256)
        o.backward(dout.to(dtype))
        return zd.grad.numpy(), qkv.detach(), float(qkv.grad.abs().max())

    dz64, qkv64, true_max = run(torch.float64)
    dz32, _, _ = run(torch.float32)
    a64 = add.double().numpy()
    _ABL[key] = dict(regime=regime, L=L, R=R, dz=dz64, ref=dz64 + a64, floor=A.rel(dz32.astype(np.float64) + a64, dz64 + a64), true_max=true_max, add=add,
                     dev=(qkv64.float().cuda(), dout.cuda(), W.t().contiguous().cuda(), z.cuda(), ln_g.cuda(), add.cuda()))
    return _ABL[key]


def _abl(c, prev):
    M = c["R"] * c["L"]
    got = torch.full((M, 256), NAN, device="cuda")
    amax, flag = C.c_float(-1.0), C.c_int32(-1)
    _lib.check(_lib.load().ramp_op_abl(*(_lib.ptr(t) for t in c["dev"]), M, c["L"], prev, _lib.ptr(got), C.byref(amax), C.byref(flag), None), "ramp_op_abl")
    return got.cpu().numpy(), amax.value, flag.value


@pytest.mark.parametrize("L,R", A.FUSED_SHAPES)
@pytest.mark.parametrize("regime", A.ACCURACY_REGIMES)
def test_abl_in_every_regime(regime, L, R):
    """ramp_op_abl (attention backward -> Wqkv^T -> LayerNorm backward, + add) against float64 autograd of the same chain, unscaled and scaled
    from the recorded maximum max |d(qkv)|."""
    c = _abl_case(regime, L, R)
    ref = c["ref"]
    b = A.bar(A.B0["abl"], c["floor"])
    got0, amax0, flag0 = _abl(c, 0.0)
    got1, amax1, flag1 = _abl(c, amax0)
    rows = [("dz", A.rel(got0, ref), c["floor"], b), ("dz, scaled", A.rel(got1, ref), c["floor"], b)]
    _report("abl", c, rows)
    assert np.isfinite(got0).all() and np.isfinite(got1).all()
    _check(rows, "abl")
    tm = c["true_max"]
    assert abs(amax0 - tm) <= A.bar(2e-5, c["floor"]) * tm and abs(amax1 - tm) <= A.bar(2e-5, c["floor"]) * tm, (amax0, amax1, tm)
    assert flag1 == 0 and (flag0 == 0 or tm < 0.125 or tm >= 60000), (flag0, flag1)


# ---- exactness ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R", A.PLAIN_SHAPES)
def test_zero_v_gives_exact_zeros(L, R):
    """v == 0: o, d(q), d(k) are exactly 0 in every kernel (an operand maximum of 0 takes scale 1, nothing divides by it), y of ato is
    exactly 0 with recorded maximum 0 and no flag, on a second launch with prev = 0.0 too; d(v) = P^T d(o) stays accurate; nothing is NaN."""
    c = A.case("zero_v", L, R)
    o, dqkv = _plain(c["qkv"], c["dout"], L)
    assert not o.any() and not dqkv[:, :512].any()
    assert A.rel(dqkv[:, 512:], c["dqkv"][:, 512:]) < A.bar(A.B0["attention_bwd"], c["floor"]["dv"])
    if not A.wave_tokens(L):
        return
    ops = _ato_operands(L, R, False)
    for _ in range(2):
        y, amax, flag = _ato(c["qkv"], ops, L, 0.0)
        assert not y.any() and amax == 0.0 and flag == 0, (np.abs(y).max(), amax, flag)
    got = _atb(c["qkv"], c["dout"], L)
    assert not got[:, :512].any()
    assert A.rel(got[:, 512:], c["dqkv"][:, 512:]) < A.bar(A.B0["atb"], c["floor"]["dv"])
    a = _abl_case("zero_v", L, R)
    got0, amax0, _ = _abl(a, 0.0)
    got1, _, flag1 = _abl(a, amax0)
    ref = a["ref"]
    assert flag1 == 0 and np.isfinite(got0).all()
    assert A.rel(got0, ref) < A.bar(A.B0["abl"], a["floor"]) and A.rel(got1, ref) < A.bar(A.B0["abl"], a["floor"])


@pytest.mark.parametrize("L,R", A.PLAIN_SHAPES)
def test_zero_dout_gives_exact_zeros(L, R):
    """d(o) == 0: d(q), d(k), d(v) are exactly 0, the output of abl is exactly `add`, its recorded maximum 0 and no flag (sds, sdo come from
    a maximum of 0); nothing is NaN."""
    c = A.case("zero_dout", L, R)
    _, dqkv = _plain(c["qkv"], c["dout"], L)
    assert not dqkv.any()
    if not A.wave_tokens(L):
        return
    assert not _atb(c["qkv"], c["dout"], L).any()
    a = _abl_case("zero_dout", L, R)
    for _ in range(2):
        got, amax, flag = _abl(a, 0.0)
        assert not (got - a["add"].numpy()).any() and amax == 0.0 and flag == 0, (amax, flag)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("L,R", A.POW2_SHAPES)
def test_power_of_two_operand_scales_are_undone_exactly(L, R):
    """sharp3.  q x 2^6 with k x 2^-6 leaves every output bit-identical; v x 2^(+-6) scales o, d(q), d(k) (and y, the recorded maximum of ato,
    with prev scaled too) by exactly 2^(+-6) and leaves d(v) unchanged -- every per-wave scale (sq, sk, sv, sdo, sds, the P planes' 8192, the
    delayed scale of o) is a power of two that is undone exactly, so a scale that is applied and not undone, or a quantity that does not
    follow its operand, shows as a changed bit.  ato runs with nothing added (y = Wo o).  abl: see the comment at its part below."""
    c = A.case("sharp3", L, R)
    qkv, dout = c["qkv"], c["dout"]
    ops = _ato_operands(L, R, False)
    fused = bool(A.wave_tokens(L))

    def run(x, prev):
        o, g = _plain(x, dout, L)
        return dict(o=o, g=g, y=_ato(x, ops, L, prev) if fused else None, b=_atb(x, dout, L) if fused else None)

    _, amax, _ = _ato(qkv, ops, L, 0.0)
    base = run(qkv, amax)
    assert base["y"][2] == 0
    swap = qkv.copy(); swap[:, :256] *= 64.0; swap[:, 256:512] /= 64.0
    got = run(swap, amax)
    assert np.array_equal(_bits(got["o"]), _bits(base["o"])) and np.array_equal(_bits(got["y"][0]), _bits(base["y"][0])) and got["y"][1:] == base["y"][1:]
    for name in ("g", "b"):
        unscale = np.concatenate([np.full(256, 64.0), np.full(256, 1 / 64.0), np.ones(256)]).astype(np.float32)      # d(q) follows 1 / its operand's scale
        assert np.array_equal(_bits(got[name] * unscale), _bits(base[name])), name
    for s in (64.0, 1 / 64.0):
        x = qkv.copy(); x[:, 512:] *= s
        got = run(x, amax * s)
        assert got["y"][2] == 0 and got["y"][1] == base["y"][1] * s, (s, got["y"][1:], base["y"][1:])
        assert np.array_equal(_bits(got["o"] / s), _bits(base["o"])) and np.array_equal(_bits(got["y"][0] / s), _bits(base["y"][0])), s
        for name in ("g", "b"):
            unscale = np.concatenate([np.full(512, 1 / s), np.ones(256)]).astype(np.float32)
            assert np.array_equal(_bits(got[name] * unscale), _bits(base[name])), (name, s)
    # abl: d(q) / 2^6 and d(k) 2^6 reach the output through Wqkv^T, so the q and k columns of W follow their operands and the true output is
    # unchanged.  Not bit-identical, and not within the entry's bar either, for a reason the code states: d(qkv) is ONE operand of the
    # projection, split into fp16 planes under one power-of-two scale taken from the tensor's maximum (scale_of: 2^-30 of that maximum is
    # kept).  d(k) 2^6 now is that maximum and d(q) / 2^6 sits 2^-12 below it -- the quiet-sample trade-off with a quiet BLOCK: 2^-18 of its
    # own size, and d(q) Wq is as large a part of the output as before.  Bound: 2^-30 2^12 and the factor 8 of head room the per-sample
    # bound 2^-17 allows the accumulation = 2^-15 (first written as the entry's bar, on the wrong assumption that only W's planes would round
    # differently: 7.3e-6 / 5.8e-6 measured against 6.4e-6 / 1.1e-5; W's own scale targets 2^10 and keeps 2^-35 of max |W|).  What this part
    # holds is that each scale is undone -- a forgotten 2^6 is off by 63 -- against float64 and against the unscaled launch.
    a = _abl_case("sharp3", L, R)
    _, amax_a, _ = _abl(a, 0.0)
    base_a, _, flag = _abl(a, amax_a)
    t = list(a["dev"])
    t[0] = t[0].clone(); t[0][:, :256] *= 64.0; t[0][:, 256:512] /= 64.0
    t[2] = t[2].clone(); t[2][:, :256] *= 64.0; t[2][:, 256:512] /= 64.0
    moved = dict(a, dev=tuple(t))
    _, amax_m, _ = _abl(moved, 0.0)
    got_a, _, flag_m = _abl(moved, amax_m)
    b = max(2.0 ** -15, A.bar(A.B0["abl"], a["floor"]))
    print(f"abl sharp3 L={L} R={R}, q x 2^6 / k x 2^-6 with W's columns following: {A.rel(got_a, a['ref']):.2e} from float64, {A.rel(got_a, base_a):.2e} from the unscaled launch (bar {b:.1e})")
    assert flag == 0 and flag_m == 0
    assert A.rel(got_a, a["ref"]) < b and A.rel(got_a, base_a) < b


# ---- one scale for several samples -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R", A.QUIET_SHAPES)
def test_per_sample_accuracy_with_a_quiet_sample(L, R):
    """The trade-off of one power-of-two scale per operand TENSOR, per sample, for ato (forward: sample R // 2 has v x 2^-10), atb and abl
    (its d(o) x 2^-10): every sample's error relative to ITS OWN largest reference entry, scaled from the recorded maximum.  Loud samples stay
    inside the entry's bar; the quiet one below 2^-17 (2^-30 of the tensor maximum = 2^-20 of its own, with head room for the accumulation:
    the bound of test_abl_per_sample_accuracy_under_a_magnitude_spread).  At (48, 4) the quiet sample owns its wave, which changes nothing for
    ato and abl: they split their projection operand (o, d(qkv)) by the TENSOR's recorded maximum either way.  Recorded, not asserted -- whether
    the quiet sample reaches the loud bar: ato (2.0e-6, 1.9e-6, 1.5e-6) and atb (<= 3.9e-7; all of its scales are per wave and head, and 2^-10
    below the wave's maximum still leaves the low plane its bits) do at every shape, abl (4.7e-6, 4.1e-6, 6.5e-6 against 4e-6) at none."""
    qs = R // 2
    f = A.case("quiet_sample", L, R, "fwd")
    ops = _ato_operands(L, R, False)
    y64 = _ato_block(f["o"], ops, L, torch.float64)
    _, amax, _ = _ato(f["qkv"], ops, L, 0.0)
    y, _, flag = _ato(f["qkv"], ops, L, amax)
    per = {"ato": A.sample_errors(y, y64, L)}
    assert flag == 0
    b = A.case("quiet_sample", L, R, "bwd")
    got = _atb(b["qkv"], b["dout"], L)
    for n, s in A.BLOCKS:
        per[f"atb {n}"] = A.sample_errors(got[:, s], b["dqkv"][:, s], L)
    a = _abl_case("quiet_sample", L, R)
    _, amax, _ = _abl(a, 0.0)
    got, _, flag = _abl(a, amax)
    assert flag == 0
    per["abl"] = A.sample_errors(got - a["add"].numpy(), a["dz"], L)
    for k, v in per.items():
        b0 = A.B0[k.split()[0]]
        print(f"quiet_sample L={L} R={R} {k}: " + " ".join(f"{e:.1e}" for e in v) + f"  (sample {qs} quiet; reaches the loud bar {b0:.0e}: {bool(v[qs] < b0)})")
    for k, v in per.items():
        assert np.delete(v, qs).max() < A.B0[k.split()[0]], (k, v)
        assert v[qs] < 2.0 ** -17, (k, v[qs])


# ---- the score network with sharp attention ----------------------------------------------------------------------------------------------
_NET = {}


def _sharp_network_reference():
    if not _NET:
        S, H = 4, 48
        g = np.load(f"{GOLDEN}/unet2d_h48.npz")
        sd = synth.sharpen_attention(weights(S, H, False), 6.0)
        x, cloud = g["x"], g["cloud"]
        u64, u32 = O.UNetOracle(sd, S, H, dtype=np.float64), O.UNetOracle(sd, S, H, dtype=np.float32)
        lat = np.tile(u64.encode_scene(cloud)[None], (x.shape[0], 1))
        lat[1::2] = 0                                              # odd rows unconditional (UnetInference.py:192-197)
        ref = {}
        for t in (3, 20):
            tt = np.full((x.shape[0],), t)
            f64, e64 = u64.forward_no_energy(x, tt, lat), u64.score(x, tt, lat)
            f32, e32 = u32.forward_no_energy(x, tt, lat), u32.score(x, tt, lat)
            ref[t] = (f64, e64, A.rel(f32, f64), A.rel(e32, e64))
        _NET.update(sd=sd, x=x, cloud=cloud, ref=ref)
    return _NET


@pytest.mark.parametrize("gemm_mode", ["fp16x3-tkw", "fp16x3", "bf16x6", "fp32"])
def test_score_network_with_sharp_attention(gemm_mode):
    """S = 4, H = 48, 4 rows, two timesteps, every attn1 query / key weight x 6 (synth.sharpen_attention: logits of standard deviation ~12,
    mean largest probability ~0.8 at the finest level -- the seeded weights keep every probability within 2 / L): f and eps (the energy
    gradient: the backward kernels) against the float64 oracle with the same weights, bars max(2e-5, 4 floor) and max(5e-5, 4 floor), floor =
    the float32 oracle against the float64 one.  "fp16x3-tkw" is the bench's plan (ato + abl), "fp16x3" the tile kernels.  As in
    test_score_with_outlier_channel_weights an fp16x3 plan may trip its range guard and return the bf16x6 answer; it may not return a
    silently degraded one."""
    from ramp_amd.models import TemporalUnetInference
    from ramp_amd.unet import load_numpy_state_dict
    n = _sharp_network_reference()
    base, plan = util.split_mode(gemm_mode) if "-" in gemm_mode else (gemm_mode, None)
    m = TemporalUnetInference(n_support_points=48, state_dim=4, max_rows=8, gemm_mode=base, launch_plan=plan)
    m = load_numpy_state_dict(m, n["sd"]).eval().to("cuda")
    x = dev(n["x"]); N = x.shape[0]
    pts = dev(n["cloud"])[None].repeat(N, 1, 1, 1)
    results = []
    for t, (f64, e64, ff, fe) in n["ref"].items():
        tt = torch.full((N,), t, dtype=torch.int64, device="cuda")
        modes = []
        for _ in range(3):
            eps = m(x, tt, None, obstacle_pts=pts).cpu().numpy()
            modes.append(m.score_mode())
        f = m.forward_no_energy(x, tt, obstacle_pts=pts).cpu().numpy()
        modes.append(m.score_mode())
        bf, be = A.bar(2e-5, ff), A.bar(5e-5, fe)
        print(f"sharp attention {gemm_mode} t={t}: evaluations ran as {modes}; f {A.rel(f, f64):.2e} (fp32 {ff:.1e}, bar {bf:.1e})  "
              f"eps {A.rel(eps, e64):.2e} (fp32 {fe:.1e}, bar {be:.1e})")
        results.append((t, A.rel(f, f64), bf, A.rel(eps, e64), be, modes))
    for t, ef, bf, ee, be, modes in results:
        assert ef < bf and ee < be, (t, ef, bf, ee, be)
        assert set(modes) <= ({"fp16x3", "bf16x6"} if base == "fp16x3" else {base}), modes
