"""edge_ref.py (the float64 statements behind test_gpu_edge_kernels.py) against independent routes -- torch.nn.functional.conv1d and
torch.autograd in float64 on the CPU, the float64 oracle's cross_attn_bias and cond_mlp line -- and the bar of the GPU test against
itself: on every case of the GPU test's tables a float32 numpy restatement with sequential sums lies inside the a-priori rounding bound
(the inputs are honest: a correct fp32 evaluation passes), a reference with one product dropped at a row's first waypoint lies outside
it (the bound separates)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_ref as E
from oracle import ramp_oracle as O
from util import weights

AGREE = 1e-12


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def ratio(got, ref, ab, n):
    """worst |got - ref| / (gamma_n abs companion); elements whose companion is 0 must be exact"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = E.gamma(n) * ab
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- float32 restatements with sequential sums (vectorised over the outputs, one float32 operation per step) ------------------------------
def conv_in_fwd32(x, W5, b5, W1, b1, n_rp):
    B, H, S = x.shape
    xp = np.pad(x, ((0, 0), (2, 2), (0, 0)))
    acc = np.zeros((B, H, W5.shape[0]), np.float32)
    for j in range(5):
        for s in range(S):
            acc = acc + xp[:, j:j + H, s, None] * W5[None, None, :, s, j]
    r = np.zeros_like(acc)
    for s in range(S):
        r = r + x[:, :, s, None] * W1[None, None, :, s, 0]
    return np.repeat(acc + b5, n_rp, axis=0), np.repeat(r + b1, n_rp, axis=0)


def conv_in_bwd32(dc1, dy, W5, W1):
    R, H, C0 = dc1.shape
    dp = np.pad(dc1, ((0, 0), (2, 2), (0, 0)))
    acc = np.zeros((R, H, W5.shape[1]), np.float32)
    for j in range(5):
        for c in range(C0):
            acc = acc + dp[:, 4 - j:4 - j + H, c, None] * W5[None, None, c, :, j]
    for c in range(C0):
        acc = acc + dy[:, :, c, None] * W1[None, None, c, :, 0]
    return acc


def conv_out32(a, Wf, bf):
    n, C0 = a.shape
    S = Wf.shape[0]
    f = np.zeros((n, S), np.float32)
    for c in range(C0):
        f = f + a[:, c, None] * Wf[None, :, c, 0]
    f = f + bf
    da = np.zeros((n, C0), np.float32)
    for s in range(S):
        da = da + f[:, s, None] * Wf[None, s, :, 0]
    return f, da


def combine32(x, w):
    n_rp = w.shape[-1]
    B = x.shape[0] // n_rp
    w = np.broadcast_to(w, (B, n_rp))
    xr = x.reshape(B, n_rp, *x.shape[1:])
    acc = xr[:, 0] * w[:, 0, None, None]
    for j in range(1, n_rp):
        acc = acc + xr[:, j] * w[:, j, None, None]
    return acc


def cross_bias32(lat, wv, wo, bo):
    out = []
    for v, o, b in zip(wv, wo, bo):
        tmp = np.zeros((lat.shape[0], 256), np.float32)
        for k in range(lat.shape[1]):
            tmp = tmp + lat[:, k, None] * v[None, :, k]
        acc = np.zeros_like(tmp)
        for k in range(256):
            acc = acc + tmp[:, k, None] * o[None, :, k]
        out.append(acc + b)
    return np.stack(out, axis=1)


# ---- the case tables cover what they claim ------------------------------------------------------------------------------------------------
def test_case_tables_cover_every_value_and_pair():
    cs = E.conv_in_cases()
    for key, vals in (("C0", E.CONV_C0), ("S", E.CONV_IN_S), ("H", E.CONV_IN_H), ("B", E.CONV_IN_B), ("n_rp", E.CONV_IN_NRP), ("regime", E.REGIMES)):
        assert {c[key] for c in cs} == set(vals), key
    for a, b in (("C0", "regime"), ("S", "regime"), ("H", "regime"), ("C0", "n_rp"), ("H", "n_rp"), ("S", "n_rp"), ("H", "B"), ("S", "B")):
        seen = {(c[a], c[b]) for c in cs}
        assert len(seen) == len({c[a] for c in cs}) * len({c[b] for c in cs}), (a, b)
    assert {c["B"] for c in cs if c["n_rp"] == 1} == set(E.CONV_IN_B)               # R in {1, 3, 7} backward
    assert any(c["H"] * c["S"] == 256 for c in cs) and any(c["H"] * c["C0"] < 256 for c in cs)
    assert any(c["H"] * c["C0"] > 256 and c["H"] * c["C0"] % 256 for c in cs) and any(c["H"] * c["S"] > 256 and c["H"] * c["S"] % 256 for c in cs)
    assert any((c["H"], c["S"], c["C0"]) == (64, 16, 64) for c in cs)
    co = E.conv_out_cases()
    assert {(c["C0"], c["S"], c["n_tok"]) for c in co} == {(a, b, c) for a in E.CONV_C0 for b in E.CONV_OUT_S for c in E.CONV_OUT_NTOK}
    assert {(c["C0"], c["regime"]) for c in co} == {(a, b) for a in E.CONV_C0 for b in E.REGIMES}
    ex = E.expand_cases()
    assert {(c["n_rp"], c["L"], c["bias"]) for c in ex} >= {(a, b, c) for a in (1, 2, 3, 8) for b in (1, 3, 48) for c in (False, True)}
    assert any(c["B"] * c["n_rp"] * c["L"] * c["C"] // 4 > E.GRID_ROUND for c in ex)
    cb = E.combine_cases()
    assert {(c["weighted"], c["n_rp"]) for c in cb} == {(False, 1), (False, 2), (False, 3), (True, 2), (True, 5), (True, 8)}
    for wtd in (False, True):
        assert any(c["weighted"] == wtd and c["B"] * c["L"] * c["C"] // 4 > E.GRID_ROUND for c in cb)
    xb = E.cross_bias_cases()
    assert {(c["ctx_dim"], c["n_var"], c["n_blk"]) for c in xb} == {(a, b, c) for a in (1, 31, 32, 512) for b in (1, 4, 9) for c in (1, 2, 12)}


# ---- conv_in ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0", E.CONV_C0)
def test_conv_in_reference_bar_and_adjoint(C0):
    worst32 = {"c1": 0.0, "res": 0.0, "eps": 0.0}
    for c in (c for c in E.conv_in_cases() if c["C0"] == C0):
        o = E.conv_in_operands(c)
        n_rp, S = c["n_rp"], c["S"]
        c1, res, c1a, resa = E.conv_in_fwd(o["x"], o["W5"], o["b5"], o["W1"], o["b1"], n_rp)
        eps, epsa = E.conv_in_bwd(o["dc1"], o["dy"], o["W5"], o["W1"])
        # torch float64: the forward by conv1d, the input gradient by autograd
        x = t64(o["x"]).requires_grad_(True)
        xr = x.repeat_interleave(n_rp, dim=0).transpose(1, 2)
        tc1 = F.conv1d(xr, t64(o["W5"]), t64(o["b5"]), padding=2).transpose(1, 2)
        tres = F.conv1d(xr, t64(o["W1"]), t64(o["b1"])).transpose(1, 2)
        assert rel(c1, tc1.detach().numpy()) < AGREE and rel(res, tres.detach().numpy()) < AGREE, c
        xrow = t64(np.repeat(o["x"], n_rp, axis=0)).requires_grad_(True)      # per network row, as the kernel computes it
        y5 = F.conv1d(xrow.transpose(1, 2), t64(o["W5"]), t64(o["b5"]), padding=2).transpose(1, 2)
        y1 = F.conv1d(xrow.transpose(1, 2), t64(o["W1"]), t64(o["b1"])).transpose(1, 2)
        ((y5 * t64(o["dc1"])).sum() + (y1 * t64(o["dy"])).sum()).backward()
        assert rel(eps, xrow.grad.numpy()) < AGREE, c
        # the companions are the same formulas on |operands|
        ab = {k: np.abs(v) for k, v in o.items()}
        c1b, resb, _, _ = E.conv_in_fwd(ab["x"], ab["W5"], ab["b5"], ab["W1"], ab["b1"], n_rp)
        epsb, _ = E.conv_in_bwd(ab["dc1"], ab["dy"], ab["W5"], ab["W1"])
        assert np.array_equal(c1a, c1b) and np.array_equal(resa, resb) and np.array_equal(epsa, epsb)
        # eps is the adjoint of the forward's linear part: <conv_in(x) - bias, d> == <x, eps(d)>
        lhs = ((c1 - o["b5"].astype(np.float64)) * o["dc1"]).sum() + ((res - o["b1"].astype(np.float64)) * o["dy"]).sum()
        rhs = (np.repeat(o["x"].astype(np.float64), n_rp, axis=0) * eps).sum()
        scale = (c1a * np.abs(o["dc1"])).sum() + (resa * np.abs(o["dy"])).sum()
        assert abs(lhs - rhs) <= AGREE * scale, (c, lhs, rhs)
        # the bar: a float32 evaluation with sequential sums lies inside it ...
        g1, gr = conv_in_fwd32(o["x"], o["W5"], o["b5"], o["W1"], o["b1"], n_rp)
        ge = conv_in_bwd32(o["dc1"], o["dy"], o["W5"], o["W1"])
        r = dict(c1=ratio(g1, c1, c1a, E.n_conv_in_fwd(S)), res=ratio(gr, res, resa, E.n_conv_in_fwd(S)), eps=ratio(ge, eps, epsa, E.n_conv_in_bwd(C0)))
        assert max(r.values()) <= 1.0, (c, r)
        worst32 = {k: max(worst32[k], v) for k, v in r.items()}
        # ... and a reference with the centre tap's first product dropped at a row's first waypoint lies outside it
        # (the product of the waypoint's largest operand, so that one Gaussian factor's chance smallness does not decide)
        xr0 = np.repeat(o["x"][:, 0].astype(np.float64), n_rp, axis=0)          # (R, S)
        k = np.abs(xr0).argmax(axis=1)
        bad = c1.copy(); bad[:, 0, :] -= xr0[np.arange(len(k)), k, None] * o["W5"][:, k, 2].T.astype(np.float64)
        assert ratio(bad, c1, c1a, E.n_conv_in_fwd(S)) > 1.0, c
        d0 = o["dc1"][:, 0].astype(np.float64)                                 # (R, C0)
        k = np.abs(d0).argmax(axis=1)
        bad = eps.copy(); bad[:, 0, :] -= d0[np.arange(len(k)), k, None] * o["W5"][k, :, 2].astype(np.float64)
        assert ratio(bad, eps, epsa, E.n_conv_in_bwd(C0)) > 1.0, c
    print(f"conv_in C0={C0}: float32 restatement's worst share of the bound {worst32}")


# ---- conv_out -----------------------------------------------------------------------------------------------------------------------------
def test_conv_out_reference_and_bar():
    worst = {"f": 0.0, "da": 0.0}
    for c in E.conv_out_cases():
        o = E.conv_out_operands(c)
        f, da, fa, daa = E.conv_out(o["a"], o["Wf"], o["bf"])
        a = t64(o["a"]).requires_grad_(True)
        tf = F.conv1d(a.t()[None], t64(o["Wf"]), t64(o["bf"]))[0].t()           # (n_tok, S)
        (0.5 * (tf ** 2).sum()).backward()                                      # E = 0.5 sum f^2  =>  dE/da = f Wf
        assert rel(f, tf.detach().numpy()) < AGREE and rel(da, a.grad.numpy()) < AGREE, c
        fb, _, _, _ = E.conv_out(np.abs(o["a"]), np.abs(o["Wf"]), np.abs(o["bf"]))
        assert np.array_equal(fa, fb) and np.array_equal(daa, fa @ np.abs(o["Wf"][:, :, 0].astype(np.float64)))
        gf, gda = conv_out32(o["a"], o["Wf"], o["bf"])
        r = dict(f=ratio(gf, f, fa, E.n_conv_out_f(c["C0"])), da=ratio(gda, da, daa, E.n_conv_out_da(c["C0"], c["S"])))
        assert max(r.values()) <= 1.0, (c, r)
        worst = {k: max(worst[k], v) for k, v in r.items()}
        bad = f.copy(); bad[0, 0] -= np.float64(o["a"][0, 0]) * np.float64(o["Wf"][0, 0, 0])
        assert ratio(bad, f, fa, E.n_conv_out_f(c["C0"])) > 1.0, c
        assert ratio(bad @ o["Wf"][:, :, 0].astype(np.float64), da, daa, E.n_conv_out_da(c["C0"], c["S"])) > 1.0, c
    print(f"conv_out: float32 restatement's worst share of the bound {worst}")


# ---- expand / combine -----------------------------------------------------------------------------------------------------------------------
def test_expand_rows_reference_by_loops():
    for c in E.expand_cases():
        if c["B"] > 7:
            continue
        o = E.expand_operands(c)
        out = E.expand_rows(o["x"], c["n_rp"], E.expand_slice(o, c), o.get("rowvar"), c["row0"])
        assert out.dtype == np.float32 and out.shape == (c["B"] * c["n_rp"], c["L"], c["C"])
        for r in range(out.shape[0]):
            for l in range(c["L"]):
                want = o["x"][r // c["n_rp"], l]
                if c["bias"]:
                    want = want + o["rowbias"][o["rowvar"][c["row0"] + r], E.EXPAND_OFF:E.EXPAND_OFF + c["C"]]
                assert np.array_equal(out[r, l], want), (c, r, l)


def test_combine_rows_reference_and_bar():
    worst = 0.0
    for c in E.combine_cases():
        o = E.combine_operands(c)
        out, outa = E.combine_rows(o["x"], o["w"])
        n_rp, B = c["n_rp"], c["B"]
        if B <= 7:
            w = np.broadcast_to(o["w"].astype(np.float64), (B, n_rp))
            for b in range(B):
                want = sum(w[b, j] * o["x"][b * n_rp + j].astype(np.float64) for j in range(n_rp))
                assert rel(out[b], want) < AGREE, (c, b)
        r = ratio(combine32(o["x"], o["w"]), out, outa, E.n_combine(n_rp))
        assert r <= 1.0, (c, r)
        worst = max(worst, r)
        bad = out.copy(); bad[:, 0] -= np.broadcast_to(o["w"].astype(np.float64), (B, n_rp))[:, 0, None] * o["x"][::n_rp, 0].astype(np.float64)
        assert ratio(bad, out, outa, E.n_combine(n_rp)) > 1.0, c
    print(f"combine: float32 restatement's worst share of the bound {worst:.3f}")


# ---- cross_bias ---------------------------------------------------------------------------------------------------------------------------
def test_cross_bias_reference_and_bar():
    worst = 0.0
    for c in E.cross_bias_cases():
        o = E.cross_bias_operands(c)
        out, outa = E.cross_bias(o["lat"], o["wv"], o["wo"], o["bo"])
        sd = {}
        for k in range(c["n_blk"]):
            t = f"st.transformer_blocks.{k}.attn2"
            sd[f"{t}.to_v.weight"], sd[f"{t}.to_out.0.weight"], sd[f"{t}.to_out.0.bias"] = o["wv"][k], o["wo"][k], o["bo"][k]
        uo = O.UNetOracle(sd, 4, 48, dtype=np.float64)
        for k in range(c["n_blk"]):
            assert rel(out[:, k], uo.cross_attn_bias("st", k, o["lat"].astype(np.float64))) < AGREE, (c, k)
        r = ratio(cross_bias32(o["lat"], o["wv"], o["wo"], o["bo"]), out, outa, E.n_cross_bias(c["ctx_dim"]))
        assert r <= 1.0, (c, r)
        worst = max(worst, r)
        bad = out.copy(); bad[:, 0, :] -= (o["lat"][:, 0, None].astype(np.float64) *o["wv"][0][None, :, 0].astype(np.float64)) @ o["wo"][0].T.astype(np.float64)
        assert ratio(bad, out, outa, E.n_cross_bias(c["ctx_dim"])) > 1.0, c
    print(f"cross_bias: float32 restatement's worst share of the bound {worst:.3f}")


# ---- the time table's lines -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H,o3", E.TIME_NETS)
def test_time_lines_reference_and_bars(S, H, o3):
    sd = weights(S, H, o3)
    uo = O.UNetOracle(sd, S, H, obstacle_3d=o3, dtype=np.float64)
    temb = uo.time_embedding(np.arange(E.TIME_T))
    names = E.rtb_names(sd)
    assert len(names) == 16 and "downs.0.0" in names and "mid_block1" in names
    for name in names:
        W, b = uo.p[name + ".cond_mlp.1.weight"], uo.p[name + ".cond_mlp.1.bias"]
        assert rel(E.cond_line(temb, W, b), O.silu(temb) @ W.T + b) < AGREE, name
    bars = E.time_line_bars(sd, temb)
    for name, (bar, e) in bars.items():
        assert np.isfinite(e) and bar >= E.TIME_BAR and (bar == E.TIME_BAR or bar == 4.0 * e), (name, bar, e)
        assert e < bar
    print(f"time lines ({S}, {H}): restatement's worst rel {max(e for _, e in bars.values()):.2e}; raised bars "
          f"{ {n: b for n, (b, e) in bars.items() if b != E.TIME_BAR} }")
