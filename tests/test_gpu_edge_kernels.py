"""The plain-C++ kernels at the two ends of the score network and where the shared prefix fans out (rowops.hip: conv_in forward /
backward, conv_out, expand_rows, combine_rows(_weighted), cross_bias, the time table's per-block lines), one launch at a time through
the tools library's ramp_probe_* entries, against the float64 statements of tests/edge_ref.py (checked on the CPU by
tests/test_edge_ref_host.py, which also shows that a float32 evaluation of every case below lies inside the bar and a dropped product
outside it).

The bar.  The kernels are fp32 sums whose order and FMA contraction are the compiler's, so the bar is the a-priori rounding bound,
elementwise: |got - ref64| <= gamma_N abs_companion, gamma_N = N u / (1 - N u), u = 2^-24, N per kernel as edge_ref.n_* state it
(conv_in forward 5 S + 1, backward 6 C0 + 1, conv_out f C0 + 1, da C0 + 1 + S, cross_bias ctx_dim + 257, combine 2 n_rp).  It holds for
any correct fp32 evaluation; nothing about it is measured.  expand_rows is a copy or one float32 addition and is compared bit for bit.
The time table's lines pass through expf / sinf / Mish, so they are held to the project's bar for temb (5e-6, util.rel per block slice
and timestep), raised per block by edge_ref.time_line_bars only where a float32 restatement itself comes within 2x of it.

Every output starts as a sentinel and carries a guard tail of one extra row: what the operation does not own keeps the sentinel bit for
bit.  The worst error-to-bound ratio and the worst util.rel per kernel are printed; with RAMP_ACCURACY_LOG set the same lines are
appended to that file (profiles/edge_kernels_accuracy.txt is one such run) -- observations for the next rewrite, not bars."""
import os

import numpy as np
import pytest
import torch

import edge_ref as E
from oracle import ramp_oracle as O
from ramp_amd import _lib
from util import build_unet, dev, rel, weights

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.125e29)


def sentinel(rows, row_elems):
    """(rows + 1) x row_elems floats of sentinel: the last row is the guard tail"""
    return torch.full(((rows + 1) * row_elems,), float(SENTINEL), device="cuda")


def is_sentinel(a):
    a = np.ascontiguousarray(a)
    return bool((a.view(np.uint32) == SENTINEL.view(np.uint32)).all())


def owned(buf, rows, row_elems, shape):
    """the operation's part of a sentinel buffer as a host array; the guard tail must be untouched"""
    h = buf.cpu().numpy()
    assert is_sentinel(h[rows * row_elems:]), "guard tail written"
    return h[:rows * row_elems].reshape(shape)


POISON = np.float32(3.0e6)


def shared_rows(x, rows):
    """x (B, ...) on the device, followed by poison up to `rows` rows: a kernel that gives network row r trajectory r instead of
    r // n_rp reads a wrong finite value, inside the allocation"""
    pad = np.full((rows - x.shape[0],) + x.shape[1:], POISON, np.float32)
    return dev(np.concatenate([x, pad], axis=0))


def log(line):
    print(line)
    path = os.environ.get("RAMP_ACCURACY_LOG")
    if path:
        with open(path, "a", encoding="utf-8") as fh:
            fh.write(line + "\n")


class Worst:
    """worst error-to-bound ratio and worst util.rel of one kernel output over a test's cases"""

    def __init__(self, what):
        self.what, self.ratio, self.rel, self.at = what, 0.0, 0.0, None

    def check(self, got, ref, ab, n, label):
        err = np.abs(got.astype(np.float64) - ref)
        bound = E.gamma(n) * ab
        pos = bound > 0
        r = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
        if r > self.ratio:
            self.ratio, self.at = r, label
        self.rel = max(self.rel, rel(got, ref))
        assert np.isfinite(got).all(), (self.what, label)
        assert (err <= bound).all(), (self.what, label, f"worst error / bound {r:.3f}")

    def report(self):
        log(f"{self.what:34s} worst error/bound {self.ratio:.3f}  worst rel {self.rel:.3e}  ({self.at})")


# ---- conv_in ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0", E.CONV_C0)
def test_conv_in_forward_and_backward(C0):
    """Forward (c1, res) and backward (eps) on the same float64 weights, every case of edge_ref.conv_in_cases at this C0; eps is also the
    adjoint of the forward as the kernels compute them: <conv_in(x) - bias, d> == <x, eps(d)> within what the two bounds allow."""
    wc1, wres, weps = Worst(f"conv_in_fwd<{C0}> c1"), Worst(f"conv_in_fwd<{C0}> res"), Worst(f"conv_in_bwd<{C0}> eps")
    for c in (c for c in E.conv_in_cases() if c["C0"] == C0):
        o = E.conv_in_operands(c)
        S, H, n_rp, R = c["S"], c["H"], c["n_rp"], c["B"] * c["n_rp"]
        W5, W1 = dev(E.pack_w5(o["W5"])), dev(E.pack_w1(o["W1"]))
        c1b, resb, epsb = sentinel(R, H * C0), sentinel(R, H * C0), sentinel(R, H * S)
        rc, msg = _lib.probe_conv_in_fwd(shared_rows(o["x"], R), W5, dev(o["b5"]), W1, dev(o["b1"]), c1b, resb, R, n_rp, H, S, C0)
        assert rc == 0, (c, msg)
        rc, msg = _lib.probe_conv_in_bwd(dev(o["dc1"]), dev(o["dy"]), W5, W1, epsb, R, H, S, C0)
        assert rc == 0, (c, msg)
        c1, res, eps = owned(c1b, R, H * C0, (R, H, C0)), owned(resb, R, H * C0, (R, H, C0)), owned(epsb, R, H * S, (R, H, S))
        rc1, rres, c1a, resa = E.conv_in_fwd(o["x"], o["W5"], o["b5"], o["W1"], o["b1"], n_rp)
        reps, epsa = E.conv_in_bwd(o["dc1"], o["dy"], o["W5"], o["W1"])
        wc1.check(c1, rc1, c1a, E.n_conv_in_fwd(S), c)
        wres.check(res, rres, resa, E.n_conv_in_fwd(S), c)
        weps.check(eps, reps, epsa, E.n_conv_in_bwd(C0), c)
        d1, d2, xr = o["dc1"].astype(np.float64), o["dy"].astype(np.float64), np.repeat(o["x"].astype(np.float64), n_rp, axis=0)
        lhs = ((c1.astype(np.float64) - o["b5"]) * d1).sum() + ((res.astype(np.float64) - o["b1"]) * d2).sum()
        rhs = (xr * eps.astype(np.float64)).sum()
        slack = (E.gamma(E.n_conv_in_fwd(S)) * (c1a * np.abs(d1) + resa * np.abs(d2))).sum() + (E.gamma(E.n_conv_in_bwd(C0)) * epsa * np.abs(xr)).sum()
        assert abs(lhs - rhs) <= slack, (c, lhs, rhs, slack)
    for w in (wc1, wres, weps):
        w.report()


# ---- conv_out -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C0", E.CONV_C0)
def test_conv_out_three_forms(C0):
    """f and da, f only, da only: da alone has the bits it has when f is stored too, and an output not asked for is not written."""
    wf, wda = Worst(f"conv_out<{C0}> f"), Worst(f"conv_out<{C0}> da")
    for c in (c for c in E.conv_out_cases() if c["C0"] == C0):
        o = E.conv_out_operands(c)
        n, S = c["n_tok"], c["S"]
        a, Wf, bf = dev(o["a"]), dev(E.pack_wf(o["Wf"])), dev(o["bf"])
        rf, rda, fa, daa = E.conv_out(o["a"], o["Wf"], o["bf"])
        got = {}
        for form in ("both", "f", "da"):
            fb, dab = sentinel(n, S), sentinel(n, C0)
            rc, msg = _lib.probe_conv_out(a, Wf, bf, fb if form != "da" else None, dab if form != "f" else None, n, S, C0)
            assert rc == 0, (c, form, msg)
            if form == "da":
                assert is_sentinel(fb.cpu().numpy()), (c, "f written by the da-only form")
            else:
                got[form, "f"] = owned(fb, n, S, (n, S))
                wf.check(got[form, "f"], rf, fa, E.n_conv_out_f(C0), (c, form))
            if form == "f":
                assert is_sentinel(dab.cpu().numpy()), (c, "da written by the f-only form")
            else:
                got[form, "da"] = owned(dab, n, C0, (n, C0))
                wda.check(got[form, "da"], rda, daa, E.n_conv_out_da(C0, S), (c, form))
        assert np.array_equal(got["da", "da"].view(np.uint32), got["both", "da"].view(np.uint32)), (c, "da alone differs from da with f")
        assert np.array_equal(got["f", "f"].view(np.uint32), got["both", "f"].view(np.uint32)), (c, "f alone differs from f with da")
    wf.report(); wda.report()


# ---- expand_rows ----------------------------------------------------------------------------------------------------------------------------
def test_expand_rows_bit_for_bit():
    """A copy without the row constant, one float32 addition with it: n_rp 1 / 2 / 3 / 8, L 1 / 3 / 48 (w % c4 wraps), a constant table of
    9 variants whose lines are longer than C, entered at its block's offset and at row0 = 5 of a longer row -> variant table; one case
    just above one round of the grid."""
    n = 0
    for c in E.expand_cases():
        o = E.expand_operands(c)
        R, L, C = c["B"] * c["n_rp"], c["L"], c["C"]
        outb = sentinel(R, L * C)
        x = shared_rows(o["x"], R)
        if c["bias"]:       # (poison behind the table, a row long: an index that does not wrap at C stays inside the allocation)
            rb = dev(np.concatenate([o["rowbias"].ravel(), np.full(L * C, POISON, np.float32)]))
            rc, msg = _lib.probe_expand_rows(x, outb, R, c["n_rp"], L, C, rb[E.EXPAND_OFF:], E.EXPAND_STRIDE, dev(o["rowvar"]), c["row0"])
        else:
            rc, msg = _lib.probe_expand_rows(x, outb, R, c["n_rp"], L, C)
        assert rc == 0, (c, msg)
        want = E.expand_rows(o["x"], c["n_rp"], E.expand_slice(o, c), o.get("rowvar"), c["row0"])
        assert np.array_equal(owned(outb, R, L * C, (R, L, C)).view(np.uint32), want.view(np.uint32)), c
        n += 1
    log(f"{'expand_rows':34s} {n} cases bit for bit")


# ---- combine_rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_combine_rows(weighted):
    """Host weights at n_rp 1 / 2 / 3; per-row device weights at n_rp 2 / 5 / 8 through a pointer offset by the chunk's first trajectory,
    as combine_prefix passes it; one case each just above one round of the grid."""
    w_ = Worst("combine_rows_weighted" if weighted else "combine_rows")
    for c in (c for c in E.combine_cases() if c["weighted"] == weighted):
        o = E.combine_operands(c)
        B, n_rp, L, C = c["B"], c["n_rp"], c["L"], c["C"]
        outb = sentinel(B, L * C)
        if weighted:
            rc, msg = _lib.probe_combine_rows_weighted(dev(o["x"]), outb, B, n_rp, L, C, dev(o["w_all"]), E.COMBINE_B0 * n_rp)
        else:
            rc, msg = _lib.probe_combine_rows(dev(o["x"]), outb, B, n_rp, L, C, o["w"])
        assert rc == 0, (c, msg)
        ref, ab = E.combine_rows(o["x"], o["w"])
        w_.check(owned(outb, B, L * C, (B, L, C)), ref, ab, E.n_combine(n_rp), c)
    w_.report()


# ---- cross_bias -----------------------------------------------------------------------------------------------------------------------------
def test_cross_bias():
    w_ = Worst("cross_bias")
    for c in E.cross_bias_cases():
        o = E.cross_bias_operands(c)
        nv, nb = c["n_var"], c["n_blk"]
        outb = sentinel(nv, nb * 256)
        rc, msg = _lib.probe_cross_bias(dev(o["lat"]), nv, c["ctx_dim"], [dev(w) for w in o["wv"]], [dev(w) for w in o["wo"]],
                                        [dev(b) for b in o["bo"]], outb)
        assert rc == 0, (c, msg)
        ref, ab = E.cross_bias(o["lat"], o["wv"], o["wo"], o["bo"])
        w_.check(owned(outb, nv, nb * 256, (nv, nb, 256)), ref, ab, E.n_cross_bias(c["ctx_dim"]), c)
    w_.report()


# ---- the time table's per-block lines -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,H,o3", E.TIME_NETS)
def test_time_table_lines_of_every_block(S, H, o3):
    """The cond_mlp line every residual block adds behind its Mish, for every t of a 100-step table, per block slice against the float64
    oracle; an unknown block, a t outside the table and a wrong length are refused and write nothing."""
    sd = weights(S, H, o3)
    m = build_unet(S, H, o3, max_rows=4)
    m.prepare_time_table(E.TIME_T)
    uo = O.UNetOracle(sd, S, H, obstacle_3d=o3, dtype=np.float64)
    temb = uo.time_embedding(np.arange(E.TIME_T))
    bars = E.time_line_bars(sd, temb)
    worst, worst_at = 0.0, None
    for name in E.rtb_names(sd):
        W, b = uo.p[name + ".cond_mlp.1.weight"], uo.p[name + ".cond_mlp.1.bias"]
        ref = O.silu(temb) @ W.T + b
        cout = W.shape[0]
        buf = sentinel(E.TIME_T, cout)
        for t in range(E.TIME_T):
            rc, msg = _lib.probe_time_bias(m.ctx(), name, t, buf[t * cout:(t + 1) * cout])
            assert rc == 0, (name, t, msg)
        got = owned(buf, E.TIME_T, cout, (E.TIME_T, cout))
        for t in range(E.TIME_T):
            err = rel(got[t], ref[t])
            if err / bars[name][0] > worst:
                worst, worst_at = err / bars[name][0], (name, t, err)
            assert err < bars[name][0], (name, t, err, bars[name])
    raised = {n: f"{b:.2e}" for n, (b, e) in bars.items() if b != E.TIME_BAR}
    log(f"{f'time_table lines ({S}, {H})':34s} worst rel {worst_at[2]:.3e} = {worst:.3f} of its bar at {worst_at[:2]}; bars raised above {E.TIME_BAR:.0e}: {raised or 'none'}")
    out = sentinel(1, 512)
    for args, want in ((("no.such.block", 0, out[:32]), "no residual block"), (("downs.0.0", E.TIME_T, out[:32]), "outside the prepared time table"),
                       (("downs.0.0", -1, out[:32]), "outside the prepared time table"), (("downs.0.0", 0, out[:33]), "output channels")):
        rc, msg = _lib.probe_time_bias(m.ctx(), *args)
        assert rc != 0 and want in msg, (args[:2], rc, msg)
    assert is_sentinel(out.cpu().numpy())


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _small(shape, seed=3):
    return dev(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def test_refusals_write_nothing():
    """What the launchers refuse is refused through the probes with ramp_last_error set, and every output is still sentinel."""
    def refused(call, outs, want):
        rc, msg = call()
        assert rc != 0 and msg and want in msg, (want, rc, msg)
        for o in outs:
            assert is_sentinel(o.cpu().numpy()), want
    H = 5
    for S, C0, want in ((17, 32, "bad conv_in dims"), (4, 48, "C0 in {16, 32, 64}")):      # S = 17; C0 = 48
        x, W5, W1, b = _small((2, H, S)), _small((5, S, C0)), _small((S, C0)), _small((C0,))
        c1, res, eps = sentinel(2, H * C0), sentinel(2, H * C0), sentinel(2, H * S)
        refused(lambda: _lib.probe_conv_in_fwd(x, W5, b, W1, b, c1, res, 2, 1, H, S, C0), (c1, res), want)
        refused(lambda: _lib.probe_conv_in_bwd(_small((2, H, C0)), _small((2, H, C0)), W5, W1, eps, 2, H, S, C0), (eps,), want)
        a, Wf, bf = _small((7, C0)), _small((S, C0)), _small((S,))
        f, da = sentinel(7, S), sentinel(7, C0)
        refused(lambda: _lib.probe_conv_out(a, Wf, bf, f, da, 7, S, C0), (f, da), "bad conv_out dims" if S == 17 else "C0 in {16, 32, 64}")
    a, Wf, bf, f, da = _small((7, 32)), _small((4, 32)), _small((4,)), sentinel(7, 4), sentinel(7, 32)
    refused(lambda: _lib.probe_conv_out(a, Wf, bf, f, da, 0, 4, 32), (f, da), "bad conv_out dims")                       # n_tok = 0
    x, out = _small((4, 3, 32)), sentinel(8, 3 * 32)
    refused(lambda: _lib.probe_expand_rows(x, out, 7, 2, 3, 32), (out,), "bad expand_rows arguments")                    # R % n_rp != 0
    x6 = _small((4, 3, 6))
    refused(lambda: _lib.probe_expand_rows(x6, out, 8, 2, 3, 6), (out,), "bad expand_rows arguments")                    # C % 4 != 0
    rb = _small((9, 256))
    refused(lambda: _lib.probe_expand_rows(x, out, 8, 2, 3, 32, rb, 256, None, 0), (out,), "bad expand_rows arguments")  # a row constant without rowvar
    xin, o2 = _small((18, 3, 32)), sentinel(2, 3 * 32)
    refused(lambda: _lib.probe_combine_rows(xin, o2, 2, 4, 3, 32, [1.0, 2.0, 3.0, 4.0]), (o2,), "bad combine_rows arguments")       # n_rp = 4
    refused(lambda: _lib.probe_combine_rows(_small((4, 3, 6)), o2, 2, 2, 3, 6, [1.0, 2.0]), (o2,), "bad combine_rows arguments")    # C % 4 != 0
    rw = _small((2, 9))
    for n_rp in (1, 9):                                                                                                              # weighted: n_rp 1 and 9
        refused(lambda: _lib.probe_combine_rows_weighted(xin, o2, 2, n_rp, 3, 32, rw), (o2,), "bad combine_rows_weighted arguments")
    lat, wv, wo, bo, ob = _small((2, 513)), _small((256, 513)), _small((256, 256)), _small((256,)), sentinel(2, 256)
    refused(lambda: _lib.probe_cross_bias(lat, 2, 513, [wv], [wo], [bo], ob), (ob,), "bad cross-bias dims")              # ctx_dim = 513
