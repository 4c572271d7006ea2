"""The fused token- and sample-owning kernels (ffx.hip / ffx16.hip, tkl.hip / tkl16.hip / tklb_kernel, tkw.hip / tkc.hip) and the
stand-alone LayerNorm / GEGLU kernels, through their ramp_op_* entry points, on offset, flat, constant, spiked, quiet and loud rows and
samples: the regimes of fused_ref.py (test_fused_ref_host.py proves them on the CPU) against float64, tensor-wide AND per row / sample,
with bars max(b0, 4 x the float32 evaluation's error on the same case in the same metric).

The contract of the delayed operand scale, asserted in every run (`_contract`): from the float64 operand's row maxima and the maximum
the launch was given, core.h's guard MUST raise the flag, must NEVER raise it, or may do EITHER (fused_ref.guard_state); whenever the
flag stays down every output meets its bar -- "the flag is raised or the result is as accurate as with a fresh scale".
Regimes that leave the guard's window by themselves, all in the unscaled run (prev = 0, scale 1):
  tkl N = 256 / 96 on `quiet` rows (max |X| ~ 5e-3) and `flat` rows (0.02): the whole operand lies below 2^-3 -> the flag must be up;
  ffx on `const` rows: every row has the same a gelu(g), its maximum below 2^-3 -> must (the LayerNorm output, beta, is inside);
  `mixed` rows / samples, `quiet_*`, the GroupNorm-backward operand with `flat` samples (rstd = eps^-1/2 makes them 300 x the others):
  some waves' rows all lie below the window -> either.
The narrow convolutions (tkc.hip) have no guard in the unscaled run: every wave tile is scaled from its own maximum (tkc.hip:97-100).

Quiet rows and samples (2^-10 of the operand's largest rows, in `quiet_sample`, `quiet_*` and `mixed` alike) get the documented bound of
one scale per tensor instead of the bar: error relative to the row's own maximum < 2^-17 (fused_ref.QUIET_BOUND, the bound of
test_abl_per_sample_accuracy_under_a_magnitude_spread), in the unscaled and in the scaled run, whatever the kernel measures."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_ref as R
from ramp_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).cuda()      # (a copy: the shared case arrays are read-only)


def P(t):
    return _lib.ptr(t) if t is not None else None


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def _rows(got, c, name, b0, n_rows=None, quiet=None):
    """[(label, measured, floor, bar)] of one output: tensor-wide and per row; quiet rows (a mask) against QUIET_BOUND instead."""
    ref, (f_all, f_rows) = c["ref"][name], c["floor"][name]
    per = R.row_errors(got, ref, n_rows, c.get("scale", {}).get(name))
    if quiet is not None and quiet.any():          # (tensor-wide over the other rows: the quiet ones have their own, wider bound)
        n = len(quiet)
        g2, r2 = np.asarray(got).reshape(n, -1)[~quiet], np.asarray(ref).reshape(n, -1)[~quiet]
        return [(name + "/others", R.rel(g2, r2), f_all, R.bar(b0, f_all)), (name + "/other rows", float(per[~quiet].max()), f_rows, R.bar(b0, f_rows)),
                (name + "/quiet rows", float(per[quiet].max()), f_rows, R.QUIET_BOUND)]
    return [(name, R.rel(got, ref), f_all, R.bar(b0, f_all)), (name + "/rows", float(per.max()), f_rows, R.bar(b0, f_rows))]


def _contract(what, c, prevs, flag, rows, finite, guard=True):
    """Print everything, then: finite outputs; the flag as guard_state demands; the bars whenever the flag is down."""
    states = [R.guard_state(rm, p) for rm, p in zip(c["sites"], prevs)] if guard else ["never"]
    state = "must" if "must" in states else ("either" if "either" in states else "never")
    print(f"{what} {c['regime']} prev={['%.3g' % p for p in prevs]}: flag {flag} (guard: {state})  "
          + "  ".join(f"{n} {e:.2e} (fp32 {f:.1e}, bar {b:.1e})" for n, e, f, b in rows))
    assert finite, what
    if state == "must":
        assert flag != 0, (what, "the operand leaves the window: the flag must be raised", states)
        return
    if state == "never":
        assert flag == 0, (what, flag, states)
    if flag == 0:
        for n, e, f, b in rows:
            assert e < b, (what, c["regime"], n, e, f, b)


def _maxima(what, rec, c, ops, tol):
    """The recorded maxima are the float64 operands' (tolerance: the existing tests', or 4 x the float32 evaluation's error on that operand)."""
    for r, (name, t) in zip(rec, zip(ops, tol)):
        m64 = np.abs(c["ref"][name]).max() if isinstance(name, str) else name
        f32 = R.rel(c["ref32"][name], c["ref"][name]) if isinstance(name, str) else 0.0
        assert abs(r - m64) <= R.bar(t, f32) * m64, (what, name, r, m64)


# ---- ffx / ffx16 ------------------------------------------------------------------------------------------------------------------------
_DEV = {}


def _ffx_dev(c):
    key = ("ffx", c["regime"], c["M"])
    if key not in _DEV:
        _DEV.clear()                                             # (one case's tensors at a time)
        p = c["p"]
        _DEV[key] = [dev(a) for a in (c["z1"], c["dz"], p["W1"], p["b1"], p["W2"], p["b2"], p["g"], p["b"])]
    return _DEV[key]


def _ffx(entry, c, prev, d=None):
    d = d or _ffx_dev(c)
    M = c["M"]
    z2, dz1 = nans(M, 256), nans(M, 256)
    out, flag = (C.c_float * 4)(), C.c_int32(0)
    _lib.check(getattr(_lib.load(), entry)(*[P(t) for t in d], M, (C.c_float * 4)(*prev), P(z2), P(dz1), out, C.byref(flag), None), entry)
    return z2.cpu().numpy(), dz1.cpu().numpy(), list(out), flag.value


def _ffx_rows(c, z2, dz1):
    q = c["quiet"] if c["quiet"].any() else None
    return _rows(z2, c, "z2", R.B0["ffx"]) + _rows(dz1, c, "dz1", R.B0["ffx"], quiet=q)


FFX_CASES = [(r, M) for r in R.LN_REGIMES + ["gate"] for M in R.LN_M]


@pytest.mark.parametrize("entry,regime,M", [(e, r, M) for e in ("ramp_op_ffx16", "ramp_op_ffx") for r, M in FFX_CASES] + [("ramp_op_ffx16", "mixed", 20000)])
def test_ffx_in_every_row_regime(entry, regime, M):
    """z2 and dz1 against float64 autograd, tensor-wide and per token, unscaled and scaled from the recorded maxima; the four recorded
    maxima (LN output, a gelu(g), dz, d[a | g]) are the float64 operands'.  M = 20000 (full tiles) for ffx16's `mixed` case only."""
    c = R.ffx_case(regime, M)
    z2, dz1, rec, flag = _ffx(entry, c, [0.0] * 4)
    _contract(entry, c, [0.0] * 4, flag, _ffx_rows(c, z2, dz1), np.isfinite(z2).all() and np.isfinite(dz1).all())
    _maxima(entry, rec, c, ("y", "hg", float(np.abs(c["dz"]).max()), "dag"), (1e-6, 1e-6, 1e-6, 2e-5))
    z2, dz1, _, flag = _ffx(entry, c, rec)
    _contract(entry, c, rec, flag, _ffx_rows(c, z2, dz1), np.isfinite(z2).all() and np.isfinite(dz1).all())
    if regime == "gate":
        # rows of z1 that are zero: LN output = beta = 0, a = 0 (no bias on that half), hidden = 0 x gelu(g) = 0, z2 = 0 + 0 + b2 -- exact in
        # any order of the three additions
        assert np.array_equal(z2[::3], np.tile(c["p"]["b2"], (len(z2[::3]), 1)))


# ---- tkl / tkl16 ------------------------------------------------------------------------------------------------------------------------
def _tkl(entry, c, prev, X=None):
    M, N, epi = c["M"], c["N"], c["epi"]
    d = [dev(X if X is not None else c["X"]), dev(c["W"]), dev(c["bias"]) if epi else None, dev(c["resid"]) if epi & 1 else None,
         dev(c["rowbias"]) if epi & 2 else None, dev(c["rowvar"]) if epi & 2 else None, dev(c["g"]) if c["ln"] else None, dev(c["b"]) if c["ln"] else None]
    Y = nans(M, N)
    out, flag = C.c_float(0), C.c_int32(0)
    _lib.check(getattr(_lib.load(), entry)(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]), P(d[5]), R.TKL_NVAR if epi & 2 else 0, R.TKL_L, P(d[6]), P(d[7]),
                                           M, N, prev, P(Y), C.byref(out), C.byref(flag), None), entry)
    return Y.cpu().numpy(), out.value, flag.value


@pytest.mark.parametrize("N,ln,epi", R.TKL_FORMS)
@pytest.mark.parametrize("M", R.LN_M)
@pytest.mark.parametrize("regime", R.LN_REGIMES)
@pytest.mark.parametrize("entry", ["ramp_op_tkl16", "ramp_op_tkl"])
def test_tkl_in_every_row_regime(entry, regime, M, N, ln, epi):
    """Y against float64, tensor-wide and per token, unscaled and scaled from the recorded maximum; the recorded maximum is the float64
    operand's (the LayerNorm output where the norm is folded in)."""
    c = R.tkl_case(regime, M, N, ln, epi)
    Y, rec, flag = _tkl(entry, c, 0.0)
    _contract(entry, c, [0.0], flag, _rows(Y, c, "Y", R.B0["tkl"]), np.isfinite(Y).all())
    _maxima(entry, [rec], c, ("op",), (1e-6,))
    Y, _, flag = _tkl(entry, c, rec)
    _contract(entry, c, [rec], flag, _rows(Y, c, "Y", R.B0["tkl"]), np.isfinite(Y).all())


# ---- tklb -------------------------------------------------------------------------------------------------------------------------------
def _tklb(c, prev, dqkv=None):
    M = c["M"]
    d = [dev(dqkv if dqkv is not None else c["dqkv"]), dev(np.ascontiguousarray(c["Wqkv"].T)), dev(c["z"]), dev(c["g"]), dev(c["add"])]
    out = nans(M, 256)
    amax, flag = C.c_float(0), C.c_int32(0)
    _lib.check(_lib.load().ramp_op_tklb(*[P(t) for t in d], M, prev, P(out), C.byref(amax), C.byref(flag), None), "ramp_op_tklb")
    return out.cpu().numpy(), amax.value, flag.value


@pytest.mark.parametrize("M", R.LN_M)
@pytest.mark.parametrize("regime", R.LN_REGIMES)
def test_tklb_in_every_row_regime(regime, M):
    """d(qkv) Wqkv^T + LayerNorm backward + add on z in every row regime, per token (natural scale: fused_ref's docstring)."""
    c = R.tklb_case(regime, M)
    out, rec, flag = _tklb(c, 0.0)
    _contract("tklb", c, [0.0], flag, _rows(out, c, "out", R.B0["tklb"]), np.isfinite(out).all())
    _maxima("tklb", [rec], c, (float(np.abs(c["dqkv"]).max()),), (1e-6,))
    out, _, flag = _tklb(c, rec)
    _contract("tklb", c, [rec], flag, _rows(out, c, "out", R.B0["tklb"]), np.isfinite(out).all())


# ---- plain LayerNorm and GEGLU -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,M", [(r, R.LN_M[0]) for r in R.LN_REGIMES] + [("mixed", R.LN_M[1])])
def test_layernorm_in_every_row_regime(regime, M):
    c = R.layernorm_case(regime, M)
    d = {k: dev(c[k]) for k in ("x", "g", "b", "dy", "add")}
    y, dx = nans(M, 256), nans(M, 256)
    lib = _lib.load(); S = _lib.current_stream()
    _lib.check(lib.ramp_op_layernorm(P(d["x"]), P(d["g"]), P(d["b"]), P(y), M, S))
    _lib.check(lib.ramp_op_layernorm_bwd(P(d["dy"]), P(d["x"]), P(d["g"]), P(d["add"]), P(dx), M, S))
    y, dx = y.cpu().numpy(), dx.cpu().numpy()
    c = dict(c, sites=[])
    _contract("layernorm", c, [], 0, _rows(y, c, "y", R.B0["layernorm"]) + _rows(dx, c, "dx", R.B0["layernorm_bwd"]),
              np.isfinite(y).all() and np.isfinite(dx).all(), guard=False)
    if regime == "const":
        assert R.rel_rows(y, np.tile(c["b"].astype(np.float64), (M, 1))) < R.B0["layernorm"]      # LN of a zero-variance row is beta


@pytest.mark.parametrize("regime", ["gauss", "tails"])
def test_geglu_gate_tails(regime):
    """a gelu(g) and its gradient with g out to +-12 and beyond (both Phi tails), per row; rows whose "a" half is zero give exact zeros."""
    c = R.geglu_case(regime)
    M, Fh = c["M"], R.GEGLU_F
    ag, dh = dev(c["ag"]), dev(c["dh"])
    h, dag = nans(M, Fh), nans(M, 2 * Fh)
    lib = _lib.load(); S = _lib.current_stream()
    _lib.check(lib.ramp_op_geglu(P(ag), P(h), M, Fh, S))
    _lib.check(lib.ramp_op_geglu_bwd(P(dh), P(ag), P(dag), M, Fh, S))
    h, dag = h.cpu().numpy(), dag.cpu().numpy()
    c = dict(c, sites=[])
    _contract("geglu", c, [], 0, _rows(h, c, "h", R.B0["geglu"]) + _rows(dag, c, "dag", R.B0["geglu"]), np.isfinite(h).all() and np.isfinite(dag).all(), guard=False)
    if regime == "tails":
        assert (h[::3] == 0).all() and (dag[::3, Fh:] == 0).all()


# ---- tkw / tkc: conv5 + bias -> GroupNorm(8) -> Mish + extras, and the input gradient ---------------------------------------------------
def _tkw_fwd(c, prev, X=None):
    M, L, N, K, K1 = c["M"], c["L"], c["N"], c["K"], c["K1"]
    X = c["X"] if X is None else X
    xa, xb = (dev(X[:, :K1]), dev(X[:, K1:])) if K1 else (dev(X), None)
    d = [dev(c[k]) for k in ("W", "bias", "gam", "bet")]
    tb = dev(c["tb"]) if c["tb"].any() else None
    res = dev(c["res"]) if c["res"].any() else None
    Y, Cs, st = nans(M, N), nans(M, N), nans(c["R"], 8, 2)
    amax, flag = C.c_float(0.0), C.c_int32(0)
    _lib.check(_lib.load().ramp_op_tkw(P(xa), P(xb), K1, P(d[0]), P(d[1]), P(res), None, None, None, None, None, P(d[2]), P(d[3]), P(tb), M, L, N, K, 1, N,
                                       prev, P(Y), None, P(Cs), P(st), C.byref(amax), C.byref(flag), _lib.current_stream()), "ramp_op_tkw")
    st = st.cpu().numpy()
    return dict(stash=Cs.cpu().numpy(), mean=st[..., 0], rstd=st[..., 1], y=Y.cpu().numpy()), amax.value, flag.value


def _gn_fwd_rows(c, got):
    Rn = c["R"]
    q = c["quiet"] if c["quiet"].any() else None
    rows = []
    for name, b0 in (("stash", "tkw_stash"), ("mean", "tkw_stats"), ("rstd", "tkw_stats"), ("y", "tkw_y")):
        rows += _rows(got[name], c, name, R.B0[b0], Rn, q)
    return rows


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("shape", list(R.GN_SHAPES))
def test_tkw_forward_in_every_sample_regime(shape, regime):
    """Stash, statistics and y per sample against float64, unscaled and scaled from the recorded maximum (exactly max |X|); flat samples:
    y = mish(beta) + extras to b0 and rstd = eps^-1/2 to 2e-6."""
    c = R.tkw_fwd_case(shape, regime)
    narrow = shape.startswith("tkc")
    got, rec, flag = _tkw_fwd(c, 0.0)
    fin = all(np.isfinite(v).all() for v in got.values())
    _contract("tkw fwd " + shape, c, [0.0], flag, _gn_fwd_rows(c, got), fin, guard=not narrow)
    assert rec == float(np.abs(c["X"]).max())
    got, _, flag = _tkw_fwd(c, rec)
    fin = all(np.isfinite(v).all() for v in got.values())
    _contract("tkw fwd " + shape, c, [rec], flag, _gn_fwd_rows(c, got), fin)
    if c["flat"].any() and flag == 0:
        L, N, Rn = c["L"], c["N"], c["R"]
        f = c["flat"]
        y = got["y"].reshape(Rn, L, N)[f]
        want = R._mish64(c["bet"].astype(np.float64)) + c["tb"] + c["res"].reshape(Rn, L, N)[f]
        e_y, e_r = R.rel_rows(y, want), float(np.abs(got["rstd"][f] * np.sqrt(R.EPS) - 1).max())
        print(f"tkw fwd {shape} {regime}, flat samples: y against mish(beta) + extras {e_y:.2e} (bar {R.B0['tkw_y']:.0e}), rstd against eps^-1/2 {e_r:.2e} (bar 2e-6)")
        assert e_y < R.B0["tkw_y"] and e_r < 2e-6


def _tkw_bwd(c, prev, dy=None):
    M, L, N, K, N1 = c["M"], c["L"], c["N"], c["K"], c["N1"]
    d = [dev(c["dy"] if dy is None else dy), dev(c["W"]), dev(c["cst"]), dev(c["stats"]), dev(c["gam"]), dev(c["bet"])]
    r1 = dev(c["r1"]) if c["r1"].any() else None
    Ya = nans(M, N1 or N); Yb = nans(M, N - N1) if N1 else None
    amax, flag = C.c_float(0.0), C.c_int32(0)
    _lib.check(_lib.load().ramp_op_tkw(P(d[0]), None, 0, P(d[1]), None, P(r1), None, P(d[2]), P(d[3]), P(d[4]), P(d[5]), None, None, None, M, L, N, K, -1,
                                       N1 or N, prev, P(Ya), P(Yb), None, None, C.byref(amax), C.byref(flag), _lib.current_stream()), "ramp_op_tkw")
    got = Ya.cpu().numpy() if not N1 else np.concatenate([Ya.cpu().numpy(), Yb.cpu().numpy()], axis=1)
    return got, amax.value, flag.value


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("shape", list(R.GN_BWD_SHAPES))
def test_tkw_input_gradient_in_every_sample_regime(shape, regime):
    """conv5^T(GNbwd(dY mish'(.) gamma)) + residual per sample against float64, unscaled and scaled from the recorded maximum of the operand the
    kernel never materialises (2e-5, as test_tkw_groupnorm_backward_conv_input_gradient)."""
    c = R.tkw_bwd_case(shape, regime)
    narrow = shape.startswith("tkc")
    q = c["quiet"] if c["quiet"].any() else None
    got, rec, flag = _tkw_bwd(c, 0.0)
    _contract("tkw bwd " + shape, c, [0.0], flag, _rows(got, c, "dx", R.B0["tkw_dx"], c["R"], q),
              np.isfinite(got).all(), guard=not narrow)
    _maxima("tkw bwd", [rec], c, ("dc",), (2e-5,))
    got, _, flag = _tkw_bwd(c, rec)
    _contract("tkw bwd " + shape, c, [rec], flag, _rows(got, c, "dx", R.B0["tkw_dx"], c["R"], q), np.isfinite(got).all())


def _tkc(c, prev, A=None, bias=None, resid=None):
    out = nans(c["M"], c["N"])
    dA, dW, db, dr = dev(c["A"] if A is None else A), dev(c["W"]), dev(bias), dev(resid)
    amax, flag = _lib.op_gemm(dA, dW, db, dr, out, c["M"], c["N"], c["K"], 5, -2, 1, c["L"], mode="fp16x3-tkc", a_absmax_prev=prev)
    return out.cpu().numpy(), amax, flag


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["ramp_op_tkl16", "ramp_op_tkl"])
def test_constant_rows_give_the_projection_of_beta(entry):
    """LayerNorm of a zero-variance row is beta whatever the row's value, so on `const` rows (0.7 everywhere) LN -> linear is W beta, to the
    entry's own bar b0 -- in a whole tensor of them and between other rows in `mixed`."""
    N, ln, epi = R.TKL_FORMS[1]
    for regime in ("const", "mixed"):
        c = R.tkl_case(regime, R.LN_M[0], N, ln, epi)
        const = np.array([k == "const" for k in R.row_kind_of(regime, c["M"])])
        want = np.tile(c["W"].astype(np.float64) @ c["b"].astype(np.float64), (int(const.sum()), 1))
        for prev in (0.0, float(np.abs(c["ref"]["op"]).max())):
            Y, _, flag = _tkl(entry, c, prev)
            e = R.rel_rows(Y[const], want)
            print(f"{entry} {regime} prev={prev:.3g}: const rows against W beta {e:.2e} (bar {R.B0['tkl']:.0e}), flag {flag}")
            assert flag == 0 and e < R.B0["tkl"], (regime, prev, e)


@pytest.mark.parametrize("entry", ["ramp_op_ffx16", "ramp_op_ffx"])
def test_ffx_backward_on_constant_rows(entry):
    """On `const` rows x^ = 0 and rstd = eps^-1/2: the LayerNorm backward is eps^-1/2 (gamma d - mean(gamma d)) there, 300 x a Gaussian row's, and
    dz1 = dz + that against float64 per row, on the natural scale of fused_ref's docstring (the row's own maximum)."""
    c = R.ffx_case("const", R.LN_M[0])
    z2, dz1, rec, flag = _ffx(entry, c, [0.0] * 4)
    # (unscaled, every row's a gelu(g) is the same vector, its maximum below 2^-3: the guard's business, _contract)
    _contract(entry, c, [0.0] * 4, flag, _rows(dz1, c, "dz1", R.B0["ffx"]), np.isfinite(dz1).all())
    z2, dz1, _, flag = _ffx(entry, c, rec)
    _contract(entry, c, rec, flag, _rows(dz1, c, "dz1", R.B0["ffx"]), np.isfinite(dz1).all())
    assert flag == 0
    assert np.abs(c["ref"]["dz1"] - c["dz"]).max() > 30 * np.abs(c["dz"]).max()          # (the backward term dominates the bypass)


def test_all_zero_operands_with_a_recorded_maximum_give_the_bias_only_result():
    """A zero operand under a scale from an earlier maximum: no NaN, the epilogue's terms alone, and no flag (`bm > 0` guards the shrink
    test, core.h:75)."""
    c = R.tkl_case("gauss", R.LN_M[0], 96, False, 1)
    for entry in ("ramp_op_tkl16", "ramp_op_tkl"):
        Y, rec, flag = _tkl(entry, c, 3.0, X=np.zeros_like(c["X"]))
        assert flag == 0 and rec == 0 and np.array_equal(Y, c["bias"][None, :] + c["resid"]), entry
    c = R.tklb_case("gauss", R.LN_M[0])
    out, rec, flag = _tklb(c, 3.0, dqkv=np.zeros_like(c["dqkv"]))
    assert flag == 0 and rec == 0 and R.rel_rows(out, c["add"]) < 1e-7
    c = R.ffx_case("gauss", R.LN_M[0])
    d = list(_ffx_dev(c)); d[1] = dev(np.zeros_like(c["dz"]))
    for entry in ("ramp_op_ffx16", "ramp_op_ffx"):
        z2, dz1, rec, flag = _ffx(entry, c, [0.0, 0.0, 3.0, 3.0], d)
        assert flag == 0 and rec[2] == 0 and rec[3] == 0 and (dz1 == 0).all(), entry
    for shape in ("tkw128", "tkc64"):
        c = R.tkw_fwd_case(shape, "gauss", 1)
        got, rec, flag = _tkw_fwd(c, 3.0, X=np.zeros_like(c["X"]))
        want = R.tkw_fwd_ref64(dict(c, X=np.zeros_like(c["X"])))["y"]          # GroupNorm + Mish of the bias alone
        assert flag == 0 and rec == 0 and np.array_equal(got["stash"], np.tile(c["bias"], (c["M"], 1))), shape
        e = R.rel_rows(got["y"], want, c["R"])
        print(f"tkw fwd {shape}, X = 0: y against mish(GN(bias)) + time bias {e:.2e}")
        assert e < R.B0["tkw_y"]
    c = R.tkc_case("gauss")
    bias = np.linspace(-1, 1, c["N"]).astype(np.float32)
    out, rec, flag = _tkc(c, 3.0, A=np.zeros_like(c["A"]), bias=bias)
    assert flag == 0 and rec == 0 and np.array_equal(out, np.tile(bias, (c["M"], 1)))


# ---- guard-or-accurate sweep ----------------------------------------------------------------------------------------------------------------
KS = list(range(-14, 9)) + [R.K_SHRUNK]


def _sweep(what, c, n_sites, site, true_max, run):
    """run(prevs) -> (rows, finite, flag).  At every k: the flag, or the bars of the fresh scale; at K_OVERFLOW and below and at K_SHRUNK the flag
    (fused_ref.K_OVERFLOW / K_SHRUNK: from tokmma.h:28 and core.h:69, 75, not from the kernel's behaviour)."""
    line = []
    for k in KS:
        prevs = list(true_max)
        prevs[site] = true_max[site] * 2.0 ** k
        rows, finite, flag = run(prevs)
        worst = max(e / b for _, e, _, b in rows)
        line.append(f"{k}:{'F' if flag else '%.2f' % worst}")
        if k <= R.K_OVERFLOW or k >= R.K_SHRUNK:
            assert flag != 0, (what, site, k)
        if flag == 0:
            assert finite and worst < 1.0, (what, site, k, rows)
        if k == 0:
            assert flag == 0, (what, site)
    print(f"{what} site {site}: k:worst error / bar (F = flag)  " + " ".join(line))


@pytest.mark.parametrize("entry", ["ramp_op_ffx16", "ramp_op_ffx"])
def test_guard_or_accurate_sweep_ffx(entry):
    c = R.ffx_case("gauss", R.LN_M[0])
    true_max = [float(np.abs(c["ref"][k]).max()) for k in ("y", "hg")] + [float(np.abs(c["dz"]).max()), float(np.abs(c["ref"]["dag"]).max())]

    def run(prevs):
        z2, dz1, _, flag = _ffx(entry, c, prevs)
        return _ffx_rows(c, z2, dz1), bool(np.isfinite(z2).all() and np.isfinite(dz1).all()), flag
    for site in range(4):
        _sweep(entry, c, 4, site, true_max, run)


@pytest.mark.parametrize("what", ["ramp_op_tkl16", "ramp_op_tkl", "tklb", "tkw fwd", "tkw bwd", "tkc fwd", "tkc bwd", "tkc"])
def test_guard_or_accurate_sweep(what):
    if what.startswith("ramp_op_tkl"):
        c = R.tkl_case("gauss", R.LN_M[0], *R.TKL_FORMS[0])
        run = lambda p: (lambda Y, _, flag: (_rows(Y, c, "Y", R.B0["tkl"]), bool(np.isfinite(Y).all()), flag))(*_tkl(what, c, p[0]))
        top = np.abs(c["ref"]["op"]).max()
    elif what == "tklb":
        c = R.tklb_case("gauss", R.LN_M[0])
        run = lambda p: (lambda o, _, flag: (_rows(o, c, "out", R.B0["tklb"]), bool(np.isfinite(o).all()), flag))(*_tklb(c, p[0]))
        top = np.abs(c["dqkv"]).max()
    elif what.endswith("fwd"):
        c = R.tkw_fwd_case("tkw128" if what == "tkw fwd" else "tkc64", "gauss", 1)
        run = lambda p: (lambda g, _, flag: (_gn_fwd_rows(c, g), all(np.isfinite(v).all() for v in g.values()), flag))(*_tkw_fwd(c, p[0]))
        top = np.abs(c["X"]).max()
    elif what.endswith("bwd"):
        c = R.tkw_bwd_case("tkw128" if what == "tkw bwd" else "tkc64", "gauss", 1)
        run = lambda p: (lambda g, _, flag: (_rows(g, c, "dx", R.B0["tkw_dx"], c["R"]), bool(np.isfinite(g).all()), flag))(*_tkw_bwd(c, p[0]))
        top = np.abs(c["ref"]["dc"]).max()
    else:
        c = R.tkc_case("gauss")
        run = lambda p: (lambda o, _, flag: (_rows(o, c, "out", R.B0["tkc"], c["R"]), bool(np.isfinite(o).all()), flag))(*_tkc(c, p[0]))
        top = np.abs(c["A"]).max()
    _sweep(what, c, 1, 0, [float(top)], run)


def test_a_nan_in_the_operand_stays_in_its_row():
    """The guard sees the operand through its maximum, and the maximum (v_max3_f32, fmaxf) drops a NaN: `!(x s < 60000)` (core.h:69) never
    meets it, so today one NaN element raises no flag -- the documented limit of the guard (delayed scaling; attention_ref.py's
    scope note).  The flag is printed, not asserted (a NaN-aware guard may raise it); what is asserted is that the NaN does no more than
    arithmetic demands: the recorded maximum is finite, the rows the NaN enters are NaN, every other row or sample meets its bar.
    One element, one launch per entry."""
    def report(what, flag, rec, e):
        print(f"{what}, one NaN in row 5: flag {flag}, recorded maximum {rec}, rows out of its reach {e:.2e}")

    M = R.LN_M[0]
    keep = np.arange(M) != 5
    c = R.tkl_case("gauss", M, *R.TKL_FORMS[0])
    X = c["X"].copy(); X[5, 7] = np.nan
    Y, rec, flag = _tkl("ramp_op_tkl16", c, float(np.abs(c["X"]).max()), X=X)
    e = R.rel_rows(Y[keep], c["ref"]["Y"][keep])
    report("tkl16", flag, rec, e)
    assert rec == float(np.nanmax(np.abs(X))) and np.isnan(Y[5]).all() and e < R.bar(R.B0["tkl"], c["floor"]["Y"][1])
    c = R.tklb_case("gauss", M)
    dq = c["dqkv"].copy(); dq[5, 7] = np.nan
    out, rec, flag = _tklb(c, float(np.abs(c["dqkv"]).max()), dqkv=dq)
    e = R.rel_rows(out[keep], c["ref"]["out"][keep])
    report("tklb", flag, rec, e)
    assert rec == float(np.nanmax(np.abs(dq))) and np.isnan(out[5]).all() and e < R.bar(R.B0["tklb"], c["floor"]["out"][1])
    c = R.ffx_case("gauss", M)                                   # the NaN in dz: dz1 of its row, nothing of the forward
    dz = c["dz"].copy(); dz[5, 7] = np.nan
    d = list(_ffx_dev(c)); d[1] = dev(dz)
    prev = [float(np.abs(c["ref"][k]).max()) for k in ("y", "hg")] + [float(np.abs(c["dz"]).max()), float(np.abs(c["ref"]["dag"]).max())]
    for entry in ("ramp_op_ffx16", "ramp_op_ffx"):
        z2, dz1, rec, flag = _ffx(entry, c, prev, d)
        e = max(R.rel_rows(dz1[keep], c["ref"]["dz1"][keep]), R.rel_rows(z2, c["ref"]["z2"]))
        report(entry, flag, rec, e)
        assert np.isfinite(rec).all() and np.isnan(dz1[5]).all() and e < R.bar(R.B0["ffx"], max(c["floor"]["dz1"][1], c["floor"]["z2"][1]))
    c = R.tkw_fwd_case("tkw128", "gauss")                        # the NaN's sample is lost to its statistics; the other samples are not
    X = c["X"].copy(); X[5, 7] = np.nan
    got, rec, flag = _tkw_fwd(c, float(np.abs(c["X"]).max()), X=X)
    ks = np.arange(c["R"]) != 5 // c["L"]
    e = max(R.rel_rows(got[k].reshape(c["R"], -1)[ks], c["ref"][k].reshape(c["R"], -1)[ks]) for k in ("stash", "y"))
    report("tkw forward", flag, rec, e)
    assert rec == float(np.nanmax(np.abs(X))) and np.isnan(got["y"].reshape(c["R"], -1)[~ks]).all() and e < R.bar(R.B0["tkw_y"], c["floor"]["y"][1])
    c = R.tkc_case("gauss")
    A = c["A"].copy(); A[5, 7] = np.nan
    out, rec, flag = _tkc(c, float(np.abs(c["A"]).max()), A=A)
    keep = np.abs(np.arange(c["M"]) - 5) > 2
    e = R.rel_rows(out[keep], c["ref"]["out"][keep])
    report("tkc", flag, rec, e)
    assert rec == float(np.nanmax(np.abs(A))) and np.isnan(out[3:8]).all() and e < R.bar(R.B0["tkc"], c["floor"]["out"][1])


# ---- per-row accuracy under a magnitude spread ----------------------------------------------------------------------------------------------
def _spread_report(what, c, got, name, n_rows, flag, b0):
    """Tensor-wide and per row: the tensor-wide number alone would pass a quiet row that is wrong from its third digit on (2^-10 x 1e-3 < 3e-6)."""
    q, ref, (f_all, f_rows) = c["quiet"], c["ref"][name], c["floor"][name]
    per = R.row_errors(got, ref, n_rows)
    e_all, b_all, b = R.rel(got, ref), R.bar(b0, f_all), R.bar(b0, f_rows)
    print(f"{what} {c['regime']}: flag {flag}; tensor-wide {e_all:.1e} (bar {b_all:.1e}); relative to the row's own maximum: quiet rows worst {per[q].max():.1e} "
          f"median {np.median(per[q]):.1e} (bound {R.QUIET_BOUND:.1e}), the others worst {per[~q].max():.1e} (bar {b:.1e})")
    assert np.isfinite(per).all()
    assert e_all < b_all or flag != 0
    assert per[~q].max() < b or flag != 0
    assert per[q].max() < R.QUIET_BOUND or flag != 0


@pytest.mark.parametrize("regime", ["quiet_shared", "quiet_own"])
def test_per_row_accuracy_under_a_magnitude_spread_token_kernels(regime):
    """The abl test's trade-off for the token-owning kernels: rows 2^-10 of their neighbours keep 2^-30 of the TENSOR's maximum, i.e. < 2^-17
    of their own, under the one scale per operand tensor; the other rows keep the ordinary bar.  quiet_shared: the quiet rows sit among loud
    ones in every wave (no flag: every wave's maximum is in range); quiet_own: a whole 128-token tile is quiet -- the control: the kernels
    judge "the operand shrank" on a wave's or a block's rows, so either the flag is raised or the bound holds."""
    M = R.LN_M[0]
    c = R.tkl_case(regime, M, 256, False, 0)
    top = float(np.abs(c["X"]).max())
    for entry in ("ramp_op_tkl16", "ramp_op_tkl"):
        Y, _, flag = _tkl(entry, c, top)
        _spread_report(entry, c, Y, "Y", None, flag, R.B0["tkl"])
        assert flag == 0 or regime == "quiet_own"
    c = R.tklb_case(regime, M)
    out, _, flag = _tklb(c, float(np.abs(c["dqkv"]).max()))
    _spread_report("tklb", c, out, "out", None, flag, R.B0["tklb"])
    assert flag == 0 or regime == "quiet_own"
    c = R.ffx_case(regime, M)
    for entry in ("ramp_op_ffx16", "ramp_op_ffx"):
        _, _, rec, _ = _ffx(entry, c, [0.0] * 4)
        _, dz1, _, flag = _ffx(entry, c, rec)
        _spread_report(entry, c, dz1, "dz1", None, flag, R.B0["ffx"])
        assert flag == 0 or regime == "quiet_own"


def test_per_sample_accuracy_under_a_magnitude_spread_bare_convolution():
    """The same for tkc's bare convolution (L = 24: two samples per wave, the quiet ones share theirs): scaled from the tensor's maximum the
    quiet samples keep < 2^-17 of their own maximum; unscaled every wave tile is scaled from its own maximum (printed)."""
    c = R.tkc_case("quiet_sample")
    for prev in (0.0, float(np.abs(c["A"]).max())):
        out, _, flag = _tkc(c, prev)
        c2 = dict(c, regime=f"quiet_sample prev={prev:.3g}")
        _spread_report("tkc", c2, out, "out", c["R"], flag, R.B0["tkc"])
        assert flag == 0
