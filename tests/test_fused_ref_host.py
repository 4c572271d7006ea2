"""The regimes of fused_ref.py are what they claim, measured on the generated data; its float64 references agree with torch float64
autograd and with the oracle; every float32 floor stays under the cap, so a correct kernel has room inside every bar (CPU only)."""
import numpy as np
import pytest
import torch

import fused_ref as R
from oracle import ramp_oracle as O

M0 = R.LN_M[0]


def _ln_stats(x):
    x = np.asarray(x, np.float64)
    mean = x.mean(1); var = x.var(1)
    return mean, var, 1.0 / np.sqrt(var + R.EPS)


def test_row_regimes_are_what_they_say():
    """offset: |mean| rstd in [30, 50]; flat: variance < eps / 50 (rstd within 1 % of eps^-1/2); const: variance exactly 0; spike: one element
    at 300, at least 40 x the row's next largest; quiet / loud: 2^-10 / 2^10 of the Gaussian rows; mixed: every kind in every 16 consecutive
    rows and in the partial last tile, row maxima spread over more than 2^19."""
    g = lambda: np.random.Generator(np.random.PCG64(5))
    x = {k: R.ln_rows(k, M0, g()) for k in R.LN_REGIMES}
    mean, var, rstd = _ln_stats(x["offset"])
    assert 30 < (np.abs(mean) * rstd).min() and (np.abs(mean) * rstd).max() < 50
    mean, var, rstd = _ln_stats(x["flat"])
    assert var.max() < R.EPS / 50 and np.abs(rstd * np.sqrt(R.EPS) - 1).max() < 0.01
    mean, var, rstd = _ln_stats(x["const"])
    assert (var == 0).all() and (mean == np.float64(np.float32(0.7))).all()
    top2 = np.sort(np.abs(x["spike"]), axis=1)[:, -2:]
    assert (top2[:, 1] == 300).all() and (top2[:, 1] > 40 * top2[:, 0]).all()
    assert np.array_equal(x["quiet"], x["gauss"] * np.float32(2.0 ** -10)) and np.array_equal(x["loud"], x["gauss"] * np.float32(2.0 ** 10))
    kinds = R.row_kind_of("mixed", M0)
    for r0 in list(range(0, M0 - 16, 16)) + [M0 - (M0 % 128)]:
        assert set(kinds[r0:r0 + 16]) == set(R.ROW_KINDS) or r0 + 16 > M0
    assert set(kinds[M0 - (M0 % 128):]) == set(R.ROW_KINDS)
    top = R.rowmax(x["mixed"])
    assert top.max() / top.min() > 2.0 ** 19
    for i, k in enumerate(R.ROW_KINDS):          # a mixed tensor's rows have their kind's property
        mean, var, rstd = _ln_stats(x["mixed"][i::7])
        if k == "const":
            assert (var == 0).all()
        if k == "flat":
            assert var.max() < R.EPS / 50
        if k == "offset":
            assert (np.abs(mean) * rstd).min() > 30


def test_gate_regime_reaches_both_tails_and_has_exact_zero_rows():
    """g spans about +-12: more than 0.3 % of the gate arguments beyond +-6 on either side, none beyond +-20; the rows of z1 that are zero have
    a = 0, hidden = 0 and z2 = z1 + b2 = b2 exactly, in float64 and in float32."""
    c = R.ffx_case("gate", M0)
    gt = c["ref"]["gate"]
    print(f"gate arguments: min {gt.min():.2f} max {gt.max():.2f}  share < -6: {(gt < -6).mean():.4f}  > 6: {(gt > 6).mean():.4f}  beyond 20: {(np.abs(gt) > 20).mean():.1e}")
    assert gt.min() < -11 and gt.max() > 11
    assert (gt < -6).mean() > 0.003 and (gt > 6).mean() > 0.003 and (np.abs(gt) > 20).mean() == 0
    for ref in (c["ref"], c["ref32"]):
        assert (ref["hg"][::3] == 0).all() and np.abs(ref["hg"][1::3]).max() > 1
        assert (ref["z2"][::3] == c["p"]["b2"].astype(ref["z2"].dtype)).all()
    t = R.geglu_case("tails")
    gt = t["ag"][:, R.GEGLU_F:]
    assert gt.min() < -12 and gt.max() > 12 and (np.abs(gt) > 6).mean() > 0.05
    assert (t["ref"]["h"][::3] == 0).all()


def _gn_stats(c):
    ref = c["ref"]
    return np.abs(ref["mean"]) * ref["rstd"], ref["var"]


@pytest.mark.parametrize("shape", list(R.GN_SHAPES))
def test_sample_regimes_are_what_they_say(shape):
    """Forward (on the stash c = conv + bias) and backward (on the given stash): offset: |mean| rstd in [25, 60]; flat: variance exactly 0 in
    the special samples, rstd = eps^-1/2, y = mish(beta) + extras; outlier_group: group 3's spread ten times its neighbours'; saturated: mish's
    argument beyond +-40 on both sides; quiet_sample: the special samples' stash (forward) / gradient (backward) 2^-12 .. 2^-8 of the others';
    the special samples sit in the first tile and in the partly empty last one."""
    L, K, N, Rn, _ = R.GN_SHAPES[shape]
    tile = 96 if shape.startswith("tkw") else 4 * (48 if 48 % L == 0 else 32 if 32 % L == 0 else 64)
    sp = R.special_samples(Rn)
    assert (Rn * L) % tile != 0 and sp[0] * L < tile and sp[1] * L >= (Rn * L // tile) * tile
    kappa, var = _gn_stats(R.tkw_fwd_case(shape, "offset"))
    assert 25 < kappa.min() and kappa.max() < 60, (kappa.min(), kappa.max())
    c = R.tkw_fwd_case(shape, "flat")
    assert (c["ref"]["var"][sp] == 0).all() and (c["ref"]["var"][2] > 0.1).all()
    assert np.abs(c["ref"]["rstd"][sp] * np.sqrt(R.EPS) - 1).max() < 1e-12
    y = c["ref"]["y"].reshape(Rn, L, N)[sp]
    want = R._mish64(c["bet"].astype(np.float64)) + c["tb"] + c["res"].reshape(Rn, L, N)[sp]
    assert np.abs(y - want).max() < 1e-13
    c = R.tkw_fwd_case(shape, "outlier_group")
    sd = np.sqrt(c["ref"]["var"])
    assert (sd[:, 3] > 5 * np.delete(sd, 3, axis=1).max(1)).all()
    a = R.tkw_fwd_case(shape, "saturated")["ref"]["arg"]
    assert a.min() < -40 and a.max() > 40
    c = R.tkw_fwd_case(shape, "quiet_sample")
    top = R.rowmax(c["ref"]["stash"], Rn)
    ratio = top[sp] / np.delete(top, sp).max()
    assert (2.0 ** -12 < ratio).all() and (ratio < 2.0 ** -8).all(), ratio
    assert tuple(R._sample_scale("mixed", Rn)[0][:3]) == (1.0, 1.0, R.QUIET_SHIFT) and R._sample_scale("mixed", Rn)[1][1]
    for case, key in ((R.tkw_fwd_case(shape, "mixed"), "X"), (R.tkw_bwd_case(shape, "mixed"), None)):      # the quiet samples: 2^-10 of the operand's maximum
        top = R.rowmax(case["sites"][0], case["R"])
        ratio = top[case["quiet"]] / top.max()
        assert (2.0 ** -12 < ratio).all() and (ratio < 2.0 ** -8).all(), (shape, ratio)
    for case in (R.tkw_fwd_case(shape, "mixed"), R.tkw_bwd_case(shape, "mixed"), R.tkw_fwd_case(shape, "quiet_sample"), R.tkw_bwd_case(shape, "quiet_sample")):
        assert 32 <= case["sites"][0].max() < 64 and R.operand_scale(case["sites"][0].max()) == 1      # scale 1 is the fresh scale: to_window
    # backward
    Lb, Kb, Nb, Rb, _ = R.GN_BWD_SHAPES[shape]
    c = R.tkw_bwd_case(shape, "offset")
    kb = np.abs(c["stats"][..., 0]) * c["stats"][..., 1]
    assert 25 < kb.min() and kb.max() < 60
    c = R.tkw_bwd_case(shape, "flat")
    assert np.abs(c["stats"][sp][..., 1] * np.sqrt(R.EPS) - 1).max() < 1e-6
    cg = c["cst"].reshape(Rb, Lb, 8, Kb // 8)[sp]
    assert (cg == cg[:, :1, :, :1]).all()
    a = R.tkw_bwd_case(shape, "saturated")["ref"]["arg"]
    assert a.min() < -40 and a.max() > 40
    c = R.tkw_bwd_case(shape, "quiet_sample")
    top = R.rowmax(c["ref"]["dx"], Rb)
    ratio = top[sp] / np.delete(top, sp).max()
    assert (2.0 ** -12 < ratio).all() and (ratio < 2.0 ** -8).all(), ratio


def _ln_cases():
    for regime in R.LN_REGIMES + ["gate", "quiet_shared", "quiet_own"]:
        for M in R.LN_M:
            yield f"ffx {regime} M={M}", R.ffx_case(regime, M)
    yield "ffx mixed M=20000", R.ffx_case("mixed", 20000)
    for regime in R.LN_REGIMES:
        for M in R.LN_M:
            for N, ln, epi in R.TKL_FORMS:
                yield f"tkl {regime} M={M} N={N}", R.tkl_case(regime, M, N, ln, epi)
            yield f"tklb {regime} M={M}", R.tklb_case(regime, M)
            yield f"layernorm {regime} M={M}", R.layernorm_case(regime, M)
    for regime in ("quiet_shared", "quiet_own"):
        yield f"tkl {regime}", R.tkl_case(regime, M0, 256, False, 0)
        yield f"tklb {regime}", R.tklb_case(regime, M0)
    for regime in ("gauss", "tails"):
        yield f"geglu {regime}", R.geglu_case(regime)


def _gn_cases():
    for shape in R.GN_SHAPES:
        for regime in R.GN_REGIMES:
            yield f"tkw fwd {shape} {regime}", R.tkw_fwd_case(shape, regime)
            yield f"tkw bwd {shape} {regime}", R.tkw_bwd_case(shape, regime)
    for regime in ("gauss", "quiet_sample"):
        yield f"tkc {regime}", R.tkc_case(regime)


@pytest.mark.parametrize("family", ["layernorm", "groupnorm"])
def test_float32_floor_of_every_case_is_below_the_cap(family):
    """The float32 evaluation against float64, tensor-wide and per row / sample, for every (composition, regime, output): all <= 2e-5, so
    no bar max(b0, 4 floor) exceeds 8e-5; nothing non-finite in any reference."""
    worst = 0.0
    for name, c in (_ln_cases() if family == "layernorm" else _gn_cases()):
        print(f"{name}: " + "  ".join(f"{k} {a:.1e} / rows {b:.1e}" for k, (a, b) in c["floor"].items()))
        for k, (a, b) in c["floor"].items():
            assert np.isfinite(c["ref"][k]).all() and np.isfinite(c["ref32"][k]).all(), (name, k)
            assert a <= R.FLOOR_CAP and b <= R.FLOOR_CAP, (name, k, a, b)
            worst = max(worst, a, b)
            q = c.get("quiet")
            if q is not None and q.any() and k != "z2":      # the quiet rows' own floor leaves the factor 4 inside the 2^-17 bound, and the operand sits in the window
                fq = R.row_errors(c["ref32"][k], c["ref"][k], len(q), c.get("scale", {}).get(k))[q].max()
                print(f"    quiet rows of {k}: float32 floor {fq:.1e}")
                assert 4 * fq <= R.QUIET_BOUND, (name, k, fq)
    print(f"worst float32 floor ({family}): {worst:.2e}")
    assert max(R.bar(b0, worst) for b0 in R.B0.values()) <= 8e-5


def test_layernorm_references_agree_with_the_oracle():
    for regime in R.LN_REGIMES:
        c = R.layernorm_case(regime, M0)
        y, cache = O.layernorm_fwd(c["x"].astype(np.float64), c["g"].astype(np.float64), c["b"].astype(np.float64))
        dx = O.layernorm_bwd(c["dy"].astype(np.float64), c["g"].astype(np.float64), cache) + c["add"]
        assert R.rel_rows(c["ref"]["y"], y) < 1e-11 and R.rel_rows(c["ref"]["dx"], dx) < 1e-9, regime
    c = R.geglu_case("tails")
    a, gg = c["ag"][:, :R.GEGLU_F].astype(np.float64), c["ag"][:, R.GEGLU_F:].astype(np.float64)
    assert R.rel(c["ref"]["h"], a * O.gelu(gg)) < 1e-12
    assert R.rel(c["ref"]["dag"], np.concatenate([c["dh"] * O.gelu(gg), c["dh"] * a * O.gelu_grad(gg)], axis=-1)) < 1e-12


@pytest.mark.parametrize("regime", R.GN_REGIMES)
def test_groupnorm_references_agree_with_the_oracle_and_with_torch_float64(regime):
    """The numpy formulas (test_gpu_ops.py's) against oracle.groupnorm_fwd / _bwd + mish / mish_grad and against the torch evaluation in
    float64 (its mish' is autograd's, its convolutions torch's)."""
    for shape in ("tkw128", "tkc64", "tkw_split"):
        c = R.tkw_fwd_case(shape, regime)
        L, N, Rn = c["L"], c["N"], c["R"]
        st = c["ref"]["stash"]
        n, cache = O.groupnorm_fwd(st.reshape(Rn, L, N), c["gam"].astype(np.float64), c["bet"].astype(np.float64), 8, R.EPS)
        y = O.mish(n).reshape(Rn * L, N) + c["tb"] + c["res"]
        assert R.rel_rows(c["ref"]["y"], y, Rn) < 1e-10 and R.rel(c["ref"]["rstd"], cache[1].reshape(Rn, 8)) < 1e-12
        t64 = R.tkw_fwd_eval(c, torch.float64)
        for k in ("stash", "mean", "rstd", "y"):
            assert R.rel_rows(t64[k], c["ref"][k], Rn) < 1e-9, (shape, k)
        b = R.tkw_bwd_case(shape, regime)
        L, K, Rn = b["L"], b["K"], b["R"]
        t64 = R.tkw_bwd_eval(b, torch.float64)
        assert R.rel_rows(t64["dx"], b["ref"]["dx"], Rn) < 1e-9 and R.rel_rows(t64["dc"], b["ref"]["dc"], Rn) < 1e-9, shape
        m32, r32 = b["stats"][..., 0].astype(np.float64), b["stats"][..., 1].astype(np.float64)
        xhat = ((b["cst"].astype(np.float64).reshape(Rn, L, 8, K // 8) - m32[:, None, :, None]) * r32[:, None, :, None]).reshape(Rn, L, K)
        gam = b["gam"].astype(np.float64)
        dn = b["dy"].astype(np.float64).reshape(Rn, L, K) * O.mish_grad(xhat * gam + b["bet"])
        dc = O.groupnorm_bwd(dn, gam, (xhat, r32[:, None, :, None], 8))
        assert R.rel_rows(b["ref"]["dc"], dc.reshape(Rn * L, K), Rn) < 1e-9, shape


def test_exact_expectations_of_const_and_flat_rows_hold_in_float64():
    """const rows: LN output = beta exactly, so the tkl output is W beta + bias (+ extras).  The LayerNorm backward of a zero-variance row is NOT
    zero: x^ = 0 and rstd = eps^-1/2 leave dx = eps^-1/2 (gamma dy - mean(gamma dy)), which is what ffx's dz1 - dz equals on those rows."""
    for N, ln, epi in R.TKL_FORMS:
        if not ln:
            continue
        c = R.tkl_case("const", M0, N, ln, epi)
        want = c["W"].astype(np.float64) @ c["b"].astype(np.float64)
        assert np.abs(c["ref"]["Y"] - want).max() < 1e-13
    c = R.ffx_case("const", M0)
    assert np.array_equal(c["ref"]["y"], np.tile(c["p"]["b"].astype(np.float64), (M0, 1)))
    lc = R.layernorm_case("const", M0)
    gv = lc["dy"].astype(np.float64) * lc["g"]
    want = (gv - gv.mean(1, keepdims=True)) / np.sqrt(R.EPS) + lc["add"]
    assert R.rel_rows(lc["ref"]["dx"], want) < 1e-12
    assert (lc["ref"]["y"] == lc["b"].astype(np.float64)).all()


def test_scale_rule_and_guard_states():
    """operand_scale is tokmma.h's rule (max -> [2^5, 2^6)); the two ends of the window sit where K_OVERFLOW / K_SHRUNK say, for every mantissa."""
    for mx, want in ((1.0, 32.0), (1.999, 32.0), (2.0, 16.0), (47.0, 1.0), (0.0, 1.0), (3e-5, 2.0 ** 21)):
        assert R.operand_scale(mx) == want, (mx, R.operand_scale(mx))
    for m in (1.0, 1.5, 1.83, 1.999):
        rm = np.array([m, m / 3])
        assert R.guard_state(rm, m * 2.0 ** R.K_OVERFLOW) == "must" and R.guard_state(rm, m * 2.0 ** R.K_SHRUNK) == "must"
        assert R.guard_state(rm, m * 2.0 ** (R.K_SHRUNK - 1)) != "must" and R.guard_state(rm, m * 2.0 ** (R.K_OVERFLOW + 2)) != "must"
        assert R.guard_state(rm, m) == "never" and R.guard_state(np.array([m, 0.0]), m) == "never"
        assert R.guard_state(np.array([m, m * 2.0 ** -10]), m) == "either"
    assert R.guard_state(np.array([1.0, np.nan]), 1.0) == "must"
    assert R.row_errors(np.zeros((2, 3)), np.zeros((2, 3))).max() == 0 and np.isinf(R.row_errors(np.array([[1e-30, 0.0]]), np.zeros((1, 2)))).all()
