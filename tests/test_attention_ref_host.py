"""The attention regimes of attention_ref.py are what they claim, on float64, and the float32 yardstick and the emulation of atk.hip's
arithmetic leave a correct kernel room inside every bar (CPU only)."""
import numpy as np
import pytest

import attention_ref as A
from oracle import ramp_oracle as O
from ramp_amd import synth
from util import GOLDEN, weights

CASES = [(regime, L, R) for regime in A.ACCURACY_REGIMES + ["zero_v", "zero_dout"] for (L, R) in A.PLAIN_SHAPES]
QUIET = [("quiet_sample", L, R, side) for (L, R) in A.QUIET_SHAPES for side in ("fwd", "bwd")]


def _all_cases():
    return [A.case(*c) for c in CASES] + [A.case(*c) for c in QUIET]


@pytest.mark.parametrize("regime", ["sharp3", "sharp6"])
def test_sharp_regimes_are_peaked(regime):
    """Mean over queries of the largest probability >= 0.8 (sharp3) / 0.95 (sharp6) at every length; the logits reach far past what
    exp() stands without the maximum subtracted in sharp6 (|logit| > 88 overflows float32)."""
    for L, R in A.PLAIN_SHAPES:
        c = A.case(regime, L, R)
        P = A.probs_ref64(c["qkv"], L)
        assert P.max(-1).mean() >= A.MEAN_MAX_P[regime], (L, R, P.max(-1).mean())
        if L >= 16:
            top = np.abs(A.logits_ref64(c["qkv"], L)).max()
            assert top > (25 if regime == "sharp3" else 100), (L, top)


def test_onehot_puts_every_query_on_its_own_key():
    for L, R in A.PLAIN_SHAPES:
        c = A.case("onehot", L, R)
        P = A.probs_ref64(c["qkv"], L)
        assert (np.diagonal(P, axis1=-2, axis2=-1) > 1 - 1e-6).all()
        v = np.asarray(c["qkv"][:, 512:], np.float64)
        assert np.abs(c["o"] - v).max() <= 1e-6 * np.abs(v).max()
        # d(q), d(k) are cancellation residue: orders of magnitude below d(v) and below their natural scale
        nq, nk = A.natural_scales(c["qkv"], c["dout"])
        dv = np.abs(c["dqkv"][:, 512:]).max()
        assert np.abs(c["dqkv"][:, :256]).max() < 1e-6 * dv and np.abs(c["dqkv"][:, 256:512]).max() < 1e-6 * dv
        assert np.abs(c["dqkv"][:, :256]).max() < 1e-6 * nq and np.abs(c["dqkv"][:, 256:512]).max() < 1e-6 * nk
        assert A.logits_ref64(c["qkv"], L).max() > 100


@pytest.mark.parametrize("regime", ["equal_large", "flat_q0", "flat_k0"])
def test_equal_logits_give_exactly_uniform_probabilities(regime):
    """All logits of a query are equal (and ~300 in equal_large: exp() of them is inf in float32 and 1e130 in float64 -- uniform only
    with the maximum subtracted); P = 1 / L to float64 rounding, o = the mean of v over the sample, and the true d(q) of equal_large is 0."""
    for L, R in A.PLAIN_SHAPES:
        c = A.case(regime, L, R)
        lg = A.logits_ref64(c["qkv"], L)
        assert np.abs(lg - lg[..., :1]).max() <= 1e-13 * max(np.abs(lg).max(), 1.0)      # (equal up to the summation order of the float64 products)
        if regime == "equal_large":
            assert np.abs(lg).max() > 200
        else:
            assert (lg == 0).all()
        P = A.probs_ref64(c["qkv"], L)
        assert np.abs(P * L - 1).max() < 1e-12
        v = np.asarray(c["qkv"][:, 512:], np.float64).reshape(R, L, 256)
        mean = np.repeat(v.mean(1, keepdims=True), L, axis=1).reshape(R * L, 256)
        assert np.abs(c["o"] - mean).max() < 1e-12
        if regime == "equal_large":
            nq, _ = A.natural_scales(c["qkv"], c["dout"])
            assert np.abs(c["dqkv"][:, :256]).max() < 1e-12 * nq
        if regime == "flat_q0":
            assert (c["dqkv"][:, 256:512] == 0).all()          # d(k) = dS^T q / 8
        if regime == "flat_k0":
            assert (c["dqkv"][:, :256] == 0).all()


def test_zero_operands_give_exact_zero_references():
    for L, R in A.PLAIN_SHAPES:
        c = A.case("zero_v", L, R)
        assert (c["o"] == 0).all() and (c["dqkv"][:, :512] == 0).all() and np.abs(c["dqkv"][:, 512:]).max() > 0
        c = A.case("zero_dout", L, R)
        assert (c["dqkv"] == 0).all() and np.abs(c["o"]).max() > 0


def test_quiet_sample_and_loud_head_are_what_they_say():
    for L, R in A.QUIET_SHAPES:
        for side, ref in (("fwd", "o"), ("bwd", "dqkv")):
            c = A.case("quiet_sample", L, R, side)
            per = np.abs(c[ref]).reshape(R, -1).max(1)
            others = np.delete(per, R // 2)
            assert 2.0 ** -12 < per[R // 2] / others.min() and per[R // 2] / others.max() < 2.0 ** -8, (L, side, per)
        # the quiet sample shares its wave exactly where L < 48
        T = A.wave_tokens(L)
        assert (T // L > 1) == (L < 48)
    for L, R in A.PLAIN_SHAPES:
        c = A.case("loud_head", L, R)
        q = np.abs(c["qkv"][:, :256]).reshape(-1, 4, 64).max((0, 2))
        assert q[2] > 8 * max(q[0], q[1], q[3])
        o = np.abs(c["o"]).reshape(-1, 4, 64).max((0, 2))
        assert o[0] < 2.0 ** -6 * o[1:].min()


def test_no_reference_holds_a_non_finite_value():
    for c in _all_cases():
        for name in ("qkv", "dout", "o", "dqkv", "o32", "dqkv32"):
            assert np.isfinite(c[name]).all(), (c["regime"], c["L"], c["R"], name)


def test_float32_floor_of_every_case_is_below_the_cap():
    """The float32 evaluation's error against float64, in each case's own metric, stays below 2e-5: no bar max(b0, 4 floor) exceeds 8e-5."""
    worst = {}
    for c in _all_cases():
        f = c["floor"]
        vals = [f["o"], f["dq"], f["dk"], f["dv"]] + (f["heads_o"] + sum(f["heads"].values(), []) if c["regime"] == "loud_head" else [])
        assert max(vals) < A.FLOOR_CAP, (c["regime"], c["L"], c["R"], f)
        worst[c["regime"]] = max(worst.get(c["regime"], 0.0), max(vals))
    print("float32 floors, worst per regime: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for b0 in A.B0.values():
        assert A.bar(b0, max(worst.values())) <= 8e-5


def test_split_emulation_fits_every_forward_bar():
    """A kernel with atk.hip's documented arithmetic (per-head power-of-two scales to 2^13, hi / lo fp16 planes, three products, exp2 of
    the scaled logits minus the maximum, P 8192 split into planes) provably fits the forward bar of every case -- per head in loud_head and
    per sample in quiet_sample too -- and gives exact zeros for v == 0."""
    worst = {}
    for c in _all_cases():
        L, R = c["L"], c["R"]
        if not A.wave_tokens(L):
            continue
        em = A.ato_split_emulation(c["qkv"], L)
        assert np.isfinite(em).all()
        e = A.rel(em, c["o"])
        assert e < A.bar(A.B0["ato"], c["floor"]["o"]), (c["regime"], L, R, e)
        worst[c["regime"]] = max(worst.get(c["regime"], 0.0), e)
        if c["regime"] == "loud_head":
            for h, (eh, fh) in enumerate(zip(A.head_errors(em, c["o"]), c["floor"]["heads_o"])):
                assert eh < A.bar(A.B0["ato"], fh), (L, R, h, eh)
        if c["regime"] == "zero_v":
            assert (em == 0).all()
        if c["regime"] == "quiet_sample":
            assert A.sample_errors(em, c["o"], L).max() < A.B0["ato"]
        if c["regime"] in ("equal_large", "flat_q0", "flat_k0"):
            rows = em.reshape(R, L, 256)
            assert (rows == rows[:, :1]).all()                  # equal logits: every row of a sample gets the same bits
    print("emulation of the fp16x3 forward, worst per regime: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_emulation_scale_rule_matches_pow2_scale():
    for mx, want in ((0.0, 1.0), (1.0, 8192.0), (1.999, 8192.0), (2.0, 4096.0), (8192.0, 1.0), (3e-5, 2.0 ** 29), (np.inf, 1.0)):
        assert A.pow2_scale(mx) == want, (mx, A.pow2_scale(mx))
    hi, lo = A.split_planes(np.float32([1.0 + 2.0 ** -12, 3.1415927]), 8192.0)
    assert np.abs(hi + lo - np.float64(np.float32([1.0 + 2.0 ** -12, 3.1415927])) * 8192).max() <= 2.0 ** -22 * 8192 * 4


def test_sharpen_attention_gives_the_network_a_peaked_softmax():
    """synth.sharpen_attention(sd, 6): only the attn1 query / key weights change (x 6); in the float64 oracle the logits of the finest
    level's first transformer block then have a standard deviation above 8 and a mean largest probability above 0.5 (plain weights: ~0.3
    and ~1.9 / L)."""
    S, H = 4, 48
    sd = weights(S, H, False)
    sharp = synth.sharpen_attention(sd, 6.0)
    for k in sd:
        if k.endswith("attn1.to_q.weight") or k.endswith("attn1.to_k.weight"):
            assert np.array_equal(sharp[k], sd[k] * np.float32(6.0))
        else:
            assert np.array_equal(sharp[k], sd[k]) and sharp[k] is not sd[k]
    g = np.load(f"{GOLDEN}/unet2d_h48.npz")
    x, t = g["x"][:4], g["t"][:4]
    stats = {}
    for name, w in (("plain", sd), ("sharp", sharp)):
        u = O.UNetOracle(w, S, H, dtype=np.float64)
        lat = np.tile(u.encode_scene(g["cloud"])[None], (x.shape[0], 1))
        _, (tape, _, _) = u.forward_no_energy(x, t, lat, return_tape=True)
        _, q, k, _, P = tape[2][1][0][:5]                          # downs.0.3, transformer block 0
        assert P.shape[-1] == H
        stats[name] = (((q @ k.transpose(0, 1, 3, 2)) * 0.125).std(), P.max(-1).mean())
    print(f"finest-level attention, (logit std, mean max P): plain {stats['plain'][0]:.2f} {stats['plain'][1]:.3f}  gain 6 {stats['sharp'][0]:.2f} {stats['sharp'][1]:.3f}")
    assert stats["plain"][0] < 1 and stats["plain"][1] < 3.0 / H
    assert stats["sharp"][0] > 8 and stats["sharp"][1] > 0.5
