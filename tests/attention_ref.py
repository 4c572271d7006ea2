"""References and case tables for the attention kernels at sharp, flat and unevenly scaled softmax (numpy / torch on the CPU, no GPU).

Layout everywhere: qkv (R L, 768) = [q | k | v], each 4 heads x 64, samples of L consecutive tokens; d(o) (R L, 256); softmax(q k^T / 8) v
per head and sample (layers_attention_mini.py:101-127) -- the layout of test_atb_attention_backward_against_float64_autograd.

  attn_ref64 / attn_grad_ref64   float64 truth (forward in numpy with the maximum subtracted, backward by float64 autograd)
  attn_fp32                      the same two in float32 with torch on the CPU: the yardstick of the bars (shares no code with the kernels)
  ato_split_emulation            numpy model of the forward arithmetic of atk.hip: the second opinion when a kernel exceeds a bar
  make_case                      the regimes of REGIMES at the shapes of FUSED_SHAPES / PLAIN_SHAPES
  rel / natural_scales / bar     the metrics and the bar max(b0, 4 floor) shared by the host and the GPU tests

Out of scope: non-finite inputs (the kernels' fmaxf drops a NaN that these references keep) and operand maxima below about 2^-100 (the
product of the two power-of-two operand scales overflows there, and the true logits are zero anyway)."""
import numpy as np
import torch

HEADS, DH = 4, 64
LOG2E = 1.4426950408889634

# (L, R) -- fused kernels (atk / atb / atl): L = 32 is the only length on the two-group path (wave tile 32), the others are on the three-group
# path (wave tile 48); (6, 9): eight samples in one wave, one in the next; (3, 50), (1, 20): the last wave partly empty
FUSED_SHAPES = [(48, 4), (32, 3), (16, 5), (6, 9), (3, 50), (1, 20)]
# plain attention.hip kernels: the same plus lengths the fused kernels refuse
PLAIN_SHAPES = FUSED_SHAPES + [(64, 2), (40, 3), (7, 5), (5, 7)]
QUIET_SHAPES = [(16, 5), (6, 9), (48, 4)]          # (48, 4): the control -- the quiet sample owns its wave
POW2_SHAPES = [(16, 5), (48, 4)]

ACCURACY_REGIMES = ["sharp3", "sharp6", "onehot", "equal_large", "flat_q0", "flat_k0", "loud_head"]
SATURATED = ("onehot", "equal_large")              # d(q), d(k) are cancellation residue: measured on their natural scale
REGIMES = ACCURACY_REGIMES + ["zero_v", "zero_dout", "quiet_sample"]
MEAN_MAX_P = {"sharp3": 0.8, "sharp6": 0.95}       # lower bounds of the mean over queries of max_k P, at L >= 16

QUIET_SHIFT = 2.0 ** -10
FLOOR_CAP = 2e-5                                   # every float32 floor stays below this, so no bar exceeds 8e-5
B0 = {"attention": 3e-6, "attention_bwd": 5e-6, "ato": 3e-6, "atb": 3e-6, "abl": 4e-6}      # the entries' bars in test_gpu_ops.py


def wave_tokens(L):
    """Tokens a sample-owning wave holds (ato_applicable): 48 where L divides 48, else 32 where it divides 32, else 0 (refused)."""
    return 48 if 48 % L == 0 else (32 if 32 % L == 0 else 0)


def case_seed(regime, L, R):
    return 1009 * REGIMES.index(regime) + 31 * L + R


def make_case(regime, L, R, seed=None, side="fwd"):
    """qkv (R L, 768) and dout (R L, 256), float32.  `side` matters for quiet_sample only: "fwd" scales the quiet sample's v, "bwd" its d(o)."""
    assert regime in REGIMES, regime
    g = np.random.Generator(np.random.PCG64([case_seed(regime, L, R) if seed is None else seed, 17]))
    M = R * L
    q = g.standard_normal((M, 256)); k = g.standard_normal((M, 256))
    v = g.standard_normal((M, 256)) * 0.4 + 0.1
    dout = g.standard_normal((M, 256))
    noise = g.standard_normal((M, 256))
    if regime in ("sharp3", "sharp6"):
        gain = 3.0 if regime == "sharp3" else 6.0
        q *= gain; k *= gain
    elif regime == "onehot":
        q *= 2.0
        k = 8.0 * q + 0.01 * noise
    elif regime == "equal_large":
        q *= 30.0
        k = np.repeat(3.0 * g.standard_normal((R, 1, 256)), L, axis=1).reshape(M, 256)
    elif regime == "flat_q0":
        q[:] = 0.0; k *= 1.3
    elif regime == "flat_k0":
        k[:] = 0.0; q *= 1.3
    elif regime == "zero_v":
        q *= 1.3; k *= 1.3; v[:] = 0.0
    elif regime == "zero_dout":
        q *= 1.3; k *= 1.3; dout[:] = 0.0
    elif regime == "quiet_sample":
        q *= 1.3; k *= 1.3
        s = slice((R // 2) * L, (R // 2 + 1) * L)
        if side == "fwd":
            v[s] *= QUIET_SHIFT
        else:
            dout[s] *= QUIET_SHIFT
    elif regime == "loud_head":
        q *= 0.4; k *= 0.4
        q[:, 128:192] *= 16.0; k[:, 128:192] *= 16.0
        v[:, 0:64] *= 2.0 ** -8
    return np.concatenate([q, k, v], axis=1).astype(np.float32), dout.astype(np.float32)


def heads_of(x, L):
    """(R L, 256) -> (R, 4, L, 64)"""
    return np.asarray(x).reshape(-1, L, HEADS, DH).transpose(0, 2, 1, 3)


def probs_ref64(qkv, L):
    """P (R, 4, L, L) in float64, the row maximum subtracted."""
    x = np.asarray(qkv, np.float64)
    q, k = heads_of(x[:, :256], L), heads_of(x[:, 256:512], L)
    s = (q @ k.transpose(0, 1, 3, 2)) * 0.125
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def logits_ref64(qkv, L):
    x = np.asarray(qkv, np.float64)
    return (heads_of(x[:, :256], L) @ heads_of(x[:, 256:512], L).transpose(0, 1, 3, 2)) * 0.125


def attn_ref64(qkv, L):
    """o (R L, 256), float64."""
    v = heads_of(np.asarray(qkv, np.float64)[:, 512:], L)
    return (probs_ref64(qkv, L) @ v).transpose(0, 2, 1, 3).reshape(-1, 256)


def _torch_attention(x, L):
    M = x.shape[0]
    y = x.reshape(M // L, L, 3, HEADS, DH)
    q, k, v = y[:, :, 0].transpose(1, 2), y[:, :, 1].transpose(1, 2), y[:, :, 2].transpose(1, 2)
    # (the logits through a plain float32 matrix product on purpose: summing them pairwise instead -- an elementwise product and
    # torch's sum -- is more accurate than the serial fp32 accumulation of attention.hip itself, and puts 4 x that floor below the exact-fp32
    # kernel's own error in loud_head.  The price: the float32 floor of equal_large, whose logits of ~300 then differ by an ulp or
    # two from key to key, depends on the CPU's GEMM -- 3e-7 to 1.3e-5 seen, under the 2e-5 cap either way.)
    return (torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1) @ v).transpose(1, 2).reshape(M, 256)


def _torch_both(qkv, dout, L, dtype):
    x = torch.from_numpy(np.ascontiguousarray(qkv)).to(dtype).requires_grad_(True)
    o = _torch_attention(x, L)
    (gr,) = torch.autograd.grad(o, x, torch.from_numpy(np.ascontiguousarray(dout)).to(dtype))
    return o.detach().numpy(), gr.numpy()


def attn_grad_ref64(qkv, dout, L):
    """d(qkv) (R L, 768), float64 autograd."""
    return _torch_both(qkv, dout, L, torch.float64)[1]


def attn_fp32(qkv, dout, L):
    """(o, dqkv) evaluated in float32 with torch on the CPU: what plain single precision gives on the case."""
    return _torch_both(qkv, dout, L, torch.float32)


# ---- metrics ----------------------------------------------------------------------------------------------------------------------
def rel(a, b, scale=None):
    """max |a - b| over max |b| (util.rel), or over a given natural scale."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max() if scale is None else scale, 1e-30))


def natural_scales(qkv, dout):
    """Scales of d(q) and d(k) where the true gradients are cancellation residue: max|dout| max|v| max|k| / 8, and the same with max|q|."""
    m = lambda x: float(np.abs(np.asarray(x, np.float64)).max())
    c = m(dout) * m(qkv[:, 512:]) / 8.0
    return c * m(qkv[:, 256:512]), c * m(qkv[:, :256])


BLOCKS = (("dq", slice(0, 256)), ("dk", slice(256, 512)), ("dv", slice(512, 768)))


def grad_errors(regime, got, ref, qkv, dout):
    """{"dq", "dk", "dv"} -> error of `got` against `ref` in the regime's metric."""
    nq, nk = natural_scales(qkv, dout)
    sat = regime in SATURATED
    return {"dq": rel(got[:, :256], ref[:, :256], nq if sat else None),
            "dk": rel(got[:, 256:512], ref[:, 256:512], nk if sat else None),
            "dv": rel(got[:, 512:], ref[:, 512:])}


def head_errors(got, ref):
    """Per head: error over columns 64 h .. 64 h + 63 relative to that head's own maximum."""
    return [rel(got[:, 64 * h:64 * h + 64], ref[:, 64 * h:64 * h + 64]) for h in range(HEADS)]


def sample_errors(got, ref, L):
    """Per sample: error relative to the sample's own largest reference entry."""
    a = np.asarray(got, np.float64).reshape(-1, L * got.shape[1]); b = np.asarray(ref, np.float64).reshape(a.shape)
    return np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1e-300)


def bar(b0, floor):
    """max(b0, 4 floor): b0 the entry's existing bar, floor the float32 evaluation's error in the same metric; 4 = the two significand
    bits the three-product fp16 split gives up against fp32 (22 against 24).  Never derived from a kernel's output."""
    return max(b0, 4.0 * floor)


_CASES = {}


def case(regime, L, R, side="fwd"):
    """Everything the tests share about a case, computed once per process and left unchanged: inputs, float64 references, the float32
    evaluation and its errors (`floor`) in the regime's metric."""
    key = (regime, L, R, side)
    if key not in _CASES:
        qkv, dout = make_case(regime, L, R, side=side)
        o64, g64 = _torch_both(qkv, dout, L, torch.float64)
        o64 = attn_ref64(qkv, L)
        o32, g32 = attn_fp32(qkv, dout, L)
        floor = {"o": rel(o32, o64)}
        floor.update(grad_errors(regime, g32, g64, qkv, dout))
        floor["heads_o"] = head_errors(o32, o64)
        floor["heads"] = {n: head_errors(g32[:, s], g64[:, s]) for n, s in BLOCKS}
        for a in (qkv, dout, o64, g64):
            a.setflags(write=False)
        _CASES[key] = dict(regime=regime, L=L, R=R, qkv=qkv, dout=dout, o=o64, dqkv=g64, o32=o32, dqkv32=g32, floor=floor)
    return _CASES[key]


# ---- numpy model of atk.hip's forward arithmetic -----------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, np.float32)


def pow2_scale(mx, target=13):
    """atkmma.h pow2_scale: 2^(target - floor(log2 mx)) with the exponent clamped to a normal float; 1 for mx == 0 / non-finite."""
    mx = np.float32(mx)
    if not (mx > 0 and mx < 3.0e38):
        return np.float32(1.0)
    eb = int((mx.view(np.uint32) >> 23) & 0xFF)
    sb = min(max(254 + target - eb, 1), 254)
    return np.uint32(sb << 23).view(np.float32)


def split_planes(x, s):
    """x s = hi + lo: hi = fp16(x s), lo = fp16(x s - hi) (the residual formed exactly, as v_fma_mix does), both returned as float64."""
    xs = np.asarray(x, np.float64) * np.float64(s)                   # exact: a power of two (and P 8192) times a float32
    with np.errstate(over="ignore"):
        hi = xs.astype(np.float32).astype(np.float16).astype(np.float64)
        lo = (xs - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def _x3(ah, al, bh, bl):
    """The three products hi hi + hi lo + lo hi, accumulated (here in float64) and rounded to float32."""
    return _f32(ah @ bh + ah @ bl + al @ bh)


def ato_split_emulation(qkv, L):
    """o (R L, 256) as atk.hip's attention part forms it, as float64 values of float32 results: per wave (48 or 32 consecutive tokens) and
    head, power-of-two scales that put max|q|, max|k|, max|v| into [2^13, 2^14); hi / lo fp16 planes; S = (kh ql + kl qh + kh qh) ssc
    with ssc = 0.125 log2(e) / (sq sk); exp2(S - max) over the query's own sample; P 8192 / sum split into planes; o = (vh pl + vl ph +
    vh ph) / (sv 8192).  The model does not reproduce the MFMA's summation order (float64 sums rounded once), so it agrees with the
    kernel to float32 rounding, not bitwise."""
    qkv = _f32(qkv)
    M = qkv.shape[0]
    T = wave_tokens(L)
    assert T and M % L == 0
    out = np.zeros((M, 256), np.float64)
    for w0 in range(0, M, T):
        rows = slice(w0, min(w0 + T, M))
        for h in range(HEADS):
            q, k, v = (qkv[rows, 256 * i + 64 * h:256 * i + 64 * h + 64] for i in range(3))
            sq, sk, sv = (pow2_scale(np.abs(x).max()) for x in (q, k, v))
            qh, ql = split_planes(q, sq); kh, kl = split_planes(k, sk); vh, vl = split_planes(v, sv)
            ssc = np.float32(np.float32(0.125 * LOG2E) / np.float32(sq * sk))
            so = np.float32(1.0) / np.float32(sv * np.float32(8192.0))
            n = q.shape[0]
            for s0 in range(0, n, L):
                s = slice(s0, s0 + L)
                st = _f32(_x3(qh[s], ql[s], kh[s].T, kl[s].T) * ssc)                         # [query][key]
                e = _f32(np.exp2((st - st.max(1, keepdims=True)).astype(np.float64)))
                tot = e[:, 0].copy()
                for j in range(1, L):
                    tot = _f32(tot + e[:, j])
                inv = _f32(np.float32(8192.0) * _f32(1.0 / tot.astype(np.float64)))
                ph, pl = split_planes(_f32(e * inv[:, None]), 1.0)
                out[w0 + s0:w0 + s0 + L, 64 * h:64 * h + 64] = _f32(_x3(ph, pl, vh[s], vl[s]) * so)
    return out
