"""References, row / sample regimes and metrics for the fused token- and sample-owning kernels (numpy / torch on the CPU, no GPU):
ffx.hip / ffx16.hip, tkl.hip / tkl16.hip / tklb_kernel, tkw.hip / tkc.hip, and the stand-alone LayerNorm and GEGLU kernels.

  *_eval(case, dtype)       one torch-CPU evaluation per composition; float64 = the truth of the LayerNorm compositions, float32 = the
                            yardstick of the bars everywhere (plain single precision; shares no code with the kernels)
  tkw_fwd_ref64 / tkw_bwd_ref64   the float64 formulas of test_gpu_ops.py (_conv5_f64, _mish64, _mish_grad64: imported, not rewritten)
  ln_rows / LN_REGIMES      the row regimes of the 256-wide LayerNorm operands
  GN_REGIMES                the sample regimes of the GroupNorm kernels (they act on the stash c = conv + bias per sample and group)
  rel / rel_rows / bar      max |err| / max |ref| tensor-wide and per row (token or sample), and the bar max(b0, 4 floor)
  operand_scale / guard_state     the delayed-scale rule (tokmma.h scale_of) and what core.h's record_amax_block_guarded promises

Natural scale of the LayerNorm-backward outputs (dz1 of ffx, the output of tklb, ramp_op_layernorm_bwd): all three ADD the gradient that
bypasses the norm (dz / add) to the LayerNorm backward, so on const / flat / loud rows, where the backward term itself is cancellation
residue or tiny, the row's own largest reference entry (bypass included) is the natural scale, and rel_rows uses it unchanged.

Natural scale of a sample's GroupNorm means (per sample only; tensor-wide they keep max |mean|): a mean is a sum with cancellation, its
error is that of the values averaged, so a sample's eight means are measured against max over its groups of |mean| + standard deviation.

Out of scope: non-finite inputs except the single NaN of the guard test; operand maxima outside float16's reach after scaling are the
guard's business (guard_state), not an accuracy case."""
import numpy as np
import torch
import torch.nn.functional as F

from test_gpu_ops import _conv5_f64, _mish64, _mish_grad64

FLOOR_CAP = 2e-5                                   # every float32 floor stays below this, so no bar exceeds 8e-5
QUIET_SHIFT = 2.0 ** -10
QUIET_BOUND = 2.0 ** -17                           # the documented per-row bound of one scale per tensor (test_abl_per_sample_accuracy_...)
EPS = 1e-5
# the entries' bars in test_gpu_ops.py
B0 = {"ffx": 3e-6, "tkl": 3e-6, "tklb": 3e-6, "tkc": 3e-6, "tkw_stash": 3e-6, "tkw_stats": 3e-6, "tkw_y": 5e-6, "tkw_dx": 5e-6,
      "layernorm": 2e-6, "layernorm_bwd": 3e-6, "geglu": 2e-6}

ROW_KINDS = ["gauss", "offset", "flat", "const", "spike", "quiet", "loud"]
LN_REGIMES = ROW_KINDS + ["mixed"]
GN_REGIMES = ["gauss", "offset", "flat", "outlier_group", "saturated", "quiet_sample", "mixed"]
LN_M = [293, 4173]                                 # half tiles + a partial last tile + 16-token waves; many tiles
TKL_FORMS = [(256, False, 3), (768, True, 0), (96, False, 1)]      # N, LayerNorm in front, epilogue (1 residual, 2 row-variant constant)

# GroupNorm kernels, one shape per kernel path: name -> (L, C_in, C_out, samples, split).  Sample counts leave the last tile (tkw: 96 tokens)
# or the last wave / block (tkc: a wave holds 48, 32 or 64 tokens) partly empty
GN_SHAPES = {
    "tkw256": (6, 256, 256, 21, 0), "tkw128": (12, 128, 128, 11, 0), "tkw_split": (6, 512, 128, 21, 256), "tkw512": (6, 256, 512, 19, 0),
    "tkc32": (48, 32, 32, 7, 0), "tkc64": (24, 64, 64, 11, 0), "tkc_ng4": (64, 32, 32, 7, 0), "tkc_l32": (32, 32, 64, 7, 0),
}


def hash_str(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s))


def _gen(*key):
    return np.random.Generator(np.random.PCG64([hash_str(k) if isinstance(k, str) else int(k) for k in key]))


def _t(a, dtype):
    return torch.tensor(np.ascontiguousarray(a)).to(dtype)         # (a copy: the cached case arrays are read-only)


# ---- row regimes of the LayerNorm operands -------------------------------------------------------------------------------------------
def _row_kind(kind, z, rows):
    """z: standard normal (n, 256); rows: the rows' indices in the tensor (the spike's channel depends on them)."""
    if kind == "gauss":
        return 1.3 * z + 0.2
    if kind == "offset":                           # |mean| rstd ~ 40
        return 4.0 + 0.1 * z
    if kind == "flat":                             # variance ~ 1e-7 << eps: rstd is set by eps
        return 0.02 + 3e-4 * z
    if kind == "const":                            # variance exactly 0
        return np.full_like(z, 0.7)
    if kind == "spike":                            # one channel at 300 in a Gaussian row
        x = 1.3 * z + 0.2
        x[np.arange(len(rows)), (7 * rows) % 256] = 300.0
        return x
    if kind == "quiet":
        return (1.3 * z + 0.2) * QUIET_SHIFT
    if kind == "loud":
        return (1.3 * z + 0.2) / QUIET_SHIFT
    raise ValueError(kind)


def ln_rows(regime, M, g):
    """(M, 256) float32 in the regime; `mixed`: row i takes ROW_KINDS[i % 7]."""
    z = g.standard_normal((M, 256))
    if regime != "mixed":
        return _row_kind(regime, z, np.arange(M)).astype(np.float32)
    x = np.empty((M, 256))
    for i, kind in enumerate(ROW_KINDS):
        rows = np.arange(i, M, 7)
        x[rows] = _row_kind(kind, z[rows], rows)
    return x.astype(np.float32)


def row_kind_of(regime, M):
    """The kind of every row of a tensor in `regime`."""
    return [ROW_KINDS[i % 7] if regime == "mixed" else regime for i in range(M)]


# ---- metrics ----------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """max |a - b| over max |b| (util.rel)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def row_errors(got, ref, rows=None, scale=None):
    """Per row (rows = number of rows the arrays are folded to; default: the first axis): max |err| over the row's own max |ref|, or over
    a given natural scale per row.  A row whose reference is all zero gives 0 where `got` is exactly zero there and inf otherwise."""
    a = np.asarray(got, np.float64); b = np.asarray(ref, np.float64)
    n = a.shape[0] if rows is None else rows
    a = a.reshape(n, -1); b = b.reshape(n, -1)
    err = np.abs(a - b).max(1); top = np.abs(b).max(1) if scale is None else np.asarray(scale, np.float64)
    out = np.where(top > 0, err / np.where(top > 0, top, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, out)


def rel_rows(got, ref, rows=None, scale=None):
    return float(row_errors(got, ref, rows, scale).max())


def bar(b0, floor):
    """max(b0, 4 floor): b0 the entry's bar in test_gpu_ops.py, floor the float32 evaluation's error in the same metric; 4 = the two
    significand bits the three-product fp16 split gives up against fp32.  Never derived from a kernel's output."""
    return max(b0, 4.0 * floor)


def floors(ref32, ref64, names, rows=None, scale=None):
    """{name: (tensor-wide, per-row)} errors of the float32 evaluation; scale: {name: per-row natural scale}."""
    return {n: (rel(ref32[n], ref64[n]), rel_rows(ref32[n], ref64[n], rows, (scale or {}).get(n))) for n in names}


# ---- the delayed operand scale and its guard ----------------------------------------------------------------------------------------------
def operand_scale(prev):
    """tokmma.h scale_of: 2^(5 - floor(log2 prev)) with the exponent field clamped to [1, 254]; 1 for prev <= 0 (the operand runs unscaled)."""
    prev = np.float32(prev)
    if not prev > 0:
        return 1.0
    eb = int((prev.view(np.uint32) >> 23) & 0xFF)
    return float(np.uint32(min(max(259 - eb, 1), 254) << 23).view(np.float32))


K_OVERFLOW = -11      # prev = max 2^k: the scaled maximum is m 2^(5 - k), m in [1, 2) (tokmma.h:28 sb = 259 - eb) -> >= 2^16 > 60000 for k <= -11 (core.h:69)
K_SHRUNK = 9          # ... and < 2^(6 - k) <= 2^-3 for k >= 9 (core.h:75)


def guard_state(rowmax, prev):
    """What record_amax_block_guarded (core.h:65-77) promises about the flag, from the float64 operand's per-row maxima: "must" -- an element
    reaches 60000 after scaling, or the whole tensor's maximum falls below 2^-3; "never" -- every nonzero row lies inside the window, so every
    wave and block does, however the rows are grouped; "either" in between (the kernels judge a wave's or a block's rows together) and within
    1e-4 of a threshold (the kernel's maximum is a float32 one)."""
    m = np.asarray(rowmax, np.float64)
    if np.isnan(m).any():
        return "must"
    m = m[m > 0] * operand_scale(prev)
    if m.size == 0:
        return "never"
    if m.max() >= 60000.0 * (1 + 1e-4) or m.max() < 0.125 * (1 - 1e-4):
        return "must"
    if m.max() < 60000.0 * (1 - 1e-4) and m.min() >= 0.125 * (1 + 1e-4):
        return "never"
    return "either"


def rowmax(x, rows=None):
    a = np.abs(np.asarray(x, np.float64))
    return a.reshape(a.shape[0] if rows is None else rows, -1).max(1)


# ---- feed-forward: z2 = z1 + W2 (a gelu(g)) + b2, [a | g] = W1 LN(z1) + b1, and dz1 (ffx / ffx16) -----------------------------------------
GATE_GAIN = 2.6       # gate half of W1 x 2.6: g ~ N(0, 2.6^2), +-12 over the 3e5 gate arguments of M = 293


def ffx_params(gate):
    g = _gen("ffx", int(gate))
    p = dict(W1=g.standard_normal((2048, 256)) / 16, b1=0.1 * g.standard_normal(2048), W2=g.standard_normal((256, 1024)) / 32,
             b2=0.1 * g.standard_normal(256), g=1 + 0.1 * g.standard_normal(256), b=0.1 * g.standard_normal(256))
    if gate:          # both Phi tails in play; LN beta = 0 and no bias on the "a" half, so an all-zero row of z1 has a = 0 exactly
        p["W1"][1024:] *= GATE_GAIN
        p["b"][:] = 0.0
        p["b1"][:1024] = 0.0
    return {k: v.astype(np.float32) for k, v in p.items()}


def ffx_eval(z1, dz, p, dtype):
    zz = _t(z1, dtype).requires_grad_(True)
    y = F.layer_norm(zz, (256,), _t(p["g"], dtype), _t(p["b"], dtype), EPS)
    ag = y @ _t(p["W1"], dtype).T + _t(p["b1"], dtype)
    ag.retain_grad()
    hg = ag[:, :1024] * F.gelu(ag[:, 1024:])
    z2 = zz + hg @ _t(p["W2"], dtype).T + _t(p["b2"], dtype)
    z2.backward(_t(dz, dtype))
    return dict(z2=z2.detach().numpy(), dz1=zz.grad.numpy(), y=y.detach().numpy(), hg=hg.detach().numpy(), dag=ag.grad.numpy(),
                gate=ag.detach()[:, 1024:].numpy())


_CASES = {}


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _freeze(v)
    return c


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = _freeze(make())
    return _CASES[key]


def ffx_case(regime, M):
    """regime: one of LN_REGIMES (rows of z1), "gate" (Gaussian rows, every third one all zero, the gate half of W1 x GATE_GAIN), or
    "quiet_shared" / "quiet_own" (Gaussian z1; rows of dz x 2^-10: every 7th row, resp. the whole second 128-token tile)."""
    def make():
        g = _gen("ffx", regime, M)
        gate = regime == "gate"
        z1 = ln_rows("gauss" if gate or regime.startswith("quiet_") else regime, M, g)
        dz = (0.7 * g.standard_normal((M, 256))).astype(np.float32)
        quiet = np.zeros(M, bool)
        if gate:
            z1[::3] = 0.0
        if regime.startswith("quiet_"):
            quiet = quiet_rows(regime, M)
            dz[quiet] *= np.float32(QUIET_SHIFT)
        p = ffx_params(gate)
        r64, r32 = ffx_eval(z1, dz, p, torch.float64), ffx_eval(z1, dz, p, torch.float32)
        return dict(regime=regime, M=M, z1=z1, dz=dz, p=p, ref=r64, ref32=r32, quiet=quiet, floor=floors(r32, r64, ("z2", "dz1")),
                    sites=[rowmax(r64["y"]), rowmax(r64["hg"]), rowmax(dz), rowmax(r64["dag"])])
    return _cached(("ffx", regime, M), make)


def quiet_rows(regime, M):
    """quiet_shared: every 7th row from row 3 on -- quiet rows inside every 16- and 32-token wave group, the partial last tile included;
    quiet_own: rows 128 .. 255, a whole token tile (the control: nothing loud shares its waves)."""
    q = np.zeros(M, bool)
    if regime == "quiet_shared":
        q[3::7] = True
    else:
        q[128:256] = True
    return q


# ---- LN -> linear with bias / residual / row-variant constant (tkl / tkl16) ---------------------------------------------------------------
TKL_L, TKL_NVAR = 6, 3


def tkl_eval(c, dtype):
    x = _t(c["X"], dtype)
    if c["ln"]:
        x = F.layer_norm(x, (256,), _t(c["g"], dtype), _t(c["b"], dtype), EPS)
    y = x @ _t(c["W"], dtype).T
    if c["epi"]:
        y = y + _t(c["bias"], dtype)
    if c["epi"] & 1:
        y = y + _t(c["resid"], dtype)
    if c["epi"] & 2:
        y = y + _t(c["rowbias"], dtype)[torch.from_numpy(c["rowvar"]).long()[torch.arange(c["M"]) // TKL_L]]
    return dict(Y=y.numpy(), op=x.numpy())


def tkl_case(regime, M, N, ln, epi):
    """regime: LN_REGIMES on X, or "quiet_shared" / "quiet_own" (Gaussian X with the quiet rows of quiet_rows x 2^-10)."""
    def make():
        g = _gen("tkl", regime, M, N, int(ln), epi)
        q = regime.startswith("quiet_")
        X = ln_rows("gauss" if q else regime, M, g)
        quiet = quiet_rows(regime, M) if q else np.zeros(M, bool)
        X[quiet] *= np.float32(QUIET_SHIFT)
        c = dict(regime=regime, M=M, N=N, ln=ln, epi=epi, X=X, quiet=quiet, W=(g.standard_normal((N, 256)) / 16).astype(np.float32),
                 bias=(0.3 * g.standard_normal(N)).astype(np.float32), resid=g.standard_normal((M, N)).astype(np.float32),
                 rowbias=(0.5 * g.standard_normal((TKL_NVAR, N))).astype(np.float32),
                 rowvar=(np.arange((M + TKL_L - 1) // TKL_L) % TKL_NVAR).astype(np.int32),
                 g=(1 + 0.1 * g.standard_normal(256)).astype(np.float32), b=(0.1 * g.standard_normal(256)).astype(np.float32))
        c["ref"], c["ref32"] = tkl_eval(c, torch.float64), tkl_eval(c, torch.float32)
        c["floor"] = floors(c["ref32"], c["ref"], ("Y",))
        c["sites"] = [rowmax(c["ref"]["op"])]
        return c
    return _cached(("tkl", regime, M, N, ln, epi), make)


# ---- d(qkv) Wqkv^T + LayerNorm backward + add (tklb) ---------------------------------------------------------------------------------------
def tklb_eval(c, dtype):
    zz = _t(c["z"], dtype).requires_grad_(True)
    qkv = F.layer_norm(zz, (256,), _t(c["g"], dtype), _t(c["b"], dtype), EPS) @ _t(c["Wqkv"], dtype).T
    (dz,) = torch.autograd.grad(qkv, zz, _t(c["dqkv"], dtype))
    return dict(out=(dz + _t(c["add"], dtype)).numpy())


def tklb_case(regime, M):
    """regime: LN_REGIMES on z, or "quiet_shared" / "quiet_own" (Gaussian z; the quiet rows of d(qkv) x 2^-10 and add = 0, so that a quiet
    row's output is quiet too)."""
    def make():
        g = _gen("tklb", regime, M)
        q = regime.startswith("quiet_")
        z = ln_rows("gauss" if q else regime, M, g)
        dqkv = (0.7 * g.standard_normal((M, 768))).astype(np.float32)
        add = g.standard_normal((M, 256)).astype(np.float32)
        quiet = quiet_rows(regime, M) if q else np.zeros(M, bool)
        if q:
            dqkv[quiet] *= np.float32(QUIET_SHIFT); add[:] = 0.0
        c = dict(regime=regime, M=M, z=z, dqkv=dqkv, add=add, quiet=quiet, Wqkv=(g.standard_normal((768, 256)) / 16).astype(np.float32),
                 g=(1 + 0.1 * g.standard_normal(256)).astype(np.float32), b=(0.1 * g.standard_normal(256)).astype(np.float32))
        c["ref"], c["ref32"] = tklb_eval(c, torch.float64), tklb_eval(c, torch.float32)
        c["floor"] = floors(c["ref32"], c["ref"], ("out",))
        c["sites"] = [rowmax(dqkv)]
        return c
    return _cached(("tklb", regime, M), make)


# ---- plain LayerNorm and GEGLU, forward and backward -------------------------------------------------------------------------------------
def layernorm_eval(c, dtype):
    xx = _t(c["x"], dtype).requires_grad_(True)
    y = F.layer_norm(xx, (256,), _t(c["g"], dtype), _t(c["b"], dtype), EPS)
    (dx,) = torch.autograd.grad(y, xx, _t(c["dy"], dtype))
    return dict(y=y.detach().numpy(), dx=(dx + _t(c["add"], dtype)).numpy())


def layernorm_case(regime, M):
    def make():
        g = _gen("layernorm", regime, M)
        c = dict(regime=regime, M=M, x=ln_rows(regime, M, g), dy=g.standard_normal((M, 256)).astype(np.float32),
                 add=g.standard_normal((M, 256)).astype(np.float32),
                 g=(1 + 0.1 * g.standard_normal(256)).astype(np.float32), b=(0.1 * g.standard_normal(256)).astype(np.float32))
        c["ref"], c["ref32"] = layernorm_eval(c, torch.float64), layernorm_eval(c, torch.float32)
        c["floor"] = floors(c["ref32"], c["ref"], ("y", "dx"))
        return c
    return _cached(("layernorm", regime, M), make)


GEGLU_F = 1024


def geglu_eval(c, dtype):
    ag = _t(c["ag"], dtype).requires_grad_(True)
    h = ag[:, :GEGLU_F] * F.gelu(ag[:, GEGLU_F:])
    (dag,) = torch.autograd.grad(h, ag, _t(c["dh"], dtype))
    return dict(h=h.detach().numpy(), dag=dag.numpy())


def geglu_case(regime, M=37):
    """regime "gauss": [a | g] = 2 N(0, 1) (test_geglu_fwd_bwd); "tails": g = 4 N(0, 1), so +-12 and beyond, and every third row's "a" half 0."""
    def make():
        g = _gen("geglu", regime, M)
        ag = (2.0 * g.standard_normal((M, 2 * GEGLU_F))).astype(np.float32)
        if regime == "tails":
            ag[:, GEGLU_F:] *= 2.0
            ag[::3, :GEGLU_F] = 0.0
        c = dict(regime=regime, M=M, ag=ag, dh=g.standard_normal((M, GEGLU_F)).astype(np.float32))
        c["ref"], c["ref32"] = geglu_eval(c, torch.float64), geglu_eval(c, torch.float32)
        c["floor"] = floors(c["ref32"], c["ref"], ("h", "dag"))
        return c
    return _cached(("geglu", regime, M), make)


# ---- conv5 + bias -> GroupNorm(8) -> Mish + time bias / residual (tkw / tkc forward) --------------------------------------------------------
SAMPLE_KINDS = ["gauss", "flat", "quiet"]                  # `mixed`: sample r takes SAMPLE_KINDS[r % 3]; the quiet samples sit 2^-10 below the operand's maximum
FLAT_DY = 2.0 ** -8                                         # `mixed`, backward: dY of the flat samples, whose rstd = eps^-1/2 = 2^8.3 would otherwise set the operand's maximum
SATURATION = 15.0                                           # gamma, beta x 15: mish's argument ~ 15 N(0, 1) + 3, about [-60, 60]
OFFSET_KAPPA = 40.0


def to_window(mx):
    """The power of two that puts a maximum into [2^5, 2^6), the delayed scale's target (tokmma.h scale_from).  The cases with quiet samples are
    built with their operand's maximum there, so that the unscaled launch (scale 1) meets the premise of the documented 2^-17 bound -- a scale
    fresh from the tensor's maximum -- exactly as the scaled one does."""
    return 2.0 ** (5 - int(np.floor(np.log2(mx))))


def special_samples(R):
    """The flat / quiet samples of a case: one in the first (full) tile / wave, one in the last (partly empty) one."""
    return [1, R - 1]


def _conv_torch(A, W, L, direction, dtype):
    """_conv5_f64's convolution with torch: A (M, K), W (5, N, K)."""
    M, K = A.shape
    x = _t(A, dtype).reshape(M // L, L, K).transpose(1, 2)
    w = _t(W if direction == 1 else W[::-1], dtype).permute(1, 2, 0)
    return F.conv1d(x, w, padding=2).transpose(1, 2).reshape(M, W.shape[1])


def tkw_fwd_ref64(c):
    """The float64 formulas of test_tkw_conv_groupnorm_mish_forward."""
    L, R, N = c["L"], c["R"], c["N"]
    st = _conv5_f64(c["X"].astype(np.float64), c["W"].astype(np.float64), L, 1) + c["bias"]
    cg = st.reshape(R, L, 8, N // 8)
    mean = cg.mean(axis=(1, 3)); var = cg.var(axis=(1, 3)); rstd = 1.0 / np.sqrt(var + EPS)
    nrm = ((cg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(R * L, N) * c["gam"] + c["bet"]
    return dict(stash=st, mean=mean, rstd=rstd, var=var, arg=nrm, y=_mish64(nrm) + c["tb"] + c["res"])


def tkw_fwd_eval(c, dtype):
    L, R, N = c["L"], c["R"], c["N"]
    st = _conv_torch(c["X"], c["W"], L, 1, dtype) + _t(c["bias"], dtype)
    cg = st.reshape(R, L, 8, N // 8)
    mean = cg.mean(dim=(1, 3)); var = cg.var(dim=(1, 3), unbiased=False); rstd = 1.0 / torch.sqrt(var + EPS)
    nrm = ((cg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(R * L, N) * _t(c["gam"], dtype) + _t(c["bet"], dtype)
    y = F.mish(nrm) + _t(c["tb"], dtype) + _t(c["res"], dtype)
    return dict(stash=st.numpy(), mean=mean.numpy(), rstd=rstd.numpy(), y=y.numpy())


def _sample_scale(regime, R):
    """Per-sample factor on X (forward) / dY (backward) and the flat samples."""
    f = np.ones(R); flat = np.zeros(R, bool)
    if regime == "flat":
        flat[special_samples(R)] = True
    elif regime == "quiet_sample":
        f[special_samples(R)] = QUIET_SHIFT
    elif regime == "mixed":
        for r in range(R):
            kind = SAMPLE_KINDS[r % 3]
            flat[r] = kind == "flat"
            f[r] = QUIET_SHIFT if kind == "quiet" else 1.0
    return f, flat


GN_EXTRAS = {"gauss": 1, "offset": 2, "flat": 1, "outlier_group": 2, "saturated": 1, "quiet_sample": 0, "mixed": 2}


def tkw_fwd_case(shape, regime, extras=None):
    extras = GN_EXTRAS[regime] if extras is None else extras

    """shape: a key of GN_SHAPES; extras 1: time bias (the first Conv1dBlock), 2: residual (the second), 0: neither; default: GN_EXTRAS.
    offset: bias = 40 x the convolution's spread (+ 0.3 N(0, 1));  flat: X = 0 in the special samples and the bias constant within each group;
    outlier_group: group 3's weights x 10 and bias + 5;  saturated: gamma, beta x 15;  quiet_sample: the special samples' X x 2^-10 and no bias
    (their stash is quiet then);  mixed: sample r is Gaussian / flat / quiet (x 2^-10) by r % 3, bias constant within each group, group 3's
    weights x 10."""
    def make():
        L, K, N, R, K1 = GN_SHAPES[shape]
        g = _gen("tkwf", shape, regime)
        M = L * R
        X = 1.3 * g.standard_normal((M, K))
        W = g.standard_normal((5, N, K)) / np.sqrt(5 * K)
        bias = 0.3 * g.standard_normal(N)
        gam = 1 + 0.2 * g.standard_normal(N); bet = 0.2 * g.standard_normal(N)
        gs = N // 8
        f, flat = _sample_scale(regime, R)
        X = X.reshape(R, L, K) * f[:, None, None]
        X[flat] = 0.0
        X = X.reshape(M, K)
        if f.min() < 1.0:
            X = X * to_window(np.abs(X).max())
        if regime == "offset":
            bias = bias + OFFSET_KAPPA * 1.3
        if regime in ("flat", "mixed"):
            bias = np.repeat(0.15 * g.standard_normal(8), gs)      # (0.5 put the float32 floor of y past the cap: |bias| u eps^-1/2)
        if regime in ("outlier_group", "mixed"):
            W[:, 3 * gs:4 * gs] *= 10.0
        if regime == "outlier_group":              # (not in `mixed`: its flat and quiet samples have rstd ~ eps^-1/2, and 5 u eps^-1/2 put the float32 floor of y past the cap)
            bias[3 * gs:4 * gs] += 5.0
        if regime == "saturated":
            gam = gam * SATURATION; bet = bet * SATURATION
        if regime == "quiet_sample":
            bias[:] = 0.0
        c = dict(shape=shape, regime=regime, L=L, K=K, N=N, R=R, K1=K1, M=M, X=X.astype(np.float32), W=W.astype(np.float32),
                 bias=bias.astype(np.float32), gam=gam.astype(np.float32), bet=bet.astype(np.float32),
                 tb=(g.standard_normal(N) if extras & 1 else np.zeros(N)).astype(np.float32),
                 res=(g.standard_normal((M, N)) if extras & 2 else np.zeros((M, N))).astype(np.float32),
                 flat=flat, quiet=f < 1.0)
        c["ref"], c["ref32"] = tkw_fwd_ref64(c), tkw_fwd_eval(c, torch.float32)
        c["scale"] = {"mean": (np.abs(c["ref"]["mean"]) + np.sqrt(c["ref"]["var"])).max(1)}
        c["floor"] = floors(c["ref32"], c["ref"], ("stash", "mean", "rstd", "y"), rows=R, scale=c["scale"])
        c["sites"] = [rowmax(c["X"])]
        return c
    return _cached(("tkwf", shape, regime, extras), make)


# ---- GroupNorm + Mish backward -> conv5^T (tkw / tkc input gradient) ------------------------------------------------------------------------
def tkw_bwd_ref64(c):
    """The float64 formulas of test_tkw_groupnorm_backward_conv_input_gradient: the statistics are the float32 ones the kernel reads."""
    L, R, K = c["L"], c["R"], c["K"]
    cg = c["cst"].astype(np.float64).reshape(R, L, 8, K // 8)
    m32, r32 = c["stats"][..., 0].astype(np.float64), c["stats"][..., 1].astype(np.float64)
    h = (cg - m32[:, None, :, None]) * r32[:, None, :, None]
    gg = c["gam"].astype(np.float64).reshape(8, K // 8); bb = c["bet"].astype(np.float64).reshape(8, K // 8)
    d = c["dy"].astype(np.float64).reshape(R, L, 8, K // 8) * _mish_grad64(h * gg + bb) * gg
    m1 = d.mean(axis=(1, 3), keepdims=True); m2 = (d * h).mean(axis=(1, 3), keepdims=True)
    dc = ((d - m1 - h * m2) * r32[:, None, :, None]).reshape(R * L, K)
    return dict(dc=dc, dx=_conv5_f64(dc, c["W"].astype(np.float64), L, -1) + c["r1"], arg=(h * gg + bb).reshape(R * L, K))


def tkw_bwd_eval(c, dtype):
    """The same composition with torch: mish' by autograd of F.mish, the transposed convolution as a convolution with reversed taps."""
    L, R, K = c["L"], c["R"], c["K"]
    cg = _t(c["cst"], dtype).reshape(R, L, 8, K // 8)
    st = _t(c["stats"], dtype)
    h = (cg - st[..., 0][:, None, :, None]) * st[..., 1][:, None, :, None]
    gg = _t(c["gam"], dtype).reshape(8, K // 8); bb = _t(c["bet"], dtype).reshape(8, K // 8)
    arg = (h * gg + bb).detach().requires_grad_(True)
    (mg,) = torch.autograd.grad(F.mish(arg).sum(), arg)
    d = _t(c["dy"], dtype).reshape(R, L, 8, K // 8) * mg * gg
    m1 = d.mean(dim=(1, 3), keepdim=True); m2 = (d * h).mean(dim=(1, 3), keepdim=True)
    dc = ((d - m1 - h * m2) * st[..., 1][:, None, :, None]).reshape(R * L, K)
    dx = _conv_torch(dc.numpy(), c["W"], L, -1, dtype) + _t(c["r1"], dtype)
    return dict(dc=dc.numpy(), dx=dx.numpy())


# backward shapes: name -> (L, K = C_out of the forward layer, N = C_in, samples, N1 output split)
GN_BWD_SHAPES = {
    "tkw256": (6, 256, 256, 21, 0), "tkw128": (12, 128, 128, 11, 0), "tkw_split": (6, 128, 512, 21, 256), "tkw512": (6, 512, 512, 19, 0),
    "tkc32": (48, 32, 32, 7, 0), "tkc64": (24, 64, 64, 11, 0), "tkc_ng4": (64, 32, 32, 7, 0), "tkc_l32": (32, 64, 32, 7, 0),
}


def tkw_bwd_case(shape, regime, extras=1):
    """The regimes act on the forward layer's stash, an input here:  offset: 60 + 1.5 N(0, 1) (|mean| rstd = 40);  flat: the special samples'
    stash constant within each group (x^ = 0, rstd = eps^-1/2);  outlier_group: group 3 x 10 + 5;  saturated: gamma, beta x 15;
    quiet_sample: the special samples' dY x 2^-10 and no residual;  mixed: by sample, r % 3, group 3 an outlier; the flat samples' dY x 2^-8, so that their rstd = eps^-1/2 does not
    put the operand's maximum 2^8 above the Gaussian samples' and the quiet ones 2^-18 below it."""
    def make():
        L, K, N, R, N1 = GN_BWD_SHAPES[shape]
        g = _gen("tkwb", shape, regime)
        M = L * R
        dy = g.standard_normal((M, K))
        cst = (1.5 * g.standard_normal((M, K)) + 0.3).reshape(R, L, 8, K // 8)
        gam = 1 + 0.2 * g.standard_normal(K); bet = 0.2 * g.standard_normal(K)
        W = g.standard_normal((5, N, K)) / np.sqrt(5 * K)
        f, flat = _sample_scale(regime, R)
        if regime == "offset":
            cst += OFFSET_KAPPA * 1.5 - 0.3
        if regime in ("outlier_group", "mixed"):
            cst[:, :, 3] = cst[:, :, 3] * 10.0 + 5.0
        cst[flat] = (0.5 * g.standard_normal((int(flat.sum()), 1, 8, 1)))
        if regime == "saturated":
            gam = gam * SATURATION; bet = bet * SATURATION
        if regime == "mixed":
            f = np.where(flat, FLAT_DY, f)
        dy = (dy.reshape(R, L, K) * f[:, None, None]).reshape(M, K)
        cst = cst.astype(np.float32)
        if f.min() < 1.0:              # (the operand dc is linear in dY: one float64 evaluation gives the power of two that puts its maximum into the window)
            cg = cst.astype(np.float64)
            probe = dict(L=L, R=R, K=K, cst=cst.reshape(M, K), dy=dy, gam=gam, bet=bet, W=W, r1=np.zeros((M, N)),
                         stats=np.stack([cg.mean(axis=(1, 3)), 1.0 / np.sqrt(cg.var(axis=(1, 3)) + EPS)], axis=-1).astype(np.float32))
            dy = dy * to_window(np.abs(tkw_bwd_ref64(probe)["dc"]).max())
        r1 = g.standard_normal((M, N)) if (extras & 1 and regime != "quiet_sample") else np.zeros((M, N))
        cst = cst.astype(np.float32)
        cg = cst.astype(np.float64)
        stats = np.stack([cg.mean(axis=(1, 3)), 1.0 / np.sqrt(cg.var(axis=(1, 3)) + EPS)], axis=-1).astype(np.float32)
        c = dict(shape=shape, regime=regime, L=L, K=K, N=N, R=R, N1=N1, M=M, dy=dy.astype(np.float32), cst=cst.reshape(M, K), stats=stats,
                 gam=gam.astype(np.float32), bet=bet.astype(np.float32), W=W.astype(np.float32), r1=r1.astype(np.float32), flat=flat, quiet=f == QUIET_SHIFT)
        c["ref"], c["ref32"] = tkw_bwd_ref64(c), tkw_bwd_eval(c, torch.float32)
        c["floor"] = floors(c["ref32"], c["ref"], ("dx",), rows=R)
        c["sites"] = [rowmax(c["ref"]["dc"])]
        return c
    return _cached(("tkwb", shape, regime, extras), make)


# ---- the bare narrow convolution (tkc through ramp_op_gemm_mode) -----------------------------------------------------------------------------
def tkc_case(regime, L=24, R=11, N=64, K=64):
    """regime "gauss" or "quiet_sample" (the special samples' operand x 2^-10; no bias / residual, so their output is quiet)."""
    def make():
        g = _gen("tkc", regime, L, R, N, K)
        M = L * R
        f, _ = _sample_scale(regime, R)
        A = ((1.7 * g.standard_normal((M, K)) + 0.1).reshape(R, L, K) * f[:, None, None]).reshape(M, K)
        A = (A * to_window(np.abs(A).max()) if f.min() < 1.0 else A).astype(np.float32)
        W = (g.standard_normal((5, N, K)) / np.sqrt(5 * K)).astype(np.float32)
        c = dict(regime=regime, L=L, R=R, N=N, K=K, M=M, A=A, W=W, quiet=f < 1.0)
        c["ref"] = dict(out=_conv5_f64(A.astype(np.float64), W.astype(np.float64), L, 1))
        c["ref32"] = dict(out=_conv_torch(A, W, L, 1, torch.float32).numpy())
        c["floor"] = floors(c["ref32"], c["ref"], ("out",), rows=R)
        c["sites"] = [rowmax(A)]
        return c
    return _cached(("tkc", regime, L, R, N, K), make)
