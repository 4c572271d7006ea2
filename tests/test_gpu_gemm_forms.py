"""Every GEMM operand form the engine launches, at kernel level: ramp_probe_gemm (tools library) against the float64 statement of
the args_gemm.h contract (gemm_contract.py), at the shapes of the six served networks, on every arithmetic mode.

The outputs start as a sentinel: every element the contract says the launch writes is compared with float64, every other one must
still hold the sentinel bit for bit (a write to the wrong phase, row, column block or destination is caught even where it does not
move a network output)."""
import numpy as np
import pytest
import torch

from gemm_contract import FORMS, form_cases, launch_fields, expected_outputs
from ramp_amd import _lib
from util import dev, rel

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.125e29)
R_SMALL = 3             # samples: M = 3 L is not a multiple of the 128- (or 64-) row tiles at most level lengths
M_LARGE = 10_000        # one case per form with M above this: the persistent grid wraps several rounds of tiles
BAR = 3e-6              # test_gemm_taps' bar, for reductions of up to 2560 products (5 taps x 512 channels) ...
K_BAR = 2560            # ... beyond which it grows as the fp32 rounding of a length-n sum does, sqrt(n): the up blocks' concat convs
                        # of the C0 = 64 network reduce 5 x 1024 products (exact-fp32 MFMA chains: 3.1e-6 over 2.6 M outputs)
BAR_NARROW = 2e-6       # the narrow kernel (K % 32 != 0): exact fp32 FMAs
# mode name -> (probe mode, a_absmax_prev as a multiple of the true max |A| (None: unscaled))
MODES = {"fp32": ("fp32", None), "bf16x6": ("bf16x6", None), "bf16x6-lds": ("bf16x6-lds", None), "fp16x3": ("fp16x3", None),
         "fp16x3-max": ("fp16x3", 1.0), "fp16x3-8max": ("fp16x3", 8.0)}

_CASES = {}


def cases(form):
    """(label, fields, shapes) of one form: every de-duplicated engine case at R_SMALL (the out-projection with four row-variant
    launches), plus the largest-channel case at M > M_LARGE.  Built once per form and shared by the mode tests."""
    if form not in _CASES:
        g = np.random.default_rng(sum(map(ord, form)))
        out = []
        table = form_cases(form)
        for case in table:
            for variant in ((0, 1, 2, 3) if case["kind"] == "outproj" else (0,)):
                f, shapes = launch_fields(case, R_SMALL, g, variant)
                out.append((f"{case} v{variant} R={R_SMALL}", f, shapes))
        big = max(table, key=lambda c: (c.get("C", 0) + c.get("Ca", 0) + c.get("Cout", 0), c["L"],
                                         c.get("par", 0), c.get("res", False)))
        R = M_LARGE // big["L"] + 1
        f, shapes = launch_fields(big, R, g, 1)
        assert f["M"] > M_LARGE
        out.append((f"{big} R={R}", f, shapes))
        _CASES[form] = [(lab, f, shapes, expected_outputs(f, shapes, float(SENTINEL))) for lab, f, shapes in out]
    return _CASES[form]


_DEV = {}


def run_probe(f, shapes, mode, a_absmax_prev=0.0):
    """One ramp_probe_gemm launch on device copies of the operands (made once per case); returns (rc, outputs {name: host
    array}, amax, flag, msg)."""
    if id(f) not in _DEV:
        _DEV[id(f)] = (f, {k: dev(f[k]) for k in ("A", "A2", "W", "bias", "rowbias", "rowvar", "resid", "resid2") if k in f})
    d = _DEV[id(f)][1]
    lds = {"A": "lda", "A2": "lda2", "resid": "ldr", "resid2": "ldr2"}
    ints = {k: v for k, v in f.items() if k not in d}
    for k, ld in lds.items():
        if k in f:
            ints[ld] = f[k].shape[1]
    outs = {}
    for name, shp in shapes.items():
        outs[name] = torch.full(shp, float(SENTINEL), device="cuda")
        ints["ldc" if name == "C" else "ldc2"] = shp[1]
    rc, amax, flag, msg = _lib.probe_gemm(mode, a_absmax_prev, **d, **outs, **ints)
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}, amax, flag, msg


def fragment_shape(f):
    return f["N"] >= 64 and f["N"] % 32 == 0 and f["K"] % 32 == 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form", FORMS)
def test_gemm_form_matches_float64(form, mode):
    """F1 downsample forward, F2 its input gradient (both phases, +- strided residual), F3 upsample forward (both phases), F4 its
    input gradient, F5 the up blocks' two-source convs, F6 the split-output / second-residual input gradients, F7 the
    out-projection with its per-variant row constant, F8 the narrow linears and convs of a C0 = 16 network.  fp16x3 runs
    unscaled and with the delayed operand scale of the true max |A| and of 8x it: on the fragment kernels the recorded maximum is
    max(|A|, |A2|) bit for bit and the range flag stays clear.  Where K % 32 != 0 (the narrow kernel) every mode gives the
    exact-fp32 result bit for bit."""
    pmode, scale = MODES[mode]
    worst, worst_lab, n_run = 0.0, None, 0
    for lab, f, shapes, exp in cases(form):
        amax_true = max(float(np.abs(f["A"]).max()), float(np.abs(f["A2"]).max()) if "A2" in f else 0.0)
        prev = 0.0 if scale is None else scale * amax_true
        rc, outs, amax, flag, msg = run_probe(f, shapes, pmode, prev)
        assert rc == 0, (lab, msg)
        narrow = f["K"] % 32 != 0
        for name, (e, mask) in exp.items():
            got = outs[name]
            assert np.array_equal(got[~mask].view(np.uint32), np.full((~mask).sum(), SENTINEL).view(np.uint32)), \
                (lab, name, "element outside the launch's output was written")
            err = rel(got[mask], e[mask])
            if err > worst:
                worst, worst_lab = err, f"{lab} {name}"
            bar = BAR_NARROW if narrow else BAR * max(1.0, np.sqrt(f.get("taps", 1) * f["K"] / K_BAR))
            assert err < bar, (lab, name, err, bar)
        if narrow and pmode != "fp32":
            _, outs32, _, _, _ = run_probe(f, shapes, "fp32")
            for name in outs:
                assert np.array_equal(outs[name].view(np.uint32), outs32[name].view(np.uint32)), (lab, name, "narrow kernel differs from fp32 mode")
        if pmode == "fp16x3" and fragment_shape(f):
            assert amax == np.float32(amax_true), (lab, amax, amax_true)
            assert flag == 0, (lab, flag)
        n_run += 1
    print(f"{form} {mode}: {n_run} launches, worst rel {worst:.2e} ({worst_lab})")


def _refusal(**over):
    g = np.random.default_rng(1)
    M, N, K = 48, 64, 64
    f = dict(M=M, N=N, K=K, L=1, A=g.standard_normal((M, K)).astype(np.float32),
             W=g.standard_normal((1, N, K)).astype(np.float32))
    f.update(over)
    return f


@pytest.mark.parametrize("mode", ["fp32", "fp16x3"])
@pytest.mark.parametrize("what", ["narrow_N1", "tile_K1", "tile_rowbias", "narrow_rowbias"])
def test_gemm_probe_refusals(what, mode):
    """Launch arguments the kernels cannot serve are refused with ramp_last_error set, and nothing is written."""
    g = np.random.default_rng(2)
    shapes = {"C": (48, 64)}
    if what == "narrow_N1":          # narrow kernel: N1 must be a multiple of 4
        f = _refusal(K=16, A=g.standard_normal((48, 16)).astype(np.float32), W=g.standard_normal((1, 64, 16)).astype(np.float32), N1=30)
        shapes = {"C": (48, 32), "C2": (48, 36)}
        want = "narrow GEMM"
    elif what == "tile_K1":          # tile kernels: the second source starts on a 32-wide K tile
        f = _refusal(A=g.standard_normal((48, 16)).astype(np.float32), A2=g.standard_normal((48, 48)).astype(np.float32), K1=16)
        want = "split-K source must start on a K tile"
    else:                            # a row bias without its variant table
        f = _refusal(rowbias=g.standard_normal(4 * 64).astype(np.float32), rb_stride=64)
        if what == "narrow_rowbias":
            f.update(K=16, A=g.standard_normal((48, 16)).astype(np.float32), W=g.standard_normal((1, 64, 16)).astype(np.float32))
        want = "rowvar"
    rc, outs, _, _, msg = run_probe(f, shapes, mode)
    assert rc != 0 and msg and want in msg, (rc, msg)
    for name, o in outs.items():
        assert np.array_equal(o.view(np.uint32), np.full(o.shape, SENTINEL).view(np.uint32)), name
