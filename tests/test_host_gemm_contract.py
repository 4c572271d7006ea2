"""The float64 GEMM contract of tests/gemm_contract.py, which test_gpu_gemm_forms.py holds the kernels to, checked on the CPU: against
an element-by-element restatement of the args_gemm.h formula for every form, and against torch's Conv1d / ConvTranspose1d for the
resampling convolutions it stands for.  The GPU tests then test the kernels, not their reference."""
import numpy as np
import pytest
import torch

from gemm_contract import FORMS, expected_outputs, form_cases, launch_fields, reference, reference_loop


def smallest(form):
    return min(form_cases(form), key=lambda c: (c.get("C", 0) + c.get("Ca", 0) + c.get("Cout", 0)) * c["L"])


@pytest.mark.parametrize("form", FORMS)
def test_contract_matches_elementwise_loop(form):
    """gemm_contract equals the loop statement of the formula on the smallest engine case of each form (and, F7, on all four
    row-variant launches), at R = 2 samples; expected_outputs writes exactly the (row, column) set the loop names."""
    g = np.random.default_rng(len(form))
    case = smallest(form)
    for variant in ((0, 1, 2, 3) if case["kind"] == "outproj" else (0,)):
        f, shapes = launch_fields(case, 2, g, variant)
        orow, out = reference(f)
        loop = reference_loop(f)
        N = f["N"]
        assert len(loop) == f["M"] * N
        for m in range(f["M"]):
            got = [loop[(int(orow[m]), n)] for n in range(N)]
            np.testing.assert_allclose(out[m], got, rtol=1e-12, atol=1e-12)
        N1 = f.get("N1", N)
        exp = expected_outputs(f, shapes, -1.0)
        written = {(r, n) for r, n in zip(*np.nonzero(exp["C"][1]))}
        if "C2" in exp:
            written |= {(r, n + N1) for r, n in zip(*np.nonzero(exp["C2"][1]))}
        assert written == set(loop), (form, case)


def test_case_table_reaches_every_kernel_family():
    """The forms reach the narrow kernel (K % 32 != 0), the tile kernels at N < 64, 64 <= N < 128 and N >= 128, and the split-K /
    split-N forms on both sides of K % 32; every case's operands are sized for the rows its launch reads and writes."""
    seen = set()
    g = np.random.default_rng(0)
    for form in FORMS:
        for case in form_cases(form):
            f, shapes = launch_fields(case, 1, g)
            seen.add(("narrow" if f["K"] % 32 else "tile", "N<64" if f["N"] < 64 else "N<128" if f["N"] < 128 else "N>=128",
                      "A2" if "A2" in f else "C2" if "C2" in shapes else "-"))
            M, L, a_s, c_s = f["M"], f.get("L", 1), f.get("a_stride", 1), f.get("c_rstride", 1)
            assert M % L == 0
            assert f["A"].shape[0] == M * a_s and ("A2" not in f or f["A2"].shape[0] == M * a_s)
            assert all(s[0] == M * c_s for s in shapes.values()) and f.get("c_roff", 0) < c_s
    for want in [("narrow", "N<64", "-"), ("narrow", "N>=128", "-"), ("narrow", "N<128", "C2"), ("tile", "N<64", "A2"),
                 ("tile", "N<64", "-"), ("tile", "N<128", "-"), ("tile", "N>=128", "-"), ("tile", "N>=128", "A2"),
                 ("tile", "N>=128", "C2")]:
        assert want in seen, (want, sorted(seen))


@pytest.mark.parametrize("C,Lout,R", [(32, 4, 3), (64, 1, 2), (16, 12, 2)])
def test_downsample_form_is_conv1d_stride2(C, Lout, R):
    """F1 (3 taps, shift -1, source stride 2, L = L_out) is torch's Conv1d(C, C, 3, stride=2, padding=1) in channels-last rows."""
    g = np.random.default_rng(C + Lout)
    f, _ = launch_fields(dict(kind="down_fwd", C=C, L=Lout), R, g)
    x = torch.from_numpy(f["A"].astype(np.float64)).reshape(R, 2 * Lout, C).permute(0, 2, 1)
    w = torch.from_numpy(f["W"].astype(np.float64)).permute(1, 2, 0)                      # W[tap][n][k] -> weight[n][k][tap]
    y = torch.nn.functional.conv1d(x, w, torch.from_numpy(f["bias"].astype(np.float64)), stride=2, padding=1)
    _, out = reference(f)
    np.testing.assert_allclose(out, y.permute(0, 2, 1).reshape(R * Lout, C).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("C,Lin,R", [(32, 4, 3), (64, 1, 2), (16, 6, 2)])
def test_upsample_form_is_conv_transpose1d(C, Lin, R):
    """F3 (per output phase par: 2 taps, shift par, step -1, output rows 2 m + par) is torch's ConvTranspose1d(C, C, 4, stride=2,
    padding=1): phase 0 takes the kernel taps (1, 3), phase 1 the taps (0, 2)."""
    g = np.random.default_rng(C + Lin)
    wt = g.standard_normal((C, C, 4))                                                         # ConvTranspose1d weight [in][out][k]
    out = np.zeros((R * 2 * Lin, C))
    for par, taps in ((0, (1, 3)), (1, (0, 2))):
        f, shapes = launch_fields(dict(kind="up_fwd", C=C, L=Lin, par=par), R, g)
        if par == 1:
            f["A"], f["bias"] = A, bias
        A, bias = f["A"], f["bias"]
        f["W"] = np.stack([wt[:, :, j].T for j in taps]).astype(np.float64)
        exp, mask = expected_outputs(f, shapes, 0.0)["C"]
        out[mask] = exp[mask]
    x = torch.from_numpy(A.astype(np.float64)).reshape(R, Lin, C).permute(0, 2, 1)
    y = torch.nn.functional.conv_transpose1d(x, torch.from_numpy(wt), torch.from_numpy(bias.astype(np.float64)), stride=2, padding=1)
    np.testing.assert_allclose(out, y.permute(0, 2, 1).reshape(R * 2 * Lin, C).numpy(), rtol=1e-12, atol=1e-12)
