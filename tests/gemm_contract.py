"""The GEMM launch contract of ramp_amd/csrc/args_gemm.h as a float64 numpy function, and the forms the engine launches it in.

C[orow(m), n] = sum_tap sum_k Asrc(m, tap)[k] W[tap][n][k] + bias[n] + rowbias[rowvar[row0 + m / L] * rb_stride + n]
                + resid[orow(m), n] + resid2[orow(m), n]
  source row of output token (seg, l) = (m / L, m % L): seg * (L * a_stride) + l * a_stride + shift0 + tap * shift_step,
  zero outside the segment; k < K1 reads A, k >= K1 reads A2; orow(m) = m * c_rstride + c_roff; n < N1 goes to C, the rest to C2.

Operands are 2-D arrays whose row length is their leading dimension (lda = A.shape[1], ...); rowbias is flat.
"""
from __future__ import annotations

import numpy as np

from ramp_amd.spec import ATTN_DEPTH, ATTN_INNER, UNET_DIM_MULTS, make_unet_spec


def gemm_contract(A, W, M, N, K, taps=1, shift0=0, shift_step=0, L=1, a_stride=1, c_rstride=1, c_roff=0, A2=None, K1=None,
                  bias=None, rowbias=None, rowvar=None, row0=0, rb_stride=None, resid=None, resid2=None, N1=None):
    """-> (orow (M,) output rows, out (M, N) float64): what the launch writes, row orow[m] of C (columns < N1) / C2 (the rest)."""
    K1 = K if A2 is None else K1
    rb_stride = N if rb_stride is None else rb_stride
    m = np.arange(M)
    seg, l = m // L, m % L
    Lin = L * a_stride
    out = np.zeros((M, N))
    for tap in range(taps):
        ls = l * a_stride + shift0 + tap * shift_step
        ok = (ls >= 0) & (ls < Lin)
        src = np.where(ok, seg * Lin + ls, 0)
        X = A[src, :K1].astype(np.float64)
        if K1 < K:
            X = np.concatenate([X, A2[src, :K - K1].astype(np.float64)], axis=1)
        X[~ok] = 0.0
        out += X @ W[tap].astype(np.float64).T
    orow = m * c_rstride + c_roff
    if bias is not None:
        out += bias.astype(np.float64)
    if rowbias is not None:
        out += rowbias.astype(np.float64)[rowvar[row0 + m // L][:, None] * rb_stride + np.arange(N)[None]]
    if resid is not None:
        out += resid[orow, :N]
    if resid2 is not None:
        out += resid2[orow, :N]
    return orow, out


def gemm_contract_loop(A, W, M, N, K, taps=1, shift0=0, shift_step=0, L=1, a_stride=1, c_rstride=1, c_roff=0, A2=None, K1=None,
                       bias=None, rowbias=None, rowvar=None, row0=0, rb_stride=None, resid=None, resid2=None, N1=None):
    """The same formula one element at a time, written out as args_gemm.h states it (the check of gemm_contract itself)."""
    K1 = K if A2 is None else K1
    rb_stride = N if rb_stride is None else rb_stride
    out = {}
    for m in range(M):
        seg, l = divmod(m, L)
        orow = m * c_rstride + c_roff
        for n in range(N):
            acc = 0.0
            for tap in range(taps):
                ls = l * a_stride + shift0 + tap * shift_step
                if not 0 <= ls < L * a_stride:
                    continue
                src = seg * L * a_stride + ls
                for k in range(K):
                    x = float(A[src, k]) if k < K1 else float(A2[src, k - K1])
                    acc += x * float(W[tap, n, k])
            if bias is not None:
                acc += float(bias[n])
            if rowbias is not None:
                acc += float(rowbias[int(rowvar[row0 + m // L]) * rb_stride + n])
            if resid is not None:
                acc += float(resid[orow, n])
            if resid2 is not None:
                acc += float(resid2[orow, n])
            out[(orow, n)] = acc
    return out


# ---- the forms the engine launches (engine.hip) -------------------------------------------------------------------------------
FORMS = ("F1", "F2", "F3", "F4", "F5", "F6", "F7", "F8")
SHAPES = [(opt, c0) for opt in (0, 1) for c0 in (16, 32, 64)]          # the six served networks: n_levels 3 / 4 x C0 16 / 32 / 64
HORIZONS = tuple(range(8, 72, 8))


def form_cases(form):
    """De-duplicated launch descriptions of one form over the six networks and H = 8 .. 64, as dicts: `kind` names the engine
    call, the other keys the per-sample geometry (L = tokens of one sample in the launch, channel counts, output phase); the
    operand sizes follow from R (samples) in launch_fields."""
    seen = []
    for opt, c0 in SHAPES:
        nl = len(UNET_DIM_MULTS[opt])
        for H in HORIZONS:
            if H % (1 << (nl - 1)):
                continue
            sp = make_unet_spec(4, H, c0, UNET_DIM_MULTS[opt])
            n_blk = len(sp.all_sts()) * ATTN_DEPTH
            cases = []
            if form == "F1":        # Downsample1d forward: 3 taps over stride-2 source rows
                cases += [dict(kind="down_fwd", C=lv.channels, L=lv.length // 2) for lv in sp.downs if lv.resample]
            elif form == "F2":      # its input gradient, per output phase, with / without the strided skip-gradient residual
                cases += [dict(kind="down_dx", C=lv.channels, L=lv.length // 2, par=par, res=res)
                          for lv in sp.downs if lv.resample for par in (0, 1) for res in (False, True)]
            elif form == "F3":      # Upsample1d (ConvTranspose1d k4 s2 p1) forward, per output phase
                cases += [dict(kind="up_fwd", C=lv.channels, L=lv.length, par=par) for lv in sp.ups for par in (0, 1)]
            elif form == "F4":      # its input gradient: 4 taps over stride-2 source rows
                cases += [dict(kind="up_dx", C=lv.channels, L=lv.length) for lv in sp.ups]
            elif form == "F5":      # up block: channel concat of (x, skip) into the k = 5 conv and the 1 x 1 residual conv
                cases += [dict(kind=k, Ca=lv.rtb0.cin // 2, Cb=lv.rtb0.cin // 2, Cout=lv.rtb0.cout, L=lv.length)
                          for lv in sp.ups for k in ("cat_conv5", "cat_res1")]
            elif form == "F6":      # up block input gradient split into (dx, d skip); mid_block1's with the skip gradient added
                cases += [dict(kind="split_dx", Ca=lv.rtb0.cin // 2, Cb=lv.rtb0.cin // 2, Cout=lv.rtb0.cout, L=lv.length)
                          for lv in sp.ups]
                cases += [dict(kind="add2_dx", C=sp.mid1.cin, L=sp.mid1.length)]
            elif form == "F7":      # cross-attention out-projection with the per-variant constant
                cases += [dict(kind="outproj", L=st.length, rb_stride=n_blk * ATTN_INNER, n_blk=n_blk) for st in sp.all_sts()]
            elif form == "F8":      # the narrow plain linears / finest convs of a C0 = 16 network
                if c0 == 16:
                    fin = sp.downs[0]
                    cases += [dict(kind="proj_in", C=fin.channels, L=fin.length), dict(kind="proj_out_dx", C=fin.channels, L=fin.length),
                              dict(kind="conv5_fwd", C=fin.channels, L=fin.length), dict(kind="conv5_dx", C=fin.channels, L=fin.length)]
            for c in cases:
                key = tuple(sorted(c.items()))
                if key not in seen:
                    seen.append(key)
    return [dict(k) for k in seen]


def launch_fields(case, R, g, variant=0):
    """numpy operands and probe fields of one case for R samples (g: numpy Generator).  Returns (fields, out_shapes): fields maps
    ramp_probe_gemm_args members to arrays / ints (the ints M, N, K, ... included); out_shapes = {"C": (rows, ld), "C2": ...}."""
    kind = case["kind"]
    f, shapes = {}, {}

    def mat(r, c, scale=1.0):
        return (g.standard_normal((r, c)) * scale).astype(np.float32)

    def weights(taps, N, K):
        return (g.standard_normal((taps, N, K)) / np.sqrt(taps * K)).astype(np.float32)

    if kind in ("down_fwd", "down_dx", "up_fwd", "up_dx"):
        C, L = case["C"], case["L"]
        M = R * L
        f.update(M=M, N=C, K=C, L=L)
        if kind == "down_fwd":
            f.update(taps=3, shift0=-1, shift_step=1, a_stride=2, A=mat(2 * M, C), W=weights(3, C, C), bias=mat(1, C)[0])
            shapes["C"] = (M, C)
        elif kind == "down_dx":
            par = case["par"]
            f.update(taps=2 if par else 1, shift0=par, shift_step=-1, c_rstride=2, c_roff=par, A=mat(M, C),
                     W=weights(2 if par else 1, C, C))
            if case["res"]:
                f["resid"] = mat(2 * M, C)
            shapes["C"] = (2 * M, C)
        elif kind == "up_fwd":
            par = case["par"]
            f.update(taps=2, shift0=par, shift_step=-1, c_rstride=2, c_roff=par, A=mat(M, C), W=weights(2, C, C),
                     bias=mat(1, C)[0])
            shapes["C"] = (2 * M, C)
        else:
            f.update(taps=4, shift0=-1, shift_step=1, a_stride=2, A=mat(2 * M, C), W=weights(4, C, C))
            shapes["C"] = (M, C)
    elif kind in ("cat_conv5", "cat_res1"):
        Ca, Cb, N, L = case["Ca"], case["Cb"], case["Cout"], case["L"]
        M, K = R * L, Ca + Cb
        taps = 5 if kind == "cat_conv5" else 1
        f.update(M=M, N=N, K=K, L=L if taps == 5 else 1, taps=taps, shift0=-2 if taps == 5 else 0, shift_step=1 if taps == 5 else 0,
                 A=mat(M, Ca), A2=mat(M, Cb, 2.0), K1=Ca, W=weights(taps, N, K), bias=mat(1, N)[0])
        shapes["C"] = (M, N)
    elif kind == "split_dx":
        Ca, Cb, Co, L = case["Ca"], case["Cb"], case["Cout"], case["L"]
        M, N = R * L, Ca + Cb
        # padded leading dimensions of both destinations: a kernel that strides by its column count instead of ldc / ldc2 writes
        # into the padding, which must keep the sentinel
        f.update(M=M, N=N, K=Co, L=L, taps=5, shift0=2, shift_step=-1, A=mat(M, Co), W=weights(5, N, Co), resid=mat(M, N), N1=Ca)
        shapes["C"] = (M, Ca + 4)
        shapes["C2"] = (M, Cb + 8)
    elif kind == "add2_dx":
        C, L = case["C"], case["L"]
        M = R * L
        f.update(M=M, N=C, K=C, L=L, taps=5, shift0=2, shift_step=-1, A=mat(M, C), W=weights(5, C, C), resid=mat(M, C),
                 resid2=mat(M, C))
        shapes["C"] = (M, C)
    elif kind == "outproj":
        L, D, n_blk = case["L"], ATTN_INNER, case["n_blk"]
        M = R * L
        # rowvar: interleaved cond / uncond rows (2 variants, variant 0) or one of three compose variants per sample (1: in turn,
        # 2 and 3: at random), for a later chunk
        # (row0 > 0) of a longer row table; the constant of block `blk` of n_blk starts at blk * D inside rows of rb_stride
        n_var = 2 if variant == 0 else 3
        row0 = 2 * R + 1
        table = np.arange(row0 + R, dtype=np.int32) % n_var if variant < 2 else g.integers(0, n_var, row0 + R).astype(np.int32)
        blk = n_blk - 1 - (variant % n_blk)
        full = mat(n_var, case["rb_stride"])
        f.update(M=M, N=D, K=D, L=L, A=mat(M, D), W=weights(1, D, D), bias=mat(1, D)[0], resid=mat(M, D),
                 rowbias=full.reshape(-1)[blk * D:], rowvar=table, row0=row0, rb_stride=case["rb_stride"])
        if variant == 3:        # the same launch with its residual in two halves: a second residual selects the GEN kernels,
            f["resid2"] = mat(M, D)   # so the row-variant constant is held to the contract on both epilogue paths
        shapes["C"] = (M, D)
    elif kind in ("proj_in", "proj_out_dx", "conv5_fwd", "conv5_dx"):
        C, L = case["C"], case["L"]
        M = R * L
        if kind == "proj_in":
            f.update(M=M, N=ATTN_INNER, K=C, A=mat(M, C), W=weights(1, ATTN_INNER, C), bias=mat(1, ATTN_INNER)[0])
            shapes["C"] = (M, ATTN_INNER)
        elif kind == "proj_out_dx":
            f.update(M=M, N=ATTN_INNER, K=C, A=mat(M, C), W=weights(1, ATTN_INNER, C), resid=mat(M, ATTN_INNER))
            shapes["C"] = (M, ATTN_INNER)
        elif kind == "conv5_fwd":
            f.update(M=M, N=C, K=C, L=L, taps=5, shift0=-2, shift_step=1, A=mat(M, C), W=weights(5, C, C), bias=mat(1, C)[0])
            shapes["C"] = (M, C)
        else:
            f.update(M=M, N=C, K=C, L=L, taps=5, shift0=2, shift_step=-1, A=mat(M, C), W=weights(5, C, C), resid=mat(M, C))
            shapes["C"] = (M, C)
    else:
        raise ValueError(kind)
    return f, shapes


_REF_ARGS = ("M", "N", "K", "taps", "shift0", "shift_step", "L", "a_stride", "c_rstride", "c_roff", "A2", "K1", "bias", "rowbias",
             "rowvar", "row0", "rb_stride", "resid", "resid2", "N1")


def reference(fields):
    """gemm_contract on a launch_fields() dict."""
    return gemm_contract(fields["A"], fields["W"], **{k: v for k, v in fields.items() if k in _REF_ARGS})


def reference_loop(fields):
    return gemm_contract_loop(fields["A"], fields["W"], **{k: v for k, v in fields.items() if k in _REF_ARGS})


def expected_outputs(fields, shapes, sentinel):
    """(C, C2) as the launch must leave them: every written element from the float64 reference, all others the sentinel;
    plus the boolean masks of the written elements."""
    orow, out = reference(fields)
    N = fields["N"]
    N1 = fields.get("N1", N)
    res = {}
    for name, cols, lo in (("C", range(0, N1), 0), ("C2", range(N1, N), N1)):
        if name not in shapes:
            continue
        exp = np.full(shapes[name], sentinel, np.float64)
        mask = np.zeros(shapes[name], bool)
        c = np.arange(len(cols))
        exp[orow[:, None], c[None]] = out[:, lo:lo + len(cols)]
        mask[orow[:, None], c[None]] = True
        res[name] = (exp, mask)
    return res
