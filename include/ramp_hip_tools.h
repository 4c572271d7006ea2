/* Diagnostics behind the RAMP sampler's C ABI (include/ramp_hip.h): the per-kernel micro-benchmark, its stress form, the GEMM contract probe and the probes of the network-edge and row kernels.  NOT part of the
 * product boundary -- no reference interface corresponds to them (the reference has no micro-benchmarks; its kernels are ATen's).  They are
 * compiled from ramp_amd/csrc/bench.hip into ramp_amd/lib/libramp_hip_tools.so, which also contains every object of libramp_hip.so, and
 * bound by ramp_amd._lib.load_tools() for tests/ (bitwise stress / soak tests of every hand-scheduled kernel) and ramp_amd/tools/. */
#ifndef RAMP_HIP_TOOLS_H
#define RAMP_HIP_TOOLS_H

#include "ramp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* micro-benchmark (profiling tools only): one GEMM shape on the kernel `mode` names (as ramp_op_gemm_mode), operands
 * allocated and filled inside, weights packed once, `warmup` untimed then `iters` timed back-to-back launches on `stream`
 * between two HIP events; *avg_us = microseconds per launch.  flags: 1 bias, 2 residual, 4 GEGLU-forward epilogue
 * (N = 2F), 8 A-multiplier operand (the FF1-dX loader; K = 2 x the operand width), 16 force the 128 x 128 tile,
 * 32 force 3 blocks per CU. */
int ramp_bench_gemm(int32_t M, int32_t N, int32_t K, int32_t taps, int32_t L, int32_t mode, int32_t flags,
                    int32_t warmup, int32_t iters, float* avg_us, void* stream);
/* stress form of the micro-benchmark (tests): `iters` back-to-back launches of the kernel `mode` / `flags` name on the same
 * operands, every launch's output compared bit for bit with the first one's on the device (*mismatching_words: 32-bit words
 * that ever differed; a deterministic kernel gives 0), and -- modes 1..4, rel_err_vs_fp32 non-NULL -- the first output
 * against the exact-fp32 MFMA kernel's on the same operands (max |diff| / max |ref|; -1 where there is no fp32 twin). */
int ramp_stress_gemm(int32_t M, int32_t N, int32_t K, int32_t taps, int32_t L, int32_t mode, int32_t flags, int32_t iters,
                     int64_t* mismatching_words, float* rel_err_vs_fp32, void* stream);

/* probe of the whole GEMM operand contract (tests): one launch of the GEMM kernels on caller-owned device operands with every
 * operand field of the engine's launch arguments.  C[m, n] = sum_tap sum_k Asrc(m, tap)[k] W[tap][n][k] + bias[n]
 * + rowbias[rowvar[row0 + m / L] * rb_stride + n] + resid[orow] + resid2[orow], where the source row of output token
 * (seg, l) = (m / L, m % L) is seg * (L * a_stride) + l * a_stride + shift0 + tap * shift_step (zero outside the segment), k < K1
 * reads A and k >= K1 reads A2 (A2 NULL: K1 = K), the output row is orow = m * c_rstride + c_roff, and n < N1 goes to C, n >= N1
 * to C2 (C2 NULL: N1 = N).  W is raw fp32 [taps][N][K], packed for `mode` (0 fp32, 1 bf16x6, 2 bf16x6 with LDS-staged weights,
 * 3 fp16x3) as ramp_op_gemm_mode packs it; a_absmax_prev, *a_absmax_out and *range_flag_out as there.  Synchronises `stream`. */
typedef struct ramp_probe_gemm_args {
  const float* A; int32_t lda;
  const float* A2; int32_t lda2; int32_t K1;
  const float* W;
  const float* bias;
  const float* rowbias; const int32_t* rowvar; int32_t row0; int32_t rb_stride;
  const float* resid; int32_t ldr;
  const float* resid2; int32_t ldr2;
  float* C; int32_t ldc;
  float* C2; int32_t ldc2; int32_t N1;
  int32_t M, N, K;
  int32_t taps, shift0, shift_step, L;
  int32_t a_stride, c_rstride, c_roff;
} ramp_probe_gemm_args;
int ramp_probe_gemm(const ramp_probe_gemm_args* args, int32_t mode, float a_absmax_prev, float* a_absmax_out,
                    int32_t* range_flag_out, void* stream);

/* probes of the plain-C++ kernels at the two ends of the score network and where the shared prefix fans out (tests): each is one launch
 * of the engine's own launcher on caller-owned device buffers, with the launcher's refusals, and synchronises `stream`.
 *   conv_in forward: x (R / n_rp, H, S) -> c1, res (R, H, C0), row r reads x[r / n_rp]; W5 packed [5][S][C0] from the Conv1d's (C0, S, 5),
 *     W1 [S][C0] from the residual Conv1d's (C0, S, 1); S <= 16, C0 in {16, 32, 64}
 *   conv_in backward: dc1, dy (R, H, C0) -> eps (R, H, S), the input gradient of the pair
 *   conv_out: a (n_tok, C0) -> f (n_tok, S) = a Wf^T + bf and da (n_tok, C0) = f Wf; Wf [S][C0]; f or da may be NULL
 *   expand_rows: in (R / n_rp, L, C) -> out (R, L, C), out[r] = in[r / n_rp] + rowbias[rowvar[row0 + r] * rb_stride + c] (rowbias NULL: a copy)
 *   combine_rows: in (B n_rp, L, C) -> out (B, L, C) = sum_j w_host[j] in[b n_rp + j], n_rp <= 3, w_host HOST floats
 *   combine_rows_weighted: the same with row_weight DEVICE floats (B, n_rp), 2 <= n_rp <= 8 */
int ramp_probe_conv_in_fwd(const float* x, const float* W5, const float* b5, const float* W1, const float* b1, float* c1, float* res,
                           int32_t R, int32_t n_rp, int32_t H, int32_t S, int32_t C0, void* stream);
int ramp_probe_conv_in_bwd(const float* dc1, const float* dy, const float* W5, const float* W1, float* eps, int32_t R, int32_t H,
                           int32_t S, int32_t C0, void* stream);
int ramp_probe_conv_out(const float* a, const float* Wf, const float* bf, float* f, float* da, int32_t n_tok, int32_t S, int32_t C0,
                        void* stream);
int ramp_probe_expand_rows(const float* in, float* out, int32_t R, int32_t n_rp, int32_t L, int32_t C, const float* rowbias,
                           int32_t rb_stride, const int32_t* rowvar, int32_t row0, void* stream);
int ramp_probe_combine_rows(const float* in, float* out, int32_t B, int32_t n_rp, int32_t L, int32_t C, const float* w_host,
                            void* stream);
int ramp_probe_combine_rows_weighted(const float* in, float* out, int32_t B, int32_t n_rp, int32_t L, int32_t C,
                                     const float* row_weight, void* stream);
/* the cross-attention constants out (n_var, n_blk, 256) = Wo_blk (Wv_blk lat[v]) + bo_blk of lat (n_var, ctx_dim), ctx_dim <= 512;
 * wv_host / wo_host / bo_host: HOST arrays of n_blk DEVICE pointers (Wv (256, ctx_dim), Wo (256, 256), bo (256)) */
int ramp_probe_cross_bias(const float* lat, int32_t n_var, int32_t ctx_dim, const float* const* wv_host, const float* const* wo_host,
                          const float* const* bo_host, int32_t n_blk, float* out, void* stream);
/* block `module_name`'s (a ResidualTemporalBlock, named as in ramp_debug_read) n = cout floats of line t of the context's prepared
 * time table, copied to out (device); an unknown name, another n or a t outside the table is refused */
int ramp_probe_time_bias(ramp_ctx* ctx, const char* module_name, int32_t t, float* out, int32_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* RAMP_HIP_TOOLS_H */
