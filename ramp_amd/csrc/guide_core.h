// The device code the three cost-guide files share (guide.hip, guide_replan.hip, guide_prims.hip): the cloud term, the stencils, the clipped
// update and the cost kernels' reductions, each stated once, so that "the same bits as guide_step_kernel / guide_cost_kernel" holds between
// the kernels by construction.  Include it ONLY from files built with -ffp-contract=off (ramp_amd/build.py): every product and sum below is
// meant to be rounded once, as written, and a contracted build would change the three files' bits together without a compile error.
//
// Everything here is block-level code for one 256-thread block per trajectory: tid = threadIdx.x, lane = tid & 63, wave = tid >> 6; thread h
// owns waypoint h in the stencil passes, wave w owns waypoints w, w + 4, ... in the cloud passes.  The kernels keep their own __shared__
// arrays (their LDS footprints differ on purpose) and pass them in.
//
// Order of the fp32 sums over points, fixed by (P, GUIDE_TILE) alone: lane l adds points l, l + 64, ... of a tile in that order, the 64 lane
// sums are added in a butterfly (xor 32, 16, .., 1: the same bits in every lane), the tiles' sums are added in tile order.
#pragma once
#include "args_sampler.h"

namespace ramp {

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// the cheap filter in front of the square root: d2 < guide_r2hi(r) lets every pair with d < r through; `d < r` decides
__device__ __forceinline__ float guide_r2hi(float r) { return mul(mul(r, r), 1.00001f); }

// the four waves' partial sums, in this association everywhere
__device__ __forceinline__ double guide_sum4(const double* r) { return ((r[0] + r[1]) + r[2]) + r[3]; }

// the block's scene sc and the span [first, first + P) of its cloud in the concatenated (P_total, D) table, clamped to the table's total
struct GuideSpan { int sc; const float* cloud; int P; };
// false: a scene index outside the table (uniform over the block) -- the trajectory is left as it is.  Args: GuideArgs or MovingGuideArgs
template <class Args>
__device__ __forceinline__ bool guide_scene(const Args& a, int D, int b, GuideSpan* s) {
  const int sc = a.scene ? a.scene[b] : 0;
  if (sc < 0 || sc >= a.n_scenes) return false;
  const int first = min(max(a.cloud_off[sc], 0), a.P_total), end = min(max(a.cloud_off[sc + 1], first), a.P_total);
  s->sc = sc; s->cloud = a.cloud + (size_t)first * D; s->P = end - first;
  return true;
}

// np points from `cloud` (np, D) into the planes cl[c][e]: consecutive threads read consecutive words
template <int D>
__device__ __forceinline__ void guide_load_tile(float (*cl)[GUIDE_TILE], const float* __restrict__ cloud, int np, int tid) {
  for (int i = tid; i < np * D; i += 256) { const int e = i / D; cl[i - e * D][e] = cloud[i]; }
}

// -dC/dq of the pairs (q, tile point e), e = lane, lane + 64, ... < np, summed over the wave: the same bits in every lane
template <int D>
__device__ __forceinline__ void guide_pair_force(const float (&q)[D], const float (*cl)[GUIDE_TILE], int np, int lane, float r, float r2hi,
                                                 float (&sum)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) sum[c] = 0.f;
  for (int e = lane; e < np; e += 64) {
    float dx[D];
#pragma unroll
    for (int c = 0; c < D; ++c) dx[c] = sub(q[c], cl[c][e]);
    float d2 = mul(dx[0], dx[0]);
#pragma unroll
    for (int c = 1; c < D; ++c) d2 = add(d2, mul(dx[c], dx[c]));
    if (d2 < r2hi) {
      const float d = __fsqrt_rn(d2);
      if (d < r && d > 0.f) {                 // a pair at distance zero contributes no gradient
        const float f = __fdiv_rn(sub(r, d), d);      // -d/dp 1/2 (r - d)^2 = (r - d) (p - c) / d
#pragma unroll
        for (int c = 0; c < D; ++c) sum[c] = sub(sum[c], mul(f, dx[c]));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum[c] = add(sum[c], __shfl_xor(sum[c], m));
  }
}

// the pairs' cost values 1/2 (r - d)^2 of one lane: fp32 values, added to *t in fp64 in the lane's order
template <int D>
__device__ __forceinline__ void guide_pair_cost(const float (&q)[D], const float (*cl)[GUIDE_TILE], int np, int lane, float r, float r2hi,
                                                double* t) {
  for (int e = lane; e < np; e += 64) {
    float d2 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) { const float dx = sub(q[c], cl[c][e]); d2 = c == 0 ? mul(dx, dx) : add(d2, mul(dx, dx)); }
    if (d2 < r2hi) {
      const float d = __fsqrt_rn(d2);
      if (d < r) { const float u = sub(r, d); *t += (double)mul(0.5f, mul(u, u)); }
    }
  }
}

// the cloud term of iteration `it` of a step kernel: gob[h] = d C_obs / d p_h of the free waypoints (P > 0).  A cloud of at most one tile
// is loaded once per launch, a longer one is re-read on every iteration
template <int D>
__device__ __forceinline__ void guide_cloud_force(float (*cl)[GUIDE_TILE], const float (*pos)[D], float (*gob)[D], const int* pin,
                                                  const float* cloud, int P, int H, int it, float r, float r2hi, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < D; ++c) gob[tid][c] = 0.f;
  }
  for (int p0 = 0; p0 < P; p0 += GUIDE_TILE) {
    const int np = min(GUIDE_TILE, P - p0);
    __syncthreads();
    if (it == 0 || P > GUIDE_TILE) guide_load_tile<D>(cl, cloud + (size_t)p0 * D, np, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4) {
      if (pin[h]) continue;                       // its gradient is zeroed anyway (uniform over the wave)
      float q[D], sum[D];
#pragma unroll
      for (int c = 0; c < D; ++c) q[c] = pos[h][c];
      guide_pair_force<D>(q, cl, np, lane, r, r2hi, sum);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < D; ++c) gob[h][c] = add(gob[h][c], sum[c]);
      }
    }
  }
}

// the cloud term of a cost kernel: C_obs of every waypoint against every tile, a thread's own pairs added to *t in order
template <int D>
__device__ __forceinline__ void guide_cloud_cost(float (*cl)[GUIDE_TILE], const float (*pos)[D], const float* cloud, int P, int H, float r,
                                                 float r2hi, int tid, double* t) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int p0 = 0; p0 < P; p0 += GUIDE_TILE) {
    const int np = min(GUIDE_TILE, P - p0);
    __syncthreads();
    guide_load_tile<D>(cl, cloud + (size_t)p0 * D, np, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4) {
      float q[D];
#pragma unroll
      for (int c = 0; c < D; ++c) q[c] = pos[h][c];
      guide_pair_cost<D>(q, cl, np, lane, r, r2hi, t);
    }
  }
}

// the last hard condition that names waypoint h, or -1: later entries win, like hard_value
__device__ __forceinline__ int guide_last_cond(const HardConds& hc, int h) {
  int k_last = -1;
  for (int k = 0; k < hc.n; ++k) if (hc.idx[k] == h) k_last = k;
  return k_last;
}

// the working copy and the pins of trajectory b (tr) from its hard conditions alone: pin[h] = 1 + the last condition that names h, 0 = free;
// a pinned waypoint holds its conditioned value
template <int D>
__device__ __forceinline__ void guide_pin_hard(const GuideArgs& a, int b, const float* tr, float (*pos)[D], int* pin, int tid) {
  if (tid < a.H) {
    const int k_last = guide_last_cond(a.hc, tid);
    pin[tid] = k_last + 1;
    const float* src = k_last >= 0 ? a.hc.val + ((size_t)k_last * a.B + b) * a.S : tr + (size_t)tid * a.S;
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = src[c];
  }
}

// the trajectory as it is (the cost kernels' working copy)
template <int D>
__device__ __forceinline__ void guide_load_pos(const float* tr, int H, int S, float (*pos)[D], int tid) {
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = tr[(size_t)tid * S + c];
  }
}

// acc[h] = p_{h+1} - 2 p_h + p_{h-1}, zero at both ends, between two barriers: the positions and the terms' gradients of this iteration
// are in place before it, acc after it
template <int D>
__device__ __forceinline__ void guide_second_difference(const float (*pos)[D], float (*acc)[D], int H, int tid) {
  __syncthreads();
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < D; ++c)
      acc[tid][c] = (tid >= 1 && tid <= H - 2) ? add(sub(pos[tid + 1][c], mul(2.f, pos[tid][c])), pos[tid - 1][c]) : 0.f;
  }
  __syncthreads();
}

// the scalars of the update, as GuideArgs and MovingGuideArgs name them
struct GuideWeights { float w_obs, w_smooth, w_acc, max_norm, step; };

// The rest of an iteration, after guide_second_difference: g = w_obs g_obs + (w_extra g_extra + (w_smooth g_smooth + w_acc g_acc)) on the
// free waypoints (the first term only with obs; the second only with extra: g_extra = thread h's D values of the kernel's own term), its
// norm over the trajectory (fp64, block reduction through red[4]), the clip and the step
template <int D>
__device__ __forceinline__ void guide_update(float (*pos)[D], const float (*acc)[D], const float (*gob)[D], const int* pin, double* red, int H,
                                             const GuideWeights& w, bool obs, bool extra, float w_extra, const float (&g_extra)[D], int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  float g[D];
  double n2 = 0.0;
  if (tid < H) {
    const int h = tid;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      // smoothness: (p_h - p_{h+1}) + (p_h - p_{h-1}); acceleration: a_{h-1} - 2 a_h + a_{h+1}
      float gs = 0.f, ga = mul(-2.f, acc[h][c]);
      if (h + 1 < H) { gs = add(gs, sub(pos[h][c], pos[h + 1][c])); ga = add(ga, acc[h + 1][c]); }
      if (h >= 1) { gs = add(gs, sub(pos[h][c], pos[h - 1][c])); ga = add(ga, acc[h - 1][c]); }
      float v = add(mul(w.w_smooth, gs), mul(w.w_acc, ga));
      if (extra) v = add(mul(w_extra, g_extra[c]), v);
      if (obs) v = add(mul(w.w_obs, gob[h][c]), v);
      g[c] = pin[h] ? 0.f : v;
      n2 += (double)g[c] * (double)g[c];
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m);
  if (lane == 0) red[wave] = n2;
  __syncthreads();
  const float n = (float)sqrt(guide_sum4(red));
  float s = 1.f;
  if (w.max_norm > 0.f && n > 0.f) s = fminf(1.f, __fdiv_rn(w.max_norm, n));
  const float ss = mul(w.step, s);
  if (tid < H && !pin[tid]) {
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = sub(pos[tid][c], mul(ss, g[c]));
  }
}

// the free waypoints back to the trajectory (every thread writes back only what it updated last: no barrier needed)
template <int D>
__device__ __forceinline__ void guide_write_back(float* tr, int H, int S, const float (*pos)[D], const int* pin, int tid) {
  if (tid < H && !pin[tid]) {
#pragma unroll
    for (int c = 0; c < D; ++c) tr[(size_t)tid * S + c] = pos[tid][c];
  }
}

// the smoothness and acceleration values of thread h (one value each per thread, so `=`, not `+=`)
template <int D>
__device__ __forceinline__ void guide_stencil_costs(const float (*pos)[D], int H, int tid, double* t_smooth, double* t_acc) {
  if (tid < H) {
    const int h = tid;
    if (h + 1 < H) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) { const float dx = sub(pos[h + 1][c], pos[h][c]); v = c == 0 ? mul(dx, dx) : add(v, mul(dx, dx)); }
      *t_smooth = (double)mul(0.5f, v);
    }
    if (h >= 1 && h + 1 < H) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const float ac = add(sub(pos[h + 1][c], mul(2.f, pos[h][c])), pos[h - 1][c]);
        v = c == 0 ? mul(ac, ac) : add(v, mul(ac, ac));
      }
      *t_acc = (double)mul(0.5f, v);
    }
  }
}

// the K columns of a cost kernel's row: the threads' fp64 sums over lanes, then waves (through red[K][4]), into terms[0 .. K)
template <int K>
__device__ __forceinline__ void guide_store_terms(double (&t)[K], double (*red)[4], double* __restrict__ terms, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t[k] += __shfl_xor(t[k], m);
    if (lane == 0) red[k][wave] = t[k];
  }
  __syncthreads();
  if (tid < K) terms[tid] = guide_sum4(red[tid]);
}
// the row of a trajectory whose scene index is outside the table
template <int K>
__device__ __forceinline__ void guide_store_nan(double* __restrict__ terms, int tid) {
  if (tid < K) terms[tid] = __longlong_as_double(0x7ff8000000000000ll);
}

// ---- launch side: what the three families require of their common arguments, with the caller's texts ----
template <class Args>
inline int require_guide_common(const Args& a, const char* dims, const char* table, const char* conds) {
  RAMP_REQUIRE(a.traj && a.B > 0 && a.H > 0 && a.H <= GUIDE_MAX_H, dims);
  RAMP_REQUIRE(a.n_scenes >= 1 && a.cloud_off && a.P_total >= 0 && (a.P_total == 0 || a.cloud), table);
  RAMP_REQUIRE(a.hc.n == 0 || (a.hc.idx && a.hc.val), conds);
  return 0;
}
inline int require_guide_args(const GuideArgs& a, const char* dims, const char* point_dim, const char* conds) {
  if (int rc = require_guide_common(a, dims, "bad guide cloud table", conds)) return rc;
  RAMP_REQUIRE((a.D == 2 || a.D == 3) && a.D <= a.S, point_dim);
  return 0;
}

}  // namespace ramp
