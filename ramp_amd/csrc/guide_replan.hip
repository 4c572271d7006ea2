// Cost guidance of the replanning jobs (ramp_replan_guide in include/ramp_hip.h): guide.hip's clipped gradient steps on
//
//   C = w_obs sum_h sum_j 1/2 max(0, r - |p_h - c_j|)^2 + w_mov sum_h sum_j 1/2 max(0, r_mov - |(p_h - delta_h) - m_j|)^2
//       + w_smooth sum_h 1/2 |p_{h+1} - p_h|^2 + w_acc sum_h 1/2 |p_{h+1} - 2 p_h + p_{h-1}|^2
//
// over the positions p_h = x[h, 0:2] of one candidate, the static cloud c of its episode, the episode's moving cloud m (the pursuer's sphere
// points now) and its track delta (H, 2), the cloud's predicted displacement at waypoint h -- with pins that differ from row to row: the
// executed history [0, n_hist) of the row's episode, the goal H - 1 and the hard-conditioned waypoints (MovingGuideArgs in args_sampler.h).
//
// The structure is guide_step_kernel's: one 256-thread block per row, positions, pins and the track in LDS for all iterations of the launch,
// the clouds as planes of 1024 fp32 (lane l reads word l: every ds_read_b32 of the inner loop is conflict-free), wave w owns waypoints
// w, w + 4, ..., lanes split a tile's points, wavefront-shuffle reductions, stencils, norm, clip and update in the same launch.  The moving
// cloud is at most one tile and has planes of its own (8 KiB), so it is loaded once per launch and a static cloud of at most one tile stays
// resident beside it; the block's 22 KiB of LDS leave the wave limit to decide occupancy.
//
// Order of the fp32 sums over points: guide.hip's rule per cloud (a lane's points in order, a butterfly over the lanes, the tiles in order),
// the static tiles first, then the moving tile; g = w_obs g_obs + (w_mov g_mov + (w_smooth g_smooth + w_acc g_acc)), so that without a
// moving term the bits are guide_step_kernel<2>'s.  Built with -ffp-contract=off: every product and sum is rounded once, as written.
#include "args_sampler.h"

#include <algorithm>

namespace ramp {

namespace {

constexpr int MG_TILE = 1024;
constexpr int MG_MAXH = 128;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// the block's scene e, the span [first, first + P) of its static cloud (clamped to the table's total).  false: a scene index outside the
// table (uniform over the block)
__device__ __forceinline__ bool mg_scene(const MovingGuideArgs& a, int b, int* e, const float** cloud, int* P) {
  const int sc = a.scene ? a.scene[b] : 0;
  if (sc < 0 || sc >= a.n_scenes) return false;
  const int first = min(max(a.cloud_off[sc], 0), a.P_total), end = min(max(a.cloud_off[sc + 1], first), a.P_total);
  *e = sc; *cloud = a.cloud + (size_t)first * 2; *P = end - first;
  return true;
}

// np points from `cloud` (np, 2) into the planes cl[c][e]: consecutive threads read consecutive words
__device__ __forceinline__ void mg_load_tile(float (*cl)[MG_TILE], const float* __restrict__ cloud, int np, int tid) {
  for (int i = tid; i < np * 2; i += 256) cl[i & 1][i >> 1] = cloud[i];
}

// -dC/dq of the pairs (q, tile point e), e = lane, lane + 64, ... < np, summed over the wave: the same bits in every lane
__device__ __forceinline__ void mg_force(float q0, float q1, const float (*cl)[MG_TILE], int np, int lane, float r, float r2hi, float* s0,
                                         float* s1) {
  float a0 = 0.f, a1 = 0.f;
  for (int e = lane; e < np; e += 64) {
    const float dx = sub(q0, cl[0][e]), dy = sub(q1, cl[1][e]);
    const float d2 = add(mul(dx, dx), mul(dy, dy));
    if (d2 < r2hi) {                              // cheap filter in front of the square root; `d < r` decides
      const float d = __fsqrt_rn(d2);
      if (d < r && d > 0.f) {                     // a pair at distance zero contributes no gradient
        const float f = __fdiv_rn(sub(r, d), d);
        a0 = sub(a0, mul(f, dx)); a1 = sub(a1, mul(f, dy));
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a0 = add(a0, __shfl_xor(a0, m));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a1 = add(a1, __shfl_xor(a1, m));
  *s0 = a0; *s1 = a1;
}

// the pairs' cost values 1/2 (r - d)^2 of one lane, in fp64, added to *t in the lane's order
__device__ __forceinline__ void mg_pair_cost(float q0, float q1, const float (*cl)[MG_TILE], int np, int lane, float r, float r2hi, double* t) {
  for (int e = lane; e < np; e += 64) {
    const float dx = sub(q0, cl[0][e]), dy = sub(q1, cl[1][e]);
    const float d2 = add(mul(dx, dx), mul(dy, dy));
    if (d2 < r2hi) {
      const float d = __fsqrt_rn(d2);
      if (d < r) { const float u = sub(r, d); *t += (double)mul(0.5f, mul(u, u)); }
    }
  }
}

__global__ __launch_bounds__(256) void guide_step_moving_kernel(MovingGuideArgs a) {
  __shared__ float cl[2][MG_TILE];          // the static cloud's current tile
  __shared__ float mv[2][MG_TILE];          // the moving cloud, resident
  __shared__ float pos[MG_MAXH][2];         // the working copy: pinned waypoints hold their pinned values
  __shared__ float trk[MG_MAXH][2];         // delta_h
  __shared__ float gob[MG_MAXH][2];         // d C_obs / d p_h
  __shared__ float gmv[MG_MAXH][2];         // d C_mov / d p_h
  __shared__ float acc[MG_MAXH][2];         // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ int pin[MG_MAXH];              // != 0: pinned
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  const float* cloud; int P, e;
  if (!mg_scene(a, b, &e, &cloud, &P)) return;
  if (a.est && a.est[e].active == 0) return;                     // an ended episode's rows stay as they are (uniform over the block)
  const int n_first = a.pin_first ? a.pin_first[b] : a.est ? a.est[e].n_hist : a.rst ? a.rst->n_hist : 0;
  float* tr = a.traj + (size_t)b * H * S;
  const bool obs = a.w_obs != 0.f && P > 0, mov = a.w_mov != 0.f && a.n_mov > 0;
  if (tid < H) {
    const int h = tid;
    int k_last = -1;
    for (int k = 0; k < a.hc.n; ++k) if (a.hc.idx[k] == h) k_last = k;        // later entries win, like hard_value
    pin[h] = (k_last >= 0 || h < n_first || h == H - 1) ? 1 : 0;
    const float* src = k_last >= 0 ? a.hc.val + ((size_t)k_last * a.B + b) * S : tr + (size_t)h * S;
    if (a.hist && h < n_first) src = a.hist + ((size_t)e * H + h) * S;        // replan_pin_row's order: conditions, history, goal
    if (a.x_clean && h == H - 1) src = a.x_clean + ((size_t)e * H + h) * S;
    pos[h][0] = src[0]; pos[h][1] = src[1];
    if (mov) { trk[h][0] = a.track[((size_t)e * H + h) * 2]; trk[h][1] = a.track[((size_t)e * H + h) * 2 + 1]; }
  }
  if (mov) mg_load_tile(mv, a.mov + (size_t)e * a.n_mov * 2, a.n_mov, tid);
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);
  const float rm = a.radius_mov, rm2hi = mul(mul(rm, rm), 1.00001f);
  for (int it = 0; it < a.n_iter; ++it) {
    if (tid < H) { gob[tid][0] = 0.f; gob[tid][1] = 0.f; gmv[tid][0] = 0.f; gmv[tid][1] = 0.f; }
    if (obs) {
      for (int p0 = 0; p0 < P; p0 += MG_TILE) {
        const int np = min(MG_TILE, P - p0);
        __syncthreads();
        if (it == 0 || P > MG_TILE) mg_load_tile(cl, cloud + (size_t)p0 * 2, np, tid);
        __syncthreads();
        for (int h = wave; h < H; h += 4) {
          if (pin[h]) continue;                       // its gradient is zeroed anyway (uniform over the wave)
          float s0, s1;
          mg_force(pos[h][0], pos[h][1], cl, np, lane, r, r2hi, &s0, &s1);
          if (lane == 0) { gob[h][0] = add(gob[h][0], s0); gob[h][1] = add(gob[h][1], s1); }
        }
      }
    }
    if (mov) {
      __syncthreads();                                // mv, trk and the positions of this iteration are in place
      for (int h = wave; h < H; h += 4) {
        if (pin[h]) continue;
        float s0, s1;
        mg_force(sub(pos[h][0], trk[h][0]), sub(pos[h][1], trk[h][1]), mv, a.n_mov, lane, rm, rm2hi, &s0, &s1);
        if (lane == 0) { gmv[h][0] = add(gmv[h][0], s0); gmv[h][1] = add(gmv[h][1], s1); }
      }
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
        acc[tid][c] = (tid >= 1 && tid <= H - 2) ? add(sub(pos[tid + 1][c], mul(2.f, pos[tid][c])), pos[tid - 1][c]) : 0.f;
    }
    __syncthreads();
    float g[2];
    double n2 = 0.0;
    if (tid < H) {
      const int h = tid;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        // smoothness: (p_h - p_{h+1}) + (p_h - p_{h-1}); acceleration: a_{h-1} - 2 a_h + a_{h+1}
        float gs = 0.f, ga = mul(-2.f, acc[h][c]);
        if (h + 1 < H) { gs = add(gs, sub(pos[h][c], pos[h + 1][c])); ga = add(ga, acc[h + 1][c]); }
        if (h >= 1) { gs = add(gs, sub(pos[h][c], pos[h - 1][c])); ga = add(ga, acc[h - 1][c]); }
        float v = add(mul(a.w_smooth, gs), mul(a.w_acc, ga));
        if (mov) v = add(mul(a.w_mov, gmv[h][c]), v);
        if (obs) v = add(mul(a.w_obs, gob[h][c]), v);
        g[c] = pin[h] ? 0.f : v;
        n2 += (double)g[c] * (double)g[c];
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m);
    if (lane == 0) red[wave] = n2;
    __syncthreads();
    const float n = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
    float s = 1.f;
    if (a.max_norm > 0.f && n > 0.f) s = fminf(1.f, __fdiv_rn(a.max_norm, n));
    const float ss = mul(a.step, s);
    if (tid < H && !pin[tid]) {
#pragma unroll
      for (int c = 0; c < 2; ++c) pos[tid][c] = sub(pos[tid][c], mul(ss, g[c]));
    }
  }
  // (every thread writes back only what it updated last: no barrier needed)
  if (a.n_iter > 0 && tid < H && !pin[tid]) { tr[(size_t)tid * S] = pos[tid][0]; tr[(size_t)tid * S + 1] = pos[tid][1]; }
}

// the four unweighted terms of one row: fp32 pair values, fp64 sums (a thread's own pairs in order -- static tiles, then the moving tile --
// then lanes, then waves)
__global__ __launch_bounds__(256) void guide_cost_moving_kernel(MovingGuideArgs a, double* __restrict__ terms) {
  __shared__ float cl[2][MG_TILE];
  __shared__ float pos[MG_MAXH][2];
  __shared__ float trk[MG_MAXH][2];
  __shared__ double red[4][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  const float* cloud; int P, e;
  if (!mg_scene(a, b, &e, &cloud, &P)) {
    if (tid < 4) terms[(size_t)b * 4 + tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const float* tr = a.traj + (size_t)b * H * S;
  const bool mov = a.n_mov > 0;
  if (tid < H) {
    pos[tid][0] = tr[(size_t)tid * S]; pos[tid][1] = tr[(size_t)tid * S + 1];
    if (mov) { trk[tid][0] = a.track[((size_t)e * H + tid) * 2]; trk[tid][1] = a.track[((size_t)e * H + tid) * 2 + 1]; }
  }
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);
  const float rm = a.radius_mov, rm2hi = mul(mul(rm, rm), 1.00001f);
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < P; p0 += MG_TILE) {
    const int np = min(MG_TILE, P - p0);
    __syncthreads();
    mg_load_tile(cl, cloud + (size_t)p0 * 2, np, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4) mg_pair_cost(pos[h][0], pos[h][1], cl, np, lane, r, r2hi, &t[0]);
  }
  if (mov) {
    __syncthreads();
    mg_load_tile(cl, a.mov + (size_t)e * a.n_mov * 2, a.n_mov, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4)
      mg_pair_cost(sub(pos[h][0], trk[h][0]), sub(pos[h][1], trk[h][1]), cl, a.n_mov, lane, rm, rm2hi, &t[1]);
  }
  __syncthreads();
  if (tid < H) {
    const int h = tid;
    if (h + 1 < H) {
      const float dx = sub(pos[h + 1][0], pos[h][0]), dy = sub(pos[h + 1][1], pos[h][1]);
      t[2] = (double)mul(0.5f, add(mul(dx, dx), mul(dy, dy)));
    }
    if (h >= 1 && h + 1 < H) {
      const float ax = add(sub(pos[h + 1][0], mul(2.f, pos[h][0])), pos[h - 1][0]);
      const float ay = add(sub(pos[h + 1][1], mul(2.f, pos[h][1])), pos[h - 1][1]);
      t[3] = (double)mul(0.5f, add(mul(ax, ax), mul(ay, ay)));
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t[k] += __shfl_xor(t[k], m);
    if (lane == 0) red[k][wave] = t[k];
  }
  __syncthreads();
  if (tid < 4) terms[(size_t)b * 4 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

__global__ __launch_bounds__(256) void copy_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
}

int check_moving_args(const MovingGuideArgs& a) {
  RAMP_REQUIRE(a.traj && a.B > 0 && a.H > 0 && a.H <= MG_MAXH && a.S >= 2, "bad moving-guide dims (H up to 128, state width at least 2)");
  RAMP_REQUIRE(a.n_scenes >= 1 && a.cloud_off && a.P_total >= 0 && (a.P_total == 0 || a.cloud), "bad moving-guide cloud table");
  RAMP_REQUIRE(a.n_mov >= 0 && a.n_mov <= MG_TILE && (a.n_mov == 0 || (a.mov && a.track)), "bad moving cloud (up to 1024 points, with its track)");
  RAMP_REQUIRE(a.hc.n == 0 || (a.hc.idx && a.hc.val), "moving guide: missing hard conditions");
  RAMP_REQUIRE(!a.hist == !a.x_clean, "moving guide: history and clean plans come together");
  return 0;
}

}  // namespace

int launch_guide_step_moving(const MovingGuideArgs& a, hipStream_t s) {
  if (int rc = check_moving_args(a)) return rc;
  RAMP_REQUIRE(a.n_iter >= 0, "moving guide: negative iteration count");
  if (a.n_iter == 0) return 0;
  hipLaunchKernelGGL(guide_step_moving_kernel, dim3(a.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_guide_cost_moving(const MovingGuideArgs& a, double* terms, hipStream_t s) {
  if (int rc = check_moving_args(a)) return rc;
  RAMP_REQUIRE(terms, "moving guide: null output");
  hipLaunchKernelGGL(guide_cost_moving_kernel, dim3(a.B), dim3(256), 0, s, a, terms);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_copy_f32(float* dst, const float* src, long n, hipStream_t s) {
  RAMP_REQUIRE(dst && src && n > 0, "bad copy");
  hipLaunchKernelGGL(copy_f32_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, s, dst, src, n);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
