// Cost-gradient guidance (ramp_cost_guide in include/ramp_hip.h): a few clipped gradient steps on a differentiable trajectory cost,
//
//   C = w_obs sum_h sum_j 1/2 max(0, r - |p_h - c_j|)^2 + w_smooth sum_h 1/2 |p_{h+1} - p_h|^2 + w_acc sum_h 1/2 |p_{h+1} - 2 p_h + p_{h-1}|^2
//
// over the positions p_h = x[h, 0:D] of one trajectory and the cloud c of its scene, D = 2 or 3.  This is no mirror of reference code: the
// reference's guide_gradient_steps is a stub (sample_functionsdynamic.py:280-292); the definition is the header's.
//
// One 256-thread block owns one trajectory, as apf_kernel does: its positions live in LDS for all iterations of the launch, its scene's cloud
// streams through LDS in tiles of GUIDE_TILE points (selected by the scene / offset tables), wave w owns waypoints w, w + 4, ..., lanes split
// the tile's points and the per-waypoint force sums are reduced with wavefront shuffles.  Stencils, pinning, the norm (block reduction, fp64),
// the clip and the update run in the same launch, once per iteration.
//
// Tile: 1024 points as three (two) planes of fp32 = 12 (8) KiB -- lane l reads word l of a plane, so every ds_read_b32 of the inner loop is
// conflict-free, a tile gives each lane 16 points per waypoint (the 6-step shuffle reduction that follows costs about one point's work per
// plane) and the block's 17 KiB leave the wave limit, not LDS (160 KiB per CU), to decide occupancy.  A cloud of at most one tile is loaded
// once per launch; a longer one is re-read from L2 on every iteration.
//
// Order of the fp32 sums over points, fixed by (P, GUIDE_TILE) alone: lane l adds points l, l + 64, ... of a tile in that order, the 64 lane
// sums are added in a butterfly (xor 32, 16, .., 1: the same bits in every lane), the tiles' sums are added in tile order.  Built with
// -ffp-contract=off like sampler.hip: every product and sum below is rounded once, as written.
#include "args_sampler.h"

namespace ramp {

constexpr int GUIDE_TILE = 1024;
constexpr int GUIDE_MAXH = 128;

namespace {

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// the block's scene: its span [first, first + P) of the concatenated clouds, clamped to the table's total.  false: a scene index outside
// the table (uniform over the block) -- the trajectory is left as it is
__device__ __forceinline__ bool guide_scene(const GuideArgs& a, int b, const float** cloud, int* P) {
  const int sc = a.scene ? a.scene[b] : 0;
  if (sc < 0 || sc >= a.n_scenes) return false;
  const int first = min(max(a.cloud_off[sc], 0), a.P_total), end = min(max(a.cloud_off[sc + 1], first), a.P_total);
  *cloud = a.cloud + (size_t)first * a.D; *P = end - first;
  return true;
}

// np points from `cloud` (np, D) into the planes cl[c][e]: consecutive threads read consecutive words
template <int D>
__device__ __forceinline__ void guide_load_tile(float (*cl)[GUIDE_TILE], const float* __restrict__ cloud, int np, int tid) {
  for (int i = tid; i < np * D; i += 256) { const int e = i / D; cl[i - e * D][e] = cloud[i]; }
}

}  // namespace

template <int D>
__global__ __launch_bounds__(256) void guide_step_kernel(GuideArgs a) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAXH][D];      // the working copy: pinned waypoints hold their conditioned values
  __shared__ float gob[GUIDE_MAXH][D];      // d C_obs / d p_h
  __shared__ float acc[GUIDE_MAXH][D];      // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ int pin[GUIDE_MAXH];           // 1 + the last hard condition that names waypoint h, 0 = free
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  const float* cloud; int P;
  if (!guide_scene(a, b, &cloud, &P)) return;
  float* tr = a.traj + (size_t)b * H * S;
  if (tid < H) {
    int k_last = -1;
    for (int k = 0; k < a.hc.n; ++k) if (a.hc.idx[k] == tid) k_last = k;      // later entries win, like hard_value
    pin[tid] = k_last + 1;
    const float* src = k_last >= 0 ? a.hc.val + ((size_t)k_last * a.B + b) * S : tr + (size_t)tid * S;
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = src[c];
  }
  const bool obs = a.w_obs != 0.f && P > 0;
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);      // cheap filter in front of the square root; `d < r` decides
  for (int it = 0; it < a.n_iter; ++it) {
    if (obs) {
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
          for (int c = 0; c < D; ++c) { q[c] = pos[h][c]; sum[c] = 0.f; }
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
          if (lane == 0) {
#pragma unroll
            for (int c = 0; c < D; ++c) gob[h][c] = add(gob[h][c], sum[c]);
          }
        }
      }
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
      for (int c = 0; c < D; ++c)
        acc[tid][c] = (tid >= 1 && tid <= H - 2) ? add(sub(pos[tid + 1][c], mul(2.f, pos[tid][c])), pos[tid - 1][c]) : 0.f;
    }
    __syncthreads();
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
        float v = add(mul(a.w_smooth, gs), mul(a.w_acc, ga));
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
      for (int c = 0; c < D; ++c) pos[tid][c] = sub(pos[tid][c], mul(ss, g[c]));
    }
  }
  // (every thread writes back only what it updated last: no barrier needed)
  if (a.n_iter > 0 && tid < H && !pin[tid]) {
#pragma unroll
    for (int c = 0; c < D; ++c) tr[(size_t)tid * S + c] = pos[tid][c];
  }
}

// the three unweighted terms of one trajectory: fp32 pair values, fp64 sums (a thread's own pairs in order, then lanes, then waves)
template <int D>
__global__ __launch_bounds__(256) void guide_cost_kernel(GuideArgs a, double* __restrict__ terms) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAXH][D];
  __shared__ double red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  const float* cloud; int P;
  if (!guide_scene(a, b, &cloud, &P)) {
    if (tid < 3) terms[(size_t)b * 3 + tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const float* tr = a.traj + (size_t)b * H * S;
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = tr[(size_t)tid * S + c];
  }
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);
  double t[3] = {0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < P; p0 += GUIDE_TILE) {
    const int np = min(GUIDE_TILE, P - p0);
    __syncthreads();
    guide_load_tile<D>(cl, cloud + (size_t)p0 * D, np, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4) {
      float q[D];
#pragma unroll
      for (int c = 0; c < D; ++c) q[c] = pos[h][c];
      for (int e = lane; e < np; e += 64) {
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < D; ++c) { const float dx = sub(q[c], cl[c][e]); d2 = c == 0 ? mul(dx, dx) : add(d2, mul(dx, dx)); }
        if (d2 < r2hi) {
          const float d = __fsqrt_rn(d2);
          if (d < r) { const float u = sub(r, d); t[0] += (double)mul(0.5f, mul(u, u)); }
        }
      }
    }
  }
  __syncthreads();
  if (tid < H) {
    const int h = tid;
    if (h + 1 < H) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) { const float dx = sub(pos[h + 1][c], pos[h][c]); v = c == 0 ? mul(dx, dx) : add(v, mul(dx, dx)); }
      t[1] = (double)mul(0.5f, v);
    }
    if (h >= 1 && h + 1 < H) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const float ac = add(sub(pos[h + 1][c], mul(2.f, pos[h][c])), pos[h - 1][c]);
        v = c == 0 ? mul(ac, ac) : add(v, mul(ac, ac));
      }
      t[2] = (double)mul(0.5f, v);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t[k] += __shfl_xor(t[k], m);
    if (lane == 0) red[k][wave] = t[k];
  }
  __syncthreads();
  if (tid < 3) terms[(size_t)b * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

static int check_guide_args(const GuideArgs& a) {
  RAMP_REQUIRE(a.traj && a.B > 0 && a.H > 0 && a.H <= GUIDE_MAXH, "bad guide dims (H up to 128)");
  RAMP_REQUIRE((a.D == 2 || a.D == 3) && a.D <= a.S, "guide point_dim must be 2 or 3 and at most the state width");
  RAMP_REQUIRE(a.n_scenes >= 1 && a.cloud_off && a.P_total >= 0 && (a.P_total == 0 || a.cloud), "bad guide cloud table");
  RAMP_REQUIRE(a.hc.n == 0 || (a.hc.idx && a.hc.val), "guide: missing hard conditions");
  return 0;
}

int launch_guide_step(const GuideArgs& a, hipStream_t s) {
  if (int rc = check_guide_args(a)) return rc;
  RAMP_REQUIRE(a.n_iter >= 0, "guide: negative iteration count");
  if (a.n_iter == 0) return 0;
  if (a.D == 2) hipLaunchKernelGGL(guide_step_kernel<2>, dim3(a.B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(guide_step_kernel<3>, dim3(a.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_guide_cost(const GuideArgs& a, double* terms, hipStream_t s) {
  if (int rc = check_guide_args(a)) return rc;
  RAMP_REQUIRE(terms, "guide: null output");
  if (a.D == 2) hipLaunchKernelGGL(guide_cost_kernel<2>, dim3(a.B), dim3(256), 0, s, a, terms);
  else hipLaunchKernelGGL(guide_cost_kernel<3>, dim3(a.B), dim3(256), 0, s, a, terms);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
