// Cost guidance of the replanning jobs (ramp_replan_guide in include/ramp_hip.h): guide.hip's clipped gradient steps on
//
//   C = w_obs sum_h sum_j 1/2 max(0, r - |p_h - c_j|)^2 + w_mov sum_h sum_j 1/2 max(0, r_mov - |(p_h - delta_h) - m_j|)^2
//       + w_smooth sum_h 1/2 |p_{h+1} - p_h|^2 + w_acc sum_h 1/2 |p_{h+1} - 2 p_h + p_{h-1}|^2
//
// over the positions p_h = x[h, 0:2] of one candidate, the static cloud c of its episode, the episode's moving cloud m (the pursuer's sphere
// points now) and its track delta (H, 2), the cloud's predicted displacement at waypoint h -- with pins that differ from row to row: the
// executed history [0, n_hist) of the row's episode, the goal H - 1 and the hard-conditioned waypoints (MovingGuideArgs in args_sampler.h).
//
// The structure is guide_step_kernel's, built from the same pieces (guide_core.h, at D = 2): one 256-thread block per row, positions, pins
// and the track in LDS for all iterations of the launch, the clouds as planes of 1024 fp32 (lane l reads word l: every ds_read_b32 of the
// inner loop is conflict-free), wave w owns waypoints w, w + 4, ..., lanes split a tile's points, wavefront-shuffle reductions, stencils,
// norm, clip and update in the same launch.  This file adds the moving term, the track and the per-row pins.  The moving cloud is at most
// one tile and has planes of its own (8 KiB), so it is loaded once per launch and a static cloud of at most one tile stays resident beside
// it; the block's 22 KiB of LDS leave the wave limit to decide occupancy.
//
// Order of the fp32 sums over points: guide_core.h's rule per cloud (a lane's points in order, a butterfly over the lanes, the tiles in
// order), the static tiles first, then the moving tile; g = w_obs g_obs + (w_mov g_mov + (w_smooth g_smooth + w_acc g_acc)) is guide_update's
// sum with the moving term as its extra term, so that without a moving term the bits are guide_step_kernel<2>'s.  Built with
// -ffp-contract=off: every product and sum is rounded once, as written.
#include "guide_core.h"

#include <algorithm>

namespace ramp {

namespace {

__global__ __launch_bounds__(256) void guide_step_moving_kernel(MovingGuideArgs a) {
  __shared__ float cl[2][GUIDE_TILE];       // the static cloud's current tile
  __shared__ float mv[2][GUIDE_TILE];       // the moving cloud, resident
  __shared__ float pos[GUIDE_MAX_H][2];     // the working copy: pinned waypoints hold their pinned values
  __shared__ float trk[GUIDE_MAX_H][2];     // delta_h
  __shared__ float gob[GUIDE_MAX_H][2];     // d C_obs / d p_h
  __shared__ float gmv[GUIDE_MAX_H][2];     // d C_mov / d p_h
  __shared__ float acc[GUIDE_MAX_H][2];     // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ int pin[GUIDE_MAX_H];          // != 0: pinned
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  GuideSpan sp;
  if (!guide_scene(a, 2, b, &sp)) return;
  const int e = sp.sc;
  if (a.est && a.est[e].active == 0) return;                     // an ended episode's rows stay as they are (uniform over the block)
  const int n_first = a.pin_first ? a.pin_first[b] : a.est ? a.est[e].n_hist : 0;
  float* tr = a.traj + (size_t)b * H * S;
  const bool obs = a.w_obs != 0.f && sp.P > 0, mov = a.w_mov != 0.f && a.n_mov > 0;
  if (tid < H) {
    const int h = tid, k_last = guide_last_cond(a.hc, h);
    pin[h] = (k_last >= 0 || h < n_first || h == H - 1) ? 1 : 0;
    const float* src = k_last >= 0 ? a.hc.val + ((size_t)k_last * a.B + b) * S : tr + (size_t)h * S;
    if (a.hist && h < n_first) src = a.hist + ((size_t)e * H + h) * S;        // replan_pin_row's order: conditions, history, goal
    if (a.x_clean && h == H - 1) src = a.x_clean + ((size_t)e * H + h) * S;
    pos[h][0] = src[0]; pos[h][1] = src[1];
    if (mov) { trk[h][0] = a.track[((size_t)e * H + h) * 2]; trk[h][1] = a.track[((size_t)e * H + h) * 2 + 1]; }
  }
  if (mov) guide_load_tile<2>(mv, a.mov + (size_t)e * a.n_mov * 2, a.n_mov, tid);
  const float r = a.radius, r2hi = guide_r2hi(r);
  const float rm = a.radius_mov, rm2hi = guide_r2hi(rm);
  const GuideWeights w = {a.w_obs, a.w_smooth, a.w_acc, a.max_norm, a.step};
  for (int it = 0; it < a.n_iter; ++it) {
    if (obs) guide_cloud_force<2>(cl, pos, gob, pin, sp.cloud, sp.P, H, it, r, r2hi, tid);
    if (mov) {
      if (tid < H) { gmv[tid][0] = 0.f; gmv[tid][1] = 0.f; }
      __syncthreads();                                // mv, trk and the positions of this iteration are in place
      for (int h = wave; h < H; h += 4) {
        if (pin[h]) continue;
        const float q[2] = {sub(pos[h][0], trk[h][0]), sub(pos[h][1], trk[h][1])};
        float sum[2];
        guide_pair_force<2>(q, mv, a.n_mov, lane, rm, rm2hi, sum);
        if (lane == 0) { gmv[h][0] = add(gmv[h][0], sum[0]); gmv[h][1] = add(gmv[h][1], sum[1]); }
      }
    }
    guide_second_difference<2>(pos, acc, H, tid);
    float gm[2] = {0.f, 0.f};                         // d C_mov / d p_h of thread h
    if (mov && tid < H) { gm[0] = gmv[tid][0]; gm[1] = gmv[tid][1]; }
    guide_update<2>(pos, acc, gob, pin, red, H, w, obs, mov, a.w_mov, gm, tid);
  }
  if (a.n_iter > 0) guide_write_back<2>(tr, H, S, pos, pin, tid);
}

// the four unweighted terms of one row: fp32 pair values, fp64 sums (a thread's own pairs in order -- static tiles, then the moving tile --
// then lanes, then waves)
__global__ __launch_bounds__(256) void guide_cost_moving_kernel(MovingGuideArgs a, double* __restrict__ terms) {
  __shared__ float cl[2][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAX_H][2];
  __shared__ float trk[GUIDE_MAX_H][2];
  __shared__ double red[4][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H;
  GuideSpan sp;
  if (!guide_scene(a, 2, b, &sp)) { guide_store_nan<4>(terms + (size_t)b * 4, tid); return; }
  const int e = sp.sc;
  const bool mov = a.n_mov > 0;
  guide_load_pos<2>(a.traj + (size_t)b * H * a.S, H, a.S, pos, tid);
  if (mov && tid < H) { trk[tid][0] = a.track[((size_t)e * H + tid) * 2]; trk[tid][1] = a.track[((size_t)e * H + tid) * 2 + 1]; }
  double t[4] = {0.0, 0.0, 0.0, 0.0};      // {C_obs, C_mov, C_smooth, C_acc}
  guide_cloud_cost<2>(cl, pos, sp.cloud, sp.P, H, a.radius, guide_r2hi(a.radius), tid, &t[0]);
  if (mov) {
    __syncthreads();
    guide_load_tile<2>(cl, a.mov + (size_t)e * a.n_mov * 2, a.n_mov, tid);
    __syncthreads();
    for (int h = wave; h < H; h += 4) {
      const float q[2] = {sub(pos[h][0], trk[h][0]), sub(pos[h][1], trk[h][1])};
      guide_pair_cost<2>(q, cl, a.n_mov, lane, a.radius_mov, guide_r2hi(a.radius_mov), &t[1]);
    }
  }
  __syncthreads();
  guide_stencil_costs<2>(pos, H, tid, &t[2], &t[3]);
  guide_store_terms<4>(t, red, terms + (size_t)b * 4, tid);
}

__global__ __launch_bounds__(256) void copy_f32_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
}

int check_moving_args(const MovingGuideArgs& a) {
  const char* dims = "bad moving-guide dims (H up to 128, state width at least 2)";
  if (int rc = require_guide_common(a, dims, "bad moving-guide cloud table", "moving guide: missing hard conditions")) return rc;
  RAMP_REQUIRE(a.S >= 2, dims);
  RAMP_REQUIRE(a.n_mov >= 0 && a.n_mov <= GUIDE_TILE && (a.n_mov == 0 || (a.mov && a.track)), "bad moving cloud (up to 1024 points, with its track)");
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
