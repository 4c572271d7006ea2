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
// the clip and the update run in the same launch, once per iteration.  The pieces are guide_core.h's, which guide_replan.hip and
// guide_prims.hip build on too; this file holds the two kernels that are nothing but those pieces.
//
// Tile: 1024 points as three (two) planes of fp32 = 12 (8) KiB -- lane l reads word l of a plane, so every ds_read_b32 of the inner loop is
// conflict-free, a tile gives each lane 16 points per waypoint (the 6-step shuffle reduction that follows costs about one point's work per
// plane) and the block's 17 KiB leave the wave limit, not LDS (160 KiB per CU), to decide occupancy.  A cloud of at most one tile is loaded
// once per launch; a longer one is re-read from L2 on every iteration.
//
// The order of the fp32 sums over points is stated in guide_core.h.  Built with -ffp-contract=off like sampler.hip: every product and sum
// is rounded once, as written.
#include "guide_core.h"

namespace ramp {

template <int D>
__global__ __launch_bounds__(256) void guide_step_kernel(GuideArgs a) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAX_H][D];     // the working copy: pinned waypoints hold their conditioned values
  __shared__ float gob[GUIDE_MAX_H][D];     // d C_obs / d p_h
  __shared__ float acc[GUIDE_MAX_H][D];     // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ int pin[GUIDE_MAX_H];          // 1 + the last hard condition that names waypoint h, 0 = free
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x, H = a.H;
  GuideSpan sp;
  if (!guide_scene(a, a.D, b, &sp)) return;
  float* tr = a.traj + (size_t)b * H * a.S;
  guide_pin_hard<D>(a, b, tr, pos, pin, tid);
  const bool obs = a.w_obs != 0.f && sp.P > 0;
  const float r = a.radius, r2hi = guide_r2hi(r);
  const GuideWeights w = {a.w_obs, a.w_smooth, a.w_acc, a.max_norm, a.step};
  const float none[D] = {};                 // this kernel has no term of its own
  for (int it = 0; it < a.n_iter; ++it) {
    if (obs) guide_cloud_force<D>(cl, pos, gob, pin, sp.cloud, sp.P, H, it, r, r2hi, tid);
    guide_second_difference<D>(pos, acc, H, tid);
    guide_update<D>(pos, acc, gob, pin, red, H, w, obs, false, 0.f, none, tid);
  }
  if (a.n_iter > 0) guide_write_back<D>(tr, H, a.S, pos, pin, tid);
}

// the three unweighted terms of one trajectory: fp32 pair values, fp64 sums (a thread's own pairs in order, then lanes, then waves)
template <int D>
__global__ __launch_bounds__(256) void guide_cost_kernel(GuideArgs a, double* __restrict__ terms) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAX_H][D];
  __shared__ double red[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, H = a.H;
  GuideSpan sp;
  if (!guide_scene(a, a.D, b, &sp)) { guide_store_nan<3>(terms + (size_t)b * 3, tid); return; }
  guide_load_pos<D>(a.traj + (size_t)b * H * a.S, H, a.S, pos, tid);
  double t[3] = {0.0, 0.0, 0.0};      // {C_obs, C_smooth, C_acc}
  guide_cloud_cost<D>(cl, pos, sp.cloud, sp.P, H, a.radius, guide_r2hi(a.radius), tid, &t[0]);
  __syncthreads();
  guide_stencil_costs<D>(pos, H, tid, &t[1], &t[2]);
  guide_store_terms<3>(t, red, terms + (size_t)b * 3, tid);
}

static int check_guide_args(const GuideArgs& a) {
  return require_guide_args(a, "bad guide dims (H up to 128)", "guide point_dim must be 2 or 3 and at most the state width",
                            "guide: missing hard conditions");
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
