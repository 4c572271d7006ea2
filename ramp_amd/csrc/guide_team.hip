// Teams of robots in one job (ramp_team_guide in include/ramp_hip.h): the cost guide of guide.hip plus a separation term between the rows of
// a team,
//
//   C_team = sum_{a < a'} sum_h 1/2 max(0, r_t - |p_{a,h} - p_{a',h}|)^2,
//
// over the positions p_{a,h} = x[row a of the team, h, 0:D] at equal waypoint index.  The gradient of a pair is guide_pair_force's
// arithmetic with the teammate's waypoint in the place of a cloud point.  One iteration is Jacobi: every agent's gradient is taken from
// the positions all agents had at the start of the iteration, then all agents move; the norm, the clip and the step are per agent.
//
// One 256-thread block owns one TEAM: the positions of all its agents live in LDS in two buffers (old / new), so teammates' positions never
// cross a block -- several iterations run in one launch, and an exchange between blocks inside a kernel is the pattern DESIGN.md section
// 8-3 records as broken.  No atomics, no fences.  Per iteration the agents are served one after the other with guide_core.h's pieces on
// the agent's slice of the NEW buffer (filled with the old values first, so every piece reads old positions and guide_update steps in
// place), gob / acc / red reused agent by agent; thread h adds the agent's team gradient from the OLD buffer.  Behind the last agent the
// buffers swap, behind a barrier.
//
// LDS at D = 3: tile 12 KiB + two position buffers 2 x 12 KiB + pins 4 KiB + gob / acc 3 KiB = 43 KiB (30 KiB at D = 2), static and sized
// for RAMP_TEAM_MAX agents, under the 64 KiB static limit: LDS, not the wave limit, decides occupancy here (3 blocks per CU at D = 3, 5 at
// D = 2, of 160 KiB) -- a block serves A rows, so per row that is what guide_step_kernel's 8 blocks give from A = 3 (2) on.
//
// The cloud tile: a cloud of at most one tile is loaded once per launch -- by the first agent that needs it -- and again only when an agent's
// span differs from the one the tile holds (agents of a team share a scene in every job the host lays out; the kernel never reads a stale
// tile if they do not).  Built with -ffp-contract=off like guide.hip: every product and sum is rounded once, as written.
#include "guide_core.h"

namespace ramp {

// d C_team / d p_{a,h} for thread h: teammates in ascending a', skipping a, added serially in fp32; guide_pair_force's pair arithmetic
template <int D>
__device__ __forceinline__ void team_force(const float (*old)[GUIDE_MAX_H][D], int A, int a, int h, float r, float r2hi, float (&sum)[D]) {
  float q[D];
#pragma unroll
  for (int c = 0; c < D; ++c) { q[c] = old[a][h][c]; sum[c] = 0.f; }
  for (int o = 0; o < A; ++o) {
    if (o == a) continue;
    float dx[D];
#pragma unroll
    for (int c = 0; c < D; ++c) dx[c] = sub(q[c], old[o][h][c]);
    float d2 = mul(dx[0], dx[0]);
#pragma unroll
    for (int c = 1; c < D; ++c) d2 = add(d2, mul(dx[c], dx[c]));
    if (d2 < r2hi) {
      const float d = __fsqrt_rn(d2);
      if (d < r && d > 0.f) {                 // a pair at distance zero contributes no gradient
        const float f = __fdiv_rn(sub(r, d), d);
#pragma unroll
        for (int c = 0; c < D; ++c) sum[c] = sub(sum[c], mul(f, dx[c]));
      }
    }
  }
}

// false: some row of the team has a scene index outside the table (uniform over the block)
__device__ __forceinline__ bool team_scenes_ok(const GuideArgs& g, int b0, int A) {
  if (!g.scene) return true;
  for (int a = 0; a < A; ++a) { const int sc = g.scene[b0 + a]; if (sc < 0 || sc >= g.n_scenes) return false; }
  return true;
}

template <int D>
__global__ __launch_bounds__(256) void guide_team_step_kernel(TeamGuideArgs t) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float buf[2][TEAM_MAX][GUIDE_MAX_H][D];   // the agents' working copies, old / new: pinned waypoints hold their conditioned values
  __shared__ float gob[GUIDE_MAX_H][D];
  __shared__ float acc[GUIDE_MAX_H][D];
  __shared__ int pin[TEAM_MAX][GUIDE_MAX_H];
  __shared__ double red[4];
  const GuideArgs& g = t.g;
  const int A = t.team, b0 = blockIdx.x * A, tid = threadIdx.x, H = g.H;
  if (!team_scenes_ok(g, b0, A)) return;               // the team is left unchanged as a whole
  for (int a = 0; a < A; ++a) guide_pin_hard<D>(g, b0 + a, g.traj + (size_t)(b0 + a) * H * g.S, buf[0][a], pin[a], tid);
  const float r = g.radius, r2hi = guide_r2hi(r), rt = t.radius_team, rt2hi = guide_r2hi(rt);
  const GuideWeights w = {g.w_obs, g.w_smooth, g.w_acc, g.max_norm, g.step};
  const bool team_on = t.w_team != 0.f && A > 1;
  const float* tile_cloud = nullptr;                   // the span a one-tile cloud in `cl` was loaded from (uniform)
  int tile_P = -1, cur = 0;
  __syncthreads();
  for (int it = 0; it < g.n_iter; ++it) {
    const float (*old)[GUIDE_MAX_H][D] = buf[cur];
    float (*nw)[GUIDE_MAX_H][D] = buf[cur ^ 1];
    for (int a = 0; a < A; ++a) {
      GuideSpan sp;
      guide_scene(g, D, b0 + a, &sp);                  // (inside the table: checked above)
      const bool obs = g.w_obs != 0.f && sp.P > 0;
      if (tid < H) {
#pragma unroll
        for (int c = 0; c < D; ++c) nw[a][tid][c] = old[a][tid][c];
      }
      if (obs) {
        const bool fresh = sp.P > GUIDE_TILE || sp.cloud != tile_cloud || sp.P != tile_P;
        guide_cloud_force<D>(cl, nw[a], gob, pin[a], sp.cloud, sp.P, H, fresh ? 0 : 1, r, r2hi, tid);
        tile_cloud = sp.P > GUIDE_TILE ? nullptr : sp.cloud;      // (a longer cloud leaves its last tile behind)
        tile_P = sp.P > GUIDE_TILE ? -1 : sp.P;
      }
      guide_second_difference<D>(nw[a], acc, H, tid);
      float gt[D] = {};
      if (team_on && tid < H) team_force<D>(old, A, a, tid, rt, rt2hi, gt);
      guide_update<D>(nw[a], acc, gob, pin[a], red, H, w, obs, team_on, t.w_team, gt, tid);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (g.n_iter > 0)
    for (int a = 0; a < A; ++a) guide_write_back<D>(g.traj + (size_t)(b0 + a) * H * g.S, H, g.S, buf[cur][a], pin[a], tid);
}

// per row {C_obs, C_smooth, C_acc} with guide_cost_kernel's bits, and the row's share of the team term: thread h adds the fp32 values
// 1/2 (r_t - d)^2 of its teammates (a' ascending; d correctly rounded) in fp64, the threads' sums are reduced like the other columns
template <int D>
__global__ __launch_bounds__(256) void guide_team_cost_kernel(TeamGuideArgs t, double* __restrict__ terms) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[TEAM_MAX][GUIDE_MAX_H][D];
  __shared__ double red[4][4];
  const GuideArgs& g = t.g;
  const int A = t.team, b0 = blockIdx.x * A, tid = threadIdx.x, H = g.H;
  if (!team_scenes_ok(g, b0, A)) {
    for (int a = 0; a < A; ++a) guide_store_nan<4>(terms + (size_t)(b0 + a) * 4, tid);
    return;
  }
  for (int a = 0; a < A; ++a) guide_load_pos<D>(g.traj + (size_t)(b0 + a) * H * g.S, H, g.S, pos[a], tid);
  const float rt = t.radius_team, rt2hi = guide_r2hi(rt);
  for (int a = 0; a < A; ++a) {
    __syncthreads();                                   // the positions are in place; the last agent's sums have left `red`
    GuideSpan sp;
    guide_scene(g, D, b0 + a, &sp);
    double v[4] = {0.0, 0.0, 0.0, 0.0};                // {C_obs, C_smooth, C_acc, the row's team share}
    guide_cloud_cost<D>(cl, pos[a], sp.cloud, sp.P, H, g.radius, guide_r2hi(g.radius), tid, &v[0]);
    __syncthreads();
    guide_stencil_costs<D>(pos[a], H, tid, &v[1], &v[2]);
    if (tid < H && rt > 0.f) {
      for (int o = 0; o < A; ++o) {
        if (o == a) continue;
        float d2 = 0.f;
#pragma unroll
        for (int c = 0; c < D; ++c) { const float dx = sub(pos[a][tid][c], pos[o][tid][c]); d2 = c == 0 ? mul(dx, dx) : add(d2, mul(dx, dx)); }
        if (d2 < rt2hi) {
          // sqrtf: the correctly rounded root.  __fsqrt_rn is the bare hardware instruction (1 ulp), which guide_pair_cost's sums over
          // thousands of points average out and a row's few pair values would show
          const float d = sqrtf(d2);
          if (d < rt) { const float u = sub(rt, d); v[3] += (double)mul(0.5f, mul(u, u)); }
        }
      }
    }
    guide_store_terms<4>(v, red, terms + (size_t)(b0 + a) * 4, tid);
  }
}

static int check_team_args(const TeamGuideArgs& a) {
  if (int rc = require_guide_args(a.g, "bad team guide dims (H up to 128)", "team guide point_dim must be 2 or 3 and at most the state width",
                                  "team guide: missing hard conditions")) return rc;
  RAMP_REQUIRE(a.team >= 1 && a.team <= TEAM_MAX && a.g.B % a.team == 0, "team guide: team size outside 1 .. 8 or no divisor of the batch");
  return 0;
}

int launch_guide_team_step(const TeamGuideArgs& a, hipStream_t s) {
  if (int rc = check_team_args(a)) return rc;
  RAMP_REQUIRE(a.g.n_iter >= 0, "team guide: negative iteration count");
  if (a.team == 1 || a.w_team == 0.f) return launch_guide_step(a.g, s);
  if (a.g.n_iter == 0) return 0;
  if (a.g.D == 2) hipLaunchKernelGGL(guide_team_step_kernel<2>, dim3(a.g.B / a.team), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(guide_team_step_kernel<3>, dim3(a.g.B / a.team), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_guide_team_cost(const TeamGuideArgs& a, double* terms, hipStream_t s) {
  if (int rc = check_team_args(a)) return rc;
  RAMP_REQUIRE(terms, "team guide: null output");
  if (a.g.D == 2) hipLaunchKernelGGL(guide_team_cost_kernel<2>, dim3(a.g.B / a.team), dim3(256), 0, s, a, terms);
  else hipLaunchKernelGGL(guide_team_cost_kernel<3>, dim3(a.g.B / a.team), dim3(256), 0, s, a, terms);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
