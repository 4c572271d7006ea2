// Robot-robot separation of teams (ramp_team_clearance in include/ramp_hip.h): row b of a (B, H, S) batch is agent b % A of team b / A, the
// same waypoint index means the same time for every agent, and between two waypoints every agent moves on its straight segment at constant
// speed.  For a pair a < a' the difference of the two motions over segment h is itself a straight motion from D0 = p_{a,h} - p_{a',h} to
// D1 = p_{a,h+1} - p_{a',h+1}, so the closest approach has the closed form of a point against a segment: e = D1 - D0,
// t = clamp(-(D0 . e) / |e|^2, 0, 1) (0 when |e|^2 == 0), d_seg = |D0 + t e|, min-ed with |D0| and |D1| so that sep_seg <= sep_wp always.
//
// One 256-thread block owns one team: positions in LDS as [agent][D planes][H], threads run over (pair, waypoint) items -- item (k, h) is
// waypoint h of pair k and, for h < H - 1, the segment behind it.  Minima are exact and order-free, counts are integer sums (wave
// butterflies, four words in LDS, one thread finishes); the fp32 sums over the members' path lengths run serially on that thread.  One
// launch, no atomics on floats.  Built with -ffp-contract=off like clearance.hip: every product and sum is rounded once, as written.
#include "args_clearance.h"

namespace ramp {

constexpr int TMC_MAXH = 128;
constexpr int TMC_MAXA = 8;
constexpr int TMC_PAIRS = TMC_MAXA * (TMC_MAXA - 1) / 2;

namespace {
__device__ __forceinline__ float tmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float tadd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float tsub(float a, float b) { return __fsub_rn(a, b); }
template <int D> __device__ __forceinline__ float tnorm2(const float (&v)[D]) {
  float s = tadd(tmul(v[0], v[0]), tmul(v[1], v[1]));
  if (D == 3) s = tadd(s, tmul(v[2], v[2]));
  return s;
}
template <int D> __device__ __forceinline__ float tdot(const float (&u)[D], const float (&v)[D]) {
  float s = tadd(tmul(u[0], v[0]), tmul(u[1], v[1]));
  if (D == 3) s = tadd(s, tmul(u[2], v[2]));
  return s;
}
}  // namespace

template <int D>
__global__ __launch_bounds__(256) void team_clearance_kernel(TeamClearanceArgs a) {
  __shared__ float pos[TMC_MAXA][D][TMC_MAXH];
  __shared__ int pair_a[TMC_PAIRS], pair_b[TMC_PAIRS];
  __shared__ float rmin[2][4];
  __shared__ int cnt[2][4];
  __shared__ int bad;
  const int team = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.team, H = a.H, S = a.S, b0 = team * A;
  const int n_pairs = A * (A - 1) / 2;
  if (tid == 0) {
    bad = 0;
    int k = 0;
    for (int i = 0; i < A; ++i) for (int j = i + 1; j < A; ++j) { pair_a[k] = i; pair_b[k] = j; ++k; }
  }
  __syncthreads();
  int nonfinite = 0;
  for (int i = tid; i < A * H * D; i += 256) {
    const int ag = i / (H * D), r = i - ag * H * D, h = r / D, c = r - h * D;
    const float v = a.traj[((long)(b0 + ag) * H + h) * S + c];
    pos[ag][c][h] = v;
    nonfinite |= !(fabsf(v) < INFINITY);
  }
  if (nonfinite) atomicOr(&bad, 1);
  __syncthreads();
  const bool is_bad = bad != 0;                              // (uniform over the block)
  float mw = INFINITY, ms = INFINITY;
  int cw = 0, cs = 0;
  if (!is_bad) {
    for (int i = tid; i < n_pairs * H; i += 256) {
      const int k = i / H, h = i - k * H, p = pair_a[k], q = pair_b[k];
      float d0[D];
#pragma unroll
      for (int c = 0; c < D; ++c) d0[c] = tsub(pos[p][c][h], pos[q][c][h]);
      const float l0 = sqrtf(tnorm2<D>(d0));
      mw = fminf(mw, l0);
      cw += l0 < a.min_sep;
      if (h + 1 < H) {
        float d1[D], e[D], v[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { d1[c] = tsub(pos[p][c][h + 1], pos[q][c][h + 1]); e[c] = tsub(d1[c], d0[c]); }
        const float e2 = tnorm2<D>(e);
        const float t = e2 > 0.f ? fminf(fmaxf(__fdiv_rn(-tdot<D>(d0, e), e2), 0.f), 1.f) : 0.f;
#pragma unroll
        for (int c = 0; c < D; ++c) v[c] = tadd(d0[c], tmul(t, e[c]));
        const float ds = fminf(fminf(sqrtf(tnorm2<D>(v)), l0), sqrtf(tnorm2<D>(d1)));
        ms = fminf(ms, ds);
        cs += ds < a.min_sep;
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    mw = fminf(mw, __shfl_xor(mw, m)); ms = fminf(ms, __shfl_xor(ms, m));
    cw += __shfl_xor(cw, m); cs += __shfl_xor(cs, m);
  }
  if (lane == 0) { rmin[0][wave] = mw; rmin[1][wave] = ms; cnt[0][wave] = cw; cnt[1][wave] = cs; }
  __syncthreads();
  if (tid != 0) return;
  const float nan = __int_as_float(0x7fc00000);
  const float w = fminf(fminf(rmin[0][0], rmin[0][1]), fminf(rmin[0][2], rmin[0][3]));
  const float sg = fminf(fminf(fminf(rmin[1][0], rmin[1][1]), fminf(rmin[1][2], rmin[1][3])), w);
  const int nw = is_bad ? n_pairs * H : (cnt[0][0] + cnt[0][1]) + (cnt[0][2] + cnt[0][3]);
  const int ns = is_bad ? n_pairs * (H - 1) : (cnt[1][0] + cnt[1][1]) + (cnt[1][2] + cnt[1][3]);
  if (a.sep_wp) a.sep_wp[team] = is_bad ? nan : w;
  if (a.sep_seg) a.sep_seg[team] = is_bad ? nan : sg;
  if (a.wp_conflicts) a.wp_conflicts[team] = nw;
  if (a.seg_conflicts) a.seg_conflicts[team] = ns;
  // the team-level arrays of the selection: members in agent order, fp32 sums added serially
  int any = is_bad || (a.swept ? ns : nw) != 0;
  float tl = 0.f, ts = 0.f;
  for (int g = 0; g < A; ++g) {
    if (a.row_mask) any |= a.row_mask[b0 + g] != 0;
    if (a.row_len) tl = tadd(tl, a.row_len[b0 + g]);
    if (a.row_smooth) ts = tadd(ts, a.row_smooth[b0 + g]);
  }
  if (a.team_mask) a.team_mask[team] = any;
  if (a.team_len) a.team_len[team] = tl;
  if (a.team_smooth) a.team_smooth[team] = ts;
}

int launch_team_clearance(const TeamClearanceArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.traj && a.B > 0 && a.H >= 2 && a.H <= TMC_MAXH && (a.D == 2 || a.D == 3) && a.D <= a.S && a.team >= 1 && a.team <= TMC_MAXA &&
               a.B % a.team == 0, "bad team clearance dims");
  if (a.D == 3) hipLaunchKernelGGL(team_clearance_kernel<3>, dim3(a.B / a.team), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(team_clearance_kernel<2>, dim3(a.B / a.team), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
