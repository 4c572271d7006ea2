// Swept collision checks and clearances of a batch of trajectories in 2 or 3 dimensions (ramp_traj_clearance in include/ramp_hip.h):
// for every trajectory, its waypoints p_h = x[h, 0:D] and its segments [p_h, p_{h+1}] against the axis-aligned boxes, the spheres and the
// cloud points of its own scene, plus path length and smoothness.  This is no mirror of reference code: the reference tests waypoints only
// (metrics.py:49-82, cost.py:25-54); the definitions are the header's.
//
// One 256-thread block owns one trajectory.  Its positions live in LDS as D planes of H floats: lane l reads word l of a plane, so the
// per-waypoint reads are conflict-free (an [h][3] array read with ds_read_b32 would be too -- stride 3 is coprime with the 32 banks -- but an
// [h][2] one is a 2-way conflict).
//   boxes / spheres (tens): threads [0, 128) own one waypoint each, threads [128, 256) one segment each; the scene's primitives pass
//     through LDS in chunks of CLR_PRIMS, already widened by the margin, and every thread loops the chunk (all lanes read the same word: a
//     broadcast).  Flags are integers in LDS; a segment's flag is OR-ed with its two endpoints' flags there, so seg >= wp holds by construction.
//   cloud (thousands): tiles of CLR_TILE points as D planes (12 KiB at D = 3); wave w owns waypoints / segments w, w + 4, ..., its lanes
//     split the tile's points.  Every thread keeps two running minima of SQUARED distances (sqrtf is monotone, so one root at the end gives
//     the same bits as a minimum of roots); a butterfly over the wave, four words in LDS, one thread finishes.  A minimum does not depend on
//     the order, so nothing here depends on the launch's timing.
//   path length / smoothness: traj_costs_block's order (sampler.hip): per-segment values into LDS, one thread adds them serially.
// About 20 KiB of LDS per block at D = 3: the 32-wave limit (8 blocks per CU), not LDS, decides occupancy.
// Built with -ffp-contract=off like sampler.hip: every product and sum below is rounded once, as written.
#include "args_clearance.h"

namespace ramp {

constexpr int CLR_TILE = 1024;
constexpr int CLR_MAXH = 128;
constexpr int CLR_PRIMS = 64;

namespace {

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// the scene of row b: the s in [0, n) with first[s] <= b < first[s + 1]
__device__ __forceinline__ int clr_scene_of_row(const int* __restrict__ first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= b) lo = mid; else hi = mid - 1; }
  return lo;
}
// the scene's span [*k0, *k1) of a concatenated array of `total` entries, clamped to it: a wrong table reads wrong entries, never outside
__device__ __forceinline__ void clr_span(const int* __restrict__ off, int s, int total, int* k0, int* k1) {
  *k0 = min(max(off[s], 0), total);
  *k1 = min(max(off[s + 1], *k0), total);
}
template <int D> __device__ __forceinline__ float norm2(const float (&v)[D]) {
  float s = add(mul(v[0], v[0]), mul(v[1], v[1]));
  if (D == 3) s = add(s, mul(v[2], v[2]));
  return s;
}
template <int D> __device__ __forceinline__ float dot(const float (&u)[D], const float (&v)[D]) {
  float s = add(mul(u[0], v[0]), mul(u[1], v[1]));
  if (D == 3) s = add(s, mul(u[2], v[2]));
  return s;
}

}  // namespace

template <int D>
__global__ __launch_bounds__(256) void traj_clearance_kernel(ClearanceArgs a) {
  __shared__ float cl[D][CLR_TILE];
  __shared__ float pos[D][CLR_MAXH];
  __shared__ float plo[CLR_PRIMS][D], phi[CLR_PRIMS][D];   // boxes: lower / upper corner; spheres: centre in plo, r + margin in phi[k][0]
  __shared__ int wpf[CLR_MAXH], sgf[CLR_MAXH];
  __shared__ float segl[CLR_MAXH], segs[CLR_MAXH];
  __shared__ float rmin[2][4];
  __shared__ int cnt[4];
  __shared__ int bad;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S;
  const float* __restrict__ tr = a.traj + (long)b * H * S;
  const int sc = clr_scene_of_row(a.traj_first, a.n_scenes, b);

  if (tid == 0) bad = 0;
  if (tid < CLR_MAXH) { wpf[tid] = 0; sgf[tid] = 0; }
  __syncthreads();
  int nonfinite = 0;
  for (int i = tid; i < H * D; i += 256) {
    const int h = i / D, c = i - h * D;
    const float v = tr[h * S + c];
    pos[c][h] = v;
    nonfinite |= !(fabsf(v) < INFINITY);
  }
  if (nonfinite) atomicOr(&bad, 1);
  // path length and smoothness, traj_costs_block's expressions
  for (int h = tid; h < H - 1; h += 256) {
    float d[D];
#pragma unroll
    for (int c = 0; c < D; ++c) d[c] = sub(tr[(h + 1) * S + c], tr[h * S + c]);
    segl[h] = sqrtf(norm2<D>(d));
    float ss = 0.f;
    for (int c = D; c < S; ++c) { const float dv = sub(tr[(h + 1) * S + c], tr[h * S + c]); ss = add(ss, mul(dv, dv)); }
    segs[h] = sqrtf(ss);
  }
  __syncthreads();
  const bool is_bad = bad != 0;                              // (uniform over the block)
  float mw = INFINITY, ms = INFINITY;                        // running minima of squared distances: waypoints, segments

  if (!is_bad) {
    // ---- boxes and spheres: one waypoint (threads 0..127) or one segment (threads 128..255) per thread
    const bool seg_role = tid >= CLR_MAXH;
    const int h = seg_role ? tid - CLR_MAXH : tid;
    const bool active = seg_role ? (a.swept && h < H - 1) : h < H;
    float pa[D], ab[D];
    float l2 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) { pa[c] = active ? pos[c][h] : 0.f; ab[c] = (active && seg_role) ? sub(pos[c][h + 1], pa[c]) : 0.f; }
    if (seg_role) l2 = norm2<D>(ab);
    bool hit = false;
    int k0, k1;
    clr_span(a.box_off, sc, a.n_boxes, &k0, &k1);
    for (int kc = k0; kc < k1; kc += CLR_PRIMS) {
      const int n = min(CLR_PRIMS, k1 - kc);
      __syncthreads();
      for (int i = tid; i < n * D; i += 256) {
        const int k = i / D, c = i - k * D;
        const float cen = a.box_c[(long)kc * D + i], hf = __fdiv_rn(a.box_s[(long)kc * D + i], 2.f);
        plo[k][c] = sub(sub(cen, hf), a.margin);
        phi[k][c] = add(add(cen, hf), a.margin);
      }
      __syncthreads();
      if (!active) continue;
      for (int k = 0; k < n; ++k) {
        if (!seg_role) {
          bool in = true;
#pragma unroll
          for (int c = 0; c < D; ++c) in &= (pa[c] >= plo[k][c]) && (pa[c] <= phi[k][c]);
          hit |= in;
        } else {
          // slab clipping of t in [0, 1]; an axis the segment does not move along passes iff its start lies in the slab
          float t0 = 0.f, t1 = 1.f;
          bool ok = true;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            const float lo = plo[k][c], hi = phi[k][c];
            if (ab[c] == 0.f) {
              ok &= (pa[c] >= lo) && (pa[c] <= hi);
            } else {
              const float u = __fdiv_rn(sub(lo, pa[c]), ab[c]), v = __fdiv_rn(sub(hi, pa[c]), ab[c]);
              t0 = fmaxf(t0, fminf(u, v));
              t1 = fminf(t1, fmaxf(u, v));
            }
          }
          hit |= ok && (t0 <= t1);
        }
      }
    }
    clr_span(a.sph_off, sc, a.n_spheres, &k0, &k1);
    for (int kc = k0; kc < k1; kc += CLR_PRIMS) {
      const int n = min(CLR_PRIMS, k1 - kc);
      __syncthreads();
      for (int i = tid; i < n * D; i += 256) { const int k = i / D; plo[k][i - k * D] = a.sph_c[(long)kc * D + i]; }
      for (int k = tid; k < n; k += 256) phi[k][0] = add(a.sph_r[kc + k], a.margin);
      __syncthreads();
      if (!active) continue;
      for (int k = 0; k < n; ++k) {
        float w[D];
#pragma unroll
        for (int c = 0; c < D; ++c) w[c] = sub(plo[k][c], pa[c]);
        if (seg_role) {
          // the segment's point nearest to the centre: t = clamp(w . ab / |ab|^2, 0, 1), 0 for a zero-length segment
          const float t = l2 > 0.f ? fminf(fmaxf(__fdiv_rn(dot<D>(w, ab), l2), 0.f), 1.f) : 0.f;
#pragma unroll
          for (int c = 0; c < D; ++c) w[c] = sub(w[c], mul(t, ab[c]));
        }
        hit |= sqrtf(norm2<D>(w)) <= phi[k][0];
      }
    }
    if (active) { if (seg_role) sgf[h] = hit; else wpf[h] = hit; }

    // ---- cloud: wave w owns waypoints / segments w, w + 4, ...; lanes split the tile's points
    clr_span(a.cloud_off, sc, a.n_points, &k0, &k1);
    const float* __restrict__ cloud = a.cloud + (long)k0 * D;
    const int P = k1 - k0;
    for (int p0 = 0; p0 < P; p0 += CLR_TILE) {
      const int np = min(CLR_TILE, P - p0);
      __syncthreads();
      for (int i = tid; i < np * D; i += 256) { const int e = i / D; cl[i - e * D][e] = cloud[(long)p0 * D + i]; }
      __syncthreads();
      for (int hh = wave; hh < H; hh += 4) {
        const bool sg = a.swept && hh + 1 < H;               // (uniform over the wave)
        float qa[D], qd[D];
        float inv = 0.f;
#pragma unroll
        for (int c = 0; c < D; ++c) { qa[c] = pos[c][hh]; qd[c] = sg ? sub(pos[c][hh + 1], qa[c]) : 0.f; }
        if (sg) { const float q2 = norm2<D>(qd); inv = q2 > 0.f ? __fdiv_rn(1.f, q2) : 0.f; }
        for (int e = lane; e < np; e += 64) {
          float w[D];
#pragma unroll
          for (int c = 0; c < D; ++c) w[c] = sub(cl[c][e], qa[c]);
          mw = fminf(mw, norm2<D>(w));
          if (sg) {
            const float t = fminf(fmaxf(mul(dot<D>(w, qd), inv), 0.f), 1.f);     // (fmaxf drops a NaN from 0 * inf: t = 0)
#pragma unroll
            for (int c = 0; c < D; ++c) w[c] = sub(w[c], mul(t, qd[c]));
            ms = fminf(ms, norm2<D>(w));
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- counts: a segment's flag with both endpoints' flags OR-ed in
  int flag = 0;
  if (!is_bad) {
    if (tid < CLR_MAXH) flag = tid < H ? wpf[tid] : 0;
    else { const int h = tid - CLR_MAXH; flag = (a.swept && h < H - 1) ? (sgf[h] | wpf[h] | wpf[h + 1]) : 0; }
  }
  const int n_set = __popcll(__ballot(flag));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { mw = fminf(mw, __shfl_xor(mw, m)); ms = fminf(ms, __shfl_xor(ms, m)); }
  if (lane == 0) { cnt[wave] = n_set; rmin[0][wave] = mw; rmin[1][wave] = ms; }
  __syncthreads();
  if (tid != 0) return;
  float pl = 0.f, sm = 0.f;
  for (int h = 0; h < H - 1; ++h) { pl = add(pl, segl[h]); sm = add(sm, segs[h]); }
  if (a.plen) a.plen[b] = pl;
  if (a.smooth) a.smooth[b] = sm;
  const float nan = __int_as_float(0x7fc00000);
  const float w2 = fminf(fminf(rmin[0][0], rmin[0][1]), fminf(rmin[0][2], rmin[0][3]));
  const float s2 = fminf(fminf(fminf(rmin[1][0], rmin[1][1]), fminf(rmin[1][2], rmin[1][3])), w2);     // min-ed with every endpoint's distance
  if (a.wp_hits) a.wp_hits[b] = is_bad ? H : cnt[0] + cnt[1];
  if (a.clear_wp) a.clear_wp[b] = is_bad ? nan : sqrtf(w2);
  if (a.swept) {
    if (a.seg_hits) a.seg_hits[b] = is_bad ? H - 1 : cnt[2] + cnt[3];
    if (a.clear_seg) a.clear_seg[b] = is_bad ? nan : sqrtf(s2);
  }
}

int launch_traj_clearance(const ClearanceArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.B > 0 && a.H >= 2 && a.H <= CLR_MAXH && (a.D == 2 || a.D == 3) && a.D <= a.S && a.n_scenes > 0, "bad clearance dims");
  if (a.D == 3) hipLaunchKernelGGL(traj_clearance_kernel<3>, dim3(a.B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(traj_clearance_kernel<2>, dim3(a.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
