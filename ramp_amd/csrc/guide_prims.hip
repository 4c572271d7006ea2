// Swept box and sphere terms of the cost guide (ramp_prim_guide in include/ramp_hip.h): guide.hip's clipped gradient steps on
//
//   C = w_obs C_obs + w_prim C_prim + w_smooth C_smooth + w_acc C_acc,   C_prim = sum_u sum_k 1/2 max(0, band - phi_k(u))^2
//
// over the samples u_{h,m} = p_h + (m / n_sub) (p_{h+1} - p_h) of one trajectory's path and the signed distances phi_k to the boxes and spheres
// of its scene, widened by the margin -- what ramp_traj_clearance counts afterwards.  The gradient at a sample goes back to the two waypoints
// of its segment with the weights (1 - t, t).  This is no mirror of reference code; the definition is the header's.
//
// The structure is guide_step_kernel's: one 256-thread block per trajectory for all iterations of the launch, positions, pins and stencils in
// LDS, the cloud term's tile loop as it is there (repeated here, as guide_replan.hip repeats it).  For the new term thread tid owns the samples
// tid, tid + 256, ... (at most 4: (H - 1) n_sub + 1 <= 1017) and keeps their gradients in registers while the scene's primitives pass
// through LDS in chunks of GP_PRIMS, boxes first, then spheres, in table order -- every lane reads the same primitive (a broadcast, no bank
// conflict).  The gradients go to LDS as D planes (lane l writes word l), and after a barrier thread h gathers its <= 2 n_sub - 1
// contributions in the header's order (reads at stride n_sub: up to n_sub-way conflicts on 2 n_sub - 1 reads per plane of one or two waves,
// against n_sub * primitives * D arithmetic per sample).  No atomics, nothing handed between blocks, no dependence on timing.
// LDS at D = 3: 12 KiB cloud tile + 12 KiB sample gradients + 4.5 KiB positions and stencils + 1.5 KiB primitives + pins = 31.3 KiB.
//
// Without a primitive in the block's scene, or with w_prim == 0, the block runs guide_step_kernel<D>'s arithmetic, bit for bit (the cloud loop
// keeps that kernel's __fsqrt_rn; the new term takes sqrtf, which is correctly rounded here, as clearance.hip does).
// Built with -ffp-contract=off like guide.hip: every product and sum below is rounded once, as written.
#include "args_sampler.h"

namespace ramp {

namespace {

constexpr int GP_TILE = 1024;
constexpr int GP_MAXH = 128;
constexpr int GP_PRIMS = 64;
constexpr int GP_MAXSUB = 8;
constexpr int GP_SAMPLES = 1024;      // >= (GP_MAXH - 1) * GP_MAXSUB + 1 = 1017, 4 per thread
constexpr int GP_SLOTS = GP_SAMPLES / 256;

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

// the block's scene sc and the span [first, first + P) of its cloud, clamped to the table's total.  false: a scene index outside the table
// (uniform over the block) -- the trajectory is left as it is
__device__ __forceinline__ bool gp_scene(const GuideArgs& a, int b, int* sc_out, const float** cloud, int* P) {
  const int sc = a.scene ? a.scene[b] : 0;
  if (sc < 0 || sc >= a.n_scenes) return false;
  const int first = min(max(a.cloud_off[sc], 0), a.P_total), end = min(max(a.cloud_off[sc + 1], first), a.P_total);
  *sc_out = sc; *cloud = a.cloud + (size_t)first * a.D; *P = end - first;
  return true;
}
// the scene's span [*k0, *k1) of a concatenated table of `total` entries, clamped to it: a wrong table reads wrong entries, never outside
__device__ __forceinline__ void gp_span(const int* __restrict__ off, int sc, int total, int* k0, int* k1) {
  *k0 = (off && total > 0) ? min(max(off[sc], 0), total) : 0;
  *k1 = (off && total > 0) ? min(max(off[sc + 1], *k0), total) : 0;
}

// np points from `cloud` (np, D) into the planes cl[c][e]: consecutive threads read consecutive words
template <int D>
__device__ __forceinline__ void gp_load_tile(float (*cl)[GP_TILE], const float* __restrict__ cloud, int np, int tid) {
  for (int i = tid; i < np * D; i += 256) { const int e = i / D; cl[i - e * D][e] = cloud[i]; }
}

// n boxes from chunk kc of the table into pc (centres) and ph (half sides widened by the margin)
template <int D>
__device__ __forceinline__ void gp_load_boxes(float (*pc)[D], float (*ph)[D], const PrimGuideArgs& a, int kc, int n, int tid) {
  for (int i = tid; i < n * D; i += 256) {
    const int k = i / D, c = i - k * D;
    pc[k][c] = a.box_c[(size_t)kc * D + i];
    ph[k][c] = add(__fdiv_rn(a.box_s[(size_t)kc * D + i], 2.f), a.margin);
  }
}
// n spheres: centres into pc, r + margin into ph[k][0]
template <int D>
__device__ __forceinline__ void gp_load_spheres(float (*pc)[D], float (*ph)[D], const PrimGuideArgs& a, int kc, int n, int tid) {
  for (int i = tid; i < n * D; i += 256) { const int k = i / D; pc[k][i - k * D] = a.sph_c[(size_t)kc * D + i]; }
  for (int k = tid; k < n; k += 256) ph[k][0] = add(a.sph_r[kc + k], a.margin);
}

// sample i = h n + m of the path in pos: u = p_h for m == 0 (the waypoint's own bits), p_h + t_m (p_{h+1} - p_h) otherwise
template <int D>
__device__ __forceinline__ void gp_sample(const float (*pos)[D], int i, int n, float (&u)[D]) {
  const int h = i / n, m = i - h * n;
  if (m == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) u[c] = pos[h][c];
  } else {
    const float t = __fdiv_rn((float)m, (float)n);
#pragma unroll
    for (int c = 0; c < D; ++c) u[c] = add(pos[h][c], mul(t, sub(pos[h + 1][c], pos[h][c])));
  }
}

// One box (centre pc, widened half sides ph) at the sample u: phi and, with GRAD, g -= (band - phi) grad phi where phi < band.
// Returns band - phi, or a negative number where the pair contributes nothing
template <int D, bool GRAD>
__device__ __forceinline__ float gp_box(const float (&u)[D], const float* pc, const float* ph, float band, float (&g)[D]) {
  float e[D], q[D];
  bool out = false;
#pragma unroll
  for (int c = 0; c < D; ++c) { e[c] = sub(u[c], pc[c]); q[c] = sub(fabsf(e[c]), ph[c]); out |= q[c] > 0.f; }
  if (out) {
    float mx[D];
#pragma unroll
    for (int c = 0; c < D; ++c) mx[c] = fmaxf(q[c], 0.f);
    float s2 = mul(mx[0], mx[0]);
#pragma unroll
    for (int c = 1; c < D; ++c) s2 = add(s2, mul(mx[c], mx[c]));
    const float phi = sqrtf(s2);
    if (!(phi < band)) return -1.f;
    const float w = sub(band, phi);
    if (GRAD) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const float nc = __fdiv_rn(e[c] < 0.f ? -mx[c] : mx[c], phi);
        g[c] = sub(g[c], mul(w, nc));
      }
    }
    return w;
  }
  // inside: the face that is nearest, the lowest axis on a tie; sign(0) = +1
  float phi = q[0];
#pragma unroll
  for (int c = 1; c < D; ++c) phi = fmaxf(phi, q[c]);
  if (!(phi < band)) return -1.f;
  const float w = sub(band, phi);
  if (GRAD) {
    bool taken = false;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const bool mine = !taken && q[c] == phi;
      if (mine) g[c] = sub(g[c], e[c] < 0.f ? -w : w);
      taken |= mine;
    }
  }
  return w;
}

// One sphere (centre pc, widened radius R); a sample at the centre contributes cost and no gradient
template <int D, bool GRAD>
__device__ __forceinline__ float gp_sphere(const float (&u)[D], const float* pc, float R, float band, float (&g)[D]) {
  float e[D];
#pragma unroll
  for (int c = 0; c < D; ++c) e[c] = sub(u[c], pc[c]);
  float d2 = mul(e[0], e[0]);
#pragma unroll
  for (int c = 1; c < D; ++c) d2 = add(d2, mul(e[c], e[c]));
  const float d = sqrtf(d2), phi = sub(d, R);
  if (!(phi < band)) return -1.f;
  const float w = sub(band, phi);
  if (GRAD && d > 0.f) {
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = sub(g[c], mul(w, __fdiv_rn(e[c], d)));
  }
  return w;
}

}  // namespace

template <int D>
__global__ __launch_bounds__(256) void guide_prims_step_kernel(PrimGuideArgs pa) {
  __shared__ float cl[D][GP_TILE];
  __shared__ float gu[D][GP_SAMPLES];     // d C_prim / d u of every sample
  __shared__ float pos[GP_MAXH][D];       // the working copy: pinned waypoints hold their conditioned values
  __shared__ float gob[GP_MAXH][D];       // d C_obs / d p_h
  __shared__ float acc[GP_MAXH][D];       // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ float pc[GP_PRIMS][D], ph[GP_PRIMS][D];
  __shared__ int pin[GP_MAXH];            // 1 + the last hard condition that names waypoint h, 0 = free
  __shared__ double red[4];
  const GuideArgs& a = pa.g;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S, n = pa.n_sub;
  const float* cloud; int P, sc;
  if (!gp_scene(a, b, &sc, &cloud, &P)) return;
  int b0, b1, s0, s1;
  gp_span(pa.box_off, sc, pa.n_boxes, &b0, &b1);
  gp_span(pa.sph_off, sc, pa.n_spheres, &s0, &s1);
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
  const bool prim = pa.w_prim != 0.f && (b1 > b0 || s1 > s0);      // (uniform over the block)
  const int NS = (H - 1) * n + 1;
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);      // cheap filter in front of the square root; `d < r` decides
  const float band = pa.band;
  for (int it = 0; it < a.n_iter; ++it) {
    if (obs) {
      if (tid < H) {
#pragma unroll
        for (int c = 0; c < D; ++c) gob[tid][c] = 0.f;
      }
      for (int p0 = 0; p0 < P; p0 += GP_TILE) {
        const int np = min(GP_TILE, P - p0);
        __syncthreads();
        if (it == 0 || P > GP_TILE) gp_load_tile<D>(cl, cloud + (size_t)p0 * D, np, tid);
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
    float gp[D];                                      // d C_prim / d p_h of thread h
#pragma unroll
    for (int c = 0; c < D; ++c) gp[c] = 0.f;
    if (prim) {
      __syncthreads();                                // the positions of this iteration are in place
      float u[GP_SLOTS][D], g[GP_SLOTS][D];
#pragma unroll
      for (int j = 0; j < GP_SLOTS; ++j) {
        const int i = tid + 256 * j;
#pragma unroll
        for (int c = 0; c < D; ++c) { u[j][c] = 0.f; g[j][c] = 0.f; }
        if (i < NS) gp_sample<D>(pos, i, n, u[j]);
      }
      for (int kc = b0; kc < b1; kc += GP_PRIMS) {
        const int nk = min(GP_PRIMS, b1 - kc);
        __syncthreads();
        gp_load_boxes<D>(pc, ph, pa, kc, nk, tid);
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
#pragma unroll
          for (int j = 0; j < GP_SLOTS; ++j)
            if (tid + 256 * j < NS) gp_box<D, true>(u[j], pc[k], ph[k], band, g[j]);
        }
      }
      for (int kc = s0; kc < s1; kc += GP_PRIMS) {
        const int nk = min(GP_PRIMS, s1 - kc);
        __syncthreads();
        gp_load_spheres<D>(pc, ph, pa, kc, nk, tid);
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
#pragma unroll
          for (int j = 0; j < GP_SLOTS; ++j)
            if (tid + 256 * j < NS) gp_sphere<D, true>(u[j], pc[k], ph[k][0], band, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < GP_SLOTS; ++j) {
        const int i = tid + 256 * j;
        if (i < NS) {
#pragma unroll
          for (int c = 0; c < D; ++c) gu[c][i] = g[j][c];
        }
      }
      __syncthreads();
      if (tid < H) {
        const int h = tid;
        // the hand-back: this segment's samples with 1 - t_m, then the previous segment's with t_m
#pragma unroll
        for (int c = 0; c < D; ++c) gp[c] = gu[c][h * n];            // m = 0: (1 - 0) g
        if (h + 1 < H) {
          for (int m = 1; m < n; ++m) {
            const float wt = sub(1.f, __fdiv_rn((float)m, (float)n));
#pragma unroll
            for (int c = 0; c < D; ++c) gp[c] = add(gp[c], mul(wt, gu[c][h * n + m]));
          }
        }
        if (h >= 1) {
          for (int m = 1; m < n; ++m) {
            const float t = __fdiv_rn((float)m, (float)n);
#pragma unroll
            for (int c = 0; c < D; ++c) gp[c] = add(gp[c], mul(t, gu[c][(h - 1) * n + m]));
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
    float gg[D];
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
        if (prim) v = add(mul(pa.w_prim, gp[c]), v);
        if (obs) v = add(mul(a.w_obs, gob[h][c]), v);
        gg[c] = pin[h] ? 0.f : v;
        n2 += (double)gg[c] * (double)gg[c];
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n2 += __shfl_xor(n2, m);
    if (lane == 0) red[wave] = n2;
    __syncthreads();
    const float nrm = (float)sqrt(((red[0] + red[1]) + red[2]) + red[3]);
    float s = 1.f;
    if (a.max_norm > 0.f && nrm > 0.f) s = fminf(1.f, __fdiv_rn(a.max_norm, nrm));
    const float ss = mul(a.step, s);
    if (tid < H && !pin[tid]) {
#pragma unroll
      for (int c = 0; c < D; ++c) pos[tid][c] = sub(pos[tid][c], mul(ss, gg[c]));
    }
  }
  // (every thread writes back only what it updated last: no barrier needed)
  if (a.n_iter > 0 && tid < H && !pin[tid]) {
#pragma unroll
    for (int c = 0; c < D; ++c) tr[(size_t)tid * S + c] = pos[tid][c];
  }
}

// the four unweighted terms of one trajectory as it is: columns 0 .. 2 are guide_cost_kernel's (the same pair values in the same order),
// column 3 = C_prim: fp32 values 1/2 (band - phi)^2, fp64 sums (a thread's own samples and primitives in order, then lanes, then waves)
template <int D>
__global__ __launch_bounds__(256) void guide_prims_cost_kernel(PrimGuideArgs pa, double* __restrict__ terms) {
  __shared__ float cl[D][GP_TILE];
  __shared__ float pos[GP_MAXH][D];
  __shared__ float pc[GP_PRIMS][D], ph[GP_PRIMS][D];
  __shared__ double red[4][4];
  const GuideArgs& a = pa.g;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, S = a.S, n = pa.n_sub;
  const float* cloud; int P, sc;
  if (!gp_scene(a, b, &sc, &cloud, &P)) {
    if (tid < 4) terms[(size_t)b * 4 + tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  int b0, b1, s0, s1;
  gp_span(pa.box_off, sc, pa.n_boxes, &b0, &b1);
  gp_span(pa.sph_off, sc, pa.n_spheres, &s0, &s1);
  const float* tr = a.traj + (size_t)b * H * S;
  if (tid < H) {
#pragma unroll
    for (int c = 0; c < D; ++c) pos[tid][c] = tr[(size_t)tid * S + c];
  }
  const float r = a.radius, r2hi = mul(mul(r, r), 1.00001f);
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < P; p0 += GP_TILE) {
    const int np = min(GP_TILE, P - p0);
    __syncthreads();
    gp_load_tile<D>(cl, cloud + (size_t)p0 * D, np, tid);
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
  const int NS = (H - 1) * n + 1;
  const float band = pa.band;
  float u[GP_SLOTS][D], unused[D];
#pragma unroll
  for (int j = 0; j < GP_SLOTS; ++j) {
    const int i = tid + 256 * j;
#pragma unroll
    for (int c = 0; c < D; ++c) u[j][c] = 0.f;
    if (i < NS) gp_sample<D>(pos, i, n, u[j]);
  }
  for (int kc = b0; kc < b1; kc += GP_PRIMS) {
    const int nk = min(GP_PRIMS, b1 - kc);
    __syncthreads();
    gp_load_boxes<D>(pc, ph, pa, kc, nk, tid);
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
#pragma unroll
      for (int j = 0; j < GP_SLOTS; ++j) {
        if (tid + 256 * j >= NS) continue;
        const float w = gp_box<D, false>(u[j], pc[k], ph[k], band, unused);
        if (w >= 0.f) t[3] += (double)mul(0.5f, mul(w, w));
      }
    }
  }
  for (int kc = s0; kc < s1; kc += GP_PRIMS) {
    const int nk = min(GP_PRIMS, s1 - kc);
    __syncthreads();
    gp_load_spheres<D>(pc, ph, pa, kc, nk, tid);
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
#pragma unroll
      for (int j = 0; j < GP_SLOTS; ++j) {
        if (tid + 256 * j >= NS) continue;
        const float w = gp_sphere<D, false>(u[j], pc[k], ph[k][0], band, unused);
        if (w >= 0.f) t[3] += (double)mul(0.5f, mul(w, w));
      }
    }
  }
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
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t[k] += __shfl_xor(t[k], m);
    if (lane == 0) red[k][wave] = t[k];
  }
  __syncthreads();
  if (tid < 4) terms[(size_t)b * 4 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

static int check_prim_args(const PrimGuideArgs& p) {
  const GuideArgs& a = p.g;
  RAMP_REQUIRE(a.traj && a.B > 0 && a.H > 0 && a.H <= GP_MAXH, "bad primitive-guide dims (H up to 128)");
  RAMP_REQUIRE((a.D == 2 || a.D == 3) && a.D <= a.S, "primitive guide: point_dim must be 2 or 3 and at most the state width");
  RAMP_REQUIRE(a.n_scenes >= 1 && a.cloud_off && a.P_total >= 0 && (a.P_total == 0 || a.cloud), "bad guide cloud table");
  RAMP_REQUIRE(a.hc.n == 0 || (a.hc.idx && a.hc.val), "primitive guide: missing hard conditions");
  RAMP_REQUIRE(p.n_sub >= 1 && p.n_sub <= GP_MAXSUB, "primitive guide: n_sub outside 1 .. 8");
  RAMP_REQUIRE(p.n_boxes >= 0 && (p.n_boxes == 0 || (p.box_c && p.box_s && p.box_off)), "primitive guide: bad box table");
  RAMP_REQUIRE(p.n_spheres >= 0 && (p.n_spheres == 0 || (p.sph_c && p.sph_r && p.sph_off)), "primitive guide: bad sphere table");
  RAMP_REQUIRE(p.margin >= 0.f && p.band >= 0.f, "primitive guide: negative margin or band");
  return 0;
}

int launch_guide_prims_step(const PrimGuideArgs& a, hipStream_t s) {
  if (int rc = check_prim_args(a)) return rc;
  RAMP_REQUIRE(a.g.n_iter >= 0, "primitive guide: negative iteration count");
  if (a.g.n_iter == 0) return 0;
  if (a.g.D == 2) hipLaunchKernelGGL(guide_prims_step_kernel<2>, dim3(a.g.B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(guide_prims_step_kernel<3>, dim3(a.g.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_guide_prims_cost(const PrimGuideArgs& a, double* terms, hipStream_t s) {
  if (int rc = check_prim_args(a)) return rc;
  RAMP_REQUIRE(terms, "primitive guide: null output");
  if (a.g.D == 2) hipLaunchKernelGGL(guide_prims_cost_kernel<2>, dim3(a.g.B), dim3(256), 0, s, a, terms);
  else hipLaunchKernelGGL(guide_prims_cost_kernel<3>, dim3(a.g.B), dim3(256), 0, s, a, terms);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
