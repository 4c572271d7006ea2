// Swept box and sphere terms of the cost guide (ramp_prim_guide in include/ramp_hip.h): guide.hip's clipped gradient steps on
//
//   C = w_obs C_obs + w_prim C_prim + w_smooth C_smooth + w_acc C_acc,   C_prim = sum_u sum_k 1/2 max(0, band - phi_k(u))^2
//
// over the samples u_{h,m} = p_h + (m / n_sub) (p_{h+1} - p_h) of one trajectory's path and the signed distances phi_k to the boxes and spheres
// of its scene, widened by the margin -- what ramp_traj_clearance counts afterwards.  The gradient at a sample goes back to the two waypoints
// of its segment with the weights (1 - t, t).  This is no mirror of reference code; the definition is the header's.
//
// The structure is guide_step_kernel's: one 256-thread block per trajectory for all iterations of the launch, positions, pins and stencils in
// LDS, the cloud term, the stencils and the update from guide_core.h as they are there.  For the new term thread tid owns the samples
// tid, tid + 256, ... (at most 4: (H - 1) n_sub + 1 <= 1017) and keeps their gradients in registers while the scene's primitives pass
// through LDS in chunks of GP_PRIMS, boxes first, then spheres, in table order -- every lane reads the same primitive (a broadcast, no bank
// conflict).  The gradients go to LDS as D planes (lane l writes word l), and after a barrier thread h gathers its <= 2 n_sub - 1
// contributions in the header's order (reads at stride n_sub: up to n_sub-way conflicts on 2 n_sub - 1 reads per plane of one or two waves,
// against n_sub * primitives * D arithmetic per sample).  No atomics, nothing handed between blocks, no dependence on timing.
// LDS at D = 3: 12 KiB cloud tile + 12 KiB sample gradients + 4.5 KiB positions and stencils + 1.5 KiB primitives + pins = 31.3 KiB.
//
// Without a primitive in the block's scene, or with w_prim == 0, the block runs guide_step_kernel<D>'s arithmetic, bit for bit: the same
// guide_core.h calls with no extra term (the cloud term keeps its own square root there; the new term takes sqrtf, which is correctly rounded
// here, as clearance.hip does).
// Built with -ffp-contract=off like guide.hip: every product and sum below is rounded once, as written.
#include "guide_core.h"

namespace ramp {

namespace {

constexpr int GP_PRIMS = 64;
constexpr int GP_MAXSUB = 8;
constexpr int GP_SAMPLES = 1024;      // >= (GUIDE_MAX_H - 1) * GP_MAXSUB + 1 = 1017, 4 per thread
constexpr int GP_SLOTS = GP_SAMPLES / 256;

// the scene's span [*k0, *k1) of a concatenated table of `total` entries, clamped to it: a wrong table reads wrong entries, never outside
__device__ __forceinline__ void gp_span(const int* __restrict__ off, int sc, int total, int* k0, int* k1) {
  *k0 = (off && total > 0) ? min(max(off[sc], 0), total) : 0;
  *k1 = (off && total > 0) ? min(max(off[sc + 1], *k0), total) : 0;
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
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float gu[D][GP_SAMPLES];     // d C_prim / d u of every sample
  __shared__ float pos[GUIDE_MAX_H][D];   // the working copy: pinned waypoints hold their conditioned values
  __shared__ float gob[GUIDE_MAX_H][D];   // d C_obs / d p_h
  __shared__ float acc[GUIDE_MAX_H][D];   // p_{h+1} - 2 p_h + p_{h-1}, zero at both ends
  __shared__ float pc[GP_PRIMS][D], ph[GP_PRIMS][D];
  __shared__ int pin[GUIDE_MAX_H];        // 1 + the last hard condition that names waypoint h, 0 = free
  __shared__ double red[4];
  const GuideArgs& a = pa.g;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, n = pa.n_sub;
  GuideSpan sp;
  if (!guide_scene(a, a.D, b, &sp)) return;
  int b0, b1, s0, s1;
  gp_span(pa.box_off, sp.sc, pa.n_boxes, &b0, &b1);
  gp_span(pa.sph_off, sp.sc, pa.n_spheres, &s0, &s1);
  float* tr = a.traj + (size_t)b * H * a.S;
  guide_pin_hard<D>(a, b, tr, pos, pin, tid);
  const bool obs = a.w_obs != 0.f && sp.P > 0;
  const bool prim = pa.w_prim != 0.f && (b1 > b0 || s1 > s0);      // (uniform over the block)
  const int NS = (H - 1) * n + 1;
  const float r = a.radius, r2hi = guide_r2hi(r);
  const float band = pa.band;
  const GuideWeights w = {a.w_obs, a.w_smooth, a.w_acc, a.max_norm, a.step};
  for (int it = 0; it < a.n_iter; ++it) {
    if (obs) guide_cloud_force<D>(cl, pos, gob, pin, sp.cloud, sp.P, H, it, r, r2hi, tid);
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
    guide_second_difference<D>(pos, acc, H, tid);
    guide_update<D>(pos, acc, gob, pin, red, H, w, obs, prim, pa.w_prim, gp, tid);
  }
  if (a.n_iter > 0) guide_write_back<D>(tr, H, a.S, pos, pin, tid);
}

// the four unweighted terms of one trajectory as it is: columns 0 .. 2 are guide_cost_kernel's (the same pair values in the same order),
// column 3 = C_prim: fp32 values 1/2 (band - phi)^2, fp64 sums (a thread's own samples and primitives in order, then lanes, then waves)
template <int D>
__global__ __launch_bounds__(256) void guide_prims_cost_kernel(PrimGuideArgs pa, double* __restrict__ terms) {
  __shared__ float cl[D][GUIDE_TILE];
  __shared__ float pos[GUIDE_MAX_H][D];
  __shared__ float pc[GP_PRIMS][D], ph[GP_PRIMS][D];
  __shared__ double red[4][4];
  const GuideArgs& a = pa.g;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int H = a.H, n = pa.n_sub;
  GuideSpan sp;
  if (!guide_scene(a, a.D, b, &sp)) { guide_store_nan<4>(terms + (size_t)b * 4, tid); return; }
  int b0, b1, s0, s1;
  gp_span(pa.box_off, sp.sc, pa.n_boxes, &b0, &b1);
  gp_span(pa.sph_off, sp.sc, pa.n_spheres, &s0, &s1);
  guide_load_pos<D>(a.traj + (size_t)b * H * a.S, H, a.S, pos, tid);
  double t[4] = {0.0, 0.0, 0.0, 0.0};      // {C_obs, C_smooth, C_acc, C_prim}
  guide_cloud_cost<D>(cl, pos, sp.cloud, sp.P, H, a.radius, guide_r2hi(a.radius), tid, &t[0]);
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
  guide_stencil_costs<D>(pos, H, tid, &t[1], &t[2]);
  guide_store_terms<4>(t, red, terms + (size_t)b * 4, tid);
}

static int check_prim_args(const PrimGuideArgs& p) {
  if (int rc = require_guide_args(p.g, "bad primitive-guide dims (H up to 128)",
                                  "primitive guide: point_dim must be 2 or 3 and at most the state width",
                                  "primitive guide: missing hard conditions")) return rc;
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
