// Sampler arithmetic around the score network: classifier-free-guidance combine, x0 prediction,
// posterior mean, DDPM / DDIM update, hard conditioning, artificial potential field, costs.
//
//   p_mean_variance (CFG, x0, clamp, posterior)   diffusion_model_static.py:149-186, 188-229; diffusion_model_3d.py:147-182
//   ddpm_sample_fn                                 sample_functions.py:19-48
//   ddim_p_sample                                  diffusion_model_static.py:259-333
//   apply_hard_conditioning                        sample_functions.py:5-10
//   avoidance (static APF)                         APFhelper.py:37-104
//   collision mask / path length / smoothness      cost.py:3-54
//
// These kernels are HBM-bound elementwise work; every product/sum is written with explicit
// round-to-nearest intrinsics in the reference's own evaluation order so that no FMA contraction
// changes a rounding (the x0 clamp makes borderline elements sensitive to single ulps).
#include "args_sampler.h"

#include <algorithm>

namespace ramp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float sub(float a, float b) { return __fsub_rn(a, b); }

__global__ __launch_bounds__(256) void cfg_mean_kernel(CfgMeanArgs a) {
  const long n = (long)a.B * a.HS;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const long b = idx / a.HS; const int e = (int)(idx - b * a.HS);
    const float* ep = a.eps + (b * a.n_rp) * a.HS + e;
    float ec;
    if (a.n_rp == 2) {
      // e_comb = (1 + w) * cond - w * uncond          (diffusion_model_static.py:164-165)
      ec = sub(mul(a.w0p1, ep[0]), mul(a.w0, ep[a.HS]));
    } else if (a.n_rp == 3) {
      // e_comb = u + w1 (c1 - u) + w2 (c2 - u)         (diffusion_model_static.py:214)
      const float u = ep[2 * a.HS];
      ec = add(add(u, mul(a.w0, sub(ep[0], u))), mul(a.w1, sub(ep[a.HS], u)));
    } else {
      ec = ep[0];
    }
    const float xv = a.x[idx];
    // predict_start_from_noise (diffusion_model_static.py:109-118): predict_epsilon=False returns the network output itself
    float x0 = a.predict_x0 ? ec : sub(mul(a.sqrt_recip, xv), mul(a.sqrt_recipm1, ec));
    if (a.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    if (a.ecomb) a.ecomb[idx] = ec;
    if (a.x0) a.x0[idx] = x0;
    if (a.mean) a.mean[idx] = add(mul(a.coef1, x0), mul(a.coef2, xv));
  }
}
int launch_cfg_mean(const CfgMeanArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.B > 0 && a.HS > 0 && a.n_rp >= 1 && a.n_rp <= 3, "bad cfg_mean dims");
  const long n = (long)a.B * a.HS;
  long g = (n + 255) / 256; if (g > 8192) g = 8192;
  hipLaunchKernelGGL(cfg_mean_kernel, dim3((int)g), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// Composition over any number of obstacle sets, e = u + sum_k w_k (c_k - u) (diffusion_model_static.py:188-229; diffusion_model_3d.py:163-182,
// the three-set form at :165-174) written as one weight per row, e_comb[b] = sum_j rw[b][j] eps[b n_rp + j]: the unconditional row carries
// 1 - sum_k w_k.  Four elements per thread (HS % 4 == 0 keeps them inside one trajectory); x0, clamp and posterior mean as in cfg_mean_kernel.
__global__ __launch_bounds__(256) void cfg_mean_rows_kernel(CfgMeanArgs a, const float* __restrict__ rw) {
  const int hs4 = a.HS / 4;
  const long n4 = (long)a.B * hs4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long b = i / hs4; const int e4 = (int)(i - b * hs4);
    const f32x4* ep = reinterpret_cast<const f32x4*>(a.eps) + (b * a.n_rp) * hs4 + e4;
    const float* wb = rw + b * a.n_rp;
    const f32x4 e0 = ep[0]; const float w0 = wb[0];
    f32x4 ec = f32x4{mul(w0, e0[0]), mul(w0, e0[1]), mul(w0, e0[2]), mul(w0, e0[3])};
    for (int j = 1; j < a.n_rp; ++j) {
      const f32x4 ej = ep[j * (long)hs4]; const float wj = wb[j];
      ec = f32x4{add(ec[0], mul(wj, ej[0])), add(ec[1], mul(wj, ej[1])), add(ec[2], mul(wj, ej[2])), add(ec[3], mul(wj, ej[3]))};
    }
    const f32x4 xv = reinterpret_cast<const f32x4*>(a.x)[i];
    f32x4 x0, mean;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = a.predict_x0 ? ec[q] : sub(mul(a.sqrt_recip, xv[q]), mul(a.sqrt_recipm1, ec[q]));
      if (a.clip) v = fminf(fmaxf(v, -1.f), 1.f);
      x0[q] = v;
      mean[q] = add(mul(a.coef1, v), mul(a.coef2, xv[q]));
    }
    if (a.ecomb) reinterpret_cast<f32x4*>(a.ecomb)[i] = ec;
    if (a.x0) reinterpret_cast<f32x4*>(a.x0)[i] = x0;
    if (a.mean) reinterpret_cast<f32x4*>(a.mean)[i] = mean;
  }
}
int launch_cfg_mean_rows(const CfgMeanArgs& a, const float* row_weight, hipStream_t s) {
  RAMP_REQUIRE(a.B > 0 && a.HS > 0 && a.HS % 4 == 0 && a.n_rp >= 2 && a.n_rp <= 8 && row_weight, "bad cfg_mean_rows dims");
  const long n4 = (long)a.B * (a.HS / 4);
  long g = (n4 + 255) / 256; if (g > 8192) g = 8192;
  hipLaunchKernelGGL(cfg_mean_rows_kernel, dim3((int)g), dim3(256), 0, s, a, row_weight);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// returns true and the conditioned value when waypoint h of sample b is hard-conditioned
__device__ __forceinline__ bool hard_value(const HardConds& hc, int b, int h, int si, int B, int S, float* out) {
  bool hit = false;
  for (int k = 0; k < hc.n; ++k)            // later entries win, like the reference's dict loop
    if (hc.idx[k] == h) { *out = hc.val[((long)k * B + b) * S + si]; hit = true; }
  return hit;
}

__global__ __launch_bounds__(256) void ddpm_finish_kernel(const float* __restrict__ mean, const float* __restrict__ noise,
                                                           float stdv, float noise_scale,
                                                           int use_noise, HardConds hc, float* __restrict__ x,
                                                           float* __restrict__ chain, int B, int H, int S) {
  const long n = (long)B * H * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int si = (int)(idx % S); const long bh = idx / S; const int h = (int)(bh % H); const int b = (int)(bh / H);
    // x = mean + std * noise * noise_std, noise zeroed at t == 0   (sample_functions.py:34-48)
    const float z = use_noise ? noise[idx] : 0.f;
    float v = add(mean[idx], mul(mul(stdv, z), noise_scale));
    float hv;
    if (hard_value(hc, b, h, si, B, S, &hv)) v = hv;
    x[idx] = v;
    if (chain) chain[idx] = v;
  }
}

__global__ __launch_bounds__(256) void ddim_finish_kernel(const float* __restrict__ x_in, const float* __restrict__ x0,
                                                           float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                                           float dir_coef, HardConds hc, float* __restrict__ x,
                                                           float* __restrict__ chain, int B, int H, int S) {
  const long n = (long)B * H * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int si = (int)(idx % S); const long bh = idx / S; const int h = (int)(bh % H); const int b = (int)(bh / H);
    // model_output = (x - sqrt(a_t) x0) / sqrt(1 - a_t); x = sqrt(a_prev) x0 + sqrt(1 - a_prev) model_output
    // (diffusion_model_static.py:321-333, eta = 0)
    const float p0 = x0[idx];
    const float mo = __fdiv_rn(sub(x_in[idx], mul(sqrt_a_t, p0)), sqrt_1m_a_t);
    float v = add(mul(sqrt_a_prev, p0), mul(dir_coef, mo));
    float hv;
    if (hard_value(hc, b, h, si, B, S, &hv)) v = hv;
    x[idx] = v;
    if (chain) chain[idx] = v;
  }
}

__global__ __launch_bounds__(256) void hard_cond_kernel(float* __restrict__ x, HardConds hc, int B, int H, int S) {
  const long n = (long)hc.n * B * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int si = (int)(idx % S); const long kb = idx / S; const int b = (int)(kb % B); const int k = (int)(kb / B);
    // duplicate indices: the last one wins
    bool later = false;
    for (int k2 = k + 1; k2 < hc.n; ++k2) later |= (hc.idx[k2] == hc.idx[k]);
    if (!later) x[((long)b * H + hc.idx[k]) * S + si] = hc.val[idx];
  }
}

static inline int ew_grid(long n) { long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g)); }

int launch_ddpm_finish(const float* mean, const float* noise, float stdv, float noise_scale, int use_noise,
                        HardConds hc, float* x, float* chain_out, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0, "bad dims");
  RAMP_REQUIRE(!use_noise || noise != nullptr, "noise required");
  hipLaunchKernelGGL(ddpm_finish_kernel, dim3(ew_grid((long)B * H * S)), dim3(256), 0, s, mean, noise, stdv,
                     noise_scale, use_noise, hc, x, chain_out, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_ddim_finish(const float* x_in, const float* x0, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                       float dir_coef, HardConds hc, float* x, float* chain_out, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0, "bad dims");
  hipLaunchKernelGGL(ddim_finish_kernel, dim3(ew_grid((long)B * H * S)), dim3(256), 0, s, x_in, x0, sqrt_a_t,
                     sqrt_1m_a_t, sqrt_a_prev, dir_coef, hc, x, chain_out, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
// q_sample per row + endpoint pinning (the training-side forward process, diffusion_model_static.py:467-486): the reference's
// extract(a, t) * x_start + extract(b, t) * noise, two products and one sum in fp32 (this file is built without FMA contraction)
__global__ __launch_bounds__(256)
void q_sample_rows_kernel(const float* __restrict__ x_start, const float* __restrict__ noise, const float* __restrict__ sqrt_ac,
                          const float* __restrict__ sqrt_1m_ac, const int* __restrict__ t_rows, int T, float* __restrict__ x_noisy,
                          int B, int H, int S, int pin) {
  const long n = (long)B * H * S, HS = (long)H * S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int b = (int)(i / HS), h = (int)((i - (long)b * HS) / S);
    const int t = t_rows[b];
    const float x = x_start[i];
    float v;
    if (pin && (h == 0 || h == H - 1)) v = x;
    else if (t < 0 || t >= T) v = __builtin_nanf("");
    else v = sqrt_ac[t] * x + sqrt_1m_ac[t] * noise[i];
    x_noisy[i] = v;
  }
}
int launch_q_sample_rows(const float* x_start, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int* t_rows, int T,
                         float* x_noisy, int B, int H, int S, int pin, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && T > 0, "bad q_sample dims");
  const long n = (long)B * H * S;
  const int nblk = (int)std::min<long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(q_sample_rows_kernel, dim3(nblk), dim3(256), 0, s, x_start, noise, sqrt_ac, sqrt_1m_ac, t_rows, T, x_noisy, B, H, S, pin);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_hard_cond(float* x, HardConds hc, int B, int H, int S, hipStream_t s) {
  if (hc.n == 0) return 0;
  hipLaunchKernelGGL(hard_cond_kernel, dim3(ew_grid((long)hc.n * B * S)), dim3(256), 0, s, x, hc, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// APF: one 256-thread block per trajectory.  The cloud streams through LDS in tiles of 1024
// points as double2; each wave owns waypoints w, w+4, ...; lanes split the tile's points and the
// (d^2, index) minimum is reduced with wavefront shuffles (lowest index wins ties, like argmin).
// Distances are float64 like the reference's cKDTree query; directions float32; magnitudes
// float64; forces accumulate hit by hit in waypoint order with a float32 rounding after each add,
// exactly as the reference's sequential `force_field[...] +=` does (APFhelper.py:94-101).
// ------------------------------------------------------------------------------------------
constexpr int APF_TILE = 1024;
constexpr int APF_MAXH = 128;

// SC: the trajectory's own cloud (ApfArgs.scene): block b streams only the points of its scene, indexed from that cloud's first
// point, so every comparison, tie and sum is the single-cloud kernel's on that cloud.  A scene index outside the table leaves the
// trajectory as it is.
template <bool SC>
__global__ __launch_bounds__(256) void apf_kernel(ApfArgs a) {
  __shared__ double2 cl[APF_TILE];
  __shared__ double best_d2[APF_MAXH];
  __shared__ int best_i[APF_MAXH];
  __shared__ float fx[APF_MAXH], fy[APF_MAXH];   // per-hit force (mag * dir), zero if no hit
  __shared__ double fmag[APF_MAXH];
  __shared__ float dirx[APF_MAXH], diry[APF_MAXH];
  __shared__ int hitf[APF_MAXH];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* tr = a.traj + (long)b * a.H * a.S;
  if (SC) {
    const int sc = a.scene[b];
    if (sc < 0 || sc >= a.n_scenes) return;                  // (uniform over the block)
    const int first = a.scene_off[sc];
    a.cloud += 2l * first; a.P = a.scene_off[sc + 1] - first;
  }
  for (int h = tid; h < a.H; h += 256) { best_d2[h] = 1.0e300; best_i[h] = -1; }
  for (int p0 = 0; p0 < a.P; p0 += APF_TILE) {
    const int np = min(APF_TILE, a.P - p0);
    __syncthreads();
    for (int e = tid; e < np; e += 256) cl[e] = make_double2((double)a.cloud[(p0 + e) * 2], (double)a.cloud[(p0 + e) * 2 + 1]);
    __syncthreads();
    for (int h = wave; h < a.H; h += 4) {
      const double qx = (double)tr[h * a.S], qy = (double)tr[h * a.S + 1];
      double bd = 1.0e300; int bi = -1;
      for (int e = lane; e < np; e += 64) {
        const double dx = qx - cl[e].x, dy = qy - cl[e].y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; bi = p0 + e; }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        if (od < bd || (od == bd && oi >= 0 && (bi < 0 || oi < bi))) { bd = od; bi = oi; }
      }
      if (lane == 0 && bi >= 0 && (bd < best_d2[h] )) { best_d2[h] = bd; best_i[h] = bi; }
    }
  }
  __syncthreads();
  for (int h = tid; h < a.H; h += 256) {
    const double d = sqrt(best_d2[h]);
    const bool hit = best_i[h] >= 0 && d < a.thr;
    hitf[h] = hit;
    if (hit) {
      const float px = a.cloud[best_i[h] * 2], py = a.cloud[best_i[h] * 2 + 1];
      const float ddx = sub(tr[h * a.S], px), ddy = sub(tr[h * a.S + 1], py);
      const float nrm = sqrtf(add(mul(ddx, ddx), mul(ddy, ddy)));
      const float den = add(nrm, 1e-8f);
      dirx[h] = __fdiv_rn(ddx, den);
      diry[h] = __fdiv_rn(ddy, den);
      fmag[h] = a.strength * exp(-d / a.thr);
    }
  }
  __syncthreads();
  for (int sidx = tid; sidx < a.H; sidx += 256) {
    float Fx = 0.f, Fy = 0.f;
    const int lo = max(0, sidx - a.win), hi = min(a.H - 1, sidx + a.win);
    for (int tau = lo; tau <= hi; ++tau) {
      if (!hitf[tau]) continue;
      const double w = (double)a.window[sidx - tau + a.win];
      Fx = (float)((double)Fx + fmag[tau] * (double)dirx[tau] * w);
      Fy = (float)((double)Fy + fmag[tau] * (double)diry[tau] * w);
    }
    fx[sidx] = Fx; fy[sidx] = Fy;
  }
  __syncthreads();
  for (int h = tid; h < a.H; h += 256) {
    tr[h * a.S] = add(tr[h * a.S], fx[h]);
    tr[h * a.S + 1] = add(tr[h * a.S + 1], fy[h]);
  }
}
int launch_apf(const ApfArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.B > 0 && a.H > 0 && a.H <= APF_MAXH && a.S >= 2 && (a.P > 0 || a.scene) && a.win >= 0, "bad APF dims");
  RAMP_REQUIRE(!a.scene || (a.scene_off && a.n_scenes > 0), "APF with per-trajectory scenes needs the scene offset table");
  if (a.scene) hipLaunchKernelGGL(apf_kernel<true>, dim3(a.B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(apf_kernel<false>, dim3(a.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// Receding-horizon replanning (diffusion_model_dynamic.py:495-624): the elementwise pieces between the score
// evaluations of one replan.  What changes from replan to replan (how many waypoints have been executed, the current
// waypoint, the pursuer's position) lives in a small device record, so the captured graph of one replan never changes.
// ------------------------------------------------------------------------------------------
// x = q_sample(repeat(x_clean), t) = sqrt_ac[t] * x_clean + sqrt_1m_ac[t] * noise (diffusion_model_dynamic.py:671-680),
// then x[:, 0, 2:] = 0, the executed history, and the goal waypoint of the clean plan (:540-546).
// Each of the four steps below is a per-row rule (replan_*_row) and its kernel over a batch of episodes: row b reads the record,
// history and clean plan of episode row_ep[b] (ramp_replan's single episode: every row reads episode 0's).  x_clean, hist: the (H,S)
// blocks of the row's own episode.
__device__ __forceinline__ float replan_init_value(const float* __restrict__ x_clean, const float* __restrict__ hist, float nz,
                                                   float sa, float s1a, int n_hist, int h, int si, int H, int S) {
  float v = add(mul(sa, x_clean[h * S + si]), mul(s1a, nz));
  if (h == 0 && si >= 2) v = 0.f;
  if (h < n_hist) v = hist[h * S + si];
  if (h == H - 1) v = x_clean[h * S + si];
  return v;
}
__global__ __launch_bounds__(256) void replan_init_episodes_kernel(float* __restrict__ x, const float* __restrict__ x_clean,
                                                                    const float* __restrict__ noise, float sa, float s1a,
                                                                    const float* __restrict__ hist, EpisodeTable ep, int B, int H, int S) {
  const long n = (long)B * H * S, HS = (long)H * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int si = (int)(idx % S); const int h = (int)((idx / S) % H);
    const int e = ep.row_ep[idx / HS];
    x[idx] = replan_init_value(x_clean + e * HS, hist + e * HS, noise[idx], sa, s1a, ep.st[e].n_hist, h, si, H, S);
  }
}
// after every DDIM step: apply_hard_conditioning, then the executed history, the goal of the clean plan, x[:, 0, 2:] = 0
// (diffusion_model_dynamic.py:563-568); one thread per (trajectory, state component), the pinned waypoints in order
__device__ __forceinline__ void replan_pin_row(float* __restrict__ xb, const HardConds& hc, const float* __restrict__ hist,
                                               const float* __restrict__ x_clean, int n_hist, int b, int si, int B, int H, int S) {
  for (int k = 0; k < hc.n; ++k) xb[hc.idx[k] * S + si] = hc.val[((long)k * B + b) * S + si];
  for (int h = 0; h < n_hist; ++h) xb[h * S + si] = hist[h * S + si];
  xb[(H - 1) * S + si] = x_clean[(H - 1) * S + si];
  if (si >= 2) xb[si] = 0.f;
}
__global__ __launch_bounds__(256) void replan_pin_episodes_kernel(float* __restrict__ x, HardConds hc, const float* __restrict__ hist,
                                                                   const float* __restrict__ x_clean, EpisodeTable ep, int B, int H, int S) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * S) return;
  const int b = idx / S, si = idx - b * S;
  const int e = ep.row_ep[b];
  const long HS = (long)H * S;
  replan_pin_row(x + b * HS, hc, hist + e * HS, x_clean + e * HS, ep.st[e].n_hist, b, si, B, H, S);
}
// sm(): velocity-limited straight-line states between waypoints stepp and stepp + window, written to
// stepp + 1 .. stepp + window (diffusion_model_dynamic.py:192-214), torch's fp32 evaluation order
__device__ __forceinline__ void replan_sm_row(float* __restrict__ xb, int stepp, int window, float dt, float max_vel, int H, int S) {
  if (stepp + window >= H) return;                        // the reference would index past the horizon here
  const float* s1 = xb + stepp * S; const float* s2 = xb + (stepp + window) * S;
  const float dx = sub(s2[0], s1[0]), dy = sub(s2[1], s1[1]);
  const float dist = sqrtf(add(mul(dx, dx), mul(dy, dy)));
  const float ux = dist > 1e-6f ? __fdiv_rn(dx, dist) : 0.f, uy = dist > 1e-6f ? __fdiv_rn(dy, dist) : 0.f;
  const float span = (float)((double)window * (double)dt);          // python: num_steps * dt, then one fp32 division
  const float vx0 = __fdiv_rn(dx, span), vy0 = __fdiv_rn(dy, span);
  const bool fast = sqrtf(add(mul(vx0, vx0), mul(vy0, vy0))) > max_vel;
  const float vx = fast ? mul(ux, max_vel) : vx0, vy = fast ? mul(uy, max_vel) : vy0;
  for (int j = 1; j <= window; ++j) {
    const float tt = mul((float)j, dt);
    float* o = xb + (stepp + j) * S;
    o[0] = add(s1[0], mul(tt, vx)); o[1] = add(s1[1], mul(tt, vy));
    o[2] = vx; o[3] = vy;
  }
}
__global__ __launch_bounds__(256) void replan_sm_episodes_kernel(float* __restrict__ x, EpisodeTable ep, int window, float dt,
                                                                  float max_vel, int B, int H, int S) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  replan_sm_row(x + (long)b * H * S, ep.st[ep.row_ep[b]].stepp, window, dt, max_vel, H, S);
}
// en[b] = || x[b, stepp, :2] - pursuer || < thr   (diffusion_model_dynamic.py:414-420: which trajectories get the
// pursuer pass); x0[:, -1] = x[:, -1] afterwards is replan_goal_kernel
__device__ __forceinline__ int replan_near_row(const float* __restrict__ q, const float* __restrict__ pursuer, float thr) {
  const float dx = sub(q[0], pursuer[0]), dy = sub(q[1], pursuer[1]);
  return sqrtf(add(mul(dx, dx), mul(dy, dy))) < thr;
}
__global__ __launch_bounds__(256) void replan_near_episodes_kernel(const float* __restrict__ x, EpisodeTable ep, float thr,
                                                                    int* __restrict__ en, int B, int H, int S) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const EpisodeState* st = ep.st + ep.row_ep[b];
  en[b] = replan_near_row(x + ((long)b * H + st->stepp) * S, st->pursuer, thr);
}
__global__ __launch_bounds__(256) void replan_goal_kernel(float* __restrict__ x0, const float* __restrict__ x, int B, int H, int S) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * S) return;
  const int b = idx / S, si = idx - b * S;
  x0[((long)b * H + H - 1) * S + si] = x[((long)b * H + H - 1) * S + si];
}
// The order of a selection, stated once for select_block and the diverse selection below (ramp_select_diverse_scenes in ramp_hip.h).
// select_ranges: the ranges of the min-max normalisation over the free rows of [0, B) and their number, block-wide (1024 threads; every
// thread gets the same record)
struct SelectRanges { float pl_lo, pl_rng, sm_lo, sm_rng; int n_free; };
__device__ __forceinline__ SelectRanges select_ranges(const int* __restrict__ mask, const float* __restrict__ plen,
                                                      const float* __restrict__ smooth, int B) {
  __shared__ float r_min[2][16], r_max[2][16]; __shared__ int r_cnt[16];
  __shared__ float s_lo[2], s_hi[2]; __shared__ int s_free;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float lo0 = INFINITY, hi0 = -INFINITY, lo1 = INFINITY, hi1 = -INFINITY; int cnt = 0;
  for (int b = tid; b < B; b += 1024)
    if (!mask[b]) { lo0 = fminf(lo0, plen[b]); hi0 = fmaxf(hi0, plen[b]); lo1 = fminf(lo1, smooth[b]); hi1 = fmaxf(hi1, smooth[b]); ++cnt; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo0 = fminf(lo0, __shfl_xor(lo0, m)); hi0 = fmaxf(hi0, __shfl_xor(hi0, m));
    lo1 = fminf(lo1, __shfl_xor(lo1, m)); hi1 = fmaxf(hi1, __shfl_xor(hi1, m)); cnt += __shfl_xor(cnt, m);
  }
  if (lane == 0) { r_min[0][wave] = lo0; r_max[0][wave] = hi0; r_min[1][wave] = lo1; r_max[1][wave] = hi1; r_cnt[wave] = cnt; }
  __syncthreads();
  if (tid == 0) {
    float a0 = INFINITY, b0 = -INFINITY, a1 = INFINITY, b1 = -INFINITY; int c = 0;
    for (int w = 0; w < 16; ++w) { a0 = fminf(a0, r_min[0][w]); b0 = fmaxf(b0, r_max[0][w]); a1 = fminf(a1, r_min[1][w]); b1 = fmaxf(b1, r_max[1][w]); c += r_cnt[w]; }
    s_lo[0] = a0; s_hi[0] = b0; s_lo[1] = a1; s_hi[1] = b1; s_free = c;
  }
  __syncthreads();
  return {s_lo[0], sub(s_hi[0], s_lo[0]), s_lo[1], sub(s_hi[1], s_lo[1]), s_free};
}
// total of a free row: w_s sm + w_l pl on the normalised values, one fp32 rounding per operation
__device__ __forceinline__ float select_total(float pl_b, float sm_b, const SelectRanges& r, float w_s, float w_l) {
  const float pl = __fdiv_rn(sub(pl_b, r.pl_lo), r.pl_rng), sm = __fdiv_rn(sub(sm_b, r.sm_lo), r.sm_rng);
  return add(mul(w_s, sm), mul(w_l, pl));
}
// row (ot, oi) comes before row (bt, bi): a NaN total (0 / 0 when every free trajectory ties) ranks first, as in torch.argmin, then the
// smaller total, then the lower row
__device__ __forceinline__ bool select_before(float ot, int oi, float bt, int bi) {
  return (ot != ot) ? (!(bt != bt) || oi < bi) : (!(bt != bt) && (ot < bt || (ot == bt && oi < bi)));
}
constexpr int SELECT_NONE = 0x7fffffff;     // "no row yet" of a running first-in-order
__device__ __forceinline__ void select_take(float ot, int oi, float& bt, int& bi) {
  if (oi == SELECT_NONE) return;
  if (bi == SELECT_NONE || select_before(ot, oi, bt, bi)) { bt = ot; bi = oi; }
}
// the first row in the order among the 1024 threads' running firsts, handed to every thread (SELECT_NONE: no thread has one); one use per kernel
__device__ __forceinline__ int select_first_in_block(float bt, int bi) {
  __shared__ float r_tot[16]; __shared__ int r_idx[16]; __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const float ot = __shfl_xor(bt, m); const int oi = __shfl_xor(bi, m);
    select_take(ot, oi, bt, bi);
  }
  if (lane == 0) { r_tot[wave] = bt; r_idx[wave] = bi; }
  __syncthreads();
  if (tid == 0) {
    float t = INFINITY; int i = SELECT_NONE;
    for (int w = 0; w < 16; ++w) select_take(r_tot[w], r_idx[w], t, i);
    s_best = i;
  }
  __syncthreads();
  return s_best;
}
// compute_trajectory_costs (cost.py:56-88) over the B per-trajectory scalars: min-max normalisation over the
// collision-free ones, total = w_s * smooth + w_l * length, first minimum; the winner is gathered with x[0, 2:] = 0
// (diffusion_model_dynamic.py:607).  One block of 1024 threads over rows [0, B) of the arrays it is given.
// result: {n_free, rank of the winner among the free ones, its row + row0, 0}.  SCENES: the static flow of a many-scene batch --
// the winner is copied unmodified, a block with no free row gets a NaN `best` and {0, -1, -1, 0}.  EPISODE: one episode of a many-episode
// replan -- the replan's rule on the winner (x[0, 2:] = 0), result[3] = 0 written, and without a free row `best` stays as it is.
template <bool SCENES, bool EPISODE = false>
__device__ __forceinline__ void select_block(const float* __restrict__ traj, const int* __restrict__ mask,
                                             const float* __restrict__ plen, const float* __restrict__ smooth,
                                             float w_s, float w_l, float* __restrict__ best,
                                             int* __restrict__ result, int B, int H, int S, int row0) {
  __shared__ int r_cnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const SelectRanges rg = select_ranges(mask, plen, smooth, B);
  float bt = INFINITY; int bi = SELECT_NONE;
  for (int b = tid; b < B; b += 1024) {
    if (mask[b]) continue;
    select_take(select_total(plen[b], smooth[b], rg, w_s, w_l), b, bt, bi);
  }
  const int bb = select_first_in_block(bt, bi);
  if (bb == SELECT_NONE) {
    if (tid == 0) { result[0] = 0; result[1] = -1; result[2] = -1; if (SCENES || EPISODE) result[3] = 0; }
    if (SCENES) for (int e = tid; e < H * S; e += 1024) best[e] = __int_as_float(0x7fc00000);
    return;
  }
  int rank = 0;
  for (int b = tid; b < bb; b += 1024) rank += !mask[b];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) rank += __shfl_xor(rank, m);
  if (lane == 0) r_cnt[wave] = rank;
  __syncthreads();
  if (tid == 0) { int r = 0; for (int w = 0; w < 16; ++w) r += r_cnt[w]; result[0] = rg.n_free; result[1] = r; result[2] = bb + row0; if (SCENES || EPISODE) result[3] = 0; }
  if (traj == nullptr) return;                            // selection from gathered costs only (multi-GPU merge): the winner's owner holds the row
  for (int e = tid; e < H * S; e += 1024) {
    float v = traj[(long)bb * H * S + e];
    if (!SCENES && e < S && e >= 2) v = 0.f;
    best[e] = v;
  }
}

__global__ __launch_bounds__(1024) void replan_select_kernel(const float* __restrict__ traj, const int* __restrict__ mask,
                                                              const float* __restrict__ plen, const float* __restrict__ smooth,
                                                              float w_s, float w_l, float* __restrict__ best,
                                                              int* __restrict__ result, int B, int H, int S) {
  select_block<false>(traj, mask, plen, smooth, w_s, w_l, best, result, B, H, S, 0);
}
// the same rule, one block per scene over the scene's rows [traj_first[s], traj_first[s + 1]) of a many-scene batch
__global__ __launch_bounds__(1024) void select_scenes_kernel(const float* __restrict__ traj, const int* __restrict__ mask,
                                                              const float* __restrict__ plen, const float* __restrict__ smooth,
                                                              float w_s, float w_l, const int* __restrict__ traj_first,
                                                              float* __restrict__ best, int* __restrict__ result, int B, int H, int S) {
  const int s = blockIdx.x;
  const int first = min(max(traj_first[s], 0), B), end = min(max(traj_first[s + 1], first), B);
  select_block<true>(traj + (long)first * H * S, mask + first, plen + first, smooth + first, w_s, w_l, best + (long)s * H * S,
                     result + 4 * s, end - first, H, S, first);
}
// the replan's rule, one block per episode of a many-episode replan over the episode's rows; an episode that has ended is skipped
__global__ __launch_bounds__(1024) void select_episodes_kernel(const float* __restrict__ traj, const int* __restrict__ mask,
                                                                const float* __restrict__ plen, const float* __restrict__ smooth,
                                                                float w_s, float w_l, const int* __restrict__ traj_first, EpisodeTable ep,
                                                                float* __restrict__ best, int* __restrict__ result, int B, int H, int S) {
  const int e = blockIdx.x;
  if (!ep.st[e].active) {                                   // (uniform over the block)
    if (threadIdx.x < 4) result[4 * e + threadIdx.x] = threadIdx.x < 3 ? -1 : 0;
    return;
  }
  const int first = min(max(traj_first[e], 0), B), end = min(max(traj_first[e + 1], first), B);
  select_block<false, true>(traj + (long)first * H * S, mask + first, plen + first, smooth + first, w_s, w_l, best + (long)e * H * S,
                            result + 4 * e, end - first, H, S, first);
}

// ---- K cheapest free rows per scene that are pairwise >= min_sep apart, and the mode of every free row (ramp_select_diverse_scenes in
// ramp_hip.h states the definition).  Pass k = one pick launch (one block per scene: the first row in select_block's order among the
// scene's candidates) and one update launch (one wave per row of the batch: its distance to that pick; suppressed flag, nearest slot and
// nearest distance).  Nothing is handed between blocks inside a launch: a pick reads what the update before it wrote, an update what
// the pick before it wrote.  A row's state in scratch: candidate, suppressed, representative or colliding.
enum { DIV_CANDIDATE = 0, DIV_SUPPRESSED = 1, DIV_REP = 2, DIV_COLLIDING = 3 };
// FIRST (pass 0): the scene's ranges and totals, as select_block forms them, and every row's state
template <bool FIRST>
__global__ __launch_bounds__(1024) void diverse_pick_kernel(DiverseArgs a, int k) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const int first = min(max(a.traj_first[s], 0), a.B), end = min(max(a.traj_first[s + 1], first), a.B), n = end - first;
  int* state = a.state + first; float* tot = a.tot + first;
  if (FIRST) {
    const SelectRanges rg = select_ranges(a.mask + first, a.plen + first, a.smooth + first, n);
    for (int b = tid; b < n; b += 1024) {             // (thread tid reads back only what it wrote here)
      const bool hit = a.mask[first + b] != 0;
      state[b] = hit ? DIV_COLLIDING : DIV_CANDIDATE;
      if (!hit) tot[b] = select_total(a.plen[first + b], a.smooth[first + b], rg, a.w_s, a.w_l);
    }
    if (tid == 0) a.result[4 * s] = rg.n_free;
  }
  float bt = INFINITY; int bi = SELECT_NONE;
  for (int b = tid; b < n; b += 1024)
    if (state[b] == DIV_CANDIDATE) select_take(tot[b], b, bt, bi);
  const int bb = select_first_in_block(bt, bi);
  const long slot = (long)s * a.K + k;
  if (tid == 0) { a.pick[s] = bb == SELECT_NONE ? -1 : first + bb; a.rows[slot] = bb == SELECT_NONE ? -1 : first + bb; }
  float* best = a.best + slot * a.H * a.S;
  const float* row = a.traj + (long)(first + (bb == SELECT_NONE ? 0 : bb)) * a.H * a.S;
  for (int e = tid; e < a.H * a.S; e += 1024) best[e] = bb == SELECT_NONE ? __int_as_float(0x7fc00000) : row[e];
}
// a NaN on either side stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float max_keep_nan(float x, float y) { return x != x ? x : (y != y ? y : fmaxf(x, y)); }
// d(b, r) of the definition, the same value in every lane of the wave: per-waypoint norm over D coordinates in fp32 (differences, squares
// added in coordinate order, root); metric 0: the norms added in fp64 in ascending h, over H, rounded to fp32 once; metric 1: their maximum
template <int D>
__device__ __forceinline__ float diverse_distance(const float* __restrict__ pb, const float* __restrict__ pr, int H, int S, int metric,
                                                  int lane) {
  float nrm[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {                        // H <= 128: waypoints lane and lane + 64
    const int h = lane + 64 * i;
    nrm[i] = 0.f;
    if (h < H) {
      const float dx = sub(pb[h * S], pr[h * S]), dy = sub(pb[h * S + 1], pr[h * S + 1]);
      float d2 = add(mul(dx, dx), mul(dy, dy));
      if (D == 3) { const float dz = sub(pb[h * S + 2], pr[h * S + 2]); d2 = add(d2, mul(dz, dz)); }
      nrm[i] = __fsqrt_rn(d2);
    }
  }
  if (metric == 1) {
    float m = max_keep_nan(nrm[0], nrm[1]);            // (norms are >= 0: the 0 of a waypoint past H changes nothing)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max_keep_nan(m, __shfl_xor(m, o));
    return m;
  }
  double acc = 0.0;
  for (int h = 0; h < min(H, 64); ++h) acc += (double)__shfl(nrm[0], h);
  for (int h = 64; h < H; ++h) acc += (double)__shfl(nrm[1], h - 64);
  return (float)(acc / (double)H);
}
// one wave per row b of the batch, 4 rows per block; the row's scene by bisection of the clamped table (non-decreasing)
template <int D>
__global__ __launch_bounds__(256) void diverse_update_kernel(DiverseArgs a, int k) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                                 // (uniform over the wave; the kernel has no block-wide step)
  if (k == 0 && lane == 0) { a.mode_of[b] = -1; a.sep[b] = __int_as_float(0x7fc00000); }
  int lo = 0, hi = a.n_scenes;                          // the first i in [1, n_scenes] with traj_first[i] > b, or n_scenes + 1; s = i - 1
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (min(max(a.traj_first[mid + 1], 0), a.B) > b) hi = mid; else lo = mid + 1;
  }
  const int s = lo;
  if (s >= a.n_scenes || min(max(a.traj_first[s], 0), a.B) > b) return;      // a row of no scene
  const int st = a.state[b];
  if (st >= DIV_REP) return;
  const int r = a.pick[s];
  if (r < 0) return;                                    // the scene has run out of candidates
  const float d = diverse_distance<D>(a.traj + (long)b * a.H * a.S, a.traj + (long)r * a.H * a.S, a.H, a.S, a.metric, lane);
  if (lane != 0) return;
  if (b == r) { a.state[b] = DIV_REP; a.mode_of[b] = k; a.sep[b] = d; return; }      // a representative belongs to its own slot
  if (st == DIV_CANDIDATE && !(d >= a.min_sep)) a.state[b] = DIV_SUPPRESSED;          // (a NaN distance suppresses)
  if (d == d && (a.mode_of[b] < 0 || d < a.sep[b])) { a.mode_of[b] = k; a.sep[b] = d; }   // the lowest slot keeps a tie; a NaN never wins
}
// rows per slot, and the scene's record
__global__ __launch_bounds__(256) void diverse_finish_kernel(DiverseArgs a) {
  __shared__ int cnt[DIVERSE_MAX_K];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int first = min(max(a.traj_first[s], 0), a.B), end = min(max(a.traj_first[s + 1], first), a.B);
  if (tid < DIVERSE_MAX_K) cnt[tid] = 0;
  __syncthreads();
  for (int b = first + tid; b < end; b += 256) {
    const int m = a.mode_of[b];
    if (m >= 0 && m < a.K) atomicAdd(&cnt[m], 1);
  }
  __syncthreads();
  if (tid < a.K) a.mode_count[(long)s * a.K + tid] = cnt[tid];
  if (tid == 0) {
    int n_sel = 0;
    for (int j = 0; j < a.K; ++j) n_sel += a.rows[(long)s * a.K + j] >= 0;
    a.result[4 * s + 1] = n_sel; a.result[4 * s + 2] = a.rows[(long)s * a.K]; a.result[4 * s + 3] = 0;
  }
}
// 2 K + 1 launches whatever the scenes, the rows and the data
int launch_select_diverse(const DiverseArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.B >= 0 && a.H >= 1 && a.H <= 128 && (a.D == 2 || a.D == 3) && a.D <= a.S && a.n_scenes >= 1 && a.K >= 1 &&
               a.K <= DIVERSE_MAX_K, "bad diverse selection dims");
  const dim3 rows((a.B + 3) / 4 > 0 ? (a.B + 3) / 4 : 1);
  for (int k = 0; k < a.K; ++k) {
    if (k == 0) hipLaunchKernelGGL(diverse_pick_kernel<true>, dim3(a.n_scenes), dim3(1024), 0, s, a, k);
    else hipLaunchKernelGGL(diverse_pick_kernel<false>, dim3(a.n_scenes), dim3(1024), 0, s, a, k);
    RAMP_HIP_CHECK(hipGetLastError());
    if (a.D == 3) hipLaunchKernelGGL(diverse_update_kernel<3>, rows, dim3(256), 0, s, a, k);
    else hipLaunchKernelGGL(diverse_update_kernel<2>, rows, dim3(256), 0, s, a, k);
    RAMP_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(diverse_finish_kernel, dim3(a.n_scenes), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

static int check_episode_table(const EpisodeTable& ep, int B) {
  RAMP_REQUIRE(ep.st && ep.row_ep && ep.n_episodes > 0 && ep.n_episodes <= B, "bad episode table");
  return 0;
}
int launch_replan_init_episodes(float* x, const float* x_clean, const float* noise, float sa, float s1a, const float* hist,
                                EpisodeTable ep, int B, int H, int S, hipStream_t s) {
  if (int rc = check_episode_table(ep, B)) return rc;
  hipLaunchKernelGGL(replan_init_episodes_kernel, dim3(ew_grid((long)B * H * S)), dim3(256), 0, s, x, x_clean, noise, sa, s1a, hist, ep, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_replan_pin_episodes(float* x, HardConds hc, const float* hist, const float* x_clean, EpisodeTable ep, int B, int H, int S,
                               hipStream_t s) {
  if (int rc = check_episode_table(ep, B)) return rc;
  hipLaunchKernelGGL(replan_pin_episodes_kernel, dim3((B * S + 255) / 256), dim3(256), 0, s, x, hc, hist, x_clean, ep, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_replan_sm_episodes(float* x, EpisodeTable ep, int window, float dt, float max_vel, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(S >= 4 && window >= 1, "sm needs (x, y, vx, vy) states");
  if (int rc = check_episode_table(ep, B)) return rc;
  hipLaunchKernelGGL(replan_sm_episodes_kernel, dim3((B + 255) / 256), dim3(256), 0, s, x, ep, window, dt, max_vel, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_replan_near_episodes(const float* x, EpisodeTable ep, float thr, int* en, int B, int H, int S, hipStream_t s) {
  if (int rc = check_episode_table(ep, B)) return rc;
  hipLaunchKernelGGL(replan_near_episodes_kernel, dim3((B + 255) / 256), dim3(256), 0, s, x, ep, thr, en, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_select_episodes(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                           const int* traj_first, EpisodeTable ep, float* best, int* result, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 0 && S >= 2 && traj && best && result && traj_first, "bad selection dims");
  if (int rc = check_episode_table(ep, B)) return rc;
  hipLaunchKernelGGL(select_episodes_kernel, dim3(ep.n_episodes), dim3(1024), 0, s, traj, mask, plen, smooth, w_s, w_l, traj_first, ep,
                     best, result, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_replan_goal(float* x0, const float* x, int B, int H, int S, hipStream_t s) {
  hipLaunchKernelGGL(replan_goal_kernel, dim3((B * S + 255) / 256), dim3(256), 0, s, x0, x, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_replan_select(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                         float* best, int* result, int B, int H, int S, hipStream_t s) {
  hipLaunchKernelGGL(replan_select_kernel, dim3(1), dim3(1024), 0, s, traj, mask, plen, smooth, w_s, w_l, best, result, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_select_scenes(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                         const int* traj_first, int n_scenes, float* best, int* result, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 0 && S >= 2 && n_scenes > 0 && n_scenes <= B, "bad selection dims");
  hipLaunchKernelGGL(select_scenes_kernel, dim3(n_scenes), dim3(1024), 0, s, traj, mask, plen, smooth, w_s, w_l, traj_first, best,
                     result, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// Dynamic-planner APF (APFhelper_dynamic.py:107-142), one block per trajectory, points in float64 like the
// reference's numpy clouds.  window >= 0: static pass, pushes only waypoints [ci - w, min(H-1, ci + w)) around the
// waypoint ci nearest to the cloud; window < 0: pursuer pass over waypoints [0, affected) with the 0.9 / 0.1
// avoid / goal blend.  Each waypoint update is independent (no accumulation across waypoints).
// ------------------------------------------------------------------------------------------
// EP: the trajectory's own episode (ApfDynArgs.episode): block b streams only its episode's points, indexed from that cloud's first
// point, and blends towards its own goal, so every comparison, tie and sum is the one-cloud kernel's on that cloud.  An episode
// index outside the table leaves the trajectory as it is.
template <bool EP>
__global__ __launch_bounds__(256) void apf_dyn_kernel(ApfDynArgs a) {
  __shared__ double2 cl[APF_TILE];
  __shared__ double best_d2[APF_MAXH];
  __shared__ int best_i[APF_MAXH];
  __shared__ int s_lo, s_hi;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (a.enable && !a.enable[b]) return;
  if (EP) {
    const int e = a.episode[b];
    if (e < 0 || e >= a.n_episodes) return;                  // (uniform over the block)
    if (a.ep_off) {
      const int p0 = min(max(a.ep_off[e], 0), a.P), p1 = min(max(a.ep_off[e + 1], p0), a.P);
      a.points += 2l * p0; a.P = p1 - p0;
    } else {
      a.points += 2l * e * a.P;
    }
    if (a.goal) a.goal += (long)b * a.H * a.S;
  }
  float* tr = a.traj + (long)b * a.H * a.S;
  const int nq = a.window >= 0 ? a.H : min(a.affected, a.H);
  for (int h = tid; h < a.H; h += 256) { best_d2[h] = 1.0e300; best_i[h] = -1; }
  for (int p0 = 0; p0 < a.P; p0 += APF_TILE) {
    const int np = min(APF_TILE, a.P - p0);
    __syncthreads();
    for (int e = tid; e < np; e += 256) cl[e] = make_double2(a.points[(p0 + e) * 2], a.points[(p0 + e) * 2 + 1]);
    __syncthreads();
    for (int h = wave; h < nq; h += 4) {
      const double qx = (double)tr[h * a.S], qy = (double)tr[h * a.S + 1];
      double bd = 1.0e300; int bi = -1;
      for (int e = lane; e < np; e += 64) {
        const double dx = qx - cl[e].x, dy = qy - cl[e].y;
        const double d2 = dx * dx + dy * dy;
        if (d2 < bd) { bd = d2; bi = p0 + e; }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        if (od < bd || (od == bd && oi >= 0 && (bi < 0 || oi < bi))) { bd = od; bi = oi; }
      }
      if (lane == 0 && bi >= 0 && bd < best_d2[h]) { best_d2[h] = bd; best_i[h] = bi; }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double bm = 1.0e300; int ci = 0;                     // np.argmin over distances with inf for misses
    for (int h = 0; h < nq; ++h) {
      const double d = sqrt(best_d2[h]);
      if (best_i[h] >= 0 && d < a.thr_query && d < bm) { bm = d; ci = h; }
    }
    if (a.window >= 0) { s_lo = max(0, ci - a.window); s_hi = min(a.H - 1, ci + a.window); }
    else { s_lo = 0; s_hi = nq; }
  }
  __syncthreads();
  for (int h = s_lo + tid; h < s_hi; h += 256) {
    const double d = sqrt(best_d2[h]);
    if (!(best_i[h] >= 0 && d < a.thr_query)) continue;
    const float tx = tr[h * a.S], ty = tr[h * a.S + 1];
    double ax = (double)tx - a.points[best_i[h] * 2], ay = (double)ty - a.points[best_i[h] * 2 + 1];
    const double an = sqrt(ax * ax + ay * ay) + 1e-8;
    ax /= an; ay /= an;
    double cx = ax, cy = ay;
    if (a.goal) {
      float gx = sub(a.goal[0], tx), gy = sub(a.goal[1], ty);
      const float gn = add(sqrtf(add(mul(gx, gx), mul(gy, gy))), 1e-8f);
      gx = __fdiv_rn(gx, gn); gy = __fdiv_rn(gy, gn);
      cx = 0.9 * ax + 0.1 * (double)gx; cy = 0.9 * ay + 0.1 * (double)gy;
      const double cn = sqrt(cx * cx + cy * cy) + 1e-8;
      cx /= cn; cy /= cn;
    }
    const double force = a.strength * exp(-d / a.thr_force);
    tr[h * a.S] = (float)((double)tx + force * cx);
    tr[h * a.S + 1] = (float)((double)ty + force * cy);
  }
}
int launch_apf_dynamic(const ApfDynArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.B > 0 && a.H > 0 && a.H <= APF_MAXH && a.S >= 2 && a.P > 0 && a.traj && a.points, "bad dynamic-APF dims");
  RAMP_REQUIRE(!a.episode || a.n_episodes > 0, "dynamic APF with per-trajectory episodes needs their count");
  if (a.episode) hipLaunchKernelGGL(apf_dyn_kernel<true>, dim3(a.B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(apf_dyn_kernel<false>, dim3(a.B), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// trajectory costs: collision mask against the cloud, path length, smoothness (cost.py:3-54)
// ------------------------------------------------------------------------------------------
// one block of 256 threads per trajectory `tr` against the P points of `cloud`; shared by the one-cloud and the per-scene kernel
__device__ __forceinline__ void traj_costs_block(const float* __restrict__ tr, const float* __restrict__ cloud,
                                                 int H, int S, int P, float thr, int* __restrict__ mask,
                                                 float* __restrict__ plen, float* __restrict__ smooth) {
  __shared__ float2 cl[APF_TILE];
  __shared__ float xy[APF_MAXH * 2];
  __shared__ int any_hit;
  __shared__ float segl[APF_MAXH], segs[APF_MAXH];
  const int tid = threadIdx.x;
  if (tid == 0) any_hit = 0;
  for (int h = tid; h < H; h += 256) { xy[2 * h] = tr[h * S]; xy[2 * h + 1] = tr[h * S + 1]; }
  for (int p0 = 0; p0 < P; p0 += APF_TILE) {
    const int np = min(APF_TILE, P - p0);
    __syncthreads();
    for (int e = tid; e < np; e += 256) cl[e] = make_float2(cloud[(p0 + e) * 2], cloud[(p0 + e) * 2 + 1]);
    __syncthreads();
    int hit = 0;
    for (int e = tid; e < np * H; e += 256) {
      const int h = e / np, pi = e - h * np;
      const float dx = sub(xy[2 * h], cl[pi].x), dy = sub(xy[2 * h + 1], cl[pi].y);
      // torch.norm(diff, dim=-1) < thr
      hit |= (sqrtf(add(mul(dx, dx), mul(dy, dy))) < thr);
    }
    if (__any(hit) && (tid & 63) == 0) atomicOr(&any_hit, 1);
  }
  for (int h = tid; h < H - 1; h += 256) {
    const float dx = sub(tr[(h + 1) * S], tr[h * S]), dy = sub(tr[(h + 1) * S + 1], tr[h * S + 1]);
    segl[h] = sqrtf(add(mul(dx, dx), mul(dy, dy)));
    float ss = 0.f;
    for (int c = 2; c < S; ++c) { const float dv = sub(tr[(h + 1) * S + c], tr[h * S + c]); ss = add(ss, mul(dv, dv)); }
    segs[h] = sqrtf(ss);
  }
  __syncthreads();
  if (tid == 0) {
    float pl = 0.f, sm = 0.f;
    for (int h = 0; h < H - 1; ++h) { pl = add(pl, segl[h]); sm = add(sm, segs[h]); }
    *mask = any_hit; *plen = pl; *smooth = sm;
  }
}
__global__ __launch_bounds__(256) void traj_costs_kernel(const float* __restrict__ traj, const float* __restrict__ cloud,
                                                          int H, int S, int P, float thr, int* __restrict__ mask,
                                                          float* __restrict__ plen, float* __restrict__ smooth) {
  const int b = blockIdx.x;
  traj_costs_block(traj + (long)b * H * S, cloud, H, S, P, thr, mask + b, plen + b, smooth + b);
}
// traj_costs_kernel for a batch of many scenes: row b reads the points [cloud_off[s], cloud_off[s + 1]) of its own scene s,
// found by bisection of traj_first (n_scenes + 1, increasing).  Spans are clamped to [0, P_total]: a wrong table reads wrong
// points, never outside the cloud.
__global__ __launch_bounds__(256) void traj_costs_scenes_kernel(const float* __restrict__ traj, const float* __restrict__ cloud,
                                                                 const int* __restrict__ traj_first, const int* __restrict__ cloud_off,
                                                                 int n_scenes, int P_total, int H, int S, float thr,
                                                                 int* __restrict__ mask, float* __restrict__ plen,
                                                                 float* __restrict__ smooth) {
  const int b = blockIdx.x;
  int lo = 0, hi = n_scenes - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (traj_first[mid] <= b) lo = mid; else hi = mid - 1; }
  const int p0 = min(max(cloud_off[lo], 0), P_total), p1 = min(max(cloud_off[lo + 1], p0), P_total);
  traj_costs_block(traj + (long)b * H * S, cloud + 2 * (long)p0, H, S, p1 - p0, thr, mask + b, plen + b, smooth + b);
}
// the cost segments of a many-episode replan: block e copies episode e's static cost points, then its n_extra extra points
__global__ __launch_bounds__(256) void episode_cost_segments_kernel(float2* __restrict__ dst, const float2* __restrict__ cloud,
                                                                     const float2* __restrict__ extra, const int* __restrict__ seg_off,
                                                                     int n_extra, int P_total) {
  const int e = blockIdx.x;
  const int d0 = min(max(seg_off[e], 0), P_total), d1 = min(max(seg_off[e + 1], d0), P_total);
  const int nc = max(d1 - d0 - n_extra, 0);                 // static points of this episode
  const long s0 = (long)d0 - (long)e * n_extra;              // its first point in `cloud`
  if (s0 < 0) return;
  for (int i = threadIdx.x; i < d1 - d0; i += 256)
    dst[d0 + i] = i < nc ? cloud[s0 + i] : extra[(long)e * n_extra + (i - nc)];
}
int launch_episode_cost_segments(float* dst, const float* cloud, const float* extra, const int* seg_off, int n_episodes, int n_extra,
                                 int P_total, hipStream_t s) {
  RAMP_REQUIRE(dst && cloud && seg_off && n_episodes > 0 && n_extra >= 0 && P_total > 0 && (extra || n_extra == 0), "bad cost segments");
  RAMP_REQUIRE(((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(cloud) | reinterpret_cast<uintptr_t>(extra)) & 7) == 0, "cost points must be 8-byte aligned");
  hipLaunchKernelGGL(episode_cost_segments_kernel, dim3(n_episodes), dim3(256), 0, s, reinterpret_cast<float2*>(dst),
                     reinterpret_cast<const float2*>(cloud), reinterpret_cast<const float2*>(extra), seg_off, n_extra, P_total);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_traj_costs(const float* traj, const float* cloud, int B, int H, int S, int P, float thr, int* mask,
                      float* plen, float* smooth, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 1 && H <= APF_MAXH && S >= 2 && P > 0, "bad cost dims");
  hipLaunchKernelGGL(traj_costs_kernel, dim3(B), dim3(256), 0, s, traj, cloud, H, S, P, thr, mask, plen, smooth);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_traj_costs_scenes(const float* traj, const float* cloud, const int* traj_first, const int* cloud_off, int n_scenes,
                             int P_total, int B, int H, int S, float thr, int* mask, float* plen, float* smooth, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && S >= 2 && n_scenes > 0 && n_scenes <= B && P_total > 0, "bad cost dims");
  RAMP_REQUIRE(H > 1 && H <= APF_MAXH, "horizon beyond the cost kernel's limit");
  hipLaunchKernelGGL(traj_costs_scenes_kernel, dim3(B), dim3(256), 0, s, traj, cloud, traj_first, cloud_off, n_scenes, P_total, H, S,
                     thr, mask, plen, smooth);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- Gaussian noise inside the job: counter-based Philox4x32-10 (Salmon et al., SC'11) + Box-Muller --------------------------
// The reference draws torch.randn on the host stream (sample_functions.py:36, diffusion_model_static.py:239); a throughput job
// draws the same N(0, I) inside its captured graph instead.  Element 4 g + j of the stream is output j of
// philox4x32_10(counter = (lo32(g + offset), hi32(g + offset), 0, 0), key = (lo32(seed), hi32(seed))) turned into a normal:
// u = ((r >> 9) + 0.5) * 2^-23 in (0, 1) (exact in fp32); (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1), (z2, z3) likewise from (u2, u3).
// Host-replicable from (seed, offset) alone (tests/util.py restates it in numpy); seed / offset live in a 16-byte device
// record so that a captured graph draws fresh noise on every replay.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// grp_row = groups of four per (sample, block) = HS / 4; a shard's local group g = (j B + b) grp_row + q is the stream's group
// (j B_total + sample0 + b) grp_row + q.  grp_row == 0: the flat stream (local group = stream group).
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, long n, const unsigned long long* __restrict__ rec,
                                                             long grp_row, long B, long sample0, long B_total) {
  const unsigned long long seed = rec[0], offset = rec[1];
  const long n_grp = (n + 3) >> 2;
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n_grp; g += (long)gridDim.x * 256) {
    long gg = g;
    if (grp_row > 0) {
      const long sb = g / grp_row, q = g - sb * grp_row;      // sb = j B + b
      const long j = sb / B, b = sb - j * B;
      gg = (j * B_total + sample0 + b) * grp_row + q;
    }
    const unsigned long long ctr = (unsigned long long)gg + offset;
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    float z[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u0 = ((float)(c[2 * h] >> 9) + 0.5f) * 1.1920928955078125e-7f;
      const float u1 = ((float)(c[2 * h + 1] >> 9) + 0.5f) * 1.1920928955078125e-7f;
      const float rad = sqrtf(-2.f * logf(u0));
      float sn, cs;
      sincosf(6.283185307179586f * u1, &sn, &cs);
      z[2 * h] = rad * cs; z[2 * h + 1] = rad * sn;
    }
    const long e = g << 2;
    if (e + 3 < n) *reinterpret_cast<float4*>(out + e) = make_float4(z[0], z[1], z[2], z[3]);
    else for (int j = 0; j < 4 && e + j < n; ++j) out[e + j] = z[j];
  }
}
int launch_philox_normal(float* out, long n, const unsigned long long* rec, hipStream_t s) {
  RAMP_REQUIRE(out && rec && n > 0, "philox: null operand");
  RAMP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "philox: output must be 16-byte aligned");
  const long n_grp = (n + 3) >> 2;
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)std::min<long>((n_grp + 255) / 256, 8192)), dim3(256), 0, s, out, n, rec, 0l, 1l, 0l, 1l);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_philox_normal_sharded(float* out, int n_blocks, int B, int HS, long sample0, long B_total, const unsigned long long* rec, hipStream_t s,
                                 long block0) {
  RAMP_REQUIRE(out && rec && n_blocks > 0 && B > 0 && HS > 0 && HS % 4 == 0, "philox: bad shard dims (H S must be a multiple of 4)");
  RAMP_REQUIRE(sample0 >= 0 && B_total >= sample0 + B && block0 >= 0, "philox: the shard [sample0, sample0 + B) must lie inside the job's B_total samples");
  RAMP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "philox: output must be 16-byte aligned");
  const long n = (long)n_blocks * B * HS, n_grp = n >> 2;
  // (block j of this launch is block block0 + j of the stream: (block0 + j) B_total + sample0 + b = j B_total + (block0 B_total + sample0) + b)
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)std::min<long>((n_grp + 255) / 256, 8192)), dim3(256), 0, s, out, n, rec,
                     (long)(HS / 4), (long)B, block0 * B_total + sample0, B_total);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// out[k B + b] = the uniform of (inner step k, global sample sample0 + b): u = ((r >> 9) + 0.5) 2^-23 in (0, 1), r = output 0 of the stream's group
// group0 + k B_total + sample0 + b (one group per uniform, its other three words unused)
__global__ __launch_bounds__(256) void philox_uniform_kernel(float* __restrict__ out, long n, const unsigned long long* __restrict__ rec,
                                                              long group0, long B, long sample0, long B_total) {
  const unsigned long long seed = rec[0], offset = rec[1];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long k = i / B, b = i - k * B;
    const unsigned long long ctr = (unsigned long long)(group0 + k * B_total + sample0 + b) + offset;
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    out[i] = ((float)(c[0] >> 9) + 0.5f) * 1.1920928955078125e-7f;
  }
}
int launch_philox_uniform_sharded(float* out, int n_blocks, int B, long group0, long sample0, long B_total, const unsigned long long* rec,
                                  hipStream_t s) {
  RAMP_REQUIRE(out && rec && n_blocks > 0 && B > 0 && group0 >= 0, "philox uniform: bad dims");
  RAMP_REQUIRE(sample0 >= 0 && B_total >= sample0 + B, "philox uniform: the shard [sample0, sample0 + B) must lie inside the job's B_total samples");
  const long n = (long)n_blocks * B;
  hipLaunchKernelGGL(philox_uniform_kernel, dim3((unsigned)std::min<long>((n + 255) / 256, 8192)), dim3(256), 0, s, out, n, rec, group0, (long)B,
                     sample0, B_total);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- energies and Langevin refinement (ULA / MALA) ---------------------------------------------------------------------------
// The score is an energy gradient, eps = grad_x 1/2 ||f(x, t, scene)||^2 (UnetInference.py:26-32 returns the energy next to it), so two
// states can be compared: E[r] = 1/2 sum_{h,s} f[r,h,s]^2.  One wave per row: lane l adds the fp32 squares of elements l, l + 64, ... in
// fp64 in that order, then the 64 partial sums meet in a fixed butterfly -- no atomics, the same bits whatever the launch's row count is.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__global__ __launch_bounds__(256) void row_energy_kernel(const float* __restrict__ f, double* __restrict__ E, int R, int HS) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;                                  // (a whole wave leaves together)
  const float* fr = f + (size_t)r * HS;
  double acc = 0.0;
  for (int e = lane; e < HS; e += 64) { const float v = fr[e]; acc += (double)mul(v, v); }
  acc = wave_sum(acc);
  if (lane == 0) E[r] = 0.5 * acc;
}
int launch_row_energy(const float* f, double* E, int R, int HS, hipStream_t s) {
  RAMP_REQUIRE(f && E && R > 0 && HS > 0, "row_energy: bad operands");
  hipLaunchKernelGGL(row_energy_kernel, dim3((R + 3) / 4), dim3(256), 0, s, f, E, R, HS);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
// E_comb[b] = sum_j w_j E[b n_rp + j] in fp64, j ascending: w the job's three host scalars (w.rw == nullptr) or line b of the device table
__global__ __launch_bounds__(256) void combine_energy_kernel(const double* __restrict__ E, EnergyWeights w, double* __restrict__ out, int B, int n_rp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double acc = 0.0;
  for (int j = 0; j < n_rp; ++j) {
    const float wj = w.rw ? w.rw[(size_t)b * n_rp + j] : w.w[j];
    acc += (double)wj * E[(size_t)b * n_rp + j];
  }
  out[b] = acc;
}
int launch_combine_energy(const double* E_rows, const EnergyWeights& w, double* E_comb, int B, int n_rp, hipStream_t s) {
  RAMP_REQUIRE(E_rows && E_comb && B > 0 && n_rp >= 1 && n_rp <= 8 && (w.rw || n_rp <= 3), "combine_energy: bad operands");
  hipLaunchKernelGGL(combine_energy_kernel, dim3((B + 255) / 256), dim3(256), 0, s, E_rows, w, E_comb, B, n_rp);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

__device__ __forceinline__ bool pinned(const HardConds& hc, int h) {
  bool hit = false;
  for (int k = 0; k < hc.n; ++k) hit |= (hc.idx[k] == h);
  return hit;
}
// Langevin proposal: x' = (x - a eps) + c z on free waypoints (two products, a difference and a sum in fp32, no contraction), x' = x on the
// waypoints the hard conditions pin
__global__ __launch_bounds__(256) void mcmc_propose_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ z,
                                                            float a, float cz, HardConds hc, float* __restrict__ xp, int B, int H, int S) {
  const long n = (long)B * H * S;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int h = (int)((idx / S) % H);
    const float xv = x[idx];
    xp[idx] = pinned(hc, h) ? xv : add(sub(xv, mul(a, eps[idx])), mul(cz, z[idx]));
  }
}
int launch_mcmc_propose(const float* x, const float* eps, const float* z, float a, float cz, HardConds hc, float* xp, int B, int H, int S,
                        hipStream_t s) {
  RAMP_REQUIRE(x && eps && z && xp && B > 0 && H > 0 && S > 0, "mcmc_propose: bad operands");
  hipLaunchKernelGGL(mcmc_propose_kernel, dim3(ew_grid((long)B * H * S)), dim3(256), 0, s, x, eps, z, a, cz, hc, xp, B, H, S);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
// Accept / reject, one wave per trajectory.  mala: log alpha = -(E' - E) / sigma - (||x - x' + a eps'||^2 - ||x' - x + a eps||^2) / (4 eta), every
// term and both sums in fp64 over the free elements (lane l adds elements l, l + 64, ... in order, then the butterfly); accepted when
// log u < log alpha with E' and log alpha finite.  !mala (ULA): always.  An accepted trajectory's x, eps (and E) become the proposal's.
__global__ __launch_bounds__(256) void mcmc_accept_kernel(McmcAcceptArgs a) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= a.B) return;
  const int HS = a.H * a.S;
  const size_t o = (size_t)b * HS;
  bool acc = true;
  double la = 0.0;
  if (a.mala) {
    double fwd = 0.0, rev = 0.0;
    for (int e = lane; e < HS; e += 64) {
      if (pinned(a.hc, e / a.S)) continue;
      const double xv = a.x[o + e], xq = a.xp[o + e];
      const double dr = xv - xq + (double)a.a * (double)a.eps_p[o + e];      // x - mean(x')
      const double df = xq - xv + (double)a.a * (double)a.eps[o + e];        // x' - mean(x)
      rev += dr * dr; fwd += df * df;
    }
    rev = wave_sum(rev); fwd = wave_sum(fwd);
    const double Ep = a.E_p[b];
    la = -(Ep - a.E[b]) * a.inv_sigma - (rev - fwd) * a.inv_4eta;
    acc = isfinite(Ep) && isfinite(la) && log((double)a.u[b]) < la;
    if (lane == 0 && a.log_alpha) a.log_alpha[b] = la;
  }
  if (acc) {
    for (int e = lane; e < HS; e += 64) { a.x[o + e] = a.xp[o + e]; a.eps[o + e] = a.eps_p[o + e]; }
    if (lane == 0 && a.mala) a.E[b] = a.E_p[b];
  }
  if (lane == 0) a.flag[b] = acc ? 1 : 0;
}
int launch_mcmc_accept(const McmcAcceptArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.x && a.xp && a.eps && a.eps_p && a.flag && a.B > 0 && a.H > 0 && a.S > 0, "mcmc_accept: bad operands");
  RAMP_REQUIRE(!a.mala || (a.E && a.E_p && a.u), "mcmc_accept: MALA needs the energies and the uniforms");
  hipLaunchKernelGGL(mcmc_accept_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
