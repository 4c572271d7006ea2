// Stitched windows (ramp_stitch in include/ramp_hip.h): a long trajectory of L = H + (W - 1) st waypoints, st = H - O, lives as W overlapping
// windows of H waypoints in adjacent rows of one batch -- row c W + w is window w of chain c and covers the long waypoints [w st, w st + H).
// O <= H / 2, so a long waypoint lies in at most two windows and a window's head [0, O) and tail [st, H) are disjoint.
//
// stitch_kernel makes the windows of every chain agree, in place and in ONE launch:
//   blend  l = a[r, st + k, s], q = a[r + 1, k, s] (w < W - 1, k < O): both become m = l + alpha_k (q - l); q == l returns l itself
//   pins   every window that covers the long waypoint idx_i holds val[i, c, :] there; later pins win, pins win over the blend
// No element is written by two threads: thread (c, w, k, s) of the first section owns BOTH locations of its overlap element and writes either
// the blend or the pin that names that waypoint; thread (i, c, s) of the second section writes a pin only where its waypoint lies in ONE
// window and no later pin names it.  Nothing else of the array is touched.
//
// assemble_kernel reads the long trajectory back: long[c, l, :] from the window with the smallest w that covers l.
//
// Built with -ffp-contract=off like guide.hip: the difference, the product and the sum are rounded once each, as written.
#include "args_sampler.h"

namespace ramp {

namespace {

// the last pin that names the long waypoint l, or -1
__device__ __forceinline__ int stitch_pin_of(const StitchArgs& a, int l) {
  int last = -1;
  for (int i = 0; i < a.n_pin; ++i) if (a.pin_idx[i] == l) last = i;
  return last;
}

}  // namespace

__global__ __launch_bounds__(256) void stitch_kernel(StitchArgs a) {
  const int W = a.W, H = a.H, S = a.S, O = a.W > 1 ? a.O : 0, st = H - O;
  const long n_blend = (long)a.C * (W - 1) * O * S, n_pinned = (long)a.n_pin * a.C * S;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < n_blend) {
    const int s = (int)(idx % S), k = (int)((idx / S) % O), w = (int)((idx / ((long)S * O)) % (W - 1));
    const long c = idx / ((long)S * O * (W - 1)), r = c * W + w;
    float* pl = a.x + ((size_t)r * H + st + k) * S + s;
    float* pq = a.x + ((size_t)(r + 1) * H + k) * S + s;
    const int pin = stitch_pin_of(a, (w + 1) * st + k);
    float m;
    if (pin >= 0) {
      m = a.pin_val[((size_t)pin * a.C + c) * S + s];
    } else {
      const float l = *pl, q = *pq;
      m = q == l ? l : __fadd_rn(l, __fmul_rn(a.alpha[k], __fsub_rn(q, l)));
    }
    *pl = m; *pq = m;
  } else if (idx - n_blend < n_pinned) {
    const long j = idx - n_blend;
    const int s = (int)(j % S), i = (int)(j / ((long)S * a.C));
    const long c = (j / S) % a.C;
    const int l = a.pin_idx[i];
    for (int i2 = i + 1; i2 < a.n_pin; ++i2) if (a.pin_idx[i2] == l) return;      // a later pin wins
    const int wq = l / st;
    if (wq >= 1 && wq <= W - 1 && l - wq * st < O) return;                          // in two windows: the blend section writes it
    const int w = min(wq, W - 1), h = l - w * st;
    if (l < 0 || h >= H) return;                                                    // (outside the long trajectory: the host refuses it)
    a.x[((size_t)(c * W + w) * H + h) * S + s] = a.pin_val[j];
  }
}

__global__ __launch_bounds__(256) void assemble_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int W, int H, int S, int O) {
  const int st = H - (W > 1 ? O : 0), L = H + (W - 1) * st;
  const long n = (long)C * L * S, idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int s = (int)(idx % S), l = (int)((idx / S) % L);
  const long c = idx / ((long)S * L);
  const int w = l < H ? 0 : (l - H) / st + 1;
  out[idx] = x[((size_t)(c * W + w) * H + (l - w * st)) * S + s];
}

static int check_stitch_dims(int C, int W, int H, int S, int O) {
  RAMP_REQUIRE(C > 0 && W >= 1 && H > 0 && S > 0, "stitch: bad dims");
  RAMP_REQUIRE(W == 1 || (O >= 1 && 2 * O <= H), "stitch: overlap outside 1 .. H / 2");
  RAMP_REQUIRE((long)C * W * H * S < (1l << 31), "stitch: batch too large");
  return 0;
}

int launch_stitch(const StitchArgs& a, hipStream_t s) {
  if (int rc = check_stitch_dims(a.C, a.W, a.H, a.S, a.O)) return rc;
  RAMP_REQUIRE(a.x && (a.W == 1 || a.alpha), "stitch: null array or blend table");
  RAMP_REQUIRE(a.n_pin >= 0 && a.n_pin <= STITCH_MAX_PINS && (a.n_pin == 0 || a.pin_val), "stitch: bad pins");
  const long n = (long)a.C * (a.W - 1) * (a.W > 1 ? a.O : 0) * a.S + (long)a.n_pin * a.C * a.S;
  if (n == 0) return 0;
  hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_stitch_assemble(const float* x, float* out, int C, int W, int H, int S, int O, hipStream_t s) {
  if (int rc = check_stitch_dims(C, W, H, S, O)) return rc;
  RAMP_REQUIRE(x && out, "stitch: null array");
  const int st = H - (W > 1 ? O : 0);
  const long n = (long)C * (H + (long)(W - 1) * st) * S;
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, C, W, H, S, O);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
