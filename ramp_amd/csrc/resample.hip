// Resampling trajectories by cost inside the sampling job (SMC steering; ramp_resample_params in ramp_hip.h): the weight update of an event,
// the per-group normalisation / ESS / systematic resampling, and the row gather.  Everything here is fp64 on B numbers plus one copy of the
// batch; plain C++ and vector stores, nothing handed between blocks inside a kernel (one block owns one group from its first read to its
// last write).  Built with -ffp-contract=off: the fp64 expressions are rounded as written.
#include "args_resample.h"
#include <algorithm>

namespace ramp {
namespace {

constexpr int RS_BLOCK = 256;      // 4 waves

__device__ __forceinline__ double rs_ninf() { return __longlong_as_double(0xfff0000000000000ll); }

// the block's sum / maximum, the same value in every thread: a fixed butterfly per wave, then the 4 wave results in a fixed order (red: 4 doubles
// of LDS, free again when the call returns)
__device__ __forceinline__ double rs_block_sum(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}
__device__ __forceinline__ double rs_block_max(double v, double* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(RS_BLOCK) void resample_weights_kernel(ResampleWeightArgs a) {
  const int b = blockIdx.x * RS_BLOCK + threadIdx.x;
  if (b >= a.B) return;
  const double* t = a.terms + (size_t)b * 3;
  const double c = (a.w_obs * t[0] + a.w_smooth * t[1]) + a.w_acc * t[2];
  double lw = a.logw[b] + (-a.lambda) * (c - a.c_prev[b]);
  if (!isfinite(lw)) lw = rs_ninf();
  a.logw[b] = lw;
  a.c_prev[b] = c;
  if (a.cost_out) a.cost_out[b] = c;
}

__global__ __launch_bounds__(RS_BLOCK) void resample_groups_kernel(ResampleGroupsArgs a) {
  __shared__ double red[4];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first = a.group_first[g], n = a.group_first[g + 1] - first;
  if (first < 0 || n <= 0 || n > a.B - first) return;      // (a table the host checks refuse: nothing is touched)
  double* lw = a.logw + first;
  int* anc = a.ancestor + first;
  // 1. the largest finite log-weight; a non-finite one is a weight of 0
  double m = rs_ninf();
  for (int i = tid; i < n; i += RS_BLOCK) { const double v = lw[i]; if (isfinite(v)) m = fmax(m, v); }
  m = rs_block_max(m, red);
  if (!(m > rs_ninf())) {      // every weight is 0: ESS 0, identity, nothing changes
    for (int i = tid; i < n; i += RS_BLOCK) anc[i] = first + i;
    if (tid == 0 && a.ess_out) a.ess_out[g] = 0.0;
    return;
  }
  // 2. the sum of exp(logw - max)
  double s = 0.0;
  for (int i = tid; i < n; i += RS_BLOCK) { const double v = lw[i]; s += isfinite(v) ? exp(v - m) : 0.0; }
  s = rs_block_sum(s, red);
  // 3. W, sum W^2 and the inclusive prefix sums, a chunk of RS_BLOCK elements at a time: a shuffle scan inside each wave, the waves' totals
  // through LDS, the running total carried in a register (the same value in every thread).  The carry is the chunk's last prefix sum itself
  double* cum = a.cum + first;
  double carry = 0.0, q = 0.0;
  for (int base = 0; base < n; base += RS_BLOCK) {
    const int i = base + tid;
    double W = 0.0;
    if (i < n) { const double v = lw[i]; W = isfinite(v) ? exp(v - m) / s : 0.0; }
    q += W * W;
    double x = W;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const double y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) red[wave] = x;
    __syncthreads();
    const double o1 = carry + red[0], o2 = o1 + red[1], o3 = o2 + red[2];
    const double off = wave == 0 ? carry : wave == 1 ? o1 : wave == 2 ? o2 : o3;
    if (i < n) cum[i] = i == n - 1 ? 1.0 : off + x;
    carry = o3 + red[3];
    __syncthreads();
  }
  q = rs_block_sum(q, red);
  const double ess = 1.0 / q;
  if (tid == 0 && a.ess_out) a.ess_out[g] = ess;
  // 4. the gate
  if (!(ess < a.ess_frac * (double)n)) {
    for (int i = tid; i < n; i += RS_BLOCK) anc[i] = first + i;
    return;
  }
  __syncthreads();      // (cum is complete and visible to the block)
  const double u = (double)a.u[g], dn = (double)n;
  for (int i = tid; i < n; i += RS_BLOCK) {
    const double thr = ((double)i + u) / dn;
    int lo = 0, hi = n;      // #{k : cum_k <= thr}
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[mid] <= thr) lo = mid + 1; else hi = mid; }
    anc[i] = first + min(lo, n - 1);
  }
  if (a.c_prev) {
    double* cp = a.c_prev + first; double* tmp = a.tmp + first;
    for (int i = tid; i < n; i += RS_BLOCK) tmp[i] = cp[i];
    __syncthreads();
    for (int i = tid; i < n; i += RS_BLOCK) cp[i] = tmp[anc[i] - first];      // (anc[i] is this thread's own write)
  }
  for (int i = tid; i < n; i += RS_BLOCK) lw[i] = 0.0;
}

__global__ __launch_bounds__(RS_BLOCK) void resample_gather_kernel(const float4* __restrict__ x, const int* __restrict__ anc, float4* __restrict__ tmp,
                                                                   int B, int V) {
  const long n = (long)B * V;
  for (long e = (long)blockIdx.x * RS_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * RS_BLOCK) {
    const int i = (int)(e / V), v = (int)(e - (long)i * V);
    int src = anc[i];
    if ((unsigned)src >= (unsigned)B) src = i;
    tmp[e] = x[(long)src * V + v];
  }
}

}  // namespace

int launch_resample_weights(const ResampleWeightArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.terms && a.logw && a.c_prev && a.B > 0, "resample weights: null operand");
  hipLaunchKernelGGL(resample_weights_kernel, dim3((a.B + RS_BLOCK - 1) / RS_BLOCK), dim3(RS_BLOCK), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_resample_groups(const ResampleGroupsArgs& a, hipStream_t s) {
  RAMP_REQUIRE(a.logw && a.group_first && a.u && a.cum && a.ancestor && a.B > 0 && a.n_groups > 0 && a.n_groups <= a.B, "resample groups: bad operands");
  RAMP_REQUIRE(!a.c_prev || a.tmp, "resample groups: c_prev needs the scratch array");
  RAMP_REQUIRE(resample_ess_frac_ok(a.ess_frac), "resample groups: ess_frac outside [0, 2]");
  hipLaunchKernelGGL(resample_groups_kernel, dim3(a.n_groups), dim3(RS_BLOCK), 0, s, a);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_resample_gather(const float* x, const int* ancestor, float* tmp, int B, int HS, hipStream_t s) {
  RAMP_REQUIRE(x && ancestor && tmp && B > 0 && HS > 0 && HS % 4 == 0, "resample gather: bad operands (H S must be a multiple of 4)");
  RAMP_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(tmp)) & 15) == 0, "resample gather: arrays must be 16-byte aligned");
  const long n = (long)B * (HS / 4);
  hipLaunchKernelGGL(resample_gather_kernel, dim3((unsigned)std::min<long>((n + RS_BLOCK - 1) / RS_BLOCK, 8192)), dim3(RS_BLOCK), 0, s,
                     reinterpret_cast<const float4*>(x), ancestor, reinterpret_cast<float4*>(tmp), B, HS / 4);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
