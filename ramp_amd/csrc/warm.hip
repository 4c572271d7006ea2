// Warm-started jobs (ramp_warm_start in include/ramp_hip.h; ramp_amd/warm.py is the definition): every row starts from its own prior,
// noised to its own level, and is held at that start state until the job's schedule reaches the level.
//
// warm_init_kernel  x[b] = (sa_row[b] * prior[b]) + (s1a_row[b] * noise0[b]) for a row with a prior, noise0[b]'s bits for one without
// warm_hold_kernel  rows with j0[b] > j: x[b] (and the chain block's row) = x_init[b]; every other row keeps its bytes
//
// Both are one row-contiguous pass of 16-byte accesses: element e of the (B, H S / 4) float4 view belongs to row e / (H S / 4), a wave's
// 64 lanes read 1 KiB in a line, and the per-row tables are one cached word per row.  The level is a per-row quantity, so the launch count
// never depends on B or on the number of scenes.
//
// Built with -ffp-contract=off like sampler.hip: the two products and the sum are rounded once each, as warm_init_reference writes them.
#include "args_sampler.h"

namespace ramp {

namespace {

constexpr int WARM_BLOCK = 256;

__global__ __launch_bounds__(WARM_BLOCK) void warm_init_kernel(float4* x, const float4* noise0, const float4* __restrict__ prior,
                                                               const float* __restrict__ sa_row, const float* __restrict__ s1a_row,
                                                               const int* __restrict__ has_prior, int B, int V) {
  const long n = (long)B * V;
  for (long e = (long)blockIdx.x * WARM_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * WARM_BLOCK) {
    const int b = (int)(e / V);
    float4 z = noise0[e];      // (noise0 may be x itself: every element is read and written by the same thread)
    if (has_prior[b]) {
      const float a = sa_row[b], c = s1a_row[b];
      const float4 p = prior[e];
      z.x = __fadd_rn(__fmul_rn(a, p.x), __fmul_rn(c, z.x));
      z.y = __fadd_rn(__fmul_rn(a, p.y), __fmul_rn(c, z.y));
      z.z = __fadd_rn(__fmul_rn(a, p.z), __fmul_rn(c, z.z));
      z.w = __fadd_rn(__fmul_rn(a, p.w), __fmul_rn(c, z.w));
    }
    x[e] = z;
  }
}

__global__ __launch_bounds__(WARM_BLOCK) void warm_hold_kernel(float4* __restrict__ x, float4* __restrict__ chain_block,
                                                               const float4* __restrict__ x_init, const int* __restrict__ j0, int j, int B, int V) {
  const long n = (long)B * V;
  for (long e = (long)blockIdx.x * WARM_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * WARM_BLOCK) {
    const int b = (int)(e / V);
    if (j0[b] <= j) continue;
    const float4 v = x_init[e];
    x[e] = v;
    if (chain_block) chain_block[e] = v;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

unsigned warm_grid(long n) { return (unsigned)std::min<long>((n + WARM_BLOCK - 1) / WARM_BLOCK, 8192); }

}  // namespace

int launch_warm_init(float* x, const float* noise0, const float* prior, const float* sa_row, const float* s1a_row, const int* has_prior,
                     int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(x && noise0 && prior && sa_row && s1a_row && has_prior, "warm init: null operand");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && ((long)H * S) % 4 == 0, "warm init: bad dims (H * S must be a multiple of 4)");
  RAMP_REQUIRE((long)B * H * S < (1l << 31), "warm init: batch too large");
  RAMP_REQUIRE(aligned16(x) && aligned16(noise0) && aligned16(prior), "warm init: arrays must be 16-byte aligned");
  const int V = H * S / 4;
  hipLaunchKernelGGL(warm_init_kernel, dim3(warm_grid((long)B * V)), dim3(WARM_BLOCK), 0, s, reinterpret_cast<float4*>(x),
                     reinterpret_cast<const float4*>(noise0), reinterpret_cast<const float4*>(prior), sa_row, s1a_row, has_prior, B, V);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_warm_hold(float* x, float* chain_block, const float* x_init, const int* j0, int j, int B, int H, int S, hipStream_t s) {
  RAMP_REQUIRE(x && x_init && j0, "warm hold: null operand");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && ((long)H * S) % 4 == 0, "warm hold: bad dims (H * S must be a multiple of 4)");
  RAMP_REQUIRE((long)B * H * S < (1l << 31), "warm hold: batch too large");
  RAMP_REQUIRE(aligned16(x) && aligned16(chain_block) && aligned16(x_init), "warm hold: arrays must be 16-byte aligned");
  const int V = H * S / 4;
  hipLaunchKernelGGL(warm_hold_kernel, dim3(warm_grid((long)B * V)), dim3(WARM_BLOCK), 0, s, reinterpret_cast<float4*>(x),
                     reinterpret_cast<float4*>(chain_block), reinterpret_cast<const float4*>(x_init), j0, j, B, V);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
