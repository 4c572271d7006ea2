// Solution-quality metrics of a batch of sampled trajectories, on the device
// (scripts/inference/core/metrics.py:8-81 of the reference): AABB collision intensity, path length, velocity
// smoothness per trajectory, and the waypoint variance (variance of ALL B x B entries of the strictly-upper-
// triangular pairwise distance matrix, per waypoint, summed over waypoints).
#include "args_sampler.h"

#include <algorithm>

namespace ramp {

// one wave per trajectory; lane = waypoint (strided when H > 64).  The arithmetic of one row, shared by the one-scene and
// the many-scene kernel so that both give the same bits for the same row and boxes.
__device__ __forceinline__ void traj_metrics_row(const float* __restrict__ t, int H, int S, const float* __restrict__ centers,
                                                 const float* __restrict__ sizes, int n_boxes, float* __restrict__ intensity,
                                                 float* __restrict__ path_len, float* __restrict__ smooth) {
  const int lane = threadIdx.x;
  float hits = 0.f, len = 0.f, sm = 0.f;
  for (int h = lane; h < H; h += 64) {
    const float x = t[h * S], y = t[h * S + 1];
    bool in = false;
    for (int k = 0; k < n_boxes; ++k) {
      // metrics.py:68-75: lower = c - s / 2, upper = c + s / 2, inclusive on both sides
      const float cx = centers[2 * k], cy = centers[2 * k + 1], hx = sizes[2 * k] / 2.f, hy = sizes[2 * k + 1] / 2.f;
      in |= (x >= cx - hx) && (x <= cx + hx) && (y >= cy - hy) && (y <= cy + hy);
    }
    hits += in ? 1.f : 0.f;
    if (h + 1 < H) {
      const float dx = t[(h + 1) * S] - x, dy = t[(h + 1) * S + 1] - y;
      len += sqrtf(dx * dx + dy * dy);
      float acc = 0.f;
      for (int d = 2; d < S; ++d) { const float dv = t[(h + 1) * S + d] - t[h * S + d]; acc += dv * dv; }
      sm += sqrtf(acc);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    hits += __shfl_xor(hits, o); len += __shfl_xor(len, o); sm += __shfl_xor(sm, o);
  }
  if (lane == 0) { *intensity = hits / (float)H; *path_len = len; *smooth = sm; }
}
__global__ __launch_bounds__(64)
void traj_metrics_kernel(const float* __restrict__ traj, int B, int H, int S, const float* __restrict__ centers,
                         const float* __restrict__ sizes, int n_boxes, float* __restrict__ intensity,
                         float* __restrict__ path_len, float* __restrict__ smooth) {
  const int b = blockIdx.x;
  traj_metrics_row(traj + (long)b * H * S, H, S, centers, sizes, n_boxes, intensity + b, path_len + b, smooth + b);
}
// the scene of row b: the s in [0, n) with first[s] <= b < first[s + 1] (first is increasing, first[0] = 0, first[n] = B)
__device__ __forceinline__ int scene_of_row(const int* __restrict__ first, int n, int b) {
  int lo = 0, hi = n - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (first[mid] <= b) lo = mid; else hi = mid - 1; }
  return lo;
}
// traj_metrics_kernel for a batch of many scenes: row b tests the boxes [box_off[s], box_off[s + 1]) of its own scene only.
// Spans are clamped to [0, n_boxes_total], so a wrong table reads wrong boxes, never outside the arrays.
__global__ __launch_bounds__(64)
void traj_metrics_scenes_kernel(const float* __restrict__ traj, int H, int S, const int* __restrict__ traj_first, int n_scenes,
                                const float* __restrict__ centers, const float* __restrict__ sizes, const int* __restrict__ box_off,
                                int n_boxes_total, float* __restrict__ intensity, float* __restrict__ path_len,
                                float* __restrict__ smooth) {
  const int b = blockIdx.x, s = scene_of_row(traj_first, n_scenes, b);
  const int k0 = min(max(box_off[s], 0), n_boxes_total), k1 = min(max(box_off[s + 1], k0), n_boxes_total);
  traj_metrics_row(traj + (long)b * H * S, H, S, centers + 2 * k0, sizes + 2 * k0, k1 - k0, intensity + b, path_len + b, smooth + b);
}

// partial sums over pairs (i in this block's 256 rows, all j > i) of d_ij and d_ij^2 at waypoint blockIdx.y
__global__ __launch_bounds__(256)
void waypoint_pairs_kernel(const float* __restrict__ traj, int B, int H, int S, double* __restrict__ partial) {
  __shared__ float2 tile[256];
  __shared__ double red[2][4];
  const int h = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  float2 pi = {0.f, 0.f};
  if (i < B) pi = {traj[((long)i * H + h) * S], traj[((long)i * H + h) * S + 1]};
  double s1 = 0.0, s2 = 0.0;
  for (int j0 = blockIdx.x * 256; j0 < B; j0 += 256) {     // tiles left of the diagonal hold no pair with j > i
    const int j = j0 + threadIdx.x;
    __syncthreads();
    tile[threadIdx.x] = j < B ? float2{traj[((long)j * H + h) * S], traj[((long)j * H + h) * S + 1]} : float2{0.f, 0.f};
    __syncthreads();
    const int n = min(256, B - j0);
    float a1 = 0.f, a2 = 0.f;                                // a tile's worth in fp32, tiles in fp64
    for (int jj = 0; jj < n; ++jj) {
      const float dx = pi.x - tile[jj].x, dy = pi.y - tile[jj].y;
      const float d2 = dx * dx + dy * dy;
      const bool use = (j0 + jj > i) && (i < B);
      a1 += use ? sqrtf(d2) : 0.f;
      a2 += use ? d2 : 0.f;
    }
    s1 += a1; s2 += a2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((long)h * gridDim.x + blockIdx.x) * 2;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}
// var over the N = B*B entries (the B(B+1)/2 zeros of the lower triangle and diagonal included, unbiased), summed over h
__global__ void waypoint_var_kernel(const double* __restrict__ partial, int nblk, int H, int B, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double N = (double)B * (double)B;
  double total = 0.0;
  for (int h = 0; h < H; ++h) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nblk; ++k) { s1 += partial[((long)h * nblk + k) * 2]; s2 += partial[((long)h * nblk + k) * 2 + 1]; }
    total += (s2 - s1 * s1 / N) / (N - 1.0);
  }
  out[0] = total;
}

int launch_traj_metrics(const float* traj, int B, int H, int S, const float* centers, const float* sizes, int n_boxes,
                        float* intensity, float* path_len, float* smooth, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 1 && S >= 2 && n_boxes >= 0, "bad metric dims");
  hipLaunchKernelGGL(traj_metrics_kernel, dim3(B), dim3(64), 0, s, traj, B, H, S, centers, sizes, n_boxes, intensity, path_len, smooth);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_waypoint_variance(const float* traj, int B, int H, int S, double* scratch, double* out, hipStream_t s) {
  RAMP_REQUIRE(B > 1 && H > 0 && S >= 2, "bad metric dims");
  const int nblk = (B + 255) / 256;
  hipLaunchKernelGGL(waypoint_pairs_kernel, dim3(nblk, H), dim3(256), 0, s, traj, B, H, S, scratch);
  hipLaunchKernelGGL(waypoint_var_kernel, dim3(1), dim3(64), 0, s, scratch, nblk, H, B, out);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- denoising loss: stage 1 -- block k owns the contiguous elements [k per, (k + 1) per), pins the endpoints of x_recon in place and
// sums its fp32 terms in fp64 (thread-strided, then a fixed shuffle / LDS tree); stage 2 -- one thread adds the block sums in order.
// Nothing depends on the launch's timing: the same inputs give the same bits.
__global__ __launch_bounds__(256)
void denoise_loss_kernel(float* __restrict__ x_recon, const float* __restrict__ x_start, const float* __restrict__ target, long n, long per,
                         int H, int S, int l1, double* __restrict__ partial) {
  __shared__ double red[4];
  const long lo = (long)blockIdx.x * per, hi = min(lo + per, n);
  double acc = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) {
    const int h = (int)((i / S) % H);
    float r = x_recon[i];
    if (h == 0 || h == H - 1) { r = x_start[i]; x_recon[i] = r; }
    const float d = r - target[i];
    const float term = l1 ? fabsf(d) : d * d;
    acc += (double)term;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void denoise_loss_finish_kernel(const double* __restrict__ partial, int nblk, long n, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double total = 0.0;
  for (int k = 0; k < nblk; ++k) total += partial[k];
  out[0] = total / (double)n;
}
int launch_denoise_loss(float* x_recon, const float* x_start, const float* target, int B, int H, int S, int l1, double* scratch, double* out,
                        hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 1 && S > 0, "bad loss dims");
  const long n = (long)B * H * S;
  const int nblk = (int)std::min<long>((n + 255) / 256, DENOISE_LOSS_BLOCKS);
  const long per = (n + nblk - 1) / nblk;
  hipLaunchKernelGGL(denoise_loss_kernel, dim3(nblk), dim3(256), 0, s, x_recon, x_start, target, n, per, H, S, l1, scratch);
  hipLaunchKernelGGL(denoise_loss_finish_kernel, dim3(1), dim3(64), 0, s, scratch, nblk, n, out);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

// ---- per-scene summary of a many-scene batch (what Metrics.trajectory_success_and_metrics reports, metrics.py:83-126, per
// scene): free = intensity <= threshold.  Every sum is laid out relative to the scene's first row, never to the batch, so a
// scene's record has the same bits alone and inside any batch.
//
// scratch (doubles): [0, 2 H W) the tile partials, W = ceil(B / 256) + n_scenes an upper bound of sum_s ceil(n_s / 256);
//                    then n_scenes + 1 int32 (in n_scenes + 1 double slots): tile_first[s] = sum_{k < s} ceil(n_k / 256)
constexpr int SUMMARY_TILE = 256;
__host__ __device__ inline long summary_tiles(int B, int n_scenes) { return (long)(B + SUMMARY_TILE - 1) / SUMMARY_TILE + n_scenes; }

// stage 0: tile_first by an in-block scan, 256 scenes at a time
__global__ __launch_bounds__(256)
void scene_tiles_kernel(const int* __restrict__ traj_first, int n_scenes, int* __restrict__ tile_first) {
  __shared__ int v[2][256];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; tile_first[0] = 0; }
  for (int s0 = 0; s0 < n_scenes; s0 += 256) {
    const int s = s0 + tid;
    const int n = s < n_scenes ? max(traj_first[s + 1] - traj_first[s], 0) : 0;
    int cur = 0;
    v[0][tid] = (n + SUMMARY_TILE - 1) / SUMMARY_TILE;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                     // Hillis-Steele inclusive scan
      v[cur ^ 1][tid] = v[cur][tid] + (tid >= o ? v[cur][tid - o] : 0);
      cur ^= 1;
      __syncthreads();
    }
    if (s < n_scenes) tile_first[s + 1] = carry + v[cur][tid];
    __syncthreads();
    if (tid == 255) carry += v[cur][255];
    __syncthreads();
  }
}
// stage 1: block (w, h) = rows [256 t, 256 t + 256) of scene s (w = tile_first[s] + t) at waypoint h: sums of d_ij and d_ij^2
// over the pairs i in the tile, j > i in the scene, both free -- waypoint_pairs_kernel with the free test in place of a
// compaction.  A j-tile in fp32, j-tiles in fp64, as there.
// D = 2 or 3 position coordinates; D = 2 is the code ramp_scene_summary has always run (no z value is loaded or used there)
template <int D>
__global__ __launch_bounds__(256)
void scene_pairs_kernel(const float* __restrict__ traj, int B, int H, int S, const int* __restrict__ traj_first, int n_scenes,
                        const int* __restrict__ tile_first, const float* __restrict__ intensity, float thr,
                        double* __restrict__ partial) {
  __shared__ float2 tile[256];
  __shared__ float tilez[D == 3 ? 256 : 1];
  __shared__ int tfree[256];
  __shared__ double red[2][4];
  const int w = blockIdx.x, h = blockIdx.y;
  if (w >= tile_first[n_scenes]) return;
  const int s = scene_of_row(tile_first, n_scenes, w);      // tile_first repeats no value: every scene has a row
  const int first = min(max(traj_first[s], 0), B), end = min(max(traj_first[s + 1], first), B);
  const int i0 = first + (w - tile_first[s]) * 256, i = i0 + threadIdx.x;
  float2 pi = {0.f, 0.f};
  float piz = 0.f;
  bool fi = false;
  if (i < end) { pi = {traj[((long)i * H + h) * S], traj[((long)i * H + h) * S + 1]}; fi = intensity[i] <= thr; }
  if (D == 3 && i < end) piz = traj[((long)i * H + h) * S + 2];
  double s1 = 0.0, s2 = 0.0;
  for (int j0 = i0; j0 < end; j0 += 256) {                  // tiles left of the diagonal hold no pair with j > i
    const int j = j0 + threadIdx.x;
    __syncthreads();
    tile[threadIdx.x] = j < end ? float2{traj[((long)j * H + h) * S], traj[((long)j * H + h) * S + 1]} : float2{0.f, 0.f};
    if (D == 3) tilez[threadIdx.x] = j < end ? traj[((long)j * H + h) * S + 2] : 0.f;
    tfree[threadIdx.x] = j < end && intensity[j] <= thr;
    __syncthreads();
    const int n = min(256, end - j0);
    float a1 = 0.f, a2 = 0.f;
    for (int jj = 0; jj < n; ++jj) {
      const float dx = pi.x - tile[jj].x, dy = pi.y - tile[jj].y;
      float d2 = dx * dx + dy * dy;
      if (D == 3) { const float dz = piz - tilez[jj]; d2 += dz * dz; }
      const bool use = (j0 + jj > i) && fi && tfree[jj];
      a1 += use ? sqrtf(d2) : 0.f;
      a2 += use ? d2 : 0.f;
    }
    s1 += a1; s2 += a2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s1; red[1][threadIdx.x >> 6] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial + ((long)w * H + h) * 2;
    o[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    o[1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}
// sum of one double per thread over the block's 256 threads, in a fixed order; every thread gets the result
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// stage 2: one block per scene: the record {n_traj, n_free, mean intensity, mean / unbiased std of the free path lengths,
// waypoint variance of the free rows} and the scene's part of the free mask
__global__ __launch_bounds__(256)
void scene_summary_kernel(int B, int H, int W, const int* __restrict__ traj_first, const int* __restrict__ tile_first,
                          const float* __restrict__ intensity, const float* __restrict__ path_len, float thr,
                          const double* __restrict__ partial, double* __restrict__ summary, int* __restrict__ free_mask) {
  __shared__ double red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int first = min(max(traj_first[s], 0), B), end = min(max(traj_first[s + 1], first), B);
  double ci = 0.0, pl = 0.0, cnt = 0.0;
  for (int b = first + tid; b < end; b += 256) {
    const bool f = intensity[b] <= thr;
    free_mask[b] = f;
    ci += (double)intensity[b];
    if (f) { pl += (double)path_len[b]; cnt += 1.0; }
  }
  ci = block_sum_256(ci, red); pl = block_sum_256(pl, red); cnt = block_sum_256(cnt, red);
  const double mean = pl / cnt;                             // NaN when no row is free
  double ss = 0.0;
  for (int b = first + tid; b < end; b += 256)
    if (intensity[b] <= thr) { const double d = (double)path_len[b] - mean; ss += d * d; }
  ss = block_sum_256(ss, red);
  if (tid != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double var = nan;
  if (cnt == 1.0) var = 0.0;
  if (cnt > 1.0) {
    // var over the N = n_free^2 entries (zeros of the lower triangle and diagonal included, unbiased), summed over h
    const double N = cnt * cnt;
    const int t0 = min(tile_first[s], W), t1 = min(tile_first[s + 1], W);
    var = 0.0;
    for (int h = 0; h < H; ++h) {
      double s1 = 0.0, s2 = 0.0;
      for (int k = t0; k < t1; ++k) { s1 += partial[((long)k * H + h) * 2]; s2 += partial[((long)k * H + h) * 2 + 1]; }
      var += (s2 - s1 * s1 / N) / (N - 1.0);
    }
  }
  double* o = summary + (long)s * 6;
  o[0] = (double)(end - first); o[1] = cnt; o[2] = ci / (double)(end - first);
  o[3] = cnt > 0.0 ? mean : nan; o[4] = cnt > 1.0 ? sqrt(ss / (cnt - 1.0)) : nan; o[5] = var;
}

int launch_traj_metrics_scenes(const float* traj, int B, int H, int S, const int* traj_first, int n_scenes, const float* centers,
                               const float* sizes, const int* box_off, int n_boxes_total, float* intensity, float* path_len,
                               float* smooth, hipStream_t s) {
  RAMP_REQUIRE(B > 0 && H > 1 && S >= 2 && n_scenes > 0 && n_scenes <= B && n_boxes_total >= 0, "bad metric dims");
  hipLaunchKernelGGL(traj_metrics_scenes_kernel, dim3(B), dim3(64), 0, s, traj, H, S, traj_first, n_scenes, centers, sizes, box_off,
                     n_boxes_total, intensity, path_len, smooth);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}
int launch_scene_summary(const float* traj, int B, int H, int S, const int* traj_first, int n_scenes, const float* intensity,
                         const float* path_len, float thr, double* scratch, double* summary, int* free_mask, hipStream_t s, int D) {
  RAMP_REQUIRE(B > 0 && H > 0 && H <= 65535 && S >= 2 && n_scenes > 0 && n_scenes <= B, "bad metric dims");
  RAMP_REQUIRE((D == 2 || D == 3) && D <= S, "point_dim must be 2 or 3 and at most S");
  const long W = summary_tiles(B, n_scenes);
  int* tile_first = reinterpret_cast<int*>(scratch + 2 * H * W);
  hipLaunchKernelGGL(scene_tiles_kernel, dim3(1), dim3(256), 0, s, traj_first, n_scenes, tile_first);
  if (D == 3) hipLaunchKernelGGL(scene_pairs_kernel<3>, dim3((unsigned)W, H), dim3(256), 0, s, traj, B, H, S, traj_first, n_scenes, tile_first,
                                 intensity, thr, scratch);
  else hipLaunchKernelGGL(scene_pairs_kernel<2>, dim3((unsigned)W, H), dim3(256), 0, s, traj, B, H, S, traj_first, n_scenes, tile_first,
                          intensity, thr, scratch);
  hipLaunchKernelGGL(scene_summary_kernel, dim3(n_scenes), dim3(256), 0, s, B, H, (int)W, traj_first, tile_first, intensity, path_len, thr,
                     scratch, summary, free_mask);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace ramp
