// Helpers shared by the three host translation units behind the C ABI -- engine.hip (context, weight packing, the network schedule, sampler
// loops, graph capture), ops.hip (the context-free kernel-level entry points ramp_apf ... ramp_op_*) and bench.hip (the micro-benchmark /
// stress harness, linked into the tools library only) -- as internal-linkage definitions: small device kernels, the device arena, the
// fp16x3 weight scale of a device weight, the check of a scene batch, the weight packing of the fused feed-forward on raw fp32 weights.
#pragma once
#include "common.h"
#include "weight_scale.h"
#include "../../include/ramp_hip.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>


#define CK(expr) do { int _r = (expr); if (_r != 0) return _r; } while (0)

namespace ramp {

// The body of ramp_op_gemm_mode for modes 0 fp32, 1 bf16x6, 2 bf16x6 (LDS-staged weights), 3 fp16x3 (ops.hip), shared with the
// tools library's ramp_probe_gemm (bench.hip): packs a.W (raw fp32 [taps][N][K]) for `mode` as ramp_finalize_weights does,
// launches `a`, synchronises `s` and reports the recorded max |A| and the range flag (zeros outside fp16x3).  Hidden: the
// product library exports no new symbol for it.
__attribute__((visibility("hidden"))) int op_gemm_packed(GemmArgs a, int mode, float a_absmax_prev, float* a_absmax_out_host,
                                                         int32_t* range_flag_out_host, hipStream_t s);

// Block `module`'s (a ResidualTemporalBlock's name, as in ramp_debug_read) cout floats of line t of a context's prepared time table
// (engine.hip), for the tools library's ramp_probe_time_bias (bench.hip); an unknown name or a t outside the table is refused.  Hidden.
__attribute__((visibility("hidden"))) int ctx_time_line(ramp_ctx* c, const char* module, int t, const float** line, int* cout);

namespace {

inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
__global__ void permute3_kernel(const float* __restrict__ in, float* __restrict__ out, int D0, int D1, int D2,
                                int p0, int p1, int p2) {
  // out[i_p0][i_p1][i_p2] = in[i0][i1][i2]
  const long n = (long)D0 * D1 * D2;
  const int dims[3] = {D0, D1, D2};
  const int O1 = dims[p1], O2 = dims[p2];
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    int i[3];
    i[2] = (int)(idx % D2); i[1] = (int)((idx / D2) % D1); i[0] = (int)(idx / ((long)D1 * D2));
    out[((long)i[p0] * O1 + i[p1]) * O2 + i[p2]] = in[idx];
  }
}
// (a kernel node rather than a memset node: in the T = 50 jobs (config 5) the memset nodes of the captured graph were
//  replayed with a stale fill pattern -- 0x1c1c1c1c instead of 0 -- on ROCm 7.2; eager runs and T = 25 graphs were fine)
__global__ void log_flag_kernel(const int* __restrict__ flag, int* __restrict__ log, int j) { if (threadIdx.x == 0) log[j] = *flag; }
__global__ void zero_words_kernel(unsigned* __restrict__ p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0u;
}
// rows of ff.net.0.proj (2F, K) -> tiles of [G a-rows | G matching g-rows] (EPI_GEGLU_FWD; G = 64 for the block-level LDS
// epilogue, 32 for the wave-private epilogue of the pipelined kernels); K = 1 for the bias
__global__ void geglu_pack_kernel(const float* __restrict__ in, float* __restrict__ out, int F, int K, int G) {
  const long n = (long)2 * F * K;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int p = (int)(idx / K), k = (int)(idx - (long)p * K);
    const int t = p / (2 * G), c = p - t * 2 * G;
    const int src = c < G ? G * t + c : F + G * t + (c - G);
    out[idx] = in[(long)src * K + k];
  }
}
__global__ void fill_pattern_kernel(int* out, const int* pat, int n_pat, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = pat[i % n_pat];
}

struct DevArena {
  std::vector<void*> blocks;
  size_t total = 0;
  ~DevArena() { for (void* p : blocks) (void)hipFree(p); }
  float* alloc(size_t n_floats) {
    void* p = nullptr;
    size_t bytes = std::max<size_t>(n_floats, 4) * sizeof(float);
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    blocks.push_back(p);
    total += bytes;
    return static_cast<float*>(p);
  }
};

// the static fp16x3 scale (fp16_weight_scale, weight_scale.h) of a device weight of n floats: one download and a host max |w|
int device_weight_scale(const float* w_dev, size_t n, float* scale) {
  std::vector<float> hw(n);
  RAMP_HIP_CHECK(hipMemcpy(hw.data(), w_dev, n * sizeof(float), hipMemcpyDeviceToHost));
  float mx = 0.f;
  for (float v : hw) mx = std::max(mx, std::fabs(v));
  *scale = fp16_weight_scale(mx);
  return 0;
}

// what ramp_sample_scenes and ramp_apf_scenes (`who`) require of a scene batch: at least one scene and the trajectory -> scene table;
// where the per-scene clouds are used (need_cloud), the points and host offsets that start at 0 and give every scene a point
int check_scene_batch(const ramp_scene_batch* sc, bool need_cloud, const char* who) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(sc && sc->n_scenes >= 1 && sc->traj_scene, w + "bad scene batch (at least one scene, a trajectory -> scene table)");
  if (!need_cloud) return 0;
  RAMP_REQUIRE(sc->cloud_points && sc->cloud_offset_host && sc->cloud_offset_host[0] == 0, w + "bad scene batch (cloud points, offsets from 0)");
  for (int i = 0; i < sc->n_scenes; ++i)
    RAMP_REQUIRE(sc->cloud_offset_host[i + 1] > sc->cloud_offset_host[i], w + "every scene needs at least one cloud point (increasing offsets)");
  return 0;
}

// what ramp_sample_guided, ramp_guide_step and ramp_guide_cost (`who`) require of a cost guide on S-wide states, n_guide / step aside: host
// checks only, made before anything is staged or launched
int check_cost_guide(const ramp_cost_guide* cg, int S, const char* who) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(cg, w + "null cost guide");
  RAMP_REQUIRE((cg->point_dim == 2 || cg->point_dim == 3) && cg->point_dim <= S, w + "point_dim must be 2 or 3 and at most state_dim");
  RAMP_REQUIRE(std::isfinite(cg->radius) && std::isfinite(cg->w_obs) && std::isfinite(cg->w_smooth) && std::isfinite(cg->w_acc) &&
               std::isfinite(cg->max_norm), w + "radius, w_obs, w_smooth, w_acc and max_norm must be finite");
  RAMP_REQUIRE(cg->w_obs == 0.0 || cg->radius > 0.0, w + "radius must be positive where w_obs != 0");
  RAMP_REQUIRE(cg->n_scenes >= 1 && cg->cloud_offset_host && cg->cloud_offset_host[0] == 0, w + "bad cloud table (at least one scene, offsets from 0)");
  for (int i = 0; i < cg->n_scenes; ++i)
    RAMP_REQUIRE(cg->cloud_offset_host[i + 1] >= cg->cloud_offset_host[i], w + "cloud offsets must be non-decreasing");
  RAMP_REQUIRE(cg->cloud_offset_host[cg->n_scenes] == 0 || cg->cloud_points, w + "null cloud_points with a non-empty table");
  return 0;
}
// the kernel's arguments from a checked guide; the table pointers (cloud, cloud_off, scene) and the hard conditions are the caller's to fill
GuideArgs guide_args(const ramp_cost_guide* cg, float* traj, int B, int H, int S) {
  GuideArgs a; a.traj = traj; a.B = B; a.H = H; a.S = S; a.D = cg->point_dim; a.n_scenes = cg->n_scenes;
  a.P_total = cg->cloud_offset_host[cg->n_scenes];
  a.radius = (float)cg->radius; a.w_obs = (float)cg->w_obs; a.w_smooth = (float)cg->w_smooth; a.w_acc = (float)cg->w_acc;
  a.max_norm = (float)cg->max_norm;
  return a;
}

// what ramp_sample_guided_prims, ramp_guide_step_prims and ramp_guide_cost_prims (`who`) require of a primitive table next to the checked cost
// guide cg, on (H, S) trajectories: host checks only, made before anything is staged or launched
int check_prim_guide(const ramp_prim_guide* pg, const ramp_cost_guide* cg, int H, int S, const char* who) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(pg && cg, w + "null primitive table or cost guide");
  RAMP_REQUIRE((pg->point_dim == 2 || pg->point_dim == 3) && pg->point_dim <= S, w + "the primitives' point_dim must be 2 or 3 and at most state_dim");
  RAMP_REQUIRE(pg->point_dim == cg->point_dim, w + "the primitives' point_dim differs from the cost guide's");
  RAMP_REQUIRE(pg->n_sub >= 1 && pg->n_sub <= RAMP_PRIM_GUIDE_MAX_SUB, w + "n_sub outside 1 .. RAMP_PRIM_GUIDE_MAX_SUB");
  RAMP_REQUIRE(H <= GUIDE_MAX_H, w + "the primitive guide kernel serves horizons up to 128");
  RAMP_REQUIRE(std::isfinite(pg->margin) && pg->margin >= 0.0 && std::isfinite(pg->band) && pg->band >= 0.0,
               w + "margin and band must be finite and not negative");
  RAMP_REQUIRE(std::isfinite(pg->w_prim), w + "w_prim must be finite");
  RAMP_REQUIRE(pg->n_scenes >= 1 && pg->n_scenes == cg->n_scenes, w + "the primitives' n_scenes differs from the cost guide's");
  RAMP_REQUIRE(pg->box_offset_host && pg->sphere_offset_host && pg->box_offset_host[0] == 0 && pg->sphere_offset_host[0] == 0,
               w + "bad primitive offsets (both tables, from 0)");
  for (int i = 0; i < pg->n_scenes; ++i)
    RAMP_REQUIRE(pg->box_offset_host[i + 1] >= pg->box_offset_host[i] && pg->sphere_offset_host[i + 1] >= pg->sphere_offset_host[i],
                 w + "primitive offsets must be non-decreasing");
  RAMP_REQUIRE(pg->box_offset_host[pg->n_scenes] == 0 || (pg->box_centers && pg->box_sizes), w + "null box_centers / box_sizes with a non-empty table");
  RAMP_REQUIRE(pg->sphere_offset_host[pg->n_scenes] == 0 || (pg->sphere_centers && pg->sphere_radii),
               w + "null sphere_centers / sphere_radii with a non-empty table");
  return 0;
}
// true: the table changes the guide (a primitive somewhere and w_prim != 0); otherwise the call is the cost guide's own
bool prim_guide_active(const ramp_prim_guide* pg) {
  return pg && pg->w_prim != 0.0 && (float)pg->w_prim != 0.f && (pg->box_offset_host[pg->n_scenes] > 0 || pg->sphere_offset_host[pg->n_scenes] > 0);
}
// the kernel's arguments from a checked table; the array and offset pointers are the caller's to fill
PrimGuideArgs prim_guide_args(const ramp_prim_guide* pg, const GuideArgs& g) {
  PrimGuideArgs a; a.g = g;
  a.n_boxes = pg->box_offset_host[pg->n_scenes]; a.n_spheres = pg->sphere_offset_host[pg->n_scenes];
  a.margin = (float)pg->margin; a.band = (float)pg->band; a.w_prim = (float)pg->w_prim; a.n_sub = pg->n_sub;
  return a;
}

// what ramp_sample_guided_team, ramp_guide_step_team and ramp_guide_cost_team (`who`) require of a team table next to the checked cost guide, on
// B rows of H waypoints: host checks only, made before anything is staged or launched
int check_team_guide(const ramp_team_guide* tg, int B, int H, const char* who) {
  static_assert(TEAM_MAX == RAMP_TEAM_MAX, "one team limit");
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(tg, w + "null team table");
  RAMP_REQUIRE(tg->team_size >= 1 && tg->team_size <= RAMP_TEAM_MAX, w + "team_size outside 1 .. RAMP_TEAM_MAX");
  RAMP_REQUIRE(B > 0 && B % tg->team_size == 0, w + "the batch must be a multiple of team_size");
  RAMP_REQUIRE(std::isfinite(tg->w_team), w + "w_team must be finite");
  RAMP_REQUIRE(tg->w_team == 0.0 || (std::isfinite(tg->radius_team) && tg->radius_team > 0.0), w + "radius_team must be positive and finite where w_team != 0");
  RAMP_REQUIRE(H <= GUIDE_MAX_H, w + "the team guide kernel serves horizons up to 128");
  return 0;
}
// true: the table changes the guide (more than one agent and w_team != 0); otherwise the call is the cost guide's own
bool team_guide_active(const ramp_team_guide* tg) { return tg && tg->team_size > 1 && tg->w_team != 0.0 && (float)tg->w_team != 0.f; }
// the kernel's arguments from a checked table (tg may be null: no team term) around the filled guide arguments
TeamGuideArgs team_guide_args(const ramp_team_guide* tg, const GuideArgs& g) {
  TeamGuideArgs a; a.g = g;
  if (tg) { a.team = tg->team_size; a.radius_team = (float)tg->radius_team; a.w_team = (float)tg->w_team; }
  return a;
}

// what ramp_sample_stitched and ramp_stitch_windows (`who`) require of a stitch table on B rows of H waypoints: host checks only, made before
// anything is staged or launched
int check_stitch(const ramp_stitch* st, int B, int H, const char* who) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(st, w + "null stitch table");
  const int W = st->n_windows, O = st->overlap;
  RAMP_REQUIRE(W >= 1, w + "n_windows must be at least 1");
  RAMP_REQUIRE(B > 0 && B % W == 0, w + "the batch must be a multiple of n_windows (B = C * W rows)");
  if (W > 1) {
    RAMP_REQUIRE(O >= 1 && 2 * O <= H, w + "overlap outside 1 .. H / 2");
    RAMP_REQUIRE(st->alpha_host, w + "null alpha table");
    for (int k = 0; k < O; ++k)
      RAMP_REQUIRE(std::isfinite(st->alpha_host[k]) && st->alpha_host[k] >= 0.f && st->alpha_host[k] <= 1.f, w + "alpha must be finite and lie in [0, 1]");
  }
  RAMP_REQUIRE(st->n_pin >= 0 && st->n_pin <= RAMP_STITCH_MAX_PINS, w + "n_pin outside 0 .. RAMP_STITCH_MAX_PINS");
  RAMP_REQUIRE(st->n_pin == 0 || (st->pin_idx_host && st->pin_val), w + "null pin table");
  const int L = H + (W - 1) * (H - (W > 1 ? O : 0));
  for (int i = 0; i < st->n_pin; ++i) RAMP_REQUIRE(st->pin_idx_host[i] >= 0 && st->pin_idx_host[i] < L, w + "pin index outside [0, L)");
  return 0;
}
// the kernel's arguments from a checked table; x, alpha and pin_val are the caller's to fill
StitchArgs stitch_args(const ramp_stitch* st, int B, int H, int S) {
  static_assert(STITCH_MAX_PINS == RAMP_STITCH_MAX_PINS, "one pin limit");
  StitchArgs a; a.W = st->n_windows; a.C = B / a.W; a.H = H; a.S = S; a.O = a.W > 1 ? st->overlap : 0; a.n_pin = st->n_pin;
  for (int i = 0; i < st->n_pin; ++i) a.pin_idx[i] = st->pin_idx_host[i];
  return a;
}

// what the guided replans, ramp_guide_step_moving and ramp_guide_cost_moving (`who`) require of a replan guide on (H, S) rows: host checks
// only, made before anything is staged or launched.  n_scenes > 0: the scene count the job asks for; n_steps > 0: a job, whose n_guide /
// step tables are checked too and whose guide iterations are counted into *total
int check_replan_guide(const ramp_replan_guide* rg, int n_scenes, int H, int S, int n_steps, const char* who, int* total = nullptr) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(rg, w + "null replan guide");
  RAMP_REQUIRE(H <= GUIDE_MAX_H, w + "the guide kernel serves horizons up to 128");
  RAMP_REQUIRE(S >= 2, w + "state_dim must be at least 2");
  RAMP_REQUIRE(rg->n_mov >= 0 && rg->n_mov <= GUIDE_TILE, w + "n_mov outside 0 .. 1024");
  RAMP_REQUIRE(rg->n_scenes >= 1 && (n_scenes <= 0 || rg->n_scenes == n_scenes), w + "the guide's n_scenes must be 1 for one episode and the episode count for many");
  RAMP_REQUIRE(std::isfinite(rg->radius) && std::isfinite(rg->radius_mov) && std::isfinite(rg->w_obs) && std::isfinite(rg->w_mov) &&
               std::isfinite(rg->w_smooth) && std::isfinite(rg->w_acc) && std::isfinite(rg->max_norm),
               w + "radius, radius_mov, w_obs, w_mov, w_smooth, w_acc and max_norm must be finite");
  RAMP_REQUIRE(rg->w_obs == 0.0 || rg->radius > 0.0, w + "radius must be positive where w_obs != 0");
  RAMP_REQUIRE(rg->w_mov == 0.0 || rg->n_mov == 0 || rg->radius_mov > 0.0, w + "radius_mov must be positive where w_mov != 0 and n_mov > 0");
  RAMP_REQUIRE(rg->cloud_offset_host && rg->cloud_offset_host[0] == 0, w + "bad cloud table (offsets from 0)");
  for (int i = 0; i < rg->n_scenes; ++i)
    RAMP_REQUIRE(rg->cloud_offset_host[i + 1] >= rg->cloud_offset_host[i], w + "cloud offsets must be non-decreasing");
  RAMP_REQUIRE(rg->cloud_offset_host[rg->n_scenes] == 0 || rg->cloud_points, w + "null cloud_points with a non-empty table");
  RAMP_REQUIRE(rg->n_mov == 0 || (rg->mov_points_host && rg->mov_track_host), w + "null moving points or track with n_mov > 0");
  if (n_steps > 0) {
    RAMP_REQUIRE(rg->n_guide && rg->step, w + "missing n_guide / step arrays");
    int sum = 0;
    for (int j = 0; j < n_steps; ++j) {
      RAMP_REQUIRE(rg->n_guide[j] >= 0 && rg->n_guide[j] <= RAMP_GUIDE_MAX_STEPS, w + "n_guide outside 0 .. RAMP_GUIDE_MAX_STEPS");
      RAMP_REQUIRE(std::isfinite(rg->step[j]), w + "step sizes must be finite");
      sum += rg->n_guide[j];
    }
    if (total) *total = sum;
  }
  return 0;
}
// the kernel's arguments from a checked replan guide; the table pointers (clouds, offsets, moving points, track, scene), the pins and the
// hard conditions are the caller's to fill
MovingGuideArgs moving_guide_args(const ramp_replan_guide* rg, float* traj, int B, int H, int S) {
  MovingGuideArgs a; a.traj = traj; a.B = B; a.H = H; a.S = S; a.n_scenes = rg->n_scenes; a.n_mov = rg->n_mov;
  a.P_total = rg->cloud_offset_host[rg->n_scenes];
  a.radius = (float)rg->radius; a.radius_mov = (float)rg->radius_mov; a.w_obs = (float)rg->w_obs; a.w_mov = (float)rg->w_mov;
  a.w_smooth = (float)rg->w_smooth; a.w_acc = (float)rg->w_acc; a.max_norm = (float)rg->max_norm;
  return a;
}

}  // namespace
}  // namespace ramp

using namespace ramp;

// ---- the token-owning fused feed-forward (ffx.hip) on raw fp32 weights: packs as ramp_finalize_weights does, with its scale function ---
namespace {
struct FfxPack {
  unsigned short *stream_f = nullptr, *stream_b = nullptr;   // 96 x 32 KB each
  float *b1_pk = nullptr; float wsi_w1 = 1.f, wsi_w2 = 1.f;
};
// W1 [2048][256] (rows: 1024 a then 1024 g), W2 [256][1024]; everything allocated from `ar`
int ffx_pack_all(DevArena& ar, const float* W1, const float* b1, const float* W2, FfxPack* out, hipStream_t s, bool s16 = false) {
  float sc1 = 1.f, sc2 = 1.f;
  CK(device_weight_scale(W1, 2048 * 256, &sc1)); CK(device_weight_scale(W2, 256 * 1024, &sc2));
  float* w1_pk = ar.alloc(2048 * 256); out->b1_pk = ar.alloc(2048);
  float* w1t = ar.alloc(2048 * 256); float* w2t = ar.alloc(1024 * 256); float* tmp = ar.alloc(2048 * 256);
  auto planes = [&](size_t n) { return reinterpret_cast<unsigned short*>(ar.alloc(n + 4)); };   // 2 n halves
  unsigned short *p_w1 = planes(2048 * 256), *p_w2p = planes(256 * 1024), *p_w2t = planes(1024 * 256), *p_w1tp = planes(256 * 2048);
  out->stream_f = planes(96 * 8192); out->stream_b = planes(96 * 8192);
  RAMP_REQUIRE(w1_pk && out->b1_pk && w1t && w2t && tmp && p_w1 && p_w2p && p_w2t && p_w1tp && out->stream_f && out->stream_b, "hipMalloc failed");
  hipLaunchKernelGGL(geglu_pack_kernel, dim3(1024), dim3(256), 0, s, W1, w1_pk, 1024, 256, 32);
  hipLaunchKernelGGL(geglu_pack_kernel, dim3(8), dim3(256), 0, s, b1, out->b1_pk, 1024, 1, 32);
  hipLaunchKernelGGL(permute3_kernel, dim3(2048), dim3(256), 0, s, W1, w1t, 2048, 256, 1, 1, 0, 2);      // [256][2048]
  hipLaunchKernelGGL(permute3_kernel, dim3(1024), dim3(256), 0, s, W2, w2t, 256, 1024, 1, 1, 0, 2);      // [1024][256]
  RAMP_HIP_CHECK(hipGetLastError());
  if (s16) {      // 16 x 32 fragments for the v_mfma_f32_16x16x32_f16 kernels (ffx16.hip)
    CK(ffx16_pack(w1_pk, 2048, 256, 0, sc1, tmp, p_w1, s));
    CK(ffx16_pack(W2, 256, 1024, 1, sc2, tmp, p_w2p, s));
    CK(ffx16_pack(w2t, 1024, 256, 0, sc2, tmp, p_w2t, s));
    CK(ffx16_pack(w1t, 256, 2048, 2, sc1, tmp, p_w1tp, s));
    CK(ffx16_build_stream(p_w1, p_w2p, out->stream_f, false, s));
    CK(ffx16_build_stream(p_w2t, p_w1tp, out->stream_b, true, s));
  } else {
    CK(launch_pack_h3(w1_pk, p_w1, 2048, 256, sc1, s));
    CK(ffx_pack_second(W2, 256, 1024, 0, sc2, tmp, p_w2p, s));
    CK(launch_pack_h3(w2t, p_w2t, 1024, 256, sc2, s));
    CK(ffx_pack_second(w1t, 256, 2048, 1, sc1, tmp, p_w1tp, s));
    CK(ffx_build_stream(p_w1, p_w2p, out->stream_f, false, s));
    CK(ffx_build_stream(p_w2t, p_w1tp, out->stream_b, true, s));
  }
  out->wsi_w1 = 1.f / sc1; out->wsi_w2 = 1.f / sc2;
  return 0;
}
}  // namespace

