// The context-free kernel-level entry points of the C ABI (include/ramp_hip.h): ramp_apf ... ramp_ddim_finish (what the Python mirror of the
// reference's helper functions calls one kernel at a time) and the ramp_op_* unit entry points the parity tests drive every kernel family through
// (each packs its weights from raw fp32 with the scale function ramp_finalize_weights uses, device_weight_scale -> fp16_weight_scale, and
// the same pack routine).  Split from engine.hip in round 6: an edit of a kernel family's argument struct rebuilds this file and its own,
// not the sampler.
#include "engine_util.h"

#include <functional>

namespace {
// What every ramp_op_* entry point with a scaled operand does around its own pack call and argument struct.  Device memory lives as long
// as the call (a DevArena).  begin(), called behind the pack: the slots of `n` operand sites -- previous maxima [0, n), recorded maxima
// [n, 2n), range flag [2n] -- uploaded on the stream.  finish(): one synchronisation, the slots read back into the caller's outputs
// (zeros where begin() never ran); a failed call leaves the outputs untouched.
struct ScaledOp {
  hipStream_t s; const int n;
  DevArena ar;
  float* slots = nullptr;
  float host[12] = {0};
  ScaledOp(hipStream_t st, int n_sites = 1) : s(st), n(n_sites) {}
  size_t n_slots() const { return (size_t)(2 * n + 1 + 3) / 4 * 4; }
  unsigned short* planes(size_t n_floats) { return reinterpret_cast<unsigned short*>(ar.alloc(n_floats)); }     // 2 n_floats halves
  int begin(const float* absmax_prev) {      // n previous maxima (null: none given)
    slots = ar.alloc(n_slots());
    RAMP_REQUIRE(slots, "hipMalloc failed");
    for (int i = 0; i < n; ++i) host[i] = absmax_prev ? absmax_prev[i] : 0.f;
    RAMP_HIP_CHECK(hipMemcpyAsync(slots, host, n_slots() * sizeof(float), hipMemcpyHostToDevice, s));
    return 0;
  }
  const float* amax_in(int i = 0) const { return host[i] > 0.f ? slots + i : nullptr; }      // null: no maximum given, the operand runs unscaled
  float* amax_out(int i = 0) const { return slots + n + i; }
  int* range_flag() const { return reinterpret_cast<int*>(slots + 2 * n); }
  // the four fields every single-site argument struct has
  template <class Args> void attach(Args& a, float w_scale) const {
    a.amax_in = amax_in(); a.amax_out = amax_out(); a.wsi = 1.f / w_scale; a.range_flag = range_flag();
  }
  int finish(int rc, float* absmax_out_host, int32_t* range_flag_out_host) {
    hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e == hipSuccess) {
      if (slots) e = hipMemcpy(host, slots, n_slots() * sizeof(float), hipMemcpyDeviceToHost);
      if (absmax_out_host) for (int i = 0; i < n; ++i) absmax_out_host[i] = host[n + i];
      if (range_flag_out_host) std::memcpy(range_flag_out_host, &host[2 * n], 4);
    }
    RAMP_HIP_CHECK(e);
    return rc;
  }
};
}  // namespace

namespace ramp {
int op_gemm_packed(GemmArgs a, int mode, float a_absmax_prev, float* a_absmax_out_host, int32_t* range_flag_out_host, hipStream_t s) {
  RAMP_REQUIRE(mode >= 0 && mode <= 3, "mode: 0 fp32, 1 bf16x6, 2 bf16x6 (LDS-staged weights), 3 fp16x3");
  const int N = a.N, K = a.K;
  const size_t n = (size_t)a.taps * N * K;
  const bool frag_ok = N >= 64 && N % 32 == 0 && K % 16 == 0;
  ScaledOp h(s);
  if (mode == 3 && frag_ok) {
    float sc = 1.f; CK(device_weight_scale(a.W, n, &sc));
    unsigned short* planes = h.planes(n + 4);
    RAMP_REQUIRE(planes, "hipMalloc failed");
    CK(launch_pack_h3(a.W, planes, (long)a.taps * N, K, sc, s));
    CK(h.begin(&a_absmax_prev));
    a.Wx = planes; a.wx_packed = 2; a.w_scale_inv = 1.f / sc;
    a.a_absmax_in = h.amax_in(); a.a_absmax_out = h.amax_out(); a.range_flag = h.range_flag();
  } else if (mode == 1 && frag_ok) {
    unsigned short* planes = h.planes((3 * n + 1) / 2 + 4);
    RAMP_REQUIRE(planes, "hipMalloc failed");
    CK(launch_pack_x6(a.W, planes, (long)a.taps * N, K, s));
    a.Wx = planes; a.wx_packed = 1;
  } else if ((mode == 1 || mode == 2) && N >= 128) {
    unsigned short* planes = h.planes((3 * n + 1) / 2 + 4);
    RAMP_REQUIRE(planes, "hipMalloc failed");
    CK(launch_split3(a.W, planes, (long)n, s));
    a.Wx = planes; a.wx_plane = (long)n;
  }
  return h.finish(launch_gemm(a, s), a_absmax_out_host, range_flag_out_host);     // (no slots outside fp16x3: reports 0 / 0)
}
}  // namespace ramp

extern "C" {

// ---- kernel-level entry points ---------------------------------------------------------------------
// The context-free entry points take small HOST arrays (window weights, waypoint indices).  They are staged through a
// per-thread ring of device slots allocated once, so a call neither allocates nor synchronises; a slot is reused after
// RING calls, by which time the stream-ordered kernel that read it has long been submitted behind 63 others.
namespace {
struct HostArgRing {
  static constexpr int RING = 64, SLOT = 1024;       // bytes per slot: 129 window weights or 256 indices
  // one ring per device (a thread that alternates devices keeps both); every slot carries the event recorded behind the
  // kernel that reads it, on whatever stream that was: before a slot is reused the event is waited for, so calls on
  // different streams cannot overwrite an array an earlier kernel has not read yet (normally complete long ago: 63 calls)
  struct PerDevice { char* base = nullptr; int next = 0; hipEvent_t ev[RING] = {}; bool used[RING] = {}; };
  std::map<int, PerDevice> rings;
  int cur_dev = -1, cur_slot = -1;
  int stage(const void* host, size_t bytes, hipStream_t s, void** out) {
    RAMP_REQUIRE(bytes <= (size_t)SLOT, "host argument array too long");
    int dev = 0; RAMP_HIP_CHECK(hipGetDevice(&dev));
    PerDevice& r = rings[dev];
    if (!r.base) RAMP_HIP_CHECK(hipMalloc(&r.base, (size_t)RING * SLOT));
    const int slot = r.next++ % RING;
    if (r.used[slot]) RAMP_HIP_CHECK(hipEventSynchronize(r.ev[slot]));
    else { RAMP_HIP_CHECK(hipEventCreateWithFlags(&r.ev[slot], hipEventDisableTiming)); r.used[slot] = true; }
    char* p = r.base + (size_t)slot * SLOT;
    RAMP_HIP_CHECK(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s));
    *out = p; cur_dev = dev; cur_slot = slot;
    return 0;
  }
  // after the kernel that reads the staged array has been launched on `s`
  int done(hipStream_t s) {
    if (cur_slot >= 0) RAMP_HIP_CHECK(hipEventRecord(rings[cur_dev].ev[cur_slot], s));
    cur_slot = -1;
    return 0;
  }
};
thread_local HostArgRing g_ring;
}  // namespace

int ramp_apf(float* traj, int32_t B, int32_t H, int32_t S, const ramp_apf_params* p, void* stream) {
  RAMP_REQUIRE(traj && p && p->cloud && p->window_weights_host, "null argument");
  RAMP_REQUIRE(p->window >= 0 && p->window <= 64, "bad window");
  hipStream_t s = as_stream(stream);
  void* w = nullptr;
  CK(g_ring.stage(p->window_weights_host, (2 * p->window + 1) * 4, s, &w));
  ApfArgs a; a.traj = traj; a.cloud = p->cloud; a.window = static_cast<const float*>(w); a.B = B; a.H = H; a.S = S;
  a.P = p->n_points; a.win = p->window; a.thr = p->threshold; a.strength = p->strength;
  for (int q = 0; q < std::max(1, p->passes); ++q) CK(launch_apf(a, s));
  return g_ring.done(s);
}

int ramp_apf_scenes(float* traj, int32_t B, int32_t H, int32_t S, const ramp_apf_params* p, const ramp_scene_batch* sc,
                    void* stream) {
  RAMP_REQUIRE(traj && p && sc && p->window_weights_host, "null argument");
  RAMP_REQUIRE(!p->cloud, "ramp_apf_scenes: apf.cloud must be NULL (the clouds come with the scene batch)");
  RAMP_REQUIRE(p->window >= 0 && p->window <= 64, "bad window");
  CK(check_scene_batch(sc, true, "ramp_apf_scenes"));
  hipStream_t s = as_stream(stream);
  // window weights | scene offsets in one block of its own (the offsets of many scenes outgrow a slot of the host-argument ring);
  // synchronises `stream`
  const int nw = 2 * p->window + 1;
  std::vector<int32_t> blk(nw + sc->n_scenes + 1);
  std::memcpy(blk.data(), p->window_weights_host, nw * 4);
  std::memcpy(blk.data() + nw, sc->cloud_offset_host, (sc->n_scenes + 1) * 4);
  int32_t* w = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&w, blk.size() * 4));
  int rc = 0;
  if (hipMemcpy(w, blk.data(), blk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error("ramp_apf_scenes: copy of the tables failed"); rc = -1; }
  ApfArgs a; a.traj = traj; a.cloud = sc->cloud_points; a.window = reinterpret_cast<const float*>(w); a.B = B; a.H = H; a.S = S;
  a.win = p->window; a.thr = p->threshold; a.strength = p->strength;
  a.scene = sc->traj_scene; a.scene_off = w + nw; a.n_scenes = sc->n_scenes;
  for (int q = 0; rc == 0 && q < std::max(1, p->passes); ++q) rc = launch_apf(a, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(w);
  return rc;
}

// the guide's kernels on the caller's arrays: offsets | hard-condition indices go to the device in one block of their own (synchronises `stream`)
// team != nullptr: the kernels of guide_team.hip with these team arguments around `a` (terms_out is then (B, 4))
static int guide_op(GuideArgs a, const ramp_cost_guide* cg, const int32_t* traj_scene, int32_t n_hard, const int32_t* hard_idx_host,
                    const float* hard_val, double* terms_out, hipStream_t s, const TeamGuideArgs* team = nullptr) {
  std::vector<int32_t> blk(cg->cloud_offset_host, cg->cloud_offset_host + cg->n_scenes + 1);
  blk.insert(blk.end(), hard_idx_host, hard_idx_host + n_hard);
  int32_t* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, blk.size() * 4));
  int rc = 0;
  if (hipMemcpy(d, blk.data(), blk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error("guide: copy of the tables failed"); rc = -1; }
  a.cloud = cg->cloud_points; a.cloud_off = d; a.scene = traj_scene;
  a.hc.idx = d + cg->n_scenes + 1; a.hc.val = hard_val; a.hc.n = n_hard;
  if (rc == 0 && team) {
    TeamGuideArgs t = *team; t.g = a;
    rc = terms_out ? launch_guide_team_cost(t, terms_out, s) : launch_guide_team_step(t, s);
  } else if (rc == 0) {
    rc = terms_out ? launch_guide_cost(a, terms_out, s) : launch_guide_step(a, s);
  }
  (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

int ramp_guide_step(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const int32_t* traj_scene, int32_t n_iter,
                    float step, int32_t n_hard, const int32_t* hard_idx_host, const float* hard_val, void* stream) {
  RAMP_REQUIRE(traj && cg, "ramp_guide_step: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_step: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_step"));
  RAMP_REQUIRE(n_iter >= 0 && n_iter <= RAMP_GUIDE_MAX_STEPS, "ramp_guide_step: n_iter outside 0 .. RAMP_GUIDE_MAX_STEPS");
  RAMP_REQUIRE(std::isfinite(step), "ramp_guide_step: step must be finite");
  RAMP_REQUIRE(n_hard >= 0 && n_hard <= 256 && (n_hard == 0 || (hard_idx_host && hard_val)), "ramp_guide_step: bad hard conditions");
  for (int j = 0; j < n_hard; ++j) RAMP_REQUIRE(hard_idx_host[j] >= 0 && hard_idx_host[j] < H, "ramp_guide_step: hard index out of range");
  if (n_iter == 0) return 0;
  GuideArgs a = guide_args(cg, traj, B, H, S);
  a.n_iter = n_iter; a.step = step;
  return guide_op(a, cg, traj_scene, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream));
}

int ramp_guide_cost(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const int32_t* traj_scene,
                    double* terms_out, void* stream) {
  RAMP_REQUIRE(traj && cg && terms_out, "ramp_guide_cost: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_cost: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_cost"));
  return guide_op(guide_args(cg, const_cast<float*>(traj), B, H, S), cg, traj_scene, 0, nullptr, nullptr, terms_out, as_stream(stream));
}

// ramp_guide_step with the team term of ramp_team_guide.  tg == NULL, one agent per team or w_team == 0 is that entry itself
int ramp_guide_step_team(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                         const int32_t* traj_scene, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                         const float* hard_val, void* stream) {
  RAMP_REQUIRE(traj && cg, "ramp_guide_step_team: null argument (a team table needs its cost guide)");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_step_team: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_step_team"));
  if (tg) CK(check_team_guide(tg, B, H, "ramp_guide_step_team"));
  RAMP_REQUIRE(n_iter >= 0 && n_iter <= RAMP_GUIDE_MAX_STEPS, "ramp_guide_step_team: n_iter outside 0 .. RAMP_GUIDE_MAX_STEPS");
  RAMP_REQUIRE(std::isfinite(step), "ramp_guide_step_team: step must be finite");
  RAMP_REQUIRE(n_hard >= 0 && n_hard <= 256 && (n_hard == 0 || (hard_idx_host && hard_val)), "ramp_guide_step_team: bad hard conditions");
  for (int j = 0; j < n_hard; ++j) RAMP_REQUIRE(hard_idx_host[j] >= 0 && hard_idx_host[j] < H, "ramp_guide_step_team: hard index out of range");
  if (n_iter == 0) return 0;
  GuideArgs a = guide_args(cg, traj, B, H, S);
  a.n_iter = n_iter; a.step = step;
  if (!team_guide_active(tg)) return guide_op(a, cg, traj_scene, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream));
  const TeamGuideArgs t = team_guide_args(tg, a);
  return guide_op(a, cg, traj_scene, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream), &t);
}

int ramp_guide_cost_team(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                         const int32_t* traj_scene, double* terms_out, void* stream) {
  RAMP_REQUIRE(traj && cg && terms_out, "ramp_guide_cost_team: null argument (a team table needs its cost guide)");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_cost_team: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_cost_team"));
  if (tg) CK(check_team_guide(tg, B, H, "ramp_guide_cost_team"));
  const GuideArgs a = guide_args(cg, const_cast<float*>(traj), B, H, S);
  const TeamGuideArgs t = team_guide_args(tg, a);      // (no table: teams of one, column 3 = 0)
  return guide_op(a, cg, traj_scene, 0, nullptr, nullptr, terms_out, as_stream(stream), &t);
}

// every refusal of ramp_team_clearance is made here, on the host, before anything is launched
int ramp_team_clearance(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, int32_t team_size, float min_sep,
                        int32_t swept, const int32_t* row_mask, const float* row_len, const float* row_smooth, float* sep_wp,
                        float* sep_seg, int32_t* wp_conflicts, int32_t* seg_conflicts, int32_t* team_mask, float* team_len,
                        float* team_smooth, void* stream) {
  const std::string w = "ramp_team_clearance: ";
  RAMP_REQUIRE(traj, w + "null trajectories");
  RAMP_REQUIRE(B > 0 && S > 0 && (long)B * H * S < (1l << 31), w + "bad dims");
  RAMP_REQUIRE(H >= 2 && H <= 128, w + "the horizon must be 2 .. 128");
  RAMP_REQUIRE((point_dim == 2 || point_dim == 3) && point_dim <= S, w + "point_dim must be 2 or 3 and at most S");
  RAMP_REQUIRE(team_size >= 1 && team_size <= RAMP_TEAM_MAX, w + "team_size outside 1 .. RAMP_TEAM_MAX");
  RAMP_REQUIRE(B % team_size == 0, w + "the batch must be a multiple of team_size");
  RAMP_REQUIRE(min_sep >= 0.f, w + "min_sep must not be negative or NaN");
  TeamClearanceArgs a;
  a.traj = traj; a.B = B; a.H = H; a.S = S; a.D = point_dim; a.team = team_size; a.min_sep = min_sep; a.swept = swept != 0;
  a.row_mask = row_mask; a.row_len = row_len; a.row_smooth = row_smooth;
  a.sep_wp = sep_wp; a.sep_seg = sep_seg; a.wp_conflicts = wp_conflicts; a.seg_conflicts = seg_conflicts;
  a.team_mask = team_mask; a.team_len = team_len; a.team_smooth = team_smooth;
  return launch_team_clearance(a, as_stream(stream));
}

// the primitive guide's kernels on the caller's arrays: cloud offsets | box offsets | sphere offsets | hard-condition indices go to the device in
// one block of their own (synchronises `stream`)
static int prim_guide_op(GuideArgs g, const ramp_cost_guide* cg, const ramp_prim_guide* pg, const int32_t* traj_scene, int32_t n_hard,
                         const int32_t* hard_idx_host, const float* hard_val, double* terms_out, hipStream_t s) {
  const size_t no = (size_t)cg->n_scenes + 1;
  std::vector<int32_t> blk(cg->cloud_offset_host, cg->cloud_offset_host + no);
  blk.insert(blk.end(), pg->box_offset_host, pg->box_offset_host + no);
  blk.insert(blk.end(), pg->sphere_offset_host, pg->sphere_offset_host + no);
  blk.insert(blk.end(), hard_idx_host, hard_idx_host + n_hard);
  int32_t* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, blk.size() * 4));
  int rc = 0;
  if (hipMemcpy(d, blk.data(), blk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error("primitive guide: copy of the tables failed"); rc = -1; }
  g.cloud = cg->cloud_points; g.cloud_off = d; g.scene = traj_scene;
  g.hc.idx = d + 3 * no; g.hc.val = hard_val; g.hc.n = n_hard;
  PrimGuideArgs a = prim_guide_args(pg, g);
  a.box_c = pg->box_centers; a.box_s = pg->box_sizes; a.sph_c = pg->sphere_centers; a.sph_r = pg->sphere_radii;
  a.box_off = d + no; a.sph_off = d + 2 * no;
  if (rc == 0) rc = terms_out ? launch_guide_prims_cost(a, terms_out, s) : launch_guide_prims_step(a, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

int ramp_guide_step_prims(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                          const int32_t* traj_scene, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                          const float* hard_val, void* stream) {
  RAMP_REQUIRE(traj && cg, "ramp_guide_step_prims: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_step_prims: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_step_prims"));
  if (pg) CK(check_prim_guide(pg, cg, H, S, "ramp_guide_step_prims"));
  RAMP_REQUIRE(n_iter >= 0 && n_iter <= RAMP_GUIDE_MAX_STEPS, "ramp_guide_step_prims: n_iter outside 0 .. RAMP_GUIDE_MAX_STEPS");
  RAMP_REQUIRE(std::isfinite(step), "ramp_guide_step_prims: step must be finite");
  RAMP_REQUIRE(n_hard >= 0 && n_hard <= 256 && (n_hard == 0 || (hard_idx_host && hard_val)), "ramp_guide_step_prims: bad hard conditions");
  for (int j = 0; j < n_hard; ++j) RAMP_REQUIRE(hard_idx_host[j] >= 0 && hard_idx_host[j] < H, "ramp_guide_step_prims: hard index out of range");
  if (n_iter == 0) return 0;
  GuideArgs a = guide_args(cg, traj, B, H, S);
  a.n_iter = n_iter; a.step = step;
  if (!prim_guide_active(pg)) return guide_op(a, cg, traj_scene, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream));
  return prim_guide_op(a, cg, pg, traj_scene, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream));
}

int ramp_guide_cost_prims(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                          const int32_t* traj_scene, double* terms_out, void* stream) {
  RAMP_REQUIRE(traj && cg && terms_out, "ramp_guide_cost_prims: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && H <= GUIDE_MAX_H && S > 0, "ramp_guide_cost_prims: bad dims (H up to 128)");
  CK(check_cost_guide(cg, S, "ramp_guide_cost_prims"));
  if (pg) CK(check_prim_guide(pg, cg, H, S, "ramp_guide_cost_prims"));
  GuideArgs a = guide_args(cg, const_cast<float*>(traj), B, H, S);
  if (pg) return prim_guide_op(a, cg, pg, traj_scene, 0, nullptr, nullptr, terms_out, as_stream(stream));
  // no table: an empty one of the guide's shape (C_prim = 0)
  std::vector<int32_t> zero((size_t)cg->n_scenes + 1, 0);
  ramp_prim_guide none{};
  none.point_dim = cg->point_dim; none.n_scenes = cg->n_scenes; none.box_offset_host = zero.data(); none.sphere_offset_host = zero.data(); none.n_sub = 1;
  return prim_guide_op(a, cg, &none, traj_scene, 0, nullptr, nullptr, terms_out, as_stream(stream));
}

// the stitch on the caller's array: the blend weights go to the device in a block of their own (synchronises `stream`)
int ramp_stitch_windows(float* x, int32_t C, int32_t W, int32_t H, int32_t S, const ramp_stitch* st, void* stream) {
  RAMP_REQUIRE(x && st, "ramp_stitch_windows: null argument");
  RAMP_REQUIRE(C > 0 && W >= 1 && H > 0 && S > 0 && (long)C * W * H * S < (1l << 31), "ramp_stitch_windows: bad dims");
  RAMP_REQUIRE(st->n_windows == W, "ramp_stitch_windows: W differs from the table's n_windows");
  CK(check_stitch(st, C * W, H, "ramp_stitch_windows"));
  hipStream_t s = as_stream(stream);
  StitchArgs a = stitch_args(st, C * W, H, S);
  a.x = x; a.pin_val = st->pin_val;
  float* d = nullptr;
  int rc = 0;
  if (W > 1) {
    RAMP_HIP_CHECK(hipMalloc(&d, (size_t)a.O * 4));
    if (hipMemcpy(d, st->alpha_host, (size_t)a.O * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error("ramp_stitch_windows: copy of the blend table failed"); rc = -1; }
    a.alpha = d;
  }
  if (rc == 0) rc = launch_stitch(a, s);
  (void)hipStreamSynchronize(s);
  if (d) (void)hipFree(d);
  return rc;
}

int ramp_stitch_assemble(const float* x, int32_t C, int32_t W, int32_t H, int32_t S, int32_t O, float* long_out, void* stream) {
  RAMP_REQUIRE(x && long_out, "ramp_stitch_assemble: null argument");
  RAMP_REQUIRE(C > 0 && W >= 1 && H > 0 && S > 0 && (long)C * W * H * S < (1l << 31), "ramp_stitch_assemble: bad dims");
  RAMP_REQUIRE(W == 1 || (O >= 1 && 2 * O <= H), "ramp_stitch_assemble: overlap outside 1 .. H / 2");
  hipStream_t s = as_stream(stream);
  const int rc = launch_stitch_assemble(x, long_out, C, W, H, S, O, s);
  (void)hipStreamSynchronize(s);
  return rc;
}

// the warm start's two kernels on the caller's arrays: the per-row tables go to the device in one block of their own (synchronises `stream`)
static int warm_op(const char* who, const int32_t* ints_host, const float* f0_host, const float* f1_host, int32_t B, hipStream_t s,
                   const std::function<int(const int*, const float*, const float*)>& launch) {
  static_assert(sizeof(float) == sizeof(int32_t), "one block of 4-byte words");
  std::vector<int32_t> blk(3 * (size_t)B, 0);
  std::memcpy(blk.data(), ints_host, (size_t)B * 4);
  if (f0_host) std::memcpy(blk.data() + B, f0_host, (size_t)B * 4);
  if (f1_host) std::memcpy(blk.data() + 2 * (size_t)B, f1_host, (size_t)B * 4);
  int32_t* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, blk.size() * 4));
  int rc = 0;
  if (hipMemcpy(d, blk.data(), blk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error(std::string(who) + ": copy of the tables failed"); rc = -1; }
  if (rc == 0) rc = launch(d, reinterpret_cast<const float*>(d + B), reinterpret_cast<const float*>(d + 2 * (size_t)B));
  (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

int ramp_warm_init(float* x, const float* noise0, const float* prior, const float* sa_host, const float* s1a_host,
                   const int32_t* has_prior_host, int32_t B, int32_t H, int32_t S, void* stream) {
  RAMP_REQUIRE(x && noise0 && prior && sa_host && s1a_host && has_prior_host, "ramp_warm_init: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && ((long)H * S) % 4 == 0 && (long)B * H * S < (1l << 31),
               "ramp_warm_init: bad dims (H * S must be a multiple of 4)");
  hipStream_t s = as_stream(stream);
  return warm_op("ramp_warm_init", has_prior_host, sa_host, s1a_host, B, s, [&](const int* has, const float* sa, const float* s1a) {
    return launch_warm_init(x, noise0, prior, sa, s1a, has, B, H, S, s);
  });
}

int ramp_warm_hold(float* x, float* chain_block, const float* x_init, const int32_t* j0_host, int32_t j, int32_t B, int32_t H, int32_t S,
                   void* stream) {
  RAMP_REQUIRE(x && x_init && j0_host, "ramp_warm_hold: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && ((long)H * S) % 4 == 0 && (long)B * H * S < (1l << 31),
               "ramp_warm_hold: bad dims (H * S must be a multiple of 4)");
  hipStream_t s = as_stream(stream);
  return warm_op("ramp_warm_hold", j0_host, nullptr, nullptr, B, s, [&](const int* j0, const float*, const float*) {
    return launch_warm_hold(x, chain_block, x_init, j0, j, B, H, S, s);
  });
}

// the replans' guide kernels on the caller's arrays: offsets | hard-condition indices | moving points | tracks go to the device in one block
// of their own (synchronises `stream`)
static int moving_guide_op(MovingGuideArgs a, const ramp_replan_guide* rg, const int32_t* traj_scene, const int32_t* pin_first, int32_t n_hard,
                           const int32_t* hard_idx_host, const float* hard_val, double* terms_out, hipStream_t s) {
  static_assert(sizeof(float) == sizeof(int32_t), "one block of 4-byte words");
  const size_t n_off = (size_t)rg->n_scenes + 1, n_mv = (size_t)rg->n_scenes * rg->n_mov * 2, n_tr = rg->n_mov ? (size_t)rg->n_scenes * a.H * 2 : 0;
  std::vector<int32_t> blk(n_off + n_hard + n_mv + n_tr);
  std::memcpy(blk.data(), rg->cloud_offset_host, n_off * 4);
  if (n_hard) std::memcpy(blk.data() + n_off, hard_idx_host, (size_t)n_hard * 4);
  if (n_mv) std::memcpy(blk.data() + n_off + n_hard, rg->mov_points_host, n_mv * 4);
  if (n_tr) std::memcpy(blk.data() + n_off + n_hard + n_mv, rg->mov_track_host, n_tr * 4);
  int32_t* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, blk.size() * 4));
  int rc = 0;
  if (hipMemcpy(d, blk.data(), blk.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_last_error("moving guide: copy of the tables failed"); rc = -1; }
  a.cloud = rg->cloud_points; a.cloud_off = d; a.scene = traj_scene; a.pin_first = pin_first;
  a.hc.idx = d + n_off; a.hc.val = hard_val; a.hc.n = n_hard;
  a.mov = reinterpret_cast<const float*>(d + n_off + n_hard); a.track = a.mov + n_mv;
  if (rc == 0) rc = terms_out ? launch_guide_cost_moving(a, terms_out, s) : launch_guide_step_moving(a, s);
  (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

int ramp_guide_step_moving(float* traj, int32_t B, int32_t H, int32_t S, const ramp_replan_guide* rg, const int32_t* traj_scene,
                           const int32_t* pin_first, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                           const float* hard_val, void* stream) {
  RAMP_REQUIRE(traj && rg, "ramp_guide_step_moving: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0, "ramp_guide_step_moving: bad dims");
  CK(check_replan_guide(rg, 0, H, S, 0, "ramp_guide_step_moving"));
  RAMP_REQUIRE(n_iter >= 0 && n_iter <= RAMP_GUIDE_MAX_STEPS, "ramp_guide_step_moving: n_iter outside 0 .. RAMP_GUIDE_MAX_STEPS");
  RAMP_REQUIRE(std::isfinite(step), "ramp_guide_step_moving: step must be finite");
  RAMP_REQUIRE(n_hard >= 0 && n_hard <= 256 && (n_hard == 0 || (hard_idx_host && hard_val)), "ramp_guide_step_moving: bad hard conditions");
  for (int j = 0; j < n_hard; ++j) RAMP_REQUIRE(hard_idx_host[j] >= 0 && hard_idx_host[j] < H, "ramp_guide_step_moving: hard index out of range");
  if (n_iter == 0) return 0;
  MovingGuideArgs a = moving_guide_args(rg, traj, B, H, S);
  a.n_iter = n_iter; a.step = step;
  return moving_guide_op(a, rg, traj_scene, pin_first, n_hard, hard_idx_host, hard_val, nullptr, as_stream(stream));
}

int ramp_guide_cost_moving(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_replan_guide* rg, const int32_t* traj_scene,
                           double* terms_out, void* stream) {
  RAMP_REQUIRE(traj && rg && terms_out, "ramp_guide_cost_moving: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0, "ramp_guide_cost_moving: bad dims");
  CK(check_replan_guide(rg, 0, H, S, 0, "ramp_guide_cost_moving"));
  return moving_guide_op(moving_guide_args(rg, const_cast<float*>(traj), B, H, S), rg, traj_scene, nullptr, 0, nullptr, nullptr, terms_out,
                         as_stream(stream));
}

// steps 3 and 4 of a resampling event on the caller's arrays, in place: one block of scratch {cum | tmp | x's second buffer | group table |
// ancestors} of its own (synchronises `stream`)
int ramp_resample_groups(float* x, int32_t B, int32_t H, int32_t S, double* logw, double* c_prev, const int32_t* group_first_host,
                         int32_t n_groups, const float* u, double ess_frac, int32_t* ancestor_out, double* ess_out, void* stream) {
  RAMP_REQUIRE(x && logw && u, "ramp_resample_groups: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && ((long)H * S) % 4 == 0, "ramp_resample_groups: bad dims (H * S must be a multiple of 4)");
  RAMP_REQUIRE(resample_group_table_fault(group_first_host, n_groups, B) == 0,
               "ramp_resample_groups: malformed group table (n_groups >= 1, [0] = 0, strictly increasing, [n_groups] = B)");
  RAMP_REQUIRE(resample_ess_frac_ok(ess_frac), "ramp_resample_groups: ess_frac must be finite and lie in [0, 2]");
  hipStream_t s = as_stream(stream);
  const size_t n = (size_t)B * H * S;
  const size_t bytes = 2 * (size_t)B * 8 + n * 4 + ((size_t)n_groups + 1 + B) * 4;      // (every part a multiple of 16 bytes or the last ones)
  char* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, bytes));
  ResampleGroupsArgs a; a.logw = logw; a.c_prev = c_prev; a.u = u; a.ess_frac = ess_frac; a.ess_out = ess_out; a.B = B; a.n_groups = n_groups;
  float* xtmp = reinterpret_cast<float*>(d);                                   // hipMalloc's alignment serves the 16-byte vectors
  a.cum = reinterpret_cast<double*>(d + n * 4); a.tmp = a.cum + B;
  int* gf = reinterpret_cast<int*>(d + n * 4 + 2 * (size_t)B * 8);
  int* anc = gf + n_groups + 1;
  a.group_first = gf; a.ancestor = anc;
  int rc = 0;
  if (hipMemcpyAsync(gf, group_first_host, ((size_t)n_groups + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess) { set_last_error("ramp_resample_groups: copy of the group table failed"); rc = -1; }
  if (rc == 0) rc = launch_resample_groups(a, s);
  if (rc == 0) rc = launch_resample_gather(x, anc, xtmp, B, H * S, s);
  if (rc == 0 && hipMemcpyAsync(x, xtmp, n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_last_error("ramp_resample_groups: copy back failed"); rc = -1; }
  if (rc == 0 && ancestor_out && hipMemcpyAsync(ancestor_out, anc, (size_t)B * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) { set_last_error("ramp_resample_groups: copy of the ancestors failed"); rc = -1; }
  (void)hipStreamSynchronize(s);
  (void)hipFree(d);
  return rc;
}

int ramp_apf_dynamic(float* traj, int32_t B, int32_t H, int32_t S, const double* points, int32_t n_points,
                     double thr_query, double thr_force, double strength, int32_t window, int32_t affected,
                     const float* goal, const int32_t* enable, void* stream) {
  RAMP_REQUIRE(traj && points, "null argument");
  ApfDynArgs a; a.traj = traj; a.points = points; a.goal = goal; a.enable = enable; a.B = B; a.H = H; a.S = S;
  a.P = n_points; a.window = window; a.affected = affected; a.thr_query = thr_query; a.thr_force = thr_force;
  a.strength = strength;
  return launch_apf_dynamic(a, as_stream(stream));
}

int ramp_hard_cond(float* x, int32_t B, int32_t H, int32_t S, int32_t n, const int32_t* idx_host, const float* val,
                   void* stream) {
  RAMP_REQUIRE(x && (n == 0 || (idx_host && val)), "null argument");
  if (n == 0) return 0;
  RAMP_REQUIRE(n <= 256, "too many hard conditions");
  for (int j = 0; j < n; ++j) RAMP_REQUIRE(idx_host[j] >= 0 && idx_host[j] < H, "hard index out of range");
  hipStream_t s = as_stream(stream);
  void* d = nullptr;
  CK(g_ring.stage(idx_host, (size_t)n * 4, s, &d));
  HardConds hc; hc.idx = static_cast<const int*>(d); hc.val = val; hc.n = n;
  CK(launch_hard_cond(x, hc, B, H, S, s));
  return g_ring.done(s);
}

int ramp_traj_costs(const float* traj, int32_t B, int32_t H, int32_t S, const float* cloud, int32_t n_points,
                    float threshold, int32_t* mask, float* path_len, float* smooth, void* stream) {
  RAMP_REQUIRE(traj && cloud && mask && path_len && smooth, "null argument");
  return launch_traj_costs(traj, cloud, B, H, S, n_points, threshold, mask, path_len, smooth, as_stream(stream));
}
int ramp_traj_metrics(const float* traj, int32_t B, int32_t H, int32_t S, const float* box_centers, const float* box_sizes,
                      int32_t n_boxes, float* intensity, float* path_len, float* smooth, void* stream) {
  RAMP_REQUIRE(traj && intensity && path_len && smooth && (n_boxes == 0 || (box_centers && box_sizes)), "null argument");
  return launch_traj_metrics(traj, B, H, S, box_centers, box_sizes, n_boxes, intensity, path_len, smooth, as_stream(stream));
}
int ramp_waypoint_variance(const float* traj, int32_t B, int32_t H, int32_t S, double* scratch, double* out, void* stream) {
  RAMP_REQUIRE(traj && scratch && out, "null argument");
  return launch_waypoint_variance(traj, B, H, S, scratch, out, as_stream(stream));
}
int ramp_q_sample_rows(const float* x_start, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int32_t* t_rows, int32_t T,
                       float* x_noisy, int32_t B, int32_t H, int32_t S, int32_t pin_endpoints, void* stream) {
  RAMP_REQUIRE(x_start && noise && sqrt_ac && sqrt_1m_ac && t_rows && x_noisy, "null argument");
  return launch_q_sample_rows(x_start, noise, sqrt_ac, sqrt_1m_ac, t_rows, T, x_noisy, B, H, S, pin_endpoints != 0, as_stream(stream));
}
int ramp_denoise_loss(float* x_recon, const float* x_start, const float* target, int32_t B, int32_t H, int32_t S, int32_t l1, double* scratch,
                      double* out, void* stream) {
  RAMP_REQUIRE(x_recon && x_start && target && scratch && out && (l1 == 0 || l1 == 1), "null argument or bad loss type");
  return launch_denoise_loss(x_recon, x_start, target, B, H, S, l1, scratch, out, as_stream(stream));
}


// ---- a many-scene batch (ramp_sample_scenes' layout: a scene's rows adjacent, scenes in order), every table on the device ----
#define RAMP_REQUIRE_SCENES(B, S, n_scenes) \
  do { RAMP_REQUIRE((n_scenes) > 0, "n_scenes must be positive"); RAMP_REQUIRE((B) > 0, "empty batch (B <= 0)"); \
       RAMP_REQUIRE((S) >= 2, "trajectories need xy states (S >= 2)"); } while (0)
int ramp_traj_metrics_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                             const float* box_centers, const float* box_sizes, const int32_t* box_offset, int32_t n_boxes_total,
                             float* intensity, float* path_len, float* smooth, void* stream) {
  RAMP_REQUIRE(traj && intensity && path_len && smooth, "null argument");
  RAMP_REQUIRE(traj_first && box_offset, "null scene table");
  RAMP_REQUIRE(n_boxes_total == 0 || (box_centers && box_sizes), "null boxes");
  RAMP_REQUIRE_SCENES(B, S, n_scenes);
  return launch_traj_metrics_scenes(traj, B, H, S, traj_first, n_scenes, box_centers, box_sizes, box_offset, n_boxes_total, intensity,
                                    path_len, smooth, as_stream(stream));
}
int ramp_scene_summary(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                       const float* intensity, const float* path_len, float threshold, double* scratch, double* summary,
                       int32_t* free_mask, void* stream) {
  RAMP_REQUIRE(traj && intensity && path_len && scratch && summary && free_mask, "null argument");
  RAMP_REQUIRE(traj_first, "null scene table");
  RAMP_REQUIRE_SCENES(B, S, n_scenes);
  return launch_scene_summary(traj, B, H, S, traj_first, n_scenes, intensity, path_len, threshold, scratch, summary, free_mask,
                              as_stream(stream));
}
int ramp_traj_costs_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                           const float* cloud, const int32_t* cloud_offset, int32_t n_points_total, float threshold, int32_t* mask,
                           float* path_len, float* smooth, void* stream) {
  RAMP_REQUIRE(traj && cloud && mask && path_len && smooth, "null argument");
  RAMP_REQUIRE(traj_first && cloud_offset, "null scene table");
  RAMP_REQUIRE_SCENES(B, S, n_scenes);
  return launch_traj_costs_scenes(traj, cloud, traj_first, cloud_offset, n_scenes, n_points_total, B, H, S, threshold, mask, path_len,
                                  smooth, as_stream(stream));
}
int ramp_select_best_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                            const float* cloud, const int32_t* cloud_offset, int32_t n_points_total, float threshold, float w_smooth,
                            float w_len, int32_t* mask, float* path_len, float* smooth, float* best_out, int32_t* result_dev,
                            void* stream) {
  RAMP_REQUIRE(traj && cloud && mask && path_len && smooth && best_out && result_dev, "null argument");
  RAMP_REQUIRE(traj_first && cloud_offset, "null scene table");
  RAMP_REQUIRE_SCENES(B, S, n_scenes);
  hipStream_t s = as_stream(stream);
  CK(launch_traj_costs_scenes(traj, cloud, traj_first, cloud_offset, n_scenes, n_points_total, B, H, S, threshold, mask, path_len,
                              smooth, s));
  return launch_select_scenes(traj, mask, path_len, smooth, w_smooth, w_len, traj_first, n_scenes, best_out, result_dev, B, H, S, s);
}

int ramp_scene_summary_nd(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, const int32_t* traj_first, int32_t n_scenes,
                          const float* intensity, const float* path_len, float threshold, double* scratch, double* summary,
                          int32_t* free_mask, void* stream) {
  RAMP_REQUIRE(traj && intensity && path_len && scratch && summary && free_mask, "ramp_scene_summary_nd: null argument");
  RAMP_REQUIRE(traj_first, "ramp_scene_summary_nd: null scene table");
  RAMP_REQUIRE((point_dim == 2 || point_dim == 3) && point_dim <= S, "ramp_scene_summary_nd: point_dim must be 2 or 3 and at most S");
  RAMP_REQUIRE_SCENES(B, S, n_scenes);
  return launch_scene_summary(traj, B, H, S, traj_first, n_scenes, intensity, path_len, threshold, scratch, summary, free_mask,
                              as_stream(stream), point_dim);
}
int ramp_select_scored_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                              const int32_t* mask, const float* path_len, const float* smooth, float w_smooth, float w_len,
                              float* best_out, int32_t* result_dev, void* stream) {
  RAMP_REQUIRE(traj && mask && path_len && smooth && best_out && result_dev, "ramp_select_scored_scenes: null argument");
  RAMP_REQUIRE(traj_first, "ramp_select_scored_scenes: null scene table");
  RAMP_REQUIRE(B > 0 && H > 0 && S >= 2 && n_scenes > 0 && n_scenes <= B, "ramp_select_scored_scenes: bad dims (B, H > 0, S >= 2, 1 <= n_scenes <= B)");
  return launch_select_scenes(traj, mask, path_len, smooth, w_smooth, w_len, traj_first, n_scenes, best_out, result_dev, B, H, S,
                              as_stream(stream));
}
static_assert(RAMP_DIVERSE_MAX_K == DIVERSE_MAX_K, "ramp_hip.h and args_sampler.h state the same K limit");
// every refusal of ramp_select_diverse_scenes is made here, on the host, before anything is launched
int ramp_select_diverse_scenes(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, const int32_t* traj_first,
                               int32_t n_scenes, const int32_t* mask, const float* path_len, const float* smooth, float w_smooth,
                               float w_len, int32_t K, float min_sep, int32_t metric, float* best_out, int32_t* rows_out,
                               int32_t* result_dev, int32_t* mode_of, float* sep_out, int32_t* mode_count, void* scratch, void* stream) {
  const std::string w = "ramp_select_diverse_scenes: ";
  RAMP_REQUIRE(traj && mask && path_len && smooth, w + "null trajectories, mask, path_len or smooth");
  RAMP_REQUIRE(traj_first, w + "null scene table");
  RAMP_REQUIRE(best_out && rows_out && result_dev && mode_of && sep_out && mode_count, w + "null output");
  RAMP_REQUIRE(scratch, w + "null scratch");
  RAMP_REQUIRE(B >= 0 && n_scenes >= 1, w + "B must not be negative and n_scenes must be at least 1");
  RAMP_REQUIRE(H >= 1 && H <= 128, w + "the horizon must be 1 .. 128");
  RAMP_REQUIRE((point_dim == 2 || point_dim == 3) && point_dim <= S, w + "point_dim must be 2 or 3 and at most S");
  RAMP_REQUIRE(K >= 1 && K <= RAMP_DIVERSE_MAX_K, w + "K must be 1 .. RAMP_DIVERSE_MAX_K");
  RAMP_REQUIRE(min_sep >= 0.f, w + "min_sep must not be negative or NaN");
  RAMP_REQUIRE(metric == 0 || metric == 1, w + "metric must be 0 (mean) or 1 (maximum)");
  DiverseArgs a;
  a.traj = traj; a.B = B; a.H = H; a.S = S; a.D = point_dim; a.traj_first = traj_first; a.n_scenes = n_scenes;
  a.mask = mask; a.plen = path_len; a.smooth = smooth; a.w_s = w_smooth; a.w_l = w_len; a.K = K; a.min_sep = min_sep; a.metric = metric;
  a.best = best_out; a.rows = rows_out; a.result = result_dev; a.mode_of = mode_of; a.sep = sep_out; a.mode_count = mode_count;
  a.state = static_cast<int*>(scratch); a.tot = reinterpret_cast<float*>(a.state + B); a.pick = a.state + 2 * (size_t)B;
  return launch_select_diverse(a, as_stream(stream));
}
// every refusal of ramp_traj_clearance is made here, on the host, before anything is launched
int ramp_traj_clearance(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_obstacles* ob, const int32_t* traj_first,
                        int32_t swept, int32_t* wp_hits, int32_t* seg_hits, float* clear_wp, float* clear_seg, float* path_len,
                        float* smooth, void* stream) {
  const std::string w = "ramp_traj_clearance: ";
  RAMP_REQUIRE(traj && ob, w + "null trajectories or obstacles");
  RAMP_REQUIRE(B > 0 && S >= 2, w + "empty batch or states narrower than 2");
  RAMP_REQUIRE((ob->point_dim == 2 || ob->point_dim == 3) && ob->point_dim <= S, w + "point_dim must be 2 or 3 and at most S");
  RAMP_REQUIRE(H >= 2 && H <= 128, w + "the horizon must be 2 .. 128");
  RAMP_REQUIRE(ob->margin >= 0.f && std::isfinite(ob->margin), w + "margin must be finite and not negative");
  RAMP_REQUIRE(ob->n_scenes >= 1 && ob->n_scenes <= B, w + "n_scenes must be 1 .. B");
  RAMP_REQUIRE(traj_first && ob->box_offset && ob->sphere_offset && ob->cloud_offset, w + "missing table (traj_first, box_offset, sphere_offset, cloud_offset)");
  RAMP_REQUIRE(ob->n_boxes_total >= 0 && ob->n_spheres_total >= 0 && ob->n_points_total >= 0, w + "negative total");
  RAMP_REQUIRE(ob->n_boxes_total == 0 || (ob->box_centers && ob->box_sizes), w + "null boxes with n_boxes_total > 0");
  RAMP_REQUIRE(ob->n_spheres_total == 0 || (ob->sphere_centers && ob->sphere_radii), w + "null spheres with n_spheres_total > 0");
  RAMP_REQUIRE(ob->n_points_total == 0 || ob->cloud, w + "null cloud with n_points_total > 0");
  ClearanceArgs a;
  a.traj = traj; a.B = B; a.H = H; a.S = S; a.D = ob->point_dim; a.traj_first = traj_first; a.n_scenes = ob->n_scenes;
  a.box_c = ob->box_centers; a.box_s = ob->box_sizes; a.box_off = ob->box_offset; a.n_boxes = ob->n_boxes_total;
  a.sph_c = ob->sphere_centers; a.sph_r = ob->sphere_radii; a.sph_off = ob->sphere_offset; a.n_spheres = ob->n_spheres_total;
  a.cloud = ob->cloud; a.cloud_off = ob->cloud_offset; a.n_points = ob->n_points_total;
  a.margin = ob->margin; a.swept = swept != 0;
  a.wp_hits = wp_hits; a.seg_hits = seg_hits; a.clear_wp = clear_wp; a.clear_seg = clear_seg; a.plen = path_len; a.smooth = smooth;
  return launch_traj_clearance(a, as_stream(stream));
}

int ramp_cfg_mean(const float* x, const float* eps, int32_t B, int32_t HS, int32_t n_rp, double w0, double w1,
                  float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, int32_t clip, int32_t predict_x0, float* x0_out,
                  float* mean_out, float* ecomb_out, void* stream) {
  RAMP_REQUIRE(x && eps, "null argument");
  CfgMeanArgs m; m.x = x; m.eps = eps; m.B = B; m.HS = HS; m.n_rp = n_rp; m.w0 = (float)w0; m.w1 = (float)w1;
  m.w0p1 = (float)(1.0 + w0); m.sqrt_recip = sqrt_recip; m.sqrt_recipm1 = sqrt_recipm1; m.coef1 = coef1; m.coef2 = coef2;
  m.clip = clip; m.predict_x0 = predict_x0 != 0; m.x0 = x0_out; m.mean = mean_out; m.ecomb = ecomb_out;
  return launch_cfg_mean(m, as_stream(stream));
}

int ramp_cfg_mean_rows(const float* x, const float* eps, int32_t B, int32_t HS, int32_t n_rp, const float* row_weight,
                       float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, int32_t clip, int32_t predict_x0, float* x0_out,
                       float* mean_out, float* ecomb_out, void* stream) {
  RAMP_REQUIRE(x && eps && row_weight, "ramp_cfg_mean_rows: null argument");
  RAMP_REQUIRE(n_rp >= 2 && n_rp <= RAMP_MAX_ROWS_PER_TRAJ, "ramp_cfg_mean_rows: n_rp outside 2 .. RAMP_MAX_ROWS_PER_TRAJ");
  RAMP_REQUIRE(B > 0 && HS > 0 && HS % 4 == 0, "ramp_cfg_mean_rows: B > 0 and H * S a positive multiple of 4");
  for (const void* q : {(const void*)x, (const void*)eps, (const void*)x0_out, (const void*)mean_out, (const void*)ecomb_out})
    RAMP_REQUIRE(((uintptr_t)q & 15) == 0, "ramp_cfg_mean_rows: tensors must be 16-byte aligned");
  CfgMeanArgs m; m.x = x; m.eps = eps; m.B = B; m.HS = HS; m.n_rp = n_rp;
  m.sqrt_recip = sqrt_recip; m.sqrt_recipm1 = sqrt_recipm1; m.coef1 = coef1; m.coef2 = coef2;
  m.clip = clip; m.predict_x0 = predict_x0 != 0; m.x0 = x0_out; m.mean = mean_out; m.ecomb = ecomb_out;
  return launch_cfg_mean_rows(m, row_weight, as_stream(stream));
}

int ramp_ddim_finish(const float* x, const float* x0, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                     float dir_coef, float* x_out, int32_t B, int32_t H, int32_t S, void* stream) {
  RAMP_REQUIRE(x && x0 && x_out, "null argument");
  HardConds hc;
  return launch_ddim_finish(x, x0, sqrt_a_t, sqrt_1m_a_t, sqrt_a_prev, dir_coef, hc, x_out, nullptr, B, H, S,
                            as_stream(stream));
}

int ramp_row_energy(const float* f, int32_t R, int32_t HS, double* energy_out, void* stream) {
  RAMP_REQUIRE(f && energy_out, "ramp_row_energy: null argument");
  RAMP_REQUIRE(R > 0 && HS > 0, "ramp_row_energy: R > 0 and H * S > 0");
  return launch_row_energy(f, energy_out, R, HS, as_stream(stream));
}

int ramp_combine_energy(const double* energy_rows, int32_t B, int32_t n_rp, const float* weights_host, const float* row_weight,
                        double* energy_out, void* stream) {
  RAMP_REQUIRE(energy_rows && energy_out, "ramp_combine_energy: null argument");
  RAMP_REQUIRE((weights_host != nullptr) != (row_weight != nullptr), "ramp_combine_energy: exactly one of weights_host and row_weight");
  RAMP_REQUIRE(B > 0 && n_rp >= 1 && n_rp <= (row_weight ? RAMP_MAX_ROWS_PER_TRAJ : 3), "ramp_combine_energy: n_rp outside 1 .. 3 (host weights) / 1 .. RAMP_MAX_ROWS_PER_TRAJ (table)");
  EnergyWeights w; w.rw = row_weight;
  if (weights_host) for (int j = 0; j < n_rp; ++j) w.w[j] = weights_host[j];
  return launch_combine_energy(energy_rows, w, energy_out, B, n_rp, as_stream(stream));
}

int ramp_mcmc_propose(const float* x, const float* eps, const float* z, float a, float c, const int32_t* pinned_idx, int32_t n_pinned,
                      float* x_prop, int32_t B, int32_t H, int32_t S, void* stream) {
  RAMP_REQUIRE(x && eps && z && x_prop, "ramp_mcmc_propose: null argument");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && n_pinned >= 0 && (n_pinned == 0 || pinned_idx), "ramp_mcmc_propose: bad dims");
  HardConds hc; hc.idx = pinned_idx; hc.n = n_pinned;
  return launch_mcmc_propose(x, eps, z, a, c, hc, x_prop, B, H, S, as_stream(stream));
}

int ramp_mcmc_accept(float* x, const float* x_prop, float* eps, const float* eps_prop, double* energy, const double* energy_prop,
                     const float* u, int32_t kind, float a, double sigma, double eta, const int32_t* pinned_idx, int32_t n_pinned,
                     int32_t* accept_out, double* log_alpha_out, int32_t B, int32_t H, int32_t S, void* stream) {
  RAMP_REQUIRE(x && x_prop && eps && eps_prop && accept_out, "ramp_mcmc_accept: null argument");
  RAMP_REQUIRE(kind == 1 || kind == 2, "ramp_mcmc_accept: kind must be 1 (ULA) or 2 (MALA)");
  RAMP_REQUIRE(kind == 1 || (energy && energy_prop && u), "ramp_mcmc_accept: MALA needs energy, energy_prop and u");
  RAMP_REQUIRE(kind == 1 || (sigma > 0 && eta > 0), "ramp_mcmc_accept: sigma and eta must be positive");
  RAMP_REQUIRE(B > 0 && H > 0 && S > 0 && n_pinned >= 0 && (n_pinned == 0 || pinned_idx), "ramp_mcmc_accept: bad dims");
  McmcAcceptArgs m; m.x = x; m.xp = x_prop; m.eps = eps; m.eps_p = eps_prop; m.E = energy; m.E_p = energy_prop; m.u = u;
  m.flag = accept_out; m.log_alpha = log_alpha_out; m.hc.idx = pinned_idx; m.hc.n = n_pinned; m.B = B; m.H = H; m.S = S;
  m.mala = kind == 2; m.a = a;
  if (m.mala) { m.inv_sigma = 1.0 / sigma; m.inv_4eta = 1.0 / (4.0 * eta); }
  return launch_mcmc_accept(m, as_stream(stream));
}

// the sample-owning k = 5 convolution (tkc.hip) on the raw weight W [5][N][K]: mode 5 of ramp_op_gemm_mode and the narrow layers of
// ramp_op_tkw; `t` carries the caller's operands
static int op_tkc(TkcArgs t, const float* W, float absmax_prev, float* absmax_out_host, int32_t* range_flag_out_host, hipStream_t s) {
  ScaledOp h(s);
  float sc = 1.f; CK(device_weight_scale(W, (size_t)5 * t.N * t.K, &sc));
  unsigned short* pl = h.planes(tkc_packed_halves(t.N, t.K) / 2 + 4);
  RAMP_REQUIRE(pl, "hipMalloc failed");
  CK(init_tkc_attributes());
  CK(tkc_pack(W, t.N, t.K, sc, pl, s));
  CK(h.begin(&absmax_prev));
  t.W = pl; h.attach(t, sc);
  return h.finish(launch_tkc(t, s), absmax_out_host, range_flag_out_host);
}

int ramp_op_gemm(const float* A, const float* W, const float* bias, const float* resid, float* C, int32_t M, int32_t N,
                 int32_t K, int32_t taps, int32_t shift0, int32_t shift_step, int32_t L, void* stream) {
  return ramp_op_gemm_mode(A, W, bias, resid, C, M, N, K, taps, shift0, shift_step, L, 0, 0.f, nullptr, nullptr, stream);
}

int ramp_op_gemm_mode(const float* A, const float* W, const float* bias, const float* resid, float* C, int32_t M,
                      int32_t N, int32_t K, int32_t taps, int32_t shift0, int32_t shift_step, int32_t L, int32_t mode,
                      float a_absmax_prev, float* a_absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(A && W && C, "null argument");
  RAMP_REQUIRE(mode >= 0 && mode <= 5 && mode != 4, "mode: 0 fp32, 1 bf16x6, 2 bf16x6 (LDS-staged weights), 3 fp16x3, 5 fp16x3 "
                                       "sample-owning k = 5 convolution (tkc.hip)");
  hipStream_t s = as_stream(stream);
  if (mode == 5) {
    RAMP_REQUIRE(taps == 5 && ((shift0 == -2 && shift_step == 1) || (shift0 == 2 && shift_step == -1)) && tkc_applicable(M, L, N, K, nullptr),
                 "mode 5: a k = 5 convolution (or its input gradient) with C_in, C_out in {32, 64}, L >= 8 dividing 48 or 32");
    TkcArgs t; t.M = M; t.L = L; t.N = N; t.K = K; t.dir = shift_step; t.X = A; t.ldx = K; t.bias = bias; t.resid = resid; t.ldr = N;
    t.Y = C; t.ldy = N;
    return op_tkc(t, W, a_absmax_prev, a_absmax_out_host, range_flag_out_host, s);
  }
  GemmArgs a; a.A = A; a.lda = K; a.W = W; a.bias = bias; a.resid = resid; a.ldr = N; a.C = C; a.ldc = N;
  a.M = M; a.N = N; a.K = K; a.taps = taps; a.shift0 = shift0; a.shift_step = shift_step; a.L = L;
  return op_gemm_packed(a, mode, a_absmax_prev, a_absmax_out_host, range_flag_out_host, s);
}
static int op_ffx_impl(const float* z1, const float* dz, const float* W1, const float* b1, const float* W2, const float* b2,
                       const float* ln_g, const float* ln_b, int32_t M, const float* absmax_prev_host, float* z2, float* dz1,
                       float* absmax_out_host, int32_t* range_flag_out_host, void* stream, bool s16) {
  RAMP_REQUIRE(z1 && W1 && b1 && W2 && b2 && ln_g && ln_b && z2 && M > 0, "null argument");
  hipStream_t s = as_stream(stream);
  ScaledOp h(s, 4);        // sites: forward LN(z1), forward a gelu(g), backward dz, backward second product
  FfxPack pk;
  CK(ffx_pack_all(h.ar, W1, b1, W2, &pk, s, s16));
  auto launch_ffx = [s16](const FfxArgs& a, bool bwd, hipStream_t st) { return s16 ? ramp::launch_ffx16(a, bwd, st) : ramp::launch_ffx(a, bwd, st); };
  const size_t mt = ((size_t)M + 127) / 128;
  float* stash = h.ar.alloc(mt * 128 * 2048);
  RAMP_REQUIRE(stash, "hipMalloc failed");
  CK(h.begin(absmax_prev_host));
  FfxArgs f; f.M = M; f.X = z1; f.Z1 = z1; f.Y = z2; f.stash = stash; f.ln_g = ln_g; f.ln_b = ln_b; f.Wstream = pk.stream_f;
  f.b1 = pk.b1_pk; f.b2 = b2; f.range_flag = h.range_flag();
  f.amax_in1 = h.amax_in(0); f.amax_out1 = h.amax_out(0); f.wsi1 = pk.wsi_w1; f.site1 = 0;
  f.amax_in2 = h.amax_in(1); f.amax_out2 = h.amax_out(1); f.wsi2 = pk.wsi_w2; f.site2 = 1;
  int rc = launch_ffx(f, false, s);
  if (rc == 0 && dz && dz1) {
    FfxArgs g; g.M = M; g.X = dz; g.Z1 = z1; g.Y = dz1; g.stash = stash; g.ln_g = ln_g; g.ln_b = ln_b; g.Wstream = pk.stream_b;
    g.range_flag = h.range_flag();
    g.amax_in1 = h.amax_in(2); g.amax_out1 = h.amax_out(2); g.wsi1 = pk.wsi_w2; g.site1 = 2;
    g.amax_in2 = h.amax_in(3); g.amax_out2 = h.amax_out(3); g.wsi2 = pk.wsi_w1; g.site2 = 3;
    rc = launch_ffx(g, true, s);
  }
  return h.finish(rc, absmax_out_host, range_flag_out_host);
}
int ramp_op_ffx(const float* z1, const float* dz, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* ln_g, const float* ln_b, int32_t M, const float* absmax_prev_host, float* z2, float* dz1,
                float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  return op_ffx_impl(z1, dz, W1, b1, W2, b2, ln_g, ln_b, M, absmax_prev_host, z2, dz1, absmax_out_host, range_flag_out_host, stream, false);
}
int ramp_op_ffx16(const float* z1, const float* dz, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* ln_g, const float* ln_b, int32_t M, const float* absmax_prev_host, float* z2, float* dz1,
                  float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  return op_ffx_impl(z1, dz, W1, b1, W2, b2, ln_g, ln_b, M, absmax_prev_host, z2, dz1, absmax_out_host, range_flag_out_host, stream, true);
}

static int op_tkl_impl(const float* X, const float* W, const float* bias, const float* resid, const float* rowbias,
                       const int32_t* rowvar, int32_t n_var, int32_t L, const float* ln_g, const float* ln_b, int32_t M, int32_t N,
                       float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream, bool s16) {
  RAMP_REQUIRE(X && W && Y && M > 0 && N >= 32 && N % 32 == 0 && N <= 768, "bad arguments");
  hipStream_t s = as_stream(stream);
  ScaledOp h(s);
  float sc = 1.f; CK(device_weight_scale(W, (size_t)N * 256, &sc));
  unsigned short* planes = h.planes((size_t)N * 256 + 4);
  RAMP_REQUIRE(planes, "hipMalloc failed");
  if (s16) {      // 16 x 32 fragments (tkl16.hip)
    float* tmp = h.ar.alloc((size_t)N * 256);
    RAMP_REQUIRE(tmp, "hipMalloc failed");
    CK(ffx16_pack(W, N, 256, 0, sc, tmp, planes, s));
  } else CK(launch_pack_h3(W, planes, N, 256, sc, s));
  CK(h.begin(&absmax_prev));
  TklArgs a; a.M = M; a.N = N; a.X = X; a.Y = Y; a.ldy = N; a.W = planes; a.bias = bias; a.resid = resid; a.ldr = N;
  a.rowbias = rowbias; a.rowvar = rowvar; a.row0 = 0; a.rb_stride = N; a.L = L > 0 ? L : 1; a.n_var = n_var;
  a.ln_g = ln_g; a.ln_b = ln_b; h.attach(a, sc);
  return h.finish(s16 ? launch_tkl16(a, s) : launch_tkl(a, s), absmax_out_host, range_flag_out_host);
}

int ramp_op_tkl(const float* X, const float* W, const float* bias, const float* resid, const float* rowbias,
                const int32_t* rowvar, int32_t n_var, int32_t L, const float* ln_g, const float* ln_b, int32_t M, int32_t N,
                float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  return op_tkl_impl(X, W, bias, resid, rowbias, rowvar, n_var, L, ln_g, ln_b, M, N, absmax_prev, Y, absmax_out_host, range_flag_out_host, stream, false);
}
int ramp_op_tkl16(const float* X, const float* W, const float* bias, const float* resid, const float* rowbias,
                  const int32_t* rowvar, int32_t n_var, int32_t L, const float* ln_g, const float* ln_b, int32_t M, int32_t N,
                  float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  return op_tkl_impl(X, W, bias, resid, rowbias, rowvar, n_var, L, ln_g, ln_b, M, N, absmax_prev, Y, absmax_out_host, range_flag_out_host, stream, true);
}

int ramp_op_ato(const float* qkv, const float* Wo, const float* bias, const float* resid, const float* rowbias, const int32_t* rowvar,
                int32_t n_var, int32_t L, int32_t M, float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(qkv && Wo && resid && Y && M > 0 && L > 0, "bad arguments");
  hipStream_t s = as_stream(stream);
  ScaledOp h(s);
  float sc = 1.f; CK(device_weight_scale(Wo, (size_t)256 * 256, &sc));
  unsigned short* stream_w = h.planes(8 * 8192 + 4);
  RAMP_REQUIRE(stream_w, "hipMalloc failed");
  CK(init_atk_attributes());
  CK(ato_pack(Wo, sc, stream_w, s));
  CK(h.begin(&absmax_prev));
  AtoArgs a; a.M = M; a.L = L; a.QKV = qkv; a.W = stream_w; a.bias = bias; a.resid = resid; a.Y = Y;
  a.rowbias = rowbias; a.rowvar = rowvar; a.row0 = 0; a.rb_stride = 256; a.n_var = rowbias ? n_var : 0;
  h.attach(a, sc);
  return h.finish(launch_ato(a, s), absmax_out_host, range_flag_out_host);
}

int ramp_op_atb(const float* qkv, const float* dout, float* dqkv, int32_t M, int32_t L, void* stream) {
  RAMP_REQUIRE(qkv && dout && dqkv && M > 0 && L > 0, "bad arguments");
  AtbArgs a; a.M = M; a.L = L; a.QKV = qkv; a.dO = dout; a.dQKV = dqkv;
  return launch_atb(a, as_stream(stream));
}

int ramp_op_abl(const float* qkv, const float* dout, const float* W, const float* z, const float* ln_g, const float* add, int32_t M, int32_t L,
                float absmax_prev, float* out, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(qkv && dout && W && z && ln_g && add && out && M > 0 && L > 0, "bad arguments");
  hipStream_t s = as_stream(stream);
  ScaledOp h(s);
  float sc = 1.f; CK(device_weight_scale(W, (size_t)256 * 768, &sc));
  unsigned short* stream_w = h.planes((size_t)256 * 768 + 4);
  RAMP_REQUIRE(stream_w, "hipMalloc failed");
  CK(init_atl_attributes());
  CK(abl_pack(W, sc, stream_w, s));
  CK(h.begin(&absmax_prev));
  AblArgs a; a.M = M; a.L = L; a.QKV = qkv; a.dO = dout; a.W = stream_w; a.Z = z; a.add = add; a.ln_g = ln_g; a.Y = out;
  h.attach(a, sc);
  return h.finish(launch_abl(a, s), absmax_out_host, range_flag_out_host);
}

// ramp_op_tkw and ramp_op_tkw_rows: t_rows == nullptr -> tbias is the (N) time bias; else tbias is the time table (line stride tt_stride) and sample r adds line t_rows[r]
static int op_tkw(const float* X, const float* X2, int32_t K1, const float* W, const float* bias, const float* resid, const float* resid2,
                  const float* gn_c, const float* gn_stats, const float* gn_gamma, const float* gn_beta, const float* gamma, const float* beta,
                  const float* tbias, const int32_t* t_rows, int32_t tt_stride, int32_t M, int32_t L, int32_t N, int32_t K, int32_t dir, int32_t N1,
                  float absmax_prev, float* Y, float* Y2, float* Cst, float* stats, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(X && W && Y && M > 0 && L > 0 && N % 32 == 0 && K % 16 == 0, "bad arguments");
  hipStream_t s = as_stream(stream);
  if (N <= 64 && K <= 64) {      // the narrow layers: the same fusion on sample-owning WAVES (tkc.hip)
    RAMP_REQUIRE(!X2 && !Y2 && tkc_applicable(M, L, N, K, nullptr), "narrow fused convolution: C_in, C_out in {32, 64}, L >= 8 dividing 48 or 32, one operand, one output");
    TkcArgs t; t.M = M; t.L = L; t.N = N; t.K = K; t.dir = dir; t.X = X; t.ldx = K; t.bias = bias; t.resid = resid; t.ldr = N;
    t.resid2 = resid2; t.ldr2 = N; t.Y = Y; t.ldy = N;
    t.gn_c = gn_c; t.gn_stats = gn_stats; t.gn_gamma = gn_gamma; t.gn_beta = gn_beta;
    t.Cst = Cst; t.stats = stats; t.gamma = gamma; t.beta = beta; t.tbias = tbias; t.t_rows = t_rows; t.tt_stride = tt_stride; t.eps = 1e-5f;
    return op_tkc(t, W, absmax_prev, absmax_out_host, range_flag_out_host, s);
  }
  ScaledOp h(s);
  const size_t n = (size_t)5 * N * K;
  float sc = 1.f; CK(device_weight_scale(W, n, &sc));
  unsigned short* planes = h.planes(n + 4);
  RAMP_REQUIRE(planes, "hipMalloc failed");
  CK(init_tkw_attributes());
  CK(launch_pack_h3(W, planes, (long)5 * N, K, sc, s));
  CK(h.begin(&absmax_prev));
  TkwArgs a; a.M = M; a.L = L; a.N = N; a.K = K; a.dir = dir; a.X = X; a.ldx = X2 ? K1 : K; a.X2 = X2; a.ldx2 = X2 ? K - K1 : 0; a.K1 = X2 ? K1 : K;
  a.gn_c = gn_c; a.gn_stats = gn_stats; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta; a.W = planes; a.bias = bias;
  a.resid = resid; a.ldr = N; a.resid2 = resid2; a.ldr2 = N; a.Y = Y; a.ldy = Y2 ? N1 : N; a.Y2 = Y2; a.ldy2 = Y2 ? N - N1 : 0; a.N1 = Y2 ? N1 : N;
  a.Cst = Cst; a.stats = stats; a.gamma = gamma; a.beta = beta; a.tbias = tbias; a.t_rows = t_rows; a.tt_stride = tt_stride; a.eps = 1e-5f;
  h.attach(a, sc);
  return h.finish(launch_tkw(a, s), absmax_out_host, range_flag_out_host);
}


int ramp_op_tkw(const float* X, const float* X2, int32_t K1, const float* W, const float* bias, const float* resid, const float* resid2,
                const float* gn_c, const float* gn_stats, const float* gn_gamma, const float* gn_beta, const float* gamma, const float* beta,
                const float* tbias, int32_t M, int32_t L, int32_t N, int32_t K, int32_t dir, int32_t N1, float absmax_prev, float* Y, float* Y2,
                float* Cst, float* stats, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  return op_tkw(X, X2, K1, W, bias, resid, resid2, gn_c, gn_stats, gn_gamma, gn_beta, gamma, beta, tbias, nullptr, 0, M, L, N, K, dir, N1, absmax_prev,
                Y, Y2, Cst, stats, absmax_out_host, range_flag_out_host, stream);
}
int ramp_op_tkw_rows(const float* X, const float* W, const float* bias, const float* resid, const float* gamma, const float* beta,
                     const float* time_table, int32_t tt_stride, const int32_t* t_rows, int32_t M, int32_t L, int32_t N, int32_t K, float absmax_prev,
                     float* Y, float* Cst, float* stats, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(time_table && t_rows && Cst && stats && gamma && beta && tt_stride >= N, "bad arguments (the forward convolution with its GroupNorm epilogue, a time table and a row -> timestep table)");
  return op_tkw(X, nullptr, K, W, bias, resid, nullptr, nullptr, nullptr, nullptr, nullptr, gamma, beta, time_table, t_rows, tt_stride, M, L, N, K, 1, N,
                absmax_prev, Y, nullptr, Cst, stats, absmax_out_host, range_flag_out_host, stream);
}

int ramp_op_tklb(const float* dqkv, const float* W, const float* z, const float* ln_g, const float* add, int32_t M,
                 float absmax_prev, float* out, float* absmax_out_host, int32_t* range_flag_out_host, void* stream) {
  RAMP_REQUIRE(dqkv && W && z && ln_g && add && out && M > 0, "bad arguments");
  hipStream_t s = as_stream(stream);
  ScaledOp h(s);
  float sc = 1.f; CK(device_weight_scale(W, (size_t)256 * 768, &sc));
  unsigned short* planes = h.planes((size_t)256 * 768 + 4);
  RAMP_REQUIRE(planes, "hipMalloc failed");
  CK(launch_pack_h3(W, planes, 256, 768, sc, s));
  CK(h.begin(&absmax_prev));
  TklbArgs a; a.M = M; a.X = dqkv; a.Z = z; a.add = add; a.Y = out; a.W = planes; a.ln_g = ln_g;
  h.attach(a, sc);
  return h.finish(launch_tklb(a, s), absmax_out_host, range_flag_out_host);
}

int ramp_op_groupnorm(const float* x, const float* gamma, const float* beta, const float* tbias, const float* resid,
                      float* y, float* stats, int32_t R, int32_t L, int32_t C, float eps, int32_t mish, void* stream) {
  RAMP_REQUIRE(x && gamma && beta && y, "null argument");
  GnArgs g; g.x = x; g.gamma = gamma; g.beta = beta; g.tbias = tbias; g.resid = resid; g.y = y; g.stats = stats;
  g.R = R; g.L = L; g.C = C; g.eps = eps; g.mish = mish;
  return launch_gn_fwd(g, as_stream(stream));
}
int ramp_op_groupnorm_rows(const float* x, const float* gamma, const float* beta, const float* time_table, int32_t tt_stride,
                           const int32_t* t_rows, const float* resid, float* y, float* stats, int32_t R, int32_t L, int32_t C, float eps,
                           int32_t mish, void* stream) {
  RAMP_REQUIRE(x && gamma && beta && y && time_table && t_rows && tt_stride >= C, "null argument");
  GnArgs g; g.x = x; g.gamma = gamma; g.beta = beta; g.tbias = time_table; g.t_rows = t_rows; g.tt_stride = tt_stride; g.resid = resid; g.y = y;
  g.stats = stats; g.R = R; g.L = L; g.C = C; g.eps = eps; g.mish = mish;
  return launch_gn_fwd(g, as_stream(stream));
}
int ramp_op_groupnorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* beta,
                          const float* add, float* dx, int32_t R, int32_t L, int32_t C, int32_t mish, void* stream) {
  RAMP_REQUIRE(dy && x && stats && gamma && beta && dx, "null argument");
  GnBwdArgs g; g.dy = dy; g.x = x; g.stats = stats; g.gamma = gamma; g.beta = beta; g.add = add; g.dx = dx;
  g.R = R; g.L = L; g.C = C; g.mish = mish;
  return launch_gn_bwd(g, as_stream(stream));
}
int ramp_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t n_tok, void* stream) {
  RAMP_REQUIRE(x && gamma && beta && y, "null argument");
  return launch_ln_fwd(x, gamma, beta, y, n_tok, as_stream(stream));
}
int ramp_op_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* add, float* dx,
                          int32_t n_tok, void* stream) {
  RAMP_REQUIRE(dy && x && gamma && dx, "null argument");
  return launch_ln_bwd(dy, x, gamma, add, dx, n_tok, as_stream(stream));
}
int ramp_op_geglu(const float* ag, float* hg, int32_t n_tok, int32_t F, void* stream) {
  RAMP_REQUIRE(ag && hg, "null argument");
  return launch_geglu_fwd(ag, hg, n_tok, F, as_stream(stream));
}
int ramp_op_geglu_bwd(const float* dhg, const float* ag, float* dag, int32_t n_tok, int32_t F, void* stream) {
  RAMP_REQUIRE(dhg && ag && dag, "null argument");
  return launch_geglu_bwd(dhg, ag, dag, n_tok, F, as_stream(stream));
}
int ramp_op_attention(const float* qkv, float* o, int32_t R, int32_t L, void* stream) {
  RAMP_REQUIRE(qkv && o, "null argument");
  return launch_attn_fwd(qkv, o, R, L, as_stream(stream));
}
int ramp_op_attention_bwd(const float* qkv, const float* dout, float* dqkv, int32_t R, int32_t L, void* stream) {
  RAMP_REQUIRE(qkv && dout && dqkv, "null argument");
  return launch_attn_bwd(qkv, dout, dqkv, R, L, as_stream(stream));
}

// ---- the scene encoders' kernels that look across tokens (scene.hip), single-scene and segmented; every table a device int32 array ----
int ramp_op_scene_attention(const float* qkv, float* o, int32_t T, int32_t heads, int32_t dh, float scale, void* stream) {
  RAMP_REQUIRE(qkv && o, "ramp_op_scene_attention: null argument");
  RAMP_REQUIRE(T > 0 && heads > 0, "ramp_op_scene_attention: T and heads must be positive");
  RAMP_REQUIRE(dh == 16 || dh == 64, "ramp_op_scene_attention: dh must be 16 or 64");
  return scene_attention(qkv, o, T, heads, dh, scale, as_stream(stream));
}
int ramp_op_scene_attention_seg(const float* qkv, float* o, const int32_t* tiles, int32_t n_tiles, int32_t heads, int32_t dh, float scale,
                                void* stream) {
  RAMP_REQUIRE(qkv && o && tiles, "ramp_op_scene_attention_seg: null argument");
  RAMP_REQUIRE(n_tiles > 0 && heads > 0, "ramp_op_scene_attention_seg: n_tiles and heads must be positive");
  RAMP_REQUIRE(dh == 16 || dh == 64, "ramp_op_scene_attention_seg: dh must be 16 or 64");
  return scene_attention_seg(qkv, o, tiles, n_tiles, heads, dh, scale, as_stream(stream));
}
int ramp_op_scene_colreduce(const float* x, float* out, int32_t n_seg, int32_t seglen, int32_t C, int32_t mode, void* stream) {
  RAMP_REQUIRE(x && out, "ramp_op_scene_colreduce: null argument");
  RAMP_REQUIRE(n_seg > 0 && seglen > 0 && C > 0, "ramp_op_scene_colreduce: n_seg, seglen and C must be positive");
  RAMP_REQUIRE(mode == 0 || mode == 1, "ramp_op_scene_colreduce: mode must be 0 (mean) or 1 (max)");
  return scene_colreduce(x, out, n_seg, seglen, C, mode, as_stream(stream));
}
int ramp_op_scene_colreduce_seg(const float* x, float* out, const int32_t* first, int32_t n_seg, int32_t C, int32_t ldo, int32_t mode,
                                void* stream) {
  RAMP_REQUIRE(x && out && first, "ramp_op_scene_colreduce_seg: null argument");
  RAMP_REQUIRE(n_seg > 0 && C > 0 && ldo >= C, "ramp_op_scene_colreduce_seg: n_seg and C must be positive, ldo at least C");
  RAMP_REQUIRE(mode == 0 || mode == 1, "ramp_op_scene_colreduce_seg: mode must be 0 (mean) or 1 (max)");
  return scene_colreduce_seg(x, out, first, n_seg, C, ldo, mode, as_stream(stream));
}
int ramp_op_scene_enc2d_prep(const float* cloud, int32_t No, int32_t Np, float* centers, float* maxd, void* stream) {
  RAMP_REQUIRE(cloud && centers && maxd, "ramp_op_scene_enc2d_prep: null argument");
  RAMP_REQUIRE(No > 0 && Np > 0, "ramp_op_scene_enc2d_prep: No and Np must be positive");
  return scene_enc2d_prep(cloud, No, Np, centers, maxd, as_stream(stream));
}
int ramp_op_scene_enc2d_prep_seg(const float* cloud, const int32_t* obstacle_first, int32_t No, float* centers, float* maxd, void* stream) {
  RAMP_REQUIRE(cloud && obstacle_first && centers && maxd, "ramp_op_scene_enc2d_prep_seg: null argument");
  RAMP_REQUIRE(No > 0, "ramp_op_scene_enc2d_prep_seg: No must be positive");
  return scene_enc2d_prep_seg(cloud, obstacle_first, No, centers, maxd, as_stream(stream));
}


}  // extern "C"
