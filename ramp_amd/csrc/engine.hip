// Context, weight packing and the forward / input-VJP schedule of the RAMP score network,
// plus the sampler loops and their hipGraph capture.  Host-side C++ over the kernels in
// gemm.hip / rowops.hip / sampler.hip; exported through the C ABI in include/ramp_hip.h.
//
// Reference structure being scheduled: TemporalUnetInference.forward_no_energy
// (UnetInference.py:176-224) and EnergyGradFunction (UnetInference.py:19-37) whose
// autograd.grad is replaced by the explicit dX chain below (all parameters are frozen, so no
// dW / db products exist anywhere).
#include "engine_util.h"
#include "encode_plan.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

namespace ramp {

static thread_local std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
int device_cu_count() {
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cached[dev]) {
    hipDeviceProp_t p;
    cached[dev] = hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return cached[dev];
}
const char* last_error_cstr() { return g_err.c_str(); }

struct ConvW {       // k=5 conv as 5-tap GEMM
  float* fwd = nullptr;   // [5][Cout][Cin]
  float* bwd = nullptr;   // [5][Cin][Cout]
  float* bias = nullptr;
  int cin = 0, cout = 0;
};
struct RTB {
  std::string name;
  int cin = 0, cout = 0, L = 0, tb_off = 0;
  bool has_res = false, first = false;
  ConvW c1, c2;
  float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
  float *res_f = nullptr, *res_b = nullptr, *res_bias = nullptr;   // [Cout][Cin], [Cin][Cout]
  float *w5in = nullptr, *w1in = nullptr;                           // first layer packed [5][S][C0], [S][C0]
  // activations (capacity rows)
  float *a_c1 = nullptr, *a_st1 = nullptr, *a_h = nullptr, *a_c2 = nullptr, *a_st2 = nullptr, *a_out = nullptr;
};
struct STBlock {
  float *wqkv_f = nullptr, *wqkv_b = nullptr, *wo_f = nullptr, *wo_b = nullptr, *bo = nullptr;
  float *w1_f = nullptr, *w1_b = nullptr, *b1 = nullptr, *w2_f = nullptr, *w2_b = nullptr, *b2 = nullptr;
  float *w1_pk = nullptr, *b1_pk = nullptr;        // GEGLU-packed forward weight / bias
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln3_g = nullptr, *ln3_b = nullptr;
  const float *wv2 = nullptr, *wo2 = nullptr, *bo2 = nullptr;    // attn2 (cross) raw
  float *a_qkv = nullptr, *a_z1 = nullptr, *a_ag = nullptr, *a_z2 = nullptr;
  // token-owning fused feed-forward (ffx.hip): the two weight streams, the weight scales of their first / second product
  unsigned short *ffx_f = nullptr, *ffx_b = nullptr; float ffx_wsi_w1 = 1.f, ffx_wsi_w2 = 1.f;
  unsigned short *ffx16_f = nullptr, *ffx16_b = nullptr;     // the same streams in 16 x 32 fragments (ffx16.hip)
  // self-attention fused with the output projection (atk.hip): the projection's weight stream
  unsigned short* ato_w = nullptr; float ato_wsi = 1.f;
  unsigned short* abl_w = nullptr;       // weight stream of the fused attention backward + d(ln1) (atl.hip), scale = the wqkv_b planes'
};
struct ST {
  std::string name;
  int C = 0, L = 0, blk0 = 0;
  float *gn_g = nullptr, *gn_b = nullptr, *wpi_f = nullptr, *wpi_b = nullptr, *bpi = nullptr;
  float *wpo_f = nullptr, *wpo_b = nullptr, *bpo = nullptr;
  STBlock blk[2];
  float *a_gst = nullptr, *a_z0 = nullptr, *a_y = nullptr;
};
struct Resample {
  std::string name;
  float *w_f = nullptr, *w_b = nullptr, *bias = nullptr;
  int C = 0, Lin = 0, Lout = 0, taps = 0;
  float* a_y = nullptr;
};

}  // namespace ramp

using namespace ramp;

#ifndef RAMP_DEFAULT_GEMM_MODE
#define RAMP_DEFAULT_GEMM_MODE 0
#endif

// the operand-maxima tables of the fp16x3 delayed scaling (ramp_ctx::obs)
enum { TABLE_EVEN = 0, TABLE_ODD = 1,      // ping-pong by evaluation: evaluation j of a job writes table j & 1 and reads its predecessor's
       TABLE_CANONICAL = 2,                // what evaluation 0 of a steady sampling job reads: the canonical calibration, written outside any job
       TABLE_REPLAN_CARRY = 3 };           // written by a replan's last evaluation, read by the next replan's first

struct ramp_ctx {
  ramp_config cfg{};
  int device = 0;
  DevArena arena;
  std::unordered_map<std::string, std::pair<float*, std::vector<int64_t>>> raw;   // device copies
  bool finalized = false;
  std::vector<int> chan;       // channels per level
  std::vector<RTB> rtbs;       // order: downs (2/level), mid1, mid2, ups (2/level)
  std::vector<ST> sts;         // order: downs, mid, ups
  std::vector<Resample> downs, ups;
  ConvW final_conv; float *fin_g = nullptr, *fin_b = nullptr, *fin_w = nullptr, *fin_bias = nullptr;
  float *a_fin_c = nullptr, *a_fin_st = nullptr, *a_fin_a = nullptr, *a_fin_da = nullptr;
  // shared temporaries
  float *t_res = nullptr, *t_xn = nullptr, *t_ln = nullptr, *t_o = nullptr, *t_hg = nullptr;
  float *t_dag = nullptr, *t_dqkv = nullptr, *t_dln = nullptr, *t_dz = nullptr, *t_dz1 = nullptr;
  float *g_a = nullptr, *g_b = nullptr, *g_t1 = nullptr, *g_t2 = nullptr, *g_tr = nullptr;
  std::vector<float*> skip_grad;   // per level
  // time table / scene
  float* time_table = nullptr; int tt_stride = 0, tt_T = 0; float* time_temb = nullptr;
  float* cross_bias = nullptr; int n_variants = 0; int* row_variant = nullptr; int row_variant_cap = 0;
  int cross_bias_cap = 0;            // variants the cross_bias allocation holds (n_variants: the ones the current scene table uses)
  int rv_rows = 0;                   // > 0: the row -> variant table is an EXPLICIT one of that many rows (ramp_set_scenes); 0: a cyclic pattern over the whole capacity
  unsigned scene_epoch = 0;          // identity of the scene table: counts ramp_set_scene / ramp_set_scenes calls
  int n_blocks_total = 0;
  // device pointer tables for setup kernels
  void* d_ptr_tables = nullptr;
  // sampler state
  float *s_x = nullptr, *s_eps = nullptr, *s_mean = nullptr, *s_x0 = nullptr, *s_noise = nullptr, *s_chain = nullptr;
  size_t s_cap_B = 0, s_eps_cap = 0, s_noise_cap = 0, s_chain_cap = 0;      // s_cap_B in trajectories (s_x, s_mean, s_x0), every other capacity in elements
  unsigned long long* s_philox = nullptr;      // device {seed, offset} of a job that draws its own noise (ramp_sample_params.noise_mode 1)
  int* s_hard_idx = nullptr; float* s_hard_val = nullptr; size_t s_hard_val_cap = 0; float* s_window = nullptr;
  float* s_cloud = nullptr; size_t s_cloud_cap = 0;
  int *s_traj_scene = nullptr, *s_scene_off = nullptr; size_t s_traj_scene_cap = 0, s_scene_off_cap = 0;      // per-scene APF of ramp_sample_scenes
  // ramp_sample_composed: the job's (B, n_rp) guidance weights, copied here before the launch (the captured graph reads this buffer, so the
  // weights are data of a replay); g_weight_cur is non-null only while that job's evaluations are being launched or captured -- the
  // shared-prefix backward and the guidance step then take a trajectory's weights from its line instead of the host scalars
  float* g_weight = nullptr; size_t g_weight_cap = 0; const float* g_weight_cur = nullptr;
  // energies E = 1/2 ||f||^2 of an evaluation (ramp_score_energy, the MALA steps of ramp_sample_mcmc): e_rows_cur is non-null only while such
  // an evaluation is being launched or captured -- score_all then adds the energy of every row of a chunk to e_rows_cur[row] (the chunk's f
  // goes to the caller's f_out, or to m_f).  Nothing of this is allocated or launched by a job that asks for no energy.
  double* e_rows_cur = nullptr;
  float* m_f = nullptr; size_t m_f_cap = 0;                  // f of all rows (rows, H, S) where the caller gives no f_out
  double* m_Erows = nullptr; size_t m_Erows_cap = 0;         // per-row energies (rows)
  // Langevin refinement inside a sampling job (ramp_sample_mcmc): proposal, cached combined gradient at the state and at the proposal, their
  // combined energies (MALA), the inner steps' normals (sum K, B, H, S), uniforms (sum K, B) and accept flags (sum K, B).  The step sizes
  // are kernel arguments, hence part of the graph key: a job with other step sizes is captured anew
  float *m_xp = nullptr, *m_eps = nullptr, *m_eps_p = nullptr; size_t m_cap_B = 0;
  double *m_E = nullptr, *m_Ep = nullptr; size_t m_E_cap = 0;
  float *m_noise = nullptr, *m_u = nullptr; int* m_flag = nullptr; size_t m_noise_cap = 0, m_u_cap = 0;
  // cost-gradient guidance inside a sampling job (ramp_sample_guided): the guide's own clouds (sum P, point_dim) and their offsets (n_scenes + 1),
  // copied here before the launch -- the captured graph reads these buffers, so the clouds' contents are data of a replay.  The iteration
  // counts, step sizes and the five scalars are kernel arguments, hence part of the graph key
  float* cg_cloud = nullptr; size_t cg_cloud_cap = 0; int* cg_off = nullptr; size_t cg_off_cap = 0;
  // its swept box and sphere terms (ramp_sample_guided_prims): centres, sizes / radii and the two offset tables, copied here before the launch
  // like the clouds -- data of a replay.  The counts, n_sub, margin, band and w_prim are kernel arguments, hence part of the graph key
  float* pg_boxc = nullptr; size_t pg_boxc_cap = 0; float* pg_boxs = nullptr; size_t pg_boxs_cap = 0;
  float* pg_sphc = nullptr; size_t pg_sphc_cap = 0; float* pg_sphr = nullptr; size_t pg_sphr_cap = 0;
  int* pg_boff = nullptr; size_t pg_boff_cap = 0; int* pg_soff = nullptr; size_t pg_soff_cap = 0;
  // resampling inside a sampling job (ramp_sample_steered): per trajectory {logw | c_prev | cum | tmp} (4 B doubles) and the cost terms (3 B), the
  // gather's second buffer, and per event the ancestors, ESS, costs and uniforms; the group table, the uniforms (noise_mode 0) and the potential's
  // clouds are copied here before the launch -- data of a replay.  Flags, lambda, ess_frac and the potential's scalars are in the graph key
  double* rs_state = nullptr; size_t rs_state_cap = 0; double* rs_terms = nullptr; size_t rs_terms_cap = 0;
  float* rs_xtmp = nullptr; size_t rs_xtmp_cap = 0;
  int* rs_anc = nullptr; size_t rs_anc_cap = 0; double* rs_ess = nullptr; size_t rs_ess_cap = 0; double* rs_cost = nullptr; size_t rs_cost_cap = 0;
  float* rs_u = nullptr; size_t rs_u_cap = 0; int* rs_gf = nullptr; size_t rs_gf_cap = 0;
  float* rs_cloud = nullptr; size_t rs_cloud_cap = 0; int* rs_off = nullptr; size_t rs_off_cap = 0;
  // stitched windows inside a sampling job (ramp_sample_stitched): {alpha | zeros} (2 O floats; the zeros are the noise stitch's table) and the
  // pin values (n_pin, C, S), copied here before the launch -- data of a replay.  Windows, overlap, n_pin and the pin indices are kernel
  // arguments, hence part of the graph key
  float* st_alpha = nullptr; size_t st_alpha_cap = 0; float* st_pin_val = nullptr; size_t st_pin_val_cap = 0;
  // warm-started jobs (ramp_sample_warm): the rows' priors (B, H, S), {j0 | has_prior} (2 B int32) and {sa | s1a} (2 B floats), copied here
  // before the launch -- data of a replay: levels and priors are not in the graph key -- and x_init (B, H, S), which the job itself writes and
  // the holds read (it exists only for a job with n_hold > 0; n_hold is in the key)
  float* w_prior = nullptr; size_t w_prior_cap = 0; int* w_tab = nullptr; size_t w_tab_cap = 0; float* w_coef = nullptr; size_t w_coef_cap = 0;
  float* w_xinit = nullptr; size_t w_xinit_cap = 0;
  // graph cache: five slots, every one captured and replayed by replay() and released by drop_graphs().  s_graph belongs to graph_key (the job
  // shape): [0] the job whose first evaluation calibrates itself, [1] the steady job, [2] the repeat of a flagged job (graph_rerun_key).
  hipGraphExec_t s_graph[3] = {nullptr, nullptr, nullptr}; std::string graph_key, graph_rerun_key;
  bool buffers_moved = false;        // grow() gave a buffer a captured node may hold a new address: staging_done() drops BOTH families' keys
  // Round 6: a job the range guard flagged is repeated IN fp16x3 (ramp_set_fallback(ctx, 2)): the guard's state after every evaluation of a
  // job is logged on the device (trip_log[j]), ramp_range_status finds the first flagged evaluation, and the repeat runs exactly that
  // evaluation as a calibrating one (bf16x6 kernels that record every call site's operand maximum: range-free, and its successor is scaled
  // from maxima that are true) -- a function of the job alone, 1.03 x a steady job instead of the 1.83 x of an all-bf16x6 repeat
  int* trip_log = nullptr; size_t trip_log_cap = 0; int last_job_steps = 0; int trip_eval = -1; int trip_site = -1; int rerun = 0;
  // Round 5: the calibration a job's first evaluation is scaled from is CANONICAL -- one bf16x6 evaluation, outside the job, on Philox noise of
  // a fixed seed with NO hard conditions applied, at the job's first timestep (TABLE_CANONICAL) -- instead of whatever the previous job left
  // behind: no job contains a bf16x6 evaluation, and a job's result does not depend on what ran before it on the context.
  // ramp_set_calibration_reuse(ctx, 0) turns it off: every job's first evaluation then calibrates itself.
  int cal_reuse = 1;
  bool c_cal_valid = false; std::string c_cal_key; unsigned long long* c_cal_rec = nullptr;
  std::map<std::string, float*> c_cal_saved;     // canonical tables already computed, by key: switching between job shapes copies 4 KB instead of re-evaluating
  std::vector<float*> c_cal_free;                // their buffers after an invalidation (scene / plan change), for reuse
  // receding-horizon replanning: ONE job, the replan of E episodes in lock-step (ramp_replan_episodes); ramp_replan is its one-episode
  // case.  Fixed device buffers the captured graphs read -- per row (e_cap_B rows), per episode (e_cap_E episodes) and the episodes'
  // concatenated clouds (in points; e_extra is staging only) --, the graph of a replan whose first evaluation calibrates ([0]) and of one
  // that continues from the previous replan's operand maxima ([1], TABLE_REPLAN_CARRY), and their key.  e_best_E: the episode count e_best
  // holds winners (or plans) for
  float *e_noise = nullptr, *e_hist = nullptr, *e_xclean = nullptr, *e_best = nullptr, *e_plen = nullptr, *e_smooth = nullptr,
        *e_cost = nullptr, *e_extra = nullptr, *e_hard_val = nullptr;
  double *e_static = nullptr, *e_dyn = nullptr;
  int *e_mask = nullptr, *e_en = nullptr, *e_result = nullptr, *e_hard_idx = nullptr, *e_row_ep = nullptr, *e_first = nullptr,
      *e_static_off = nullptr, *e_cost_off = nullptr;
  EpisodeState* e_state = nullptr;
  size_t e_cap_B = 0, e_cap_E = 0, e_cap_static = 0, e_cap_dyn = 0, e_cap_cost = 0, e_cap_extra = 0; int e_best_E = 0;
  hipGraphExec_t e_graph[2] = {nullptr, nullptr}; std::string e_key;
  // which entry ran the previous replan (whose winners e_best holds: x_clean == NULL continues the same entry's only), and which one's
  // operand maxima TABLE_REPLAN_CARRY holds (a call of the other entry, or after an invalidation, calibrates)
  enum ReplanEntry { REPLAN_NOBODY = 0, REPLAN_SINGLE, REPLAN_EPISODES };
  ReplanEntry replan_last = REPLAN_NOBODY, replan_carry = REPLAN_NOBODY;
  // cost guidance inside the replans (ramp_replan_guided, ramp_replan_episodes_guided): the static guide clouds (sum P, 2), their offsets
  // (n_scenes + 1), the moving clouds (n_scenes, n_mov, 2) and their tracks (n_scenes, H, 2), copied here before the launch -- data of a replay
  // -- and the tap (2, B, H, S).  Scalars, counts, step sizes, n_mov, the clouds' total and the tap's presence are in the graph key
  float *rg_cloud = nullptr, *rg_mov = nullptr, *rg_track = nullptr, *rg_tap = nullptr; int* rg_off = nullptr;
  size_t rg_cloud_cap = 0, rg_mov_cap = 0, rg_track_cap = 0, rg_tap_cap = 0, rg_off_cap = 0;
  // scene-encoder scratch
  float* scene_ws = nullptr; size_t scene_ws_cap = 0;
  int* enc_tab = nullptr; size_t enc_tab_cap = 0;      // ramp_encode_scenes: the pass-local CSR and tile tables of every pass of the call
  // bf16x6 weight planes: fp32 weight base pointer -> (planes, element count)
  int gemm_mode = 0;                 // 0 = exact fp32 MFMA, 1 = bf16x6 split on the bf16 matrix cores, 2 = fp16x3 split with delayed operand scaling
                                     // (evaluations in phase 2; its calibration evaluations, phase 1, run the bf16x6 kernels): the default build
  struct X6W { unsigned short* planes; size_t n; int K; unsigned short* packed; unsigned short* packed3; float w_scale_inv; };
  std::map<const float*, X6W> x6;
  int x6_pipe = 1;                   // 1 = fragment-packed weights + pipelined kernel (RAMP_X6_PIPE=0: LDS-staged weights)
  int geglu_group = 64;              // GEGLU weight tiling (32 with the pipelined kernels' wave-private epilogue)
  // fp16x3 (gemm_mode 2): delayed operand scaling.  phase 0 = bf16x6; 1 = bf16x6 that records max|A| per GEMM call site
  // (a calibration evaluation: the canonical one outside the sampling jobs, the first evaluation of a job with calibration reuse off, the
  // flagged evaluation of a repeat, the first replan / single evaluation after a change); 2 = fp16x3 scaled from the
  // previous evaluation's maxima, recording its own.  obs[N_OBS_TABLES][MAX_SITES] floats; an evaluation reads one table and writes another
  // (the roles: TABLE_EVEN ... TABLE_REPLAN_CARRY above).
  static constexpr int MAX_SITES = 1024, N_OBS_TABLES = 4;
  float* table(int i) const { return obs + (size_t)i * MAX_SITES; }
  int phase = 0, site = 0;
  int ff_fused = 150000;             // fp16x3 evaluations: FF1 -> GEGLU -> FF2 as one launch for M >= this many rows
                                     // (RAMP_FF_FUSED: 0 never, 1 always, n > 1 that threshold)
  int three_blocks = 1;              // launch plan: third resident block for the bias-only linears
  int mfma16 = 1;                    // launch plan: the token-owning fused feed-forward on v_mfma_f32_16x16x32_f16 (ffx16.hip; 0: the 32x32x16 kernels of
                                     // ffx.hip) -- the shape that holds the higher clock under the power cap (RAMP_MFMA16)
  int ffx_min_rows = 32768;          // fp16x3 evaluations: feed-forward pairs with at least this many tokens run the token-owning fused
                                     // kernels of ffx.hip, forward and backward (RAMP_FFX: 0 never, n that threshold)
  int tkl_min_rows = 65536;          // fp16x3 evaluations: K = 256 transformer linears (LN1 -> QKV, out-proj, d(o)) with at least this many
                                     // tokens run the token-owning kernel of tkl.hip (RAMP_TKL: 0 never, n that threshold)
  int atk_min_rows = 40000;          // fp16x3 evaluations: self-attention + output projection as one launch of sample-owning waves (atk.hip)
                                     // from this many tokens where the level's token count divides 48 or 32 (RAMP_ATK: 0 never, n that threshold)
  int tkc_gn = 3;                    // ... and the GroupNorm + Mish of their Conv1dBlock inside the same launch: bit 0 forward (epilogue), bit 1 input
                                     // gradient (operand); RAMP_TKC_GN=0: separate gn kernels
  int tkc_min_rows = 16384;          // fp16x3 evaluations: the k = 5 convolutions with C_in, C_out in {32, 64} as sample-owning waves (tkc.hip) from this
                                     // many tokens, on levels whose token count (>= 8) divides 48 or 32 (RAMP_TKC: 0 never, n that threshold)
  int tkw_min_rows = 16384;          // fp16x3 evaluations: the k = 5 convolutions with C_out in {128, 256, 512} with GroupNorm + Mish fused around them as
                                     // sample-owning blocks (tkw.hip) from this many tokens, on levels whose token count (>= 3) divides 96 (RAMP_TKW)
  std::map<const float*, unsigned short*> tk16_w;          // K = 256 linear weight (fp32 base pointer) -> its 16 x 32 fragment planes (tkl16.hip; scale = the tile kernels' planes')
  struct TkcW { unsigned short* planes; float wsi; };
  std::map<const float*, TkcW> tkc_w;                       // fp32 conv weight [5][N][K] -> its tkc planes
  int share_prefix = 1;              // sampling jobs: rows of one trajectory share the network prefix (RAMP_SHARE_PREFIX=0: off)
  int force_x6 = 0;                  // ramp_set_fallback: run ramp_sample entirely in bf16x6 although the mode is fp16x3
  // single evaluations (ramp_score): the tables of the last evaluation stay valid as the next one's calibration
  bool score_calibrated = false; bool score_calibrated_bwd = false; int score_parity = 0; int score_last_mode = 0;
  // ramp_score_rows: the row -> timestep table of the call (device, its entries range-checked on the host); t_rows_cur is non-null only
  // while that call's evaluations are being launched -- rtb_forward hands it, offset by the chunk's first row, to the time-bias consumers
  int* t_rows_dev = nullptr; size_t t_rows_cap = 0; const int* t_rows_cur = nullptr;
  float* obs = nullptr; float *obs_in = nullptr, *obs_out = nullptr;
  int* range_flag = nullptr;
  // debug
  std::map<std::string, std::pair<float*, size_t>> dbg;
  int64_t launches = 0;
  // per-launch HIP-event profiler (eager mode only): category, algorithmic flops, start/stop events
  bool prof_on = false, prof_dump = false; int ffx_ablate = 0; bool tklb_off = false; bool abl_on = true;
  std::vector<hipEvent_t> prof_ev; size_t prof_used = 0;
  std::vector<int> prof_cat; std::vector<double> prof_flops; std::vector<std::array<int, 4>> prof_shape;
};

enum { CAT_GEMM = 0, CAT_ATTN = 1, CAT_ROW = 2, CAT_SMALLCONV = 3, CAT_SAMPLER = 4, CAT_N = 5 };

static void prof_pre(ramp_ctx* c, hipStream_t s, int cat, double flops, std::array<int, 4> shape = {0, 0, 0, 0}) {
  if (!c->prof_on) return;
  c->prof_shape.push_back(shape);
  if (c->prof_used + 2 > c->prof_ev.size()) {
    const size_t old = c->prof_ev.size();
    c->prof_ev.resize(old + 4096);
    for (size_t i = old; i < c->prof_ev.size(); ++i) (void)hipEventCreate(&c->prof_ev[i]);
  }
  c->prof_cat.push_back(cat); c->prof_flops.push_back(flops);
  (void)hipEventRecord(c->prof_ev[c->prof_used++], s);
}
static void prof_post(ramp_ctx* c, hipStream_t s) {
  if (!c->prof_on) return;
  (void)hipEventRecord(c->prof_ev[c->prof_used++], s);
}
// One kernel launch with launch counting and optional event bracketing: fn() launches and returns the launch's code.  Whatever else can fail
// (weight-plane lookup, call-site budget) is done BEFORE this, so that a profile holds whole start / stop pairs whatever happens.
template <class F> static int bracket(ramp_ctx* c, hipStream_t s, int cat, double flops, std::array<int, 4> shape, F&& fn) {
  prof_pre(c, s, cat, flops, shape);
  const int rc = fn();
  prof_post(c, s);
  c->launches++;
  return rc;
}
// ... of a launch expression without a shape tag, returning from the caller if it fails
#define LAUNCH(ctx_, stream_, cat_, flops_, expr_) \
  CK(bracket((ctx_), (stream_), (cat_), (double)(flops_), {0, 0, 0, 0}, [&] { return (expr_); }))

namespace {


int dev_alloc(ramp_ctx* c, float** out, size_t n) {
  *out = c->arena.alloc(n);
  RAMP_REQUIRE(*out != nullptr, "hipMalloc failed for " + std::to_string(n * 4) + " bytes");
  return 0;
}

int get_raw(ramp_ctx* c, const std::string& key, std::initializer_list<int64_t> shape, float** out) {
  auto it = c->raw.find(key);
  RAMP_REQUIRE(it != c->raw.end(), "missing weight '" + key + "'");
  std::vector<int64_t> want(shape);
  RAMP_REQUIRE(it->second.second == want, "weight '" + key + "' has the wrong shape");
  *out = it->second.first;
  return 0;
}

int permute3(ramp_ctx* c, const float* in, int D0, int D1, int D2, int p0, int p1, int p2, float** out) {
  CK(dev_alloc(c, out, (size_t)D0 * D1 * D2));
  hipLaunchKernelGGL(permute3_kernel, dim3(std::min<long>(((long)D0 * D1 * D2 + 255) / 256, 4096)), dim3(256), 0, 0,
                     in, *out, D0, D1, D2, p0, p1, p2);
  RAMP_HIP_CHECK(hipGetLastError());
  return 0;
}

int pack_conv5(ramp_ctx* c, const std::string& prefix, int cin, int cout, ConvW* w) {
  float* raw; float* b;
  CK(get_raw(c, prefix + ".weight", {cout, cin, 5}, &raw));
  CK(get_raw(c, prefix + ".bias", {cout}, &b));
  w->cin = cin; w->cout = cout; w->bias = b;
  CK(permute3(c, raw, cout, cin, 5, 2, 0, 1, &w->fwd));   // [5][Cout][Cin]
  CK(permute3(c, raw, cout, cin, 5, 2, 1, 0, &w->bwd));   // [5][Cin][Cout]
  return 0;
}

int pack_linear(ramp_ctx* c, const std::string& key, int n, int k, bool conv1, float** fwd, float** bwd) {
  float* raw;
  if (conv1) CK(get_raw(c, key, {n, k, 1}, &raw)); else CK(get_raw(c, key, {n, k}, &raw));
  *fwd = raw;
  CK(permute3(c, raw, n, k, 1, 1, 0, 2, bwd));            // [K][N]
  return 0;
}

int build_rtb(ramp_ctx* c, RTB& r) {
  const std::string& n = r.name;
  if (r.first) {
    float* raw;
    CK(get_raw(c, n + ".blocks.0.block.0.weight", {r.cout, r.cin, 5}, &raw));
    CK(get_raw(c, n + ".blocks.0.block.0.bias", {r.cout}, &r.c1.bias));
    CK(permute3(c, raw, r.cout, r.cin, 5, 2, 1, 0, &r.w5in));            // [5][S][C0]
    CK(get_raw(c, n + ".residual_conv.weight", {r.cout, r.cin, 1}, &raw));
    CK(permute3(c, raw, r.cout, r.cin, 1, 2, 1, 0, &r.w1in));            // [1][S][C0]
    CK(get_raw(c, n + ".residual_conv.bias", {r.cout}, &r.res_bias));
    r.c1.cin = r.cin; r.c1.cout = r.cout;
  } else {
    CK(pack_conv5(c, n + ".blocks.0.block.0", r.cin, r.cout, &r.c1));
    if (r.has_res) {
      CK(pack_linear(c, n + ".residual_conv.weight", r.cout, r.cin, true, &r.res_f, &r.res_b));
      CK(get_raw(c, n + ".residual_conv.bias", {r.cout}, &r.res_bias));
    }
  }
  CK(pack_conv5(c, n + ".blocks.1.block.0", r.cout, r.cout, &r.c2));
  CK(get_raw(c, n + ".blocks.0.block.2.weight", {r.cout}, &r.g1));
  CK(get_raw(c, n + ".blocks.0.block.2.bias", {r.cout}, &r.b1));
  CK(get_raw(c, n + ".blocks.1.block.2.weight", {r.cout}, &r.g2));
  CK(get_raw(c, n + ".blocks.1.block.2.bias", {r.cout}, &r.b2));
  const size_t cap = (size_t)c->cfg.max_rows, lc = (size_t)r.L * r.cout;
  CK(dev_alloc(c, &r.a_c1, cap * lc)); CK(dev_alloc(c, &r.a_st1, cap * 16));
  CK(dev_alloc(c, &r.a_h, cap * lc));  CK(dev_alloc(c, &r.a_c2, cap * lc));
  CK(dev_alloc(c, &r.a_st2, cap * 16)); CK(dev_alloc(c, &r.a_out, cap * lc));
  return 0;
}

int build_st(ramp_ctx* c, ST& s) {
  const std::string& n = s.name;
  const int D = 256, ctx = c->cfg.context_dim;
  CK(get_raw(c, n + ".norm.weight", {s.C}, &s.gn_g));
  CK(get_raw(c, n + ".norm.bias", {s.C}, &s.gn_b));
  CK(pack_linear(c, n + ".proj_in.weight", D, s.C, true, &s.wpi_f, &s.wpi_b));
  CK(get_raw(c, n + ".proj_in.bias", {D}, &s.bpi));
  CK(pack_linear(c, n + ".proj_out.weight", s.C, D, true, &s.wpo_f, &s.wpo_b));
  CK(get_raw(c, n + ".proj_out.bias", {s.C}, &s.bpo));
  const size_t cap = (size_t)c->cfg.max_rows, tok = cap * s.L;
  CK(dev_alloc(c, &s.a_gst, cap * 16)); CK(dev_alloc(c, &s.a_z0, tok * D)); CK(dev_alloc(c, &s.a_y, cap * s.L * s.C));
  for (int b = 0; b < 2; ++b) {
    STBlock& k = s.blk[b];
    const std::string t = n + ".transformer_blocks." + std::to_string(b);
    float *q, *kk, *v;
    CK(get_raw(c, t + ".attn1.to_q.weight", {D, D}, &q));
    CK(get_raw(c, t + ".attn1.to_k.weight", {D, D}, &kk));
    CK(get_raw(c, t + ".attn1.to_v.weight", {D, D}, &v));
    CK(dev_alloc(c, &k.wqkv_f, 3 * D * D));
    RAMP_HIP_CHECK(hipMemcpy(k.wqkv_f, q, D * D * 4, hipMemcpyDeviceToDevice));
    RAMP_HIP_CHECK(hipMemcpy(k.wqkv_f + D * D, kk, D * D * 4, hipMemcpyDeviceToDevice));
    RAMP_HIP_CHECK(hipMemcpy(k.wqkv_f + 2 * D * D, v, D * D * 4, hipMemcpyDeviceToDevice));
    CK(permute3(c, k.wqkv_f, 3 * D, D, 1, 1, 0, 2, &k.wqkv_b));      // [256][768]
    CK(pack_linear(c, t + ".attn1.to_out.0.weight", D, D, false, &k.wo_f, &k.wo_b));
    CK(get_raw(c, t + ".attn1.to_out.0.bias", {D}, &k.bo));
    CK(pack_linear(c, t + ".ff.net.0.proj.weight", 2048, D, false, &k.w1_f, &k.w1_b));
    CK(get_raw(c, t + ".ff.net.0.proj.bias", {2048}, &k.b1));
    CK(dev_alloc(c, &k.w1_pk, 2048 * D)); CK(dev_alloc(c, &k.b1_pk, 2048));
    hipLaunchKernelGGL(geglu_pack_kernel, dim3(1024), dim3(256), 0, 0, k.w1_f, k.w1_pk, 1024, D, c->geglu_group);
    hipLaunchKernelGGL(geglu_pack_kernel, dim3(8), dim3(256), 0, 0, k.b1, k.b1_pk, 1024, 1, c->geglu_group);
    RAMP_HIP_CHECK(hipGetLastError());
    CK(pack_linear(c, t + ".ff.net.2.weight", D, 1024, false, &k.w2_f, &k.w2_b));
    CK(get_raw(c, t + ".ff.net.2.bias", {D}, &k.b2));
    CK(get_raw(c, t + ".norm1.weight", {D}, &k.ln1_g)); CK(get_raw(c, t + ".norm1.bias", {D}, &k.ln1_b));
    CK(get_raw(c, t + ".norm3.weight", {D}, &k.ln3_g)); CK(get_raw(c, t + ".norm3.bias", {D}, &k.ln3_b));
    float* tmp;
    CK(get_raw(c, t + ".attn2.to_v.weight", {D, ctx}, &tmp)); k.wv2 = tmp;
    CK(get_raw(c, t + ".attn2.to_out.0.weight", {D, D}, &tmp)); k.wo2 = tmp;
    CK(get_raw(c, t + ".attn2.to_out.0.bias", {D}, &tmp)); k.bo2 = tmp;
    // attn2.to_q / to_k / norm2 only feed a softmax over a single key (== 1): checked present, unused
    CK(get_raw(c, t + ".attn2.to_q.weight", {D, D}, &tmp));
    CK(get_raw(c, t + ".attn2.to_k.weight", {D, ctx}, &tmp));
    CK(get_raw(c, t + ".norm2.weight", {D}, &tmp)); CK(get_raw(c, t + ".norm2.bias", {D}, &tmp));
    CK(dev_alloc(c, &k.a_qkv, tok * 768)); CK(dev_alloc(c, &k.a_z1, tok * D));
    CK(dev_alloc(c, &k.a_ag, (tok + 127) * 2048)); CK(dev_alloc(c, &k.a_z2, tok * D));     // (+ 127: ffx.hip stashes whole 128-token tiles)
  }
  return 0;
}

// ---- routing: which kernel serves each product of a score evaluation ---------------------------
// One GEMM call site of the fp16x3 delayed scaling: where the operand's maximum of the previous evaluation is read and this evaluation's is
// recorded, the weight's scale, the site's number (what the range guard reports) and the guard's word.  Run::take_site fills it.
struct Site { const float* in = nullptr; float* out = nullptr; float wsi = 1.f; int id = 0; int* flag = nullptr; };
template <class A> void attach(A& t, const Site& v) { t.amax_in = v.in; t.amax_out = v.out; t.wsi = v.wsi; t.site = v.id; t.range_flag = v.flag; }
// the fused feed-forward's two sites, in the order of the launches it replaces (forward: FF1, FF2; backward: d(hg), FF1-dX); one guard word
void attach(FfxArgs& f, const Site& v1, const Site& v2) {
  f.amax_in1 = v1.in; f.amax_out1 = v1.out; f.wsi1 = v1.wsi; f.site1 = v1.id;
  f.amax_in2 = v2.in; f.amax_out2 = v2.out; f.wsi2 = v2.wsi; f.site2 = v2.id;
  f.range_flag = v1.flag;
}

struct Run {
  ramp_ctx* c; hipStream_t s; int R; int row0;
  template <class F> int launch(int cat, double flops, std::array<int, 4> shape, F&& fn) { return bracket(c, s, cat, flops, shape, fn); }

  // ---- weight planes and call sites ----
  // the split-precision planes of the packed weight W points into (ramp_ctx::x6) and W's offset inside it, or nothing
  struct Planes { const ramp_ctx::X6W* e = nullptr; size_t off = 0; };
  Planes planes(const float* W) const {
    auto it = c->x6.upper_bound(W);
    if (it == c->x6.begin()) return {};
    --it;
    if (!(W >= it->first && W < it->first + it->second.n)) return {};
    return {&it->second, (size_t)(W - it->first)};
  }
  // ... hold W [N][K] in the 32-row fragments the pipelined kernels stream: the bf16 ones, and (h3) the fp16 ones of the fp16x3 evaluations too
  bool fragments(const Planes& p, int N, int K, bool h3) const {
    return c->x6_pipe && p.e && p.e->packed && (!h3 || p.e->packed3) && p.e->K == K && p.off % (32ul * K) == 0 && N % 32 == 0;
  }
  bool has_h3(const float* W, int N, int K) const { return fragments(planes(W), N, K, true); }
  // the products that run on weight planes at all: not in exact-fp32 mode, not the narrow outputs, not K = 16 (the narrow exact-fp32 kernel)
  bool on_planes(int N, int K) const { return c->gemm_mode >= 1 && (N >= 128 || (c->x6_pipe && N >= 64)) && K % 32 == 0; }
  // The next call site.  The ONLY place a site is numbered: every evaluation of a job must number its sites alike, whichever kernels
  // serve them, because an evaluation is scaled from the maxima its predecessor recorded under the same numbers.  By phase: 2 reads the
  // delayed scale and arms the guard (which judges the delayed scale); 1 (calibration: unscaled operands) only records; 0 numbers, nothing else.
  int take_site(float wsi, Site* v) {
    RAMP_REQUIRE(c->site < ramp_ctx::MAX_SITES, "too many GEMM call sites for the scale table");
    const bool scaled = c->phase == 2;
    *v = Site{scaled ? c->obs_in + c->site : nullptr, c->phase >= 1 ? c->obs_out + c->site : nullptr, wsi, c->site, scaled ? c->range_flag : nullptr};
    c->site++;
    return 0;
  }
  // ... of a token- or sample-owning launch on the weight W [N][K], with W's fp16 fragment planes: the site, planes and scale prep() attaches
  // to the tile launch it replaces (same operand, same maxima)
  int h3_site(const char* who, const float* W, int N, int K, const unsigned short** Wx, Site* v) {
    const Planes p = planes(W);
    RAMP_REQUIRE(on_planes(N, K) && fragments(p, N, K, true), std::string(who) + ": weight without fp16 fragment planes (its use_* predicate must have been checked)");
    if (Wx) *Wx = p.e->packed3 + 2 * p.off;
    return take_site(p.e->w_scale_inv, v);
  }
  // attach the split-precision weight planes and the delayed-scaling slots of the next call site to a tile launch; returns 2 when the launch
  // will run the fp16x3 fragment kernels, 1 for bf16x6 fragments, 0 otherwise (< 0: error).  Only fragment launches take a site.
  int prep(GemmArgs& b) {
    if (!on_planes(b.N, b.K)) return 0;
    const Planes p = planes(b.W);
    if (!p.e) return 0;
    if (!fragments(p, b.N, b.K, false)) { b.Wx = p.e->planes + p.off; b.wx_plane = (long)p.e->n; return 0; }
    Site v;
    CK(take_site(p.e->w_scale_inv, &v));
    if (c->phase == 2 && p.e->packed3) {
      b.Wx = p.e->packed3 + 2 * p.off; b.wx_packed = 2; b.w_scale_inv = v.wsi;
      b.a_absmax_in = v.in; b.a_absmax_out = v.out; b.range_flag = v.flag; b.site_id = v.id;
      return 2;
    }
    b.Wx = p.e->packed + 3 * p.off; b.wx_packed = 1; b.a_absmax_out = v.out;      // bf16x6 fragments: unscaled, unguarded; the maximum recorded in phases >= 1
    return 1;
  }

  // ---- the fast-path predicates ----
  // A family serves a product when the evaluation is steady() (tkc: or the calibration one), the launch has at least the family's row
  // threshold (ramp_launch_plan; 0 = never), the family's shape rule holds and the planes it streams exist (h3 = has_h3 of the weight):
  //   family       threshold                  shape rule                                                                        phases
  //   ff_fwd       ff_fused                   FF1 -> GEGLU -> FF2 forward, both weights h3 (gemm.hip)                             2
  //   ffx / ffx16  ffx_min_rows               a feed-forward pair, forward and backward; STBlock::ffx_f                          2
  //   tkl / tkl16  tkl_min_rows               K = lda = 256, one tap, N % 32 == 0, N <= 768, no second operand / output; h3       2
  //   tklb         tkl_min_rows               d(ln1) + LN1 backward: W [256][768] h3; not tklb_off                                2
  //   ato, atb     atk_min_rows               ato_applicable (atk.hip): L divides 48 or 32; ato: STBlock::ato_w                   2
  //   abl          atk_min_rows               atb's rule, STBlock::abl_w, wqkv_b h3; abl_on, not tklb_off, tkl_min_rows > 0       2
  //   tkc          tkc_min_rows               plain k = 5 conv, tkc_applicable (tkc.hip), 32-bit row offsets; ramp_ctx::tkc_w     1, 2
  //   tkw          tkw_min_rows               plain k = 5 conv + its GroupNorm, tkw_applicable (tkw.hip); h3                      2
  // No predicate tests force_x6: phase is non-zero only where the caller has established gemm_mode == 2 && !force_x6 first (ramp_score,
  // sample_body, replan_body, and the steady jobs' canonical_calibration), and replan_job raises force_x6 only around a phase-0 repeat --
  // so the !force_x6 that tkc_planes and use_tkw used to carry was implied by their phase test.
  bool steady() const { return c->gemm_mode == 2 && c->phase == 2 && c->x6_pipe; }
  static bool from(int min_rows, int M) { return min_rows > 0 && M >= min_rows; }
  static bool plain_conv5(const GemmArgs& a) {
    return a.taps == 5 && !a.Amul && !a.rowbias && a.epi == EPI_LINEAR && a.a_stride == 1 && a.c_rstride == 1 && a.c_roff == 0 &&
           ((a.shift0 == -2 && a.shift_step == 1) || (a.shift0 == 2 && a.shift_step == -1));
  }
  // a k = 5 convolution with C_in, C_out in {32, 64} on the sample-owning kernel (tkc.hip): in the calibration evaluation too (unscaled
  // operand, maximum recorded), so that the call sites number the same in every fp16x3 evaluation of a job
  const ramp_ctx::TkcW* tkc_planes(const GemmArgs& a) const {
    const bool calibrating = c->gemm_mode == 2 && c->phase == 1 && c->x6_pipe;
    if (!(from(c->tkc_min_rows, a.M) && (steady() || calibrating) && plain_conv5(a) && !a.A2 && !a.C2)) return nullptr;
    if (!tkc_applicable(a.M, a.L, a.N, a.K, nullptr)) return nullptr;
    if (!((long)a.M * a.lda * 4 < (1l << 32))) return nullptr;      // (32-bit row offsets: larger launches keep the tile kernels)
    auto it = c->tkc_w.find(a.W);
    return it == c->tkc_w.end() ? nullptr : &it->second;
  }
  // ... with the GroupNorm + Mish of its Conv1dBlock fused like tkw below (epi: behind the forward convolution; else the input gradient's operand)
  const ramp_ctx::TkcW* tkc_gn_planes(const GemmArgs& a, bool epi) const {
    if (!(c->tkc_gn & (epi ? 1 : 2)) || (epi && a.resid2)) return nullptr;
    return tkc_planes(a);
  }
  // a wide k = 5 convolution (forward: C_out in {128, 256, 512}, C_in up to 1024 from two sources; input gradient: outputs up to 1024)
  // with its GroupNorm fused (tkw.hip): forward = GroupNorm + Mish behind it (epi), input gradient = GroupNorm backward folded into the
  // operand (pro); neither with a second operand / output on the fused side
  bool use_tkw(const GemmArgs& a, bool pro, bool epi) const {
    return from(c->tkw_min_rows, a.M) && steady() && plain_conv5(a) && tkw_applicable(a.M, a.L, a.N, a.K, pro, epi) &&
           (!a.A2 || !pro) && (!a.C2 || !epi) && has_h3(a.W, a.N, a.K);
  }
  // the token-owning fused feed-forward (ffx.hip) serves this feed-forward pair, forward AND backward (the stash layout is
  // private to the two kernels, so both directions of an evaluation must agree: same phase, same M)
  bool use_ffx(const STBlock& k, int M) const { return k.ffx_f && from(c->ffx_min_rows, M) && steady(); }
  // a K = 256 linear on the token-owning kernel (tkl.hip); a weight without fp16 fragment planes keeps its launch on the tile kernels
  bool use_tkl(const GemmArgs& a) const {
    return from(c->tkl_min_rows, a.M) && steady() && a.K == 256 && a.lda == 256 && a.taps == 1 && a.N % 32 == 0 && a.N <= 768 && !a.A2 &&
           !a.Amul && !a.resid2 && !a.C2 && a.epi == EPI_LINEAR && has_h3(a.W, a.N, a.K);
  }
  // self-attention + output projection in one launch of sample-owning waves (atk.hip); atb: the attention backward on the same waves
  bool use_atb(int M, int L) const { return from(c->atk_min_rows, M) && steady() && ato_applicable(M, L, nullptr); }
  bool use_ato(const STBlock& k, int M, int L) const { return k.ato_w && use_atb(M, L); }
  // attention backward + d(ln1) + LayerNorm-1 backward in one launch of sample-owning waves (atl.hip), from atk_min_rows tokens on
  bool use_abl(const STBlock& k, int M, int L) const {
    return c->abl_on && k.abl_w && use_atb(M, L) && !c->tklb_off && c->tkl_min_rows > 0 && has_h3(k.wqkv_b, 256, 768);
  }
  // d(ln1) = d(qkv) Wqkv^T and the LayerNorm-1 backward behind it in one token-owning launch (tkl.hip, tklb_kernel)
  bool use_tklb(int M, const float* W) const { return !c->tklb_off && from(c->tkl_min_rows, M) && steady() && has_h3(W, 256, 768); }

  // ---- the launch wrappers: take the call site(s) of the tile launch(es) they replace, then launch ----
  // The GroupNorm around a sample-owning convolution, from the arguments of the launch it absorbs.  pro = the gn_bwd in front of an input
  // gradient: the operand becomes its dy, normalised against the stash pro->x.  epi = the gn_fwd behind a forward convolution: the
  // convolution's own output (t.Y so far) is the stash, the activation (+ time bias, + residual) goes to epi->y.
  template <class T> static void fuse_gn(T& t, const GnBwdArgs* pro, const GnArgs* epi) {
    if (pro) { t.X = pro->dy; t.ldx = pro->C; t.gn_c = pro->x; t.gn_stats = pro->stats; t.gn_gamma = pro->gamma; t.gn_beta = pro->beta; }
    if (epi) {
      t.Cst = t.Y; t.stats = epi->stats; t.gamma = epi->gamma; t.beta = epi->beta; t.tbias = epi->tbias; t.t_rows = epi->t_rows; t.tt_stride = epi->tt_stride; t.eps = epi->eps;
      t.Y = epi->y; t.ldy = epi->C;
      if (epi->resid) { t.resid = epi->resid; t.ldr = epi->C; }
    }
  }
  int tkc(const GemmArgs& a, const ramp_ctx::TkcW& w, const GnBwdArgs* pro = nullptr, const GnArgs* epi = nullptr) {
    Site v;
    CK(take_site(w.wsi, &v));
    TkcArgs t; t.M = a.M; t.L = a.L; t.N = a.N; t.K = a.K; t.dir = a.shift_step; t.X = a.A; t.ldx = a.lda; t.W = w.planes; t.bias = a.bias;
    t.resid = a.resid; t.ldr = a.ldr; t.resid2 = a.resid2; t.ldr2 = a.ldr2; t.Y = a.C; t.ldy = a.ldc;
    attach(t, v); fuse_gn(t, pro, epi);
    return launch(CAT_GEMM, 2.0 * a.M * a.N * a.K * a.taps, {a.M, a.N, a.K, -5}, [&] { return launch_tkc(t, s); });
  }
  int tkw(const GemmArgs& a, const GnBwdArgs* pro, const GnArgs* epi) {
    const unsigned short* Wx; Site v;
    CK(h3_site("tkw", a.W, a.N, a.K, &Wx, &v));
    TkwArgs t; t.M = a.M; t.L = a.L; t.N = a.N; t.K = a.K; t.dir = a.shift_step; t.X = a.A; t.ldx = a.lda; t.X2 = a.A2; t.ldx2 = a.lda2;
    t.K1 = a.A2 ? a.K1 : a.K; t.W = Wx; t.bias = a.bias; t.resid = a.resid; t.ldr = a.ldr; t.resid2 = a.resid2; t.ldr2 = a.ldr2;
    t.Y = a.C; t.ldy = a.ldc; t.Y2 = a.C2; t.ldy2 = a.ldc2; t.N1 = a.C2 ? a.N1 : a.N;
    attach(t, v); fuse_gn(t, pro, epi);
    return launch(CAT_GEMM, 2.0 * a.M * a.N * a.K * 5, {a.M, a.N, a.K, -7}, [&] { return launch_tkw(t, s); });
  }
  // any GEMM-class product: the narrow convolutions on tkc where it applies, else the tile kernels
  int gemm(const GemmArgs& a) {
    if (const ramp_ctx::TkcW* w = tkc_planes(a)) return tkc(a, *w);
    GemmArgs b = a;
    if (a.K % 32 == 0) {      // (else 16-wide operands, unet_input_dim = 16: the exact fp32 narrow kernel, no weight planes, no call site)
      b.three_ok = c->three_blocks;
      const int kind = prep(b);
      if (kind < 0) return kind;
    }
    return launch(CAT_GEMM, 2.0 * a.M * a.N * a.K * a.taps, {a.M, a.N, a.K, a.taps}, [&] { return launch_gemm(b, s); });
  }
  // A k = 5 convolution and the GroupNorm + Mish of its Conv1dBlock.  a = the convolution, writing the stash g.x; g = the gn_fwd that follows
  // it.  One launch on tkw, else on tkc, else the pair.  gn_due: the caller has a launch to put between the pair and launches g itself if told to.
  int conv_gn(const GemmArgs& a, const GnArgs& g, bool* gn_due = nullptr) {
    RAMP_REQUIRE(a.C == g.x, "conv_gn: the convolution must write the GroupNorm's input");
    if (gn_due) *gn_due = false;
    if (use_tkw(a, false, true)) return tkw(a, nullptr, &g);
    if (const ramp_ctx::TkcW* w = tkc_gn_planes(a, true)) return tkc(a, *w, nullptr, &g);
    CK(gemm(a));
    if (gn_due) { *gn_due = true; return 0; }
    return launch(CAT_ROW, 0, {0, 0, 0, 0}, [&] { return launch_gn_fwd(g, s); });
  }
  // The input gradient of that pair.  g = the gn_bwd (into g.dx), a = the transposed convolution reading g.dx.  One launch on tkw or tkc
  // (the GroupNorm backward is the operand staging of the convolution: g.dx is never written), else the pair.
  int gn_conv_bwd(const GnBwdArgs& g, const GemmArgs& a) {
    RAMP_REQUIRE(a.A == g.dx && !g.add, "gn_conv_bwd: the convolution must read the GroupNorm backward's plain result");
    if (use_tkw(a, true, false)) return tkw(a, &g, nullptr);
    if (const ramp_ctx::TkcW* w = tkc_gn_planes(a, false)) return tkc(a, *w, &g, nullptr);
    CK(launch(CAT_ROW, 0, {0, 0, 0, 0}, [&] { return launch_gn_bwd(g, s); }));
    return gemm(a);
  }
  int ffx(const STBlock& k, bool bwd, const float* X, const float* z1, float* Y, int M) {
    Site v1, v2;
    CK(take_site(bwd ? k.ffx_wsi_w2 : k.ffx_wsi_w1, &v1)); CK(take_site(bwd ? k.ffx_wsi_w1 : k.ffx_wsi_w2, &v2));
    FfxArgs f; f.M = M; f.X = X; f.Z1 = z1; f.Y = Y; f.stash = k.a_ag; f.ln_g = k.ln3_g; f.ln_b = k.ln3_b;
    const bool s16 = c->mfma16 && k.ffx16_f;
    f.Wstream = s16 ? (bwd ? k.ffx16_b : k.ffx16_f) : (bwd ? k.ffx_b : k.ffx_f); f.b1 = k.b1_pk; f.b2 = k.b2;
    f.ablate = s16 ? 0 : c->ffx_ablate;
    attach(f, v1, v2);
    return launch(CAT_GEMM, 2.0 * M * (2048.0 * 256 + 256.0 * 1024), {M, bwd ? -3 : -2, 256, 2}, [&] { return s16 ? launch_ffx16(f, bwd, s) : launch_ffx(f, bwd, s); });
  }
  // optionally with LayerNorm folded into the operand
  int tkl(const GemmArgs& a, const float* ln_g, const float* ln_b) {
    const unsigned short* Wx; Site v;
    CK(h3_site("tkl", a.W, a.N, a.K, &Wx, &v));
    TklArgs t; t.M = a.M; t.N = a.N; t.X = a.A; t.Y = a.C; t.ldy = a.ldc; t.W = Wx; t.bias = a.bias; t.resid = a.resid; t.ldr = a.ldr;
    t.rowbias = a.rowbias; t.rowvar = a.rowvar; t.row0 = a.row0; t.rb_stride = a.rb_stride; t.L = a.L; t.n_var = a.rowbias ? c->n_variants : 0;
    t.ln_g = ln_g; t.ln_b = ln_b;
    attach(t, v);
    auto w16 = c->mfma16 ? c->tk16_w.find(a.W) : c->tk16_w.end();      // the same linear on v_mfma_f32_16x16x32_f16 (tkl16.hip): its own fragment planes, same scale
    const bool m16 = w16 != c->tk16_w.end();
    if (m16) t.W = w16->second;
    return launch(CAT_GEMM, 2.0 * a.M * a.N * a.K, {a.M, a.N, a.K, ln_g ? -11 : -10}, [&] { return m16 ? launch_tkl16(t, s) : launch_tkl(t, s); });
  }
  // a plain linear: on tkl where it applies, else the tile kernels
  int linear(const GemmArgs& a) { return use_tkl(a) ? tkl(a, nullptr, nullptr) : gemm(a); }
  // (+ bias, + the row variant's cross-attention constant, + residual); the site is the out-projection's (operand o)
  int ato(const STBlock& k, const float* qkv, const float* resid, float* Y, int M, int L, const float* rowbias, int rb_stride) {
    Site v;
    CK(take_site(k.ato_wsi, &v));
    AtoArgs t; t.M = M; t.L = L; t.QKV = qkv; t.W = k.ato_w; t.bias = k.bo; t.resid = resid; t.Y = Y;
    t.rowbias = rowbias; t.rowvar = c->row_variant; t.row0 = row0; t.rb_stride = rb_stride; t.n_var = rowbias ? c->n_variants : 0;
    attach(t, v);
    return launch(CAT_GEMM, 2.0 * M * 256 * 256 + 16.0 * M * L * 64, {M, 256, 256, -4}, [&] { return launch_ato(t, s); });
  }
  // d(qkv) never reaches HBM; the site is the d(ln1) GEMM's (scale: the wqkv_b planes', weights: the block's own stream)
  int abl(const STBlock& k, const float* qkv, const float* dout, const float* z, const float* add, float* out, int M, int L) {
    Site v;
    CK(h3_site("abl", k.wqkv_b, 256, 768, nullptr, &v));
    AblArgs t; t.M = M; t.L = L; t.QKV = qkv; t.dO = dout; t.W = k.abl_w; t.Z = z; t.add = add; t.ln_g = k.ln1_g; t.Y = out;
    attach(t, v);
    return launch(CAT_GEMM, 2.0 * M * 256 * 768 + 32.0 * M * L * 64, {M, 256, 768, -6}, [&] { return launch_abl(t, s); });
  }
  int tklb(const float* dqkv, const float* W, const float* z, const float* ln_g, const float* add, float* out, int M) {
    const unsigned short* Wx; Site v;
    CK(h3_site("tklb", W, 256, 768, &Wx, &v));
    TklbArgs t; t.M = M; t.X = dqkv; t.Z = z; t.add = add; t.Y = out; t.W = Wx; t.ln_g = ln_g;
    attach(t, v);
    return launch(CAT_GEMM, 2.0 * M * 256 * 768, {M, 256, 768, -12}, [&] { return launch_tklb(t, s); });
  }
  // FF1 -> GEGLU -> FF2 of one transformer block (layers_attention_mini.py:38-45, 147): one fused launch in the fp16x3
  // evaluations (the 1024-wide hidden stays in LDS), two launches otherwise.  Either way the two call sites are
  // numbered in the same order, so calibration and fused evaluations read each other's maxima.
  int ff_forward(const GemmArgs& u, const GemmArgs& f2) {
    if (!(c->ff_fused && u.M >= c->ff_fused && steady())) { CK(gemm(u)); return gemm(f2); }
    GemmArgs b1 = u, b2 = f2;
    const int k1 = prep(b1); if (k1 < 0) return k1;
    const int k2 = prep(b2); if (k2 < 0) return k2;
    RAMP_REQUIRE(k1 == 2 && k2 == 2, "fused feed-forward: weights without fp16 planes");
    return launch(CAT_GEMM, 2.0 * u.M * u.N * u.K + 2.0 * f2.M * f2.N * f2.K, {u.M, -1, u.K, 2}, [&] { return launch_ff_fwd(b1, b2, s); });
  }
};

GemmArgs lin(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N, int K) {
  GemmArgs a; a.A = A; a.lda = lda; a.W = W; a.bias = bias; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  a.taps = 1; a.shift0 = 0; a.shift_step = 0; a.L = 1;
  return a;
}
GemmArgs conv5(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int M, int N, int K,
               int L, bool backward) {
  GemmArgs a = lin(A, lda, W, bias, C, ldc, M, N, K);
  a.taps = 5; a.L = L;
  if (backward) { a.shift0 = 2; a.shift_step = -1; } else { a.shift0 = -2; a.shift_step = 1; }
  return a;
}

int dbg_store(ramp_ctx* c, const std::string& key, const float* src, size_t n, hipStream_t s) {
  if (!c->cfg.debug_taps) return 0;
  auto it = c->dbg.find(key);
  if (it == c->dbg.end() || it->second.second < n) {
    float* p; CK(dev_alloc(c, &p, n));
    c->dbg[key] = {p, n};
    it = c->dbg.find(key);
  }
  RAMP_HIP_CHECK(hipMemcpyAsync(it->second.first, src, n * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// ---- ResidualTemporalBlock ---------------------------------------------------------------------
// xa (R,L,Ca) [, xb (R,L,Cb) concatenated along channels]; x_first: (B,H,S) for the first layer
int rtb_forward(Run& r, RTB& m, const float* xa, int ca, const float* xb, int cb, const float* x_first, int n_rp,
                int t) {
  ramp_ctx* c = r.c; const int R = r.R, M = R * m.L;
  const float* tbias = c->time_table + (size_t)t * c->tt_stride + m.tb_off;
  GnArgs g; g.x = m.a_c1; g.gamma = m.g1; g.beta = m.b1; g.tbias = tbias; g.resid = nullptr; g.y = m.a_h;
  // ramp_score_rows: every row picks its own table line (t == 0 here: tbias is line 0 at this block's offset)
  if (c->t_rows_cur) { g.t_rows = c->t_rows_cur + r.row0; g.tt_stride = c->tt_stride; }
  g.stats = m.a_st1; g.R = R; g.L = m.L; g.C = m.cout; g.eps = 1e-5f; g.mish = 1;
  const float* resid;
  bool gn_due = true;
  if (m.first) {
    LAUNCH(c, r.s, CAT_SMALLCONV, 0, launch_conv_in_fwd(x_first, m.w5in, m.c1.bias, m.w1in, m.res_bias, m.a_c1, c->t_res, R, n_rp, m.L, m.cin, r.s, m.cout));
    resid = c->t_res;
  } else {
    GemmArgs a = conv5(xa, ca, m.c1.fwd, m.c1.bias, m.a_c1, m.cout, M, m.cout, m.cin, m.L, false);
    if (xb) { a.A2 = xb; a.lda2 = cb; a.K1 = ca; }
    // conv -> (stash c1, statistics) -> GroupNorm -> Mish -> + time bias = h: one launch where tkw / tkc take it; else the GroupNorm follows
    // the residual product below
    CK(r.conv_gn(a, g, &gn_due));
    if (m.has_res) {
      GemmArgs b = lin(xa, ca, m.res_f, m.res_bias, c->t_res, m.cout, M, m.cout, m.cin);
      if (xb) { b.A2 = xb; b.lda2 = cb; b.K1 = ca; }
      CK(r.gemm(b));
      resid = c->t_res;
    } else {
      resid = xa;
    }
  }
  if (gn_due) LAUNCH(c, r.s, CAT_ROW, 0, launch_gn_fwd(g, r.s));
  // conv -> (stash c2, statistics) -> GroupNorm -> Mish -> + residual = the block's output
  GemmArgs c2a = conv5(m.a_h, m.cout, m.c2.fwd, m.c2.bias, m.a_c2, m.cout, M, m.cout, m.cout, m.L, false);
  g.x = m.a_c2; g.gamma = m.g2; g.beta = m.b2; g.tbias = nullptr; g.t_rows = nullptr; g.resid = resid; g.y = m.a_out; g.stats = m.a_st2;
  CK(r.conv_gn(c2a, g));
  CK(dbg_store(c, "out/" + m.name, m.a_out, (size_t)M * m.cout, r.s));
  return 0;
}

// dy (R,L,Cout) -> dxa (R,L,Ca) [, dxb (R,L,Cb)] ; add2: optional extra addend on dxa (same shape)
int rtb_backward(Run& r, RTB& m, const float* dy, float* dxa, int ca, float* dxb, int cb, const float* add2,
                 float* eps_out) {
  ramp_ctx* c = r.c; const int R = r.R, M = R * m.L;
  CK(dbg_store(c, "gout/" + m.name, dy, (size_t)M * m.cout, r.s));
  GnBwdArgs g; g.dy = dy; g.x = m.a_c2; g.stats = m.a_st2; g.gamma = m.g2; g.beta = m.b2; g.add = nullptr;
  g.dx = c->g_t1; g.R = R; g.L = m.L; g.C = m.cout; g.mish = 1;
  // dh = conv2^T(dc2), dc2 = GNbwd(dy mish'; c2)
  CK(r.gn_conv_bwd(g, conv5(c->g_t1, m.cout, m.c2.bwd, nullptr, c->g_t2, m.cout, M, m.cout, m.cout, m.L, true)));
  g.dy = c->g_t2; g.x = m.a_c1; g.stats = m.a_st1; g.gamma = m.g1; g.beta = m.b1; g.dx = c->g_t1;
  if (m.first) {
    LAUNCH(c, r.s, CAT_ROW, 0, launch_gn_bwd(g, r.s));                                                   // dc1
    LAUNCH(c, r.s, CAT_SMALLCONV, 0, launch_conv_in_bwd(c->g_t1, dy, m.w5in, m.w1in, eps_out, R, m.L, m.cin, r.s, m.cout));
    return 0;
  }
  const float* resid; int ldr;
  if (m.has_res) {
    CK(r.gemm(lin(dy, m.cout, m.res_b, nullptr, c->g_tr, m.cin, M, m.cin, m.cout)));
    resid = c->g_tr; ldr = m.cin;
  } else {
    resid = dy; ldr = m.cout;
  }
  // dx = conv1^T(dc1) + residual path (+ skip gradient), dc1 = GNbwd(dh mish'; c1)
  GemmArgs a = conv5(c->g_t1, m.cout, m.c1.bwd, nullptr, dxa, ca, M, m.cin, m.cout, m.L, true);
  a.resid = resid; a.ldr = ldr;
  if (dxb) { a.C2 = dxb; a.ldc2 = cb; a.N1 = ca; }
  if (add2) { RAMP_REQUIRE(dxb == nullptr, "add2 with split output"); a.resid2 = add2; a.ldr2 = ca; }
  return r.gn_conv_bwd(g, a);
}

// ---- SpatialTransformer ------------------------------------------------------------------------
// share > 1 (first transformer of the network inside a sampling job): x and everything up to the first block's
// attention output projection hold ONE row per trajectory (r.R / share rows); the rows part ways where the
// cross-attention constant of their scene variant is added (expand_rows), and the outer residual uses x expanded.
int st_forward(Run& r, ST& m, const float* x, int share = 1) {
  ramp_ctx* c = r.c; const int R = r.R, M = R * m.L, D = 256;
  const int Rp = R / share, Mp = Rp * m.L;              // prefix rows
  GnArgs g; g.x = x; g.gamma = m.gn_g; g.beta = m.gn_b; g.y = c->t_xn; g.stats = m.a_gst; g.R = Rp; g.L = m.L;
  g.C = m.C; g.eps = 1e-6f; g.mish = 0;
  LAUNCH(c, r.s, CAT_ROW, 0, launch_gn_fwd(g, r.s));
  CK(r.gemm(lin(c->t_xn, m.C, m.wpi_f, m.bpi, m.a_z0, D, Mp, D, m.C)));
  const float* zin = m.a_z0;
  for (int b = 0; b < 2; ++b) {
    STBlock& k = m.blk[b];
    const bool pre = share > 1 && b == 0;
    const int Rb = pre ? Rp : R, Mb = Rb * m.L;
    {
      GemmArgs q = lin(c->t_ln, D, k.wqkv_f, nullptr, k.a_qkv, 768, Mb, 768, D);
      if (r.use_tkl(q)) {      // LayerNorm-1 on the operand registers of the token-owning QKV kernel: no ln_fwd, no t_ln round trip
        q.A = zin;
        CK(r.tkl(q, k.ln1_g, k.ln1_b));
      } else {
        LAUNCH(c, r.s, CAT_ROW, 0, launch_ln_fwd(zin, k.ln1_g, k.ln1_b, c->t_ln, Mb, r.s));
        CK(r.gemm(q));
      }
    }
    const float* rowbias = c->cross_bias + (size_t)(m.blk0 + b) * D; const int rb_stride = c->n_blocks_total * D;
    if (r.use_ato(k, Mb, m.L)) {      // softmax(q k^T / 8) v -> out-projection + bias + constant + residual: o never reaches HBM
      CK(r.ato(k, k.a_qkv, zin, pre ? c->t_ln : k.a_z1, Mb, m.L, pre ? nullptr : rowbias, rb_stride));
    } else {
      LAUNCH(c, r.s, CAT_ATTN, 16.0 * Rb * m.L * m.L * 64, launch_attn_fwd(k.a_qkv, c->t_o, Rb, m.L, r.s));
      GemmArgs a = lin(c->t_o, D, k.wo_f, k.bo, pre ? c->t_ln : k.a_z1, D, Mb, D, D);
      a.resid = zin; a.ldr = D; a.L = m.L;
      if (!pre) { a.rowbias = rowbias; a.rb_stride = rb_stride; a.rowvar = c->row_variant; a.row0 = r.row0; }
      CK(r.linear(a));
    }
    if (pre) LAUNCH(c, r.s, CAT_ROW, 0, launch_expand_rows(c->t_ln, k.a_z1, R, share, m.L, D, rowbias, rb_stride, c->row_variant, r.row0, r.s));
    if (r.use_ffx(k, M)) {      // LN3 -> FF1 -> GEGLU -> FF2 -> + z1 in one launch, nothing but the stash and z2 written
      CK(r.ffx(k, false, k.a_z1, k.a_z1, k.a_z2, M));
      zin = k.a_z2;
      continue;
    }
    LAUNCH(c, r.s, CAT_ROW, 0, launch_ln_fwd(k.a_z1, k.ln3_g, k.ln3_b, c->t_ln, M, r.s));
    GemmArgs u = lin(c->t_ln, D, k.w1_pk, k.b1_pk, k.a_ag, 2048, M, 2048, D);
    u.epi = EPI_GEGLU_FWD; u.aux_out = c->t_hg; u.ld_aux = 1024;        // writes ag (stash) and hg = a * gelu(g)
    u.geglu_group = c->geglu_group;
    GemmArgs f = lin(c->t_hg, 1024, k.w2_f, k.b2, k.a_z2, D, M, D, 1024);
    f.resid = k.a_z1; f.ldr = D;
    CK(r.ff_forward(u, f));
    zin = k.a_z2;
  }
  GemmArgs o = lin(zin, D, m.wpo_f, m.bpo, m.a_y, m.C, M, m.C, D);
  o.resid = x; o.ldr = m.C;
  if (share > 1) {
    LAUNCH(c, r.s, CAT_ROW, 0, launch_expand_rows(x, c->t_xn, R, share, m.L, m.C, nullptr, 0, nullptr, 0, r.s));
    o.resid = c->t_xn;
  }
  CK(r.gemm(o));
  CK(dbg_store(c, "out/" + m.name, m.a_y, (size_t)M * m.C, r.s));
  return 0;
}

// share > 1: see st_forward; comb = the weights of the rows' gradients in what the sampler uses.  dy, and everything down
// to d(z1) of the first block, have r.R rows; from there on (and dx) one COMBINED row per trajectory.
// out[b] = sum_j w_j in[b share + j] where the rows of a trajectory meet again: the job's host scalars, or (a composed job) the chunk's lines of
// the device weight table -- r.row0 = b0 * share is the chunk's first row, hence its first trajectory's first weight
int combine_prefix(Run& r, const float* in, float* out, int Rp, int share, int L, int C, const float* comb) {
  ramp_ctx* c = r.c;
  if (c->g_weight_cur) LAUNCH(c, r.s, CAT_ROW, 0, launch_combine_rows_weighted(in, out, Rp, share, L, C, c->g_weight_cur + r.row0, r.s));
  else LAUNCH(c, r.s, CAT_ROW, 0, launch_combine_rows(in, out, Rp, share, L, C, comb, r.s));
  return 0;
}
int st_backward(Run& r, ST& m, const float* x, const float* dy, float* dx, int share = 1, const float* comb = nullptr) {
  ramp_ctx* c = r.c; const int R = r.R, M = R * m.L, D = 256;
  const int Rp = R / share, Mp = Rp * m.L;
  CK(dbg_store(c, "gout/" + m.name, dy, (size_t)M * m.C, r.s));
  float* dz = c->t_dz; float* dz1 = c->t_dz1;
  CK(r.gemm(lin(dy, m.C, m.wpo_b, nullptr, dz, D, M, D, m.C)));
  for (int b = 1; b >= 0; --b) {
    STBlock& k = m.blk[b];
    const float* zin = (b == 0) ? m.a_z0 : m.blk[0].a_z2;
    if (r.use_ffx(k, M)) {      // dz1 = dz + LN3bwd(W1^T (d(hg) (.) stash)), d(hg) = W2^T dz: one launch
      CK(r.ffx(k, true, dz, k.a_z1, dz1, M));
    } else {
      if (c->gemm_mode >= 1 && c->x6_pipe) {
        // d(hg) only (1024 wide); d(ag) = [d(hg) s1 | d(hg) s2] is formed by the next GEMM's operand loader from the
        // forward stash: the 2048-wide d(ag) never goes to HBM (saves a 2048-float write and a 2048-float read per token)
        CK(r.gemm(lin(dz, D, k.w2_b, nullptr, c->t_hg, 1024, M, 1024, D)));
        GemmArgs v = lin(c->t_hg, 1024, k.w1_b, nullptr, c->t_dln, D, M, D, 2048);         // d(ln3)
        v.Amul = k.a_ag; v.lda_mul = 2048; v.a_period = 1024;
        CK(r.gemm(v));
      } else {
        GemmArgs w = lin(dz, D, k.w2_b, nullptr, c->t_dag, 2048, M, 1024, D);   // d(hg) -> d(ag) in the epilogue
        w.epi = EPI_GEGLU_BWD; w.aux_in = k.a_ag; w.ld_aux = 2048;
        CK(r.gemm(w));
        CK(r.gemm(lin(c->t_dag, 2048, k.w1_b, nullptr, c->t_dln, D, M, D, 2048)));        // d(ln3)
      }
      LAUNCH(c, r.s, CAT_ROW, 0, launch_ln_bwd(c->t_dln, k.a_z1, k.ln3_g, dz, dz1, M, r.s));         // dz1
    }
    const bool pre = share > 1 && b == 0;
    const int Rb = pre ? Rp : R, Mb = Rb * m.L;
    if (pre) {      // the rows of a trajectory meet again: dz (free now) <- sum_j comb_j dz1[row j]
      CK(combine_prefix(r, dz1, dz, Rp, share, m.L, D, comb));
      std::swap(dz, dz1);
    }
    CK(r.linear(lin(dz1, D, k.wo_b, nullptr, c->t_o, D, Mb, D, D)));                    // d(o)
    if (r.use_abl(k, Mb, m.L)) {   // d(q, k, v), d(ln1) and the LayerNorm-1 backward in ONE launch: dz = dz1 + LN1bwd(attention-backward(d(o)) Wqkv^T)
      CK(r.abl(k, k.a_qkv, c->t_o, zin, dz1, dz, Mb, m.L));
    } else {
      if (r.use_atb(Mb, m.L)) {      // d(q, k, v) on sample-owning waves (atk.hip, atb_kernel): fp16x3 MFMAs, no LDS tile, two waves per SIMD
        AtbArgs t; t.M = Mb; t.L = m.L; t.QKV = k.a_qkv; t.dO = c->t_o; t.dQKV = c->t_dqkv;
        LAUNCH(c, r.s, CAT_ATTN, 32.0 * Rb * m.L * m.L * 64, launch_atb(t, r.s));
      } else {
        LAUNCH(c, r.s, CAT_ATTN, 32.0 * Rb * m.L * m.L * 64, launch_attn_bwd(k.a_qkv, c->t_o, c->t_dqkv, Rb, m.L, r.s));
      }
      if (r.use_tklb(Mb, k.wqkv_b)) {      // d(ln1) and the LayerNorm-1 backward in one token-owning launch: dz = dz1 + LN1bwd(d(qkv) Wqkv^T)
        CK(r.tklb(c->t_dqkv, k.wqkv_b, zin, k.ln1_g, dz1, dz, Mb));
      } else {
        CK(r.gemm(lin(c->t_dqkv, 768, k.wqkv_b, nullptr, c->t_dln, D, Mb, D, 768)));        // d(ln1)
        LAUNCH(c, r.s, CAT_ROW, 0, launch_ln_bwd(c->t_dln, zin, k.ln1_g, dz1, dz, Mb, r.s));           // dz (block input)
      }
    }
  }
  CK(r.gemm(lin(dz, D, m.wpi_b, nullptr, c->t_xn, m.C, Mp, m.C, D)));                   // d(xn)
  GnBwdArgs g; g.dy = c->t_xn; g.x = x; g.stats = m.a_gst; g.gamma = m.gn_g; g.beta = m.gn_b; g.add = dy; g.dx = dx;
  g.R = Rp; g.L = m.L; g.C = m.C; g.mish = 0;
  if (share > 1) {   // the gradient through the outer residual, combined (t_o is free after the attention backward)
    CK(combine_prefix(r, dy, c->t_o, Rp, share, m.L, m.C, comb));
    g.add = c->t_o;
  }
  LAUNCH(c, r.s, CAT_ROW, 0, launch_gn_bwd(g, r.s));
  return 0;
}

// ---- whole network -----------------------------------------------------------------------------
// x (B,H,S) device pointer of the FIRST trajectory of this chunk; rows [row0, row0 + R)
// share = n_rp (> 1) inside a sampling job: the rows of a trajectory carry the same x and t, so the two residual blocks
// of level 0 and the first transformer down to its first cross-attention constant run on one row per trajectory
int net_forward(ramp_ctx* c, const float* x_chunk, int row0, int R, int n_rp, int t, float* f_out, bool want_grad,
                hipStream_t s, int share = 1) {
  Run r{c, s, R, row0};
  Run rp{c, s, R / share, row0 / share};
  const int nl = c->cfg.n_levels;
  const float* cur = nullptr; int cc = 0;
  for (int k = 0; k < nl; ++k) {
    RTB& a = c->rtbs[2 * k]; RTB& b = c->rtbs[2 * k + 1]; ST& st = c->sts[k];
    const bool pre = share > 1 && k == 0;
    CK(rtb_forward(pre ? rp : r, a, cur, cc, nullptr, 0, x_chunk, pre ? 1 : n_rp, t));
    CK(rtb_forward(pre ? rp : r, b, a.a_out, a.cout, nullptr, 0, nullptr, pre ? 1 : n_rp, t));
    CK(st_forward(r, st, b.a_out, pre ? share : 1));
    if (k < nl - 1) {
      Resample& d = c->downs[k];
      // Downsample1d: y[lo] = b + sum_j x[2 lo + j - 1] W_j^T  -> 3 taps over stride-2 source rows
      GemmArgs ga = lin(st.a_y, d.C, d.w_f, d.bias, d.a_y, d.C, R * d.Lout, d.C, d.C);
      ga.taps = 3; ga.shift0 = -1; ga.shift_step = 1; ga.L = d.Lout; ga.a_stride = 2;
      CK(r.gemm(ga));
      CK(dbg_store(c, "out/" + d.name, d.a_y, (size_t)R * d.Lout * d.C, s));
      cur = d.a_y; cc = d.C;
    } else {
      cur = st.a_y; cc = st.C;
    }
  }
  RTB& m1 = c->rtbs[2 * nl]; RTB& m2 = c->rtbs[2 * nl + 1]; ST& ms = c->sts[nl];
  CK(rtb_forward(r, m1, cur, cc, nullptr, 0, nullptr, n_rp, t));
  CK(st_forward(r, ms, m1.a_out));
  CK(rtb_forward(r, m2, ms.a_y, ms.C, nullptr, 0, nullptr, n_rp, t));
  cur = m2.a_out; cc = m2.cout;
  for (int k = 0; k < nl - 1; ++k) {
    RTB& a = c->rtbs[2 * nl + 2 + 2 * k]; RTB& b = c->rtbs[2 * nl + 3 + 2 * k]; ST& st = c->sts[nl + 1 + k];
    ST& skip = c->sts[nl - 1 - k];
    CK(rtb_forward(r, a, cur, cc, skip.a_y, skip.C, nullptr, n_rp, t));
    CK(rtb_forward(r, b, a.a_out, a.cout, nullptr, 0, nullptr, n_rp, t));
    CK(st_forward(r, st, b.a_out));
    Resample& u = c->ups[k];
    // Upsample1d (ConvTranspose1d k4 s2 p1): y[2i] = b + x[i] W_1 + x[i-1] W_3 ; y[2i+1] = b + x[i+1] W_0 + x[i] W_2
    for (int par = 0; par < 2; ++par) {
      GemmArgs ga = lin(st.a_y, u.C, u.w_f + (size_t)par * 2 * u.C * u.C, u.bias, u.a_y, u.C, R * u.Lin, u.C, u.C);
      ga.taps = 2; ga.shift0 = par; ga.shift_step = -1; ga.L = u.Lin; ga.c_rstride = 2; ga.c_roff = par;
      CK(r.gemm(ga));
    }
    CK(dbg_store(c, "out/" + u.name, u.a_y, (size_t)R * u.Lout * u.C, s));
    cur = u.a_y; cc = u.C;
  }
  const int H = c->cfg.horizon, C0 = c->cfg.unet_input_dim, M = R * H;
  // the final Conv1dBlock.  (Through the common helper although only tkc ever took it: tkw's rule wants C_out in {128, 256, 512, 1024}
  // -- tw_geometry, tkw.hip -- and this convolution has unet_input_dim in {16, 32, 64} channels, so use_tkw is false here.)
  GnArgs g; g.x = c->a_fin_c; g.gamma = c->fin_g; g.beta = c->fin_b; g.y = c->a_fin_a; g.stats = c->a_fin_st;
  g.R = R; g.L = H; g.C = C0; g.eps = 1e-5f; g.mish = 1;
  CK(r.conv_gn(conv5(cur, cc, c->final_conv.fwd, c->final_conv.bias, c->a_fin_c, C0, M, C0, C0, H, false), g));
  LAUNCH(c, s, CAT_SMALLCONV, 0, launch_conv_out(c->a_fin_a, c->fin_w, c->fin_bias, f_out, want_grad ? c->a_fin_da : nullptr, M, c->cfg.state_dim, s, C0));
  return 0;
}

// share > 1: eps_out gets ONE row per trajectory, sum_j comb[j] * (input gradient of row j)
int net_backward(ramp_ctx* c, int row0, int R, float* eps_out, hipStream_t s, int share = 1, const float* comb = nullptr) {
  Run r{c, s, R, row0};
  Run rp{c, s, R / share, row0 / share};
  const int nl = c->cfg.n_levels, H = c->cfg.horizon, C0 = c->cfg.unet_input_dim, M = R * H;
  GnBwdArgs g; g.dy = c->a_fin_da; g.x = c->a_fin_c; g.stats = c->a_fin_st; g.gamma = c->fin_g; g.beta = c->fin_b;
  g.dx = c->g_t1; g.R = R; g.L = H; g.C = C0; g.mish = 1;
  float* d = c->g_a; float* e = c->g_b;
  CK(r.gn_conv_bwd(g, conv5(c->g_t1, C0, c->final_conv.bwd, nullptr, d, C0, M, C0, C0, H, true)));      // (tkc or the pair, as in net_forward)
  for (int k = nl - 2; k >= 0; --k) {
    RTB& a = c->rtbs[2 * nl + 2 + 2 * k]; RTB& b = c->rtbs[2 * nl + 3 + 2 * k]; ST& st = c->sts[nl + 1 + k];
    Resample& u = c->ups[k];
    CK(dbg_store(c, "gout/" + u.name, d, (size_t)R * u.Lout * u.C, s));
    {   // dX of Upsample1d: dx[i] = sum_j dy[2i - 1 + j] W_j^T   (4 taps over stride-2 source rows)
      GemmArgs ga = lin(d, u.C, u.w_b, nullptr, e, u.C, R * u.Lin, u.C, u.C);
      ga.taps = 4; ga.shift0 = -1; ga.shift_step = 1; ga.L = u.Lin; ga.a_stride = 2;
      CK(r.gemm(ga)); std::swap(d, e);
    }
    CK(st_backward(r, st, b.a_out, d, e)); std::swap(d, e);
    CK(rtb_backward(r, b, d, e, b.cin, nullptr, 0, nullptr, nullptr)); std::swap(d, e);
    const int lvl = nl - 1 - k;                      // the skip consumed by ups.k
    const int ca = a.cin - c->sts[lvl].C;
    CK(rtb_backward(r, a, d, e, ca, c->skip_grad[lvl], c->sts[lvl].C, nullptr, nullptr)); std::swap(d, e);
  }
  RTB& m1 = c->rtbs[2 * nl]; RTB& m2 = c->rtbs[2 * nl + 1]; ST& ms = c->sts[nl];
  CK(rtb_backward(r, m2, d, e, m2.cin, nullptr, 0, nullptr, nullptr)); std::swap(d, e);
  CK(st_backward(r, ms, m1.a_out, d, e)); std::swap(d, e);
  // the deepest level's transformer output feeds both mid_block1 and (as skip) ups.0
  CK(rtb_backward(r, m1, d, e, m1.cin, nullptr, 0, c->skip_grad[nl - 1], nullptr)); std::swap(d, e);
  for (int k = nl - 1; k >= 0; --k) {
    RTB& a = c->rtbs[2 * k]; RTB& b = c->rtbs[2 * k + 1]; ST& st = c->sts[k];
    if (k < nl - 1) {
      Resample& dn = c->downs[k];
      CK(dbg_store(c, "gout/" + dn.name, d, (size_t)R * dn.Lout * dn.C, s));
      // dX of Downsample1d: dx[2i] = dy[i] W_1 ; dx[2i+1] = dy[i+1] W_0 + dy[i] W_2   (+ skip gradient)
      for (int par = 0; par < 2; ++par) {
        GemmArgs ga = lin(d, dn.C, dn.w_b + (size_t)par * dn.C * dn.C, nullptr, e, dn.C, R * dn.Lout, dn.C, dn.C);
        ga.taps = par ? 2 : 1; ga.shift0 = par; ga.shift_step = -1; ga.L = dn.Lout; ga.c_rstride = 2; ga.c_roff = par;
        if (k >= 1) { ga.resid = c->skip_grad[k]; ga.ldr = dn.C; }
        CK(r.gemm(ga));
      }
      std::swap(d, e);
    }
    const bool pre = share > 1 && k == 0;
    CK(st_backward(r, st, b.a_out, d, e, pre ? share : 1, comb)); std::swap(d, e);
    CK(rtb_backward(pre ? rp : r, b, d, e, b.cin, nullptr, 0, nullptr, nullptr)); std::swap(d, e);
    if (k > 0) { CK(rtb_backward(r, a, d, e, a.cin, nullptr, 0, nullptr, nullptr)); std::swap(d, e); }
    else CK(rtb_backward(pre ? rp : r, a, d, nullptr, 0, nullptr, 0, nullptr, eps_out));
  }
  return 0;
}

// ---- scene encoders (once per scene) ------------------------------------------------------------
GemmArgs slin(const float* A, int K, const float* W, const float* bias, float* C, int M, int N, const float* resid = nullptr) {
  GemmArgs a = lin(A, K, W, bias, C, N, M, N, K);
  if (resid) { a.resid = resid; a.ldr = N; }
  return a;
}
int sw(ramp_ctx* c, const std::string& key, float** out) {
  auto it = c->raw.find("scene_encoder." + key);
  RAMP_REQUIRE(it != c->raw.end(), "missing scene-encoder weight '" + key + "'");
  *out = it->second.first;
  return 0;
}
int scene_scratch(ramp_ctx* c, size_t n) {
  if (n > c->scene_ws_cap) { CK(dev_alloc(c, &c->scene_ws, n)); c->scene_ws_cap = n; }
  return 0;
}

// ObstacleEncoderSet.forward for one scene (obstacle_encoder.py:125-152); cloud (No, Np, 2) -> latent (320)
int encode_scene_2d(ramp_ctx* c, const float* cloud, int No, int Np, float* out, hipStream_t s) {
  const int T = No * Np;
  CK(scene_scratch(c, (size_t)T * (192 + 64 * 4 + 192 + 256) + 4096));
  float* p = c->scene_ws;
  float* F = p; p += (size_t)T * 192;
  float* COMB = p; p += (size_t)T * 64;
  float* X = p; p += (size_t)T * 64;
  float* X2 = p; p += (size_t)T * 64;
  float* LNb = p; p += (size_t)T * 64;
  float* QKV = p; p += (size_t)T * 192;
  float* Hb = p; p += (size_t)T * 256;
  float* centers = p; p += 2 * ((No + 3) & ~3);
  float* maxd = p; p += (No + 3) & ~3;
  float* P0 = p; p += 64; float* P1 = p; p += 256;
  float *w, *b, *g, *be, *div;
  CK(sw(c, "pos_encoder.div_term", &div));
  CK(sw(c, "point_embedding.0.weight", &w)); CK(sw(c, "point_embedding.0.bias", &b));
  CK(sw(c, "point_embedding.1.weight", &g)); CK(sw(c, "point_embedding.1.bias", &be));
  CK(scene_enc2d_prep(cloud, No, Np, centers, maxd, s));
  CK(scene_enc2d_feat(cloud, centers, maxd, div, w, b, g, be, F, Np, T, s));
  CK(sw(c, "combined_encoder.0.weight", &w)); CK(sw(c, "combined_encoder.0.bias", &b));
  CK(launch_gemm(slin(F, 192, w, b, X2, T, 64), s));
  CK(sw(c, "combined_encoder.1.weight", &g)); CK(sw(c, "combined_encoder.1.bias", &be));
  CK(scene_ln64(X2, g, be, COMB, T, 1, s));
  const int dims[3] = {64, 96, 160};
  int off = 0;
  for (int i = 0; i < 3; ++i) {
    const float* xin = COMB;
    for (int j = 0; j < 3; ++j) {
      const std::string t = "set_transformers." + std::to_string(i) + "." + std::to_string(j);
      CK(sw(c, t + ".norm1.weight", &g)); CK(sw(c, t + ".norm1.bias", &be));
      CK(scene_ln64(xin, g, be, LNb, T, 0, s));
      CK(sw(c, t + ".attn.qkv.weight", &w));
      CK(launch_gemm(slin(LNb, 64, w, nullptr, QKV, T, 192), s));
      CK(scene_attention(QKV, LNb, T, 4, 16, 0.25f, s));
      CK(sw(c, t + ".attn.proj.weight", &w)); CK(sw(c, t + ".attn.proj.bias", &b));
      CK(launch_gemm(slin(LNb, 64, w, b, X2, T, 64, xin), s));
      CK(sw(c, t + ".norm2.weight", &g)); CK(sw(c, t + ".norm2.bias", &be));
      CK(scene_ln64(X2, g, be, LNb, T, 0, s));
      CK(sw(c, t + ".mlp.0.weight", &w)); CK(sw(c, t + ".mlp.0.bias", &b));
      CK(launch_gemm(slin(LNb, 64, w, b, Hb, T, 256), s));
      CK(scene_affine_act(Hb, nullptr, nullptr, nullptr, Hb, (long)T * 256, 256, 1, s));
      CK(sw(c, t + ".mlp.3.weight", &w)); CK(sw(c, t + ".mlp.3.bias", &b));
      CK(launch_gemm(slin(Hb, 256, w, b, X, T, 64, X2), s));
      xin = X;
    }
    const int d = dims[i];
    const std::string q = "poolings." + std::to_string(i);
    CK(scene_colreduce(X, P0, 1, T, 64, 0, s));
    CK(sw(c, q + ".0.weight", &w)); CK(sw(c, q + ".0.bias", &b));
    CK(launch_gemm(slin(P0, 64, w, b, P1, 1, d), s));
    CK(scene_affine_act(P1, nullptr, nullptr, nullptr, P1, d, d, 1, s));
    CK(sw(c, q + ".2.weight", &w)); CK(sw(c, q + ".2.bias", &b));
    CK(launch_gemm(slin(P1, d, w, b, out + off, 1, d), s));
    off += d;
  }
  return 0;
}

// ObstacleEncoder.forward, eval mode, one scene (obstacle_encoder3d.py:77-94); cloud (No, Np, 3) -> latent (256)
int encode_scene_3d(ramp_ctx* c, const float* cloud, int No, int Np, float* out, hipStream_t s) {
  const int T = No * Np, E = 256;
  CK(scene_scratch(c, (size_t)T * (64 + 256) + (size_t)No * (256 * 4 + 768 + 512) + 4096));
  float* p = c->scene_ws;
  float* H1 = p; p += (size_t)T * 64;
  float* H2 = p; p += (size_t)T * E;
  float* X = p; p += (size_t)No * E; float* X2 = p; p += (size_t)No * E;
  float* LNb = p; p += (size_t)No * E; float* O = p; p += (size_t)No * E;
  float* QKV = p; p += (size_t)No * 768; float* Hb = p; p += (size_t)No * 512;
  float* sc = p; p += 256; float* sh = p; p += 256; float* S0 = p; p += 256; float* S1 = p; p += 256;
  float *w, *b, *g, *be, *rm, *rv;
  CK(sw(c, "point_processor.conv1.weight", &w)); CK(sw(c, "point_processor.conv1.bias", &b));
  CK(scene_linear_small(cloud, w, b, H1, T, 64, 3, s));
  CK(sw(c, "point_processor.bn1.weight", &g)); CK(sw(c, "point_processor.bn1.bias", &be));
  CK(sw(c, "point_processor.bn1.running_mean", &rm)); CK(sw(c, "point_processor.bn1.running_var", &rv));
  CK(scene_bn_fold(g, be, rm, rv, sc, sh, 64, s));
  CK(scene_affine_act(H1, sc, sh, nullptr, H1, (long)T * 64, 64, 2, s));
  CK(sw(c, "point_processor.conv2.weight", &w)); CK(sw(c, "point_processor.conv2.bias", &b));
  CK(launch_gemm(slin(H1, 64, w, b, H2, T, E), s));
  CK(sw(c, "point_processor.bn2.weight", &g)); CK(sw(c, "point_processor.bn2.bias", &be));
  CK(sw(c, "point_processor.bn2.running_mean", &rm)); CK(sw(c, "point_processor.bn2.running_var", &rv));
  CK(scene_bn_fold(g, be, rm, rv, sc, sh, E, s));
  CK(scene_affine_act(H2, sc, sh, nullptr, H2, (long)T * E, E, 2, s));
  CK(scene_colreduce(H2, X, No, Np, E, 1, s));                     // max over the points of each obstacle
  for (int i = 0; i < 2; ++i) {
    const std::string t = "set_transformer_blocks." + std::to_string(i);
    CK(sw(c, t + ".norm1.weight", &g)); CK(sw(c, t + ".norm1.bias", &be));
    CK(launch_ln_fwd(X, g, be, LNb, No, s));
    CK(sw(c, t + ".mha.in_proj_weight", &w)); CK(sw(c, t + ".mha.in_proj_bias", &b));
    CK(launch_gemm(slin(LNb, E, w, b, QKV, No, 768), s));
    CK(scene_attention(QKV, O, No, 4, 64, 0.125f, s));
    CK(sw(c, t + ".mha.out_proj.weight", &w)); CK(sw(c, t + ".mha.out_proj.bias", &b));
    CK(launch_gemm(slin(O, E, w, b, X2, No, E, X), s));
    CK(sw(c, t + ".norm2.weight", &g)); CK(sw(c, t + ".norm2.bias", &be));
    CK(launch_ln_fwd(X2, g, be, LNb, No, s));
    CK(sw(c, t + ".ffn.0.weight", &w)); CK(sw(c, t + ".ffn.0.bias", &b));
    CK(launch_gemm(slin(LNb, E, w, b, Hb, No, 512), s));
    CK(scene_affine_act(Hb, nullptr, nullptr, nullptr, Hb, (long)No * 512, 512, 2, s));
    CK(sw(c, t + ".ffn.3.weight", &w)); CK(sw(c, t + ".ffn.3.bias", &b));
    CK(launch_gemm(slin(Hb, 512, w, b, X, No, E, X2), s));
  }
  CK(sw(c, "output_proj.weight", &w)); CK(sw(c, "output_proj.bias", &b));
  CK(launch_gemm(slin(X, E, w, b, O, No, E), s));
  CK(scene_colreduce(O, S0, 1, No, E, 1, s));
  CK(sw(c, "global_pooling.0.weight", &w)); CK(sw(c, "global_pooling.0.bias", &b));
  CK(launch_gemm(slin(S0, E, w, b, S1, 1, E), s));
  CK(scene_affine_act(S1, nullptr, nullptr, nullptr, S1, E, E, 2, s));
  CK(sw(c, "global_pooling.2.weight", &w)); CK(sw(c, "global_pooling.2.bias", &b));
  CK(launch_gemm(slin(S1, E, w, b, out, 1, E), s));
  return 0;
}


// ---- many scenes in one pass (ramp_encode_scenes) -------------------------------------------------
// The schedules of encode_scene_2d / encode_scene_3d over the concatenated tokens of a pass: every per-token stage and every GEMM is
// the single-scene launch with M = the pass's rows (launch_gemm picks its tile from N and K, a row's result does not depend on M);
// only the stages that look across tokens take the tables.  The device tables of one pass, rebased to the pass's first obstacle / point:
struct EncodeTables {
  const int* obstacle_first;   // [n_obstacles + 1] first point of each obstacle
  const int* scene_first;      // [n_scenes + 1] first TOKEN of each scene (2-D: point, 3-D: obstacle)
  const int* tiles;            // [n_tiles][3] attention tiles over the scenes' tokens
  int n_scenes, n_obstacles, n_points, n_tiles;
};
size_t encode_scratch_2d(size_t T, size_t No, size_t Ns) { return T * (192 + 64 * 4 + 192 + 256) + 3 * ((No + 3) & ~(size_t)3) + Ns * (64 + 256) + 4096; }
size_t encode_scratch_3d(size_t T, size_t No, size_t Ns) { return T * (64 + 256) + No * (256 * 4 + 768 + 512) + 512 + Ns * 512 + 4096; }

// cloud: the pass's points (T, 2); out: the pass's first latent row (n_scenes, 320)
int encode_scenes_2d(ramp_ctx* c, const float* cloud, const EncodeTables& tb, float* out, hipStream_t s) {
  const int T = tb.n_points, No = tb.n_obstacles, Ns = tb.n_scenes, CTX = 320;
  float* p = c->scene_ws;
  float* F = p; p += (size_t)T * 192;
  float* COMB = p; p += (size_t)T * 64;
  float* X = p; p += (size_t)T * 64;
  float* X2 = p; p += (size_t)T * 64;
  float* LNb = p; p += (size_t)T * 64;
  float* QKV = p; p += (size_t)T * 192;
  float* Hb = p; p += (size_t)T * 256;
  float* centers = p; p += 2 * ((No + 3) & ~3);
  float* maxd = p; p += (No + 3) & ~3;
  float* P0 = p; p += (size_t)Ns * 64; float* P1 = p; p += (size_t)Ns * 256;
  float *w, *b, *g, *be, *div;
  CK(sw(c, "pos_encoder.div_term", &div));
  CK(sw(c, "point_embedding.0.weight", &w)); CK(sw(c, "point_embedding.0.bias", &b));
  CK(sw(c, "point_embedding.1.weight", &g)); CK(sw(c, "point_embedding.1.bias", &be));
  CK(scene_enc2d_prep_seg(cloud, tb.obstacle_first, No, centers, maxd, s));
  CK(scene_enc2d_feat_seg(cloud, tb.obstacle_first, No, centers, maxd, div, w, b, g, be, F, T, s));
  CK(sw(c, "combined_encoder.0.weight", &w)); CK(sw(c, "combined_encoder.0.bias", &b));
  CK(launch_gemm(slin(F, 192, w, b, X2, T, 64), s));
  CK(sw(c, "combined_encoder.1.weight", &g)); CK(sw(c, "combined_encoder.1.bias", &be));
  CK(scene_ln64(X2, g, be, COMB, T, 1, s));
  const int dims[3] = {64, 96, 160};
  int off = 0;
  for (int i = 0; i < 3; ++i) {
    const float* xin = COMB;
    for (int j = 0; j < 3; ++j) {
      const std::string t = "set_transformers." + std::to_string(i) + "." + std::to_string(j);
      CK(sw(c, t + ".norm1.weight", &g)); CK(sw(c, t + ".norm1.bias", &be));
      CK(scene_ln64(xin, g, be, LNb, T, 0, s));
      CK(sw(c, t + ".attn.qkv.weight", &w));
      CK(launch_gemm(slin(LNb, 64, w, nullptr, QKV, T, 192), s));
      CK(scene_attention_seg(QKV, LNb, tb.tiles, tb.n_tiles, 4, 16, 0.25f, s));
      CK(sw(c, t + ".attn.proj.weight", &w)); CK(sw(c, t + ".attn.proj.bias", &b));
      CK(launch_gemm(slin(LNb, 64, w, b, X2, T, 64, xin), s));
      CK(sw(c, t + ".norm2.weight", &g)); CK(sw(c, t + ".norm2.bias", &be));
      CK(scene_ln64(X2, g, be, LNb, T, 0, s));
      CK(sw(c, t + ".mlp.0.weight", &w)); CK(sw(c, t + ".mlp.0.bias", &b));
      CK(launch_gemm(slin(LNb, 64, w, b, Hb, T, 256), s));
      CK(scene_affine_act(Hb, nullptr, nullptr, nullptr, Hb, (long)T * 256, 256, 1, s));
      CK(sw(c, t + ".mlp.3.weight", &w)); CK(sw(c, t + ".mlp.3.bias", &b));
      CK(launch_gemm(slin(Hb, 256, w, b, X, T, 64, X2), s));
      xin = X;
    }
    const int d = dims[i];
    const std::string q = "poolings." + std::to_string(i);
    CK(scene_colreduce_seg(X, P0, tb.scene_first, Ns, 64, 64, 0, s));           // mean over each scene's own tokens
    CK(sw(c, q + ".0.weight", &w)); CK(sw(c, q + ".0.bias", &b));
    CK(launch_gemm(slin(P0, 64, w, b, P1, Ns, d), s));
    CK(scene_affine_act(P1, nullptr, nullptr, nullptr, P1, (long)Ns * d, d, 1, s));
    CK(sw(c, q + ".2.weight", &w)); CK(sw(c, q + ".2.bias", &b));
    GemmArgs last = slin(P1, d, w, b, out + off, Ns, d);
    last.ldc = CTX;                                                            // a scene's three pooled parts side by side in its latent row
    CK(launch_gemm(last, s));
    off += d;
  }
  return 0;
}

// cloud: the pass's points (T, 3); out: the pass's first latent row (n_scenes, 256)
int encode_scenes_3d(ramp_ctx* c, const float* cloud, const EncodeTables& tb, float* out, hipStream_t s) {
  const int T = tb.n_points, No = tb.n_obstacles, Ns = tb.n_scenes, E = 256;
  float* p = c->scene_ws;
  float* H1 = p; p += (size_t)T * 64;
  float* H2 = p; p += (size_t)T * E;
  float* X = p; p += (size_t)No * E; float* X2 = p; p += (size_t)No * E;
  float* LNb = p; p += (size_t)No * E; float* O = p; p += (size_t)No * E;
  float* QKV = p; p += (size_t)No * 768; float* Hb = p; p += (size_t)No * 512;
  float* sc = p; p += 256; float* sh = p; p += 256; float* S0 = p; p += (size_t)Ns * E; float* S1 = p; p += (size_t)Ns * E;
  float *w, *b, *g, *be, *rm, *rv;
  CK(sw(c, "point_processor.conv1.weight", &w)); CK(sw(c, "point_processor.conv1.bias", &b));
  CK(scene_linear_small(cloud, w, b, H1, T, 64, 3, s));
  CK(sw(c, "point_processor.bn1.weight", &g)); CK(sw(c, "point_processor.bn1.bias", &be));
  CK(sw(c, "point_processor.bn1.running_mean", &rm)); CK(sw(c, "point_processor.bn1.running_var", &rv));
  CK(scene_bn_fold(g, be, rm, rv, sc, sh, 64, s));
  CK(scene_affine_act(H1, sc, sh, nullptr, H1, (long)T * 64, 64, 2, s));
  CK(sw(c, "point_processor.conv2.weight", &w)); CK(sw(c, "point_processor.conv2.bias", &b));
  CK(launch_gemm(slin(H1, 64, w, b, H2, T, E), s));
  CK(sw(c, "point_processor.bn2.weight", &g)); CK(sw(c, "point_processor.bn2.bias", &be));
  CK(sw(c, "point_processor.bn2.running_mean", &rm)); CK(sw(c, "point_processor.bn2.running_var", &rv));
  CK(scene_bn_fold(g, be, rm, rv, sc, sh, E, s));
  CK(scene_affine_act(H2, sc, sh, nullptr, H2, (long)T * E, E, 2, s));
  CK(scene_colreduce_seg(H2, X, tb.obstacle_first, No, E, E, 1, s));            // max over the points of each obstacle
  for (int i = 0; i < 2; ++i) {
    const std::string t = "set_transformer_blocks." + std::to_string(i);
    CK(sw(c, t + ".norm1.weight", &g)); CK(sw(c, t + ".norm1.bias", &be));
    CK(launch_ln_fwd(X, g, be, LNb, No, s));
    CK(sw(c, t + ".mha.in_proj_weight", &w)); CK(sw(c, t + ".mha.in_proj_bias", &b));
    CK(launch_gemm(slin(LNb, E, w, b, QKV, No, 768), s));
    CK(scene_attention_seg(QKV, O, tb.tiles, tb.n_tiles, 4, 64, 0.125f, s));
    CK(sw(c, t + ".mha.out_proj.weight", &w)); CK(sw(c, t + ".mha.out_proj.bias", &b));
    CK(launch_gemm(slin(O, E, w, b, X2, No, E, X), s));
    CK(sw(c, t + ".norm2.weight", &g)); CK(sw(c, t + ".norm2.bias", &be));
    CK(launch_ln_fwd(X2, g, be, LNb, No, s));
    CK(sw(c, t + ".ffn.0.weight", &w)); CK(sw(c, t + ".ffn.0.bias", &b));
    CK(launch_gemm(slin(LNb, E, w, b, Hb, No, 512), s));
    CK(scene_affine_act(Hb, nullptr, nullptr, nullptr, Hb, (long)No * 512, 512, 2, s));
    CK(sw(c, t + ".ffn.3.weight", &w)); CK(sw(c, t + ".ffn.3.bias", &b));
    CK(launch_gemm(slin(Hb, 512, w, b, X, No, E, X2), s));
  }
  CK(sw(c, "output_proj.weight", &w)); CK(sw(c, "output_proj.bias", &b));
  CK(launch_gemm(slin(X, E, w, b, O, No, E), s));
  CK(scene_colreduce_seg(O, S0, tb.scene_first, Ns, E, E, 1, s));               // max over the obstacles of each scene
  CK(sw(c, "global_pooling.0.weight", &w)); CK(sw(c, "global_pooling.0.bias", &b));
  CK(launch_gemm(slin(S0, E, w, b, S1, Ns, E), s));
  CK(scene_affine_act(S1, nullptr, nullptr, nullptr, S1, (long)Ns * E, E, 2, s));
  CK(sw(c, "global_pooling.2.weight", &w)); CK(sw(c, "global_pooling.2.bias", &b));
  CK(launch_gemm(slin(S1, E, w, b, out, Ns, E), s));
  return 0;
}


// ---- device buffers of the job layer: typed, grow-only, from the arena (which never frees: an old block stays valid for whatever still holds
// its address).  A captured graph holds the addresses of the buffers its nodes touch, so every reallocation is noted in the context and
// staging_done() -- once per job, after its staging and before a graph is chosen -- drops the keys of BOTH graph families: the sampling jobs'
// and the replans' graphs read the same s_x, s_eps, s_x0 and operand-maxima tables, and one re-capture after a growth is the whole cost.
template <class T> int renew(ramp_ctx* c, T*& p, size_t n) {      // p = a new block of n T
  float* q;
  CK(dev_alloc(c, &q, (n * sizeof(T) + sizeof(float) - 1) / sizeof(float)));
  // (a first allocation moves nothing -- PROVIDED that a graph captured while the buffer did not exist never meets it: the graph keys carry
  // whatever decides that a job touches an optional buffer, see where they are built)
  if (p) c->buffers_moved = true;
  p = reinterpret_cast<T*>(q);
  return 0;
}
template <class T> int grow(ramp_ctx* c, T*& p, size_t& cap, size_t n) {
  if (n > cap) { CK(renew(c, p, n)); cap = n; }
  return 0;
}
// a job's table of n elements into its grow-only buffer (at least `floor` elements, so that an empty table has an address too); a copy from
// pageable host memory is staged before the call returns
template <class T> int stage_table(ramp_ctx* c, T*& p, size_t& cap, const T* src, size_t n, size_t floor, hipMemcpyKind kind, hipStream_t s) {
  CK(grow(c, p, cap, std::max(floor, n)));
  if (n) RAMP_HIP_CHECK(hipMemcpyAsync(p, src, n * sizeof(T), kind, s));
  return 0;
}
void staging_done(ramp_ctx* c) {
  if (c->buffers_moved) { c->graph_key.clear(); c->e_key.clear(); c->buffers_moved = false; }
}

int ensure_sampler_buffers(ramp_ctx* c, int B, int n_rp, int n_steps, bool chain) {
  const size_t HS = (size_t)c->cfg.horizon * c->cfg.state_dim;
  if ((size_t)B > c->s_cap_B) {
    CK(renew(c, c->s_x, B * HS)); CK(renew(c, c->s_mean, B * HS)); CK(renew(c, c->s_x0, B * HS));
    c->s_cap_B = B;
  }
  CK(grow(c, c->s_eps, c->s_eps_cap, (size_t)B * n_rp * HS));
  const size_t nn = (size_t)(n_steps + 1) * B * HS;
  CK(grow(c, c->s_noise, c->s_noise_cap, nn));
  if (chain) CK(grow(c, c->s_chain, c->s_chain_cap, nn));
  return 0;
}

// one score evaluation over all rows of a batch, chunked to the context capacity
// comb != nullptr (n_rp host floats; sampling jobs): the rows of a trajectory share the network prefix they have in
// common and eps_out receives (B, H, S) = sum_j comb[j] * eps of row j instead of the (B n_rp, H, S) row gradients.
// In a composed job (c->g_weight_cur set) comb is ONLY that non-null flag: the weights are the lines of the device table and combine_prefix
// never reads comb, which holds three floats whatever n_rp is
int score_all(ramp_ctx* c, const float* x, int B, int n_rp, int t, float* f_out, float* eps_out, hipStream_t s,
              const float* comb = nullptr) {
  const int H = c->cfg.horizon, S = c->cfg.state_dim;
  RAMP_REQUIRE(c->finalized, "weights not finalized");
  RAMP_REQUIRE(c->time_table != nullptr && t >= 0 && t < c->tt_T, "timestep outside the prepared time table");
  RAMP_REQUIRE(c->cross_bias != nullptr, "ramp_set_scene has not been called");
  RAMP_REQUIRE(B > 0 && n_rp >= 1 && n_rp <= RAMP_MAX_ROWS_PER_TRAJ, "bad batch");
  RAMP_REQUIRE(c->row_variant_cap >= B * n_rp, "row-variant table shorter than the batch (call ramp_set_scene after sizing)");
  RAMP_REQUIRE(c->rv_rows == 0 || B * n_rp <= c->rv_rows, "the batch has more rows (B * n_rp) than the row -> variant table given to ramp_set_scenes");
  const int cap_traj = c->cfg.max_rows / n_rp;
  RAMP_REQUIRE(cap_traj >= 1, "max_rows smaller than n_rp");
  for (int b0 = 0; b0 < B; b0 += cap_traj) {
    const int nb = std::min(cap_traj, B - b0), R = nb * n_rp, row0 = b0 * n_rp;
    float* fo = f_out ? f_out + (size_t)row0 * H * S : nullptr;
    c->site = 0;                                       // every chunk walks the same GEMM call sites
    const int share = (comb && n_rp > 1 && c->share_prefix) ? n_rp : 1;
    // (a combined evaluation hands out f only as the scratch its rows' energies are taken from)
    RAMP_REQUIRE(!comb || (eps_out && (!f_out || c->e_rows_cur)), "combined evaluation: gradient (and energies) only");
    RAMP_REQUIRE(!c->e_rows_cur || f_out, "energies need f of every row");
    CK(net_forward(c, x + (size_t)b0 * H * S, row0, R, n_rp, t, fo, eps_out != nullptr, s, share));
    if (c->e_rows_cur) LAUNCH(c, s, CAT_SAMPLER, 0, launch_row_energy(fo, c->e_rows_cur + row0, R, H * S, s));
    if (eps_out && share > 1) CK(net_backward(c, row0, R, eps_out + (size_t)b0 * H * S, s, share, comb));
    else if (eps_out) CK(net_backward(c, row0, R, eps_out + (size_t)row0 * H * S, s));
  }
  return 0;
}

// One score evaluation of a job under the fp16x3 delayed scaling.  phase 1: the bf16x6 kernels, recording every GEMM call site's operand
// maximum; 2: fp16x3 scaled from the maxima in table t_in; both write their own maxima into table t_out, zeroed first.  phase 0: the context's
// plain arithmetic (bf16x6 / exact fp32), no tables.  log != nullptr: the range guard's word after the evaluation goes to log[j].
int guarded_eval(ramp_ctx* c, int phase, int t_in, int t_out, const float* x, int B, int n_rp, int t, float* f_out, float* eps_out,
                 hipStream_t s, const float* comb = nullptr, int* log = nullptr, int j = 0) {
  if (phase) {
    c->obs_in = c->table(t_in); c->obs_out = c->table(t_out);
    hipLaunchKernelGGL(zero_words_kernel, dim3(ramp_ctx::MAX_SITES / 256), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->obs_out), ramp_ctx::MAX_SITES);
    RAMP_HIP_CHECK(hipGetLastError());
  }
  c->phase = phase;
  const int rc = score_all(c, x, B, n_rp, t, f_out, eps_out, s, comb);
  c->phase = 0;
  CK(rc);
  if (log) {
    hipLaunchKernelGGL(log_flag_kernel, dim3(1), dim3(64), 0, s, c->range_flag, log, j);
    RAMP_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// the weights of the rows' gradients in e_comb (diffusion_model_static.py:164-165, 214; CFG: (1 + w) e_cond - w e_uncond): the network prefix
// the rows of a trajectory have in common is evaluated once and its input gradient once, on the combined gradient
std::array<float, 3> comb_weights(int n_rp, double w0, double w1) {
  if (n_rp == 2) return {(float)(1.0 + w0), -(float)w0, (float)(1.0 - w0 - w1)};
  return {(float)w0, (float)w1, (float)(1.0 - w0 - w1)};
}

// ---- captured graphs: *slot empty -> body(capture stream) is captured and instantiated into it; then *slot is launched on s
template <class Body> int replay(hipGraphExec_t* slot, hipStream_t s, Body&& body) {
  if (!*slot) {
    hipStream_t cs;
    RAMP_HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    RAMP_HIP_CHECK(hipStreamSynchronize(s));
    RAMP_HIP_CHECK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    int rc = body(cs);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc != 0) { if (g) (void)hipGraphDestroy(g); (void)hipStreamDestroy(cs); return rc; }
    if (e != hipSuccess) { (void)hipStreamDestroy(cs); RAMP_HIP_CHECK(e); }
    e = hipGraphInstantiate(slot, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g); (void)hipStreamDestroy(cs);
    RAMP_HIP_CHECK(e);
  }
  RAMP_HIP_CHECK(hipGraphLaunch(*slot, s));
  return 0;
}
void drop_graphs(hipGraphExec_t* slots, int n) {
  for (int i = 0; i < n; ++i) if (slots[i]) { (void)hipGraphExecDestroy(slots[i]); slots[i] = nullptr; }
}

// the key of a captured graph / a kept calibration: the bytes of everything baked into it
struct Key {
  std::string bytes;
  template <class T> void put(const T& v) {
    static_assert(!std::is_pointer<T>::value && !std::is_array<T>::value, "an array goes in with its count: put(a, n)");
    bytes.append(reinterpret_cast<const char*>(&v), sizeof(T));
  }
  template <class T> void put(const T* a, size_t count) { bytes.append(reinterpret_cast<const char*>(a), sizeof(T) * count); }
};

// kept fp16x3 calibrations that a change makes stale: the single evaluations' tables (ramp_score), the replans' carried table, the sampling
// jobs' canonical table
enum { CAL_SCORE = 1, CAL_REPLAN = 2, CAL_CANONICAL = 4, CAL_ALL = 7 };
void invalidate_calibrations(ramp_ctx* c, int what) {
  if (what & CAL_SCORE) c->score_calibrated = false;
  if (what & CAL_REPLAN) c->replan_carry = ramp_ctx::REPLAN_NOBODY;
  if (what & CAL_CANONICAL) c->c_cal_valid = false;
}
// ramp_score's evaluations end the single entry's carried calibration and leave the episode entry's: an asymmetry inherited as it is
void forget_single_replan_carry(ramp_ctx* c) {
  if (c->replan_carry == ramp_ctx::REPLAN_SINGLE) c->replan_carry = ramp_ctx::REPLAN_NOBODY;
}

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char* ramp_last_error(void) { return last_error_cstr(); }
int ramp_version(void) { return 1; }

int ramp_create(const ramp_config* cfg, ramp_ctx** out) {
  RAMP_REQUIRE(cfg && out, "null argument");
  RAMP_REQUIRE(cfg->state_dim >= 2 && cfg->state_dim <= 16, "state_dim out of range");
  RAMP_REQUIRE((cfg->n_levels == 3 || cfg->n_levels == 4) && (cfg->unet_input_dim == 16 || cfg->unet_input_dim == 32 || cfg->unet_input_dim == 64),
               "network shape: n_levels in {3, 4} (UNET_DIM_MULTS[0] = (1,2,4), [1] = (1,2,4,8)) and unet_input_dim in {16, 32, 64}");
  RAMP_REQUIRE(cfg->horizon >= 8 && cfg->horizon <= 64 && cfg->horizon % 8 == 0, "horizon (n_support_points) must be a multiple of 8 in [8, 64] (three stride-2 levels; attention tiles of at most 64 tokens)");
  RAMP_REQUIRE(cfg->context_dim > 0 && cfg->context_dim <= 512, "context_dim out of range");
  RAMP_REQUIRE(cfg->max_rows >= 1, "max_rows must be positive");
  int ndev = 0;
  RAMP_HIP_CHECK(hipGetDeviceCount(&ndev));
  RAMP_REQUIRE(ndev > 0, "no HIP device: the RAMP sampler has no CPU fallback");
  auto* c = new ramp_ctx();
  c->cfg = *cfg;
  RAMP_HIP_CHECK(hipGetDevice(&c->device));
  {   // the environment only supplies DEFAULTS of the launch plan / arithmetic mode, read here and nowhere below
    const char* env = getenv("RAMP_GEMM_MODE");
    c->gemm_mode = cfg->gemm_mode == 1 ? 0 : cfg->gemm_mode == 2 ? 1 : cfg->gemm_mode == 3 ? 2
                 : (env && std::string(env) == "fp16x3") ? 2 : (env && std::string(env) == "bf16x6") ? 1
                 : (env && std::string(env) == "fp32") ? 0 : RAMP_DEFAULT_GEMM_MODE;
    const char* pe = getenv("RAMP_X6_PIPE");
    c->x6_pipe = !(pe && pe[0] == '0');
    const char* fe = getenv("RAMP_FF_FUSED");
    if (fe) c->ff_fused = atoi(fe);
    const char* xe = getenv("RAMP_FFX");
    if (xe) c->ffx_min_rows = atoi(xe);
    if (const char* me = getenv("RAMP_MFMA16")) c->mfma16 = atoi(me) != 0;
    const char* ke = getenv("RAMP_TKL");
    if (ke) c->tkl_min_rows = atoi(ke);
    const char* tce = getenv("RAMP_TKC");
    if (tce) c->tkc_min_rows = atoi(tce);
    if (const char* tg = getenv("RAMP_TKC_GN")) c->tkc_gn = atoi(tg) & 3;
    const char* twe = getenv("RAMP_TKW");
    if (twe) c->tkw_min_rows = atoi(twe);
    const char* ate = getenv("RAMP_ATK");
    if (ate) c->atk_min_rows = atoi(ate);
    const char* se = getenv("RAMP_SHARE_PREFIX");
    if (se) c->share_prefix = atoi(se) != 0;
    const char* te = getenv("RAMP_X6_THREE");
    if (te) c->three_blocks = te[0] != '0';
    c->prof_dump = getenv("RAMP_PROFILE_DUMP") != nullptr;
    const char* ae = getenv("RAMP_FFX_ABLATE");              // diagnostic A/B of the fused feed-forward inside a whole job
    if (ae) {   // only the variants that compute the SAME result may ride a product launch (16: LayerNorm tables from LDS, 32: no
                // bounding wait at the tile switch, 48: both); the result-changing twins (1, 2, 4, 8, ...) stay in ramp_bench_gemm
      const int av = atoi(ae);
      if (!(av == 0 || av == 16 || av == 32 || av == 48)) {
        delete c;
        RAMP_REQUIRE(false, "RAMP_FFX_ABLATE accepts 0, 16, 32 or 48 (result-preserving variants) on a context; the others change results and exist in ramp_bench_gemm only");
      }
      c->ffx_ablate = av;
    }
    c->tklb_off = getenv("RAMP_TKLB_OFF") != nullptr;
    if (const char* e = getenv("RAMP_ABL")) c->abl_on = atoi(e) != 0;      // diagnostic: 0 = attention backward and d(ln1) as separate launches       // diagnostic: d(ln1) + LN1 backward on the tile kernel + ln_bwd pair
  }
  *out = c;
  return 0;
}

int ramp_get_launch_plan(ramp_ctx* c, ramp_launch_plan* out) {
  RAMP_REQUIRE(c && out, "null argument");
  *out = ramp_launch_plan{c->ff_fused, c->ffx_min_rows, c->share_prefix, c->three_blocks, c->x6_pipe, c->tkl_min_rows, c->atk_min_rows, c->tkc_min_rows, c->tkw_min_rows, c->mfma16};
  return 0;
}
int ramp_set_launch_plan(ramp_ctx* c, const ramp_launch_plan* p) {
  RAMP_REQUIRE(c && p, "null argument");
  RAMP_REQUIRE(p->ff_fused_rows >= 0 && p->ffx_rows >= 0 && p->tkl_rows >= 0 && p->atk_rows >= 0 && p->tkc_rows >= 0 && p->tkw_rows >= 0, "row thresholds must be >= 0");
  RAMP_REQUIRE(!c->finalized || (p->x6_pipe != 0) == (c->x6_pipe != 0), "x6_pipe is fixed once the weights are packed (ramp_finalize_weights)");
  const bool changed = p->ff_fused_rows != c->ff_fused || p->ffx_rows != c->ffx_min_rows || (p->share_prefix != 0) != (c->share_prefix != 0) ||
                       (p->three_blocks != 0) != (c->three_blocks != 0) || p->tkl_rows != c->tkl_min_rows || p->atk_rows != c->atk_min_rows ||
                       p->tkc_rows != c->tkc_min_rows || p->tkw_rows != c->tkw_min_rows || (p->mfma16 != 0) != (c->mfma16 != 0);
  c->ff_fused = p->ff_fused_rows; c->ffx_min_rows = p->ffx_rows; c->tkl_min_rows = p->tkl_rows; c->share_prefix = p->share_prefix != 0;
  c->atk_min_rows = p->atk_rows; c->tkc_min_rows = p->tkc_rows; c->tkw_min_rows = p->tkw_rows;
  c->three_blocks = p->three_blocks != 0; c->x6_pipe = p->x6_pipe != 0; c->mfma16 = p->mfma16 != 0;
  if (changed && c->finalized) {   // other kernels from here on: captured graphs and kept calibrations belong to the old plan
    c->graph_key.clear(); c->e_key.clear();
    invalidate_calibrations(c, CAL_ALL);
  }
  return 0;
}

int ramp_destroy(ramp_ctx* c) {
  if (!c) return 0;
  drop_graphs(c->s_graph, 3);
  drop_graphs(c->e_graph, 2);
  if (c->d_ptr_tables) (void)hipFree(c->d_ptr_tables);
  delete c;
  return 0;
}

int ramp_load_weight(ramp_ctx* c, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
  RAMP_REQUIRE(c && name && data && (shape || ndim == 0), "null argument");
  RAMP_REQUIRE(!c->finalized, "weights already finalized");
  std::string key(name);
  size_t n = 1; std::vector<int64_t> shp;
  for (int i = 0; i < ndim; ++i) { RAMP_REQUIRE(shape[i] > 0, "bad shape"); n *= (size_t)shape[i]; shp.push_back(shape[i]); }
  float* d; CK(dev_alloc(c, &d, n));
  RAMP_HIP_CHECK(hipMemcpy(d, data, n * sizeof(float), hipMemcpyHostToDevice));
  c->raw[key] = {d, shp};
  return 0;
}

int ramp_finalize_weights(ramp_ctx* c) {
  RAMP_REQUIRE(c && !c->finalized, "bad context state");
  {
    c->geglu_group = (c->gemm_mode >= 1 && c->x6_pipe) ? 32 : 64;
  }
  const int nl = c->cfg.n_levels, S = c->cfg.state_dim, H = c->cfg.horizon, C0 = c->cfg.unet_input_dim;
  const size_t cap = (size_t)c->cfg.max_rows;
  std::vector<int> dims = {S};
  for (int k = 0; k < nl; ++k) dims.push_back(C0 << k);
  int L = H, tb = 0;
  auto add_rtb = [&](const std::string& name, int ci, int co, int len, bool first) {
    RTB r; r.name = name; r.cin = ci; r.cout = co; r.L = len; r.has_res = ci != co; r.first = first; r.tb_off = tb;
    tb += co; c->rtbs.push_back(r);
  };
  int blk = 0;
  auto add_st = [&](const std::string& name, int ch, int len) {
    ST s; s.name = name; s.C = ch; s.L = len; s.blk0 = blk; blk += 2; c->sts.push_back(s);
  };
  for (int k = 0; k < nl; ++k) {
    const std::string p = "downs." + std::to_string(k);
    add_rtb(p + ".0", dims[k], dims[k + 1], L, k == 0);
    add_rtb(p + ".1", dims[k + 1], dims[k + 1], L, false);
    add_st(p + ".3", dims[k + 1], L);
    if (k < nl - 1) {
      Resample d; d.name = p + ".4"; d.C = dims[k + 1]; d.Lin = L; d.Lout = L / 2; d.taps = 3;
      c->downs.push_back(d); L /= 2;
    }
  }
  RAMP_REQUIRE(dims[1] != S, "first block must have a residual conv");
  const int mid = dims[nl];
  add_rtb("mid_block1", mid, mid, L, false);
  add_rtb("mid_block2", mid, mid, L, false);
  add_st("mid_attention", mid, L);
  for (int k = 0; k < nl - 1; ++k) {
    const std::string p = "ups." + std::to_string(k);
    const int ci = dims[nl - 1 - k], co = dims[nl - k];      // (dim_in, dim_out) of reversed(in_out[1:])
    add_rtb(p + ".0", co * 2, ci, L, false);
    add_rtb(p + ".1", ci, ci, L, false);
    add_st(p + ".3", ci, L);
    Resample u; u.name = p + ".4"; u.C = ci; u.Lin = L; u.Lout = 2 * L; u.taps = 4;
    c->ups.push_back(u); L *= 2;
  }
  RAMP_REQUIRE(L == H, "level bookkeeping");
  c->tt_stride = tb; c->n_blocks_total = blk;
  for (auto& r : c->rtbs) CK(build_rtb(c, r));
  for (auto& s : c->sts) CK(build_st(c, s));
  for (auto& d : c->downs) {
    float *raw, *t;
    CK(get_raw(c, d.name + ".conv.weight", {d.C, d.C, 3}, &raw));
    CK(get_raw(c, d.name + ".conv.bias", {d.C}, &d.bias));
    CK(permute3(c, raw, d.C, d.C, 3, 2, 0, 1, &d.w_f));      // forward taps [j][co][ci] = W[co][ci][j]
    CK(permute3(c, raw, d.C, d.C, 3, 2, 1, 0, &t));          // dX taps      [j][ci][co]
    // even output rows use tap 1, odd rows taps (0, 2): store [W_1 | W_0 | W_2]
    const size_t cc2 = (size_t)d.C * d.C;
    CK(dev_alloc(c, &d.w_b, 3 * cc2));
    RAMP_HIP_CHECK(hipMemcpy(d.w_b, t + cc2, cc2 * 4, hipMemcpyDeviceToDevice));
    RAMP_HIP_CHECK(hipMemcpy(d.w_b + cc2, t, cc2 * 4, hipMemcpyDeviceToDevice));
    RAMP_HIP_CHECK(hipMemcpy(d.w_b + 2 * cc2, t + 2 * cc2, cc2 * 4, hipMemcpyDeviceToDevice));
    CK(dev_alloc(c, &d.a_y, cap * d.Lout * d.C));
  }
  for (auto& u : c->ups) {
    float *raw, *t;
    CK(get_raw(c, u.name + ".conv.weight", {u.C, u.C, 4}, &raw));   // ConvTranspose1d (Cin,Cout,4)
    CK(get_raw(c, u.name + ".conv.bias", {u.C}, &u.bias));
    CK(permute3(c, raw, u.C, u.C, 4, 2, 1, 0, &t));          // forward taps [j][co][ci] = W[ci][co][j]
    // even output rows use taps (1, 3), odd rows taps (0, 2): store [W_1 | W_3 | W_0 | W_2]
    const size_t cc2 = (size_t)u.C * u.C;
    CK(dev_alloc(c, &u.w_f, 4 * cc2));
    const int order[4] = {1, 3, 0, 2};
    for (int q = 0; q < 4; ++q)
      RAMP_HIP_CHECK(hipMemcpy(u.w_f + q * cc2, t + order[q] * cc2, cc2 * 4, hipMemcpyDeviceToDevice));
    CK(permute3(c, raw, u.C, u.C, 4, 2, 0, 1, &u.w_b));      // dX taps [j][ci][co] = W[ci][co][j]
    CK(dev_alloc(c, &u.a_y, cap * u.Lout * u.C));
  }
  CK(pack_conv5(c, "final_conv.0.block.0", C0, C0, &c->final_conv));
  CK(get_raw(c, "final_conv.0.block.2.weight", {C0}, &c->fin_g));
  CK(get_raw(c, "final_conv.0.block.2.bias", {C0}, &c->fin_b));
  CK(get_raw(c, "final_conv.1.weight", {S, C0, 1}, &c->fin_w));
  CK(get_raw(c, "final_conv.1.bias", {S}, &c->fin_bias));
  for (const char* k : {"time_mlp.encoder.1.weight", "time_mlp.encoder.1.bias", "time_mlp.encoder.3.weight",
                        "time_mlp.encoder.3.bias"})
    RAMP_REQUIRE(c->raw.count(k), std::string("missing weight '") + k + "'");
  CK(dev_alloc(c, &c->a_fin_c, cap * H * C0)); CK(dev_alloc(c, &c->a_fin_st, cap * 16));
  CK(dev_alloc(c, &c->a_fin_a, cap * H * C0)); CK(dev_alloc(c, &c->a_fin_da, cap * H * C0));
  // shared temporaries
  size_t max_lc = 0, max_l = 0;
  for (auto& r : c->rtbs) max_lc = std::max(max_lc, (size_t)r.L * std::max(r.cin, r.cout));
  for (auto& s : c->sts) max_l = std::max(max_l, (size_t)s.L);
  max_lc = std::max(max_lc, (size_t)H * C0);
  CK(dev_alloc(c, &c->t_res, cap * max_lc)); CK(dev_alloc(c, &c->t_xn, cap * max_lc));
  CK(dev_alloc(c, &c->t_ln, cap * max_l * 256)); CK(dev_alloc(c, &c->t_o, cap * max_l * 256));
  CK(dev_alloc(c, &c->t_hg, cap * max_l * 1024)); CK(dev_alloc(c, &c->t_dag, cap * max_l * 2048));
  CK(dev_alloc(c, &c->t_dqkv, cap * max_l * 768)); CK(dev_alloc(c, &c->t_dln, cap * max_l * 256));
  CK(dev_alloc(c, &c->t_dz, cap * max_l * 256)); CK(dev_alloc(c, &c->t_dz1, cap * max_l * 256));
  CK(dev_alloc(c, &c->g_a, cap * max_lc)); CK(dev_alloc(c, &c->g_b, cap * max_lc));
  CK(dev_alloc(c, &c->g_t1, cap * max_lc)); CK(dev_alloc(c, &c->g_t2, cap * max_lc)); CK(dev_alloc(c, &c->g_tr, cap * max_lc));
  c->skip_grad.assign(nl, nullptr);
  for (int k = 1; k < nl; ++k) CK(dev_alloc(c, &c->skip_grad[k], cap * c->sts[k].L * c->sts[k].C));
  // bf16x6 planes of every GEMM weight with N >= 128
  if (c->gemm_mode >= 1) {
    auto reg = [&](const float* w, size_t n, int K) -> int {
      if (!w || c->x6.count(w)) return 0;
      float *p, *q = nullptr;
      CK(dev_alloc(c, &p, (3 * n + 1) / 2 + 4));
      CK(launch_split3(w, reinterpret_cast<unsigned short*>(p), (long)n, 0));
      if (n % K == 0 && (n / K) % 32 == 0 && K % 16 == 0) {
        CK(dev_alloc(c, &q, (3 * n + 1) / 2 + 4));
        CK(launch_pack_x6(w, reinterpret_cast<unsigned short*>(q), (long)(n / K), K, 0));
      }
      float* q3 = nullptr; float wsi = 1.f;
      if (q && c->gemm_mode == 2) {
        float sc = 1.f; CK(device_weight_scale(w, n, &sc));          // static power-of-two weight scale: max |w| -> [2^10, 2^11)
        CK(dev_alloc(c, &q3, n + 4));
        CK(launch_pack_h3(w, reinterpret_cast<unsigned short*>(q3), (long)(n / K), K, sc, 0));
        wsi = 1.f / sc;
      }
      c->x6[w] = {reinterpret_cast<unsigned short*>(p), n, K, reinterpret_cast<unsigned short*>(q),
                  reinterpret_cast<unsigned short*>(q3), wsi};
      return 0;
    };
    if (c->gemm_mode == 2) {
      const size_t nt = (size_t)ramp_ctx::N_OBS_TABLES * ramp_ctx::MAX_SITES;
      float* o; CK(dev_alloc(c, &o, nt + 4));
      c->obs = o; c->range_flag = reinterpret_cast<int*>(o + nt);
      RAMP_HIP_CHECK(hipMemset(o, 0, (nt + 4) * sizeof(float)));
    }
    for (auto& r : c->rtbs) {
      if (!r.first) { CK(reg(r.c1.fwd, 5ul * r.cin * r.cout, r.cin)); CK(reg(r.c1.bwd, 5ul * r.cin * r.cout, r.cout)); }
      CK(reg(r.c2.fwd, 5ul * r.cout * r.cout, r.cout)); CK(reg(r.c2.bwd, 5ul * r.cout * r.cout, r.cout));
      if (r.has_res && !r.first) { CK(reg(r.res_f, (size_t)r.cin * r.cout, r.cin)); CK(reg(r.res_b, (size_t)r.cin * r.cout, r.cout)); }
    }
    for (auto& st : c->sts) {
      CK(reg(st.wpi_f, 256ul * st.C, st.C)); CK(reg(st.wpi_b, 256ul * st.C, 256));
      CK(reg(st.wpo_f, 256ul * st.C, 256)); CK(reg(st.wpo_b, 256ul * st.C, st.C));
      for (auto& k : st.blk) {
        CK(reg(k.wqkv_f, 768ul * 256, 256)); CK(reg(k.wqkv_b, 768ul * 256, 768));
        CK(reg(k.wo_f, 256ul * 256, 256)); CK(reg(k.wo_b, 256ul * 256, 256));
        CK(reg(k.w1_pk, 2048ul * 256, 256)); CK(reg(k.w1_b, 2048ul * 256, 2048));
        CK(reg(k.w2_f, 1024ul * 256, 1024)); CK(reg(k.w2_b, 1024ul * 256, 256));
      }
    }
    if (c->gemm_mode == 2 && c->x6_pipe && c->geglu_group == 32) {
      // weight streams of the token-owning fused feed-forward: first products from the fragment planes the tile kernels use,
      // second products re-packed with the k order of the first one's accumulator rows (ffx_pack_second)
      float* tmp; CK(dev_alloc(c, &tmp, 2048 * 256));
      unsigned short *p2f, *p2b;
      { float* q; CK(dev_alloc(c, &q, 256 * 1024 + 4)); p2f = reinterpret_cast<unsigned short*>(q); }
      { float* q; CK(dev_alloc(c, &q, 256 * 2048 + 4)); p2b = reinterpret_cast<unsigned short*>(q); }
      unsigned short* p1x; { float* q; CK(dev_alloc(c, &q, 256 * 2048 + 4)); p1x = reinterpret_cast<unsigned short*>(q); }
      for (auto& st : c->sts)
        for (auto& k : st.blk) {
          const auto& e1 = c->x6.at(k.w1_pk); const auto& e1b = c->x6.at(k.w1_b);
          const auto& e2 = c->x6.at(k.w2_f); const auto& e2b = c->x6.at(k.w2_b);
          RAMP_REQUIRE(e1.packed3 && e2b.packed3 && e1.w_scale_inv == e1b.w_scale_inv && e2.w_scale_inv == e2b.w_scale_inv, "ffx: weight planes missing");
          float *sf, *sb; CK(dev_alloc(c, &sf, 96 * 8192 + 4)); CK(dev_alloc(c, &sb, 96 * 8192 + 4));
          k.ffx_f = reinterpret_cast<unsigned short*>(sf); k.ffx_b = reinterpret_cast<unsigned short*>(sb);
          CK(ffx_pack_second(k.w2_f, 256, 1024, 0, 1.f / e2.w_scale_inv, tmp, p2f, 0));
          CK(ffx_build_stream(e1.packed3, p2f, k.ffx_f, false, 0));
          CK(ffx_pack_second(k.w1_b, 256, 2048, 1, 1.f / e1.w_scale_inv, tmp, p2b, 0));
          CK(ffx_build_stream(e2b.packed3, p2b, k.ffx_b, true, 0));
          k.ffx_wsi_w1 = e1.w_scale_inv; k.ffx_wsi_w2 = e2.w_scale_inv;
          // the same two streams in 16 x 32 fragments for the v_mfma_f32_16x16x32_f16 kernels (ffx16.hip), same scales
          float *sf6, *sb6; CK(dev_alloc(c, &sf6, 96 * 8192 + 4)); CK(dev_alloc(c, &sb6, 96 * 8192 + 4));
          k.ffx16_f = reinterpret_cast<unsigned short*>(sf6); k.ffx16_b = reinterpret_cast<unsigned short*>(sb6);
          CK(ffx16_pack(k.w1_pk, 2048, 256, 0, 1.f / e1.w_scale_inv, tmp, p1x, 0));
          CK(ffx16_pack(k.w2_f, 256, 1024, 1, 1.f / e2.w_scale_inv, tmp, p2f, 0));
          CK(ffx16_build_stream(p1x, p2f, k.ffx16_f, false, 0));
          CK(ffx16_pack(k.w2_b, 1024, 256, 0, 1.f / e2.w_scale_inv, tmp, p1x, 0));
          CK(ffx16_pack(k.w1_b, 256, 2048, 2, 1.f / e1.w_scale_inv, tmp, p2b, 0));
          CK(ffx16_build_stream(p1x, p2b, k.ffx16_b, true, 0));
          // ... and the K = 256 attention linears the token-owning kernel serves (LN1 -> QKV, out-projection, d(o)) for tkl16.hip
          for (const auto& wn : {std::make_pair((const float*)k.wqkv_f, 768), std::make_pair((const float*)k.wo_f, 256), std::make_pair((const float*)k.wo_b, 256)}) {
            const auto& ew = c->x6.at(wn.first);
            if (!ew.packed3) continue;
            float* q16; CK(dev_alloc(c, &q16, (size_t)wn.second * 256 + 4));          // 2 planes x N x 256 halves
            CK(ffx16_pack(wn.first, wn.second, 256, 0, 1.f / ew.w_scale_inv, tmp, reinterpret_cast<unsigned short*>(q16), 0));
            c->tk16_w[wn.first] = reinterpret_cast<unsigned short*>(q16);
          }
        }
    }
    if (c->gemm_mode == 2 && c->x6_pipe) {
      // weight streams of the fused self-attention + output projection (atk.hip): Wo in head order, k permuted to the row order
      // of the attention output's accumulator tiles, with the scale the tile kernels' planes of the same weight carry
      for (auto& st : c->sts)
        for (auto& k : st.blk) {
          const auto& eo = c->x6.at(k.wo_f);
          float* q; CK(dev_alloc(c, &q, 8 * 8192 + 4));
          k.ato_w = reinterpret_cast<unsigned short*>(q); k.ato_wsi = eo.w_scale_inv;
          CK(ato_pack(k.wo_f, 1.f / eo.w_scale_inv, k.ato_w, 0));
          const auto& eq = c->x6.at(k.wqkv_b);             // the same for the backward half (atl.hip): Wqkv^T in the order its gradient tiles appear
          float* q2; CK(dev_alloc(c, &q2, 256 * 768 + 4));
          k.abl_w = reinterpret_cast<unsigned short*>(q2);
          CK(abl_pack(k.wqkv_b, 1.f / eq.w_scale_inv, k.abl_w, 0));
        }
    }
    if (c->gemm_mode == 2 && c->x6_pipe) {
      // fragment planes of the narrow k = 5 convolutions (tkc.hip), forward and input-gradient weights: static power-of-two scale,
      // max |w| -> [2^10, 2^11) like every other fp16x3 weight
      auto reg_tkc = [&](const float* w, int N, int K) -> int {
        if (!w || c->tkc_w.count(w) || !((N == 32 || N == 64) && (K == 32 || K == 64))) return 0;
        const size_t n = 5ul * N * K;
        float sc = 1.f; CK(device_weight_scale(w, n, &sc));
        float* q; CK(dev_alloc(c, &q, tkc_packed_halves(N, K) / 2 + 4));
        CK(tkc_pack(w, N, K, sc, reinterpret_cast<unsigned short*>(q), 0));
        c->tkc_w[w] = {reinterpret_cast<unsigned short*>(q), 1.f / sc};
        return 0;
      };
      for (auto& r : c->rtbs) {
        if (!r.first) { CK(reg_tkc(r.c1.fwd, r.cout, r.cin)); CK(reg_tkc(r.c1.bwd, r.cin, r.cout)); }
        CK(reg_tkc(r.c2.fwd, r.cout, r.cout)); CK(reg_tkc(r.c2.bwd, r.cout, r.cout));
      }
      CK(reg_tkc(c->final_conv.fwd, C0, C0)); CK(reg_tkc(c->final_conv.bwd, C0, C0));
    }
    for (auto& d : c->downs) { CK(reg(d.w_f, 3ul * d.C * d.C, d.C)); CK(reg(d.w_b, 3ul * d.C * d.C, d.C)); }
    for (auto& u : c->ups) { CK(reg(u.w_f, 4ul * u.C * u.C, u.C)); CK(reg(u.w_b, 4ul * u.C * u.C, u.C)); }
  }
  RAMP_HIP_CHECK(hipDeviceSynchronize());
  CK(init_gemm_attributes());          // hipFuncSetAttribute calls must not happen inside a graph capture
  CK(init_attention_attributes());
  CK(init_ffx_attributes()); CK(init_ffx16_attributes()); CK(init_tkl16_attributes());
  CK(init_tkl_attributes());
  CK(init_atk_attributes());
  CK(init_atl_attributes());
  CK(init_tkc_attributes());
  CK(init_tkw_attributes());
  c->finalized = true;
  return 0;
}

int ramp_prepare_time_table(ramp_ctx* c, int32_t T, void* stream) {
  RAMP_REQUIRE(c && c->finalized && T > 0 && T <= 4096, "bad arguments");
  hipStream_t s = as_stream(stream);
  const int n = (int)c->rtbs.size();
  std::vector<const float*> cw(n), cb(n); std::vector<int> couts(n), offs(n);
  for (int i = 0; i < n; ++i) {
    float *w, *b;
    CK(get_raw(c, c->rtbs[i].name + ".cond_mlp.1.weight", {c->rtbs[i].cout, 32}, &w));
    CK(get_raw(c, c->rtbs[i].name + ".cond_mlp.1.bias", {c->rtbs[i].cout}, &b));
    cw[i] = w; cb[i] = b; couts[i] = c->rtbs[i].cout; offs[i] = c->rtbs[i].tb_off;
  }
  const size_t bytes = n * (2 * sizeof(void*) + 2 * sizeof(int));
  char* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, bytes));
  std::vector<char> h(bytes);
  std::memcpy(h.data(), cw.data(), n * sizeof(void*));
  std::memcpy(h.data() + n * sizeof(void*), cb.data(), n * sizeof(void*));
  std::memcpy(h.data() + 2 * n * sizeof(void*), couts.data(), n * sizeof(int));
  std::memcpy(h.data() + 2 * n * sizeof(void*) + n * sizeof(int), offs.data(), n * sizeof(int));
  RAMP_HIP_CHECK(hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice));
  if (T > c->tt_T) { CK(dev_alloc(c, &c->time_table, (size_t)T * c->tt_stride)); CK(dev_alloc(c, &c->time_temb, (size_t)T * 32)); }
  TimeTableArgs a;
  a.w1 = c->raw["time_mlp.encoder.1.weight"].first; a.b1 = c->raw["time_mlp.encoder.1.bias"].first;
  a.w2 = c->raw["time_mlp.encoder.3.weight"].first; a.b2 = c->raw["time_mlp.encoder.3.bias"].first;
  a.cond_w = reinterpret_cast<const float* const*>(d);
  a.cond_b = reinterpret_cast<const float* const*>(d + n * sizeof(void*));
  a.couts = reinterpret_cast<const int*>(d + 2 * n * sizeof(void*));
  a.offs = reinterpret_cast<const int*>(d + 2 * n * sizeof(void*) + n * sizeof(int));
  a.n_rtb = n; a.table = c->time_table; a.stride = c->tt_stride; a.T = T; a.temb = c->time_temb;
  int rc = launch_time_table(a, s);
  RAMP_HIP_CHECK(hipStreamSynchronize(s));
  RAMP_HIP_CHECK(hipFree(d));
  if (rc) return rc;
  c->tt_T = T;
  return 0;
}

int ramp_time_embedding(ramp_ctx* c, int32_t t, float* out32, void* stream) {
  RAMP_REQUIRE(c && out32 && c->time_temb && t >= 0 && t < c->tt_T, "time table not prepared for this t (ramp_prepare_time_table)");
  RAMP_HIP_CHECK(hipMemcpyAsync(out32, c->time_temb + (size_t)t * 32, 32 * sizeof(float), hipMemcpyDeviceToDevice, as_stream(stream)));
  return 0;
}

// block `module`'s slice of line t of the prepared time table (the tools library's ramp_probe_time_bias, bench.hip)
namespace ramp {
extern "C++" int ctx_time_line(ramp_ctx* c, const char* module, int t, const float** line, int* cout) {
  RAMP_REQUIRE(c && module && line && cout, "null argument");
  RAMP_REQUIRE(c->time_table != nullptr && t >= 0 && t < c->tt_T, "timestep outside the prepared time table");
  for (const RTB& r : c->rtbs)
    if (r.name == module) {
      *line = c->time_table + (size_t)t * c->tt_stride + r.tb_off; *cout = r.cout;
      return 0;
    }
  RAMP_REQUIRE(false, std::string("no residual block '") + module + "' in the time table");
  return 1;
}
}  // namespace ramp

// cross-attention constants of `n_variants` latents (cross_bias_kernel) + the row -> variant table: a cyclic pattern over the table's whole
// capacity (n_rows == 0: ramp_set_scene) or the n_rows explicit entries (ramp_set_scenes); `table` is host memory
static int set_scene_table(ramp_ctx* c, const float* latents, int n_variants, const int32_t* table, int n_table, int n_rows, hipStream_t s) {
  const int nb = c->n_blocks_total;
  if (n_variants > c->cross_bias_cap) { CK(dev_alloc(c, &c->cross_bias, (size_t)n_variants * nb * 256)); c->cross_bias_cap = n_variants; }
  c->n_variants = n_variants;
  std::vector<const float*> wv(nb), wo(nb), bo(nb);
  for (auto& st : c->sts) for (int b = 0; b < 2; ++b) {
    wv[st.blk0 + b] = st.blk[b].wv2; wo[st.blk0 + b] = st.blk[b].wo2; bo[st.blk0 + b] = st.blk[b].bo2;
  }
  // row -> variant table for the largest batch this context may see in one ramp_sample call
  const int want = std::max(std::max(c->row_variant_cap, 1 << 20), n_rows);
  if (c->row_variant_cap < want) {
    float* p; CK(dev_alloc(c, &p, want)); c->row_variant = reinterpret_cast<int*>(p); c->row_variant_cap = want;
  }
  char* d = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&d, 3 * nb * sizeof(void*) + (n_rows ? 0 : n_table * sizeof(int))));
  auto body = [&]() -> int {
    RAMP_HIP_CHECK(hipMemcpy(d, wv.data(), nb * sizeof(void*), hipMemcpyHostToDevice));
    RAMP_HIP_CHECK(hipMemcpy(d + nb * sizeof(void*), wo.data(), nb * sizeof(void*), hipMemcpyHostToDevice));
    RAMP_HIP_CHECK(hipMemcpy(d + 2 * nb * sizeof(void*), bo.data(), nb * sizeof(void*), hipMemcpyHostToDevice));
    if (!n_rows) RAMP_HIP_CHECK(hipMemcpy(d + 3 * nb * sizeof(void*), table, n_table * sizeof(int), hipMemcpyHostToDevice));
    CK(launch_cross_bias(latents, n_variants, c->cfg.context_dim, reinterpret_cast<const float* const*>(d),
                         reinterpret_cast<const float* const*>(d + nb * sizeof(void*)),
                         reinterpret_cast<const float* const*>(d + 2 * nb * sizeof(void*)), nb, c->cross_bias, s));
    if (n_rows) {
      RAMP_HIP_CHECK(hipStreamSynchronize(s));                // (hipMemcpy below is ordered against the NULL stream only)
      RAMP_HIP_CHECK(hipMemcpy(c->row_variant, table, (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice));
    } else {
      hipLaunchKernelGGL(fill_pattern_kernel, dim3(1024), dim3(256), 0, s, c->row_variant,
                         reinterpret_cast<const int*>(d + 3 * nb * sizeof(void*)), n_table, c->row_variant_cap);
      RAMP_HIP_CHECK(hipGetLastError());
    }
    RAMP_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  };
  const int rc = body();
  (void)hipFree(d);
  c->rv_rows = n_rows;
  c->scene_epoch++;
  c->graph_key.clear();     // scene changed: cross_bias pointer may have moved
  c->e_key.clear();
  invalidate_calibrations(c, CAL_ALL);
  return rc;
}

int ramp_set_scene(ramp_ctx* c, const float* latents, int32_t n_variants, const int32_t* row_variant_host,
                   int32_t n_rows_pattern, void* stream) {
  RAMP_REQUIRE(c && c->finalized && latents && n_variants >= 1 && n_variants <= 8, "bad arguments");
  RAMP_REQUIRE(row_variant_host && n_rows_pattern >= 1 && n_rows_pattern <= 64, "bad row-variant pattern");
  for (int i = 0; i < n_rows_pattern; ++i)
    RAMP_REQUIRE(row_variant_host[i] >= 0 && row_variant_host[i] < n_variants, "row variant out of range");
  return set_scene_table(c, latents, n_variants, row_variant_host, n_rows_pattern, 0, as_stream(stream));
}

int ramp_set_scenes(ramp_ctx* c, const float* latents, int32_t n_variants, const int32_t* row_variant_host, int32_t n_rows,
                    void* stream) {
  RAMP_REQUIRE(c && c->finalized && latents && n_variants >= 1 && n_variants <= 65536, "bad arguments (1 .. 65536 latent variants)");
  RAMP_REQUIRE((long)n_variants * c->n_blocks_total * 256 < (1l << 31), "too many variants for 32-bit offsets into the cross-attention constants");
  RAMP_REQUIRE(row_variant_host && n_rows >= 1 && n_rows <= (1 << 24), "bad row -> variant table");
  for (int i = 0; i < n_rows; ++i)
    RAMP_REQUIRE(row_variant_host[i] >= 0 && row_variant_host[i] < n_variants, "row variant out of range");
  return set_scene_table(c, latents, n_variants, row_variant_host, n_rows, n_rows, as_stream(stream));
}

int ramp_encode_scene(ramp_ctx* c, const float* cloud, int32_t n_obstacles, int32_t n_points, int32_t point_dim,
                      float* latent_out, void* stream) {
  RAMP_REQUIRE(c && c->finalized && cloud && latent_out && n_obstacles > 0 && n_points > 0, "bad arguments");
  RAMP_REQUIRE((reinterpret_cast<uintptr_t>(latent_out) & 15) == 0, "latent_out must be 16-byte aligned");
  if (point_dim == 2) {
    RAMP_REQUIRE(c->cfg.context_dim == 320, "2-D scene encoder produces a 320-d latent");
    return encode_scene_2d(c, cloud, n_obstacles, n_points, latent_out, as_stream(stream));
  }
  RAMP_REQUIRE(point_dim == 3 && c->cfg.context_dim == 256, "3-D scene encoder takes (No,Np,3) and produces 256-d");
  return encode_scene_3d(c, cloud, n_obstacles, n_points, latent_out, as_stream(stream));
}

int ramp_encode_scenes(ramp_ctx* c, const float* points, const int32_t* obstacle_first_host, const int32_t* scene_first_host,
                       int32_t n_scenes, int32_t point_dim, int32_t max_points, float* latents_out, int32_t* n_passes_out, void* stream) {
  static_assert(ENCODE_DEFAULT_MAX_POINTS == RAMP_ENCODE_DEFAULT_MAX_POINTS, "the planner's default budget is the header's");
  const std::string who = "ramp_encode_scenes: ";
  // everything is checked on the host before the first launch
  RAMP_REQUIRE(c && c->finalized && points && latents_out, who + "bad arguments (context with finalized weights, points, latents_out)");
  RAMP_REQUIRE((reinterpret_cast<uintptr_t>(latents_out) & 15) == 0, who + "latents_out must be 16-byte aligned");
  RAMP_REQUIRE(point_dim == (c->cfg.context_dim == 320 ? 2 : 3) && (c->cfg.context_dim == 320 || c->cfg.context_dim == 256),
               who + "point_dim is not the model's (the 2-D encoder takes (.., 2) points and produces 320-d latents, the 3-D one (.., 3) and 256-d)");
  std::vector<EncodePass> passes;
  const std::string refusal = plan_encode_passes(scene_first_host, obstacle_first_host, n_scenes, max_points, &passes);
  RAMP_REQUIRE(refusal.empty(), who + refusal);
  const bool two_d = point_dim == 2;
  const long n_points = obstacle_first_host[scene_first_host[n_scenes]];
  RAMP_REQUIRE(n_points * point_dim < (1l << 31) && (long)n_scenes * c->cfg.context_dim < (1l << 31), who + "the batch does not fit 32-bit offsets");
  // the tables of every pass, rebased to the pass, in ONE host array and one upload: [obstacle_first | scene's first token | tiles] per pass
  std::vector<int32_t> tab;
  std::vector<size_t> at(passes.size());
  size_t scratch = 0;
  for (size_t k = 0; k < passes.size(); ++k) {
    const EncodePass& ps = passes[k];
    at[k] = tab.size();
    for (int o = ps.obstacle0; o <= ps.obstacle1; ++o) tab.push_back(obstacle_first_host[o] - ps.point0);
    for (int sc = ps.scene0; sc <= ps.scene1; ++sc)
      tab.push_back(two_d ? obstacle_first_host[scene_first_host[sc]] - ps.point0 : scene_first_host[sc] - ps.obstacle0);
    for (int sc = ps.scene0; sc < ps.scene1; ++sc) {
      const int base = two_d ? obstacle_first_host[scene_first_host[sc]] - ps.point0 : scene_first_host[sc] - ps.obstacle0;
      const int Ts = two_d ? obstacle_first_host[scene_first_host[sc + 1]] - obstacle_first_host[scene_first_host[sc]]
                           : scene_first_host[sc + 1] - scene_first_host[sc];
      for (int q0 = 0; q0 < Ts; q0 += ENCODE_TILE) { tab.push_back(base); tab.push_back(Ts); tab.push_back(q0); }
    }
    const size_t T = ps.point1 - ps.point0, No = ps.obstacle1 - ps.obstacle0, Ns = ps.scene1 - ps.scene0;
    scratch = std::max(scratch, two_d ? encode_scratch_2d(T, No, Ns) : encode_scratch_3d(T, No, Ns));
  }
  hipStream_t s = as_stream(stream);
  CK(scene_scratch(c, scratch));
  if (tab.size() > c->enc_tab_cap) {
    float* q; CK(dev_alloc(c, &q, tab.size())); c->enc_tab = reinterpret_cast<int*>(q); c->enc_tab_cap = tab.size();
  }
  RAMP_HIP_CHECK(hipMemcpyAsync(c->enc_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));   // (pageable host memory: staged before the call returns)
  for (size_t k = 0; k < passes.size(); ++k) {
    const EncodePass& ps = passes[k];
    EncodeTables tb;
    tb.n_scenes = ps.scene1 - ps.scene0; tb.n_obstacles = ps.obstacle1 - ps.obstacle0; tb.n_points = ps.point1 - ps.point0;
    tb.n_tiles = two_d ? ps.point_tiles : ps.obstacle_tiles;
    tb.obstacle_first = c->enc_tab + at[k];
    tb.scene_first = tb.obstacle_first + tb.n_obstacles + 1;
    tb.tiles = tb.scene_first + tb.n_scenes + 1;
    const float* cloud = points + (size_t)ps.point0 * point_dim;
    float* out = latents_out + (size_t)ps.scene0 * c->cfg.context_dim;
    if (two_d) CK(encode_scenes_2d(c, cloud, tb, out, s));
    else CK(encode_scenes_3d(c, cloud, tb, out, s));
  }
  if (n_passes_out) *n_passes_out = (int32_t)passes.size();
  return 0;
}

int ramp_score(ramp_ctx* c, const float* x, int32_t B, int32_t n_rp, int32_t t, float* f_out, float* eps_out,
               void* stream) {
  RAMP_REQUIRE(c && x, "null argument");
  c->launches = 0;
  hipStream_t s = as_stream(stream);
  if (c->gemm_mode != 2 || c->force_x6) {
    c->score_last_mode = c->gemm_mode == 2 ? 1 : c->gemm_mode;
    return guarded_eval(c, 0, 0, 0, x, B, n_rp, t, f_out, eps_out, s);
  }
  // fp16x3: the same delayed scaling as inside ramp_sample, with the calibration kept across calls.  The first
  // evaluation after context creation / a scene change / a ramp_sample runs the bf16x6 kernels and records every call
  // site's operand maximum; every later one runs fp16x3 scaled from its predecessor's maxima, and is repeated at once
  // with the bf16x6 kernels (recording again) if the range guard fired -- the caller never sees a flagged result.
  const int t_out = c->score_parity ? TABLE_ODD : TABLE_EVEN, t_in = c->score_parity ? TABLE_EVEN : TABLE_ODD;
  // (a forward-only evaluation leaves the call sites of the input-gradient pass without maxima)
  if (c->score_calibrated && (c->score_calibrated_bwd || eps_out == nullptr)) {
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->range_flag), 1);
    CK(guarded_eval(c, 2, t_in, t_out, x, B, n_rp, t, f_out, eps_out, s));
    int flag = 0;
    RAMP_HIP_CHECK(hipMemcpyAsync(&flag, c->range_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    RAMP_HIP_CHECK(hipStreamSynchronize(s));
    forget_single_replan_carry(c);
    if (!flag) { c->score_parity ^= 1; c->score_last_mode = 2; c->score_calibrated_bwd = eps_out != nullptr; return 0; }
  }
  CK(guarded_eval(c, 1, t_in, t_out, x, B, n_rp, t, f_out, eps_out, s));
  c->score_calibrated = true; c->score_calibrated_bwd = eps_out != nullptr; c->score_parity ^= 1; c->score_last_mode = 1;
  forget_single_replan_carry(c);
  return 0;
}

// ramp_score plus the rows' energies: the same evaluation (arithmetic modes, kept calibration, range guard and its repeat, chunking -- a
// repeated evaluation overwrites its energies too), with score_all taking each chunk's energies from the chunk's f
int ramp_score_energy(ramp_ctx* c, const float* x, int32_t B, int32_t n_rp, int32_t t, float* f_out, float* eps_out, double* energy_out,
                      void* stream) {
  RAMP_REQUIRE(c && x && energy_out, "ramp_score_energy: null argument");
  RAMP_REQUIRE(B > 0 && n_rp >= 1 && n_rp <= RAMP_MAX_ROWS_PER_TRAJ && (long)B * n_rp <= (1l << 24), "ramp_score_energy: bad batch");
  float* f = f_out;
  if (!f) {
    CK(grow(c, c->m_f, c->m_f_cap, (size_t)B * n_rp * c->cfg.horizon * c->cfg.state_dim));
    staging_done(c);
    f = c->m_f;
  }
  c->e_rows_cur = energy_out;
  const int rc = ramp_score(c, x, B, n_rp, t, f, eps_out, stream);
  c->e_rows_cur = nullptr;
  return rc;
}

int ramp_score_rows(ramp_ctx* c, const float* x, int32_t B, int32_t n_rp, const int32_t* t_rows_host, float* f_out, float* eps_out,
                    void* stream) {
  RAMP_REQUIRE(c && x && t_rows_host, "null argument");
  RAMP_REQUIRE(B > 0 && n_rp >= 1 && n_rp <= RAMP_MAX_ROWS_PER_TRAJ && (long)B * n_rp <= (1l << 24), "bad batch");
  RAMP_REQUIRE(c->time_table != nullptr && c->tt_T > 0, "time table not prepared (ramp_prepare_time_table)");
  const size_t n = (size_t)B * n_rp;
  for (size_t i = 0; i < n; ++i)
    RAMP_REQUIRE(t_rows_host[i] >= 0 && t_rows_host[i] < c->tt_T, "a row's timestep is outside the prepared time table");
  hipStream_t s = as_stream(stream);
  if (c->t_rows_cap < n) {
    float* p; CK(dev_alloc(c, &p, n)); c->t_rows_dev = reinterpret_cast<int*>(p); c->t_rows_cap = n;
  }
  RAMP_HIP_CHECK(hipStreamSynchronize(s));                  // (an earlier call's kernels may still read the table; hipMemcpy is ordered against the NULL stream only)
  RAMP_HIP_CHECK(hipMemcpy(c->t_rows_dev, t_rows_host, n * sizeof(int), hipMemcpyHostToDevice));
  // everything else -- arithmetic modes, the kept fp16x3 calibration and its range guard, taps, chunking -- is ramp_score's, run with t = 0:
  // the consumers then see line 0 of the table as their base and add the row's line offset
  c->t_rows_cur = c->t_rows_dev;
  const int rc = ramp_score(c, x, B, n_rp, 0, f_out, eps_out, stream);
  c->t_rows_cur = nullptr;
  return rc;
}

// The Langevin refinement of a job (ramp_sample_mcmc): kind 1 ULA / 2 MALA, total = sum of n_inner (filled by check_mcmc)
struct McmcJob { int kind; const int32_t* n_inner; const float* step_size; const float* sigma; int total; };
// The resampling events of a job (ramp_sample_steered): n_events = flags set in rs->resample.  The injected uniforms (noise_mode 0) and the four
// outputs travel with it
struct ResampleJob {
  const ramp_resample_params* rs; int n_events;
  const float* u; int32_t* ancestor_out; double* ess_out; double* cost_out; double* logw_out;
};
// One sampling job, stated once: what its entry was given, named after the entry (`who`, for the messages).  The entry fills it, run_sample
// checks every option and switches off what changes nothing, sample_job stages and keys it, sample_body enqueues it.
// sc: a job of many scenes (ramp_sample_scenes) -- the APF of trajectory b runs against the cloud of scene traj_scene[b]
// g: a composed job (ramp_sample_composed) -- n_rp up to RAMP_MAX_ROWS_PER_TRAJ, the rows' weights in e_comb come from its device table
// (c->g_weight_cur while the job runs), p->w0 / p->w1 are not read
// mj: behind the checks active (mcmc()) only with an inner step somewhere; mcmc_noise / mcmc_u are its injected draws (noise_mode 0),
// accept_out (sum K, B) its accept flags
// cg: the cost guide (ramp_sample_guided); behind the checks set only with n_guide > 0 somewhere.  pg: its swept box and sphere terms
// (ramp_sample_guided_prims), tg: the separation term between the rows of a team (ramp_sample_guided_team): behind the checks each is set only
// next to such a guide and where its table changes the guide (a primitive with w_prim != 0; more than one agent with w_team != 0)
// rj: active (resampling()) only with an event somewhere;  st: stitched windows (ramp_sample_stitched)
// ws: a warm start (ramp_sample_warm): the rows' priors and levels; p and every option table hold the tail of the schedule only
struct SampleJob {
  const char* who; const ramp_sample_params* p; const ramp_scene_batch* sc;
  const float* noise; float* chain_out; float* x_out;
  const ramp_guidance_rows* g = nullptr; const ramp_cost_guide* cg = nullptr;
  McmcJob mj = {0, nullptr, nullptr, nullptr, 0}; const float* mcmc_noise = nullptr; const float* mcmc_u = nullptr; int32_t* accept_out = nullptr;
  const ramp_prim_guide* pg = nullptr; const ramp_team_guide* tg = nullptr;
  ResampleJob rj = {nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
  const ramp_stitch* st = nullptr;
  const ramp_warm_start* ws = nullptr;
  const McmcJob* mcmc() const { return mj.total > 0 ? &mj : nullptr; }
  const ResampleJob* resampling() const { return rj.n_events > 0 ? &rj : nullptr; }
};

// mj != nullptr: K_j = mj->n_inner[j] inner steps (propose -> one evaluation at x' -> accept) follow the evaluation of iteration j, and the reverse
// step uses the cached combined gradient of the state they ended on; every evaluation, inner ones included, is one link of the calibration chain
// cg != nullptr: on iteration j with n_guide[j] > 0 ONE launch runs that many guide iterations on the posterior mean (DDPM) / x0 (DDIM), behind the APF hook
// st != nullptr: stitched windows -- the stitch runs wherever the plain job applies its hard conditions (the job carries none: hc.n == 0) and on the
// array the hooks work on, in front of them and (where one ran) behind them; every noise block is stitched with alpha = 0 first
// rj != nullptr: on iteration j with resample[j] != 0 the cost of that array (behind the guide) updates the log-weights, and at the end of the
// iteration every group is resampled: three launches and the copy back, unconditional (identity where nothing resampled), so the graph has no branch
// ws != nullptr: the warm init takes the place of the x_T copy, and on iteration j < ws->n_hold ONE launch at the end of the iteration puts
// every row that has not started yet (j0 > j) back to x_init, in the state and in the chain block
static int sample_body(ramp_ctx* c, const SampleJob& job, hipStream_t s, bool chain, bool steady, int cal_eval) {
  const ramp_sample_params* p = job.p; const ramp_scene_batch* sc = job.sc; const ramp_cost_guide* cg = job.cg; const ramp_stitch* st = job.st;
  const McmcJob* mj = job.mcmc(); const ResampleJob* rj = job.resampling(); const ramp_warm_start* ws = job.ws;
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  const size_t HS = (size_t)H * S, n = (size_t)B * HS;
  HardConds hc; hc.idx = c->s_hard_idx; hc.val = c->s_hard_val; hc.n = p->n_hard;
  // noise_mode 1: the job's whole noise block is drawn here, inside the (captured) job, from the device record {seed, offset}
  if (p->noise_mode == 1)
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_philox_normal_sharded(c->s_noise, p->ddim ? 1 : p->n_steps + 1, B, (int)HS, (long)p->philox_sample0,
                                                              p->philox_total > 0 ? (long)p->philox_total : (long)B, c->s_philox, s));
  const int n_evals = p->n_steps + (mj ? mj->total : 0);
  const bool mala = mj && mj->kind == 2;
  if (mj && p->noise_mode == 1) {      // the inner steps' draws: behind the main block, see ramp_sample_mcmc in ramp_hip.h
    const long total = p->philox_total > 0 ? (long)p->philox_total : (long)B;
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_philox_normal_sharded(c->m_noise, mj->total, B, (int)HS, (long)p->philox_sample0, total, c->s_philox, s,
                                                              (long)p->n_steps + 1));
    if (mala)
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_philox_uniform_sharded(c->m_u, mj->total, B, ((long)p->n_steps + 1 + mj->total) * total * (long)(HS / 4),
                                                                 (long)p->philox_sample0, total, c->s_philox, s));
  }
  StitchArgs sa;
  if (st) {
    sa = stitch_args(st, B, H, S);
    sa.alpha = c->st_alpha; sa.pin_val = c->st_pin_val;
    // the noise blocks are (blocks, C W, H, S): blocks * C chains of W windows; the right window takes the left window's draws
    StitchArgs na = sa;
    na.x = c->s_noise; na.C = (p->ddim ? 1 : p->n_steps + 1) * sa.C; na.alpha = c->st_alpha + sa.O; na.n_pin = 0;
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_stitch(na, s));
  }
  // the stitch of `target` (blend and pins), in the places of the plain job's hard conditioning
  auto stitch_at = [&](float* target) -> int {
    sa.x = target;
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_stitch(sa, s));
    return 0;
  };
  // x_T = noise[0] (a warm start: every row with a prior its prior noised to its own level); apply_hard_conditioning; chain[0]
  if (ws) LAUNCH(c, s, CAT_SAMPLER, 0, launch_warm_init(c->s_x, c->s_noise, c->w_prior, c->w_coef, c->w_coef + B, c->w_tab + B, B, H, S, s));
  else RAMP_HIP_CHECK(hipMemcpyAsync(c->s_x, c->s_noise, n * 4, hipMemcpyDeviceToDevice, s));
  if (st) CK(stitch_at(c->s_x));
  else LAUNCH(c, s, CAT_SAMPLER, 0, launch_hard_cond(c->s_x, hc, B, H, S, s));
  if (chain) RAMP_HIP_CHECK(hipMemcpyAsync(c->s_chain, c->s_x, n * 4, hipMemcpyDeviceToDevice, s));
  const int n_hold = ws ? ws->n_hold : 0;
  if (n_hold > 0) RAMP_HIP_CHECK(hipMemcpyAsync(c->w_xinit, c->s_x, n * 4, hipMemcpyDeviceToDevice, s));      // x_init, for the holds
  ApfArgs ap; ap.cloud = c->s_cloud; ap.window = c->s_window; ap.B = B; ap.H = H; ap.S = S; ap.P = p->apf.n_points;
  ap.win = p->apf.window; ap.thr = p->apf.threshold; ap.strength = p->apf.strength;
  const bool sc_apf = sc && sc->cloud_points;
  if (sc_apf) { ap.scene = c->s_traj_scene; ap.scene_off = c->s_scene_off; ap.n_scenes = sc->n_scenes; ap.P = 0; }
  GuideArgs ga;
  if (cg) {
    ga = guide_args(cg, nullptr, B, H, S);
    ga.cloud = c->cg_cloud; ga.cloud_off = c->cg_off; ga.scene = sc ? c->s_traj_scene : nullptr; ga.hc = hc;
  }
  // the guide's launch of iteration j on `target`, if it has one: with primitives the kernel that carries their term, the guide's own otherwise
  auto guide_at = [&](int j, float* target) -> int {
    if (!cg || cg->n_guide[j] <= 0) return 0;
    ga.traj = target; ga.n_iter = cg->n_guide[j]; ga.step = cg->step[j];
    if (job.tg) {      // one block per team; a job carries a team or primitives, never both
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_guide_team_step(team_guide_args(job.tg, ga), s));
    } else if (job.pg) {
      PrimGuideArgs pa = prim_guide_args(job.pg, ga);
      pa.box_c = c->pg_boxc; pa.box_s = c->pg_boxs; pa.sph_c = c->pg_sphc; pa.sph_r = c->pg_sphr; pa.box_off = c->pg_boff; pa.sph_off = c->pg_soff;
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_guide_prims_step(pa, s));
    } else {
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_guide_step(ga, s));
    }
    return 0;
  };
  GuideArgs ra;
  int ke = 0;      // events so far
  if (rj) {
    const ramp_resample_params* rs = rj->rs;
    ra = guide_args(rs->cost, nullptr, B, H, S);
    ra.cloud = c->rs_cloud; ra.cloud_off = c->rs_off; ra.scene = sc ? c->s_traj_scene : nullptr;
    hipLaunchKernelGGL(zero_words_kernel, dim3((4 * B + 255) / 256), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->rs_state), 4 * B);      // logw = c_prev = 0
    RAMP_HIP_CHECK(hipGetLastError());
    if (p->noise_mode == 1) {      // one uniform per (event, group): behind the inner steps' draws, see ramp_resample_params in ramp_hip.h
      const long T = p->philox_total > 0 ? (long)p->philox_total : (long)B, K = mj ? mj->total : 0;
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_philox_uniform_sharded(c->rs_u, rj->n_events, rs->n_groups, ((long)p->n_steps + 1 + K) * T * (long)(HS / 4) + K * T,
                                                                 (long)rs->group0, rs->groups_total > 0 ? (long)rs->groups_total : (long)rs->n_groups, c->s_philox, s));
    }
  }
  // steps 1 and 2 of the event of iteration j, if it has one: the cost of `target` and the weight update
  auto weigh_at = [&](int j, float* target) -> int {
    if (!rj || !rj->rs->resample[j]) return 0;
    ra.traj = target;
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_guide_cost(ra, c->rs_terms, s));
    ResampleWeightArgs w; w.terms = c->rs_terms; w.logw = c->rs_state; w.c_prev = c->rs_state + B; w.cost_out = c->rs_cost + (size_t)ke * B; w.B = B;
    w.w_obs = rj->rs->cost->w_obs; w.w_smooth = rj->rs->cost->w_smooth; w.w_acc = rj->rs->cost->w_acc; w.lambda = rj->rs->lambda[j];
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_resample_weights(w, s));
    return 0;
  };
  // steps 3 to 5, on the state the iteration ended on
  auto resample_at = [&](int j, float* chain_j) -> int {
    if (!rj || !rj->rs->resample[j]) return 0;
    ResampleGroupsArgs g; g.logw = c->rs_state; g.c_prev = c->rs_state + B; g.cum = c->rs_state + 2 * (size_t)B; g.tmp = c->rs_state + 3 * (size_t)B;
    g.group_first = c->rs_gf; g.u = c->rs_u + (size_t)ke * rj->rs->n_groups; g.ess_frac = rj->rs->ess_frac;
    g.ancestor = c->rs_anc + (size_t)ke * B; g.ess_out = c->rs_ess + (size_t)ke * rj->rs->n_groups; g.B = B; g.n_groups = rj->rs->n_groups;
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_resample_groups(g, s));
    LAUNCH(c, s, CAT_SAMPLER, 0, launch_resample_gather(c->s_x, g.ancestor, c->rs_xtmp, B, (int)HS, s));
    RAMP_HIP_CHECK(hipMemcpyAsync(c->s_x, c->rs_xtmp, n * 4, hipMemcpyDeviceToDevice, s));
    if (chain_j) RAMP_HIP_CHECK(hipMemcpyAsync(chain_j, c->rs_xtmp, n * 4, hipMemcpyDeviceToDevice, s));
    ++ke;
    return 0;
  };
  if (c->gemm_mode == 2) {
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->range_flag), 1);
    if (!c->force_x6) hipLaunchKernelGGL(zero_words_kernel, dim3((n_evals + 255) / 256), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->trip_log), n_evals);
    RAMP_HIP_CHECK(hipGetLastError());
  }
  const bool h3 = c->gemm_mode == 2 && !c->force_x6;
  // (a composed job: comb below only says "combined evaluation", see score_all; its weights are c->g_weight_cur's)
  const std::array<float, 3> comb = c->g_weight_cur ? std::array<float, 3>{0.f, 0.f, 0.f} : comb_weights(p->n_rp, p->w0, p->w1);
  const bool shared = p->n_rp > 1 && c->share_prefix;
  int ev = 0, kk = 0;      // evaluations / inner steps so far
  // One evaluation of the job, link `ev` of its calibration chain (a plain job: ev == j).
  // fp16x3: evaluation 0 runs scaled from the context's CANONICAL maxima (canonical_calibration below) -- or, with
  // ramp_set_calibration_reuse(ctx, 0), calibrates itself (bf16x6 + recorded operand maxima); evaluation e >= 1 runs fp16x3
  // scaled from e - 1
  // (e == cal_eval, cal_eval + 1: the evaluation the range guard flagged first in this job's previous run calibrates instead -- see
  // ramp_ctx::trip_log -- and so does its successor: an excursion that is gone one step later (a spike) would otherwise trip the guard
  // again from the other side, its successor being scaled from the spike's maxima; 3 % of a job per calibrating evaluation)
  auto eval_at = [&](const float* x, int t, float* f_out, float* eps_out) -> int {
    const int e = ev++;
    const int phase = !h3 ? 0 : ((e == 0 && !steady) || e == cal_eval || (cal_eval >= 0 && e == cal_eval + 1)) ? 1 : 2;
    const int t_out = (e & 1) ? TABLE_ODD : TABLE_EVEN, t_in = e == 0 ? TABLE_CANONICAL : (e & 1) ? TABLE_EVEN : TABLE_ODD;
    return guarded_eval(c, phase, t_in, t_out, x, B, p->n_rp, t, f_out, eps_out, s, shared ? comb.data() : nullptr, h3 ? c->trip_log : nullptr, e);
  };
  // The evaluation of a job with inner steps: the combined gradient of x into eps_comb (B, H, S) and, E != nullptr, the combined energy into E (B)
  auto eval_comb = [&](const float* x, int t, float* eps_comb, double* E) -> int {
    c->e_rows_cur = E ? c->m_Erows : nullptr;
    const int rc = eval_at(x, t, E ? c->m_f : nullptr, shared ? eps_comb : c->s_eps);
    c->e_rows_cur = nullptr;
    CK(rc);
    if (!shared) {      // the rows' gradients are still apart: the guidance step's own combination, nothing else of it
      CfgMeanArgs m; m.x = x; m.eps = c->s_eps; m.B = B; m.HS = (int)HS; m.n_rp = p->n_rp; m.ecomb = eps_comb;
      m.w0 = (float)p->w0; m.w1 = (float)p->w1; m.w0p1 = (float)(1.0 + p->w0);
      LAUNCH(c, s, CAT_SAMPLER, 0, c->g_weight_cur ? launch_cfg_mean_rows(m, c->g_weight_cur, s) : launch_cfg_mean(m, s));
    }
    if (E) {
      EnergyWeights w; w.rw = c->g_weight_cur;
      if (p->n_rp == 1) w.w[0] = 1.f; else for (int q = 0; q < 3; ++q) w.w[q] = comb[q];
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_combine_energy(c->m_Erows, w, E, B, p->n_rp, s));
    }
    return 0;
  };
  for (int j = 0; j < p->n_steps; ++j) {
    if (!mj) {
      CK(eval_at(c->s_x, p->t[j], nullptr, c->s_eps));
    } else {
      const int K = mj->n_inner[j];
      const bool wantE = mala && K > 0;
      CK(eval_comb(c->s_x, p->t[j], c->m_eps, wantE ? c->m_E : nullptr));
      const double eta = (double)mj->step_size[j], sig = (double)mj->sigma[j];
      const float a = (float)(eta / sig), cz = (float)std::sqrt(2.0 * eta);
      for (int k = 0; k < K; ++k, ++kk) {
        LAUNCH(c, s, CAT_SAMPLER, 0, launch_mcmc_propose(c->s_x, c->m_eps, c->m_noise + (size_t)kk * n, a, cz, hc, c->m_xp, B, H, S, s));
        CK(eval_comb(c->m_xp, p->t[j], c->m_eps_p, wantE ? c->m_Ep : nullptr));
        McmcAcceptArgs ac; ac.x = c->s_x; ac.xp = c->m_xp; ac.eps = c->m_eps; ac.eps_p = c->m_eps_p; ac.E = c->m_E; ac.E_p = c->m_Ep;
        ac.u = c->m_u + (size_t)kk * B; ac.flag = c->m_flag + (size_t)kk * B; ac.hc = hc; ac.B = B; ac.H = H; ac.S = S; ac.mala = mala; ac.a = a;
        ac.inv_sigma = 1.0 / sig; ac.inv_4eta = 1.0 / (4.0 * eta);
        LAUNCH(c, s, CAT_SAMPLER, 0, launch_mcmc_accept(ac, s));
      }
    }
    // (with inner steps the gradient is the cached COMBINED one of the state they ended on: one row per trajectory, as after the shared prefix)
    const bool combined = shared || mj != nullptr;
    CfgMeanArgs m; m.x = c->s_x; m.eps = mj ? c->m_eps : c->s_eps; m.B = B; m.HS = (int)HS; m.n_rp = combined ? 1 : p->n_rp;
    m.w0 = (float)p->w0; m.w1 = (float)p->w1; m.w0p1 = (float)(1.0 + p->w0);
    m.sqrt_recip = p->sqrt_recip[j]; m.sqrt_recipm1 = p->sqrt_recipm1[j]; m.clip = p->clip_denoised; m.predict_x0 = p->predict_x0 != 0;
    float* chain_j = chain ? c->s_chain + (size_t)(j + 1) * n : nullptr;
    float* chain_fin = st ? nullptr : chain_j;     // (a stitched job's chain block is the state after the closing stitch)
    const bool apf = (p->apf.cloud != nullptr || sc_apf) && p->apply_apf && p->apply_apf[j];
    const bool hooked = st && (apf || (cg && cg->n_guide[j] > 0));      // a hook moves the array on this iteration: one more stitch behind it
    // the guidance step: the shared prefix has combined the rows already (one row left); otherwise by the job's scalars or its weight table
    const bool by_table = c->g_weight_cur && !combined;
    if (!p->ddim) {
      m.coef1 = p->coef1[j]; m.coef2 = p->coef2[j]; m.mean = c->s_mean; m.x0 = nullptr;
      LAUNCH(c, s, CAT_SAMPLER, 0, by_table ? launch_cfg_mean_rows(m, c->g_weight_cur, s) : launch_cfg_mean(m, s));
      if (st) CK(stitch_at(c->s_mean));
      if (apf) { ap.traj = c->s_mean; for (int q = 0; q < std::max(1, p->apf.passes); ++q) LAUNCH(c, s, CAT_SAMPLER, 0, launch_apf(ap, s)); }
      CK(guide_at(j, c->s_mean));
      if (hooked) CK(stitch_at(c->s_mean));
      CK(weigh_at(j, c->s_mean));
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_ddpm_finish(c->s_mean, c->s_noise + (size_t)(j + 1) * n, p->stdv[j], p->noise_scale ? p->noise_scale[j] : 1.f, p->use_noise[j],
                            hc, c->s_x, chain_fin, B, H, S, s));
    } else {
      m.mean = nullptr; m.x0 = c->s_x0;
      LAUNCH(c, s, CAT_SAMPLER, 0, by_table ? launch_cfg_mean_rows(m, c->g_weight_cur, s) : launch_cfg_mean(m, s));
      if (st) CK(stitch_at(c->s_x0));
      if (apf) {
        ap.traj = c->s_x0;
        for (int q = 0; q < std::max(1, p->apf.passes); ++q) {
          LAUNCH(c, s, CAT_SAMPLER, 0, launch_apf(ap, s));
          if (st) CK(stitch_at(c->s_x0));
          else LAUNCH(c, s, CAT_SAMPLER, 0, launch_hard_cond(c->s_x0, hc, B, H, S, s));
        }
      }
      CK(guide_at(j, c->s_x0));      // (the hard conditioning that follows is ddim_finish's own)
      if (hooked) CK(stitch_at(c->s_x0));
      CK(weigh_at(j, c->s_x0));
      LAUNCH(c, s, CAT_SAMPLER, 0, launch_ddim_finish(c->s_x, c->s_x0, p->sqrt_a_t[j], p->sqrt_1m_a_t[j], p->sqrt_a_prev[j], p->dir_coef[j], hc,
                            c->s_x, chain_fin, B, H, S, s));
    }
    if (st) {      // the update ran without hard conditions: the blend is the identity here, the pins act
      CK(stitch_at(c->s_x));
      if (chain_j) RAMP_HIP_CHECK(hipMemcpyAsync(chain_j, c->s_x, n * 4, hipMemcpyDeviceToDevice, s));
    }
    CK(resample_at(j, chain_j));
    if (j < n_hold) LAUNCH(c, s, CAT_SAMPLER, 0, launch_warm_hold(c->s_x, chain_j, c->w_xinit, c->w_tab, j, B, H, S, s));
  }
  return 0;
}

// The calibration every job's first evaluation is scaled from (fp16x3 mode): ONE score evaluation on the bf16x6 kernels that only records the
// operand maxima of every GEMM call site (phase 1) into TABLE_CANONICAL, on a CANONICAL input -- x ~ N(0, I) from Philox4x32-10 with a fixed
// seed, at the job's first timestep, with no hard conditions applied -- not on anybody's data, not even the job's start / goal values (ADVICE
// r5: with them the table depended on whichever job triggered it): x_T of every job is a draw of the same distribution, the
// recorded maxima only pick power-of-two scales (the operand may then grow 2^9.9-fold before the range guard fires, elements down to 2^-8 of the
// maximum keep all 22 bits), and the guard covers a caller whose x_T is something else.  Runs eagerly on the job's stream, outside its graph,
// once per (batch, row variants and weights, first timestep, scene).
static int canonical_calibration(ramp_ctx* c, const ramp_sample_params* p, hipStream_t s) {
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  if (!c->c_cal_rec) {
    CK(renew(c, c->c_cal_rec, 2));
    const unsigned long long rec[2] = {0x52414d5043414cull /* "RAMPCAL" */, 0ull};
    RAMP_HIP_CHECK(hipMemcpyAsync(c->c_cal_rec, rec, 16, hipMemcpyHostToDevice, s));
    RAMP_HIP_CHECK(hipStreamSynchronize(s));       // (rec is a stack array)
  }
  RAMP_REQUIRE((H * S) % 4 == 0, "H * S must be a multiple of 4");
  CK(launch_philox_normal(c->s_x, (long)B * H * S, c->c_cal_rec, s));
  const std::array<float, 3> comb = c->g_weight_cur ? std::array<float, 3>{0.f, 0.f, 0.f} : comb_weights(p->n_rp, p->w0, p->w1);      // (composed: a flag only, as in sample_body)
  const bool shared = p->n_rp > 1 && c->share_prefix;
  return guarded_eval(c, 1, TABLE_EVEN, TABLE_CANONICAL, c->s_x, B, p->n_rp, p->t[0], nullptr, c->s_eps, s, shared ? comb.data() : nullptr);
}

int ramp_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  RAMP_REQUIRE(out && n > 0, "null argument");
  hipStream_t s = as_stream(stream);
  unsigned long long* rec = nullptr;
  RAMP_HIP_CHECK(hipMalloc(&rec, 16));
  const unsigned long long h[2] = {seed, offset};
  hipError_t e = hipMemcpyAsync(rec, h, 16, hipMemcpyHostToDevice, s);
  int rc = e == hipSuccess ? launch_philox_normal(out, (long)n, rec, s) : -1;
  if (e != hipSuccess) set_last_error(std::string("hipMemcpyAsync failed: ") + hipGetErrorString(e));
  (void)hipStreamSynchronize(s);
  (void)hipFree(rec);
  return rc;
}

// APF staging of both kinds of job: the window weights (host) and the n_points obstacle points (device, (n_points, 2)) into the context's buffers
static int stage_apf(ramp_ctx* c, const ramp_apf_params& a, const float* cloud, int n_points, hipStream_t s) {
  RAMP_REQUIRE(n_points > 0 && a.window >= 0 && a.window <= 64 && a.window_weights_host, "bad APF params");
  if (!c->s_window) CK(renew(c, c->s_window, 256));
  CK(grow(c, c->s_cloud, c->s_cloud_cap, (size_t)n_points * 2));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->s_window, a.window_weights_host, (2 * a.window + 1) * 4, hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->s_cloud, cloud, (size_t)n_points * 8, hipMemcpyDeviceToDevice, s));
  return 0;
}

// ---- the options of a sampling job.  Per option: its check for the entry job.who (beside check_cost_guide / check_prim_guide / check_team_guide /
// check_stitch in engine_util.h; every refusal is a host check made before anything is staged or launched), the staging of its buffers (grown
// with the job's other buffers, before staging_done) and what it adds to the graph key.  A key_ function carries everything of its option that
// is baked into the captured nodes, and whatever decides that the job touches a buffer that may not exist yet: renew() relies on that when it
// lets a first allocation pass without dropping the graphs.  A new option brings its own four functions and one field of SampleJob.

// what a guidance table must satisfy, for every entry that takes one (`who` names the entry in the message)
static int check_guidance(ramp_ctx* c, const ramp_sample_params* p, const ramp_guidance_rows* g, const char* who) {
  const std::string w = std::string(who) + ": ";
  RAMP_REQUIRE(g->row_weight, w + "null row_weight");
  RAMP_REQUIRE(g->n_rp >= 2 && g->n_rp <= RAMP_MAX_ROWS_PER_TRAJ, w + "n_rp outside 2 .. RAMP_MAX_ROWS_PER_TRAJ");
  RAMP_REQUIRE(g->n_rp == p->n_rp, w + "the guidance table's n_rp differs from the job's");
  RAMP_REQUIRE(p->B > 0 && (long)p->B * p->n_rp <= (1l << 24), w + "bad batch");
  RAMP_REQUIRE((c->cfg.horizon * c->cfg.state_dim) % 4 == 0, w + "H * S must be a multiple of 4 (the guidance step moves four elements per access)");
  RAMP_REQUIRE(c->rv_rows > 0, w + "the row -> latent table comes from ramp_set_scenes (none is in place)");
  RAMP_REQUIRE(c->rv_rows >= p->B * p->n_rp, w + "the ramp_set_scenes table is shorter than B * n_rp rows");
  return 0;
}
// the weight table onto the device; g_host: the weights on the host, where the canonical calibration's key carries them
static int stage_guidance(ramp_ctx* c, const SampleJob& job, hipStream_t s, std::vector<float>& g_host) {
  const size_t nw = (size_t)job.p->B * job.p->n_rp;
  CK(stage_table(c, c->g_weight, c->g_weight_cap, job.g->row_weight, nw, 0, hipMemcpyDeviceToDevice, s));
  if (c->gemm_mode == 2 && !c->force_x6 && c->cal_reuse) {
    g_host.resize(nw);
    RAMP_HIP_CHECK(hipMemcpyAsync(g_host.data(), c->g_weight, nw * 4, hipMemcpyDeviceToHost, s));
    RAMP_HIP_CHECK(hipStreamSynchronize(s));      // (the key reads g_host)
  }
  c->g_weight_cur = c->g_weight;      // (run_sample clears it when the job returns)
  return 0;
}

// The scene batch: its APF clouds where it brings them, and the trajectory -> scene table for every kernel that indexes by scene (the APF, the
// guide, the potential)
static int stage_scenes(ramp_ctx* c, const SampleJob& job, hipStream_t s) {
  const ramp_scene_batch* sc = job.sc;
  if (sc->cloud_points) {
    CK(stage_apf(c, job.p->apf, sc->cloud_points, sc->cloud_offset_host[sc->n_scenes], s));
    CK(stage_table(c, c->s_scene_off, c->s_scene_off_cap, sc->cloud_offset_host, (size_t)sc->n_scenes + 1, 0, hipMemcpyHostToDevice, s));
  }
  if (sc->cloud_points || job.cg || job.resampling())
    CK(stage_table(c, c->s_traj_scene, c->s_traj_scene_cap, sc->traj_scene, (size_t)job.p->B, 0, hipMemcpyDeviceToDevice, s));
  return 0;
}
// (a single-scene job's key has no such tail.  With clouds the job reads s_scene_off, and s_cloud holds that many points of that many scenes:
// kernel arguments; s_traj_scene exists with them, or with the `scenes` word of key_guide / key_resample)
static void key_scenes(Key& key, const ramp_scene_batch* sc) {
  const int tag[3] = {0x5343454e /* "SCEN" */, sc->cloud_points ? sc->n_scenes : 0, sc->cloud_points ? sc->cloud_offset_host[sc->n_scenes] : 0}; key.put(tag, 3);
}

// Langevin refinement (ramp_sample_mcmc).  kind 0, or no inner step anywhere, is the plain job: mj.total stays 0
static int check_mcmc(SampleJob& job) {
  const std::string w = std::string(job.who) + ": ";
  const ramp_sample_params* p = job.p; const McmcJob* m = &job.mj; const float *mcmc_noise = job.mcmc_noise, *mcmc_u = job.mcmc_u;
  const int kind = m->kind;
  if (kind == 0) return 0;      // (off)
  RAMP_REQUIRE(p->predict_x0 == 0, w + "predict_x0 != 0 -- the combined network output is then x0, not a score: there is no density to correct");
  RAMP_REQUIRE(p->n_steps > 0 && m->n_inner && m->step_size && m->sigma, w + "missing n_inner / step_size / sigma arrays");
  for (int j = 0; j < p->n_steps; ++j) {
    RAMP_REQUIRE(m->n_inner[j] >= 0 && m->n_inner[j] <= RAMP_MCMC_MAX_INNER, w + "n_inner outside 0 .. 16");
    if (m->n_inner[j] == 0) continue;
    RAMP_REQUIRE(std::isfinite(m->step_size[j]) && m->step_size[j] > 0.f, w + "step_size must be positive and finite where n_inner > 0");
    RAMP_REQUIRE(std::isfinite(m->sigma[j]) && m->sigma[j] > 0.f, w + "sigma must be positive and finite where n_inner > 0");
    job.mj.total += m->n_inner[j];
  }
  if (job.mj.total > 0 && p->noise_mode == 0) {
    RAMP_REQUIRE(mcmc_noise, w + "null mcmc_noise (noise_mode 0 injects the inner steps' normals)");
    RAMP_REQUIRE(kind != 2 || mcmc_u, w + "null mcmc_u (noise_mode 0 injects MALA's uniforms)");
  }
  return 0;
}
static int grow_mcmc(ramp_ctx* c, const ramp_sample_params* p, const McmcJob* mj) {
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  const size_t n = (size_t)B * H * S, nk = (size_t)mj->total, rows = (size_t)B * p->n_rp;
  if ((size_t)B > c->m_cap_B) { CK(renew(c, c->m_xp, n)); CK(renew(c, c->m_eps, n)); CK(renew(c, c->m_eps_p, n)); c->m_cap_B = B; }
  CK(grow(c, c->m_noise, c->m_noise_cap, nk * n));
  if (nk * B > c->m_u_cap) { CK(renew(c, c->m_u, nk * B)); CK(renew(c, c->m_flag, nk * B)); c->m_u_cap = nk * B; }
  if (mj->kind == 2) {      // MALA alone asks for energies: f of every row, the rows' energies, the combined energy of state and proposal
    CK(grow(c, c->m_f, c->m_f_cap, rows * H * S));
    CK(grow(c, c->m_Erows, c->m_Erows_cap, rows));
    if ((size_t)B > c->m_E_cap) { CK(renew(c, c->m_E, (size_t)B)); CK(renew(c, c->m_Ep, (size_t)B)); c->m_E_cap = B; }
  }
  return 0;
}
// (the m_* buffers exist only for such a job, the energies' only for kind 2; the counts and step sizes are kernel arguments of the captured nodes)
static void key_mcmc(Key& key, const McmcJob* mj, int n_steps) {
  const int tag[2] = {0x4d434d43 /* "MCMC" */, mj->kind}; key.put(tag, 2);
  key.put(mj->n_inner, n_steps); key.put(mj->step_size, n_steps); key.put(mj->sigma, n_steps);
}

// The cost guide and the two tables that travel with it, tried in the order team, primitives, guide.  A table that does not change the guide
// (one agent per team or w_team == 0; no primitive or w_prim == 0) is dropped, and a guide without an iteration anywhere is the unguided job
static int check_guide(ramp_ctx* c, SampleJob& job) {
  const std::string w = std::string(job.who) + ": ";
  const ramp_sample_params* p = job.p; const ramp_scene_batch* scenes = job.sc;
  const ramp_cost_guide* cg = job.cg; const ramp_prim_guide* pg = job.pg; const ramp_team_guide* tg = job.tg;
  if (tg) {
    RAMP_REQUIRE(cg, w + "a team table needs its cost guide");
    CK(check_cost_guide(cg, c->cfg.state_dim, job.who));
    CK(check_team_guide(tg, p->B, c->cfg.horizon, job.who));
    RAMP_REQUIRE(p->philox_total == 0 || p->philox_sample0 % tg->team_size == 0, w + "a shard must hold whole teams (philox_sample0 % team_size == 0)");
    if (!team_guide_active(tg)) job.tg = nullptr;
  }
  if (pg) {
    RAMP_REQUIRE(cg, w + "a primitive table needs its cost guide");
    CK(check_cost_guide(cg, c->cfg.state_dim, job.who));
    CK(check_prim_guide(pg, cg, c->cfg.horizon, c->cfg.state_dim, job.who));
    if (!prim_guide_active(pg)) job.pg = nullptr;
  }
  if (!cg) return 0;
  int guide_total = 0;
  CK(check_cost_guide(cg, c->cfg.state_dim, job.who));
  RAMP_REQUIRE(c->cfg.horizon <= 128, w + "the guide kernel serves horizons up to 128");
  RAMP_REQUIRE(scenes ? cg->n_scenes == scenes->n_scenes : cg->n_scenes == 1,
               w + "the guide's n_scenes must equal the scene batch's (1 without a scene batch)");
  RAMP_REQUIRE(p->n_steps > 0 && cg->n_guide && cg->step, w + "missing n_guide / step arrays");
  for (int j = 0; j < p->n_steps; ++j) {
    RAMP_REQUIRE(cg->n_guide[j] >= 0 && cg->n_guide[j] <= RAMP_GUIDE_MAX_STEPS, w + "n_guide outside 0 .. RAMP_GUIDE_MAX_STEPS");
    RAMP_REQUIRE(std::isfinite(cg->step[j]), w + "step must be finite");
    guide_total += cg->n_guide[j];
  }
  if (guide_total == 0) { job.cg = nullptr; job.pg = nullptr; job.tg = nullptr; }
  return 0;
}
// a table of per-scene clouds -- device points (points, point_dim), host offsets (n_scenes + 1) -- into one of the context's buffer pairs: the
// guide's own cloud table and the potential's (the trajectory -> scene table is the scene batch's, stage_scenes)
static int stage_cloud_table(ramp_ctx* c, const ramp_cost_guide* t, float*& cloud, size_t& cloud_cap, int*& off, size_t& off_cap, hipStream_t s) {
  const size_t points = (size_t)t->cloud_offset_host[t->n_scenes];
  CK(stage_table(c, cloud, cloud_cap, t->cloud_points, points * t->point_dim, 4, hipMemcpyDeviceToDevice, s));
  return stage_table(c, off, off_cap, t->cloud_offset_host, (size_t)t->n_scenes + 1, 0, hipMemcpyHostToDevice, s);
}
static int stage_guide(ramp_ctx* c, const SampleJob& job, hipStream_t s) {
  CK(stage_cloud_table(c, job.cg, c->cg_cloud, c->cg_cloud_cap, c->cg_off, c->cg_off_cap, s));
  const ramp_prim_guide* pg = job.pg;
  if (!pg) return 0;      // with primitives: their tables, staged like the clouds
  const size_t D = pg->point_dim, no = (size_t)pg->n_scenes + 1;
  const size_t boxes = pg->box_offset_host[pg->n_scenes], spheres = pg->sphere_offset_host[pg->n_scenes];
  CK(stage_table(c, c->pg_boxc, c->pg_boxc_cap, pg->box_centers, boxes * D, 4, hipMemcpyDeviceToDevice, s));
  CK(stage_table(c, c->pg_boxs, c->pg_boxs_cap, pg->box_sizes, boxes * D, 4, hipMemcpyDeviceToDevice, s));
  CK(stage_table(c, c->pg_sphc, c->pg_sphc_cap, pg->sphere_centers, spheres * D, 4, hipMemcpyDeviceToDevice, s));
  CK(stage_table(c, c->pg_sphr, c->pg_sphr_cap, pg->sphere_radii, spheres, 4, hipMemcpyDeviceToDevice, s));
  CK(stage_table(c, c->pg_boff, c->pg_boff_cap, pg->box_offset_host, no, 0, hipMemcpyHostToDevice, s));
  return stage_table(c, c->pg_soff, c->pg_soff_cap, pg->sphere_offset_host, no, 0, hipMemcpyHostToDevice, s);
}
static void key_guide(Key& key, const SampleJob& job) {
  // (cg_cloud / cg_off exist only for such a job, s_traj_scene with `scenes`; counts, step sizes and scalars are kernel arguments of the captured nodes)
  const ramp_cost_guide* cg = job.cg;
  const int tag[5] = {0x47554944 /* "GUID" */, cg->point_dim, cg->n_scenes, cg->cloud_offset_host[cg->n_scenes], job.sc ? 1 : 0}; key.put(tag, 5);
  const double sc5[5] = {cg->radius, cg->w_obs, cg->w_smooth, cg->w_acc, cg->max_norm}; key.put(sc5, 5);
  key.put(cg->n_guide, job.p->n_steps); key.put(cg->step, job.p->n_steps);
  if (const ramp_prim_guide* pg = job.pg) {      // (the pg_* buffers exist only for such a job; counts, n_sub and the three scalars are kernel arguments of the captured nodes)
    const int ptag[5] = {0x5052494d /* "PRIM" */, pg->n_scenes, pg->box_offset_host[pg->n_scenes], pg->sphere_offset_host[pg->n_scenes], pg->n_sub}; key.put(ptag, 5);
    const double sc3[3] = {pg->margin, pg->band, pg->w_prim}; key.put(sc3, 3);
  }
  if (const ramp_team_guide* tg = job.tg) {      // (no buffer of its own; the team size and the two scalars are kernel arguments of the captured nodes)
    const int ttag[2] = {0x5445414d /* "TEAM" */, tg->team_size}; key.put(ttag, 2);
    const double sc2[2] = {tg->radius_team, tg->w_team}; key.put(sc2, 2);
  }
}

// Resampling events (ramp_sample_steered); the entry hands over only a table with a flag set
static int check_resample(ramp_ctx* c, const SampleJob& job) {
  const ResampleJob* rj = job.resampling();
  if (!rj) return 0;
  const std::string w = std::string(job.who) + ": ";
  const ramp_sample_params* p = job.p; const ramp_scene_batch* scenes = job.sc; const ramp_resample_params* rs = rj->rs; const McmcJob& mj = job.mj;
  RAMP_REQUIRE(resample_group_table_fault(rs->group_first_host, rs->n_groups, p->B) == 0,
               w + "malformed group table (n_groups >= 1, [0] = 0, strictly increasing, [n_groups] = B)");
  RAMP_REQUIRE(resample_ess_frac_ok(rs->ess_frac), w + "ess_frac must be finite and lie in [0, 2]");
  RAMP_REQUIRE(rs->lambda, w + "missing lambda array");
  for (int j = 0; j < p->n_steps; ++j) RAMP_REQUIRE(std::isfinite(rs->lambda[j]), w + "lambda must be finite");
  RAMP_REQUIRE(rj->n_events <= RAMP_RESAMPLE_MAX_EVENTS, w + "more than RAMP_RESAMPLE_MAX_EVENTS events");
  RAMP_REQUIRE(!p->ddim || mj.total > 0, w + "DDIM (eta = 0) never separates duplicates: resampling needs MCMC inner steps there");
  RAMP_REQUIRE(p->predict_x0 == 0, w + "predict_x0 != 0 is not served with resampling");
  CK(check_cost_guide(rs->cost, c->cfg.state_dim, job.who));
  RAMP_REQUIRE(c->cfg.horizon <= 128, w + "the cost kernel serves horizons up to 128");
  RAMP_REQUIRE((c->cfg.horizon * c->cfg.state_dim) % 4 == 0, w + "H * S must be a multiple of 4 (the gather moves four elements per access)");
  RAMP_REQUIRE(scenes ? rs->cost->n_scenes == scenes->n_scenes : rs->cost->n_scenes == 1,
               w + "the potential's n_scenes must equal the scene batch's (1 without a scene batch)");
  RAMP_REQUIRE(rs->group0 >= 0 && rs->groups_total >= 0 && (rs->groups_total == 0 ? rs->group0 == 0 : rs->group0 + rs->n_groups <= rs->groups_total),
               w + "group0 + n_groups must lie inside groups_total");
  RAMP_REQUIRE(p->noise_mode != 0 || rj->u, w + "null resample_u (noise_mode 0 injects the events' uniforms)");
  return 0;
}
// the potential's own cloud table, the group table and (noise_mode 0) the uniforms
static int stage_resample(ramp_ctx* c, const SampleJob& job, hipStream_t s) {
  const ResampleJob* rj = job.resampling(); const ramp_resample_params* rs = rj->rs;
  const size_t B = (size_t)job.p->B, n = B * c->cfg.horizon * c->cfg.state_dim, ne = (size_t)rj->n_events, ng = (size_t)rs->n_groups;
  CK(grow(c, c->rs_state, c->rs_state_cap, 4 * B)); CK(grow(c, c->rs_terms, c->rs_terms_cap, 3 * B));
  CK(grow(c, c->rs_xtmp, c->rs_xtmp_cap, n));
  CK(grow(c, c->rs_anc, c->rs_anc_cap, ne * B)); CK(grow(c, c->rs_ess, c->rs_ess_cap, ne * ng)); CK(grow(c, c->rs_cost, c->rs_cost_cap, ne * B));
  CK(grow(c, c->rs_u, c->rs_u_cap, ne * ng));
  CK(stage_cloud_table(c, rs->cost, c->rs_cloud, c->rs_cloud_cap, c->rs_off, c->rs_off_cap, s));
  if (job.p->noise_mode == 0) RAMP_HIP_CHECK(hipMemcpyAsync(c->rs_u, rj->u, ne * ng * 4, hipMemcpyDeviceToDevice, s));
  return stage_table(c, c->rs_gf, c->rs_gf_cap, rs->group_first_host, ng + 1, 0, hipMemcpyHostToDevice, s);
}
// (the rs_* buffers exist only for such a job, s_traj_scene with `scenes`; flags, lambda, ess_frac, the scalars and the Philox group fields are
// kernel arguments of the captured nodes)
static void key_resample(Key& key, const SampleJob& job) {
  const ResampleJob* rj = job.resampling(); const ramp_resample_params* rs = rj->rs; const ramp_cost_guide* rc = rs->cost;
  const int tag[9] = {0x52534d50 /* "RSMP" */, rs->n_groups, rj->n_events, rs->group0, rs->groups_total, rc->point_dim, rc->n_scenes,
                      rc->cloud_offset_host[rc->n_scenes], job.sc ? 1 : 0}; key.put(tag, 9);
  const double sc5[5] = {rs->ess_frac, rc->radius, rc->w_obs, rc->w_smooth, rc->w_acc}; key.put(sc5, 5);
  key.put(rs->resample, job.p->n_steps); key.put(rs->lambda, job.p->n_steps);
}

// Stitched windows (ramp_sample_stitched, the only entry that brings a table)
static int check_stitch_job(ramp_ctx* c, const SampleJob& job) {
  const ramp_stitch* st = job.st; const ramp_sample_params* p = job.p;
  if (!st) return 0;
  const std::string w = std::string(job.who) + ": ";
  CK(check_stitch(st, p->B, c->cfg.horizon, job.who));
  RAMP_REQUIRE(p->n_hard == 0, w + "p->n_hard must be 0 (the pins are the job's conditions)");
  RAMP_REQUIRE(p->philox_total == 0, w + "a sharded job is not served (the windows of a chain must sit in one shard)");
  return 0;
}
// {alpha | zeros} and the pin values
static int stage_stitch(ramp_ctx* c, const SampleJob& job, hipStream_t s) {
  const ramp_stitch* st = job.st;
  const int O = st->n_windows > 1 ? st->overlap : 0;
  std::vector<float> al(2 * (size_t)O, 0.f);
  for (int k = 0; k < O; ++k) al[k] = st->alpha_host[k];
  const size_t pv = (size_t)st->n_pin * (job.p->B / st->n_windows) * c->cfg.state_dim;
  // (al is pageable host memory: its copy is staged before the call returns, so the vector may go out of scope)
  CK(stage_table(c, c->st_alpha, c->st_alpha_cap, (const float*)al.data(), al.size(), 4, hipMemcpyHostToDevice, s));
  return stage_table(c, c->st_pin_val, c->st_pin_val_cap, st->pin_val, pv, 4, hipMemcpyDeviceToDevice, s);
}
// (st_alpha / st_pin_val exist only for such a job; the layout and the pin indices are kernel arguments of the captured nodes)
static void key_stitch(Key& key, const ramp_stitch* st) {
  const int tag[4] = {0x53544348 /* "STCH" */, st->n_windows, st->n_windows > 1 ? st->overlap : 0, st->n_pin}; key.put(tag, 4);
  if (st->n_pin) key.put(st->pin_idx_host, st->n_pin);
}

// A warm start (ramp_sample_warm, the only entry that brings one)
static int check_warm(ramp_ctx* c, const SampleJob& job) {
  const ramp_warm_start* ws = job.ws; const ramp_sample_params* p = job.p;
  if (!ws) return 0;
  const std::string w = std::string(job.who) + ": ";
  RAMP_REQUIRE(p->B > 0 && p->n_steps > 0, w + "bad sample dims");
  RAMP_REQUIRE(ws->j0_host && ws->has_prior_host, w + "null j0 / has_prior table");
  RAMP_REQUIRE((c->cfg.horizon * c->cfg.state_dim) % 4 == 0, w + "H * S must be a multiple of 4 (the warm start moves four elements per access)");
  RAMP_REQUIRE(ws->n_hold >= 0 && ws->n_hold < p->n_steps, w + "n_hold outside 0 .. n_steps - 1");
  int top = 0;
  for (int b = 0; b < p->B; ++b) {
    const int j0 = ws->j0_host[b];
    RAMP_REQUIRE(j0 >= 0 && j0 <= ws->n_hold, w + "j0 outside 0 .. n_hold");
    top = std::max(top, j0);
    if (!ws->has_prior_host[b]) { RAMP_REQUIRE(j0 == 0, w + "a row without a prior starts at iteration 0 (j0 != 0)"); continue; }
    RAMP_REQUIRE(ws->prior && ws->sa_host && ws->s1a_host, w + "null prior / coefficient table with a prior somewhere");
    RAMP_REQUIRE(std::isfinite(ws->sa_host[b]) && std::isfinite(ws->s1a_host[b]), w + "a start coefficient is not finite");
  }
  RAMP_REQUIRE(top == ws->n_hold, w + "n_hold must be the largest j0");
  if (ws->n_hold > 0) {      // mixed levels
    RAMP_REQUIRE(!job.resampling(), w + "mixed levels with resampling events are not served (a held row could become an ancestor)");
    RAMP_REQUIRE(!job.tg, w + "mixed levels with a team are not served (a held agent would face moving team mates)");
    RAMP_REQUIRE(!job.st, w + "mixed levels on stitched windows are not served (the windows of a chain start together)");
  }
  return 0;
}
// priors, {j0 | has_prior} and {sa | s1a} into the context; x_init's buffer where a hold will read it
static int stage_warm(ramp_ctx* c, const SampleJob& job, hipStream_t s) {
  const ramp_warm_start* ws = job.ws;
  const size_t B = (size_t)job.p->B, n = B * c->cfg.horizon * c->cfg.state_dim;
  std::vector<int32_t> tab(2 * B); std::vector<float> coef(2 * B, 0.f);
  bool any = false;
  for (size_t b = 0; b < B; ++b) {
    tab[b] = ws->j0_host[b]; tab[B + b] = ws->has_prior_host[b] != 0;
    if (tab[B + b]) { coef[b] = ws->sa_host[b]; coef[B + b] = ws->s1a_host[b]; any = true; }
  }
  // (tab / coef are pageable host memory: their copies are staged before the call returns, so the vectors may go out of scope)
  CK(stage_table(c, c->w_tab, c->w_tab_cap, (const int*)tab.data(), tab.size(), 0, hipMemcpyHostToDevice, s));
  CK(stage_table(c, c->w_coef, c->w_coef_cap, (const float*)coef.data(), coef.size(), 0, hipMemcpyHostToDevice, s));
  CK(stage_table(c, c->w_prior, c->w_prior_cap, ws->prior, any ? n : 0, n, hipMemcpyDeviceToDevice, s));
  if (ws->n_hold > 0) CK(grow(c, c->w_xinit, c->w_xinit_cap, n));
  return 0;
}
// (w_prior / w_tab / w_coef exist only for such a job, w_xinit only with a hold; levels, coefficients and priors are data of the graph.  The
// hold's iteration index is a kernel argument, and n_hold decides how many holds the graph has)
static void key_warm(Key& key, const ramp_warm_start* ws) {
  const int tag[2] = {0x5741524d /* "WARM" */, ws->n_hold}; key.put(tag, 2);
}

// A checked job (run_sample): parameter checks, buffers, staging, the canonical calibration, the graph and the copy-out
static int sample_job(ramp_ctx* c, const SampleJob& job, void* stream) {
  const ramp_sample_params* p = job.p; const ramp_scene_batch* sc = job.sc; const ramp_guidance_rows* g = job.g; const float* noise = job.noise;
  const McmcJob* mj = job.mcmc(); const ResampleJob* rj = job.resampling();
  RAMP_REQUIRE(p->noise_mode == 0 || p->noise_mode == 1, "noise_mode must be 0 (injected) or 1 (Philox inside the job)");
  RAMP_REQUIRE(p->philox_total == 0 || (p->philox_sample0 >= 0 && p->philox_sample0 + p->B <= p->philox_total), "philox shard outside the job (philox_sample0 + B <= philox_total)");
  RAMP_REQUIRE(p->noise_mode == 0 || (c->cfg.horizon * c->cfg.state_dim) % 4 == 0, "noise_mode 1 needs H * S to be a multiple of 4");
  RAMP_REQUIRE(noise || p->noise_mode == 1, "null noise (only a job that draws its own, noise_mode 1, may omit it)");
  RAMP_REQUIRE(p->B > 0 && p->n_steps > 0 && p->n_rp >= 1 && p->n_rp <= (g ? RAMP_MAX_ROWS_PER_TRAJ : 3), "bad sample dims");
  RAMP_REQUIRE(p->t && p->sqrt_recip && p->sqrt_recipm1, "missing schedule arrays");
  if (p->ddim) RAMP_REQUIRE(p->sqrt_a_t && p->sqrt_1m_a_t && p->sqrt_a_prev && p->dir_coef, "missing DDIM arrays");
  else RAMP_REQUIRE(p->coef1 && p->coef2 && p->stdv && p->use_noise, "missing DDPM arrays");
  RAMP_REQUIRE(p->n_hard == 0 || (p->hard_idx_host && p->hard_val), "missing hard conditions");
  hipStream_t s = as_stream(stream);
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  const size_t n = (size_t)B * H * S, n_noise = (p->ddim ? 1 : (size_t)p->n_steps + 1) * n;
  const bool chain = job.chain_out != nullptr;
  CK(ensure_sampler_buffers(c, B, p->n_rp, p->n_steps, chain));
  const int n_evals = p->n_steps + (mj ? mj->total : 0);
  CK(grow(c, c->trip_log, c->trip_log_cap, (size_t)std::max(256, n_evals)));
  if (mj) CK(grow_mcmc(c, p, mj));
  for (int j = 0; j < p->n_hard; ++j) RAMP_REQUIRE(p->hard_idx_host[j] >= 0 && p->hard_idx_host[j] < H, "hard index out of range");
  if (!c->s_hard_idx) CK(renew(c, c->s_hard_idx, 256));
  RAMP_REQUIRE(p->n_hard <= 256, "too many hard conditions");
  if (p->apf.cloud) CK(stage_apf(c, p->apf, p->apf.cloud, p->apf.n_points, s));
  if (sc) {
    RAMP_REQUIRE(!p->apf.cloud, "ramp_sample_scenes: apf.cloud must be NULL (the clouds come with the scene batch)");
    CK(check_scene_batch(sc, sc->cloud_points != nullptr, "ramp_sample_scenes"));
    CK(stage_scenes(c, job, s));
  }
  if (job.cg) CK(stage_guide(c, job, s));
  if (rj) CK(stage_resample(c, job, s));
  if (job.st) CK(stage_stitch(c, job, s));
  if (job.ws) CK(stage_warm(c, job, s));
  std::vector<float> g_host;      // a composed job's weights on the host: part of the canonical calibration's key below
  if (g) CK(stage_guidance(c, job, s, g_host));
  if (p->n_hard) RAMP_HIP_CHECK(hipMemcpyAsync(c->s_hard_idx, p->hard_idx_host, p->n_hard * 4, hipMemcpyHostToDevice, s));
  CK(stage_table(c, c->s_hard_val, c->s_hard_val_cap, p->hard_val, (size_t)p->n_hard * B * S, 0, hipMemcpyDeviceToDevice, s));
  if (p->noise_mode == 1) {
    if (!c->s_philox) CK(renew(c, c->s_philox, 2));
    const unsigned long long rec[2] = {p->philox_seed, p->philox_offset};
    RAMP_HIP_CHECK(hipMemcpyAsync(c->s_philox, rec, 16, hipMemcpyHostToDevice, s));     // (pageable host memory: the copy is staged before the call returns)
  } else {
    RAMP_HIP_CHECK(hipMemcpyAsync(c->s_noise, noise, n_noise * 4, hipMemcpyDeviceToDevice, s));
    if (mj) RAMP_HIP_CHECK(hipMemcpyAsync(c->m_noise, job.mcmc_noise, (size_t)mj->total * n * 4, hipMemcpyDeviceToDevice, s));
    if (mj && mj->kind == 2) RAMP_HIP_CHECK(hipMemcpyAsync(c->m_u, job.mcmc_u, (size_t)mj->total * B * 4, hipMemcpyDeviceToDevice, s));
  }
  c->launches = 0;
  invalidate_calibrations(c, CAL_SCORE | CAL_REPLAN);      // the loop below overwrites the delayed-scaling tables
  // key: everything baked into the captured nodes, and whatever decides that the job touches a buffer that may not exist yet (s_chain: ch;
  // s_cloud / s_window: has_apf and apply_apf; s_hard_val: n_hard; s_philox: noise_mode; g_weight: the COMP tag); the options add their own
  Key key;
  const double kw0 = g ? 0.0 : p->w0, kw1 = g ? 0.0 : p->w1;      // (a composed job's weights are data of the graph, not part of its shape)
  key.put(p->B); key.put(p->n_rp); key.put(p->n_steps); key.put(p->ddim); key.put(kw0); key.put(kw1);
  key.put(p->t, p->n_steps); key.put(p->sqrt_recip, p->n_steps); key.put(p->sqrt_recipm1, p->n_steps);
  if (p->ddim) { key.put(p->sqrt_a_t, p->n_steps); key.put(p->sqrt_1m_a_t, p->n_steps); key.put(p->sqrt_a_prev, p->n_steps); key.put(p->dir_coef, p->n_steps); }
  else { key.put(p->coef1, p->n_steps); key.put(p->coef2, p->n_steps); key.put(p->stdv, p->n_steps); key.put(p->use_noise, p->n_steps); }
  if (p->apply_apf) key.put(p->apply_apf, p->n_steps);
  if (p->noise_scale) key.put(p->noise_scale, p->n_steps);
  key.put(p->clip_denoised); key.put(p->predict_x0); key.put(p->n_hard);
  key.put(p->philox_sample0); key.put(p->philox_total);
  const int has_apf = p->apf.cloud != nullptr; key.put(has_apf);
  key.put(p->apf.n_points); key.put(p->apf.window); key.put(p->apf.threshold); key.put(p->apf.strength); key.put(p->apf.passes);
  const int ch = chain; key.put(ch); key.put(c->force_x6); key.put(p->noise_mode);
  if (g) { const int tag = 0x434f4d50 /* "COMP" */; key.put(tag); }
  if (sc) key_scenes(key, sc);
  if (mj) key_mcmc(key, mj, p->n_steps);
  if (job.cg) key_guide(key, job);
  if (rj) key_resample(key, job);
  if (job.st) key_stitch(key, job.st);
  if (job.ws) key_warm(key, job.ws);
  const bool h3 = c->gemm_mode == 2 && !c->force_x6;
  const bool steady = h3 && c->cal_reuse;
  if (steady) {
    // what the canonical maxima depend on: batch, row variants and their weights, first timestep (the scene and the launch plan invalidate it
    // where they change) -- nothing of the caller's data
    Key ck;
    ck.put(p->B); ck.put(p->n_rp); ck.put(p->t[0]); ck.put(kw0); ck.put(kw1);
    const int sp = c->share_prefix; ck.put(sp);
    if (g) { const int tag = 0x434f4d50; ck.put(tag); ck.put(g_host.data(), (int)g_host.size()); }      // (the operand maxima of the prefix backward follow the weights)
    ck.put(c->scene_epoch);                                 // the scene table's identity; redundant today: set_scene_table drops every saved table (c_cal_valid)
    if (!c->c_cal_valid) {                                  // (scene / plan / mode changed: every saved table is stale; its buffer is reused)
      for (auto& kv : c->c_cal_saved) c->c_cal_free.push_back(kv.second);
      c->c_cal_saved.clear();
    }
    if (!c->c_cal_valid || c->c_cal_key != ck.bytes) {
      float* t2 = c->table(TABLE_CANONICAL);
      auto it = c->c_cal_saved.find(ck.bytes);
      if (it != c->c_cal_saved.end()) {                      // a job shape seen before: its table back into place
        RAMP_HIP_CHECK(hipMemcpyAsync(t2, it->second, ramp_ctx::MAX_SITES * sizeof(float), hipMemcpyDeviceToDevice, s));
      } else {
        CK(canonical_calibration(c, p, s));
        if (c->c_cal_saved.size() < 16) {
          float* keep = nullptr;
          if (!c->c_cal_free.empty()) { keep = c->c_cal_free.back(); c->c_cal_free.pop_back(); }
          else CK(dev_alloc(c, &keep, ramp_ctx::MAX_SITES));      // (no graph holds it: not a move)
          RAMP_HIP_CHECK(hipMemcpyAsync(keep, t2, ramp_ctx::MAX_SITES * sizeof(float), hipMemcpyDeviceToDevice, s));
          c->c_cal_saved[ck.bytes] = keep;
        }
      }
      c->c_cal_valid = true; c->c_cal_key = ck.bytes;
      c->launches = 0;
    }
  }
  staging_done(c);      // (after the last grow, before the graph key is compared)
  const int cal_eval = (h3 && c->rerun) ? c->trip_eval : -1;
  c->last_job_steps = h3 ? n_evals : 0;
  if (!p->use_graph) {
    CK(sample_body(c, job, s, chain, steady, cal_eval));
  } else {
    if (key.bytes != c->graph_key) { drop_graphs(c->s_graph, 3); c->graph_key = key.bytes; c->graph_rerun_key.clear(); }
    hipGraphExec_t* slot = &c->s_graph[steady ? 1 : 0];
    if (cal_eval >= 0) {     // the repeat of a flagged job: a graph of its own (kept: a checkpoint that trips at one evaluation does so every job)
      Key rk = key; rk.put(cal_eval); rk.put((int)steady);
      slot = &c->s_graph[2];
      if (rk.bytes != c->graph_rerun_key) drop_graphs(slot, 1);
      c->graph_rerun_key = rk.bytes;
    }
    CK(replay(slot, s, [&](hipStream_t cs) { return sample_body(c, job, cs, chain, steady, cal_eval); }));
  }
  if (mj && job.accept_out) RAMP_HIP_CHECK(hipMemcpyAsync(job.accept_out, c->m_flag, (size_t)mj->total * B * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (rj) {
    const size_t ne = (size_t)rj->n_events, ng = (size_t)rj->rs->n_groups;
    if (rj->ancestor_out) RAMP_HIP_CHECK(hipMemcpyAsync(rj->ancestor_out, c->rs_anc, ne * B * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (rj->ess_out) RAMP_HIP_CHECK(hipMemcpyAsync(rj->ess_out, c->rs_ess, ne * ng * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (rj->cost_out) RAMP_HIP_CHECK(hipMemcpyAsync(rj->cost_out, c->rs_cost, ne * B * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (rj->logw_out) RAMP_HIP_CHECK(hipMemcpyAsync(rj->logw_out, c->rs_state, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  if (job.chain_out) RAMP_HIP_CHECK(hipMemcpyAsync(job.chain_out, c->s_chain, (size_t)(p->n_steps + 1) * n * 4, hipMemcpyDeviceToDevice, s));
  if (job.x_out) RAMP_HIP_CHECK(hipMemcpyAsync(job.x_out, c->s_x, n * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// The one runner behind the nine entries (each has made its own null checks): plain (g, scenes NULL), many-scene (scenes) and composed (g)
// jobs with whatever options the entry has a slot for.  The option checks run in the order in which refusals have always been tried (the first
// message wins) and switch off what changes nothing; a job whose options are all off is the plain entry's, bit for bit.
static int run_sample(ramp_ctx* c, const SampleJob& stated, void* stream) {
  SampleJob job = stated;
  const std::string w = std::string(job.who) + ": ";
  const int kind = job.mj.kind;
  const int rc = [&]() -> int {
    CK(check_stitch_job(c, job));
    RAMP_REQUIRE(kind >= 0 && kind <= 2, w + "kind must be 0 (off), 1 (ULA) or 2 (MALA)");      // (in front of the guidance table's checks)
    if (job.g) CK(check_guidance(c, job.p, job.g, job.who));
    CK(check_mcmc(job)); CK(check_guide(c, job)); CK(check_resample(c, job)); CK(check_warm(c, job));
    return sample_job(c, job, stream);
  }();
  c->g_weight_cur = nullptr;      // on every return path
  return rc;
}
// what the entries of the ramp_sample_mcmc family have in common
static SampleJob refined_job(const char* who, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_mcmc_params* m,
                             const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise, const float* mcmc_noise,
                             const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out) {
  const McmcJob mj = m ? McmcJob{m->kind, m->n_inner, m->step_size, m->sigma, 0} : McmcJob{0, nullptr, nullptr, nullptr, 0};
  return SampleJob{who, p, scenes, noise, chain_out, x_out, g, cg, mj, mcmc_noise, mcmc_u, accept_out};
}

int ramp_sample(ramp_ctx* c, const ramp_sample_params* p, const float* noise, float* chain_out, float* x_out, void* stream) {
  RAMP_REQUIRE(c && p, "null argument");
  return run_sample(c, SampleJob{"ramp_sample", p, nullptr, noise, chain_out, x_out}, stream);
}

int ramp_sample_scenes(ramp_ctx* c, const ramp_sample_params* p, const ramp_scene_batch* scenes, const float* noise, float* chain_out, float* x_out, void* stream) {
  RAMP_REQUIRE(scenes, "null scene batch");
  RAMP_REQUIRE(c && p, "null argument");
  return run_sample(c, SampleJob{"ramp_sample_scenes", p, scenes, noise, chain_out, x_out}, stream);
}

// Composition over any number of obstacle sets (diffusion_model_static.py:188-229; diffusion_model_3d.py:163-182, three sets at :165-174) and many
// scenes per job: rows and weights are data.
int ramp_sample_composed(ramp_ctx* c, const ramp_sample_params* p, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                         float* chain_out, float* x_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_composed: null argument");
  RAMP_REQUIRE(g, "ramp_sample_composed: null guidance table");
  return run_sample(c, SampleJob{"ramp_sample_composed", p, scenes, noise, chain_out, x_out, g}, stream);
}

// Langevin refinement inside the job.  kind 0 / no inner step anywhere is the matching plain entry, bit for bit
int ramp_sample_mcmc(ramp_ctx* c, const ramp_sample_params* p, const ramp_mcmc_params* m, const ramp_guidance_rows* g,
                     const ramp_scene_batch* scenes, const float* noise, const float* mcmc_noise, const float* mcmc_u, float* chain_out,
                     float* x_out, int32_t* accept_out, void* stream) {
  RAMP_REQUIRE(c && p && m, "ramp_sample_mcmc: null argument");
  return run_sample(c, refined_job("ramp_sample_mcmc", p, nullptr, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out, x_out, accept_out), stream);
}

// ramp_sample_mcmc plus cost-gradient guidance.  cg == NULL / no guide iteration anywhere is that entry itself
int ramp_sample_guided(ramp_ctx* c, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_mcmc_params* m,
                       const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise, const float* mcmc_noise,
                       const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_guided: null argument");
  return run_sample(c, refined_job("ramp_sample_guided", p, cg, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out, x_out, accept_out), stream);
}

// ramp_sample_guided with the swept box and sphere terms.  pg == NULL, w_prim == 0 or no primitive anywhere is that entry itself
int ramp_sample_guided_prims(ramp_ctx* c, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                             const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                             const float* mcmc_noise, const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_guided_prims: null argument");
  SampleJob job = refined_job("ramp_sample_guided_prims", p, cg, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out, x_out, accept_out);
  job.pg = pg;
  return run_sample(c, job, stream);
}

// ramp_sample_guided with the separation term between the rows of a team.  tg == NULL, one agent per team or w_team == 0 is that entry itself
int ramp_sample_guided_team(ramp_ctx* c, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                            const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                            const float* mcmc_noise, const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_guided_team: null argument");
  SampleJob job = refined_job("ramp_sample_guided_team", p, cg, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out, x_out, accept_out);
  job.tg = tg;
  return run_sample(c, job, stream);
}

// ramp_sample_guided plus the resampling events.  rs == NULL or no flag set is that entry itself, and reports under its name
int ramp_sample_steered(ramp_ctx* c, const ramp_sample_params* p, const ramp_resample_params* rs, const ramp_cost_guide* cg,
                        const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                        const float* mcmc_noise, const float* mcmc_u, const float* resample_u, float* chain_out, float* x_out,
                        int32_t* accept_out, int32_t* ancestor_out, double* ess_out, double* cost_out, double* logw_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_steered: null argument");
  ResampleJob rj{rs, 0, resample_u, ancestor_out, ess_out, cost_out, logw_out};
  if (rs && rs->resample) for (int j = 0; j < p->n_steps; ++j) rj.n_events += rs->resample[j] != 0;
  if (rj.n_events) RAMP_REQUIRE(rs->cost, "ramp_sample_steered: null cost table");
  SampleJob job = refined_job(rj.n_events ? "ramp_sample_steered" : "ramp_sample_guided", p, cg, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out,
                              x_out, accept_out);
  job.rj = rj;
  return run_sample(c, job, stream);
}

// ramp_sample_guided (no MCMC, no composed weights) on stitched windows.  st == NULL is that entry itself, and reports under its name
int ramp_sample_stitched(ramp_ctx* c, const ramp_sample_params* p, const ramp_stitch* st, const ramp_cost_guide* cg, const ramp_scene_batch* scenes,
                         const float* noise, float* chain_out, float* x_out, float* long_out, void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_stitched: null argument");
  if (!st) RAMP_REQUIRE(!long_out, "ramp_sample_stitched: long_out needs a stitch table");
  SampleJob job{st ? "ramp_sample_stitched" : "ramp_sample_guided", p, scenes, noise, chain_out, x_out, nullptr, cg};
  job.st = st;
  CK(run_sample(c, job, stream));
  if (!st || !long_out) return 0;
  return launch_stitch_assemble(c->s_x, long_out, p->B / st->n_windows, st->n_windows, c->cfg.horizon, c->cfg.state_dim, st->overlap, as_stream(stream));
}

// Any job of the family above from a warm start: ws == NULL is the entry that takes the same options, and launches what it launches
int ramp_sample_warm(ramp_ctx* c, const ramp_sample_params* p, const ramp_warm_start* ws, const ramp_stitch* st,
                     const ramp_resample_params* rs, const ramp_cost_guide* cg, const ramp_prim_guide* pg, const ramp_team_guide* tg,
                     const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                     const float* mcmc_noise, const float* mcmc_u, const float* resample_u, float* chain_out, float* x_out,
                     int32_t* accept_out, int32_t* ancestor_out, double* ess_out, double* cost_out, double* logw_out, float* long_out,
                     void* stream) {
  RAMP_REQUIRE(c && p, "ramp_sample_warm: null argument");
  RAMP_REQUIRE(!(pg && tg), "ramp_sample_warm: a job carries a team or primitives, never both");
  RAMP_REQUIRE(!st || !(rs || pg || tg || m || g), "ramp_sample_warm: stitched windows take no resampling, primitives, team, MCMC or composed weights");
  RAMP_REQUIRE(st || !long_out, "ramp_sample_warm: long_out needs a stitch table");
  ResampleJob rj{rs, 0, resample_u, ancestor_out, ess_out, cost_out, logw_out};
  if (rs && rs->resample) for (int j = 0; j < p->n_steps; ++j) rj.n_events += rs->resample[j] != 0;
  if (rj.n_events) RAMP_REQUIRE(rs->cost, "ramp_sample_warm: null cost table");
  SampleJob job = refined_job("ramp_sample_warm", p, cg, m, g, scenes, noise, mcmc_noise, mcmc_u, chain_out, x_out, accept_out);
  job.pg = pg; job.tg = tg; job.rj = rj; job.st = st; job.ws = ws;
  CK(run_sample(c, job, stream));
  if (!st || !long_out) return 0;
  return launch_stitch_assemble(c->s_x, long_out, p->B / st->n_windows, st->n_windows, c->cfg.horizon, c->cfg.state_dim, st->overlap, as_stream(stream));
}

// ---- receding-horizon replanning --------------------------------------------------------------------
// One replan of DynamicGaussianDiffusionModel.ddim_p_sample_loop (diffusion_model_dynamic.py:533-612) as ONE captured
// graph: q_sample of the current plan -> n_steps x [score, CFG + x0, (last step: static + pursuer APF), DDIM update,
// pinned waypoints] -> smoothing -> collision mask / costs -> selection.  The pursuer's new position is computed by the
// caller BEFORE the replan: the reference hands the environment x[:, stepp, :2], which is the pinned executed state.
// The job is the replan of E episodes in lock-step: row b reads the record, history, clean plan, clouds and goal of its own episode
// (the e_* buffers); ramp_replan's single episode is E = 1, where every row reads episode 0's.
// rg != nullptr: the cost guide (checked by the entry, its tables staged by stage_replan_guide): on step j with n_guide[j] > 0 ONE launch on x0, behind the CFG
// combination and, on the last step, behind both APF passes and the goal copy, in front of the DDIM update
struct EpisodeJob { int E, P_static, P_cost; };      // episodes; points of the concatenated static APF clouds / of the cost segments
static int replan_body(ramp_ctx* c, const ramp_replan_params* p, hipStream_t s, bool calibrate, const EpisodeJob& ej, const ramp_replan_guide* rg) {
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  const size_t HS = (size_t)H * S;
  HardConds hc; hc.idx = c->e_hard_idx; hc.val = c->e_hard_val; hc.n = p->n_hard;
  HardConds none;
  EpisodeTable et; et.st = c->e_state; et.row_ep = c->e_row_ep; et.n_episodes = ej.E;
  CK(launch_replan_init_episodes(c->s_x, c->e_xclean, c->e_noise, p->q_sqrt_a, p->q_sqrt_1m_a, c->e_hist, et, B, H, S, s));
  const bool h3 = c->gemm_mode == 2 && !c->force_x6;
  if (h3) {
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned*>(c->range_flag), 1);
    RAMP_HIP_CHECK(hipGetLastError());
  }
  const std::array<float, 3> comb = comb_weights(p->n_rp, p->w, 0.0);
  const bool shared = p->n_rp > 1 && c->share_prefix;
  MovingGuideArgs ga; int j_tap = -1;
  if (rg) {
    ga = moving_guide_args(rg, c->s_x0, B, H, S);
    ga.cloud = c->rg_cloud; ga.cloud_off = c->rg_off; ga.mov = c->rg_mov; ga.track = c->rg_track; ga.hc = hc;
    ga.scene = c->e_row_ep; ga.est = c->e_state; ga.hist = c->e_hist; ga.x_clean = c->e_xclean;
    if (rg->tap_out) for (int j = 0; j < p->n_steps; ++j) if (rg->n_guide[j] > 0) j_tap = j;
  }
  for (int j = 0; j < p->n_steps; ++j) {
    const bool last = p->t[j] == 0;                       // the reference's `i == 0`: smoothing + APF on the final step
    if (last) CK(launch_replan_sm_episodes(c->s_x, et, p->sm_window_last, p->sm_dt, p->sm_max_vel, B, H, S, s));
    // delayed-scaling tables: evaluation j writes table j & 1, the last one TABLE_REPLAN_CARRY, which the first evaluation of the
    // NEXT replan reads: every steady-state replan sees the same pointers, so its graph is captured once
    // (no flag log: a flagged replan is repeated whole by replan_job, and the sampling jobs' log stays theirs)
    const int t_out = j + 1 == p->n_steps ? TABLE_REPLAN_CARRY : (j & 1) ? TABLE_ODD : TABLE_EVEN;
    const int t_in = j == 0 ? TABLE_REPLAN_CARRY : (j & 1) ? TABLE_EVEN : TABLE_ODD;
    CK(guarded_eval(c, !h3 ? 0 : (calibrate && j == 0) ? 1 : 2, t_in, t_out, c->s_x, B, p->n_rp, p->t[j], nullptr, c->s_eps, s,
                    shared ? comb.data() : nullptr));
    CfgMeanArgs m; m.x = c->s_x; m.eps = c->s_eps; m.B = B; m.HS = (int)HS; m.n_rp = shared ? 1 : p->n_rp;
    m.w0 = (float)p->w; m.w1 = 0.f; m.w0p1 = (float)(1.0 + p->w);
    m.sqrt_recip = p->sqrt_recip[j]; m.sqrt_recipm1 = p->sqrt_recipm1[j]; m.clip = p->clip_denoised; m.predict_x0 = p->predict_x0 != 0;
    m.mean = nullptr; m.x0 = c->s_x0;
    CK(launch_cfg_mean(m, s));
    if (last) {
      CK(launch_replan_near_episodes(c->s_x, et, (float)p->thr_pred, c->e_en, B, H, S, s));
      ApfDynArgs a; a.traj = c->s_x0; a.B = B; a.H = H; a.S = S;
      a.points = c->e_static; a.P = ej.P_static; a.window = p->window_static; a.affected = H;
      a.thr_query = p->thr_static; a.thr_force = p->thr_static; a.strength = p->strength_static;
      a.episode = c->e_row_ep; a.ep_off = c->e_static_off; a.n_episodes = ej.E;
      CK(launch_apf_dynamic(a, s));
      a.points = c->e_dyn; a.P = p->n_dyn; a.ep_off = nullptr; a.window = -1; a.affected = H; a.thr_query = p->thr_pred;      // (n_dyn points per episode;
      a.strength = p->strength_pred; a.goal = c->s_x + (size_t)(H - 1) * S; a.enable = c->e_en;                              // every row its own goal)
      CK(launch_apf_dynamic(a, s));
      CK(launch_replan_goal(c->s_x0, c->s_x, B, H, S, s));
    }
    if (rg && rg->n_guide[j] > 0) {
      const long n_tap = (long)B * H * S;
      if (j == j_tap) CK(launch_copy_f32(c->rg_tap, c->s_x0, n_tap, s));
      ga.n_iter = rg->n_guide[j]; ga.step = rg->step[j];
      CK(launch_guide_step_moving(ga, s));
      if (j == j_tap) CK(launch_copy_f32(c->rg_tap + n_tap, c->s_x0, n_tap, s));
    }
    CK(launch_ddim_finish(c->s_x, c->s_x0, p->sqrt_a_t[j], p->sqrt_1m_a_t[j], p->sqrt_a_prev[j], p->dir_coef[j], none,
                          c->s_x, nullptr, B, H, S, s));
    CK(launch_replan_pin_episodes(c->s_x, hc, c->e_hist, c->e_xclean, et, B, H, S, s));
  }
  CK(launch_replan_sm_episodes(c->s_x, et, p->sm_window_final, p->sm_dt, p->sm_max_vel, B, H, S, s));
  CK(launch_traj_costs_scenes(c->s_x, c->e_cost, c->e_first, c->e_cost_off, ej.E, ej.P_cost, B, H, S, p->cost_thr, c->e_mask, c->e_plen,
                              c->e_smooth, s));
  CK(launch_select_episodes(c->s_x, c->e_mask, c->e_plen, c->e_smooth, p->w_smooth, p->w_len, c->e_first, et, c->e_best, c->e_result, B,
                            H, S, s));
  return 0;
}

// The guide of a replan: checked for the entry `who` (*active is false for rg == NULL or a guide without an iteration anywhere, which is the
// unguided call), its buffers grown with the job's other buffers (before staging_done), its tables copied with the job's other inputs
static int check_replan_job_guide(ramp_ctx* c, const ramp_replan_params* p, const ramp_replan_guide* rg, int n_scenes, const char* who, bool* active) {
  *active = false;
  if (!rg) return 0;
  int total = 0;
  CK(check_replan_guide(rg, n_scenes, c->cfg.horizon, c->cfg.state_dim, p->n_steps, who, &total));
  *active = total > 0;
  return 0;
}
static int grow_replan_guide(ramp_ctx* c, const ramp_replan_guide* rg, int B) {
  const size_t HS = (size_t)c->cfg.horizon * c->cfg.state_dim;
  CK(grow(c, c->rg_cloud, c->rg_cloud_cap, std::max<size_t>(4, (size_t)rg->cloud_offset_host[rg->n_scenes] * 2)));
  CK(grow(c, c->rg_off, c->rg_off_cap, (size_t)rg->n_scenes + 1));
  CK(grow(c, c->rg_mov, c->rg_mov_cap, std::max<size_t>(4, (size_t)rg->n_scenes * rg->n_mov * 2)));
  CK(grow(c, c->rg_track, c->rg_track_cap, std::max<size_t>(4, (size_t)rg->n_scenes * c->cfg.horizon * 2)));
  if (rg->tap_out) CK(grow(c, c->rg_tap, c->rg_tap_cap, 2 * (size_t)B * HS));
  return 0;
}
static int stage_replan_guide(ramp_ctx* c, const ramp_replan_guide* rg, hipStream_t s) {
  const size_t P = (size_t)rg->cloud_offset_host[rg->n_scenes];
  if (P) RAMP_HIP_CHECK(hipMemcpyAsync(c->rg_cloud, rg->cloud_points, P * 8, hipMemcpyDeviceToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->rg_off, rg->cloud_offset_host, ((size_t)rg->n_scenes + 1) * 4, hipMemcpyHostToDevice, s));
  if (rg->n_mov) {
    RAMP_HIP_CHECK(hipMemcpyAsync(c->rg_mov, rg->mov_points_host, (size_t)rg->n_scenes * rg->n_mov * 8, hipMemcpyHostToDevice, s));
    RAMP_HIP_CHECK(hipMemcpyAsync(c->rg_track, rg->mov_track_host, (size_t)rg->n_scenes * c->cfg.horizon * 8, hipMemcpyHostToDevice, s));
  }
  return 0;
}
// what a guide adds to a replan's graph key
static void key_replan_guide(Key& key, const ramp_replan_guide* rg, int n_steps) {
  key.put(rg->n_scenes); key.put(rg->n_mov); key.put(rg->cloud_offset_host[rg->n_scenes]);
  key.put(rg->radius); key.put(rg->radius_mov); key.put(rg->w_obs); key.put(rg->w_mov); key.put(rg->w_smooth); key.put(rg->w_acc);
  key.put(rg->max_norm); key.put(rg->n_guide, n_steps); key.put(rg->step, n_steps); key.put((int)(rg->tap_out != nullptr));
}

static_assert(sizeof(ramp_episode_state) == sizeof(EpisodeState) && sizeof(EpisodeState) == 32, "the host record is copied as the device record");
static_assert(offsetof(ramp_episode_state, active) == offsetof(EpisodeState, active) && offsetof(ramp_episode_state, pursuer) == offsetof(EpisodeState, pursuer), "the host record is copied as the device record");

// The replan of both entries behind their argument checks (`who` ran them, rg is an active guide or null, the tables of `ep` are sound
// and end at P_static / n_cost points): buffers, staging, graph key, run, the one read-back, the bf16x6 repeat of a flagged call and the
// outputs.  hist_floats: what `ep->history` holds -- whole (H, S) blocks per episode, or the single entry's n_hist rows.
static int replan_job(ramp_ctx* c, const ramp_replan_params* p, const ramp_episode_batch* ep, const ramp_replan_guide* rg, ramp_ctx::ReplanEntry who,
                      int P_static, int n_cost, size_t hist_floats, float* best_out, float* batch_out, int32_t* mask_out, int32_t* results_host,
                      ramp_replan_result* result_host, hipStream_t s) {
  const int B = p->B, E = ep->n_episodes, H = c->cfg.horizon, S = c->cfg.state_dim;
  const size_t HS = (size_t)H * S, n = (size_t)B * HS, nE = (size_t)E * HS;
  const int P_cost = n_cost + E * p->n_extra;
  // ---- fixed buffers the graphs read
  CK(ensure_sampler_buffers(c, B, p->n_rp, 0, false));
  if (rg) CK(grow_replan_guide(c, rg, B));
  if (!c->e_hard_idx) CK(renew(c, c->e_hard_idx, 16));
  if ((size_t)B > c->e_cap_B) {
    CK(renew(c, c->e_noise, n)); CK(renew(c, c->e_plen, B)); CK(renew(c, c->e_smooth, B));
    CK(renew(c, c->e_mask, B)); CK(renew(c, c->e_en, B)); CK(renew(c, c->e_row_ep, B));
    CK(renew(c, c->e_hard_val, (size_t)16 * B * S));
    c->e_cap_B = B;
  }
  if ((size_t)E > c->e_cap_E) {
    CK(renew(c, c->e_hist, nE)); CK(renew(c, c->e_xclean, nE)); CK(renew(c, c->e_best, nE)); CK(renew(c, c->e_state, E));
    CK(renew(c, c->e_result, (size_t)4 * E)); CK(renew(c, c->e_first, (size_t)E + 1)); CK(renew(c, c->e_static_off, (size_t)E + 1));
    CK(renew(c, c->e_cost_off, (size_t)E + 1));
    c->e_cap_E = E;
  }
  CK(grow(c, c->e_static, c->e_cap_static, (size_t)P_static * 2));
  CK(grow(c, c->e_dyn, c->e_cap_dyn, (size_t)E * p->n_dyn * 2));
  CK(grow(c, c->e_cost, c->e_cap_cost, (size_t)P_cost * 2));
  CK(grow(c, c->e_extra, c->e_cap_extra, std::max<size_t>((size_t)E * p->n_extra * 2, 2)));      // (staging only: no graph reads it)
  staging_done(c);
  // ---- this call's inputs.  Host staging lives until the synchronisation below.
  std::vector<int> row_ep(B), cost_off(E + 1);
  std::vector<float> extra((size_t)E * p->n_extra * 2, 1.0e9f);      // far-away fillers where the pursuer is not near
  for (int e = 0; e < E; ++e) {
    for (int b = ep->traj_first_host[e]; b < ep->traj_first_host[e + 1]; ++b) row_ep[b] = e;
    cost_off[e] = ep->cost_offset_host[e] + e * p->n_extra;
    if (ep->near_host[e] && p->n_extra)
      std::copy(ep->extra_pts_host + (size_t)e * p->n_extra * 2, ep->extra_pts_host + (size_t)(e + 1) * p->n_extra * 2, extra.begin() + (size_t)e * p->n_extra * 2);
  }
  cost_off[E] = P_cost;
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_noise, ep->noise, n * 4, hipMemcpyDeviceToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_hist, ep->history, hist_floats * 4, hipMemcpyDeviceToDevice, s));
  if (ep->x_clean) {      // (also what `best` holds for an episode that selects nothing in this call)
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_xclean, ep->x_clean, nE * 4, hipMemcpyDeviceToDevice, s));
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_best, ep->x_clean, nE * 4, hipMemcpyDeviceToDevice, s));
  } else {
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_xclean, c->e_best, nE * 4, hipMemcpyDeviceToDevice, s));
  }
  c->e_best_E = E; c->replan_last = who;
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_row_ep, row_ep.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_first, ep->traj_first_host, ((size_t)E + 1) * 4, hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_state, ep->state_host, (size_t)E * sizeof(EpisodeState), hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_static, ep->static_pts, (size_t)P_static * 16, hipMemcpyDeviceToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_static_off, ep->static_offset_host, ((size_t)E + 1) * 4, hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_dyn, ep->dyn_pts_host, (size_t)E * p->n_dyn * 16, hipMemcpyHostToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(c->e_cost_off, cost_off.data(), ((size_t)E + 1) * 4, hipMemcpyHostToDevice, s));
  // the cost segments (an episode's static cloud, then its n_extra slots) in one copy and one launch, whatever the number of episodes
  if (p->n_extra) RAMP_HIP_CHECK(hipMemcpyAsync(c->e_extra, extra.data(), extra.size() * 4, hipMemcpyHostToDevice, s));
  CK(launch_episode_cost_segments(c->e_cost, ep->cost_cloud, c->e_extra, c->e_cost_off, E, p->n_extra, P_cost, s));
  if (p->n_hard) {
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_hard_idx, p->hard_idx_host, p->n_hard * 4, hipMemcpyHostToDevice, s));
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_hard_val, p->hard_val, (size_t)p->n_hard * B * S * 4, hipMemcpyDeviceToDevice, s));
  }
  if (rg) CK(stage_replan_guide(c, rg, s));
  c->launches = 0;
  invalidate_calibrations(c, CAL_SCORE);      // (the replans carry their maxima in TABLE_REPLAN_CARRY: the sampling jobs' canonical table survives)
  if (c->replan_carry != who) c->replan_carry = ramp_ctx::REPLAN_NOBODY;      // (the other entry's maxima are not continued from)
  const bool h3 = c->gemm_mode == 2 && !c->force_x6;
  const EpisodeJob ej{E, P_static, P_cost};
  auto run = [&](bool calibrate) -> int {
    if (!p->use_graph) return replan_body(c, p, s, calibrate, ej, rg);
    Key key;      // everything baked into the nodes: the params' fields, the episode count, the row table and the clouds' totals
    key.put(p->B); key.put(p->n_steps); key.put(p->w); key.put(p->t, p->n_steps); key.put(p->sqrt_recip, p->n_steps);
    key.put(p->sqrt_recipm1, p->n_steps); key.put(p->sqrt_a_t, p->n_steps); key.put(p->sqrt_1m_a_t, p->n_steps);
    key.put(p->sqrt_a_prev, p->n_steps); key.put(p->dir_coef, p->n_steps); key.put(p->q_sqrt_a); key.put(p->q_sqrt_1m_a);
    key.put(p->clip_denoised); key.put(p->predict_x0); key.put(p->n_hard); key.put(p->sm_window_last); key.put(p->sm_window_final); key.put(p->sm_dt);
    key.put(p->sm_max_vel); key.put(p->n_dyn); key.put(p->thr_static); key.put(p->thr_pred);
    key.put(p->strength_static); key.put(p->strength_pred); key.put(p->window_static); key.put(p->n_extra);
    key.put(p->cost_thr); key.put(p->w_smooth); key.put(p->w_len); key.put(c->force_x6);
    key.put(E); key.put(ep->traj_first_host, (size_t)E + 1); key.put(P_static); key.put(P_cost);
    key.put((int)who);      // (a one-episode call of the episode entry would replay the single entry's graph unharmed; each keeps capturing its own,
                            // so that the launch count after a call says what it said when the two had a graph pair each)
    if (rg) key_replan_guide(key, rg, p->n_steps);
    if (key.bytes != c->e_key) { drop_graphs(c->e_graph, 2); c->e_key = key.bytes; }
    return replay(&c->e_graph[(h3 && !calibrate) ? 1 : 0], s, [&](hipStream_t cs) { return replan_body(c, p, cs, calibrate, ej, rg); });
  };
  // a one-step replan has no second table to carry its maxima in (its only evaluation reads and clears TABLE_REPLAN_CARRY): it always
  // calibrates, on the bf16x6 kernels, instead of running fp16x3 from an empty table
  CK(run(h3 && (c->replan_carry != who || p->n_steps == 1)));
  // ---- the one read-back: E result records {n_free, rank, row, 0} + the range flag
  std::vector<int> back((size_t)4 * E + 1, 0);
  RAMP_HIP_CHECK(hipMemcpyAsync(back.data(), c->e_result, (size_t)E * 16, hipMemcpyDeviceToHost, s));
  if (h3) RAMP_HIP_CHECK(hipMemcpyAsync(back.data() + 4 * E, c->range_flag, 4, hipMemcpyDeviceToHost, s));
  RAMP_HIP_CHECK(hipStreamSynchronize(s));
  result_host->fell_back = 0;
  if (h3 && back[4 * E]) {
    // an operand left the range the delayed scaling assumed: the whole call again (same inputs) on the bf16x6 kernels, and the next one
    // calibrates.  The flagged run left winners in e_best: back to the plans it started from first, which is what an episode that
    // selects nothing keeps
    RAMP_HIP_CHECK(hipMemcpyAsync(c->e_best, c->e_xclean, nE * 4, hipMemcpyDeviceToDevice, s));
    c->force_x6 = 1;
    int rc = replan_body(c, p, s, false, ej, rg);
    c->force_x6 = 0;
    CK(rc);
    const int flag = back[4 * E];
    RAMP_HIP_CHECK(hipMemcpyAsync(back.data(), c->e_result, (size_t)E * 16, hipMemcpyDeviceToHost, s));
    RAMP_HIP_CHECK(hipStreamSynchronize(s));
    c->replan_carry = ramp_ctx::REPLAN_NOBODY;
    result_host->fell_back = flag;
  } else if (h3) {
    c->replan_carry = who;
  }
  int n_free = 0;
  for (int e = 0; e < E; ++e) if (back[4 * e] > 0) n_free += back[4 * e];
  std::copy(back.begin(), back.begin() + (size_t)4 * E, results_host);
  result_host->n_free = n_free; result_host->best_rank = -1; result_host->best_row = -1;
  if (best_out) RAMP_HIP_CHECK(hipMemcpyAsync(best_out, c->e_best, nE * 4, hipMemcpyDeviceToDevice, s));
  if (batch_out) RAMP_HIP_CHECK(hipMemcpyAsync(batch_out, c->s_x, n * 4, hipMemcpyDeviceToDevice, s));
  if (mask_out) RAMP_HIP_CHECK(hipMemcpyAsync(mask_out, c->e_mask, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  if (rg && rg->tap_out) RAMP_HIP_CHECK(hipMemcpyAsync(rg->tap_out, c->rg_tap, 2 * n * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

int ramp_replan(ramp_ctx* c, const ramp_replan_params* p, const ramp_replan_state* st, float* best_out, float* batch_out,
                int32_t* mask_out, ramp_replan_result* result_host, void* stream) {
  return ramp_replan_guided(c, p, st, nullptr, best_out, batch_out, mask_out, result_host, stream);
}

// the one-episode job: the table of `p` and `st` as a ramp_episode_batch on the stack, the result from record 0.  It runs on whatever row ->
// latent table ramp_set_scene installed
int ramp_replan_guided(ramp_ctx* c, const ramp_replan_params* p, const ramp_replan_state* st, const ramp_replan_guide* rg, float* best_out,
                       float* batch_out, int32_t* mask_out, ramp_replan_result* result_host, void* stream) {
  RAMP_REQUIRE(c && p && st && result_host, rg ? "ramp_replan_guided: null argument" : "null argument");
  RAMP_REQUIRE(c->finalized && c->cross_bias, "context not ready (weights / scene)");
  const int B = p->B, H = c->cfg.horizon, S = c->cfg.state_dim;
  RAMP_REQUIRE(B > 0 && p->n_rp == 2 && p->n_steps >= 1 && p->n_steps <= 64, "bad replan dims");
  RAMP_REQUIRE(p->t && p->sqrt_recip && p->sqrt_recipm1 && p->sqrt_a_t && p->sqrt_1m_a_t && p->sqrt_a_prev && p->dir_coef, "missing schedule arrays");
  RAMP_REQUIRE(p->n_hard >= 0 && p->n_hard <= 16 && (p->n_hard == 0 || (p->hard_idx_host && p->hard_val)), "bad hard conditions");
  RAMP_REQUIRE(p->static_pts && p->n_static > 0 && p->n_dyn > 0 && p->cost_cloud && p->n_cost > 0 && p->n_extra >= 0, "bad clouds");
  RAMP_REQUIRE(st->noise && st->history && st->n_hist >= 1 && st->n_hist <= H && st->stepp >= 0 && st->stepp < H, "bad replan state");
  RAMP_REQUIRE(st->dyn_pts_host && (st->near == 0 || p->n_extra == 0 || st->extra_pts_host), "missing pursuer points");
  RAMP_REQUIRE(st->x_clean || c->replan_last == ramp_ctx::REPLAN_SINGLE, "no current plan: pass x_clean on the first replan");
  for (int j = 0; j < p->n_hard; ++j) RAMP_REQUIRE(p->hard_idx_host[j] >= 0 && p->hard_idx_host[j] < H, "hard index out of range");
  bool guided = false;
  CK(check_replan_job_guide(c, p, rg, 1, "ramp_replan_guided", &guided));
  if (!guided) rg = nullptr;
  const int32_t traj_first[2] = {0, B}, static_off[2] = {0, p->n_static}, cost_off[2] = {0, p->n_cost}, near = st->near;
  ramp_episode_state es{}; es.n_hist = st->n_hist; es.stepp = st->stepp; es.active = 1; es.pursuer[0] = st->pursuer[0]; es.pursuer[1] = st->pursuer[1];
  ramp_episode_batch ep{};
  ep.n_episodes = 1; ep.traj_first_host = traj_first; ep.noise = st->noise; ep.x_clean = st->x_clean; ep.history = st->history; ep.state_host = &es;
  ep.static_pts = p->static_pts; ep.static_offset_host = static_off; ep.dyn_pts_host = st->dyn_pts_host;
  ep.cost_cloud = p->cost_cloud; ep.cost_offset_host = cost_off; ep.near_host = &near; ep.extra_pts_host = st->extra_pts_host;
  int32_t record[4];
  CK(replan_job(c, p, &ep, rg, ramp_ctx::REPLAN_SINGLE, p->n_static, p->n_cost, (size_t)st->n_hist * S, best_out, batch_out, mask_out, record,
                result_host, as_stream(stream)));
  result_host->n_free = record[0]; result_host->best_rank = record[1]; result_host->best_row = record[2];
  return 0;
}

// (E + 1) first-entry table of host memory: [0] = 0, strictly increasing; returns the total through *total
static int check_offsets(const int32_t* off, int E, const char* what, int* total) {
  RAMP_REQUIRE(off && off[0] == 0, std::string(what) + ": the offset table must start at 0");
  for (int e = 0; e < E; ++e) RAMP_REQUIRE(off[e + 1] > off[e], std::string(what) + ": the offset table must be strictly increasing");
  *total = off[E];
  return 0;
}

int ramp_replan_episodes(ramp_ctx* c, const ramp_replan_params* p, const ramp_episode_batch* ep, float* best_out, float* batch_out,
                         int32_t* mask_out, int32_t* results_host, ramp_replan_result* result_host, void* stream) {
  return ramp_replan_episodes_guided(c, p, ep, nullptr, best_out, batch_out, mask_out, results_host, result_host, stream);
}

int ramp_replan_episodes_guided(ramp_ctx* c, const ramp_replan_params* p, const ramp_episode_batch* ep, const ramp_replan_guide* rg,
                                float* best_out, float* batch_out, int32_t* mask_out, int32_t* results_host,
                                ramp_replan_result* result_host, void* stream) {
  RAMP_REQUIRE(c && p && ep && results_host && result_host, rg ? "ramp_replan_episodes_guided: null argument" : "null argument");
  RAMP_REQUIRE(c->finalized && c->cross_bias, "context not ready (weights / scene)");
  const int B = p->B, E = ep->n_episodes, H = c->cfg.horizon;
  RAMP_REQUIRE(B > 0 && p->n_rp == 2 && p->n_steps >= 1 && p->n_steps <= 64, "bad replan dims");
  RAMP_REQUIRE(E >= 1 && E <= B && E <= 65536, "bad episode count (1 .. min(B, 65536))");
  RAMP_REQUIRE(c->rv_rows >= B * p->n_rp, "the row -> latent table of a many-episode replan comes from ramp_set_scenes (B * n_rp rows)");
  RAMP_REQUIRE(p->t && p->sqrt_recip && p->sqrt_recipm1 && p->sqrt_a_t && p->sqrt_1m_a_t && p->sqrt_a_prev && p->dir_coef, "missing schedule arrays");
  RAMP_REQUIRE(p->n_hard >= 0 && p->n_hard <= 16 && (p->n_hard == 0 || (p->hard_idx_host && p->hard_val)), "bad hard conditions");
  RAMP_REQUIRE(p->n_dyn > 0 && p->n_extra >= 0 && p->n_dyn <= (1 << 20) && p->n_extra <= (1 << 20), "bad clouds");
  RAMP_REQUIRE(ep->noise && ep->history && ep->state_host && ep->static_pts && ep->dyn_pts_host && ep->cost_cloud && ep->near_host, "missing episode inputs");
  int n_rows = 0, P_static = 0, n_cost = 0;
  CK(check_offsets(ep->traj_first_host, E, "traj_first", &n_rows));
  RAMP_REQUIRE(n_rows == B, "traj_first must end at the batch size");
  CK(check_offsets(ep->static_offset_host, E, "static clouds", &P_static));
  CK(check_offsets(ep->cost_offset_host, E, "cost clouds", &n_cost));
  RAMP_REQUIRE((long)n_cost + (long)E * p->n_extra < (1l << 31) && (long)E * p->n_dyn < (1l << 30), "the concatenated clouds do not fit 32-bit offsets");
  bool any_near = false;
  for (int e = 0; e < E; ++e) {
    const ramp_episode_state& st = ep->state_host[e];
    RAMP_REQUIRE(st.n_hist >= 1 && st.n_hist <= H && st.stepp >= 0 && st.stepp < H, "bad episode state");
    any_near |= ep->near_host[e] != 0;
  }
  RAMP_REQUIRE(!any_near || p->n_extra == 0 || ep->extra_pts_host, "missing pursuer points");
  RAMP_REQUIRE(ep->x_clean || (c->replan_last == ramp_ctx::REPLAN_EPISODES && c->e_best_E == E), "no current plans: pass x_clean on the first call");
  for (int j = 0; j < p->n_hard; ++j) RAMP_REQUIRE(p->hard_idx_host[j] >= 0 && p->hard_idx_host[j] < H, "hard index out of range");
  bool guided = false;
  CK(check_replan_job_guide(c, p, rg, E, "ramp_replan_episodes_guided", &guided));
  if (!guided) rg = nullptr;
  return replan_job(c, p, ep, rg, ramp_ctx::REPLAN_EPISODES, P_static, n_cost, (size_t)E * H * c->cfg.state_dim, best_out, batch_out, mask_out,
                    results_host, result_host, as_stream(stream));
}

/* compute_trajectory_costs + the winner (cost.py:56-88) for a finished batch, e.g. the high-level plan */
int ramp_select_best(const float* traj, int32_t B, int32_t H, int32_t S, const float* cloud, int32_t n_points, float threshold,
                     float w_smooth, float w_len, int32_t* mask, float* path_len, float* smooth, float* best_out,
                     int32_t* result_dev, void* stream) {
  RAMP_REQUIRE(traj && cloud && mask && path_len && smooth && best_out && result_dev, "null argument");
  hipStream_t s = as_stream(stream);
  CK(launch_traj_costs(traj, cloud, B, H, S, n_points, threshold, mask, path_len, smooth, s));
  return launch_replan_select(traj, mask, path_len, smooth, w_smooth, w_len, best_out, result_dev, B, H, S, s);
}

int ramp_select_from_costs(const int32_t* mask, const float* path_len, const float* smooth, int32_t B, float w_smooth, float w_len,
                           int32_t* result_dev, void* stream) {
  RAMP_REQUIRE(mask && path_len && smooth && result_dev && B > 0, "bad arguments");
  return launch_replan_select(nullptr, mask, path_len, smooth, w_smooth, w_len, nullptr, result_dev, B, 1, 1, as_stream(stream));
}

int ramp_replan_costs(ramp_ctx* c, int32_t B, int32_t* mask_out, float* path_len_out, float* smooth_out, void* stream) {
  RAMP_REQUIRE(c && c->e_mask && mask_out && path_len_out && smooth_out && B > 0 && (size_t)B <= c->e_cap_B, "no replan of this size has run on the context");
  hipStream_t s = as_stream(stream);
  RAMP_HIP_CHECK(hipMemcpyAsync(mask_out, c->e_mask, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(path_len_out, c->e_plen, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  RAMP_HIP_CHECK(hipMemcpyAsync(smooth_out, c->e_smooth, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

int ramp_debug_read(ramp_ctx* c, const char* kind, const char* module, float* out, int64_t n_floats,
                    int64_t* n_copied, void* stream) {
  RAMP_REQUIRE(c && kind && module && out && n_copied, "null argument");
  auto it = c->dbg.find(std::string(kind) + "/" + module);
  RAMP_REQUIRE(it != c->dbg.end(), std::string("no debug tap '") + kind + "/" + module + "' (debug_taps off or module unknown)");
  const size_t n = std::min<size_t>((size_t)n_floats, it->second.second);
  RAMP_HIP_CHECK(hipMemcpyAsync(out, it->second.first, n * 4, hipMemcpyDeviceToDevice, as_stream(stream)));
  *n_copied = (int64_t)n;
  return 0;
}

int ramp_profile(ramp_ctx* c, int32_t enable) {
  RAMP_REQUIRE(c, "null argument");
  c->prof_on = enable != 0;
  c->prof_used = 0; c->prof_cat.clear(); c->prof_flops.clear(); c->prof_shape.clear();
  return 0;
}
int ramp_profile_read(ramp_ctx* c, double* ms, double* flops, int64_t* count) {
  RAMP_REQUIRE(c && ms && flops && count, "null argument");
  RAMP_HIP_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < CAT_N; ++i) { ms[i] = 0; flops[i] = 0; count[i] = 0; }
  for (size_t i = 0; i < c->prof_cat.size(); ++i) {
    float t = 0.f;
    RAMP_HIP_CHECK(hipEventElapsedTime(&t, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
    ms[c->prof_cat[i]] += t; flops[c->prof_cat[i]] += c->prof_flops[i]; count[c->prof_cat[i]]++;
  }
  if (c->prof_dump) {      // per-shape GEMM table on stderr
    std::map<std::array<int, 4>, std::pair<double, int>> agg;
    for (size_t i = 0; i < c->prof_cat.size(); ++i) {
      if (c->prof_cat[i] != CAT_GEMM) continue;
      float t = 0.f; (void)hipEventElapsedTime(&t, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]);
      auto& e = agg[c->prof_shape[i]]; e.first += t; e.second++;
    }
    fprintf(stderr, "[ramp profile] %8s %5s %5s %4s %6s %10s %9s %8s\n", "M", "N", "K", "taps", "calls", "total_ms", "avg_us", "TFLOP/s");
    for (auto& kv : agg) {
      const auto& sh = kv.first; const double fl = 2.0 * sh[0] * sh[1] * sh[2] * sh[3];
      fprintf(stderr, "[ramp profile] %8d %5d %5d %4d %6d %10.2f %9.1f %8.1f\n", sh[0], sh[1], sh[2], sh[3], kv.second.second,
              kv.second.first, kv.second.first * 1e3 / kv.second.second, fl * kv.second.second / (kv.second.first * 1e-3) / 1e12);
    }
  }
  return 0;
}

// per-kernel sums of the profiled launches (the shape codes the launch wrappers record): index 0 ffx forward, 1 ffx backward,
// 2 tkl (LN1 -> QKV, d(o), out-projection), 3 tklb, 4 ato, 5 abl, 6 tkc, 7 tkw (wide k = 5 convolutions, GroupNorm fused),
// 8 every other launch of the GEMM class (tile kernels, exact-fp32 layers, the round-2 fused forward)
int ramp_profile_read_kernels(ramp_ctx* c, int32_t n, double* ms, double* flops, int64_t* count) {
  RAMP_REQUIRE(c && ms && flops && count && n >= 1 && n <= 16, "bad arguments");
  RAMP_HIP_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < n; ++i) { ms[i] = 0; flops[i] = 0; count[i] = 0; }
  for (size_t i = 0; i < c->prof_cat.size(); ++i) {
    if (c->prof_cat[i] != CAT_GEMM) continue;
    const auto& sh = c->prof_shape[i];
    int k = 8;
    if (sh[1] == -2) k = 0; else if (sh[1] == -3) k = 1;
    else if (sh[3] == -10 || sh[3] == -11) k = 2; else if (sh[3] == -12) k = 3; else if (sh[3] == -4) k = 4; else if (sh[3] == -6) k = 5;
    else if (sh[3] == -5) k = 6; else if (sh[3] == -7) k = 7;
    if (k >= n) continue;
    float t = 0.f;
    RAMP_HIP_CHECK(hipEventElapsedTime(&t, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
    ms[k] += t; flops[k] += c->prof_flops[i]; count[k]++;
  }
  return 0;
}

int ramp_set_fallback(ramp_ctx* c, int32_t mode) {
  RAMP_REQUIRE(c, "null argument");
  RAMP_REQUIRE(mode >= 0 && mode <= 2, "ramp_set_fallback: mode 0 (none), 1 (every evaluation on the bf16x6 kernels) or 2 (fp16x3, the flagged evaluation calibrating)");
  RAMP_REQUIRE(mode != 2 || c->trip_eval >= 0, "ramp_set_fallback(ctx, 2): no flagged evaluation on record (ramp_range_status of a flagged ramp_sample first)");
  c->force_x6 = mode == 1 ? 1 : 0;
  c->rerun = mode == 2 ? 1 : 0;
  invalidate_calibrations(c, CAL_SCORE | CAL_REPLAN);      // (the canonical table survives: nothing writes it in a bf16x6 job)
  return 0;
}
int ramp_score_mode(ramp_ctx* c, int32_t* mode) {
  RAMP_REQUIRE(c && mode, "null argument");
  *mode = c->score_last_mode;
  return 0;
}
int ramp_range_status(ramp_ctx* c, int32_t* flag, void* stream) {
  RAMP_REQUIRE(c && flag, "null argument");
  *flag = 0;
  if (c->range_flag) {
    RAMP_HIP_CHECK(hipStreamSynchronize(as_stream(stream)));
    RAMP_HIP_CHECK(hipMemcpy(flag, c->range_flag, sizeof(int), hipMemcpyDeviceToHost));
    if (!c->rerun) { c->trip_eval = -1; c->trip_site = -1; }      // (a repeat keeps its predecessor's record: what it was built from)
    if (*flag && !c->rerun && c->last_job_steps > 0 && c->trip_log) {      // the first evaluation of the last job that left the guard raised
      std::vector<int> log((size_t)c->last_job_steps);
      RAMP_HIP_CHECK(hipMemcpy(log.data(), c->trip_log, log.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int j = 0; j < c->last_job_steps; ++j) if (log[j]) { c->trip_eval = j; c->trip_site = log[j] - 1; break; }
    }
  }
  return 0;
}
int ramp_range_trip(ramp_ctx* c, int32_t* eval, int32_t* site) {
  RAMP_REQUIRE(c && eval, "null argument");
  *eval = c->trip_eval;
  if (site) *site = c->trip_site;
  return 0;
}
int ramp_set_calibration_reuse(ramp_ctx* c, int32_t on) {
  RAMP_REQUIRE(c, "null argument");
  c->cal_reuse = on ? 1 : 0;
  invalidate_calibrations(c, CAL_CANONICAL);
  return 0;
}
int ramp_workspace_bytes(ramp_ctx* c, int64_t* bytes) {
  RAMP_REQUIRE(c && bytes, "null argument");
  *bytes = (int64_t)c->arena.total;
  return 0;
}
int ramp_launch_count(ramp_ctx* c, int64_t* n) {
  RAMP_REQUIRE(c && n, "null argument");
  *n = c->launches;
  return 0;
}

}  // extern "C"
