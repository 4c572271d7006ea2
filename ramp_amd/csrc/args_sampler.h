// Launch arguments of the sampler, replanning, cost and metric kernels (sampler.hip, metrics.hip).
#pragma once
#include "core.h"

namespace ramp {

// ---- sampler (sampler.hip) ------------------------------------------------------------------
struct CfgMeanArgs {
  const float* x = nullptr;     // (B,H,S)
  const float* eps = nullptr;   // (B*n_rp,H,S) interleaved [v0,v1,(v2)] per trajectory
  float* x0 = nullptr; float* mean = nullptr;   // either may be null
  float* ecomb = nullptr;       // optional
  int B = 0, HS = 0, n_rp = 2;
  float w0 = 0, w1 = 0, w0p1 = 1; // n_rp=2: e=w0p1*v0 - w0*v1 (w0p1 = float(1+w)) ; n_rp=3: e=v2+w0*(v0-v2)+w1*(v1-v2)
  float sqrt_recip = 0, sqrt_recipm1 = 0, coef1 = 0, coef2 = 0; int clip = 1;
  int predict_x0 = 0;           // predict_epsilon=False (the reference constructor's default): the combined network output IS x0
};
int launch_cfg_mean(const CfgMeanArgs& a, hipStream_t s);
// the same step with e_comb[b] = sum_j row_weight[b n_rp + j] eps[b n_rp + j] (j = 0 .. n_rp - 1 in that order; row_weight device (B, n_rp),
// 2 <= n_rp <= 8, HS a multiple of 4); w0 / w1 / w0p1 are not read
int launch_cfg_mean_rows(const CfgMeanArgs& a, const float* row_weight, hipStream_t s);

struct HardConds { const int* idx = nullptr; const float* val = nullptr; int n = 0; };  // val (n,B,S)

// x = mean + (std * z) * noise_scale ; z = 0 when !use_noise (t == 0) ; then hard conditioning
int launch_ddpm_finish(const float* mean, const float* noise, float stdv, float noise_scale, int use_noise,
                       HardConds hc, float* x, float* chain_out, int B, int H, int S, hipStream_t s);
int launch_ddim_finish(const float* x_in, const float* x0, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                       float dir_coef, HardConds hc, float* x, float* chain_out, int B, int H, int S, hipStream_t s);
int launch_hard_cond(float* x, HardConds hc, int B, int H, int S, hipStream_t s);
// q_sample with one timestep per row (diffusion_model_static.py:467-476) and, with pin, both endpoints overwritten by x_start (:483-484):
// x_noisy[b] = sqrt_ac[t[b]] x_start[b] + sqrt_1m_ac[t[b]] noise[b]; pin: waypoints 0 and H - 1 = x_start's.  t device (B), schedules device (T);
// a row whose t is outside [0, T) is written as NaN, never read with it
int launch_q_sample_rows(const float* x_start, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int* t_rows, int T,
                         float* x_noisy, int B, int H, int S, int pin, hipStream_t s);
// out[0..n) ~ N(0, 1): Philox4x32-10 + Box-Muller, rec = device {seed, offset in groups of four elements} (sampler.hip)
int launch_philox_normal(float* out, long n, const unsigned long long* rec, hipStream_t s);
// the same stream addressed by GLOBAL sample index: out is this shard's (n_blocks, B, HS) noise block of a job whose whole
// noise block is (n_blocks, B_total, HS); local sample b is global sample sample0 + b, i.e. out[(j B + b) HS + e] = element
// (j B_total + sample0 + b) HS + e of the stream (HS % 4 == 0).  B_total == B, sample0 == 0 is launch_philox_normal.
// block0 > 0: the launch's block j is block block0 + j of the job's stream (the MCMC draws behind a job's main block)
int launch_philox_normal_sharded(float* out, int n_blocks, int B, int HS, long sample0, long B_total, const unsigned long long* rec, hipStream_t s,
                                 long block0 = 0);
// out (n_blocks, B) uniforms in (0, 1): out[k B + b] = ((r >> 9) + 0.5) 2^-23 with r = output 0 of the stream's group
// group0 + k B_total + sample0 + b (one group of four per uniform)
int launch_philox_uniform_sharded(float* out, int n_blocks, int B, long group0, long sample0, long B_total, const unsigned long long* rec,
                                  hipStream_t s);

// ---- energies and Langevin refinement (sampler.hip) ------------------------------------------------
// E[r] = 1/2 sum_e f[r, e]^2 for the R rows of f (R, HS): fp32 squares, fp64 sum in a fixed order, one wave per row
int launch_row_energy(const float* f, double* E, int R, int HS, hipStream_t s);
// the weights of the rows' energies in a trajectory's combined energy: the job's host scalars (comb_weights; n_rp <= 3) or, rw != nullptr,
// the lines of the device (B, n_rp) table of a composed job
struct EnergyWeights { float w[3] = {0.f, 0.f, 0.f}; const float* rw = nullptr; };
// E_comb[b] = sum_j w_j E_rows[b n_rp + j] (fp64, j ascending)
int launch_combine_energy(const double* E_rows, const EnergyWeights& w, double* E_comb, int B, int n_rp, hipStream_t s);
// x' = x - a eps + cz z on free waypoints, x' = x on the waypoints hc lists (only hc.idx / hc.n are read)
int launch_mcmc_propose(const float* x, const float* eps, const float* z, float a, float cz, HardConds hc, float* xp, int B, int H, int S,
                        hipStream_t s);
struct McmcAcceptArgs {
  float* x = nullptr; const float* xp = nullptr;       // (B,H,S) state (overwritten where accepted) and proposal
  float* eps = nullptr; const float* eps_p = nullptr;  // (B,H,S) cached combined gradient at x (overwritten where accepted) / at x'
  double* E = nullptr; const double* E_p = nullptr;    // (B) cached combined energy at x (overwritten where accepted) / at x'; MALA only
  const float* u = nullptr;                            // (B) uniforms in (0, 1); MALA only
  int* flag = nullptr;                                 // (B) 1 = accepted
  double* log_alpha = nullptr;                         // optional (B): MALA's log acceptance ratio
  HardConds hc;                                        // pinned waypoints (idx / n)
  int B = 0, H = 0, S = 0, mala = 0;
  float a = 0;                                         // eta / sigma_t, the proposal's own fp32 value
  double inv_sigma = 0, inv_4eta = 0;                  // 1 / sigma_t, 1 / (4 eta)
};
int launch_mcmc_accept(const McmcAcceptArgs& a, hipStream_t s);

struct ApfArgs {
  float* traj = nullptr;        // (B,H,S) modified in place (xy channels only)
  const float* cloud = nullptr; // (P,2)
  const float* window = nullptr;// (2*win+1) Gaussian weights
  int B = 0, H = 0, S = 0, P = 0, win = 0;
  double thr = 0, strength = 0;
  // one cloud per scene (a job of many scenes, ramp_sample_scenes): trajectory b avoids the points
  // [scene_off[scene[b]], scene_off[scene[b] + 1]) of `cloud`, the scenes' clouds concatenated; P is then unused
  const int* scene = nullptr;     // (B) scene of each trajectory, or null = one cloud of P points for all
  const int* scene_off = nullptr; // (n_scenes + 1) first point of each scene's cloud
  int n_scenes = 0;
};
int launch_apf(const ApfArgs& a, hipStream_t s);
// ---- cost-gradient guidance (guide.hip, device code shared with the two families below in guide_core.h; ramp_cost_guide in ramp_hip.h) ----
constexpr int GUIDE_TILE = 1024;    // points of a cloud tile in LDS; also the most points of a moving cloud
constexpr int GUIDE_MAX_H = 128;    // the longest horizon the guide kernels serve
struct GuideArgs {
  float* traj = nullptr;            // (B,H,S): channels [0, D) of the free waypoints are updated in place (the cost kernel only reads)
  int B = 0, H = 0, S = 0, D = 2;   // D = point_dim, 2 or 3, <= S; H <= GUIDE_MAX_H
  const float* cloud = nullptr;     // (P_total, D): the scenes' clouds, concatenated
  const int* cloud_off = nullptr;   // device (n_scenes + 1): first point of each scene's cloud (an empty span is allowed; spans are clamped to P_total)
  const int* scene = nullptr;       // (B) scene of each trajectory, or null = scene 0 for all; an index outside the table leaves the trajectory alone
  int n_scenes = 1, P_total = 0;
  float radius = 0, w_obs = 0, w_smooth = 0, w_acc = 0, max_norm = 0;
  float step = 0; int n_iter = 0;   // (the cost kernel reads neither, nor hc)
  HardConds hc;                     // pinned waypoints: their conditioned values enter the cost, their gradient is zero, their memory is not written
};
// n_iter guide iterations in ONE launch, one block per trajectory; n_iter == 0 launches nothing
int launch_guide_step(const GuideArgs& a, hipStream_t s);
// terms (B, 3) doubles = {C_obs, C_smooth, C_acc} unweighted (NaN for a trajectory whose scene index is outside the table)
int launch_guide_cost(const GuideArgs& a, double* terms, hipStream_t s);
// ---- swept box and sphere terms of the cost guide (guide_prims.hip + guide_core.h; ramp_prim_guide in ramp_hip.h) ---------------
// GuideArgs plus the scenes' boxes and spheres: C_prim over n_sub samples per segment, handed back to the segment's two waypoints.  The scene
// of a trajectory is g.scene's; the spans of both tables are clamped to their totals
struct PrimGuideArgs {
  GuideArgs g;
  const float* box_c = nullptr; const float* box_s = nullptr;   // (n_boxes, D) centres and full sides, scenes concatenated
  const float* sph_c = nullptr; const float* sph_r = nullptr;   // (n_spheres, D) centres, (n_spheres) radii
  const int* box_off = nullptr; const int* sph_off = nullptr;   // device (g.n_scenes + 1) each
  int n_boxes = 0, n_spheres = 0;                               // totals
  float margin = 0, band = 0, w_prim = 0;
  int n_sub = 1;                                                // 1 .. 8
};
// n_iter guide iterations in ONE launch, one block per trajectory; n_iter == 0 launches nothing.  Without a primitive in the trajectory's
// scene, or with w_prim == 0, a block's arithmetic is guide_step_kernel's
int launch_guide_prims_step(const PrimGuideArgs& a, hipStream_t s);
// terms (B, 4) doubles = {C_obs, C_smooth, C_acc, C_prim} unweighted (NaN for a trajectory whose scene index is outside the table)
int launch_guide_prims_cost(const PrimGuideArgs& a, double* terms, hipStream_t s);
// ---- teams of robots in one job: the separation term of the cost guide (guide_team.hip + guide_core.h; ramp_team_guide in ramp_hip.h) ----
// GuideArgs plus the team layout: row b is agent b % team of team b / team, a team's rows are adjacent; C_team couples the rows of a team at
// equal waypoint index.  One block owns a whole team (positions of all its agents in LDS), so nothing crosses a block
constexpr int TEAM_MAX = 8;         // the largest team (RAMP_TEAM_MAX)
struct TeamGuideArgs {
  GuideArgs g;
  int team = 1;                     // 1 .. TEAM_MAX, g.B % team == 0
  float radius_team = 0, w_team = 0;
};
// n_iter Jacobi iterations in ONE launch, one block per team; n_iter == 0 launches nothing.  team == 1 or w_team == 0 launches
// guide_step_kernel itself
int launch_guide_team_step(const TeamGuideArgs& a, hipStream_t s);
// terms (B, 4) doubles = {C_obs, C_smooth, C_acc, the row's share of C_team} unweighted (NaN for every row of a team with a scene index
// outside the table)
int launch_guide_team_cost(const TeamGuideArgs& a, double* terms, hipStream_t s);
// ---- stitched windows (stitch.hip; ramp_stitch in ramp_hip.h) ---------------------------------------
constexpr int STITCH_MAX_PINS = 64;
struct StitchArgs {
  float* x = nullptr;               // (C W, H, S) in place: row c W + w is window w of chain c
  int C = 0, W = 1, H = 0, S = 0;
  int O = 0;                        // overlap, 1 .. H / 2 (not read with W == 1); stride H - O
  const float* alpha = nullptr;     // device (O) blend weights in [0, 1]
  int n_pin = 0;                    // 0 .. STITCH_MAX_PINS
  const float* pin_val = nullptr;   // device (n_pin, C, S)
  int pin_idx[STITCH_MAX_PINS] = {};// long waypoint of each pin, in [0, H + (W - 1)(H - O)): a kernel argument, baked into a captured node
};
// blend and pins in ONE launch, no element written twice; nothing to do (W == 1 and no pin) launches nothing
int launch_stitch(const StitchArgs& a, hipStream_t s);
// out (C, L, S): every long waypoint from the window with the smallest w that covers it
int launch_stitch_assemble(const float* x, float* out, int C, int W, int H, int S, int O, hipStream_t s);
// ---- warm-started jobs (warm.hip; ramp_warm_start in ramp_hip.h) --------------------------------------
// x[b] = has_prior[b] ? (sa_row[b] * prior[b]) + (s1a_row[b] * noise0[b]) : noise0[b] (the same bits); every array (B, H, S) and 16-byte
// aligned, H S a multiple of 4, the three tables device (B).  x may be noise0 (in place); prior is not read for a row without one
int launch_warm_init(float* x, const float* noise0, const float* prior, const float* sa_row, const float* s1a_row, const int* has_prior,
                     int B, int H, int S, hipStream_t s);
// rows with j0[b] > j: x[b] = x_init[b] and, chain_block != nullptr, chain_block[b] = x_init[b]; the other rows are not touched
int launch_warm_hold(float* x, float* chain_block, const float* x_init, const int* j0, int j, int B, int H, int S, hipStream_t s);
struct ApfDynArgs {
  float* traj = nullptr;          // (B,H,S) in place (xy only)
  const double* points = nullptr; // (P,2) float64
  const float* goal = nullptr;    // (S) goal state for the pursuer pass, or null
  const int* enable = nullptr;    // (B) per-trajectory switch, or null = all
  int B = 0, H = 0, S = 0, P = 0;
  int window = -1;                // >= 0: static pass around the closest waypoint; < 0: waypoints [0, affected)
  int affected = 0;
  double thr_query = 0, thr_force = 0, strength = 0;
  // one cloud per episode (a job of many episodes, ramp_replan_episodes): trajectory b reads the points of episode episode[b] --
  // [ep_off[e], ep_off[e + 1]) of `points` (the episodes' clouds concatenated, P = their total, spans clamped to it), or, without
  // ep_off, the e-th block of P points -- and `goal` is row 0's goal state inside a (B,H,S) batch: row b blends towards its own
  const int* episode = nullptr;   // (B) episode of each trajectory, or null = one cloud of P points and one goal for all
  const int* ep_off = nullptr;    // (n_episodes + 1) first point of each episode's cloud, or null = P points each
  int n_episodes = 0;
};
int launch_apf_dynamic(const ApfDynArgs& a, hipStream_t s);
int launch_replan_goal(float* x0, const float* x, int B, int H, int S, hipStream_t s);
// receding-horizon replanning (sampler.hip) of a batch of episodes advancing in lock-step (ramp_replan_episodes; ramp_replan is one
// episode): what changes from replan to replan is resident on the device, one record per episode.  Row b belongs to episode row_ep[b]
// and reads that episode's record, history (E,H,S) and clean plan (E,H,S).  `active` = 0 marks an episode that has ended: its rows
// still run (from its last plan), its selection is skipped.
struct EpisodeState { int n_hist; int stepp; int active; int pad0; float pursuer[2]; float pad1[2]; };
struct EpisodeTable { const EpisodeState* st = nullptr; const int* row_ep = nullptr; int n_episodes = 0; };
int launch_replan_init_episodes(float* x, const float* x_clean, const float* noise, float sa, float s1a, const float* hist,
                                EpisodeTable ep, int B, int H, int S, hipStream_t s);
int launch_replan_pin_episodes(float* x, HardConds hc, const float* hist, const float* x_clean, EpisodeTable ep, int B, int H, int S,
                               hipStream_t s);
int launch_replan_sm_episodes(float* x, EpisodeTable ep, int window, float dt, float max_vel, int B, int H, int S, hipStream_t s);
int launch_replan_near_episodes(const float* x, EpisodeTable ep, float thr, int* en, int B, int H, int S, hipStream_t s);
// dst segment e = [seg_off[e], seg_off[e + 1]) (device table, E + 1 entries, seg_off[e] = first static cost point of episode e + e * n_extra):
// the episode's points of `cloud` (the episodes' static cost clouds, concatenated) followed by its n_extra points of `extra` (E, n_extra, 2).
// Writes stay inside the P_total points of dst; a wrong table copies wrong points
int launch_episode_cost_segments(float* dst, const float* cloud, const float* extra, const int* seg_off, int n_episodes, int n_extra,
                                 int P_total, hipStream_t s);
// one block per episode over its rows [traj_first[e], traj_first[e + 1]): the replan's selection (winner with x[0, 2:] = 0) into
// best (E,H,S) and result (E,4) = {n_free, rank, row in the whole batch, 0}; no free row: {0, -1, -1, 0}, inactive: {-1, -1, -1, 0},
// and in both cases the episode's `best` block stays as it is
int launch_select_episodes(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                           const int* traj_first, EpisodeTable ep, float* best, int* result, int B, int H, int S, hipStream_t s);
// ---- the cost guide of the replanning jobs (guide_replan.hip + guide_core.h; ramp_replan_guide in ramp_hip.h) -------------------
// The static term of GuideArgs (2-D) plus a moving cloud of n_mov <= GUIDE_TILE points per scene displaced by a per-waypoint track, and pins that
// differ from row to row: waypoints < n_first(b), waypoint H - 1 and the hard-conditioned ones.  n_first(b) = pin_first[b], or the n_hist of
// the row's episode record (est, with its `active` switch: a row of an ended episode is left alone).
// The working copy's pinned values: the hard condition's (later entries win), then -- only with hist / x_clean, the replans' buffers
// (n_scenes, H, S) -- the history rows and the clean plan's goal, replan_pin_row's order; a pinned waypoint nothing names keeps the array's own
struct MovingGuideArgs {
  float* traj = nullptr;            // (B,H,S): channels 0:2 of the free waypoints are updated in place (the cost kernel only reads)
  int B = 0, H = 0, S = 0;          // H <= GUIDE_MAX_H, S >= 2
  const float* cloud = nullptr;     // (P_total, 2): the scenes' static clouds, concatenated
  const int* cloud_off = nullptr;   // device (n_scenes + 1); an empty span is allowed, spans are clamped to P_total
  const float* mov = nullptr;       // device (n_scenes, n_mov, 2): every scene's moving cloud now
  const float* track = nullptr;     // device (n_scenes, H, 2): its displacement at waypoint h
  const int* scene = nullptr;       // (B) scene (episode) of each row, or null = 0 for all; an index outside the table leaves the row alone
  int n_scenes = 1, P_total = 0, n_mov = 0;
  const int* pin_first = nullptr; const EpisodeState* est = nullptr;   // where n_first(b) comes from (both null: 0)
  const float* hist = nullptr; const float* x_clean = nullptr;
  float radius = 0, radius_mov = 0, w_obs = 0, w_mov = 0, w_smooth = 0, w_acc = 0, max_norm = 0;
  float step = 0; int n_iter = 0;   // (the cost kernel reads neither, nor the pins)
  HardConds hc;
};
// n_iter iterations in ONE launch, one block per row; n_iter == 0 launches nothing
int launch_guide_step_moving(const MovingGuideArgs& a, hipStream_t s);
// terms (B, 4) doubles = {C_obs, C_mov, C_smooth, C_acc} unweighted of the rows as they are (NaN for a scene index outside the table)
int launch_guide_cost_moving(const MovingGuideArgs& a, double* terms, hipStream_t s);
// dst[0..n) = src[0..n) as a kernel node (the tap of a guided replan inside its captured graph)
int launch_copy_f32(float* dst, const float* src, long n, hipStream_t s);
int launch_replan_select(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                         float* best, int* result, int B, int H, int S, hipStream_t s);
// one block per scene of a many-scene batch (rows [traj_first[s], traj_first[s + 1])): result (n_scenes, 4) with the row in the whole
// batch, best (n_scenes, H, S) the winner unmodified; a scene without a free row gets {0, -1, -1, 0} and a NaN block
int launch_select_scenes(const float* traj, const int* mask, const float* plen, const float* smooth, float w_s, float w_l,
                         const int* traj_first, int n_scenes, float* best, int* result, int B, int H, int S, hipStream_t s);
// ---- K distinct plans per scene (sampler.hip; ramp_select_diverse_scenes in ramp_hip.h states the definition) --------------------------
constexpr int DIVERSE_MAX_K = 16;
struct DiverseArgs {
  const float* traj = nullptr;      // (B,H,S)
  int B = 0, H = 0, S = 0, D = 2;   // D = point_dim, 2 or 3, <= S; 1 <= H <= 128
  const int* traj_first = nullptr;  // device (n_scenes + 1), non-decreasing; spans are clamped to [0, B], an empty span is allowed
  int n_scenes = 1;
  const int* mask = nullptr; const float* plen = nullptr; const float* smooth = nullptr;   // (B) each; mask 1 = colliding
  float w_s = 0, w_l = 0;
  int K = 1; float min_sep = 0; int metric = 0;   // 1 <= K <= DIVERSE_MAX_K; metric 0 = mean, 1 = maximum waypoint distance
  float* best = nullptr;            // (n_scenes, K, H, S), NaN in the slots nothing fills
  int* rows = nullptr;              // (n_scenes, K) rows in the whole batch, -1 padded
  int* result = nullptr;            // (n_scenes, 4) = {n_free, n_selected, rows[s][0], 0}
  int* mode_of = nullptr; float* sep = nullptr;   // (B): every row's slot and its distance to that representative (-1 / NaN); the passes' working arrays
  int* mode_count = nullptr;        // (n_scenes, K)
  int* state = nullptr; float* tot = nullptr; int* pick = nullptr;   // scratch: (B) row states, (B) totals of the free rows, (n_scenes) the pass's pick
};
// 2 K + 1 launches: K x (pick per scene, update per row), then the counts; nothing is allocated, copied or read back
int launch_select_diverse(const DiverseArgs& a, hipStream_t s);
// mask[b] = any_{h,p} ||xy - p|| < thr ; plen[b], smooth[b]
int launch_traj_costs(const float* traj, const float* cloud, int B, int H, int S, int P, float thr,
                      int* mask, float* plen, float* smooth, hipStream_t s);
// the same with row b reading only the points [cloud_off[s], cloud_off[s + 1]) of its scene s (traj_first[s] <= b < traj_first[s + 1])
int launch_traj_costs_scenes(const float* traj, const float* cloud, const int* traj_first, const int* cloud_off, int n_scenes,
                             int P_total, int B, int H, int S, float thr, int* mask, float* plen, float* smooth, hipStream_t s);
int launch_traj_metrics(const float* traj, int B, int H, int S, const float* centers, const float* sizes, int n_boxes,
                        float* intensity, float* path_len, float* smooth, hipStream_t s);
// scratch: 2 * H * ceil(B / 256) doubles; out: 1 double
int launch_waypoint_variance(const float* traj, int B, int H, int S, double* scratch, double* out, hipStream_t s);
// denoising loss (diffusion_model_static.py:497-505, helpers.py:71-100): waypoints 0 and H - 1 of x_recon are overwritten with x_start's (in
// place), then out[0] = mean over all elements of (x_recon - target)^2 (l1 = 0) or |x_recon - target| (l1 = 1): fp32 terms, fp64 sums in a fixed
// order (two stages).  scratch: DENOISE_LOSS_BLOCKS doubles; out: 1 double
constexpr int DENOISE_LOSS_BLOCKS = 1024;
int launch_denoise_loss(float* x_recon, const float* x_start, const float* target, int B, int H, int S, int l1, double* scratch, double* out,
                        hipStream_t s);
// many-scene batch: row b tests the boxes [box_off[s], box_off[s + 1]) of its scene only
int launch_traj_metrics_scenes(const float* traj, int B, int H, int S, const int* traj_first, int n_scenes, const float* centers,
                               const float* sizes, const int* box_off, int n_boxes_total, float* intensity, float* path_len,
                               float* smooth, hipStream_t s);
// per-scene records of 6 doubles {n_traj, n_free, mean intensity, mean and unbiased std of the free path lengths, waypoint variance
// of the free rows} and the (B) free mask.  scratch: 2 * H * W + n_scenes + 1 doubles, W = ceil(B / 256) + n_scenes.  D = 2 or 3: the
// position coordinates the pairwise waypoint distance is taken over
int launch_scene_summary(const float* traj, int B, int H, int S, const int* traj_first, int n_scenes, const float* intensity,
                         const float* path_len, float thr, double* scratch, double* summary, int* free_mask, hipStream_t s, int D = 2);
}  // namespace ramp
