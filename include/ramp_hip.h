/* ramp_hip.h — C ABI of the MI355X-native RAMP trajectory sampler (libramp_hip.so, gfx950).
 *
 * The reference (wondmgezahu/RAMP) has no FFI: its boundary for this path is two Python
 * nn.Module surfaces.  Each entry point below names the reference call it
 * replaces; the Python shim in ramp_amd/ binds them with ctypes and re-creates the reference's
 * own signatures on top (INTEGRATION.md shows the stub a RAMP maintainer would add).
 *
 * Conventions: every function returns 0 on success, a negative code on failure with a message
 * available from ramp_last_error().  All tensor pointers are DEVICE pointers to contiguous fp32
 * (or int32 where noted) owned by the caller (e.g. torch tensors' data_ptr()) unless a parameter
 * is documented as host memory.  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  A context is bound to the HIP device current at creation; it is thread-compatible,
 * not thread-safe.  Layouts: trajectories (B, H, S) row-major exactly as the reference's
 * `x : [batch x horizon x state_dim]` (UnetInference.py:177-181); network rows are interleaved
 * per trajectory [variant 0, variant 1, (variant 2)] like `repeat_interleave`
 * (diffusion_model_static.py:131-147).
 */
#ifndef RAMP_HIP_H
#define RAMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ramp_ctx ramp_ctx;

/* most network rows one trajectory may have: ramp_score / ramp_score_rows accept n_rp up to it, ramp_sample_composed composes up to
 * RAMP_MAX_ROWS_PER_TRAJ - 1 obstacle sets (the last row is the unconditional one) */
#define RAMP_MAX_ROWS_PER_TRAJ 8

/* Architecture of TemporalUnetInference.__init__ (UnetInference.py:42-56, 93-145). */
typedef struct ramp_config {
  int32_t state_dim;       /* S: 4 (Maze2D) or 6 (Maze3D)                              */
  int32_t horizon;         /* H = n_support_points: any multiple of 8 in [8, 64]       */
  int32_t unet_input_dim;  /* C0: 16, 32 or 64 (channels C0 * dim_mults[k])           */
  int32_t n_levels;        /* len(dim_mults): 3 for UNET_DIM_MULTS[0] = (1,2,4),        *
                            * 4 for UNET_DIM_MULTS[1] = (1,2,4,8)                       */
  int32_t context_dim;     /* 320 (2-D scene encoder) or 256 (3-D)                     */
  int32_t max_rows;        /* capacity in network rows per chunk (rows = B * n_rp)     */
  int32_t debug_taps;      /* 1: keep per-module outputs / output-grads for ramp_debug_read */
  int32_t gemm_mode;       /* 0 = library default (env RAMP_GEMM_MODE=fp32|bf16x6|fp16x3), 1 = exact fp32 MFMA, 2 = bf16x6 split,
                            * 3 = fp16x3 split with delayed operand scaling (ramp_sample calibrates on its first evaluation
                            *     unless it continues from the previous job, see ramp_set_calibration_reuse;
                            *     ramp_score keeps its calibration from call to call; see ramp_score) */
} ramp_config;

const char* ramp_last_error(void);
int ramp_version(void);

/* Launch plan: which kernels serve the feed-forward pairs and the shared CFG prefix.  Pure performance knobs -- every plan
 * meets the same parity bar (tests/test_gpu_unet.py, test_gpu_sampler.py run all of them against the reference fixtures).
 * ramp_create fills the plan with the library defaults; the environment variables RAMP_FF_FUSED, RAMP_FFX, RAMP_SHARE_PREFIX,
 * RAMP_X6_THREE, RAMP_X6_PIPE, read ONCE there, override those defaults; nothing below ramp_create reads the environment.
 * ramp_set_launch_plan may be called any time; after ramp_finalize_weights `x6_pipe` can no longer change (the weight
 * packing depends on it) and a change of the other fields drops the captured graphs and the kept fp16x3 calibration. */
typedef struct ramp_launch_plan {
  int32_t ff_fused_rows;  /* FF1 -> GEGLU -> FF2 forward as one launch (gemm.hip, ff_fwd_kernel) from this many tokens: 0 never, 1 always */
  int32_t ffx_rows;       /* token-owning fused feed-forward, forward AND backward with LayerNorm-3 folded in (ffx.hip), from
                           * this many tokens (takes precedence over ff_fused_rows): 0 never, 1 always */
  int32_t share_prefix;   /* sampling jobs: the CFG rows of a trajectory share the network prefix (0 / 1) */
  int32_t three_blocks;   /* a third resident block for the bias-only linears where it measured faster (0 / 1) */
  int32_t x6_pipe;        /* fragment-packed weights + pipelined split-precision kernels (1) or LDS-staged weights (0) */
  int32_t tkl_rows;       /* K = 256 transformer linears (LayerNorm-1 -> QKV with the norm folded in, attention out-projection, its
                           * input gradient) on the token-owning kernel (tkl.hip) from this many tokens: 0 never, 1 always */
  int32_t atk_rows;       /* self-attention + output projection (+ bias, cross-attention constant, residual) as ONE launch of
                           * sample-owning waves (atk.hip) from this many tokens, on levels whose token count divides 48 or 32:
                           * 0 never, 1 always */
  int32_t tkc_rows;       /* the k = 5 convolutions with C_in, C_out in {32, 64} (the two finest levels' residual blocks, the final block) and
                           * their input gradients on sample-owning waves (tkc.hip) from this many tokens, on levels whose token count
                           * (>= 8) divides 48 or 32: 0 never, 1 always */
  int32_t tkw_rows;       /* the k = 5 convolutions with C_out in {128, 256, 512} (the residual blocks of the coarse levels) with their
                           * GroupNorm + Mish fused -- forward: behind the convolution; input gradient: GroupNorm backward folded into the
                           * operand -- on sample-owning blocks (tkw.hip) from this many tokens, on levels whose token count (>= 3)
                           * divides 96: 0 never, 1 always */
  int32_t mfma16;         /* the token-owning kernels -- the fused feed-forward and the K = 256 attention linears -- issue v_mfma_f32_16x16x32_f16
                           * (ffx16.hip / tkl16.hip, 1: the default) or v_mfma_f32_32x32x16_f16 (ffx.hip / tkl.hip, 0): same products and call sites, another summation tiling; the 16-wide
                           * shape holds a higher clock under the socket power cap (profiles/r06_mfma_shape_probe.txt).  Default from
                           * RAMP_MFMA16, read once in ramp_create */
} ramp_launch_plan;
int ramp_get_launch_plan(ramp_ctx* ctx, ramp_launch_plan* out);
int ramp_set_launch_plan(ramp_ctx* ctx, const ramp_launch_plan* plan);

/* nn.Module construction / .to(device)  (inference_static.py:99-105). */
int ramp_create(const ramp_config* cfg, ramp_ctx** out);
int ramp_destroy(ramp_ctx* ctx);

/* load_state_dict (inference_static.py:107-111): one call per U-Net tensor, `name` is the
 * reference key without the leading "model." (e.g. "downs.0.0.blocks.0.block.0.weight").
 * `data` is HOST memory, fp32, `shape[ndim]` as in the checkpoint.  scene_encoder.* float tensors (weights and
 * BatchNorm running statistics) are loaded the same way for ramp_encode_scene. */
int ramp_load_weight(ramp_ctx* ctx, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* after the last ramp_load_weight: verifies every required tensor arrived, packs GEMM layouts. */
int ramp_finalize_weights(ramp_ctx* ctx);

/* time_mlp + every cond_mlp for t = 0..T-1 (layers.py:233-259, 340-344): the reference evaluates
 * these inside each forward; t is identical across the batch (make_timesteps,
 * diffusion_model_static.py:16-18) so they are tabulated once. */
int ramp_prepare_time_table(ramp_ctx* ctx, int32_t T, void* stream);
/* the TimeEncoder output itself for timestep t (SinusoidalPosEmb(32) -> Linear 32->128 -> Mish -> Linear 128->32,
 * layers.py:233-259) as the table holds it: out32 device, 32 floats.  Parity tests compare it with the reference's. */
int ramp_time_embedding(ramp_ctx* ctx, int32_t t, float* out32, void* stream);

/* cache_scene_encoding + latent masking + attn2 (UnetInference.py:146-156,190-197;
 * layers_attention_mini.py:101-127): `latents` (n_variants, context_dim); an unconditional
 * variant is an all-zero row.  Row r of the network uses variant row_variant[r] (int32, HOST
 * array of length n_rows_pattern, applied cyclically: [0,1] = CFG, [0,1,2] = compose). */
int ramp_set_scene(ramp_ctx* ctx, const float* latents, int32_t n_variants,
                   const int32_t* row_variant_host, int32_t n_rows_pattern, void* stream);

/* Many scenes in one job: the loop over experiment directories of scripts/inference/inference_static.py (one cache_scene_encoding +
 * run_inference per experiment, :113-190) as ONE batch whose rows carry their own scene.  `latents` device (n_variants, context_dim),
 * 1 <= n_variants <= 65536 (N scene rows plus the shared all-zero unconditional row); row r of the network uses variant
 * row_variant_host[r] (int32, HOST array, an EXPLICIT table of n_rows = B * n_rp entries, not a pattern).  Computes the
 * cross-attention constants like ramp_set_scene and drops the captured graphs and every kept calibration like it; a later
 * ramp_set_scene returns the context to pattern mode.  While the explicit table is in place ramp_score / ramp_sample refuse a
 * batch with more rows than n_rows.  The launch plan is the single-scene job's: from 5 variants on, the fused kernels read the row
 * constant from global memory instead of LDS (atk.hip, tkl.hip, tkl16.hip). */
int ramp_set_scenes(ramp_ctx* ctx, const float* latents, int32_t n_variants, const int32_t* row_variant_host, int32_t n_rows,
                    void* stream);

/* scene_encoder(obstacle_pts) for ONE scene: ObstacleEncoderSet.forward (obstacle_encoder.py:125-152, point_dim 2,
 * latent 320) or ObstacleEncoder.forward in eval mode (obstacle_encoder3d.py:77-94, point_dim 3, latent 256).
 * cloud: device (n_obstacles, n_points, point_dim); latent_out: device (context_dim), 16-byte aligned. */
int ramp_encode_scene(ramp_ctx* ctx, const float* cloud, int32_t n_obstacles, int32_t n_points, int32_t point_dim,
                      float* latent_out, void* stream);

/* scene_encoder for MANY scenes in one call, with a launch count per pass that does not depend on the number of scenes: the
 * per-scene loop that run_inference_scenes / run_inference_episodes would otherwise make over ramp_encode_scene.
 * points: device (sum P, point_dim), the scenes' clouds concatenated.  Two HOST int32 CSR tables (copied before the call returns):
 * scene_first_host[n_scenes + 1], the first obstacle of each scene, and obstacle_first_host[n_obstacles + 1], the first point of each
 * obstacle.  Scenes may differ in obstacle count and in points per obstacle; inside one scene every obstacle has the same point
 * count (the reference's (No, Np, D) tensor).  latents_out: device (n_scenes, context_dim), 16-byte aligned; row i holds, BIT FOR
 * BIT, what ramp_encode_scene writes for scene i alone, whatever else is in the batch and whatever the budget.
 * Scenes are encoded in passes of consecutive scenes: a pass holds as many whole scenes as fit in max_points points (0 = the default
 * below) and always at least one, so a scene larger than the budget gets a pass of its own; the scratch buffer is sized to the
 * largest pass (the 2-D encoder keeps 960 floats per point: about 126 MB at the default).  n_passes_out (host, may be NULL)
 * receives the number of passes.  Everything is checked on the host before the first launch; refused (non-zero, the entry's name in
 * ramp_last_error): n_scenes < 1, tables that do not start at 0 or are not strictly increasing (an empty scene or obstacle), a
 * scene whose obstacles differ in point count, a point_dim other than the model's, totals beyond 32-bit offsets. */
#define RAMP_ENCODE_DEFAULT_MAX_POINTS 32768
int ramp_encode_scenes(ramp_ctx* ctx, const float* points, const int32_t* obstacle_first_host, const int32_t* scene_first_host,
                       int32_t n_scenes, int32_t point_dim, int32_t max_points, float* latents_out, int32_t* n_passes_out,
                       void* stream);

/* TemporalUnetInference.forward / forward_no_energy (UnetInference.py:157-224).
 * x (B,H,S); each trajectory is evaluated n_rp times (rows b*n_rp + v, 1 <= n_rp <= RAMP_MAX_ROWS_PER_TRAJ).  f_out (B*n_rp,H,S)
 * receives forward_no_energy's output, eps_out (B*n_rp,H,S) the energy gradient; either may be
 * NULL.  t is the diffusion timestep of EVERY row, 0 <= t < T of the prepared table (what the samplers pass: make_timesteps'
 * batch-uniform vector); one timestep per row is ramp_score_rows below.
 * fp16x3 mode: the first call after ramp_create / ramp_set_scene / ramp_sample / ramp_set_fallback runs the bf16x6
 * kernels and records every GEMM call site's operand maximum; later calls run the fp16x3 kernels scaled from their
 * predecessor's maxima.  If the range guard fires the evaluation is repeated at once with the bf16x6 kernels (one
 * 4-byte read-back per call decides), so a flagged result is never returned. */
int ramp_score(ramp_ctx* ctx, const float* x, int32_t B, int32_t n_rp, int32_t t,
               float* f_out, float* eps_out, void* stream);
/* ramp_score with one diffusion timestep per network row (UnetInference.py:198 embeds `time` per row; the reference's own
 * loss / p_losses draws t = randint(0, T, (B,)), diffusion_model_static.py:478-511).  t_rows_host: HOST int32 array of B * n_rp
 * entries, entry r the timestep of row r (the row_variant_host convention); every entry is checked against the prepared table
 * (0 <= t < T) before anything is launched, then the table is copied to a device buffer of the context (sliced per chunk when
 * B * n_rp exceeds max_rows).  The time-conditioning arithmetic is the same precomputed table; only the row -> table-line choice is
 * per row, so a row's result has the bits ramp_score gives it at that row's t.  Arithmetic modes, the fp16x3 calibration kept from
 * call to call (shared with ramp_score), the range guard and its bf16x6 repeat, debug taps and ramp_set_scenes tables: ramp_score's.
 * The samplers (ramp_sample*, ramp_replan) keep the uniform path. */
int ramp_score_rows(ramp_ctx* ctx, const float* x, int32_t B, int32_t n_rp, const int32_t* t_rows_host,
                    float* f_out, float* eps_out, void* stream);
/* ramp_score plus the energies of the evaluation: the score is an energy gradient, eps = grad_x 1/2 ||f(x, t, scene)||^2 (EnergyGradFunction
 * returns that energy as its second value, UnetInference.py:26-32), and energy_out[r] = 1/2 sum_{h,s} f[r,h,s]^2 for every network row r --
 * device double (B * n_rp).  fp32 squares, fp64 sum in a fixed order (one wave per row: lane l takes elements l, l + 64, ..., then a fixed
 * butterfly), so an energy has the same bits from run to run and however max_rows chunks the batch.  f_out and eps_out (either may be
 * NULL) have the bits ramp_score gives them; everything else -- arithmetic modes, kept calibration, range guard and its repeat -- is
 * ramp_score's. */
int ramp_score_energy(ramp_ctx* ctx, const float* x, int32_t B, int32_t n_rp, int32_t t, float* f_out, float* eps_out,
                      double* energy_out, void* stream);
/* arithmetic the last ramp_score / ramp_score_rows call's result was computed in: 0 exact fp32, 1 bf16x6, 2 fp16x3 */
int ramp_score_mode(ramp_ctx* ctx, int32_t* mode);

/* ---- sampler loops: run_inference -> conditional_sample -> p_sample_loop / ddim_p_sample_loop
 *      (diffusion_model_static.py:232-256, 347-384, 438-463; diffusion_model_3d.py:185-218) ---- */
typedef struct ramp_apf_params {
  const float* cloud;      /* device (P,2) obstacle points, or NULL = APF off             */
  int32_t n_points;
  int32_t window;          /* avoidance_window                                            */
  const float* window_weights_host; /* host (2*window+1) Gaussian weights (APFhelper.py:42-44) */
  double threshold;        /* distance_threshold                                          */
  double strength;         /* avoidance_strength                                          */
  int32_t passes;          /* DDIM: 3 sequential passes with hard-conditioning; DDPM: 1   */
  int32_t reserved;
} ramp_apf_params;

typedef struct ramp_sample_params {
  int32_t B;               /* trajectories                                                */
  int32_t n_rp;            /* 2 = CFG, 3 = compose; ramp_sample_composed: 2 .. 8          */
  int32_t n_steps;         /* loop iterations                                             */
  int32_t ddim;            /* 0 = DDPM (ddpm_sample_fn), 1 = DDIM eta=0                   */
  double w0, w1;           /* guidance weights (w for CFG; w1,w2 for compose)             */
  /* per-iteration HOST arrays of length n_steps (computed by the caller exactly like the
   * reference's registered buffers / extract(): see ramp_amd/diffusion.py) */
  const int32_t* t;              /* timestep fed to the network                          */
  const float* sqrt_recip;       /* sqrt_recip_alphas_cumprod[t]                          */
  const float* sqrt_recipm1;     /* sqrt_recipm1_alphas_cumprod[t]                        */
  const float* coef1;            /* posterior_mean_coef1[t]         (DDPM)                */
  const float* coef2;            /* posterior_mean_coef2[t]         (DDPM)                */
  const float* stdv;             /* exp(0.5*posterior_log_variance_clipped[t]) (DDPM)     */
  const int32_t* use_noise;      /* 0 where t == 0                  (DDPM)                */
  const float* sqrt_a_t;         /* alphas_cumprod[t]**0.5          (DDIM)                */
  const float* sqrt_1m_a_t;      /* (1-alphas_cumprod[t])**0.5      (DDIM)                */
  const float* sqrt_a_prev;      /* alpha_prod_t_prev**0.5          (DDIM)                */
  const float* dir_coef;         /* (1-alpha_prod_t_prev)**0.5      (DDIM)                */
  const int32_t* apply_apf;      /* 1 on iterations where the APF hook fires              */
  const float* noise_scale;      /* noise_std_extra_schedule_fn(t) per iteration (scripts: 0.5); NULL = 1.0 */
  int32_t clip_denoised;
  int32_t predict_x0;            /* predict_epsilon=False (the reference constructor's default, diffusion_model_static.py:28, 109-118):
                                  * 1 = the guidance-combined network output IS x0 (then clamped); 0 = it is epsilon */
  /* hard conditioning (sample_functions.py:5-10) */
  int32_t n_hard;                /* number of conditioned waypoints                       */
  const int32_t* hard_idx_host;  /* host (n_hard) waypoint indices                        */
  const float* hard_val;         /* device (n_hard, B, S)                                 */
  ramp_apf_params apf;
  int32_t use_graph;             /* 1: capture the whole loop in a hipGraph and replay it */
  int32_t reserved;
  /* noise_mode 0: the caller injects the noise (the `noise` argument; the parity runs and every torch.randn-compatible
   * caller).  noise_mode 1: the job draws its own N(0, I) INSIDE the captured graph -- counter-based Philox4x32-10 +
   * Box-Muller (ramp_philox_normal below), element i of the job's (n_steps+1, B, H, S) noise block = element i of the
   * stream (philox_seed, philox_offset); `noise` may be NULL.  Seed and offset sit in a device record the graph reads,
   * so every replay draws fresh numbers without re-capturing. */
  int32_t noise_mode;
  int32_t reserved2;
  uint64_t philox_seed;
  uint64_t philox_offset;        /* in groups of four elements */
  /* noise_mode 1 in a job that is ONE SHARD of a larger one (the sample batch split over GPUs): this call's B
   * trajectories are samples [philox_sample0, philox_sample0 + B) of a job of philox_total trajectories whose noise block is
   * (n_steps+1, philox_total, H, S) -- every shard draws exactly the elements the unsharded job draws for its samples, so
   * N shards reproduce the 1-GPU job of the same total.  philox_total == 0 means "this call is the whole job" (= B, 0). */
  int64_t philox_sample0;
  int64_t philox_total;
} ramp_sample_params;

/* noise: device (n_steps+1, B, H, S) for DDPM — noise[0] = x_T, noise[1+j] the randn_like of
 * iteration j; for DDIM only noise[0] is read (NULL with noise_mode 1).  chain_out: device (n_steps+1, B, H, S) or NULL.
 * x_out: device (B,H,S) final trajectories or NULL. */
int ramp_sample(ramp_ctx* ctx, const ramp_sample_params* p, const float* noise, float* chain_out,
                float* x_out, void* stream);
/* ramp_sample over trajectories of SEVERAL scenes (the experiment loop of scripts/inference/inference_static.py:113-190 as one
 * job; the row -> latent table comes from ramp_set_scenes): trajectory b avoids the cloud of scene traj_scene[b] in the APF hook
 * (APFhelper.py:37-104 with that experiment's ObstacleField).  p->apf.cloud must be NULL and p->apf.n_points is ignored; window,
 * weights, threshold, strength and passes keep their meaning.  cloud_points == NULL = APF off.  Graph capture, Philox noise, range
 * guard, fallback modes and calibration reuse are ramp_sample's. */
typedef struct ramp_scene_batch {
  int32_t n_scenes;
  int32_t reserved;
  const int32_t* traj_scene;          /* device (B) int32: scene of each trajectory, 0 <= . < n_scenes               */
  const float* cloud_points;          /* device (sum P, 2): the scenes' obstacle points, concatenated; NULL = APF off */
  const int32_t* cloud_offset_host;   /* host (n_scenes + 1): first point of each scene, [0] = 0, strictly increasing */
} ramp_scene_batch;
int ramp_sample_scenes(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_scene_batch* scenes, const float* noise,
                       float* chain_out, float* x_out, void* stream);
/* Composition over ANY number of obstacle sets, many scenes per job: p_mean_variance_compose samples with
 * e = u + sum_k w_k (c_k - u) over obstacle sets (diffusion_model_static.py:188-229, diffusion_model_3d.py:163-182; the 3-D file carries the
 * three-set form as commented-out code, "for 2 compose (more than two obstacle sets)", :165-174).  Here a trajectory's rows and their weights
 * are data: n_rp = (most sets of any scene) + 1 rows per trajectory, row b * n_rp + j reads the latent the ramp_set_scenes table gives it
 * and its gradient enters e_comb[b] = sum_j row_weight[b][j] eps[b * n_rp + j] (j ascending) -- set k of the scene with w_k, the
 * unconditional row with 1 - sum_k w_k, a padding row (a scene with fewer sets) with 0.  p->w0 and p->w1 are ignored.  The table is
 * copied into a buffer of the context before the launch and the captured graph reads that buffer: the graph is keyed on n_rp and
 * "composed", not on the weights, so a second job of the same shape with other weights replays the same graph and gets its own
 * weights.  `scenes` gives every trajectory its own APF cloud exactly as in ramp_sample_scenes (NULL = no APF clouds).  Graph capture,
 * Philox noise, the range guard, the fp16x3 repeat and calibration reuse are ramp_sample's.  Refused on the host before any launch
 * (non-zero, the entry's name in ramp_last_error): g == NULL, row_weight == NULL, n_rp outside 2 .. RAMP_MAX_ROWS_PER_TRAJ,
 * n_rp != p->n_rp, no ramp_set_scenes table in place, a table shorter than B * n_rp rows. */
typedef struct ramp_guidance_rows {
  int32_t n_rp;               /* rows per trajectory, 2 .. RAMP_MAX_ROWS_PER_TRAJ; must equal p->n_rp */
  int32_t reserved;
  const float* row_weight;    /* device (B, n_rp): weight of each row's gradient in e_comb */
} ramp_guidance_rows;
int ramp_sample_composed(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_guidance_rows* g, const ramp_scene_batch* scenes,
                         const float* noise, float* chain_out, float* x_out, void* stream);
/* ---- Langevin refinement inside the sampling job (ULA / MALA) ----
 * Composed reverse diffusion with summed scores is biased; a few MCMC steps per noise level, Metropolis-corrected where the model exposes
 * an energy, remove the bias (Du et al., "Reduce, Reuse, Recycle", ICML 2023).  With sigma_t = sqrt(1 - alphas_cumprod[t]), step size eta,
 * a = eta / sigma_t, c = sqrt(2 eta), eps the guidance-combined gradient and E the guidance-combined energy (sum_j w_j E_row_j with the
 * weights that form eps, fp64), iteration j of the job evaluates eps(x, t_j) (and E, MALA) as ever, then runs n_inner[j] inner steps:
 *   propose   x' = x - a eps(x) + c z on free waypoints, x' = x on the waypoints the hard conditions pin           (fp32)
 *   evaluate  eps' = eps(x', t_j), E' = E(x', t_j): ONE evaluation, a link of the job's calibration chain like any other
 *   accept    ULA: always.  MALA: log alpha = -(E' - E) / sigma_t - (||x - x' + a eps'||^2 - ||x' - x + a eps||^2) / (4 eta), fp64 over the
 *             free elements, a the proposal's own fp32 value; accepted when log u < log alpha and E', log alpha are finite.  An accepted
 *             trajectory's x, cached eps and cached E become the proposal's.
 * The reverse step (guidance step, APF hook, DDPM / DDIM update, hard conditioning) then uses the CACHED eps of the state the inner steps
 * ended on: a job runs n_steps + sum n_inner evaluations.  ULA requests no energies.  The range guard logs every evaluation (ramp_range_trip
 * counts inner ones too) and a flagged job is repeated as ever.
 *
 * kind: 0 off (the call IS ramp_sample / ramp_sample_scenes / ramp_sample_composed, bit for bit), 1 ULA, 2 MALA.  n_inner, step_size, sigma:
 * HOST arrays of n_steps entries; sigma[j] = sqrt_one_minus_alphas_cumprod[t[j]] (ramp_sample_params carries no such table for the DDPM loop,
 * and the library never derives schedule values itself: the caller hands them over like every other per-iteration array).  g (NULL = p's CFG / compose scalars) and scenes (NULL = one
 * scene) as in ramp_sample_composed / ramp_sample_scenes.
 * noise_mode 0: mcmc_noise device (sum n_inner, B, H, S) normals and mcmc_u device (sum n_inner, B) uniforms in (0, 1), inner steps in job
 * order; ULA ignores mcmc_u.  noise_mode 1: both come from the job's Philox stream (seed, offset), BEHIND the main block: with K = sum
 * n_inner, T = philox_total (or B), g = sample0 + b the global sample and blocks of T * H * S elements,
 *   main block      blocks 0 .. n_steps (DDIM draws block 0 only, as ever)
 *   normal of (inner step k, sample g, element e)   = element ((n_steps + 1 + k) T + g) H S + e of the stream
 *   uniform of (inner step k, sample g)             = ((r >> 9) + 0.5) 2^-23, r = output 0 of group (n_steps + 1 + K) T H S / 4 + k T + g
 * (groups of four elements, counted from philox_offset), so a shard draws what the whole job draws for its samples.
 * accept_out: device int32 (sum n_inner, B), 1 = accepted, or NULL.  The captured graph is keyed on the job's shape, kind, n_inner and the
 * step sizes (kernel arguments): a job with other step sizes is captured anew, never replayed from a stale graph; composed weights stay data.
 * Refused on the host before any launch (non-zero, "ramp_sample_mcmc" in ramp_last_error): kind outside 0 .. 2; with kind != 0,
 * p->predict_x0 != 0 (the combined output is then no score: no density to correct), n_inner outside 0 .. RAMP_MCMC_MAX_INNER, a non-positive or
 * non-finite step_size / sigma where n_inner > 0, NULL mcmc_noise / mcmc_u where noise_mode 0 needs them; g->n_rp != p->n_rp and the other
 * guidance-table checks of ramp_sample_composed. */
#define RAMP_MCMC_MAX_INNER 16
typedef struct ramp_mcmc_params {
  int32_t kind;               /* 0 off, 1 ULA, 2 MALA                                        */
  int32_t reserved;
  const int32_t* n_inner;     /* host (n_steps): inner steps after iteration j's evaluation  */
  const float* step_size;     /* host (n_steps): eta, > 0 wherever n_inner > 0               */
  const float* sigma;         /* host (n_steps): sqrt(1 - alphas_cumprod[t[j]])              */
} ramp_mcmc_params;
int ramp_sample_mcmc(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_mcmc_params* m, const ramp_guidance_rows* g,
                     const ramp_scene_batch* scenes, const float* noise, const float* mcmc_noise, const float* mcmc_u,
                     float* chain_out, float* x_out, int32_t* accept_out, void* stream);
/* ---- cost-gradient guidance steps inside the sampling job, 2-D and 3-D ----
 * The reference samplers accept guide / n_guide_steps / t_start_guide and ignore them (guide_gradient_steps is a stub that returns x,
 * sample_functionsdynamic.py:280-292); this is what those names mean in cost-guided trajectory diffusion: a few gradient steps on a
 * differentiable trajectory cost inside the reverse step.  For one trajectory x (H, S), d = point_dim, p_h = x[h, 0:d] and its scene's cloud
 * c (P, d):
 *   C_obs    = sum_h sum_j 1/2 max(0, r - |p_h - c_j|)^2          every cloud point inside radius r (C1, no argmin)
 *   C_smooth = sum_{h=0}^{H-2} 1/2 |p_{h+1} - p_h|^2
 *   C_acc    = sum_{h=1}^{H-2} 1/2 |p_{h+1} - 2 p_h + p_{h-1}|^2
 *   C        = w_obs C_obs + w_smooth C_smooth + w_acc C_acc
 * A pair at distance 0 contributes no gradient; an empty cloud makes C_obs = 0.  One guide iteration: (1) the waypoints the job's hard
 * conditions pin take their conditioned values in the working copy, (2) g = dC/dp, (3) g = 0 on the pinned waypoints, (4) n = |g|_2 over the
 * trajectory, (5) s = min(1, max_norm / n), s = 1 if max_norm <= 0 or n = 0, (6) p <- p - (step s) g on the free waypoints.  Pinned
 * waypoints and the channels >= d of the array in memory keep their bits.  All arithmetic is fp32 (the five scalars are rounded to fp32
 * once), every product and sum rounded as written; |g|^2 is summed in fp64.  The fp32 sums over points run in an order fixed by (P, the
 * kernel's tile of 1024 points): same inputs, same bits, whatever the batch.  H <= 128.
 * Place in the reverse step of iteration j with n_guide[j] > 0: after the guidance-combined posterior mean (DDPM) resp. x0 (DDIM) and after
 * the APF hook where that fires, before the noise / DDIM update and its hard conditioning; ONE launch runs the n_guide[j] iterations for all
 * trajectories and scenes.  With inner MCMC steps the guide belongs to the reverse step, not to the inner steps.  It draws no random
 * numbers: the Philox layout of a job, and what a shard needs, are unchanged.
 * The clouds are the guide's own table (scenes->cloud_points stays the 2-D APF table and may be NULL): points and offsets are copied into
 * buffers of the context before the launch and the captured graph reads those, so other cloud CONTENTS of the same sizes replay the same
 * graph and are honoured.  n_guide, step and the five scalars are kernel arguments and part of the graph key: a job with other values is
 * captured anew. */
#define RAMP_GUIDE_MAX_STEPS 16
typedef struct ramp_cost_guide {
  int32_t point_dim;                 /* 2 or 3, <= state_dim */
  int32_t n_scenes;                  /* clouds in the table; 1 for a single-scene job */
  const float* cloud_points;         /* device (sum P, point_dim), scenes concatenated */
  const int32_t* cloud_offset_host;  /* host (n_scenes + 1), [0] = 0, non-decreasing (an empty cloud is allowed) */
  double radius, w_obs, w_smooth, w_acc, max_norm;
  const int32_t* n_guide;            /* host (n_steps): guide iterations on loop iteration j, 0 .. RAMP_GUIDE_MAX_STEPS */
  const float* step;                 /* host (n_steps): step size on iteration j (the caller folds any schedule factor in) */
} ramp_cost_guide;
/* ramp_sample_mcmc plus the guide: one entry for plain, many-scene, composed and MCMC jobs (m == NULL = no inner steps).  cg == NULL, or
 * n_guide zero on every iteration, IS ramp_sample_mcmc, bit for bit.  On DDPM the guide acts on the posterior mean, on DDIM on x0.
 * scenes->traj_scene maps trajectories to cg's clouds: cg->n_scenes must equal scenes->n_scenes, or be 1 with scenes == NULL.
 * Refused on the host before any launch (non-zero, "ramp_sample_guided" in ramp_last_error): point_dim outside {2, 3} or > state_dim,
 * n_guide[j] outside 0 .. RAMP_GUIDE_MAX_STEPS, non-finite scalars or step, radius <= 0 with w_obs != 0, offsets that are not
 * non-decreasing from 0, a scene-count mismatch, cloud_points == NULL with a non-empty table, H > 128; and what ramp_sample_mcmc refuses.
 * ramp_replan / ramp_replan_episodes take a guide of their own, with a moving-cloud term and per-episode pins: ramp_replan_guide below. */
int ramp_sample_guided(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_mcmc_params* m,
                       const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise, const float* mcmc_noise,
                       const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream);
/* the kernel alone on (B, H, S) trajectories in place, the counterpart of ramp_apf / ramp_apf_scenes: n_iter (0 .. RAMP_GUIDE_MAX_STEPS)
 * iterations with step size `step` in one launch; cg->n_guide and cg->step are not read.  traj_scene device int32 (B) or NULL = scene 0;
 * a trajectory whose scene index is outside [0, n_scenes) is left unchanged.  hard_idx_host host (n_hard) waypoint indices (later entries
 * win), hard_val device (n_hard, B, S) as in ramp_sample_params.  Refusals as above, with "ramp_guide_step".  Synchronises `stream`. */
int ramp_guide_step(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const int32_t* traj_scene, int32_t n_iter,
                    float step, int32_t n_hard, const int32_t* hard_idx_host, const float* hard_val, void* stream);
/* the three unweighted terms per trajectory, terms_out device (B, 3) doubles = {C_obs, C_smooth, C_acc}: fp64 sums over fp32 pair values in
 * a fixed order, for ranking and diagnostics (no hard conditions: the trajectory as it is; NaN for a scene index outside the table).
 * Synchronises `stream`. */
int ramp_guide_cost(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const int32_t* traj_scene,
                    double* terms_out, void* stream);
/* ---- swept box and sphere terms in the cost guide, 2-D and 3-D ----
 * ramp_traj_clearance counts waypoints AND the segments between them against the boxes and spheres of a trajectory's scene, widened by a
 * robot margin; ramp_cost_guide's obstacle term sees waypoints and cloud points only.  This term lets the guide push on what is counted
 * afterwards: a signed-distance hinge on the scene's primitives at n_sub samples per segment, its gradient handed back to the segment's two
 * waypoints (the collision cost on interpolated points of motion-planning diffusion; the reference's configs carry
 * factor_num_interpolated_points_for_collision for it and its code never reads it).
 * For one trajectory x (H, S): D = point_dim in {2, 3}, p_h = x[h, 0:D], n = n_sub in 1 .. 8.
 *   Samples   u_{h,m} = p_h + t_m (p_{h+1} - p_h), t_m = m / n, for h < H - 1 and m = 0 .. n - 1, and u_{H-1,0} = p_{H-1}; m = 0 is the
 *             waypoint itself, bit for bit.  (H - 1) n + 1 samples, at most 1017.
 *   Box k     (centre c, full sides s, margin >= 0): half_d = s_d / 2 + margin, q_d = |x_d - c_d| - half_d.  If any q_d > 0:
 *             phi = sqrt(sum_d max(q_d, 0)^2), grad phi_d = sign(x_d - c_d) max(q_d, 0) / phi.  Otherwise phi = max_d q_d and
 *             grad phi = sign(x_k - c_k) e_k for the lowest index k that attains the maximum, sign(0) = +1.  phi <= 0 is
 *             ramp_traj_clearance's "inside the widened box".
 *   Sphere k  (centre c, radius r): phi = |x - c| - (r + margin), grad phi = (x - c) / |x - c|; a sample at the centre contributes cost and
 *             no gradient.
 *   Cost      C_prim = sum over samples u and primitives k with phi_k(u) < band of 1/2 (band - phi_k(u))^2, band >= 0 (band = 0 penalises
 *             penetration only).  The gradient at a sample: g_u = - sum_k (band - phi_k) grad phi_k, boxes then spheres, in table order.
 *   Hand-back for h < H - 1: g_prim[h] = sum_{m=0}^{n-1} (1 - t_m) g_{u_{h,m}}; for h = H - 1: g_prim[h] = g_{u_{H-1,0}}; then, for h >= 1,
 *             + sum_{m=1}^{n-1} t_m g_{u_{h-1,m}}, in this order.
 *   Total     C = w_obs C_obs + w_prim C_prim + w_smooth C_smooth + w_acc C_acc.  One iteration is ramp_cost_guide's six steps with
 *             g = w_obs g_obs + (w_prim g_prim + (w_smooth g_s + w_acc g_a)).
 * All fp32 (margin, band and w_prim rounded to fp32 once), every product and sum rounded as written, the square roots and quotients
 * correctly rounded; |g|^2 in fp64.  The result for a trajectory does not depend on the rest of the batch.  A trajectory whose scene has no
 * primitive, and any trajectory with w_prim == 0, gets ramp_cost_guide's arithmetic, bit for bit.
 * The struct travels WITH a ramp_cost_guide, which keeps supplying the cloud term (possibly an empty table with w_obs = 0), w_smooth, w_acc,
 * max_norm, n_guide[] and step[].  The four arrays and the two offset tables are copied into buffers of the context before the launch and the
 * captured graph reads those: other centres, sizes or radii with the same counts replay the same graph and are honoured.  n_scenes, the two
 * totals, n_sub, margin, band and w_prim are part of the graph key. */
#define RAMP_PRIM_GUIDE_MAX_SUB 8
typedef struct ramp_prim_guide {
  int32_t point_dim;                 /* 2 or 3, <= state_dim, the cost guide's                                    */
  int32_t n_scenes;                  /* the cost guide's                                                          */
  const float* box_centers;          /* device (sum n_boxes, point_dim), scenes concatenated                      */
  const float* box_sizes;            /* device (sum n_boxes, point_dim), full sides                               */
  const float* sphere_centers;       /* device (sum n_spheres, point_dim)                                         */
  const float* sphere_radii;         /* device (sum n_spheres)                                                    */
  const int32_t* box_offset_host;    /* host (n_scenes + 1), [0] = 0, non-decreasing (a scene may have no box)    */
  const int32_t* sphere_offset_host; /* host (n_scenes + 1), [0] = 0, non-decreasing (a scene may have no sphere) */
  double margin, band, w_prim;       /* margin >= 0, band >= 0, all finite                                        */
  int32_t n_sub;                     /* samples per segment, 1 .. RAMP_PRIM_GUIDE_MAX_SUB                         */
  int32_t reserved;
} ramp_prim_guide;
/* ramp_sample_guided plus the primitive term: plain, many-scene, composed and MCMC jobs.  pg == NULL, w_prim == 0 or no primitive in any
 * scene IS ramp_sample_guided, bit for bit.  The bf16x6 repeat of a flagged job runs the same guide.  ramp_sample_steered and
 * ramp_sample_stitched keep their signatures and take no primitives.
 * Refused on the host before any launch (non-zero, "ramp_sample_guided_prims" in ramp_last_error): pg without cg; point_dim outside {2, 3}
 * or > state_dim or different from cg's; n_sub outside 1 .. 8; H > 128; a negative or non-finite margin or band; a non-finite w_prim; offsets
 * that are missing or not non-decreasing from 0; a total > 0 with a NULL array; pg->n_scenes different from cg's or the scene batch's; and
 * what ramp_sample_guided refuses. */
int ramp_sample_guided_prims(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                             const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                             const float* mcmc_noise, const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream);
/* the kernel alone, the counterpart of ramp_guide_step: its arguments plus pg (NULL = ramp_guide_step).  Refusals as above, with
 * "ramp_guide_step_prims".  Synchronises `stream`. */
int ramp_guide_step_prims(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                          const int32_t* traj_scene, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                          const float* hard_val, void* stream);
/* terms_out device (B, 4) doubles = {C_obs, C_smooth, C_acc, C_prim} unweighted of the trajectories as they are: columns 0 .. 2 are
 * ramp_guide_cost's bits, column 3 sums the fp32 values 1/2 (band - phi)^2 in fp64 in a fixed order (0 with pg == NULL; NaN for a scene
 * index outside the table).  Refusals as above, with "ramp_guide_cost_prims".  Synchronises `stream`. */
int ramp_guide_cost_prims(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_prim_guide* pg,
                          const int32_t* traj_scene, double* terms_out, void* stream);
/* ---- teams of robots in one job: separation guide, swept check, selection ----
 * Every row of a sampling job is one robot alone in its scene.  Several robots that share a scene are sampled in one batch with the
 * single-robot model and coupled only through a separation cost inside the guide (how multi-robot diffusion planners compose single-robot
 * models); the joint plan is then checked for conflicts and the best conflict-free team is picked.
 * Layout.  A job of B rows with team size A: 1 <= A <= RAMP_TEAM_MAX, B % A == 0, row b is agent b % A of team b / A; a team's rows are
 * adjacent and belong to one scene.  D = point_dim, p_{a,h} = x[row a, h, 0:D]; the same h means the same time for every agent.
 *   Team term  C_team = sum_{a<a'} sum_h 1/2 max(0, r_t - |p_{a,h} - p_{a',h}|)^2, r_t = radius_team > 0.
 *              g_team[a][h] = dC_team/dp_{a,h} with exactly the arithmetic of the cloud term, the teammate's waypoint in the place of a cloud
 *              point: fp32 dx, d2 in coordinate order, the filter d2 < (r_t r_t) 1.00001f in front of the cloud term's square root, the
 *              test d < r_t && d > 0, f = (r_t - d) / d correctly rounded, sum_c -= f dx_c; teammates in ascending a', skipping a, added
 *              serially in fp32.  A pair at distance 0 contributes cost and no gradient.
 *   Iteration  Jacobi: every agent's gradient is taken from the positions all agents had at the start of the iteration, then all agents
 *              move.  Per agent the step is ramp_cost_guide's six steps with g = w_obs g_obs + (w_team g_team + (w_smooth g_s + w_acc g_a));
 *              the norm, the clip and the step are taken per agent trajectory, not per team.  A pinned waypoint holds its conditioned value
 *              and pushes on its teammates; it receives no gradient and its memory is not written.  Channels >= D keep their bits.  Each
 *              agent's cloud term reads the cloud of that row's own scene.  A team in which any row's scene index lies outside the table is
 *              left unchanged as a whole.
 * With team_size == 1, w_team == 0 or tg == NULL the result is ramp_guide_step / ramp_sample_guided, bit for bit (the same kernel is
 * launched).  A team's result does not depend on the rest of the batch.  team_size, radius_team and w_team are kernel arguments and part of
 * the graph key; the team term draws no random numbers, the Philox layout is unchanged (a shard must hold whole teams: philox_sample0 % A
 * == 0). */
#define RAMP_TEAM_MAX 8
typedef struct ramp_team_guide {
  int32_t team_size;                 /* A, 1 .. RAMP_TEAM_MAX, a divisor of B */
  int32_t reserved;
  double radius_team, w_team;        /* r_t > 0 and finite where w_team != 0; w_team finite */
} ramp_team_guide;
/* ramp_sample_guided with the team term: plain, many-scene, composed and MCMC jobs; the guide belongs to the reverse step as there.
 * Refused on the host before any launch (non-zero, "ramp_sample_guided_team" in ramp_last_error): tg without cg; team_size outside
 * 1 .. RAMP_TEAM_MAX; B % team_size != 0; radius_team <= 0 or non-finite with w_team != 0; a non-finite w_team; H > 128; a sharded job with
 * philox_sample0 % team_size != 0; and what ramp_sample_guided refuses.  ramp_sample_guided_prims, ramp_sample_steered and
 * ramp_sample_stitched keep their signatures and take no team. */
int ramp_sample_guided_team(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                            const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                            const float* mcmc_noise, const float* mcmc_u, float* chain_out, float* x_out, int32_t* accept_out, void* stream);
/* the kernel alone, the counterpart of ramp_guide_step: its arguments plus tg (NULL = ramp_guide_step).  Refusals as above, with
 * "ramp_guide_step_team".  Synchronises `stream`. */
int ramp_guide_step_team(float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                         const int32_t* traj_scene, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                         const float* hard_val, void* stream);
/* terms_out device (B, 4) doubles: columns 0 .. 2 are ramp_guide_cost's bits; column 3 of a row is sum_{a' != a} sum_h 1/2 (r_t - d)^2,
 * fp32 values (d = the correctly rounded root) summed in fp64 in a fixed order (per waypoint over a' ascending, then over the waypoints in
 * the order of the other columns' reduction), 0 with tg == NULL.  A team's C_team is half the sum of its rows' column 3.  Every row of a team with a scene index outside
 * the table gets NaN.  Refusals as above, with "ramp_guide_cost_team".  Synchronises `stream`. */
int ramp_guide_cost_team(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_cost_guide* cg, const ramp_team_guide* tg,
                         const int32_t* traj_scene, double* terms_out, void* stream);
/* The joint check of teams, synchronous swept, closed form.  For a pair a < a' and h < H - 1: D0 = p_{a,h} - p_{a',h},
 * D1 = p_{a,h+1} - p_{a',h+1}, e = D1 - D0, t = clamp(-(D0 . e) / |e|^2, 0, 1) with t = 0 when |e|^2 == 0, d_seg = |D0 + t e| min-ed with
 * |D0| and |D1| (so sep_seg <= sep_wp always, the rule of ramp_traj_clearance).  Per team: sep_wp = min over pairs and waypoints of |D_h|,
 * sep_seg = min over pairs and segments of d_seg, wp_conflicts = #(pair, h) with |D_h| < min_sep, seg_conflicts = #(pair, segment) with
 * d_seg < min_sep (both strict).  All fp32, rounded as written.  A team with a non-finite position coordinate gets NaN separations, all
 * counts at their maximum and is never free; team_size == 1 gives +inf separations and zero counts.
 * The reduction for the selection, in the same launch, from the optional per-row arrays of ramp_traj_clearance, ramp_traj_costs_scenes or
 * ramp_traj_metrics_scenes: team_mask = 1 if any member's row_mask is non-zero or the conflict count `swept` chooses (1: seg_conflicts,
 * 0: wp_conflicts) is non-zero; team_len / team_smooth = the members' values added serially in fp32 in agent order (0 without the array).
 * Selection is then ramp_select_scored_scenes on the team-level arrays with the trajectories viewed as (B / A, A H, S) and
 * team_first = traj_first / A.
 * All arrays on the device: the inputs (B) or NULL, the outputs (B / team_size), any of them NULL.  Asynchronous on `stream`, capturable,
 * one launch.  Refused on the host before any launch ("ramp_team_clearance" in ramp_last_error): NULL traj, B <= 0, H outside 2 .. 128,
 * point_dim outside {2, 3} or > S, team_size outside 1 .. RAMP_TEAM_MAX, B % team_size != 0, a negative or NaN min_sep. */
int ramp_team_clearance(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, int32_t team_size, float min_sep,
                        int32_t swept, const int32_t* row_mask, const float* row_len, const float* row_smooth, float* sep_wp,
                        float* sep_seg, int32_t* wp_conflicts, int32_t* seg_conflicts, int32_t* team_mask, float* team_len,
                        float* team_smooth, void* stream);
/* ---- resampling trajectories by cost inside the sampling job (SMC steering) ----
 * A job draws B candidates per scene and ranks them when it has finished; sequential Monte Carlo steering (Feynman-Kac steering, twisted SMC
 * for diffusion) weights every candidate at chosen noise levels by a potential on the job's current clean estimate and resamples within the
 * scene, so that the remaining evaluations go to candidates that are still promising.
 * Groups: the B trajectories are partitioned into n_groups contiguous groups by the host table group_first_host (n_groups + 1): [0] = 0,
 * strictly increasing, [n_groups] = B.  A plain job has one group of B, a many-scene or composed job one group per scene.  Resampling never
 * crosses a group.  Per trajectory the job keeps logw and c_prev (fp64, both 0 at the start of the job).
 * Event: on iteration j with resample[j] != 0,
 *   1. c_b = w_obs C_obs + w_smooth C_smooth + w_acc C_acc, the three terms exactly what ramp_guide_cost returns on the array the cost guide
 *      works on (the posterior mean on DDPM, x0 on DDIM) as it stands after the APF hook and the guide, no hard conditions applied, before
 *      the noise / DDIM update; the products and the two sums in fp64, left to right.  Clouds and scalars come from rs->cost (a ramp_cost_guide
 *      of the event's own, whose n_guide, step and max_norm are not read; it may be the job's guide table).
 *   2. logw_b += -lambda[j] (c_b - c_prev_b), then c_prev_b = c_b: the difference potential -- with constant lambda the product of an
 *      unresampled lineage telescopes to exp(-lambda c).  A non-finite logw_b counts as -inf (weight 0).
 *   3. after the iteration's update and hard conditioning, per group of size n: W_i = exp(logw_i - max logw) / sum, ESS = 1 / sum W_i^2.
 *      Every weight 0: ESS = 0, identity, nothing changes.
 *   4. ESS < ess_frac n (ess_frac in [0, 2]: 0 never, above 1 always): systematic resampling with ONE uniform u per (event, group).  cum =
 *      the inclusive fp64 prefix sums of W with cum_{n-1} taken as 1; a_i = min(n - 1, #{k : cum_k <= (i + u) / n}); then x[i] <- x[a_i] for
 *      the whole (H, S) row, c_prev[i] <- c[a_i], logw <- 0 in that group.  Otherwise the ancestors are the identity and x, logw stay.
 *   5. with chain_out, block j + 1 is the state after the event.
 * The order of the fp64 sums (max, sum, prefix sums, ESS) is the implementation's; nothing else is free.
 * Outputs per event k (events in job order), any of them NULL: ancestor_out device int32 (n_events, B), indices within the batch; ess_out
 * device double (n_events, n_groups); cost_out device double (n_events, B), the c_b of that event; logw_out device double (B) at the end of
 * the job.
 * Randomness.  noise_mode 0: resample_u is a device (n_events, n_groups) float array in (0, 1).  noise_mode 1: u comes from the job's Philox
 * stream behind everything a job draws today; in the notation of ramp_sample_mcmc above, with G = groups_total (0 means n_groups) and
 * g = group0 + the local group index,
 *   uniform of (event k, global group g) = ((r >> 9) + 0.5) 2^-23, r = output 0 of group (n_steps + 1 + K) T H S / 4 + K T + k G + g
 * (the K T groups of MALA's uniforms are reserved whether or not the job is MALA).  A repeat of a flagged job replays the same uniforms.
 * Group boundaries and u are data in buffers of the context that the captured graph reads: other boundaries with equal n_groups replay the same
 * graph and are honoured.  n_groups, the resample[] flags, lambda[], ess_frac and the potential's scalars are part of the graph key. */
#define RAMP_RESAMPLE_MAX_EVENTS 64
typedef struct ramp_resample_params {
  int32_t n_groups;
  int32_t group0;                     /* Philox: global index of this call's first group (0 for a whole job)       */
  int32_t groups_total;               /* Philox: groups of the whole job; 0 = n_groups                              */
  int32_t reserved;
  const int32_t* group_first_host;    /* host (n_groups + 1): [0] = 0, strictly increasing, [n_groups] = B          */
  const int32_t* resample;            /* host (n_steps): != 0 = an event on iteration j; at most 64 events          */
  const double* lambda;               /* host (n_steps): the potential's inverse temperature on iteration j         */
  double ess_frac;                    /* in [0, 2]                                                                  */
  const ramp_cost_guide* cost;        /* clouds and scalars of the cost; n_guide, step and max_norm are not read    */
} ramp_resample_params;
/* ramp_sample_guided plus the resampling events: the one entry for plain, many-scene, composed, MCMC and guided jobs.  rs == NULL, or no
 * flag set, IS ramp_sample_guided, bit for bit.  rs->cost->n_scenes must equal scenes->n_scenes, or be 1 with scenes == NULL.
 * Refused on the host before any launch (non-zero, "ramp_sample_steered" in ramp_last_error): a malformed group table; ess_frac outside
 * [0, 2] or non-finite; a missing or non-finite lambda; more than RAMP_RESAMPLE_MAX_EVENTS events; p->ddim != 0 without MCMC inner steps
 * (m->kind != 0 and sum n_inner > 0: eta = 0 DDIM never separates duplicates); p->predict_x0 != 0; what the cost table's own checks refuse
 * (see ramp_sample_guided), H > 128; group0 / groups_total that do not hold the call's groups; NULL resample_u in noise_mode 0; and what
 * ramp_sample_guided refuses.  ramp_replan / ramp_replan_episodes take no resampling (their guide is ramp_replan_guide). */
int ramp_sample_steered(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_resample_params* rs, const ramp_cost_guide* cg,
                        const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                        const float* mcmc_noise, const float* mcmc_u, const float* resample_u, float* chain_out, float* x_out,
                        int32_t* accept_out, int32_t* ancestor_out, double* ess_out, double* cost_out, double* logw_out, void* stream);
/* steps 3 and 4 alone on (B, H, S) trajectories in place (H S a multiple of 4): logw device double (B), c_prev device double (B) or NULL, u
 * device float (n_groups), ancestor_out device int32 (B) or NULL, ess_out device double (n_groups) or NULL.  Refused with
 * "ramp_resample_groups": a malformed group table, ess_frac outside [0, 2] or non-finite, null x / logw / u, H S no multiple of 4.
 * Synchronises `stream`. */
int ramp_resample_groups(float* x, int32_t B, int32_t H, int32_t S, double* logw, double* c_prev, const int32_t* group_first_host,
                         int32_t n_groups, const float* u, double ess_frac, int32_t* ancestor_out, double* ess_out, void* stream);
/* ---- plans longer than the network's horizon: stitched windows in one job ----
 * The score network serves whole samples of H <= 64 waypoints.  A long trajectory of L waypoints is sampled as W overlapping windows of H
 * waypoints that sit in adjacent rows of one batch and are made to agree, after every reverse step, on the waypoints they share
 * (MultiDiffusion / DiffStitch-style fusion of overlapping diffusion windows, here on trajectories).
 * Layout: W >= 1 windows per chain, overlap O with 1 <= O <= H / 2, stride st = H - O, L = H + (W - 1) st.  A job of C chains has B = C W
 * rows; row c W + w is window w of chain c and covers the long waypoints [w st, w st + H).  O <= H / 2: a long waypoint lies in at most two
 * windows.  With W == 1 the overlap is not read and L = H.
 * Stitch of an array a (B, H, S):
 *   blend  for w < W - 1, k < O, channel s: l = a[c W + w, st + k, s], q = a[c W + w + 1, k, s], m = l + alpha_k (q - l) in fp32, the
 *          difference, the product and the sum rounded once each; both locations receive m.  q == l returns l itself (bit for bit; for
 *          zeros of either sign, l's).  alpha: O floats in [0, 1].
 *   pins   pin i = 0 .. n_pin - 1 names a long waypoint idx_i in [0, L) and values val[i, c, :]: every window w with 0 <= idx_i - w st < H
 *          gets a[c W + w, idx_i - w st, :] = val[i, c, :].  Later pins win; pins win over the blend.
 * One launch; no element is written twice; nothing else of the array is touched.  Assemble: long[c, l, :] comes from the window with the
 * smallest w that covers l (after a stitch the other window holds the same bits).
 * The job: wherever the plain job applies its hard conditions, the stitched job runs the stitch, and it runs it on the array the hooks work on:
 *   noise  every noise block of the job (0 .. n_steps on DDPM, block 0 on DDIM) is stitched in the context's own buffer with alpha = 0 and
 *          no pins, behind the Philox draw (noise_mode 1) resp. the copy-in (noise_mode 0): an overlapping waypoint receives ONE draw, the
 *          left window's -- an average of two would shrink the variance there.  The caller's array is never written.
 *   start  x_T = noise[0], then stitch: chain block 0.
 *   iteration j: evaluation and guidance combination as ever; stitch of the posterior mean (DDPM) / x0 (DDIM); APF hook and cost guide as
 *          ever, per window, each window against the cloud of its own scene (on DDIM the stitch takes the place of the hard conditioning
 *          between APF passes); if either hook ran, one more stitch; the DDPM / DDIM update without hard conditions, then stitch of x: chain
 *          block j + 1.  (That last blend is the identity: equal inputs went through one elementwise expression; only the pins act.)
 * The job carries no hard conditions of its own: the cost guide therefore pins nothing, sees the pinned values in its target and may move
 * them; the stitch behind it restores them.
 * alpha and the pin values are copied into buffers of the context before the launch and the captured graph reads those: other values of the
 * same shape replay the same graph and are honoured.  n_windows, overlap, n_pin and the pin indices are part of the graph key. */
#define RAMP_STITCH_MAX_PINS 64
typedef struct ramp_stitch {
  int32_t n_windows;                 /* W >= 1; p->B must be a multiple of it                                      */
  int32_t overlap;                   /* O, 1 .. H / 2 (not read with W == 1)                                        */
  const float* alpha_host;           /* host (O) blend weights in [0, 1]; may be NULL with W == 1                    */
  int32_t n_pin;                     /* 0 .. RAMP_STITCH_MAX_PINS                                                    */
  int32_t reserved;
  const int32_t* pin_idx_host;       /* host (n_pin): long waypoint of each pin, in [0, L)                           */
  const float* pin_val;              /* device (n_pin, C, S), C = B / W                                              */
} ramp_stitch;
/* ramp_sample_guided (without MCMC and composed weights) on stitched windows.  st == NULL IS ramp_sample_guided(p, cg, NULL, NULL, scenes,
 * ...), bit for bit.  long_out: device (C, L, S), the assembled final trajectories, or NULL; chain_out / x_out hold the windows.
 * Refused on the host before any launch (non-zero, "ramp_sample_stitched" in ramp_last_error): n_windows < 1; B no multiple of n_windows;
 * overlap outside 1 .. H / 2 with n_windows > 1; an alpha outside [0, 1] or non-finite; n_pin outside 0 .. RAMP_STITCH_MAX_PINS; a pin index
 * outside [0, L); a NULL table where one is needed; p->n_hard != 0 (the pins are the job's conditions); a sharded job (p->philox_total != 0:
 * the windows of a chain must sit in one shard); and what ramp_sample_guided refuses. */
int ramp_sample_stitched(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_stitch* st, const ramp_cost_guide* cg,
                         const ramp_scene_batch* scenes, const float* noise, float* chain_out, float* x_out, float* long_out, void* stream);
/* the operation alone on x (C W, H, S) in place, the counterpart of ramp_guide_step.  Refusals as above, with "ramp_stitch_windows".
 * Synchronises `stream`. */
int ramp_stitch_windows(float* x, int32_t C, int32_t W, int32_t H, int32_t S, const ramp_stitch* st, void* stream);
/* long_out device (C, L, S) from the windows x (C W, H, S); O is not read with W == 1.  Refused with "ramp_stitch_assemble": bad dims, O
 * outside 1 .. H / 2 with W > 1, a NULL array.  Synchronises `stream`. */
int ramp_stitch_assemble(const float* x, int32_t C, int32_t W, int32_t H, int32_t S, int32_t O, float* long_out, void* stream);
/* ---- warm-started jobs: every row starts from a given plan at a level of its own ----
 * A sampling job starts at x_T = noise[0] and pays for the whole schedule.  A warm-started job starts every row from a prior plan noised to
 * an intermediate level (q_sample, as the reference's dynamic planner does at diffusion_model_dynamic.py:256/285/561) and runs only the tail
 * of the schedule.  The level is a per-row quantity: in one batch some rows have a prior and some do not.  ramp_amd/warm.py states the
 * definition in numpy (warm_tables, warm_init_reference, warm_hold_reference); in short, for a job whose params p hold the iterations
 * J .. n - 1 of the model's schedule (p->n_steps = n' = n - J; the caller truncates every per-iteration table of p and of the options):
 *   start  row b without a prior: x_init[b] = noise[0][b], the same bits.  With one: x_init[b] = (sa[b] * prior[b]) + (s1a[b] * noise[0][b])
 *          in fp32, two products and a sum rounded once each; sa / s1a are sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod at the
 *          timestep of the row's first own iteration, p->t[j0[b]].  Then the hard conditioning (the stitch of a stitched job), as on x_T:
 *          chain block 0, kept as x_init.
 *   hold   after iteration j (reverse step, hooks, hard conditioning or stitch, chain write) every row with j0[b] > j is x_init[b] again, in
 *          the state and in chain block j + 1: one launch on each iteration j < n_hold = max_b j0[b], none in a job of uniform levels.  The
 *          network still evaluates a held row (wasted on it, harmless); no hook result, inner step or accept survives on it.
 * The noise block is (n' + 1, B, H, S) on DDPM, (1, B, H, S) on DDIM, block 0 the start draw; with noise_mode 1 the job draws it as ever.
 * prior, the tables and the coefficients are copied into buffers of the context before the launch and the captured graph reads those: the
 * graph key gains the presence of a warm start and n_hold only, so two jobs that differ in levels at equal n_hold (and equal p) replay one
 * graph.  The launch count depends on n_hold alone, never on B or the number of scenes. */
typedef struct ramp_warm_start {
  const float* prior;                /* device (B, H, S): the rows' plans, normalised; a row without a prior is not read (NULL if no row has one) */
  const int32_t* j0_host;            /* host (B): the row's first own iteration, 0 .. n_hold; 0 for a row without a prior      */
  const int32_t* has_prior_host;     /* host (B): 0 = the row starts from noise[0], anything else = from its prior              */
  const float* sa_host;              /* host (B): sqrt_alphas_cumprod at the row's start timestep (not read without a prior)    */
  const float* s1a_host;             /* host (B): sqrt_one_minus_alphas_cumprod there                                            */
  int32_t n_hold;                    /* max_b j0_host[b], 0 .. p->n_steps - 1                                                    */
  int32_t reserved;
} ramp_warm_start;
/* THE entry of the sampling jobs with a warm start: behind ws every option struct a job knows, each of which may be NULL -- st (stitched
 * windows), rs (resampling events), cg / pg / tg (the cost guide, its primitives, its team), m (Langevin steps), g (composed weights),
 * scenes -- with the inputs and outputs of the entries that take them (ramp_sample_steered, ramp_sample_stitched).  ws == NULL IS the entry
 * that takes the same options, bit for bit, and launches what it launches.
 * Refused on the host before any launch (non-zero, "ramp_sample_warm" in ramp_last_error): a NULL table; j0 outside 0 .. n_hold; n_hold not
 * max j0 or >= p->n_steps; j0 != 0 on a row without a prior; a NULL prior or coefficient table, or a non-finite coefficient, with a prior
 * somewhere; H S no multiple of 4; with n_hold > 0 (mixed levels): resampling events (a held row could become an ancestor), a team, stitched
 * windows; pg and tg together; st together with rs / pg / tg / m / g; and what the entry of the same options refuses. */
int ramp_sample_warm(ramp_ctx* ctx, const ramp_sample_params* p, const ramp_warm_start* ws, const ramp_stitch* st,
                     const ramp_resample_params* rs, const ramp_cost_guide* cg, const ramp_prim_guide* pg, const ramp_team_guide* tg,
                     const ramp_mcmc_params* m, const ramp_guidance_rows* g, const ramp_scene_batch* scenes, const float* noise,
                     const float* mcmc_noise, const float* mcmc_u, const float* resample_u, float* chain_out, float* x_out,
                     int32_t* accept_out, int32_t* ancestor_out, double* ess_out, double* cost_out, double* logw_out, float* long_out,
                     void* stream);
/* the start state alone: x (B, H, S) device, may be noise0 itself; noise0 and prior device (B, H, S), 16-byte aligned; the three tables host
 * (B).  Neither the hard conditioning nor the stitch is applied.  Refused with "ramp_warm_init": a NULL argument, bad dims, H S no multiple
 * of 4.  Synchronises `stream`. */
int ramp_warm_init(float* x, const float* noise0, const float* prior, const float* sa_host, const float* s1a_host,
                   const int32_t* has_prior_host, int32_t B, int32_t H, int32_t S, void* stream);
/* the hold behind iteration j alone: rows with j0_host[b] > j become x_init[b] in x and, chain_block != NULL, in chain_block; nothing else is
 * written.  Refused with "ramp_warm_hold" likewise.  Synchronises `stream`. */
int ramp_warm_hold(float* x, float* chain_block, const float* x_init, const int32_t* j0_host, int32_t j, int32_t B, int32_t H, int32_t S,
                   void* stream);
/* torch.randn stand-in of the throughput jobs (sample_functions.py:36; diffusion_model_static.py:239): out[0..n) ~ N(0, 1),
 * element 4 g + j = output j of philox4x32_10(counter = (lo32(g + offset), hi32(g + offset), 0, 0), key = (lo32(seed),
 * hi32(seed))) through Box-Muller: u = ((r >> 9) + 0.5) 2^-23, (z0, z1) = sqrt(-2 ln u0) (cos, sin)(2 pi u1), (z2, z3) from
 * (u2, u3).  Host-replicable from (seed, offset); `out` device, 16-byte aligned. */
int ramp_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* ---- receding-horizon replanning: DynamicGaussianDiffusionModel.ddim_p_sample_loop, STAGE II
 *      (diffusion_model_dynamic.py:533-612) ----
 * One call = one replan iteration, run as ONE captured hipGraph: q_sample of the current best plan for all B candidates
 * (:671-680), the executed history / goal / zero start velocity pinned (:540-546, :563-568), n_steps DDIM steps of the
 * score network with CFG (:338-447), on the last one (t == 0) the velocity smoothing `sm` (:192-214, :551-553) and the
 * per-trajectory static + pursuer APF (:375-435, APFhelper_dynamic.py:107-142), the final smoothing (:570-571), the
 * collision mask / path length / smoothness against the cost cloud and the min-max-normalised argmin
 * (cost.py:25-88, :572-590) with `x[0, 2:] = 0` on the winner (:607).  What differs between two replans -- executed
 * history, current waypoint, noise, the pursuer's cloud and position -- is copied into fixed device buffers first, so the
 * graph is captured once (twice in fp16x3 mode: the first replan after a scene change calibrates the delayed operand
 * scales on its first evaluation, later ones continue from their predecessor's maxima).  The single device-to-host
 * transfer of a replan is the 16-byte result record.  The environment callback of the reference (the pursuer's dynamics,
 * fed x[:, stepp, :2], which is the pinned executed state and therefore known beforehand) runs in the caller BEFORE this
 * call; the "no collision-free candidate" restart (:591-605) is left to the caller too (result.n_free == 0). */
typedef struct ramp_replan_params {
  int32_t B;               /* candidate trajectories                                       */
  int32_t n_rp;            /* 2 (CFG)                                                      */
  int32_t n_steps;         /* DDIM steps of one replan (ddim_num_inference_steps_low = 5)  */
  int32_t clip_denoised;
  double w;                /* CFG weight (2.5)                                             */
  /* per-step HOST arrays of length n_steps, as in ramp_sample_params */
  const int32_t* t;
  const float* sqrt_recip; const float* sqrt_recipm1;
  const float* sqrt_a_t; const float* sqrt_1m_a_t; const float* sqrt_a_prev; const float* dir_coef;
  float q_sqrt_a, q_sqrt_1m_a;     /* q_sample at t[0]: sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod */
  int32_t n_hard; int32_t predict_x0;   /* predict_x0: as in ramp_sample_params */
  const int32_t* hard_idx_host;    /* host (n_hard)                                        */
  const float* hard_val;           /* device (n_hard, B, S)                                */
  int32_t sm_window_last;          /* 3: smoothing before the last DDIM step               */
  int32_t sm_window_final;         /* 2: smoothing before the selection                    */
  float sm_dt, sm_max_vel;         /* 0.1, 0.8                                             */
  const double* static_pts;        /* device (n_static, 2) float64: APF cloud of the static boxes */
  int32_t n_static;
  int32_t n_dyn;                   /* points of the pursuer's sphere cloud                 */
  double thr_static, thr_pred, strength_static, strength_pred;   /* 0.2, 0.5, 0.15, 0.15    */
  int32_t window_static;           /* 8                                                    */
  int32_t n_cost;                  /* points of the static cost cloud                      */
  const float* cost_cloud;         /* device (n_cost, 2)                                   */
  int32_t n_extra;                 /* pursuer points appended to the cost cloud when it is near (64); 0 = never */
  float cost_thr;                  /* collision threshold of the selection (0.05)          */
  float w_smooth, w_len;           /* 0.1, 0.9                                             */
  int32_t use_graph;
} ramp_replan_params;

typedef struct ramp_replan_state {
  const float* noise;              /* device (B, H, S): the randn_like of q_sample         */
  const float* x_clean;            /* device (H, S) current best plan, or NULL = the previous replan's winner */
  const float* history;            /* device (n_hist, S): executed states, pinned at waypoints 0 .. n_hist-1 */
  int32_t n_hist;
  int32_t stepp;                   /* current waypoint (= n_hist - 1 in the reference loop) */
  const double* dyn_pts_host;      /* host (n_dyn, 2) float64: pursuer sphere cloud after its update */
  float pursuer[2];                /* its centre                                            */
  int32_t near;                    /* 1: append extra_pts_host to the cost cloud            */
  int32_t reserved;
  const float* extra_pts_host;     /* host (n_extra, 2) or NULL                             */
} ramp_replan_state;

typedef struct ramp_replan_result {
  int32_t n_free;                  /* collision-free candidates                             */
  int32_t best_rank;               /* winner's index among the free ones (what the reference's argmin returns) */
  int32_t best_row;                /* its row in the batch                                  */
  int32_t fell_back;               /* != 0: fp16x3 range guard fired (1 + call site) and the replan was repeated in bf16x6 */
} ramp_replan_result;

/* best_out device (H,S) or NULL; batch_out device (B,H,S) or NULL (the batch handed to the selection); mask_out device
 * (B) int32 or NULL (1 = in collision).  Without a collision-free candidate (n_free == 0) best_out holds the plan the replan started from.
 * Synchronises `stream` (the result record is in host memory on return). */
int ramp_replan(ramp_ctx* ctx, const ramp_replan_params* p, const ramp_replan_state* st, float* best_out, float* batch_out,
                int32_t* mask_out, ramp_replan_result* result_host, void* stream);
/* ---- many episodes replanned in lock-step: the evaluation campaign of scripts/inference/inference_dynamic.py (run_multiple_experiments:
 *      contexts x experiments, each one ddim_p_sample_loop of up to 60 replans with 35 candidates) as ONE job per replan iteration ----
 * One call = one replan iteration of E independent episodes, in one captured hipGraph of its own: the B = sum of the episodes' candidate
 * counts rows run ramp_replan's body, every row against the record, executed history, clean plan, static cloud, pursuer cloud, goal and cost
 * cloud of ITS episode; per row the arithmetic is ramp_replan's.  The row -> latent table is the one given to ramp_set_scenes (B * 2
 * rows).  `p` carries what the episodes share (schedule, CFG weight, hard-condition layout (n_hard, B, S), smoothing, thresholds, strengths,
 * n_dyn, n_extra, cost threshold and weights); its B is the whole batch and its static_pts / n_static / cost_cloud / n_cost are not read.
 * An episode with active = 0 has ended: its rows stay in the batch (initialised from its clean plan, so everything stays finite) and its
 * selection is skipped.  Removing ended episodes from the batch, or refilling their slots, is not provided. */
typedef struct ramp_episode_state {
  int32_t n_hist;                  /* executed states of this episode, pinned at waypoints 0 .. n_hist-1 (1 .. H)         */
  int32_t stepp;                   /* its current waypoint                                                            */
  int32_t active;                  /* 0: the episode has ended                                                        */
  int32_t reserved;
  float pursuer[2];                /* its pursuer's centre                                                            */
  float reserved2[2];
} ramp_episode_state;

typedef struct ramp_episode_batch {
  int32_t n_episodes;              /* E                                                                               */
  int32_t reserved;
  const int32_t* traj_first_host;  /* host (E + 1): first row of each episode, [0] = 0, [E] = p->B, strictly increasing  */
  const float* noise;              /* device (B, H, S)                                                                */
  const float* x_clean;            /* device (E, H, S) current plans, or NULL = the previous call's winners           */
  const float* history;            /* device (E, H, S): rows [0, n_hist) of an episode's block are read               */
  const ramp_episode_state* state_host;   /* host (E)                                                                 */
  const double* static_pts;        /* device (sum n_static, 2) float64: the episodes' static APF clouds, concatenated */
  const int32_t* static_offset_host;      /* host (E + 1): first point of each, [0] = 0, strictly increasing          */
  const double* dyn_pts_host;      /* host (E, n_dyn, 2) float64: every pursuer's sphere cloud after its update        */
  const float* cost_cloud;         /* device (sum n_cost, 2): the episodes' static cost clouds, concatenated          */
  const int32_t* cost_offset_host; /* host (E + 1), [0] = 0, strictly increasing                                      */
  const int32_t* near_host;        /* host (E): 1 = this episode's extra points join its cost cloud                    */
  const float* extra_pts_host;     /* host (E, n_extra, 2): read for the near episodes only; NULL if n_extra == 0 or none is near */
} ramp_episode_batch;

/* best_out device (E,H,S) or NULL; batch_out device (B,H,S) or NULL; mask_out device (B) int32 or NULL; results_host host int32 (E,4) =
 * per episode {n_free, rank of the winner among the episode's free rows, its row in the whole batch, 0}, {0, -1, -1, 0} when no candidate
 * is free, {-1, -1, -1, 0} for an ended episode -- in both cases the episode's block of best_out is its previous plan.  result_host:
 * n_free = free candidates over all active episodes, best_rank = best_row = -1, fell_back as in ramp_replan (the call is repeated whole).
 * One synchronisation of `stream`: E x 16 bytes of results and the range flag. */
int ramp_replan_episodes(ramp_ctx* ctx, const ramp_replan_params* p, const ramp_episode_batch* ep, float* best_out, float* batch_out,
                         int32_t* mask_out, int32_t* results_host, ramp_replan_result* result_host, void* stream);
/* ---- cost guidance inside the replanning jobs, with a moving-pursuer term ----
 * ramp_cost_guide's gradient steps for ramp_replan / ramp_replan_episodes.  What a replan needs and that guide cannot give: pins that differ
 * from row to row (the executed history of the row's own episode and the goal of its clean plan), a static cloud AND a pursuer per row, and
 * an obstacle that is where it WILL be at waypoint h, not where it is now.  For one candidate x (H, S) of episode e (the planner is 2-D):
 * p_h = x[h, 0:2], c (P, 2) the episode's static cloud, m (M, 2) its moving cloud now (the pursuer's sphere points), delta (H, 2) its track --
 * the displacement of that cloud at waypoint h, predicted by the caller:
 *   C_obs    = sum_h sum_j 1/2 max(0, r     - |p_h - c_j|)^2
 *   C_mov    = sum_h sum_j 1/2 max(0, r_mov - |(p_h - delta_h) - m_j|)^2
 *   C_smooth, C_acc as in ramp_cost_guide
 *   C        = w_obs C_obs + w_mov C_mov + w_smooth C_smooth + w_acc C_acc
 * fp32, every product and sum rounded once, as written; the moving pair's difference is sub(sub(p, delta), m) per component; a pair at
 * distance 0 contributes no gradient; an empty static cloud or M = 0 drops its term; g = w_obs g_obs + (w_mov g_mov + (w_smooth g_smooth +
 * w_acc g_acc)); |g|^2 is summed in fp64.  The fp32 sums over points follow ramp_cost_guide's rule (a lane's points in order, a butterfly
 * over the lanes, the tiles of 1024 points in order), the static tiles first, then the moving tile: the bits do not depend on the batch.
 * M <= 1024 (one tile), H <= 128.
 * One iteration is ramp_cost_guide's six steps with the pinned waypoints of row b of episode e: every waypoint < n_hist[e], waypoint H - 1
 * and every waypoint of the hard-condition table.  Their values in the working copy are what the replan's pinning writes there, in its
 * order: the hard-condition values in table order, then the rows of the history, then x_clean[e][H - 1].  Only channels 0:2 are touched;
 * pinned waypoints and channels >= 2 keep their bits in memory; a row whose episode has active == 0 is left unchanged.
 * Place in the replan, on DDIM step j with n_guide[j] > 0: on x0, after the CFG combination and, on the last step, after both APF passes and
 * the goal copy, before the DDIM update.  ONE launch per guided step, whatever E and the iteration count.  No random numbers.
 * Static clouds, moving points, tracks and offsets are copied into buffers of the context before the launch and the captured graph reads
 * those: other CONTENTS of equal sizes replay the same graph and are honoured.  The seven scalars, n_guide[], step[], n_mov, the clouds'
 * total and whether tap_out is set are part of the graph key.  The bf16x6 repeat of a flagged replan runs the same guide. */
typedef struct ramp_replan_guide {
  int32_t n_scenes;                  /* 1 for ramp_replan, E for ramp_replan_episodes */
  int32_t n_mov;                     /* points of each episode's moving cloud, 0 .. 1024 */
  const float*   cloud_points;       /* device (sum P, 2): static guide clouds, concatenated (an empty one allowed) */
  const int32_t* cloud_offset_host;  /* host (n_scenes + 1): [0] = 0, non-decreasing */
  const float*   mov_points_host;    /* host (n_scenes, n_mov, 2) */
  const float*   mov_track_host;     /* host (n_scenes, H, 2) */
  double radius, radius_mov, w_obs, w_mov, w_smooth, w_acc, max_norm;
  const int32_t* n_guide;            /* host (p->n_steps), 0 .. RAMP_GUIDE_MAX_STEPS */
  const float*   step;               /* host (p->n_steps) */
  float* tap_out;                    /* device (2, B, H, S) or NULL: x0 just before / just after the LAST guided launch of the call */
} ramp_replan_guide;
/* ramp_replan / ramp_replan_episodes with the guide: rg == NULL, or n_guide zero on every step, IS the unguided call, bit for bit (and
 * ramp_replan / ramp_replan_episodes are these entries with rg == NULL).  Refused on the host before any launch (non-zero, the entry's
 * name in ramp_last_error): n_mov outside 0 .. 1024; n_scenes != 1 (ramp_replan_guided) resp. != E; offsets that are not non-decreasing
 * from 0; non-finite scalars or step; radius <= 0 with w_obs != 0; radius_mov <= 0 with w_mov != 0 and n_mov > 0; n_guide[j] outside
 * 0 .. RAMP_GUIDE_MAX_STEPS; a NULL table where one is needed (offsets, n_guide, step, cloud_points with a non-empty table, moving points
 * and track with n_mov > 0); H > 128; state_dim < 2. */
int ramp_replan_guided(ramp_ctx* ctx, const ramp_replan_params* p, const ramp_replan_state* st, const ramp_replan_guide* rg, float* best_out,
                       float* batch_out, int32_t* mask_out, ramp_replan_result* result_host, void* stream);
int ramp_replan_episodes_guided(ramp_ctx* ctx, const ramp_replan_params* p, const ramp_episode_batch* ep, const ramp_replan_guide* rg,
                                float* best_out, float* batch_out, int32_t* mask_out, int32_t* results_host,
                                ramp_replan_result* result_host, void* stream);
/* the kernel alone on (B, H, S) rows in place: n_iter (0 .. RAMP_GUIDE_MAX_STEPS) iterations of size `step` in one launch; rg->n_guide,
 * rg->step and rg->tap_out are not read, rg->n_scenes >= 1.  traj_scene device int32 (B) or NULL = scene 0; a row whose index is outside
 * the table is left unchanged.  pin_first device int32 (B) or NULL (= 0): waypoints < pin_first[b] and waypoint H - 1 are pinned, together
 * with the hard_idx_host (n_hard) waypoints; a pinned waypoint's value in the working copy is hard_val's (device (n_hard, B, S), later
 * entries win) where the table names it and the array's own otherwise -- so a replan's launch is this call with its history rows and its
 * goal appended to the table.  Refusals as above, with "ramp_guide_step_moving".  Synchronises `stream`. */
int ramp_guide_step_moving(float* traj, int32_t B, int32_t H, int32_t S, const ramp_replan_guide* rg, const int32_t* traj_scene,
                           const int32_t* pin_first, int32_t n_iter, float step, int32_t n_hard, const int32_t* hard_idx_host,
                           const float* hard_val, void* stream);
/* terms_out device (B, 4) doubles = {C_obs, C_mov, C_smooth, C_acc}, unweighted, of the rows as they are: fp64 sums over fp32 pair values
 * in a fixed order (NaN for a scene index outside the table; with n_mov == 0 columns 0, 2, 3 are ramp_guide_cost's).  Synchronises `stream`. */
int ramp_guide_cost_moving(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_replan_guide* rg, const int32_t* traj_scene,
                           double* terms_out, void* stream);
/* the selection alone (compute_trajectory_costs + winner with x[0, 2:] = 0) for a finished batch, e.g. the high-level plan
 * (diffusion_model_dynamic.py:524-530): mask / path_len / smooth device (B), best_out device (H,S), result_dev device
 * int32[4] = {n_free, best_rank, best_row, 0}.  Asynchronous. */
int ramp_select_best(const float* traj, int32_t B, int32_t H, int32_t S, const float* cloud, int32_t n_points, float threshold,
                     float w_smooth, float w_len, int32_t* mask, float* path_len, float* smooth, float* best_out,
                     int32_t* result_dev, void* stream);
/* Multi-GPU planning (the candidates are sharded over the ranks, the selection needs the global batch): the
 * per-candidate collision mask / path length / smoothness of the context's LAST ramp_replan (device arrays of B), to be
 * all-gathered, and the selection of compute_trajectory_costs (cost.py:56-88; min-max normalisation over ALL collision-free
 * candidates, first minimum) on the gathered arrays: result_dev device int32[4] = {n_free, best_rank, best_row, 0}; the rank
 * that owns best_row broadcasts the trajectory (reference call sites: diffusion_model_dynamic.py:547, 592-608). */
int ramp_replan_costs(ramp_ctx* ctx, int32_t B, int32_t* mask_out, float* path_len_out, float* smooth_out, void* stream);
int ramp_select_from_costs(const int32_t* mask, const float* path_len, const float* smooth, int32_t B, float w_smooth,
                           float w_len, int32_t* result_dev, void* stream);

/* ---- kernel-level entry points (same kernels the loops use; exported for parity tests) ---- */
/* avoidance(trajectories, ObstacleField(cloud, thr), window, strength) in place (APFhelper.py:37-104) */
int ramp_apf(float* traj, int32_t B, int32_t H, int32_t S, const ramp_apf_params* p, void* stream);
/* the same with one cloud per scene (the kernel ramp_sample_scenes runs; inference_static.py:113-190, one ObstacleField per
 * experiment): trajectory b is pushed away from scene traj_scene[b]'s points only, bit for bit what ramp_apf gives for that
 * cloud.  p->cloud must be NULL; a trajectory whose scene index is outside [0, n_scenes) is left unchanged. */
int ramp_apf_scenes(float* traj, int32_t B, int32_t H, int32_t S, const ramp_apf_params* p, const ramp_scene_batch* scenes,
                    void* stream);
/* per-trajectory APF of the dynamic planner: avoidance(trajectory, obstacle_field, is_dynamic, ...)
 * (APFhelper_dynamic.py:107-142) for B trajectories at once.  points: device (P,2) FLOAT64 (the reference's numpy
 * clouds).  window >= 0: static pass (pushes waypoints [ci-w, min(H-1, ci+w)) around the waypoint ci nearest to the
 * cloud, force length strength*exp(-d/thr_force), hit iff d < thr_query); window < 0: pursuer pass over waypoints
 * [0, affected) with the 0.9/0.1 avoid/goal blend (goal: device (S) or NULL).  enable: device (B) int32 or NULL. */
int ramp_apf_dynamic(float* traj, int32_t B, int32_t H, int32_t S, const double* points, int32_t n_points,
                     double thr_query, double thr_force, double strength, int32_t window, int32_t affected,
                     const float* goal, const int32_t* enable, void* stream);
/* apply_hard_conditioning (sample_functions.py:5-10); idx host, val device (n,B,S) */
int ramp_hard_cond(float* x, int32_t B, int32_t H, int32_t S, int32_t n, const int32_t* idx_host,
                   const float* val, void* stream);
/* compute_collision_with_pointcloud + compute_path_length + compute_smoothness (cost.py:3-54):
 * mask (B) int32, path_len (B), smooth (B) */
int ramp_traj_costs(const float* traj, int32_t B, int32_t H, int32_t S, const float* cloud, int32_t n_points,
                    float threshold, int32_t* mask, float* path_len, float* smooth, void* stream);
/* Metrics.compute_collision_intensity / compute_path_length / compute_smoothness (scripts/inference/core/metrics.py:21-81):
 * per trajectory, the fraction of waypoints inside any axis-aligned box (centre +- size/2, inclusive), the xy path
 * length and sum_h |v_{h+1} - v_h| over the state dims >= 2.  box_centers / box_sizes: device (n_boxes, 2). */
int ramp_traj_metrics(const float* traj, int32_t B, int32_t H, int32_t S, const float* box_centers, const float* box_sizes,
                      int32_t n_boxes, float* intensity, float* path_len, float* smooth, void* stream);
/* Metrics.compute_variance_waypoints (metrics.py:8-19): sum over waypoints of the unbiased variance of all B*B entries
 * of triu(cdist(p, p), 1).  scratch: device, 2 * H * ceil(B/256) doubles; out: device, 1 double. */
int ramp_waypoint_variance(const float* traj, int32_t B, int32_t H, int32_t S, double* scratch, double* out, void* stream);
/* The two elementwise ends of the denoising loss (p_losses, diffusion_model_static.py:467-505), one launch / one two-stage reduction:
 * ramp_q_sample_rows: x_noisy[b] = sqrt_ac[t_rows[b]] x_start[b] + sqrt_1m_ac[t_rows[b]] noise[b]; pin_endpoints != 0: waypoints 0 and
 *   H - 1 overwritten by x_start's.  Everything on the device: schedules (T), t_rows int32 (B); a row whose t is outside [0, T) comes back NaN.
 * ramp_denoise_loss: overwrites waypoints 0 and H - 1 of x_recon with x_start's IN PLACE, then out[0] = mean of (x_recon - target)^2
 *   (l1 = 0: WeightedL2, helpers.py:97-100) or |x_recon - target| (l1 = 1: WeightedL1, :91-94), no weights; fp32 terms, fp64 sums in
 *   a fixed order (bit-reproducible).  scratch: device, 1024 doubles; out: device, 1 double. */
int ramp_q_sample_rows(const float* x_start, const float* noise, const float* sqrt_ac, const float* sqrt_1m_ac, const int32_t* t_rows,
                       int32_t T, float* x_noisy, int32_t B, int32_t H, int32_t S, int32_t pin_endpoints, void* stream);
int ramp_denoise_loss(float* x_recon, const float* x_start, const float* target, int32_t B, int32_t H, int32_t S, int32_t l1,
                      double* scratch, double* out, void* stream);

/* ---- evaluation and selection of a many-scene batch (what ramp_sample_scenes returns), per scene, in a fixed number of launches ----
 * Layout: a scene's trajectories are adjacent, scenes in order.  Every table is a DEVICE int32 array of n_scenes + 1 entries:
 * traj_first ([0] = 0, [n_scenes] = B, strictly increasing) the first row of each scene; box_offset / cloud_offset the first box /
 * point of each scene in the boxes / cost clouds concatenated over the scenes (box_offset may repeat a value: a scene without
 * boxes has intensity 0; cloud_offset is strictly increasing).  n_boxes_total / n_points_total: entries of the concatenated arrays;
 * a span is clamped to them.  Nothing here copies or synchronises: asynchronous on `stream`, capturable.  No float atomics, every
 * sum in an order fixed by the scene's own rows: a scene's results do not depend on the rest of the batch. */
/* ramp_traj_metrics with each trajectory testing the boxes of its own scene (the loop over experiments around
 * Metrics.compute_collision_intensity, scripts/inference/inference_static.py:113-190 + core/metrics.py:21-81): a scene's rows are bit
 * for bit what ramp_traj_metrics gives for that slice and that scene's boxes. */
int ramp_traj_metrics_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                             const float* box_centers, const float* box_sizes, const int32_t* box_offset, int32_t n_boxes_total,
                             float* intensity, float* path_len, float* smooth, void* stream);
/* Metrics.trajectory_success_and_metrics (core/metrics.py:83-126) per scene, free = intensity <= threshold, without compacting the
 * free rows: summary device (n_scenes, 6) doubles = {n_traj, n_free, mean intensity over all rows, mean path length over the free
 * rows, their unbiased std, waypoint variance (compute_variance_waypoints, metrics.py:8-19) of the free rows}; n_free == 0: the last
 * three are NaN; n_free == 1: std NaN, variance 0.  free_mask: device (B) int32.  intensity / path_len: device (B), e.g. from
 * ramp_traj_metrics_scenes.  H <= 65535.
 * scratch: device, 2 * H * W + n_scenes + 1 doubles with W = ceil(B / 256) + n_scenes (pair sums of every 256-row tile of every
 * scene per waypoint, then the scenes' tile table). */
int ramp_scene_summary(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                       const float* intensity, const float* path_len, float threshold, double* scratch, double* summary,
                       int32_t* free_mask, void* stream);
/* ramp_traj_costs with each trajectory reading its own scene's span of the concatenated cost cloud (cost.py:3-54 inside the loop
 * over experiments): bit for bit ramp_traj_costs with that scene's cloud.  H within the cost kernel's limit (128). */
int ramp_traj_costs_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                           const float* cloud, const int32_t* cloud_offset, int32_t n_points_total, float threshold, int32_t* mask,
                           float* path_len, float* smooth, void* stream);
/* ramp_select_best per scene (compute_trajectory_costs, cost.py:56-88, once per experiment): min-max normalisation over the scene's
 * collision-free rows, w_smooth * smooth + w_len * length, first minimum.  result_dev device (n_scenes, 4) int32 = {n_free, rank of
 * the winner among the scene's free rows, its row in the whole batch, 0}; best_out device (n_scenes, H, S): the winner, unmodified
 * (the x[0, 2:] = 0 of the dynamic planner is not part of the static flow).  A scene without a free row: {0, -1, -1, 0} and a NaN
 * block. */
int ramp_select_best_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                            const float* cloud, const int32_t* cloud_offset, int32_t n_points_total, float threshold, float w_smooth,
                            float w_len, int32_t* mask, float* path_len, float* smooth, float* best_out, int32_t* result_dev,
                            void* stream);
/* ramp_scene_summary with the pairwise waypoint distance of the variance taken over the first point_dim (2 or 3, <= S) state entries.
 * point_dim = 2 is ramp_scene_summary, bit for bit.  Refusals name "ramp_scene_summary_nd". */
int ramp_scene_summary_nd(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, const int32_t* traj_first,
                          int32_t n_scenes, const float* intensity, const float* path_len, float threshold, double* scratch,
                          double* summary, int32_t* free_mask, void* stream);
/* The selection of ramp_select_best_scenes alone, on per-row arrays the caller already holds: mask device (B) int32, 1 = colliding (as
 * ramp_select_best_scenes writes it), path_len / smooth device (B).  Same result layout, same NaN block for a scene without a free row. */
int ramp_select_scored_scenes(const float* traj, int32_t B, int32_t H, int32_t S, const int32_t* traj_first, int32_t n_scenes,
                              const int32_t* mask, const float* path_len, const float* smooth, float w_smooth, float w_len,
                              float* best_out, int32_t* result_dev, void* stream);

/* ---- K distinct plans per scene: the K cheapest collision-free trajectories that are pairwise at least min_sep apart, and the mode
 * (the nearest of them) of every other free row.  Per scene s over its rows [traj_first[s], traj_first[s + 1]); traj_first device
 * (n_scenes + 1), non-decreasing (an empty scene is allowed), spans clamped to [0, B].  Free rows: mask[b] == 0.
 * Order.  That of ramp_select_scored_scenes: tot = w_smooth sm + w_len pl on path_len and smooth min-max normalised over the scene's free
 *   rows, fp32 with one rounding per operation.  Row a comes before row b if tot_a is NaN and (tot_b is not NaN or a < b), or if neither
 *   is NaN and (tot_a < tot_b, or tot_a == tot_b and a < b).  A scene whose free rows all tie (0 / 0) is therefore ordered by row.
 * Distance.  D = point_dim (2 or 3, <= S), p_{b,h} = traj[b, h, 0:D].  metric 0: d = (1 / H) sum_h |p_{a,h} - p_{b,h}|; metric 1:
 *   d = max_h |p_{a,h} - p_{b,h}|.  Per waypoint the differences, the squares (added in coordinate order) and the root are fp32; metric 0 adds
 *   the norms in fp64 in ascending h, divides by H in fp64 and rounds to fp32 once; metric 1 is NaN as soon as one norm is.  The value of
 *   a pair depends on the two rows alone.
 * Selection.  rep_0 = the first free row in the order; rep_k = the first free row in the order with d(b, rep_j) >= min_sep for every j < k:
 *   a row with d < min_sep, or a NaN d, to an earlier representative is suppressed.  It stops at K representatives or when no row is left;
 *   min_sep = 0 returns the K first rows of the order (NaN distances aside), and slot 0 is always the row ramp_select_scored_scenes picks.
 * Modes.  Every free row belongs to the slot j with the smallest d(b, rep_j), the lowest j on a tie; a NaN distance never wins; a
 *   representative belongs to its own slot.  Colliding rows, rows of no scene and free rows whose every distance is NaN get -1.
 * Outputs (all device, all required): best_out (n_scenes, K, H, S) the representatives unmodified, NaN in the slots nothing fills;
 *   rows_out (n_scenes, K) their rows in the whole batch, -1 padded; result_dev (n_scenes, 4) = {n_free, n_selected, rows_out[s][0], 0};
 *   mode_of (B) the slot of every row; sep_out (B) its distance to that slot's representative, NaN where mode_of is -1;
 *   mode_count (n_scenes, K) rows per slot.
 * scratch: device, 2 * B + n_scenes 32-bit words (row states, totals, the passes' picks); nothing is allocated inside the call.
 * 2 K + 1 launches whatever n_scenes, B and the data; asynchronous on `stream`, capturable, no copies, no host reads, no float atomics; a
 * scene's outputs depend on that scene's rows alone.  Refused on the host before any launch (non-zero, "ramp_select_diverse_scenes" in
 * ramp_last_error): K outside 1 .. RAMP_DIVERSE_MAX_K, min_sep negative or NaN, metric outside {0, 1}, point_dim outside {2, 3} or > S,
 * H outside 1 .. 128, B < 0, n_scenes < 1, a NULL pointer (stream aside). */
#define RAMP_DIVERSE_MAX_K 16
int ramp_select_diverse_scenes(const float* traj, int32_t B, int32_t H, int32_t S, int32_t point_dim, const int32_t* traj_first,
                               int32_t n_scenes, const int32_t* mask, const float* path_len, const float* smooth, float w_smooth,
                               float w_len, int32_t K, float min_sep, int32_t metric, float* best_out, int32_t* rows_out,
                               int32_t* result_dev, int32_t* mode_of, float* sep_out, int32_t* mode_count, void* scratch, void* stream);

/* ---- swept collision checks and clearances, 2-D and 3-D ----
 * Position p_h of waypoint h = the first D = point_dim (2 or 3, <= S) entries of the state; margin >= 0 is the robot's radius.  Every
 * trajectory meets only the primitives of its own scene (traj_first as above; the three offset tables may repeat a value: a scene may lack
 * any kind of primitive; spans are clamped to the totals).
 *   box k      the closed set lower_d <= x_d <= upper_d, d < D, lower = c - s / 2 - margin, upper = c + s / 2 + margin (fp32, s / 2.f;
 *              at margin 0 the comparisons of ramp_traj_metrics)
 *   sphere k   |x - c| <= r + margin
 *   wp_hits    waypoints inside any box or sphere
 *   seg_hits   segments [p_h, p_{h+1}], h < H - 1, that meet any box or sphere.  Box: slab clipping of t in [0, 1] per axis (an axis with a
 *              zero direction component passes iff the start lies inside the slab, inclusive), hit iff the clipped interval is not empty.
 *              Sphere: distance from the centre to the segment, t = clamp((c - a).(b - a) / |b - a|^2, 0, 1), t = 0 for a zero-length
 *              segment; hit iff it is <= r + margin.  Both are OR-ed with the two endpoint tests: a segment's flag is never below either
 *              endpoint's.
 *   clear_wp   min over waypoints and cloud points of |p_h - q|; clear_seg the min over segments and points of the point-segment
 *              distance (the same t), min-ed with every endpoint distance: clear_seg <= clear_wp always.  +inf for a scene without cloud
 *              points.  A caller's collision test is clear < threshold, strict (cost.py:45-49).
 *   path_len   sum_h |p_{h+1} - p_h| over the D position entries; smooth: sum_h of the norm of the difference of the entries >= D (0 when
 *              S == D).  Per-segment values are added serially in fp32, ramp_traj_costs's order: at D = 2 the same bits.
 * A trajectory with a non-finite position coordinate gets wp_hits = H, seg_hits = H - 1 and NaN clearances: it is never free. */
typedef struct ramp_obstacles {
  int32_t point_dim;               /* 2 or 3, <= S */
  int32_t n_scenes;                /* 1 for a single scene */
  const float* box_centers;        /* device (n_boxes_total, D) */
  const float* box_sizes;          /* device (n_boxes_total, D): full side lengths */
  const float* sphere_centers;     /* device (n_spheres_total, D) */
  const float* sphere_radii;       /* device (n_spheres_total) */
  const float* cloud;              /* device (n_points_total, D) */
  const int32_t* box_offset;       /* DEVICE int32 (n_scenes + 1) each */
  const int32_t* sphere_offset;
  const int32_t* cloud_offset;
  int32_t n_boxes_total, n_spheres_total, n_points_total;
  float margin;
} ramp_obstacles;
/* Outputs are device (B): wp_hits / seg_hits int32, the rest fp32; any of them may be NULL.  swept == 0 skips all segment work and leaves
 * seg_hits / clear_seg untouched.  One launch, one 256-thread block per trajectory; asynchronous on `stream`, capturable, no copies, no
 * float atomics; a scene's rows do not depend on the rest of the batch.  Refused on the host before any launch (non-zero,
 * "ramp_traj_clearance" in ramp_last_error): point_dim outside {2, 3} or > S, H < 2 or H > 128, a negative margin, a missing table, a
 * total > 0 with a NULL array. */
int ramp_traj_clearance(const float* traj, int32_t B, int32_t H, int32_t S, const ramp_obstacles* ob, const int32_t* traj_first,
                        int32_t swept, int32_t* wp_hits, int32_t* seg_hits, float* clear_wp, float* clear_seg, float* path_len,
                        float* smooth, void* stream);
/* one p_mean_variance evaluation given eps (diffusion_model_static.py:161-172); predict_x0 != 0: predict_epsilon=False,
 * x0 = the combined network output (diffusion_model_static.py:109-118) */
int ramp_cfg_mean(const float* x, const float* eps, int32_t B, int32_t HS, int32_t n_rp, double w0, double w1,
                  float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, int32_t clip, int32_t predict_x0,
                  float* x0_out, float* mean_out, float* ecomb_out, void* stream);
/* ramp_cfg_mean with one weight per network row (the guidance step of ramp_sample_composed when the prefix is not shared;
 * diffusion_model_static.py:188-229, diffusion_model_3d.py:165-174): e_comb[b] = sum_j row_weight[b * n_rp + j] eps[b * n_rp + j], j = 0 .. n_rp - 1
 * in that order, then x0, clamp and posterior mean exactly as ramp_cfg_mean.  row_weight device (B, n_rp), 2 <= n_rp <=
 * RAMP_MAX_ROWS_PER_TRAJ; HS a multiple of 4 and every tensor 16-byte aligned (four elements per access). */
int ramp_cfg_mean_rows(const float* x, const float* eps, int32_t B, int32_t HS, int32_t n_rp, const float* row_weight,
                       float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, int32_t clip, int32_t predict_x0,
                       float* x0_out, float* mean_out, float* ecomb_out, void* stream);
/* the kernels of ramp_score_energy / ramp_sample_mcmc one at a time (all pointers device unless said otherwise):
 * ramp_row_energy: energy_out[r] = 1/2 sum_e f[r, e]^2, f (R, HS).
 * ramp_combine_energy: energy_out[b] = sum_j w_j energy_rows[b n_rp + j] in fp64, j ascending; w = weights_host (HOST, n_rp <= 3 floats) or
 * line b of row_weight (device (B, n_rp)) -- exactly one of the two.
 * ramp_mcmc_propose: x_prop = (x - a eps) + c z (fp32: two products, a difference, a sum) on free waypoints, x on the n_pinned waypoints
 * pinned_idx (device int32) lists.
 * ramp_mcmc_accept: kind 1 accepts always; kind 2 forms log alpha as documented at ramp_sample_mcmc from (x, x_prop, eps, eps_prop, energy,
 * energy_prop, a, sigma, eta), writes it to log_alpha_out (optional) and accepts where log u < log alpha and energy_prop, log alpha are
 * finite.  Accepted trajectories: x <- x_prop, eps <- eps_prop, energy <- energy_prop.  accept_out int32 (B). */
int ramp_row_energy(const float* f, int32_t R, int32_t HS, double* energy_out, void* stream);
int ramp_combine_energy(const double* energy_rows, int32_t B, int32_t n_rp, const float* weights_host, const float* row_weight,
                        double* energy_out, void* stream);
int ramp_mcmc_propose(const float* x, const float* eps, const float* z, float a, float c, const int32_t* pinned_idx, int32_t n_pinned,
                      float* x_prop, int32_t B, int32_t H, int32_t S, void* stream);
int ramp_mcmc_accept(float* x, const float* x_prop, float* eps, const float* eps_prop, double* energy, const double* energy_prop,
                     const float* u, int32_t kind, float a, double sigma, double eta, const int32_t* pinned_idx, int32_t n_pinned,
                     int32_t* accept_out, double* log_alpha_out, int32_t B, int32_t H, int32_t S, void* stream);
/* the DDIM update of ddim_p_sample given x0 (diffusion_model_static.py:321-333 / _dynamic.py:436-447), eta = 0:
 * x_out = sqrt_a_prev * x0 + dir_coef * (x - sqrt_a_t * x0) / sqrt_1m_a_t */
int ramp_ddim_finish(const float* x, const float* x0, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                     float dir_coef, float* x_out, int32_t B, int32_t H, int32_t S, void* stream);
/* generic exact-fp32 MFMA GEMM with taps: C[M,N] = sum_tap shift(A)[M,K] W[tap][N][K]^T + bias + resid */
int ramp_op_gemm(const float* A, const float* W, const float* bias, const float* resid, float* C,
                 int32_t M, int32_t N, int32_t K, int32_t taps, int32_t shift0, int32_t shift_step,
                 int32_t L, void* stream);
/* the same product on a named GEMM kernel (parity tests, micro-benchmarks): mode 0 exact fp32, 1 bf16x6 with
 * fragment-packed weights, 2 bf16x6 with LDS-staged weights, 3 fp16x3 (shapes a split kernel does not cover run fp32).
 * fp16x3 only: a_absmax_prev > 0 is the operand maximum the delayed scaling assumes (0 = unscaled operand);
 * *a_absmax_out_host receives the maximum |A| the launch recorded and *range_flag_out_host != 0 reports that the scaled
 * operand left the fp16 range (either may be NULL).  Synchronises `stream`; packs W on every call. */
int ramp_op_gemm_mode(const float* A, const float* W, const float* bias, const float* resid, float* C,
                      int32_t M, int32_t N, int32_t K, int32_t taps, int32_t shift0, int32_t shift_step,
                      int32_t L, int32_t mode, float a_absmax_prev, float* a_absmax_out_host,
                      int32_t* range_flag_out_host, void* stream);
/* the fused feed-forward with token-owning waves (ffx.hip) on raw weights, forward then (dz, dz1 non-NULL) backward:
 *   z2 = z1 + W2 (a gelu(g)) + b2, [a | g] = W1 LN(z1; ln_g, ln_b) + b1          (reference: layers_attention_mini.py:38-45, 147)
 *   dz1 = dz + LNbwd(W1^T [d(hg) gelu(g) | d(hg) a gelu'(g)]; z1), d(hg) = W2^T dz  (its input gradient)
 * W1 (2048, 256) rows = 1024 value then 1024 gate features, W2 (256, 1024), z1 / dz / z2 / dz1 (M, 256), all device fp32.
 * absmax_prev_host[4]: the operand maxima the delayed fp16 scaling assumes for LN(z1), a gelu(g), dz, d(ag) (0 = unscaled);
 * absmax_out_host[4] the maxima recorded, *range_flag_out_host the range guard.  Packs the weights on every call (tests). */
int ramp_op_ffx(const float* z1, const float* dz, const float* W1, const float* b1, const float* W2, const float* b2,
                const float* ln_g, const float* ln_b, int32_t M, const float* absmax_prev_host, float* z2, float* dz1,
                float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* the same operation on the v_mfma_f32_16x16x32_f16 kernel pair (ffx16.hip; ramp_launch_plan.mfma16 = 1, what the product runs).  Its tiling follows M and
 * the device's CU count exactly as in a job: 128-token tiles, 64-token half tiles for a last round that would idle half of the CUs and for launches of at
 * most CUs / 2 tiles (on 256 CUs: M <= 16384 half tiles only; M = 20000 full tiles only; M = 33000 or 49152 both). */
int ramp_op_ffx16(const float* z1, const float* dz, const float* W1, const float* b1, const float* W2, const float* b2,
                  const float* ln_g, const float* ln_b, int32_t M, const float* absmax_prev_host, float* z2, float* dz1,
                  float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* Token-owning linear layer with K = 256 (tkl.hip; the product path uses it for LayerNorm-1 -> QKV, the attention output
 * projection and its input gradient -- reference layers_attention_mini.py:60-120, 130-149):
 *   Y[m][n] = sum_k pro(X)[m][k] W[n][k] + bias[n] + rowbias[rowvar[m / L]][n] + resid[m][n],  pro = LayerNorm(256) when ln_g
 * is given, identity otherwise.  X (M, 256), W (N, 256) with N a multiple of 32 (<= 768), Y / resid (M, N), rowbias
 * (n_var, N) with N == 256 (n_var <= 4: staged in LDS; more: read from global memory in the epilogue), all device fp32;
 * bias / resid / rowbias / ln_g, ln_b may be NULL.  absmax_prev: the operand maximum the delayed fp16 scaling assumes
 * (0 = unscaled); *absmax_out_host the maximum recorded, *range_flag_out_host the range guard.  Packs the weight on every
 * call (tests). */
int ramp_op_tkl(const float* X, const float* W, const float* bias, const float* resid, const float* rowbias,
                const int32_t* rowvar, int32_t n_var, int32_t L, const float* ln_g, const float* ln_b, int32_t M, int32_t N,
                float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* the same linear on the v_mfma_f32_16x16x32_f16 kernel (tkl16.hip; what the product runs with ramp_launch_plan.mfma16 = 1) */
int ramp_op_tkl16(const float* X, const float* W, const float* bias, const float* resid, const float* rowbias,
                  const int32_t* rowvar, int32_t n_var, int32_t L, const float* ln_g, const float* ln_b, int32_t M, int32_t N,
                  float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* Self-attention fused with its output projection (atk.hip; the product path's replacement of the attention kernel + the
 * out-projection launch -- reference layers_attention_mini.py:101-127 and :132):
 *   Y[m] = resid[m] + Wo softmax(q k^T / 8) v [m] + bias + rowbias[rowvar[m / L]],  4 heads x 64, softmax over the L tokens of
 * m's sample.  qkv (M, 768) = [q | k | v] rows, Wo (256, 256), resid / Y (M, 256), rowbias (n_var, 256; n_var <= 4: staged
 * in LDS, more: read from global memory in the epilogue), device fp32; L must divide 48 or 32 and M be whole samples.
 * Scaling arguments as ramp_op_tkl (the operand is the attention output o). */
int ramp_op_ato(const float* qkv, const float* Wo, const float* bias, const float* resid, const float* rowbias, const int32_t* rowvar,
                int32_t n_var, int32_t L, int32_t M, float absmax_prev, float* Y, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* Backward of the self-attention itself on sample-owning waves (atk.hip, atb_kernel; the product path's replacement of the exact-fp32
 * attention backward kernel on levels whose token count divides 48 or 32 -- CrossAttention.forward, layers_attention_mini.py:101-127,
 * differentiated): dqkv (M, 768) = d[q | k | v] given dout (M, 256) = d(o) and qkv (M, 768); 4 heads x 64, samples of L tokens; fp16x3 products
 * with exact per-wave operand scales (no call site, no range guard needed). */
int ramp_op_atb(const float* qkv, const float* dout, float* dqkv, int32_t M, int32_t L, void* stream);
/* One wide k = 5 convolution on the sample-owning block kernel (tkw.hip) from raw weights W [5][N][K] (tap, c_out, c_in; for the input
 * gradient the transposed weight, same tap order, dir = -1): Conv1dBlock / ResidualTemporalBlock of the coarse levels (layers.py:280-297, 327-361).
 *   operand: X (M, K) -- channels [0, K1) from X and [K1, K) from X2 when X2 is given -- or, when gn_c is given, the GroupNorm + Mish input
 *            gradient GNbwd(X (.) mish'(gn_gamma x^ + gn_beta) gn_gamma) with x^ from gn_c (M, K) and gn_stats (M / L, 8, 2) [mean, rstd];
 *   result:  Y = conv + bias + resid + resid2 (channels [0, N1) to Y, the rest to Y2 when Y2 is given), or, when Cst is given,
 *            Cst = conv + bias, stats = its GroupNorm(8) statistics, Y = mish(GN(Cst) gamma + beta) + tbias + resid.
 * absmax_prev > 0: the operand is scaled from that maximum (delayed scaling); the maximum of this call is returned.
 * Narrow layers (N, K in {32, 64}; one operand, one output; L >= 8 dividing 48 or 32) run the same fusion on sample-owning WAVES (tkc.hip), as
 * ramp_sample does for the two finest levels and the final Conv1dBlock (UnetInference.py:142-145). */
int ramp_op_tkw(const float* X, const float* X2, int32_t K1, const float* W, const float* bias, const float* resid, const float* resid2,
                const float* gn_c, const float* gn_stats, const float* gn_gamma, const float* gn_beta, const float* gamma, const float* beta,
                const float* tbias, int32_t M, int32_t L, int32_t N, int32_t K, int32_t dir, int32_t N1, float absmax_prev, float* Y, float* Y2,
                float* Cst, float* stats, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* The forward form of ramp_op_tkw (one operand, one output, GroupNorm epilogue) with one timestep per sample: sample r (L tokens) adds
 * time_table[t_rows[r] * tt_stride + n] behind the Mish instead of tbias[n].  time_table device (T, tt_stride) at this layer's column offset,
 * t_rows device int32 (M / L), every entry in [0, T) -- the caller's duty here, ramp_score_rows checks it on the host.  Samples that carry
 * timestep t equal, bit for bit, ramp_op_tkw with tbias = time_table + t * tt_stride. */
int ramp_op_tkw_rows(const float* X, const float* W, const float* bias, const float* resid, const float* gamma, const float* beta,
                     const float* time_table, int32_t tt_stride, const int32_t* t_rows, int32_t M, int32_t L, int32_t N, int32_t K, float absmax_prev,
                     float* Y, float* Cst, float* stats, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* d(ln1) = d(qkv) Wqkv^T with the LayerNorm-1 backward in its epilogue (tkl.hip, tklb_kernel; the product path's replacement of
 * the d(ln1) GEMM + ln_bwd pair, reference layers_attention_mini.py:132 differentiated): out = add + LNbwd(dqkv W^T; z, ln_g).
 * dqkv (M, 768), W (256, 768) = [Wq | Wk | Wv]^T rows, z / add / out (M, 256), device fp32.  Scaling arguments as ramp_op_tkl. */
int ramp_op_tklb(const float* dqkv, const float* W, const float* z, const float* ln_g, const float* add, int32_t M,
                 float absmax_prev, float* out, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* Attention backward, d(ln1) and the LayerNorm-1 backward as ONE launch (atl.hip, abl_kernel; the product path's replacement of
 * ramp_op_atb + ramp_op_tklb on levels whose token count divides 48 or 32 -- BasicTransformerBlock.forward's `attn1(norm1(x)) + x`,
 * layers_attention_mini.py:101-127 and :132, differentiated from d(o) back to the block input):
 *   out = add + LNbwd( attention-backward(qkv, dout) W^T ; z, ln_g ).  Operands as ramp_op_atb / ramp_op_tklb; scaling arguments as
 * ramp_op_tkl (the operand is d(qkv), which never reaches memory). */
int ramp_op_abl(const float* qkv, const float* dout, const float* W, const float* z, const float* ln_g, const float* add, int32_t M, int32_t L,
                float absmax_prev, float* out, float* absmax_out_host, int32_t* range_flag_out_host, void* stream);
/* (ramp_bench_gemm / ramp_stress_gemm, the micro-benchmark and stress harness, are diagnostics: declared in ramp_hip_tools.h, exported by
 * ramp_amd/lib/libramp_hip_tools.so only -- round 6) */
int ramp_op_groupnorm(const float* x, const float* gamma, const float* beta, const float* tbias,
                      const float* resid, float* y, float* stats, int32_t R, int32_t L, int32_t C,
                      float eps, int32_t mish, void* stream);
/* ramp_op_groupnorm with one timestep per row: row r adds time_table[t_rows[r] * tt_stride + c]; t_rows device int32 (R), entries in [0, T) */
int ramp_op_groupnorm_rows(const float* x, const float* gamma, const float* beta, const float* time_table, int32_t tt_stride,
                           const int32_t* t_rows, const float* resid, float* y, float* stats, int32_t R, int32_t L, int32_t C,
                           float eps, int32_t mish, void* stream);
int ramp_op_groupnorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma,
                          const float* beta, const float* add, float* dx, int32_t R, int32_t L, int32_t C,
                          int32_t mish, void* stream);
int ramp_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t n_tok, void* stream);
int ramp_op_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* add, float* dx,
                          int32_t n_tok, void* stream);
int ramp_op_geglu(const float* ag, float* hg, int32_t n_tok, int32_t F, void* stream);
int ramp_op_geglu_bwd(const float* dhg, const float* ag, float* dag, int32_t n_tok, int32_t F, void* stream);
int ramp_op_attention(const float* qkv, float* o, int32_t R, int32_t L, void* stream);
int ramp_op_attention_bwd(const float* qkv, const float* dout, float* dqkv, int32_t R, int32_t L, void* stream);
/* The scene encoders' kernels that look across tokens, one launch each (what ramp_encode_scene / ramp_encode_scenes schedule); every
 * table is a DEVICE int32 array.  Refused on the host before any launch (non-zero, the entry's name in ramp_last_error): a null
 * pointer, a non-positive size, dh outside {16, 64}, mode outside {0, 1}, ldo < C.
 *   attention   qkv (T, 3 heads dh) = [q | k | v], head h at column h dh; o (T, heads dh) = softmax(scale q k^T) v per head.
 *               _seg: tiles (n_tiles, 3) = {scene's first row, scene's row count, first query of the tile inside the scene}, one tile
 *               per 64 queries of a scene; a query attends to its own scene's keys only
 *   colreduce   x (n_seg seglen, C) -> out (n_seg, C): mode 0 the mean, 1 the maximum over each segment's rows.
 *               _seg: segment s owns the rows [first[s], first[s + 1]); out has row stride ldo >= C, the gap columns are not written
 *   enc2d_prep  cloud (No, Np, 2) -> centers (No, 2) the mean point, maxd (No) the largest |coordinate - centre| of each obstacle.
 *               _seg: obstacle o owns the points [obstacle_first[o], obstacle_first[o + 1]) */
int ramp_op_scene_attention(const float* qkv, float* o, int32_t T, int32_t heads, int32_t dh, float scale, void* stream);
int ramp_op_scene_attention_seg(const float* qkv, float* o, const int32_t* tiles, int32_t n_tiles, int32_t heads, int32_t dh, float scale,
                                void* stream);
int ramp_op_scene_colreduce(const float* x, float* out, int32_t n_seg, int32_t seglen, int32_t C, int32_t mode, void* stream);
int ramp_op_scene_colreduce_seg(const float* x, float* out, const int32_t* first, int32_t n_seg, int32_t C, int32_t ldo, int32_t mode,
                                void* stream);
int ramp_op_scene_enc2d_prep(const float* cloud, int32_t No, int32_t Np, float* centers, float* maxd, void* stream);
int ramp_op_scene_enc2d_prep_seg(const float* cloud, const int32_t* obstacle_first, int32_t No, float* centers, float* maxd, void* stream);

/* debug taps (cfg.debug_taps = 1): kind "out" = module output, "gout" = dE/d(module output) of
 * the last ramp_score call; module names as in the reference ("downs.0.3", "mid_block1", ...).
 * Copies min(n_floats, available) floats, channels-last (rows, L, C); returns count via *n_copied. */
int ramp_debug_read(ramp_ctx* ctx, const char* kind, const char* module, float* out, int64_t n_floats,
                    int64_t* n_copied, void* stream);

/* bookkeeping for bench / profiling */
/* fp16x3 mode only: waits for `stream`, then *flag != 0 if any GEMM of the last ramp_sample found an operand that, scaled by
 * the previous evaluation's maximum, left the fp16 range (the results of that call must be discarded and the job repeated:
 * ramp_set_fallback); always 0 in the other modes.  Round 6: the guard's state is logged on the device after every evaluation
 * of a job; a flagged status also records WHICH evaluation raised it first (ramp_range_trip). */
int ramp_range_status(ramp_ctx* ctx, int32_t* flag, void* stream);
/* the first flagged evaluation (0-based index into ramp_sample_params.t) and the highest flagged GEMM call site of it, as the last
 * flagged ramp_range_status found them; *eval = -1 when the last status was clean.  `site` may be NULL. */
int ramp_range_trip(ramp_ctx* ctx, int32_t* eval, int32_t* site);
/* fp16x3 mode: how the following ramp_sample calls run.
 *   0  normally (fp16x3, every evaluation scaled from its predecessor's operand maxima);
 *   1  every evaluation on the bf16x6 kernels (range-free, 1.83 x the time);
 *   2  (round 6) fp16x3 again, but the evaluation ramp_range_trip reports AND its successor run as CALIBRATING ones -- bf16x6 kernels
 *      that record every call site's true operand maximum: they cannot overflow, and what follows is scaled from maxima that are
 *      right whether the excursion persists or was a one-evaluation spike.
 *      This is what the Python wrapper does first to repeat a flagged job (diffusion_model_static.py:232-256 as one job): the
 *      repeat is a function of the job alone (same inputs, same bits, whatever ran before), costs 1.06 x a steady job and stays
 *      on the fast kernels; only if the repeat is flagged too (a second, later excursion) does the job run a third time in
 *      mode 1.  Needs a flagged ramp_range_status on record. */
int ramp_set_fallback(ramp_ctx* ctx, int32_t mode);
/* fp16x3 mode: where a sampling job's FIRST score evaluation takes its operand scales from (every later one: the evaluation before it).
 * on = 1 (default, round 5): from the context's CANONICAL calibration -- one bf16x6 evaluation that only records the operand maxima, run once,
 * outside any job, on x ~ N(0, I) drawn with a fixed Philox seed under the job's hard conditions at the job's first timestep (x_T of every job
 * is a draw of the same distribution; the maxima only pick power-of-two scales with 2^9.9 of head room, and the range guard covers callers whose
 * x_T is something else).  No job contains a bf16x6 evaluation, the first job on a context costs that one extra evaluation, and a job's result
 * does not depend on which jobs ran before it (same inputs -> same bits, whatever happened in between).
 * on = 0: every job calibrates itself in its first evaluation (bf16x6 kernels), ~3 % slower, equally independent of history. */
int ramp_set_calibration_reuse(ramp_ctx* ctx, int32_t on);
/* per-launch HIP-event timing (eager, non-graph calls only).  Categories: 0 = MFMA GEMM (linears + k5/k1
 * convs), 1 = attention, 2 = GroupNorm/LayerNorm/GEGLU rows, 3 = stride-2 / first / last convs, 4 = sampler
 * (CFG, DDPM/DDIM update, APF).  ramp_profile_read sums elapsed ms, algorithmic FLOPs and launch counts
 * per category since ramp_profile(ctx, 1); arrays of length 5. */
int ramp_profile(ramp_ctx* ctx, int32_t enable);
int ramp_profile_read(ramp_ctx* ctx, double* ms, double* flops, int64_t* count);
/* the same launches of category 0 by KERNEL (arrays of length n <= 9): 0 ffx_kernel forward, 1 ffx_kernel backward (the token-owning
 * fused feed-forward: the dominant kernel, bench.py's roofline.frac), 2 tkl_kernel, 3 tklb_kernel, 4 ato_kernel, 5 abl_kernel,
 * 6 tkc_kernel, 7 tkw_kernel, 8 every other launch of the class (tile kernels, exact-fp32 layers) */
int ramp_profile_read_kernels(ramp_ctx* ctx, int32_t n, double* ms, double* flops, int64_t* count);
int ramp_workspace_bytes(ramp_ctx* ctx, int64_t* bytes);
int ramp_launch_count(ramp_ctx* ctx, int64_t* kernels_last_score);

#ifdef __cplusplus
}
#endif
#endif /* RAMP_HIP_H */
