"""ctypes binding of libramp_hip.so (the C ABI declared in include/ramp_hip.h).

There is no CPU fallback: if the library is missing, or fails to load, every use raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libramp_hip.so")
TOOLS_LIB_PATH = os.path.join(HERE, "lib", "libramp_hip_tools.so")

c_f32p = C.POINTER(C.c_float)
c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)


class RampConfig(C.Structure):
    _fields_ = [("state_dim", C.c_int32), ("horizon", C.c_int32), ("unet_input_dim", C.c_int32),
                ("n_levels", C.c_int32), ("context_dim", C.c_int32), ("max_rows", C.c_int32),
                ("debug_taps", C.c_int32), ("gemm_mode", C.c_int32)]


class RampLaunchPlan(C.Structure):
    _fields_ = [("ff_fused_rows", C.c_int32), ("ffx_rows", C.c_int32), ("share_prefix", C.c_int32),
                ("three_blocks", C.c_int32), ("x6_pipe", C.c_int32), ("tkl_rows", C.c_int32), ("atk_rows", C.c_int32),
                ("tkc_rows", C.c_int32), ("tkw_rows", C.c_int32), ("mfma16", C.c_int32)]


class RampApfParams(C.Structure):
    _fields_ = [("cloud", C.c_void_p), ("n_points", C.c_int32), ("window", C.c_int32),
                ("window_weights_host", c_f32p), ("threshold", C.c_double), ("strength", C.c_double),
                ("passes", C.c_int32), ("reserved", C.c_int32)]


class RampSceneBatch(C.Structure):
    """ramp_scene_batch: the scenes of a many-scene job (ramp_sample_scenes, ramp_apf_scenes)."""
    _fields_ = [("n_scenes", C.c_int32), ("reserved", C.c_int32), ("traj_scene", C.c_void_p), ("cloud_points", C.c_void_p),
                ("cloud_offset_host", c_i32p)]


class RampGuidanceRows(C.Structure):
    """ramp_guidance_rows: the per-trajectory guidance weights of a composed job (ramp_sample_composed)."""
    _fields_ = [("n_rp", C.c_int32), ("reserved", C.c_int32), ("row_weight", C.c_void_p)]


MAX_ROWS_PER_TRAJ = 8       # RAMP_MAX_ROWS_PER_TRAJ
MCMC_MAX_INNER = 16         # RAMP_MCMC_MAX_INNER
MCMC_KINDS = {'ula': 1, 'mala': 2}


class RampMcmcParams(C.Structure):
    """ramp_mcmc_params: the Langevin refinement of a sampling job (ramp_sample_mcmc)."""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("n_inner", c_i32p), ("step_size", c_f32p), ("sigma", c_f32p)]


GUIDE_MAX_STEPS = 16        # RAMP_GUIDE_MAX_STEPS


class RampCostGuide(C.Structure):
    """ramp_cost_guide: the cost-gradient guidance of a sampling job (ramp_sample_guided) and of the kernel-level ramp_guide_step / ramp_guide_cost."""
    _fields_ = [("point_dim", C.c_int32), ("n_scenes", C.c_int32), ("cloud_points", C.c_void_p), ("cloud_offset_host", c_i32p),
                ("radius", C.c_double), ("w_obs", C.c_double), ("w_smooth", C.c_double), ("w_acc", C.c_double), ("max_norm", C.c_double),
                ("n_guide", c_i32p), ("step", c_f32p)]


PRIM_GUIDE_MAX_SUB = 8      # RAMP_PRIM_GUIDE_MAX_SUB


class RampPrimGuide(C.Structure):
    """ramp_prim_guide: the swept box and sphere terms that travel with a ramp_cost_guide (ramp_sample_guided_prims) and the kernel-level
    ramp_guide_step_prims / ramp_guide_cost_prims."""
    _fields_ = [("point_dim", C.c_int32), ("n_scenes", C.c_int32), ("box_centers", C.c_void_p), ("box_sizes", C.c_void_p),
                ("sphere_centers", C.c_void_p), ("sphere_radii", C.c_void_p), ("box_offset_host", c_i32p), ("sphere_offset_host", c_i32p),
                ("margin", C.c_double), ("band", C.c_double), ("w_prim", C.c_double), ("n_sub", C.c_int32), ("reserved", C.c_int32)]


TEAM_MAX = 8                # RAMP_TEAM_MAX


class RampTeamGuide(C.Structure):
    """ramp_team_guide: the separation term between the rows of a team that travels with a ramp_cost_guide (ramp_sample_guided_team) and the
    kernel-level ramp_guide_step_team / ramp_guide_cost_team."""
    _fields_ = [("team_size", C.c_int32), ("reserved", C.c_int32), ("radius_team", C.c_double), ("w_team", C.c_double)]


STITCH_MAX_PINS = 64        # RAMP_STITCH_MAX_PINS


class RampStitch(C.Structure):
    """ramp_stitch: the stitch table of a job on stitched windows (ramp_sample_stitched) and of the kernel-level ramp_stitch_windows."""
    _fields_ = [("n_windows", C.c_int32), ("overlap", C.c_int32), ("alpha_host", c_f32p), ("n_pin", C.c_int32), ("reserved", C.c_int32),
                ("pin_idx_host", c_i32p), ("pin_val", C.c_void_p)]


class RampWarmStart(C.Structure):
    """ramp_warm_start: the rows' priors and levels of a warm-started job (ramp_sample_warm)."""
    _fields_ = [("prior", C.c_void_p), ("j0_host", c_i32p), ("has_prior_host", c_i32p), ("sa_host", c_f32p), ("s1a_host", c_f32p),
                ("n_hold", C.c_int32), ("reserved", C.c_int32)]


class RampReplanGuide(C.Structure):
    """ramp_replan_guide: the cost guide of the replanning jobs (ramp_replan_guided, ramp_replan_episodes_guided) and of the kernel-level
    ramp_guide_step_moving / ramp_guide_cost_moving."""
    _fields_ = [("n_scenes", C.c_int32), ("n_mov", C.c_int32), ("cloud_points", C.c_void_p), ("cloud_offset_host", c_i32p),
                ("mov_points_host", c_f32p), ("mov_track_host", c_f32p),
                ("radius", C.c_double), ("radius_mov", C.c_double), ("w_obs", C.c_double), ("w_mov", C.c_double), ("w_smooth", C.c_double),
                ("w_acc", C.c_double), ("max_norm", C.c_double), ("n_guide", c_i32p), ("step", c_f32p), ("tap_out", C.c_void_p)]


class RampObstacles(C.Structure):
    """ramp_obstacles: the boxes, spheres and cloud points of the scenes ramp_traj_clearance tests trajectories against."""
    _fields_ = [("point_dim", C.c_int32), ("n_scenes", C.c_int32), ("box_centers", C.c_void_p), ("box_sizes", C.c_void_p),
                ("sphere_centers", C.c_void_p), ("sphere_radii", C.c_void_p), ("cloud", C.c_void_p), ("box_offset", C.c_void_p),
                ("sphere_offset", C.c_void_p), ("cloud_offset", C.c_void_p), ("n_boxes_total", C.c_int32), ("n_spheres_total", C.c_int32),
                ("n_points_total", C.c_int32), ("margin", C.c_float)]


RESAMPLE_MAX_EVENTS = 64   # RAMP_RESAMPLE_MAX_EVENTS
c_f64p = C.POINTER(C.c_double)


class RampResampleParams(C.Structure):
    """ramp_resample_params: the resampling events of a sampling job (ramp_sample_steered)."""
    _fields_ = [("n_groups", C.c_int32), ("group0", C.c_int32), ("groups_total", C.c_int32), ("reserved", C.c_int32),
                ("group_first_host", c_i32p), ("resample", c_i32p), ("lambda_", c_f64p), ("ess_frac", C.c_double),
                ("cost", C.POINTER(RampCostGuide))]


class RampSampleParams(C.Structure):
    _fields_ = [("B", C.c_int32), ("n_rp", C.c_int32), ("n_steps", C.c_int32), ("ddim", C.c_int32),
                ("w0", C.c_double), ("w1", C.c_double),
                ("t", c_i32p), ("sqrt_recip", c_f32p), ("sqrt_recipm1", c_f32p), ("coef1", c_f32p),
                ("coef2", c_f32p), ("stdv", c_f32p), ("use_noise", c_i32p), ("sqrt_a_t", c_f32p),
                ("sqrt_1m_a_t", c_f32p), ("sqrt_a_prev", c_f32p), ("dir_coef", c_f32p), ("apply_apf", c_i32p),
                ("noise_scale", c_f32p), ("clip_denoised", C.c_int32), ("predict_x0", C.c_int32),
                ("n_hard", C.c_int32), ("hard_idx_host", c_i32p), ("hard_val", C.c_void_p),
                ("apf", RampApfParams), ("use_graph", C.c_int32), ("reserved", C.c_int32),
                ("noise_mode", C.c_int32), ("reserved2", C.c_int32), ("philox_seed", C.c_uint64), ("philox_offset", C.c_uint64),
                ("philox_sample0", C.c_int64), ("philox_total", C.c_int64)]


class RampReplanParams(C.Structure):
    _fields_ = [("B", C.c_int32), ("n_rp", C.c_int32), ("n_steps", C.c_int32), ("clip_denoised", C.c_int32),
                ("w", C.c_double), ("t", c_i32p), ("sqrt_recip", c_f32p), ("sqrt_recipm1", c_f32p), ("sqrt_a_t", c_f32p),
                ("sqrt_1m_a_t", c_f32p), ("sqrt_a_prev", c_f32p), ("dir_coef", c_f32p), ("q_sqrt_a", C.c_float),
                ("q_sqrt_1m_a", C.c_float), ("n_hard", C.c_int32), ("predict_x0", C.c_int32), ("hard_idx_host", c_i32p),
                ("hard_val", C.c_void_p), ("sm_window_last", C.c_int32), ("sm_window_final", C.c_int32),
                ("sm_dt", C.c_float), ("sm_max_vel", C.c_float), ("static_pts", C.c_void_p), ("n_static", C.c_int32),
                ("n_dyn", C.c_int32), ("thr_static", C.c_double), ("thr_pred", C.c_double), ("strength_static", C.c_double),
                ("strength_pred", C.c_double), ("window_static", C.c_int32), ("n_cost", C.c_int32),
                ("cost_cloud", C.c_void_p), ("n_extra", C.c_int32), ("cost_thr", C.c_float), ("w_smooth", C.c_float),
                ("w_len", C.c_float), ("use_graph", C.c_int32)]


class RampReplanState(C.Structure):
    _fields_ = [("noise", C.c_void_p), ("x_clean", C.c_void_p), ("history", C.c_void_p), ("n_hist", C.c_int32),
                ("stepp", C.c_int32), ("dyn_pts_host", C.c_void_p), ("pursuer", C.c_float * 2), ("near", C.c_int32),
                ("reserved", C.c_int32), ("extra_pts_host", C.c_void_p)]


class RampEpisodeState(C.Structure):
    """ramp_episode_state: what differs between the episodes of a many-episode replan (32 bytes, the device record's layout)."""
    _fields_ = [("n_hist", C.c_int32), ("stepp", C.c_int32), ("active", C.c_int32), ("reserved", C.c_int32),
                ("pursuer", C.c_float * 2), ("reserved2", C.c_float * 2)]


class RampEpisodeBatch(C.Structure):
    """ramp_episode_batch: the per-episode inputs of ramp_replan_episodes."""
    _fields_ = [("n_episodes", C.c_int32), ("reserved", C.c_int32), ("traj_first_host", c_i32p), ("noise", C.c_void_p),
                ("x_clean", C.c_void_p), ("history", C.c_void_p), ("state_host", C.POINTER(RampEpisodeState)),
                ("static_pts", C.c_void_p), ("static_offset_host", c_i32p), ("dyn_pts_host", C.c_void_p),
                ("cost_cloud", C.c_void_p), ("cost_offset_host", c_i32p), ("near_host", c_i32p), ("extra_pts_host", C.c_void_p)]


class RampProbeGemmArgs(C.Structure):
    """ramp_probe_gemm_args (include/ramp_hip_tools.h): the operand fields of the engine's GEMM launch arguments."""
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int32), ("A2", C.c_void_p), ("lda2", C.c_int32), ("K1", C.c_int32),
                ("W", C.c_void_p), ("bias", C.c_void_p), ("rowbias", C.c_void_p), ("rowvar", C.c_void_p), ("row0", C.c_int32),
                ("rb_stride", C.c_int32), ("resid", C.c_void_p), ("ldr", C.c_int32), ("resid2", C.c_void_p), ("ldr2", C.c_int32),
                ("C", C.c_void_p), ("ldc", C.c_int32), ("C2", C.c_void_p), ("ldc2", C.c_int32), ("N1", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("taps", C.c_int32), ("shift0", C.c_int32),
                ("shift_step", C.c_int32), ("L", C.c_int32), ("a_stride", C.c_int32), ("c_rstride", C.c_int32),
                ("c_roff", C.c_int32)]


class RampReplanResult(C.Structure):
    _fields_ = [("n_free", C.c_int32), ("best_rank", C.c_int32), ("best_row", C.c_int32), ("fell_back", C.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/ramp_hip.h
PROTOTYPES = {
    "ramp_last_error": (C.c_char_p, []),
    "ramp_version": (C.c_int, []),
    "ramp_create": (C.c_int, [C.POINTER(RampConfig), C.POINTER(C.c_void_p)]),
    "ramp_destroy": (C.c_int, [C.c_void_p]),
    "ramp_get_launch_plan": (C.c_int, [C.c_void_p, C.POINTER(RampLaunchPlan)]),
    "ramp_set_launch_plan": (C.c_int, [C.c_void_p, C.POINTER(RampLaunchPlan)]),
    "ramp_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, c_f32p, c_i64p, C.c_int32]),
    "ramp_finalize_weights": (C.c_int, [C.c_void_p]),
    "ramp_prepare_time_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ramp_time_embedding": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ramp_set_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_i32p, C.c_int32, C.c_void_p]),
    "ramp_set_scenes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, c_i32p, C.c_int32, C.c_void_p]),
    "ramp_encode_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ramp_encode_scenes": (C.c_int, [C.c_void_p, C.c_void_p, c_i32p, c_i32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, c_i32p,
                                     C.c_void_p]),
    "ramp_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                             C.c_void_p]),
    "ramp_score_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, c_i32p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "ramp_score_mode": (C.c_int, [C.c_void_p, c_i32p]),
    "ramp_sample": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p]),
    "ramp_sample_scenes": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampSceneBatch), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "ramp_sample_composed": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_sample_mcmc": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampMcmcParams), C.POINTER(RampGuidanceRows),
                                   C.POINTER(RampSceneBatch)] + [C.c_void_p] * 7),
    "ramp_sample_guided": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampCostGuide), C.POINTER(RampMcmcParams),
                                     C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch)] + [C.c_void_p] * 7),
    "ramp_sample_steered": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampResampleParams), C.POINTER(RampCostGuide),
                                      C.POINTER(RampMcmcParams), C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch)] + [C.c_void_p] * 12),
    "ramp_resample_groups": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, c_i32p, C.c_int32, C.c_void_p,
                                       C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_guide_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.c_void_p, C.c_int32, C.c_float,
                                  C.c_int32, c_i32p, C.c_void_p, C.c_void_p]),
    "ramp_guide_cost": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_sample_guided_prims": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampCostGuide), C.POINTER(RampPrimGuide),
                                           C.POINTER(RampMcmcParams), C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch)] + [C.c_void_p] * 7),
    "ramp_guide_step_prims": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.POINTER(RampPrimGuide), C.c_void_p,
                                        C.c_int32, C.c_float, C.c_int32, c_i32p, C.c_void_p, C.c_void_p]),
    "ramp_guide_cost_prims": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.POINTER(RampPrimGuide), C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "ramp_sample_guided_team": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampCostGuide), C.POINTER(RampTeamGuide),
                                          C.POINTER(RampMcmcParams), C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch)] + [C.c_void_p] * 7),
    "ramp_guide_step_team": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.POINTER(RampTeamGuide), C.c_void_p,
                                       C.c_int32, C.c_float, C.c_int32, c_i32p, C.c_void_p, C.c_void_p]),
    "ramp_guide_cost_team": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampCostGuide), C.POINTER(RampTeamGuide), C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "ramp_team_clearance": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_float, C.c_int32] + [C.c_void_p] * 11),
    "ramp_sample_stitched": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampStitch), C.POINTER(RampCostGuide),
                                       C.POINTER(RampSceneBatch)] + [C.c_void_p] * 5),
    "ramp_sample_warm": (C.c_int, [C.c_void_p, C.POINTER(RampSampleParams), C.POINTER(RampWarmStart), C.POINTER(RampStitch),
                                   C.POINTER(RampResampleParams), C.POINTER(RampCostGuide), C.POINTER(RampPrimGuide), C.POINTER(RampTeamGuide),
                                   C.POINTER(RampMcmcParams), C.POINTER(RampGuidanceRows), C.POINTER(RampSceneBatch)] + [C.c_void_p] * 13),
    "ramp_warm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f32p, c_f32p, c_i32p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_warm_hold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_i32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_stitch_windows": (C.c_int,[C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampStitch), C.c_void_p]),
    "ramp_stitch_assemble": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "ramp_score_energy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "ramp_row_energy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ramp_combine_energy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, c_f32p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_mcmc_propose": (C.c_int, [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p]),
    "ramp_mcmc_accept": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_float, C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                                       C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p]),
    "ramp_philox_normal": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]),
    "ramp_replan": (C.c_int, [C.c_void_p, C.POINTER(RampReplanParams), C.POINTER(RampReplanState), C.c_void_p, C.c_void_p,
                              C.c_void_p, C.POINTER(RampReplanResult), C.c_void_p]),
    "ramp_replan_episodes": (C.c_int, [C.c_void_p, C.POINTER(RampReplanParams), C.POINTER(RampEpisodeBatch), C.c_void_p, C.c_void_p,
                                       C.c_void_p, c_i32p, C.POINTER(RampReplanResult), C.c_void_p]),
    "ramp_replan_guided": (C.c_int, [C.c_void_p, C.POINTER(RampReplanParams), C.POINTER(RampReplanState), C.POINTER(RampReplanGuide), C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(RampReplanResult), C.c_void_p]),
    "ramp_replan_episodes_guided": (C.c_int, [C.c_void_p, C.POINTER(RampReplanParams), C.POINTER(RampEpisodeBatch), C.POINTER(RampReplanGuide),
                                              C.c_void_p, C.c_void_p, C.c_void_p, c_i32p, C.POINTER(RampReplanResult), C.c_void_p]),
    "ramp_guide_step_moving": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampReplanGuide), C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_float, C.c_int32, c_i32p, C.c_void_p, C.c_void_p]),
    "ramp_guide_cost_moving": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampReplanGuide), C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "ramp_select_best": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float, C.c_float,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_replan_costs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_select_from_costs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                         C.c_void_p]),
    "ramp_apf": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampApfParams), C.c_void_p]),
    "ramp_apf_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampApfParams),
                                  C.POINTER(RampSceneBatch), C.c_void_p]),
    "ramp_apf_dynamic": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                   C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_hard_cond": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32p, C.c_void_p,
                                 C.c_void_p]),
    "ramp_traj_metrics": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_waypoint_variance": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_q_sample_rows": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_denoise_loss": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p] * 3),
    "ramp_traj_costs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_traj_metrics_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_scene_summary": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_traj_costs_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_select_best_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "ramp_scene_summary_nd": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_select_scored_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_select_diverse_scenes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_int32] +
                                   [C.c_void_p] * 8),
    "ramp_traj_clearance": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RampObstacles), C.c_void_p, C.c_int32] +
                            [C.c_void_p] * 7),
    "ramp_cfg_mean": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "ramp_cfg_mean_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "ramp_ddim_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_gemm": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 7 + [C.c_void_p]),
    "ramp_op_gemm_mode": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 8 + [C.c_float, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_ffx": (C.c_int, [C.c_void_p] * 8 + [C.c_int32, c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_ffx16": (C.c_int, [C.c_void_p] * 8 + [C.c_int32, c_f32p, C.c_void_p, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_tkl": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_tkl16": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_ato": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_atb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_abl": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_float, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_tkw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 11 + [C.c_int32] * 6 + [C.c_float] + [C.c_void_p] * 4 + [c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_tkw_rows": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_void_p] + [C.c_int32] * 4 + [C.c_float] + [C.c_void_p] * 3 + [c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_tklb": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_float, C.c_void_p, c_f32p, c_i32p, C.c_void_p]),
    "ramp_op_groupnorm": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 3 + [C.c_float, C.c_int32, C.c_void_p]),
    "ramp_op_groupnorm_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_float, C.c_int32, C.c_void_p]),
    "ramp_op_groupnorm_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.c_void_p]),
    "ramp_op_layernorm": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "ramp_op_layernorm_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]),
    "ramp_op_geglu": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_geglu_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_scene_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "ramp_op_scene_attention_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "ramp_op_scene_colreduce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_scene_colreduce_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ramp_op_scene_enc2d_prep": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_op_scene_enc2d_prep_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ramp_debug_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int64, c_i64p, C.c_void_p]),
    "ramp_profile": (C.c_int, [C.c_void_p, C.c_int32]),
    "ramp_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), c_i64p]),
    "ramp_profile_read_kernels": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), c_i64p]),
    "ramp_set_fallback": (C.c_int, [C.c_void_p, C.c_int32]),
    "ramp_set_calibration_reuse": (C.c_int, [C.c_void_p, C.c_int32]),
    "ramp_range_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "ramp_range_trip": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ramp_workspace_bytes": (C.c_int, [C.c_void_p, c_i64p]),
    "ramp_launch_count": (C.c_int, [C.c_void_p, c_i64p]),
}

# Diagnostics, exported by ramp_amd/lib/libramp_hip_tools.so only (csrc/bench.hip: the product library carries no harness code)
TOOL_PROTOTYPES = {
    "ramp_bench_gemm": (C.c_int, [C.c_int32] * 9 + [c_f32p, C.c_void_p]),
    "ramp_stress_gemm": (C.c_int, [C.c_int32] * 8 + [c_i64p, c_f32p, C.c_void_p]),
    "ramp_probe_gemm": (C.c_int, [C.POINTER(RampProbeGemmArgs), C.c_int32, C.c_float, c_f32p, c_i32p, C.c_void_p]),
    "ramp_probe_conv_in_fwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 5 + [C.c_void_p]),
    "ramp_probe_conv_in_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]),
    "ramp_probe_conv_out": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 3 + [C.c_void_p]),
    "ramp_probe_expand_rows": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ramp_probe_combine_rows": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 4 + [c_f32p, C.c_void_p]),
    "ramp_probe_combine_rows_weighted": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "ramp_probe_cross_bias": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.POINTER(C.c_void_p)] * 3 + [C.c_int32, C.c_void_p, C.c_void_p]),
    "ramp_probe_time_bias": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
}

_lib: Optional[C.CDLL] = None
_tools: Optional[C.CDLL] = None


class RampHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load libramp_hip.so and bind every prototype.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64; the process must hold ONE HIP runtime (torch's
    # streams and allocations are handed to this library), so torch is always imported first and this library's
    # NEEDED libamdhip64.so.7 then resolves to the copy already mapped.  Loaded the other way round the second
    # runtime finds no device.
    import torch  # noqa: F401
    # RAMP_HIP_LIB: another build of the same library for a same-box A/B (ramp_amd/tools/ab_libs.sh); the in-tree one is never
    # overwritten, so later runs cannot pick up a stale alternate by accident
    path = os.environ.get("RAMP_HIP_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise RampHipError(f"{path} not found: build it with `python -m ramp_amd.build` "
                           "(hipcc --offload-arch=gfx950). The RAMP sampler has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def load_tools() -> C.CDLL:
    """The tools library: every object of the product library plus the micro-benchmark / stress harness (ramp_bench_gemm,
    ramp_stress_gemm; csrc/bench.hip).  For tests/ and ramp_amd/tools/ only -- nothing in the product path imports it."""
    global _tools
    if _tools is not None:
        return _tools
    import torch  # noqa: F401  (one HIP runtime per process: see load())
    path = os.environ.get("RAMP_HIP_TOOLS_LIB") or TOOLS_LIB_PATH
    if not os.path.exists(path):
        raise RampHipError(f"{path} not found: build it with `python -m ramp_amd.build`")
    lib = C.CDLL(path)
    for name, (res, args) in list(PROTOTYPES.items()) + list(TOOL_PROTOTYPES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _tools = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().ramp_last_error()
        raise RampHipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def check_tools(rc: int, what: str = "") -> None:
    """check() for a call made through load_tools() (each library keeps its own thread-local error message)."""
    if rc != 0:
        msg = load_tools().ramp_last_error()
        raise RampHipError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


GEMM_MODES = {"fp32": 0, "bf16x6": 1, "bf16x6-lds": 2, "fp16x3": 3, "fp16x3-tkc": 5}       # ramp_op_gemm_mode


def op_gemm(A, W, bias, resid, out, M, N, K, taps, shift0, step, L, mode="fp32", a_absmax_prev=0.0):
    """ramp_op_gemm_mode on torch tensors; returns (recorded max|A|, range flag) (zeros outside fp16x3)."""
    amax, flag = C.c_float(0.0), C.c_int32(0)
    check(load().ramp_op_gemm_mode(ptr(A), ptr(W), ptr(bias), ptr(resid), ptr(out), M, N, K, taps, shift0, step, L,
                                   GEMM_MODES[mode], float(a_absmax_prev), C.byref(amax), C.byref(flag),
                                   current_stream()), "ramp_op_gemm_mode")
    return amax.value, flag.value


_PROBE_TENSORS = ("A", "A2", "W", "bias", "rowbias", "rowvar", "resid", "resid2", "C", "C2")


def probe_gemm(mode="fp32", a_absmax_prev=0.0, **fields):
    """ramp_probe_gemm (tools library) on torch tensors: `fields` are the ramp_probe_gemm_args members (tensors for the operands,
    ints for the rest; omitted ones are NULL / 0, except taps, L, a_stride and c_rstride, which default to 1).  Returns (rc, recorded max|A|, range
    flag, error message or None) without raising, so that tests can check refusals too."""
    a = RampProbeGemmArgs(taps=1, L=1, a_stride=1, c_rstride=1)
    for k, v in fields.items():
        setattr(a, k, ptr(v) if k in _PROBE_TENSORS else int(v))
    amax, flag = C.c_float(0.0), C.c_int32(0)
    tools = load_tools()
    rc = tools.ramp_probe_gemm(C.byref(a), GEMM_MODES[mode], float(a_absmax_prev), C.byref(amax), C.byref(flag), current_stream())
    msg = None
    if rc != 0:
        m = tools.ramp_last_error()
        msg = m.decode() if m else ""
    return rc, amax.value, flag.value, msg


def _probe(name, *args):
    """One ramp_probe_* call of the tools library (args before the stream); (rc, error message or None) without raising, so that tests
    can check refusals too."""
    tools = load_tools()
    rc = getattr(tools, name)(*args, current_stream())
    msg = None
    if rc != 0:
        m = tools.ramp_last_error()
        msg = m.decode() if m else ""
    return rc, msg


def probe_conv_in_fwd(x, W5, b5, W1, b1, c1, res, R, n_rp, H, S, C0):
    """launch_conv_in_fwd on torch tensors: W5 packed [5][S][C0], W1 [S][C0]."""
    return _probe("ramp_probe_conv_in_fwd", ptr(x), ptr(W5), ptr(b5), ptr(W1), ptr(b1), ptr(c1), ptr(res), R, n_rp, H, S, C0)


def probe_conv_in_bwd(dc1, dy, W5, W1, eps, R, H, S, C0):
    return _probe("ramp_probe_conv_in_bwd", ptr(dc1), ptr(dy), ptr(W5), ptr(W1), ptr(eps), R, H, S, C0)


def probe_conv_out(a, Wf, bf, f, da, n_tok, S, C0):
    """launch_conv_out: Wf [S][C0]; f or da may be None."""
    return _probe("ramp_probe_conv_out", ptr(a), ptr(Wf), ptr(bf), ptr(f), ptr(da), n_tok, S, C0)


def probe_expand_rows(x, out, R, n_rp, L, Cc, rowbias=None, rb_stride=0, rowvar=None, row0=0):
    return _probe("ramp_probe_expand_rows", ptr(x), ptr(out), R, n_rp, L, Cc, ptr(rowbias), rb_stride, ptr(rowvar), row0)


def probe_combine_rows(x, out, B, n_rp, L, Cc, w):
    """launch_combine_rows: w the host weights (a sequence of floats)."""
    wa = (C.c_float * max(len(w), 1))(*[float(v) for v in w])
    return _probe("ramp_probe_combine_rows", ptr(x), ptr(out), B, n_rp, L, Cc, wa)


def probe_combine_rows_weighted(x, out, B, n_rp, L, Cc, row_weight, weight_offset=0):
    """launch_combine_rows_weighted: row_weight a device tensor, entered `weight_offset` floats in (a chunk's first trajectory)."""
    return _probe("ramp_probe_combine_rows_weighted", ptr(x), ptr(out), B, n_rp, L, Cc, ptr(row_weight) + 4 * int(weight_offset))


def probe_cross_bias(lat, n_var, ctx_dim, wv, wo, bo, out):
    """launch_cross_bias: wv / wo / bo lists of n_blk device tensors."""
    n = len(wv)
    tabs = [(C.c_void_p * n)(*[ptr(t) for t in ts]) for ts in (wv, wo, bo)]
    return _probe("ramp_probe_cross_bias", ptr(lat), n_var, ctx_dim, *tabs, n, ptr(out))


def probe_time_bias(ctx, module, t, out):
    """Block `module`'s slice of line t of the context's prepared time table into out (device, cout floats)."""
    return _probe("ramp_probe_time_bias", ctx, module.encode(), int(t), ptr(out), out.numel())


def ptr(t) -> Optional[int]:
    """Device (or host) address of a contiguous torch tensor, None for None."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def current_stream() -> Optional[int]:
    import torch
    return torch.cuda.current_stream().cuda_stream
