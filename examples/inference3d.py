#!/usr/bin/env python3
"""Drop-in counterpart of the reference's scripts/inference/inference3d.py (main, lines 19-156) on the MI355X-native
sampler: Maze3D, GaussianDiffusionModel3d (classifier-free guidance w = 5.75), 3-D scene encoder.

Same flow, same calls (``mpd.*`` -> ``ramp_amd.*``):

    data = dataset[traj_id]: obstacle_points (n_obstacles, n_points, 3), box / sphere centres and sizes           :38-47
    get_model(model_class='GaussianDiffusionModel3d', model=TemporalUnetInference(..., obstacle_3d=True), ...)     :91-113
    load_state_dict(torch.load(<models>/<model_id>/checkpoints/ema_model_current_state_dict.pth))                  :115-118
    start = (-0.8, -0.25, -0.8), goal = (0.8, -0.4, 0.9); hard_conds = dataset.get_hard_conditions(..., normalize) :124-131
    run_inference(context, hard_conds, n_samples, horizon, return_chain=True, obstacle_pts=..., sample_fn=...)     :141-151
    trajs = dataset.unnormalize_trajectories(chain)                                                                :154

(The reference's 3-D wrapper indexes output rows 0 / 1 and is only valid for n_samples = 1; here every
sample gets its own cond / uncond pair, so ``--n-samples N`` equals N independent reference runs.)  Plotting is left out.
``--make-synthetic DIR`` writes an experiment tree in the reference's layout (mpd/datasets/trajectories.py:316-351) first:
``DIR/data/EnvSmall3D/0/{obstacle_points.pt, box_centers.npy, sphere_centers.npy, metadata.yaml}`` and the checkpoint.

    python examples/inference3d.py --make-synthetic /tmp/ramp_exp3d --n-samples 8

``--evaluate`` (opt-in; the reference only plots the boxes and spheres) tests the final batch against them, at the waypoints and on the
segments between them, and picks a free trajectory: ``Metrics3d.evaluate_scenes`` + ``select_best_clear_scenes``, one more JSON line.
``--guide-obstacles`` (opt-in; the reference's guide is a stub) guides the samples against the same boxes and spheres inside the job, segments
included, with the margin ``--evaluate`` uses: the swept primitive term of ``cost_guide=`` (``obstacle_guide`` below).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from math import ceil

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from ramp_amd import compat, synth  # noqa: E402
from ramp_amd.models import UNET_DIM_MULTS, TemporalUnetInference  # noqa: E402
from ramp_amd.sample_functions import ddpm_sample_fn  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.trainer import get_model  # noqa: E402


class Config3d:
    """The fields of the reference's config/base_config.py Config3d that the script reads."""
    device = "cuda"
    seed = 0
    dataset_subdir = "EnvSmall3D"
    trained_models_dir = ""
    dataset_path = ""
    model_id = "synthetic3d"
    use_ema = True
    diffusion_model_class = "GaussianDiffusionModel3d"
    variance_schedule = "exponential"
    n_diffusion_steps = 25
    predict_epsilon = True
    compose = False
    unet_input_dim = 32
    unet_dim_mults_option = 1
    include_velocity = True
    n_samples = 1
    n_support_points = 48
    state_dim = 6
    n_guide_steps = 1
    start_guide_steps_fraction = 0.07
    n_diffusion_steps_without_noise = 0
    trajectory_duration = 5.0


def make_synthetic_experiment(root: str, cfg: Config3d, cloud=None, n_obstacles: int = 20, n_points: int = 200, seed: int = 43) -> None:
    import yaml
    from ramp_amd.models import GaussianDiffusionModel3d
    env_dir = os.path.join(root, "data", cfg.dataset_subdir, "0")
    os.makedirs(env_dir, exist_ok=True)
    cloud = synth.make_cloud(n_obstacles, n_points, 3, seed=seed) if cloud is None else np.asarray(cloud, np.float32)
    n_obstacles = cloud.shape[0]
    torch.save(torch.from_numpy(cloud), os.path.join(env_dir, "obstacle_points.pt"))
    centres = cloud.mean(axis=1).astype(np.float32)
    np.save(os.path.join(env_dir, "box_centers.npy"), centres[: n_obstacles // 2])
    np.save(os.path.join(env_dir, "sphere_centers.npy"), centres[n_obstacles // 2:])
    with open(os.path.join(env_dir, "metadata.yaml"), "w") as fh:
        yaml.safe_dump({"box_sizes": [[0.26, 0.26, 0.26]] * (n_obstacles // 2), "sphere_radii": [0.1] * (n_obstacles - n_obstacles // 2),
                        "limits": [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]}, fh)
    sp = make_unet_spec(cfg.state_dim, cfg.n_support_points, cfg.unet_input_dim, UNET_DIM_MULTS[cfg.unet_dim_mults_option], obstacle_3d=True)
    dm = GaussianDiffusionModel3d(model=TemporalUnetInference(n_support_points=cfg.n_support_points, state_dim=cfg.state_dim,
                                                               unet_input_dim=cfg.unet_input_dim, dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option], obstacle_3d=True),
                                  variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps, predict_epsilon=True)
    full = dm.state_dict()
    for k, v in synth.make_unet_state_dict(sp, seed=0).items():
        full["model." + k] = torch.from_numpy(np.asarray(v))
    ck = os.path.join(root, "models", cfg.model_id, "checkpoints")
    os.makedirs(ck, exist_ok=True)
    torch.save(full, os.path.join(ck, "ema_model_current_state_dict.pth"))


class Dataset3dView:
    """What the script uses of TrajectoryDataset3d (mpd/datasets/trajectories.py): the item's tensors, the limits
    normaliser (normalization.py:144-167) behind get_hard_conditions / unnormalize_trajectories, state_dim, n_support_points."""

    def __init__(self, env_dir: str, cfg: Config3d):
        import yaml
        self.state_dim, self.n_support_points = cfg.state_dim, cfg.n_support_points
        self.item = {"obstacle_points": torch.load(os.path.join(env_dir, "obstacle_points.pt"), map_location="cpu"),
                     "box_centers": np.load(os.path.join(env_dir, "box_centers.npy")),
                     "sphere_centers": np.load(os.path.join(env_dir, "sphere_centers.npy")),
                     "traj_normalized": torch.zeros(cfg.n_support_points, cfg.state_dim)}
        with open(os.path.join(env_dir, "metadata.yaml")) as fh:
            meta = yaml.safe_load(fh)
        self.item["box_sizes"] = torch.tensor(meta["box_sizes"]); self.item["sphere_radii"] = torch.tensor(meta["sphere_radii"])
        lo, hi = meta["limits"]
        z = [0.0] * 3 if cfg.include_velocity else []
        vmax = [1.0] * 3 if cfg.include_velocity else []
        self.normalizer = compat.LimitsNormalizer(lo + [-v for v in vmax], hi + vmax)     # positions | velocities

    def get_hard_conditions(self, pos: torch.Tensor, normalize: bool = True):
        start, goal = pos[0], pos[-1]
        start = torch.cat((start, torch.zeros_like(start))); goal = torch.cat((goal, torch.zeros_like(goal)))
        if normalize:
            self.normalizer.to(start.device)
            start, goal = self.normalizer.normalize(start), self.normalizer.normalize(goal)
        return {0: start, self.n_support_points - 1: goal}

    def unnormalize_trajectories(self, x: torch.Tensor):
        self.normalizer.to(x.device)
        return self.normalizer.unnormalize(x)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--make-synthetic", metavar="DIR"); ap.add_argument("--dataset-path"); ap.add_argument("--trained-models-dir")
    ap.add_argument("--model-id", default=Config3d.model_id); ap.add_argument("--env", type=int, default=0)
    ap.add_argument("--n-samples", type=int, default=Config3d.n_samples)
    ap.add_argument("--n-diffusion-steps", type=int, default=Config3d.n_diffusion_steps)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--unet-input-dim", type=int, choices=[16, 32, 64], default=Config3d.unet_input_dim)
    ap.add_argument("--unet-dim-mults-option", type=int, choices=sorted(UNET_DIM_MULTS), default=Config3d.unet_dim_mults_option)
    ap.add_argument("--evaluate", action="store_true",
                    help="evaluate the batch against the experiment's boxes and spheres, waypoints and segments (Metrics3d), and pick a winner")
    ap.add_argument("--guide-obstacles", action="store_true",
                    help="guide the samples away from the experiment's boxes and spheres inside the job: the swept primitive term of cost_guide= "
                         "(segments included, the margin --evaluate uses)")
    ap.add_argument("--alternatives", type=int, default=0, metavar="K",
                    help="with --evaluate: K free plans that are pairwise at least --min-sep apart, cheapest first, and how many free samples "
                         "are nearest to each (select_diverse_clear_scenes)")
    ap.add_argument("--min-sep", type=float, default=0.1, help="mean waypoint distance two of the --alternatives keep from each other")
    ap.add_argument("--warm-start", default=None, metavar="{line,FILE}",
                    help="start from a prior instead of pure noise: the straight line from start to goal, or a .pt file of normalised trajectories")
    ap.add_argument("--warm-level", type=int, default=None, metavar="T", help="the diffusion level the prior is noised to (0 .. n_diffusion_steps - 1)")
    args = ap.parse_args(argv)
    if args.alternatives and not args.evaluate:
        ap.error("--alternatives goes with --evaluate")
    if (args.warm_start is None) != (args.warm_level is None):
        ap.error("--warm-start and --warm-level go together")
    cfg = Config3d(); cfg.n_samples, cfg.n_diffusion_steps, cfg.model_id, cfg.seed = args.n_samples, args.n_diffusion_steps, args.model_id, args.seed
    cfg.unet_input_dim, cfg.unet_dim_mults_option = args.unet_input_dim, args.unet_dim_mults_option
    if args.make_synthetic:
        make_synthetic_experiment(args.make_synthetic, cfg, cloud=getattr(main, "synthetic_cloud", None))
        cfg.dataset_path = os.path.join(args.make_synthetic, "data"); cfg.trained_models_dir = os.path.join(args.make_synthetic, "models")
    else:
        if not (args.dataset_path and args.trained_models_dir):
            ap.error("--dataset-path and --trained-models-dir (or --make-synthetic DIR) are required")
        cfg.dataset_path, cfg.trained_models_dir = args.dataset_path, args.trained_models_dir
    tensor_args = {'device': cfg.device, 'dtype': torch.float32}
    dataset = Dataset3dView(os.path.join(cfg.dataset_path, cfg.dataset_subdir, str(args.env)), cfg)
    data = dataset.item
    obstacle_pts, traj_normalized = data["obstacle_points"], data["traj_normalized"]
    n_support_points = dataset.n_support_points
    diffusion_configs = dict(variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps,
                             predict_epsilon=cfg.predict_epsilon, training=False, compose=cfg.compose)
    unet_configs = dict(state_dim=dataset.state_dim, n_support_points=n_support_points, unet_input_dim=cfg.unet_input_dim,
                        dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option], obstacle_3d=True)
    model = get_model(model_class=cfg.diffusion_model_class, model=TemporalUnetInference(max_rows=2 * cfg.n_samples, **unet_configs),
                      tensor_args=tensor_args, **diffusion_configs, **unet_configs)
    compat.load_checkpoint(model, cfg.trained_models_dir, cfg.model_id, use_ema=cfg.use_ema, device="cpu")
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    start_state_pos = torch.tensor([-0.8, -0.25, -0.8]).to(cfg.device)        # inference3d.py:124-125
    goal_state_pos = torch.tensor([0.8, -0.4, 0.9]).to(cfg.device)
    hard_conds = dataset.get_hard_conditions(torch.vstack((start_state_pos, goal_state_pos)), normalize=True)
    context = {'dataset': dataset}
    t_start_guide = ceil(cfg.start_guide_steps_fraction * model.n_diffusion_steps)
    sample_fn_kwargs = dict(guide=None, n_guide_steps=cfg.n_guide_steps, t_start_guide=t_start_guide, noise_std_extra_schedule_fn=lambda x: 0.5)
    if args.guide_obstacles:
        sample_fn_kwargs["cost_guide"] = obstacle_guide(data, dataset.normalizer, t_start=t_start_guide)
    if args.warm_start is not None:      # (hard_conds holds the normalised start and goal states)
        from ramp_amd.warm import straight_line_prior
        prior = (straight_line_prior(hard_conds[0].detach().cpu().numpy(), hard_conds[n_support_points - 1].detach().cpu().numpy(), n_support_points)
                 if args.warm_start == "line" else torch.load(args.warm_start, map_location="cpu"))
        sample_fn_kwargs["warm_start"] = dict(prior=prior, level=args.warm_level)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    trajs_normalized_iters = model.run_inference(context, hard_conds, n_samples=cfg.n_samples, horizon=n_support_points, return_chain=True,
                                                 traj_normalized=traj_normalized, obstacle_pts=obstacle_pts, sample_fn=ddpm_sample_fn,
                                                 **sample_fn_kwargs, n_diffusion_steps_without_noise=cfg.n_diffusion_steps_without_noise)
    torch.cuda.synchronize(); elapsed = time.perf_counter() - t0
    trajs_iters = dataset.unnormalize_trajectories(trajs_normalized_iters)
    pos_final = trajs_iters[-1][..., :3]                                       # robot.get_position
    out = {"n_chain_states": int(trajs_normalized_iters.shape[0]), "n_samples": int(pos_final.shape[0]), "total_time": elapsed,
           "start_error": float((pos_final[:, 0] - start_state_pos).abs().max()), "goal_error": float((pos_final[:, -1] - goal_state_pos).abs().max())}
    print(json.dumps(out))
    if args.evaluate:
        out["evaluation"] = evaluate(trajs_iters[-1], data, alternatives=args.alternatives, min_sep=args.min_sep)
        print(json.dumps({"evaluation": out["evaluation"]}))
    return out, trajs_normalized_iters


EVAL_MARGIN = 0.0      # the robot radius --evaluate widens the boxes and spheres by; --guide-obstacles guides against the same


def obstacle_guide(data, normalizer, margin: float = EVAL_MARGIN, band: float = 0.05, step: float = 0.5, n_steps: int = 8, n_sub: int = 4,
                   t_start: float = float("inf")) -> dict:
    """``cost_guide=`` against the experiment's own boxes and spheres (the primitives-only guide: no cloud term), in the normalised
    coordinates the sampler works in: the limits normaliser is x -> 2 (x - lo) / (hi - lo) - 1 per axis, so a box keeps its shape; a sphere
    does only where the three position axes share one scale, which is asked for.  ``t_start``: the reverse steps with t < t_start are
    guided -- the script hands over the t_start_guide the reference computes and never uses."""
    lo, hi = (torch.as_tensor(v, dtype=torch.float32).cpu()[:3] for v in (normalizer.mins, normalizer.maxs))
    scale = 2.0 / (hi - lo)
    if not torch.allclose(scale, scale[0].expand(3)):
        raise NotImplementedError("--guide-obstacles: the normaliser scales the position axes differently (spheres would become ellipsoids)")
    norm = lambda c: (torch.as_tensor(c, dtype=torch.float32) - lo) * scale - 1.0      # noqa: E731
    sizes = torch.as_tensor(data["box_sizes"], dtype=torch.float32)
    boxes = (norm(data["box_centers"]), sizes * (scale if sizes.dim() == 2 else scale[0]))
    spheres = (norm(data["sphere_centers"]), torch.as_tensor(data["sphere_radii"], dtype=torch.float32) * scale[0])
    return dict(cloud=None, w_obs=0.0, boxes=boxes, spheres=spheres, margin=margin * float(scale[0]), band=band, step=step, n_steps=n_steps,
                n_sub=n_sub, t_start=t_start)


def evaluate(trajs_final, data, threshold: float = 0.01, alternatives: int = 0, min_sep: float = 0.1):
    """What the reference's script leaves out: are the sampled trajectories free of the experiment's boxes and spheres -- at the
    waypoints and on the segments between them -- and which free one to execute.  ``alternatives`` = K > 0 adds the rows of K free plans
    that are pairwise at least ``min_sep`` apart (the first is ``best_row``) and the number of free samples nearest to each."""
    from ramp_amd.cost import select_best_clear_scenes, select_diverse_clear_scenes
    from ramp_amd.metrics import Metrics3d
    boxes = (torch.as_tensor(data["box_centers"]), torch.as_tensor(data["box_sizes"]))
    spheres = (torch.as_tensor(data["sphere_centers"]), torch.as_tensor(data["sphere_radii"]))
    n = trajs_final.shape[0]
    per_scene, free = Metrics3d.evaluate_scenes(trajs_final, [n], [boxes], [spheres], threshold=threshold, swept=True, margin=EVAL_MARGIN)
    _, n_free, _, best_row, _ = select_best_clear_scenes(trajs_final, [n], boxes=boxes, spheres=spheres, point_dim=3, swept=True,
                                                         intensity_threshold=threshold)
    m = per_scene[0]
    ev = {"success": m["success"], "collision_intensity": m["collision_intensity"],
          "swept_collision_intensity": m["swept_collision_intensity"], "n_free_trajectories": m["n_free_trajectories"],
          "path_length": m["path_length"], "best_row": int(best_row[0]), "n_free_selected": int(n_free[0])}
    if alternatives:
        sel = select_diverse_clear_scenes(trajs_final, [n], boxes=boxes, spheres=spheres, k=alternatives, min_sep=min_sep, point_dim=3,
                                          swept=True, intensity_threshold=threshold)
        ev["alternative_rows"] = sel.rows[0].tolist()
        ev["mode_count"] = sel.mode_count[0].tolist()
    return ev


if __name__ == "__main__":
    main()
