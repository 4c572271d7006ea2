#!/usr/bin/env python3
"""Drop-in counterpart of the reference's scripts/inference/inference_static.py (StaticInference.run_single_experiment,
lines 37-180) on the MI355X-native sampler.

Same flow, same calls, same on-disk layout; only the imports change (``mpd.*`` -> ``ramp_amd.*``):

    get_model(model_class=..., model=TemporalUnetInference(**unet_configs), tensor_args=..., **diffusion_configs)   :99-105
    model.load_state_dict(torch.load(<trained_models_dir>/<model_id>/checkpoints/ema_model_current_state_dict.pth))  :107-111
    model.eval(); model.warmup(horizon, traj_normalized, obstacle_pts, batch_size, device)                           :112-121
    start, goal = ContextManager.load_context(<env_dir>/contexts, context_idx); hard_conds = get_hard_cond_custom()  :123-134
    run_inference(context, hard_conds, n_samples, horizon, return_chain=True, obstacle_pts=..., sample_fn=..., ...)  :146-157
    Metrics.compute_collision_intensity / trajectory_success_and_metrics                                              :159-169

(``torch.compile(mode='reduce-overhead')``, :114, is the reference's way of removing launch overhead; here the whole
reverse-diffusion loop is one captured hipGraph inside ``run_inference``.)

The reference ships neither checkpoints nor datasets, so ``--make-synthetic DIR`` first writes an experiment tree in the
reference's layout -- ``DIR/data/<subdir>/<env>/{obstacle_points.pt, box_centers.npy, metadata.yaml, contexts/context_000.pt}``
and ``DIR/models/<model_id>/checkpoints/ema_model_current_state_dict.pth`` with seeded random weights under the reference's
state-dict keys -- and then runs the experiment on it, exactly as it would on the authors' files.

    python examples/inference_static.py --make-synthetic /tmp/ramp_exp --n-samples 64
    python examples/inference_static.py --dataset-path /data/ramp --dataset-subdir EnvSimple2D --model-id my_run --env 3

Not the reference's: ``--agents A --team-sep d`` plans for TEAMS of A robots per experiment (``ramp_amd.team``): every experiment directory
is a scene, ``--n-samples`` counts teams, the A start / goal pairs are the context's pair turned about its midpoint (their straight lines
cross), the robots are coupled through the separation term of the cost guide, and the best conflict-free team is picked.  The run reports,
per scene, the free teams and the winner's swept separation, next to the same figures of the job without the team term.

    python examples/inference_static.py --make-synthetic /tmp/ramp_exp --n-samples 16 --agents 2 --team-sep 0.1
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

from ramp_amd import compat, cost, synth  # noqa: E402
from ramp_amd.metrics import Metrics  # noqa: E402
from ramp_amd.models import UNET_DIM_MULTS, TemporalUnetInference  # noqa: E402
from ramp_amd.sample_functions import ddpm_sample_fn  # noqa: E402
from ramp_amd.spec import make_unet_spec  # noqa: E402
from ramp_amd.trainer import get_model  # noqa: E402


class StaticConfig:
    """The fields of the reference's config/base_config.py StaticConfig that the script reads."""
    device = "cuda"
    dataset_path = ""
    dataset_subdir = "EnvSimple2D-RobotPointMass"
    trained_models_dir = ""
    model_id = "synthetic"
    use_ema = True
    diffusion_model_class = "StaticGaussianDiffusionModel"
    variance_schedule = "exponential"
    n_diffusion_steps = 100
    predict_epsilon = True
    compose = False
    use_apf = False
    unet_input_dim = 32
    unet_dim_mults_option = 1
    include_velocity = True
    n_samples = 20
    n_support_points = 48
    state_dim = 4
    n_guide_steps = 1
    start_guide_steps_fraction = 0.07
    n_diffusion_steps_without_noise = 5
    sampler = None           # None = the reference's hard-coded default (DDIM-5); 'ddpm' for the full chain
    alternatives = 0         # not the reference's: K > 0 stores K distinct plans per experiment next to best_trajectory (--all-envs)
    min_sep = 0.1            # the mean waypoint distance two of them keep from each other
    agents = 0               # not the reference's: A > 1 plans for teams of A robots per experiment (--agents)
    team_sep = 0.1           # the separation two robots of a team must keep (--team-sep)
    team_radius = None       # the radius of the guide's separation term; default 1.5 team_sep
    team_guide = dict(radius=0.1, step=0.05, w_obs=1.0, w_smooth=2.0, n_steps=16, max_norm=2.0)  # the cost guide the team term travels with
    team_guide_fraction = 1.0   # the guide runs on the iterations with t < this fraction of the diffusion steps
    warm_start = None        # not the reference's: 'line' or a .pt file of normalised trajectories the job starts from (--warm-start)
    warm_level = None        # the diffusion level the prior is noised to, 0 .. n_diffusion_steps - 1 (--warm-level)


def make_synthetic_experiment(root: str, cfg: StaticConfig, n_obstacles: int = 6, n_points: int = 64, seed: int = 42) -> None:
    """An experiment tree in the reference's on-disk layout (mpd/datasets/trajectories.py:316-347,
    scripts/inference/core/utils.py:28-75, inference_static.py:107-111) with synthetic content."""
    import yaml
    from ramp_amd.models import StaticGaussianDiffusionModel
    env_dir = os.path.join(root, "data", cfg.dataset_subdir, "0")
    os.makedirs(env_dir, exist_ok=True)
    boxes = synth.make_boxes(n_obstacles, 2, seed=seed)
    torch.save(torch.from_numpy(synth.make_cloud(n_obstacles, n_points, 2, seed=seed)), os.path.join(env_dir, "obstacle_points.pt"))
    np.save(os.path.join(env_dir, "box_centers.npy"), boxes.astype(np.float32))
    with open(os.path.join(env_dir, "metadata.yaml"), "w") as fh:
        yaml.safe_dump({"box_sizes": [[0.26, 0.26]] * n_obstacles}, fh)
    compat.ContextManager.save_context(torch.tensor([-0.8, -0.8]), torch.tensor([0.8, 0.8]), env_dir, cfg.dataset_subdir, 0)
    sp = make_unet_spec(cfg.state_dim, cfg.n_support_points, cfg.unet_input_dim, UNET_DIM_MULTS[cfg.unet_dim_mults_option])
    dm = StaticGaussianDiffusionModel(model=TemporalUnetInference(n_support_points=cfg.n_support_points, state_dim=cfg.state_dim,
                                                               unet_input_dim=cfg.unet_input_dim, dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option]),
                                      variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps,
                                      predict_epsilon=True)
    full = dm.state_dict()                                     # the 12 schedule buffers + scene encoder defaults
    for k, v in synth.make_unet_state_dict(sp, seed=0).items():
        full["model." + k] = torch.from_numpy(np.asarray(v))
    ck = os.path.join(root, "models", cfg.model_id, "checkpoints")
    os.makedirs(ck, exist_ok=True)
    torch.save(full, os.path.join(ck, "ema_model_current_state_dict.pth"))


class StaticInference:
    def __init__(self, config: StaticConfig):
        self.config = config
        self.device = config.device
        self.tensor_args = {'device': config.device, 'dtype': torch.float32}
        self.metrics_calculator = Metrics()
        self.context_manager = compat.ContextManager()
        self.model = None

    def warm_start_kwargs(self, hard_conds_list):
        """Opt-in (--warm-start {line,FILE} --warm-level T): the ``warm_start=`` keyword of run_inference / run_inference_scenes, or nothing.
        'line': per experiment the straight line between its start and goal states; FILE: a .pt tensor of normalised trajectories, (H, S)
        for every row, one per experiment, or one per row (``ramp_amd.warm.prior_rows``)."""
        cfg = self.config
        if cfg.warm_start is None:
            return {}
        from ramp_amd.warm import straight_line_prior
        H = cfg.n_support_points
        if cfg.warm_start == 'line':
            prior = [straight_line_prior(hc[0].detach().cpu().numpy(), hc[H - 1].detach().cpu().numpy(), H) for hc in hard_conds_list]
            prior = prior[0] if len(prior) == 1 else prior
        else:
            prior = torch.load(cfg.warm_start, map_location='cpu')
        return dict(warm_start=dict(prior=prior, level=int(cfg.warm_level)))

    def run_single_experiment(self, current_dir: int, context_idx: int):
        cfg = self.config
        torch.cuda.set_device(0)
        env_dir = os.path.join(cfg.dataset_path, cfg.dataset_subdir, str(current_dir))
        data = compat.load_environment_dir(env_dir)            # CPU tensors, as the reference's dataset hands them over
        obstacle_pts = data['obstacle_points']
        box_centers, box_size = data['box_centers'], data['box_sizes']
        n_support_points = cfg.n_support_points
        traj_normalized = torch.zeros(n_support_points, cfg.state_dim)      # accepted and unused by the samplers
        if cfg.compose:                                        # inference_static.py:64-70
            first_batch, remaining = obstacle_pts[:6], obstacle_pts[6:]
            indices = torch.randperm(4)[:2]
            obstacle_pts = torch.stack([first_batch, torch.cat([remaining, remaining[indices]], dim=0)], dim=0)
        diffusion_configs = dict(variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps,
                                 predict_epsilon=cfg.predict_epsilon, compose=cfg.compose, use_apf=cfg.use_apf)
        if cfg.sampler is not None:
            diffusion_configs['sampler'] = cfg.sampler
        unet_configs = dict(state_dim=cfg.state_dim, n_support_points=n_support_points, unet_input_dim=cfg.unet_input_dim,
                            dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option])
        self.model = get_model(model_class=cfg.diffusion_model_class,
                               model=TemporalUnetInference(max_rows=3 * cfg.n_samples, **unet_configs),
                               tensor_args=self.tensor_args, **diffusion_configs, **unet_configs)
        compat.load_checkpoint(self.model, cfg.trained_models_dir, cfg.model_id, use_ema=cfg.use_ema, device="cpu")
        self.model.eval()
        for p in self.model.parameters():                      # freeze_torch_model_params
            p.requires_grad_(False)
        self.model.warmup(horizon=n_support_points, traj_normalized=traj_normalized, obstacle_pts=obstacle_pts,
                          batch_size=cfg.n_samples, device=self.device)
        start_state_pos, goal_state_pos = self.context_manager.load_context(os.path.join(env_dir, 'contexts'), context_idx,
                                                                            self.device)
        hard_conds = compat.StateGenerator.get_hard_cond_custom(torch.vstack((start_state_pos, goal_state_pos)),
                                                                horizon=n_support_points, include_velocity=cfg.include_velocity)
        context = {'dataset': None}
        t_start_guide = ceil(cfg.start_guide_steps_fraction * self.model.n_diffusion_steps)
        sample_fn_kwargs = dict(guide=None, n_guide_steps=cfg.n_guide_steps, t_start_guide=t_start_guide,
                                noise_std_extra_schedule_fn=lambda x: 0.5)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        trajs_normalized_iters = self.model.run_inference(
            context, hard_conds, n_samples=cfg.n_samples, horizon=n_support_points, return_chain=True,
            traj_normalized=traj_normalized, obstacle_pts=obstacle_pts, sample_fn=ddpm_sample_fn, **sample_fn_kwargs,
            n_diffusion_steps_without_noise=cfg.n_diffusion_steps_without_noise, **self.warm_start_kwargs([hard_conds]))
        torch.cuda.synchronize(); elapsed = time.perf_counter() - t0
        trajs_final = trajs_normalized_iters[-1]
        collision_intensities = self.metrics_calculator.compute_collision_intensity(trajs_final, box_centers, box_size)
        metrics = self.metrics_calculator.trajectory_success_and_metrics(trajs_final, collision_intensities)
        metrics['total_time'] = elapsed
        metrics['n_chain_states'] = int(trajs_normalized_iters.shape[0])
        self.last_trajectories = trajs_final
        return metrics


    def run_all_experiments(self, context_idx: int):
        """Opt-in (--all-envs): every experiment directory of the tree as ONE job (``run_inference_scenes``) instead of the reference's
        loop of one ``run_inference`` per directory.  Returns one metrics dict per experiment, in directory order."""
        cfg = self.config
        if cfg.compose:
            raise ValueError("--all-envs does not support compose")
        torch.cuda.set_device(0)
        base = os.path.join(cfg.dataset_path, cfg.dataset_subdir)
        dirs = sorted((d for d in os.listdir(base) if d.isdigit()), key=int)
        datas = [compat.load_environment_dir(os.path.join(base, d)) for d in dirs]
        n_support_points = cfg.n_support_points
        diffusion_configs = dict(variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps,
                                 predict_epsilon=cfg.predict_epsilon, compose=False, use_apf=cfg.use_apf)
        if cfg.sampler is not None:
            diffusion_configs['sampler'] = cfg.sampler
        unet_configs = dict(state_dim=cfg.state_dim, n_support_points=n_support_points, unet_input_dim=cfg.unet_input_dim,
                            dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option])
        self.model = get_model(model_class=cfg.diffusion_model_class,
                               model=TemporalUnetInference(max_rows=2 * cfg.n_samples * len(dirs), **unet_configs),
                               tensor_args=self.tensor_args, **diffusion_configs, **unet_configs)
        compat.load_checkpoint(self.model, cfg.trained_models_dir, cfg.model_id, use_ema=cfg.use_ema, device="cpu")
        self.model.eval()
        hard_conds = []
        for d in dirs:
            start, goal = self.context_manager.load_context(os.path.join(base, d, 'contexts'), context_idx, self.device)
            hard_conds.append(compat.StateGenerator.get_hard_cond_custom(torch.vstack((start, goal)), horizon=n_support_points,
                                                                         include_velocity=cfg.include_velocity))
        t_start_guide = ceil(cfg.start_guide_steps_fraction * self.model.n_diffusion_steps)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        trajs, traj_scene = self.model.run_inference_scenes(
            [d['obstacle_points'] for d in datas], hard_conds, n_samples=cfg.n_samples, horizon=n_support_points, sample_fn=ddpm_sample_fn,
            guide=None, n_guide_steps=cfg.n_guide_steps, t_start_guide=t_start_guide, noise_std_extra_schedule_fn=lambda x: 0.5,
            n_diffusion_steps_without_noise=cfg.n_diffusion_steps_without_noise, **self.warm_start_kwargs(hard_conds))
        torch.cuda.synchronize(); elapsed = time.perf_counter() - t0
        # every experiment scored in one pass (four launches, one copy back) instead of a dozen launches and syncs per directory
        counts = [cfg.n_samples] * len(dirs)
        out, free_mask = self.metrics_calculator.evaluate_scenes(trajs, counts, [d['box_centers'] for d in datas],
                                                                 [d['box_sizes'] for d in datas])
        best = cost.compute_trajectory_costs_scenes(trajs, counts, [d['obstacle_points'] for d in datas])[0]
        alt = None
        if cfg.alternatives:                    # K plans per experiment that keep min_sep from each other, cheapest first
            alt = cost.select_diverse_clear_scenes(trajs, counts, clouds=[d['obstacle_points'] for d in datas], k=cfg.alternatives,
                                                   min_sep=cfg.min_sep, point_dim=2, swept=False)
        for i, m in enumerate(out):                            # m['free_trajectories'] is gathered when read (SceneMetrics)
            m['best_trajectory'] = best[i]
            if alt is not None:
                m['alternative_trajectories'], m['alternative_rows'], m['mode_count'] = alt.best[i], alt.rows[i], alt.mode_count[i]
                m['n_alternatives'] = int(alt.n_selected[i])
            m['env'], m['total_time_all_envs'] = int(dirs[i]), elapsed
        self.last_trajectories = trajs
        return out


    @staticmethod
    def team_endpoints(start, goal, agents: int):
        """(starts (A, 2), goals (A, 2)): the context's pair turned about its midpoint by a pi / A, so that the A straight lines cross there."""
        start, goal = start.reshape(-1)[:2].cpu().double(), goal.reshape(-1)[:2].cpu().double()
        mid, half = (start + goal) / 2, (goal - start) / 2
        starts, goals = [], []
        for a in range(agents):
            c, sn = np.cos(np.pi * a / agents), np.sin(np.pi * a / agents)
            v = torch.stack([c * half[0] - sn * half[1], sn * half[0] + c * half[1]])
            starts.append(mid - v); goals.append(mid + v)
        return torch.stack(starts).float(), torch.stack(goals).float()

    def run_team_experiments(self, context_idx: int):
        """Opt-in (--agents A): teams of A robots in every experiment directory of the tree, as ONE job (``team.run_inference_teams``), once
        with the separation term and once without it (same seed).  Returns one dict per experiment: the free teams, the winner's team and
        its swept separation, the smallest swept separation over the scene's teams -- and the same under ``without_team_term``."""
        from ramp_amd import team
        from ramp_amd.clearance import trajectory_clearance
        cfg = self.config
        if cfg.compose or cfg.state_dim != 4:
            raise ValueError("--agents plans 2-D point robots without compose")
        torch.cuda.set_device(0)
        A = cfg.agents
        base = os.path.join(cfg.dataset_path, cfg.dataset_subdir)
        dirs = sorted((d for d in os.listdir(base) if d.isdigit()), key=int)
        datas = [compat.load_environment_dir(os.path.join(base, d)) for d in dirs]
        H = cfg.n_support_points
        diffusion_configs = dict(variance_schedule=cfg.variance_schedule, n_diffusion_steps=cfg.n_diffusion_steps,
                                 predict_epsilon=cfg.predict_epsilon, compose=False, use_apf=cfg.use_apf)
        if cfg.sampler is not None:
            diffusion_configs['sampler'] = cfg.sampler
        unet_configs = dict(state_dim=cfg.state_dim, n_support_points=H, unet_input_dim=cfg.unet_input_dim,
                            dim_mults=UNET_DIM_MULTS[cfg.unet_dim_mults_option])
        self.model = get_model(model_class=cfg.diffusion_model_class,
                               model=TemporalUnetInference(max_rows=2 * cfg.n_samples * A * len(dirs), **unet_configs),
                               tensor_args=self.tensor_args, **diffusion_configs, **unet_configs)
        compat.load_checkpoint(self.model, cfg.trained_models_dir, cfg.model_id, use_ema=cfg.use_ema, device="cpu")
        self.model.eval()
        starts, goals = [], []
        for d in dirs:
            start, goal = self.context_manager.load_context(os.path.join(base, d, 'contexts'), context_idx, self.device)
            s2, g2 = self.team_endpoints(start, goal, A)
            starts.append(torch.cat([s2, torch.zeros(A, cfg.state_dim - 2)], 1)); goals.append(torch.cat([g2, torch.zeros(A, cfg.state_dim - 2)], 1))
        clouds = [d['obstacle_points'].reshape(-1, 2) for d in datas]
        r_t = cfg.team_radius if cfg.team_radius is not None else 1.5 * cfg.team_sep
        counts = [cfg.n_samples * A] * len(dirs)
        out = [dict(env=int(d), agents=A, team_sep=cfg.team_sep, team_radius=r_t) for d in dirs]
        for name, w in (("with_team_term", 1.0), ("without_team_term", 0.0)):
            guide = dict(cfg.team_guide, clouds=clouds, t_start=ceil(cfg.team_guide_fraction * self.model.n_diffusion_steps),
                         team=dict(size=A, radius=r_t, w=w))
            torch.manual_seed(0)
            teams, team_first = team.run_inference_teams(self.model, [d['obstacle_points'] for d in datas], starts, goals, cfg.n_samples, guide,
                                                         horizon=H, sample_fn=ddpm_sample_fn, noise_std_extra_schedule_fn=lambda x: 0.5,
                                                         n_diffusion_steps_without_noise=cfg.n_diffusion_steps_without_noise)
            rows = teams.reshape(-1, H, cfg.state_dim)
            r = trajectory_clearance(rows, clouds=clouds, counts=counts, point_dim=2, swept=False)
            tc = team.team_clearance(rows, A, cfg.team_sep, 2, True, r.colliding(0.0, 0.0, swept=False), r.path_length, r.smoothness)
            winners, res = cost.select_best_teams_scenes(rows, A, team_first, tc['team_mask'], tc['team_len'], tc['team_smooth'])
            res, sep = res.cpu().numpy(), tc['sep_seg'].cpu().numpy()
            for i, m in enumerate(out):
                mine = sep[team_first[i]:team_first[i + 1]]
                m[name] = dict(n_teams=int(len(mine)), free_teams=int(res[i, 0]), winner=int(res[i, 2]),
                               winner_sep_seg=float(sep[res[i, 2]]) if res[i, 2] >= 0 else None, min_sep_seg=float(np.nanmin(mine)))
                if w:
                    m['best_team'] = winners[i]
        self.last_trajectories = teams
        return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--make-synthetic", metavar="DIR", help="write a synthetic experiment tree (reference layout) to DIR and run on it")
    ap.add_argument("--dataset-path"); ap.add_argument("--dataset-subdir", default=StaticConfig.dataset_subdir)
    ap.add_argument("--trained-models-dir"); ap.add_argument("--model-id", default=StaticConfig.model_id)
    ap.add_argument("--env", type=int, default=0); ap.add_argument("--context", type=int, default=0)
    ap.add_argument("--n-samples", type=int, default=StaticConfig.n_samples)
    ap.add_argument("--n-diffusion-steps", type=int, default=StaticConfig.n_diffusion_steps)
    ap.add_argument("--sampler", choices=["ddim", "ddpm"], default=None)
    ap.add_argument("--use-apf", action="store_true")
    ap.add_argument("--all-envs", action="store_true", help="run every experiment directory of the tree as ONE job (run_inference_scenes)")
    ap.add_argument("--n-steps-without-noise", type=int, default=StaticConfig.n_diffusion_steps_without_noise)
    ap.add_argument("--unet-input-dim", type=int, choices=[16, 32, 64], default=StaticConfig.unet_input_dim)
    ap.add_argument("--unet-dim-mults-option", type=int, choices=sorted(UNET_DIM_MULTS), default=StaticConfig.unet_dim_mults_option)
    ap.add_argument("--alternatives", type=int, default=0, metavar="K",
                    help="with --all-envs: K plans per experiment that are pairwise at least --min-sep apart, next to best_trajectory")
    ap.add_argument("--min-sep", type=float, default=0.1, help="mean waypoint distance two of the --alternatives keep from each other")
    ap.add_argument("--warm-start", default=None, metavar="{line,FILE}",
                    help="start from a prior instead of pure noise: the straight line from start to goal, or a .pt file of normalised trajectories")
    ap.add_argument("--warm-level", type=int, default=None, metavar="T", help="the diffusion level the prior is noised to (0 .. n_diffusion_steps - 1)")
    ap.add_argument("--agents", type=int, default=0, metavar="A", help="plan for teams of A robots (2 .. 8) per experiment; --n-samples counts teams")
    ap.add_argument("--team-sep", type=float, default=StaticConfig.team_sep, help="the separation two robots of a team must keep")
    ap.add_argument("--team-radius", type=float, default=None, help="radius of the guide's separation term (default 1.5 x --team-sep)")
    args = ap.parse_args(argv)
    if args.agents and not 2 <= args.agents <= 8:
        ap.error("--agents takes 2 .. 8")
    if args.alternatives and not args.all_envs:
        ap.error("--alternatives goes with --all-envs")
    if (args.warm_start is None) != (args.warm_level is None):
        ap.error("--warm-start and --warm-level go together")
    if args.warm_start is not None and args.agents:
        ap.error("--warm-start is not wired into --agents")
    cfg = StaticConfig()
    cfg.warm_start, cfg.warm_level = args.warm_start, args.warm_level
    cfg.alternatives, cfg.min_sep = args.alternatives, args.min_sep
    cfg.agents, cfg.team_sep, cfg.team_radius = args.agents, args.team_sep, args.team_radius
    cfg.n_samples, cfg.n_diffusion_steps, cfg.sampler, cfg.use_apf = args.n_samples, args.n_diffusion_steps, args.sampler, args.use_apf
    cfg.dataset_subdir, cfg.model_id = args.dataset_subdir, args.model_id
    cfg.n_diffusion_steps_without_noise = args.n_steps_without_noise
    cfg.unet_input_dim, cfg.unet_dim_mults_option = args.unet_input_dim, args.unet_dim_mults_option
    if args.make_synthetic:
        make_synthetic_experiment(args.make_synthetic, cfg)
        cfg.dataset_path = os.path.join(args.make_synthetic, "data")
        cfg.trained_models_dir = os.path.join(args.make_synthetic, "models")
    else:
        if not (args.dataset_path and args.trained_models_dir):
            ap.error("--dataset-path and --trained-models-dir (or --make-synthetic DIR) are required")
        cfg.dataset_path, cfg.trained_models_dir = args.dataset_path, args.trained_models_dir
    runner = StaticInference(cfg)
    if args.agents:
        per_env = runner.run_team_experiments(args.context)
        for m in per_env:
            print(json.dumps({k: v for k, v in m.items() if not torch.is_tensor(v)}))
        return per_env, runner
    if args.all_envs:
        per_env = runner.run_all_experiments(args.context)
        for m in per_env:
            print(json.dumps({k: v for k, v in m.items() if v is None or isinstance(v, (int, float))}))
        return per_env, runner
    metrics = runner.run_single_experiment(args.env, args.context)
    print(json.dumps({k: v for k, v in metrics.items() if v is None or isinstance(v, (int, float))}))
    return metrics, runner


if __name__ == "__main__":
    main()
