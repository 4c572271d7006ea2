"""examples/inference_static.py --all-envs: every experiment directory of a tree (the reference's on-disk layout) as ONE job."""
import os

import numpy as np
import pytest
import torch
import yaml

from ramp_amd import compat, synth

pytestmark = pytest.mark.gpu


def _add_experiment(tree, subdir, name, n_obstacles, seed, start, goal):
    """A second experiment directory beside the one make_synthetic_experiment writes: its own cloud, boxes and context."""
    env_dir = os.path.join(tree, "data", subdir, name)
    os.makedirs(env_dir, exist_ok=True)
    torch.save(torch.from_numpy(synth.make_cloud(n_obstacles, 64, 2, seed=seed)), os.path.join(env_dir, "obstacle_points.pt"))
    np.save(os.path.join(env_dir, "box_centers.npy"), synth.make_boxes(n_obstacles, 2, seed=seed).astype(np.float32))
    with open(os.path.join(env_dir, "metadata.yaml"), "w") as fh:
        yaml.safe_dump({"box_sizes": [[0.26, 0.26]] * n_obstacles}, fh)
    compat.ContextManager.save_context(torch.tensor(start), torch.tensor(goal), env_dir, subdir, 0)


def test_all_envs_runs_every_experiment_directory_as_one_job(tmp_path):
    """Three experiment directories with clouds of 6, 9 and 4 obstacles and their own start / goal: --all-envs returns one metrics
    dict per directory, in directory order, from ONE (12, 48, 4) batch whose rows carry their own experiment's hard conditions; and
    experiment 0's rows are what the default flow (one run_inference for --env 0) gives on the same noise, to the 2e-4 by which two
    fp32-faithful evaluations of a free-running T = 25 chain agree (test_sharded_philox_jobs_reproduce_the_unsharded_job: the same
    rows inside batches of different sizes).  APF off: its decisions are stiff, the chain tests teacher-force those steps."""
    import examples.inference_static as ex
    from util import NoiseInjector
    cfg = ex.StaticConfig()
    cfg.n_diffusion_steps = 25
    ex.make_synthetic_experiment(str(tmp_path), cfg)
    _add_experiment(str(tmp_path), cfg.dataset_subdir, "1", 9, 7, [-0.7, 0.6], [0.7, -0.6])
    _add_experiment(str(tmp_path), cfg.dataset_subdir, "2", 4, 8, [0.5, -0.8], [-0.5, 0.8])
    common = ["--dataset-path", str(tmp_path / "data"), "--trained-models-dir", str(tmp_path / "models"), "--n-samples", "4",
              "--sampler", "ddpm", "--n-diffusion-steps", "25", "--n-steps-without-noise", "0"]
    noise = synth.make_noise((26, 12, 48, 4), seed=21)
    with NoiseInjector(list(noise)) as inj:
        per_env, runner = ex.main(common + ["--all-envs"])
        assert inj.used == 26
    x = runner.last_trajectories
    assert [m["env"] for m in per_env] == [0, 1, 2] and len(per_env) == 3
    assert x.shape == (12, 48, 4) and bool(torch.isfinite(x).all())
    ends = [([-0.8, -0.8], [0.8, 0.8]), ([-0.7, 0.6], [0.7, -0.6]), ([0.5, -0.8], [-0.5, 0.8])]
    for i, (a, b) in enumerate(ends):
        rows = x[4 * i:4 * i + 4]
        assert torch.equal(rows[:, 0, :2], torch.tensor(a, device="cuda").expand(4, -1)), i
        assert torch.equal(rows[:, 47, :2], torch.tensor(b, device="cuda").expand(4, -1)), i
        assert per_env[i]["total_time_all_envs"] > 0
    warm = synth.make_noise((1, 4, 48, 4), seed=77)                    # the default flow's warmup() draws one randn first
    with NoiseInjector([warm[0]] + list(noise[:, :4])):
        _, single = ex.main(common + ["--env", "0"])
    d = float((single.last_trajectories - x[:4]).abs().max())
    print(f"--all-envs, experiment 0's rows vs the default flow on the same noise: {d:.2e}")
    assert d < 2e-4
