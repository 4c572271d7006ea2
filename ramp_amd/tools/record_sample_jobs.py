"""The sampling entries (ramp_sample .. ramp_sample_stitched) pinned byte for byte: records tests/golden/sample_jobs_parent.npz.

Run once by hand on the GPU against the build whose results are to be kept (the commit before the nine entries were put behind one job
descriptor; another build of the library is selected with RAMP_HIP_LIB); tests/test_gpu_sample_one_job.py replays the same walks through
``replay`` and requires every stored output bit for bit.  The fixture holds every input except the network weights (``in/...``: loop noise,
the inner steps' normals and uniforms, the events' uniforms, the scene clouds, the guide cloud, boxes, start and goal) and per call
``out/<walk>/<nn>_<job>/<run>/`` x, chain, the launch count and, where the job has them, accept, ancestors / ess / cost / logw and long.  The
weights are the seeded synthetic ones (ramp_amd/synth.py) of the smallest network: H = 8, S = 4, B = 6, 3 iterations of T = 100.

What such a change can break is not arithmetic but the graph key (a lost field: the next job replays the previous job's graph), the
staging (a copy lost, or placed in front of the growth of its buffer) and the first allocation of an optional buffer.  So a walk runs its
jobs ON ONE CONTEXT, every job twice in a row (run 0 captures, run 1 replays), and neighbours differ in one keyed field:
  graph    WALK below with use_graph = 1; its last job is its first again
  eager    the same jobs with use_graph = 0 on a second context
  bf16x6   plain, guided, steered and stitched on the bf16x6 kernels, use_graph = 1
usage: python ramp_amd/tools/record_sample_jobs.py [--out PATH]"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "sample_jobs_parent.npz")
B, H, S, T, N_IT = 6, 8, 4, 100, 3
STEPS = [66, 33, 0]                      # the iterations' timesteps, DDPM and DDIM (K = 3) alike
W, O, CHAINS = 3, 2, 2                   # stitched: B = CHAINS * W windows, L = H + (W - 1)(H - O) = 20
GUIDE = dict(radius=0.3, step=0.05, n_steps=2, w_obs=1.0, w_smooth=0.5)
RESAMPLE = dict(flags=[1, 0, 1], lambda_=2.0, ess_frac=2.0, radius=0.3, w_obs=1.0, w_smooth=0.5)      # (ess_frac 2: every event resamples)
# job -> (kind, options).  kind: plain | scenes (2 scenes x 3) | composed (2 scenes x 3, two sets each: n_rp = 3) | stitched.  Options:
# ddim, apf, philox (noise_mode 1), mcmc, guide (overrides of GUIDE; `prims` / `team` add the term), resample, pin (the goal's long waypoint)
JOBS = {
    "ddpm": ("plain", {}),
    "ddim": ("plain", dict(ddim=True)),
    "scenes_apf": ("scenes", dict(apf=True)),
    "composed": ("composed", {}),
    "ula": ("plain", dict(mcmc=dict(kind="ula", steps=1, step_scale=0.05))),
    "composed_mala": ("composed", dict(mcmc=dict(kind="mala", steps=[1, 2, 0], step_scale=0.05))),
    "guided": ("plain", dict(guide={})),
    "guided_w_obs": ("plain", dict(guide=dict(w_obs=0.5))),
    "prims": ("plain", dict(guide=dict(prims=0.05))),
    "prims_margin": ("plain", dict(guide=dict(prims=0.1))),
    "team": ("plain", dict(guide=dict(team=0.4))),
    "team_radius": ("plain", dict(guide=dict(team=0.6))),
    "steered": ("scenes", dict(ddim=True, mcmc=dict(kind="ula", steps=1, step_scale=0.05), guide={}, resample=True)),
    "stitched": ("stitched", dict(guide={}, pin=-1)),
    "stitched_pin": ("stitched", dict(guide={}, pin=-2)),
    "philox": ("plain", dict(philox=True)),
    "philox_mala": ("plain", dict(philox=True, mcmc=dict(kind="mala", steps=1, step_scale=0.05))),
    "philox_steered": ("plain", dict(philox=True, resample=True)),
}
WALK = ("ddpm", "ddim", "scenes_apf", "composed", "ula", "composed_mala", "guided", "guided_w_obs", "prims", "prims_margin", "team",
        "team_radius", "steered", "stitched", "stitched_pin", "philox", "philox_mala", "philox_steered", "ddpm")
WALKS = {"graph": (WALK, 1, "default"), "eager": (WALK, 0, "default"), "bf16x6": (("ddpm", "guided", "steered", "stitched"), 1, "bf16x6")}


def make_inputs() -> dict:
    """Every input of the walks, as numpy arrays (seeded)."""
    from ramp_amd import synth
    rng = np.random.RandomState(7)
    inp = {f"scene{i}": synth.make_cloud(3 + i, 12, seed=40 + i) for i in range(3)}      # (3 | 4 | 5, 12, 2): what the network sees
    inp["guide_cloud"] = np.ascontiguousarray(synth.make_cloud(4, 16, seed=50).reshape(-1, 2))
    inp["box_centers"] = synth.make_boxes(3, seed=51).astype(np.float32)
    inp["box_sizes"] = np.full((3, 2), 0.26, np.float32)
    hc = synth.default_hard_conds(S, H)
    inp["start"], inp["goal"] = hc[0], hc[H - 1]
    inp["noise"] = rng.standard_normal((N_IT + 1, B, H, S)).astype(np.float32)
    inp["mcmc_noise"] = rng.standard_normal((N_IT, B, H, S)).astype(np.float32)         # (a job takes the first sum K blocks)
    inp["mcmc_u"] = rng.uniform(0.01, 0.99, (N_IT, B)).astype(np.float32)
    inp["resample_u"] = rng.uniform(0.01, 0.99, (2, 2)).astype(np.float32)              # (events, groups)
    return inp


class _Walk:
    """One context (the smallest network with the seeded synthetic weights) and the jobs run on it."""

    def __init__(self, inp, use_graph, gemm_mode):
        import torch

        from ramp_amd import synth
        from ramp_amd.models import StaticGaussianDiffusionModel, TemporalUnetInference
        from ramp_amd.spec import UNET_DIM_MULTS, make_unet_spec
        from ramp_amd.unet import load_numpy_state_dict
        torch.cuda.set_device(0)
        self.torch = torch
        u = TemporalUnetInference(n_support_points=H, state_dim=S, obstacle_3d=False, unet_input_dim=16, dim_mults=UNET_DIM_MULTS[0],
                                  max_rows=4 * B, gemm_mode=gemm_mode)
        load_numpy_state_dict(u, synth.make_unet_state_dict(make_unet_spec(S, H, 16, UNET_DIM_MULTS[0], False)))
        self.m = u.eval().to("cuda")
        self.dm = StaticGaussianDiffusionModel(model=self.m, n_diffusion_steps=T, predict_epsilon=True, sampler="ddpm", use_graph=bool(use_graph),
                                               noise_source="torch", noise_seed=5, use_apf=True).eval().to("cuda")
        self.d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}

    def _guide(self, over, clouds):
        g = dict(GUIDE, **{k: v for k, v in over.items() if k not in ("prims", "team")})
        g.update(clouds)
        if "prims" in over:
            g.update(boxes=(self.d["box_centers"], self.d["box_sizes"]), band=0.1, margin=over["prims"])
        if "team" in over:
            g["team"] = dict(size=2, radius=over["team"], w=1.0)
        return g

    def run(self, name) -> dict:
        """One call of job `name`: its outputs as numpy arrays."""
        torch, dm, d = self.torch, self.dm, self.d
        kind, opt = JOBS[name]
        ddim, philox = bool(opt.get("ddim")), bool(opt.get("philox"))
        hc = {0: d["start"], H - 1: d["goal"]}
        scene_job = guidance = stitch = obstacle_pts = None
        n_scenes = 1
        if kind == "plain":
            obstacle_pts, hard = d["scene0"], {k: v.unsqueeze(0).expand(B, -1).contiguous() for k, v in hc.items()}
            if "team" in opt.get("guide", {}):      # the two agents of a team start and end 0.2 apart
                hard = {k: v + torch.tensor([0.0, 0.2, 0.0, 0.0], device="cuda") * (torch.arange(B, device="cuda") % 2).unsqueeze(1) for k, v in hard.items()}
        elif kind == "scenes":
            scene_job, hard, _ = dm._prepare_scene_job([d["scene0"], d["scene1"]], [hc, hc], B // 2)
            n_scenes = 2
        elif kind == "composed":
            scene_job, guidance, hard, _ = dm._prepare_composed_job([[d["scene0"], d["scene1"]], [d["scene1"], d["scene2"]]], [hc, hc], B // 2,
                                                                    weights=[[2.0, 1.0], [1.5, 0.5]])
            n_scenes = 2
        else:      # stitched: one scene for all windows; the job's conditions are the pins
            from ramp_amd import stitch as st
            pins = {0: d["start"], opt["pin"]: d["goal"]}
            tab = st.build_stitch_tables(H, W, O, CHAINS, 1, list(pins.keys()), None)
            stitch = {"n_windows": W, "overlap": O, "alpha": st.blend_table("ramp", O), "pin_idx": tab["pin_idx"],
                      "pin_val": st.pin_values(pins, CHAINS, S, "cuda")}
            lat = torch.cat([self.m.encode_scenes([d["scene0"]]), torch.zeros(1, self.m.context_dim, device="cuda")])
            self.m.set_scenes(lat, tab["row_variant"])
            scene_job = {"n_scenes": 1, "traj_scene": torch.from_numpy(tab["traj_scene"]).cuda(), "cloud_offset": None, "cloud_points": None}
            hard = {}
        clouds = dict(cloud=d["guide_cloud"]) if n_scenes == 1 else dict(clouds=[d["guide_cloud"], d["guide_cloud"][:20]])
        mcmc = dict(opt["mcmc"]) if "mcmc" in opt else None
        if mcmc is not None and not philox:
            total = int(np.broadcast_to(mcmc["steps"], N_IT).sum())
            mcmc.update(noise=d["mcmc_noise"][:total], u=d["mcmc_u"][:total])
        guide = self._guide(opt["guide"], clouds) if "guide" in opt else None
        resample = dict(RESAMPLE, **clouds) if opt.get("resample") else None
        if resample is not None and not philox:
            resample["u"] = d["resample_u"][:, :n_scenes]
        apf = [0, 1, 1] if opt.get("apf") else [0] * N_IT
        cfg = (dict(dm.apf_ddim) if ddim else dict(dm.apf_ddpm, passes=1)) if any(apf) else None
        noise = None if philox else (d["noise"][:1] if ddim else d["noise"])
        dm._philox_offset, dm.last_mcmc, dm.last_resample = 0, None, None
        long = torch.full((CHAINS, H + (W - 1) * (H - O), S), float("nan"), device="cuda") if stitch is not None else None
        with _long_out(long):
            x, chain = dm._launch(B, noise, hard, obstacle_pts, ddim, STEPS, apf, None if ddim else [0.5] * N_IT, cfg, True, ddim_K=N_IT,
                                  scene_job=scene_job, guidance=guidance, mcmc=mcmc, cost_guide=guide, resample=resample, stitch=stitch)
        torch.cuda.synchronize()
        out = dict(x=x.cpu().numpy(), chain=chain.cpu().numpy(), launches=np.array([self.m.launch_count()], np.int64))
        if mcmc is not None:
            out["accept"] = dm.last_mcmc["accept"].numpy()
        if resample is not None:
            r = dm.last_resample
            out.update(ancestors=r["ancestors"].numpy(), ess=r["ess"].numpy(), cost=r["cost"].numpy(), logw=r["logw"].numpy())
        if long is not None:
            out["long"] = long.cpu().numpy()
        return out


class _long_out:
    """While active, ramp_sample_stitched receives `long` as its long_out (the Python layer passes none and assembles the windows itself)."""

    def __init__(self, long):
        self.long = long

    def __enter__(self):
        if self.long is None:
            return
        from ramp_amd import _lib
        self.lib, self.fn = _lib.load(), _lib.load().ramp_sample_stitched
        self.lib.ramp_sample_stitched = lambda *a: self.fn(*a[:8], self.long.data_ptr(), a[9])

    def __exit__(self, *exc):
        if self.long is not None:
            self.lib.ramp_sample_stitched = self.fn


def replay(inp, walks=tuple(WALKS)) -> dict:
    """{'<walk>/<nn>_<job>/<run>/<output>': array} of the listed walks, each on a fresh context."""
    out = {}
    for wname in walks:
        jobs, use_graph, gemm_mode = WALKS[wname]
        walk = _Walk(inp, use_graph, gemm_mode)
        for i, name in enumerate(jobs):
            for run in range(2):
                out.update({f"{wname}/{i:02d}_{name}/{run}/{key}": v for key, v in walk.run(name).items()})
    return out


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    inp = make_inputs()
    out = replay(inp)
    for k in sorted(out):
        if k.endswith("/launches"):
            print(f"{k}: {int(out[k][0])}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez_compressed(path, **{f"in/{k}": v for k, v in inp.items()}, **{f"out/{k}": v for k, v in out.items()})
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} outputs of {len(WALKS)} walks")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main()
