"""DynamicGaussianDiffusionModel (mpd/models/diffusion_models/diffusion_model_dynamic.py:24-680), re-exported by ``ramp_amd.diffusion``.
Its planner exists twice -- ``ddim_p_sample_loop`` on ``ramp_sample`` / ``ramp_replan`` and ``ddim_p_sample_loop_eager``, the host
restatement it is tested against -- and the two share only what is literally the same: ``_Episode``, ``_replan_from_scratch``.
``run_inference_episodes`` advances MANY episodes in lock-step on ``ramp_sample_scenes`` / ``ramp_replan_episodes``; it shares the
per-episode environment step (``_environment_step``) and book-keeping (``_Episode``) with the one-episode planner."""
import warnings

import ctypes as C
from copy import copy

import numpy as np
import torch

from . import _lib
from .diffusion import _GaussianDiffusionBase, _HostArrays
from .sample_functions import apply_hard_conditioning, extract


class _Episode:
    """One episode as both planner loops keep it (diffusion_model_dynamic.py:495-520, 606-624): the environment's fixed boxes
    (handed to the APF through ``context``) and sphere, the cloud, the thresholds, and the executed plan's book-keeping."""
    safe_threshold, distance_threshold_pred = 0.2, 0.4
    thr_high, thr_low = 0.02, 0.05

    def __init__(self, context, hard_conds, obstacle_pts, device, return_chain):
        env = context['dataset'].env
        fixed = env.obj_fixed_list[0].fields[0]
        context['static_obstacle_centers'] = fixed.centers.cpu().numpy()[:4]
        context['static_obstacle_sizes'] = fixed.sizes.cpu().numpy()[:4]
        self.sphere = env.obj_extra_list[0].fields[0]
        self.cloud = obstacle_pts.to(device).contiguous()
        self.chain_obs = []
        self.chain_start = [hard_conds[0][0].unsqueeze(0)]
        self.chain = [] if return_chain else None
        self.stepp = 0

    def start(self, plan):
        """The selected high-level plan: its first state is executed."""
        self.high_plan = plan.clone()
        self.executed_history = [plan[0].clone().unsqueeze(0)]

    def record(self, x):
        """Execute one more state of the plan ``x`` the replan selected."""
        self.executed_history.append(x[self.stepp + 1].clone().unsqueeze(0))
        updated_start_state = x[self.stepp].clone()
        self.stepp += 1
        if self.chain is not None:
            if self.stepp == 1:
                self.chain.append(self.high_plan.unsqueeze(0).clone())
            self.chain.append(x.unsqueeze(0).clone())
        self.chain_obs.append(self.sphere.centers.clone())
        self.chain_start.append(updated_start_state.unsqueeze(0).clone())

    def reached(self, goal_distance) -> bool:
        """Termination: the state just executed lies within ``safe_threshold`` of the goal."""
        return bool(goal_distance < self.safe_threshold)

    def result(self, x):
        chain = torch.stack(self.chain, dim=1) if self.chain is not None else None
        return x, chain, self.chain_obs, self.chain_start


class DynamicGaussianDiffusionModel(_GaussianDiffusionBase):
    """Pursuit-evasion wrapper (diffusion_model_dynamic.py:24-680): the pieces on the sampler hot path — CFG
    (w = 2.5) + x0 + clamp + posterior (``p_mean_variance``), one DDIM step with the per-trajectory static /
    pursuer APF (``ddim_p_sample``), velocity smoothing ``sm`` and ``q_sample`` re-noising, and the receding-horizon
    replanning state machine around them (``ddim_p_sample_loop`` / ``ddim_replan_scratch`` / ``run_inference``,
    :461-667; SURVEY.md §8(f) "next" row 1), which reaches the environment through the same attribute path as the
    reference (``context['dataset'].env.obj_fixed_list / obj_extra_list``).

    ``cfg_mode='reference_compat'`` reproduces the reference's row pairing exactly: it
    lays rows out blocked [x_0..x_{B-1}, x_0..x_{B-1}] while the net zeroes the latent of every odd GLOBAL row, so
    for even B even samples get pure eps_cond and odd samples pure eps_uncond, and for odd B odd samples get the
    inverted combination.  ``cfg_mode='intended'`` is true classifier-free guidance."""
    _default_cfg_weight = 2.5          # diffusion_model_dynamic.py:157
    _default_ddim = True               # diffusion_model_dynamic.py:46
    _supports_apf = False
    _scenes_supported = False          # the replanning loop keeps one scene per job

    def __init__(self, model=None, variance_schedule='exponential', n_diffusion_steps=100, clip_denoised=True,
                 predict_epsilon=False, loss_type='l2', context_model=None, mask_type=None, traj_len=None,
                 cfg_mode: str = 'reference_compat', **kwargs):
        super().__init__(model=model, variance_schedule=variance_schedule, n_diffusion_steps=n_diffusion_steps,
                         clip_denoised=clip_denoised, predict_epsilon=predict_epsilon, loss_type=loss_type,
                         context_model=context_model, **kwargs)
        self.mask_type = mask_type
        self.traj_len = traj_len
        self.ddim_num_inference_steps_high = 10
        self.ddim_num_inference_steps_low = 5
        assert cfg_mode in ('reference_compat', 'intended')
        self.cfg_mode = cfg_mode

    # dynamic APF constants hard-coded in the reference (diffusion_model_dynamic.py:380-389)
    apf_dynamic = dict(obs_radius=0.1, points_per_obstacle=64, threshold_static=0.2, threshold_pred=0.5,
                       strength_static=0.15, strength_pred=0.15, window_static=8, window_pred=5)

    def deep_repeat_tensor(self, x, t, traj_normalized, obstacle_pts, n_rp):
        """diffusion_model_dynamic.py:129-147: blocked ``repeat`` (the layout behind quirk Q1, see ``cfg_mode``)."""
        rep = lambda v: v.repeat((n_rp,) + (1,) * (v.dim() - 1))
        return rep(x), t.repeat((n_rp,)), rep(traj_normalized), rep(obstacle_pts)

    def _row_pattern(self, B):
        if self.cfg_mode == 'intended' or B is None:
            return [0, 1]
        # rows here are [b*2 + v]; v = 0 plays global row b, v = 1 plays global row B + b of the reference
        return [0, 0, 1, 1] if B % 2 == 0 else [0, 1, 1, 0]

    @torch.no_grad()
    def ddim_p_sample(self, x, hard_conds, context, t, obstacle_pts, traj_normalized=None, forward_t=None, eta=0.0,
                      use_apf=False, use_clipped_model_output=False, obstacle_field=None, pursuer_pos=None):
        """One DDIM step of the high-level plan (diffusion_model_dynamic.py:338-447).  With ``use_apf`` the
        caller supplies ``obstacle_field`` (ramp_amd.apf_dynamic.ObstacleField, dynamic cloud already updated) and
        the pursuer position; every trajectory gets the static pass, those whose current waypoint is within
        ``threshold_pred`` of the pursuer also the pursuer pass, then the goal waypoint is restored."""
        assert use_clipped_model_output and eta == 0.0
        from .apf_dynamic import avoidance
        dev = self._device()
        B, H, S = x.shape
        ti = int(t.reshape(-1)[0])
        x0 = self._x0_mean_eps(x, t, obstacle_pts)[0]
        xx = x.detach().to(dev, torch.float32).contiguous()
        if use_apf:
            if obstacle_field is None or pursuer_pos is None:
                raise ValueError("use_apf=True needs obstacle_field and pursuer_pos (the reference pulls them from "
                                 "context['dataset'].env, which is outside the sampler hot path)")
            c = self.apf_dynamic
            x_start = xx[:, forward_t].clone()
            x_goal = xx[:, -1].clone()
            avoidance(x0, obstacle_field, is_dynamic=False, avoidance_window=c['window_static'],
                      avoidance_strength=c['strength_static'], avoidance_strength_pred=c['strength_pred'])
            near = (torch.norm(x_start[:, :2] - pursuer_pos.to(dev, torch.float32)[None, :2], dim=1)
                    < c['threshold_pred']).to(torch.int32)
            avoidance(x0, obstacle_field, is_dynamic=True, avoidance_window=c['window_pred'],
                      avoidance_strength=c['strength_static'], avoidance_strength_pred=c['strength_pred'],
                      affected_states=H, goal_state=x_goal[0], enable=near)
            x0[:, -1] = x_goal
        return self._ddim_finish(xx, x0, ti, self.ddim_num_inference_steps_high)      # (no hard conds here)

    def sm(self, s1, s2, dt=0.1, num_steps=3, max_vel=.8):
        """Velocity-limited straight-line states between s1 and s2 (diffusion_model_dynamic.py:192-214)."""
        delta_pos = s2[:, :2] - s1[:, :2]
        dist = torch.norm(delta_pos, dim=1, keepdim=True)
        direc = torch.where(dist > 1e-6, delta_pos / dist, torch.zeros_like(delta_pos))
        desired_v = delta_pos / (num_steps * dt)
        base_v = torch.where(torch.norm(desired_v, dim=1, keepdim=True) > max_vel, direc * max_vel, desired_v)
        tt = torch.arange(1, num_steps + 1, device=s1.device).float().view(1, num_steps, 1) * dt
        pos = s1[:, None, :2] + tt * base_v[:, None, :]
        return torch.cat([pos, base_v.unsqueeze(1).expand(-1, num_steps, -1)], dim=-1)

    def q_sample(self, x_start, t, noise=None):
        """diffusion_model_dynamic.py:671-680."""
        if noise is None:
            noise = torch.randn_like(x_start)
        return (extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + extract(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    # ------------------------------------------------------------------ receding-horizon planner
    def _obstacle_field(self, context, rng=np.random):
        """Lazily build the APF clouds exactly where the reference does (diffusion_model_dynamic.py:391-411): static
        boxes from context['static_obstacle_centers'/'sizes'], pursuer from the env's moving sphere field.  ``rng``: the stream the
        field draws its clouds from when it is built here (an episode of a many-episode job has its own)."""
        from .apf_dynamic import ObstacleField
        if 'obstacle_field' not in context:
            sphere = context['dataset'].env.obj_extra_list[0].fields[0]
            c = self.apf_dynamic

            def dynamic_obstacle_fn(t, start_pos, replan_guide=True, best_idx=None):
                if replan_guide and best_idx is not None:
                    start_pos = start_pos[best_idx].unsqueeze(0)
                sphere.update_centers(t, start_pos)
                return sphere.centers[0].cpu().numpy(), c['obs_radius']

            context['obstacle_field'] = ObstacleField(context['static_obstacle_centers'], context['static_obstacle_sizes'],
                                                      dynamic_obstacle_fn, c['points_per_obstacle'],
                                                      distance_threshold=c['threshold_static'],
                                                      distance_threshold_pred=c['threshold_pred'], device=self._device(), rng=rng)
        return context['obstacle_field']

    def _step(self, x, hard_conds, context, i, obstacle_pts, traj_normalized, forward_t, use_apf):
        """ddim_p_sample as the loops call it: with use_apf the pursuer cloud is advanced to ``forward_t`` first."""
        B = x.shape[0]
        t = torch.full((B,), int(i), device=self._device(), dtype=torch.long)
        field, pursuer = None, None
        if use_apf:
            field = self._obstacle_field(context)
            field.update_dynamic(forward_t, x[:, forward_t, :2].clone(), replan_guide=True)
            pursuer = torch.as_tensor(np.asarray(field.dynamic_center), dtype=torch.float32)
        return self.ddim_p_sample(x, hard_conds, context, t, obstacle_pts, traj_normalized=traj_normalized,
                                  forward_t=forward_t, eta=0.0, use_apf=use_apf, use_clipped_model_output=True,
                                  obstacle_field=field, pursuer_pos=pursuer)

    @torch.no_grad()
    def ddim_replan_scratch(self, shape, hard_conds, context=None, traj_normalized=None, forward_t=None,
                            obstacle_pts=None, use_apf=False, executed_history=None):
        """diffusion_model_dynamic.py:461-493."""
        x = torch.randn(shape, device=self._device())
        x = apply_hard_conditioning(x, hard_conds)
        for h, st in enumerate(executed_history):
            x[:, h] = st
        for i in self.ddim_set_timesteps(self.ddim_num_inference_steps_high):
            if i == 0:
                use_apf = True
            x = self._step(x, hard_conds, context, i, obstacle_pts, traj_normalized, forward_t, use_apf)
            x = apply_hard_conditioning(x, hard_conds)
            for h, st in enumerate(executed_history):
                x[:, h] = st
        return x

    # ------------------------------------------------------------------ receding-horizon planner, one graph per replan
    @torch.no_grad()
    def _plan_high_level(self, shape, ts, hard_conds, ep: _Episode, cost_cloud, sel, log, sharded):
        """STAGE I: the high-level plan (DDIM steps ``ts``, hard conditioning after each: one captured job), then the selection."""
        from . import dist as rdist
        device = self._device()
        B, H, S = shape
        x = torch.randn(shape, device=device)
        xb, _ = self._launch(B, x.unsqueeze(0), hard_conds, ep.cloud, True, ts, [0] * len(ts), None, None, False,
                             ddim_K=self.ddim_num_inference_steps_high)
        res_dev = torch.zeros(4, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.load().ramp_select_best(_lib.ptr(xb), B, H, S, _lib.ptr(cost_cloud), cost_cloud.shape[0], ep.thr_high, 0.1,
                                                    0.9, _lib.ptr(sel.mask), _lib.ptr(sel.plen), _lib.ptr(sel.smooth), _lib.ptr(sel.best),
                                                    _lib.ptr(res_dev), _lib.current_stream()), "ramp_select_best")
        n_free, rank, _row, _ = (int(v) for v in res_dev.cpu())
        if log is not None:
            log.append(dict(batch=xb.clone(), npts=cost_cloud.shape[0], idx=rank if n_free else -1, free=(sel.mask == 0).clone()))
        if sharded:
            x_plan, n_free, _row = rdist.select_best_sharded(xb, sel.mask, sel.plen, sel.smooth, 0.1, 0.9, zero_start=False)
        if n_free == 0:
            raise RuntimeError("no collision-free high-level plan (the reference dereferences None here)")
        if not sharded:
            x_plan = xb[_row].clone()   # (the selection kernel zeroes x[0, 2:] as the replans need; the high-level winner stays as is)
        return xb, x_plan

    def _replan_params(self, B, low, hard_conds, cost_cloud, cost_thr, arrays: _HostArrays):
        """ramp_replan_params of an episode; ``low`` is the low-level tail of the high-level schedule, ``arrays`` owns the tables."""
        c = self.apf_dynamic
        p = _lib.RampReplanParams()
        p.B, p.n_rp, p.n_steps, p.clip_denoised, p.w = B, 2, len(low), int(bool(self.clip_denoised)), float(self.cfg_weight)
        p.predict_x0 = int(not self.predict_epsilon)
        p.t = arrays.i32(low)
        for k, v in self._ddim_coefficients(low, self.ddim_num_inference_steps_high).items():
            setattr(p, k, arrays.f32(v))
        p.q_sqrt_a = float(self.sqrt_alphas_cumprod[low[0]]); p.q_sqrt_1m_a = float(self.sqrt_one_minus_alphas_cumprod[low[0]])
        self._fill_hard(p, arrays, hard_conds, B)
        p.sm_window_last, p.sm_window_final, p.sm_dt, p.sm_max_vel = 3, 2, 0.1, 0.8
        p.thr_static, p.thr_pred = float(c['threshold_static']), float(c['threshold_pred'])
        p.strength_static, p.strength_pred, p.window_static = float(c['strength_static']), float(c['strength_pred']), int(c['window_static'])
        p.n_dyn = int(c['points_per_obstacle'])
        p.cost_cloud, p.n_cost, p.n_extra = _lib.ptr(cost_cloud), cost_cloud.shape[0], 64
        p.cost_thr, p.w_smooth, p.w_len = cost_thr, 0.1, 0.9
        p.use_graph = int(self.use_graph)
        return p

    def _environment_step(self, k, context, ep: _Episode, B, best_host, rng=np.random):
        """One episode's environment step before replan ``k`` (diffusion_model_dynamic.py:396-411), in the reference's order of host
        random draws: the pursuer's dynamics see x[:, stepp, :2] -- the pinned executed state of all B candidates -- and its sphere
        cloud is re-sampled (``update_dynamic``), then the near-check draws the sphere points that join the cost cloud.
        Returns (field, pursuer centre float64 (2), pursuer cloud float64 (n_dyn, 2), near, extra cost points float32 (64, 2) or None)."""
        from .apf_dynamic import generate_sphere_points
        field = self._obstacle_field(context, rng)
        field.update_dynamic(k, ep.executed_history[-1][:, :2].expand(B, 2).clone(), replan_guide=True)
        centre = np.asarray(field.dynamic_center, np.float64)
        dyn = np.ascontiguousarray(field.dynamic_points, np.float64)
        sphere = ep.sphere
        near = bool(np.linalg.norm(best_host[ep.stepp, :2] - sphere.centers[0].cpu().numpy()) < ep.distance_threshold_pred)
        extra = None
        if near:
            extra = np.ascontiguousarray(generate_sphere_points(sphere.centers[0].cpu().numpy(),
                                                                sphere.radii[0].cpu().numpy(), 64, rng=rng), np.float32)
        return field, centre, dyn, near, extra

    def _replan_state(self, p, k, context, ep: _Episode, B, best_host, noise, x_clean, hist_dev):
        """The environment step of the reference's last DDIM step (diffusion_model_dynamic.py:396-411) as a ramp_replan_state: the
        pursuer sees x[:, stepp, :2], which is the pinned executed state of every candidate.  Returns (state, near, its host arrays)."""
        field, centre, dyn, near, extra = self._environment_step(k, context, ep, B, best_host)
        p.static_pts, p.n_static = _lib.ptr(field._static_dev), field._static_dev.shape[0]
        assert dyn.shape == (p.n_dyn, 2)
        st = _lib.RampReplanState()
        st.noise, st.x_clean, st.history = _lib.ptr(noise), _lib.ptr(x_clean), _lib.ptr(hist_dev)
        st.n_hist, st.stepp = len(ep.executed_history), ep.stepp
        st.dyn_pts_host = dyn.ctypes.data
        st.pursuer[0], st.pursuer[1] = float(np.float32(centre[0])), float(np.float32(centre[1]))
        st.near = int(near)
        st.extra_pts_host = extra.ctypes.data if near else None
        return st, near, (dyn, extra, centre)

    # ------------------------------------------------------------------ cost guidance inside the replans (replan_guide=)
    def _replan_guide_setup(self, replan_guide, low, clouds, arrays: _HostArrays):
        """``replan_guide=`` of an episode (``clouds``: one static cost cloud) or of a many-episode job (one per episode) as a
        ramp_replan_guide whose moving points and tracks are filled per replan by ``_replan_guide_update``.  Returns None without a guide
        iteration anywhere (the unguided job), else a namespace (rg, tab, mov, track, prev) that owns every table."""
        from types import SimpleNamespace
        from .guide import cloud_table, fill_replan_guide, replan_guide_tables
        tab = replan_guide_tables(replan_guide, low)
        self.last_replan_guide = []
        if tab['total'] == 0:
            return None
        E, H = len(clouds), self.model.n_support_points
        own = tab['cloud']
        if own is not None:
            own = list(own) if isinstance(own, (list, tuple)) else [own] * E
            if len(own) != E:
                raise ValueError(f"replan_guide=: cloud has {len(own)} entries for {E} episodes")
            clouds = own
        points, off, d = cloud_table(clouds, self._device())
        if d != 2:
            raise ValueError("replan_guide=: the replanning jobs are 2-D; the guide cloud must be (P, 2)")
        n_mov = int(self.apf_dynamic['points_per_obstacle'])
        mov, track = np.zeros((E, n_mov, 2), np.float32), np.zeros((E, H, 2), np.float32)
        rg = fill_replan_guide(arrays.keep(points), arrays.keep(off), mov, track, tab)
        rg.n_guide, rg.step = arrays.i32(tab['n_guide']), arrays.f32(tab['step'])
        return SimpleNamespace(rg=rg, tab=tab, mov=mov, track=track, prev=[None] * E)

    @staticmethod
    def _replan_guide_update(gs, e, centre, dyn, plan_xy, stepp):
        """Episode ``e``'s moving cloud (the pursuer's sphere cloud of this environment step, as fp32) and its predicted track, in place in
        the guide's host tables; no random numbers."""
        from .guide import predict_track
        gs.mov[e] = dyn
        gs.track[e] = predict_track(gs.tab['predict'], centre, gs.prev[e], plan_xy, stepp)
        gs.prev[e] = np.array(centre, np.float64)

    def _replan_from_scratch(self, ep: _Episode, nb, shape, hard_conds, context, traj_normalized, k, cost_cloud):
        """One round of the reference's from-scratch re-plan (:591-605) with ``nb`` candidates: the winner, or None."""
        from .cost import compute_trajectory_costs
        new_hc = {kk: v[:nb].clone() for kk, v in hard_conds.items()}
        x = self.ddim_replan_scratch((nb, shape[1], shape[2]), new_hc, context, traj_normalized, forward_t=k,
                                     obstacle_pts=ep.cloud, use_apf=False, executed_history=ep.executed_history)
        window = 2
        x[:, ep.stepp + 1:ep.stepp + 1 + window] = self.sm(x[:, ep.stepp], x[:, ep.stepp + window], num_steps=window)
        x, _, _, _, _ = compute_trajectory_costs(x, cost_cloud, collision_threshold=ep.thr_low)
        return x

    def _replan_until_free(self, ep: _Episode, shape, hard_conds, context, traj_normalized, k, cost_cloud, best, sharded):
        """No candidate survived: the reference re-plans from scratch until one does (:591-605), eager path; the winner goes to ``best``.
        Sharded: the ranks re-plan round by round in LOCK-STEP (every rank draws the same number of torch / numpy random numbers,
        so their pursuer clouds stay identical afterwards, and nobody waits in a collective while another rank is still looping);
        after each round the lowest rank that found a collision-free plan broadcasts it."""
        from . import dist as rdist
        import torch.distributed as tdist
        device = self._device()
        nb = min(30, rdist.min_over_ranks(shape[0], device) if sharded else shape[0])      # the SAME count on every rank: equal RNG consumption
        while True:
            xs = self._replan_from_scratch(ep, nb, shape, hard_conds, context, traj_normalized, k, cost_cloud)
            if xs is not None:
                xs = xs.clone(); xs[0, 2:] = 0.0
                best.copy_(xs)
            if not sharded:
                if xs is not None:
                    break
                continue
            src = rdist.lowest_rank_with(xs is not None, device)
            if src >= 0:
                tdist.broadcast(best, src=src)
                break

    @torch.no_grad()
    def ddim_p_sample_loop(self, shape, hard_conds, context=None, return_chain=False, traj_normalized=None,
                           obstacle_pts=None, t_start_guide=float('inf'), guide=None, n_guide_steps=1,
                           max_iteration=60, replan_guide=None, **sample_kwargs):
        """Pursuit-evasion receding-horizon planner (diffusion_model_dynamic.py:495-624), MI355X-shaped: the 10-step
        high-level plan is ONE ``ramp_sample`` job and every replan ONE ``ramp_replan`` graph replay (q_sample of the
        current plan, 5 DDIM steps with the executed history / goal pinned, smoothing, static + pursuer APF on the last
        step, collision mask, costs, selection -- all on the device), with a 16-byte result record and the winning
        trajectory as the only read-backs.  Host work per replan is what the reference leaves to the environment: the
        pursuer's dynamics callback (fed x[:, stepp, :2], i.e. the pinned executed state, known before the replan starts),
        its re-sampled sphere cloud (numpy RNG, same call order as the reference) and the termination test.
        ``self.replan_log`` (a list, optional) receives every batch handed to a selection, for the parity tests.
        ``replan_guide=`` (a dict, ``ramp_amd.guide.replan_guide_tables``): cost-gradient steps inside every replan's graph
        (``ramp_replan_guided``) against the static cost cloud and the pursuer's sphere cloud moved along a predicted track;
        ``self.last_replan_guide`` then lists the (H, 2) track of every replan.  The reference's ``guide`` / ``n_guide_steps`` /
        ``t_start_guide`` stay accepted and ignored, as there.  The high-level plan and the from-scratch fallback are not guided."""
        from types import SimpleNamespace
        from . import dist as rdist
        import torch.distributed as tdist
        device = self._device()
        B, H, S = shape
        lib = _lib.load()
        m = self.model
        log = getattr(self, 'replan_log', None)
        # several GPUs: `shape[0]` is THIS rank's share of the candidates; every selection merges the ranks' candidates
        # (12 bytes per candidate all-gathered, the winner's owner broadcasts its trajectory: ramp_amd.dist.select_best_sharded),
        # so all ranks execute the same plan and feed the same environment
        sharded = tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
        if replan_guide is not None and sharded:
            raise NotImplementedError("replan_guide= under a multi-rank process group: sharding a guided replan is out of scope")
        # 1. set-up
        ep = _Episode(context, hard_conds, obstacle_pts, device, return_chain)
        cost_cloud = ep.cloud.reshape(-1, 2).to(torch.float32).contiguous()
        sel = SimpleNamespace(mask=torch.empty(B, dtype=torch.int32, device=device), plen=torch.empty(B, device=device),
                              smooth=torch.empty(B, device=device), best=torch.empty((H, S), device=device))
        # 2. STAGE I: high-level plan and selection
        ts = [int(i) for i in self.ddim_set_timesteps(self.ddim_num_inference_steps_high)]
        xb, x_plan = self._plan_high_level(shape, ts, hard_conds, ep, cost_cloud, sel, log, sharded)
        ep.start(x_plan)
        hist_dev = torch.zeros((H, S), device=device)
        hist_dev[0] = x_plan[0]
        best_host = x_plan.cpu().numpy()
        # 3. STAGE II: the replan's parameters
        arrays = _HostArrays()
        low = ts[-self.ddim_num_inference_steps_low:]
        p = self._replan_params(B, low, hard_conds, cost_cloud, ep.thr_low, arrays)
        gs = self._replan_guide_setup(replan_guide, low, [cost_cloud], arrays) if replan_guide is not None else None
        x_clean = x_plan.contiguous()
        want_batch = log is not None or sharded
        batch = torch.empty((B, H, S), device=device) if want_batch else None
        for k in range(max_iteration):
            # 4. the environment step
            noise = torch.randn_like(xb)                           # q_sample's randn_like(x_start)
            st, near, _host = self._replan_state(p, k, context, ep, B, best_host, noise, x_clean, hist_dev)
            if gs is not None:
                self._replan_guide_update(gs, 0, _host[2], _host[0], best_host[:, :2], ep.stepp)
                self.last_replan_guide.append(gs.track[0].copy())
            # 5. the replan: one graph replay
            res = _lib.RampReplanResult()
            with torch.cuda.device(device):
                _lib.check(lib.ramp_replan_guided(m.ctx(), C.byref(p), C.byref(st), C.byref(gs.rg) if gs is not None else None,
                                                  _lib.ptr(sel.best), _lib.ptr(batch), _lib.ptr(sel.mask) if want_batch else None,
                                                  C.byref(res), _lib.current_stream()), "ramp_replan_guided")
            if res.fell_back:
                self.range_fallbacks += 1
                warnings.warn(f"fp16x3 range guard tripped at GEMM call site {res.fell_back - 1}: replan repeated in bf16x6")
            if log is not None:
                log.append(dict(batch=batch.clone(), npts=cost_cloud.shape[0] + (64 if near else 0),
                                idx=res.best_rank if res.n_free else -1, free=(sel.mask == 0).clone()))
            # 6. merge over the ranks, from-scratch fallback, book-keeping
            n_free_all = res.n_free
            if sharded:                                            # the local winner is only a candidate: merge over the ranks
                with torch.cuda.device(device):
                    _lib.check(lib.ramp_replan_costs(m.ctx(), B, _lib.ptr(sel.mask), _lib.ptr(sel.plen), _lib.ptr(sel.smooth),
                                                     _lib.current_stream()), "ramp_replan_costs")
                merged, n_free_all, _ = rdist.select_best_sharded(batch, sel.mask, sel.plen, sel.smooth, 0.1, 0.9)
                if merged is not None:
                    sel.best.copy_(merged)
            if n_free_all == 0:
                self._replan_until_free(ep, shape, hard_conds, context, traj_normalized, k, cost_cloud, sel.best, sharded)
            x_cur = sel.best.clone()
            best_host = x_cur.cpu().numpy()
            x_clean = x_cur
            hist_dev[ep.stepp + 1] = x_cur[ep.stepp + 1]
            ep.record(x_cur)
            if ep.reached(float(np.linalg.norm(best_host[ep.stepp - 1, :2] - best_host[-1, :2]))):
                break
        return ep.result(x_cur)

    @torch.no_grad()
    def ddim_p_sample_loop_eager(self, shape, hard_conds, context=None, return_chain=False, traj_normalized=None,
                                 obstacle_pts=None, t_start_guide=float('inf'), guide=None, n_guide_steps=1,
                                 max_iteration=60, **sample_kwargs):
        """The same planner as a host loop over the step-at-a-time entry points (one launch sequence and several syncs
        per DDIM step): kept as the readable restatement the graph path is tested against."""
        from .apf_dynamic import generate_sphere_points
        from .cost import compute_trajectory_costs
        device = self._device()
        B = shape[0]
        x = torch.randn(shape, device=device)
        x = apply_hard_conditioning(x, hard_conds)
        ep = _Episode(context, hard_conds, obstacle_pts, device, return_chain)
        sphere, cloud = ep.sphere, ep.cloud                   # cloud (n_obstacles, n_points, 2); the reference replicates it per row
        cost_cloud = cloud.reshape(-1, 2)
        # STAGE I: high-level plan
        for i in self.ddim_set_timesteps(self.ddim_num_inference_steps_high):
            x = self._step(x, hard_conds, context, i, cloud, traj_normalized, None, False)
            x = apply_hard_conditioning(x, hard_conds)
        best_traj, _, _, _, _ = compute_trajectory_costs(x, cost_cloud, collision_threshold=ep.thr_high)
        if best_traj is None:
            raise RuntimeError("no collision-free high-level plan (the reference dereferences None here)")
        ep.start(best_traj)
        x = best_traj.clone()
        # STAGE II: receding-horizon replanning
        ts = self.ddim_set_timesteps(self.ddim_num_inference_steps_high)
        low = ts[-self.ddim_num_inference_steps_low:]
        for k in range(max_iteration):
            stepp = ep.stepp
            x_clean = x.clone()
            x = x.unsqueeze(0).repeat(B, 1, 1).contiguous()
            noise_t = torch.tensor([int(low[0])], device=device)
            x = self.q_sample(x, noise_t).contiguous()
            x[:, 0, 2:] = 0
            for h, st in enumerate(ep.executed_history):
                x[:, h] = st
            x[:, -1] = x_clean[-1]
            for i in low:
                use_apf = False
                if i == 0:
                    use_apf = True
                    window = 3
                    x[:, stepp + 1:stepp + 1 + window] = self.sm(x[:, stepp], x[:, stepp + window], num_steps=window)
                x = self._step(x, hard_conds, context, i, cloud, traj_normalized, k, use_apf)
                x = apply_hard_conditioning(x, hard_conds)
                for h, st in enumerate(ep.executed_history):
                    x[:, h] = st
                x[:, -1] = x_clean[-1]
                x[:, 0, 2:] = 0.0
            window = 2
            x[:, stepp + 1:stepp + 1 + window] = self.sm(x[:, stepp], x[:, stepp + window], num_steps=window)
            near = np.linalg.norm(x[0, stepp, :2].cpu().numpy() - sphere.centers[0].cpu().numpy()) < ep.distance_threshold_pred
            if near:
                pts = generate_sphere_points(sphere.centers[0].cpu().numpy(), sphere.radii[0].cpu().numpy(), 64)
                allpts = torch.cat([cost_cloud, torch.from_numpy(pts).to(device, cloud.dtype)])
                x, _, _, _, _ = compute_trajectory_costs(x, allpts, collision_threshold=ep.thr_low)
            else:
                x, _, _, _, _ = compute_trajectory_costs(x, cost_cloud, collision_threshold=ep.thr_low)
            while x is None:      # the reference hard-codes a (30, 48, 4) batch
                x = self._replan_from_scratch(ep, min(30, B), shape, hard_conds, context, traj_normalized, k, cost_cloud)
            x = x.clone()
            x[0, 2:] = 0.0
            ep.record(x)
            if ep.reached(torch.norm(x[ep.stepp - 1, :2] - x[-1, :2])):
                break
        return ep.result(x)


    # ------------------------------------------------------------------ many episodes in lock-step, one graph per replan iteration
    def _check_episode_lists(self, contexts, hard_conds, obstacle_pts, n_samples, rngs):
        """The refusals of ``run_inference_episodes`` that need no device work: returns the per-episode candidate counts."""
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            raise NotImplementedError("run_inference_episodes under a multi-rank process group: sharding a many-episode job is out of scope")
        E = len(contexts)
        if E == 0:
            raise ValueError("no episodes given")
        counts = [int(n_samples)] * E if isinstance(n_samples, (int, np.integer)) else [int(n) for n in n_samples]
        for name, v in (('hard_conds', hard_conds), ('obstacle_pts', obstacle_pts), ('n_samples', counts), ('rngs', rngs)):
            if v is not None and len(v) != E:
                raise ValueError(f"{name} has {len(v)} entries for {E} episodes")
        if min(counts) <= 0:
            raise ValueError("every episode needs at least one candidate")
        k0 = list(hard_conds[0].keys())
        for e, h in enumerate(hard_conds):
            if list(h.keys()) != k0:
                raise ValueError(f"episode {e} conditions waypoints {list(h.keys())}, episode 0 {k0}: every episode of a job must "
                                 "condition the same waypoints in the same order")
        if 2 * sum(counts) > self.model.max_rows:
            raise ValueError(f"{sum(counts)} candidates are {2 * sum(counts)} network rows, beyond the network's max_rows = {self.model.max_rows}")
        return counts

    @torch.no_grad()
    def run_inference_episodes(self, contexts, hard_conds, obstacle_pts, n_samples=35, rngs=None, return_chain=False,
                               max_iteration=60, traj_normalized=None, replan_guide=None):
        """MANY pursuit-evasion episodes in ONE job per replan iteration: the loop over contexts and experiments of the reference's
        scripts/inference/inference_dynamic.py (``run_multiple_experiments``: one ``run_inference`` per episode, each up to 60 replans of
        35 candidates) advanced in lock-step, so that a replan is E x n rows wide instead of n.

        contexts      list of per-episode contexts (``{'dataset': ...}``: each episode its own environment)
        hard_conds    list of one dict per episode, the same waypoint indices in every episode; values (S,) or (n_e, S)
        obstacle_pts  list of per-episode clouds (n_obstacles, n_points, 2); shapes may differ
        n_samples     candidates per episode: an int, or one count per episode
        rngs          list of ``numpy.random.RandomState`` (or None = the global ``numpy.random`` for all): the stream episode e's
                      APF clouds, pursuer clouds and cost points are drawn from, in the one-episode planner's order

        STAGE I is one many-scene DDIM job (``ramp_sample_scenes``) and one per-episode selection (``ramp_select_best_scenes``);
        STAGE II loops while any episode is active: per active episode the environment step, then ONE ``ramp_replan_episodes`` call
        for all, then the per-episode book-keeping.  An episode that has reached its goal or ``max_iteration`` keeps its rows in the
        batch (the job's shape, buffers and graph never change) and its results are ignored.  An episode without a collision-free
        candidate falls back to the eager from-scratch re-plan of the one-episode planner, alone; that path installs a single scene,
        so the job's scene table is installed again afterwards and the next call calibrates.
        ``self.replan_log`` (a list, optional) receives one entry per selection and episode: ``episode``, ``active``, ``record`` (the
        episode's result record of that call) and, for an active episode, ``batch``, ``npts``, ``idx``, ``free``.
        ``replan_guide=``: as in ``ddim_p_sample_loop``, one launch per guided DDIM step for all episodes (``ramp_replan_episodes_guided``);
        ``cloud`` may list one static guide cloud per episode; ``self.last_replan_guide`` lists the (E, H, 2) tracks of every call.

        Returns a list with, per episode, what ``run_inference`` returns: ``(chain (iters, 1, H, S), chain_obs, chain_start)`` if
        ``return_chain`` else the final plan (1, H, S).  Raises ``NotImplementedError`` under a multi-rank process group and
        ``ValueError`` for lists of different lengths, differing hard-condition keys or more than ``max_rows`` network rows."""
        from .scenes import build_episode_tables
        counts = self._check_episode_lists(contexts, hard_conds, obstacle_pts, n_samples, rngs)
        device, m, lib = self._device(), self.model, _lib.load()
        E, B, H, S = len(contexts), sum(counts), m.n_support_points, self.state_dim
        rngs = [np.random] * E if rngs is None else list(rngs)
        log = getattr(self, 'replan_log', None)
        tab = build_episode_tables(counts, [self._row_pattern(n) for n in counts])
        first = [int(v) for v in tab['traj_first']]
        rows = [slice(first[e], first[e + 1]) for e in range(E)]
        # 1. set-up: per-episode contexts, hard conditions of the whole batch, cost clouds, the job's scene table
        contexts = [copy(c) for c in contexts]
        hcs = []                                               # per episode, expanded to its rows: what the eager fallback takes
        for h, n in zip(hard_conds, counts):
            hc = {}
            for kk, v in h.items():
                v = v.to(device, torch.float32)
                hc[kk] = (v.unsqueeze(0).expand(n, -1) if v.dim() == 1 else v).contiguous()
                if hc[kk].shape[0] != n:
                    raise ValueError(f"hard condition {kk}: {hc[kk].shape[0]} rows for an episode of {n} candidates")
            hcs.append(hc)
        hard = {kk: torch.cat([hc[kk] for hc in hcs]).contiguous() for kk in hcs[0]}
        eps = [_Episode(c, hc, pts, device, True) for c, hc, pts in zip(contexts, hcs, obstacle_pts)]
        clouds = [ep.cloud.reshape(-1, 2).to(torch.float32).contiguous() for ep in eps]
        cost_cloud = torch.cat(clouds).contiguous()
        cost_off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int32)
        m.ctx()
        latents = torch.cat([m.encode_scenes([ep.cloud for ep in eps]), torch.zeros(1, m.context_dim, device=device)])
        m.set_scenes(latents, tab['row_variant'])
        first_dev = torch.from_numpy(tab['traj_first']).to(device)
        mask, plen, smooth = torch.empty(B, dtype=torch.int32, device=device), torch.empty(B, device=device), torch.empty(B, device=device)
        best = torch.empty((E, H, S), device=device)
        # 2. STAGE I: one many-scene DDIM job, one selection per episode (the winner unmodified, as the high-level plan wants)
        ts = [int(i) for i in self.ddim_set_timesteps(self.ddim_num_inference_steps_high)]
        x = torch.randn((B, H, S), device=device)
        job = {'n_scenes': E, 'traj_scene': torch.from_numpy(tab['row_episode']).to(device), 'cloud_offset': None, 'cloud_points': None}
        xb, _ = self._launch(B, x.unsqueeze(0), hard, None, True, ts, [0] * len(ts), None, None, False,
                             ddim_K=self.ddim_num_inference_steps_high, scene_job=job)
        res_dev = torch.zeros((E, 4), dtype=torch.int32, device=device)
        cost_off_dev = torch.from_numpy(cost_off).to(device)
        with torch.cuda.device(device):
            _lib.check(lib.ramp_select_best_scenes(_lib.ptr(xb), B, H, S, _lib.ptr(first_dev), E, _lib.ptr(cost_cloud),
                                                   _lib.ptr(cost_off_dev), cost_cloud.shape[0], eps[0].thr_high,
                                                   0.1, 0.9, _lib.ptr(mask), _lib.ptr(plen), _lib.ptr(smooth), _lib.ptr(best),
                                                   _lib.ptr(res_dev), _lib.current_stream()), "ramp_select_best_scenes")
        res = res_dev.cpu().numpy()
        for e, ep in enumerate(eps):
            n_free, rank, row = (int(v) for v in res[e, :3])
            if log is not None:
                log.append(dict(episode=e, active=True, record=[int(v) for v in res[e]], batch=xb[rows[e]].clone(), npts=clouds[e].shape[0],
                                idx=rank if n_free else -1, free=(mask[rows[e]] == 0).clone()))
            if n_free == 0:
                raise RuntimeError(f"episode {e}: no collision-free high-level plan (the reference dereferences None here)")
            ep.start(xb[row].clone())
        cur = best.clone()                                    # (E, H, S) current plans, and their host copy
        best_host = cur.cpu().numpy()
        hist = torch.zeros((E, H, S), device=device)
        hist[:, 0] = best[:, 0]
        # 3. STAGE II: what the episodes share, and the per-episode tables of the call
        arrays = _HostArrays()
        p = self._replan_params(B, ts[-self.ddim_num_inference_steps_low:], hard, cost_cloud, eps[0].thr_low, arrays)
        p.cost_cloud, p.n_cost = None, 0                      # (the clouds come per episode)
        gs = None
        if replan_guide is not None:
            gs = self._replan_guide_setup(replan_guide, ts[-self.ddim_num_inference_steps_low:], clouds, arrays)
        n_dyn, n_extra = p.n_dyn, p.n_extra
        state = (_lib.RampEpisodeState * E)()
        dyn = np.zeros((E, n_dyn, 2), np.float64)
        near = np.zeros(E, np.int32)
        extra = np.zeros((E, n_extra, 2), np.float32)
        eb = _lib.RampEpisodeBatch()
        eb.n_episodes = E
        eb.traj_first_host = tab['traj_first'].ctypes.data_as(_lib.c_i32p)
        eb.state_host = state
        eb.dyn_pts_host, eb.near_host, eb.extra_pts_host = dyn.ctypes.data, near.ctypes.data_as(_lib.c_i32p), extra.ctypes.data
        eb.cost_cloud, eb.cost_offset_host = _lib.ptr(cost_cloud), cost_off.ctypes.data_as(_lib.c_i32p)
        active = [True] * E
        x_clean = best.clone()                                # explicit on the first call and after a fallback; else the previous winners
        static_pts = static_off = None
        want_batch = log is not None
        batch = torch.empty((B, H, S), device=device) if want_batch else None
        results = np.zeros((E, 4), np.int32)
        for k in range(max_iteration):
            if not any(active):
                break
            # 4. the environment step of every active episode
            noise = torch.randn_like(xb)                           # q_sample's randn_like(x_start), all episodes' rows
            fields = []
            for e, ep in enumerate(eps):
                state[e].active = int(active[e])
                if not active[e]:
                    continue
                field, centre, dyn[e], near_e, extra_e = self._environment_step(k, contexts[e], ep, counts[e], best_host[e], rngs[e])
                fields.append(field)
                near[e] = int(near_e)
                if near_e:
                    extra[e] = extra_e
                state[e].n_hist, state[e].stepp = len(ep.executed_history), ep.stepp
                state[e].pursuer[0], state[e].pursuer[1] = float(np.float32(centre[0])), float(np.float32(centre[1]))
                if gs is not None:
                    self._replan_guide_update(gs, e, centre, dyn[e], best_host[e][:, :2], ep.stepp)
            if gs is not None:
                self.last_replan_guide.append(gs.track.copy())
            if static_pts is None:                                 # (every field exists after the first step: all episodes start active)
                static_pts = torch.cat([f._static_dev for f in fields]).contiguous()
                static_off = np.concatenate([[0], np.cumsum([f._static_dev.shape[0] for f in fields])]).astype(np.int32)
                eb.static_pts, eb.static_offset_host = _lib.ptr(static_pts), static_off.ctypes.data_as(_lib.c_i32p)
            eb.noise, eb.history, eb.x_clean = _lib.ptr(noise), _lib.ptr(hist), _lib.ptr(x_clean)
            # 5. the replan of all episodes: one graph replay
            rr = _lib.RampReplanResult()
            with torch.cuda.device(device):
                _lib.check(lib.ramp_replan_episodes_guided(m.ctx(), C.byref(p), C.byref(eb), C.byref(gs.rg) if gs is not None else None,
                                                           _lib.ptr(best), _lib.ptr(batch), _lib.ptr(mask) if want_batch else None,
                                                           results.ctypes.data_as(_lib.c_i32p), C.byref(rr), _lib.current_stream()),
                           "ramp_replan_episodes_guided")
            if rr.fell_back:
                self.range_fallbacks += 1
                warnings.warn(f"fp16x3 range guard tripped at GEMM call site {rr.fell_back - 1}: replan repeated in bf16x6")
            x_clean = None
            # 6. from-scratch fallback (one episode alone, eager), then the book-keeping of every active episode
            for e, ep in enumerate(eps):
                if log is not None and not active[e]:
                    log.append(dict(episode=e, active=False, record=results[e].tolist()))
                elif log is not None:
                    log.append(dict(episode=e, active=True, record=results[e].tolist(), batch=batch[rows[e]].clone(),
                                    npts=clouds[e].shape[0] + (n_extra if near[e] else 0),
                                    idx=int(results[e, 1]) if results[e, 0] else -1, free=(mask[rows[e]] == 0).clone()))
                if active[e] and results[e, 0] == 0:
                    self._replan_until_free(ep, (counts[e], H, S), hcs[e], contexts[e], traj_normalized, k, clouds[e], best[e], False)
                    x_clean = best                                 # the next call takes its plans from here, not from its own winners
            if x_clean is not None:
                m.set_scenes(latents, tab['row_variant'])          # (the eager path installed one episode's scene)
            cur = best.clone()
            best_host = cur.cpu().numpy()
            moved = [e for e in range(E) if active[e]]
            at = torch.tensor([eps[e].stepp + 1 for e in moved], device=device)
            sel = torch.tensor(moved, device=device)
            hist[sel, at] = cur[sel, at]
            for e in moved:
                ep = eps[e]
                ep.record(cur[e])
                if ep.reached(float(np.linalg.norm(best_host[e][ep.stepp - 1, :2] - best_host[e][-1, :2]))):
                    active[e] = False
        out = []
        for e, ep in enumerate(eps):
            _x, chain, chain_obs, chain_start = ep.result(cur[e])
            chain = chain.permute(1, 0, 2, 3)
            out.append((chain, chain_obs, chain_start) if return_chain else chain[-1])
        return out

    @torch.no_grad()
    def conditional_sample(self, hard_conds, horizon=None, batch_size=1, ddim=False, traj_normalized=None,
                           obstacle_pts=None, **sample_kwargs):
        horizon = horizon or self.model.n_support_points
        shape = (batch_size, horizon, self.state_dim)
        if sample_kwargs.get('mcmc') is not None:
            raise NotImplementedError("mcmc=: DynamicGaussianDiffusionModel has no Langevin refinement (the replanning jobs are out of scope)")
        if sample_kwargs.get('cost_guide') is not None:
            raise NotImplementedError("cost_guide=: DynamicGaussianDiffusionModel has no cost guide of the sampling jobs' kind (the replanning jobs take replan_guide=)")
        if sample_kwargs.get('resample') is not None:
            raise NotImplementedError("resample=: DynamicGaussianDiffusionModel has no resampling (the replanning jobs are out of scope)")
        if sample_kwargs.get('warm_start') is not None:
            raise NotImplementedError("warm_start=: DynamicGaussianDiffusionModel keeps its own replanning (every replan already starts from "
                                      "the running plan noised to an intermediate level)")
        for k in ('sample_fn', 'n_diffusion_steps_without_noise', 'noise_std_extra_schedule_fn'):
            sample_kwargs.pop(k, None)
        return self.ddim_p_sample_loop(shape, hard_conds, traj_normalized=traj_normalized, obstacle_pts=obstacle_pts,
                                       **sample_kwargs)

    @torch.no_grad()
    def run_inference(self, context=None, hard_conds=None, n_samples=1, return_chain=False, traj_normalized=None,
                      obstacle_pts=None, **diffusion_kwargs):
        """diffusion_model_dynamic.py:649-667: (chain (iters, 1, H, S), chain_obs, chain_start) if return_chain."""
        hard_conds = copy(hard_conds)
        context = copy(context)
        for k, v in hard_conds.items():
            hard_conds[k] = v.to(self._device()).unsqueeze(0).expand(n_samples, -1).contiguous() if v.dim() == 1 else v
        samples, chain, chain_obs, chain_start = self.conditional_sample(
            hard_conds, context=context, batch_size=n_samples, return_chain=True, traj_normalized=traj_normalized,
            obstacle_pts=obstacle_pts, **diffusion_kwargs)
        chain = chain.permute(1, 0, 2, 3)
        if return_chain:
            return chain, chain_obs, chain_start
        return chain[-1]
