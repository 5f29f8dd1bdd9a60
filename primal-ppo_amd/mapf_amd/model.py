"""Model: action sampling, value bootstrap and the PPO-Lagrangian update.

Mirrors the reference's Model (model.py:13-231) and Lagrangian multipliers
(lagrange.py:26-88), with the device-resident pieces of the hot path:
  * step(): the policy forward + on-device categorical sampling (mapf_sample_actions
    in place of np.random.choice, model.py:38-40);
  * train(): advantage normalisation by the HIP kernels (mapf_normalize_advantages_dlam,
    model.py:106-113) -- statistics over the GLOBAL minibatch when distributed (two-pass
    fp64 moments all-reduced, mapf_normalize_advantages_stats_dlam; _DeviceUpdate.body) --
    then the reference's loss (:115-170), AMP GradScaler, and between backward and
    unscale the RCCL all-reduce of the flattened gradient bucket (SURVEY.md §3.4:
    the only exchange step of the path).  Every rank then holds the same gradient, so
    found-inf, clipping, Adam and the loss scale agree across ranks; the returned stats are
    averaged over the ranks (the global minibatch's means when the shards are equal);
  * imitation_train() / imitate_rows(): the behaviour-cloning update (model.py:205-231) -- the
    cross-entropy of the policy logits against an expert's actions and its gradient in one HIP
    launch (mapf_imitation_loss), then train()'s own AMP / clip / Adam tail (_DeviceImitation).
"""
import ctypes

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _lib
from .config import EnvParameters, LagrangianParameters, NetParameters, TrainingParameters
from .net import SCRIMPNet


class _FusedPPOLoss(torch.autograd.Function):
    """model.py:115-175's loss terms and their gradient in one HIP launch
    (csrc/mapf_ppo.hip, mapf_ppo_loss).  Returns (all_loss, terms[7] = policy, entropy,
    critic, valid, cost critic, cost, clip_frac); only all_loss carries a gradient."""

    @staticmethod
    def forward(ctx, new_ps, new_v, new_cv, policy_sig, old_ps, action, old_v, returns, old_cv, cost_returns,
                advantage, cost_advantage, train_valid, coef):
        A = new_ps.shape[-1]
        R = new_ps.numel() // A
        f = lambda t, *shape: t.detach().float().reshape(*shape).contiguous()
        ins = [f(new_ps, R, A), f(old_ps, R, A), action.detach().long().reshape(R).contiguous()]
        vecs = [f(t, R) for t in (new_v, old_v, returns, new_cv, old_cv, cost_returns, advantage, cost_advantage)]
        sig, tv = f(policy_sig, R, A), f(train_valid, R, A)
        loss = torch.empty((), device=new_ps.device)
        terms = torch.empty(7, device=new_ps.device)
        grads = [torch.empty(R, A, device=new_ps.device), torch.empty(R, device=new_ps.device),
                 torch.empty(R, device=new_ps.device), torch.empty(R, A, device=new_ps.device)]
        if isinstance(coef, torch.Tensor):     # device coefficients (the captured update)
            fn = "mapf_ppo_loss_dcoef"
        else:
            fn, coef = "mapf_ppo_loss", (ctypes.c_float * 6)(*coef)
        _lib.call(fn, *ins, *vecs, sig, int(policy_sig.dtype == torch.float16), tv, R, A, coef, loss, terms, *grads)
        ctx.save_for_backward(*grads)
        ctx.meta = [(t.shape, t.dtype) for t in (new_ps, new_v, new_cv, policy_sig)]
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        out = [(g * g_loss).reshape(shape).to(dtype) for g, (shape, dtype) in zip(ctx.saved_tensors, ctx.meta)]
        return (*out,) + (None,) * 10


class _FusedImitationLoss(torch.autograd.Function):
    """model.py:221-222's cross-entropy and its gradient in one HIP launch (csrc/mapf_imitation.hip,
    mapf_imitation_loss).  logits [..., A] fp32 or fp16 (the autocast policy layer's output, read as
    it is), action [...] int32 or int64 (read as it is).  Returns (imitation_loss, terms[2] =
    agreement with the expert, the expert action's mean probability); only the loss carries a
    gradient."""

    @staticmethod
    def forward(ctx, logits, action):
        A = logits.shape[-1]
        R = logits.numel() // A
        lg = logits.detach()
        if lg.dtype not in (torch.float32, torch.float16):
            lg = lg.float()
        lg = lg.reshape(R, A).contiguous()
        act = action.detach()
        if act.dtype not in (torch.int32, torch.int64):
            act = act.long()
        act = act.reshape(R).contiguous()
        loss = torch.empty((), device=logits.device)
        terms = torch.empty(2, device=logits.device)
        grad = torch.empty(R, A, device=logits.device)
        _lib.call("mapf_imitation_loss", lg, int(lg.dtype == torch.float16), act, int(act.dtype == torch.int64), R, A,
                  loss, terms, grad)
        ctx.save_for_backward(grad)
        ctx.meta = (logits.shape, logits.dtype)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        grad, = ctx.saved_tensors
        shape, dtype = ctx.meta
        return (grad * g_loss).reshape(shape).to(dtype), None


class Lagrangian:
    """lagrange.py:26-53: softplus-parameterised multiplier trained by Adam."""

    def __init__(self, cost_limit):
        self.cost_limit = cost_limit
        self.lagrangian_param = torch.tensor(max(0.0, LagrangianParameters.INIT_VALUE), requires_grad=True).float()
        self.lagrangian_optimizer = torch.optim.Adam([self.lagrangian_param], lr=LagrangianParameters.LR)

    def get_lagrangian_param(self):
        return F.softplus(self.lagrangian_param).detach().item()

    def update_lagrangian_multiplier(self, ep_cost_avg):
        loss = -self.lagrangian_param * (ep_cost_avg - self.cost_limit)
        self.lagrangian_optimizer.zero_grad()
        loss.backward()
        self.lagrangian_optimizer.step()
        self.lagrangian_param.data.clamp_(0.0, LagrangianParameters.UPPER_BOUND)


class PIDLagrangian:
    """lagrange.py:55-88: PID-controlled multiplier (CPPO-PID)."""

    def __init__(self, cost_limit):
        self.cost_limit = cost_limit
        self.i_term = max(0.0, LagrangianParameters.INIT_VALUE)
        self.lagrangian_param = 0.0
        self.delta_moving_avg = 0.0
        self.cost_moving_avg = 0.0
        self.cost_moving_avg_prev = 0.0

    def get_lagrangian_param(self):
        return self.lagrangian_param

    def update_lagrangian_multiplier(self, ep_cost_avg):
        P = LagrangianParameters
        delta = ep_cost_avg - self.cost_limit
        self.delta_moving_avg = self.delta_moving_avg * P.DELTA_MOVING_AVG_ALPHA + (1 - P.DELTA_MOVING_AVG_ALPHA) * delta
        self.cost_moving_avg = self.cost_moving_avg * P.COST_MOVING_AVG_ALPHA + (1 - P.COST_MOVING_AVG_ALPHA) * ep_cost_avg
        d_term = max(0.0, self.cost_moving_avg - self.cost_moving_avg_prev)
        self.i_term = max(0.0, self.i_term + delta * P.KI)
        self.lagrangian_param = max(0.0, P.KP * self.delta_moving_avg + self.i_term + P.KD * d_term)
        self.cost_moving_avg_prev = self.cost_moving_avg


def get_lagrangian(kind, cost_limit):
    return Lagrangian(cost_limit) if kind == 0 else PIDLagrangian(cost_limit)


def _normalize(x):
    """model.py:106: (x - mean) / (std_unbiased + 1e-6); global statistics across ranks."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        s = torch.stack([x.sum(), (x * x).sum(), torch.tensor(float(x.numel()), device=x.device)]).double()
        dist.all_reduce(s)
        n = s[2]
        mean = s[0] / n
        var = (s[1] - n * mean * mean) / (n - 1)
        return (x - mean.float()) / (var.clamp_min(0).sqrt().float() + 1e-6)
    return (x - x.mean()) / (x.std() + 1e-6)


class Model:
    # PyTorch TunableOp with the shipped per-shape GEMM solutions (gemm_tuning.py).  PROCESS-WIDE: once a
    # CUDA Model is built, every later GEMM of the process whose shape is in the file (user code too)
    # takes the listed hipBLASLt solution.  Set Model.tuned_gemms = False before the first Model to keep
    # torch's defaults (or set PYTORCH_TUNABLEOP_ENABLED yourself).
    tuned_gemms = True

    def __init__(self, env_id, device, global_model=False, numChannel=None, num_agents=None, fov=None):
        self.ID = env_id
        self.device = torch.device(device)
        self.network = SCRIMPNet(numChannel=numChannel, num_agents=num_agents, fov=fov).to(self.device)
        if self.device.type == "cuda":     # NHWC convolutions: no layout transposes around MIOpen's kernels
            self.network = self.network.to(memory_format=torch.channels_last)
            if self.tuned_gemms:
                from .gemm_tuning import use_tuned_gemms
                use_tuned_gemms()          # the measured-best hipBLASLt solution per GEMM shape (gemm_tuning.py)
            # MIOpen find mode: the per-shape conv solver is measured once and cached
            # (c3 policy forward 23.1 -> 20.7 ms at 32,768 agents)
            torch.backends.cudnn.benchmark = True
        self.num_agents = num_agents or EnvParameters.N_AGENTS
        self._flat = None
        self.fused_loss = True        # GPU: the loss terms + their gradient in one launch (_FusedPPOLoss)
        self.graph_update = True      # GPU: the update replayed from captured hipGraphs (_DeviceUpdate)
        self.distributed_update = None  # None: the all-reduced update when world size > 1; True / False: forced
        self._updates = {}
        if global_model:
            # fused Adam on the GPU: one launch for every parameter, and the AMP found-inf skip taken
            # on the device (optimizer.found_inf), so the update has no host synchronisation
            gpu = self.device.type == "cuda"
            self.net_optimizer = torch.optim.Adam(self.network.parameters(), lr=TrainingParameters.lr, fused=gpu,
                                                  capturable=gpu)
            self.lagrange = get_lagrangian(LagrangianParameters.LAGRANGIAN_TYPE, TrainingParameters.COST_LIMIT_PER_AGENT)
            self.net_scaler = torch.amp.GradScaler(self.device.type, enabled=self.device.type == "cuda")
            self.broadcast_weights()

    def broadcast_weights(self, src=0):
        """SURVEY.md §8(e) "weights broadcast at init": when torch.distributed is initialised with
        more than one rank, every rank takes rank `src`'s parameters and buffers (one RCCL / gloo
        broadcast per dtype bucket), so ranks constructed with different seeds hold one model
        before the first all-reduced update (the reference has one global model, driver.py:50).
        Collective: every rank must construct its global Model (or call this) in the same order.
        Returns True if a broadcast ran."""
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return False
        tensors = list(self.network.parameters()) + list(self.network.buffers())
        for dtype in sorted({t.dtype for t in tensors}, key=str):
            group = [t for t in tensors if t.dtype == dtype]
            flat = torch.cat([t.detach().reshape(-1) for t in group])
            dist.broadcast(flat, src)
            off = 0
            with torch.no_grad():
                for t in group:      # copy_ bumps the version: the fp16 weight cache (acting.half) re-reads
                    t.copy_(flat[off:off + t.numel()].view_as(t))
                    off += t.numel()
        return True

    # ------------------------------------------------------------ acting
    @torch.no_grad()
    def step(self, observation, vector, input_state=None, seed=0, step=0, actions_out=None, actions32_out=None):
        """model.py:26-41 on device: returns (actions int64, ps, v, block, output_state, cv) as tensors.
        Sampling: inverse CDF with a Philox uniform (mapf_sample_actions); actions32_out: also
        write the actions as int32 (the env's action format) in the same launch."""
        ps, v, block, _, out_state, _, cv = self.network(observation, vector, input_state)
        ps32 = ps.float().contiguous()
        if self.device.type == "cuda":
            from .env import sample_actions
            a = actions_out if actions_out is not None else torch.empty(ps32.shape[:-1], dtype=torch.int64,
                                                                         device=self.device)
            sample_actions(ps32, seed, step, out32=actions32_out, out64=a)
        else:
            a = torch.multinomial(ps32.reshape(-1, ps32.shape[-1]), 1).reshape(ps32.shape[:-1])
        return a, ps32, v.float(), block.float(), out_state, cv.float()

    @torch.no_grad()
    def value(self, obs, vector, input_state=None):
        """model.py:62-69."""
        _, v, _, _, _, _, cv = self.network(obs, vector, input_state)
        return v.float(), cv.float()

    def set_weights(self, weights):
        self.network.load_state_dict(weights)

    # ------------------------------------------------------------ learning
    def _allreduce_grads(self):
        """One bucketed all-reduce (RCCL over xGMI) of every gradient, averaged over ranks."""
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        params = [p for p in self.network.parameters() if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        dist.all_reduce(flat)
        flat.div_(dist.get_world_size())
        off = 0
        for p in params:
            n = p.grad.numel()
            p.grad.copy_(flat[off:off + n].view_as(p.grad))
            off += n

    def train(self, observation, vector, returns, cost_returns, old_v, old_cv, action, old_ps, input_state,
              train_valid, episode_cost):
        """model.py:78-199.  Inputs may be numpy arrays (reference contract) or device tensors."""
        dev = self.device
        t = lambda x: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(dev)
        observation, vector = t(observation), t(vector)
        if observation.dtype == torch.int32:       # packed (one bit per cell): the update reads floats
            from .env import unpack_obs
            observation = unpack_obs(observation.contiguous(), self.network.num_channel, self.network.fov)
        returns, old_v, cost_returns, old_cv = t(returns).float(), t(old_v).float(), t(cost_returns).float(), t(old_cv).float()
        action = t(action).long().unsqueeze(-1)
        old_ps, train_valid = t(old_ps).float(), t(train_valid).float()

        lam = self.lagrange.get_lagrangian_param()
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if self.distributed_update is not None:     # forced (measurement: the c4 path at world size 1)
            distributed = bool(self.distributed_update) and dist.is_available() and dist.is_initialized()
        if dev.type == "cuda" and self.fused_loss:      # the device update (fused loss, captured graph)
            return self._train_device(observation, vector, returns, cost_returns, old_v, old_cv, action, old_ps,
                                      input_state, train_valid, episode_cost, lam, distributed)
        if dev.type == "cuda":
            # the HIP normalisation; distributed: global two-pass moments all-reduced into it
            from .env import normalize_advantages, normalize_advantages_distributed
            fn = normalize_advantages_distributed if distributed else normalize_advantages
            advantage, cost_advantage = fn(returns.contiguous(), old_v.contiguous(), cost_returns.contiguous(),
                                           old_cv.contiguous(), lagrange=lam, mix=TrainingParameters.MINUS_ADV_WITH_CADV)
        else:                   # CPU (the gloo tests' host path): torch, global statistics when distributed
            advantage = _normalize(returns - old_v)
            cost_advantage = _normalize(cost_returns - old_cv)
            if TrainingParameters.MINUS_ADV_WITH_CADV:
                advantage = (advantage - lam * cost_advantage) / (lam + 1)

        self.net_optimizer.zero_grad()
        with torch.autocast(device_type=dev.type, enabled=dev.type == "cuda"):
            new_ps, new_v, block, policy_sig, _, _, new_cv = self.network(observation, vector, input_state)
            new_p = new_ps.gather(-1, action)
            old_p = old_ps.gather(-1, action)
            ratio = torch.exp(torch.log(torch.clamp(new_p, 1e-6, 1.0)) - torch.log(torch.clamp(old_p, 1e-6, 1.0)))
            entropy = torch.mean(-torch.sum(new_ps * torch.log(torch.clamp(new_ps, 1e-6, 1.0)), dim=-1, keepdim=True))
            clip = TrainingParameters.CLIP_RANGE
            new_v = torch.squeeze(new_v)
            v_clip = old_v + torch.clamp(new_v - old_v, -clip, clip)
            critic_loss = torch.mean(torch.maximum(torch.square(new_v - returns), torch.square(v_clip - returns)))
            new_cv = torch.squeeze(new_cv)
            cv_clip = old_cv + torch.clamp(new_cv - old_cv, -clip, clip)
            cost_critic_loss = torch.mean(torch.maximum(torch.square(new_cv - cost_returns),
                                                        torch.square(cv_clip - cost_returns)))
            ratio = torch.squeeze(ratio)
            policy_loss = torch.mean(torch.min(advantage * ratio, advantage * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)))
            valid_loss = -torch.mean(torch.log(torch.clamp(policy_sig, 1e-6, 1.0 - 1e-6)) * train_valid +
                                     torch.log(torch.clamp(1 - policy_sig, 1e-6, 1.0 - 1e-6)) * (1 - train_valid))
            cost_loss = torch.mean(ratio * cost_advantage)
            all_loss = (-policy_loss - entropy * TrainingParameters.ENTROPY_COEF
                        + TrainingParameters.VALUE_COEF * critic_loss + TrainingParameters.VALID_COEF * valid_loss
                        + TrainingParameters.COST_VALUE_COEF * cost_critic_loss
                        + TrainingParameters.COST_COEF * lam * cost_loss)
        clip_frac = torch.mean(torch.greater(torch.abs(ratio - 1.0), clip).float())
        return self._finish_update(all_loss, policy_loss, entropy, critic_loss, valid_loss, cost_critic_loss,
                                   cost_loss, clip_frac, advantage, cost_advantage, episode_cost, distributed)

    # ------------------------------------------------------------ the device update
    def _train_device(self, observation, vector, returns, cost_returns, old_v, old_cv, action, old_ps, input_state,
                      train_valid, episode_cost, lam, distributed):
        """model.py:78-199 on the GPU with no host synchronisation inside the update: HIP
        normalisation (multiplier in device memory), autocast forward, the fused loss (its
        coefficients in device memory), backward, [RCCL all-reduce of the gradient bucket],
        AMP unscale + found-inf on the device, clip, fused Adam skipping on found-inf, loss-scale
        update -- GradScaler's semantics (init 2^16, x2 every 2000 finite steps, x0.5 on inf).
        After two eager updates of a minibatch shape the body is captured and every later update of
        that shape replays it (the host launched ~1,500 small ops per update): one hipGraph on one
        rank; distributed, two graph segments with the collectives between them run eagerly -- the
        advantage moments' two all-reduces (global statistics) before segment A (normalise ->
        forward -> loss -> backward into a static gradient bucket), the bucket's all-reduce between
        backward and unscale (model.py:177-185), segment B (unscale -> clip -> Adam -> scale update),
        then the stats' all-reduce (_DeviceUpdate.run).  input_state is ignored, as the network ignores it (net.py:102-155 never
        reads it): driver.py passes the rollout's zero hiddenState rows, never None.
        The loss scale and its growth tracker are net_scaler's own tensors (one AMP state per
        model, as the reference's one GradScaler, shared by every minibatch shape and by the
        eager path)."""
        upd = self._device_update(observation, vector, returns, old_ps, train_valid, action)
        upd.load(observation, vector, returns, cost_returns, old_v, old_cv, action, old_ps, train_valid,
                 coef=self._loss_coef(lam), lam=lam)
        return self._run_device_update(upd, episode_cost, distributed)

    @staticmethod
    def _loss_coef(lam):
        T = TrainingParameters
        return (T.CLIP_RANGE, T.ENTROPY_COEF, T.VALUE_COEF, T.VALID_COEF, T.COST_VALUE_COEF, T.COST_COEF * lam)

    def _device_update(self, observation, vector, returns, old_ps, train_valid, action):
        """The _DeviceUpdate of this minibatch shape (the arguments give shapes only; a new one is made
        when net_scaler was replaced or reconfigured)."""
        key = (tuple(observation.shape), tuple(vector.shape), tuple(old_ps.shape), tuple(train_valid.shape))
        sc = self.net_scaler
        if sc._scale is None:
            sc._lazy_init_scale_growth_tracker(self.device)
        upd = self._updates.get(key)
        if upd is not None and not upd.uses(sc):
            upd = None                        # net_scaler replaced or reconfigured: re-capture
        if upd is None:
            upd = self._updates[key] = _DeviceUpdate(self, observation, vector, returns, old_ps, train_valid, action)
        return upd

    def _run_device_update(self, upd, episode_cost, distributed):
        """One update from upd's loaded static inputs, the Lagrangian step, and the 12 stats."""
        upd.run(graph=self.graph_update, allreduce=distributed)
        # the Lagrangian step (host, model.py:180) depends only on the episode cost
        if distributed:   # every rank must update the multiplier with the same episode cost
            c = torch.tensor([float(episode_cost)], dtype=torch.float64, device=self.device)
            dist.all_reduce(c)
            episode_cost = c.item() / dist.get_world_size()
        self.lagrange.update_lagrangian_multiplier(episode_cost / EnvParameters.N_AGENTS)
        self.network.weights_updated()        # replays bump no tensor version: drop the fp16 acting copies
        stats = upd.stats.cpu().numpy()       # one device -> host copy
        return [np.asarray(v) for v in stats] + [self.lagrange.get_lagrangian_param()]

    def train_rows(self, runner, rows, episode_cost, checked=False, sym=None):
        """One update on the env-major rows `rows` of runner's last rollout (a DeviceRunner; row r =
        env r // T, step r % T, runner.EnvMajorRows' order), read straight from its device buffers:
        _train_device with _DeviceUpdate.load_rows in place of load -- one HIP launch gathers the nine
        training arrays into the captured update's static inputs (no host indices, no per-array
        indexing or copy launches).  Keyed and captured exactly as Model.train's device update, whose
        _DeviceUpdate of the same minibatch shape it shares.  rows: int64 device tensor (e.g.
        env.minibatch_rows) or any driver-style host index; range-checked as runner._row_index does
        unless checked=True says the caller has (device rows then cost no read-back).  Returns the
        same 12 stats as train().  A model that is not on the GPU, or has fused_loss off, trains
        through train() on torch-indexed rows.
        sym: one grid symmetry per row, as in imitate_rows: the actions are remapped and old_ps and
        train_valid have their columns permuted with the observation and vec, so the ratio is taken
        against the permuted old_ps (opt-in: INTEGRATION.md)."""
        from .runner import _row_index
        T, B = runner.T, runner.env.B
        dev = self.device
        if getattr(runner, "returns", True) is None:
            raise RuntimeError("train_rows: the runner holds no rollout yet (call runner.run() first)")
        if not (checked and isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.dim() == 1):
            rows, _ = _row_index(rows, T * B, dev)
        if dev.type != "cuda" or not self.fused_loss:
            mb = runner.batch()
            o, v, a, p, tv = (mb.observations[rows], mb.vectors[rows], mb.actions[rows], mb.ps[rows],
                              mb.trainValid[rows])
            if sym is not None:
                from .env import sym_apply
                g = self._sym_rows(sym, len(rows), "cpu")
                o, v, a, p = sym_apply(o, v, a, p, g)
                tv = sym_apply(None, None, None, tv, g)[3]
            return self.train(o, v, mb.returns[rows], mb.costReturns[rows], mb.values[rows], mb.costValues[rows],
                              a, p, mb.hiddenState[rows], tv, episode_cost)
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(rows)
        rows = rows.to(dev, non_blocking=True).contiguous()
        packed = getattr(runner, "packed", False)      # DeviceRunner(obs_bits=True): packed rows, unpacked below
        buffers = (runner.obs_bits[:T] if packed else runner.obs[:T], runner.vec[:T], runner.returns, runner.cost_returns, runner.values,
                   runner.cost_values, runner.actions, runner.ps, runner.train_valid)
        M = rows.numel()
        meta = lambda x, *tail: torch.empty((M,) + tuple(x.shape[2:]) + tail, device="meta")   # noqa: E731
        obs, vec, ret, _, _, _, act, ps, tv = buffers
        C_, F_ = runner.env.C, runner.env.F
        obs_meta = torch.empty((M, obs.shape[2], C_, F_, F_), device="meta") if packed else meta(obs)
        upd = self._device_update(obs_meta, meta(vec), meta(ret), meta(ps), meta(tv), meta(act, 1))
        lam = self.lagrange.get_lagrangian_param()
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if self.distributed_update is not None:
            distributed = bool(self.distributed_update) and dist.is_available() and dist.is_initialized()
        upd.load_rows(buffers, T, B, rows, coef=self._loss_coef(lam), lam=lam, packed=(C_, F_) if packed else None,
                      sym=self._sym_rows(sym, M, dev))
        return self._run_device_update(upd, episode_cost, distributed)

    # ------------------------------------------------------------ imitation
    @torch.no_grad()
    def generate_state(self, obs, vector, input_state=None):
        """model.py:71-76: the network's fifth output (the per-agent features handed on as the next
        hidden state in imitation learning).  Inputs may be numpy arrays or device tensors."""
        t = lambda x: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(self.device)   # noqa: E731
        _, _, _, _, output_state, _, _ = self.network(t(obs), t(vector), input_state)
        return output_state

    @staticmethod
    def _distributed():
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def imitation_train(self, observation, vector, optimal_action, input_state=None):
        """model.py:205-231: one behaviour-cloning update -- the cross-entropy of the policy logits
        against the expert's optimal_action [rows, agents], under the same AMP, clip and Adam tail as
        train().  Inputs may be numpy arrays (reference contract) or device tensors; the observation may
        be the packed int32 form; the actions int32 or int64.  input_state is ignored, as the network
        ignores it.  Returns [imitation_loss, grad_norm].
        CPU: plain torch.  GPU with fused_loss off: F.cross_entropy under autocast, then net_scaler's
        scale / unscale / clip / step / update.  GPU default: _DeviceImitation (the fused loss
        mapf_imitation_loss; captured and replayed after two eager updates of a minibatch shape).
        World size > 1: the gradients are all-reduced between backward and unscale and the returned
        stats averaged over the ranks; the device update then runs eagerly (segmented captured graphs
        exist for the PPO update only)."""
        dev = self.device
        t = lambda x: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(dev)   # noqa: E731
        observation, vector, optimal_action = t(observation), t(vector).float(), t(optimal_action)
        if observation.dtype == torch.int32:       # packed (one bit per cell): the update reads floats
            from .env import unpack_obs
            observation = unpack_obs(observation.contiguous(), self.network.num_channel, self.network.fov)
        if dev.type == "cuda" and self.fused_loss:
            upd = self._device_imitation(observation.shape, vector.shape, optimal_action.shape)
            upd.load(observation, vector, optimal_action)
            return self._run_device_imitation(upd)[:2]
        optimal_action = optimal_action.long()
        self.net_optimizer.zero_grad()
        with torch.autocast(device_type=dev.type, enabled=dev.type == "cuda"):
            _, _, _, _, _, logits, _ = self.network(observation, vector, input_state)
            imitation_loss = F.cross_entropy(torch.swapaxes(logits, 1, 2), optimal_action)
        self.net_scaler.scale(imitation_loss).backward()
        self._allreduce_grads()
        self.net_scaler.unscale_(self.net_optimizer)
        grad_norm = torch.nn.utils.clip_grad_norm_(self.network.parameters(), TrainingParameters.MAX_GRAD_NORM)
        self.net_scaler.step(self.net_optimizer)
        self.net_scaler.update()
        stats = torch.stack([imitation_loss.detach().float().reshape(()), grad_norm.detach().float().reshape(())])
        if self._distributed():
            dist.all_reduce(stats)
            stats /= dist.get_world_size()
        return [np.asarray(v) for v in stats.cpu().numpy()]

    def _device_imitation(self, obs_shape, vec_shape, action_shape):
        """The _DeviceImitation of this minibatch shape, keyed ("imitation", shapes) beside the PPO
        updates in _updates; it shares their optimizer and their one GradScaler."""
        key = ("imitation", tuple(obs_shape), tuple(vec_shape), tuple(action_shape))
        sc = self.net_scaler
        if sc._scale is None:
            sc._lazy_init_scale_growth_tracker(self.device)
        upd = self._updates.get(key)
        if upd is not None and not upd.uses(sc):
            upd = None                        # net_scaler replaced or reconfigured: re-capture
        if upd is None:
            upd = self._updates[key] = _DeviceImitation(self, obs_shape, vec_shape, action_shape)
        return upd

    def _run_device_imitation(self, upd):
        """One update from upd's loaded static inputs; the 4 stats (loss, grad norm, agreement with the
        expert, the expert action's mean probability)."""
        distributed = self._distributed()
        upd.run(graph=self.graph_update and not distributed, allreduce=distributed)
        self.network.weights_updated()        # replays bump no tensor version: drop the fp16 acting copies
        return [np.asarray(v) for v in upd.stats.cpu().numpy()]       # one device -> host copy

    def _sym_rows(self, sym, M, device):
        """sym= of train_rows / imitate_rows: None, or one grid symmetry per row -> uint8 [M] on `device`"""
        if sym is None:
            return None
        s = torch.as_tensor(sym)
        if s.dim() != 1 or s.numel() != M or s.dtype.is_floating_point:
            raise ValueError(f"sym: expected {M} integers in 0..7, one per row")
        return s.to(device=device, dtype=torch.uint8, non_blocking=True).contiguous()

    def imitate_rows(self, source, rows, checked=False, sym=None):
        """One imitation update on the env-major rows `rows` of source's last rollout, the twin of
        train_rows: one gather launch (env.gather_rows) moves the rows' observations (packed rows are
        unpacked by one more launch, as _DeviceUpdate.load_rows does), vectors and expert actions into
        _DeviceImitation's static inputs.  source: anything with T, env, packed, obs / obs_bits (T + 1
        slots, slot t = the state the expert saw at step t), vec and expert_actions (int32 [T, B, N]) --
        imitation.DemoRunner, or a DeviceRunner built with expert=.  rows as in train_rows.  Returns
        the 4 stats (loss, grad norm, agreement, expert probability).  A model that is not on the GPU,
        or has fused_loss off, trains through imitation_train() on torch-indexed rows (2 stats).
        sym: one grid symmetry g in 0..7 per row (env.sym_draw; a uint8 device tensor costs no copy) --
        observation, vec and expert action are transformed together in the one gather launch
        (env.gather_rows_sym; the fallback applies env.sym_apply).  None: the rows as they are."""
        from .runner import _row_index
        T, B = source.T, source.env.B
        dev = self.device
        if getattr(source, "expert_actions", None) is None:
            raise RuntimeError("imitate_rows: the source holds no expert actions")
        if not (checked and isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.dim() == 1):
            rows, _ = _row_index(rows, T * B, dev)
        if isinstance(rows, np.ndarray):
            rows = torch.from_numpy(rows)
        packed = bool(getattr(source, "packed", False))
        obs = source.obs_bits[:T] if packed else source.obs[:T]
        vec, act = source.vec[:T], source.expert_actions
        if dev.type != "cuda" or not self.fused_loss:
            r = rows.to(obs.device)
            ts, bs = r % T, r // T
            o, v, a = obs[ts, bs], vec[ts, bs], act[ts, bs]
            if sym is not None:
                from .env import sym_apply, unpack_obs
                if packed:
                    o = unpack_obs(o.contiguous(), source.env.C, source.env.F)
                o, v, a, _ = sym_apply(o, v, a, None, self._sym_rows(sym, r.numel(), "cpu"))
            return self.imitation_train(o, v, a, None)
        rows = rows.to(dev, non_blocking=True).contiguous()
        M = rows.numel()
        C_, F_ = source.env.C, source.env.F
        obs_shape = (M, obs.shape[2], C_, F_, F_) if packed else (M,) + tuple(obs.shape[2:])
        upd = self._device_imitation(obs_shape, (M,) + tuple(vec.shape[2:]), (M,) + tuple(act.shape[2:]))
        upd.load_rows((obs, vec, act), T, B, rows, packed=(C_, F_) if packed else None, sym=self._sym_rows(sym, M, dev))
        return self._run_device_imitation(upd)

    def _finish_update(self, all_loss, policy_loss, entropy, critic_loss, valid_loss, cost_critic_loss, cost_loss,
                       clip_frac, advantage, cost_advantage, episode_cost, distributed):
        """model.py:177-199: backward, gradient exchange, Lagrangian step, clip, Adam, stats."""
        dev = self.device
        self.net_scaler.scale(all_loss).backward()
        self._allreduce_grads()
        self.net_scaler.unscale_(self.net_optimizer)
        if distributed:   # every rank must update the multiplier with the same episode cost
            c = torch.tensor([float(episode_cost)], dtype=torch.float64, device=dev)
            dist.all_reduce(c)
            episode_cost = c.item() / dist.get_world_size()
        self.lagrange.update_lagrangian_multiplier(episode_cost / EnvParameters.N_AGENTS)
        grad_norm = torch.nn.utils.clip_grad_norm_(self.network.parameters(), TrainingParameters.MAX_GRAD_NORM)
        self.net_scaler.step(self.net_optimizer)
        self.net_scaler.update()
        stats = torch.stack([t.detach().float().reshape(()) for t in (
            all_loss, policy_loss, entropy, critic_loss, valid_loss, cost_critic_loss, cost_loss, clip_frac, grad_norm,
            torch.mean(advantage), torch.mean(cost_advantage))]).cpu().numpy()       # one device -> host copy
        return [np.asarray(v) for v in stats] + [self.lagrange.get_lagrangian_param()]


_REDUCTIONS_OK = {}


def captured_reductions_ok(device):
    """Whether a captured multi-block torch reduction gives the right sum on every replay in this
    process (mapf_amd/__init__.py: with the HIP runtime's packet capture on, the captured memset that
    zeroes the reduction's semaphores takes effect on the first replay only).  One exact fp32 sum of
    1088 x 1536 ones, captured, its output poisoned with NaN before each of three replays."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _REDUCTIONS_OK:
        x = torch.ones(1088, 1536, device=dev)
        want = float(x.numel())                   # < 2^24: exact in fp32 whatever the order
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                y = x.sum().reshape(1)
        torch.cuda.current_stream(dev).wait_stream(s)
        got = []
        for _ in range(3):
            y.fill_(float("nan"))
            g.replay()
            got.append(y.item())
        del g
        _REDUCTIONS_OK[key] = all(v == want for v in got)
        if not _REDUCTIONS_OK[key]:
            import warnings
            warnings.warn(f"captured torch reductions replay wrong on this HIP runtime ({got}, want {want}; "
                          f"is DEBUG_CLR_GRAPH_PACKET_CAPTURE=1?): the PPO update runs eagerly", RuntimeWarning)
    return _REDUCTIONS_OK[key]


class _DeviceUpdate:
    """The static buffers and the body of one minibatch shape's device update (Model._train_device)."""

    WARMUP = 2          # eager updates before the capture (allocator, MIOpen find, Adam state)

    def __init__(self, model, observation, vector, returns, old_ps, train_valid, action):
        dev = model.device
        self.model = model
        e = lambda x, dt=torch.float32: torch.zeros(tuple(x.shape), dtype=dt, device=dev)   # noqa: E731
        self.obs, self.vec = e(observation), e(vector)
        self.ret, self.cret, self.v, self.cv = e(returns), e(returns), e(returns), e(returns)
        self.action = e(action, torch.int64)
        self.old_ps, self.tv = e(old_ps), e(train_valid)
        self.dyn = torch.zeros(8, dtype=torch.float32, device=dev)     # coef[6], lam, f32(lam + 1)
        self.nstats = torch.zeros(4, dtype=torch.float64, device=dev)    # global advantage statistics (distributed)
        self._init_tail(11)

    def _init_tail(self, n_stats):
        """the state of the shared tail (_tail) and of run(): the AMP tensors, found-inf, the stats, the
        gradient bucket and the captured graph"""
        model = self.model
        dev = model.device
        sc = model.net_scaler                  # its live state and settings (GradScaler: 2^16, x2 / 2000, x0.5)
        self.scaler = sc
        self.scale, self.growth = sc._scale, sc._growth_tracker        # 0-dim device tensors, updated in place
        self.amp = self._amp_settings(sc)
        self.found_inf = torch.zeros((), dtype=torch.float32, device=dev)
        self.stats = torch.zeros(n_stats, dtype=torch.float32, device=dev)
        self.grad_params, self.flat = None, None                          # the gradient bucket (distributed)
        self.live = None
        self.graph = None                    # one CUDAGraph, or (segment A, segment B) when distributed
        self.graph_allreduce = False
        self.eager_runs = 0

    @staticmethod
    def _amp_settings(sc):
        return float(sc._growth_factor), float(sc._backoff_factor), int(sc._growth_interval)

    def uses(self, sc):
        """True while this update's captured AMP state is `sc`'s (same tensors, same settings)."""
        return (self.scaler is sc and self.scale is sc._scale and self.growth is sc._growth_tracker
                and self.amp == self._amp_settings(sc))

    def load(self, observation, vector, returns, cost_returns, old_v, old_cv, action, old_ps, train_valid, coef, lam):
        for dst, src in ((self.obs, observation), (self.vec, vector), (self.ret, returns), (self.cret, cost_returns),
                         (self.v, old_v), (self.cv, old_cv), (self.old_ps, old_ps), (self.tv, train_valid)):
            dst.copy_(src.reshape(dst.shape), non_blocking=True)
        self.action.copy_(action.reshape(self.action.shape), non_blocking=True)
        self._load_dyn(coef, lam)

    def _load_dyn(self, coef, lam):
        # host double -> f32 exactly as the host-argument kernels round them
        h = torch.tensor(list(coef) + [lam, lam + 1.0], dtype=torch.float64).float()
        self.dyn.copy_(h.pin_memory() if torch.cuda.is_available() else h, non_blocking=True)

    def load_rows(self, buffers, T, B, rows, coef, lam, packed=None, sym=None):
        """load() straight from a rollout's t-major [T, B, ...] device buffers: buffers = (obs, vec,
        returns, cost returns, values, cost values, actions int64, ps, train_valid), rows = int64
        device tensor of env-major row ids in [0, B * T), one per minibatch row.  One gather launch
        (env.gather_rows) fills the nine static inputs; with the coefficients' copy that is two
        launches per minibatch.  packed = (C, F): buffers[0] is the packed observation buffer (int32
        [T, B, N, WPA]); its rows (N * WPA * 4 bytes each) are gathered into a staging tensor by the same
        launch and unpacked into the static float input (env.unpack_obs: one more launch).
        sym: uint8 device tensor, one grid symmetry per row (env.sym_draw) -- ONE env.gather_rows_sym
        launch then fills the inputs transformed (packed rows too: no staging, no unpack launch): the
        actions remapped, old_ps and train_valid with their columns permuted."""
        from .env import gather_rows, unpack_obs
        if sym is not None:
            from .env import gather_rows_sym
            N, F = self.obs.shape[1], self.obs.shape[-1]
            gather_rows_sym(buffers, T, B, rows, (self.obs, self.vec, self.ret, self.cret, self.v, self.cv, self.action,
                                                  self.old_ps, self.tv),
                            ("obs_bits" if packed is not None else "obs", "vec", "plain", "plain", "plain", "plain",
                             "action64", "cols", "cols"), sym=sym, geometry=(N, self.obs.shape[2], F))
            self._load_dyn(coef, lam)
            return
        obs_dst = self.obs
        if packed is not None:
            shape = (rows.numel(),) + tuple(buffers[0].shape[2:])
            if getattr(self, "obs_stage", None) is None or tuple(self.obs_stage.shape) != shape:
                self.obs_stage = torch.zeros(shape, dtype=torch.int32, device=self.obs.device)
            obs_dst = self.obs_stage
        gather_rows(buffers, T, B, rows, (obs_dst, self.vec, self.ret, self.cret, self.v, self.cv, self.action,
                                          self.old_ps, self.tv))
        if packed is not None:
            unpack_obs(self.obs_stage, packed[0], packed[1], out=self.obs)
        self._load_dyn(coef, lam)

    def _front(self, allreduce):
        """normalise -> forward -> fused loss -> backward (graph segment A when distributed); with
        allreduce, the normalisation reads the global statistics in self.nstats (computed and
        all-reduced by _moments before the segment) and the gradients end in the static bucket"""
        net, opt = self.model.network, self.model.net_optimizer
        T = TrainingParameters
        opt.zero_grad(set_to_none=True)
        from .env import normalize_advantages_dlam, normalize_advantages_with_stats
        ins = (self.ret.reshape(-1), self.v.reshape(-1), self.cret.reshape(-1), self.cv.reshape(-1))
        if allreduce:    # model.py:106-113 over the GLOBAL minibatch: moments all-reduced
            adv, cadv = normalize_advantages_with_stats(*ins, self.nstats, mix=T.MINUS_ADV_WITH_CADV,
                                                        lam2=self.dyn[6:8])
        else:
            adv, cadv = normalize_advantages_dlam(*ins, self.dyn[6:8], T.MINUS_ADV_WITH_CADV)
        adv, cadv = adv.view(self.ret.shape), cadv.view(self.ret.shape)
        with torch.autocast(device_type="cuda", cache_enabled=False):
            new_ps, new_v, block, policy_sig, _, _, new_cv = net(self.obs, self.vec, None)
        all_loss, terms = _FusedPPOLoss.apply(new_ps, new_v, new_cv, policy_sig, self.old_ps, self.action.unsqueeze(-1),
                                              self.v, self.ret, self.cv, self.cret, adv, cadv, self.tv, self.dyn[:6])
        (all_loss * self.scale).backward()
        self.live = (all_loss, terms, adv, cadv)       # read by _back (kept alive: graph A writes them)
        if allreduce:    # the flattened gradient bucket (model.py:177-185: all-reduced between backward and unscale)
            self._fill_bucket()

    def _fill_bucket(self):
        """the gradients of the backward just run, flattened into the static bucket the ranks all-reduce"""
        gp = [p for p in self.model.network.parameters() if p.grad is not None]
        if self.grad_params is None:
            self.grad_params = gp
            self.flat = torch.empty(sum(p.numel() for p in gp), dtype=torch.float32, device=self.model.device)
        assert len(gp) == len(self.grad_params) and all(a is b for a, b in zip(gp, self.grad_params))
        # each gradient's elements in memory order (AccumulateGrad lays a dense parameter's gradient out
        # like the parameter: contiguous or channels_last), so _tail's views of the bucket take the
        # parameter's own strides -- fused Adam wants parameter and gradient alike
        assert all(p.grad.stride() == p.stride() for p in gp)
        torch.cat([p.grad.as_strided((p.numel(),), (1,)) for p in gp], out=self.flat)

    def _tail(self, allreduce):
        """[bucket averaged over the ranks] -> unscale + found-inf -> clip -> fused Adam -> loss-scale
        update: the tail the PPO update and the imitation update (_DeviceImitation) share.  Returns the
        gradient norm before clipping."""
        net, opt = self.model.network, self.model.net_optimizer
        T = TrainingParameters
        if allreduce:    # the parameters' gradients become views of the all-reduced bucket (no copy back)
            self.flat.div_(dist.get_world_size())
            off = 0
            for p in self.grad_params:
                p.grad = self.flat.as_strided(p.shape, p.stride(), off)
                off += p.numel()
        params = [p for p in net.parameters() if p.grad is not None]
        self.found_inf.zero_()
        torch._amp_foreach_non_finite_check_and_unscale_([p.grad for p in params], self.found_inf,
                                                         self.scale.double().reciprocal().float())
        grad_norm = torch.nn.utils.clip_grad_norm_(params, T.MAX_GRAD_NORM)
        opt.grad_scale, opt.found_inf = None, self.found_inf     # fused Adam: skipped on the device when inf
        opt.step()
        opt.grad_scale = opt.found_inf = None
        torch._amp_update_scale_(self.scale, self.growth, self.found_inf, *self.amp)
        return grad_norm

    def _back(self, allreduce):
        """_tail -> stats (graph segment B when distributed)"""
        grad_norm = self._tail(allreduce)
        all_loss, terms, adv, cadv = self.live
        self.stats.copy_(torch.stack([t.detach().float().reshape(()) for t in (
            all_loss, terms[0], terms[1], terms[2], terms[3], terms[4], terms[5], terms[6], grad_norm,
            torch.mean(adv), torch.mean(cadv))]))

    def _moments(self):
        """eager, before segment A: the global advantage statistics (two all-reduced moment passes)"""
        from .env import advantage_stats_distributed
        advantage_stats_distributed(self.ret.reshape(-1), self.v.reshape(-1), self.cret.reshape(-1),
                                    self.cv.reshape(-1), out=self.nstats)

    def _exchange(self):
        """eager, between the segments: the gradient bucket's all-reduce (RCCL over xGMI)"""
        dist.all_reduce(self.flat)

    def _exchange_stats(self):
        """eager, after segment B: the loss terms' and advantages' means over the global minibatch"""
        dist.all_reduce(self.stats)
        self.stats.div_(dist.get_world_size())

    def body(self, allreduce=False):
        """one whole update, eagerly (or captured whole when not distributed)"""
        if allreduce:
            self._moments()
        self._front(allreduce)
        if allreduce:
            self._exchange()
        self._back(allreduce)
        if allreduce:
            self._exchange_stats()

    @staticmethod
    def _capture(fn):
        """fn captured into a hipGraph on a side stream.  thread_local capture mode: the process group's
        watchdog thread keeps querying the events of earlier RCCL work while the capture runs, which the
        default (global) mode forbids -- it killed the process (hipErrorStreamCaptureUnsupported) in the
        c4-shaped distributed update on a 1-rank RCCL group.  The eager collectives are also drained
        (synchronize) before the capture begins."""
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
                fn()
        torch.cuda.current_stream().wait_stream(s)
        return g

    def run(self, graph=True, allreduce=False):
        """graph: after WARMUP eager updates of this shape, replay captured graphs -- one graph for the
        whole update on one rank; distributed, two segments (A: normalise -> backward into the static
        gradient bucket; B: unscale -> clip -> Adam -> scale update -> stats) with the collectives run
        eagerly around and between them (moments before A, the bucket all-reduce between, the stats
        after B), so the c4 update replays its ~1,500 small ops too."""
        if graph and self.graph is None and not captured_reductions_ok(self.model.device):
            graph = False                   # the runtime would replay the update wrong: eager
        if not graph or self.eager_runs < self.WARMUP:
            if graph:                       # warm-up on a side stream, as capture wants
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self.body(allreduce=allreduce)
                torch.cuda.current_stream().wait_stream(s)
            else:
                self.body(allreduce=allreduce)
            self.eager_runs += 1
            return
        if self.graph is None:
            self.graph = (self._capture(lambda: self._front(True)), self._capture(lambda: self._back(True))) \
                if allreduce else self._capture(self.body)
            self.graph_allreduce = allreduce
        if self.graph_allreduce != allreduce:
            raise RuntimeError("a minibatch shape's captured update switched between one rank and distributed")
        if allreduce:
            self._moments()
            self.graph[0].replay()
            self._exchange()
            self.graph[1].replay()
            self._exchange_stats()
        else:
            self.graph.replay()


class _DeviceImitation(_DeviceUpdate):
    """The static buffers and the body of one minibatch shape's device imitation update
    (Model.imitation_train / imitate_rows): zero-grad -> autocast forward -> fused cross-entropy
    (mapf_imitation_loss) -> (loss * scale).backward(), then _DeviceUpdate's own tail (unscale with
    found-inf, clip, fused Adam, loss-scale update) on the model's one optimizer and one GradScaler.
    Warm-ups, capture and replay are _DeviceUpdate.run's.  stats[4] = loss, grad norm, agreement with
    the expert, the expert action's mean probability."""

    def __init__(self, model, obs_shape, vec_shape, action_shape):
        dev = model.device
        self.model = model
        self.obs = torch.zeros(tuple(obs_shape), dtype=torch.float32, device=dev)
        self.vec = torch.zeros(tuple(vec_shape), dtype=torch.float32, device=dev)
        self.action = torch.zeros(tuple(action_shape), dtype=torch.int32, device=dev)    # the rollouts' format
        self._init_tail(4)

    def load(self, observation, vector, action):
        self.obs.copy_(observation.reshape(self.obs.shape), non_blocking=True)
        self.vec.copy_(vector.reshape(self.vec.shape), non_blocking=True)
        self.action.copy_(action.reshape(self.action.shape), non_blocking=True)      # int64 -> int32 in the copy

    def load_rows(self, buffers, T, B, rows, packed=None, sym=None):
        """load() straight from t-major [T, B, ...] device buffers (observations or packed observations,
        vec, expert actions int32) in one gather launch; packed = (C, F) and sym: as
        _DeviceUpdate.load_rows (with sym, one env.gather_rows_sym launch and nothing else)."""
        from .env import gather_rows, unpack_obs
        if sym is not None:
            from .env import gather_rows_sym
            gather_rows_sym(buffers, T, B, rows, (self.obs, self.vec, self.action),
                            ("obs_bits" if packed is not None else "obs", "vec", "action32"), sym=sym,
                            geometry=(self.obs.shape[1], self.obs.shape[2], self.obs.shape[-1]))
            return
        obs_dst = self.obs
        if packed is not None:
            shape = (rows.numel(),) + tuple(buffers[0].shape[2:])
            if getattr(self, "obs_stage", None) is None or tuple(self.obs_stage.shape) != shape:
                self.obs_stage = torch.zeros(shape, dtype=torch.int32, device=self.obs.device)
            obs_dst = self.obs_stage
        gather_rows(buffers, T, B, rows, (obs_dst, self.vec, self.action))
        if packed is not None:
            unpack_obs(self.obs_stage, packed[0], packed[1], out=self.obs)

    def _front(self, allreduce):
        net, opt = self.model.network, self.model.net_optimizer
        opt.zero_grad(set_to_none=True)
        with torch.autocast(device_type="cuda", cache_enabled=False):
            _, _, _, _, _, logits, _ = net(self.obs, self.vec, None)
        loss, terms = _FusedImitationLoss.apply(logits, self.action)
        (loss * self.scale).backward()
        self.live = (loss, terms)          # read by _back (kept alive: the graph writes them)
        if allreduce:
            self._fill_bucket()

    def _back(self, allreduce):
        grad_norm = self._tail(allreduce)
        loss, terms = self.live
        self.stats.copy_(torch.stack([t.detach().float().reshape(()) for t in (loss, grad_norm, terms[0], terms[1])]))

    def _moments(self):
        """nothing to normalise: the imitation loss has no advantage statistics"""
