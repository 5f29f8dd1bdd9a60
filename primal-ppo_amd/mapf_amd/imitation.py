"""DemoRunner: expert demonstrations for behaviour cloning, one launch per rollout.

The reference trains its policy on an expert's actions too (Model.imitation_train, model.py:205-231;
its expert, od_mstar3, plans on the host).  Here the expert is a rollout policy of the persistent
kernels (env.rollout: "pibt" the collision-free planner, "descent" the goal-seeking baseline, or
"tape" for an outside planner's actions), so one launch yields T steps of expert actions and the
observations the expert saw, in the layout Model.imitate_rows gathers from.

ALIGNMENT.  The persistent kernels write the observation AFTER step t.  The buffers therefore hold
T + 1 slots: slot 0 is observed before the launch, and the launch writes its step t's observation
into slot t + 1 (it is handed ob[1:], vec[1:]).  The state the expert saw when it chose
expert_actions[t] is slot t, so (ob[:T], vec[:T], expert_actions) are aligned [T, B, ...] buffers --
ob[:T] is a contiguous view, gathered without a copy -- and slot T is the state after the last step.
"""
import torch

from .config import NetParameters, TrainingParameters
from .env import BatchedMapfGym, noise_q16
from .runner import DeviceMaps


class DemoRunner:
    """env: a BatchedMapfGym ("pibt" and "descent" need keep_bfs).  policy: "pibt", "descent" or "tape"
    (run(tape=...) then takes the int32 [T, B, N] actions to play); "random" is no expert and raises.
    human_weight (policy="pibt" only, ValueError otherwise): the planner's human weight, set on the env once
    here (env.set_pibt_human_weight); None leaves the env's setting alone.  human_horizon: likewise the
    planner's human horizon (env.set_pibt_human_horizon).
    noise (policy "pibt" / "descent" only, ValueError for "tape"): action noise eps in [0, 1] on the
    demonstrations, set on the env once here (env.set_action_noise); None leaves the env's setting alone.
    With probability eps an agent plays a uniform random action, so the rollouts visit states the expert
    alone never reaches; expert_actions stay the expert's picks for the states observed (the labels).
    new_maps, seed: as DeviceRunner.  obs_bits: keep the observations packed (`obs_bits` int32
    [T + 1, B, N, WPA]; the default) or as floats (`obs` [T + 1, B, N, C, F, F]).
    Exposes T, env, packed, obs / obs_bits, vec and expert_actions (int32 [T, B, N]): a source of
    Model.imitate_rows and DeviceTrainer.imitate."""

    def __init__(self, env: BatchedMapfGym, n_steps=None, policy="pibt", new_maps=None, obs_bits=True, seed=0,
                 human_weight=None, human_horizon=None, noise=None):
        if policy not in ("pibt", "descent", "tape"):
            raise ValueError(f"DemoRunner: policy must be 'pibt', 'descent' or 'tape' (an expert), got {policy!r}")
        if human_weight is not None and policy != "pibt":
            raise ValueError(f"human_weight belongs to policy='pibt', not {policy!r}")
        if human_horizon is not None and policy != "pibt":
            raise ValueError(f"human_horizon belongs to policy='pibt', not {policy!r}")
        if noise is not None:
            if policy == "tape":
                raise ValueError("noise= belongs to policy 'pibt' or 'descent', not 'tape'")
            noise = noise_q16(noise)
        if human_weight is not None:
            env.set_pibt_human_weight(human_weight)
        if human_horizon is not None:
            env.set_pibt_human_horizon(human_horizon)
        if noise is not None:
            env.set_action_noise(q16=noise)
        self.env, self.policy = env, policy
        self.T = TrainingParameters.N_STEPS if n_steps is None else int(n_steps)
        if self.T < 1:
            raise ValueError("DemoRunner: n_steps must be >= 1")
        self.seed, self.new_maps, self.rollouts = seed, new_maps, 0
        B, N, C, F, T = env.B, env.N, env.C, env.F, self.T
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=env.device)   # noqa: E731
        self.packed = bool(obs_bits)
        if self.packed:
            self.obs, self.obs_bits = None, z(T + 1, B, N, env.obs_words, dt=torch.int32)
        else:
            self.obs, self.obs_bits = z(T + 1, B, N, C, F, F), None
        self.vec = z(T + 1, B, N, NetParameters.VECTOR_LEN)
        self.expert_actions = z(T, B, N, dt=torch.int32)
        self.status = z(T, B, N, dt=torch.int8)
        self.goals = z(T, B, N)
        self.constraints = z(T, B, N)

    @torch.no_grad()
    def run(self, tape=None):
        """One rollout of T expert steps in one launch.  tape (policy="tape"): int32 [T, B, N] on the
        device, the outside planner's actions to play; expert_actions receives a copy of them.
        Returns performance_per_env()."""
        env, T = self.env, self.T
        if isinstance(self.new_maps, DeviceMaps):
            self.new_maps.reset(env, self.rollouts, (self.seed << 20) + self.rollouts + 1)
        elif self.new_maps is not None:
            env.reset_seeded(self.new_maps(self.rollouts), seed=(self.seed << 20) + self.rollouts + 1)
        ob = self.obs_bits if self.packed else self.obs
        (env.observe_bits if self.packed else env.observe)(ob[0], self.vec[0])
        out = {"status": self.status, "goals_reached": self.goals, "constraints": self.constraints}
        if self.policy == "tape":
            if tape is None:
                raise ValueError("DemoRunner(policy='tape').run needs the actions to play: tape=...")
            env.rollout(T, "tape", slots=True, tape=tape, obs=ob[1:], vec=self.vec[1:], out=out, obs_bits=self.packed)
            self.expert_actions.copy_(tape)           # the labels are the planner's choices
        else:
            if tape is not None:
                raise ValueError(f"tape= goes with policy='tape', not {self.policy!r}")
            env.rollout(T, self.policy, slots=True, actions=self.expert_actions, obs=ob[1:], vec=self.vec[1:], out=out,
                        obs_bits=self.packed)
        self.rollouts += 1
        return self.performance_per_env()

    def performance_per_env(self):
        """The counters DeviceRunner.performance_per_env derives from the same outputs, float64 numpy [B]
        each: totalGoals, staticCollide, humanCollide, agentCollide, constraintViolations."""
        st = self.status
        per = {"totalGoals": self.goals.sum(dim=(0, 2)), "staticCollide": (st == -1).sum(dim=(0, 2)),
               "humanCollide": (st == -2).sum(dim=(0, 2)), "agentCollide": (st == -3).sum(dim=(0, 2)),
               "constraintViolations": self.constraints.sum(dim=(0, 2))}
        return {k: v.double().cpu().numpy() for k, v in per.items()}
