"""us per step of three routes to the eight OneEpPerformance numbers of every env (mapf_perf, mapf.h), for
the BASELINE presets c2, c4, c5 and the four rollout policies:

  perf        env.rollout_perf(T, policy): one launch, no observation (0 B per agent-step; 32 B per env once)
  slots+acc   env.rollout(T, policy, slots=True) + perf_accumulate(out): float observations into [T] slots
  bits+torch  env.rollout(T, policy, slots=True, obs_bits=True) + the torch reductions of
              replay_fixed_episodes: the cheapest route before mapf_rollout_perf existed

`--warmup` untimed rounds, then `--repeats` timed rounds; a round runs every route once, in turn, so that
drift of the clocks or of the box falls on all routes alike.  A timed window is one call of T = `--steps`
steps (256: several milliseconds) between two device events, the reductions included; the line reports the
median and the min..max spread per route, all on the same handle in the same process.  One JSON line per
(config, policy).  Where the float slots of T steps do not fit the device (c5) the slots+acc route is left out.

    python tools/bench_perf.py [--configs c2,c4,c5] [--steps 256] [--repeats 9] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "primal-ppo_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

KEYS = ("status", "reward_total", "cost", "goals_reached", "shadow_goals", "constraints")


def torch_reduce(out):
    """replay_fixed_episodes' reductions over [T]-slot outputs."""
    st = out["status"]
    return torch.stack([out["reward_total"].double().sum((0, 2)), out["cost"].double().sum((0, 2)),
                        (st == -2).sum((0, 2)).double(), (st == -1).sum((0, 2)).double(),
                        (st == -3).sum((0, 2)).double(), out["goals_reached"].double().sum((0, 2)),
                        out["shadow_goals"].double().sum(0), out["constraints"].double().sum((0, 2))], dim=1)


def timed(routes, warmup, repeats):
    """{name: [ms per call]}: rounds over all routes in turn, the first `warmup` rounds untimed."""
    ms = {name: [] for name in routes}
    for r in range(warmup + repeats):
        for name, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


def main():
    from mapf_amd.env import perf_accumulate
    from rollout_harness import preset_envs
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4,c5")
    ap.add_argument("--policies", default="random,tape,descent,pibt")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    T = args.steps
    for cfg in args.configs.split(","):
        env = preset_envs(cfg, 1)[0]
        dev = env.device
        out = {k: torch.empty((T,) + tuple(env.out[k].shape), dtype=env.out[k].dtype, device=dev) for k in KEYS}
        vec = torch.empty((T,) + tuple(env.vec.shape), device=dev)
        bits = torch.empty((T,) + tuple(env._bits_buffer(None, 1).shape), dtype=torch.int32, device=dev)
        acts = torch.zeros(T, env.B, env.N, dtype=torch.int32, device=dev)
        perf = torch.zeros(env.B, 8, dtype=torch.int32, device=dev)
        env.rollout(T, "random", slots=True, actions=acts, obs=bits, vec=vec, out=out, obs_bits=True)
        tape = acts.clone()
        obs = None
        try:
            obs = torch.empty((T,) + tuple(env.obs.shape), device=dev)
        except RuntimeError:          # c5's float slots may not fit beside the rest
            pass
        agent_steps = env.B * env.N
        for policy in args.policies.split(","):
            kw = dict(tape=tape) if policy == "tape" else dict(actions=acts)
            routes = {"perf": lambda: env.rollout_perf(T, policy, perf=perf, **({"tape": tape} if policy == "tape" else {})),
                      "bits+torch": lambda: torch_reduce(env.rollout(T, policy, slots=True, obs=bits, vec=vec, out=out,
                                                                      obs_bits=True, **kw)[0])}
            if obs is not None:
                routes["slots+acc"] = lambda: perf_accumulate(env.rollout(T, policy, slots=True, obs=obs, vec=vec, out=out,
                                                                            **kw)[0], perf=perf)
            # bytes written per agent-step.  The slot routes: the observation (floats, or WPA packed words), vec
            # (16), the action (4; none under the tape), and the six outputs the reduction reads: status (1),
            # reward_total, cost, goals_reached, constraints (16), shadow_goals (4 per env).  perf: nothing per
            # step (no actions asked for); the 32-byte record per env once per launch.
            rest = 16 + (0 if policy == "tape" else 4) + 1 + 16 + 4.0 / env.N
            line = dict(config=cfg, policy=policy, steps=T, envs=env.B, agents=env.N, plan=env.rollout_perf_plan(policy),
                        bytes_per_agent_step={"perf": round(32.0 / (env.N * T), 4),
                                              "bits+torch": round(4.0 * env.obs_words + rest, 2),
                                              "slots+acc": round(4.0 * env.C * env.F * env.F + rest, 2)})
            ms = timed(routes, args.warmup, args.repeats)
            for name in routes:
                us = [1000.0 * m / T for m in ms[name]]
                line[name] = dict(us_per_step_median=round(statistics.median(us), 3), min=round(min(us), 3),
                                  max=round(max(us), 3), agent_steps_per_s=round(agent_steps / statistics.median(us) * 1e6))
            print(json.dumps(line), flush=True)
        env.close()
        del out, vec, bits, acts, obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
