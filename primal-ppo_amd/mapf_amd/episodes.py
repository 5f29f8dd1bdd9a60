"""Fixed evaluation episodes: the reference's on-disk format and a batched
evaluation loop on the device env.

On-disk format (evaluate.py:32-135): a folder holding
  infos.json          {"obstacleMap": ["obstacleMap0.npy", ...],
                       "agentsSequence": [[[[r, c], ...] per agent] per episode],
                       "humanSequence": [[[r, c], ...] per episode],
                       "humanStart": [[r, c], ...], "humanGoal": [[r, c], ...],
                       "numEpisodes": E}        (json.dump indent=4, sort_keys)
  obstacleMap{i}.npy  int64 [H, W], 0 free / -1 obstacle (np.save)
Files are read with json and np.load(allow_pickle=False) only.

generate_fixed_episode_infos restates generateFixedEpisodeInfos
(evaluate.py:50-103) with a numpy Generator in place of the global
np.random stream (the reference's MT19937 draws are not reproducible on the
device; the episodes themselves are the parity anchor once written).

evaluate_fixed_episodes runs evaluate() (evaluate.py:169-269) for every
episode at once: one BatchedMapfGym per map shape (FixedMapfGym semantics:
agentsSequence goals, LoopingHuman or FixedPathHuman, useDA / useHP), the
policy forward batched over episodes, and the OneEpPerformance sums
(evaluate.py:226-256) accumulated on the device.
"""
import json
import os

import numpy as np
import torch

from .config import make_config
from .maps import generate_warehouse


def create_fixed_episode_info():
    return {"obstacleMap": [], "agentsSequence": [], "humanSequence": [], "humanStart": [], "humanGoal": [],
            "numEpisodes": 0}


def _manhattan(a, b):
    return abs(a[0] - b[0]) + abs(a[1] - b[1])


def _free_cell(rng, world):
    """util.getFreeCell (util.py:67-76): rejection-sample a cell whose value is 0."""
    H, W = world.shape
    while True:
        i, j = int(rng.integers(0, H)), int(rng.integers(0, W))
        if world[i, j] == 0:
            return (i, j)


def _entrance(rng, world):
    """Human.getEntrance (mapf_gym.py:17-22): a free cell on row 0 or column 0."""
    while True:
        e = _free_cell(rng, world)
        if e[0] == 0 or e[1] == 0:
            return e


def generate_fixed_episode_infos(episodes, n_agents, max_steps, world_size=(10, 40), rng=None):
    """evaluate.py:50-103 (generateFixedEpisodeInfos), same marking protocol on tempMap."""
    rng = np.random.default_rng(0) if rng is None else rng
    infos = create_fixed_episode_info()
    for _ in range(episodes):
        length = int(rng.integers(world_size[0], world_size[1] + 1))
        obstacle_map = generate_warehouse(length).astype(np.int64)
        temp = obstacle_map.copy()
        human_start = _entrance(rng, temp)
        human_seq = [human_start]
        temp[human_start] = 1
        path_len = 0
        human_goal = human_start
        while path_len <= max_steps:
            prev = human_seq[-1]
            human_goal = _free_cell(rng, temp)
            path_len += _manhattan(prev, human_goal)
            temp[human_goal] = 1
            temp[human_start] = 0
            human_seq.append(human_goal)
        temp[human_seq[-1]] = 0
        temp[human_start] = 1
        seqs = [[] for _ in range(n_agents)]
        for a in range(n_agents):
            s = _free_cell(rng, temp)
            temp[s] = 2
            seqs[a].append(s)
        lens = [0] * n_agents
        done = [False] * n_agents
        while not all(done):
            for a in range(n_agents):
                if done[a]:
                    continue
                start = seqs[a][-1]
                goal = _free_cell(rng, temp)
                temp[goal] = 3
                seqs[a].append(goal)
                lens[a] += _manhattan(start, goal)
                if lens[a] > max_steps:
                    done[a] = True
            for s in seqs:       # free the cell before the last one
                temp[s[-2]] = 0
        infos["obstacleMap"].append(obstacle_map)
        infos["agentsSequence"].append(seqs)
        infos["humanSequence"].append(human_seq)
        infos["humanStart"].append(human_start)
        infos["humanGoal"].append(human_goal)
        infos["numEpisodes"] += 1
    return infos


def save_fixed_episode_infos(infos, folder):
    """saveFixedEpisodeInfos (evaluate.py:105-123)."""
    os.makedirs(folder, exist_ok=True)
    out = dict(infos)
    names = []
    for i in range(infos["numEpisodes"]):
        name = f"obstacleMap{i}.npy"
        np.save(os.path.join(folder, name), np.asarray(infos["obstacleMap"][i], dtype=np.int64))
        names.append(name)
    out["obstacleMap"] = names
    out["agentsSequence"] = [[[list(map(int, c)) for c in seq] for seq in ep] for ep in infos["agentsSequence"]]
    out["humanSequence"] = [[list(map(int, c)) for c in ep] for ep in infos["humanSequence"]]
    out["humanStart"] = [list(map(int, c)) for c in infos["humanStart"]]
    out["humanGoal"] = [list(map(int, c)) for c in infos["humanGoal"]]
    with open(os.path.join(folder, "infos.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, indent=4, sort_keys=True)


def load_fixed_episode_infos(folder):
    """loadFixedEpisodeInfos (evaluate.py:125-137): cells as tuples, maps via np.load (no pickle)."""
    with open(os.path.join(folder, "infos.json")) as f:
        js = json.load(f)
    infos = create_fixed_episode_info()
    for i in range(js["numEpisodes"]):
        infos["obstacleMap"].append(np.load(os.path.join(folder, js["obstacleMap"][i]), allow_pickle=False))
        infos["agentsSequence"].append([[tuple(c) for c in seq] for seq in js["agentsSequence"][i]])
        infos["humanSequence"].append([tuple(c) for c in js["humanSequence"][i]])
    infos["humanStart"] = [tuple(c) for c in js["humanStart"]]
    infos["humanGoal"] = [tuple(c) for c in js["humanGoal"]]
    infos["numEpisodes"] = js["numEpisodes"]
    return infos


def _groups_by_shape(infos):
    groups = {}
    for i in range(infos["numEpisodes"]):
        groups.setdefault(tuple(np.shape(infos["obstacleMap"][i])), []).append(i)
    return groups


METRIC_KEYS = ("episodeReward", "episodeCostReward", "humanCollide", "staticCollide", "agentCollide", "totalGoals",
               "shadowGoals", "constraintViolations")


def _group_env(infos, idx, H, W, device, num_channel, fov, use_da, use_hp, human_movement_type, k_predict, fix_choice,
               keep_bfs=False):
    """The BatchedMapfGym of one map-shape group of episodes, reset to their starts (FixedMapfGym)."""
    from .env import BatchedMapfGym
    n = len(infos["agentsSequence"][idx[0]])
    S = max(len(s) for i in idx for s in infos["agentsSequence"][i])
    HS = max(len(infos["humanSequence"][i]) for i in idx) if human_movement_type == 1 else 2
    cfg = make_config(len(idx), H, W, num_agents=n, fov=fov, num_channel=num_channel, use_da=int(use_da),
                      use_hp=int(use_hp), human_mode="fixed_path" if human_movement_type == 1 else "looping",
                      goal_mode="sequence", fix_choice=fix_choice, shared_map=False, keep_bfs=bool(keep_bfs), max_seq=S,
                      max_human_seq=HS)
    cfg.k_predict = k_predict
    env = BatchedMapfGym(cfg, device=device)
    env.episodes = idx
    maps = np.stack([np.asarray(infos["obstacleMap"][i]) for i in idx]).astype(np.int8)
    seqs = [infos["agentsSequence"][i] for i in idx]
    if human_movement_type == 1:
        env.reset_fixed(maps, seqs, human_seq=[infos["humanSequence"][i] for i in idx])
    else:
        env.reset_fixed(maps, seqs, human_start=[infos["humanStart"][i] for i in idx],
                        human_goal=[infos["humanGoal"][i] for i in idx])
    return env


def _bfs_policy(method, name):
    """A policy(obs, vec, env, t) for evaluate_fixed_episodes that calls env.<method>(); the env must
    keep the agents' BFS maps: evaluate_fixed_episodes(..., keep_bfs=True)."""
    def policy(obs, vec, env, t):
        if not env.cfg.keep_bfs:
            raise RuntimeError(f"{name} needs the agents' BFS maps: evaluate_fixed_episodes(..., keep_bfs=True)")
        return getattr(env, method)()
    return policy


def descent_policy():
    """The heuristic baseline: every agent one step down its own BFS map (env.descent_actions,
    mapf_descent_actions), ignoring the other agents and the human."""
    return _bfs_policy("descent_actions", "descent_policy")


def pibt_policy(human_weight=None, human_horizon=None):
    """The PIBT planner: one collision-free step for all agents from their BFS maps
    (env.pibt_actions, mapf_pibt_actions).  human_weight / human_horizon: None leaves the env's setting
    alone; an int in 0..16 / 1..8 is set on the env the policy is called with
    (env.set_pibt_human_weight / env.set_pibt_human_horizon)."""
    pick = _bfs_policy("pibt_actions", "pibt_policy")
    if human_weight is None and human_horizon is None:
        return pick

    done = []                           # the env the settings were last made on: one library call per env, not per step

    def policy(obs, vec, env, t):
        if not done or done[0] is not env:
            if human_weight is not None:
                env.set_pibt_human_weight(human_weight)
            if human_horizon is not None:
                env.set_pibt_human_horizon(human_horizon)
            done[:] = [env]
        return pick(obs, vec, env, t)
    return policy


def noisy_policy(policy, eps):
    """`policy` (a per-step policy of evaluate_fixed_episodes, e.g. pibt_policy()) under action noise
    eps in [0, 1]: what it picks is the label, what is played is env.noise_actions(label) -- with
    probability eps the uniform random policy's action (mapf_set_action_noise; mapf.h has the rule).
    The noise is set on the env the policy is called with, once per env."""
    from .env import noise_q16
    q16 = noise_q16(eps)
    done = []

    def noisy(obs, vec, env, t):
        if not done or done[0] is not env:
            env.set_action_noise(q16=q16)
            done[:] = [env]
        return env.noise_actions(policy(obs, vec, env, t))
    return noisy


def evaluate_fixed_episodes(infos, policy, device=None, num_channel=6, fov=9, use_da=False, use_hp=False,
                            human_movement_type=0, max_steps=256, k_predict=5, fix_choice=1, record_actions=False,
                            keep_bfs=False):
    """evaluate() (evaluate.py:169-269) for every episode at once.

    policy(obs [B,N,C,F,F], vec [B,N,4], env, t) -> int32 [B,N] device actions
    (e.g. make_network_policy(network) below, or a random policy); env.episodes
    lists the episode indices of env's rows (one env per map shape).
    fix_choice: fixActions' random.choice -- 1 Philox, 0 the rotating rule.
    human_movement_type 0: LoopingHuman(humanStart, humanGoal); 1: FixedPathHuman(humanSequence).
    Returns {metric: float64 numpy [E]} in episode order (OneEpPerformance fields).
    record_actions: return (metrics, tapes) instead -- tapes[(H, W)] = the policy's actions of that
    map-shape group (not the executed actions_fixed), int32 [max_steps, len(group), N] on the
    device: what replay_fixed_episodes plays back.
    keep_bfs: the envs keep every agent's BFS map current (descent_policy and pibt_policy read them)."""
    device = torch.device("cuda") if device is None else torch.device(device)
    E = infos["numEpisodes"]
    res = {k: np.zeros(E, np.float64) for k in METRIC_KEYS}
    tapes = {}
    for (H, W), idx in sorted(_groups_by_shape(infos).items()):
        env = _group_env(infos, idx, H, W, device, num_channel, fov, use_da, use_hp, human_movement_type, k_predict,
                         fix_choice, keep_bfs)
        if record_actions:
            tapes[(H, W)] = torch.empty(max_steps, env.B, env.N, dtype=torch.int32, device=env.device)
        acc = torch.zeros((len(idx), len(METRIC_KEYS)), dtype=torch.float64, device=device)
        obs, vec = env.observe()
        for t in range(max_steps):
            acts = policy(obs, vec, env, t)
            if record_actions:
                tapes[(H, W)][t].copy_(acts)
            out, obs, vec = env.step_observe(acts)
            st = out["status"]
            acc[:, 0] += out["reward_total"].double().sum(1)
            acc[:, 1] += out["cost"].double().sum(1)
            acc[:, 2] += (st == -2).sum(1)
            acc[:, 3] += (st == -1).sum(1)
            acc[:, 4] += (st == -3).sum(1)
            acc[:, 5] += out["goals_reached"].double().sum(1)
            acc[:, 6] += out["shadow_goals"].double()
            acc[:, 7] += out["constraints"].double().sum(1)
        a = acc.cpu().numpy()
        for k, key in enumerate(METRIC_KEYS):
            res[key][idx] = a[:, k]
        env.close()
    return (res, tapes) if record_actions else res


def replay_fixed_episodes(infos, tapes, device=None, num_channel=6, fov=9, use_da=False, use_hp=False,
                          human_movement_type=0, k_predict=5, fix_choice=1):
    """evaluate_fixed_episodes over recorded actions: tapes[(H, W)] = int32 [T, len(group), N] device
    tensors keyed like its map-shape groups (evaluate_fixed_episodes(..., record_actions=True), or any
    recorded or planned joint actions).  One rollout_actions launch per group into [T]-slot step
    outputs, the OneEpPerformance sums taken once at the end in float64; the observations go to
    scratch slots (the metrics do not read them).  Same env arguments, same {metric: float64 [E]}:
    the integer metrics equal evaluate_fixed_episodes', the float sums up to summation order."""
    device = torch.device("cuda") if device is None else torch.device(device)
    E = infos["numEpisodes"]
    res = {k: np.zeros(E, np.float64) for k in METRIC_KEYS}
    for (H, W), idx in sorted(_groups_by_shape(infos).items()):
        env = _group_env(infos, idx, H, W, device, num_channel, fov, use_da, use_hp, human_movement_type, k_predict,
                         fix_choice)
        tape = tapes[(H, W)]
        T = int(tape.shape[0])
        keys = ("status", "reward_total", "cost", "goals_reached", "shadow_goals", "constraints")
        out = {k: torch.empty((T,) + tuple(env.out[k].shape), dtype=env.out[k].dtype, device=env.device) for k in keys}
        obs = torch.empty((T,) + tuple(env.obs.shape), dtype=torch.float32, device=env.device)
        vec = torch.empty((T,) + tuple(env.vec.shape), dtype=torch.float32, device=env.device)
        env.rollout_actions(tape, slots=True, obs=obs, vec=vec, out=out)
        st = out["status"]
        acc = torch.stack([out["reward_total"].double().sum((0, 2)), out["cost"].double().sum((0, 2)),
                           (st == -2).sum((0, 2)).double(), (st == -1).sum((0, 2)).double(),
                           (st == -3).sum((0, 2)).double(), out["goals_reached"].double().sum((0, 2)),
                           out["shadow_goals"].double().sum(0), out["constraints"].double().sum((0, 2))], dim=1)
        a = acc.cpu().numpy()
        for k, key in enumerate(METRIC_KEYS):
            res[key][idx] = a[:, k]
        env.close()
    return res


def evaluate_fixed_episodes_device(infos, policy, *, tapes=None, human_weight=None, human_horizon=None, device=None,
                                   num_channel=6, fov=9, use_da=False, use_hp=False, human_movement_type=0,
                                   max_steps=256, k_predict=5, fix_choice=1, noise=None):
    """evaluate_fixed_episodes for a policy the rollout kernels run themselves: one rollout_perf launch
    per map-shape group, which steps the whole episode on the device and writes only the eight
    OneEpPerformance numbers of every env (mapf_rollout_perf) -- no observation is computed or stored.
    policy: "descent" | "pibt" (max_steps steps; human_weight / human_horizon as pibt_policy's) or
    "tape" (tapes[(H, W)] = int32 [T, len(group), N], as replay_fixed_episodes takes them).
    noise ("descent" / "pibt" only): action noise eps in [0, 1], as noisy_policy's (env.rollout_perf(noise=)).
    Same env arguments, same {metric: float64 numpy [E]}.  Numerically: the six integer metrics equal
    evaluate_fixed_episodes' exactly; the two float metrics are the reference's own float32 running sums
    (`perf.episodeReward += np.sum(rewards)`: numpy's pairwise float32 sum over the agents, accumulated
    in float32 over the steps), converted to float64 at the end, whereas evaluate_fixed_episodes and
    replay_fixed_episodes sum in float64 -- they agree up to float32 rounding, not bit for bit."""
    from .env import perf_dict
    if policy not in ("descent", "pibt", "tape"):
        raise ValueError(f"policy: expected 'descent', 'pibt' or 'tape', got {policy!r}")
    if policy == "tape" and tapes is None:
        raise ValueError("policy='tape' needs tapes=")
    if noise is not None and policy == "tape":
        raise ValueError("noise= goes with policy 'descent' or 'pibt', not 'tape'")
    device = torch.device("cuda") if device is None else torch.device(device)
    E = infos["numEpisodes"]
    res = {k: np.zeros(E, np.float64) for k in METRIC_KEYS}
    for (H, W), idx in sorted(_groups_by_shape(infos).items()):
        env = _group_env(infos, idx, H, W, device, num_channel, fov, use_da, use_hp, human_movement_type, k_predict,
                         fix_choice, keep_bfs=policy != "tape")
        if policy == "pibt":
            if human_weight is not None:
                env.set_pibt_human_weight(human_weight)
            if human_horizon is not None:
                env.set_pibt_human_horizon(human_horizon)
        if policy == "tape":
            perf = env.rollout_perf(policy="tape", tape=tapes[(H, W)])
        else:
            perf = env.rollout_perf(max_steps, policy, noise=noise)
        for key, col in perf_dict(perf).items():
            res[key][idx] = col.cpu().numpy().astype(np.float64)
        env.close()
    return res


def make_network_policy(network, greedy=False, seed=0):
    """Model.evaluate (model.py:43-60): softmax policy, argmax when greedy, else a
    per-agent categorical draw (Philox inverse CDF in place of np.random.choice)."""
    from .env import sample_actions

    @torch.no_grad()
    def policy(obs, vec, env, t):
        network.num_agents = env.N
        ps = network(obs, vec)[0].float().reshape(env.B, env.N, -1).contiguous()
        if greedy:
            return ps.argmax(-1).to(torch.int32).contiguous()
        return sample_actions(ps, seed, t, out32=env.actions)
    return policy


def summarize(res):
    """The per-metric mean / std over episodes that evaluate() writes to METRICS_JSON_PATH."""
    key = {"hc": "humanCollide", "ecr": "episodeCostReward", "cv": "constraintViolations", "goals": "totalGoals"}
    return {k: {"mean": float(np.mean(res[v])), "std": float(np.std(res[v]))} for k, v in key.items()}
