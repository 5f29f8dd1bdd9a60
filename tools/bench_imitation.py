"""Behaviour cloning at the c3 shape (4096 envs x 8 agents, 20 x 20 warehouse, FOV 9, packed observations):

  python tools/bench_imitation.py                       # all three parts
  python tools/bench_imitation.py --envs 256 --updates 40   # a quick look

  1. DemoRunner.run() per rollout (T = 32 PIBT steps in one launch, plus the slot-0 observe), HIP events
     around the call, median of --reps after one untimed call.
  2. One update at 256 x 8 and 256 x 16 rows, imitation beside PPO of the same build, eager and captured:
     HIP events around _DeviceImitation.run / _DeviceUpdate.run on loaded static inputs (the loads are
     not timed), median of 20 after the two warm-ups and the capture.  The four series are alternated.
  3. The loss and agreement-with-PIBT curves over --updates captured updates (256 x 8 rows each) on PIBT
     demonstrations: a new rollout (the envs run on) every (T * B) // 256 updates, dropout on, the default
     learning rate.
  4. --own-steps K (default 0: skipped) steps of DeviceRunner(expert="pibt") with the model part 3 trained: the
     learner acts, the planner labels the learner's own states, and the share of agent-steps where the policy's
     most probable action is the label is printed -- the agreement off the demonstrations' distribution.

  python tools/bench_imitation.py --noise 0.1 --skip-timing --own-steps 32   # parts 1, 3, 4 on demonstrations under action noise

--noise EPS puts action noise eps on the demonstrations (DemoRunner(noise=...), mapf_set_action_noise): the rollouts
play a uniform random action with probability eps, the labels stay the planner's.  Part 4's labels are clean.

--augment MASK trains part 3 with grid-symmetry augmentation (DeviceTrainer(augment=MASK): 0xFF the whole group,
0x0F rotations only, 0x01 identity only = off) and adds two lines: the time of one whole imitate_rows call
(row gather + captured update) without and with a symmetry per row, alternated, and the agreement with PIBT on
--heldout-rows rows of one more rollout that is not trained on and not augmented (dropout off).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "primal-ppo_amd")]


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=None, help="action noise eps in [0, 1] on the demonstrations")
    ap.add_argument("--own-steps", type=int, default=0, help="part 4: steps the learner acts, the planner labelling (0: skip)")
    ap.add_argument("--skip-timing", action="store_true", help="leave out part 2, the update times")
    ap.add_argument("--augment", type=lambda x: int(x, 0), default=None,
                    help="mask of grid symmetries drawn per minibatch row in part 3 (0xFF: all eight)")
    ap.add_argument("--heldout-rows", type=int, default=4096, help="--augment: rows of the held-out agreement")
    args = ap.parse_args()
    import mapf_amd  # noqa: F401
    import torch
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.imitation import DemoRunner
    from mapf_amd.maps import generate_warehouse
    from mapf_amd.model import Model
    from mapf_amd.trainer import DeviceTrainer
    torch.cuda.set_device(0)
    B, N, S, F, C, T = args.envs, 8, 20, 9, 6, args.T

    # ---- 1. demonstrations
    env = BatchedMapfGym(make_config(B, S, S, num_agents=N, fov=F, num_channel=C, human_mode="random",
                                     goal_mode="random", fix_choice=1, keep_bfs=True, seed=1234))
    env.reset_seeded(generate_warehouse(S, S))
    demo = DemoRunner(env, n_steps=T, policy="pibt", obs_bits=True, seed=args.seed, noise=args.noise)
    demo.run()
    ms = timed(demo.run, args.reps)
    perf = demo.performance_per_env()
    print(json.dumps({"part": "demo", "envs": B, "agents": N, "T": T, "noise_q16": env.action_noise, "plan": env.rollout_plan(True, False, True, policy="pibt"),
                      "ms_per_rollout": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                      "us_per_step": round(statistics.median(ms) * 1e3 / T, 2),
                      "agent_steps_per_s": round(B * N * T / (statistics.median(ms) * 1e-3)),
                      "goals_per_env_step": round(float(perf["totalGoals"].mean()) / T, 4),
                      "agent_collisions": float(perf["agentCollide"].sum())}), flush=True)

    # ---- 2. update times
    torch.manual_seed(args.seed)
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (() if args.skip_timing else (8, 16)):
        rows = 256
        series = {}
        for graph in (False, True):
            model = Model(0, "cuda", global_model=True, numChannel=C, num_agents=n, fov=F)
            model.graph_update = graph
            obs = (torch.rand(rows, n, C, F, F, device="cuda", generator=g) < 0.3).float()
            vec = torch.randn(rows, n, 4, device="cuda", generator=g)
            act = torch.randint(0, 5, (rows, n), device="cuda", generator=g)
            ret, v, cret, cv = (torch.randn(rows, n, device="cuda", generator=g) for _ in range(4))
            ps = torch.softmax(torch.randn(rows, n, 5, device="cuda", generator=g), -1)
            tv = (torch.rand(rows, n, 5, device="cuda", generator=g) < 0.7).float()
            for _ in range(4):                       # two warm-ups, the capture, one replay
                model.imitation_train(obs, vec, act, None)
                model.train(obs, vec, ret, cret, v, cv, act, ps, None, tv, 1.0)
            il = model._updates[next(k for k in model._updates if k[0] == "imitation")]
            ppo = model._updates[next(k for k in model._updates if k[0] != "imitation")]
            assert (il.graph is not None) == graph and (ppo.graph is not None) == graph
            t_il, t_ppo = [], []
            for _ in range(args.reps):               # alternated
                t_il += timed(lambda: il.run(graph=graph), 1)
                t_ppo += timed(lambda: ppo.run(graph=graph), 1)
            mode = "captured" if graph else "eager"
            series[f"imitation {mode}"], series[f"ppo {mode}"] = t_il, t_ppo
            del model, il, ppo
        print(json.dumps({"part": "update", "rows": rows, "agents": n,
                          "ms": {k: {"median": round(statistics.median(x), 3), "min": round(min(x), 3),
                                     "max": round(max(x), 3)} for k, x in series.items()}}), flush=True)

    # ---- 3. learning curve on PIBT demonstrations (the envs run on from rollout to rollout: new states every time)
    env.reset_seeded(generate_warehouse(S, S), seed=7)
    model = Model(0, "cuda", global_model=True, numChannel=C, num_agents=N, fov=F)
    tr = DeviceTrainer(demo, model, minibatch=256, n_epochs=1, seed=args.seed,
                       **({} if args.augment is None else {"augment": args.augment}))
    curve, k = [], 0
    while k < args.updates:
        demo.run()
        for s in tr.imitate(demo)[:args.updates - k]:
            curve.append([float(x) for x in s])
            k += 1
    step = max(1, len(curve) // 30)
    for i in range(0, len(curve), step):
        w = curve[i:i + step]
        print(json.dumps({"part": "curve", "updates": f"{i}..{i + len(w) - 1}",
                          "loss": round(statistics.mean(x[0] for x in w), 4),
                          "agreement": round(statistics.mean(x[2] for x in w), 4),
                          "expert_prob": round(statistics.mean(x[3] for x in w), 4)}), flush=True)
    assert not env.counters()[:8 if not env.action_noise else 1].any()      # (noise boxes agents in: counters 1, 2 may count)

    # ---- 3b. --augment: the held-out agreement (the whole imitate_rows call is timed last: it trains on)
    if args.augment is not None:
        from mapf_amd.env import minibatch_rows, sym_draw, unpack_obs
        n_rows = T * B
        demo.run()                                   # states no update has seen
        held = min(args.heldout_rows, n_rows) // 256 * 256
        hits, was_training = 0.0, model.network.training
        model.network.eval()
        with torch.no_grad():
            for k in range(held // 256):
                r = minibatch_rows(n_rows, args.seed + 1, 0, k * 256, 256)
                ts, bs = r % T, r // T
                obs = unpack_obs(demo.obs_bits[:T][ts, bs].contiguous(), C, F)
                ps = model.network(obs, demo.vec[:T][ts, bs], None)[0]
                hits += float((ps.argmax(-1).to(torch.int32) == demo.expert_actions[ts, bs]).float().mean())
        model.network.train(was_training)
        print(json.dumps({"part": "heldout", "augment": args.augment, "updates": len(curve), "rows": held,
                          "agreement": round(hits / max(1, held // 256), 4)}), flush=True)

    # ---- 4. the learner on its own states, labelled by the planner (no noise: the sampler explores)
    if args.own_steps > 0:
        from mapf_amd.runner import DeviceRunner
        own = BatchedMapfGym(make_config(B, S, S, num_agents=N, fov=F, num_channel=C, human_mode="random",
                                         goal_mode="random", fix_choice=1, keep_bfs=True, seed=4321))
        own.reset_seeded(generate_warehouse(S, S), seed=11)
        runner = DeviceRunner(own, model, n_steps=args.own_steps, seed=args.seed, obs_bits=True, expert="pibt")
        runner.run()
        agree = (runner.ps.argmax(-1).to(torch.int32) == runner.expert_actions).float().mean()
        print(json.dumps({"part": "own_states", "steps": args.own_steps, "demo_noise_q16": env.action_noise,
                          "agreement": round(float(agree), 4),
                          "goals_per_env_step": round(float(runner.goals.sum()) / (args.own_steps * B), 4),
                          "agent_collisions_per_env_step": round(float((runner.status == -3).sum()) / (args.own_steps * B), 4)}),
              flush=True)

    # ---- 5. --augment: the whole imitate_rows call without and with a symmetry per row
    if args.augment is not None:
        rows = minibatch_rows(n_rows, args.seed, 0, 0, 256)
        sym = sym_draw(args.seed, 0, 0, 256, args.augment if args.augment != 1 else 0xFF)
        t_plain, t_sym = [], []
        for _ in range(args.reps):                   # alternated
            t_plain += timed(lambda: model.imitate_rows(demo, rows, checked=True), 1)
            t_sym += timed(lambda: model.imitate_rows(demo, rows, checked=True, sym=sym), 1)
        print(json.dumps({"part": "imitate_rows", "rows": 256, "agents": N,
                          "ms": {k: {"median": round(statistics.median(x), 3), "min": round(min(x), 3),
                                     "max": round(max(x), 3)} for k, x in (("sym=None", t_plain), ("sym", t_sym))}}),
              flush=True)


if __name__ == "__main__":
    main()
