"""PIBT rollouts (mapf_rollout_pibt) beside random- and descent-policy rollouts, beside the same policy
through per-step launches, and against a baseline build of the library, in one alternated series on
one GPU.

  python tools/bench_pibt.py --config c2                       # this build: random / descent / pibt / per-step
  python tools/bench_pibt.py --config c2 --baseline-lib primal-ppo_amd/lib/libmapf_parent.so --rounds 3
  python tools/bench_pibt.py --config c4 --human-weight 2 --skip-per-step      # the planner at human weight 2
  python tools/bench_pibt.py --config c4 --human-weight 2 --human-horizon 3 --skip-per-step      # ... pricing 3 cells ahead
  python tools/bench_pibt.py --config c2 --noise 0.25 --skip-per-step          # descent and the planner under action noise

Each measurement process builds the preset's env (bench.py's presets and maps), prepares one launcher
per policy over the same [T]-slot buffers (T = 256, c5: 87), every policy on a handle of its own (so
each plays its own episode from the same reset), runs one untimed round, then `--pairs` alternated
rounds random / descent / pibt, each launch between two HIP events, and then `--pairs` per-step
series: PIBT as T x (pibt_actions, step_observe) calls in place, between two HIP events over the whole
series (--skip-per-step leaves it out).  --human-weight W sets the PIBT handle's human weight
(mapf_set_pibt_human_weight; 0, the default, is the plain policy) and --human-horizon K its human horizon
(mapf_set_pibt_human_horizon; 1, the default, prices the human's next cell alone) before its launches.  --noise EPS sets
action noise eps on the descent and the PIBT handle (mapf_set_action_noise; 0, the default, is off; the per-step series
then plays pibt_actions, noise_actions, step_observe; "rewritten" below then compares with the labels).  From the last
timed launch of descent and of PIBT, per env-step: goals reached, agents with status -3 and -2, actions
fixActions rewrote (actions_fixed != actions), agents counted in `constraints`, and the mean cost reward
per agent-step.  With --baseline-lib the driver (which never opens the GPU) starts fresh child processes
in turn, baseline / this build, `--rounds` times: a baseline library runs the policies it has -- a build
from before the PIBT entry points its random and descent policies only, one from before the human weight
its PIBT policy at weight 0 whatever W is, one from before the human horizon at horizon 1 whatever K is.  The
verdicts printed at the end:
  (i)   this build's random, descent and (at weight 0 or horizon 1, where the baseline has it) pibt medians lie inside
        the baseline's own min..max spreads;
  (ii)  the one-launch PIBT median is below the per-step median by more than the per-step series' own
        min..max spread.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "primal-ppo_amd")]
PIBT_FNS = ("mapf_rollout_pibt", "mapf_rollout_pibt_plan", "mapf_pibt_actions", "mapf_pibt_key", "mapf_pibt_host")
HUMAN_FNS = ("mapf_set_pibt_human_weight", "mapf_get_pibt_human_weight", "mapf_pibt_human_level")
NOISE_FNS = ("mapf_set_action_noise", "mapf_get_action_noise", "mapf_noise_actions", "mapf_action_noise_pick")
HORIZON_FNS = ("mapf_set_pibt_human_horizon", "mapf_get_pibt_human_horizon", "mapf_pibt_human_cells", "mapf_pibt_w_word")


def measure(args):
    """One process: per-launch times in us per step, {"random": [...], "descent": [...], "pibt": [...],
    "per-step": [...]}."""
    if args.lib:
        os.environ["MAPF_LIB"] = os.path.abspath(args.lib)
    import torch
    import bench
    from mapf_amd import _lib
    has = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in PIBT_FNS)
    has_weight = has and all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in HUMAN_FNS)
    if not has:                           # a build from before the PIBT entry points: random and descent only
        for n in PIBT_FNS:
            _lib.SIGNATURES.pop(n)
    if not has_weight:                    # a build from before the human weight: the plain policy
        for n in HUMAN_FNS:
            _lib.SIGNATURES.pop(n)
    has_horizon = has_weight and all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in HORIZON_FNS)
    if not has_horizon:                   # a build from before the human horizon: the next cell alone
        for n in HORIZON_FNS:
            _lib.SIGNATURES.pop(n)
    has_noise = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in NOISE_FNS)
    if not has_noise:                     # a build from before action noise: the clean policies
        for n in NOISE_FNS:
            _lib.SIGNATURES.pop(n)
    noise = args.noise if has_noise else 0.0
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    p = bench.PRESETS[args.config]
    B, N, S, F, C = args.envs or p["envs"], p["agents"], p["size"], p["fov"], p["channels"]
    T = args.T or (87 if args.config == "c5" else 256)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    maps, shared = bench.make_maps(p["maps"], B, S, S, 0)

    def make_env():
        e = BatchedMapfGym(make_config(B, S, S, num_agents=N, fov=F, num_channel=C, human_mode="random",
                                       goal_mode="random", fix_choice=1, seed=1234, shared_map=shared), device=dev)
        e.reset_seeded(maps)
        return e
    slots = not args.inplace
    K = T if slots else 1                 # in place: every step re-writes the [B]-leading buffers
    acts = torch.empty(K, B, N, dtype=torch.int32, device=dev)
    obs = torch.empty(K, B, N, C, F, F, dtype=torch.float32, device=dev)
    vec = torch.empty(K, B, N, 4, dtype=torch.float32, device=dev)
    envs = {"random": make_env(), "descent": make_env()}
    if noise:
        envs["descent"].set_action_noise(noise)
    out = {k: torch.empty((K,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in envs["random"].out.items()}
    kw = dict(slots=slots, actions=acts, obs=obs, vec=vec, out=out)
    launch = {"random": envs["random"].rollout_launcher(T, **kw),
              "descent": envs["descent"].rollout_launcher(T, policy="descent", **kw)}
    plan = {"random": envs["random"].rollout_plan(slots, slots), "descent": envs["descent"].rollout_descent_plan(slots, slots)}
    if has:
        envs["pibt"] = penv = make_env()
        if has_weight:
            penv.set_pibt_human_weight(args.human_weight)
        if has_horizon:
            penv.set_pibt_human_horizon(args.human_horizon)
        if noise:
            penv.set_action_noise(noise)
        launch["pibt"] = penv.rollout_launcher(T, policy="pibt", **kw)
        plan["pibt"] = penv.rollout_pibt_plan(slots, slots)
        out0 = {k: v[0] for k, v in out.items()}

        def per_step():
            for _ in range(T):
                a = penv.pibt_actions(acts[0])
                penv.step_observe(penv.noise_actions(a, out=a) if noise else a, obs[0], vec[0], out=out0)
        if not args.skip_per_step:
            launch["per-step"] = per_step
    times = {k: [] for k in launch}
    quality = {}
    # the persistent launches first, the per-step series after them: its launches leave the GPU mostly
    # idle (the host paces them), and a persistent launch right behind it measured slow
    order = [("random", "descent", "pibt")] * (args.pairs + 1) + [("per-step",)] * (args.pairs + 1)
    for rep, keys in enumerate(order):    # round 0 of each phase is untimed: first touch of the buffers, code load
        rep %= args.pairs + 1
        for k in keys:
            if k not in launch:
                continue
            fn = launch[k]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep:
                times[k].append(round(a.elapsed_time(b) * 1e3 / T, 4))
            if k in ("descent", "pibt") and slots:
                steps = float(T * B)
                quality[k] = {"goals": round(float(out["goals_reached"].sum()) / steps, 5),
                              "status_-3": round(float((out["status"] == -3).sum()) / steps, 5),
                              "status_-2": round(float((out["status"] == -2).sum()) / steps, 5),
                              "rewritten": round(float((out["actions_fixed"] != acts).sum()) / steps, 5),
                              "constraints": round(float(out["constraints"].sum()) / steps, 5),
                              "mean_cost": round(float(out["cost"].sum()) / (steps * N), 6)}
    c = sum(e.counters() for e in envs.values())
    print(json.dumps({"config": args.config, "envs": B, "buffers": "slots" if slots else "in place",
                      "lib": os.path.basename(_lib.LIB_PATH), "T": T,
                      "human_weight": args.human_weight if has_weight else 0,
                      "human_horizon": args.human_horizon if has_horizon else 1, "noise": noise, "us_per_step": times, "plan": plan,
                      "per_env_step": quality, "counters": [int(x) for x in c[:8]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c4", "c5"])
    ap.add_argument("--envs", type=int, default=0, help="envs instead of the preset's (a partly filled chip)")
    ap.add_argument("--T", type=int, default=0, help="steps per launch (default 256, c5: 87)")
    ap.add_argument("--pairs", type=int, default=6, help="timed rounds per process")
    ap.add_argument("--rounds", type=int, default=3, help="with --baseline-lib: baseline / this build alternations")
    ap.add_argument("--lib", default=None, help="library to measure (default: the package's)")
    ap.add_argument("--baseline-lib", default=None, help="a baseline build to alternate with (the policies it has)")
    ap.add_argument("--human-weight", type=int, default=0, help="the PIBT policy's human weight, 0..16 (default 0: off)")
    ap.add_argument("--human-horizon", type=int, default=1, help="the PIBT policy's human horizon, 1..8 (default 1: the next cell alone)")
    ap.add_argument("--noise", type=float, default=0.0, help="action noise eps in [0, 1] on descent and pibt (default 0: off)")
    ap.add_argument("--skip-per-step", action="store_true", help="leave out the per-step PIBT series")
    ap.add_argument("--inplace", action="store_true", help="the [B]-leading buffers instead of [T]-slot buffers")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or not args.baseline_lib:
        measure(args)
        return
    series = {"baseline random": [], "baseline descent": [], "baseline pibt": [], "baseline per-step": [],
              "random": [], "descent": [], "pibt": [], "per-step": []}
    for r in range(args.rounds):
        for which, lib in (("baseline", args.baseline_lib), ("new", args.lib)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config, "--T", str(args.T),
                   "--pairs", str(args.pairs)] + (["--lib", lib] if lib else []) + (["--inplace"] if args.inplace else []) + ["--envs", str(args.envs)] + \
                ["--human-weight", str(args.human_weight), "--human-horizon", str(args.human_horizon), "--noise", str(args.noise)] + \
                (["--skip-per-step"] if args.skip_per_step else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                raise SystemExit(f"round {r} {which}: exit {res.returncode}")
            d = json.loads(res.stdout.strip().splitlines()[-1])
            print(r, which, json.dumps(d), flush=True)
            for k, v in d["us_per_step"].items():
                series[("baseline " if which == "baseline" else "") + k] += v
            if which == "new":
                new = d
    print(f"\n{args.config} ({d['envs']} envs): us per step, per launch of T = {d['T']} steps " +
          ("in place" if args.inplace else "into slots (launcher, band-clean after its first call)"))
    stat = {}
    for k, v in series.items():
        if not v:                         # a series this run or the baseline does not have
            continue
        stat[k] = (statistics.median(v), min(v), max(v))
        print(f"  {k:16s} n={len(v):3d} median {stat[k][0]:9.3f} min {stat[k][1]:9.3f} max {stat[k][2]:9.3f}")
    print(f"  per env-step, last launch (pibt at human weight {new['human_weight']}, horizon {new['human_horizon']}): "
          f"{new['per_env_step']}")
    # the baseline plays the same policy: weight 0, or its own weight W at horizon 1 (a baseline with the weight)
    same_policy = (args.human_weight == 0 or args.human_horizon == 1) and args.noise == 0
    for k in ("random", "descent") + (("pibt",) if "baseline pibt" in stat and same_policy else ()):
        bm, lo, hi = stat["baseline " + k]
        print(f"  (i)  {k} median {stat[k][0]:.3f} inside the baseline's [{lo:.3f}, {hi:.3f}]: "
              f"{'PASS' if lo <= stat[k][0] <= hi else 'FAIL'}")
    if "per-step" not in stat:
        return
    pm, plo, phi = stat["per-step"]
    print(f"  (ii) pibt median {stat['pibt'][0]:.3f} < per-step {pm:.3f} - spread {phi - plo:.3f} = {pm - (phi - plo):.3f}: "
          f"{'PASS' if stat['pibt'][0] < pm - (phi - plo) else 'FAIL'}")


if __name__ == "__main__":
    main()
