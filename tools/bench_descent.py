"""Descent-policy rollouts (mapf_rollout_descent) beside random-policy rollouts, beside the same
policy through per-step launches, and against a baseline build of the library, in one alternated
series on one GPU.

  python tools/bench_descent.py --config c2                       # this build: random / descent / per-step
  python tools/bench_descent.py --config c2 --baseline-lib primal-ppo_amd/lib/libmapf_parent.so --rounds 3

Each measurement process builds the preset's env (bench.py's presets and maps), prepares one launcher
per policy over the same [T]-slot buffers (T = 256, c5: 87), runs one untimed random / descent pair,
then `--pairs` alternated pairs, each launch between two HIP events (the random policy on a handle
of its own, the descent launches and the per-step series sharing another), and then `--pairs`
per-step series: the same policy as T x (descent_actions, step_observe) calls in place, between two
HIP events over the whole series.  Goal changes per env-step come from goals_reached of the last
timed launch.  --noise EPS sets action noise eps on the descent handle (mapf_set_action_noise; 0, the
default, is off; the per-step series then plays descent_actions, noise_actions, step_observe; a
baseline from before action noise runs without).  With --baseline-lib the
driver (which never opens the GPU) starts fresh child processes in turn, baseline / this build,
`--rounds` times: the baseline library (the parent commit's build, which has no descent entry
points) runs its random policy only.  The verdicts printed at the end:
  (i)   this build's random median lies inside the baseline's own min..max spread;
  (iii) the one-launch descent median is below the per-step median by more than the per-step
        series' own min..max spread.
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
NOISE_FNS = ("mapf_set_action_noise", "mapf_get_action_noise", "mapf_noise_actions", "mapf_action_noise_pick")
DESCENT_FNS = ("mapf_rollout_descent", "mapf_rollout_descent_plan", "mapf_descent_actions", "mapf_descent_pick")


def measure(args):
    """One process: per-launch times in us per step, {"random": [...], "descent": [...], "per-step": [...]}."""
    if args.lib:
        os.environ["MAPF_LIB"] = os.path.abspath(args.lib)
    import torch
    import bench
    from mapf_amd import _lib
    has = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in DESCENT_FNS)
    if not has:                           # a build from before the descent entry points: random policy only
        for n in DESCENT_FNS:
            _lib.SIGNATURES.pop(n)
    has_noise = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in NOISE_FNS)
    if not has_noise:                     # a build from before action noise: the clean policy
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
    # the random policy keeps a handle of its own: its episode is then the baseline process's, not
    # one the descent launches moved on (agents parked next to their goals: 8x the goal changes)
    env = make_env()
    slots = not args.inplace
    K = T if slots else 1                 # in place: every step re-writes the [B]-leading buffers
    acts = torch.empty(K, B, N, dtype=torch.int32, device=dev)
    obs = torch.empty(K, B, N, C, F, F, dtype=torch.float32, device=dev)
    vec = torch.empty(K, B, N, 4, dtype=torch.float32, device=dev)
    out = {k: torch.empty((K,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in env.out.items()}
    kw = dict(slots=slots, actions=acts, obs=obs, vec=vec, out=out)
    launch = {"random": env.rollout_launcher(T, **kw)}
    plan = {"random": env.rollout_plan(slots, slots)}
    if has:
        denv = make_env()
        if noise:
            denv.set_action_noise(noise)
        launch["descent"] = denv.rollout_launcher(T, policy="descent", **kw)
        plan["descent"] = denv.rollout_descent_plan(slots, slots)
        out0 = {k: v[0] for k, v in out.items()}

        def per_step():
            for _ in range(T):
                a = denv.descent_actions(acts[0])
                denv.step_observe(denv.noise_actions(a, out=a) if noise else a, obs[0], vec[0], out=out0)
        launch["per-step"] = per_step
    times = {k: [] for k in launch}
    goals = {}
    # random / descent pairs first, the per-step series after them: its launches leave the GPU
    # mostly idle (the host paces them), and a persistent launch right behind it measured 6 % slow
    order = [("random", "descent")] * (args.pairs + 1) + [("per-step",)] * (args.pairs + 1)
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
            if k != "per-step" and slots:
                goals[k] = round(float(out["goals_reached"].sum()) / (T * B), 5)
    c = env.counters() + (denv.counters() if has else 0)
    print(json.dumps({"config": args.config, "envs": B, "buffers": "slots" if slots else "in place",
                      "lib": os.path.basename(_lib.LIB_PATH), "T": T, "noise": noise, "us_per_step": times, "plan": plan,
                      "goal_changes_per_env_step": goals, "counters": [int(x) for x in c[:8]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c4", "c5"])
    ap.add_argument("--envs", type=int, default=0, help="envs instead of the preset's (a partly filled chip)")
    ap.add_argument("--T", type=int, default=0, help="steps per launch (default 256, c5: 87)")
    ap.add_argument("--pairs", type=int, default=6, help="timed rounds per process")
    ap.add_argument("--rounds", type=int, default=3, help="with --baseline-lib: baseline / this build alternations")
    ap.add_argument("--lib", default=None, help="library to measure (default: the package's)")
    ap.add_argument("--baseline-lib", default=None, help="a baseline build to alternate with (random policy only)")
    ap.add_argument("--inplace", action="store_true", help="the [B]-leading buffers instead of [T]-slot buffers")
    ap.add_argument("--noise", type=float, default=0.0, help="action noise eps in [0, 1] on the descent policy (default 0: off)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or not args.baseline_lib:
        measure(args)
        return
    series = {"baseline random": [], "random": [], "descent": [], "per-step": []}
    for r in range(args.rounds):
        for which, lib in (("baseline", args.baseline_lib), ("new", args.lib)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config, "--T", str(args.T),
                   "--pairs", str(args.pairs)] + (["--lib", lib] if lib else []) + (["--inplace"] if args.inplace else []) + ["--envs", str(args.envs)] + \
                ["--noise", str(args.noise)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                raise SystemExit(f"round {r} {which}: exit {res.returncode}")
            d = json.loads(res.stdout.strip().splitlines()[-1])
            print(r, which, json.dumps(d), flush=True)
            for k, v in d["us_per_step"].items():
                series[("baseline " if which == "baseline" else "") + k] += v
    print(f"\n{args.config} ({d['envs']} envs): us per step, per launch of T = {d['T']} steps " +
          ("in place" if args.inplace else "into slots (launcher, band-clean after its first call)"))
    stat = {}
    for k, v in series.items():
        stat[k] = (statistics.median(v), min(v), max(v))
        print(f"  {k:16s} n={len(v):3d} median {stat[k][0]:9.3f} min {stat[k][1]:9.3f} max {stat[k][2]:9.3f}")
    print(f"  goal changes per env-step: {d['goal_changes_per_env_step']}")
    bm, lo, hi = stat["baseline random"]
    print(f"  baseline spread {hi - lo:.3f}")
    print(f"  (i)   random median {stat['random'][0]:.3f} inside [{lo:.3f}, {hi:.3f}]: "
          f"{'PASS' if lo <= stat['random'][0] <= hi else 'FAIL'}")
    pm, plo, phi = stat["per-step"]
    print(f"  (iii) descent median {stat['descent'][0]:.3f} < per-step {pm:.3f} - spread {phi - plo:.3f} = {pm - (phi - plo):.3f}: "
          f"{'PASS' if stat['descent'][0] < pm - (phi - plo) else 'FAIL'}")


if __name__ == "__main__":
    main()
