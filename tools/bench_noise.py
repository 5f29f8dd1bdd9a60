"""Action noise on the planners' rollouts (mapf_set_action_noise): what it costs and what it does.

  python tools/bench_noise.py --config c2                                   # this build: eps 0 / 0.05 / 0.25
  python tools/bench_noise.py --config c4 --baseline-lib primal-ppo_amd/lib/libmapf_parent.so --rounds 2
  python tools/bench_noise.py --config c2 --quality                         # what noise does to the planners

Times.  One process builds the preset's env (bench.py's presets and maps) once per (policy, eps) -- descent and
PIBT, each eps on a handle of its own, so every series plays its own episode from the same reset -- and measures
two forms: "bits", rollout(slots=True, obs_bits=True) through a launcher into shared [T]-slot buffers with all
step outputs, and "perf", rollout_perf.  One untimed round, then `--windows` rounds over all series in turn, each
launch of T steps (256; c5: 64) between two HIP events; us per step.  With --baseline-lib the driver (which never
opens the GPU) starts fresh child processes in turn, baseline / this build, `--rounds` times; a baseline from
before action noise runs eps 0 only.  Printed at the end: median (min-max) per series, noise 0 against the
baseline's own window-to-window spread, and eps > 0 against noise 0.  Per env-step of the last bits launch: goals,
agents with status -3, agents counted in `constraints`.

--quality: per (policy, eps), `--steps` per-step triples (the policy's pick, noise_actions, step) from the reset,
so that the action played is at hand: per env-step goals, constraints, status -3 (agentCollide) and actions
fixActions rewrote (actions_fixed != played).
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
POLICIES = ("descent", "pibt")


def setup(args):
    if args.lib:
        os.environ["MAPF_LIB"] = os.path.abspath(args.lib)
    import torch
    import bench
    from mapf_amd import _lib
    has_noise = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in NOISE_FNS)
    if not has_noise:                     # a build from before action noise
        for n in NOISE_FNS:
            _lib.SIGNATURES.pop(n)
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    p = bench.PRESETS[args.config]
    B, N, S, F, C = args.envs or p["envs"], p["agents"], p["size"], p["fov"], p["channels"]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    maps, shared = bench.make_maps(p["maps"], B, S, S, 0)

    def make_env(eps):
        e = BatchedMapfGym(make_config(B, S, S, num_agents=N, fov=F, num_channel=C, human_mode="random",
                                       goal_mode="random", fix_choice=1, seed=1234, shared_map=shared), device=dev)
        e.reset_seeded(maps)
        if eps:
            e.set_action_noise(eps)
        return e
    return torch, _lib, has_noise, make_env, dev, B, N


def measure(args):
    torch, _lib, has_noise, make_env, dev, B, N = setup(args)
    T = args.T or (64 if args.config == "c5" else 256)
    eps_list = [e for e in args.eps if e == 0 or has_noise]
    envs = {(pol, eps): make_env(eps) for pol in POLICIES for eps in eps_list}
    first = next(iter(envs.values()))
    acts = torch.empty(T, B, N, dtype=torch.int32, device=dev)
    bits = torch.empty(T, B, N, first.obs_words, dtype=torch.int32, device=dev)
    vec = torch.empty(T, B, N, 4, dtype=torch.float32, device=dev)
    out = {k: torch.empty((T,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in first.out.items()}
    perf = torch.zeros(B, 8, dtype=torch.int32, device=dev)
    launch, plan = {}, {}
    for (pol, eps), e in envs.items():
        launch[f"{pol} bits eps={eps}"] = e.rollout_launcher(T, slots=True, actions=acts, obs=bits, vec=vec, out=out, policy=pol,
                                                             obs_bits=True)
        launch[f"{pol} perf eps={eps}"] = (lambda e=e, pol=pol: e.rollout_perf(T, pol, perf=perf))
        plan[f"{pol} bits eps={eps}"] = e.rollout_plan(True, False, True, policy=pol)
        plan[f"{pol} perf eps={eps}"] = e.rollout_perf_plan(pol)
    times = {k: [] for k in launch}
    quality = {}
    for rep in range(args.windows + 1):   # round 0 is untimed: first touch of the buffers, code load
        for k, fn in launch.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep:
                times[k].append(round(a.elapsed_time(b) * 1e3 / T, 4))
            if " bits " in k and rep == args.windows:
                steps = float(T * B)
                quality[k] = {"goals": round(float(out["goals_reached"].sum()) / steps, 5),
                              "status_-3": round(float((out["status"] == -3).sum()) / steps, 5),
                              "constraints": round(float(out["constraints"].sum()) / steps, 5)}
    print(json.dumps({"config": args.config, "envs": B, "lib": os.path.basename(_lib.LIB_PATH), "T": T, "us_per_step": times,
                      "per_env_step": quality, "plan": plan}), flush=True)


def quality(args):
    torch, _lib, has_noise, make_env, dev, B, N = setup(args)
    for pol in POLICIES:
        for eps in args.eps:
            e = make_env(eps)
            pick = e.pibt_actions if pol == "pibt" else e.descent_actions
            tot = dict(goals=0.0, constraints=0.0, agentCollide=0.0, rewritten=0.0, noisy=0.0)
            for _ in range(args.steps):
                label = pick()
                played = e.noise_actions(label)
                o = e.step(played)
                tot["goals"] += float(o["goals_reached"].sum())
                tot["constraints"] += float(o["constraints"].sum())
                tot["agentCollide"] += float((o["status"] == -3).sum())
                tot["rewritten"] += float((o["actions_fixed"] != played).sum())
                tot["noisy"] += float((played != label).sum())
            print(json.dumps({"config": args.config, "envs": B, "policy": pol, "eps": eps, "steps": args.steps,
                              "per_env_step": {k: round(v / (args.steps * B), 5) for k, v in tot.items()},
                              "counters": [int(x) for x in e.counters()[:8]]}), flush=True)
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c4", "c5"])
    ap.add_argument("--envs", type=int, default=0, help="envs instead of the preset's")
    ap.add_argument("--T", type=int, default=0, help="steps per launch (default 256, c5: 64)")
    ap.add_argument("--eps", type=float, nargs="+", default=[0.0, 0.05, 0.25])
    ap.add_argument("--windows", type=int, default=6, help="timed rounds per process")
    ap.add_argument("--rounds", type=int, default=2, help="with --baseline-lib: baseline / this build alternations")
    ap.add_argument("--lib", default=None, help="library to measure (default: the package's)")
    ap.add_argument("--baseline-lib", default=None, help="a baseline build to alternate with (eps 0 only)")
    ap.add_argument("--quality", action="store_true", help="what noise does to the planners, per-step triples")
    ap.add_argument("--steps", type=int, default=128, help="--quality: steps per (policy, eps)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.quality:
        quality(args)
        return
    if args.child or not args.baseline_lib:
        measure(args)
        return
    series = {}
    for r in range(args.rounds):
        for which, lib in (("baseline", args.baseline_lib), ("new", args.lib)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config, "--T", str(args.T), "--envs",
                   str(args.envs), "--windows", str(args.windows), "--eps"] + [str(e) for e in args.eps] + (["--lib", lib] if lib else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                raise SystemExit(f"round {r} {which}: exit {res.returncode}")
            d = json.loads(res.stdout.strip().splitlines()[-1])
            print(r, which, json.dumps(d), flush=True)
            for k, v in d["us_per_step"].items():
                series.setdefault(("baseline " if which == "baseline" else "") + k, []).extend(v)
    stat = {k: (statistics.median(v), min(v), max(v)) for k, v in series.items() if v}
    print(f"\n{args.config} ({d['envs']} envs): us per step, per launch of T = {d['T']} steps")
    for k, (m, lo, hi) in sorted(stat.items()):
        print(f"  {k:34s} n={len(series[k]):3d} median {m:9.3f} min {lo:9.3f} max {hi:9.3f}")
    for k in sorted(stat):
        if k.startswith("baseline "):
            new = stat.get(k[len("baseline "):])
            if new:
                m, lo, hi = stat[k]
                print(f"  noise 0 vs baseline  {k[9:]:26s} {new[0]:.3f} inside [{lo:.3f}, {hi:.3f}]: "
                      f"{'yes' if lo <= new[0] <= hi else 'no'} ({(new[0] / m - 1) * 100:+.2f} % of the baseline's median)")
    for k in sorted(stat):
        if not k.startswith("baseline ") and not k.endswith("eps=0.0"):
            base = stat.get(k.rsplit(" ", 1)[0] + " eps=0.0")
            if base:
                print(f"  eps vs noise 0       {k:26s} {stat[k][0]:.3f} against {base[0]:.3f}: {(stat[k][0] / base[0] - 1) * 100:+.2f} %")


if __name__ == "__main__":
    main()
