"""Packed-observation rollouts (MAPF_SLOTS_OBS_BITS: one bit per cell) beside float rollouts of the same
process, and against a baseline build of the library, in one alternated series on one GPU.

  python tools/bench_bits.py --config c2                       # this build: float / packed
  python tools/bench_bits.py --config c2 --baseline-lib primal-ppo_amd/lib/libmapf_parent.so --rounds 3

Each measurement process builds the preset's env twice (bench.py's presets and maps; one handle per
output format, so both play the same episode), prepares one random-policy launcher per format over
[T]-slot buffers (T = 256; c5: 87, bench.py's slot cap -- its 256 float slots are 113 GB), runs one
untimed float / packed pair, then `--pairs` alternated pairs, each launch between two HIP events over
the whole launch.  With --baseline-lib the driver (which never opens the GPU) starts fresh child
processes in turn, baseline / this build, `--rounds` times: the baseline library (the parent commit's
build) lacks the packed entry points, so they are dropped from the binding for that process only and
it runs the float launches alone.  The verdicts printed at the end:
  (i)  this build's float median lies inside the baseline's own min..max spread;
  (ii) the packed median is no higher than this build's float median plus the baseline's spread.
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
BITS_FNS = ("mapf_obs_bits_words", "mapf_observe_bits", "mapf_step_observe_bits", "mapf_obs_pack_host",
            "mapf_obs_unpack_host", "mapf_unpack_obs", "mapf_conv_first_bits")


def measure(args):
    """One process: per-launch times in us per step, {"float": [...], "packed": [...]}."""
    if args.lib:
        os.environ["MAPF_LIB"] = os.path.abspath(args.lib)
    import torch
    import bench
    from mapf_amd import _lib
    has = all(hasattr(ctypes.CDLL(_lib.LIB_PATH), n) for n in BITS_FNS)
    if not has:                           # a build from before the packed entry points: float launches only
        for n in BITS_FNS:
            _lib.SIGNATURES.pop(n)
        _lib.lib().mapf_obs_bits_words = lambda cfg: 0
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
    envs, launch, plan, nbytes = {}, {}, {}, {}
    for fmt in ("float", "packed") if has else ("float",):
        env = envs[fmt] = make_env()
        packed = fmt == "packed"
        obs = (torch.empty(K, B, N, env.obs_words, dtype=torch.int32, device=dev) if packed else
               torch.empty(K, B, N, C, F, F, dtype=torch.float32, device=dev))
        kw = dict(slots=slots, actions=torch.empty(K, B, N, dtype=torch.int32, device=dev), obs=obs,
                  vec=torch.empty(K, B, N, 4, dtype=torch.float32, device=dev),
                  out={k: torch.empty((K,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in env.out.items()})
        if packed:
            kw["obs_bits"] = True
        launch[fmt] = env.rollout_launcher(T, **kw)
        plan[fmt] = env.rollout_plan(slots, slots, True) if packed else env.rollout_plan(slots, slots)
        nbytes[fmt] = obs.nbytes
    times = {k: [] for k in launch}
    for rep in range(args.pairs + 1):     # round 0 is untimed: first touch of the buffers, code load
        for k, fn in launch.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep:
                times[k].append(round(a.elapsed_time(b) * 1e3 / T, 4))
    c = sum(e.counters() for e in envs.values())
    print(json.dumps({"config": args.config, "envs": B, "buffers": "slots" if slots else "in place",
                      "lib": os.path.basename(_lib.LIB_PATH), "T": T, "us_per_step": times, "plan": plan,
                      "obs_bytes": nbytes, "counters": [int(x) for x in c[:8]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c4", "c5"])
    ap.add_argument("--envs", type=int, default=0, help="envs instead of the preset's (a partly filled chip)")
    ap.add_argument("--T", type=int, default=0, help="steps per launch (default 256, c5: 87)")
    ap.add_argument("--pairs", type=int, default=6, help="timed rounds per process")
    ap.add_argument("--rounds", type=int, default=3, help="with --baseline-lib: baseline / this build alternations")
    ap.add_argument("--lib", default=None, help="library to measure (default: the package's)")
    ap.add_argument("--baseline-lib", default=None, help="a baseline build to alternate with (float launches only)")
    ap.add_argument("--inplace", action="store_true", help="the [B]-leading buffers instead of [T]-slot buffers")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or not args.baseline_lib:
        measure(args)
        return
    series = {"baseline float": [], "float": [], "packed": []}
    for r in range(args.rounds):
        for which, lib in (("baseline", args.baseline_lib), ("new", args.lib)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", args.config, "--T", str(args.T),
                   "--pairs", str(args.pairs)] + (["--lib", lib] if lib else []) + (["--inplace"] if args.inplace else []) + ["--envs", str(args.envs)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                raise SystemExit(f"round {r} {which}: exit {res.returncode}")
            d = json.loads(res.stdout.strip().splitlines()[-1])
            print(r, which, json.dumps(d), flush=True)
            for k, v in d["us_per_step"].items():
                series[("baseline " if which == "baseline" else "") + k] += v
    print(f"\n{args.config} ({d['envs']} envs): us per step, per launch of T = {d['T']} steps " +
          ("in place" if args.inplace else "into slots (launcher; float: band-clean after its first call)"))
    print(f"  observation buffer bytes: {d['obs_bytes']}")
    stat = {}
    for k, v in series.items():
        stat[k] = (statistics.median(v), min(v), max(v))
        print(f"  {k:16s} n={len(v):3d} median {stat[k][0]:9.3f} min {stat[k][1]:9.3f} max {stat[k][2]:9.3f}")
    bm, lo, hi = stat["baseline float"]
    fm, pm = stat["float"][0], stat["packed"][0]
    print(f"  baseline spread {hi - lo:.3f}")
    print(f"  (i)  float median {fm:.3f} inside [{lo:.3f}, {hi:.3f}]: {'PASS' if lo <= fm <= hi else 'FAIL'}")
    print(f"  (ii) packed median {pm:.3f} <= float {fm:.3f} + spread {hi - lo:.3f} = {fm + hi - lo:.3f}: "
          f"{'PASS' if pm <= fm + (hi - lo) else 'FAIL'}")
    print(f"  packed / float: {pm / fm:.3f} ({fm / pm:.2f}x)")


if __name__ == "__main__":
    main()
