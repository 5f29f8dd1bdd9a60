"""Input load of one minibatch at the c3 shape (256 rows x 8 agents, FOV 9, 6 channels) from a T x B rollout:

  python tools/bench_gather_sym.py [--rows 256] [--envs 256] [--T 32] [--reps 200]

Routes, packed and float observations, each filling an imitation update's inputs (observation, vec, int32 actions):
  two_launch   env.gather_rows (into a staging tensor when packed) + env.unpack_obs: what sym=None does
  sym_identity env.gather_rows_sym with sym=None: one launch, no staging
  sym_random   env.gather_rows_sym with a uniform symmetry per row
and the PPO update's nine arrays (float observations), gather_rows against gather_rows_sym with random symmetries.
HIP events around each call; the routes are alternated inside every repetition; median, min and max in us.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "primal-ppo_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    import mapf_amd  # noqa: F401
    import torch
    from mapf_amd.env import gather_rows, gather_rows_sym, minibatch_rows, obs_words, sym_draw, unpack_obs
    torch.cuda.set_device(0)
    M, B, T, N, C, F = args.rows, args.envs, args.T, 8, 6, 9
    g = torch.Generator(device="cuda").manual_seed(1)
    W = obs_words(C, F)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (T, B, N, W), device="cuda", generator=g, dtype=torch.int64).int()
    bits[..., -1] &= (1 << (C * F * F - 32 * (W - 1))) - 1 if C * F * F % 32 else -1      # the padding bits are 0
    obs = unpack_obs(bits, C, F)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    vec, act = r(T, B, N, 4), torch.randint(0, 5, (T, B, N), device="cuda", generator=g).int()
    ppo = [obs, vec, r(T, B, N), r(T, B, N), r(T, B, N), r(T, B, N), act.long(), r(T, B, N, 5), r(T, B, N, 5)]
    d_obs, d_vec, d_act = torch.empty(M, N, C, F, F, device="cuda"), torch.empty(M, N, 4, device="cuda"), \
        torch.empty(M, N, dtype=torch.int32, device="cuda")
    stage = torch.empty(M, N, W, dtype=torch.int32, device="cuda")
    d_ppo = [torch.empty((M,) + tuple(x.shape[2:]), dtype=x.dtype, device="cuda") for x in ppo]
    kinds_ppo = ("obs", "vec", "plain", "plain", "plain", "plain", "action64", "cols", "cols")
    rows = minibatch_rows(T * B, 0, 0, 0, M)
    sym = sym_draw(0, 0, 0, M, 0xFF)
    geo = (N, C, F)

    def packed_two():
        gather_rows((bits, vec, act), T, B, rows, (stage, d_vec, d_act))
        unpack_obs(stage, C, F, out=d_obs)

    routes = {
        "packed two_launch": packed_two,
        "packed sym_identity": lambda: gather_rows_sym((bits, vec, act), T, B, rows, (d_obs, d_vec, d_act),
                                                       ("obs_bits", "vec", "action32"), geometry=geo),
        "packed sym_random": lambda: gather_rows_sym((bits, vec, act), T, B, rows, (d_obs, d_vec, d_act),
                                                     ("obs_bits", "vec", "action32"), sym=sym, geometry=geo),
        "float two_launch": lambda: gather_rows((obs, vec, act), T, B, rows, (d_obs, d_vec, d_act)),
        "float sym_identity": lambda: gather_rows_sym((obs, vec, act), T, B, rows, (d_obs, d_vec, d_act),
                                                      ("obs", "vec", "action32"), geometry=geo),
        "float sym_random": lambda: gather_rows_sym((obs, vec, act), T, B, rows, (d_obs, d_vec, d_act),
                                                    ("obs", "vec", "action32"), sym=sym, geometry=geo),
        "ppo9 gather_rows": lambda: gather_rows(ppo, T, B, rows, d_ppo),
        "ppo9 sym_random": lambda: gather_rows_sym(ppo, T, B, rows, d_ppo, kinds_ppo, sym=sym, geometry=geo),
    }
    times = {k: [] for k in routes}
    for rep in range(args.reps + 20):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= 20:                                # warm
                times[k].append(a.elapsed_time(b) * 1e3)
    print(json.dumps({"rows": M, "agents": N, "C": C, "F": F, "T": T, "envs": B, "reps": args.reps,
                      "us": {k: {"median": round(statistics.median(x), 1), "min": round(min(x), 1),
                                 "p90": round(sorted(x)[int(0.9 * len(x))], 1), "max": round(max(x), 1)}
                             for k, x in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
