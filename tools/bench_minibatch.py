"""Input load of one PPO minibatch at the c3 update shape (256 rows x 8 agents, FOV 9, 6 channels), two ways,
alternated in one process, HIP events around the load only:
  (a) host indices: `field[mb_inds]` over the nine EnvMajorRows fields (one H2D copy of the index pair, nine
      advanced-index launches), then _DeviceUpdate.load (nine copy_ launches + the coefficients' H2D copy);
  (b) device rows: env.minibatch_rows (one launch), then _DeviceUpdate.load_rows (one gather launch + the
      coefficients' H2D copy).
The rollout buffers are synthetic (random, --envs x --steps rows, t-major); a row's bytes do not matter to a copy.
With --update: also one DeviceTrainer.update epoch at --update-envs x --steps (minibatch 256) against the same
updates through Model.train on torch-indexed rows, wall-clock per update, from a real rollout.
One JSON line per measurement."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "primal-ppo_amd")]
import mapf_amd  # noqa: E402,F401  (first: the HIP graph-capture mode)
import torch  # noqa: E402

from mapf_amd.env import minibatch_rows  # noqa: E402
from mapf_amd.model import Model  # noqa: E402
from mapf_amd.runner import EnvMajorRows  # noqa: E402

N, C, F, M = 8, 6, 9, 256


def summary(xs):
    xs = np.asarray(xs)
    return dict(median=round(float(np.median(xs)), 2), min=round(float(xs.min()), 2), max=round(float(xs.max()), 2))


def bench_load(args):
    T, B = args.steps, args.envs
    dev = torch.device("cuda")
    model = Model(0, dev, global_model=True, numChannel=C, num_agents=N, fov=F)
    r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
    bufs = (r(T + 1, B, N, C, F, F)[:T], r(T + 1, B, N, 4)[:T], r(T, B, N), r(T, B, N), r(T, B, N), r(T, B, N),
            torch.randint(0, 5, (T, B, N), device=dev), r(T, B, N, 5), r(T, B, N, 5))
    views = [EnvMajorRows(b, T, B) for b in bufs]
    meta = lambda x, *tail: torch.empty((M,) + tuple(x.shape[2:]) + tail, device="meta")     # noqa: E731
    upd = model._device_update(meta(bufs[0]), meta(bufs[1]), meta(bufs[2]), meta(bufs[7]), meta(bufs[8]),
                               meta(bufs[6], 1))
    coef, lam = model._loss_coef(0.5), 0.5
    rows = torch.empty(M, dtype=torch.int64, device=dev)
    rng = np.random.default_rng(0)
    n = T * B

    def load_host(k):
        inds = rng.integers(0, n, M)
        obs, vec, ret, cret, v, cv, act, ps, tv = (f[inds] for f in views)
        upd.load(obs, vec, ret, cret, v, cv, act.unsqueeze(-1), ps, tv, coef=coef, lam=lam)

    def load_device(k):
        minibatch_rows(n, 0, k // (n // M), (k % (n // M)) * M, M, out=rows)
        upd.load_rows(bufs, T, B, rows, coef=coef, lam=lam)

    ways = {"host_index_then_load": load_host, "minibatch_rows_then_load_rows": load_device}
    ev = {w: [] for w in ways}
    wall = {w: [] for w in ways}
    for k in range(args.warmup + args.iters):
        for w, fn in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn(k)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ev[w].append(e0.elapsed_time(e1) * 1e3)
                wall[w].append((t1 - t0) * 1e6)
    # the two ways loaded the same bytes: check the last device load against torch indexing
    assert torch.equal(upd.obs, bufs[0][rows % T, rows // T]) and torch.equal(upd.tv, bufs[8][rows % T, rows // T])
    bytes_moved = 2 * M * sum(b[0, 0].numel() * b.element_size() for b in bufs)
    launches = {"host_index_then_load": "1 H2D index copy + 9 index + 9 copy_ launches + 1 H2D coefficient copy",
                "minibatch_rows_then_load_rows": "1 rows + 1 gather launch + 1 H2D coefficient copy"}
    for w in ways:
        print(json.dumps(dict(what="minibatch_load", way=w, rows=M, agents=N, fov=F, channels=C, envs=B, steps=T,
                              iters=args.iters, warmup=args.warmup, event_us=summary(ev[w]),
                              host_issue_us=summary(wall[w]), bytes_read_plus_written=bytes_moved,
                              launches=launches[w])), flush=True)
    del bufs, views, upd


def bench_update(args):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    from mapf_amd.runner import DeviceRunner
    from mapf_amd.trainer import DeviceTrainer
    T, B = args.steps, args.update_envs
    torch.manual_seed(0)
    model = Model(0, "cuda", global_model=True, numChannel=C, num_agents=N, fov=F)
    twin = copy.deepcopy(model)
    env = BatchedMapfGym(make_config(B, 20, 20, num_agents=N, fov=F, num_channel=C, human_mode="random",
                                     goal_mode="random", fix_choice=1, seed=1))
    env.reset_seeded(generate_warehouse(20, 20))
    runner = DeviceRunner(env, copy.deepcopy(model), n_steps=T, seed=1)
    mb, perf = runner.run()
    n, K = T * B, T * B // M
    trainer = DeviceTrainer(runner, model, minibatch=M, n_epochs=1, seed=0)

    def epoch_train():
        for k in range(K):
            rows = minibatch_rows(n, 0, 0, k * M, M)
            twin.train(mb.observations[rows], mb.vectors[rows], mb.returns[rows], mb.costReturns[rows],
                       mb.values[rows], mb.costValues[rows], mb.actions[rows], mb.ps[rows], mb.hiddenState[rows],
                       mb.trainValid[rows], perf.episodeCostReward)

    ways = {"DeviceTrainer.update": lambda: trainer.update(perf), "Model.train_on_indexed_rows": epoch_train}
    for rnd in range(args.rounds + 1):          # round 0: warm-up (eager updates, the capture, MIOpen find)
        for w, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps(dict(what="update_epoch", way=w, round=rnd, warmup=rnd == 0, envs=B, steps=T,
                                  minibatch=M, updates=K, ms_per_update=round(dt * 1e3 / K, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024, help="envs of the synthetic rollout the loads read")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--update", action="store_true", help="also time one trainer epoch against Model.train")
    ap.add_argument("--update-envs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    bench_load(args)
    torch.cuda.empty_cache()
    if args.update:
        bench_update(args)


if __name__ == "__main__":
    main()
