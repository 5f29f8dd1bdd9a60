"""Every rollout plan of a small matrix of handles, one line each: what the C plan calls return (the kind:
0 per-step launches, 1 the pair-lane kernel, 2 one wave per env) and the text they write.

    config | tuning | entry point | policy | slots | kind | text

The matrix reaches every route: the pair-lane kernel grouped (roll_occ=4) and ungrouped, the wide kernel
over u32 and u64 rows, with the BFS channel, in its three-, two- and one-wave forms, and a handle no
one-launch kernel covers; every policy; every `slots` value of the observing entry points; the sparse plan
over a 64-byte-aligned buffer and over one 16 bytes further; the perf plan; PIBT with a human weight and
horizon set.  The calls go through ctypes because the Python wrappers drop the kind.  The library is the one
MAPF_LIB names (mapf_amd/_lib.py), so two builds can be compared line by line:

    MAPF_LIB=/path/to/other/libmapf.so python tools/dump_rollout_plans.py > other.txt
    python tools/dump_rollout_plans.py > this.txt && diff other.txt this.txt
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "primal-ppo_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = {
    "pair_b16_n8": dict(B=16, H=10, W=10, num_agents=8, fov=3, num_channel=6),
    "wide_b2_n16": dict(B=2, H=12, W=12, num_agents=16, fov=5, num_channel=6),
    "wide_b2_n8_c7": dict(B=2, H=12, W=12, num_agents=8, fov=5, num_channel=7),
    "wide_b2_n4_w40": dict(B=2, H=12, W=40, num_agents=4, fov=5, num_channel=6),
    "steps_b2_n16_k64": dict(B=2, H=12, W=12, num_agents=16, fov=5, num_channel=6, use_hp=1, k_predict=64),
}
TUNINGS = ("", "roll_group=0", "roll_occ=4", "wide_obs=1", "wide_pipe=0")
POLICIES = ("random", "tape", "descent", "pibt")
SLOTS = {"0": 0, "slots": 1, "slots|band_clean": 3, "bits": 4, "slots|bits": 5}
PLAN_CALLS = {"random": "mapf_rollout_plan", "tape": "mapf_rollout_actions_plan",
              "descent": "mapf_rollout_descent_plan", "pibt": "mapf_rollout_pibt_plan"}


def make_env(name):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    kw = dict(CONFIGS[name])
    B, H, W = kw.pop("B"), kw.pop("H"), kw.pop("W")
    return BatchedMapfGym(make_config(B, H, W, human_mode="random", goal_mode="random", fix_choice=1, keep_bfs=True,
                                      seed=5, **kw))


def handle_rows(env, config, tuning):
    """(config, tuning, entry, policy, slots, kind, text) of every plan call on one handle as it is tuned now."""
    import torch
    from mapf_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(512)
    base = torch.empty(64, dtype=torch.float32, device=env.device).data_ptr()
    assert base % 64 == 0

    def row(entry, policy, slots, kind):
        return (config, tuning or "default", entry, policy, slots, int(kind), buf.value.decode())

    for k, policy in enumerate(POLICIES):
        for label, bits in SLOTS.items():
            yield row(PLAN_CALLS[policy], policy, label, getattr(L, PLAN_CALLS[policy])(env.h, bits, buf, 512))
        for label, address in (("aligned", base), ("offset16", base + 16)):
            yield row("mapf_rollout_sparse_plan", policy, label, L.mapf_rollout_sparse_plan(env.h, k, address, buf, 512))
        yield row("mapf_rollout_perf_plan", policy, "-", L.mapf_rollout_perf_plan(env.h, k, buf, 512))


def plan_rows():
    from mapf_amd.env import parse_tuning
    for config in CONFIGS:
        env = make_env(config)
        try:
            default = env.tuning()
            for tuning in TUNINGS:
                env.set_tuning(**dict(default, **parse_tuning(tuning)))
                yield from handle_rows(env, config, tuning)
            env.set_tuning(**default)
            env.set_pibt_human_weight(2)
            env.set_pibt_human_horizon(3)
            for r in handle_rows(env, config, "default human_weight=2 human_horizon=3"):
                if r[3] == "pibt":
                    yield r
        finally:
            env.close()


if __name__ == "__main__":
    for r in plan_rows():
        print(" | ".join(str(x) for x in r))
