"""The route of every rollout request (csrc: rollout_route): the kind a plan call returns and the text it
writes name the same thing, over the matrix of tools/dump_rollout_plans.py -- and the per-step route, which
the other rollout tests reach least, runs every policy through `rollout` and `rollout_perf`."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import mk_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_rollout_plans", os.path.join(ROOT, "tools", "dump_rollout_plans.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)

PICKS = {"descent": "descent_actions+", "pibt": "pibt_actions+"}
KEYS = ("status", "reward_total", "cost", "goals_reached", "shadow_goals", "constraints")
T = 3


def test_kind_and_text_agree_on_every_line():
    rows = list(dump.plan_rows())
    kinds = {}
    for config, tuning, entry, policy, slots, kind, text in rows:
        where = f"{config} {tuning} {entry} {policy} {slots}: {kind} {text!r}"
        kinds.setdefault(config, set()).add(kind)
        if kind == 1:
            assert text.startswith("rollout_random_kernel<"), where
        elif kind == 2:
            assert text.startswith("rollout_wide_kernel<") or text.startswith("rollout_wide3_kernel<"), where
        else:
            assert kind == 0 and "step" in text and "kernel" not in text, where
            for name, pick in PICKS.items():
                assert (pick in text) == (policy == name), where
    # the matrix reaches every route, each config on the one its name says
    for config, seen in kinds.items():
        assert seen == {{"pair": 1, "wide": 2, "steps": 0}[config.split("_")[0]]}, (config, seen)
    texts = {r[6].split(" ")[0].split("<")[0] for r in rows}
    assert {"rollout_random_kernel", "rollout_wide_kernel", "rollout_wide3_kernel"} <= texts, texts


def steps_twins():
    from mapf_amd.maps import keep_largest_component, random_map
    c = dump.CONFIGS["steps_b2_n16_k64"]
    world = keep_largest_component(random_map(np.random.default_rng(7), c["H"], c["W"], 0.2))
    envs = []
    for _ in range(2):
        e = mk_env(**c, human_mode="random", goal_mode="random", fix_choice=1, keep_bfs=True, seed=21)
        e.reset_seeded(world)
        envs.append(e)
    assert envs[0].rollout_kernel == 0
    return envs


@pytest.mark.parametrize("policy", dump.POLICIES)
def test_per_step_route_runs_every_policy(policy):
    from mapf_amd.env import perf_accumulate
    a, b = steps_twins()
    try:
        tape = torch.randint(0, 5, (T, a.B, a.N), dtype=torch.int32, device=a.device) if policy == "tape" else None
        out = {k: torch.full((T,) + tuple(a.out[k].shape), -7, dtype=a.out[k].dtype, device=a.device) for k in KEYS}
        obs = torch.empty((T,) + tuple(a.obs.shape), device=a.device)
        vec = torch.empty((T,) + tuple(a.vec.shape), device=a.device)
        acts = None if tape is not None else torch.full((T, a.B, a.N), -9, dtype=torch.int32, device=a.device)
        a.rollout(T, policy, slots=True, actions=acts, tape=tape, obs=obs, vec=vec, out=out)
        want = perf_accumulate(out)
        got_acts = None if tape is not None else torch.full((T, b.B, b.N), -9, dtype=torch.int32, device=b.device)
        got = b.rollout_perf(T, policy, tape=tape, actions=got_acts)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"{policy}: {got.cpu().numpy()} != {want.cpu().numpy()}"
        if acts is not None:
            assert torch.equal(got_acts, acts), policy
        sa, sb = a.get_state(), b.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{policy}: state {key}")
        # the same request without an actions buffer continues the record
        if tape is None:
            a.rollout(T, policy, slots=True, actions=acts, obs=obs, vec=vec, out=out)
            perf_accumulate(out, perf=want, accumulate=True)
            b.rollout_perf(T, policy, perf=got, accumulate=True)
            assert torch.equal(got, want), f"{policy}: continued"
    finally:
        a.close()
        b.close()
