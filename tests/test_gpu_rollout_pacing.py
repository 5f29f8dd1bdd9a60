"""GPU: the pacing of the grouped pair-lane rollout (roll_group 1, roll_slack >= 0; csrc/mapf_group.h:
arrival counters, pace_wait / pace_arrive -- the protocol itself is checked on the CPU in
tests/test_pace_protocol.py).

All 16 waves of a CU in one workgroup, paced within roll_slack steps of the slowest: one full group
(b64) and a group with envs past B (b61), slack 0 / 1 / 3, the random, tape and descent policies, slot
buffers with and without MAPF_SLOTS_BAND_CLEAN.  Two launches go back to back on one stream with no
synchronisation between them (the counters of launch 2 start clean), and every output of both is
bit-equal to the oracle and to the ungrouped form (roll_group 0) of the same two launches."""
import functools

import numpy as np
import pytest
import torch

from descent_ref import descent_actions
from oracle import oracle as O
from test_gpu_parity import assert_no_errors, mk_env
from test_gpu_rollout_band import OUT_KEYS, T, check_launch, fresh_buffers, host_skip, oracle_run, set_sentinels, setup

pytestmark = pytest.mark.gpu

NAMES = ["b64", "b61"]
POLICIES = ["random", "tape", "descent"]
PLAN = {"random": "rollout_plan", "tape": "rollout_actions_plan", "descent": "rollout_descent_plan"}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@functools.lru_cache(maxsize=None)
def descent_run(name):
    """The oracle's first 2 * T steps of the case under the descent policy (tests/descent_ref.py),
    computed once and shared (read-only), in oracle_run's layout."""
    case, maps, shared, seed = setup(name)
    B, n = case["B"], case["n"]
    cfg = O.make_config(case["H"], case["W"], n, case["fov"], case["nch"], use_da=case.get("da", 0),
                        use_hp=case.get("hp", 0), human_mode=1, goal_mode=1, fix_choice=1, seed=seed, env_offset=7)
    rows = []
    for b in range(B):
        oe = O.OracleEnv(cfg, env_id=7 + b)
        oe.reset_random(maps if shared else maps[b])
        steps = []
        for t in range(2 * T):
            a = descent_actions(oe.bfs(), oe.agents()[0], t)
            o = oe.step(a)
            oo, ov = oe.observe()
            steps.append(dict(actions=np.array(a), obs=oo, vec=ov, **{k: np.array(o[key]) for k, key in OUT_KEYS}))
        rows.append(steps)
    ref = {k: np.stack([np.stack([rows[b][t][k] for b in range(B)]) for t in range(2 * T)]) for k in rows[0][0]}
    for v in ref.values():
        v.setflags(write=False)
    return ref


def reference(name, policy):
    return descent_run(name) if policy == "descent" else oracle_run(name)


def launch(env, policy, roll, band):
    kw = dict(slots=True, band_clean=band, obs=roll["obs"], vec=roll["vec"], out=roll["out"])
    if policy == "random":
        env.rollout_random(T, actions=roll["actions"], **kw)
    elif policy == "tape":                  # roll["actions"] already holds the oracle's actions of launch k
        env.rollout_actions(roll["actions"], **kw)
    else:
        env.rollout_descent(T, actions=roll["actions"], **kw)


def two_launches(name, policy, band, tuning, expect):
    """Launch 1 (every float stored) and launch 2 (band: the band declared clean, over sentinels) into
    two sets of buffers, nothing between them on the stream; both checked against the oracle.
    Returns every buffer of both launches as raw bits."""
    case, maps, shared, seed = setup(name)
    ref = reference(name, policy)
    env = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared, seed=seed, env_offset=7,
                 tuning=tuning)
    try:
        env.reset_seeded(maps)
        plan = getattr(env, PLAN[policy])(slots=True, band_clean=band)
        assert plan.startswith(expect[0]) and expect[1] in plan, plan
        rolls = [fresh_buffers(env, case), fresh_buffers(env, case)]
        if band:
            set_sentinels(rolls[1])
        if policy == "tape":        # both tapes are in place before launch 1
            for k in (0, 1):
                rolls[k]["actions"].copy_(torch.from_numpy(np.ascontiguousarray(ref["actions"][k * T:(k + 1) * T]).astype(np.int32)))
        torch.cuda.synchronize()
        launch(env, policy, rolls[0], False)
        launch(env, policy, rolls[1], band)
        check_launch(name, ref, 0, rolls[0])
        check_launch(name, ref, 1, rolls[1], host_skip(env, case, rolls[1], True) if band else None)
        assert_no_errors(env, allow=(1, 2) if policy == "descent" else ())
        bits = {}
        for k, roll in enumerate(rolls):
            for key, v in dict(actions=roll["actions"], obs=roll["obs"], vec=roll["vec"], **roll["out"]).items():
                bits[(k, key)] = v.cpu().numpy().view(np.uint8).copy()
        return bits
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def ungrouped(name, policy, band):
    return two_launches(name, policy, band, dict(roll_occ=4, roll_group=0), ("rollout_random_kernel<true,1", " block=256 "))


@pytest.mark.parametrize("band", [False, True], ids=["full", "band"])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("slack", [0, 1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_paced_group_equals_oracle_and_ungrouped(name, slack, policy, band):
    got = two_launches(name, policy, band, dict(roll_occ=4, roll_group=1, roll_slack=slack),
                       ("rollout_random_kernel<true,4", " slack=%d " % slack))
    want = ungrouped(name, policy, band)
    assert set(got) == set(want)
    for key in sorted(got):
        assert np.array_equal(got[key], want[key]), (name, slack, policy, band, key)
