"""GPU: the one-wave form of the observation's phases 1-3 in the pair-lane rollout kernels (mapf_observe.h:
obs_wave_occ, obs_wave_rows) and what came with it: the map rows copied to LDS once per launch, the slot
offset added in the step's storing lanes.

In that form lane l works for agent l >> 3 on the FOV rows (l & 7) and (l & 7) + 8; the agent's head lane
sets the occupancy bit, the own-goal, human and path bits and stores the vector.  The shapes, all on a
10 x 10 warehouse with 6 channels (at FOV 11 every window clips the map's edge on all four sides):

    F = 11, N in 1, 2, 3, 5, 7, 8   more rows than eight: a second row on lanes 0..2 of every agent; N no
                                    power of two: idle agent groups of eight lanes (where the plan sends a
                                    small N to another kernel, that kernel's form must agree all the same)
    F in 3, 5, 7, 9, N in 8, 5      one row per lane, idle row lanes
    N = 6, F in 3, 7, 11            the N that is no power of two and still runs one wave per env (an odd N
                                    has no whole float4s per env at 6 channels and goes to another kernel)
    B = 5                           four envs per workgroup, a ragged last workgroup
    B = 13, roll_occ=4 roll_group=1 sixteen envs per workgroup, a ragged last quarter
    da, hp, da + hp at N = 8 F = 11 the danger disc and the human's path cells (branches the default
                                    workload never runs)

Every case runs T = 6 steps per launch against the CPU oracle, bit for bit (obs, vec, every step output,
the drawn actions): three calls of the default slots launcher over NaN-filled buffers (calls 2 and 3 take
the sparse form where it applies: N = 8) and one launch in place.  Policies: random and tape on every
shape, descent and PIBT on two pair-lane shapes each."""
import functools

import numpy as np
import pytest
import torch

import pibt_ref
import rollout_harness as H
from descent_ref import descent_actions
from test_gpu_parity import assert_no_errors, host

pytestmark = pytest.mark.gpu

T = 6
LAUNCHES = 3
SEED = 0x0B5E0000
GROUPED = dict(roll_occ=4, roll_group=1)


def shape(n, fov, B=5, **kw):
    return dict(B=B, H=10, W=10, n=n, fov=fov, nch=6, map="wh", **kw)


CASES = {f"n{n}_f11": shape(n, 11) for n in (1, 2, 3, 5, 7, 8)}
CASES.update({f"n{n}_f{f}": shape(n, f) for n in (8, 5) for f in (3, 5, 7, 9)})
CASES.update({f"n6_f{f}": shape(6, f) for f in (3, 7, 11)})
CASES["n8_f11_b13"] = shape(8, 11, B=13)
CASES["n8_f11_da"] = shape(8, 11, da=1)
CASES["n8_f11_hp"] = shape(8, 11, hp=1)
CASES["n8_f11_dahp"] = shape(8, 11, da=1, hp=1)
TUNING = {"n8_f11_b13": GROUPED}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@functools.lru_cache(maxsize=None)
def oracle_run(name, policy):
    """(tape, ref): the oracle's first LAUNCHES * T steps of the case under `policy`, computed once and
    shared (read-only); tape: the host tape of policy "tape", else None."""
    case = CASES[name]
    steps = LAUNCHES * T
    tape = None
    if policy == "random":
        pick = lambda oe, b, t, world: (np.array(oe.random_actions()), None)
    elif policy == "tape":
        tape = np.random.default_rng(len(name)).integers(0, 5, (steps, case["B"], case["n"])).astype(np.int32)
        tape.setflags(write=False)
        pick = lambda oe, b, t, world: (tape[t, b], None)
    elif policy == "descent":
        pick = lambda oe, b, t, world: (descent_actions(oe.bfs(), oe.agents()[0], t), None)
    else:
        ages = [pibt_ref.Ages(case["n"]) for _ in range(case["B"])]

        def pick(oe, b, t, world):
            pos, goal = oe.agents()
            hum = oe.human()
            return pibt_ref.pibt_actions(np.asarray(world, np.int8), oe.bfs(), pos, goal, hum["pos"], hum["next"], t,
                                         ages[b])[0], None
    return tape, H.oracle_rollout(CASES, name, SEED, steps, set(), pick)[0]


def buffers(env, k):
    return dict(H.slot_buffers(env, k), actions=H.action_buffer(env, k))


def check(what, ref, k, roll, policy, in_place=False):
    slots = [(0, T - 1)] if in_place else [(q, q) for q in range(T)]
    H.check_slots(what, ref, k * T, host(roll["out"]), roll["obs"], roll["vec"], slots)
    if policy != "tape":
        H.check_actions(what, ref, k * T, roll["actions"], slots)


def run_case(name, policy):
    tape, ref = oracle_run(name, policy)
    tuning = TUNING.get(name)
    case = CASES[name]
    dev_tape = lambda env, k: None if tape is None else torch.from_numpy(tape[k * T:(k + 1) * T].copy()).to(env.device)

    # the slots launcher, three calls with no writes in between
    env = H.case_env(CASES, name, SEED, tuning)[0]
    try:
        kname = env.rollout_kernel_name(slots=True, policy=policy)
        # Which cases run the pair-lane kernel (one wave per env), stated per case so that a change of the
        # routing cannot empty the coverage: N = 6 and 8.  An odd N has no whole float4s per env with 6
        # channels and an odd F (fused_per_wave), N <= 4 takes the smaller pair grids: other kernels.
        pairs = case["n"] in (6, 8)
        print(f"{name} {policy}: {kname}")
        assert kname.startswith("rollout_random_kernel<true,%d" % (4 if tuning else 1)) == pairs, kname
        roll = buffers(env, T)
        tape_in = dev_tape(env, 0)
        kw = dict(actions_in=tape_in) if policy == "tape" else dict(policy=policy, actions=roll["actions"])
        launch = env.rollout_launcher(T, slots=True, obs=roll["obs"], vec=roll["vec"], out=roll["out"], **kw)
        if pairs:
            assert (getattr(launch, "sparse", None) is not None) == (case["n"] == 8), name
        for call in range(LAUNCHES):
            if call and tape_in is not None:
                tape_in.copy_(dev_tape(env, call))
            launch()
            check(f"{name} {policy} launcher call {call}", ref, call, roll, policy)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()

    # in place
    env = H.case_env(CASES, name, SEED, tuning)[0]
    try:
        kname = env.rollout_kernel_name(slots=False, policy=policy)
        assert kname.startswith("rollout_random_kernel<false,%d" % (4 if tuning else 1)) == (case["n"] in (6, 8)), kname
        roll = buffers(env, 1)
        env.rollout(T, policy, slots=False, tape=dev_tape(env, 0), **roll)
        check(f"{name} {policy} in place", ref, 0, roll, policy, in_place=True)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()


@pytest.mark.parametrize("policy", ["random", "tape"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_wave_observation_against_the_oracle(name, policy):
    run_case(name, policy)


@pytest.mark.parametrize("policy,name", [("descent", "n6_f11"), ("descent", "n8_f11_b13"), ("pibt", "n8_f11"), ("pibt", "n6_f7")])
def test_planner_policies_share_the_include(policy, name):
    """Shapes that run the pair-lane kernel (asserted by name in run_case): descent's instantiation of the
    one-wave path, PIBT's kernels, which keep the workgroup form and the map rows' copy per step."""
    assert CASES[name]["n"] in (6, 8)
    run_case(name, policy)
