"""GPU: the one-wave observation store loop of the rollout kernels (mapf_observe.h: obs_store_wave_nt).

A wave stores its env's slice of q = N * C * F * F / 4 float4s, lane l float4 l + 64k at iteration k, in
groups of four iterations with one last partial group; the lanes past q in the last iteration are cut by
the range check of the slice's buffer descriptor.  The shapes below put q on every boundary of that loop:

    N=8 F=3   q = 108    1 whole iteration + 44 lanes: less than one group
    N=8 F=5   q = 300    4 whole iterations (exactly one group) + 44 lanes
    N=8 F=7   q = 588    9 whole iterations + 12 lanes
    N=8 F=11  q = 1452   22 whole iterations + 44 lanes (c2's row count)
    N=6 F=11  q = 1089   17 whole iterations + 1 lane; 4356 floats are no whole 64-B pieces: the band form
    N=6 F=7   q = 441    6 whole iterations + 57 lanes; the band form, grouped, its mask moving with the slot
    N=7 F=3   378 floats, no whole float4s: the route that does not use the table loop at all

Every shape runs, against the CPU oracle and bit for bit (obs, vec, every step output, the drawn actions),
T = 6 steps per launch into NaN-filled buffers: a slots launch that stores everything; a slots launch that
declares the zero band clean (sentinels survive exactly where the host's skip bitmap says); three calls of
the default slots launcher (the sparse form where it applies, calls 2 and 3 leaving out stores); one launch
in place.  Every observation buffer has one spare trailing slot of sentinels that must stay untouched.
B = 5 and B = 37 run four envs per workgroup (B = 37: a ragged last workgroup and a band mask that moves
with the slot where the slot stride is no multiple of 64 B); the grouped form (16 envs per workgroup) needs
ceil(B / 4) % 4 == 0, so it runs at B = 13, the smallest such B with a ragged last quarter.  With N = 8 a
slot is always a multiple of 64 B; the grouped form meets a band mask that moves with the slot at N = 6
(B = 13 and 61 at F = 11, B = 13 at F = 7: q = 441, 6 whole iterations + 57 lanes)."""
import ctypes
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
LAUNCHES = 3                                 # launches of T steps the oracle runs ahead
SENTINEL = 7.0
SEED = 0x570E0000
GROUPED = dict(roll_occ=4, roll_group=1)


def pair(n, fov, B):
    return dict(B=B, H=10, W=10, n=n, fov=fov, nch=6, map="wh")


SHAPES = {"n8_f3": (8, 3), "n8_f5": (8, 5), "n8_f7": (8, 7), "n8_f11": (8, 11), "n6_f11": (6, 11), "n6_f7": (6, 7),
          "n7_f3": (7, 3)}
CASES = {f"{s}_b{B}": pair(n, f, B) for s, (n, f) in SHAPES.items() for B in (5, 13, 37, 61)}
CASES["c4_form_b3"] = dict(B=3, H=40, W=40, n=16, fov=9, nch=6, map="wh", human="looping")
CASES["c5_form_b2"] = dict(B=2, H=80, W=80, n=64, fov=11, nch=7, map="rand")


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
    """Buffers of k slots, NaN-filled; `obs` is the first k slots of k + 1, the last one sentinels."""
    buf = H.slot_buffers(env, k)
    spare = torch.full((k + 1,) + tuple(env.obs.shape), float("nan"), device=env.device)
    spare[k] = SENTINEL
    return dict(buf, obs=spare[:k], actions=H.action_buffer(env, k)), spare


def assert_spare_untouched(what, spare):
    assert bool((spare[-1] == SENTINEL).all()), f"{what}: stores past the last slot's slice"


def band_skip(env, case, obs):
    """bool [T, B, N*C*F*F]: the floats a band-clean pair-lane launch into `obs` leaves alone (the host side
    of the kernel's own skip function at every slot's and env's address); empty where there are none."""
    from mapf_amd import _lib
    B, n, nch, fov = case["B"], case["n"], case["nch"], case["fov"]
    fl = n * nch * fov * fov
    skip = np.zeros((T, B, fl), bool)
    by_off = {}
    for t in range(T):
        for b in range(B):
            off = (obs.data_ptr() + (t * B + b) * fl * 4) % 128
            if off not in by_off:
                bits = np.zeros(fl // 4, np.uint8)
                assert _lib.lib().mapf_obs_band_skip(ctypes.byref(env.cfg), 0, off, bits.ctypes.data, len(bits)) == len(bits)
                by_off[off] = np.repeat(bits.astype(bool), 4)
            skip[t, b] = by_off[off]
    return skip


def check(what, ref, k, roll, policy, in_place=False, kept=None):
    """Launch k's buffers against the oracle's steps [k*T, (k+1)*T) (in place: the last of them); kept:
    bool, the floats of `obs` that hold SENTINEL instead."""
    slots = [(0, T - 1)] if in_place else [(q, q) for q in range(T)]
    obs = roll["obs"]
    if kept is not None:
        got = obs.cpu().numpy()
        assert (got.reshape(kept.shape)[kept] == SENTINEL).all(), f"{what}: a skipped float was stored"
        want = ref["obs"][k * T:(k + 1) * T].astype(np.float32).reshape(got.shape)
        obs = torch.from_numpy(np.where(kept.reshape(got.shape), want, got))
    H.check_slots(what, ref, k * T, host(roll["out"]), obs, roll["vec"], slots)
    if policy != "tape":
        H.check_actions(what, ref, k * T, roll["actions"], slots)


def run_case(name, policy="random", tuning=None, subs=None, sparse=None):
    """subs: the pair-lane kernel's envs-per-workgroup quarter count to expect (None: another kernel);
    sparse: whether the launcher's later calls must take the sparse form (None: not the pair-lane kernel)."""
    tape, ref = oracle_run(name, policy)
    dev_tape = lambda env, k: None if tape is None else torch.from_numpy(tape[k * T:(k + 1) * T].copy()).to(env.device)
    tag = "" if policy == "random" else "," + policy

    # 1. slots: everything stored, then the band declared clean
    env, case = H.case_env(CASES, name, SEED, tuning)[:2]
    try:
        if subs is not None:
            assert env.rollout_kernel_name(slots=True, policy=policy) == "rollout_random_kernel<true,%d%s>" % (subs, tag)
        roll, spare = buffers(env, T)
        env.rollout(T, policy, slots=True, tape=dev_tape(env, 0), **roll)
        check(f"{name} slots", ref, 0, roll, policy)
        assert_spare_untouched(f"{name} slots", spare)
        roll["obs"].fill_(float("nan"))
        roll["obs"][:, :, :, 5] = SENTINEL
        banded = "band64" in env.rollout_plan(slots=True, band_clean=True, policy=policy)
        assert banded == (subs is not None), env.rollout_plan(slots=True, band_clean=True, policy=policy)
        env.rollout(T, policy, slots=True, band_clean=True, tape=dev_tape(env, 1), **roll)
        kept = band_skip(env, case, roll["obs"]) if banded else None
        if kept is not None and case["fov"] >= 5:       # a band of F * F * 4 >= 100 B holds a whole 64-B piece
            assert kept.any()
        check(f"{name} band-clean", ref, 1, roll, policy, kept=kept)
        assert_spare_untouched(f"{name} band-clean", spare)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()

    # 2. the slots launcher, three calls with no writes in between
    env = H.case_env(CASES, name, SEED, tuning)[0]
    try:
        roll, spare = buffers(env, T)
        tape_in = dev_tape(env, 0)
        kw = dict(actions_in=tape_in) if policy == "tape" else dict(policy=policy, actions=roll["actions"])
        launch = env.rollout_launcher(T, slots=True, obs=roll["obs"], vec=roll["vec"], out=roll["out"], **kw)
        if sparse is not None:
            form = env.rollout_sparse_plan(roll["obs"], policy).split(" ")[0]
            assert form == "rollout_random_kernel<true,%d,%s%s>" % (subs, "sparse64" if sparse else "band64", tag), form
            assert (getattr(launch, "sparse", None) is not None) == sparse
        for call in range(LAUNCHES):
            if call and tape_in is not None:
                tape_in.copy_(dev_tape(env, call))
            launch()
            check(f"{name} launcher call {call}", ref, call, roll, policy)
            assert_spare_untouched(f"{name} launcher call {call}", spare)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()

    # 3. in place
    env = H.case_env(CASES, name, SEED, tuning)[0]
    try:
        if subs is not None:
            assert env.rollout_kernel_name(slots=False, policy=policy) == "rollout_random_kernel<false,%d%s>" % (subs, tag)
        roll, spare = buffers(env, 1)
        env.rollout(T, policy, slots=False, tape=dev_tape(env, 0), **roll)
        check(f"{name} in place", ref, 0, roll, policy, in_place=True)
        assert_spare_untouched(f"{name} in place", spare)
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()


@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("shape", ["n8_f3", "n8_f5", "n8_f7", "n8_f11"])
def test_every_loop_boundary_four_envs_per_workgroup(shape, B):
    run_case(f"{shape}_b{B}", subs=1, sparse=True)


@pytest.mark.parametrize("shape", ["n8_f3", "n8_f5", "n8_f7", "n8_f11"])
def test_every_loop_boundary_grouped(shape):
    run_case(f"{shape}_b13", tuning=GROUPED, subs=4, sparse=True)


@pytest.mark.parametrize("B,tuning,subs", [(5, None, 1), (37, None, 1), (13, GROUPED, 4), (61, GROUPED, 4)])
def test_one_lane_tail_takes_the_band_form(B, tuning, subs):
    """N = 6, F = 11: 1089 float4s, the last iteration stores one lane's; no whole pieces, so no sparse form."""
    run_case(f"n6_f11_b{B}", tuning=tuning, subs=subs, sparse=False)


def test_grouped_form_with_a_band_mask_that_moves_with_the_slot():
    """N = 6, F = 7, B = 13: a slot is 91,728 B, no multiple of 64, under 16 envs per workgroup."""
    assert (13 * 6 * 6 * 7 * 7 * 4) % 64 != 0
    run_case("n6_f7_b13", tuning=GROUPED, subs=4, sparse=False)


@pytest.mark.parametrize("B", [5, 37])
def test_slices_that_are_no_whole_float4s_take_another_route(B):
    """N = 7, F = 3: 378 floats per env."""
    name = f"n7_f3_b{B}"
    env = H.case_env(CASES, name, SEED)[0]
    try:
        assert not env.rollout_kernel_name(slots=True).startswith("rollout_random_kernel")
    finally:
        env.close()
    run_case(name)


@pytest.mark.parametrize("policy", ["tape", "descent", "pibt"])
def test_other_policies_one_group_and_a_tail(policy):
    run_case("n8_f5_b5", policy=policy, subs=1, sparse=True)


@pytest.mark.parametrize("name,kernel", [("c4_form_b3", "rollout_wide3_kernel<u64,1,true>"),
                                         ("c5_form_b2", "rollout_wide_kernel<Row2,2,true>")])
def test_wide_kernels(name, kernel):
    env = H.case_env(CASES, name, SEED)[0]
    try:
        assert env.rollout_kernel_name(slots=True) == kernel
    finally:
        env.close()
    run_case(name)
