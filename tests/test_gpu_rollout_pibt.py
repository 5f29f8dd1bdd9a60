"""GPU: persistent rollouts under the PIBT policy (mapf_rollout_pibt, mapf_pibt_actions; include/mapf.h).

The rollout kernels' PIBT forms pick every env's actions in the stepping wave: candidates from the
agents' tiled BFS maps, the solve by readlanes and ballots (lane = agent in the one-wave-per-env
kernels, the agents' head lanes in the pair-lane kernel), the ages in registers.
The oracle has no policy: tests/pibt_ref.py restates it in numpy over OracleEnv.bfs(), .agents() and
.human(), the oracle is stepped with the result, and every slot is compared bit for bit -- chosen
actions, all step outputs, observations, vectors, and the state and BFS maps after every launch.

Conditions on the inputs, asserted from the reference run alone before any device call: per case at
least 20 goal changes, 10 of them before the last step of their launch, and at least 50 inheritance
calls; per kernel family (pair-lane, wide) at least 10 backtracks and 5 failed picks across its cases.
The pair-lane family has a dense shape of its own among them (8 agents on a shared 8 x 8 map with few
obstacles).

The file ends with a guard: the PIBT kernel every BASELINE preset launches by default, into slots and
in place, has been run by an oracle-compared case above (tests/kernel_registry.py).
"""
import functools

import numpy as np
import pytest
import torch

import pibt_ref
import rollout_harness as H
from descent_ref import descent_actions
from oracle import oracle as O
from rollout_harness import check_actions, check_slots, check_state, slot_buffers
from test_gpu_parity import FUSED_CASES, GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, WIDE_SHAPES, host

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 23, 40)                       # steps per launch, in this order: 64 steps
PIBT_COVERED = set()                         # kernel names this file compared against the oracle
DENSE = "p_n8_8x8_f5_dense"                  # this file's own shape: 8 agents, shared 8 x 8 map, few obstacles
CASES = {**FUSED_CASES, **GROUP_CASES, **ROLLOUT_CASES, **RANDOM_CASES, **WIDE_SHAPES,
         DENSE: dict(B=24, H=8, W=8, n=8, fov=5, nch=6, map="sparse_shared", map_seed=2)}
SEED = 0x91B70000
covered = functools.partial(H.covered, "pibt", PIBT_COVERED)
SMALL = ["r_n6_16x16_f9_dahp", "g_n8_20x20_f11_ragged61", "g_n8_20x20_f11", "r_n6_12x12_f7_dense", DENSE]
WIDE = ["c4_40x40_n16_f9_looping", "dense_12x12_n16_f9_dahp", "c1_10x10_n4_f11", "c5_80x80_n64_f11_bfsch",
        "w_n20_48x90_f11_bfsch"]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def case_setup(name):
    return H.case_setup(CASES, name, SEED)


def case_env(name, tuning=None, **kw):
    return H.case_env(CASES, name, SEED, tuning, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(name, steps=int(np.sum(LAUNCHES))):
    """The oracle under the restated policy, computed once and shared (read-only): the actions,
    per-step outputs / observations / vectors [steps, B, ...], the state (cells, goals, human, BFS maps,
    the oracle's error count) after every launch of every path, and what the policy did: per step and
    env the failed picks standing on the human's next cell, and the run's inheritance calls,
    backtracks and failed picks."""
    n = CASES[name]["n"]
    ages = [pibt_ref.Ages(n) for _ in range(CASES[name]["B"])]
    stats = dict(inherit=0, backtracks=0, failed=0)

    def pick(oe, b, t, world):
        pos, goal = oe.agents()
        hum = oe.human()
        a, failed, st = pibt_ref.pibt_actions(np.asarray(world, np.int8), oe.bfs(), pos, goal, hum["pos"], hum["next"], t, ages[b])
        stats["inherit"] += st["inherit"]
        stats["backtracks"] += st["backtracks"]
        stats["failed"] += len(failed)
        hit = np.zeros(n, bool)
        for i in failed:
            hit[i] = tuple(pos[i]) == tuple(hum["next"])
        return a, dict(may_hit=hit)
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 41)) | {steps}
    return H.oracle_rollout(CASES, name, SEED, steps, bounds, pick) + (stats,)


def assert_inputs(name, launches=LAUNCHES):
    """The per-case conditions: goal changes (a stale map or age can only show there) and inheritance."""
    ref, _, stats = oracle_run(name)
    H.assert_goals_change(name, ref, launches)
    print(f"{name}: {stats}")
    assert stats["inherit"] >= 50, (name, stats)
    return ref


def assert_consequences(what, ref, t0, got, acts, which):
    """The header's consequences on the DEVICE outputs: no -1 and no -3; -2 only where the reference's
    pick failed on the human's next cell; actions_fixed == actions in an env-step without a -2."""
    a = acts.cpu().numpy()
    for k, dt in which:
        st = got["status"][k]
        assert not ((st == -1) | (st == -3)).any(), f"{what} t={t0 + dt}: status {np.unique(st)}"
        assert not ((st == -2) & ~ref["may_hit"][t0 + dt]).any(), f"{what} t={t0 + dt}: a -2 without a failed pick on hn"
        clean = ~(st == -2).any(axis=1)
        assert np.array_equal(got["actions_fixed"][k][clean], a[k][clean]), f"{what} t={t0 + dt}: fixActions rewrote a pick"


@pytest.mark.parametrize("family,names", [("pair-lane", SMALL), ("wide", WIDE)])
def test_inputs_exercise_backtracking_and_failed_picks(family, names):
    """Per family, from the reference runs alone (no device call): >= 10 backtracks, >= 5 failed picks."""
    tot = dict(inherit=0, backtracks=0, failed=0)
    for name in names:
        assert_inputs(name)
        for k, v in oracle_run(name)[2].items():
            tot[k] += v
    print(family, tot)
    assert tot["backtracks"] >= 10 and tot["failed"] >= 5, (family, tot)


def run_pibt_case(name, path, tuning=None, launches=LAUNCHES, expect=None):
    ref = assert_inputs(name, launches)
    t0 = H.run_policy_case("pibt", case_env, PIBT_COVERED, name, path, ref, oracle_run(name)[1], launches, tuning, expect,
                           allow=(), hook=assert_consequences)       # PIBT leaves fixActions nothing it cannot place
    assert int(np.sum(launches)) >= t0


# ------------------------------------------------------------------ 1. the pair-lane kernel
PAIR_CASES = [("r_n6_16x16_f9_dahp", None, "1"),                                            # B = 37: ragged
              ("g_n8_20x20_f11_ragged61", dict(roll_occ=4, roll_group=1, roll_slack=1), "4"),  # grouped, paced
              ("g_n8_20x20_f11", dict(roll_occ=4, roll_fair=4), "4"),                       # grouped, fair
              ("r_n6_12x12_f7_dense", None, "1"),
              (DENSE, None, "1")]


@pytest.mark.parametrize("path", ["rollout", "inplace1", "inplace"])
@pytest.mark.parametrize("name,tuning,subs", PAIR_CASES)
def test_pair_lane_pibt_matches_oracle(name, tuning, subs, path):
    """Agents on head lanes, the solve over them, the picks through the LDS row: ungrouped, grouped
    and paced, grouped and fair."""
    expect = "rollout_random_kernel<%s,%s,pibt>" % ("true" if path == "rollout" else "false", subs)
    run_pibt_case(name, path, tuning, expect=expect)


# ------------------------------------------------------------------ 2. the wide shapes
WIDE_CASES = [("c4_40x40_n16_f9_looping", None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>"),
              ("c4_40x40_n16_f9_looping", None, "inplace", "rollout_wide3_kernel<u64,1,false,pibt>"),
              ("c4_40x40_n16_f9_looping", dict(wide_obs=1), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),
              ("c4_40x40_n16_f9_looping", dict(wide_pipe=0), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),
              ("dense_12x12_n16_f9_dahp", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "inplace", None),
              ("c1_10x10_n4_f11", None, "inplace1", None),
              ("c5_80x80_n64_f11_bfsch", None, "rollout", "rollout_wide_kernel<Row2,2,true,pibt>"),
              ("w_n20_48x90_f11_bfsch", None, "rollout", None)]


@pytest.mark.parametrize("name,tuning,path,expect", WIDE_CASES)
def test_wide_pibt_matches_oracle(name, tuning, path, expect):
    """Three waves per env (c4's form, the stepper searching: bfsobs=0), two (wide_obs 1), one
    (wide_pipe 0; c5's Row2 form at B = 3, 64 agents: every lane an agent), u32 / u64 / 128-bit
    search rows, the BFS channel."""
    run_pibt_case(name, path, tuning, expect=expect)


# ------------------------------------------------------------------ 3. per-step picks, and the ages across the forms
@pytest.mark.parametrize("name", [DENSE, "dense_12x12_n16_f9_dahp"])
def test_pibt_actions_then_step_observe_matches_oracle(name):
    """The per-step entry point: T x (pibt_actions, step_observe) against the oracle (so it equals
    the one-launch form, compared above); a second pick at the same clock changes nothing."""
    T = 24
    ref, state, _ = oracle_run(name)
    env, case, _, _, _ = case_env(name)
    try:
        for t in range(T):
            acts = env.pibt_actions()
            assert np.array_equal(acts.cpu().numpy(), ref["actions"][t]), f"t={t}: actions"
            if t % 5 == 0:
                again = env.pibt_actions(torch.full_like(acts, -9))
                assert torch.equal(again, acts), f"t={t}: the second pick at one clock"
            out, obs, vec = env.step_observe(acts)
            check_slots(f"{name} per step", ref, t, {k: v[None] for k, v in host(out).items()}, obs[None], vec[None], [(0, 0)])
        check_state(env, state[T], name)
    finally:
        env.close()


@pytest.mark.parametrize("name", [DENSE, "c4_40x40_n16_f9_looping"])
def test_per_step_picks_continue_a_one_launch_rollout_and_back(name):
    """The age arrays are current at launch end: 24 steps in one launch, 8 per-step picks, 8 more in one
    launch -- the actions of all 40 steps equal the oracle's."""
    ref, state, _ = oracle_run(name)
    env, case, _, _, _ = case_env(name)
    try:
        assert env.rollout_fused
        buf = slot_buffers(env, 24)
        acts = torch.full((24, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        env.rollout_pibt(24, slots=True, actions=acts, **buf)
        check_actions("launch 1", ref, 0, acts, [(q, q) for q in range(24)])
        for t in range(24, 32):
            a = env.pibt_actions()
            assert np.array_equal(a.cpu().numpy(), ref["actions"][t]), f"t={t}: per-step pick after the launch"
            env.step_observe(a)
        env.rollout_pibt(8, slots=True, actions=acts[:8], **slot_buffers(env, 8))
        check_actions("launch 2", ref, 32, acts, [(q, q) for q in range(8)])
        check_state(env, state[40], name)
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def late_start_reference(name, idle, steps):
    """The oracle from its reset: `idle` steps of the descent policy, then `steps` PIBT picks with FRESH
    ages -- what a handle must play whose ages restarted at the reset.  Also the agents whose goal is
    still that of clock 0, and how many of the picks differ when the ages are instead the stale pairs
    (seen = the goal of clock 0, since = 0) a handle that did not restart them would hold."""
    case, maps, shared, seed = case_setup(name)
    cfg = O.make_config(case["H"], case["W"], case["n"], case["fov"], case["nch"], use_da=case.get("da", 0),
                        use_hp=case.get("hp", 0), human_mode=1, goal_mode=1, fix_choice=1, seed=seed, env_offset=7)
    acts, aged, differ = [], 0, 0
    for b in range(case["B"]):
        oe = O.OracleEnv(cfg, env_id=7 + b)
        world = np.asarray(maps if shared else maps[b], np.int8)
        oe.reset_random(world)
        g0 = oe.agents()[1].copy()
        for t in range(idle):
            oe.step(descent_actions(oe.bfs(), oe.agents()[0], t))
        aged += int((oe.agents()[1] == g0).all(axis=1).sum())
        ages, stale = pibt_ref.Ages(case["n"]), pibt_ref.Ages(case["n"])
        stale.update(g0, 0)
        row = []
        for t in range(idle, idle + steps):
            pos, goal = oe.agents()
            hum = oe.human()
            a, _, _ = pibt_ref.pibt_actions(world, oe.bfs(), pos, goal, hum["pos"], hum["next"], t, ages)
            if t == idle:
                differ += int((pibt_ref.pibt_actions(world, oe.bfs(), pos, goal, hum["pos"], hum["next"], t, stale)[0] != a).sum())
            oe.step(a)
            row.append(a)
        acts.append(np.stack(row))
    return np.stack(acts, 1), aged, differ


@pytest.mark.parametrize("how", ["reset", "set_state"])
def test_a_reset_or_a_restored_state_restarts_the_ages(how):
    """A pick at clock 0 leaves (seen = the first goal, since = 0) in the handle.  After a reset to the
    same start -- or a set_state -- and 8 steps of the descent policy, an agent still on its first goal
    would pick at clock 8 with age 8 from the stale pair where the restarted ages say 0: the 12 picks
    from there equal the reference's with fresh ages only if the handle restarted them (the reference
    itself says that the stale pairs change the very first of them)."""
    idle, steps = 8, 12
    want, aged, differ = late_start_reference(DENSE, idle, steps)
    print(f"{aged} agents still on their first goal, {differ} first picks differ under stale ages")
    assert aged >= 20 and differ >= 5, (aged, differ)
    env, case, maps, _, _ = case_env(DENSE)
    try:
        if how == "reset":
            env.rollout_pibt(1)                                    # an earlier episode: ages set at clock 0
            env.reset_seeded(maps)
            env.rollout_descent(idle)
        else:
            env.pibt_actions()                                     # ages set at clock 0, nothing stepped
            env.rollout_descent(idle)
            env.set_state(clock=env.get_state()["clock"])
        acts = torch.full((steps, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        env.rollout_pibt(steps, slots=True, actions=acts, **slot_buffers(env, steps))
        assert np.array_equal(acts.cpu().numpy(), want), "picks after the restart"
    finally:
        env.close()


def test_rollout_pibt_without_a_one_launch_form_equals_the_oracle():
    """16 agents with the HP channel and k_predict = 64 have no one-launch kernel: mapf_rollout_pibt
    issues T x (pibt_actions, step_observe) itself, and equals a twin driven by those two calls."""
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    name, T = "dense_12x12_n16_f9_dahp", 12
    case, maps, shared, seed = case_setup(name)
    envs = []
    for _ in range(2):
        cfg = make_config(case["B"], case["H"], case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                          use_da=1, use_hp=1, human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared,
                          seed=seed, env_offset=7)
        cfg.k_predict = 64
        envs.append(BatchedMapfGym(cfg))
        envs[-1].reset_seeded(maps)
    env, twin = envs
    try:
        assert not env.rollout_fused and env.rollout_pibt_plan(True) == "pibt_actions+step_observe"
        buf = slot_buffers(env, T)
        acts = torch.full((T, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        env.rollout_pibt(T, slots=True, actions=acts, **buf)
        got = host(buf["out"])
        for t in range(T):
            a = twin.pibt_actions().clone()
            out, obs, vec = twin.step_observe(a)
            out = host(out)
            assert torch.equal(acts[t], a), f"t={t}: actions"
            for key in out:
                assert np.array_equal(got[key][t], out[key]), f"t={t}: {key}"
            assert torch.equal(buf["obs"][t].view(torch.int32), obs.view(torch.int32)), f"t={t}: obs"
            assert torch.equal(buf["vec"][t].view(torch.int32), vec.view(torch.int32)), f"t={t}: vec"
        sa, sb = env.get_state(), twin.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
        assert torch.equal(env.bfs(), twin.bfs())
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 4. packed observations
@pytest.mark.parametrize("name", [DENSE, "c4_40x40_n16_f9_looping"])
def test_packed_observations_equal_the_floats(name):
    from mapf_amd.env import unpack_obs
    T = 24
    ref, state, _ = oracle_run(name)
    env, case, _, _, _ = case_env(name)
    try:
        assert ",bits,pibt>" in env.rollout_pibt_kernel_name(slots=True, obs_bits=True)
        buf = slot_buffers(env, T)
        bits = torch.full((T, env.B, env.N, env.obs_words), -1, dtype=torch.int32, device=env.device)
        acts = torch.full((T, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        env.rollout_pibt(T, slots=True, actions=acts, obs=bits, vec=buf["vec"], out=buf["out"], obs_bits=True)
        obs = unpack_obs(bits, env.C, env.F)
        which = [(q, q) for q in range(T)]
        check_actions(f"{name} bits", ref, 0, acts, which)
        check_slots(f"{name} bits", ref, 0, host(buf["out"]), obs, buf["vec"], which)
        check_state(env, state[T], f"{name} bits")
        covered(env.rollout_pibt_kernel_name(slots=True, obs_bits=True), f"{name} packed pibt vs oracle")
    finally:
        env.close()


# ------------------------------------------------------------------ 5. the launcher
@pytest.mark.parametrize("form,subs", [(dict(roll_occ=4, roll_group=1), 4), (None, 1)])
def test_pibt_launcher_declares_the_band_clean_after_its_first_call(form, subs):
    H.launcher_band_clean_case("pibt", case_env, form, subs, allow=(), mine=PIBT_COVERED)


# ------------------------------------------------------------------ 6. capture
def test_captured_pibt_rollout_continues_the_episode():
    """The ages too are carried from replay to replay through the handle's arrays."""
    H.captured_rollout_case("pibt", case_env, *oracle_run("c4_40x40_n16_f9_looping")[:2], allow=())


# ------------------------------------------------------------------ 7. errors
def test_keep_bfs_off_is_a_state_error_and_T0_is_a_no_op():
    H.keep_bfs_off_case("pibt", case_env)


# ------------------------------------------------------------------ 8. record and replay of fixed episodes
@pytest.mark.parametrize("mtype,da_hp", [(0, False), (1, True)])
def test_pibt_policy_on_fixed_episodes_replays(mtype, da_hp):
    """H.fixed_episodes_case under pibt_policy().  The planner reaches goals and never collides with an
    agent or a wall."""
    from mapf_amd.episodes import pibt_policy
    got = H.fixed_episodes_case(pibt_policy, mtype, da_hp)
    assert got["totalGoals"].sum() > 0
    assert got["staticCollide"].sum() == 0 and got["agentCollide"].sum() == 0


# ------------------------------------------------------------------ 9. coverage guard (last)
@pytest.mark.parametrize("cfg", ["c1", "c2", "c4", "c5"])
def test_default_pibt_kernels_are_covered_by_this_file(cfg):
    H.coverage_guard("pibt", PIBT_COVERED, cfg)
