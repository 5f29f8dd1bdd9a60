"""GPU: persistent rollouts under the descent policy (mapf_rollout_descent, mapf_descent_actions;
include/mapf.h).

The rollout kernels' DESCENT instantiations pick every agent's action inside the kernel from its
tiled BFS map: one step down the map, ties broken by (clock + agent) & 3.  The oracle has no policy:
tests/descent_ref.py restates it in numpy over OracleEnv.bfs() and .agents(), the oracle is stepped
with the result, and every slot is compared bit for bit.  A stale map read can only show where goals
change, so every case first asserts, from the oracle run alone, at least 20 goal changes, 10 of them
before the last step of their launch.

The file ends with a guard: the descent kernel every BASELINE preset launches by default, into
slots and in place, has been run by an oracle-compared case above (tests/kernel_registry.py).
"""
import functools

import numpy as np
import pytest
import torch

import rollout_harness as H
from descent_ref import descent_actions
from rollout_harness import check_slots, check_state, preset_envs, slot_buffers
from test_gpu_parity import FUSED_CASES, GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, WIDE_SHAPES, host

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 23, 40)                       # steps per launch, in this order: 64 steps
DESCENT_COVERED = set()                      # kernel names this file compared against the oracle
CASES = {**FUSED_CASES, **GROUP_CASES, **ROLLOUT_CASES, **RANDOM_CASES, **WIDE_SHAPES}
SEED = 0xDE5C0000


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def case_setup(name):
    return H.case_setup(CASES, name, SEED)


def case_env(name, tuning=None, **kw):
    return H.case_env(CASES, name, SEED, tuning, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(name, steps):
    """The oracle under the restated policy, computed once and shared (read-only): the actions,
    per-step outputs / observations / vectors [steps, B, ...], and the state (cells, goals, human,
    BFS maps, the oracle's error count) after every launch of every path."""
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 25)) | {steps}
    return H.oracle_rollout(CASES, name, SEED, steps, bounds,
                            lambda oe, b, t, world: (descent_actions(oe.bfs(), oe.agents()[0], t), None))


def run_descent_case(name, path, tuning=None, launches=LAUNCHES, expect=None):
    ref, state = oracle_run(name, int(np.sum(launches)))
    H.assert_goals_change(name, ref, launches)
    H.run_policy_case("descent", case_env, DESCENT_COVERED, name, path, ref, state, launches, tuning, expect)


# ------------------------------------------------------------------ 1. the pair-lane kernel
PAIR_CASES = [("r_n6_16x16_f9_dahp", None, "1"),                                            # B = 37: ragged
              ("g_n8_20x20_f11_ragged61", dict(roll_occ=4, roll_group=1, roll_slack=1), "4"),  # grouped, paced
              ("g_n8_20x20_f11", dict(roll_occ=4, roll_fair=4), "4"),                       # grouped, fair
              ("r_n6_12x12_f7_dense", None, "1")]


@pytest.mark.parametrize("path", ["rollout", "inplace1", "inplace"])
@pytest.mark.parametrize("name,tuning,subs", PAIR_CASES)
def test_pair_lane_descent_matches_oracle(name, tuning, subs, path):
    expect = "rollout_random_kernel<%s,%s,descent>" % ("true" if path == "rollout" else "false", subs)
    run_descent_case(name, path, tuning, expect=expect)


# ------------------------------------------------------------------ 2. the wide kernels
WIDE_CASES = [("c4_40x40_n16_f9_looping", None, "rollout", "rollout_wide3_kernel<u64,1,true,descent>"),
              ("c4_40x40_n16_f9_looping", None, "inplace", "rollout_wide3_kernel<u64,1,false,descent>"),
              ("c4_40x40_n16_f9_looping", dict(wide_obs=1), "rollout", "rollout_wide_kernel<u64,1,true,descent>"),
              ("c4_40x40_n16_f9_looping", dict(wide_pipe=0), "rollout", "rollout_wide_kernel<u64,1,true,descent>"),
              ("dense_12x12_n16_f9_dahp", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "inplace", None),
              ("c1_10x10_n4_f11", None, "inplace1", None),
              ("c5_80x80_n64_f11_bfsch", None, "rollout", "rollout_wide_kernel<Row2,2,true,descent>"),
              ("w_n20_48x90_f11_bfsch", None, "rollout", None)]


@pytest.mark.parametrize("name,tuning,path,expect", WIDE_CASES)
def test_wide_descent_matches_oracle(name, tuning, path, expect):
    """The one-wave-per-env kernels: three waves per env (c4's form, the stepper searching: bfsobs=0),
    two (wide_obs 1), one (wide_pipe 0; c5's Row2 form at B = 3), u32 / u64 / 128-bit search rows, the
    BFS channel."""
    run_descent_case(name, path, tuning, expect=expect)


# ------------------------------------------------------------------ 3. the per-step path
@pytest.mark.parametrize("path", ["rollout", "inplace"])
def test_single_agent_descent_matches_oracle(path):
    """n = 1 (one lane steps; the tie-break rotates with the clock alone), 300 envs."""
    run_descent_case("n1_12x12_f7_looping", path)


@pytest.mark.parametrize("name", ["n1_12x12_f7_looping", "r_n6_16x16_f9_dahp"])
def test_descent_actions_then_step_observe_matches_oracle(name):
    """The per-step entry point: T x (descent_actions, step_observe) against the oracle."""
    T = 24
    ref, state = oracle_run(name, int(np.sum(LAUNCHES)))
    env, case, _, _, _ = case_env(name)
    try:
        for t in range(T):
            acts = env.descent_actions()
            assert np.array_equal(acts.cpu().numpy(), ref["actions"][t]), f"t={t}: actions"
            out, obs, vec = env.step_observe(acts)
            check_slots(f"{name} per step", ref, t, {k: v[None] for k, v in host(out).items()}, obs[None], vec[None], [(0, 0)])
        check_state(env, state[T], name)
    finally:
        env.close()


@pytest.mark.parametrize("slots", [True, False])
def test_rollout_descent_without_a_one_launch_form_equals_the_per_step_calls(slots):
    """16 agents with the HP channel and k_predict = 64 have no one-launch kernel (the wide kernels'
    snapshot holds at most 63 predicted cells): mapf_rollout_descent issues T x (descent_actions,
    step_observe) itself, and equals a twin driven by those two calls."""
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
        assert not env.rollout_fused and env.rollout_descent_plan(slots) == "descent_actions+step_observe"
        k = T if slots else 1
        buf = slot_buffers(env, k)
        acts = torch.full((k, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        env.rollout_descent(T, slots=slots, actions=acts, **buf)
        got = host(buf["out"])
        goals = 0
        for t in range(T):
            a = twin.descent_actions().clone()
            out, obs, vec = twin.step_observe(a)
            out = host(out)
            goals += int(out["goals_reached"].sum())
            if slots or t == T - 1:
                q = t if slots else 0
                assert torch.equal(acts[q], a), f"t={t}: actions"
                for key in out:
                    assert np.array_equal(got[key][q], out[key]), f"t={t}: {key}"
                assert torch.equal(buf["obs"][q].view(torch.int32), obs.view(torch.int32)), f"t={t}: obs"
                assert torch.equal(buf["vec"][q].view(torch.int32), vec.view(torch.int32)), f"t={t}: vec"
        assert goals >= 20, goals
        sa, sb = env.get_state(), twin.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
        assert torch.equal(env.bfs(), twin.bfs())
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 4. record equals replay, full size
@pytest.mark.parametrize("cfg,T,slots", [("c2", 8, True), ("c4", 8, True), ("c5", 8, True), ("c2", 8, False)])
def test_record_equals_replay_at_full_size(cfg, T, slots):
    """rollout_descent on one handle records its actions; rollout_actions over them on a twin: every
    output, every observation bit, the state and the counters are equal."""
    rec, rep, *more = preset_envs(cfg, 2 if slots else 3)
    try:
        k = T if slots else 1
        acts = torch.full((T, rec.B, rec.N), -9, dtype=torch.int32, device=rec.device)
        a, b = slot_buffers(rec, k), slot_buffers(rep, k)
        if slots:
            rec.rollout_descent(T, slots=True, actions=acts, **a)
        else:            # in place the chosen actions are overwritten every step: a third handle records them
            more[0].rollout_descent(T, slots=True, actions=acts, **slot_buffers(more[0], T))
            more[0].close()
            rec.rollout_descent(T, slots=False, actions=torch.empty_like(acts[0]), **a)
        assert rec.rollout_descent_kernel_name(slots).replace(",descent>", ">") == rec.rollout_kernel_name(slots)
        rep.rollout_actions(acts, slots=slots, **b)
        torch.cuda.synchronize()
        assert int(acts.min()) >= 0 and int(acts.max()) <= 4
        assert torch.equal(a["obs"].view(torch.int32), b["obs"].view(torch.int32)), "obs"
        assert torch.equal(a["vec"].view(torch.int32), b["vec"].view(torch.int32)), "vec"
        for key in a["out"]:
            assert torch.equal(a["out"][key], b["out"][key]), key
        sa, sb = rec.get_state(), rep.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
        assert torch.equal(rec.bfs(), rep.bfs())
        assert (rec.counters()[:8] == rep.counters()[:8]).all()
    finally:
        rec.close()
        rep.close()


# ------------------------------------------------------------------ 5. band-clean launcher
@pytest.mark.parametrize("form,subs", [(dict(roll_occ=4, roll_group=1), 4), (None, 1)])
def test_descent_launcher_declares_the_band_clean_after_its_first_call(form, subs):
    H.launcher_band_clean_case("descent", case_env, form, subs)


# ------------------------------------------------------------------ 6. capture
def test_captured_descent_rollout_continues_the_episode():
    H.captured_rollout_case("descent", case_env, *oracle_run("c4_40x40_n16_f9_looping", int(np.sum(LAUNCHES))))


# ------------------------------------------------------------------ 7. errors
def test_keep_bfs_off_is_a_state_error_and_T0_is_a_no_op():
    H.keep_bfs_off_case("descent", case_env)


# ------------------------------------------------------------------ 8. record and replay of fixed episodes
@pytest.mark.parametrize("mtype,da_hp", [(0, False), (1, True)])
def test_descent_policy_on_fixed_episodes_replays(mtype, da_hp):
    """H.fixed_episodes_case under descent_policy().  The baseline reaches goals on these episodes."""
    from mapf_amd.episodes import descent_policy
    got = H.fixed_episodes_case(descent_policy, mtype, da_hp)
    assert got["totalGoals"].sum() > 0
    assert got["staticCollide"].sum() == 0


# ------------------------------------------------------------------ 9. coverage guard (last)
@pytest.mark.parametrize("cfg", ["c1", "c2", "c4", "c5"])
def test_default_descent_kernels_are_covered_by_this_file(cfg):
    H.coverage_guard("descent", DESCENT_COVERED, cfg)
