"""GPU: the PIBT policy's human weight (mapf_set_pibt_human_weight; include/mapf.h: mapf_pibt_actions step 2)
in every kernel that builds PIBT candidates: the per-step pick, the pair-lane rollout kernel (ungrouped,
grouped and paced, grouped and fair) and the wide one-/two-/three-wave kernels.

The oracle has no policy: tests/pibt_human_ref.py restates the weighted policy in numpy, the oracle is
stepped with its picks, and every slot is compared bit for bit -- chosen actions, all step outputs,
observations, vectors, and the state and BFS maps after every launch; allow=(): no device counter may count.

Conditions on the inputs, asserted from the reference run alone before any device call, per case:
rollout_harness.assert_goals_change, and at least 100 picks that differ from the weight-0 pick in the same
state (the reference computes both; a case without such picks cannot see the weight).  Two cases run at
penalty_radius = 3 and weight 1, which pins constr_d2 and the level against a second radius.
"""
import functools

import numpy as np
import pytest
import torch

import pibt_human_ref as PH
import pibt_ref
import rollout_harness as H
from rollout_harness import check_actions, check_slots, check_state, slot_buffers
from test_gpu_parity import FUSED_CASES, GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, WIDE_SHAPES, host

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 23, 40)                       # steps per launch, in this order: 64 steps
HUMAN_COVERED = set()                        # kernel names this file compared against the oracle
DENSE = "p_n8_8x8_f5_dense"                  # test_gpu_rollout_pibt.py's own shape: 8 agents, shared 8 x 8 map
CASES = {**FUSED_CASES, **GROUP_CASES, **ROLLOUT_CASES, **RANDOM_CASES, **WIDE_SHAPES,
         DENSE: dict(B=24, H=8, W=8, n=8, fov=5, nch=6, map="sparse_shared", map_seed=2)}
SEED = 0x48550000
G, C4, W20, R6 = "g_n8_20x20_f11", "c4_40x40_n16_f9_looping", "w_n20_48x90_f11_bfsch", "r_n6_16x16_f9_dahp"
R5 = (2, 5)                                  # (human weight, penalty radius): the default radius
R3 = (1, 3)                                  # a second radius: constr_d2 = 8


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def cfg_of(R):
    return None if R == 5 else dict(penalty_radius=R)


def env_of(w, R=5):
    """The harness's env_of for weight w and radius R: H.case_env, then set_pibt_human_weight (None: never set)."""
    def make(name, tuning=None, **kw):
        made = H.case_env(CASES, name, SEED, tuning, cfg=cfg_of(R), **kw)
        if w is not None:
            made[0].set_pibt_human_weight(w)
        return made
    return make


def key_order(key):
    """Each agent's candidates in ascending key, the actions that are not admitted (-1) last."""
    return np.argsort(np.where(key < 0, 1 << 40, key), axis=1, kind="stable")


@functools.lru_cache(maxsize=None)
def oracle_run(name, w, R, switch=0, steps=int(np.sum(LAUNCHES))):
    """The oracle under the restated policy at weight w (weight 0 before step `switch`) and radius R,
    computed once and shared (read-only): H.oracle_rollout's (ref, state), plus the run's count of picks
    that differ from the weight-0 pick in the same state and the failed picks standing on hn per step."""
    n = CASES[name]["n"]
    ages = [pibt_ref.Ages(n) for _ in range(CASES[name]["B"])]
    stats = dict(differ=0, picks=0)

    def pick(oe, b, t, world):
        world = np.asarray(world, np.int8)
        pos, goal = oe.agents()
        hum = oe.human()
        wt = w if t >= switch else 0
        bfs = oe.bfs()
        a, failed, _ = PH.pibt_actions(world, bfs, pos, goal, hum["pos"], hum["next"], t, ages[b], wt, R)
        stats["picks"] += n
        if wt:      # the ages are idempotent at one clock: the second pick sees the same ones
            k0 = pibt_ref.candidate_keys(world, bfs, pos, hum["pos"], hum["next"], t)
            kw = PH.candidate_keys(world, bfs, pos, hum["pos"], hum["next"], t, wt, R)
            if not np.array_equal(key_order(k0), key_order(kw)):       # the same orders give the same picks
                a0 = pibt_ref.pibt_actions(world, bfs, pos, goal, hum["pos"], hum["next"], t, ages[b])[0]
                stats["differ"] += int((a0 != a).sum())
        hit = np.zeros(n, bool)
        for i in failed:
            hit[i] = tuple(pos[i]) == tuple(hum["next"])
        return a, dict(may_hit=hit)
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 41)) | {steps}
    return H.oracle_rollout(CASES, name, SEED, steps, bounds, pick, cfg=cfg_of(R)) + (stats,)


def assert_inputs(name, w, R, launches=LAUNCHES):
    """The per-case conditions, from the reference run alone."""
    ref, state, stats = oracle_run(name, w, R)
    H.assert_goals_change(name, ref, launches)
    bad = int(((ref["status"] == -1) | (ref["status"] == -3)).sum())
    print(f"{name} w={w} R={R}: {stats['differ']} of {stats['picks']} picks differ from weight 0; "
          f"constraints {int(ref['constraints'].sum())}, status -1/-3 {bad}")
    assert stats["differ"] >= 100, (name, stats)
    assert bad == 0 and state[int(np.sum(LAUNCHES))]["errors"] == 0
    return ref, state


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


# ------------------------------------------------------------------ 1. every kernel family against the oracle
ROLL_CASES = [(G, R5, None, "rollout", "rollout_random_kernel<true,1,pibt>"),                  # pair-lane, ungrouped
              (G, R5, None, "inplace", "rollout_random_kernel<false,1,pibt>"),
              (G, R5, None, "inplace1", "rollout_random_kernel<false,1,pibt>"),
              (G, R5, dict(roll_occ=4, roll_group=1, roll_slack=1), "rollout", "rollout_random_kernel<true,4,pibt>"),   # paced
              (G, R5, dict(roll_occ=4, roll_fair=4), "rollout", "rollout_random_kernel<true,4,pibt>"),                  # fair
              (G, R5, dict(roll_occ=4, roll_fair=4), "inplace", "rollout_random_kernel<false,4,pibt>"),
              (DENSE, R5, None, "rollout", "rollout_random_kernel<true,1,pibt>"),
              (R6, R5, None, "rollout", "rollout_random_kernel<true,1,pibt>"),                 # B = 37: ragged
              (C4, R5, None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>"),              # three waves per env
              (C4, R5, None, "inplace", "rollout_wide3_kernel<u64,1,false,pibt>"),
              (C4, R5, None, "inplace1", "rollout_wide3_kernel<u64,1,false,pibt>"),
              (C4, R5, dict(wide_obs=1), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),   # two
              (C4, R5, dict(wide_pipe=0), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),  # one
              ("c1_10x10_n4_f11", R5, None, "rollout", None),
              (W20, R5, None, "rollout", None),
              (W20, R5, None, "inplace", None),
              ("dense_12x12_n16_f9_dahp", R5, None, "rollout", None),
              (G, R3, None, "rollout", "rollout_random_kernel<true,1,pibt>"),
              (C4, R3, None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>")]


@pytest.mark.parametrize("name,wr,tuning,path,expect", ROLL_CASES)
def test_weighted_rollout_matches_oracle(name, wr, tuning, path, expect):
    w, R = wr
    ref, state = assert_inputs(name, w, R)
    t0 = H.run_policy_case("pibt", env_of(w, R), HUMAN_COVERED, name, path, ref, state, LAUNCHES, tuning, expect,
                           allow=(), hook=assert_consequences)
    assert int(np.sum(LAUNCHES)) >= t0


# ------------------------------------------------------------------ 2. per-step picks
def test_weighted_pibt_actions_then_step_observe_matches_oracle():
    """T x (pibt_actions, step_observe) at weight 2 against the same reference as the one-launch form."""
    T = 24
    ref, state = assert_inputs(R6, 2, 5)
    env = env_of(2)(R6)[0]
    try:
        for t in range(T):
            acts = env.pibt_actions()
            assert np.array_equal(acts.cpu().numpy(), ref["actions"][t]), f"t={t}: actions"
            out, obs, vec = env.step_observe(acts)
            check_slots(f"{R6} per step", ref, t, {k: v[None] for k, v in host(out).items()}, obs[None], vec[None], [(0, 0)])
        check_state(env, state[T], R6)
        H.assert_no_errors(env, allow=())
    finally:
        env.close()


# ------------------------------------------------------------------ 3. weight 0 is the plain policy; the setter
def test_weight_0_after_weight_2_is_the_policy_of_a_handle_never_set():
    from mapf_amd import _lib
    L = _lib.lib()
    T = 24
    env, case, maps, _, _ = env_of(None)(DENSE)
    twin = env_of(None)(DENSE)[0]
    try:
        assert env.pibt_human_weight == 0 and L.mapf_get_pibt_human_weight(env.h) == 0      # mapf_create's default
        env.set_pibt_human_weight(2)
        assert env.pibt_human_weight == 2
        env.rollout_pibt(8)
        for bad in (17, -1):
            assert L.mapf_set_pibt_human_weight(env.h, bad) == -1
            assert L.mapf_get_pibt_human_weight(env.h) == 2, bad
        env.reset_seeded(maps)
        assert env.pibt_human_weight == 2                       # a reset leaves the weight alone
        env.set_state(clock=env.get_state()["clock"])
        assert env.pibt_human_weight == 2                       # and so does mapf_set_state
        env.set_pibt_human_weight(0)
        assert env.pibt_human_weight == 0
        env.reset_seeded(maps)
        twin.reset_seeded(maps)
        got, want = slot_buffers(env, T), slot_buffers(twin, T)
        a_got, a_want = H.action_buffer(env, T), H.action_buffer(twin, T)
        env.rollout_pibt(T, slots=True, actions=a_got, **got)
        twin.rollout_pibt(T, slots=True, actions=a_want, **want)
        torch.cuda.synchronize()
        assert torch.equal(a_got, a_want), "actions"
        for key in want["out"]:
            assert torch.equal(got["out"][key], want["out"][key]), key
        assert torch.equal(got["obs"].view(torch.int32), want["obs"].view(torch.int32)), "obs"
        assert torch.equal(got["vec"].view(torch.int32), want["vec"].view(torch.int32)), "vec"
        # and the twin's run is the plain policy's: pibt_ref from the same reset
        ref0, _, _ = oracle_run(DENSE, 0, 5)
        check_actions("weight 0 twin", ref0, 0, a_want, [(q, q) for q in range(T)])
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 4. a switch between launches
def test_weight_set_between_launches_takes_effect_at_the_next_one():
    """Launch 1 (1 step) at weight 0, launches 2 and 3 at weight 2; the reference switches at the same
    step and keeps its ages, as the handle does."""
    ref, state, stats = oracle_run(DENSE, 2, 5, switch=LAUNCHES[0])
    assert stats["differ"] >= 100, stats
    plain = oracle_run(DENSE, 0, 5)[0]
    assert np.array_equal(ref["actions"][0], plain["actions"][0])            # step 0 is the plain policy's
    env, case, _, _, _ = env_of(0)(DENSE)
    try:
        t0 = 0
        for n_launch, T in enumerate(LAUNCHES):
            if n_launch == 1:
                env.set_pibt_human_weight(2)
            buf, acts = slot_buffers(env, T), H.action_buffer(env, T)
            env.rollout_pibt(T, slots=True, actions=acts, **buf)
            which = [(q, q) for q in range(T)]
            check_actions(f"launch {n_launch}", ref, t0, acts, which)
            check_slots(f"launch {n_launch}", ref, t0, host(buf["out"]), buf["obs"], buf["vec"], which)
            t0 += T
            check_state(env, state[t0], f"launch {n_launch}")
        H.assert_no_errors(env, allow=())
    finally:
        env.close()


# ------------------------------------------------------------------ 5. the plan text
@pytest.mark.parametrize("name", [G, C4])
def test_plan_text_names_the_weight_and_keeps_the_kernel(name):
    env = env_of(None)(name)[0]
    try:
        for slots in (False, True):
            never = env.rollout_pibt_plan(slots)
            kname = env.rollout_pibt_kernel_name(slots)
            assert "human_weight" not in never
            env.set_pibt_human_weight(2)
            text = env.rollout_pibt_plan(slots)
            assert text == never + " human_weight=2", (text, never)
            assert env.rollout_pibt_kernel_name(slots) == kname
            assert "human_weight" not in env.rollout_plan(slots) and "human_weight" not in env.rollout_descent_plan(slots)
            env.set_pibt_human_weight(0)
            assert env.rollout_pibt_plan(slots) == never
    finally:
        env.close()


# ------------------------------------------------------------------ 6. capture
def test_captured_weighted_rollout_continues_the_episode():
    ref, state = assert_inputs(C4, 2, 5)
    H.captured_rollout_case("pibt", env_of(2), ref, state, allow=())


# ------------------------------------------------------------------ 7. the other entry points at weight 2
def test_packed_observations_at_weight_2_equal_the_floats():
    from mapf_amd.env import unpack_obs
    T = 24
    ref, state = assert_inputs(G, 2, 5)
    env, case, _, _, _ = env_of(2)(G)
    try:
        assert ",bits,pibt>" in env.rollout_pibt_kernel_name(slots=True, obs_bits=True)
        buf = slot_buffers(env, T)
        bits = torch.full((T, env.B, env.N, env.obs_words), -1, dtype=torch.int32, device=env.device)
        acts = H.action_buffer(env, T)
        env.rollout_pibt(T, slots=True, actions=acts, obs=bits, vec=buf["vec"], out=buf["out"], obs_bits=True)
        obs = unpack_obs(bits, env.C, env.F)
        which = [(q, q) for q in range(T)]
        check_actions(f"{G} bits", ref, 0, acts, which)
        check_slots(f"{G} bits", ref, 0, host(buf["out"]), obs, buf["vec"], which)
        check_state(env, state[T], f"{G} bits")
    finally:
        env.close()


def test_pibt_policy_with_a_weight_on_fixed_episodes_replays():
    """H.fixed_episodes_case under pibt_policy(human_weight=2): the weight reaches the envs the evaluation
    builds (fewer constraint violations than the plain policy on the same episodes), and the planner's
    guarantees hold."""
    from mapf_amd.episodes import pibt_policy
    got = H.fixed_episodes_case(lambda: pibt_policy(human_weight=2), 0, False)
    plain = H.fixed_episodes_case(pibt_policy, 0, False)
    print("constraintViolations:", got["constraintViolations"].sum(), "at weight 2,", plain["constraintViolations"].sum(), "plain")
    assert got["totalGoals"].sum() > 0
    assert got["staticCollide"].sum() == 0 and got["agentCollide"].sum() == 0
    assert not np.array_equal(got["constraintViolations"], plain["constraintViolations"])


def test_demo_runner_sets_the_weight_once():
    from mapf_amd.imitation import DemoRunner
    T = 8
    env = env_of(None)(G)[0]
    twin = env_of(2)(G)[0]
    try:
        demo = DemoRunner(env, T, policy="pibt", human_weight=2)
        assert env.pibt_human_weight == 2
        demo.run()
        acts = H.action_buffer(twin, T)
        twin.rollout(T, "pibt", slots=True, actions=acts, **slot_buffers(twin, T))
        torch.cuda.synchronize()
        assert torch.equal(demo.expert_actions, acts)
        ref = assert_inputs(G, 2, 5)[0]
        check_actions("demo", ref, 0, demo.expert_actions, [(q, q) for q in range(T)])
        with pytest.raises(ValueError, match="human_weight"):
            DemoRunner(env, T, policy="descent", human_weight=2)
    finally:
        env.close()
        twin.close()


def test_device_runner_labels_its_states_with_the_weighted_expert():
    """DeviceRunner(expert="pibt", expert_human_weight=2) sets the weight once: expert_actions[t] are the
    picks of a twin at weight 2 driven through the runner's own actions, and they are not all the plain
    planner's (a twin at weight 0 on the same states labels at least one agent-step differently)."""
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    from mapf_amd.model import Model
    from mapf_amd.runner import DeviceRunner
    T = 12

    def env():
        e = BatchedMapfGym(make_config(16, 20, 20, num_agents=8, fov=9, num_channel=6, human_mode="random",
                                       goal_mode="random", fix_choice=1, keep_bfs=True, seed=99))
        e.reset_seeded(generate_warehouse(20, 20))
        return e
    torch.manual_seed(0)
    model = Model(0, "cuda", global_model=True, numChannel=6, num_agents=8, fov=9)
    model.network.eval()
    own, twin, plain = env(), env(), env()
    try:
        runner = DeviceRunner(own, model, n_steps=T, seed=5, expert="pibt", expert_human_weight=2)
        assert own.pibt_human_weight == 2
        runner.run()
        twin.set_pibt_human_weight(2)
        differ = 0
        for t in range(T):
            label = twin.pibt_actions().clone()
            assert torch.equal(runner.expert_actions[t], label), t
            differ += int((plain.pibt_actions() != label).sum())
            a = runner.actions[t].int().contiguous()
            twin.step(a)
            plain.step(a)
        print(f"{differ} of {T * 16 * 8} labels differ from the plain planner's on the same states")
        assert differ > 0
        with pytest.raises(ValueError, match="expert_human_weight"):
            DeviceRunner(own, model, n_steps=T, expert="descent", expert_human_weight=2)
    finally:
        for e in (own, twin, plain):
            e.close()
