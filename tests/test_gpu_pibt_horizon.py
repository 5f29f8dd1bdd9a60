"""GPU: the PIBT policy's human horizon (mapf_set_pibt_human_horizon; include/mapf.h: mapf_pibt_actions step 2)
in every kernel that builds PIBT candidates: the per-step pick (the path cells from HBM), the pair-lane
rollout kernel (from the wave's LDS copy of the path; ungrouped, grouped and paced, grouped and fair) and the
wide one-/two-/three-wave kernels (lane j's register, loaded a step ahead), and mapf_pibt_human_cells.

The oracle has no policy: tests/pibt_horizon_ref.py restates the policy in numpy from the oracle's own
human (next cell, step, current path), the oracle is stepped with its picks, and every slot is compared bit
for bit -- chosen actions, all step outputs, observations, vectors, and the state and BFS maps after every
launch; allow=(): no device counter may count.

Conditions on the inputs, asserted from the reference run alone before any device call, per case:
rollout_harness.assert_goals_change; no status -1 / -3 and no oracle error; at least 100 picks that differ
from the horizon-1 pick in the same state (a case without such picks cannot see the horizon); at least 20
env-steps whose horizon is cut short by the path's end, and at least 5 env-steps at a path switch
(step >= len - 1), where the cells come from the buffer switched to a step later.  The 48 x 90 shape
(5 envs, paths longer than the run) cannot hold the last two and is held to the others.
"""
import functools

import numpy as np
import pytest
import torch

import pibt_horizon_ref as PZ
import pibt_human_ref as PH
import pibt_ref
import rollout_harness as H
from rollout_harness import check_actions, check_slots, check_state, slot_buffers
from test_gpu_parity import host
from test_gpu_pibt_human import C4, CASES, DENSE, G, LAUNCHES, R6, SEED, W20, assert_consequences, cfg_of, key_order

pytestmark = pytest.mark.gpu

HORIZON_COVERED = set()                      # kernel names this file compared against the oracle
K3 = (2, 5, 3)                               # (human weight, penalty radius, human horizon)
K8 = (2, 5, 8)                               # the last lane that carries a cell
R3K4 = (1, 3, 4)                             # a second weight, radius and horizon
STEPS = int(np.sum(LAUNCHES))
# 5 envs on a 48 x 90 map: the human's paths are longer than the run, so no seed brings 20 path ends into
# 320 env-steps; the shape is there for the two-lane search rows, and keeps the other conditions
LONG_PATHS = {W20}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def env_of(w, R=5, K=None):
    """The harness's env_of for weight w, radius R and horizon K (None: never set)."""
    def make(name, tuning=None, **kw):
        made = H.case_env(CASES, name, SEED, tuning, cfg=cfg_of(R), **kw)
        if w is not None:
            made[0].set_pibt_human_weight(w)
        if K is not None:
            made[0].set_pibt_human_horizon(K)
        return made
    return make


@functools.lru_cache(maxsize=None)
def oracle_run(name, w, R, K, switch=0, steps=STEPS):
    """The oracle under the restated policy at weight w, radius R and horizon K (horizon 1 before step
    `switch`), computed once and shared (read-only): H.oracle_rollout's (ref, state) -- ref["cells"][t] =
    mapf_pibt_human_cells' rows for the state BEFORE step t --, plus the run's counts: picks that differ
    from the horizon-1 pick in the same state, env-steps whose horizon the path's end cuts short,
    env-steps at a path switch."""
    n = CASES[name]["n"]
    ages = [pibt_ref.Ages(n) for _ in range(CASES[name]["B"])]
    stats = dict(differ=0, picks=0, truncated=0, switches=0)

    def pick(oe, b, t, world):
        world = np.asarray(world, np.int8)
        pos, goal = oe.agents()
        hum = oe.human()
        Kt = K if t >= switch else 1
        a, failed, _ = PZ.pibt_actions(world, oe, t, ages[b], w, R, Kt)
        stats["picks"] += n
        if Kt > 1:
            stats["truncated"] += len(PZ.human_cells(oe, Kt)) < Kt
            stats["switches"] += hum["step"] >= hum["len"] - 1
            if w:       # the ages are idempotent at one clock: the second pick sees the same ones
                bfs = oe.bfs()
                k1 = PH.candidate_keys(world, bfs, pos, hum["pos"], hum["next"], t, w, R)
                kk = PZ.candidate_keys(world, bfs, pos, hum["pos"], PZ.human_cells(oe, Kt), t, w, R)
                if not np.array_equal(key_order(k1), key_order(kk)):       # the same orders give the same picks
                    a1 = PH.pibt_actions(world, bfs, pos, goal, hum["pos"], hum["next"], t, ages[b], w, R)[0]
                    stats["differ"] += int((a1 != a).sum())
        hit = np.zeros(n, bool)
        for i in failed:
            hit[i] = tuple(pos[i]) == tuple(hum["next"])
        return a, dict(may_hit=hit, cells=PZ.packed_cells(oe))
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 41)) | {steps}
    return H.oracle_rollout(CASES, name, SEED, steps, bounds, pick, cfg=cfg_of(R)) + (stats,)


def assert_inputs(name, w, R, K, launches=LAUNCHES):
    """The per-case conditions, from the reference run alone."""
    ref, state, stats = oracle_run(name, w, R, K)
    H.assert_goals_change(name, ref, launches)
    bad = int(((ref["status"] == -1) | (ref["status"] == -3)).sum())
    print(f"{name} w={w} R={R} K={K}: {stats['differ']} of {stats['picks']} picks differ from horizon 1, "
          f"{stats['truncated']} env-steps truncated, {stats['switches']} at a switch; "
          f"constraints {int(ref['constraints'].sum())}, status -1/-3 {bad}")
    assert bad == 0 and state[STEPS]["errors"] == 0
    assert stats["differ"] >= 100, (name, stats)
    if name not in LONG_PATHS:
        assert stats["truncated"] >= 20, (name, stats)
        assert stats["switches"] >= 5, (name, stats)
    return ref, state


# ------------------------------------------------------------------ 1. every kernel family against the oracle
ROLL_CASES = [(G, K3, None, "rollout", "rollout_random_kernel<true,1,pibt>"),                  # pair-lane, ungrouped
              (G, K3, None, "inplace", "rollout_random_kernel<false,1,pibt>"),
              (G, K3, None, "inplace1", "rollout_random_kernel<false,1,pibt>"),
              (G, K3, dict(roll_occ=4, roll_group=1, roll_slack=1), "rollout", "rollout_random_kernel<true,4,pibt>"),   # paced
              (G, K3, dict(roll_occ=4, roll_fair=4), "rollout", "rollout_random_kernel<true,4,pibt>"),                  # fair
              (G, K3, dict(roll_occ=4, roll_fair=4), "inplace", "rollout_random_kernel<false,4,pibt>"),
              (DENSE, K3, None, "rollout", "rollout_random_kernel<true,1,pibt>"),
              (R6, K3, None, "rollout", "rollout_random_kernel<true,1,pibt>"),                 # B = 37: ragged
              (C4, K3, None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>"),              # three waves per env
              (C4, K3, None, "inplace", "rollout_wide3_kernel<u64,1,false,pibt>"),
              (C4, K3, None, "inplace1", "rollout_wide3_kernel<u64,1,false,pibt>"),
              (C4, K3, dict(wide_obs=1), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),   # two
              (C4, K3, dict(wide_pipe=0), "rollout", "rollout_wide_kernel<u64,1,true,pibt>"),  # one
              ("c1_10x10_n4_f11", K3, None, "rollout", None),
              ("dense_12x12_n16_f9_dahp", K3, None, "rollout", None),
              (W20, K3, None, "rollout", None),
              (G, K8, None, "rollout", "rollout_random_kernel<true,1,pibt>"),
              (C4, K8, None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>"),
              (G, R3K4, None, "rollout", "rollout_random_kernel<true,1,pibt>"),
              (C4, R3K4, None, "rollout", "rollout_wide3_kernel<u64,1,true,pibt>")]


@pytest.mark.parametrize("name,wrk,tuning,path,expect", ROLL_CASES)
def test_horizon_rollout_matches_oracle(name, wrk, tuning, path, expect):
    w, R, K = wrk
    ref, state = assert_inputs(name, w, R, K)
    t0 = H.run_policy_case("pibt", env_of(w, R, K), HORIZON_COVERED, name, path, ref, state, LAUNCHES, tuning, expect,
                           allow=(), hook=assert_consequences)
    assert STEPS >= t0


# ------------------------------------------------------------------ 2. the cells, and the per-step picks
def test_pibt_human_cells_and_per_step_picks_match_oracle_random_goals():
    """pibt_human_cells() before every step of 40, then T x (pibt_actions, step_observe) at weight 2,
    horizon 3 against the same reference as the one-launch form (the human walks to random goals)."""
    T = 40
    ref, state = assert_inputs(R6, *K3)
    env = env_of(*K3)(R6)[0]
    try:
        for t in range(T):
            assert np.array_equal(env.pibt_human_cells().cpu().numpy(), ref["cells"][t]), f"t={t}: cells"
            acts = env.pibt_actions()
            assert np.array_equal(acts.cpu().numpy(), ref["actions"][t]), f"t={t}: actions"
            out, obs, vec = env.step_observe(acts)
            check_slots(f"{R6} per step", ref, t, {k: v[None] for k, v in host(out).items()}, obs[None], vec[None], [(0, 0)])
        assert np.array_equal(env.pibt_human_cells().cpu().numpy(), ref["cells"][T])
        check_state(env, state[T], R6)
        H.assert_no_errors(env, allow=())
    finally:
        env.close()


def test_pibt_human_cells_match_oracle_looping_human():
    """The looping human (c4 shape), one-step launches at horizon 8: all eight cells before every step of
    40 and after the last, into a caller's buffer."""
    T = 40
    ref, state = assert_inputs(C4, *K8)
    env = env_of(*K8)(C4)[0]
    try:
        out = torch.empty((env.B, 8), dtype=torch.int32, device=env.device)
        for t in range(T):
            assert env.pibt_human_cells(out) is out
            assert np.array_equal(out.cpu().numpy(), ref["cells"][t]), f"t={t}: cells"
            env.rollout_pibt(1)
        assert np.array_equal(env.pibt_human_cells().cpu().numpy(), ref["cells"][T])
        check_state(env, state[T], C4)
    finally:
        env.close()


# ------------------------------------------------------------------ 3. the g6 fixed episodes
def g6_oracles(mtype, idx, infos, seed):
    from oracle import oracle as O
    n = len(infos["agentsSequence"][idx[0]])
    S = max(len(s) for i in idx for s in infos["agentsSequence"][i])
    HS = max(len(infos["humanSequence"][i]) for i in idx) if mtype == 1 else 2
    made = []
    for b, i in enumerate(idx):
        world = np.asarray(infos["obstacleMap"][i], np.int8)
        cfg = O.make_config(world.shape[0], world.shape[1], n, 9, 6, human_mode=2 if mtype == 1 else 0, goal_mode=0,
                            fix_choice=1, max_seq=S, max_human_seq=HS, seed=seed)
        oe = O.OracleEnv(cfg, env_id=b)
        oe.reset_fixed(world, infos["agentsSequence"][i], infos["humanStart"][i], infos["humanGoal"][i],
                       infos["humanSequence"][i] if mtype == 1 else None)
        made.append((world, oe))
    return made


@pytest.mark.parametrize("mtype", [0, 1])
def test_pibt_policy_with_a_horizon_on_fixed_episodes_equals_the_restatement(mtype):
    """evaluate_fixed_episodes under pibt_policy(human_weight=2, human_horizon=3) (LoopingHuman / FixedPathHuman
    over goal sequences): the recorded actions are the restatement's on oracles of the same episodes, and
    the constraint violations the oracle's; on one group, pibt_human_cells() step by step."""
    from mapf_amd import episodes as E
    from mapf_amd.config import SetupParameters
    infos = E.load_fixed_episode_infos(H.G6)
    steps = 48
    kw = dict(num_channel=6, fov=9, human_movement_type=mtype, fix_choice=1)
    got, tapes = E.evaluate_fixed_episodes(infos, E.pibt_policy(human_weight=2, human_horizon=3), max_steps=steps,
                                           record_actions=True, keep_bfs=True, **kw)
    differ = 0
    for (Hh, Ww), idx in sorted(E._groups_by_shape(infos).items()):
        tape = tapes[(Hh, Ww)].cpu().numpy()
        env = E._group_env(infos, idx, Hh, Ww, torch.device("cuda"), 6, 9, False, False, mtype, 5, 1, keep_bfs=True)
        try:
            for b, (world, oe) in enumerate(g6_oracles(mtype, idx, infos, SetupParameters.SEED)):
                ages = pibt_ref.Ages(oe.N)
                constr = 0
                for t in range(steps):
                    if b == 0:
                        assert np.array_equal(env.pibt_human_cells().cpu().numpy()[0], PZ.packed_cells(oe)), (idx, t)
                        env.step(torch.from_numpy(tape[t]).to(env.device))
                    a = PZ.pibt_actions(world, oe, t, ages, 2, 5, 3)[0]
                    assert np.array_equal(tape[t, b], a), (idx[b], t, tape[t, b], a)
                    pos, goal = oe.agents()
                    hum = oe.human()
                    a1 = PH.pibt_actions(world, oe.bfs(), pos, goal, hum["pos"], hum["next"], t, ages, 2, 5)[0]
                    differ += int((a1 != a).sum())
                    constr += int(np.sum(oe.step(a)["constr"]))
                assert oe.errors() == 0
                assert got["constraintViolations"][idx[b]] == constr, idx[b]
        finally:
            env.close()
    print(f"mtype {mtype}: {differ} picks differ from horizon 1")
    assert differ >= 10                          # of the reference alone: 4 episodes x 48 steps still see the horizon
    assert got["staticCollide"].sum() == 0 and got["agentCollide"].sum() == 0 and got["totalGoals"].sum() > 0


# ------------------------------------------------------------------ 4. horizon 1 is the policy without a horizon; the setter
def rollouts_equal(env, twin, T):
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
    return a_want


@pytest.mark.parametrize("name", [DENSE, C4])
def test_horizon_1_after_horizon_3_is_the_policy_of_a_handle_never_set(name):
    from mapf_amd import _lib
    L = _lib.lib()
    T = 24
    env, case, maps, _, _ = env_of(2)(name)
    twin = env_of(2)(name)[0]
    try:
        assert env.pibt_human_horizon == 1 and L.mapf_get_pibt_human_horizon(env.h) == 1      # mapf_create's default
        env.set_pibt_human_horizon(3)
        assert env.pibt_human_horizon == 3 and env.pibt_human_weight == 2
        env.rollout_pibt(8)
        for bad in (0, 9, -1):
            assert L.mapf_set_pibt_human_horizon(env.h, bad) == -1
            assert L.mapf_get_pibt_human_horizon(env.h) == 3, bad
        env.reset_seeded(maps)
        assert env.pibt_human_horizon == 3                      # a reset leaves the horizon alone
        env.set_state(clock=env.get_state()["clock"])
        assert env.pibt_human_horizon == 3                      # and so does mapf_set_state
        env.set_pibt_human_weight(1)
        env.set_pibt_human_weight(2)
        assert env.pibt_human_horizon == 3                      # and so does the weight's setter
        env.set_pibt_human_horizon(1)
        assert env.pibt_human_horizon == 1 and env.pibt_human_weight == 2
        env.reset_seeded(maps)
        twin.reset_seeded(maps)
        a = rollouts_equal(env, twin, T)
        ref1 = oracle_run(name, 2, 5, 1)[0]                     # and the twin's run is horizon 1's restatement
        check_actions("horizon 1 twin", ref1, 0, a, [(q, q) for q in range(T)])
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("name", [G, C4])
def test_a_horizon_at_weight_0_changes_nothing(name):
    T = 24
    env, twin = env_of(0, 5, 5)(name)[0], env_of(None)(name)[0]
    try:
        assert env.pibt_human_horizon == 5 and env.pibt_human_weight == 0
        a = rollouts_equal(env, twin, T)
        for _ in range(4):                                      # and the per-step pick
            assert torch.equal(env.pibt_actions().clone(), twin.pibt_actions())
            env.step(env.actions)
            twin.step(twin.actions)
        ref0 = oracle_run(name, 0, 5, 1)[0]
        check_actions("weight 0 twin", ref0, 0, a, [(q, q) for q in range(T)])
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 5. a switch between launches
@pytest.mark.parametrize("name", [DENSE, C4])
def test_horizon_set_between_launches_takes_effect_at_the_next_one(name):
    """Launch 1 (1 step) at horizon 1, launches 2 and 3 at horizon 3, weight 2 throughout; the reference
    switches at the same step and keeps its ages, as the handle does."""
    ref, state, stats = oracle_run(name, 2, 5, 3, switch=LAUNCHES[0])
    assert stats["differ"] >= 100, stats
    first = oracle_run(name, 2, 5, 1)[0]
    assert np.array_equal(ref["actions"][0], first["actions"][0])            # step 0 is horizon 1's
    env = env_of(2)(name)[0]
    try:
        t0 = 0
        for n_launch, T in enumerate(LAUNCHES):
            if n_launch == 1:
                env.set_pibt_human_horizon(3)
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


# ------------------------------------------------------------------ 6. the plan text
@pytest.mark.parametrize("name", [G, C4])
def test_plan_text_names_the_horizon_and_keeps_the_kernel(name):
    env = env_of(None)(name)[0]
    try:
        for slots in (False, True):
            never = env.rollout_pibt_plan(slots)
            kname = env.rollout_pibt_kernel_name(slots)
            env.set_pibt_human_horizon(3)
            assert env.rollout_pibt_plan(slots) == never                    # weight 0: nothing is added
            env.set_pibt_human_weight(2)
            text = env.rollout_pibt_plan(slots)
            assert text == never + " human_weight=2 human_horizon=3", (text, never)
            assert env.rollout_pibt_kernel_name(slots) == kname
            assert "human_horizon" not in env.rollout_plan(slots) and "human_horizon" not in env.rollout_descent_plan(slots)
            env.set_pibt_human_horizon(1)
            assert env.rollout_pibt_plan(slots) == never + " human_weight=2"
            env.set_pibt_human_weight(0)
            assert env.rollout_pibt_plan(slots) == never
    finally:
        env.close()


# ------------------------------------------------------------------ 7. capture
def test_captured_rollout_keeps_the_horizon_of_its_capture():
    """H.captured_rollout_case's two replays of a launch captured at horizon 3: the handle's horizon is set
    to 1 right after the launch is recorded (the handle's rollout is wrapped to do so), and both replays
    stay horizon 3's."""
    ref, state = assert_inputs(C4, *K3)

    def make(name, tuning=None, **kw):
        made = env_of(*K3)(name, tuning, **kw)
        env = made[0]
        rollout = env.rollout

        def capturing(T, policy, **kw2):
            r = rollout(T, policy, **kw2)                       # recorded, not run
            env.set_pibt_human_horizon(1)                       # the graph keeps horizon 3
            return r
        env.rollout = capturing
        return made
    H.captured_rollout_case("pibt", make, ref, state, allow=())


# ------------------------------------------------------------------ 8. the other entry points at horizon 3
def test_packed_observations_at_horizon_3_equal_the_floats():
    from mapf_amd.env import unpack_obs
    T = 24
    ref, state = assert_inputs(G, *K3)
    env = env_of(*K3)(G)[0]
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


def test_demo_runner_sets_the_horizon_once():
    from mapf_amd.imitation import DemoRunner
    T = 24
    env = env_of(None)(G)[0]
    twin = env_of(*K3)(G)[0]
    try:
        demo = DemoRunner(env, T, policy="pibt", human_weight=2, human_horizon=3)
        assert env.pibt_human_weight == 2 and env.pibt_human_horizon == 3
        demo.run()
        acts = H.action_buffer(twin, T)
        twin.rollout(T, "pibt", slots=True, actions=acts, **slot_buffers(twin, T))
        torch.cuda.synchronize()
        assert torch.equal(demo.expert_actions, acts)
        ref = assert_inputs(G, *K3)[0]
        check_actions("demo", ref, 0, demo.expert_actions, [(q, q) for q in range(T)])
        with pytest.raises(ValueError, match="human_horizon"):
            DemoRunner(env, T, policy="descent", human_horizon=3)
    finally:
        env.close()
        twin.close()


def test_device_runner_labels_its_states_with_the_horizon_expert():
    """DeviceRunner(expert="pibt", expert_human_weight=2, expert_human_horizon=3) sets both once:
    expert_actions[t] are the picks of a twin set by hand and driven through the runner's own actions, and
    they are not all horizon 1's (a twin at horizon 1 on the same states labels some agent-steps differently)."""
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
    own, twin, near = env(), env(), env()
    try:
        runner = DeviceRunner(own, model, n_steps=T, seed=5, expert="pibt", expert_human_weight=2, expert_human_horizon=3)
        assert own.pibt_human_weight == 2 and own.pibt_human_horizon == 3
        runner.run()
        twin.set_pibt_human_weight(2)
        twin.set_pibt_human_horizon(3)
        near.set_pibt_human_weight(2)
        differ = 0
        for t in range(T):
            label = twin.pibt_actions().clone()
            assert torch.equal(runner.expert_actions[t], label), t
            differ += int((near.pibt_actions() != label).sum())
            a = runner.actions[t].int().contiguous()
            twin.step(a)
            near.step(a)
        print(f"{differ} of {T * 16 * 8} labels differ from horizon 1's on the same states")
        assert differ > 0
        with pytest.raises(ValueError, match="expert_human_horizon"):
            DeviceRunner(own, model, n_steps=T, expert="descent", expert_human_horizon=3)
    finally:
        for e in (own, twin, near):
            e.close()
