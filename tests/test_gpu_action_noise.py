"""GPU: action noise on the picked policies' rollouts (mapf_set_action_noise, mapf_noise_actions; include/mapf.h).

The rollout kernels store the policy's pick -- the label -- and play, with probability noise_q16 / 65536, the
uniform random policy's action in its place.  The oracle has neither a policy nor noise: the numpy picks of
tests/descent_ref.py, tests/pibt_ref.py and tests/pibt_horizon_ref.py give the label, tests/explore_ref.py the
action played from the oracle's own Philox words, the oracle is stepped with `played`, and every slot is
compared bit for bit: actions_out with the labels, every step output, observation and vector and the state
after every launch with the oracle stepped with `played`.

Conditions on the inputs, asserted from the reference run alone before any device call: per case at least 50
agent-steps with played != label, for N >= 16 at least 10 of them on agents with index >= 8 (the second and later
draw groups), and the goal changes of the existing rollout files (a stale map can only show there).  The seeds
(SEED below) were chosen on the CPU so that the reference runs meet them.
"""
import functools

import numpy as np
import pytest
import torch

import explore_ref as X
import pibt_horizon_ref as PZ
import pibt_ref
import rollout_harness as H
from descent_ref import descent_actions
from kernel_registry import record_rollout_kernel
from rollout_harness import check_slots, check_state, slot_buffers
from test_gpu_parity import assert_no_errors, host
from test_gpu_rollout_pibt import CASES

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 23, 40)                       # steps per launch, in this order: 64 steps
Q16 = 16384                                  # eps = 0.25
SEED = 0xA0150000
R6, G, D16, C4, C5 = ("r_n6_16x16_f9_dahp", "g_n8_20x20_f11", "dense_12x12_n16_f9_dahp", "c4_40x40_n16_f9_looping",
                      "c5_80x80_n64_f11_bfsch")
GROUPED = dict(roll_occ=4, roll_group=1)
HUMAN = (2, 3)                               # (human weight, human horizon) of the weighted PIBT case
K64 = dict(k_predict=64)                     # 16 agents with the HP channel: no one-launch kernel


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def cfg_key(cfg):
    return tuple(sorted((cfg or {}).items()))


def env_of(q16=Q16, human=None, cfg=None):
    """The harness's env_of at action noise q16 (None: the setter is never called)."""
    def make(name, tuning=None, **kw):
        made = H.case_env(CASES, name, SEED, tuning, cfg=cfg, **kw)
        if human is not None:
            made[0].set_pibt_human_weight(human[0])
            made[0].set_pibt_human_horizon(human[1])
        if q16 is not None:
            made[0].set_action_noise(q16=q16)
        return made
    return make


BOUNDS = {1, 12, 23, 24, 63, 64}             # the steps after which some test below compares the state


def oracle_run(name, policy, human=None, cfg=None):
    """The oracle stepped with `played` at noise Q16, computed once per (case, policy, settings) and shared
    (read-only): H.oracle_rollout's (ref, state) with ref["labels"] the policy's picks and ref["actions"] what
    was played; 64 steps."""
    return _oracle_run(name, policy, human, cfg_key(cfg))


@functools.lru_cache(maxsize=None)
def _oracle_run(name, policy, human, cfg):
    case, _, _, seed = H.case_setup(CASES, name, SEED)
    steps, q16 = int(np.sum(LAUNCHES)), Q16
    n = case["n"]
    ages = [pibt_ref.Ages(n) for _ in range(case["B"])]

    def pick(oe, b, t, world):
        world = np.asarray(world, np.int8)
        if policy == "descent":
            label = descent_actions(oe.bfs(), oe.agents()[0], t)
        elif human is None:
            pos, goal = oe.agents()
            hum = oe.human()
            label = pibt_ref.pibt_actions(world, oe.bfs(), pos, goal, hum["pos"], hum["next"], t, ages[b])[0]
        else:
            label = PZ.pibt_actions(world, oe, t, ages[b], human[0], 5, human[1])[0]
        label = np.asarray(label, np.int32)
        return X.played(label, 7 + b, t, seed, q16), dict(labels=label)
    return H.oracle_rollout(CASES, name, SEED, steps, {b for b in BOUNDS if b <= steps}, pick, cfg=dict(cfg) or None)


def assert_inputs(name, policy, human=None, launches=LAUNCHES, cfg=None, goals=True):
    """The per-case conditions over the steps the launches play, from the reference run alone."""
    steps = int(np.sum(launches))
    ref, state = oracle_run(name, policy, human, cfg)
    assert steps <= len(ref["labels"])
    differ = ref["actions"][:steps] != ref["labels"][:steps]
    late = int(differ[:, :, 8:].sum())
    print(f"{name} {policy}: played != label in {int(differ.sum())} agent-steps, {late} of them on agents >= 8; "
          f"oracle errors {state[steps]['errors']}")
    assert int(differ.sum()) >= 50, (name, policy, int(differ.sum()))
    if CASES[name]["n"] >= 16:
        assert late >= 10, (name, policy, late)
    if goals:
        H.assert_goals_change(name, {k: v[:steps] for k, v in ref.items()}, launches)
    return ref, state


def check_labels(what, ref, t0, actions, slots):
    a = actions.cpu().numpy()
    for k, dt in slots:
        assert np.array_equal(a[k], ref["labels"][t0 + dt]), f"{what} t={t0 + dt}: actions_out is not the label"


def run_noise_case(policy, name, path, launches=LAUNCHES, tuning=None, expect=None, human=None, cfg=None, bits=False):
    """rollout_harness.run_policy_case with actions_out compared with the labels: path "rollout" ([T]-slot
    buffers, every slot compared) or "inplace" (the [B]-leading buffers, each launch's last step compared).
    bits: packed observations, unpacked for the comparison."""
    from mapf_amd.env import unpack_obs
    ref, state = assert_inputs(name, policy, human, launches, cfg)
    if path == "inplace":
        launches = launches[1:]
    env, case, _, _, _ = env_of(human=human, cfg=cfg)(name, tuning)
    try:
        slots = path == "rollout"
        plan = env.rollout_plan(slots=slots, obs_bits=bits, policy=policy)
        kname = env.rollout_kernel_name(slots=slots, obs_bits=bits, policy=policy)
        assert plan.endswith(f" noise={Q16}"), plan
        assert not env.rollout_kernel or kname.endswith(",noise>"), plan       # an instantiation of its own
        if expect is not None:
            assert kname == expect, plan
        t0 = 0
        for T in launches:
            k = T if slots else 1
            buf, acts = slot_buffers(env, k), H.action_buffer(env, k)
            obs = buf["obs"]
            if bits:
                obs = torch.full((k, env.B, env.N, env.obs_words), -1, dtype=torch.int32, device=env.device)
            env.rollout(T, policy, slots=slots, actions=acts, obs=obs, vec=buf["vec"], out=buf["out"], obs_bits=bits)
            what = f"{name} {policy} {path} launch [{t0}, {t0 + T})"
            which = [(q, q) for q in range(T)] if slots else [(0, T - 1)]
            check_labels(what, ref, t0, acts, which)
            check_slots(what, ref, t0, host(buf["out"]), unpack_obs(obs, env.C, env.F) if bits else obs, buf["vec"], which)
            t0 += T
            check_state(env, state[t0], what)
        assert_no_errors(env, allow=(1, 2))
        assert int(env.counters()[:8].sum()) == state[t0]["errors"]       # exactly as the oracle's
        if env.rollout_kernel:
            record_rollout_kernel(kname, f"{name} {path} {policy} at noise {Q16} vs oracle")
    finally:
        env.close()


# ------------------------------------------------------------------ 1. every route and form against the oracle
ROLL_CASES = [
    ("descent", R6, "rollout", None, None, LAUNCHES, "rollout_random_kernel<true,1,descent,noise>"),     # B = 37 ragged, lanes past N
    ("pibt", R6, "rollout", None, None, LAUNCHES, "rollout_random_kernel<true,1,pibt,noise>"),
    ("pibt", G, "rollout", GROUPED, None, LAUNCHES, "rollout_random_kernel<true,4,pibt,noise>"),         # grouped pair-lane
    ("pibt", G, "inplace", GROUPED, None, LAUNCHES, "rollout_random_kernel<false,4,pibt,noise>"),
    ("pibt", G, "rollout", None, HUMAN, LAUNCHES, "rollout_random_kernel<true,1,pibt,noise>"),           # human weight 2, horizon 3
    ("descent", D16, "rollout", None, None, LAUNCHES, None),                                       # one wave per env, two draw groups
    ("pibt", D16, "rollout", None, None, LAUNCHES, None),
    ("descent", C4, "rollout", None, None, LAUNCHES, "rollout_wide3_kernel<u64,1,true,descent,noise>"),  # three waves per env
    ("descent", C4, "inplace", None, None, LAUNCHES, "rollout_wide3_kernel<u64,1,false,descent,noise>"),
    ("pibt", C4, "rollout", None, None, LAUNCHES, "rollout_wide3_kernel<u64,1,true,pibt,noise>"),
    ("pibt", C4, "inplace", None, None, LAUNCHES, "rollout_wide3_kernel<u64,1,false,pibt,noise>"),
    # N = 64: eight draw groups, C = 7 (3 envs: 24 steps change 5 goals, the condition needs the 64)
    ("pibt", C5, "rollout", None, None, LAUNCHES, "rollout_wide_kernel<Row2,2,true,pibt,noise>"),
]


@pytest.mark.parametrize("policy,name,path,tuning,human,launches,expect", ROLL_CASES)
def test_noisy_rollout_matches_the_oracle_stepped_with_played(policy, name, path, tuning, human, launches, expect):
    run_noise_case(policy, name, path, launches, tuning, expect, human)


def test_noisy_rollout_with_packed_observations_matches_the_oracle():
    run_noise_case("pibt", G, "rollout", LAUNCHES, GROUPED, "rollout_random_kernel<true,4,bits,pibt,noise>", bits=True)


def test_noisy_rollout_without_a_one_launch_form_matches_the_oracle():
    """16 agents with the HP channel and k_predict = 64: T x (pibt_actions, the noise launch into the handle's
    row, step_observe), issued by mapf_rollout_pibt itself."""
    env = env_of(cfg=K64)(D16)[0]
    try:
        assert not env.rollout_fused and env.rollout_pibt_plan(True) == f"pibt_actions+step_observe noise={Q16}"
    finally:
        env.close()
    run_noise_case("pibt", D16, "rollout", LAUNCHES, cfg=K64)


def test_noisy_sparse_rollouts_over_the_same_buffers_match_the_oracle():
    """mapf_rollout_sparse, two launches of 12 steps on the same zero-filled buffers: the second stores only the
    pieces that change, and every byte is the oracle's."""
    T = 12
    ref, state = assert_inputs(G, "pibt", launches=(T, T), goals=False)
    env = env_of()(G, GROUPED)[0]
    try:
        buf, acts = slot_buffers(env, T, fill=0.0), H.action_buffer(env, T)
        plan = env.rollout_sparse_plan(buf["obs"], "pibt")
        assert plan.split(" ")[0] == "rollout_random_kernel<true,4,sparse64,pibt,noise>" and plan.endswith(f" noise={Q16}"), plan
        shadow = torch.zeros((T, env.B, 16), dtype=torch.int32, device=env.device)
        which = [(q, q) for q in range(T)]
        for call in range(2):
            env.rollout_sparse(T, "pibt", shadow=shadow, valid=call * T, actions=acts, **buf)
            what = f"sparse launch {call}"
            check_labels(what, ref, call * T, acts, which)
            check_slots(what, ref, call * T, host(buf["out"]), buf["obs"], buf["vec"], which)
            check_state(env, state[(call + 1) * T], what)
        assert_no_errors(env, allow=(1, 2))
        assert int(env.counters()[:8].sum()) == state[2 * T]["errors"]       # exactly as the oracle's
        record_rollout_kernel(plan.split(" ")[0], f"{G} sparse pibt at noise {Q16} vs oracle")
    finally:
        env.close()


# ------------------------------------------------------------------ 2. the setting itself
def test_setter_getter_and_what_leaves_the_setting_alone():
    from mapf_amd import _lib
    env, _, maps, _, _ = env_of(None)(G)
    try:
        L = _lib.lib()
        assert env.action_noise == 0 and L.mapf_get_action_noise(env.h) == 0          # mapf_create's default
        plain = env.rollout_pibt_plan(True)
        assert ",pibt> " in plain
        env.set_action_noise(0.25)
        assert env.action_noise == 16384
        for bad in (-1, 65537, 1 << 30):
            assert L.mapf_set_action_noise(env.h, bad) == -1
            assert L.mapf_get_action_noise(env.h) == 16384, bad
        assert env.rollout_pibt_plan(True) == plain.replace(",pibt> ", ",pibt,noise> ") + " noise=16384"
        assert env.rollout_descent_plan(False).endswith(" noise=16384")
        assert env.rollout_perf_plan("pibt").endswith(" noise=16384") and env.rollout_perf_plan("descent").endswith(" noise=16384")
        for policy in ("random", "tape"):                                             # they ignore it: same text
            assert "noise" not in env.rollout_plan(True, policy=policy) and "noise" not in env.rollout_perf_plan(policy)
        env.set_pibt_human_weight(2)
        env.set_pibt_human_horizon(3)
        assert env.rollout_pibt_plan(True).endswith(" human_weight=2 human_horizon=3 noise=16384")
        env.reset_seeded(maps)
        assert env.action_noise == 16384                                              # a reset leaves it alone
        env.set_state(clock=env.get_state()["clock"])
        assert env.action_noise == 16384                                              # and so does mapf_set_state
        env.set_action_noise(q16=65536)
        assert env.action_noise == 65536
        env.set_action_noise(0)
        assert env.action_noise == 0 and env.rollout_pibt_plan(True) == plain + " human_weight=2 human_horizon=3"
        env.rollout(2, "pibt", noise=0.05)                                            # noise= sets it before the launch
        assert env.action_noise == 3277
        env.rollout_perf(2, "descent", noise=None)                                    # None leaves it alone
        assert env.action_noise == 3277
    finally:
        env.close()


def test_noise_actions_is_the_rule_at_the_envs_clocks_and_may_work_in_place():
    case, _, _, seed = H.case_setup(CASES, D16, SEED)
    env = env_of(None)(D16)[0]
    try:
        rng = np.random.default_rng(3)
        for t in range(3):
            lab = rng.integers(0, 5, (env.B, env.N)).astype(np.int32)
            labels = torch.from_numpy(lab).to(env.device)
            env.set_action_noise(q16=0)
            assert torch.equal(env.noise_actions(labels), labels)                     # a copy at 0
            for q16 in (1, Q16, 65535, 65536):
                env.set_action_noise(q16=q16)
                want = np.stack([X.played(lab[b], 7 + b, t, seed, q16) for b in range(env.B)])
                got = env.noise_actions(labels)
                assert np.array_equal(got.cpu().numpy(), want), (t, q16)
                assert torch.equal(labels.cpu(), torch.from_numpy(lab))               # the labels are only read
            same = labels.clone()
            assert env.noise_actions(same, out=same) is same and np.array_equal(same.cpu().numpy(), want)
            assert torch.equal(env.noise_actions(labels), env.random_actions())       # 65536: the random policy's
            env.step_observe(env.random_actions())
    finally:
        env.close()


def test_noise_actions_before_a_reset_is_a_state_error():
    from mapf_amd import _lib
    from mapf_amd.env import BatchedMapfGym, _ptr, _stream
    from mapf_amd.config import make_config
    env = BatchedMapfGym(make_config(2, 8, 8, num_agents=2, fov=5, num_channel=6, keep_bfs=True))
    try:
        a = torch.zeros(2, 2, dtype=torch.int32, device=env.device)
        assert _lib.lib().mapf_noise_actions(env.h, _ptr(a), _ptr(a), _stream(env.device)) == -4
        assert _lib.lib().mapf_noise_actions(env.h, None, _ptr(a), _stream(env.device)) == -1
    finally:
        env.close()


# ------------------------------------------------------------------ 3. identities on twin handles
T24 = 24


def roll(env, T, policy, **kw):
    buf, acts = slot_buffers(env, T), H.action_buffer(env, T)
    env.rollout(T, policy, slots=True, actions=acts, **buf, **kw)
    torch.cuda.synchronize()
    return buf, acts


def assert_equal_rollouts(a, b, what, actions=True):
    (ba, aa), (bb, ab) = a, b
    if actions:
        assert torch.equal(aa, ab), f"{what}: actions"
    assert torch.equal(ba["obs"].view(torch.int32), bb["obs"].view(torch.int32)), f"{what}: obs"
    assert torch.equal(ba["vec"].view(torch.int32), bb["vec"].view(torch.int32)), f"{what}: vec"
    for key in ba["out"]:
        assert torch.equal(ba["out"][key], bb["out"][key]), f"{what}: {key}"


def assert_same_state(a, b, what):
    sa, sb = a.get_state(), b.get_state()
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{what}: state {key}")
    assert torch.equal(a.bfs(), b.bfs()), f"{what}: bfs"
    np.testing.assert_array_equal(a.counters()[:8], b.counters()[:8], err_msg=f"{what}: counters")   # (past 8: work-list counts of the per-step route)
    assert torch.equal(a.pibt_actions(), b.pibt_actions()), f"{what}: the next pibt pick (the ages)"


@pytest.mark.parametrize("name", [G, D16])
@pytest.mark.parametrize("policy", ["descent", "pibt"])
def test_noise_0_is_a_handle_that_never_called_the_setter(name, policy):
    env, twin = env_of(None)(name)[0], env_of(None)(name)[0]
    try:
        env.set_action_noise(0.5)
        env.set_action_noise(0)
        assert_equal_rollouts(roll(env, T24, policy), roll(twin, T24, policy), f"{name} {policy}")
        assert_same_state(env, twin, f"{name} {policy}")
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("name", [G, D16])
def test_noise_65536_plays_the_random_policy_and_labels_the_states_it_reaches(name):
    env, rnd, step = (env_of(None)(name)[0] for _ in range(3))
    try:
        got = roll(env, T24, "pibt", noise=1.0)
        assert env.action_noise == 65536
        want = roll(rnd, T24, "random")
        assert_equal_rollouts(got, want, f"{name} everything but actions_out", actions=False)
        for t in range(T24):            # the labels: what a per-step pibt_actions twin picks on those states
            assert torch.equal(got[1][t], step.pibt_actions()), f"{name} t={t}: label"
            step.step_observe(want[1][t].contiguous())
        sa, sb = env.get_state(), rnd.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
    finally:
        for e in (env, rnd, step):
            e.close()


@pytest.mark.parametrize("name", [G, D16])
def test_per_step_calls_and_two_chunks_equal_one_launch(name):
    """T x (pibt_actions, noise_actions, step_observe), and 8 + 16 steps in two launches, against 24 in one."""
    one, steps, two = (env_of()(name)[0] for _ in range(3))
    try:
        want = roll(one, T24, "pibt")
        for t in range(T24):
            label = steps.pibt_actions().clone()
            out, obs, vec = steps.step_observe(steps.noise_actions(label))
            assert torch.equal(label, want[1][t]), f"t={t}: label"
            assert torch.equal(obs.view(torch.int32), want[0]["obs"][t].view(torch.int32)), f"t={t}: obs"
            assert torch.equal(vec.view(torch.int32), want[0]["vec"][t].view(torch.int32)), f"t={t}: vec"
            for key in out:
                assert torch.equal(out[key], want[0]["out"][key][t]), f"t={t}: {key}"
        assert_same_state(one, steps, f"{name} per step")
        a, b = roll(two, 8, "pibt"), roll(two, 16, "pibt")
        for part, t0, T in ((a, 0, 8), (b, 8, 16)):
            assert torch.equal(part[1], want[1][t0:t0 + T]), f"chunk at {t0}: labels"
            assert torch.equal(part[0]["obs"].view(torch.int32), want[0]["obs"][t0:t0 + T].view(torch.int32)), f"chunk at {t0}: obs"
            for key in part[0]["out"]:
                assert torch.equal(part[0]["out"][key], want[0]["out"][key][t0:t0 + T]), f"chunk at {t0}: {key}"
        assert_same_state(one, two, f"{name} 8 + 16")
    finally:
        for e in (one, steps, two):
            e.close()


# ------------------------------------------------------------------ 4. rollout_perf
@pytest.mark.parametrize("name,cfg,kind", [(G, None, 1), (D16, None, 2), (D16, K64, 0)])
@pytest.mark.parametrize("policy", ["descent", "pibt"])
def test_noisy_rollout_perf_equals_the_slot_route_reduced_in_numpy(name, cfg, kind, policy):
    from test_gpu_rollout_perf import np_perf
    T = 24
    a, b, c = (env_of(cfg=cfg)(name)[0] for _ in range(3))
    try:
        assert a.rollout_kernel == kind
        plan = b.rollout_perf_plan(policy)
        assert plan.endswith(f" noise={Q16}"), plan
        assert (f",{policy},perf,noise>" in plan) if kind else plan.startswith(f"{policy}_actions+step+perf_accumulate"), plan
        buf, acts = roll(a, T, policy)
        want = np_perf(host(buf["out"]))
        got_acts = torch.full_like(acts, -9)
        got = b.rollout_perf(T, policy, actions=got_acts)
        assert np.array_equal(got.cpu().numpy(), want), f"{name} {policy}: {got.cpu().numpy()} != {want}"
        assert torch.equal(got_acts, acts), f"{name} {policy}: actions are the labels"
        assert_same_state(a, b, f"{name} {policy} perf")
        none = c.rollout_perf(T, policy)                     # no actions buffer: labels and played pass through scratch
        assert np.array_equal(none.cpu().numpy(), want), f"{name} {policy}: without an actions buffer"
        assert_same_state(a, c, f"{name} {policy} perf without actions")
    finally:
        for e in (a, b, c):
            e.close()


# ------------------------------------------------------------------ 5. capture
def test_captured_noisy_rollout_continues_the_episode_and_keeps_its_noise():
    """One launch of the c4 shape captured at noise 16384 and replayed twice: 2T steps of the oracle's episode.
    The setter called after the capture does not change the replays."""
    T = 12
    ref, state = oracle_run(C4, "pibt")
    env = env_of()(C4)[0]
    g = None
    try:
        assert env.rollout_kernel_name(slots=True, policy="pibt") == "rollout_wide3_kernel<u64,1,true,pibt,noise>"
        buf, acts = slot_buffers(env, T), H.action_buffer(env, T)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                env.rollout(T, "pibt", slots=True, actions=acts, **buf)       # recorded, not run
        torch.cuda.synchronize()
        env.set_action_noise(0)                                               # the graph keeps 16384
        for call in range(2):
            g.replay()
            torch.cuda.synchronize()
            which = [(q, q) for q in range(T)]
            check_labels(f"replay {call}", ref, call * T, acts, which)
            check_slots(f"replay {call}", ref, call * T, host(buf["out"]), buf["obs"], buf["vec"], which)
        check_state(env, state[2 * T], "after two replays")
        assert_no_errors(env, allow=(1, 2))
    finally:
        del g
        env.close()


# ------------------------------------------------------------------ 6. fixed evaluation episodes
def test_noisy_policy_on_fixed_episodes_equals_the_device_evaluator():
    from mapf_amd.episodes import (METRIC_KEYS, evaluate_fixed_episodes, evaluate_fixed_episodes_device,
                                   load_fixed_episode_infos, noisy_policy, pibt_policy)
    infos = load_fixed_episode_infos(H.G6)
    kw = dict(num_channel=6, fov=9, use_da=False, use_hp=False, human_movement_type=0, fix_choice=1, max_steps=48)
    want = evaluate_fixed_episodes(infos, noisy_policy(pibt_policy(), 0.25), keep_bfs=True, **kw)
    got = evaluate_fixed_episodes_device(infos, "pibt", noise=0.25, **kw)
    clean = evaluate_fixed_episodes_device(infos, "pibt", **kw)
    for key in METRIC_KEYS[2:]:                 # the six integer metrics
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    print({k: (clean[k].sum(), got[k].sum()) for k in METRIC_KEYS[2:]})
    assert any((clean[k] != got[k]).any() for k in METRIC_KEYS[2:])           # the noise was in force


# ------------------------------------------------------------------ 7. DemoRunner
@pytest.mark.parametrize("shape", ["pair-lane", "wide"])
def test_demo_runner_with_noise_keeps_the_alignment_and_the_experts_labels(shape):
    """Slot t holds the state the expert saw at step t (tests/test_gpu_imitation.py's alignment), on the noisy
    trajectory; expert_actions[t] is a per-step twin's pick there, not what was played."""
    from mapf_amd.imitation import DemoRunner
    from test_gpu_imitation import _env
    T = 6
    env, twin = _env(shape), _env(shape)
    try:
        demo = DemoRunner(env, n_steps=T, policy="pibt", obs_bits=False, noise=0.25)
        assert env.action_noise == 16384
        demo.run()
        twin.set_action_noise(0.25)
        differ = 0
        for t in range(T):
            o, v = twin.observe()
            assert torch.equal(demo.obs[t], o) and torch.equal(demo.vec[t], v), f"slot {t}"
            label = twin.pibt_actions().clone()
            assert torch.equal(demo.expert_actions[t], label), f"t={t}: the label"
            played = twin.noise_actions(label)
            differ += int((played != label).sum())
            twin.step_observe(played)
        o, v = twin.observe()
        assert torch.equal(demo.obs[T], o) and torch.equal(demo.vec[T], v), "slot T: after the last step"
        assert differ >= 10, differ                 # the trajectory left the expert's
    finally:
        env.close()
        twin.close()
