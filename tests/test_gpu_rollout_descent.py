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
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from descent_ref import descent_actions
from kernel_registry import COVERED, record_rollout_kernel
from oracle import oracle as O
from test_gpu_parity import (FUSED_CASES, GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, WIDE_SHAPES, assert_no_errors,
                             build_maps, host, mk_env)
from test_gpu_rollout_band import host_skip, set_sentinels
from test_gpu_rollout_tape import OUT_KEYS, check_slots, check_state, preset_envs, slot_buffers

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 23, 40)                       # steps per launch, in this order: 64 steps
DESCENT_COVERED = set()                      # kernel names this file compared against the oracle
CASES = {**FUSED_CASES, **GROUP_CASES, **ROLLOUT_CASES, **RANDOM_CASES, **WIDE_SHAPES}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def covered(kname, what):
    assert kname.endswith(",descent>"), kname
    DESCENT_COVERED.add(kname)
    record_rollout_kernel(kname, what)


def case_setup(name):
    case = CASES[name]
    maps, shared = build_maps(case, case["B"], np.random.default_rng(5))
    return case, maps, shared, 0xDE5C0000 + len(name)


def case_env(name, tuning=None, **kw):
    case, maps, shared, seed = case_setup(name)
    env = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 use_da=case.get("da", 0), use_hp=case.get("hp", 0), human_mode=case.get("human", "random"),
                 goal_mode="random", fix_choice=1, shared_map=shared, seed=seed, env_offset=7, tuning=tuning, **kw)
    env.reset_seeded(maps)
    return env, case, maps, shared, seed


@functools.lru_cache(maxsize=None)
def oracle_run(name, steps):
    """The oracle under the restated policy, computed once and shared (read-only): the actions,
    per-step outputs / observations / vectors [steps, B, ...], and the state (cells, goals, human,
    BFS maps, the oracle's error count) after every launch of every path."""
    case, maps, shared, seed = case_setup(name)
    B, n = case["B"], case["n"]
    cfg = O.make_config(case["H"], case["W"], n, case["fov"], case["nch"], use_da=case.get("da", 0),
                        use_hp=case.get("hp", 0), human_mode={"random": 1, "looping": 0}[case.get("human", "random")],
                        goal_mode=1, fix_choice=1, seed=seed, env_offset=7)
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 25)) | {steps}
    ref = {k: [] for k, _ in OUT_KEYS}
    ref.update(obs=[], vec=[], actions=[])
    state = {}
    oracles = []
    for b in range(B):
        oe = O.OracleEnv(cfg, env_id=7 + b)
        oe.reset_random(maps if shared else maps[b])
        oracles.append(oe)
    for t in range(steps):
        row = {k: [] for k in ref}
        for b, oe in enumerate(oracles):
            a = descent_actions(oe.bfs(), oe.agents()[0], t)
            o = oe.step(a)
            oo, ov = oe.observe()
            for k, key in OUT_KEYS:
                row[k].append(np.array(o[key]))
            row["obs"].append(oo)
            row["vec"].append(ov)
            row["actions"].append(a)
        for k in ref:
            ref[k].append(np.stack(row[k]))
        if t + 1 in bounds:
            state[t + 1] = dict(pos=np.stack([oe.agents()[0] for oe in oracles]),
                                goal=np.stack([oe.agents()[1] for oe in oracles]),
                                hpos=np.stack([oe.human()["pos"] for oe in oracles]),
                                hgoal=np.stack([oe.human()["goal"] for oe in oracles]),
                                bfs=np.stack([oe.bfs() for oe in oracles]),
                                errors=sum(oe.errors() for oe in oracles))
    ref = {k: np.stack(v) for k, v in ref.items()}
    for v in ref.values():
        v.setflags(write=False)
    return ref, state


def assert_goals_change(name, ref, launches):
    """The condition on the inputs: >= 20 goal changes in the run, >= 10 of them before the last
    step of their launch (a map rebuilt at a launch's last step is first read by the next launch)."""
    per_step = ref["goals_reached"].reshape(len(ref["goals_reached"]), -1).sum(1)
    total = int(np.sum(launches))
    last = set((np.cumsum(launches) - 1).tolist())
    inner = sum(int(per_step[t]) for t in range(total) if t not in last)
    print(f"{name}: {int(per_step[:total].sum())} goal changes in {total} steps, {inner} before a launch's last step")
    assert int(per_step[:total].sum()) >= 20 and inner >= 10, (name, int(per_step[:total].sum()), inner)


def check_actions(what, ref, t0, actions, slots):
    a = actions.cpu().numpy()
    for k, dt in slots:
        assert np.array_equal(a[k], ref["actions"][t0 + dt]), f"{what} t={t0 + dt}: chosen actions"


def run_descent_case(name, path, tuning=None, launches=LAUNCHES, expect=None):
    """path "rollout": [T]-slot buffers, every slot compared; "inplace": the [B]-leading buffers, each
    launch's last step compared; "inplace1": one-step launches in place, every step compared."""
    total = int(np.sum(launches))
    ref, state = oracle_run(name, total)
    assert_goals_change(name, ref, launches)
    if path == "inplace1":
        launches = (1,) * 24
    elif path == "inplace":
        launches = launches[1:]
    env, case, _, _, _ = case_env(name, tuning)
    try:
        slots = path == "rollout"
        kname = env.rollout_descent_kernel_name(slots=slots)
        plan = env.rollout_descent_plan(slots=slots)
        assert kname.endswith(",descent>"), plan
        assert kname.replace(",descent>", ">") == env.rollout_kernel_name(slots=slots), (plan, env.rollout_plan(slots))
        if kname.startswith("rollout_wide3"):
            assert " bfsobs=0 " in plan, plan       # the stepping wave searches the maps it reads
        if expect is not None:
            assert kname == expect, plan
        t0 = 0
        for T in launches:
            k = T if slots else 1
            buf = slot_buffers(env, k)
            acts = torch.full((k, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
            env.rollout_descent(T, slots=slots, actions=acts, **buf)
            got = host(buf["out"])
            what = f"{name} {path} launch [{t0}, {t0 + T})"
            which = [(q, q) for q in range(T)] if slots else [(0, T - 1)]
            check_actions(what, ref, t0, acts, which)
            check_slots(what, ref, t0, got, buf["obs"], buf["vec"], which)
            t0 += T
            check_state(env, state[t0], what)
        # agents that ignore each other may box one another in (counters 1, 2): the oracle counts
        # the same events, and nothing else is ever counted
        assert_no_errors(env, allow=(1, 2))
        assert int(env.counters()[:8].sum()) == state[t0]["errors"]
        covered(kname, f"{name} {path} descent vs oracle")
    finally:
        env.close()


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
    """rollout_launcher(policy="descent") on NaN-prefilled slot buffers: call 1 stores everything;
    calls 2 and 3 carry MAPF_SLOTS_BAND_CLEAN and leave exactly mapf_obs_band_skip's floats alone
    (sentinels survive there, every other float and output equals an unflagged twin's)."""
    name, T = "g_n8_20x20_f11", 23
    env, case, _, _, seed = case_env(name, form)
    twin = case_env(name, form)[0]
    try:
        assert env.rollout_descent_kernel_name(slots=True, band_clean=True) == "rollout_random_kernel<true,%d,band64,descent>" % subs
        acts = torch.full((T, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        roll = dict(actions=acts, **slot_buffers(env, T))
        launch = env.rollout_launcher(T, slots=True, actions=acts, obs=roll["obs"], vec=roll["vec"], out=roll["out"],
                                      policy="descent")
        for call in range(3):
            if call:
                set_sentinels(roll)
            launch()
            ref = slot_buffers(twin, T)
            ref_acts = torch.full_like(acts, -9)
            twin.rollout_descent(T, slots=True, actions=ref_acts, **ref)
            torch.cuda.synchronize()
            want = ref["obs"].clone()
            if call:
                skip = torch.from_numpy(host_skip(env, case, roll, True)).to(env.device)
                want.view(skip.shape)[skip] = 7.0
            assert torch.equal(roll["obs"].view(torch.int32), want.view(torch.int32)), f"call {call}: obs"
            assert torch.equal(roll["vec"].view(torch.int32), ref["vec"].view(torch.int32)), f"call {call}: vec"
            assert torch.equal(acts, ref_acts), f"call {call}: actions"
            for key in ref["out"]:
                assert torch.equal(roll["out"][key], ref["out"][key]), f"call {call}: {key}"
        assert_no_errors(env, allow=(1, 2))
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 6. capture
def test_captured_descent_rollout_continues_the_episode():
    """One rollout_descent launch of the c4 shape (the three-wave form) captured into a graph and
    replayed twice: 2T steps of the episode, every slot of both replays against the oracle."""
    name, T = "c4_40x40_n16_f9_looping", 12
    ref, state = oracle_run(name, int(np.sum(LAUNCHES)))
    env, case, _, _, _ = case_env(name)
    g = None
    try:
        assert env.rollout_descent_kernel_name(slots=True) == "rollout_wide3_kernel<u64,1,true,descent>"
        buf = slot_buffers(env, T)
        acts = torch.full((T, case["B"], case["n"]), -9, dtype=torch.int32, device=env.device)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                env.rollout_descent(T, slots=True, actions=acts, **buf)       # recorded, not run
        torch.cuda.synchronize()
        for call in range(2):
            g.replay()
            torch.cuda.synchronize()
            which = [(q, q) for q in range(T)]
            check_actions(f"replay {call}", ref, call * T, acts, which)
            check_slots(f"replay {call}", ref, call * T, host(buf["out"]), buf["obs"], buf["vec"], which)
        check_state(env, state[2 * T], "after two replays")
        assert_no_errors(env, allow=(1, 2))
    finally:
        del g
        env.close()


# ------------------------------------------------------------------ 7. errors
def test_keep_bfs_off_is_a_state_error_and_T0_is_a_no_op():
    from mapf_amd import _lib
    from mapf_amd.env import _ptr, _stream
    env, case, _, _, _ = case_env("r_n6_16x16_f9_dahp")
    off = case_env("r_n6_16x16_f9_dahp", keep_bfs=False)[0]
    try:
        before = env.get_state()
        env.rollout_descent(0)
        assert _lib.lib().mapf_rollout_descent(env.h, 0, 0, _ptr(env.actions), ctypes.byref(env._stepout), _ptr(env.obs),
                                               _ptr(env.vec), _stream(env.device)) == 0
        torch.cuda.synchronize()
        after = env.get_state()
        for key in before:
            np.testing.assert_array_equal(before[key], after[key])
        L = _lib.lib()
        assert L.mapf_descent_actions(off.h, _ptr(off.actions), _stream(off.device)) == -4
        assert L.mapf_rollout_descent(off.h, 4, 0, _ptr(off.actions), ctypes.byref(off._stepout), _ptr(off.obs),
                                      _ptr(off.vec), _stream(off.device)) == -4
        with pytest.raises(RuntimeError, match="keep_bfs"):
            off.descent_actions()
        with pytest.raises(RuntimeError, match="keep_bfs"):
            off.rollout_descent(4)
    finally:
        env.close()
        off.close()


# ------------------------------------------------------------------ 8. record and replay of fixed episodes
G6 = os.path.join(os.path.dirname(__file__), "golden", "g6_episodes")


@pytest.mark.parametrize("mtype,da_hp", [(0, False), (1, True)])
def test_descent_policy_on_fixed_episodes_replays(mtype, da_hp):
    """evaluate_fixed_episodes under descent_policy(), recording its actions, then
    replay_fixed_episodes over the tapes: integer metrics equal, the float64 sums of float32 terms
    within 1e-9 relative (summation order only).  The baseline reaches goals on these episodes."""
    from mapf_amd.episodes import (METRIC_KEYS, descent_policy, evaluate_fixed_episodes, load_fixed_episode_infos,
                                   replay_fixed_episodes)
    infos = load_fixed_episode_infos(G6)
    steps = 48
    kw = dict(num_channel=6, fov=9, use_da=da_hp, use_hp=da_hp, human_movement_type=mtype, fix_choice=1)
    with pytest.raises(RuntimeError, match="keep_bfs=True"):
        evaluate_fixed_episodes(infos, descent_policy(), max_steps=1, **kw)
    got, tapes = evaluate_fixed_episodes(infos, descent_policy(), max_steps=steps, record_actions=True, keep_bfs=True, **kw)
    rep = replay_fixed_episodes(infos, tapes, **kw)
    for key in METRIC_KEYS:
        if key in ("episodeReward", "episodeCostReward"):
            np.testing.assert_allclose(rep[key], got[key], rtol=1e-9, atol=0, err_msg=key)
        else:
            np.testing.assert_array_equal(rep[key], got[key], err_msg=key)
    assert got["totalGoals"].sum() > 0
    assert got["staticCollide"].sum() == 0


# ------------------------------------------------------------------ 9. coverage guard (last)
@pytest.mark.parametrize("cfg", ["c1", "c2", "c4", "c5"])
def test_default_descent_kernels_are_covered_by_this_file(cfg):
    from test_gpu_ycoverage import preset_env
    if not DESCENT_COVERED:
        pytest.fail("no oracle-compared descent case ran before the guard")
    env = preset_env(cfg)
    try:
        assert env.rollout_fused, cfg
        for slots in (False, True):
            name = env.rollout_descent_kernel_name(slots)
            assert name in DESCENT_COVERED and name in COVERED, (
                f"{cfg} slots={slots}: {env.rollout_descent_plan(slots)} is launched by default but no compared "
                f"case of this file ran it; covered: {sorted(DESCENT_COVERED)}")
    finally:
        env.close()
