"""What test_gpu_rollout_tape.py, _descent.py and _pibt.py share: case construction, the oracle loop, the
bit-for-bit comparers, the case runner and the test bodies that differ in the policy's name alone (a key of
mapf_amd.env.ROLLOUT_POLICIES).  A plain module, no tests and no fixtures: a file passes its own CASES, seed
base and *_COVERED set."""
import ctypes
import os

import numpy as np
import pytest
import torch

from kernel_registry import COVERED, record_rollout_kernel
from oracle import oracle as O
from test_gpu_parity import assert_no_errors, build_maps, c5_maps, host, mk_env
from test_gpu_rollout_band import host_skip, set_sentinels

OUT_KEYS = [("status", "status"), ("reward", "reward"), ("cost", "cost"), ("train_valid", "valid"),
            ("actions_fixed", "fixed"), ("goals_reached", "goals"), ("constraints", "constr"), ("shadow_goals", "shadow")]
G6 = os.path.join(os.path.dirname(__file__), "golden", "g6_episodes")


# ------------------------------------------------------------------ cases
def case_setup(cases, name, seed_base):
    """(case, maps, shared, seed); map="sparse_shared": one shared random map with few obstacles."""
    case = cases[name]
    if case["map"] == "sparse_shared":
        from mapf_amd.maps import keep_largest_component, random_map
        m = random_map(np.random.default_rng(case["map_seed"]), case["H"], case["W"], 0.1)
        maps, shared = keep_largest_component(m), True
    else:
        maps, shared = build_maps(case, case["B"], np.random.default_rng(5))
    return case, maps, shared, seed_base + len(name)


def case_env(cases, name, seed_base, tuning=None, cfg=None, **kw):
    """cfg: config fields off their defaults (k_predict, penalty_radius, lifelong, the costs); the same
    dict goes to oracle_rollout, so that the device and the oracle cannot differ in them."""
    case, maps, shared, seed = case_setup(cases, name, seed_base)
    env = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 use_da=case.get("da", 0), use_hp=case.get("hp", 0), human_mode=case.get("human", "random"),
                 goal_mode="random", fix_choice=1, shared_map=shared, seed=seed, env_offset=7, tuning=tuning, **dict(cfg or {}),
                 **kw)
    env.reset_seeded(maps)
    return env, case, maps, shared, seed


def slot_buffers(env, k, fill=float("nan")):
    return dict(obs=torch.full((k,) + tuple(env.obs.shape), fill, device=env.device),
                vec=torch.full((k,) + tuple(env.vec.shape), fill, device=env.device),
                out={key: torch.full((k,) + tuple(v.shape), -7, dtype=v.dtype, device=env.device)
                     for key, v in env.out.items()})


def action_buffer(env, k):
    return torch.full((k, env.B, env.N), -9, dtype=torch.int32, device=env.device)


def preset_envs(cfg, count):
    """`count` twin handles of a BASELINE preset at its full per-GPU size, reset alike."""
    import bench
    from mapf_amd.maps import generate_warehouse
    p = bench.PRESETS[cfg]
    maps = generate_warehouse(p["size"], p["size"]) if p["maps"] == "warehouse" else c5_maps(p["envs"])
    envs = []
    for _ in range(count):
        e = mk_env(B=p["envs"], H=p["size"], W=p["size"], num_agents=p["agents"], fov=p["fov"],
                   num_channel=p["channels"], human_mode="random", goal_mode="random", fix_choice=1, seed=1234,
                   shared_map=p["maps"] == "warehouse")
        e.reset_seeded(maps)
        envs.append(e)
    return envs


# ------------------------------------------------------------------ the oracle
def oracle_rollout(cases, name, seed_base, steps, bounds, pick, cfg=None):
    """`steps` steps of the case on the CPU oracle, one OracleEnv per env (cfg: as case_env's).  pick(oe, b, t, maps_b) ->
    (actions of env b at step t, None or a dict of extras).  Returns (ref, state), read-only: ref[k] =
    [steps, B, ...] for the step outputs, "obs", "vec", "actions" and the extras; state[t] = cells,
    goals, human, BFS maps and the oracle's error count after t steps, for every t in `bounds`."""
    case, maps, shared, seed = case_setup(cases, name, seed_base)
    ocfg = O.make_config(case["H"], case["W"], case["n"], case["fov"], case["nch"], use_da=case.get("da", 0),
                         use_hp=case.get("hp", 0), human_mode={"random": 1, "looping": 0}[case.get("human", "random")],
                         goal_mode=1, fix_choice=1, seed=seed, env_offset=7, **dict(cfg or {}))
    oracles = []
    for b in range(case["B"]):
        oe = O.OracleEnv(ocfg, env_id=7 + b)
        oe.reset_random(maps if shared else maps[b])
        oracles.append(oe)
    rows, state = [], {}
    for t in range(steps):
        row = {}
        for b, oe in enumerate(oracles):
            a, extras = pick(oe, b, t, maps if shared else maps[b])
            o = oe.step(a)
            oo, ov = oe.observe()
            step = dict(extras or {}, obs=oo, vec=ov, actions=a, **{k: np.array(o[key]) for k, key in OUT_KEYS})
            for k, v in step.items():
                row.setdefault(k, []).append(v)
        rows.append({k: np.stack(v) for k, v in row.items()})
        if t + 1 in bounds:
            state[t + 1] = dict(pos=np.stack([oe.agents()[0] for oe in oracles]),
                                goal=np.stack([oe.agents()[1] for oe in oracles]),
                                hpos=np.stack([oe.human()["pos"] for oe in oracles]),
                                hgoal=np.stack([oe.human()["goal"] for oe in oracles]),
                                bfs=np.stack([oe.bfs() for oe in oracles]),
                                errors=sum(oe.errors() for oe in oracles))
    ref = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
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


# ------------------------------------------------------------------ comparers
def check_state(env, state, what):
    st = env.get_state()
    np.testing.assert_array_equal(st["pos"], state["pos"], err_msg=f"{what}: pos")
    np.testing.assert_array_equal(st["goal"], state["goal"], err_msg=f"{what}: goal")
    np.testing.assert_array_equal(st["human"][:, 0:2], state["hpos"], err_msg=f"{what}: human pos")
    np.testing.assert_array_equal(st["human"][:, 4:6], state["hgoal"], err_msg=f"{what}: human goal")
    np.testing.assert_array_equal(env.bfs().cpu().numpy(), state["bfs"], err_msg=f"{what}: bfs")


def check_slots(what, ref, t0, got_out, obs, vec, slots):
    """slots: [(slot index in the buffers, step index relative to t0)] to compare, every bit."""
    obs, vec = obs.cpu().numpy(), vec.cpu().numpy()
    for k, dt in slots:
        t = t0 + dt
        for key, _ in OUT_KEYS:
            want = ref[key][t].astype(got_out[key].dtype).reshape(got_out[key][k].shape)
            assert np.array_equal(got_out[key][k], want), f"{what} t={t}: {key}"
        want = ref["vec"][t].astype(np.float32).reshape(vec[k].shape)
        assert np.array_equal(vec[k].view(np.uint32), want.view(np.uint32)), f"{what} t={t}: vec"
        want = ref["obs"][t].astype(np.float32).reshape(obs[k].shape)
        bad = np.argwhere(obs[k].view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, f"{what} t={t}: {len(bad)} obs floats differ, first (b, agent, ch, y, x) = {bad[0]}"


def check_actions(what, ref, t0, actions, slots):
    a = actions.cpu().numpy()
    for k, dt in slots:
        assert np.array_equal(a[k], ref["actions"][t0 + dt]), f"{what} t={t0 + dt}: chosen actions"


def covered(policy, mine, kname, what):
    """Record a kernel this file compared: in its own set `mine` and in the session's registry."""
    assert kname.endswith(f",{policy}>"), kname
    mine.add(kname)
    record_rollout_kernel(kname, what)


# ------------------------------------------------------------------ the case runner
def run_policy_case(policy, env_of, mine, name, path, ref, state, launches, tuning=None, expect=None, tape=None,
                    allow=(1, 2), hook=None):
    """One case of `policy` against the oracle's (ref, state).  path "rollout": [T]-slot buffers, every
    slot compared; "inplace": the [B]-leading buffers, each launch's last step compared; "inplace1":
    one-step launches in place, every step compared.  env_of: the file's case_env.  tape: the host tape
    of policy "tape" (else the chosen actions are compared too).  allow: the device counters that may
    count, and then exactly as often as the oracle's -- agents boxed in (1, 2) by a numpy tape or by
    agents that ignore each other; () for a planner that leaves fixActions nothing it cannot place.
    hook(what, ref, t0, got, acts, which): more checks per launch.  Returns the steps played."""
    if path == "inplace1":
        launches = (1,) * 24
    elif path == "inplace":
        launches = launches[1:]
    env, case, _, _, _ = env_of(name, tuning)
    try:
        slots = path == "rollout"
        kname, plan = env.rollout_kernel_name(slots=slots, policy=policy), env.rollout_plan(slots=slots, policy=policy)
        assert kname.endswith(f",{policy}>"), plan
        assert kname.replace(f",{policy}>", ">") == env.rollout_kernel_name(slots=slots), (plan, env.rollout_plan(slots))
        if policy != "tape" and kname.startswith("rollout_wide3"):
            assert " bfsobs=0 " in plan, plan       # the stepping wave searches the maps it reads
        if expect is not None:
            assert kname == expect, plan
        if tape is not None:
            tape = torch.from_numpy(tape).to(env.device)
        t0 = 0
        for T in launches:
            k = T if slots else 1
            buf, acts = slot_buffers(env, k), action_buffer(env, k)
            env.rollout(T, policy, slots=slots, actions=acts, tape=None if tape is None else tape[t0:t0 + T], **buf)
            got = host(buf["out"])
            what = f"{name} {path} launch [{t0}, {t0 + T})"
            which = [(q, q) for q in range(T)] if slots else [(0, T - 1)]
            if tape is None:
                check_actions(what, ref, t0, acts, which)
            check_slots(what, ref, t0, got, buf["obs"], buf["vec"], which)
            if hook is not None:
                hook(what, ref, t0, got, acts, which)
            t0 += T
            check_state(env, state[t0], what)
        assert_no_errors(env, allow=allow)
        if allow:
            assert int(env.counters()[:8].sum()) == state[t0]["errors"]
        else:
            assert state[t0]["errors"] == 0
        covered(policy, mine, kname, f"{name} {path} {policy} vs oracle")
    finally:
        env.close()
    return t0


# ------------------------------------------------------------------ shared test bodies
def launcher_band_clean_case(policy, env_of, form, subs, allow=(1, 2), mine=None):
    """rollout_launcher(policy=...) on NaN-prefilled slot buffers: call 1 stores everything; calls 2 and
    3 carry MAPF_SLOTS_BAND_CLEAN and leave exactly mapf_obs_band_skip's floats alone (sentinels survive
    there, every other float and output equals an unflagged twin's).  mine: record the kernel there."""
    name, T = "g_n8_20x20_f11", 23
    env, case, _, _, seed = env_of(name, form)
    twin = env_of(name, form)[0]
    try:
        kname = env.rollout_kernel_name(slots=True, band_clean=True, policy=policy)
        assert kname == "rollout_random_kernel<true,%d,band64,%s>" % (subs, policy)
        acts = action_buffer(env, T)
        roll = dict(actions=acts, **slot_buffers(env, T))
        launch = env.rollout_launcher(T, slots=True, actions=acts, obs=roll["obs"], vec=roll["vec"], out=roll["out"],
                                      policy=policy)
        for call in range(3):
            if call:
                set_sentinels(roll)
            launch()
            ref = slot_buffers(twin, T)
            ref_acts = torch.full_like(acts, -9)
            twin.rollout(T, policy, slots=True, actions=ref_acts, **ref)
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
        assert_no_errors(env, allow=allow)
        if mine is not None:
            covered(policy, mine, kname, f"{name} band-clean {policy} vs an oracle-compared twin")
    finally:
        env.close()
        twin.close()


def captured_rollout_case(policy, env_of, ref, state, allow=(1, 2)):
    """One rollout launch of the c4 shape (the three-wave form) captured into a graph and replayed
    twice: 2T steps of the episode, every slot of both replays against the oracle."""
    name, T = "c4_40x40_n16_f9_looping", 12
    env, case, _, _, _ = env_of(name)
    g = None
    try:
        assert env.rollout_kernel_name(slots=True, policy=policy) == "rollout_wide3_kernel<u64,1,true,%s>" % policy
        buf, acts = slot_buffers(env, T), action_buffer(env, T)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                env.rollout(T, policy, slots=True, actions=acts, **buf)       # recorded, not run
        torch.cuda.synchronize()
        for call in range(2):
            g.replay()
            torch.cuda.synchronize()
            which = [(q, q) for q in range(T)]
            check_actions(f"replay {call}", ref, call * T, acts, which)
            check_slots(f"replay {call}", ref, call * T, host(buf["out"]), buf["obs"], buf["vec"], which)
        check_state(env, state[2 * T], "after two replays")
        assert_no_errors(env, allow=allow)
    finally:
        del g
        env.close()


def keep_bfs_off_case(policy, env_of):
    """A policy that reads the agents' BFS maps: T = 0 is a no-op, in Python and in C, and keep_bfs off
    is a state error (-4) of the per-step pick and of the rollout, in C and in Python."""
    from mapf_amd import _lib
    from mapf_amd.env import ROLLOUT_POLICIES, _ptr, _stream
    env = env_of("r_n6_16x16_f9_dahp")[0]
    off = env_of("r_n6_16x16_f9_dahp", keep_bfs=False)[0]
    try:
        L = _lib.lib()
        c_rollout, c_pick = getattr(L, ROLLOUT_POLICIES[policy][0]), getattr(L, f"mapf_{policy}_actions")
        before = env.get_state()
        env.rollout(0, policy)
        assert c_rollout(env.h, 0, 0, _ptr(env.actions), ctypes.byref(env._stepout), _ptr(env.obs), _ptr(env.vec),
                         _stream(env.device)) == 0
        torch.cuda.synchronize()
        after = env.get_state()
        for key in before:
            np.testing.assert_array_equal(before[key], after[key])
        assert c_pick(off.h, _ptr(off.actions), _stream(off.device)) == -4
        assert c_rollout(off.h, 4, 0, _ptr(off.actions), ctypes.byref(off._stepout), _ptr(off.obs), _ptr(off.vec),
                         _stream(off.device)) == -4
        with pytest.raises(RuntimeError, match="keep_bfs"):
            getattr(off, f"{policy}_actions")()
        with pytest.raises(RuntimeError, match="keep_bfs"):
            off.rollout(4, policy)
    finally:
        env.close()
        off.close()


def fixed_episodes_case(make_policy, mtype, da_hp):
    """evaluate_fixed_episodes under make_policy() (refused without keep_bfs), recording its actions,
    then replay_fixed_episodes over the tapes: integer metrics equal, the float64 sums of float32 terms
    within 1e-9 relative (summation order only).  Returns the recorded run's metrics."""
    from mapf_amd.episodes import METRIC_KEYS, evaluate_fixed_episodes, load_fixed_episode_infos, replay_fixed_episodes
    infos = load_fixed_episode_infos(G6)
    steps = 48
    kw = dict(num_channel=6, fov=9, use_da=da_hp, use_hp=da_hp, human_movement_type=mtype, fix_choice=1)
    with pytest.raises(RuntimeError, match="keep_bfs=True"):
        evaluate_fixed_episodes(infos, make_policy(), max_steps=1, **kw)
    got, tapes = evaluate_fixed_episodes(infos, make_policy(), max_steps=steps, record_actions=True, keep_bfs=True, **kw)
    rep = replay_fixed_episodes(infos, tapes, **kw)
    for key in METRIC_KEYS:
        if key in ("episodeReward", "episodeCostReward"):
            np.testing.assert_allclose(rep[key], got[key], rtol=1e-9, atol=0, err_msg=key)
        else:
            np.testing.assert_array_equal(rep[key], got[key], err_msg=key)
    return got


def coverage_guard(policy, mine, cfg):
    """The `policy` kernel the BASELINE preset launches by default, in place and into slots, is in the
    file's own set `mine` (which must not be empty) and in the session's registry."""
    from test_gpu_ycoverage import preset_env
    if not mine:
        pytest.fail(f"no compared {policy} case of this file ran before the guard")
    env = preset_env(cfg)
    try:
        assert env.rollout_fused, cfg
        for slots in (False, True):
            name = env.rollout_kernel_name(slots, policy=policy)
            assert name in mine and name in COVERED, (
                f"{cfg} slots={slots}: {env.rollout_plan(slots, policy=policy)} is launched by default but no "
                f"compared case of this file ran it; covered: {sorted(mine)}")
    finally:
        env.close()
