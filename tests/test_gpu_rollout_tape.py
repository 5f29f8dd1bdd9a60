"""GPU: persistent rollouts driven by a caller's action tape (mapf_rollout_actions, include/mapf.h).

The rollout kernels' TAPE instantiations play row [t][b] of an int32 [T][B][N] tape instead of the
in-kernel random draw.  Every case draws its tape from numpy (not the Philox policy's stream), with
three forced rows -- one env all 0, one env always the same move, one env alternating two opposite
moves -- and compares every slot bit for bit with the CPU oracle stepping the same tape, or with
the reference's own recorded episodes (tests/golden/g1_*).  The pair-lane kernel stages TAPE_K = 32
steps of an env's actions in LDS, so its launches are 1, 23, 67, 32 (= K) and 33 (= K + 1) steps.

The file ends with a guard: the tape kernel every BASELINE preset launches by default, into slots
and in place, has been run by an oracle- or fixture-compared case above (tests/kernel_registry.py).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rollout_harness as H
from golden_io import G1_NAMES, load, unpack_obs
from rollout_harness import host_skip, preset_envs, set_sentinels, slot_buffers
from test_gpu_parity import GROUP_CASES, RANDOM_CASES, ROLLOUT_CASES, WIDE_SHAPES, assert_no_errors, host, mk_env

pytestmark = pytest.mark.gpu

TAPE_K = 32                                  # csrc/mapf_fused.hip: steps of the tape staged in LDS at a time
LAUNCHES = (1, 23, 67, TAPE_K, TAPE_K + 1)   # steps per launch, in this order
TAPE_COVERED = set()                         # kernel names this file compared against the oracle or a fixture
CASES = {**GROUP_CASES, **ROLLOUT_CASES, **RANDOM_CASES, **WIDE_SHAPES}
SEED = 0x5EED0000
covered = functools.partial(H.covered, "tape", TAPE_COVERED)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def make_tape(T, B, n, seed, bad=False):
    """Uniform 0..4 from numpy; env 0 all 0, env 1 always move 3, env 2 alternating 1 / 3 (opposites)."""
    rng = np.random.default_rng(seed)
    tape = rng.integers(0, 5, size=(T, B, n), dtype=np.int32)
    tape[:, 0] = 0
    if B > 1:
        tape[:, 1] = 3
    if B > 2:
        tape[0::2, 2] = 1
        tape[1::2, 2] = 3
    if bad:
        k = rng.random(tape.shape)
        tape[k < 0.03] = -1
        tape[(k >= 0.03) & (k < 0.06)] = 5
        tape[(k >= 0.06) & (k < 0.09)] = 99
    return tape


def case_setup(name):
    return H.case_setup(CASES, name, SEED)


def case_env(name, tuning=None):
    return H.case_env(CASES, name, SEED, tuning)


@functools.lru_cache(maxsize=None)
def oracle_run(name, steps):
    """The oracle playing make_tape's first `steps` rows of the case, computed once and shared
    (read-only): the tape, per-step outputs / observations / vectors [steps, B, ...], and the state
    (cells, goals, human, BFS maps, the oracle's error count) after every launch of every path."""
    case, _, _, seed = case_setup(name)
    tape = make_tape(steps, case["B"], case["n"], seed)
    bounds = set(np.cumsum(LAUNCHES).tolist()) | set(np.cumsum(LAUNCHES[1:]).tolist()) | set(range(1, 25)) | {steps}
    return (tape,) + H.oracle_rollout(CASES, name, SEED, steps, bounds, lambda oe, b, t, world: (tape[t, b], None))


def run_tape_case(name, path, tuning=None, launches=LAUNCHES, expect=None):
    tape, ref, state = oracle_run(name, int(np.sum(launches)))
    H.run_policy_case("tape", case_env, TAPE_COVERED, name, path, ref, state, launches, tuning, expect, tape=tape)


# ------------------------------------------------------------------ 1. the pair-lane kernel
PAIR_CASES = [("r_n6_16x16_f9_dahp", None, "1"),                                            # B = 37: ragged
              ("g_n8_20x20_f11_ragged61", dict(roll_occ=4, roll_group=1, roll_slack=1), "4"),  # grouped, paced
              ("g_n8_20x20_f11", dict(roll_occ=4, roll_fair=4), "4")]                       # grouped, fair


@pytest.mark.parametrize("path", ["rollout", "inplace1", "inplace"])
@pytest.mark.parametrize("name,tuning,subs", PAIR_CASES)
def test_pair_lane_tape_matches_oracle(name, tuning, subs, path):
    # B = 61 in place without roll_fair: the auto form (fair 4) is grouped all the same
    expect = "rollout_random_kernel<%s,%s,tape>" % ("true" if path == "rollout" else "false", subs)
    run_tape_case(name, path, tuning, expect=expect)


# ------------------------------------------------------------------ 2. the wide kernels
WIDE_CASES = [("c4_40x40_n16_f9_looping", None, "rollout", "rollout_wide3_kernel<u64,1,true,tape>"),
              ("c4_40x40_n16_f9_looping", None, "inplace", "rollout_wide3_kernel<u64,1,false,tape>"),
              ("c4_40x40_n16_f9_looping", dict(wide_obs=1), "rollout", "rollout_wide_kernel<u64,1,true,tape>"),
              ("c4_40x40_n16_f9_looping", dict(wide_pipe=0), "rollout", "rollout_wide_kernel<u64,1,true,tape>"),
              ("dense_12x12_n16_f9_dahp", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "rollout", None),
              ("c1_10x10_n4_f11", None, "inplace", None),
              ("c1_10x10_n4_f11", None, "inplace1", None),
              ("c5_80x80_n64_f11_bfsch", None, "rollout", "rollout_wide_kernel<Row2,2,true,tape>"),
              ("w_n20_48x90_f11_bfsch", None, "rollout", None)]


@pytest.mark.parametrize("name,tuning,path,expect", WIDE_CASES)
def test_wide_tape_matches_oracle(name, tuning, path, expect):
    """The one-wave-per-env kernels: three waves per env (c4's form), two (wide_obs 1), one
    (wide_pipe 0; c5's Row2 form at B = 3), u32 / u64 / 128-bit search rows, the BFS channel."""
    run_tape_case(name, path, tuning, launches=LAUNCHES[:3], expect=expect)


# ------------------------------------------------------------------ 3. the reference's trajectories
@pytest.mark.parametrize("name", G1_NAMES)
def test_reference_episode_through_the_persistent_kernel(name):
    """The reference's recorded g1 episode (its own actions, goal sequences, LoopingHuman or
    FixedPathHuman; fixActions' rotating rule) in ONE rollout_actions launch into slots: every
    slot's outputs, observation and vec equal the fixture, and the final state and BFS maps too.
    Every g1 configuration has a one-launch kernel today (rollout_fused is asserted); a configuration
    without one would still pass here through mapf_rollout_actions' per-step launches."""
    z = load(name)
    n, fov, nch = int(z["n"]), int(z["fov"]), int(z["nch"])
    world = z["map"]
    H, W = world.shape
    hmode = int(z["human_mode"])
    B, T = 9, int(z["steps"])
    env = mk_env(B=B, H=H, W=W, num_agents=n, fov=fov, num_channel=nch, use_da=int(z["use_da"]),
                 use_hp=int(z["use_hp"]), human_mode=hmode, goal_mode="sequence", fix_choice=0,
                 max_seq=z["seq"].shape[1], max_human_seq=max(2, len(z["hseq"])))
    try:
        seqs = [z["seq"][i, :z["seq_len"][i]] for i in range(n)]
        if hmode == 2:
            env.reset_fixed(world, [seqs] * B, human_seq=[z["hseq"]] * B)
        else:
            env.reset_fixed(world, [seqs] * B, [z["hstart"]] * B, [z["hgoal"]] * B)
        assert env.rollout_fused, name
        kname = env.rollout_actions_kernel_name(slots=True)
        tape = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["actions"][:T, None].astype(np.int32), (T, B, n))))
        buf = slot_buffers(env, T)
        env.rollout_actions(tape.to(env.device), slots=True, **buf)
        out = host(buf["out"])
        obs, vec = buf["obs"].cpu().numpy(), buf["vec"].cpu().numpy()
        for t in range(T):
            for k, key in [("status", "status"), ("reward", "reward"), ("cost", "cost"), ("train_valid", "valid"),
                           ("actions_fixed", "fixed"), ("goals_reached", "goals"), ("constraints", "constr")]:
                want = np.broadcast_to(z[key][t].astype(out[k].dtype), out[k][t].shape)
                assert np.array_equal(out[k][t], want), f"{name} t={t} {k}"
            assert (out["shadow_goals"][t] == int(z["shadow"][t])).all(), f"{name} t={t} shadow"
            rt = (z["reward"][t] + np.where(z["goals"][t] == 1, np.float32(1.5), np.float32(0))).astype(np.float32)
            assert np.array_equal(out["reward_total"][t], np.broadcast_to(rt, (B, n))), f"{name} t={t} reward_total"
            want = unpack_obs(z["obs"][t], (n, nch, fov, fov))
            assert (obs[t] == want[None]).all(), f"{name} t={t} obs"
            assert (vec[t] == z["vec"][t][None]).all(), f"{name} t={t} vec"
        st = env.get_state()
        for b in range(B):
            np.testing.assert_array_equal(st["pos"][b], z["pos"][T - 1])
            np.testing.assert_array_equal(st["goal"][b], z["goal"][T - 1])
            np.testing.assert_array_equal(st["human"][b, 0:2], z["hpos"][T - 1])
            np.testing.assert_array_equal(st["human"][b, 2:4], z["hnext"][T - 1])
        bfs = env.bfs().cpu().numpy()
        assert (bfs == z["bfs_final"][None]).all(), f"{name} bfs_final"
        assert_no_errors(env)
        covered(kname, f"{name} reference episode")
    finally:
        env.close()


# ------------------------------------------------------------------ 4. replay equals record, full size
@pytest.mark.parametrize("cfg,T,slots", [("c2", 8, True), ("c4", 8, True), ("c5", 4, True), ("c2", 8, False)])
def test_replay_equals_record_at_full_size(cfg, T, slots):
    """rollout_random on one handle, rollout_actions over its recorded actions on a twin: every
    output, every observation bit, the state and the counters are equal."""
    rec, rep, *more = preset_envs(cfg, 2 if slots else 3)
    try:
        k = T if slots else 1
        acts = torch.full((T, rec.B, rec.N), -9, dtype=torch.int32, device=rec.device)
        a, b = slot_buffers(rec, k), slot_buffers(rep, k)
        if slots:
            rec.rollout_random(T, slots=True, actions=acts, **a)
        else:            # in place the drawn actions are overwritten every step: a third handle records them
            more[0].rollout_random(T, slots=True, actions=acts, **slot_buffers(more[0], T))
            more[0].close()
            rec.rollout_random(T, slots=False, actions=torch.empty_like(acts[0]), **a)
        assert rep.rollout_actions_kernel_name(slots).replace(",tape>", ">") == rec.rollout_kernel_name(slots)
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


# ------------------------------------------------------------------ 5. bad actions
@pytest.mark.parametrize("name", ["r_n6_16x16_f9_dahp", "c4_40x40_n16_f9_looping"])
def test_bad_actions_are_counted_and_played_as_stay(name):
    T = 40                                    # past one staged piece of the tape
    env, case, _, _, seed = case_env(name)
    twin = case_env(name)[0]
    try:
        tape_h = make_tape(T, case["B"], case["n"], seed + 1, bad=True)
        nbad = int(((tape_h < 0) | (tape_h > 4)).sum())
        assert nbad > T
        tape = torch.from_numpy(tape_h).to(env.device)
        buf = slot_buffers(env, T)
        env.rollout_actions(tape, slots=True, **buf)
        out = host(buf["out"])
        for t in range(T):
            o, obs, vec = twin.step_observe(tape[t])
            o = host(o)
            for key in o:
                assert np.array_equal(out[key][t], o[key]), f"{name} t={t} {key}"
            assert torch.equal(buf["obs"][t], obs) and torch.equal(buf["vec"][t], vec), f"{name} t={t} obs"
        c, ct = env.counters(), twin.counters()
        assert (c[:8] == ct[:8]).all(), (c[:8], ct[:8])
        assert int(c[0]) == nbad
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 6. band-clean launcher
@pytest.mark.parametrize("form,subs", [(dict(roll_occ=4, roll_group=1), 4), (None, 1)])
def test_tape_launcher_declares_the_band_clean_after_its_first_call(form, subs):
    """rollout_launcher(actions_in=tape) on NaN-prefilled slot buffers: call 1 stores everything;
    calls 2 and 3 carry MAPF_SLOTS_BAND_CLEAN and leave exactly mapf_obs_band_skip's floats alone
    (sentinels survive there, every other float and output equals an unflagged twin's).  The tape
    tensor is refilled between calls: the launch reads it, not the launcher."""
    name, T = "g_n8_20x20_f11", 23
    env, case, _, _, seed = case_env(name, form)
    twin = case_env(name, form)[0]
    try:
        assert env.rollout_actions_kernel_name(slots=True, band_clean=True) == "rollout_random_kernel<true,%d,band64,tape>" % subs
        tapes = make_tape(3 * T, case["B"], case["n"], seed + 2)
        tape = torch.empty(T, case["B"], case["n"], dtype=torch.int32, device=env.device)
        roll = dict(actions=torch.full_like(tape, -9), **slot_buffers(env, T))
        launch = env.rollout_launcher(T, slots=True, obs=roll["obs"], vec=roll["vec"], out=roll["out"], actions_in=tape)
        for call in range(3):
            tape.copy_(torch.from_numpy(tapes[call * T:(call + 1) * T]))
            if call:
                set_sentinels(roll)
            launch()
            ref = slot_buffers(twin, T)
            twin.rollout_actions(tape, slots=True, **ref)
            torch.cuda.synchronize()
            want = ref["obs"].clone()
            if call:
                skip = torch.from_numpy(host_skip(env, case, roll, True)).to(env.device)
                want.view(skip.shape)[skip] = 7.0
            assert torch.equal(roll["obs"].view(torch.int32), want.view(torch.int32)), f"call {call}: obs"
            assert torch.equal(roll["vec"].view(torch.int32), ref["vec"].view(torch.int32)), f"call {call}: vec"
            for key in ref["out"]:
                assert torch.equal(roll["out"][key], ref["out"][key]), f"call {call}: {key}"
        assert_no_errors(env)
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------ 7. capture
def graph_shape(raw_graph):
    """(kernel nodes, other nodes, largest number of edges into or out of one node) of a hipGraph_t."""
    hip = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphGetEdges.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz)]
    hip.hipGraphNodeGetType.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    g = vp(raw_graph)
    n = sz(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (vp * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kernels = 0
    for node in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(vp(node), ctypes.byref(t)) == 0
        kernels += t.value == 0                       # hipGraphNodeTypeKernel
    ne = sz(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(ne)) == 0
    fan = 0
    if ne.value:
        src, dst = (vp * ne.value)(), (vp * ne.value)()
        assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(ne)) == 0
        for side in (list(src), list(dst)):
            fan = max([fan] + [side.count(x) for x in set(side)])
    return kernels, n.value - kernels, fan


def test_captured_tape_rollout_replays_with_a_refilled_tape():
    """One rollout_actions launch of the c4 shape (B = 16, the three-wave form) captured into a graph:
    replayed, then replayed with other actions in the same tape tensor, each replay equals a direct
    launch on a twin.  The graph is a chain without parallel branches: the one rollout kernel node
    and, before it, the store of its argument block (the three-wave form reads its arguments from
    device memory, ArgRing) -- no memcpy, memset or host node."""
    name, T = "c4_40x40_n16_f9_looping", 12
    env, case, _, _, seed = case_env(name)
    twin = case_env(name)[0]
    g = None
    try:
        assert env.rollout_actions_kernel_name(slots=True) == "rollout_wide3_kernel<u64,1,true,tape>"
        tapes = make_tape(2 * T, case["B"], case["n"], seed + 3)
        tape = torch.from_numpy(tapes[:T]).to(env.device)
        buf, ref = slot_buffers(env, T), slot_buffers(twin, T)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                env.rollout_actions(tape, slots=True, **buf)       # recorded, not run
        torch.cuda.synchronize()
        kernels, others, fan = graph_shape(g.raw_cuda_graph())
        assert others == 0 and fan <= 1 and 1 <= kernels <= 2, (kernels, others, fan)
        for call in range(2):
            tape.copy_(torch.from_numpy(tapes[call * T:(call + 1) * T]))
            g.replay()
            twin.rollout_actions(tape, slots=True, **ref)
            torch.cuda.synchronize()
            assert torch.equal(buf["obs"].view(torch.int32), ref["obs"].view(torch.int32)), f"replay {call}: obs"
            assert torch.equal(buf["vec"].view(torch.int32), ref["vec"].view(torch.int32)), f"replay {call}: vec"
            for key in ref["out"]:
                assert torch.equal(buf["out"][key], ref["out"][key]), f"replay {call}: {key}"
        sa, sb = env.get_state(), twin.get_state()
        for key in sa:
            np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"state {key}")
        assert_no_errors(env)
    finally:
        del g
        env.close()
        twin.close()


def test_tape_may_not_overlap_actions_fixed_and_T0_is_a_no_op():
    env, case, _, _, seed = case_env("r_n6_16x16_f9_dahp")
    try:
        from mapf_amd import _lib
        from mapf_amd.env import _ptr, _stream
        T = 4
        buf = slot_buffers(env, T)
        before = env.get_state()
        env.rollout_actions(torch.empty(0, case["B"], case["n"], dtype=torch.int32, device=env.device))
        assert _lib.lib().mapf_rollout_actions(env.h, 0, 0, _ptr(env.actions), ctypes.byref(env._stepout), _ptr(env.obs),
                                               _ptr(env.vec), _stream(env.device)) == 0
        torch.cuda.synchronize()
        after = env.get_state()
        for key in before:
            np.testing.assert_array_equal(before[key], after[key])
        buf["out"]["actions_fixed"].zero_()
        with pytest.raises(RuntimeError, match="overlaps"):
            env.rollout_actions(buf["out"]["actions_fixed"], slots=True, **buf)
    finally:
        env.close()


# ------------------------------------------------------------------ 9. record and replay of fixed episodes
@pytest.mark.parametrize("mtype,da_hp", [(0, False), (1, True)])
def test_replay_fixed_episodes_equals_evaluate(mtype, da_hp):
    """evaluate_fixed_episodes under uniform random actions (sample_actions over a uniform ps),
    recording them, then replay_fixed_episodes over the tapes: integer metrics equal, the float64
    sums of float32 terms within 1e-9 relative (summation order only)."""
    from mapf_amd.env import sample_actions
    from mapf_amd.episodes import METRIC_KEYS, evaluate_fixed_episodes, load_fixed_episode_infos, replay_fixed_episodes
    infos = load_fixed_episode_infos(H.G6)
    steps = 48

    def policy(obs, vec, env, t):
        ps = torch.full((env.B, env.N, 5), 0.2, dtype=torch.float32, device=env.device)
        return sample_actions(ps, 11, t, out32=env.actions)

    kw = dict(num_channel=6, fov=9, use_da=da_hp, use_hp=da_hp, human_movement_type=mtype, fix_choice=1)
    plain = evaluate_fixed_episodes(infos, policy, max_steps=steps, **kw)
    got, tapes = evaluate_fixed_episodes(infos, policy, max_steps=steps, record_actions=True, **kw)
    assert sorted(got) == sorted(plain) == sorted(METRIC_KEYS)
    for key in METRIC_KEYS:                      # the default return value is unchanged
        np.testing.assert_array_equal(got[key], plain[key], err_msg=key)
    for shape, tp in tapes.items():
        assert tp.dtype == torch.int32 and tp.shape[0] == steps and tp.is_cuda, shape
        assert len(torch.unique(tp)) == 5
    rep = replay_fixed_episodes(infos, tapes, **kw)
    for key in METRIC_KEYS:
        if key in ("episodeReward", "episodeCostReward"):
            np.testing.assert_allclose(rep[key], got[key], rtol=1e-9, atol=0, err_msg=key)
        else:
            np.testing.assert_array_equal(rep[key], got[key], err_msg=key)
    assert got["totalGoals"].sum() + got["agentCollide"].sum() + got["staticCollide"].sum() > 0


# ------------------------------------------------------------------ 8. coverage guard (last)
@pytest.mark.parametrize("cfg", ["c1", "c2", "c4", "c5"])
def test_default_tape_kernels_are_covered_by_this_file(cfg):
    H.coverage_guard("tape", TAPE_COVERED, cfg)
