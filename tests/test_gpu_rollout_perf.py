"""mapf_rollout_perf / mapf_perf_accumulate on the device (include/mapf.h: mapf_perf): the episode metrics
from one launch that writes no observation.

The reference for every comparison is the reference's own arithmetic in numpy (np_perf below:
`acc = acc + np.sum(x[t].astype(np.float32))` in float32, integer counts) over step outputs that the slot
form of the same rollout wrote on a twin handle; the comparison is bit for bit in all eight fields, and the
handle that took the perf form must end in the same state as the twin (state, counters, BFS maps, the next
observation, the next PIBT pick)."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_parity import host, mk_env

pytestmark = pytest.mark.gpu

T = 48
POLICIES = ("random", "tape", "descent", "pibt")
KEYS = ("status", "reward_total", "cost", "goals_reached", "shadow_goals", "constraints")

# kind: mapf_rollout_random_fused's.  Maps: "shared" one random map, "per_env" one random map per env (both the
# largest free component at the given obstacle density).  The seeds are chosen so that the random policy on
# handle A makes every metric non-zero in some env (asserted below).
CASES = {
    "pair_b37_n8": dict(kind=1, B=37, n=8, H=20, W=20, fov=11, nch=6, maps="shared", density=0.2, seed=11),
    # (the pair-lane kernels need N * C * F * F to be a multiple of 4: an even FOV for five agents)
    "pair_b6_n5": dict(kind=1, B=6, n=5, H=20, W=20, fov=10, nch=6, maps="shared", density=0.2, seed=12),
    "wide_b9_n16": dict(kind=2, B=9, n=16, H=24, W=24, fov=9, nch=6, maps="per_env", density=0.3, seed=13),
    "wide_b3_n64_c7": dict(kind=2, B=3, n=64, H=40, W=40, fov=9, nch=7, maps="per_env", density=0.2, seed=14),
    "wide_b5_n17": dict(kind=2, B=5, n=17, H=24, W=24, fov=9, nch=6, maps="per_env", density=0.3, seed=15),
    # no one-launch kernel: 16 agents with the HP channel and k_predict = 64 (asked of the handle below)
    "steps_b4_n16_k64": dict(kind=0, B=4, n=16, H=12, W=12, fov=9, nch=6, maps="shared", density=0.2, seed=16,
                             hp=1, k_predict=64),
}


def case_maps(case):
    from mapf_amd.maps import keep_largest_component, random_map
    rng = np.random.default_rng(1000 + case["seed"])
    one = lambda: keep_largest_component(random_map(rng, case["H"], case["W"], case["density"]))
    if case["maps"] == "shared":
        return one(), True
    return np.stack([one() for _ in range(case["B"])]), False


def twins(name, count=2, weight=None, horizon=None):
    case = CASES[name]
    maps, shared = case_maps(case)
    envs = []
    for _ in range(count):
        kw = dict(k_predict=case["k_predict"]) if "k_predict" in case else {}
        e = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                   use_hp=case.get("hp", 0), human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared,
                   keep_bfs=True, seed=case["seed"], env_offset=3, **kw)
        e.reset_seeded(maps)
        if weight is not None:
            e.set_pibt_human_weight(weight)
        if horizon is not None:
            e.set_pibt_human_horizon(horizon)
        envs.append(e)
    assert envs[0].rollout_kernel == case["kind"], (name, envs[0].rollout_kernel)
    return envs


def slot_out(env, steps):
    return {k: torch.full((steps,) + tuple(env.out[k].shape), -7, dtype=env.out[k].dtype, device=env.device) for k in KEYS}


def slot_rollout(env, steps, policy, tape=None):
    """rollout(steps, policy, slots=True) into fresh [steps] buffers: (host outputs, device actions)."""
    out = slot_out(env, steps)
    obs = torch.empty((steps,) + tuple(env.obs.shape), device=env.device)
    vec = torch.empty((steps,) + tuple(env.vec.shape), device=env.device)
    acts = torch.full((steps, env.B, env.N), -9, dtype=torch.int32, device=env.device)
    tape = tape if policy == "tape" else None
    env.rollout(steps, policy, slots=True, actions=None if tape is not None else acts, tape=tape, obs=obs, vec=vec, out=out)
    return host(out), (tape if policy == "tape" else acts)


def np_perf(o, start=None):
    """The reference's arithmetic over host step outputs [T][B][N] ([T][B]): int32 [B, 8], the float32 sums as bits."""
    steps, B = o["status"].shape[:2]
    rec = np.zeros((B, 8), np.int32) if start is None else np.array(start, np.int32)
    for b in range(B):
        er, ec = rec[b, 0:1].view(np.float32)[0], rec[b, 1:2].view(np.float32)[0]
        for t in range(steps):
            er = er + np.sum(o["reward_total"][t, b].astype(np.float32))
            ec = ec + np.sum(o["cost"][t, b].astype(np.float32))
        assert er.dtype == np.float32 and ec.dtype == np.float32
        st = o["status"][:, b]
        rec[b] = [np.float32(er).view(np.int32), np.float32(ec).view(np.int32), rec[b, 2] + np.sum(st == -2),
                  rec[b, 3] + np.sum(st == -1), rec[b, 4] + np.sum(st == -3),
                  rec[b, 5] + np.sum(o["goals_reached"][:, b] == 1), rec[b, 6] + np.sum(o["shadow_goals"][:, b]),
                  rec[b, 7] + np.sum(o["constraints"][:, b] == 1)]
    return rec


def assert_same_handle_state(a, b, what, pibt=False):
    """Everything a later call can see: state, counters, BFS maps, the next observation, the next PIBT pick."""
    torch.cuda.synchronize()
    sa, sb = a.get_state(), b.get_state()
    assert set(sa) == set(sb)
    for key in sa:
        np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{what}: state {key}")
    np.testing.assert_array_equal(a.counters(), b.counters(), err_msg=f"{what}: counters")
    assert torch.equal(a.bfs(), b.bfs()), f"{what}: bfs maps"
    (oa, va), (ob, vb) = a.observe(), b.observe()
    assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), f"{what}: next obs"
    assert torch.equal(va.view(torch.int32), vb.view(torch.int32)), f"{what}: next vec"
    if pibt:
        assert torch.equal(a.pibt_actions(), b.pibt_actions()), f"{what}: next pibt pick"


def close_all(envs):
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 1. perf_accumulate on synthetic outputs
def synthetic(n, steps=5, B=7, seed=5):
    rng = np.random.default_rng(seed + n)
    status = rng.choice(np.array([1, 1, -1, -2, -3, -4], np.int8), size=(steps, B, n))
    consts = np.array([-0.3, -0.35, -2.0, 1.2], np.float32)
    d2 = rng.integers(0, 40, size=(steps, B, n))
    return dict(status=status, reward_total=consts[rng.integers(0, 4, size=(steps, B, n))],
                cost=(np.maximum(5 - np.sqrt(d2.astype(np.float64)), 0.0) / 5).astype(np.float32),
                goals_reached=(rng.random((steps, B, n)) < 0.3).astype(np.float32),
                shadow_goals=rng.integers(0, n + 1, size=(steps, B)).astype(np.int32),
                constraints=(rng.random((steps, B, n)) < 0.4).astype(np.float32))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17, 64])
def test_perf_accumulate_equals_the_numpy_arithmetic(n):
    from mapf_amd.env import perf_accumulate
    o = synthetic(n)
    dev = {k: torch.from_numpy(v).cuda() for k, v in o.items()}
    want = np_perf(o)
    got = perf_accumulate(dev)
    assert np.array_equal(got.cpu().numpy(), want), n
    # 2 + 3 steps with the record carried over
    part = perf_accumulate({k: v[:2].contiguous() for k, v in dev.items()})
    perf_accumulate({k: v[2:].contiguous() for k, v in dev.items()}, perf=part, accumulate=True)
    assert np.array_equal(part.cpu().numpy(), want), n
    # one step's [B] buffers (T = 1)
    one = perf_accumulate({k: v[0].contiguous() for k, v in dev.items()})
    assert np.array_equal(one.cpu().numpy(), np_perf({k: v[:1] for k, v in o.items()})), n
    # a NULL field leaves its metrics at their previous value (accumulate) or zero
    keep = torch.from_numpy(want.copy()).cuda()
    perf_accumulate({k: v for k, v in dev.items() if k not in ("status", "cost")}, perf=keep, accumulate=True)
    twice = np_perf(o, start=want)
    twice[:, [1, 2, 3, 4]] = want[:, [1, 2, 3, 4]]
    assert np.array_equal(keep.cpu().numpy(), twice), n
    zero = perf_accumulate({k: v for k, v in dev.items() if k != "reward_total"})
    assert not zero[:, 0].any() and np.array_equal(zero[:, 1:].cpu().numpy(), want[:, 1:])


def test_perf_accumulate_T0_launches_nothing_and_rejects_nulls():
    from mapf_amd import _lib
    from mapf_amd.env import _stream
    perf = torch.full((7, 8), 5, dtype=torch.int32, device="cuda")
    so = _lib.StepOut()
    L = _lib.lib()
    assert L.mapf_perf_accumulate(ctypes.byref(so), 0, 7, 4, perf.data_ptr(), 0, _stream(perf.device)) == 0
    torch.cuda.synchronize()
    assert (perf == 5).all()
    assert L.mapf_perf_accumulate(ctypes.byref(so), 1, 7, 4, None, 0, _stream(perf.device)) == -1
    assert L.mapf_perf_accumulate(None, 1, 7, 4, perf.data_ptr(), 0, _stream(perf.device)) == -1


# ------------------------------------------------------------------ 2. twin-handle parity
@pytest.mark.parametrize("name", list(CASES))
def test_rollout_perf_equals_the_slot_rollout_reduced_in_numpy(name):
    case = CASES[name]
    tape = None
    for policy in POLICIES:
        a, b = twins(name)
        try:
            plan = b.rollout_perf_plan(policy)
            if case["kind"] == 0:
                pick = {"descent": "descent_actions+", "pibt": "pibt_actions+"}.get(policy, "")
                assert plan == pick + "step+perf_accumulate", plan
            else:
                tag = "" if policy == "random" else "," + policy
                assert (tag + ",perf>") in plan, plan
                assert plan.startswith("rollout_random_kernel<" if case["kind"] == 1 else "rollout_wide_kernel<"), plan
            o, acts = slot_rollout(a, T, policy, tape=tape)
            want = np_perf(o)
            if policy == "random":
                # the condition on the inputs: every metric is counted somewhere
                print(name, "columns non-zero in", (want != 0).sum(0), "envs of", case["B"])
                assert (want != 0).any(0).all(), (name, (want != 0).sum(0))
                tape = acts.clone()             # the tape policy replays A's recorded random actions
            got_acts = None if policy == "tape" else torch.full_like(acts, -9)
            got = b.rollout_perf(T, policy, tape=tape if policy == "tape" else None, actions=got_acts)
            assert np.array_equal(got.cpu().numpy(), want), f"{name} {policy}: {got.cpu().numpy()} != {want}"
            if got_acts is not None:
                assert torch.equal(got_acts, acts), f"{name} {policy}: actions"
            assert_same_handle_state(a, b, f"{name} {policy}", pibt=policy == "pibt")
            # the same launch without an actions buffer: same record (a third handle would cost a reset; b goes on
            # from the twin's state, so does a)
            o2, _ = slot_rollout(a, 5, policy, tape=tape[:5].contiguous() if policy == "tape" else None)
            got2 = b.rollout_perf(5, policy, tape=tape[:5].contiguous() if policy == "tape" else None, perf=got,
                                  accumulate=True)
            assert np.array_equal(got2.cpu().numpy(), np_perf(o2, start=want)), f"{name} {policy}: continued"
            assert_same_handle_state(a, b, f"{name} {policy} continued", pibt=policy == "pibt")
        finally:
            close_all((a, b))


# ------------------------------------------------------------------ 3. chunking on the device
@pytest.mark.parametrize("name", ["pair_b37_n8", "wide_b5_n17"])
@pytest.mark.parametrize("policy", ["random", "pibt"])
def test_one_launch_equals_two_chunks(name, policy):
    a, b = twins(name)
    try:
        one = a.rollout_perf(T, policy)
        two = b.rollout_perf(16, policy)
        b.rollout_perf(32, policy, perf=two, accumulate=True)
        assert torch.equal(one, two), (one, two)
        assert_same_handle_state(a, b, f"{name} {policy} 16 + 32", pibt=policy == "pibt")
    finally:
        close_all((a, b))


# ------------------------------------------------------------------ 4. human-aware PIBT
@pytest.mark.parametrize("name", ["pair_b37_n8", "wide_b9_n16"])
def test_human_weight_and_horizon_apply(name):
    a, b, plain = twins(name, 2, weight=2, horizon=3) + twins(name, 1)
    try:
        assert b.rollout_perf_plan("pibt").endswith(" human_weight=2 human_horizon=3")
        o, acts = slot_rollout(a, T, "pibt")
        want = np_perf(o)
        got_acts = torch.full_like(acts, -9)
        got = b.rollout_perf(T, "pibt", actions=got_acts)
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got_acts, acts)
        assert_same_handle_state(a, b, f"{name} weighted pibt", pibt=True)
        o0, _ = slot_rollout(plain, T, "pibt")
        w0 = np_perf(o0)
        print(name, "constraint violations, weight 0:", w0[:, 7], "weight 2 horizon 3:", want[:, 7])
        assert (w0[:, 7] != want[:, 7]).any()
    finally:
        close_all((a, b, plain))


# ------------------------------------------------------------------ 5. graph capture
def test_captured_launch_replayed_twice():
    a, b = twins("pair_b37_n8")
    g = None
    try:
        perf = torch.zeros(a.B, 8, dtype=torch.int32, device=a.device)
        a.flush()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                a.rollout_perf(8, "random", perf=perf, accumulate=True)      # recorded, not run
        torch.cuda.synchronize()
        assert not perf.any()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        want = b.rollout_perf(16, "random")
        assert torch.equal(perf, want)
        assert_same_handle_state(a, b, "two replays")
    finally:
        del g
        close_all((a, b))


# ------------------------------------------------------------------ 6. errors and edges
def test_error_codes_before_any_launch_and_T0():
    from mapf_amd import _lib
    from mapf_amd.env import _ptr, _stream
    case = CASES["pair_b6_n5"]
    maps, shared = case_maps(case)
    env = twins("pair_b6_n5", 1)[0]
    off = mk_env(B=case["B"], H=case["H"], W=case["W"], num_agents=case["n"], fov=case["fov"], num_channel=case["nch"],
                 human_mode="random", goal_mode="random", fix_choice=1, shared_map=shared, keep_bfs=False, seed=3)
    off.reset_seeded(maps)
    try:
        L, st = _lib.lib(), _stream(env.device)
        perf = torch.full((env.B, 8), 7, dtype=torch.int32, device=env.device)
        before = env.get_state()
        assert L.mapf_rollout_perf(env.h, 0, 4, None, None, 0, st) == -1             # null perf
        assert L.mapf_rollout_perf(None, 0, 4, None, _ptr(perf), 0, st) == -1
        assert L.mapf_rollout_perf(env.h, 4, 4, None, _ptr(perf), 0, st) == -1         # bad policy
        assert L.mapf_rollout_perf(env.h, -1, 4, None, _ptr(perf), 0, st) == -1
        assert L.mapf_rollout_perf(env.h, 1, 4, None, _ptr(perf), 0, st) == -1         # tape without actions
        assert L.mapf_rollout_perf(env.h, 0, -1, None, _ptr(perf), 0, st) == -1
        for policy in (2, 3):
            assert L.mapf_rollout_perf(off.h, policy, 4, None, _ptr(perf), 0, st) == -4   # keep_bfs off
        with pytest.raises(RuntimeError, match="keep_bfs"):
            off.rollout_perf(4, "pibt")
        assert L.mapf_rollout_perf(env.h, 0, 0, None, _ptr(perf), 0, st) == 0          # T = 0: nothing
        assert env.rollout_perf(0, "descent", perf=perf) is perf
        torch.cuda.synchronize()
        assert (perf == 7).all()
        after = env.get_state()
        for key in before:
            np.testing.assert_array_equal(before[key], after[key])
        buf = ctypes.create_string_buffer(64)
        assert L.mapf_rollout_perf_plan(env.h, 9, buf, 64) == -1
        assert L.mapf_rollout_perf_plan(env.h, 0, buf, 64) == 1
        # random and tape need no BFS maps
        assert off.rollout_perf(3, "random").shape == (off.B, 8)
    finally:
        close_all((env, off))


# ------------------------------------------------------------------ 7. fixed evaluation episodes
@pytest.mark.parametrize("policy", ["pibt", "descent"])
def test_evaluate_fixed_episodes_device(policy):
    from mapf_amd.episodes import (METRIC_KEYS, descent_policy, evaluate_fixed_episodes, evaluate_fixed_episodes_device,
                                   load_fixed_episode_infos, pibt_policy, _group_env, _groups_by_shape)
    from rollout_harness import G6
    infos = load_fixed_episode_infos(G6)
    steps = 48
    kw = dict(num_channel=6, fov=9, use_da=False, use_hp=False, human_movement_type=0, fix_choice=1)
    make = pibt_policy if policy == "pibt" else descent_policy
    want, tapes = evaluate_fixed_episodes(infos, make(), max_steps=steps, record_actions=True, keep_bfs=True, **kw)
    got = evaluate_fixed_episodes_device(infos, policy, max_steps=steps, **kw)
    assert set(got) == set(METRIC_KEYS)
    for key in METRIC_KEYS[2:]:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    rep = evaluate_fixed_episodes_device(infos, "tape", tapes=tapes, **kw)
    # the two float metrics: the float32-order numpy sum of a replay of the recorded actions
    for (H, W), idx in sorted(_groups_by_shape(infos).items()):
        env = _group_env(infos, idx, H, W, torch.device("cuda"), 6, 9, False, False, 0, 5, 1)
        try:
            o, _ = slot_rollout(env, steps, "tape", tape=tapes[(H, W)])
        finally:
            env.close()
        ref = np_perf(o)
        for k, key in enumerate(METRIC_KEYS):
            col = ref[:, k].copy().view(np.float32).astype(np.float64) if k < 2 else ref[:, k].astype(np.float64)
            np.testing.assert_array_equal(got[key][idx], col, err_msg=f"{policy} {key}")
            np.testing.assert_array_equal(rep[key][idx], col, err_msg=f"tape {key}")
