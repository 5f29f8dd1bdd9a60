"""CPU checks of the episode-metrics record (include/mapf.h: mapf_perf): the host arithmetic of
mapf_perf_add_host against the reference's own (`perf.episodeReward += np.sum(rewards)` in float32, integer
counts), chunking, the struct's layout against the ctypes mirror, the registry, and the argument validation of
BatchedMapfGym.rollout_perf / perf_accumulate / perf_dict without a device call (the shell of
test_rollout_policy_api.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 5, 7, 8, 9, 15, 16, 17, 64)
T = 6
SEED = 20240611
FIELDS = ("episode_reward", "episode_cost_reward", "human_collide", "static_collide", "agent_collide", "total_goals",
          "shadow_goals", "constraint_violations")


def draw_steps(n, steps, seed):
    """`steps` steps of n agents, as the step kernels fill them: statuses in {1, -1, -2, -3, -4}, reward_total
    from the config's cost constants (+ the goal reward where a goal was reached), cost (R - sqrt(d2)) / R in
    float64 rounded to float32, goals / constraints 0.f or 1.f, shadow_goals a count."""
    from mapf_amd.config import make_config
    c = make_config(1, 10, 10)
    rng = np.random.default_rng(seed + n)
    R = c.penalty_radius
    consts = {1: c.action_cost, -4: c.repeat_cost, -1: c.collision_cost, -3: c.collision_cost, -2: c.human_collision_cost}
    status = rng.choice(np.array([1, 1, 1, -1, -2, -3, -4], np.int8), size=(steps, n))
    goals = ((rng.random((steps, n)) < 0.2) & (status == 1)).astype(np.float32)
    rew = np.array([[consts[int(s)] for s in row] for row in status], np.float32)
    rew = np.where(goals == 1, rew + np.float32(c.goal_reward), rew).astype(np.float32)
    d2 = rng.integers(0, R * R + 8, size=(steps, n))
    cost = (np.maximum(R - np.sqrt(d2.astype(np.float64)), 0.0) / R).astype(np.float32)
    constr = (cost >= np.float32(0.01)).astype(np.float32)
    shadow = rng.integers(0, n + 1, size=steps).astype(np.int32)
    return dict(status=status, reward_total=rew, cost=cost, goals_reached=goals, constraints=constr, shadow_goals=shadow)


def reference_perf(d, t0=0, t1=None, start=None):
    """The reference's arithmetic (runner.py:64-99): float32 running sums of np.sum over the agents, counts."""
    t1 = len(d["status"]) if t1 is None else t1
    er, ec = (np.float32(0), np.float32(0)) if start is None else (np.float32(start[0]), np.float32(start[1]))
    counts = np.zeros(6, np.int64) if start is None else np.array(start[2:], np.int64)
    for t in range(t0, t1):
        er = er + np.sum(d["reward_total"][t].astype(np.float32))
        ec = ec + np.sum(d["cost"][t].astype(np.float32))
        st = d["status"][t]
        counts += [np.sum(st == -2), np.sum(st == -1), np.sum(st == -3), np.sum(d["goals_reached"][t] == 1),
                   d["shadow_goals"][t], np.sum(d["constraints"][t] == 1)]
    assert er.dtype == np.float32 and ec.dtype == np.float32
    return [np.float32(er), np.float32(ec)] + [int(x) for x in counts]


def bits(rec):
    return [np.float32(rec[0]).view(np.uint32), np.float32(rec[1]).view(np.uint32)] + [int(x) for x in rec[2:]]


def host_perf(d, t0, t1, perf=None):
    from mapf_amd import _lib
    p = _lib.Perf() if perf is None else perf
    n = d["status"].shape[1]
    fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for t in range(t0, t1):
        rows = [np.ascontiguousarray(d[k][t]) for k in ("status", "reward_total", "cost", "goals_reached", "constraints")]
        rc = _lib.lib().mapf_perf_add_host(ctypes.byref(p), n, fp(rows[0]), fp(rows[1]), fp(rows[2]), fp(rows[3]),
                                           int(d["shadow_goals"][t]), fp(rows[4]))
        assert rc == 0
    return p


def as_list(p):
    return [getattr(p, f) for f in FIELDS]


def inputs_where_left_to_right_differs():
    """Condition on the inputs: for at least one N >= 8 the plain left-to-right float32 sum of a step's values
    differs from np.sum, so that a sequential order could not pass the bit comparison below."""
    differs = []
    for n in NS:
        if n < 8:
            continue
        d = draw_steps(n, T, SEED)
        for key in ("reward_total", "cost"):
            for t in range(T):
                seq = np.float32(0)
                for x in d[key][t]:
                    seq = np.float32(seq + x)
                if seq.view(np.uint32) != np.float32(np.sum(d[key][t])).view(np.uint32):
                    differs.append((n, key, t))
    return differs


@pytest.mark.parametrize("n", NS)
def test_host_add_equals_the_reference_arithmetic_bit_for_bit(n):
    differs = inputs_where_left_to_right_differs()
    print("left-to-right differs from np.sum at", differs)
    assert differs, "the seed must make some N >= 8 tell numpy's order from a sequential one"
    d = draw_steps(n, T, SEED)
    got, want = as_list(host_perf(d, 0, T)), reference_perf(d)
    assert bits(got) == bits(want), (n, got, want)


@pytest.mark.parametrize("n", NS)
def test_chunks_with_the_record_carried_over_equal_one_pass(n):
    d = draw_steps(n, T, SEED)
    one = as_list(host_perf(d, 0, T))
    two = as_list(host_perf(d, 2, T, perf=host_perf(d, 0, 2)))
    assert bits(one) == bits(two)


def test_null_arrays_leave_their_metrics_alone():
    from mapf_amd import _lib
    d = draw_steps(9, 1, SEED)
    p = _lib.Perf(1.5, 2.5, 3, 4, 5, 6, 7, 8)
    cost = np.ascontiguousarray(d["cost"][0])
    assert _lib.lib().mapf_perf_add_host(ctypes.byref(p), 9, None, None, cost.ctypes.data_as(ctypes.c_void_p), None, -1,
                                         None) == 0
    want = np.float32(2.5) + np.sum(cost)
    assert as_list(p) == [1.5, float(want), 3, 4, 5, 6, 7, 8]
    assert _lib.lib().mapf_perf_add_host(None, 9, None, None, None, None, -1, None) == -1
    assert _lib.lib().mapf_perf_add_host(ctypes.byref(p), 0, None, None, None, None, -1, None) == -1


def test_layout_matches_the_ctypes_mirror_and_the_registry_has_the_symbols(tmp_path):
    from mapf_amd import _lib
    from mapf_amd.episodes import METRIC_KEYS
    src = tmp_path / "perf_layout.c"
    offs = ", ".join(f"offsetof(mapf_perf, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mapf.h"\n'
                   'int main(void){size_t v[] = {sizeof(mapf_perf), %s};'
                   ' for (int i = 0; i < 9; ++i) printf("%%zu ", v[i]); return 0;}\n' % offs)
    exe = tmp_path / "perf_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 32 == ctypes.sizeof(_lib.Perf)
    assert got[1:] == [getattr(_lib.Perf, f).offset for f in FIELDS] == [4 * k for k in range(8)]
    assert [f for f, _ in _lib.Perf._fields_] == list(FIELDS)
    # the field order is episodes.METRIC_KEYS' (camelCase there)
    assert [k.lower() for k in METRIC_KEYS] == [f.replace("_", "") for f in FIELDS]
    for name in ("mapf_perf_accumulate", "mapf_perf_add_host", "mapf_rollout_perf", "mapf_rollout_perf_plan"):
        assert name in _lib.SIGNATURES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


# ------------------------------------------------------------------ Python argument validation, no device call
B, N = 3, 2


class RecordingLibrary:
    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if symbol not in ("mapf_rollout_perf", "mapf_rollout_perf_plan", "mapf_perf_accumulate"):
            raise AssertionError(f"unexpected library call {symbol}")

        def fn(*args):
            self.calls.append((symbol, args))
            if symbol.endswith("plan"):
                args[2].value = f"{symbol}:{args[1]} form".encode()
            return 0
        return fn


@pytest.fixture
def shell(monkeypatch):
    from mapf_amd import _lib, env as env_mod
    lib = RecordingLibrary()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(env_mod, "_stream", lambda device: None)
    env = object.__new__(env_mod.BatchedMapfGym)
    env.h, env.device = None, torch.device("cpu")
    env.B, env.N = B, N
    return env, lib


def test_rollout_perf_validates_policy_tape_and_T(shell):
    env, lib = shell
    tape = torch.zeros(4, B, N, dtype=torch.int32)
    with pytest.raises(ValueError, match="descent.*pibt.*random.*tape"):
        env.rollout_perf(4, "nope")
    with pytest.raises(ValueError, match="nope"):
        env.rollout_perf_plan("nope")
    for policy in ("random", "descent", "pibt"):
        with pytest.raises(ValueError, match="tape"):
            env.rollout_perf(4, policy, tape=tape)
        with pytest.raises(ValueError, match="T must be >= 0"):
            env.rollout_perf(-1, policy)
    with pytest.raises(ValueError, match="tape"):
        env.rollout_perf(5, "tape", tape=tape)
    with pytest.raises(ValueError, match="tape"):
        env.rollout_perf(4, "tape", tape=torch.zeros(4, B, N + 1, dtype=torch.int32))
    with pytest.raises(TypeError, match="tape"):
        env.rollout_perf(4, "tape")
    with pytest.raises(ValueError, match="actions"):
        env.rollout_perf(4, "descent", actions=torch.zeros(3, B, N, dtype=torch.int32))
    with pytest.raises(ValueError, match="accumulate"):
        env.rollout_perf(4, "random", accumulate=True)
    assert lib.calls == []


def test_rollout_perf_validates_the_perf_tensor(shell):
    env, lib = shell
    with pytest.raises(TypeError, match="perf"):
        env.rollout_perf(4, perf=torch.zeros(B, 8, dtype=torch.float32))
    with pytest.raises(ValueError, match="perf"):
        env.rollout_perf(4, perf=torch.zeros(B + 1, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="perf"):
        env.rollout_perf(4, perf=torch.zeros(B, 8, dtype=torch.int32, device="meta"))
    with pytest.raises(TypeError, match="perf"):
        env.rollout_perf(4, perf=np.zeros((B, 8), np.int32))
    assert lib.calls == []


def test_rollout_perf_hands_policy_T_and_pointers_to_the_library(shell):
    env, lib = shell
    tape = torch.zeros(4, B, N, dtype=torch.int32)
    perf = torch.zeros(B, 8, dtype=torch.int32)
    acts = torch.zeros(6, B, N, dtype=torch.int32)
    assert env.rollout_perf(policy="tape", tape=tape, perf=perf, accumulate=True) is perf
    fresh = env.rollout_perf(6, "pibt", actions=acts)
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (B, 8) and not fresh.any()
    assert env.rollout_perf(0, "descent", perf=perf) is perf            # T = 0: no call
    assert env.rollout_perf_plan("descent") == "mapf_rollout_perf_plan:2 form"
    (s0, a0), (s1, a1), (s2, a2) = lib.calls
    assert (s0, s1, s2) == ("mapf_rollout_perf", "mapf_rollout_perf", "mapf_rollout_perf_plan")
    assert a0[1:3] == (1, 4) and a0[3].value == tape.data_ptr() and a0[4].value == perf.data_ptr() and a0[5] == 1
    assert a1[1:3] == (3, 6) and a1[3].value == acts.data_ptr() and a1[4].value == fresh.data_ptr() and a1[5] == 0
    env.rollout_perf(2, "random")
    assert lib.calls[-1][1][1:4] == (0, 2, None)                        # no actions asked for: NULL


def test_perf_accumulate_and_perf_dict_validate(shell):
    from mapf_amd.env import perf_accumulate, perf_dict
    from mapf_amd.episodes import METRIC_KEYS
    _, lib = shell
    out = dict(status=torch.zeros(5, B, N, dtype=torch.int8), cost=torch.zeros(5, B, N),
               shadow_goals=torch.zeros(5, B, dtype=torch.int32))
    perf = perf_accumulate(out)
    assert tuple(perf.shape) == (B, 8) and lib.calls[-1][1][1:4] == (5, B, N)
    so = lib.calls[-1][1][0]._obj
    assert so.status == out["status"].data_ptr() and so.cost == out["cost"].data_ptr() and not so.reward_total
    perf_accumulate(dict(status=torch.zeros(B, N, dtype=torch.int8)), perf=perf, accumulate=True)
    assert lib.calls[-1][1][1:4] == (1, B, N) and lib.calls[-1][1][5] == 1
    n = len(lib.calls)
    with pytest.raises(TypeError, match="status"):
        perf_accumulate(dict(status=torch.zeros(5, B, N), cost=torch.zeros(5, B, N)))
    with pytest.raises(ValueError, match="shadow_goals"):
        perf_accumulate(dict(cost=torch.zeros(5, B, N), shadow_goals=torch.zeros(4, B, dtype=torch.int32)))
    with pytest.raises(ValueError, match="none of"):
        perf_accumulate(dict(shadow_goals=torch.zeros(5, B, dtype=torch.int32)))
    with pytest.raises(ValueError, match="perf"):
        perf_accumulate(out, perf=torch.zeros(B, 7, dtype=torch.int32))
    assert len(lib.calls) == n
    p = torch.zeros(B, 8, dtype=torch.int32)
    p[:, 0] = int(np.float32(-1.25).view(np.int32))
    p[:, 7] = 9
    d = perf_dict(p)
    assert list(d) == list(METRIC_KEYS)
    assert d["episodeReward"].dtype == torch.float32 and d["episodeReward"].tolist() == [-1.25] * B
    assert d["constraintViolations"].dtype == torch.int32 and d["constraintViolations"].tolist() == [9] * B
    with pytest.raises(ValueError, match="perf"):
        perf_dict(torch.zeros(B, 8))
