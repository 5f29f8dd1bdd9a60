"""CPU checks of the PIBT policy's boundary (mapf_pibt_key, mapf_pibt_host, mapf_pibt_actions,
mapf_rollout_pibt, mapf_rollout_pibt_plan; include/mapf.h): the five functions are declared and bound,
the host key and the host solve equal the numpy restatement (tests/pibt_ref.py) -- the solve on 2,400
seeded random instances that hold, by the restatement's own count, hundreds of backtracks and failed
picks --, the entry points refuse null and bad arguments before any device call, BatchedMapfGym's
argument checks raise before the library is reached, and the restated policy drives the oracle with
the consequences the header states: no -1, no -3, -2 only on a failed pick standing on the human's
next cell, and actions_fixed == actions in every step without a -2."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import pibt_ref
from descent_ref import DC, DR, descent_actions
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapf.h")


def test_header_declares_and_lib_binds_the_five_functions():
    from mapf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+mapf_rollout_pibt\s*\(([^;]*)\)\s*;", txt)
    assert decl, "mapf_rollout_pibt is not declared"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 8 and args[3].replace(" ", "") == "int32_t*actions_out", args
    assert re.search(r"int\s+mapf_rollout_pibt_plan\s*\(\s*const\s+mapf_env\s*\*", txt)
    assert re.search(r"int\s+mapf_pibt_actions\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*void\s*\*", txt)
    assert re.search(r"int\s+mapf_pibt_key\s*\(\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", txt)
    host = re.search(r"int\s+mapf_pibt_host\s*\(([^;]*)\)\s*;", txt)
    assert host and len(host.group(1).split(",")) == 6 and "uint64_t" in host.group(1)
    P, I32, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    assert _lib.SIGNATURES["mapf_rollout_pibt"] == (ctypes.c_int, [P, I32, I32, P, ctypes.POINTER(_lib.StepOut), P, P, P])
    assert _lib.SIGNATURES["mapf_rollout_pibt_plan"] == (ctypes.c_int, [P, I32, ctypes.c_char_p, I32])
    assert _lib.SIGNATURES["mapf_pibt_actions"] == (ctypes.c_int, [P, P, P])
    assert _lib.SIGNATURES["mapf_pibt_key"] == (ctypes.c_int, [I32, I32, U32, I32])
    assert _lib.SIGNATURES["mapf_pibt_host"] == (ctypes.c_int, [I32, P, P, P, P, P])
    assert re.search(r"#define\s+MAPF_ABI_VERSION\s+1\b", txt)       # functions are only added


def test_host_key_equals_the_restatement():
    from mapf_amd import _lib
    key = _lib.lib().mapf_pibt_key
    for dist in (-2, -1, 0, 1, 0x7FFE):
        for a in range(5):
            for t in range(8):                      # every k0, with and without the agent's share
                for i in range(64):
                    assert key(dist, a, t, i) == pibt_ref.pibt_key(dist, a, t, i), (dist, a, t, i)
    # cost first, then stay, then descent's rotation; the five keys of an agent are distinct
    assert [key(3, a, 0, 0) for a in range(5)] == [24, 25, 26, 27, 28]
    assert [key(3, a, 1, 0) for a in range(5)] == [24, 28, 25, 26, 27]
    assert [key(3, 1, 0, i) for i in range(4)] == [25, 28, 27, 26]
    assert key(-2, 0, 0, 0) == key(-1, 0, 0, 0) == 0x7FFF * 8
    assert key(0, 1, 0xFFFFFFFF, 1) == 1                           # the sum wraps in 32 bits
    for t in range(4):
        assert len({key(5, a, t, 2) for a in range(5)}) == 5


# ------------------------------------------------------------------ the host solve
def random_instance(rng, n=None):
    """Agents on distinct cells of a g x g grid (3..8) at 30-90 % occupancy, keys of a random distance
    field (some cells unreachable) with each in-grid action admitted with probability 0.8 (off-grid
    never), ages in 0..3 so that ties are the rule."""
    g = int(rng.integers(3, 9))
    if n is None:
        n = int(np.clip(round(float(rng.uniform(0.3, 0.9)) * g * g), 1, 64))
    else:
        g = max(g, int(np.ceil(np.sqrt(n))))        # a given n: a grid that holds it
    cells = rng.permutation(g * g)[:n]
    pos = np.stack([cells // g, cells % g], 1).astype(np.int32)
    t = int(rng.integers(0, 1000))
    key = -np.ones((n, 5), np.int32)
    for i in range(n):
        goal = rng.integers(0, g, 2)
        for a in range(5):
            r, c = pos[i, 0] + DR[a], pos[i, 1] + DC[a]
            if 0 <= r < g and 0 <= c < g and rng.random() < 0.8:
                dist = -2 if rng.random() < 0.05 else abs(int(r) - int(goal[0])) + abs(int(c) - int(goal[1]))
                key[i, a] = pibt_ref.pibt_key(dist, a, t, i)
    age = rng.integers(0, 4, n).astype(np.uint32)
    return pos, key, age


@functools.lru_cache(maxsize=None)
def instances():
    rng = np.random.default_rng(0x91B7)
    out = [random_instance(rng, n) for n in (1, 1, 2, 64, 64)] + [random_instance(rng) for _ in range(2395)]
    return [(p, k, a, pibt_ref.solve(p, k, a)) for p, k, a in out]


def test_instance_set_meets_its_conditions_by_the_restatement_alone():
    inst = instances()
    assert len(inst) >= 2000
    sizes = {len(p) for p, _, _, _ in inst}
    assert 1 in sizes and 64 in sizes and len(sizes) >= 40, sorted(sizes)
    backtracks = sum(r[2]["backtracks"] for _, _, _, r in inst)
    failed = sum(len(r[1]) for _, _, _, r in inst)
    inherit = sum(r[2]["inherit"] for _, _, _, r in inst)
    print(f"{len(inst)} instances: {inherit} inheritance calls, {backtracks} backtracks, {failed} failed picks")
    assert backtracks >= 200 and failed >= 200, (backtracks, failed)
    assert any(len(set(a.tolist())) < len(a) for _, _, a, _ in inst)          # age ties


def test_host_solve_equals_the_restatement_on_every_instance():
    from mapf_amd import _lib
    host = _lib.lib().mapf_pibt_host
    for n_inst, (pos, key, age, (want, want_failed, stats, nxt)) in enumerate(instances()):
        n = len(pos)
        acts = np.full(n, -9, np.int32)
        failed = ctypes.c_uint64(0xDEAD)
        pos, key = np.ascontiguousarray(pos), np.ascontiguousarray(key)
        rc = host(n, pos.ctypes.data, key.ctypes.data, age.ctypes.data, acts.ctypes.data, ctypes.addressof(failed))
        assert rc == 0, (n_inst, rc)
        assert np.array_equal(acts, want), (n_inst, acts, want)
        assert failed.value == sum(1 << i for i in want_failed), (n_inst, failed.value, want_failed)
        # the policy's guarantees, on the host's own output
        cell = [(int(r), int(c)) for r, c in pos]
        tgt = [(cell[i][0] + DR[acts[i]], cell[i][1] + DC[acts[i]]) for i in range(n)]
        assert len(set(tgt)) == n, (n_inst, "two agents to one cell")
        at = {p: i for i, p in enumerate(cell)}
        for i in range(n):
            j = at.get(tgt[i])
            assert j is None or j == i or tgt[j] != cell[i], (n_inst, "swap", i, j)
            assert (acts[i] == 0 and i in want_failed) or key[i, acts[i]] >= 0, (n_inst, "not admitted", i)


def test_host_solve_refuses_bad_arguments():
    from mapf_amd import _lib
    host = _lib.lib().mapf_pibt_host
    pos = np.array([[0, 0], [0, 1]], np.int32)
    key = np.zeros((2, 5), np.int32)
    age = np.zeros(2, np.uint32)
    acts = np.zeros(2, np.int32)
    failed = ctypes.c_uint64(0)
    good = [2, pos.ctypes.data, key.ctypes.data, age.ctypes.data, acts.ctypes.data, ctypes.addressof(failed)]
    assert host(*good) == 0
    for k in range(1, 6):
        bad = list(good)
        bad[k] = None
        assert host(*bad) == -1, k
    for n in (0, -1, 65):
        assert host(n, *good[1:]) == -1, n
    same = np.array([[3, 4], [3, 4]], np.int32)
    assert host(2, same.ctypes.data, *good[2:]) == -1
    assert b"cell" in _lib.lib().mapf_last_error()


def test_c_calls_refuse_null_arguments_without_a_device():
    from mapf_amd import _lib
    L = _lib.lib()
    so = _lib.StepOut()
    assert L.mapf_pibt_actions(None, None, None) == -1
    assert L.mapf_rollout_pibt(None, 1, 0, None, ctypes.byref(so), None, None, None) == -1
    buf = ctypes.create_string_buffer(64)
    assert L.mapf_rollout_pibt_plan(None, 0, buf, 64) == -1


# ------------------------------------------------------------------ the Python face
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the argument checks")


@pytest.fixture
def bare_env(monkeypatch):
    """A BatchedMapfGym shell of B = 3, N = 2 with no handle: any library call fails the test."""
    from mapf_amd import _lib
    from mapf_amd.env import BatchedMapfGym
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    env = object.__new__(BatchedMapfGym)
    env.h = None
    env.B, env.N, env.F, env.C = 3, 2, 3, 6
    env.device = torch.device("cuda", 0)
    env.obs = env.vec = torch.zeros(1)      # never reached: the actions are checked first
    return env


@pytest.mark.parametrize("actions,exc", [
    (torch.zeros(3, 2, dtype=torch.int64), TypeError),                 # dtype
    (torch.zeros(3, 2, dtype=torch.int32), ValueError),                # a host tensor
    (torch.zeros(3, 4, dtype=torch.int32)[:, ::2], ValueError),        # not contiguous
    (torch.zeros(5, dtype=torch.int32), ValueError),                   # too small
])
def test_python_checks_raise_before_any_library_call(bare_env, actions, exc):
    with pytest.raises(exc, match="actions"):
        bare_env.pibt_actions(out=actions)
    with pytest.raises(exc, match="actions"):
        bare_env.rollout_pibt(4, actions=actions)
    with pytest.raises(exc, match="actions"):
        bare_env.rollout_launcher(4, actions=actions, policy="pibt")


def test_launcher_policy_and_tape_exclude_each_other(bare_env):
    tape = torch.zeros(4, 3, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        bare_env.rollout_launcher(4, actions_in=tape, policy="pibt")
    with pytest.raises(ValueError, match="'pibt'"):
        bare_env.rollout_launcher(4, policy="astar")
    with pytest.raises(ValueError, match="T must be"):
        bare_env.rollout_pibt(-1)


def test_pibt_policy_needs_keep_bfs():
    from mapf_amd.episodes import pibt_policy

    class Env:
        class cfg:
            keep_bfs = 0

        def pibt_actions(self):
            raise AssertionError("reached the library")
    with pytest.raises(RuntimeError, match="keep_bfs=True"):
        pibt_policy()(None, None, Env(), 0)


# ------------------------------------------------------------------ the policy on the oracle
def test_ages_follow_the_goal_and_are_idempotent_at_one_clock():
    ages = pibt_ref.Ages(2)
    g = np.array([[1, 1], [2, 2]])
    assert ages.update(g, 5).tolist() == [0, 0]                 # first seen
    assert ages.update(g, 5).tolist() == [0, 0]                 # the same clock again
    assert ages.update(g, 7).tolist() == [2, 2]
    g2 = np.array([[1, 1], [3, 3]])
    assert ages.update(g2, 8).tolist() == [3, 0]                # agent 1 has a new goal
    assert ages.update(g2, 2).tolist() == [0, 0]                # the clock ran back (a reset): seen anew
    ages.reset()
    assert ages.update(g2, 9).tolist() == [0, 0]


def test_restated_policy_drives_the_oracle_on_the_c2_shape():
    """64 steps of the c2 shape (20x20 warehouse, 8 agents) under the restated policy, against the
    oracle's outputs: the header's consequences, and more goals than the descent policy from the same
    reset."""
    from mapf_amd.maps import generate_warehouse
    world = np.asarray(generate_warehouse(20, 20), np.int8)
    cfg = O.make_config(20, 20, 8, 11, 6, human_mode=1, goal_mode=1, fix_choice=1, seed=11)
    goals = {}
    inherit = 0
    for policy in ("pibt", "descent"):
        oe = O.OracleEnv(cfg, env_id=0)
        oe.reset_random(world)
        ages = pibt_ref.Ages(8)
        total = 0
        for t in range(64):
            pos, goal = oe.agents()
            if policy == "descent":
                total += int(oe.step(descent_actions(oe.bfs(), pos, t))["goals"].sum())
                continue
            hum = oe.human()
            acts, failed, stats = pibt_ref.pibt_actions(world, oe.bfs(), pos, goal, hum["pos"], hum["next"], t, ages)
            inherit += stats["inherit"]
            out = oe.step(acts)
            st = out["status"]
            assert not ((st == -1) | (st == -3)).any(), (t, st)
            for i in np.flatnonzero(st == -2):
                assert i in failed and tuple(pos[i]) == tuple(hum["next"]), (t, i, st, failed)
            if not (st == -2).any():
                assert np.array_equal(out["fixed"], acts), (t, out["fixed"], acts)
            total += int(out["goals"].sum())
        assert oe.errors() == 0
        goals[policy] = total
    print(goals, "inheritance calls:", inherit)
    assert goals["pibt"] > goals["descent"], goals
