"""CPU checks of the descent policy's boundary (mapf_descent_pick, mapf_descent_actions,
mapf_rollout_descent, mapf_rollout_descent_plan; include/mapf.h): the four functions are declared and
bound (tests/test_abi.py's export check then covers the build), the host pick equals the numpy
restatement (tests/descent_ref.py) for every mask, clock and agent and over whole BFS maps, the
device entry points refuse null arguments before any device call, BatchedMapfGym's argument checks
raise before the library is reached, and the restated policy is a sane driver of the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from descent_ref import DC, DR, descent_actions, descent_mask, descent_pick
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapf.h")


def test_header_declares_and_lib_binds_the_four_functions():
    from mapf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+mapf_rollout_descent\s*\(([^;]*)\)\s*;", txt)
    assert decl, "mapf_rollout_descent is not declared"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 8 and args[3].replace(" ", "") == "int32_t*actions_out", args
    assert re.search(r"int\s+mapf_rollout_descent_plan\s*\(\s*const\s+mapf_env\s*\*", txt)
    assert re.search(r"int\s+mapf_descent_actions\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*void\s*\*", txt)
    assert re.search(r"int\s+mapf_descent_pick\s*\(\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)", txt)
    P, I32, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    assert _lib.SIGNATURES["mapf_rollout_descent"] == (ctypes.c_int, [P, I32, I32, P, ctypes.POINTER(_lib.StepOut), P, P, P])
    assert _lib.SIGNATURES["mapf_rollout_descent_plan"] == (ctypes.c_int, [P, I32, ctypes.c_char_p, I32])
    assert _lib.SIGNATURES["mapf_descent_actions"] == (ctypes.c_int, [P, P, P])
    assert _lib.SIGNATURES["mapf_descent_pick"] == (ctypes.c_int, [U32, U32, I32])
    assert re.search(r"#define\s+MAPF_ABI_VERSION\s+1\b", txt)       # functions are only added


def test_host_pick_equals_the_restatement_for_every_mask_clock_and_agent():
    from mapf_amd import _lib
    pick = _lib.lib().mapf_descent_pick
    for m4 in range(16):
        mask = m4 << 1
        for t in range(8):
            for i in range(64):
                want = descent_pick(mask, t, i)
                assert pick(mask, t, i) == want, (mask, t, i)
                assert pick(mask | 1 | 0xFFFFFFE0, t, i) == want      # bits other than 1..4 are ignored
                assert (want == 0) == (m4 == 0) and (want == 0 or (mask >> want) & 1)
    # the rotation: one clock later (or the next agent) starts one move further round
    assert [pick(0b11110, t, 0) for t in range(8)] == [1, 2, 3, 4, 1, 2, 3, 4]
    assert [pick(0b11110, 0, i) for i in range(4)] == [1, 2, 3, 4]
    assert pick(0b11110, 0xFFFFFFFF, 1) == 1                        # the sum wraps in 32 bits


def small_maps():
    from mapf_amd.maps import generate_warehouse
    wh = np.asarray(generate_warehouse(10, 10), np.int8)
    rng = np.random.default_rng(3)
    rnd = -(rng.random((12, 12)) < 0.3).astype(np.int8)
    rnd[0:3, 0:3] = 0                       # a pocket no path leaves: free cells walled off
    rnd[3, 0:4] = -1
    rnd[0:4, 3] = -1
    rnd[6, 6] = 0
    corridor = -np.ones((3, 9), np.int8)
    corridor[1, :] = 0                      # one cell wide
    return [("warehouse_10x10", wh, (5, 0)), ("random_12x12_pocket", rnd, (6, 6)), ("corridor", corridor, (1, 6))]


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_host_pick_over_whole_bfs_maps(idx):
    """Cell by cell over oracle.bfs_map: the pick from the cell's descent mask equals the
    restatement's, leads exactly one level down, and is 0 exactly where the map says stay."""
    from mapf_amd import _lib
    pick = _lib.lib().mapf_descent_pick
    name, world, goal = small_maps()[idx]
    assert world[goal] == 0, name
    D = O.bfs_map(world, goal)
    H, W = D.shape
    assert D[goal] == 0
    if name == "random_12x12_pocket":
        assert (D[0:3, 0:3] == -2).all(), "the pocket is reachable"
    moved = 0
    for r in range(H):
        for c in range(W):
            mask = descent_mask(D, r, c)
            own = int(D[r, c])
            if own <= 0:                    # the goal, an obstacle (-1) or an unreachable free cell (-2)
                assert mask == 0, (name, r, c)
            for t in range(4):
                for i in (0, 1, 5):
                    a = pick(mask, t, i)
                    assert a == descent_pick(mask, t, i), (name, r, c, t, i)
                    if own > 0:
                        assert a != 0 and int(D[r + DR[a], c + DC[a]]) == own - 1, (name, r, c, t, i)
                        moved += 1
                    else:
                        assert a == 0
    assert moved > 0


def test_c_calls_refuse_null_arguments_without_a_device():
    from mapf_amd import _lib
    L = _lib.lib()
    so = _lib.StepOut()
    assert L.mapf_descent_actions(None, None, None) == -1
    assert L.mapf_rollout_descent(None, 1, 0, None, ctypes.byref(so), None, None, None) == -1
    buf = ctypes.create_string_buffer(64)
    assert L.mapf_rollout_descent_plan(None, 0, buf, 64) == -1


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
        bare_env.descent_actions(out=actions)
    with pytest.raises(exc, match="actions"):
        bare_env.rollout_descent(4, actions=actions)
    with pytest.raises(exc, match="actions"):
        bare_env.rollout_launcher(4, actions=actions, policy="descent")


def test_launcher_policy_and_tape_exclude_each_other(bare_env):
    tape = torch.zeros(4, 3, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        bare_env.rollout_launcher(4, actions_in=tape, policy="descent")
    with pytest.raises(ValueError, match="policy"):
        bare_env.rollout_launcher(4, policy="astar")
    with pytest.raises(ValueError, match="T must be"):
        bare_env.rollout_descent(-1)


def test_descent_policy_needs_keep_bfs():
    from mapf_amd.episodes import descent_policy

    class Env:
        class cfg:
            keep_bfs = 0

        def descent_actions(self):
            raise AssertionError("reached the library")
    with pytest.raises(RuntimeError, match="keep_bfs=True"):
        descent_policy()(None, None, Env(), 0)


def test_restated_policy_drives_the_oracle_sanely_on_the_c2_shape():
    """64 steps of the c2 shape (20x20 warehouse, 8 agents) under the restated policy: never a
    static-invalid move (-1: a descent move never enters an obstacle or leaves the map), no oracle
    error, and more goals than the oracle's own random policy from the same reset."""
    from mapf_amd.maps import generate_warehouse
    world = np.asarray(generate_warehouse(20, 20), np.int8)
    cfg = O.make_config(20, 20, 8, 11, 6, human_mode=1, goal_mode=1, fix_choice=1, seed=11)
    goals = {}
    for policy in ("descent", "random"):
        oe = O.OracleEnv(cfg, env_id=0)
        oe.reset_random(world)
        total = 0
        for t in range(64):
            acts = descent_actions(oe.bfs(), oe.agents()[0], t) if policy == "descent" else oe.random_actions()
            out = oe.step(acts)
            if policy == "descent":
                assert (out["status"] != -1).all(), (t, out["status"])
            total += int(out["goals"].sum())
        assert oe.errors() == 0
        goals[policy] = total
    assert goals["descent"] > goals["random"], goals
