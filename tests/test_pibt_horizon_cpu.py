"""CPU checks of the PIBT policy's human horizon (mapf_set_pibt_human_horizon, mapf_get_pibt_human_horizon,
mapf_pibt_human_cells; include/mapf.h): the three functions are declared and bound, the entry points refuse
a null env and a horizon outside 1..8 without a device, the word the kernels take weight, radius,
constr_d2 and horizon in round-trips and is the horizon-less word at K = 1 (mapf_pibt_w_word, the
kernels' own pack / unpack functions on the host), BatchedMapfGym's and the runners' argument checks
raise before the library is reached, the restatement (tests/pibt_horizon_ref.py) at K = 1 is
pibt_human_ref's and at weight 0 pibt_ref's key for key, and the restated policy at weight 2, horizon 3
drives the oracle with the header's consequences intact and fewer constraint violations than horizon 1."""
import ctypes
import os
import re

import numpy as np
import pytest

import pibt_horizon_ref as PZ
import pibt_human_ref as PH
import pibt_ref
from oracle import oracle as O
from test_pibt_human_cpu import bare_env  # noqa: F401  (the fixture: an env shell whose library calls fail the test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapf.h")


def test_header_declares_and_lib_binds_the_three_functions():
    from mapf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+mapf_set_pibt_human_horizon\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    assert re.search(r"int\s+mapf_get_pibt_human_horizon\s*\(\s*const\s+mapf_env\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"int\s+mapf_pibt_human_cells\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", txt)
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["mapf_set_pibt_human_horizon"] == (ctypes.c_int, [P, I32])
    assert _lib.SIGNATURES["mapf_get_pibt_human_horizon"] == (ctypes.c_int, [P])
    assert _lib.SIGNATURES["mapf_pibt_human_cells"] == (ctypes.c_int, [P, P, P])
    assert re.search(r"#define\s+MAPF_ABI_VERSION\s+1\b", txt)       # functions are only added
    L = _lib.lib()
    for name in ("mapf_set_pibt_human_horizon", "mapf_get_pibt_human_horizon", "mapf_pibt_human_cells"):
        assert getattr(L, name) is not None


def test_c_calls_refuse_a_null_env_and_a_bad_horizon_without_a_device():
    from mapf_amd import _lib
    L = _lib.lib()
    for k in (0, 1, 3, 8, 9, -1):
        assert L.mapf_set_pibt_human_horizon(None, k) == -1
    assert L.mapf_get_pibt_human_horizon(None) == -1
    cells = (ctypes.c_uint32 * 8)()
    assert L.mapf_pibt_human_cells(None, ctypes.cast(cells, ctypes.c_void_p), None) == -1
    assert L.mapf_pibt_human_cells(None, None, None) == -1
    assert list(cells) == [0] * 8


def test_the_kernels_word_round_trips_and_is_the_old_word_at_horizon_1():
    """weight 8 bits | R 8 bits | constr_d2 12 bits | (K - 1) << 28, through the kernels' own functions."""
    from mapf_amd import _lib
    word = _lib.lib().mapf_pibt_w_word
    f = (ctypes.c_int32 * 4)()
    fp = ctypes.cast(f, ctypes.c_void_p)
    assert PH.constr_d2(64) == 4014                                  # the largest: it needs its 12 bits
    for R in range(1, 65):
        for cd2 in sorted({0, PH.constr_d2(R), 4095}):
            for w in (1, 2, 16):
                for K in range(1, 9):
                    got = word(w, R, cd2, K, fp)
                    assert got & 0xFFFFFFFF == w | (R << 8) | (cd2 << 16) | ((K - 1) << 28), (w, R, cd2, K)
                    assert list(f) == [w, R, cd2, K], (w, R, cd2, K, list(f))
                assert word(w, R, cd2, 1, None) == w | (R << 8) | (cd2 << 16)       # today's word
            for K in range(1, 9):                                    # weight 0: the kernels' "off", at any horizon
                assert word(0, R, cd2, K, fp) == 0 and list(f) == [0, 0, 0, 1]
    for bad in ((17, 5, 24, 1), (-1, 5, 24, 1), (2, 0, 24, 1), (2, 65, 24, 1), (2, 5, 4096, 1), (2, 5, -1, 1),
                (2, 5, 24, 0), (2, 5, 24, 9)):
        assert word(*bad, None) == -1, bad


# ------------------------------------------------------------------ the Python face
@pytest.mark.parametrize("k,exc", [(0, ValueError), (9, ValueError), (-1, ValueError), (1 << 40, ValueError), (3.0, TypeError),
                                   ("3", TypeError), (None, TypeError), (True, TypeError)])
def test_python_checks_raise_before_any_library_call(bare_env, k, exc):  # noqa: F811
    from mapf_amd.imitation import DemoRunner
    from mapf_amd.runner import DeviceRunner
    with pytest.raises(exc, match="human horizon"):
        bare_env.set_pibt_human_horizon(k)
    if k is None:
        return                                  # None means "leave the env's setting alone" below
    with pytest.raises(exc, match="human horizon"):
        DemoRunner(bare_env, 4, policy="pibt", human_horizon=k)
    with pytest.raises(exc, match="human horizon"):
        DeviceRunner(bare_env, None, 4, expert="pibt", expert_human_horizon=k)


def test_a_bad_cells_buffer_raises_before_any_library_call(bare_env):  # noqa: F811
    import torch
    with pytest.raises(TypeError, match="cells"):
        bare_env.pibt_human_cells(out=torch.zeros((3, 8), dtype=torch.float32))
    with pytest.raises(TypeError, match="cells"):
        bare_env.pibt_human_cells(out=np.zeros((3, 8), np.int32))


@pytest.mark.parametrize("policy", ["descent", "tape"])
def test_a_horizon_with_another_policy_or_expert_raises(bare_env, policy):  # noqa: F811
    from mapf_amd.imitation import DemoRunner
    from mapf_amd.runner import DeviceRunner
    with pytest.raises(ValueError, match="human_horizon"):
        DemoRunner(bare_env, 4, policy=policy, human_horizon=3)
    with pytest.raises(ValueError, match="expert_human_horizon"):
        DeviceRunner(bare_env, None, 4, expert=None if policy == "tape" else policy, expert_human_horizon=3)


def test_pibt_policy_sets_weight_and_horizon_on_the_env_it_is_called_with():
    from mapf_amd.episodes import pibt_policy

    class Env:
        class cfg:
            keep_bfs = 1

        def __init__(self):
            self.w, self.k, self.calls = 0, 1, []

        def set_pibt_human_weight(self, w):
            self.calls.append(("w", w))
            self.w = w

        def set_pibt_human_horizon(self, k):
            self.calls.append(("k", k))
            self.k = k

        def pibt_actions(self):
            return ("picked at", self.w, self.k)
    env = Env()
    assert pibt_policy()(None, None, env, 0) == ("picked at", 0, 1) and env.calls == []      # None: left alone
    pol = pibt_policy(human_weight=2, human_horizon=3)
    assert pol(None, None, env, 0) == ("picked at", 2, 3) and pol(None, None, env, 1) == ("picked at", 2, 3)
    assert env.calls == [("w", 2), ("k", 3)]
    other = Env()
    assert pol(None, None, other, 0) == ("picked at", 2, 3) and other.calls == [("w", 2), ("k", 3)]
    assert pibt_policy(human_horizon=5)(None, None, env, 2) == ("picked at", 2, 5)            # the weight left alone
    assert pibt_policy(human_weight=0)(None, None, env, 3) == ("picked at", 0, 5)             # and the horizon


# ------------------------------------------------------------------ the policy on the oracle
def c2_env(b):
    from mapf_amd.maps import generate_warehouse
    world = np.asarray(generate_warehouse(20, 20), np.int8)
    oe = O.OracleEnv(O.make_config(20, 20, 8, 11, 6, human_mode=1, goal_mode=1, fix_choice=1, seed=11), env_id=b)
    oe.reset_random(world)
    return world, oe


def drive(K, B, steps, w=2):
    """B envs x `steps` steps of the c2 shape (20 x 20 warehouse, 8 agents) under the restated policy at
    weight w and horizon K, from the same resets for every K.  Asserts the header's consequences at
    every step; returns (constraints, summed cost, goals, -2 count)."""
    constr = cost = goals = hits = 0
    for b in range(B):
        world, oe = c2_env(b)
        ages = pibt_ref.Ages(8)
        for t in range(steps):
            pos, _ = oe.agents()
            hum = oe.human()
            acts, failed, _ = PZ.pibt_actions(world, oe, t, ages, w, 5, K)
            out = oe.step(acts)
            st = out["status"]
            assert not ((st == -1) | (st == -3)).any(), (K, b, t, st)
            for i in np.flatnonzero(st == -2):
                assert i in failed and tuple(pos[i]) == tuple(hum["next"]), (K, b, t, i, st, failed)
            if not (st == -2).any():
                assert np.array_equal(out["fixed"], acts), (K, b, t, out["fixed"], acts)
            constr += int(np.sum(out["constr"]))
            cost += float(np.sum(out["cost"]))
            goals += int(np.sum(out["goals"]))
            hits += int((st == -2).sum())
        assert oe.errors() == 0
    return constr, cost, goals, hits


def test_restated_cells_are_the_humans_future_on_its_current_path():
    """P_1 is the oracle's `next`; the cells that follow are where the human stands 2, 3, ... steps later,
    for as long as it stays on the path it is on now; past that path's end there is none."""
    world, oe = c2_env(1)
    ages = pibt_ref.Ages(8)
    seen_short = seen_full = 0
    for t in range(64):
        hum, path = oe.human(), oe.human_path()
        assert tuple(path[hum["step"]]) == tuple(hum["pos"]) and hum["len"] == len(path)
        cells = PZ.human_cells(oe, 8)
        assert cells[0] == tuple(hum["next"])
        assert len(cells) == max(1, min(8, len(path) - 1 - hum["step"])), (t, hum, len(cells))
        assert cells[1:] == [tuple(c) for c in path[hum["step"] + 2:hum["step"] + 9]]
        packed = PZ.packed_cells(oe)
        assert [int(v) for v in packed[:len(cells)]] == [r | (c << 16) for r, c in cells] and (packed[len(cells):] == -1).all()
        seen_short += len(cells) < 8
        seen_full += len(cells) == 8
        oe.step(PZ.pibt_actions(world, oe, t, ages, 2, 5, 3)[0])
        assert tuple(oe.human()["pos"]) == cells[0]
        if len(cells) >= 2:                     # one step on, P_2 has become P_1
            assert tuple(oe.human()["next"]) == cells[1], t
    assert seen_short >= 5 and seen_full >= 5, (seen_short, seen_full)


def test_horizon_1_restates_the_weighted_policy_and_weight_0_the_plain_one():
    world, oe = c2_env(3)
    ages = pibt_ref.Ages(8)
    for t in range(24):
        pos, goal = oe.agents()
        hum = oe.human()
        bfs = oe.bfs()
        k1 = PZ.candidate_keys(world, bfs, pos, hum["pos"], PZ.human_cells(oe, 1), t, 2, 5)
        assert np.array_equal(k1, PH.candidate_keys(world, bfs, pos, hum["pos"], hum["next"], t, 2, 5))
        plain = pibt_ref.candidate_keys(world, bfs, pos, hum["pos"], hum["next"], t)
        for K in range(1, 9):
            assert np.array_equal(PZ.candidate_keys(world, bfs, pos, hum["pos"], PZ.human_cells(oe, K), t, 0, 5), plain), K
        oe.step(PZ.pibt_actions(world, oe, t, ages, 2, 5, 3)[0])


def test_restated_policy_at_horizon_3_keeps_the_guarantees_and_cuts_the_violations():
    """4 envs x 64 steps of the c2 shape at w = 2, horizon 3 and horizon 1 from the same resets: no -1, no
    -3, -2 only on a failed pick on hn, fixed == actions without a -2, no oracle error (asserted inside
    drive), and fewer constraint violations at horizon 3."""
    got = {K: drive(K, 4, 64) for K in (3, 1)}
    for K, (constr, cost, goals, hits) in got.items():
        print(f"K={K}: constraints {constr}, summed cost {cost:.1f}, goals {goals}, status -2 {hits}")
    assert got[3][0] < got[1][0], got
