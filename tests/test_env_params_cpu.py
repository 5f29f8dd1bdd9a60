"""CPU checks of penalty_radius and k_predict off their defaults: what mapf_create takes and refuses
(before any device call), and the oracle's radial cost and constraint threshold against a numpy float64
restatement of the reference (mapf_gym.py:513-526, 633) -- the reference side of
tests/test_gpu_env_params.py, which the golden vectors pin at R = 5 only."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O


def small_config(**kw):
    from mapf_amd.config import make_config
    return make_config(4, 10, 10, num_agents=2, fov=9, num_channel=6, use_da=True, use_hp=True, **kw)


@pytest.mark.parametrize("field,value", [("penalty_radius", 0), ("penalty_radius", 65), ("k_predict", -1), ("k_predict", 65)])
def test_create_refuses_out_of_range_before_any_device_call(field, value):
    """MAPF_EINVAL from check_config, which runs before hipSetDevice: the same answer with and without a GPU,
    and the handle stays null."""
    from mapf_amd import _lib
    L = _lib.lib()
    cfg = small_config(**{field: value})
    h = ctypes.c_void_p()
    assert L.mapf_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1
    assert field.encode() in L.mapf_last_error() and not h.value
    assert L.mapf_observe_lds(ctypes.byref(cfg), 0, 0, None) == -1        # the same checks, host only


@pytest.mark.parametrize("field,value", [("penalty_radius", 1), ("penalty_radius", 64), ("k_predict", 0), ("k_predict", 64)])
def test_create_accepts_the_ends_of_the_ranges(field, value):
    """The config passes mapf_create's checks: with a GPU the handle is created; without one the call
    gets as far as the device (MAPF_EDEVICE, -2), never MAPF_EINVAL."""
    from mapf_amd import _lib
    L = _lib.lib()
    cfg = small_config(**{field: value})
    assert getattr(cfg, field) == value
    assert L.mapf_observe_lds(ctypes.byref(cfg), 0, 0, None) > 0
    h = ctypes.c_void_p()
    rc = L.mapf_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if rc == 0:
        assert h.value
        assert L.mapf_destroy(h) == 0
    else:
        assert rc == -2 and b"hipSetDevice" in L.mapf_last_error(), (rc, L.mapf_last_error())


# ------------------------------------------------------------------ the oracle's radial cost
def radial_cost_normalized(R, human, robot):
    """calculateRadialConstraintCostNormalized (mapf_gym.py:513-526) in numpy float64."""
    return max(R - np.linalg.norm(np.asarray(human) - np.asarray(robot)), 0.0) / R


@pytest.mark.parametrize("R", [1, 2, 7, 8, 64])
def test_oracle_radial_cost_and_constraint_threshold(R):
    """64 idle agents on an empty 100x100 map, one to eight rows below the human's row, the LoopingHuman
    walking 73 cells past them and back: every step's cost is float32(max(R - |h' - x|, 0) / R) for the
    human's next cell h' (calculateCostReward: the emulated step of action 0 is the agent's cell) and
    `constraints` is int(that cost of the human's new cell >= 0.01) (jointStep, :633).  Distances 1..70
    occur, so every radius sees costs of zero and above; at R = 64 the shell 63.36 < d < 64 with a
    positive cost below the threshold occurs too (8^2 + 63^2 = 4033)."""
    H = W = 100
    n = 64
    world = np.zeros((H, W), np.int8)
    cfg = O.make_config(H, W, n, 9, 6, use_da=1, use_hp=1, human_mode=0, goal_mode=0, fix_choice=0, max_seq=2,
                        seed=3, penalty_radius=R)
    oe = O.OracleEnv(cfg)
    starts = [(50 + 1 + i % 8, 27 + 9 * (i // 8)) for i in range(n)]
    starts[0] = (50, 60)        # one agent in the human's way: distance 0, the only positive cost at R = 1
    seqs = [[s, (5 + i // 32, 5 + i % 32)] for i, s in enumerate(starts)]       # goals nobody walks to
    oe.reset_fixed(world, seqs, (50, 20), (50, 93))
    idle = np.zeros(n, np.int32)
    positive = zero = violated = shell = 0
    for t in range(80):
        nxt = oe.human()["next"]
        before, _ = oe.agents()
        o = oe.step(idle)
        want = np.array([radial_cost_normalized(R, nxt, p) for p in before])
        np.testing.assert_array_equal(o["cost"], want.astype(np.float32), err_msg=f"R={R} t={t}: cost")
        pos = oe.human()["pos"]
        after, _ = oe.agents()
        now = np.array([radial_cost_normalized(R, pos, p) for p in after])
        np.testing.assert_array_equal(o["constr"], (now >= 0.01).astype(np.float32), err_msg=f"R={R} t={t}: constraints")
        positive += int((want > 0).sum())
        zero += int((want == 0).sum())
        violated += int((now >= 0.01).sum())
        shell += int(((now > 0) & (now < 0.01)).sum())
    print(f"R={R}: cost > 0 in {positive} agent-steps, 0 in {zero}; constraints 1 in {violated}; 0 < cost < 0.01 in {shell}")
    assert positive > 0 and zero > 0
    assert violated > 0 or R == 1       # R = 1: only an agent sharing the human's cell, and fixActions moves it away
    assert (shell > 0) == (R == 64)       # no sum of two squares lies in the 1 % shell of R = 2, 7 or 8
    assert oe.errors() == 0
