"""CPU checks of action noise (mapf_set_action_noise, mapf_get_action_noise, mapf_noise_actions,
mapf_action_noise_pick; include/mapf.h): the four functions are declared and bound, the host pick -- the
function the kernels run -- equals the numpy restatement over the oracle's Philox words
(tests/explore_ref.py) on the whole grid of envs, agents, clocks, labels and noise levels, the noisy flag
has the stated frequency and is independent of the action drawn, the entry points refuse bad arguments
without a device, and the Python face raises before the library is reached."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import explore_ref as X
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapf.h")
SEED = 0x9E3779B97F4A7C15          # both key words in use
ENVS, AGENTS, CLOCKS = 64, 64, 64
Q16S = (0, 1, 16384, 65535, 65536)


@pytest.fixture(scope="module")
def draws():
    """u [env, agent, clock] (the explore half-word) and rnd [env, agent, clock] (the random policy's action)
    from the oracle's Philox words, computed once and read-only."""
    u = np.zeros((ENVS, AGENTS, CLOCKS), np.int64)
    rnd = np.zeros((ENVS, AGENTS, CLOCKS), np.int32)
    for e in range(ENVS):
        for i in range(AGENTS):
            for t in range(CLOCKS):
                u[e, i, t] = X.half(X.P_NOISE, e, i, t, SEED)
                rnd[e, i, t] = X.random_action(e, i, t, SEED)
    u.setflags(write=False)
    rnd.setflags(write=False)
    return u, rnd


def test_header_declares_and_lib_binds_the_four_functions():
    from mapf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+mapf_set_action_noise\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    assert re.search(r"int\s+mapf_get_action_noise\s*\(\s*const\s+mapf_env\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"int\s+mapf_noise_actions\s*\(\s*mapf_env\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"int\s+mapf_action_noise_pick\s*\(\s*uint64_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    P, I32, U32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    assert _lib.SIGNATURES["mapf_set_action_noise"] == (ctypes.c_int, [P, I32])
    assert _lib.SIGNATURES["mapf_get_action_noise"] == (ctypes.c_int, [P])
    assert _lib.SIGNATURES["mapf_noise_actions"] == (ctypes.c_int, [P, P, P, P])
    assert _lib.SIGNATURES["mapf_action_noise_pick"] == (ctypes.c_int, [ctypes.c_uint64, U32, I32, U32, I32, I32])
    assert re.search(r"#define\s+MAPF_ABI_VERSION\s+1\b", txt)       # functions are only added
    L = _lib.lib()
    for name in ("mapf_set_action_noise", "mapf_get_action_noise", "mapf_noise_actions", "mapf_action_noise_pick"):
        assert getattr(L, name) is not None


def test_restated_random_action_is_the_oracles():
    """explore_ref's random action from the Philox words is OracleEnv.random_actions() (the oracle's clock 0)."""
    cfg = O.make_config(12, 12, 16, 9, 6, human_mode=1, goal_mode=1, fix_choice=1, seed=SEED)
    world = np.zeros((12, 12), np.int8)
    for env_id in (0, 7, 40):
        oe = O.OracleEnv(cfg, env_id=env_id)
        oe.reset_random(world)
        for t in range(3):
            want = oe.random_actions()
            assert [X.random_action(env_id, i, t, SEED) for i in range(16)] == want.tolist(), (env_id, t)
            lab = np.full(16, 4, np.int32)
            assert np.array_equal(X.played(lab, env_id, t, SEED, 65536, random=want), want)
            assert np.array_equal(X.played(lab, env_id, t, SEED, 65536), want)
            assert np.array_equal(X.played(lab, env_id, t, SEED, 0), lab)
            oe.step(want)


def test_host_pick_equals_the_restatement(draws):
    """Env ids 0..40, agents 0..63, clocks 0..63, labels 0..4 at every q16 of Q16S; 0 returns the label,
    65536 the random action."""
    from mapf_amd import _lib
    pick = _lib.lib().mapf_action_noise_pick
    u, rnd = draws
    bad = 0
    for q16 in Q16S:
        for e in range(41):
            for i in range(AGENTS):
                ue, re_ = u[e, i].tolist(), rnd[e, i].tolist()
                for t in range(CLOCKS):
                    hit, r = ue[t] < q16, re_[t]
                    for label in range(5):
                        bad += pick(SEED, e, i, t, q16, label) != (r if hit else label)
        if q16 == 0:
            assert not (u[:41] < q16).any()
        if q16 == 65536:
            assert (u[:41] < q16).all()
        assert bad == 0, q16


def test_the_restatement_through_played_is_the_same_rule(draws):
    """explore_ref.played (what the GPU tests step the oracle with) over rows of labels equals the grid."""
    u, rnd = draws
    rng = np.random.default_rng(5)
    for e in (0, 9, 40):
        for t in (0, 1, 63):
            lab = rng.integers(0, 5, AGENTS).astype(np.int32)
            for q16 in Q16S:
                want = np.where(u[e, :, t] < q16, rnd[e, :, t], lab)
                assert np.array_equal(X.played(lab, e, t, SEED, q16), want), (e, t, q16)


def test_noisy_frequency_and_independence_from_the_action(draws):
    u, rnd = draws
    n = ENVS * AGENTS * CLOCKS
    assert n == 262144
    hit = u < 16384
    count = int(hit.sum())
    print(f"noisy: {count} of {n} (n/4 = {n // 4})")
    assert abs(count - n // 4) <= 1109                  # 5 sigma, sigma = sqrt(n * 0.25 * 0.75) = 221.7
    # among the noisy triples each random action takes 0.2 +- 5 sigma of its own binomial
    k = count
    sigma = np.sqrt(k * 0.2 * 0.8)
    shares = [int((rnd[hit] == a).sum()) for a in range(5)]
    print(f"random actions among the noisy: {shares}, 5 sigma = {5 * sigma:.0f}")
    for a, c in enumerate(shares):
        assert abs(c - 0.2 * k) <= 5 * sigma, (a, c, k)
    # agents 7 and 8 are in different draw groups: their flags are not one word's
    for i, j in ((7, 8), (0, 8), (15, 16), (55, 63)):
        differ = int((hit[:, i] != hit[:, j]).sum())
        print(f"agents {i} and {j}: flags differ in {differ} of {ENVS * CLOCKS} (env, clock) pairs")
        # two independent flags at p = 1/4 differ with probability 3/8: 1536 of 4096, sigma = 31
        assert abs(differ - 1536) <= 155, (i, j, differ)
    # and the explore half-word is not the action's half-word (another purpose, another draw)
    same = int(((u * 5) >> 16 == rnd).sum())
    assert abs(same - n / 5) <= 5 * np.sqrt(n * 0.2 * 0.8), same


def test_c_calls_refuse_bad_arguments_without_a_device():
    from mapf_amd import _lib
    L = _lib.lib()
    assert L.mapf_set_action_noise(None, 1) == -1
    assert L.mapf_get_action_noise(None) == -1
    buf = (ctypes.c_int32 * 4)()
    assert L.mapf_noise_actions(None, buf, buf, None) == -1
    assert b"null" in L.mapf_last_error()
    for agent, q16, label in ((-1, 5, 0), (64, 5, 0), (0, -1, 0), (0, 65537, 0), (0, 5, -1), (0, 5, 5), (1 << 30, 5, 0)):
        assert L.mapf_action_noise_pick(SEED, 0, agent, 0, q16, label) == -1, (agent, q16, label)
    assert L.mapf_action_noise_pick(SEED, 0xFFFFFFFF, 63, 0xFFFFFFFF, 65536, 4) in range(5)


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
    env.obs = env.vec = torch.zeros(1)

    class cfg:
        keep_bfs = 1
    env.cfg = cfg
    return env


def test_q16_of_eps():
    from mapf_amd.env import noise_q16
    assert [noise_q16(e) for e in (0, 0.0, 0.25, 0.05, 0.1, 1, 1.0)] == [0, 0, 16384, 3277, 6554, 65536, 65536]
    assert noise_q16(q16=0) == 0 and noise_q16(q16=65536) == 65536 and noise_q16(q16=np.int32(7)) == 7
    for bad in (dict(), dict(eps=0.5, q16=3)):
        with pytest.raises(ValueError, match="action noise"):
            noise_q16(**bad)


@pytest.mark.parametrize("eps,exc", [(-0.01, ValueError), (1.0001, ValueError), (float("nan"), ValueError), (2, ValueError),
                                     ("0.5", TypeError), (True, TypeError), ([0.5], TypeError)])
def test_eps_outside_0_1_raises_before_any_library_call(bare_env, eps, exc):
    from mapf_amd.episodes import noisy_policy
    from mapf_amd.imitation import DemoRunner
    with pytest.raises(exc, match="action noise"):
        bare_env.set_action_noise(eps)
    for policy in ("descent", "pibt"):
        with pytest.raises(exc, match="action noise"):
            bare_env.rollout(4, policy, noise=eps)
        with pytest.raises(exc, match="action noise"):
            bare_env.rollout_perf(4, policy, noise=eps)
        with pytest.raises(exc, match="action noise"):
            bare_env.rollout_launcher(4, policy=policy, noise=eps)
        with pytest.raises(exc, match="action noise"):
            DemoRunner(bare_env, 4, policy=policy, noise=eps)
    with pytest.raises(exc, match="action noise"):
        noisy_policy(lambda *a: None, eps)


@pytest.mark.parametrize("q16,exc", [(-1, ValueError), (65537, ValueError), (1 << 40, ValueError), (0.5, TypeError), (True, TypeError)])
def test_q16_outside_its_range_raises_before_any_library_call(bare_env, q16, exc):
    with pytest.raises(exc, match="action noise"):
        bare_env.set_action_noise(q16=q16)


@pytest.mark.parametrize("policy", ["random", "tape"])
def test_noise_with_the_random_or_tape_policy_raises(bare_env, policy):
    from mapf_amd.episodes import evaluate_fixed_episodes_device
    from mapf_amd.imitation import DemoRunner
    tape = torch.zeros(4, 3, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="noise="):
        bare_env.rollout(4, policy, noise=0.25, tape=tape if policy == "tape" else None)
    with pytest.raises(ValueError, match="noise="):
        bare_env.rollout_perf(4, policy, noise=0.25, tape=tape if policy == "tape" else None)
    with pytest.raises(ValueError, match="noise="):
        bare_env.rollout_launcher(4, policy=policy, noise=0.25)
    with pytest.raises(ValueError, match="noise="):
        bare_env.rollout_launcher(4, actions_in=tape, noise=0.25)
    if policy == "tape":
        with pytest.raises(ValueError, match="noise="):
            DemoRunner(bare_env, 4, policy="tape", noise=0.25)
        with pytest.raises(ValueError, match="noise="):
            evaluate_fixed_episodes_device({"numEpisodes": 0}, "tape", tapes={}, noise=0.25)


def test_noisy_policy_sets_the_noise_once_per_env_and_plays_the_noised_labels():
    from mapf_amd.episodes import noisy_policy

    class Env:
        def __init__(self):
            self.calls = []

        def set_action_noise(self, eps=None, *, q16=None):
            self.calls.append(("set", eps, q16))

        def noise_actions(self, labels):
            self.calls.append(("noise", labels))
            return ("played", labels)
    env, other = Env(), Env()
    pol = noisy_policy(lambda obs, vec, e, t: ("label", t), 0.25)
    assert pol(None, None, env, 0) == ("played", ("label", 0))
    assert pol(None, None, env, 1) == ("played", ("label", 1))
    assert env.calls == [("set", None, 16384), ("noise", ("label", 0)), ("noise", ("label", 1))]
    assert pol(None, None, other, 0) == ("played", ("label", 0)) and other.calls[0] == ("set", None, 16384)
