"""CPU checks of the sparse rollout launcher (mapf_amd/env.py: rollout_launcher(sparse=True), the shadow
registry) and of the host function mapf_obs_sparse_applies.  A stand-in for the library records every
rollout call, as in test_rollout_policy_api.py; the env is a shell of B = 3 with c2's agent block
(N = 8, C = 6, F = 3: 27 pieces per env) on the CPU device."""
import ctypes

import pytest
import torch

B, N, C, F, T = 3, 8, 6, 3, 4


class RecordingLibrary:
    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if not symbol.startswith("mapf_rollout_"):
            raise AssertionError(f"unexpected library call {symbol}")

        def fn(*args):
            self.calls.append((symbol, args))
            return 0
        return fn


@pytest.fixture
def shell(monkeypatch):
    from mapf_amd import _lib, env as env_mod
    lib = RecordingLibrary()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(env_mod, "_stream", lambda device: None)
    env = object.__new__(env_mod.BatchedMapfGym)
    env.h, env.device, env._roll_fast, env.rollout_kernel = None, torch.device("cpu"), None, 1
    env.B, env.N, env.C, env.F, env.obs_words = B, N, C, F, 2
    env.actions = torch.zeros(B, N, dtype=torch.int32)
    env.obs, env.vec, env.out = torch.zeros(B, N, C, F, F), torch.zeros(B, N, 4), dict(reward=torch.zeros(B, N))
    env._stepout = env._make_stepout(env.out)
    return env, lib


def aligned_obs(steps):
    """float32 [steps * B, N, C, F, F] at a 64-byte aligned address, first byte of its storage's view base."""
    n = steps * B * N * C * F * F
    while True:
        t = torch.zeros(n)
        if t.data_ptr() % 64 == 0:
            return t.view(steps * B, N, C, F, F)
        keep.append(t)          # hold the misaligned block so that the allocator hands out another


keep = []


def buffers(steps=T, obs=None):
    return dict(actions=torch.zeros(steps, B, N, dtype=torch.int32), obs=aligned_obs(steps) if obs is None else obs,
                vec=torch.zeros(steps * B, N, 4), out=dict(reward=torch.zeros(steps * B, N)))


def summary(lib):
    """(symbol, slots bits) of a legacy call, ("sparse", T, valid) of a sparse one; clears the record."""
    out = []
    for sym, a in lib.calls:
        out.append(("sparse", a[2], a[8]) if sym == "mapf_rollout_sparse" else (sym, a[2]))
    del lib.calls[:]
    return out


def test_first_call_promises_nothing_later_calls_are_sparse(shell):
    env, lib = shell
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **buf)
    assert lib.calls == []
    for _ in range(3):
        assert launch()[1] is buf["obs"]
    args = lib.calls[0][1]
    assert args[1] == 0 and args[5].value == buf["obs"].data_ptr() and args[7].value == launch.sparse.shadow.data_ptr()
    assert tuple(launch.sparse.shadow.shape) == (T, B, 16) and launch.sparse.shadow.dtype == torch.int32
    assert summary(lib) == [("sparse", T, 0), ("sparse", T, T), ("sparse", T, T)]


@pytest.mark.parametrize("policy,number", [("random", 0), ("tape", 1), ("descent", 2), ("pibt", 3)])
def test_every_policy_reaches_the_sparse_entry_point_with_its_number(shell, policy, number):
    env, lib = shell
    tape = torch.zeros(T, B, N, dtype=torch.int32)
    kw = dict(actions_in=tape) if policy == "tape" else dict(policy=policy)
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **kw, **buf)
    launch()
    sym, args = lib.calls[0]
    assert sym == "mapf_rollout_sparse" and args[1] == number
    assert args[3].value == (tape if policy == "tape" else buf["actions"]).data_ptr()


def test_a_torch_write_gets_one_band_call_then_a_store_all_call(shell):
    env, lib = shell
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **buf)
    launch()
    launch()
    buf["obs"].fill_(7.0)               # every view's _version moves
    launch()                            # today's form: the band bit, since this launcher has stored the band
    launch()                            # the shadow said nothing: everything stored, and recorded
    launch()
    assert summary(lib) == [("sparse", T, 0), ("sparse", T, T), ("mapf_rollout_random", 3), ("sparse", T, 0), ("sparse", T, T)]
    buf["obs"][:B].zero_()              # a write through a view counts as well
    launch()
    assert summary(lib) == [("mapf_rollout_random", 3)]


def test_a_write_before_the_first_call_gets_the_unflagged_form(shell):
    env, lib = shell
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **buf)
    buf["obs"].fill_(float("nan"))
    launch()
    launch()
    assert summary(lib) == [("mapf_rollout_random", 1), ("sparse", T, 0)]


def test_invalidate_forgets_the_shadow_and_the_band(shell):
    env, lib = shell
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **buf)
    launch()
    launch.invalidate()
    launch()
    launch()
    assert summary(lib) == [("sparse", T, 0), ("sparse", T, 0), ("sparse", T, T)]
    launch.invalidate()
    buf["obs"].fill_(1.0)               # and a torch write on top of it: the unflagged form, not the band one
    launch()
    assert summary(lib) == [("mapf_rollout_random", 1)]


def test_another_rollout_call_into_the_buffer_resets_valid(shell):
    env, lib = shell
    buf = buffers()
    launch = env.rollout_launcher(T, slots=True, **buf)
    launch()
    assert launch.sparse.valid == T
    env.rollout(T, "random", slots=True, **buf)
    assert launch.sparse.valid == 0
    launch()
    env.rollout_descent(2, slots=True, actions=buf["actions"][:2], obs=buf["obs"][:2 * B], vec=buf["vec"][:2 * B],
                        out=dict(reward=buf["out"]["reward"][:2 * B]))
    assert launch.sparse.valid == 0
    launch()
    shadow = torch.zeros(T, B, 16, dtype=torch.int32)
    env.rollout_sparse(T, shadow=shadow, valid=0, **buf)
    assert launch.sparse.valid == 0
    assert [s[0] for s in summary(lib)] == ["sparse", "mapf_rollout_random", "sparse", "mapf_rollout_descent", "sparse", "sparse"]


def test_launchers_over_views_of_one_buffer_share_the_entry(shell):
    env, lib = shell
    buf = buffers()
    head = dict(actions=buf["actions"][:2], obs=buf["obs"][:2 * B], vec=buf["vec"][:2 * B],
                out=dict(reward=buf["out"]["reward"][:2 * B]))
    short, full = env.rollout_launcher(2, slots=True, **head), env.rollout_launcher(T, slots=True, **buf)
    assert short.sparse is full.sparse and tuple(full.sparse.shadow.shape) == (T, B, 16)
    short()
    full()
    short()
    full()
    assert summary(lib) == [("sparse", 2, 0), ("sparse", T, 2), ("sparse", 2, T), ("sparse", T, T)]
    from mapf_amd import env as env_mod
    key = env_mod._sparse_key(buf["obs"])
    assert key in env_mod._SPARSE
    del short, full
    assert key not in env_mod._SPARSE    # the entry dies with its last launcher


def test_sparse_false_and_in_place_launchers_keep_the_band_form(shell):
    env, lib = shell
    launch = env.rollout_launcher(T, slots=True, sparse=False, **buffers())
    for call in range(4):
        if call == 3:
            launch.invalidate()
        launch()
    assert summary(lib) == [("mapf_rollout_random", 1), ("mapf_rollout_random", 3), ("mapf_rollout_random", 3),
                            ("mapf_rollout_random", 1)]
    assert not hasattr(launch, "sparse")
    inplace = env.rollout_launcher(T)
    inplace()
    inplace()
    assert summary(lib) == [("mapf_rollout_random", 0)] * 2 and not hasattr(inplace, "sparse")


def test_views_the_registry_cannot_express_get_the_band_form(shell):
    env, lib = shell
    big = aligned_obs(T + 1)
    tail = big[B:]                      # whole slots, 64-byte aligned (a slot is 3 * 27 pieces), but not from the base
    assert tail.data_ptr() % 64 == 0
    launch = env.rollout_launcher(T, slots=True, **buffers(obs=tail))
    launch()
    launch()
    assert summary(lib) == [("mapf_rollout_random", 1), ("mapf_rollout_random", 3)] and not hasattr(launch, "sparse")
    # another geometry over a registered buffer
    first = env.rollout_launcher(T, slots=True, **buffers(obs=big[:T * B]))
    env.B = 1
    other = env.rollout_launcher(T * 3, slots=True, actions=torch.zeros(T * 3, 1, N, dtype=torch.int32), obs=big[:T * B],
                                 vec=torch.zeros(T * 3, N, 4), out=dict(reward=torch.zeros(T * 3 * B, N)))
    assert hasattr(first, "sparse") and not hasattr(other, "sparse")
    # the pair-lane kernel does not run, or the slice is no whole number of pieces
    env.B, env.rollout_kernel = B, 2
    assert not hasattr(env.rollout_launcher(T, slots=True, **buffers()), "sparse")
    env.rollout_kernel, env.N = 1, 6
    obs6 = torch.zeros(T * B, 6, C, F, F)
    launch = env.rollout_launcher(T, slots=True, actions=torch.zeros(T, B, 6, dtype=torch.int32), obs=obs6,
                                  vec=torch.zeros(T * B, 6, 4), out=dict(reward=torch.zeros(T * B, N)))
    assert not hasattr(launch, "sparse")


@pytest.mark.parametrize("n", [5, 6, 7, 8])
@pytest.mark.parametrize("c", [5, 6, 7])
def test_the_host_applicability_function(n, c):
    """Whole 64-byte pieces per env and a 64-byte aligned buffer: with odd FOVs, N = 8 and an even C."""
    from mapf_amd import _lib
    from mapf_amd.config import make_config
    from mapf_amd.env import sparse_applies
    fn = _lib.lib().mapf_obs_sparse_applies
    for fov in (3, 5, 7, 9, 11):
        cfg = make_config(4, 20, 20, num_agents=n, fov=fov, num_channel=c)
        for address in (0, 16, 64, 4096, 4096 + 32, 1 << 40):
            want = (n * c * fov * fov) % 16 == 0 and address % 64 == 0
            assert want == (n == 8 and c % 2 == 0 and address % 64 == 0)
            assert fn(ctypes.byref(cfg), address) == int(want), (n, c, fov, address)
            assert sparse_applies(n, c, fov, address) == want
    assert fn(None, 0) == -1


def test_the_header_declares_the_three_functions_and_the_bindings_match():
    import os
    import re
    from mapf_amd import _lib
    txt = open(os.path.join(os.path.dirname(__file__), "..", "include", "mapf.h")).read()
    for name in ("mapf_rollout_sparse", "mapf_rollout_sparse_plan", "mapf_obs_sparse_applies"):
        assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mapf_rollout_sparse"][1]) == 10
