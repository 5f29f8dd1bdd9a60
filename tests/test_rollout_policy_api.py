"""CPU checks of the rollout policy parameter of BatchedMapfGym (mapf_amd/env.py: ROLLOUT_POLICIES,
rollout, rollout_plan, rollout_kernel_name, rollout_launcher) and of the eleven per-policy names that
delegate to it.  A stand-in for the library records (symbol, arguments) of every rollout and plan
call; the env is a shell of B = 3, N = 2 on the CPU device with the attributes _rollout_buffers reads,
and env._stream is replaced (a CPU device has no stream), so host tensors pass the buffer checks."""
import itertools

import pytest
import torch

# policy -> (C rollout, C plan, rollout method, plan method, kernel-name method): what each name reached before the table
LEGACY = {"random": ("mapf_rollout_random", "mapf_rollout_plan", "rollout_random", "rollout_plan", None),
          "tape": ("mapf_rollout_actions", "mapf_rollout_actions_plan", "rollout_actions", "rollout_actions_plan",
                   "rollout_actions_kernel_name"),
          "descent": ("mapf_rollout_descent", "mapf_rollout_descent_plan", "rollout_descent", "rollout_descent_plan",
                      "rollout_descent_kernel_name"),
          "pibt": ("mapf_rollout_pibt", "mapf_rollout_pibt_plan", "rollout_pibt", "rollout_pibt_plan",
                   "rollout_pibt_kernel_name")}
FLAGS = list(itertools.product([False, True], repeat=3))         # slots, band_clean, obs_bits
B, N, C, F, WPA, T = 3, 2, 6, 3, 2, 4


class RecordingLibrary:
    """Every mapf_rollout_* attribute is a function that records (symbol, args); a plan call also
    writes "<symbol>:<slots> form" into its buffer.  Any other symbol is an error."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        if not symbol.startswith("mapf_rollout_"):
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
    env.h, env.device, env._roll_fast = None, torch.device("cpu"), None
    env.B, env.N, env.C, env.F, env.obs_words = B, N, C, F, WPA
    env.actions = torch.zeros(B, N, dtype=torch.int32)
    env.obs, env.vec, env.out = torch.zeros(B, N, C, F, F), torch.zeros(B, N, 4), dict(reward=torch.zeros(B, N))
    env.bits = torch.zeros(B, N, WPA, dtype=torch.int32)
    env._stepout = env._make_stepout(env.out)
    return env, lib


def buffers(slots, obs_bits=False):
    k = T if slots else 1
    obs = torch.zeros(k * B, N, WPA, dtype=torch.int32) if obs_bits else torch.zeros(k * B, N, C, F, F)
    return dict(obs=obs, vec=torch.zeros(k * B, N, 4), out=dict(reward=torch.zeros(k * B, N)))


def test_the_table_names_the_four_policies_and_their_bound_symbols():
    from mapf_amd import _lib
    from mapf_amd.env import ROLLOUT_POLICIES
    assert ROLLOUT_POLICIES == {p: names[:2] for p, names in LEGACY.items()}
    assert all(s in _lib.SIGNATURES for names in LEGACY.values() for s in names[:2])


@pytest.mark.parametrize("policy", list(LEGACY))
@pytest.mark.parametrize("slots,band_clean,obs_bits", FLAGS)
def test_every_legacy_name_reaches_its_symbol_with_the_same_slot_bits(shell, policy, slots, band_clean, obs_bits):
    env, lib = shell
    c_rollout, c_plan, roll_name, plan_name, kernel_name = LEGACY[policy]
    # MAPF_SLOTS_* (include/mapf.h): 1 slots, 2 band clean (with slots only), 4 packed observations
    want = (1 | (2 if band_clean else 0) if slots else 0) | (4 if obs_bits else 0)
    buf = buffers(slots, obs_bits)
    tape = torch.zeros(T, B, N, dtype=torch.int32)
    acts = torch.zeros(T if slots else 1, B, N, dtype=torch.int32)
    if policy == "tape":            # the legacy name, arguments in their old positions, then the one entry point
        got = env.rollout_actions(tape, slots, band_clean=band_clean, obs_bits=obs_bits, **buf)
        env.rollout(policy="tape", tape=tape, slots=slots, band_clean=band_clean, obs_bits=obs_bits, **buf)
    else:
        got = getattr(env, roll_name)(T, slots, acts, band_clean=band_clean, obs_bits=obs_bits, **buf)
        env.rollout(T, policy, slots=slots, actions=acts, band_clean=band_clean, obs_bits=obs_bits, **buf)
    assert got[0] is buf["out"] and got[1] is buf["obs"] and got[2] is buf["vec"]
    assert [(s, a[1:3]) for s, a in lib.calls] == [(c_rollout, (T, want))] * 2
    args = lib.calls[0][1]
    assert args[3].value == (tape if policy == "tape" else acts).data_ptr()
    assert args[5].value == buf["obs"].data_ptr() and args[6].value == buf["vec"].data_ptr()
    # the plan and the kernel name: callers pass slots, band_clean positionally
    del lib.calls[:]
    text = f"{c_plan}:{want} form"
    assert getattr(env, plan_name)(slots, band_clean, obs_bits) == text
    assert env.rollout_plan(slots, band_clean, obs_bits, policy=policy) == text
    assert env.rollout_kernel_name(slots, obs_bits, band_clean=band_clean, policy=policy) == text.split(" ")[0]
    if kernel_name is not None:
        assert getattr(env, kernel_name)(slots, band_clean, obs_bits) == text.split(" ")[0]
    else:                           # rollout_kernel_name(slots, obs_bits): never the band bit
        assert env.rollout_kernel_name(slots, obs_bits) == f"{c_plan}:{want & ~2}"
    assert {s for s, _ in lib.calls} == {c_plan}


@pytest.mark.parametrize("policy", list(LEGACY))
def test_the_launcher_takes_its_function_from_the_table(shell, policy):
    env, lib = shell
    tape, acts = torch.zeros(T, B, N, dtype=torch.int32), torch.zeros(T, B, N, dtype=torch.int32)
    kw = dict(actions_in=tape) if policy == "tape" else dict(actions=acts, policy=policy)
    launch = env.rollout_launcher(T, slots=True, **kw, **buffers(True))
    assert lib.calls == []
    for call in range(4):
        if call == 3:
            launch.invalidate()
        launch()
    assert [s for s, _ in lib.calls] == [LEGACY[policy][0]] * 4
    assert [a[2] for _, a in lib.calls] == [1, 3, 3, 1]            # the band bit after the first call, until invalidate()
    assert lib.calls[0][1][3].value == (tape if policy == "tape" else acts).data_ptr()


def test_the_default_in_place_random_call_builds_its_arguments_once(shell):
    env, lib = shell
    assert env.rollout_random(5) == (env.out, env.obs, env.vec)
    fast = env._roll_fast
    assert fast is not None and env.rollout_random(7)[1] is env.obs and env._roll_fast is fast
    assert [(s, a[1:3]) for s, a in lib.calls] == [("mapf_rollout_random", (5, 0)), ("mapf_rollout_random", (7, 0))]
    assert lib.calls[0][1][3] is lib.calls[1][1][3] is fast[4]


def test_unknown_policies_and_misplaced_tapes_are_value_errors(shell):
    env, lib = shell
    tape = torch.zeros(T, B, N, dtype=torch.int32)
    with pytest.raises(ValueError, match="descent.*pibt.*random.*tape"):
        env.rollout(T, policy="nope")
    for call in (env.rollout_plan, env.rollout_kernel_name, lambda policy: env.rollout_launcher(T, policy=policy)):
        with pytest.raises(ValueError, match="nope"):
            call(policy="nope")
    for policy in ("random", "descent", "pibt"):
        with pytest.raises(ValueError, match="tape"):
            env.rollout(T, policy, tape=tape)
    with pytest.raises(ValueError, match="mutually exclusive"):
        env.rollout_launcher(T, policy="descent", actions_in=tape)
    with pytest.raises(ValueError, match="actions_in"):
        env.rollout_launcher(T, policy="tape")
    with pytest.raises(ValueError, match="tape"):
        env.rollout(T + 1, "tape", tape=tape)
    assert lib.calls == []
    env.rollout(T, "tape", tape=tape)                   # a T that agrees is accepted
    assert [(s, a[1]) for s, a in lib.calls] == [("mapf_rollout_actions", T)]


def test_negative_T_raises_and_T0_makes_no_library_call(shell):
    env, lib = shell
    for name in ("rollout_descent", "rollout_pibt"):
        with pytest.raises(ValueError, match="T must be >= 0"):
            getattr(env, name)(-1)
        assert getattr(env, name)(0) == (env.out, env.obs, env.vec)
    assert env.rollout_actions(torch.zeros(0, B, N, dtype=torch.int32)) == (env.out, env.obs, env.vec)
    with pytest.raises(ValueError, match="actions"):          # the buffer checks still run at T = 0
        env.rollout_descent(0, actions=torch.zeros(1, dtype=torch.int32))
    assert lib.calls == []
    env.rollout_random(0, actions=env.actions)                # random hands T to the library as it is
    assert [(s, a[1]) for s, a in lib.calls] == [("mapf_rollout_random", 0)]
