"""CPU checks of the action-tape rollout's boundary (mapf_rollout_actions, include/mapf.h): both
entry points are declared and bound (tests/test_abi.py's export check then covers the build), the
C call refuses bad arguments before any device call, and BatchedMapfGym's tape checks raise
before the library is reached."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mapf.h")


def test_header_declares_and_lib_binds_both_entry_points():
    from mapf_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int\s+mapf_rollout_actions\s*\(([^;]*)\)\s*;", txt)
    assert decl, "mapf_rollout_actions is not declared"
    args = [a.strip() for a in decl.group(1).replace("\n", " ").split(",")]
    assert len(args) == 8 and args[3].replace(" ", "") == "constint32_t*actions_in", args
    assert re.search(r"int\s+mapf_rollout_actions_plan\s*\(\s*const\s+mapf_env\s*\*", txt)
    P, I32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["mapf_rollout_actions"] == (ctypes.c_int, [P, I32, I32, P, ctypes.POINTER(_lib.StepOut), P, P, P])
    assert _lib.SIGNATURES["mapf_rollout_actions_plan"] == (ctypes.c_int, [P, I32, ctypes.c_char_p, I32])
    assert re.search(r"#define\s+MAPF_ABI_VERSION\s+1\b", txt)       # functions are only added


def test_c_call_refuses_null_arguments_without_a_device():
    from mapf_amd import _lib
    L = _lib.lib()
    so = _lib.StepOut()
    assert L.mapf_rollout_actions(None, 1, 0, None, ctypes.byref(so), None, None, None) == -1
    buf = ctypes.create_string_buffer(64)
    assert L.mapf_rollout_actions_plan(None, 0, buf, 64) == -1


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
    return env


@pytest.mark.parametrize("tape,exc", [
    (torch.zeros(4, 3, 2, dtype=torch.int64), TypeError),              # dtype
    (torch.zeros(4, 3, 2, dtype=torch.float32), TypeError),
    (torch.zeros(4, 2, 3, dtype=torch.int32), ValueError),             # [T, N, B]
    (torch.zeros(4, 6, dtype=torch.int32), ValueError),                # flattened
    (torch.zeros(24, dtype=torch.int32), ValueError),
    (torch.zeros(4, 3, 4, dtype=torch.int32)[:, :, ::2], ValueError),  # right shape, not contiguous
    (torch.zeros(4, 3, 2, dtype=torch.int32), ValueError),             # a host tensor
    ([[[0, 0]] * 3] * 4, TypeError),                                   # not a tensor
])
def test_python_tape_checks_raise_before_any_library_call(bare_env, tape, exc):
    with pytest.raises(exc, match="tape"):
        bare_env.rollout_actions(tape, slots=False)
    with pytest.raises(exc, match="tape"):
        bare_env.rollout_launcher(4, slots=False, actions_in=tape)


def test_launcher_tape_length_must_be_T(bare_env):
    with pytest.raises(ValueError, match="tape"):
        bare_env.rollout_launcher(5, actions_in=torch.zeros(4, 3, 2, dtype=torch.int32))
