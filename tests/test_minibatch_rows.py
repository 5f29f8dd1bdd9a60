"""CPU checks of the epoch permutation (include/mapf.h: mapf_minibatch_rows): the host twin
mapf_minibatch_rows_host runs the one __host__ __device__ function the device kernel runs
(csrc/mapf_common.h: shuffle_index), and libmapf.so loads without a GPU."""
import ctypes

import numpy as np
import pytest

SIZES = [1, 2, 3, 5, 255, 256, 257, 1000, 6144]


def host_rows(n, seed=0, epoch=0, start=0, count=None):
    from mapf_amd import _lib
    count = n - start if count is None else count
    buf = np.full(count + 2, -7, np.int64)               # the 2 past the end must stay untouched
    rc = _lib.lib().mapf_minibatch_rows_host(seed, epoch, n, start, count, buf.ctypes.data)
    assert rc == 0, _lib.lib().mapf_last_error()
    assert (buf[count:] == -7).all()
    return buf[:count].copy()


@pytest.mark.parametrize("n", SIZES)
def test_rows_are_a_bijection(n):
    for seed, epoch in ((0, 0), (3, 1), (2 ** 63 + 5, 2 ** 32 - 1)):
        np.testing.assert_array_equal(np.sort(host_rows(n, seed, epoch)), np.arange(n))


def test_windows_are_pieces_of_the_full_call():
    full = host_rows(1000, seed=4, epoch=2)
    parts = [host_rows(1000, 4, 2, a, b - a) for a, b in ((0, 256), (256, 512), (512, 768), (768, 1000))]
    np.testing.assert_array_equal(np.concatenate(parts), full)
    assert host_rows(1000, 4, 2, 1000, 0).size == 0       # the empty window at the end is legal


def test_the_python_wrapper_runs_the_host_twin():
    import torch
    from mapf_amd.env import minibatch_rows
    got = minibatch_rows(1000, 4, 2, 256, 256, device="cpu")
    assert got.dtype == torch.int64 and got.device.type == "cpu"
    np.testing.assert_array_equal(got.numpy(), host_rows(1000, 4, 2, 256, 256))
    out = torch.empty(10, dtype=torch.int64)
    assert minibatch_rows(1000, 4, 2, 0, 10, out=out) is out
    np.testing.assert_array_equal(out.numpy(), host_rows(1000, 4, 2, 0, 10))
    with pytest.raises(RuntimeError, match="start \\+ count"):
        minibatch_rows(10, 0, 0, 5, 6, device="cpu")


def test_deterministic_and_keyed():
    """A uniform permutation of 1024 has one expected fixed point and one expected agreement with
    another: 20 is a cap no sound cipher comes near, which an identity-like or epoch- or seed-blind
    P misses by a factor of 50."""
    n = 1024
    np.testing.assert_array_equal(host_rows(n, 1, 0), host_rows(n, 1, 0))
    for seed, epoch in ((0, 0), (1, 0), (1, 3), (2, 0)):
        fixed = int((host_rows(n, seed, epoch) == np.arange(n)).sum())
        print(f"seed {seed} epoch {epoch}: {fixed} fixed points")
        assert fixed <= 20
    for e in range(4):
        same = int((host_rows(n, 1, e) == host_rows(n, 1, e + 1)).sum())
        print(f"epochs {e} / {e + 1}: {same} positions agree")
        assert same <= 20
    same = int((host_rows(n, 1, 0) == host_rows(n, 2, 0)).sum())
    print(f"seeds 1 / 2: {same} positions agree")
    assert same <= 20


def test_bad_arguments_are_rejected():
    from mapf_amd import _lib
    L = _lib.lib()
    buf = np.zeros(16, np.int64)
    for n, start, count, word in ((10, 5, 6, b"start + count"), (10, 11, 0, b"start + count"), (0, 0, 0, b"n must"),
                                  (-1, 0, 0, b"n must"), (10, -1, 2, b">= 0"), (10, 0, -1, b">= 0")):
        assert L.mapf_minibatch_rows_host(0, 0, n, start, count, buf.ctypes.data) == -1, (n, start, count)
        assert word in L.mapf_last_error(), (n, start, count, L.mapf_last_error())
        # the device entry point validates before any device call
        assert L.mapf_minibatch_rows(0, 0, n, start, count, buf.ctypes.data, None) == -1
        assert word in L.mapf_last_error()
    assert L.mapf_minibatch_rows_host(0, 0, 10, 0, 4, None) == -1
    assert not buf.any()


def test_trainer_on_a_cpu_model_trains_through_model_train():
    """A model that is not on the GPU takes Model.train on torch-indexed rows (the plain reference
    path): DeviceTrainer over a stand-in runner with host buffers equals Model.train on the rows
    the host twin gives, update by update, and drops the remainder."""
    import copy
    import types
    import torch
    from mapf_amd.env import minibatch_rows
    from mapf_amd.model import Model
    from mapf_amd.runner import BatchValues, EnvMajorRows, ZeroRows
    from mapf_amd.trainer import DeviceTrainer
    T, B, N, M = 3, 2, 2, 4
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    bufs = dict(observations=(torch.rand(T, B, N, 6, 9, 9, generator=g) < 0.3).float(), vectors=r(T, B, N, 4),
                returns=r(T, B, N), costReturns=r(T, B, N), values=r(T, B, N), costValues=r(T, B, N),
                actions=torch.randint(0, 5, (T, B, N), generator=g), ps=torch.softmax(r(T, B, N, 5), -1),
                trainValid=(torch.rand(T, B, N, 5, generator=g) < 0.7).float(), rewards=r(T, B, N),
                costRewards=r(T, B, N))
    mb = BatchValues(hiddenState=ZeroRows(T * B, (2, N, 512), "cpu"),
                     **{k: EnvMajorRows(v, T, B) for k, v in bufs.items()})
    runner = types.SimpleNamespace(T=T, env=types.SimpleNamespace(B=B, device=torch.device("cpu")), batch=lambda: mb)
    torch.manual_seed(0)
    m1 = Model(0, "cpu", global_model=True, numChannel=6, num_agents=N, fov=9)
    m1.network.eval()
    m2 = copy.deepcopy(m1)
    perf = types.SimpleNamespace(episodeCostReward=3.0)
    trainer = DeviceTrainer(runner, m1, minibatch=M, n_epochs=2, seed=5)
    got = trainer.update(perf)
    assert len(got) == 2 * (T * B // M) and trainer.epoch_counter == 2        # 6 rows: 1 minibatch, 2 left out
    for e, s1 in enumerate(got):
        rows = minibatch_rows(T * B, 5, e, 0, M, device="cpu")
        s2 = m2.train(mb.observations[rows], mb.vectors[rows], mb.returns[rows], mb.costReturns[rows], mb.values[rows],
                      mb.costValues[rows], mb.actions[rows], mb.ps[rows], mb.hiddenState[rows], mb.trainValid[rows], 3.0)
        assert len(s1) == 12 and [float(x) for x in s1] == [float(x) for x in s2], (e, s1, s2)
    for p1, p2 in zip(m1.network.parameters(), m2.network.parameters()):
        assert torch.equal(p1, p2)
    with pytest.raises(IndexError):
        m1.train_rows(runner, [0, T * B], 3.0)                                 # explicit indices are range-checked


def test_gather_spec_layout_matches_c(tmp_path):
    import os
    import subprocess
    from mapf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mapf.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mapf_gather_spec),'
                   ' offsetof(mapf_gather_spec, rows), offsetof(mapf_gather_spec, count),'
                   ' offsetof(mapf_gather_spec, arrays), sizeof(mapf_gather_array),'
                   ' offsetof(mapf_gather_array, row_bytes)); return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S, A = _lib.GatherSpec, _lib.GatherArray
    assert got == [ctypes.sizeof(S), S.rows.offset, S.count.offset, S.arrays.offset, ctypes.sizeof(A),
                   A.row_bytes.offset]


def test_gather_rows_validates_before_any_launch():
    """mapf_gather_rows rejects a bad spec without a device call (the error codes proper, with device
    pointers, are in tests/test_gpu_minibatch.py)."""
    from mapf_amd import _lib
    L = _lib.lib()
    assert L.mapf_gather_rows(None, None) == -1
    spec = _lib.GatherSpec(T=2, B=2, M=1, rows=0, count=1)
    assert L.mapf_gather_rows(ctypes.byref(spec), None) == -1 and b"null" in L.mapf_last_error()
