"""PPO epochs over a whole device rollout (include/mapf.h: mapf_minibatch_rows, mapf_gather_rows;
mapf_amd/trainer.py): the device permutation against its host twin, the one-launch gather against
torch indexing of the t-major buffers, the update's static inputs after _DeviceUpdate.load_rows,
DeviceTrainer's epochs, and the whole path against Model.train on the same rows."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 255, 256, 257, 1000, 6144]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def test_device_rows_equal_host_rows():
    from mapf_amd.env import minibatch_rows
    for n in SIZES:
        for seed, epoch in ((0, 0), (7, 3)):
            cut = n // 3
            for start, count in ((0, cut), (cut, n - cut)):          # two windows that cover [0, n)
                want = minibatch_rows(n, seed, epoch, start, count, device="cpu")
                got = minibatch_rows(n, seed, epoch, start, count, device="cuda")
                assert got.device.type == "cuda" and got.dtype == torch.int64 and got.shape == (count,)
                assert torch.equal(got.cpu(), want), (n, seed, epoch, start, count)
    out = torch.full((12,), -7, dtype=torch.int64, device="cuda")     # into a caller's tensor, nothing past it
    minibatch_rows(1000, 1, 2, 100, 10, out=out[:10])
    assert torch.equal(out[:10].cpu(), minibatch_rows(1000, 1, 2, 100, 10, device="cpu"))
    assert (out[10:] == -7).all()


def _rollout_like(T, B, N, C, F, g):
    """The nine training arrays as DeviceRunner holds them: t-major, obs / vec as the [:T] views of
    [T + 1] buffers, real dtypes."""
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)      # noqa: E731
    return [r(T + 1, B, N, C, F, F)[:T], r(T + 1, B, N, 4)[:T], r(T, B, N), r(T, B, N), r(T, B, N), r(T, B, N),
            torch.randint(0, 5, (T, B, N), device="cuda", generator=g), r(T, B, N, 5), r(T, B, N, 5)]


def _rows(M, n, g):
    """M env-major rows in [0, n) with duplicates, row 0 and row n - 1 (where M has room for them)"""
    rows = torch.randint(0, n, (M,), device="cuda", generator=g)
    rows[-1] = n - 1
    if M >= 4:
        rows[0] = 0
        rows[2] = rows[1]
        rows[M // 2] = n - 1
    return rows


def _guarded(srcs, M):
    """destinations with one extra row, prefilled with NaN / a sentinel"""
    return [torch.full((M + 1,) + tuple(s.shape[2:]), float("nan") if s.is_floating_point() else -7,
                       dtype=s.dtype, device="cuda") for s in srcs]


@pytest.mark.parametrize("T,B,N,C,F", [(3, 2, 3, 5, 3),       # 540-byte observation rows: the 4-byte path
                                       (4, 5, 8, 6, 9),       # 15,552-byte rows: 16-byte accesses, 4 pieces
                                       (2, 3, 5, 7, 11)])     # 16,940-byte rows: 4-byte accesses, 5 pieces
def test_gather_rows_equals_torch_indexing(T, B, N, C, F):
    from mapf_amd.env import gather_rows
    g = torch.Generator(device="cuda").manual_seed(T * 100 + B)
    srcs = _rollout_like(T, B, N, C, F, g)
    for M in (1, 7, 257):
        rows = _rows(M, T * B, g)
        full = _guarded(srcs, M)
        gather_rows(srcs, T, B, rows, [d[:M] for d in full])
        for k, (s, d) in enumerate(zip(srcs, full)):
            assert torch.equal(d[:M], s[rows % T, rows // T]), (M, k)
            guard = d[M]
            assert (torch.isnan(guard) if s.is_floating_point() else guard == -7).all(), (M, k)


def test_gather_rows_from_views_inside_their_storage():
    """fp32 sources and destinations that start 4 and 8 bytes into their storage, rows of a 16-byte
    multiple (32 B: rides with the first workgroup; 2,048 B: its own pieces): the 4-byte path, nothing
    written before or after the destination's rows."""
    from mapf_amd.env import gather_rows
    g = torch.Generator(device="cuda").manual_seed(5)
    T, B, M = 4, 5, 7
    rows = _rows(M, T * B, g)
    srcs, dsts, stores = [], [], []
    for row in (8, 512):
        for so, do in ((1, 2), (2, 1), (0, 1), (2, 0)):
            s = torch.randn(T * B * row + 4, device="cuda", generator=g)
            d = torch.full((M * row + 4,), float("nan"), device="cuda")
            srcs.append(s[so:so + T * B * row].view(T, B, row))
            dsts.append(d[do:do + M * row].view(M, row))
            assert srcs[-1].data_ptr() % 16 == 4 * so and dsts[-1].data_ptr() % 16 == 4 * do
            stores.append((d, do, M * row))
    gather_rows(srcs, T, B, rows, dsts)
    for s, d, (store, do, n) in zip(srcs, dsts, stores):
        assert torch.equal(d, s[rows % T, rows // T])
        assert torch.isnan(store[:do]).all() and torch.isnan(store[do + n:]).all()


def test_gather_rows_error_codes():
    from mapf_amd import _lib
    from mapf_amd.env import gather_rows
    L = _lib.lib()
    src = torch.arange(24, dtype=torch.float32, device="cuda").view(2, 3, 4)
    dst = torch.full((2, 4), float("nan"), device="cuda")
    rows = torch.tensor([0, 5], device="cuda")

    def call(count=1, row_bytes=16, dst_ptr=dst.data_ptr(), T=2, M=2):
        spec = _lib.GatherSpec(T=T, B=3, M=M, rows=rows.data_ptr(), count=count)
        for a in range(min(max(count, 1), _lib.GATHER_MAX)):
            spec.arrays[a] = _lib.GatherArray(src.data_ptr(), dst_ptr, row_bytes)
        return L.mapf_gather_rows(ctypes.byref(spec), None)

    for kw, word in ((dict(count=0), b"count"), (dict(count=17), b"count"), (dict(row_bytes=6), b"row_bytes"),
                     (dict(row_bytes=0), b"row_bytes"), (dict(dst_ptr=None), b"null"), (dict(T=0), b"T, B and M"),
                     (dict(M=0), b"T, B and M")):
        assert call(**kw) == -1, kw
        assert word in L.mapf_last_error(), (kw, L.mapf_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                       # nothing was launched
    assert call() == 0
    assert torch.equal(dst, src[rows % 2, rows // 2])
    # the Python wrapper's own checks
    with pytest.raises(ValueError, match="contiguous"):
        gather_rows([src.transpose(0, 1)], 3, 2, rows, [dst])
    with pytest.raises(ValueError, match="destination"):
        gather_rows([src], 2, 3, rows, [dst[:1]])
    with pytest.raises(TypeError, match="dtype"):
        gather_rows([src], 2, 3, rows.int(), [dst])
    with pytest.raises(ValueError, match="float32"):
        gather_rows([src], 2, 3, rows, [dst.double()])


# ------------------------------------------------------------------ a small rollout: B = 4, T = 8
B0, T0, N0 = 4, 8, 8


def _make_runner(model, B, T, seed=5):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    from mapf_amd.runner import DeviceRunner
    env = BatchedMapfGym(make_config(B, 20, 20, num_agents=N0, fov=9, num_channel=6, human_mode="random",
                                     goal_mode="random", fix_choice=1, seed=99))
    env.reset_seeded(generate_warehouse(20, 20))
    return DeviceRunner(env, model, n_steps=T, seed=seed)


@pytest.fixture(scope="module")
def rollout():
    """(the global model before any update, the runner of an acting copy of it, the rollout's performance)"""
    from mapf_amd.model import Model
    torch.manual_seed(0)
    model = Model(0, "cuda", global_model=True, numChannel=6, num_agents=N0, fov=9)
    runner = _make_runner(copy.deepcopy(model), B0, T0)
    _, perf = runner.run()
    torch.cuda.synchronize()
    return model, runner, perf


FIELDS = ("observations", "vectors", "returns", "costReturns", "values", "costValues", "actions", "ps", "trainValid")


def test_load_rows_fills_the_static_inputs(rollout):
    from mapf_amd.env import minibatch_rows
    model, runner, _ = rollout
    model = copy.deepcopy(model)
    M = 8
    rows = minibatch_rows(B0 * T0, 3, 0, 8, M)
    buffers = (runner.obs[:T0], runner.vec[:T0], runner.returns, runner.cost_returns, runner.values,
               runner.cost_values, runner.actions, runner.ps, runner.train_valid)
    meta = lambda x, *tail: torch.empty((M,) + tuple(x.shape[2:]) + tail, device="meta")     # noqa: E731
    upd = model._device_update(meta(buffers[0]), meta(buffers[1]), meta(buffers[2]), meta(buffers[7]),
                               meta(buffers[8]), meta(buffers[6], 1))
    statics = (upd.obs, upd.vec, upd.ret, upd.cret, upd.v, upd.cv, upd.action, upd.old_ps, upd.tv)
    for t in statics:
        t.fill_(-3)
    upd.load_rows(buffers, T0, B0, rows, coef=model._loss_coef(0.25), lam=0.25)
    mb = runner.batch()
    host_rows = rows.cpu().numpy()
    assert upd.obs.shape == (M, N0, 6, 9, 9) and upd.action.shape == (M, N0, 1) and upd.action.dtype == torch.int64
    for name, t in zip(FIELDS, statics):
        want = mb[name][host_rows]
        assert torch.equal(t.reshape(want.shape), want), name
    want = torch.tensor(list(model._loss_coef(0.25)) + [0.25, 1.25], dtype=torch.float64).float()
    assert torch.equal(upd.dyn.cpu(), want)


class _RecordingModel:
    """what DeviceTrainer asks of a model, recorded"""
    device = torch.device("cuda")

    def __init__(self):
        self.calls = []

    def train_rows(self, runner, rows, episode_cost, checked=False):
        assert checked and rows.device.type == "cuda" and rows.dtype == torch.int64
        self.calls.append((rows.data_ptr(), rows.cpu().numpy().copy(), episode_cost))
        return [len(self.calls)]


def _stub_runner(B, T):
    return types.SimpleNamespace(T=T, env=types.SimpleNamespace(B=B, device=torch.device("cuda")))


def test_trainer_epochs_walk_a_permutation_each():
    from mapf_amd.trainer import DeviceTrainer
    perf = types.SimpleNamespace(episodeCostReward=1.5)
    model = _RecordingModel()
    tr = DeviceTrainer(_stub_runner(B0, T0), model, minibatch=8, n_epochs=2, seed=3)
    out = tr.update(perf)
    assert out == [[k + 1] for k in range(8)] and len(model.calls) == 2 * 4
    assert len({c[0] for c in model.calls}) == 1 and all(c[2] == 1.5 for c in model.calls)    # one reused tensor
    epochs = [np.concatenate([c[1] for c in model.calls[e * 4:(e + 1) * 4]]) for e in range(2)]
    for e in epochs:
        np.testing.assert_array_equal(np.sort(e), np.arange(B0 * T0))       # pairwise distinct: all 32 rows
    assert (epochs[0] != epochs[1]).any()
    tr.update(perf)                                                          # the epoch counter runs on
    assert tr.epoch_counter == 4
    third = np.concatenate([c[1] for c in model.calls[8:12]])
    assert (third != epochs[0]).any() and (third != epochs[1]).any()
    # B * T = 30: 3 minibatches of 8 per epoch, the 6 last rows of the permutation left out
    model = _RecordingModel()
    tr = DeviceTrainer(_stub_runner(5, 6), model, minibatch=8, n_epochs=2, seed=3)
    assert len(tr.update(perf)) == 2 * 3
    for e in range(2):
        seen = np.concatenate([c[1] for c in model.calls[e * 3:(e + 1) * 3]])
        assert len(set(seen.tolist())) == 24 and seen.min() >= 0 and seen.max() < 30
    with pytest.raises(ValueError):
        DeviceTrainer(_stub_runner(5, 6), model, minibatch=31)


@pytest.fixture
def deterministic_convs():
    """MIOpen's deterministic convolution algorithms (as tests/test_gpu_update_graph.py)"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_trainer_updates_equal_model_train_on_the_same_rows(rollout, deterministic_convs):
    """Twin A trains through DeviceTrainer.update (device rows, one gather launch, captured update);
    twins B and C through Model.train on torch-indexed rows, same rows, same order, eagerly.

    Bounds (the project's "same kernels, run-to-run spread", tests/test_gpu_update_graph.py): A's
    weight delta within max(2.5 x |C - B|, 1e-4) relative of B's; every stat within
    max(1e-5 x max(1, |b|), 3 x |c - b|)."""
    from mapf_amd.env import minibatch_rows
    from mapf_amd.trainer import DeviceTrainer
    model, runner, perf = rollout
    mA, mB, mC = (copy.deepcopy(model) for _ in range(3))
    mB.graph_update = mC.graph_update = False
    for m in (mA, mB, mC):
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    init = [p.detach().clone() for p in model.network.parameters()]
    M, E, seed = 8, 2, 3
    sA = DeviceTrainer(runner, mA, minibatch=M, n_epochs=E, seed=seed).update(perf)
    mb = runner.batch()
    sB, sC = [], []
    for m, out in ((mB, sB), (mC, sC)):
        for e in range(E):
            for k in range(B0 * T0 // M):
                rows = minibatch_rows(B0 * T0, seed, e, k * M, M)
                out.append(m.train(mb.observations[rows], mb.vectors[rows], mb.returns[rows], mb.costReturns[rows],
                                   mb.values[rows], mb.costValues[rows], mb.actions[rows], mb.ps[rows],
                                   mb.hiddenState[rows], mb.trainValid[rows], perf.episodeCostReward))
    assert len(sA) == len(sB) == len(sC) == 8 and all(len(s) == 12 for s in sA)
    for k, (s1, s2, s4) in enumerate(zip(sA, sB, sC)):
        for i, (a, b, c) in enumerate(zip(s1, s2, s4)):
            a, b, c = float(a), float(b), float(c)
            print(f"update {k} stat {i}: trainer {a!r} train {b!r} (twin {c!r})")
            if i == 8 and not np.isfinite(b):       # a skipped AMP step (inf grad norm): in both alike
                assert a == b, (k, a, b)
                continue
            assert np.isfinite(a), (k, i, a)
            assert abs(a - b) <= max(1e-5 * max(1.0, abs(b)), 3 * abs(c - b)), (k, i, a, b, c)
    upd = next(iter(mA._updates.values()))
    assert len(mA._updates) == 1 and upd.graph is not None and upd.eager_runs == upd.WARMUP    # 6 of 8 were replays
    delta = lambda m: torch.cat([(p.detach() - p0).flatten() for p, p0 in zip(m.network.parameters(), init)])  # noqa
    dA, dB, dC = delta(mA), delta(mB), delta(mC)
    r_ab = ((dA - dB).norm() / dB.norm()).item()
    r_cb = ((dC - dB).norm() / dB.norm()).item()
    print(f"relative delta difference: trainer vs train {r_ab:.6f}, train vs train {r_cb:.6f}")
    assert dB.norm() > 0 and r_ab <= max(2.5 * r_cb, 1e-4), (r_ab, r_cb)
