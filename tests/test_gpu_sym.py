"""GPU tests of the grid-symmetry gather (include/mapf.h: mapf_gather_rows_sym, mapf_sym_draw): the
identity against mapf_gather_rows (+ mapf_unpack_obs), all eight symmetries against the host twins,
the device env's equivariance on the scene of tests/test_sym_cpu.py, the draws against their host
twin, and the training paths that pass a symmetry per row down (imitate_rows, train_rows,
DeviceTrainer(augment=))."""
import copy

import numpy as np
import pytest
import torch

import test_sym_cpu as H

pytestmark = pytest.mark.gpu

T, B, M = 2, 3, 7
KINDS = ("obs", "obs_bits", "vec", "action32", "action64", "cols", "plain")
SHAPES = [(N, C, F) for F in (1, 3, 9, 11) for C in (5, 6, 7) for N in (1, 3, 8)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


@pytest.fixture
def deterministic_convs():
    """MIOpen's deterministic convolution algorithms (as tests/test_gpu_update_graph.py)"""
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def _sources(N, C, F, seed):
    """the seven arrays on the host, t-major [T, B, ...]: 0/1 planes and their packed form, vec with zeros
    and negatives, actions with an out-of-range value, random columns, a plain array"""
    from mapf_amd.env import pack_obs
    rng = np.random.default_rng(seed)
    obs = (rng.random((T, B, N, C, F, F)) < 0.4).astype(np.float32)
    vec = rng.standard_normal((T, B, N, 4)).astype(np.float32)
    vec[0, 0, :, 0] = 0.0
    vec[1, 1, :, :2] = 0.0
    act = rng.integers(0, 5, (T, B, N))
    act[0, 1, 0] = 9
    act[1, 2, -1] = -2
    cols = rng.random((T, B, N, 5)).astype(np.float32)
    plain = rng.standard_normal((T, B, N)).astype(np.float32)
    return dict(obs=torch.from_numpy(obs), obs_bits=pack_obs(obs, C, F), vec=torch.from_numpy(vec),
                action32=torch.from_numpy(act).int(), action64=torch.from_numpy(act).long(),
                cols=torch.from_numpy(cols), plain=torch.from_numpy(plain))


def _guarded(srcs, N, C, F):
    """per kind (storage, view): M rows with a guard row either side, all prefilled with a sentinel"""
    out = {}
    for k, s in srcs.items():
        tail = (N, C, F, F) if k == "obs_bits" else tuple(s.shape[2:])
        dt = torch.float32 if k == "obs_bits" else s.dtype
        full = torch.full((M + 2,) + tail, float("nan") if dt.is_floating_point else -7, dtype=dt, device="cuda")
        out[k] = (full, full[1:M + 1])
    return out


def _raw(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _guards_intact(full):
    g = torch.stack((full[0], full[-1]))
    return bool((torch.isnan(g) if g.is_floating_point() else g == -7).all())


ROWS = [0, T * B - 1, 3, 3, 1, 4, 2]                # a duplicate, the first and the last row


def _gather_sym(dev, dsts, sym, N, C, F):
    from mapf_amd.env import gather_rows_sym
    rows = torch.tensor(ROWS, device="cuda")
    gather_rows_sym([dev[k] for k in KINDS], T, B, rows, [dsts[k][1] for k in KINDS], KINDS, sym=sym, geometry=(N, C, F))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ T5: the identity
def test_identity_equals_gather_rows_and_unpack():
    from mapf_amd.env import gather_rows, unpack_obs
    rows = torch.tensor(ROWS, device="cuda")
    for N, C, F in SHAPES:
        srcs = _sources(N, C, F, seed=N * 1000 + C * 100 + F)
        dev = {k: v.cuda() for k, v in srcs.items()}
        want = {k: torch.empty((M,) + tuple(v.shape[2:]), dtype=v.dtype, device="cuda") for k, v in dev.items()}
        gather_rows([dev[k] for k in KINDS], T, B, rows, [want[k] for k in KINDS])
        want["obs_bits"] = unpack_obs(want["obs_bits"], C, F)
        for sym in (None, torch.zeros(M, dtype=torch.uint8, device="cuda")):
            if sym is not None and F % 2 == 0:
                continue
            dsts = _guarded(dev, N, C, F)
            _gather_sym(dev, dsts, sym, N, C, F)
            for k in KINDS:
                full, view = dsts[k]
                assert torch.equal(_raw(view), _raw(want[k])), (N, C, F, k, sym is not None)
                assert _guards_intact(full), (N, C, F, k)


def test_identity_on_an_even_window_without_sym():
    """F even is legal while nothing is transformed"""
    from mapf_amd.env import gather_rows_sym
    N, C, F = 3, 6, 4
    srcs = _sources(N, C, F, seed=1)
    dev = {k: v.cuda() for k, v in srcs.items()}
    dsts = _guarded(dev, N, C, F)
    _gather_sym(dev, dsts, None, N, C, F)
    rows = torch.tensor(ROWS, device="cuda")
    assert torch.equal(dsts["obs_bits"][1], dev["obs"][rows % T, rows // T])
    assert torch.equal(dsts["obs"][1], dev["obs"][rows % T, rows // T])
    with pytest.raises(RuntimeError, match="F must be odd"):
        gather_rows_sym([dev["obs"]], T, B, rows, [dsts["obs"][1]], ["obs"],
                        sym=torch.zeros(M, dtype=torch.uint8, device="cuda"), geometry=(N, C, F))


# ------------------------------------------------------------------ T6: all eight
def _expected(srcs, rows, sym):
    """the host twins applied row by row"""
    fn = dict(obs=H.sym_obs, obs_bits=H.sym_obs, vec=H.sym_vec, cols=H.sym_cols, action32=H.sym_actions,
              action64=H.sym_actions, plain=lambda x, g: x)
    out = {}
    for k in KINDS:
        src = srcs["obs" if k == "obs_bits" else k].numpy()
        out[k] = np.stack([fn[k](src[r % T, r // T], int(g)) for r, g in zip(rows, sym)])
    return out


@pytest.mark.parametrize("sym", [[0, 1, 2, 3, 4, 5, 6], [7, 6, 5, 4, 3, 2, 1], [5, 5, 5, 5, 5, 5, 5]])
def test_every_symmetry_equals_the_host_twins(sym):
    for N, C, F in SHAPES:
        srcs = _sources(N, C, F, seed=N * 1000 + C * 100 + F + 7)
        dev = {k: v.cuda() for k, v in srcs.items()}
        dsts = _guarded(dev, N, C, F)
        _gather_sym(dev, dsts, torch.tensor(sym, dtype=torch.uint8, device="cuda"), N, C, F)
        want = _expected(srcs, ROWS, sym)
        for k in KINDS:
            full, view = dsts[k]
            got = view.cpu().numpy()
            if got.dtype == np.float32:
                np.testing.assert_array_equal(H.bits(got), H.bits(want[k]), err_msg=f"{(N, C, F, k)}")
            else:
                np.testing.assert_array_equal(got, want[k].astype(got.dtype), err_msg=f"{(N, C, F, k)}")
            assert _guards_intact(full), (N, C, F, k)


def test_many_rows_and_many_agents():
    """257 rows (more than one wave of workgroups per array), and N = 80: vec, actions and columns are
    big arrays of their own, the 20-byte columns straddling the 4 KiB pieces"""
    from mapf_amd.env import gather_rows_sym, pack_obs
    N, C, F, T2, B2, M2 = 80, 5, 3, 3, 4, 257
    rng = np.random.default_rng(2)
    obs = (rng.random((T2, B2, N, C, F, F)) < 0.5).astype(np.float32)
    vec = rng.standard_normal((T2, B2, N, 4)).astype(np.float32)
    cols = rng.random((T2, B2, N, 5)).astype(np.float32)
    act = rng.integers(0, 5, (T2, B2, N))
    rows = rng.integers(0, T2 * B2, M2)
    sym = rng.integers(0, 8, M2).astype(np.uint8)
    srcs = [torch.from_numpy(obs), pack_obs(obs, C, F), torch.from_numpy(vec), torch.from_numpy(cols),
            torch.from_numpy(act).long()]
    kinds = ["obs", "obs_bits", "vec", "cols", "action64"]
    dsts = [torch.full((M2,) + tuple(s.shape[2:]), float("nan") if s.is_floating_point() else -7, dtype=s.dtype,
                       device="cuda") for s in srcs]
    dsts[1] = torch.full((M2, N, C, F, F), float("nan"), device="cuda")
    gather_rows_sym([s.cuda() for s in srcs], T2, B2, torch.from_numpy(rows).cuda(), dsts, kinds,
                    sym=torch.from_numpy(sym).cuda(), geometry=(N, C, F))
    torch.cuda.synchronize()
    pick = lambda x: x[rows % T2, rows // T2]      # noqa: E731
    from mapf_amd.env import sym_apply             # equal to the host twins (tests/test_sym_cpu.py)
    o, v, a, c = sym_apply(pick(obs), pick(vec), pick(act), pick(cols), sym)
    np.testing.assert_array_equal(H.bits(dsts[0].cpu().numpy()), H.bits(o))
    np.testing.assert_array_equal(H.bits(dsts[1].cpu().numpy()), H.bits(o))
    np.testing.assert_array_equal(H.bits(dsts[2].cpu().numpy()), H.bits(v))
    np.testing.assert_array_equal(H.bits(dsts[3].cpu().numpy()), H.bits(c))
    np.testing.assert_array_equal(dsts[4].cpu().numpy(), a)


# ------------------------------------------------------------------ T7: the device env is equivariant
def _device_scene(g):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    _, world, seqs, hs, hg = H.scene(g)
    env = BatchedMapfGym(make_config(2, world.shape[0], world.shape[1], num_agents=H.SCENE_N, fov=H.SCENE_F,
                                     num_channel=H.SCENE_C, use_da=True, use_hp=True, human_mode=0, goal_mode=0,
                                     fix_choice=0, keep_bfs=True, max_seq=2, seed=11, k_predict=3, penalty_radius=2))
    env.reset_fixed(world, [seqs] * 2, [hs] * 2, [hg] * 2)
    return env


def test_device_env_equivariance():
    from mapf_amd.env import gather_rows_sym
    base = _device_scene(0)
    obs, vec = base.observe()
    bits, _ = base.observe_bits()
    N, C, F = H.SCENE_N, H.SCENE_C, H.SCENE_F
    oracle_obs, oracle_vec = H.scene_env(0).observe()
    assert np.array_equal(obs[0].cpu().numpy(), oracle_obs) and np.array_equal(vec[1].cpu().numpy(), oracle_vec)
    slot = (obs.view(1, 2, N, C, F, F), bits.view(1, 2, N, -1), vec.view(1, 2, N, 4))     # a one-step slot buffer
    rows = torch.tensor([0, 1], device="cuda")
    for g in range(8):
        other = _device_scene(g)
        want_obs, want_vec = other.observe()
        dsts = [torch.full((2, N, C, F, F), float("nan"), device="cuda") for _ in range(2)]
        dsts.append(torch.full((2, N, 4), float("nan"), device="cuda"))
        gather_rows_sym(slot, 1, 2, rows, dsts, ("obs", "obs_bits", "vec"),
                        sym=torch.full((2,), g, dtype=torch.uint8, device="cuda"), geometry=(N, C, F))
        torch.cuda.synchronize()
        assert torch.equal(_raw(dsts[0]), _raw(want_obs)), g
        assert torch.equal(_raw(dsts[1]), _raw(want_obs)), g
        assert torch.equal(_raw(dsts[2]), _raw(want_vec)), g


# ------------------------------------------------------------------ T8: the draws
def test_device_draws_equal_the_host_twin():
    from mapf_amd.env import sym_draw
    for seed, epoch, start, count, allowed in ((0, 0, 0, 1, 0xFF), (7, 3, 250, 1000, 0xFF), (2 ** 63 + 9, 2 ** 32 - 1, 2 ** 32 - 8, 300, 0x0F),
                                               (5, 1, 0, 70000, 0xA5), (5, 1, 3, 9, 0x01)):
        got = sym_draw(seed, epoch, start, count, allowed)
        assert got.dtype == torch.uint8 and got.device.type == "cuda"
        np.testing.assert_array_equal(got.cpu().numpy(), H.host_draw(seed, epoch, start, count, allowed))
    out = torch.full((12,), 99, dtype=torch.uint8, device="cuda")
    sym_draw(1, 2, 100, 10, 0xFF, out=out[:10])
    assert torch.equal(out[:10].cpu(), sym_draw(1, 2, 100, 10, 0xFF, device="cpu")) and (out[10:] == 99).all()
    with pytest.raises(RuntimeError, match="allowed"):
        sym_draw(1, 2, 0, 4, 0)


# ------------------------------------------------------------------ T9: the training paths
def _close(a, b, c):
    """the captured-against-eager rule of tests/test_gpu_imitation.py (and test_gpu_update_graph.py): within 1e-5
    relative of the eager twin b, or within three times the distance of a second eager twin c"""
    return abs(a - b) <= max(1e-5 * max(1.0, abs(b)), 3 * abs(c - b))


def _model(seed=0):
    from mapf_amd.model import Model
    torch.manual_seed(seed)
    return Model(0, "cuda", global_model=True, numChannel=6, num_agents=8, fov=9)


def _env(B_=4, seed=31):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    env = BatchedMapfGym(make_config(B_, 20, 20, num_agents=8, fov=9, num_channel=6, human_mode="random",
                                     goal_mode="random", fix_choice=1, keep_bfs=True, seed=seed))
    env.reset_seeded(generate_warehouse(20, 20), seed=7)
    return env


class _Counting:
    """env.gather_rows / unpack_obs / gather_rows_sym behind counters"""

    def __init__(self, monkeypatch):
        import mapf_amd.env as E
        self.calls = []
        for name in ("gather_rows", "unpack_obs", "gather_rows_sym"):
            monkeypatch.setattr(E, name, self._wrap(name, getattr(E, name)))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return counted


@pytest.mark.parametrize("packed", [False, True])
def test_imitate_rows_with_a_symmetry_per_row(packed, deterministic_convs, monkeypatch):
    from mapf_amd.env import sym_apply, unpack_obs
    from mapf_amd.imitation import DemoRunner
    env = _env()
    T_, B_, M_ = 2, env.B, 8
    demo = DemoRunner(env, n_steps=T_, obs_bits=packed)
    demo.run()
    mA = _model()
    mB, mC = copy.deepcopy(mA), copy.deepcopy(mA)
    mB.graph_update = mC.graph_update = False
    for m in (mA, mB, mC):
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    rows = torch.tensor([5, 0, 7, 2, 2, 6, 1, 3], device="cuda")
    sym = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], dtype=torch.uint8, device="cuda")
    ts, bs = rows % T_, rows // T_
    ob = demo.obs_bits[:T_][ts, bs] if packed else demo.obs[:T_][ts, bs]
    ob = unpack_obs(ob.contiguous(), env.C, env.F) if packed else ob
    want_obs, want_vec, want_act, _ = sym_apply(ob, demo.vec[:T_][ts, bs], demo.expert_actions[ts, bs], None, sym)
    assert not torch.equal(want_obs, ob) and not torch.equal(want_act, demo.expert_actions[ts, bs])
    counts = _Counting(monkeypatch)
    sA = mA.imitate_rows(demo, rows, checked=True, sym=sym)
    assert counts.calls == ["gather_rows_sym"]                      # one launch: no staging, no unpack
    upd = next(iter(mA._updates.values()))
    assert len(sA) == 4 and getattr(upd, "obs_stage", None) is None
    assert torch.equal(_raw(upd.obs), _raw(want_obs)) and torch.equal(_raw(upd.vec), _raw(want_vec))
    assert upd.action.dtype == torch.int32 and torch.equal(upd.action, want_act)
    sB = mB.imitation_train(want_obs, want_vec, want_act, None)
    sC = mC.imitation_train(want_obs, want_vec, want_act.long(), None)
    for i, (a, b, c) in enumerate(zip(sA[:2], sB, sC)):
        a, b, c = float(a), float(b), float(c)
        print(f"stat {i}: imitate_rows(sym) {a!r} imitation_train {b!r} (twin {c!r})")
        assert np.isfinite(a) and _close(a, b, c), (i, a, b, c)
    assert 0.0 <= float(sA[2]) <= 1.0 and 0.0 < float(sA[3]) < 1.0
    # sym=None: the calls of before, and the inputs of before
    del counts.calls[:]
    mA.imitate_rows(demo, rows, checked=True)
    assert counts.calls == (["gather_rows", "unpack_obs"] if packed else ["gather_rows"])
    assert torch.equal(upd.obs, ob) and torch.equal(upd.action, demo.expert_actions[ts, bs])
    # a host list of symmetries is accepted; a wrong length or a float is not
    assert len(mA.imitate_rows(demo, rows, checked=True, sym=sym.tolist())) == 4
    with pytest.raises(ValueError):
        mA.imitate_rows(demo, rows, checked=True, sym=[0, 1])


def test_trainer_augment_draws_a_symmetry_per_row():
    from mapf_amd.env import sym_draw
    from mapf_amd.imitation import DemoRunner
    from mapf_amd.trainer import DeviceTrainer
    env = _env()
    demo = DemoRunner(env, n_steps=2, obs_bits=True)
    demo.run()
    model = _model()
    seen = []
    inner = model.imitate_rows

    def recording(source, rows, checked=False, sym=None):
        seen.append((rows.clone(), sym.clone(), sym.data_ptr()))
        return inner(source, rows, checked=checked, sym=sym)

    model.imitate_rows = recording
    M_, seed = 2, 9
    tr = DeviceTrainer(demo, model, minibatch=M_, n_epochs=1, seed=seed, augment=0xFF)
    out = tr.imitate(demo, n_epochs=2)                   # 2 epochs x 4 minibatches: two eager, then the graph
    assert len(out) == 8 and all(len(s) == 4 and np.isfinite(float(s[0])) for s in out)
    upd = next(iter(model._updates.values()))
    assert len(model._updates) == 1 and upd.graph is not None and upd.eager_runs == upd.WARMUP
    assert len({p for _, _, p in seen}) == 1             # one reused device tensor
    for i, (_, sym, _) in enumerate(seen):
        e, k = divmod(i, 4)
        assert torch.equal(sym.cpu(), sym_draw(seed, e, k * M_, M_, 0xFF, device="cpu")), (e, k)
    assert len({tuple(s.tolist()) for _, s, _ in seen}) > 1
    # the last replay read the last draw: the static inputs are the last minibatch's rows under it
    from mapf_amd.env import sym_apply, unpack_obs
    rows, sym, _ = seen[-1]
    ts, bs = rows % 2, rows // 2
    ob = unpack_obs(demo.obs_bits[:2][ts, bs].contiguous(), env.C, env.F)
    o, v, a, _ = sym_apply(ob, demo.vec[:2][ts, bs], demo.expert_actions[ts, bs], None, sym)
    assert torch.equal(upd.obs, o) and torch.equal(_raw(upd.vec), _raw(v)) and torch.equal(upd.action, a)
    # off: None and the identity-only mask draw nothing and pass nothing down
    for off in (None, 0x01):
        tr = DeviceTrainer(demo, model, minibatch=M_, n_epochs=1, seed=seed, augment=off)
        assert tr.augment is None and tr._sym_arg(0, M_) == {} and tr.sym is None
    with pytest.raises(ValueError):
        DeviceTrainer(demo, model, minibatch=M_, augment=0x100)


def test_train_rows_with_a_symmetry_per_row(deterministic_convs, monkeypatch):
    from mapf_amd.env import sym_apply
    from mapf_amd.runner import DeviceRunner
    model = _model()
    T_, M_ = 2, 8
    runner = DeviceRunner(_env(seed=99), copy.deepcopy(model), n_steps=T_, seed=5)
    _, perf = runner.run()
    mA, mB, mC = (copy.deepcopy(model) for _ in range(3))
    mB.graph_update = mC.graph_update = False
    for m in (mA, mB, mC):
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    rows = torch.tensor([5, 0, 7, 2, 2, 6, 1, 3], device="cuda")
    sym = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4], dtype=torch.uint8, device="cuda")
    mb = runner.batch()
    o, v, a, p = sym_apply(mb.observations[rows], mb.vectors[rows], mb.actions[rows], mb.ps[rows], sym)
    tv = sym_apply(None, None, None, mb.trainValid[rows], sym)[3]
    counts = _Counting(monkeypatch)
    sA = mA.train_rows(runner, rows, perf.episodeCostReward, checked=True, sym=sym)
    assert counts.calls == ["gather_rows_sym"]
    upd = next(iter(mA._updates.values()))
    for name, got, want in (("obs", upd.obs, o), ("vec", upd.vec, v), ("action", upd.action, a), ("ps", upd.old_ps, p),
                            ("tv", upd.tv, tv), ("ret", upd.ret, mb.returns[rows]), ("cret", upd.cret, mb.costReturns[rows]),
                            ("v", upd.v, mb.values[rows]), ("cv", upd.cv, mb.costValues[rows])):
        assert torch.equal(_raw(got.reshape(want.shape)), _raw(want)), name
    args = lambda: (o, v, mb.returns[rows], mb.costReturns[rows], mb.values[rows], mb.costValues[rows], a, p,   # noqa: E731
                    mb.hiddenState[rows], tv, perf.episodeCostReward)
    sB, sC = mB.train(*args()), mC.train(*args())
    assert len(sA) == 12
    for i, (x, b, c) in enumerate(zip(sA, sB, sC)):
        x, b, c = float(x), float(b), float(c)
        print(f"stat {i}: train_rows(sym) {x!r} train {b!r} (twin {c!r})")
        if i == 8 and not np.isfinite(b):           # a skipped AMP step (inf grad norm): in both alike
            assert x == b, (x, b)
            continue
        assert np.isfinite(x) and _close(x, b, c), (i, x, b, c)
    del counts.calls[:]
    mA.train_rows(runner, rows, perf.episodeCostReward, checked=True)
    assert counts.calls == ["gather_rows"]
    assert torch.equal(upd.obs, mb.observations[rows]) and torch.equal(upd.old_ps, mb.ps[rows])
