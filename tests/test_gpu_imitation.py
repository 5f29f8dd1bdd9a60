"""GPU tests of behaviour cloning on the device: Model.imitation_train's three paths against each other
and against the reference's update (tests/golden/g9_imitation.npz), the captured update against its
eager twins, DemoRunner's slots against a twin env stepped one call at a time, Model.imitate_rows'
gather, and DeviceRunner's expert labels."""
import copy

import numpy as np
import pytest
import torch

import imitation_ref as R
from golden_io import load

pytestmark = pytest.mark.gpu


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


def _model(seed=0):
    from mapf_amd.model import Model
    torch.manual_seed(seed)
    return Model(0, "cuda", global_model=True, numChannel=6, num_agents=8, fov=9)


def _demo_batch(g, rows=64, n=8):
    obs = (torch.rand(rows, n, 6, 9, 9, device="cuda", generator=g) < 0.3).float()
    vec = torch.randn(rows, n, 4, device="cuda", generator=g)
    act = torch.randint(0, 5, (rows, n), device="cuda", generator=g)
    return obs, vec, act


def _ppo_batch(g, rows=64, n=8):
    obs, vec, act = _demo_batch(g, rows, n)
    ret, v, cret, cv = (torch.randn(rows, n, device="cuda", generator=g) for _ in range(4))
    ps = torch.softmax(torch.randn(rows, n, 5, device="cuda", generator=g), -1)
    tv = (torch.rand(rows, n, 5, device="cuda", generator=g) < 0.7).float()
    return obs, vec, ret, cret, v, cv, act, ps, None, tv, 1.0


def _close(a, b, c):
    """the captured-against-eager rule of tests/test_gpu_update_graph.py: within 1e-5 relative of the eager
    twin b, or within three times the distance of a second eager twin c"""
    return abs(a - b) <= max(1e-5 * max(1.0, abs(b)), 3 * abs(c - b))


# ------------------------------------------------------------------ the three paths of imitation_train
def test_imitation_update_fused_equals_unfused():
    m1 = _model()
    m2 = copy.deepcopy(m1)
    m2.fused_loss = False
    g = torch.Generator(device="cuda").manual_seed(1)
    obs, vec, act = _demo_batch(g)
    for m in (m1, m2):                        # dropout off: both forwards see the same net
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)   # no fp16 overflow: Adam steps
    s1 = m1.imitation_train(obs, vec, act.int(), None)        # the rollouts' int32 actions, no conversion
    s2 = m2.imitation_train(obs, vec, act, None)
    assert len(s1) == len(s2) == 2 and all(np.isfinite(float(v)) for v in s1)
    for i, (a, b) in enumerate(zip(s1, s2)):
        print(f"stat {i}: fused {float(a)!r} unfused {float(b)!r}")
        assert abs(float(a) - float(b)) <= 1e-3 * max(1.0, abs(float(b))), (i, a, b)
    pairs = list(zip(m1.network.parameters(), m2.network.parameters()))
    assert all((p1.grad is None) == (p2.grad is None) for p1, p2 in pairs)   # the value, cost and blocking heads
    net = m1.network
    assert net.value_layer.weight.grad is None and net.cost_value_layer.weight.grad is None
    pairs = [(p1, p2) for p1, p2 in pairs if p1.grad is not None]
    g1 = torch.cat([p1.grad.flatten() for p1, _ in pairs])
    g2 = torch.cat([p2.grad.flatten() for _, p2 in pairs])
    overall = ((g1 - g2).norm() / g2.norm()).item()
    worst = max(((p1.grad - p2.grad).norm() / p2.grad.norm().clamp_min(1e-30)).item() for p1, p2 in pairs
                if p2.grad.norm() > 0)
    print(f"gradient relative L2: overall {overall:.2e}, worst parameter {worst:.2e}")
    assert overall < 3e-3
    for p1, p2 in pairs:
        if p2.grad.norm() == 0:               # token_wA: a softmax over a length-1 axis
            assert p1.grad.norm() == 0
            continue
        assert ((p1.grad - p2.grad).norm() / p2.grad.norm()).item() < 5e-2


def test_captured_imitation_updates_equal_eager_updates(deterministic_convs):
    m1 = _model()
    m2 = copy.deepcopy(m1)
    m2.graph_update = False
    m4 = copy.deepcopy(m2)                      # a second eager twin: the backward's own run-to-run spread
    for m in (m1, m2, m4):
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    g = torch.Generator(device="cuda").manual_seed(1)
    batches = [_demo_batch(g) for _ in range(6)]
    w0 = m1.network.conv1.weight.detach().clone()
    init = [p.detach().clone() for p in m1.network.parameters()]
    runs = {id(m): [] for m in (m1, m2, m4)}
    graphs = []
    with torch.no_grad():
        m1.network(batches[0][0], batches[0][1])            # fills the acting path's fp16 weight cache
    assert len(m1.network._h16) > 0
    for obs, vec, act in batches:
        for m in (m1, m2, m4):
            runs[id(m)].append(m.imitation_train(obs, vec, act, None))
        graphs.append(next(iter(m1._updates.values())).graph)
    assert [k for k in m1._updates][0][0] == "imitation" and len(m1._updates) == 1
    assert graphs[0] is None and graphs[1] is None and all(gr is not None for gr in graphs[2:])   # 3..6 were replays
    upd = next(iter(m1._updates.values()))
    assert upd.eager_runs == upd.WARMUP and next(iter(m2._updates.values())).graph is None
    for k in range(len(batches)):
        for i, (a, b, c) in enumerate(zip(runs[id(m1)][k], runs[id(m2)][k], runs[id(m4)][k])):
            a, b, c = float(a), float(b), float(c)
            print(f"update {k} stat {i}: captured {a!r} eager {b!r} (twin {c!r})")
            if i == 1 and not np.isfinite(b):       # a skipped AMP step (inf grad norm): in both alike
                assert np.isfinite(a) == np.isfinite(b) and not np.isnan(a), (k, a, b)
                continue
            assert np.isfinite(a) and _close(a, b, c), (k, i, a, b, c)
    assert len(m1.network._h16) == 0            # the acting path's fp16 weights were dropped
    assert not torch.equal(m1.network.conv1.weight, w0)            # the replays moved the weights
    delta = lambda m: torch.cat([(p.detach() - p0).flatten() for p, p0 in zip(m.network.parameters(), init)])  # noqa
    d1, d2, d4 = delta(m1), delta(m2), delta(m4)
    r_ge = ((d1 - d2).norm() / d2.norm()).item()
    r_ee = ((d4 - d2).norm() / d2.norm()).item()
    print(f"relative delta difference: graph vs eager {r_ge:.4f}, eager vs eager {r_ee:.4f}")
    assert d2.norm() > 0 and r_ge <= max(2.5 * r_ee, 1e-4), (r_ge, r_ee)
    torch.testing.assert_close(upd.scale, next(iter(m2._updates.values())).scale)
    # a PPO update between two imitation replays: its own _DeviceUpdate, the same optimizer and GradScaler
    s = m1.train(*_ppo_batch(g))
    assert len(s) == 12 and all(np.isfinite(float(x)) for i, x in enumerate(s) if i != 8)
    assert len(m1._updates) == 2 and next(iter(m1._updates.values())) is upd
    assert [u.scale is m1.net_scaler._scale for u in m1._updates.values()] == [True, True]
    before = m1.network.policy_layer.weight.detach().clone()
    s = m1.imitation_train(*batches[0], None)
    assert upd.graph is graphs[-1] and np.isfinite(float(s[0])) and not np.isnan(float(s[1]))
    assert not torch.equal(m1.network.policy_layer.weight, before)


# ------------------------------------------------------------------ the reference's update
def _fixture_model(hip):
    from mapf_amd.model import Model
    m = Model(0, "cuda", global_model=True, numChannel=R.CHANNELS, num_agents=R.AGENTS, fov=R.FOV)
    with torch.no_grad():
        sd = m.network.state_dict()
        w = R.recipe_weights([(k, v.shape) for k, v in sd.items()])
        for k, v in sd.items():               # in place: the parameters keep their channels_last layout
            v.copy_(torch.from_numpy(w[k]))
    m.network.eval()
    m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    if not hip:
        m.fused_loss = False
    return m


def test_gpu_imitation_update_matches_the_reference(monkeypatch):
    """The default path (HIP training forward and backward, mapf_imitation_loss, captured tail) on the
    reference's own update: logits within the project's fp16 figure, loss and grad norm within 2e-2, and
    per parameter the gradient slices no further from the reference's than 3 x the plain torch-autocast
    path's (MIOpen / SDPA autograd, not the code under test) -- the fp16 summation-order spread between
    two runs of one path is about 2 x.

    Measured on an MI355X: loss 8.597304 (hip) / 8.595377 (torch) against the reference's 8.595835, grad norm
    383.1131 / 383.2716 against 382.9758; the largest d_hip / d_torch is 1.42 (fully_connected_1.bias).
    Relative L2 of the stored gradient slices to the reference's, per parameter:
      parameter                                      d_hip     d_torch
      cls_token                                      9.14e-04  1.16e-03
      conv1.bias                                     2.73e-02  2.88e-02
      conv1.weight                                   4.52e-02  4.79e-02
      conv1a.bias                                    2.27e-02  2.25e-02
      conv1a.weight                                  3.03e-02  3.33e-02
      conv1b.bias                                    1.33e-02  1.39e-02
      conv1b.weight                                  7.82e-02  8.28e-02
      conv2.bias                                     1.31e-02  1.39e-02
      conv2.weight                                   2.74e-02  3.52e-02
      conv2a.bias                                    8.83e-03  9.68e-03
      conv2a.weight                                  1.41e-02  1.38e-02
      conv2b.bias                                    4.81e-03  6.30e-03
      conv2b.weight                                  1.02e-02  1.17e-02
      conv3.bias                                     4.21e-03  5.76e-03
      conv3.weight                                   4.47e-02  2.28e-01
      fully_connected_1.bias                         4.92e-03  3.47e-03
      fully_connected_1.weight                       6.44e-03  1.07e-02
      fully_connected_2.bias                         3.67e-03  5.71e-03
      fully_connected_2.weight                       4.62e-02  5.23e-02
      fully_connected_3.bias                         2.48e-03  3.74e-03
      fully_connected_3.weight                       5.39e-04  1.16e-03
      nn_same.bias                                   6.36e-04  8.59e-04
      nn_same.weight                                 1.20e-03  1.90e-03
      policy_layer.bias                              4.94e-04  9.24e-04
      policy_layer.weight                            7.52e-04  1.05e-03
      pos_embedding                                  9.14e-04  1.16e-03
      token_wV                                       7.95e-04  1.03e-03
      transformer.layers.0.0.fn.fn.nn1.bias          7.42e-04  9.56e-04
      transformer.layers.0.0.fn.fn.nn1.weight        7.06e-04  8.97e-04
      transformer.layers.0.0.fn.fn.to_qkv.bias       9.55e-04  1.26e-03
      transformer.layers.0.0.fn.fn.to_qkv.weight     5.19e-04  8.70e-04
      transformer.layers.0.0.fn.norm.bias            7.93e-04  1.02e-03
      transformer.layers.0.0.fn.norm.weight          9.66e-04  1.19e-03
      transformer.layers.0.1.fn.fn.nn1.bias          8.26e-04  1.05e-03
      transformer.layers.0.1.fn.fn.nn1.weight        7.54e-04  8.78e-04
      transformer.layers.0.1.fn.fn.nn2.bias          6.35e-04  8.81e-04
      transformer.layers.0.1.fn.fn.nn2.weight        1.23e-03  1.32e-03
      transformer.layers.0.1.fn.norm.bias            8.52e-04  1.09e-03
      transformer.layers.0.1.fn.norm.weight          1.04e-03  1.32e-03
      transformer.layers.1.0.fn.fn.nn1.bias          6.24e-04  8.66e-04
      transformer.layers.1.0.fn.fn.nn1.weight        1.48e-03  1.52e-03
      transformer.layers.1.0.fn.fn.to_qkv.bias       1.13e-03  1.39e-03
      transformer.layers.1.0.fn.fn.to_qkv.weight     6.16e-04  1.35e-03
      transformer.layers.1.0.fn.norm.bias            6.30e-04  8.19e-04
      transformer.layers.1.0.fn.norm.weight          8.03e-04  1.05e-03
      transformer.layers.1.1.fn.fn.nn1.bias          7.71e-04  1.02e-03
      transformer.layers.1.1.fn.fn.nn1.weight        1.17e-03  1.94e-03
      transformer.layers.1.1.fn.fn.nn2.bias          5.88e-04  8.50e-04
      transformer.layers.1.1.fn.fn.nn2.weight        5.92e-04  6.60e-04
      transformer.layers.1.1.fn.norm.bias            7.40e-04  9.80e-04
      transformer.layers.1.1.fn.norm.weight          8.78e-04  1.12e-03"""
    z = load("g9_imitation")
    obs, vec, action = (torch.from_numpy(x).cuda() for x in R.inputs())
    names = [str(n) for n in z["names"]]
    dist, stats = {}, {}
    from mapf_amd.net import SCRIMPNet
    for path in ("hip", "torch"):
        monkeypatch.setattr(SCRIMPNet, "hip_train", path == "hip")
        m = _fixture_model(path == "hip")
        if path == "hip":
            with torch.autocast(device_type="cuda"):
                logits = m.network(obs, vec, None)[5].detach().float()
            torch.testing.assert_close(logits.cpu(), torch.from_numpy(z["logits"]), rtol=3e-2, atol=3e-2)
        stats[path] = [float(s) for s in m.imitation_train(obs, vec, action, None)]
        got = R.grad_slices(m.network)
        assert sorted(got) == names
        dist[path] = {n: R.rel_l2(got[n][1], z[R.grad_key(n)]) for n in names if n != "token_wA"}
        assert got["token_wA"][0] == 0.0
    print(f"loss hip {stats['hip'][0]:.6f} torch {stats['torch'][0]:.6f} reference {float(z['loss']):.6f}; "
          f"grad norm hip {stats['hip'][1]:.4f} torch {stats['torch'][1]:.4f} reference {float(z['grad_norm']):.4f}")
    for n in names:
        if n != "token_wA":
            print(f"{n:50s} d_hip {dist['hip'][n]:.3e} d_torch {dist['torch'][n]:.3e}")
    for k, ref in enumerate((float(z["loss"]), float(z["grad_norm"]))):
        assert abs(stats["hip"][k] - ref) <= 2e-2 * abs(ref), (k, stats["hip"][k], ref)
    bad = [(n, dist["hip"][n], dist["torch"][n]) for n in dist["hip"] if not dist["hip"][n] <= 3 * dist["torch"][n]]
    assert not bad, bad


# ------------------------------------------------------------------ DemoRunner
SHAPES = {"pair-lane": dict(B=6, N=8, H=20, W=20, shared=True, kernel=1),
          "wide": dict(B=3, N=16, H=24, W=24, shared=False, kernel=2)}
T_DEMO = 5


def _env(shape, seed=31):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    s = SHAPES[shape]
    env = BatchedMapfGym(make_config(s["B"], s["H"], s["W"], num_agents=s["N"], fov=9, num_channel=6, human_mode="random",
                                     goal_mode="random", fix_choice=1, shared_map=s["shared"], keep_bfs=True, seed=seed))
    if s["shared"]:
        maps = generate_warehouse(s["H"], s["W"])
    else:                                       # per-env maps: another shelf length in every env
        maps = np.stack([generate_warehouse(s["H"], s["W"], shelf_size=3 + b) for b in range(s["B"])])
    env.reset_seeded(maps, seed=7)
    assert env.rollout_kernel == s["kernel"], (shape, env.rollout_kernel)
    return env


@pytest.fixture(scope="module")
def twins():
    """per shape: a twin env stepped by pibt_actions + step_observe, one call each -- the observation before
    every step (slot T: after the last) and the picks.  Computed once, read only."""
    out = {}
    for shape in SHAPES:
        env = _env(shape)
        obs, vec, acts = [], [], []
        o, v = env.observe()
        for t in range(T_DEMO):
            obs.append(o.clone())
            vec.append(v.clone())
            a = env.pibt_actions().clone()
            acts.append(a)
            _, o, v = env.step_observe(a)
        obs.append(o.clone())
        vec.append(v.clone())
        torch.cuda.synchronize()
        out[shape] = (torch.stack(obs), torch.stack(vec), torch.stack(acts))
    return out


@pytest.mark.parametrize("policy", ["pibt", "tape"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_demo_runner_slots_hold_the_state_the_expert_saw(twins, shape, packed, policy):
    from mapf_amd.env import pack_obs
    from mapf_amd.imitation import DemoRunner
    obs, vec, acts = twins[shape]
    env = _env(shape)
    demo = DemoRunner(env, n_steps=T_DEMO, policy=policy, obs_bits=packed)
    assert demo.packed == packed and demo.T == T_DEMO and demo.expert_actions.dtype == torch.int32
    perf = demo.run(tape=acts.contiguous()) if policy == "tape" else demo.run()
    torch.cuda.synchronize()
    assert torch.equal(demo.expert_actions, acts)                         # expert_actions[t]: the twin's pick at step t
    assert torch.equal(demo.vec, vec)                                     # slot t: the state before step t; slot T: the last
    if packed:
        assert demo.obs is None and demo.obs_bits.shape == (T_DEMO + 1, env.B, env.N, env.obs_words)
        assert torch.equal(demo.obs_bits.cpu(), pack_obs(obs.cpu(), env.C, env.F))
    else:
        assert demo.obs_bits is None and torch.equal(demo.obs, obs)
    assert set(perf) == {"totalGoals", "staticCollide", "humanCollide", "agentCollide", "constraintViolations"}
    assert all(v.shape == (env.B,) for v in perf.values())
    assert not perf["staticCollide"].any() and not perf["agentCollide"].any()       # PIBT: collision-free
    np.testing.assert_array_equal(perf["totalGoals"], demo.goals.sum(dim=(0, 2)).double().cpu().numpy())
    assert not env.counters()[:8].any()


def test_demo_runner_descent_and_its_argument_errors():
    from mapf_amd.imitation import DemoRunner
    env, twin = _env("pair-lane"), _env("pair-lane")
    demo = DemoRunner(env, n_steps=3, policy="descent", obs_bits=False)
    demo.run()
    for t in range(3):
        o, v = twin.observe()
        assert torch.equal(demo.obs[t], o) and torch.equal(demo.vec[t], v)
        a = twin.descent_actions()
        assert torch.equal(demo.expert_actions[t], a)
        twin.step_observe(a)
    with pytest.raises(ValueError):
        demo.run(tape=demo.expert_actions)
    with pytest.raises(ValueError):
        DemoRunner(env, n_steps=3, policy="tape").run()
    with pytest.raises(ValueError):
        DemoRunner(env, n_steps=3, policy="random")


# ------------------------------------------------------------------ imitate_rows
@pytest.mark.parametrize("packed", [False, True])
def test_imitate_rows_gathers_the_rows_and_trains_on_them(packed, deterministic_convs):
    from mapf_amd.env import minibatch_rows, unpack_obs
    from mapf_amd.imitation import DemoRunner
    from mapf_amd.trainer import DeviceTrainer
    env = _env("pair-lane")
    T, B, M = T_DEMO, env.B, 8
    demo = DemoRunner(env, n_steps=T, obs_bits=packed)
    demo.run()
    mA = _model()
    mB, mC = copy.deepcopy(mA), copy.deepcopy(mA)
    mB.graph_update = mC.graph_update = False
    for m in (mA, mB, mC):
        m.network.eval()
        m.net_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 8)
    rows = minibatch_rows(T * B, 3, 0, 8, M)
    ts, bs = rows % T, rows // T
    ob = demo.obs_bits[:T][ts, bs] if packed else demo.obs[:T][ts, bs]
    want_obs = unpack_obs(ob.contiguous(), env.C, env.F) if packed else ob
    want_vec, want_act = demo.vec[:T][ts, bs], demo.expert_actions[ts, bs]
    sA = mA.imitate_rows(demo, rows, checked=True)
    upd = next(iter(mA._updates.values()))
    assert len(sA) == 4 and upd.action.dtype == torch.int32
    assert torch.equal(upd.obs, want_obs) and torch.equal(upd.vec, want_vec) and torch.equal(upd.action, want_act)
    sB = mB.imitation_train(want_obs, want_vec, want_act, None)
    sC = mC.imitation_train(ob, want_vec, want_act.long(), None)        # packed rows / int64 actions go in as they are
    for i, (a, b, c) in enumerate(zip(sA[:2], sB, sC)):
        a, b, c = float(a), float(b), float(c)
        print(f"stat {i}: imitate_rows {a!r} imitation_train {b!r} (twin {c!r})")
        assert np.isfinite(a) and _close(a, b, c), (i, a, b, c)
    assert 0.0 <= float(sA[2]) <= 1.0 and 0.0 < float(sA[3]) < 1.0
    # host rows are checked; the trainer walks whole epochs of device rows through the same update
    assert len(mA.imitate_rows(demo, rows.cpu().numpy())) == 4
    with pytest.raises(IndexError):
        mA.imitate_rows(demo, [T * B])
    tr = DeviceTrainer(demo, mA, minibatch=M, n_epochs=1, seed=3)
    out = tr.imitate(demo, n_epochs=2)
    assert len(out) == 2 * (T * B // M) and tr.epoch_counter == 2 and all(len(s) == 4 for s in out)
    assert len(mA._updates) == 1 and upd.graph is not None


# ------------------------------------------------------------------ expert labels in DeviceRunner
def _runner(expert, model, T=6, seed=5):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    from mapf_amd.runner import DeviceRunner
    env = BatchedMapfGym(make_config(4, 20, 20, num_agents=8, fov=9, num_channel=6, human_mode="random",
                                     goal_mode="random", fix_choice=1, keep_bfs=True, seed=99))
    env.reset_seeded(generate_warehouse(20, 20))
    return DeviceRunner(env, model, n_steps=T, seed=seed, **({} if expert is None else {"expert": expert}))


@pytest.fixture(scope="module")
def acting_model():
    m = _model()
    m.network.eval()              # no dropout: two rollouts from one seed act alike
    return m


@pytest.mark.parametrize("expert", ["pibt", "descent"])
def test_device_runner_labels_its_own_states(acting_model, expert):
    T = 6
    runner = _runner(expert, acting_model, T)
    runner.run()
    twin = _runner(None, acting_model, T).env
    assert runner.expert_actions.shape == (T, 4, 8) and runner.expert_actions.dtype == torch.int32
    for t in range(T):
        o, v = twin.observe()
        assert torch.equal(runner.obs[t], o) and torch.equal(runner.vec[t], v)
        label = (twin.pibt_actions if expert == "pibt" else twin.descent_actions)().clone()
        assert torch.equal(runner.expert_actions[t], label), t
        twin.step(runner.actions[t].int().contiguous())
    stats = acting_model.imitate_rows(runner, torch.arange(8, device="cuda"))       # a source like DemoRunner
    assert len(stats) == 4 and np.isfinite(float(stats[0]))


def test_device_runner_without_expert_is_unchanged(acting_model):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.runner import DeviceRunner
    a, b, a2 = _runner(None, acting_model), _runner("pibt", acting_model), _runner(None, acting_model)
    assert a.expert is None and a.expert_actions is None
    for r in (a, b, a2):
        r.run()
    assert torch.equal(a.obs, a2.obs) and torch.equal(a.ps, a2.ps)        # the control: one seed, one rollout
    for name in ("obs", "vec", "actions", "ps", "values", "cost_values", "rewards", "cost_rewards", "train_valid",
                 "status", "returns", "cost_returns"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    env = BatchedMapfGym(make_config(2, 20, 20, num_agents=8, fov=9, num_channel=6, keep_bfs=False, seed=1))
    with pytest.raises(ValueError, match="keep_bfs"):
        DeviceRunner(env, acting_model, n_steps=2, expert="pibt")
