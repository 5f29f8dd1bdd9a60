"""Behaviour cloning on the CPU: Model.imitation_train against the reference's own update
(tests/golden/g9_imitation.npz, written by tests/golden/make_golden_il.py from model.py:205-231), the
contracts of the new entry points, two gloo ranks against one process, and mapf_imitation_loss's
argument validation (no device call)."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import imitation_ref as R
from golden_io import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4          # the project's CPU fp32 bound against the reference (g5_net)


def unpack_fixture(z):
    obs = np.unpackbits(z["obs_packed"])[:int(np.prod(z["obs_shape"]))].reshape(tuple(z["obs_shape"])).astype(np.float32)
    return obs, z["vec"], z["action"]


def make_model(agents=R.AGENTS):
    from mapf_amd.model import Model
    m = Model(0, "cpu", global_model=True, numChannel=R.CHANNELS, num_agents=agents, fov=R.FOV)
    R.load_recipe(m.network)
    m.network.eval()
    return m


@pytest.fixture(scope="module")
def z():
    return load("g9_imitation")


@pytest.fixture(scope="module")
def trained(z):
    """one imitation update on the fixture's minibatch (shared, read only): (model, stats, logits before)"""
    obs, vec, action = unpack_fixture(z)
    m = make_model()
    with torch.no_grad():
        logits = m.network(torch.from_numpy(obs), torch.from_numpy(vec), None)[5].numpy()
    stats = m.imitation_train(obs, vec, action, np.zeros((R.ROWS, 2, R.AGENTS, 512), np.float32))
    return m, stats, logits


def test_fixture_inputs_are_the_recipe(z):
    obs, vec, action = unpack_fixture(z)
    o, v, a = R.inputs()
    assert np.array_equal(obs, o) and np.array_equal(vec, v) and np.array_equal(action, a)


def test_imitation_train_matches_the_reference(z, trained):
    m, stats, logits = trained
    assert R.rel_l2(logits, z["logits"]) < TOL
    loss, grad_norm = (float(np.asarray(s)) for s in stats)
    print(f"loss {loss:.6f} (reference {float(z['loss']):.6f}), grad norm {grad_norm:.5f} ({float(z['grad_norm']):.5f})")
    assert abs(loss - float(z["loss"])) <= TOL * abs(float(z["loss"]))
    assert abs(grad_norm - float(z["grad_norm"])) <= TOL * abs(float(z["grad_norm"]))
    got = R.grad_slices(m.network)
    names = [str(n) for n in z["names"]]
    assert sorted(got) == names
    worst = 0.0
    for n, ref_norm in zip(names, z["norms"]):
        norm, sl = got[n]
        ref = z[R.grad_key(n)]
        if ref_norm == 0.0:                   # token_wA: a softmax over a length-1 axis
            assert norm == 0.0 and not sl.any(), n
            continue
        d = R.rel_l2(sl, ref)
        worst = max(worst, d, abs(norm - ref_norm) / ref_norm)
        assert d < TOL, (n, d)
        assert abs(norm - ref_norm) < TOL * ref_norm, (n, norm, ref_norm)
    print(f"worst relative distance of a gradient slice or norm: {worst:.2e}")


def test_contract_numpy_in_two_stats_out_and_heads_without_gradient(z, trained):
    m, stats, _ = trained
    assert len(stats) == 2 and all(isinstance(s, np.ndarray) and s.shape == () for s in stats)
    net = m.network
    for layer in (net.value_layer, net.cost_value_layer, net.blocking_layer):
        assert layer.weight.grad is None and layer.bias.grad is None
    assert sorted(n for n, p in net.named_parameters() if p.grad is None) == [str(n) for n in z["no_grad"]]


def test_imitation_train_takes_tensors_int32_actions_and_packed_observations(z):
    from mapf_amd.env import pack_obs
    obs, vec, action = unpack_fixture(z)
    want = [float(np.asarray(s)) for s in make_model().imitation_train(obs, vec, action, None)]
    got = make_model().imitation_train(pack_obs(obs, R.CHANNELS, R.FOV), torch.from_numpy(vec),
                                       torch.from_numpy(action).int(), None)
    assert [float(np.asarray(s)) for s in got] == want


def test_generate_state_is_the_fifth_output(z):
    obs, vec, _ = unpack_fixture(z)
    m = make_model()
    with torch.no_grad():
        want = m.network(torch.from_numpy(obs), torch.from_numpy(vec), None)[4]
    got = m.generate_state(obs, vec, None)
    assert tuple(got.shape) == (R.ROWS, R.AGENTS, 512) and torch.equal(got, want) and not got.requires_grad


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"demo.{name} was touched")


class _FakeRunner:
    """the two things DeviceTrainer reads of a runner before and in fit()"""

    def __init__(self, model):
        self.T, self.model, self.runs = 4, model, 0
        self.env = type("E", (), {"B": 2, "device": torch.device("cpu")})()

    def run(self, weights=None):
        self.runs += 1
        return None, type("P", (), {"episodeCostReward": 0.0})()


def test_fit_without_demonstrations_never_touches_demo(monkeypatch):
    from mapf_amd.config import TrainingParameters
    from mapf_amd.trainer import DeviceTrainer
    assert TrainingParameters.DEMONSTRATION_PROB == 0
    runner = _FakeRunner(object())
    runner.model = model = type("M", (), {"device": torch.device("cpu"), "calls": 0})()
    tr = DeviceTrainer(runner, model, minibatch=4, n_epochs=1)
    monkeypatch.setattr(tr, "update", lambda performance: ["ppo-stats"])
    out = tr.fit(3, demo=_Untouchable(), demonstration_prob=0)
    assert runner.runs == 3 and [e[0] for e in out] == ["ppo"] * 3 and out[0][2] == ["ppo-stats"]
    assert [e[0] for e in tr.fit(2, demo=_Untouchable())] == ["ppo"] * 2        # the default: DEMONSTRATION_PROB
    assert len(tr.fit(1)[0]) == 2                                              # no demo: (performance, mb_loss) as before
    with pytest.raises(ValueError):
        tr.fit(1, demonstration_prob=0.5)


def test_fit_marks_imitation_rollouts(monkeypatch):
    from mapf_amd.trainer import DeviceTrainer
    runner = _FakeRunner(None)
    runner.model = model = type("M", (), {"device": torch.device("cpu")})()
    demo = type("D", (), {"runs": 0, "run": lambda self: setattr(self, "runs", self.runs + 1) or {"totalGoals": 0}})()

    def kinds(seed):
        tr = DeviceTrainer(runner, model, minibatch=4, n_epochs=1, seed=seed)
        monkeypatch.setattr(tr, "update", lambda performance: ["ppo-stats"])
        monkeypatch.setattr(tr, "imitate", lambda source: ["il-stats"] if source is demo else None)
        return [e[0] for e in tr.fit(40, demo=demo, demonstration_prob=0.5)]

    a = kinds(3)
    assert a == kinds(3) and set(a) == {"ppo", "imitation"} and demo.runs == 2 * a.count("imitation")
    tr = DeviceTrainer(runner, model, minibatch=4, n_epochs=1)
    monkeypatch.setattr(tr, "imitate", lambda source: ["il-stats"])
    assert [e[0] for e in tr.fit(5, demo=demo, demonstration_prob=1.0)] == ["imitation"] * 5


def test_demo_runner_refuses_the_random_policy():
    from mapf_amd.imitation import DemoRunner
    with pytest.raises(ValueError):
        DemoRunner(None, n_steps=4, policy="random")


def test_device_runner_refuses_an_unknown_expert():
    from mapf_amd.runner import DeviceRunner
    with pytest.raises(ValueError):
        DeviceRunner(None, None, n_steps=4, expert="random")


def test_imitation_loss_rejects_bad_arguments_before_any_device_call():
    from mapf_amd import _lib
    fn = _lib.lib().mapf_imitation_loss
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(logits=p, f16=0, action=p, i64=0, R=4, A=5, loss=p, terms=p, grad=p)
    bad = [dict(logits=None), dict(action=None), dict(loss=None), dict(terms=None), dict(grad=None), dict(R=0),
           dict(R=-3), dict(A=1), dict(A=0), dict(A=17)]
    for change in bad:
        a = {**ok, **change}
        assert fn(*a.values(), None) == -1, change          # MAPF_EINVAL


# ---------------------------------------------------------------- two gloo ranks
KEYS = ["conv1.weight", "fully_connected_1.weight", "transformer.layers.0.0.fn.fn.to_qkv.weight", "token_wV",
        "policy_layer.weight", "value_layer.bias"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _imitate_once(world=1, rank=0):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "primal-ppo_amd"), os.path.join(ROOT, "tests")]
    import imitation_ref as ref
    from test_imitation_cpu import make_model
    obs, vec, action = ref.inputs()
    sl = slice(rank * ref.ROWS // world, (rank + 1) * ref.ROWS // world)
    m = make_model()
    stats = m.imitation_train(obs[sl], vec[sl], action[sl], None)
    return {k: v.clone() for k, v in m.network.state_dict().items()}, [float(np.asarray(s)) for s in stats]


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sd, stats = _imitate_once(world, rank)
        q.put((rank, {k: v.numpy() for k, v in sd.items() if k in KEYS}, stats))
    finally:
        dist.destroy_process_group()


def test_two_rank_imitation_update_equals_single_process():
    ref_sd, ref_stats = _imitate_once()
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res.sort(key=lambda x: x[0])
    for k in KEYS:
        np.testing.assert_array_equal(res[0][1][k], res[1][1][k])
        np.testing.assert_allclose(res[0][1][k], ref_sd[k].numpy(), rtol=1e-5, atol=1e-8, err_msg=k)
    assert res[0][2] == res[1][2]                      # the stats are the global minibatch's on every rank
    for got, want in zip(res[0][2], ref_stats):
        assert abs(got - want) < 1e-3 * max(1.0, abs(want))
