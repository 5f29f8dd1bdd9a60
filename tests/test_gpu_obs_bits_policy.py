"""GPU: the policy side of bit-packed observations (include/mapf.h, "Packed observations").

Model.step / Model.value read a packed observation (the fused acting forward through
mapf_conv_first_bits), DeviceRunner(obs_bits=True) keeps its rollout packed, batch().observations
and Model.train_rows unpack only the rows they use.  Everything is compared bit for bit with the
float path under the same seeds.  The file ends with the coverage guard of
tests/test_gpu_obs_bits.py's oracle-compared packed rollout kernels.
"""
import copy

import numpy as np
import pytest
import torch

from test_obs_bits_cpu import pack_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def make_env(B, N=8, H=16, W=16, F=9, seed=99):
    from mapf_amd.config import make_config
    from mapf_amd.env import BatchedMapfGym
    from mapf_amd.maps import generate_warehouse
    env = BatchedMapfGym(make_config(B, H, W, num_agents=N, fov=F, num_channel=6, human_mode="random",
                                     goal_mode="random", fix_choice=1, seed=seed))
    env.reset_seeded(generate_warehouse(H, W))
    return env


def test_model_step_and_value_on_packed_input_equal_the_float_input():
    from mapf_amd.model import Model
    B, N = 3, 8
    env = make_env(B, N)
    try:
        env.random_actions()
        env.step()
        obs, vec = env.observe()
        bits, _ = env.observe_bits()
        torch.cuda.synchronize()
        assert np.array_equal(bits.cpu().numpy().view(np.uint32).reshape(B * N, -1), pack_np(obs.cpu().numpy(), 6, 9))
        torch.manual_seed(3)
        model = Model(0, "cuda", global_model=False, numChannel=6, num_agents=N, fov=9)
        outs = []
        for x in (obs, bits):
            torch.manual_seed(11)                 # the acting forward's dropout seeds come from torch's CPU generator
            a, ps, v, block, _, cv = model.step(x, vec, None, seed=5, step=2)
            torch.manual_seed(12)
            v2, cv2 = model.value(x, vec, None)
            outs.append((a, ps, v, block, cv, v2, cv2))
        torch.cuda.synchronize()
        for name, f, p in zip(("actions", "ps", "v", "block", "cv", "value v", "value cv"), *outs):
            assert f.dtype == p.dtype and torch.equal(f.view(torch.int32) if f.dtype == torch.float32 else f,
                                                      p.view(torch.int32) if p.dtype == torch.float32 else p), name
    finally:
        env.close()


B1, N1, T1 = 5, 8, 6


def run_pair():
    """The same rollout on a float and a packed DeviceRunner (same weights, env seeds, sampling seeds)."""
    from mapf_amd.model import Model
    from mapf_amd.runner import DeviceRunner
    torch.manual_seed(0)
    model = Model(0, "cuda", global_model=True, numChannel=6, num_agents=N1, fov=9)
    runners, perfs = [], []
    for packed in (False, True):
        runner = DeviceRunner(make_env(B1, N1), copy.deepcopy(model), n_steps=T1, seed=5, obs_bits=packed)
        torch.manual_seed(21)
        _, perf = runner.run()
        torch.cuda.synchronize()
        runners.append(runner)
        perfs.append(perf)
    return model, runners, perfs


@pytest.fixture(scope="module")
def pair():
    model, runners, perfs = run_pair()
    yield model, runners, perfs
    for r in runners:
        r.env.close()


def test_packed_device_runner_equals_the_float_runner(pair):
    from mapf_amd.runner import PERF_FIELDS
    _, (f, p), perfs = pair
    assert f.obs_bits is None and p.obs is None and p.packed and not f.packed
    assert tuple(p.obs_bits.shape) == (T1 + 1, B1, N1, 16) and p.obs_bits.dtype == torch.int32
    want = pack_np(f.obs.cpu().numpy(), 6, 9).reshape(T1 + 1, B1, N1, 16)
    assert np.array_equal(p.obs_bits.cpu().numpy().view(np.uint32), want), "the rollout's observations"
    for name in ("vec", "actions", "values", "cost_values", "ps", "rewards", "cost_rewards", "train_valid", "status",
                 "goals", "constraints", "shadow", "returns", "cost_returns", "adv", "cost_adv", "last_v", "last_cv"):
        a, b = getattr(f, name), getattr(p, name)
        assert torch.equal(a, b), name
    for k in PERF_FIELDS:
        assert getattr(perfs[0], k) == getattr(perfs[1], k), k
    pf, pp = f.performance_per_env(), p.performance_per_env()
    for k in PERF_FIELDS:
        np.testing.assert_array_equal(pf[k], pp[k], err_msg=k)
    # no float tensor of the whole rollout's observations anywhere in the packed runner
    full = (T1 + 1) * B1 * N1 * 6 * 9 * 9
    for name, t in vars(p).items():
        if isinstance(t, torch.Tensor):
            assert not (t.is_floating_point() and t.numel() >= full), name


def test_packed_batch_observations_unpack_the_rows_asked_for(pair):
    _, (f, p), _ = pair
    mf, mp = f.batch(), p.batch()
    assert mp.observations.shape == mf.observations.shape == (T1 * B1, N1, 6, 9, 9)
    assert mp.observations.dtype == torch.float32
    rows = np.array([0, 7, T1 * B1 - 1, 3, 3, 11])
    for idx in (rows, torch.from_numpy(rows).cuda(), slice(2, 9), 4):
        a, b = mf.observations[idx], mp.observations[idx]
        assert a.shape == b.shape and b.dtype == torch.float32 and torch.equal(a, b), idx
    assert torch.equal(mf.observations.materialize(), mp.observations.materialize())
    for name in ("vectors", "returns", "actions", "ps"):
        assert torch.equal(mf[name][rows], mp[name][rows]), name


def test_train_rows_on_packed_rows_equals_the_float_rows(pair):
    from mapf_amd.env import minibatch_rows
    model, (f, p), _ = pair
    rows = minibatch_rows(B1 * T1, 3, 0, 4, 8)
    stats = []
    for runner in (f, p):
        m = copy.deepcopy(model)
        torch.manual_seed(31)
        s1 = m.train_rows(runner, rows, 1.5)
        torch.manual_seed(32)
        s2 = m.train_rows(runner, rows.cpu().numpy(), 1.5)
        stats.append((s1, s2, [q.detach().clone() for q in m.network.parameters()]))
        if runner is p:
            upd = next(iter(m._updates.values()))
            assert tuple(upd.obs_stage.shape) == (8, N1, 16) and upd.obs_stage.dtype == torch.int32
            assert torch.equal(upd.obs, f.batch().observations[rows.cpu().numpy()])
    for k in range(2):
        for a, b in zip(stats[0][k], stats[1][k]):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (k, a, b)
    for a, b in zip(stats[0][2], stats[1][2]):
        assert torch.equal(a, b)


def test_model_train_takes_packed_observations(pair):
    model, (f, p), _ = pair
    rows = np.arange(6)
    stats = []
    for runner in (f, p):
        m = copy.deepcopy(model)
        mb = runner.batch()
        obs = mb.observations[rows] if runner is f else p.obs_bits[:T1].transpose(0, 1).reshape(B1 * T1, N1, 16)[rows]
        assert (obs.dtype == torch.int32) == (runner is p)
        torch.manual_seed(41)
        stats.append(m.train(obs, mb.vectors[rows], mb.returns[rows], mb.costReturns[rows], mb.values[rows],
                             mb.costValues[rows], mb.actions[rows], mb.ps[rows], mb.hiddenState[rows], mb.trainValid[rows], 1.5))
    for a, b in zip(*stats):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------ coverage guard (last)
@pytest.mark.parametrize("cfg", ["c1", "c2", "c4", "c5"])
def test_default_packed_kernels_were_compared_against_the_oracle(cfg):
    from test_gpu_obs_bits import BITS_COVERED
    from test_gpu_ycoverage import preset_env
    if not BITS_COVERED:
        pytest.fail("no oracle-compared packed rollout case ran before the guard (tests/test_gpu_obs_bits.py)")
    env = preset_env(cfg)
    try:
        assert env.rollout_fused, cfg
        for slots in (False, True):
            name = env.rollout_actions_kernel_name(slots, obs_bits=True)
            assert name in BITS_COVERED, (f"{cfg} slots={slots}: {env.rollout_actions_plan(slots, obs_bits=True)} is the "
                                          f"default packed launch but no oracle-compared case ran it; covered: {sorted(BITS_COVERED)}")
    finally:
        env.close()
