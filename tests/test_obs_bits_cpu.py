"""CPU: the bit-packed observation format (include/mapf.h, "Packed observations") on the host.

mapf_obs_bits_words, mapf_obs_pack_host and mapf_obs_unpack_host -- the host entry points over the
word function the kernels store with (csrc/mapf_obs_bits.h) -- and the CPU form of env.unpack_obs,
against the format's numpy definition: np.packbits(..., bitorder="little") of each agent's C*F*F
values, zero-padded to whole uint32 words.  Every comparison is exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from mapf_amd import _lib
from mapf_amd.config import make_config
from mapf_amd.env import obs_words, pack_obs, unpack_obs, unpack_obs_host

SHAPES = [(8, 6, 11), (8, 6, 9), (16, 6, 9), (64, 7, 11), (1, 6, 7), (5, 6, 8), (3, 5, 1)]    # (agents, C, F)
DENSITIES = [0.0, 0.3, 1.0]


def pack_np(obs, C, F):
    """The format: little-endian bit k % 32 of word k / 32 = float k of the agent's block."""
    cff = C * F * F
    wpa = (cff + 31) // 32
    a = np.asarray(obs).reshape(-1, cff)
    by = np.packbits(a != 0, axis=1, bitorder="little")
    pad = np.zeros((a.shape[0], 4 * wpa), np.uint8)
    pad[:, :by.shape[1]] = by
    return pad.view("<u4")


def draw(n, C, F, density, seed=0):
    rng = np.random.default_rng([seed, n, C, F, int(density * 10)])
    return (rng.random((n, C, F, F)) < density).astype(np.float32)


@pytest.mark.parametrize("n,C,F", SHAPES)
def test_words_per_agent(n, C, F):
    cfg = make_config(4, 16, 16, num_agents=min(n, 8), fov=F, num_channel=C)
    want = (C * F * F + 31) // 32
    assert _lib.lib().mapf_obs_bits_words(ctypes.byref(cfg)) == want == obs_words(C, F)


def test_words_of_the_baseline_configs():
    assert [obs_words(6, 11), obs_words(6, 9), obs_words(7, 11)] == [23, 16, 27]


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n,C,F", SHAPES)
def test_pack_host_is_the_numpy_format(n, C, F, density):
    obs = draw(n, C, F, density)
    bits = pack_obs(obs, C, F)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (n, obs_words(C, F))
    want = pack_np(obs, C, F)
    assert np.array_equal(bits.numpy().view(np.uint32), want)
    pad = 32 * obs_words(C, F) - C * F * F                # the padding bits of the last word are 0
    if pad:
        assert not (bits.numpy().view(np.uint32)[:, -1] >> np.uint32(32 - pad)).any()
    if density == 1.0:
        assert int(np.unpackbits(want.view(np.uint8)).sum()) == n * C * F * F


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n,C,F", SHAPES)
def test_unpack_host_round_trip(n, C, F, density):
    obs = draw(n, C, F, density, seed=1)
    bits = torch.from_numpy(pack_np(obs, C, F).view(np.int32).copy())
    back = unpack_obs_host(bits, C, F)
    assert back.dtype == torch.float32 and np.array_equal(back.numpy().view(np.uint32), obs.view(np.uint32))
    assert np.array_equal(unpack_obs_host(pack_obs(obs, C, F), C, F).numpy(), obs)


def test_pack_host_takes_any_nonzero_as_one_and_crosses_its_chunks():
    """More agents than one host chunk (256), leading dimensions kept, values other than 1.0."""
    C, F = 6, 11
    obs = draw(3 * 301, C, F, 0.3, seed=2).reshape(3, 301, C, F, F)
    scaled = obs * np.float32(-2.5)
    bits = pack_obs(scaled, C, F)
    assert tuple(bits.shape) == (3, 301, obs_words(C, F))
    assert np.array_equal(bits.numpy().view(np.uint32).reshape(-1, obs_words(C, F)), pack_np(obs, C, F))


def test_pack_host_of_no_agents():
    assert tuple(pack_obs(np.zeros((0, 6, 9, 9), np.float32), 6, 9).shape) == (0, 16)
    assert _lib.lib().mapf_obs_pack_host(None, 0, 6, 9, None) == 0
    assert _lib.lib().mapf_obs_pack_host(None, 1, 6, 9, None) != 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("n,C,F", SHAPES)
def test_cpu_unpack_obs_against_numpy(n, C, F, dtype):
    obs = draw(n, C, F, 0.3, seed=3)
    bits = torch.from_numpy(pack_np(obs, C, F).view(np.int32).copy()).reshape(n, -1)
    got = unpack_obs(bits, C, F, dtype=dtype)
    assert got.dtype == dtype and tuple(got.shape) == (n, C, F, F)
    assert np.array_equal(got.float().numpy(), obs)
    out = torch.full((n, C, F, F), 7.0, dtype=dtype)
    assert unpack_obs(bits, C, F, dtype=dtype, out=out) is out and np.array_equal(out.float().numpy(), obs)
    with pytest.raises(ValueError):
        unpack_obs(bits[:, :-1].contiguous(), C, F) if obs_words(C, F) > 1 else unpack_obs(bits.float(), C, F)


def test_a_forward_without_a_packed_reader_unpacks_first():
    """Every path but the fused acting forward (here: the CPU forward, acting and training) unpacks a
    packed observation into a scratch tensor and runs as on the floats: same seeds, same outputs."""
    from mapf_amd.model import Model
    N, C, F = 2, 6, 9
    torch.manual_seed(0)
    m = Model(0, "cpu", global_model=True, numChannel=C, num_agents=N, fov=F)
    obs = torch.from_numpy(draw(3 * N, C, F, 0.3, seed=4)).reshape(3, N, C, F, F)
    bits = pack_obs(obs, C, F)
    assert tuple(bits.shape) == (3, N, obs_words(C, F))
    vec = torch.randn(3, N, 4)
    outs = []
    for x in (obs, bits):
        torch.manual_seed(5)
        outs.append(m.value(x, vec, None))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with torch.enable_grad():
        res = []
        for x in (obs, bits):
            torch.manual_seed(6)
            res.append(m.network(x, vec, None)[0])
        assert res[0].requires_grad and torch.equal(res[0], res[1])
    with pytest.raises(ValueError, match="fov"):
        Model(0, "cpu", numChannel=C, num_agents=N).network(bits, vec, None)
