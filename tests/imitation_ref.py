"""Shared by tests/golden/make_golden_il.py and the imitation tests: the weight recipe and the inputs of
tests/golden/g9_imitation.npz, and the comparison helpers.

The weights are a function of the parameter names, so no state dict is stored; unlike g5_net's
det_weights (sines of amplitude 0.05, behind which the encoder's gradients vanish) every layer keeps
its fan-in variance, so every parameter's gradient stays visible in the imitation loss."""
import zlib

import numpy as np
import torch

ROWS, AGENTS, CHANNELS, FOV = 16, 8, 6, 9
GRAD_SLICE = 1024                       # stored elements of every gradient, in the parameter's contiguous order


def recipe_weights(named_shapes):
    """{name: float32 array}: rng = default_rng(crc32(name)); `*.weight` with >= 2 dims N(0, 2 / fan_in)
    with fan_in = prod(shape[1:]); 1-D `*.weight` 1 + 0.1 N(0, 1); everything else 0.05 N(0, 1)."""
    out = {}
    for name, shape in named_shapes:
        shape = tuple(int(s) for s in shape)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        x = rng.standard_normal(shape)
        if name.endswith(".weight") and len(shape) >= 2:
            x = x * np.sqrt(2.0 / float(np.prod(shape[1:])))
        elif name.endswith(".weight") and len(shape) == 1:
            x = 1.0 + 0.1 * x
        else:
            x = 0.05 * x
        out[name] = x.astype(np.float32)
    return out


def load_recipe(network):
    """network.load_state_dict of the recipe (parameters and buffers alike, by state-dict name)."""
    sd = network.state_dict()
    w = recipe_weights([(k, v.shape) for k, v in sd.items()])
    network.load_state_dict({k: torch.from_numpy(w[k]) for k in sd})
    return network


def inputs(rows=ROWS, agents=AGENTS, seed=11):
    """(obs float32 [rows, agents, 6, 9, 9] of 0 / 1, vec float32 [rows, agents, 4], action int64 [rows, agents]),
    drawn in that order from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    obs = (rng.random((rows, agents, CHANNELS, FOV, FOV)) < 0.2).astype(np.float32)
    vec = rng.standard_normal((rows, agents, 4)).astype(np.float32)
    action = rng.integers(0, 5, (rows, agents)).astype(np.int64)
    return obs, vec, action


def grad_key(name):
    return "grad_" + name.replace(".", "__")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def grad_slices(network):
    """{name: (L2 norm, first GRAD_SLICE elements)} of every parameter that holds a gradient."""
    out = {}
    for name, p in network.named_parameters():
        if p.grad is not None:
            g = p.grad.detach().float().cpu().contiguous().reshape(-1).numpy()
            out[name] = (float(np.linalg.norm(g.astype(np.float64))), g[:GRAD_SLICE].copy())
    return out
