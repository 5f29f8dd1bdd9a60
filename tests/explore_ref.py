"""Action noise (include/mapf.h: mapf_set_action_noise) restated in numpy over the oracle's Philox words
(oracle.philox_word): the explore draw of purpose P_NOISE, the random policy's draw of purpose P_ACT, and
`played` from a row of labels.  A plain module, no tests: test_action_noise_cpu.py compares the host export
with it, test_gpu_action_noise.py steps the oracle with what it returns."""
import functools

import numpy as np

from oracle import oracle as O

P_ACT, P_NOISE = 8, 12          # mapf_common.h / oracle/mapf_oracle.c: the Philox purposes
NA = 5


@functools.lru_cache(maxsize=1 << 16)
def words(purpose, env_id, group, clock, seed):
    """The four words of philox(env_id, purpose | group << 8, clock, 0; seed): one draw serves 8 agents."""
    return tuple(O.philox_word(int(env_id), purpose | (int(group) << 8), int(clock), 0, int(seed), w) for w in range(4))


def half(purpose, env_id, agent, clock, seed):
    """16-bit half-word agent & 7 of the agent's group draw: word (agent & 7) >> 1, shifted by ((agent & 7) & 1) * 16."""
    k = agent & 7
    return (words(purpose, env_id, agent >> 3, clock, seed)[k >> 1] >> ((k & 1) * 16)) & 0xFFFF


def random_action(env_id, agent, clock, seed):
    """The uniform random policy's action (mapf_random_actions, OracleEnv.random_actions)."""
    return (half(P_ACT, env_id, agent, clock, seed) * NA) >> 16


def noisy(env_id, agent, clock, seed, q16):
    return half(P_NOISE, env_id, agent, clock, seed) < q16


def played(labels, env_id, clock, seed, q16, random=None):
    """The actions env `env_id` (env_offset + b) plays at `clock` for its agents' labels [N] at noise q16.
    random: the random policy's actions [N] for that env and clock (OracleEnv.random_actions()), else taken
    from the same Philox words."""
    labels = np.asarray(labels, np.int32)
    out = labels.copy()
    for i in range(len(labels)):
        if q16 and noisy(env_id, i, clock, seed, q16):
            out[i] = random_action(env_id, i, clock, seed) if random is None else random[i]
    return out
