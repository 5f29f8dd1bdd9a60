"""The PIBT policy with a human weight (include/mapf.h: mapf_pibt_actions step 2, mapf_set_pibt_human_weight,
mapf_pibt_human_level) restated in numpy over tests/pibt_ref.py: constr_d2 and the level from their fp64
definition, the candidate keys with the priced distance, and one pick over pibt_ref.solve and
pibt_ref.Ages, which the weight does not touch.  The oracle itself has no policy."""
import functools
import math

import numpy as np

import pibt_ref
from descent_ref import DC, DR

NA = pibt_ref.NA


@functools.lru_cache(maxsize=None)
def constr_d2(R):
    """The largest d2 with (R - sqrt(d2)) / R >= 0.01 in fp64: the step's own `constraints` rule."""
    best = -1
    for d2 in range(R * R + 1):
        if max(np.float64(R) - np.sqrt(np.float64(d2)), 0.0) / np.float64(R) >= 0.01:
            best = d2
    return best


def level(R, d2):
    """0 outside the constraint's disc, else R - floor(sqrt(d2)) (math.isqrt: the exact floor)."""
    return 0 if d2 > constr_d2(R) else R - math.isqrt(d2)


def candidate_keys(world, bfs, pos, hpos, hnext, t, w, R):
    """pibt_ref.candidate_keys with dist' = dist if dist < 0 else min(dist + w * level(R, |q - hn|^2), 0x7FFE)."""
    H, W = world.shape
    h, hn = (int(hpos[0]), int(hpos[1])), (int(hnext[0]), int(hnext[1]))
    key = -np.ones((len(pos), NA), np.int64)
    for i, (r, c) in enumerate(pos):
        p = (int(r), int(c))
        for a in range(NA):
            q = (p[0] + DR[a], p[1] + DC[a])
            if not (0 <= q[0] < H and 0 <= q[1] < W) or world[q] != 0:
                continue
            if q == hn or (p == hn and q == h):
                continue
            dist = int(bfs[i][q])
            if dist >= 0:
                dist = min(dist + w * level(R, (q[0] - hn[0]) ** 2 + (q[1] - hn[1]) ** 2), 0x7FFE)
            key[i, a] = pibt_ref.pibt_key(dist, a, t, i)
    return key


def pibt_actions(world, bfs, pos, goals, hpos, hnext, t, ages, w, R):
    """One pick for one env at human weight w and penalty radius R: (actions, failed, stats), as
    pibt_ref.pibt_actions."""
    age = ages.update(goals, t)
    act, failed, stats, _ = pibt_ref.solve(pos, candidate_keys(world, bfs, pos, hpos, hnext, t, w, R), age)
    return act, failed, stats
