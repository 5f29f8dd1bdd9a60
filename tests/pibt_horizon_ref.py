"""The PIBT policy with a human weight and a human horizon (include/mapf.h: mapf_pibt_actions step 2,
mapf_set_pibt_human_horizon) restated in numpy over tests/pibt_human_ref.py and tests/pibt_ref.py: the
human's predicted cells from the oracle's own human (`next`, `step`, its current path), the candidate
keys priced by the highest level over those cells, and one pick over pibt_ref.solve and pibt_ref.Ages,
which neither weight nor horizon touches.  The oracle itself has no policy."""
import numpy as np

import pibt_human_ref as PH
import pibt_ref
from descent_ref import DC, DR

NA = pibt_ref.NA
KMAX = 8


def human_cells(oe, K):
    """P_1..P_K of the oracle env's current state, as (row, col) tuples: P_1 = the human's next cell
    whatever the path situation, P_j = path[step + j] while step + j <= len(path) - 1; shorter than K
    where the path ends."""
    hum, path = oe.human(), oe.human_path()
    cells = [(int(hum["next"][0]), int(hum["next"][1]))]
    for j in range(2, K + 1):
        if hum["step"] + j > len(path) - 1:
            break
        cells.append((int(path[hum["step"] + j][0]), int(path[hum["step"] + j][1])))
    return cells


def packed_cells(oe):
    """mapf_pibt_human_cells' row for the oracle env: P_1..P_8 as row | col << 16 in int32, -1 past the end."""
    out = -np.ones(KMAX, np.int64)
    for j, (r, c) in enumerate(human_cells(oe, KMAX)):
        out[j] = r | (c << 16)
    return out.astype(np.int32)


def candidate_keys(world, bfs, pos, hpos, cells, t, w, R):
    """pibt_ref.candidate_keys with dist' = dist if dist < 0 else
    min(dist + w * max_j level(R, |q - P_j|^2), 0x7FFE); cells = human_cells(): P_1 (= hn) first."""
    H, W = world.shape
    h, hn = (int(hpos[0]), int(hpos[1])), cells[0]
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
                lv = max(PH.level(R, (q[0] - pr) ** 2 + (q[1] - pc) ** 2) for pr, pc in cells)
                dist = min(dist + w * lv, 0x7FFE)
            key[i, a] = pibt_ref.pibt_key(dist, a, t, i)
    return key


def pibt_actions(world, oe, t, ages, w, R, K):
    """One pick for the oracle env oe at human weight w, penalty radius R and horizon K:
    (actions, failed, stats), as pibt_ref.pibt_actions."""
    pos, goals = oe.agents()
    age = ages.update(goals, t)
    key = candidate_keys(world, oe.bfs(), pos, oe.human()["pos"], human_cells(oe, K), t, w, R)
    act, failed, stats, _ = pibt_ref.solve(pos, key, age)
    return act, failed, stats
