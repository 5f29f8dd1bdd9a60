"""The descent policy (include/mapf.h: mapf_descent_actions, mapf_descent_pick) restated in numpy over
the oracle's BFS maps and agent cells -- what the descent tests step the oracle with.  The oracle
itself has no policy."""
import numpy as np

DR = (0, 0, 1, 0, -1)      # moves 1..4 = (0, +1), (+1, 0), (0, -1), (-1, 0): dr / dc of mapf_common.h
DC = (0, 1, 0, -1, 0)


def descent_mask(D, r, c):
    """Bit k (1..4): move k from (r, c) stays inside the map and lands on 0 <= D[target] < D[r, c]."""
    own, m = int(D[r, c]), 0
    for k in range(1, 5):
        rr, cc = r + DR[k], c + DC[k]
        if 0 <= rr < D.shape[0] and 0 <= cc < D.shape[1] and 0 <= int(D[rr, cc]) < own:
            m |= 1 << k
    return m


def descent_pick(mask, t, i):
    k0 = (t + i) & 3
    for m in range(4):
        k = 1 + ((k0 + m) & 3)
        if (mask >> k) & 1:
            return k
    return 0


def descent_actions(bfs, pos, t):
    """bfs [N, H, W] (OracleEnv.bfs()), pos [N, 2] (OracleEnv.agents()[0]), t = steps since reset."""
    acts = np.zeros(len(pos), np.int32)
    for i, (r, c) in enumerate(pos):
        if int(bfs[i, r, c]) > 0:
            acts[i] = descent_pick(descent_mask(bfs[i], int(r), int(c)), t, i)
    return acts
