"""The PIBT policy (include/mapf.h: mapf_pibt_actions, mapf_pibt_key, mapf_pibt_host) restated in numpy
over the oracle's BFS maps, agent cells and goals, and human cells -- what the PIBT tests step the
oracle with.  The oracle itself has no policy.  Steps 1 (age), 2 (candidates) and 3 (solve) are
separate functions; solve() also counts what the tests' conditions on their inputs need."""
import numpy as np

from descent_ref import DC, DR

NA = 5
UNREACHABLE = 0x7FFF


def pibt_key(dist, a, t, i):
    k0 = (t + i) & 3
    cost = dist if dist >= 0 else UNREACHABLE
    rank = 0 if a == 0 else 1 + ((a - 1 - k0) & 3)
    return cost * 8 + rank


class Ages:
    """Step 1: the policy's own state, one (seen, since) pair per agent; reset() at every env reset."""

    def __init__(self, n):
        self.n = n
        self.reset()

    def reset(self):
        self.seen = [None] * self.n
        self.since = [0xFFFFFFFF] * self.n

    def update(self, goals, t):
        """The ages for a pick at clock t (idempotent at the same clock)."""
        age = np.zeros(self.n, np.uint32)
        for i in range(self.n):
            g = (int(goals[i][0]), int(goals[i][1]))
            if self.since[i] > t or self.seen[i] != g:
                self.seen[i], self.since[i] = g, t
            age[i] = t - self.since[i]
        return age


def candidate_keys(world, bfs, pos, hpos, hnext, t):
    """Step 2: key [N, 5], -1 where the action is not admitted (the step would give it -1 or -2)."""
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
            key[i, a] = pibt_key(int(bfs[i][q]), a, t, i)
    return key


def solve(pos, key, age):
    """Step 3.  Returns (actions int32 [N], failed: set of agents, stats, next cells) with stats =
    dict(inherit = calls PIBT(k, i) with a parent, backtracks = those that returned false, examined =
    candidates looked at)."""
    n = len(pos)
    cell = [(int(r), int(c)) for r, c in pos]
    at = {p: i for i, p in enumerate(cell)}
    cands = [sorted((int(key[i][a]), a) for a in range(NA) if key[i][a] >= 0) for i in range(n)]
    nxt = [None] * n
    held = {}                           # cell -> how many agents have it as their next
    act = np.zeros(n, np.int32)
    failed = set()
    stats = dict(inherit=0, backtracks=0, examined=0)

    def reserve(i, q):
        if nxt[i] is not None:
            held[nxt[i]] -= 1
        nxt[i] = q
        held[q] = held.get(q, 0) + 1

    def pibt(i, parent):
        for _, a in cands[i]:
            stats["examined"] += 1
            q = (cell[i][0] + DR[a], cell[i][1] + DC[a])
            if held.get(q, 0):                                  # vertex: some k has next_k == q
                continue
            if parent is not None and q == cell[parent]:        # swap with the agent that pushed
                continue
            reserve(i, q)
            act[i] = a
            k = at.get(q)
            if k is not None and k != i and nxt[k] is None:
                stats["inherit"] += 1
                if not pibt(k, i):
                    stats["backtracks"] += 1
                    continue
            return True
        reserve(i, cell[i])                                     # failed pick: stay, whatever the human does
        act[i] = 0
        failed.add(i)
        return False

    for i in sorted(range(n), key=lambda j: (-int(age[j]), j)):
        if nxt[i] is None:
            pibt(i, None)
    assert stats["examined"] <= 5 * n
    return act, failed, stats, nxt


def pibt_actions(world, bfs, pos, goals, hpos, hnext, t, ages):
    """One pick for one env: (actions, failed, stats).  world: its int8 map; bfs [N, H, W]
    (OracleEnv.bfs()); pos, goals [N, 2] (OracleEnv.agents()); hpos, hnext: OracleEnv.human()'s "pos"
    and "next"; t = steps since reset; ages: the env's Ages."""
    age = ages.update(goals, t)
    act, failed, stats, _ = solve(pos, candidate_keys(world, bfs, pos, hpos, hnext, t), age)
    return act, failed, stats
