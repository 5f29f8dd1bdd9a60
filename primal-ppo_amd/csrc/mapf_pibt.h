// primal-ppo_amd/csrc/mapf_pibt.h -- the PIBT policy on one wave (include/mapf.h: mapf_pibt_actions
// has the specification): priority inheritance with backtracking over the agents' BFS maps, one
// env per wave, one lane per agent.  That lane builds and sorts its five candidates in registers; the
// solve is wave-uniform: the current agent's data comes by v_readlane, "who holds / has reserved
// cell q" is a ballot, and the recursion's stack is the chain of parent indices held one per lane.
#pragma once
#include "mapf_common.h"

namespace mapf {

constexpr uint32_t PIBT_NONE = 0xFFFFFFFFu;     // a candidate that is not admitted; a target not yet chosen

// Step 1 of the policy: the age pair of one agent, updated for a pick at clock t.  Picking twice
// at the same clock changes nothing the second time.
__host__ __device__ inline uint32_t pibt_age(uint32_t &seen, uint32_t &since, uint32_t goal, uint32_t t) {
    if (since > t || seen != goal) {
        seen = goal;
        since = t;
    }
    return t - since;
}

// compare-exchange of the 5-element sorting network below
__device__ inline void pibt_cx(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}

// Step 2: the lane's candidates c[0..4] in ascending key, each (key << 3) | action, PIBT_NONE for
// the actions that are not admitted (they sort to the end).  D = the agent's tiled BFS map;
// st_mask = the static-invalid mask of its cell (smask: off the map or an obstacle), hp / hn the
// human's cell and next cell: the tests of step_group's getInvalidActions.  ahead(j), j in 2..K =
// the human's predicted cell P_j as a wave-uniform scalar (human_ahead(): NO_CELL past the path's
// end), from wherever the caller keeps the path; it is called only at a human horizon above 1.
// Five loads in flight, one wait, as descent_action().
template <class Ahead>
__device__ inline void pibt_candidates(const DevEnv &e, const int16_t *D, uint32_t p, unsigned st_mask, uint32_t hp,
                                       uint32_t hn, uint32_t clock, int agent, uint32_t c[NA], Ahead ahead) {
    const int r = prow(p), col = pcol(p);
    int v[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int rr = r + dr(k), cc = col + dc(k);
        const bool in = in_map(e, rr, cc);
        v[k] = (int)D[bfs_at(e.W, in ? rr : r, in ? cc : col)];
    }
    // The human weight (mapf.h, step 2): a reachable target costs pen = w * max_j level(R, |q - P_j|^2)
    // more, up to 0x7FFE.  The level never rises with d2, so the highest level over the cells is the
    // level of the smallest d2: the loop over j keeps five running minima of d2 (three VALU
    // instructions per target and cell) and the level is taken once, after it.  e.pibt_w (weight, R,
    // constr_d2 and the horizon in one word) is a kernel argument, so the branch and the loop are
    // wave-uniform: weight 0 runs none of it, and horizon 1 runs the j = 1 round (P_1 = hn) alone, with
    // no call of ahead().  None of it needs a loaded value, so it runs while the five map cells are in
    // flight.  The cells are consecutive on one path, so the first NO_CELL ends the loop.
    int pen[NA] = {0, 0, 0, 0, 0};
    if (e.pibt_w != 0) {
        const int w = pibt_w_weight(e.pibt_w), R = pibt_w_radius(e.pibt_w), cd2 = pibt_w_constr_d2(e.pibt_w);
        const int K = pibt_w_horizon(e.pibt_w);
        int d2[NA];
        const int hr = prow(hn), hc = pcol(hn);
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int y = r + dr(k) - hr, x = col + dc(k) - hc;
            d2[k] = y * y + x * x;
        }
        for (int j = 2; j <= K; ++j) {
            const uint32_t pj = ahead(j);
            if (pj == NO_CELL) break;
            const int jr = prow(pj), jc = pcol(pj);
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int y = r + dr(k) - jr, x = col + dc(k) - jc;
                d2[k] = min(d2[k], y * y + x * x);
            }
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) pen[k] = w * pibt_human_level(R, cd2, d2[k]);
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const uint32_t q = pack(r + dr(k), col + dc(k));
        const bool ok = !((st_mask >> k) & 1u) && q != hn && !(p == hn && q == hp);
        const int dist = v[k] < 0 ? v[k] : min(v[k] + pen[k], 0x7FFE);
        c[k] = ok ? ((uint32_t)pibt_key(dist, k, clock, agent) << 3) | (uint32_t)k : PIBT_NONE;
    }
    // optimal 9-comparator network for 5 keys
    pibt_cx(c[0], c[1]); pibt_cx(c[3], c[4]); pibt_cx(c[2], c[4]); pibt_cx(c[2], c[3]); pibt_cx(c[1], c[4]);
    pibt_cx(c[0], c[3]); pibt_cx(c[0], c[2]); pibt_cx(c[1], c[3]); pibt_cx(c[1], c[2]);
}

__device__ inline uint32_t pibt_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

// Step 3 on one wave: every lane of the wave calls it.  Agent i sits on lane i * STRIDE (1: lane =
// agent, the one-wave-per-env kernels; 8: the pair-lane kernel's head lanes); every other lane
// passes pos = NO_CELL and PIBT_NONE candidates and gets 0.  Returns the lane's action.  Agents are
// taken by (age descending, index ascending); every agent is entered at most once and at most 5 N
// candidates are examined, so the loop's hard bound of 6 N examinations is never reached -- past it
// every agent without a final pick stays.  Inside, agents are named by their lanes.
template <int STRIDE = 1>
__device__ inline int pibt_solve_wave(int N, int lane, uint32_t pos, const uint32_t c[NA], uint32_t age) {
    const bool live = lane % STRIDE == 0 && lane / STRIDE < N;
    // the agent's place in the order
    int rank = 0;
    for (int j = 0; j < N; ++j) {
        const uint32_t aj = pibt_rl(age, j * STRIDE);
        rank += (aj > age || (aj == age && j * STRIDE < lane)) ? 1 : 0;
    }
    uint32_t nxt = PIBT_NONE;       // the cell reserved (tentative while the agent is on the chain)
    int act = 0, cur = 0, par = -1; // chosen action, candidate cursor, the agent that pushed this one
    int iters = 0;
    const int bound = 6 * N;
    bool bail = false;
    for (int k = 0; k < N && !bail; ++k) {
        const uint64_t who = __ballot(live && rank == k);
        if (!who) break;                                   // cannot happen: ranks are a permutation
        int i = (int)__builtin_ctzll(who);
        if (pibt_rl(nxt, i) != PIBT_NONE) continue;        // decided as part of an earlier chain
        for (;;) {                                         // agent i: enter, or resume after a child failed
            int ci = __builtin_amdgcn_readlane(cur, i);
            const int pa = __builtin_amdgcn_readlane(par, i);
            const uint32_t pi = pibt_rl(pos, i);
            const uint32_t ppar = pa >= 0 ? pibt_rl(pos, pa) : NO_CELL;
            bool pushed = false, ok = false;
            while (ci < NA) {
                const uint32_t cv = ci == 0 ? c[0] : ci == 1 ? c[1] : ci == 2 ? c[2] : ci == 3 ? c[3] : c[4];
                const uint32_t cand = pibt_rl(cv, i);
                ++ci;
                if (cand == PIBT_NONE) { ci = NA; break; } // the admitted ones come first
                if (++iters > bound) { bail = true; break; }
                const int a = (int)(cand & 7u);
                const uint32_t q = pack(prow(pi) + dr(a), pcol(pi) + dc(a));
                if (__ballot(nxt == q)) continue;          // vertex: reserved by a decided agent
                if (q == ppar) continue;                   // swap with the agent that pushed
                if (lane == i) { nxt = q; act = a; }
                const uint64_t occ = __ballot(pos == q && nxt == PIBT_NONE);   // at most one: cells are distinct
                if (occ) {                                 // an undecided agent stands there: it inherits
                    const int child = (int)__builtin_ctzll(occ);
                    if (lane == child) par = i;
                    if (lane == i) cur = ci;
                    i = child;
                    pushed = true;
                } else {
                    ok = true;
                }
                break;
            }
            if (bail) {                                    // the chain's tentative picks become stays
                for (int n = 0; n < N && i >= 0; ++n) {
                    if (lane == i) { nxt = pos; act = 0; }
                    i = __builtin_amdgcn_readlane(par, i);
                }
                break;
            }
            if (pushed) continue;
            if (ok) break;                                 // the whole chain keeps its picks
            if (lane == i) { nxt = pos; act = 0; cur = NA; }   // failed pick: stay, whatever the human does
            if (pa < 0) break;
            i = pa;                                        // backtrack: the parent tries its next candidate
        }
    }
    return act;
}

}  // namespace mapf
