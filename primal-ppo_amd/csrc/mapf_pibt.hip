// primal-ppo_amd/csrc/mapf_pibt.hip -- the PIBT policy's actions for the current state
// (mapf_pibt_actions): one wave per env, lane = agent (mapf_pibt.h).
#include "mapf_kernels.h"
#include "mapf_pibt.h"

namespace mapf {

// Each lane reads its agent's cell, goal and age pair, the env's clock and human cells, then its
// five map cells (descent_action()'s loads); the solve exchanges everything through readlanes and
// ballots, so the kernel uses no LDS.  seen / since: the handle's age arrays [B][N].
__global__ __launch_bounds__(256) void pibt_actions_kernel(DevEnv e, int32_t *__restrict__ actions,
                                                           uint32_t *__restrict__ seen, uint32_t *__restrict__ since) {
    const int lane = (int)(threadIdx.x & 63u);
    const int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (b >= e.B) return;                 // the whole wave leaves together
    const bool live = lane < e.N;
    const size_t ai = (size_t)b * e.N + (live ? lane : 0);
    const uint32_t clock = e.clock[b], hp = e.hpos[b], hn = human_next(e, b);
    uint32_t p = NO_CELL, age = 0;
    uint32_t c[NA] = {PIBT_NONE, PIBT_NONE, PIBT_NONE, PIBT_NONE, PIBT_NONE};
    if (live) {
        p = e.pos[ai];
        uint32_t sn = seen[ai], sc = since[ai];
        age = pibt_age(sn, sc, e.goal[ai], clock);
        seen[ai] = sn;
        since[ai] = sc;
        const unsigned st = e.smask[(e.shared_map ? 0 : (size_t)b * e.H * e.W) + prow(p) * e.W + pcol(p)];
        // the human's predicted cells past hn, from its current path in HBM: uniform addresses
        pibt_candidates(e, e.bfs + ai * bfs_cells(e.H, e.W), p, st, hp, hn, clock, lane, c, [&](int j) {
            const int cur = e.hcur[b];
            return human_ahead(human_path(e, b, cur), e.hstep[b], e.hlen[b * 2 + cur], j);
        });
    }
    const int a = pibt_solve_wave(e.N, lane, p, c, age);
    if (live) actions[ai] = a;
}

// mapf_pibt_human_cells: cells [B][8] = P_1..P_8 of each env's current state, one thread per cell;
// P_1 = the human's next cell, the others by the pick's own lookup.
__global__ __launch_bounds__(256) void pibt_human_cells_kernel(DevEnv e, uint32_t *__restrict__ cells) {
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= e.B * PIBT_HORIZON_MAX) return;
    const int b = k / PIBT_HORIZON_MAX, j = k % PIBT_HORIZON_MAX + 1, cur = e.hcur[b];
    cells[k] = j == 1 ? human_next(e, b) : human_ahead(human_path(e, b, cur), e.hstep[b], e.hlen[b * 2 + cur], j);
}

void launch_pibt_human_cells(const DevEnv &e, uint32_t *cells, hipStream_t s) {
    hipLaunchKernelGGL(pibt_human_cells_kernel, dim3((e.B * PIBT_HORIZON_MAX + 255) / 256), dim3(256), 0, s, e, cells);
}

void launch_pibt_actions(const DevEnv &e, int32_t *actions, uint32_t *seen, uint32_t *since, hipStream_t s) {
    hipLaunchKernelGGL(pibt_actions_kernel, dim3((e.B + 3) / 4), dim3(256), 0, s, e, actions, seen, since);
}

}  // namespace mapf
