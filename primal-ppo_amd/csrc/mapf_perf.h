// primal-ppo_amd/csrc/mapf_perf.h -- OneEpPerformance (mapf_perf, mapf.h) arithmetic shared by the
// host entry (mapf_perf_add_host), the reducing kernels (episode_sum_kernel, perf_accumulate_kernel)
// and the persistent rollout kernels' perf forms.
//
// The two float metrics are the reference's `perf.episodeReward += np.sum(rewards)`: numpy's
// pairwise float32 sum over the env's N values of a step (np_sum_f32), then a float32 running sum
// over the steps.  Every add rounds on its own: no contraction, no reassociation.
#pragma once
#include <cstdint>

#include "mapf.h"

#if defined(__HIPCC__)
#define MAPF_HD __host__ __device__
#else
#define MAPF_HD
#endif

namespace mapf {

// (every function below that adds floats turns contraction off in its own body: the header is included
// into every translation unit and must not change their floating-point mode)
// np.sum over a float32 [1, N] array (numpy's pairwise_sum, N <= 128: sequential below 8
// elements, else 8 strided accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
// remainder in order; the reduction's identity 0 added first)
MAPF_HD inline float np_sum_f32(const float *a, int n) {
#pragma clang fp contract(off)
    float res;
    if (n < 8) {
        res = 0.f;
        for (int i = 0; i < n; ++i) res = res + a[i];
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + a[i];
    }
    return 0.f + res;
}

// One step of one env added to its record from the step's [N] outputs; a NULL array leaves the
// metrics it feeds as they are (shadow_goals < 0: none).
MAPF_HD inline void perf_add_step(mapf_perf &p, int n, const int8_t *status, const float *reward_total,
                                  const float *cost, const float *goals_reached, int shadow_goals,
                                  const float *constraints) {
#pragma clang fp contract(off)
    if (reward_total) p.episode_reward = p.episode_reward + np_sum_f32(reward_total, n);
    if (cost) p.episode_cost_reward = p.episode_cost_reward + np_sum_f32(cost, n);
    for (int i = 0; i < n; ++i) {
        if (status) {
            p.human_collide += status[i] == -2;
            p.static_collide += status[i] == -1;
            p.agent_collide += status[i] == -3;
        }
        if (goals_reached) p.total_goals += goals_reached[i] == 1.f;
        if (constraints) p.constraint_violations += constraints[i] == 1.f;
    }
    if (shadow_goals >= 0) p.shadow_goals += shadow_goals;
}

#if defined(__HIPCC__)
// What a committed step leaves for the record, taken from the registers where the step's outputs are
// stored (step_pairs_env / step_group with PERF): per agent lane, zero on the lanes that hold no agent.
struct StepVals {
    int st = 0;                    // status
    float cost = 0.f, rtot = 0.f;  // cost, reward_total
    bool reached = false, cv = false;
    int nshadow = 0;               // the env's shadow goals (wave-uniform)
};

// the record of a wave's env across the steps of a persistent kernel: wave-uniform values
struct PerfAcc {
    float er = 0.f, ec = 0.f;
    int hc = 0, sc = 0, ac = 0, tg = 0, sg = 0, cn = 0;
};

__device__ inline float perf_rl(float x, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
}

// np_sum_f32 of the wave's n <= 64 values, element k on lane k: the eight strided accumulators are
// lanes 0..7, which add the later blocks of eight in order; every lane returns the sum
__device__ inline float wave_np_sum_f32(float x, int n, int lane) {
#pragma clang fp contract(off)
    float res;
    if (n < 8) {
        res = 0.f;
        for (int i = 0; i < n; ++i) res = res + perf_rl(x, i);
    } else {
        float r = x;
        const int full = n - (n % 8);
        for (int i = 8; i < full; i += 8) r = r + __shfl(x, i + (lane & 7), 64);
        res = ((perf_rl(r, 0) + perf_rl(r, 1)) + (perf_rl(r, 2) + perf_rl(r, 3))) +
              ((perf_rl(r, 4) + perf_rl(r, 5)) + (perf_rl(r, 6) + perf_rl(r, 7)));
        for (int i = full; i < n; ++i) res = res + perf_rl(x, i);
    }
    return 0.f + res;
}

// one step into the wave's record; STRIDE: agent k's values sit on lane k * STRIDE (1: the wide
// kernels' lane per agent, 8: the pair-lane kernels' head lanes)
template <int STRIDE>
__device__ inline void perf_acc_step(PerfAcc &p, const StepVals &v, int n, int lane) {
#pragma clang fp contract(off)
    float rt = v.rtot, co = v.cost;
    if constexpr (STRIDE > 1) {        // compact: lane k < 8 takes agent k's values
        rt = __shfl(rt, (lane & 7) * STRIDE, 64);
        co = __shfl(co, (lane & 7) * STRIDE, 64);
    }
    p.er = p.er + wave_np_sum_f32(rt, n, lane);
    p.ec = p.ec + wave_np_sum_f32(co, n, lane);
    p.hc += (int)__popcll(__ballot(v.st == -2));
    p.sc += (int)__popcll(__ballot(v.st == -1));
    p.ac += (int)__popcll(__ballot(v.st == -3));
    p.tg += (int)__popcll(__ballot(v.reached));
    p.cn += (int)__popcll(__ballot(v.cv));
    p.sg += v.nshadow;
}

// the record's eight words, one per lane 0..7: ordinary vector stores, once after the loop
__device__ inline void perf_acc_store(const PerfAcc &p, mapf_perf *dst, int lane) {
    int x = __float_as_int(p.er);
    x = lane == 1 ? __float_as_int(p.ec) : x;
    x = lane == 2 ? p.hc : x;
    x = lane == 3 ? p.sc : x;
    x = lane == 4 ? p.ac : x;
    x = lane == 5 ? p.tg : x;
    x = lane == 6 ? p.sg : x;
    x = lane == 7 ? p.cn : x;
    if (lane < 8) reinterpret_cast<int *>(dst)[lane] = x;
}

// the record to continue from (accumulate) or zeros
__device__ inline PerfAcc perf_acc_load(const mapf_perf *src, int accumulate) {
    PerfAcc p;
    if (accumulate) {
        p.er = src->episode_reward; p.ec = src->episode_cost_reward;
        p.hc = src->human_collide; p.sc = src->static_collide; p.ac = src->agent_collide;
        p.tg = src->total_goals; p.sg = src->shadow_goals; p.cn = src->constraint_violations;
    }
    return p;
}
#endif

}  // namespace mapf

#undef MAPF_HD
