// primal-ppo_amd/csrc/mapf_fused.hip -- jointStep + getAllObservations in one
// launch (runner.py:84-97 calls env.jointStep then env.getAllObservations).
//
// A workgroup of 256 lanes steps E = 256 / NP^2 envs (step_pairs_env, one lane
// per agent pair) and then observes exactly those envs: the post-step cells,
// goals and human state go straight to LDS, so the observation needs no state
// reload and no second launch.  HBM traffic is the step's state + the
// observation stores; the step's latency-bound chains of one workgroup overlap
// the float4 store streams of the others.
//
// Workgroup roles, in grid order:
//  [0, nband)           the zero band (channel 5 while use_hp is off, all 0 by
//                       construction) of every agent's observation: HBM writes
//                       that need nothing from the step, issued while the step
//                       workgroups run their latency-bound chains; the step
//                       workgroups' float4 expansion skips exactly those float4s
//  [nband, +nsearch)    search work (below)
//  the rest             step + observe of E envs each
//
// The nsearch search workgroups run the search work of the PREVIOUS committed
// step (work-list slot `sslot`): humans' next paths (needed no earlier than
// two steps after they are queued -- a Human path start->goal->start has >= 3
// cells, mapf_gym.py:33-38) and agents' BFS maps (read only by mapf_bfs and
// the BFS channel, which is not fused).  The step of this launch reads none of
// what they write (the path buffer it walks is the other one).
#include <cstdio>
#include <type_traits>

#include "mapf_step_pairs.h"
#include "mapf_pibt.h"
#include "mapf_search.h"

namespace mapf {

// one wave per env observes on its own (NP = 8, shared map in registers, every
// env's observation a whole number of float4s)
__host__ __device__ inline bool fused_per_wave(const DevEnv &e) {
    return e.G == 8 && regmap_fits(e) && ((e.N * e.C * e.F * e.F) & 3) == 0;
}

// BITS: `obs` is the packed uint32 [B][N][WPA] buffer (mapf_obs_bits.h); the launch then has no
// zero-band workgroups (nband = 0: launch_np), whose float4 stores would overrun it.
template <int NP, bool HOST, bool BITS = false>
__global__ __launch_bounds__(256) void step_observe_kernel(DevEnv e, int32_t *__restrict__ actions, StepOut out,
                                                           uint32_t flags, int slot, float *__restrict__ obs,
                                                           float *__restrict__ vec, int nsearch, int sslot, int nband) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TL_STAMP(0);
    TL_HWID();
    if ((int)blockIdx.x < nband) {          // the zero band of every agent's observation
        const size_t K = (size_t)e.B * e.N;
        const size_t k0 = K * blockIdx.x / nband, k1 = K * (blockIdx.x + 1) / nband;
        obs_zero_band_store(e, obs, k0, k1, threadIdx.x, blockDim.x);
        TL_STAMP(1);
        return;
    }
    const int bx = (int)blockIdx.x - nband;
    if constexpr (HOST) {
        if (bx < nsearch) {
            const int wave = threadIdx.x >> 6;
            char *lds = smem + (size_t)wave * srch::wave_lds<uint32_t, 1>(e.H, e.W);
            srch::search_items<uint32_t, 1>(e, sslot, 0, lds, bx * (blockDim.x >> 6) + wave,
                                            nsearch * (blockDim.x >> 6));
            TL_STAMP(1);
            return;
        }
    } else {
        nsearch = 0;
    }
    constexpr int E = 256 / (NP * NP);
    const int blk = bx - nsearch;
    const int b0 = blk * E;
    const int nenv = min(E, e.B - b0);
    // the map words are loaded before the step's loads; at NP = 8 every wave holds
    // the whole shared map (lane k = word k) and the step reads it from registers,
    // and each wave then observes its own env with no workgroup barrier
    const bool regmap = NP == 8 && regmap_fits(e);
    const bool per_wave = regmap && fused_per_wave(e);
    ObsLds L = obs_layout(e, E, smem, per_wave);
    if (nband == 0) {     // the step workgroups write every float: nibble table for their store loops
        float4 *lut = reinterpret_cast<float4 *>(smem + ((obs_lds_bytes(e, E, per_wave) + 15) & ~(size_t)15));
        obs_lut_init(lut);
        __syncthreads();
        L.lut = lut;
    }
    const uint32_t mreg = obs_map_word(e, b0, nenv, regmap ? (int)(threadIdx.x & 63) : (int)threadIdx.x);
    PairsDeferred dfr;
    step_pairs_env<NP, true>(e, actions, out, flags, slot, blk * 256 + (int)threadIdx.x, L, b0,
                             RegMap{mreg, regmap}, dfr);
    TL_STAMP(1);
    if (per_wave) {
        const int le = (int)(threadIdx.x >> 6);
        if (le < nenv) {
            const ObsGroup g = obs_wave_init(e, L, le, mreg);
            TL_STAMP(2);
            obs_emit<false, BITS ? OBS_BITS : OBS_PLAIN>(e, L, obs, vec, g, b0, nband > 0);
        }
    } else {
        obs_init(e, L, E, b0, nenv, mreg);
        __syncthreads();
        TL_STAMP(2);
        obs_emit<false, BITS ? OBS_BITS : OBS_PLAIN>(e, L, obs, vec, obs_workgroup(L, nenv), b0, nband > 0);
    }
    step_pairs_finish(e, dfr, slot);
    TL_STAMP(3);
}

// The search work an INLINE step left in `d`, done by the same wave right away:
// agent.bfsMap of every agent whose goal changed (agent order), then the human's
// next path.  Same items, same results as the work-list searches.
// map: the env's padded obstacle rows in the wave's LDS; rs: the resident state,
// whose path lengths take the searched path's.
__device__ inline void step_pairs_search_inline(const DevEnv &e, const PairsDeferred &d, char *lds,
                                                const uint32_t *map, EnvRegs &rs) {
    for (uint64_t m = d.bmask; m; m &= m - 1ull) {
        const int l = __builtin_ctzll(m);
        const uint32_t ai = (uint32_t)__builtin_amdgcn_readlane((int)d.bitem, l);
        const uint32_t g = (uint32_t)__builtin_amdgcn_readlane((int)d.bgoal, l);
        srch::search_one<uint32_t, 1>(e, false, (int)(ai / (uint32_t)e.N), ai, g, NO_CELL, 0, lds, map);
    }
    if (d.rmask) {
        const int l = __builtin_ctzll(d.rmask);
        const int b = __builtin_amdgcn_readlane((int)d.ritem, l);
        const int buf = __builtin_amdgcn_readlane(d.rbuf, l);
        const int len = srch::search_one<uint32_t, 1>(e, true, b, 0u,
                                                      (uint32_t)__builtin_amdgcn_readlane((int)d.rstart, l),
                                                      (uint32_t)__builtin_amdgcn_readlane((int)d.rgoal, l), buf,
                                                      lds, map);
        if (buf) rs.hlen1 = len;
        else rs.hlen0 = len;
    }
}

// T committed random-policy steps + observations in ONE launch
// (mapf_rollout_random; runner.py:64-100 with the uniform policy, T times).
// Each wave owns one env for the whole launch and loops
//     step (pair lanes) -> observe its env (LDS bit-stream -> float4 stores)
//     -> its own search work (BFS maps, the human's next path)
// so a wave's latency-bound step runs while the other waves' observation stores
// drain: no launch boundary, dispatch ramp or state reload per step.  Step t's
// outputs go to slot t of the buffers when `slots` is set (rollout buffers).
struct RolloutOut {
    int32_t *actions;   // the drawn actions (out); TAPE: the caller's [T][B][N] tape, read only
    StepOut out;
    float *obs, *vec;
    int slots;
    int xcd_remap;
    int sub_lds;        // SUBS > 1: LDS bytes of one 4-env quarter (the pacing counters follow the quarters)
    int slack;          // SUBS > 1: a wave runs at most `slack` steps ahead of its group's slowest env (< 0: off)
    int fair;           // SUBS > 1, > 0: a wave more than `fair` steps ahead of the group's slowest env issues at
                        // priority 0, the others at 2 (no waiting; mapf_tuning.roll_fair)
};
// the kernel's arguments, read from device memory (ArgRing, mapf_kernels.h)
struct RolloutArgs {
    DevEnv e;
    RolloutOut ro;
};
// PIBT launches: the same with the handle's age arrays [B][N].  Types and a kernel of their own
// (rollout_random_pibt_kernel), so that the other policies' kernels keep their names, their
// argument layout and with it their register allocation (as mapf_rollout_wide.hip's).
struct RolloutOutPibt : RolloutOut {
    uint32_t *pibt_seen, *pibt_since;
};
struct RolloutArgsPibt {
    DevEnv e;
    RolloutOutPibt ro;
};
// Sparse launches (mapf_rollout_sparse): the same with the caller's shadow, uint32 [slots][B][16], and the
// number of leading slots it describes.  Types and a kernel of their own again (rollout_sparse_kernel):
// every other kernel keeps its arguments and its code.
struct RolloutOutSparse : RolloutOut {
    uint32_t *shadow;
    int valid;
};
struct RolloutOutPibtSparse : RolloutOutPibt {
    uint32_t *shadow;
    int valid;
};
template <class RO>
struct RolloutArgsOf {
    DevEnv e;
    RO ro;
};
// Perf launches (mapf_rollout_perf): every policy's, with the record [B] and whether the launch continues
// it; obs, vec and out are unused, `actions` is the caller's [T][B][N] (slots = 1) or the handle's [B][N]
// scratch (slots = 0: the caller asked for none).  One kernel per policy again (rollout_perf_kernel).
struct RolloutOutPerf : RolloutOutPibt {
    mapf_perf *perf;
    int accumulate;
};
__device__ inline mapf_perf *ro_perf(const RolloutOut &) { return nullptr; }
__device__ inline mapf_perf *ro_perf(const RolloutOutPerf &r) { return r.perf; }
__device__ inline int ro_accumulate(const RolloutOut &) { return 0; }
__device__ inline int ro_accumulate(const RolloutOutPerf &r) { return r.accumulate; }
__device__ inline uint32_t *ro_shadow(const RolloutOut &) { return nullptr; }
__device__ inline uint32_t *ro_shadow(const RolloutOutSparse &r) { return r.shadow; }
__device__ inline uint32_t *ro_shadow(const RolloutOutPibtSparse &r) { return r.shadow; }
__device__ inline int ro_valid(const RolloutOut &) { return 0; }
__device__ inline int ro_valid(const RolloutOutSparse &r) { return r.valid; }
__device__ inline int ro_valid(const RolloutOutPibtSparse &r) { return r.valid; }

__host__ __device__ inline bool rollout_fusable(const DevEnv &e) {
    return e.G == 8 && e.human_mode != 2 && e.goal_mode == 1 && e.C < 7 && !e.force_agent_lanes && fused_per_wave(e) &&
           e.W <= 30;
}

// LDS of a rollout workgroup: observation layout | nibble table | 4 search scratch | 4 path copies
__host__ __device__ inline size_t rollout_obs_lds(const DevEnv &e) { return ((obs_lds_bytes(e, 4, true) + 15) & ~(size_t)15) + 256; }
// TAPE: + 4 waves x TAPE_K staged rows (8 slots each, N <= 8) of the action tape (below)
// DESCENT, PIBT: + 4 waves x one row of 8 picked actions (the hand-over to the step's pair lanes)
constexpr int TAPE_K = 32;
__host__ __device__ inline size_t rollout_lds_bytes(const DevEnv &e, int policy) {
    return rollout_obs_lds(e) + 4 * srch::wave_lds<uint32_t, 1>(e.H, e.W) + 4 * (size_t)e.Lmax * 4 +
           (policy == ROLLOUT_TAPE ? 4 * (size_t)TAPE_K * 8 * 4
                                   : (policy == ROLLOUT_DESCENT || policy == ROLLOUT_PIBT ? 4 * (size_t)8 * 4 : 0));
}

// The perf form (mapf_rollout_perf) observes nothing: its LDS is the four envs' map rows | 4 search scratch |
// 4 path copies | the policy's rows
__host__ __device__ inline size_t rollout_perf_map_lds(const DevEnv &e) { return ((size_t)4 * e.Hp * e.WW * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t rollout_perf_lds_bytes(const DevEnv &e, int policy) {
    return rollout_lds_bytes(e, policy) - rollout_obs_lds(e) + rollout_perf_map_lds(e);
}

// ST (OBS_*, mapf_observe.h): OBS_NT, nontemporal observation stores -- for slot buffers (fresh HBM lines every step,
// measured faster); re-written [B]-leading buffers keep plain stores (their lines
// stay cache-resident between steps, measured faster).
// ST = OBS_BITS: ro.obs is the packed uint32 [T or 1][B][N][WPA] buffer (MAPF_SLOTS_OBS_BITS), slots
// or in place alike (plain stores: the slices are partial lines L2 merges, like the step outputs');
// never with BAND.
// SUBS 4-env quarters per workgroup: SUBS = 4 puts all 16 waves of a CU in one workgroup, so
// each can see how far the others are (pacing, below)
// BAND (0, OBS_BAND, OBS_SPARSE): OBS_BAND, a slot-buffer launch with MAPF_SLOTS_BAND_CLEAN -- the wave leaves
// out the stores that lie wholly inside its env's zero band (obs_band_skip; the band of every slot
// already holds zeros).  OBS_SPARSE (rollout_sparse_kernel, mapf_rollout_sparse): the wave leaves out
// every 64-B piece that held zeros by the caller's shadow and holds zeros again, and writes the
// shadow of what the slot holds now (mapf_observe.h); the band's pieces are always among those.
// TAPE: the caller's actions (mapf_rollout_actions) instead of the Philox draw.  Step t plays row
// [t][b] of ro.actions, [T][B][N] whatever `slots` says.  A vector load in the loop is waited
// for behind the wave's own observation stores (vmcnt counts both, in order) at every step:
// 2-3 % where the chip is partly filled and the step's latency sets the pace.
// So the wave stages its env's next TAPE_K rows in LDS -- the loop's one global read and one full
// drain per TAPE_K steps -- and the step reads its actions from LDS (step_pairs_env<.., LDSACT>).
// DESCENT: the descent policy (mapf_rollout_descent) instead of the Philox draw.  The env's state
// is in registers, so each agent's head lane reads the five cells of its tiled BFS map around
// rs.pi, picks (descent_action) and hands the action to the pair lanes through the wave's LDS row,
// as the tape does (LDSACT); ro.actions receives the picks like the random draw's.  The five loads
// are a plain per-step vector load: waited for behind the wave's observation stores.
// PIBT: the PIBT policy (mapf_rollout_pibt).  Agent i's cell, goal and age pair sit on its head lane
// 8 i; the head lanes read descent's five map cells and their cell's static mask, the wave solves
// over them (pibt_solve_wave<8>, mapf_pibt.h) and the picks go through descent's LDS row.  The age
// pair stays in registers across the steps and is written back after the last (RO = RolloutOutPibt).
// The loop is one text, mapf_fused_rollout.inc, included into both kernels below: as a device function
// called from them the other policies' kernels compiled to other code (the band form with scratch).
template <int ST, int SUBS, int BAND, int POL>      // POL: ROLLOUT_RANDOM / ROLLOUT_TAPE / ROLLOUT_DESCENT
__global__ __launch_bounds__(256 * SUBS) __attribute__((amdgpu_waves_per_eu(4))) void rollout_random_kernel(
#if MAPF_ARGS_PTR      // experiment build: arguments through a device pointer (mapf_rollout_wide.hip)
    const RolloutArgs *__restrict__ args, int T) {
    const DevEnv &e = args->e;
    const RolloutOut &ro = args->ro;
#else
    DevEnv e, int T, RolloutOut ro) {
#endif
    using RO = std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibt, RolloutOut>;     // RolloutOut: never PIBT here
    constexpr bool PERF = false;
#include "mapf_fused_rollout.inc"
}
// the PIBT form: the same loop, a kernel of its own because its arguments differ (RolloutOutPibt);
// the plan text names it by the form it shares, rollout_random_kernel<..,pibt>
// NOISY: the form with action noise (ROLLOUT_PIBT | ROLLOUT_NOISE), a symbol of its own
template <int ST, int SUBS, int BAND, bool NOISY = false>
__global__ __launch_bounds__(256 * SUBS) __attribute__((amdgpu_waves_per_eu(4))) void rollout_random_pibt_kernel(
#if MAPF_ARGS_PTR
    const RolloutArgsPibt *__restrict__ args, int T) {
    const DevEnv &e = args->e;
    const RolloutOutPibt &ro = args->ro;
#else
    DevEnv e, int T, RolloutOutPibt ro) {
#endif
    constexpr int POL = ROLLOUT_PIBT | (NOISY ? ROLLOUT_NOISE : 0);
    using RO = RolloutOutPibt;
    constexpr bool PERF = false;
#include "mapf_fused_rollout.inc"
}
// the sparse form: the same loop for all four policies (RO is a dependent type here), slot buffers only
template <int SUBS, int POL>
__global__ __launch_bounds__(256 * SUBS) __attribute__((amdgpu_waves_per_eu(4))) void rollout_sparse_kernel(
#if MAPF_ARGS_PTR
    const RolloutArgsOf<std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibtSparse, RolloutOutSparse>> *__restrict__ args, int T) {
    const DevEnv &e = args->e;
    const auto &ro = args->ro;
#else
    DevEnv e, int T, std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibtSparse, RolloutOutSparse> ro) {
#endif
    using RO = std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibtSparse, RolloutOutSparse>;
    constexpr int ST = OBS_NT, BAND = OBS_SPARSE;
    constexpr bool PERF = false;
#include "mapf_fused_rollout.inc"
}
// the perf form (mapf_rollout_perf): the same loop without the observation and without output stores,
// four envs per 256-thread workgroup, never grouped (SUBS = 1: pacing and priority by progress manage
// store drains, and this form has none)
template <int POL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void rollout_perf_kernel(DevEnv e, int T,
                                                                                                   RolloutOutPerf ro) {
    using RO = RolloutOutPerf;
    constexpr int ST = OBS_PLAIN, SUBS = 1, BAND = 0;
    constexpr bool PERF = true;
#include "mapf_fused_rollout.inc"
}
template <int ST, int SUBS, int BAND, int POL>
constexpr auto rollout_kernel_fn() {
    if constexpr (rollout_pol(POL) == ROLLOUT_PIBT) return &rollout_random_pibt_kernel<ST, SUBS, BAND, rollout_pol_noise(POL)>;
    else return &rollout_random_kernel<ST, SUBS, BAND, POL>;
}

bool rollout_random_fusable(const DevEnv &e) { return rollout_fusable(e) && rollout_lds_bytes(e, ROLLOUT_RANDOM) <= 64 * 1024; }

// a policy's LDS rows past the pair-lane kernel's 64 KiB go to the wide kernel (a tape, descent, PIBT)
int rollout_route(const DevEnv &e, const RolloutReq &q) {
    const size_t lds = q.form == ROLLOUT_PERF ? rollout_perf_lds_bytes(e, q.policy) : rollout_lds_bytes(e, q.policy);
    if (rollout_random_fusable(e) && lds <= 64 * 1024) return ROUTE_PAIRS;
    return rollout_wide_fusable(e) ? ROUTE_WIDE : ROUTE_STEPS;
}

// The pair-lane rollout's launch form for this handle's tuning (mapf.h: mapf_tuning).
struct RolloutPlan {
    int subs = 1;        // 4-env quarters per workgroup (4: the 16 waves of a CU in one workgroup)
    int grid = 0;        // workgroups
    size_t lds = 0;      // dynamic LDS request
    int sub_lds = 0, slack = -1, fair = 0, remap = 1;
    bool tape_ungrouped = false;   // tape / descent: their LDS rows did not fit the grouped form's LDS
};

// Persistent waves: every CU should hold the same number of workgroups, or the
// CUs holding more set the pace of every step.  The LDS request caps the
// workgroups per CU at occ = ceil(grid / CUs) (160 KiB of LDS per CU): a four-env workgroup's
// `lds` bytes, raised to the CU's even share
static size_t rollout_cu_share(const DevEnv &e, const mapf_tuning &tu, size_t lds, int &occ) {
    const int grid = (e.B + 3) / 4, ncu = device_cu_count();
    occ = tu.roll_occ >= 1 && tu.roll_occ <= 16 ? tu.roll_occ : (grid + ncu - 1) / ncu;
    const size_t cap = ((size_t)160 * 1024 / (size_t)occ) & ~(size_t)255;
    return occ >= 3 && cap > lds && cap <= 64 * 1024 ? cap : lds;
}

// ROUTE_PAIRS requests (the policy's LDS rows fit)
static RolloutPlan plan_rollout_random(const DevEnv &e, int slots, const mapf_tuning &tu, int policy, bool sparse) {
    RolloutPlan p;
    const int grid = (e.B + 3) / 4;
    int occ;
    const size_t lds = rollout_cu_share(e, tu, rollout_lds_bytes(e, policy), occ);
    // Slot buffers at four workgroups per CU (c2): one workgroup of all 16 waves instead,
    // each wave paced within `slack` steps of the slowest (RolloutOut::slack).  Unpaced,
    // each SIMD's four waves ran at 12.3 / 14.4 / 16.3 / 18.3 us per step by wave slot
    // (issue goes to the oldest) and the launch waited for the youngest; paced, all run
    // at 16.9 and the launch takes 17.5-17.7 us per step instead of 20.3
    // (tools/stamps_pairs.py, tools/ab_env.sh).
    // In place (c2): the same one workgroup per CU, but issue priority by progress instead of
    // waits: a wave more than 4 steps ahead of the group's slowest env drops to priority 0, the
    // rest run at 2 -- no wave ever idles, and the youngest wave of a SIMD no longer trails
    // (13.9-14.0 -> 11.9-12.0 us per step; roll_fair 0 with roll_group 0: four workgroups, unpaced).
    const size_t sub = (rollout_lds_bytes(e, policy) + 15) & ~(size_t)15;
    // Sparse launches into slots: with two thirds of the stores gone the store drain no longer sets the
    // pace, pacing's waits cost more than they save and priority by progress wins as it does in place
    // (2.41e9 against 2.01-2.03e9 agent-steps/s paced, 2.12e9 unpaced, 2.07e9 ungrouped).
    const int fair = tu.roll_fair >= 0 ? tu.roll_fair : (slots && !sparse ? 0 : 4);
    const bool want_group = occ == 4 && grid % 4 == 0 && (tu.roll_group < 0 ? slots != 0 || fair > 0 : tu.roll_group != 0);
    const bool group = want_group && 4 * sub + 64 <= (size_t)device_max_group_lds();
    p.tape_ungrouped = policy != ROLLOUT_RANDOM && want_group && !group &&
                       4 * ((rollout_lds_bytes(e, ROLLOUT_RANDOM) + 15) & ~(size_t)15) + 64 <= (size_t)device_max_group_lds();
    p.subs = group ? 4 : 1;
    p.grid = grid / p.subs;
    p.lds = group ? (size_t)device_max_group_lds() : lds;   // grouped: the whole CU
    p.sub_lds = (int)sub;
    p.fair = fair;
    p.slack = fair > 0 ? -1 : tu.roll_slack;
    p.remap = tu.xcd_remap != 0;
    return p;
}

// MAPF_SLOTS_BAND_CLEAN takes effect: slot buffers, a config-static zero band, one mask bit per store
static bool rollout_band_form(const DevEnv &e, int slots) {
    int z0, z1;
    return (slots & MAPF_SLOTS_BAND_CLEAN) && (slots & 1) && obs_zero_band(e, z0, z1) && obs_band_iters(e) <= 32;
}

// mapf_rollout_sparse takes effect: slot buffers of floats whose env slices are whole 64-B pieces
// (obs_sparse_applies); elsewhere the launch is the band-clean one
static bool rollout_sparse_form(const DevEnv &e, int slots, const float *obs) {
    return (slots & MAPF_SLOTS) && !(slots & MAPF_SLOTS_OBS_BITS) && obs_sparse_applies(e.N, e.C, e.F, (size_t)(uintptr_t)obs);
}

// what the pair-lane kernel stores of a request's observations: packed (",bits"), sparse, or all but the zero band
struct RolloutStores {
    bool bits, sparse, band;
};
static RolloutStores rollout_stores(const DevEnv &e, const RolloutReq &q) {
    RolloutStores f;
    f.bits = (q.slots & MAPF_SLOTS_OBS_BITS) != 0;
    f.sparse = q.form == ROLLOUT_SPARSE && rollout_sparse_form(e, q.slots, q.obs);
    f.band = !f.bits && !f.sparse && rollout_band_form(e, q.slots);      // packed zeros cost nothing to write
    return f;
}

void describe_rollout_random(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n) {
    const RolloutStores f = rollout_stores(e, q);
    const int slots = q.slots & 1, policy = q.policy;
    const RolloutPlan p = plan_rollout_random(e, slots, tu, policy, f.sparse);
    char band_tag[16] = "";
    if (f.band) std::snprintf(band_tag, sizeof band_tag, ",band%d", MAPF_BAND_UNIT);
    if (f.sparse) std::snprintf(band_tag, sizeof band_tag, ",sparse%d", OBS_SPARSE_PIECE * 4);
    if (f.bits) std::snprintf(band_tag, sizeof band_tag, ",bits");
    const int k = std::snprintf(buf, n, "rollout_random_kernel<%s,%d%s%s%s> grid=%d block=%d lds=%zu fair=%d slack=%d remap=%d",
                                slots ? "true" : "false", p.subs, band_tag, rollout_policy_tag(policy),
                                rollout_noise_tag(rollout_noisy(e, policy)), p.grid, 256 * p.subs,
                                p.lds, p.subs > 1 ? p.fair : 0, p.subs > 1 ? p.slack : -1, p.remap);
    if (k > 0 && (size_t)k < n) {
        if (policy == ROLLOUT_TAPE)
            std::snprintf(buf + k, n - (size_t)k, " tape_k=%d%s", TAPE_K, p.tape_ungrouped ? " ungrouped=tape_lds" : "");
        if (policy == ROLLOUT_DESCENT || policy == ROLLOUT_PIBT)
            std::snprintf(buf + k, n - (size_t)k, " fetch=load%s",
                          p.tape_ungrouped ? (policy == ROLLOUT_PIBT ? " ungrouped=pibt_lds" : " ungrouped=descent_lds") : "");
    }
}

#if MAPF_ARGS_PTR
template <class A>
A kernel_args_of(void (*)(const A *, int));      // the argument block a kernel reads (RolloutArgs*); never defined
#endif

int launch_rollout_random(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, ArgRing &ring, hipStream_t s) {
    const RolloutStores f = rollout_stores(e, q);
    const bool band = f.band && ((uintptr_t)q.obs & 15) == 0;     // whole float4s
    const int slots = q.slots & 1;
    const RolloutPlan p = plan_rollout_random(e, slots, tu, q.policy, f.sparse);
    const RolloutOut ro0{q.actions, q.out, q.obs, q.vec, slots, p.remap, p.sub_lds, p.slack, p.fair};
    auto launch = [&](auto kern, const auto &ro) -> int {
        const dim3 gd(p.grid), bd(256 * p.subs);
#if MAPF_ARGS_PTR
        using RA = decltype(kernel_args_of(kern));
        const RA *args = push_args(ring, RA{e, ro}, s);
        if (!args) return MAPF_ESTATE;      // a capture found no free argument slot: nothing launched
        hipLaunchKernelGGL(kern, gd, bd, p.lds, s, args, q.T);
#else
        (void)ring;
        hipLaunchKernelGGL(kern, gd, bd, p.lds, s, e, q.T, ro);
#endif
        return MAPF_OK;
    };
    return with_policy(q.policy, [&](auto pol) -> int {
        constexpr int POL = decltype(pol)::value;
        using RO = std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibt, RolloutOut>;
        RO ro{};
        static_cast<RolloutOut &>(ro) = ro0;
        if constexpr (rollout_pol(POL) == ROLLOUT_PIBT) {
            ro.pibt_seen = q.pibt_seen;
            ro.pibt_since = q.pibt_since;
        }
        if (f.sparse) {
            std::conditional_t<rollout_pol(POL) == ROLLOUT_PIBT, RolloutOutPibtSparse, RolloutOutSparse> rs{};
            static_cast<RO &>(rs) = ro;
            rs.shadow = q.shadow;
            rs.valid = q.valid;
            return p.subs == 4 ? launch(&rollout_sparse_kernel<4, POL>, rs) : launch(&rollout_sparse_kernel<1, POL>, rs);
        }
        if (f.bits)      // one instantiation for slots and in place (ro.slots is a run-time field)
            return p.subs == 4 ? launch(rollout_kernel_fn<OBS_BITS, 4, false, POL>(), ro) : launch(rollout_kernel_fn<OBS_BITS, 1, false, POL>(), ro);
        if (band)
            return p.subs == 4 ? launch(rollout_kernel_fn<true, 4, true, POL>(), ro) : launch(rollout_kernel_fn<true, 1, true, POL>(), ro);
        if (p.subs == 4)
            return slots ? launch(rollout_kernel_fn<true, 4, false, POL>(), ro) : launch(rollout_kernel_fn<false, 4, false, POL>(), ro);
        return slots ? launch(rollout_kernel_fn<true, 1, false, POL>(), ro) : launch(rollout_kernel_fn<false, 1, false, POL>(), ro);
    }, rollout_noisy(e, q.policy));
}

// ROLLOUT_PERF requests on the pair-lane kernel, never grouped.  The form's own request: map rows, search
// scratch, path copies, rows (c2: 4 workgroups of 4 waves per CU, the registers' 4 waves per SIMD, which this
// request leaves room for), raised like the observing forms'
static RolloutPlan plan_rollout_perf(const DevEnv &e, const mapf_tuning &tu, int policy) {
    RolloutPlan p;
    int occ;
    p.grid = (e.B + 3) / 4;
    p.lds = rollout_cu_share(e, tu, rollout_perf_lds_bytes(e, policy), occ);
    p.sub_lds = (int)((rollout_perf_lds_bytes(e, policy) + 15) & ~(size_t)15);
    p.remap = tu.xcd_remap != 0;
    return p;
}

void describe_rollout_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n) {
    const RolloutPlan p = plan_rollout_perf(e, tu, q.policy);
    std::snprintf(buf, n, "rollout_random_kernel<1%s,perf%s> grid=%d block=256 lds=%zu remap=%d", rollout_policy_tag(q.policy),
                  rollout_noise_tag(rollout_noisy(e, q.policy)), p.grid, p.lds, p.remap);
}

int launch_rollout_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, ArgRing &, hipStream_t s) {
    const RolloutPlan p = plan_rollout_perf(e, tu, q.policy);
    RolloutOutPerf ro{};
    static_cast<RolloutOut &>(ro) = RolloutOut{q.actions, StepOut{}, nullptr, nullptr, q.slots, p.remap, p.sub_lds, -1, 0};
    ro.pibt_seen = q.pibt_seen;
    ro.pibt_since = q.pibt_since;
    ro.perf = q.perf;
    ro.accumulate = q.accumulate;
    return with_policy(q.policy, [&](auto pol) -> int {
        hipLaunchKernelGGL(rollout_perf_kernel<decltype(pol)::value>, dim3(p.grid), dim3(256), p.lds, s, e, q.T, ro);
        return MAPF_OK;
    }, rollout_noisy(e, q.policy));
}

bool step_observe_fusable(const DevEnv &e) {
    if (e.G > 8 || e.force_agent_lanes || e.human_mode == 2 || e.C >= 7) return false;
    const int E = 256 / (e.G * e.G);
    return obs_lds_bytes(e, E, fused_per_wave(e)) <= 64 * 1024;
}

template <int NP>
static void launch_np(const DevEnv &e, int32_t *actions, const StepOut &out, uint32_t flags, int slot, float *obs,
                      float *vec, int nsearch, int sslot, hipStream_t s, bool bits) {
    constexpr int E = 256 / (NP * NP);
    const bool per_wave = NP == 8 && fused_per_wave(e);
    // zero-band workgroups: whole float4s only, so the step workgroups' slices
    // and the buffer must be 16-B aligned
    int z0, z1, nband = 0;
    const size_t slice = (size_t)E * e.N * e.C * e.F * e.F;
    // (never in a packed launch: the band workgroups store float4s)
    if (!bits && e.band_blocks > 0 && obs_zero_band(e, z0, z1) && (slice & 3) == 0 && ((uintptr_t)obs & 15) == 0)
        nband = e.band_blocks;
    const int grid = (e.B + E - 1) / E + nsearch + nband;
    size_t lds = obs_lds_bytes(e, E, per_wave);
    if (nband == 0) lds = ((lds + 15) & ~(size_t)15) + 256;   // + the nibble table
    if (nsearch > 0) {
        const size_t sl = 4 * srch::wave_lds<uint32_t, 1>(e.H, e.W);
        if (sl > lds) lds = sl;
        if (bits)
            hipLaunchKernelGGL((step_observe_kernel<NP, true, true>), dim3(grid), dim3(256), lds, s, e, actions, out,
                               flags, slot, obs, vec, nsearch, sslot, nband);
        else
        hipLaunchKernelGGL((step_observe_kernel<NP, true>), dim3(grid), dim3(256), lds, s, e, actions, out, flags,
                           slot, obs, vec, nsearch, sslot, nband);
    } else {
        if (bits)
            hipLaunchKernelGGL((step_observe_kernel<NP, false, true>), dim3(grid), dim3(256), lds, s, e, actions, out,
                               flags, slot, obs, vec, 0, 0, nband);
        else
        hipLaunchKernelGGL((step_observe_kernel<NP, false>), dim3(grid), dim3(256), lds, s, e, actions, out, flags,
                           slot, obs, vec, 0, 0, nband);
    }
}

void launch_step_observe(const DevEnv &e, int32_t *actions, const StepOut &out, uint32_t flags, int slot,
                         float *obs, float *vec, int nsearch, int sslot, hipStream_t s, bool bits) {
    if (!observe_hosts_search(e)) nsearch = 0;
    switch (e.G) {
        case 1: launch_np<1>(e, actions, out, flags, slot, obs, vec, nsearch, sslot, s, bits); break;
        case 2: launch_np<2>(e, actions, out, flags, slot, obs, vec, nsearch, sslot, s, bits); break;
        case 4: launch_np<4>(e, actions, out, flags, slot, obs, vec, nsearch, sslot, s, bits); break;
        default: launch_np<8>(e, actions, out, flags, slot, obs, vec, nsearch, sslot, s, bits); break;
    }
}

}  // namespace mapf
