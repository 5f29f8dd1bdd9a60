// primal-ppo_amd/csrc/mapf_kernels.h -- host-side launchers of the MAPF kernels.
#pragma once
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "mapf.h"
#include "mapf_common.h"
#include "mapf_perf.h"

namespace mapf {

// Launch-configuration queries, cached per device (a process may drive several GPUs with
// different CU counts) and safe to call from several host threads.
inline int device_cu_count() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256;
    int v = dev < 64 ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (v > 0) return v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    if (dev < 64) cache[dev].store(v, std::memory_order_relaxed);
    return v;
}

// LDS bytes one workgroup may request (160 KiB on gfx950)
inline int device_max_group_lds() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 64 * 1024;
    int v = dev < 64 ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (v > 0) return v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) v = 64 * 1024;
    if (dev < 64) cache[dev].store(v, std::memory_order_relaxed);
    return v;
}

// VGPRs per lane of a kernel (one code object per arch: the same on every device here)
inline int kernel_vgprs(const void *fn) {
    static std::mutex m;
    static std::unordered_map<const void *, int> cache;
    std::lock_guard<std::mutex> lock(m);
    auto it = cache.find(fn);
    if (it != cache.end()) return it->second;
    hipFuncAttributes fa{};
    const int v = hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0 ? fa.numRegs : 512;
    cache.emplace(fn, v);
    return v;
}

struct StepOut {          // device pointers (mapf_step_out)
    int8_t *status;
    float *reward;
    int32_t *shadow_goals;
    float *cost;
    float *train_valid;
    int32_t *actions_fixed;
    float *goals_reached;
    float *constraints;
    float *reward_total;
};

// flags: bit0 commit (jointStep), bit1 random policy (draw actions in-kernel into `actions`)
void launch_step(const DevEnv &e, int32_t *actions, const StepOut &out, uint32_t flags, int parity, hipStream_t s);
bool launch_step_pairs(const DevEnv &e, int32_t *actions, const StepOut &out, uint32_t flags, int slot,
                       hipStream_t s);   // N <= 8: one lane per agent pair; false if N > 8
void launch_random_actions(const DevEnv &e, int32_t *actions, hipStream_t s);
// action noise over a row of labels [B][N] at the envs' clocks (mapf_noise_actions); played may be labels
void launch_noise_actions(const DevEnv &e, const int32_t *labels, int32_t *played, hipStream_t s);
// the descent policy's actions from the state and the tiled BFS maps (keep_bfs; mapf_descent_actions)
void launch_descent_actions(const DevEnv &e, int32_t *actions, hipStream_t s);
// the PIBT policy's actions from the state, the tiled BFS maps and the handle's age arrays seen /
// since [B][N], which it updates (keep_bfs; mapf_pibt_actions, mapf_pibt.hip): one wave per env
void launch_pibt_actions(const DevEnv &e, int32_t *actions, uint32_t *seen, uint32_t *since, hipStream_t s);
void launch_pibt_human_cells(const DevEnv &e, uint32_t *cells, hipStream_t s);
// humans' next paths (replan_list[parity]) + agent BFS maps (bfs_list[parity]);
// all = 1: every env's next path and every agent's map, 2: every env's next path,
// 3 / 4: the step's human paths / BFS maps only
void launch_search(const DevEnv &e, int parity, int all, hipStream_t s);
// agent.bfsMap of every agent, untiled: dist[B*N][H][W] (mapf_bfs)
void launch_bfs_export(const DevEnv &e, int16_t *dist, hipStream_t s);
// plan every human's next path from the state (promote: buffer hcur^1 becomes current first)
void launch_plan(const DevEnv &e, int promote, hipStream_t s);
// observations; the first nsearch workgroups run the search work of `parity`
// bits (here and in launch_step_observe): obs is the packed uint32 [B][N][WPA] buffer (mapf_obs_bits.h)
void launch_observe(const DevEnv &e, float *obs, float *vec, int nsearch, int parity, hipStream_t s, bool bits = false);
bool observe_hosts_search(const DevEnv &e);
// LDS of an observe_kernel workgroup of E envs (bit-stream .. index image, 16-byte round-up, nibble
// table), and what launch_observe requests for it at most: the four search waves' LDS where the launch
// may host the search and that is more
size_t observe_lds(const DevEnv &e, int E);
size_t observe_launch_lds(const DevEnv &e, int E);
// envs per observe workgroup: the default rule (64 / N fills a wave's lanes for N <= 8, else 1; at most B),
// and the largest E <= want whose launch request fits max_lds bytes (0: not even one env does)
int observe_default_envs(const DevEnv &e);
int observe_fit_envs(const DevEnv &e, int want, size_t max_lds);
// after a concurrent search: rewrite the BFS channel of the agents in bfs_list[parity]
void launch_bfs_fixup(const DevEnv &e, int parity, float *obs, hipStream_t s);
// committed step + observations in one launch (mapf_fused.hip); the first nsearch
// workgroups run the search work of list slot sslot (the previous step's)
bool step_observe_fusable(const DevEnv &e);
void launch_step_observe(const DevEnv &e, int32_t *actions, const StepOut &out, uint32_t flags, int slot,
                         float *obs, float *vec, int nsearch, int sslot, hipStream_t s, bool bits = false);
// T committed steps in one launch: the pair-lane kernel (mapf_fused.hip) or, for up to 64 agents / per-env
// maps / the BFS channel, one wave per env (mapf_rollout_wide.hip).
// policy: where the actions come from, the kernels' POL template parameter and the mark inside the angle
// brackets of the plan text (with descent and PIBT also bfsobs=0 in the wide three-wave form).  The PIBT
// kernels take the handle's age arrays in argument types of their own and are therefore symbols of their
// own over the shared bodies: rollout_random_pibt_kernel, rollout_wide_pibt_kernel, rollout_wide3_pibt_kernel.
constexpr int ROLLOUT_RANDOM = 0, ROLLOUT_TAPE = 1, ROLLOUT_DESCENT = 2, ROLLOUT_PIBT = 3;
// Action noise (mapf_set_action_noise) is a bit of the kernels' POL alone, never of a caller's policy:
// ROLLOUT_DESCENT / ROLLOUT_PIBT | ROLLOUT_NOISE are instantiations of their own, launched while the
// handle's noise_q16 is above 0, so the kernels of a launch without noise are the kernels of a build
// without the feature, register for register (DESIGN.md 9p has both placements' resource tables).  The
// PIBT kernels, symbols of their own, take it as a trailing bool.  The plan text carries ",noise" before
// the closing bracket.
constexpr int ROLLOUT_NOISE = 4;
constexpr int rollout_pol(int POL) { return POL & 3; }
constexpr bool rollout_pol_noise(int POL) { return (POL & ROLLOUT_NOISE) != 0; }
inline bool rollout_noisy(const DevEnv &e, int policy) {
    return e.noise_q16 != 0 && (policy == ROLLOUT_DESCENT || policy == ROLLOUT_PIBT);
}
inline const char *rollout_noise_tag(bool noisy) { return noisy ? ",noise" : ""; }
// f(std::integral_constant<int, policy>{}): the runtime policy as a template argument
template <class F>
inline auto with_policy(int policy, F f, bool noisy = false) {       // noisy: rollout_noisy() of the launch
    if (noisy && policy == ROLLOUT_PIBT) return f(std::integral_constant<int, ROLLOUT_PIBT | ROLLOUT_NOISE>{});
    if (noisy && policy == ROLLOUT_DESCENT) return f(std::integral_constant<int, ROLLOUT_DESCENT | ROLLOUT_NOISE>{});
    if (policy == ROLLOUT_PIBT) return f(std::integral_constant<int, ROLLOUT_PIBT>{});
    if (policy == ROLLOUT_DESCENT) return f(std::integral_constant<int, ROLLOUT_DESCENT>{});
    if (policy == ROLLOUT_TAPE) return f(std::integral_constant<int, ROLLOUT_TAPE>{});
    return f(std::integral_constant<int, ROLLOUT_RANDOM>{});
}
inline const char *rollout_policy_tag(int policy) {
    return policy == ROLLOUT_PIBT ? ",pibt" : (policy == ROLLOUT_DESCENT ? ",descent" : (policy == ROLLOUT_TAPE ? ",tape" : ""));
}
// One rollout call as its entry point received it; a *_plan call fills what it has (form, policy, slots, obs).
enum RolloutForm { ROLLOUT_OBSERVE, ROLLOUT_SPARSE, ROLLOUT_PERF };
struct RolloutReq {
    RolloutForm form;    // _SPARSE: mapf_rollout_sparse, text ",sparse64" (the pair-lane kernel where
                         // rollout_sparse_form, else as _OBSERVE); _PERF: mapf_rollout_perf, text ",perf"
    int policy;          // ROLLOUT_*
    int T;
    int slots;           // MAPF_SLOTS_* bits (_SPARSE: MAPF_SLOTS, and MAPF_SLOTS_BAND_CLEAN where the shadow
                         // describes every slot; _PERF: 1 with the caller's actions, else 0).  The wide kernels
                         // ignore MAPF_SLOTS_BAND_CLEAN; with MAPF_SLOTS_OBS_BITS the text carries ",bits"
    int32_t *actions;    // ROLLOUT_TAPE: the caller's [T][B][N] tape, read only; else where the picks go
                         // (_PERF: may be null, the picks are stored nowhere)
    StepOut out;         // _PERF: unused, as obs and vec
    float *obs, *vec;    // MAPF_SLOTS_OBS_BITS: obs is the packed uint32 buffer
    uint32_t *shadow;    // _SPARSE: the caller's piece masks, uint32 [slots][B][16], and the leading
    int valid;           //   slots they describe
    mapf_perf *perf;     // _PERF: the record [B], and whether the launch continues it
    int accumulate;
    uint32_t *pibt_seen, *pibt_since;   // the handle's age arrays [B][N], read and written back under ROLLOUT_PIBT only
};
// Where a request runs: ROUTE_PAIRS where the pair-lane kernel applies (rollout_random_fusable) and the
// policy's LDS rows fit its 64 KiB, else ROUTE_WIDE where rollout_wide_fusable, else ROUTE_STEPS (per-step
// launches).  The values are the kinds the *_plan calls return.  Launch and plan entries both switch on it;
// a launch_* or describe_* called on another route than its own is a programming error.
constexpr int ROUTE_STEPS = 0, ROUTE_PAIRS = 1, ROUTE_WIDE = 2;
bool rollout_random_fusable(const DevEnv &e);
bool rollout_wide_fusable(const DevEnv &e);
int rollout_route(const DevEnv &e, const RolloutReq &q);
// launch_*: MAPF_OK, or MAPF_ESTATE (nothing launched) if a captured launch found no free argument slot
// (ArgRing).  describe_*: the kernel's form from the handle's tuning (mapf.h: mapf_tuning) as text, the
// one launch_* would take.  *_perf: the kernels' perf forms, for ROLLOUT_PERF requests.
int launch_rollout_random(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, struct ArgRing &ring, hipStream_t s);
int launch_rollout_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, struct ArgRing &ring, hipStream_t s);
int launch_rollout_wide(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, struct ArgRing &ring, hipStream_t s);
int launch_rollout_wide_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, struct ArgRing &ring, hipStream_t s);
void describe_rollout_random(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n);
void describe_rollout_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n);
void describe_rollout_wide(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n);
void describe_rollout_wide_perf(const DevEnv &e, const RolloutReq &q, const mapf_tuning &tu, char *buf, size_t n);

// Device-resident kernel argument blocks.  A persistent kernel whose arguments (DevEnv + its
// output pointers, ~0.5 KiB) do not fit in the SGPR file kept them live from the kernarg
// load on and spilled ~450 SGPRs to VGPR lanes (v_readlane at every use, plus dead stack
// slots).  Read through a `const __restrict__` pointer instead, every field is an invariant
// scalar load the register allocator re-issues where it is used.  The block is written on
// the launch stream by a one-wave kernel that takes it by value (stream-ordered), into the
// next of ARG_SLOTS ring slots: launches on different streams in flight at once never share a
// slot unless more than ARG_SLOTS are.  A launch recorded into a hipGraph keeps its slot's
// address for every replay, so captured launches never take a ring slot (a later direct
// launch would overwrite it between replays): each gets one of ARG_CAPTURE_SLOTS slots of its
// own for the life of the handle, and a capture past them fails (MAPF_ESTATE).  The block's store
// (store_args_kernel) is captured with the kernel, so each replay re-writes its own slot first;
// after release_captures a slot may be shared by two graphs, whose replays must not overlap.
constexpr size_t ARG_SLOT_BYTES = 2048, ARG_SLOTS = 16, ARG_CAPTURE_SLOTS = 16;
struct ArgRing {
    char *base = nullptr;     // (ARG_SLOTS + ARG_CAPTURE_SLOTS) * ARG_SLOT_BYTES of device memory (the handle's)
    unsigned next = 0;        // ring position
    unsigned captured = 0;    // capture slots handed out
    void release_captures() { captured = 0; }
    template <class A>
    A *slot(bool capturing) {
        static_assert(sizeof(A) <= ARG_SLOT_BYTES, "argument block larger than a slot");
        if (capturing) {
            if (captured >= ARG_CAPTURE_SLOTS) return nullptr;
            return reinterpret_cast<A *>(base + (ARG_SLOTS + captured++) * ARG_SLOT_BYTES);
        }
        return reinterpret_cast<A *>(base + (size_t)(next++ % ARG_SLOTS) * ARG_SLOT_BYTES);
    }
};

template <class A>
__global__ __launch_bounds__(64) void store_args_kernel(A a, A *dst) {
    if (threadIdx.x == 0) *dst = a;
}

// a's copy in the ring's next slot (a capture slot while s is being captured), written on
// stream s before the kernel that reads it; nullptr when no capture slot is left
template <class A>
inline const A *push_args(ArgRing &ring, const A &a, hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    A *slot = ring.slot<A>(cap != hipStreamCaptureStatusNone);
    if (!slot) return nullptr;
    hipLaunchKernelGGL(store_args_kernel<A>, dim3(1), dim3(64), 0, s, a, slot);
    return slot;
}
// renderWorld (util.py:189-232) on the device (mapf_render.hip): frames [n][H*S][W*S][3] u8
struct RenderSpec {
    int scale;
    uint8_t palette[67 * 3];        // 0 free, 1 obstacle, 2 grey (human, path), 3 + i agent i
    double star_x[15], star_y[15];  // drawStar's r cos(a), r sin(a) per vertex (host libm, as the reference's math)
};
void launch_render(const DevEnv &e, const int32_t *envs, int n, const RenderSpec &rs, uint8_t *frames, hipStream_t s);
// obstacle maps on the device (mapf_maps.hip): kind 0 warehouse (length in [lo, hi]), 1 random
// density p; largest: keep only the largest 4-connected free component (H * W <= LC_MAX_CELLS)
struct MapGen {
    int kind, lo, hi, largest;
    float density;
    uint32_t epoch;
    uint64_t seed;
};
constexpr int LC_MAX_CELLS = 8192;
void launch_mapgen(const DevEnv &e, const MapGen &g, int8_t *maps, hipStream_t s);
// the padded obstacle bitmaps and static-action masks from int8 maps [nmaps][H][W] on the device
void launch_build_maps(const DevEnv &e, const int8_t *maps, hipStream_t s);
void launch_reset_fixed(const DevEnv &e, hipStream_t s);
void launch_reset_seeded(const DevEnv &e, hipStream_t s);
void launch_gae(const float *r, const float *v, const float *vl, float *adv, float *ret, int T, int M, float g,
                float gl, hipStream_t s);
void launch_normalize(const float *ret, const float *v, const float *cret, const float *cv, float *adv,
                      float *cadv, int M, float lam, float lam1, int mix, const float *lamd, hipStream_t s);
void launch_moments(const float *ret, const float *v, const float *cret, const float *cv, int M, const double *mean,
                    double *out, hipStream_t s);
void launch_normalize_stats(const float *ret, const float *v, const float *cret, const float *cv, const double *stats,
                            float *adv, float *cadv, int M, float lam, float lam1, int mix, const float *lamd,
                            hipStream_t s);
void launch_episode_sum(const float *x, int T, int B, int N, float *out, hipStream_t s);
void launch_perf_accumulate(const StepOut &o, int T, int B, int N, mapf_perf *perf, int accumulate, hipStream_t s);
void launch_sample(const float *ps, int stride, int32_t *a32, int64_t *a64, int M, uint64_t seed, uint32_t step,
                   hipStream_t s);
// minibatch rows and their gather (mapf_minibatch.hip).  GatherArgs: the arrays of a mapf_gather_spec
// with the nbig arrays of rows longer than GATHER_SMALL first; chunk_begin[k] = the first
// GATHER_CHUNK piece of big array k within a gathered row's chunks_per_row workgroups (>= 1: the
// row's first workgroup also copies the small arrays); bit k of vec16: array k moves in 16-byte accesses.
constexpr int64_t GATHER_CHUNK = 4096, GATHER_SMALL = 1024;
struct GatherArgs {
    const int64_t *rows;
    int T, B, count, nbig, chunks_per_row;
    uint32_t vec16;
    int chunk_begin[MAPF_GATHER_MAX + 1];
    int64_t row_bytes[MAPF_GATHER_MAX];
    const char *src[MAPF_GATHER_MAX];
    char *dst[MAPF_GATHER_MAX];
};
void launch_minibatch_rows(const ShuffleKey &key, int64_t start, int64_t count, int64_t *rows, hipStream_t s);
void launch_gather_rows(const GatherArgs &a, int64_t blocks, hipStream_t s);
// the gather with a symmetry per row (mapf_sym.hip).  SymGatherArgs: GatherArgs' layout with the row
// lengths of both sides and the kind of every array; "big" and the chunks go by the destination row.
// vec16: the array's plain copy (kind plain, or an identity row of float observations) and its
// observation stores may be 16 bytes wide.
struct SymGatherArgs {
    const int64_t *rows;
    const uint8_t *sym;          // NULL: identity for every row
    int T, B, count, nbig, chunks_per_row;
    int N, C, F;
    uint32_t vec16;
    int chunk_begin[MAPF_GATHER_MAX + 1];
    int kind[MAPF_GATHER_MAX];
    int64_t src_row_bytes[MAPF_GATHER_MAX], dst_row_bytes[MAPF_GATHER_MAX];
    const char *src[MAPF_GATHER_MAX];
    char *dst[MAPF_GATHER_MAX];
};
// packed words a piece of a gathered row can need in LDS: the agents under GATHER_CHUNK / 4 floats
constexpr int SYM_LDS_WORDS = 1280;
void launch_gather_rows_sym(const SymGatherArgs &a, int64_t blocks, hipStream_t s);
void launch_sym_draw(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed, uint8_t *out,
                     hipStream_t s);

}  // namespace mapf
