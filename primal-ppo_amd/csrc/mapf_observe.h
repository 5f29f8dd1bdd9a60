// primal-ppo_amd/csrc/mapf_observe.h -- getAllObservations for one workgroup's
// envs, as device functions shared by observe_kernel (mapf_observe.hip) and the
// fused step+observe kernel (mapf_fused.hip).
//
// Reference: observe (mapf_gym.py:246-325), getAllObservations (:327-336),
// worldWithAgents (:192-198).  Per agent: C x F x F float32 channels
//   0 obstacle / off-map / self        3 visible agents' goals (clamped to FOV)
//   1 other agents                     4 human next position (+ danger disc if use_da)
//   2 own goal                         5 human.path[1:K+1] cells (use_hp)
//   6 (C = 7, this build's extension) BFS descent: bfsMap >= 0 and < own value
// and the vector [dx/d, dy/d, d, 0], d = (dx^2 + dy^2) ** .5 in float64.
//
// Every channel value is 0/1, so a workgroup first builds its agents'
// observations as ONE contiguous bit-stream in LDS (bit k of the stream =
// float k of the workgroup's slice of obs[B][N][C][F][F]) and then expands
// it with one float4 store per 4 bits: the kernel's HBM traffic is the
// C*F*F*4 bytes per agent it must write plus ~16 B of state per agent.
//
//  obs_init        zero stream / occupancy, stage the padded obstacle rows in LDS
//  obs_load_agents agents' cells and goals, human next cell and path (from HBM;
//                  the fused kernel's step writes them here instead)
//  obs_emit        1 agent occupancy bitmap of each env (worldWithAgents)
//                  2 (agent, FOV row) tasks: F-bit row segments of ch0/ch1 (+ DA, BFS)
//                  3 per agent: own goal, visible agents' goals, human, HP, vector
//                  4 stream -> float4 stores (coalesced, 1 KiB per wave instruction)
#pragma once
#include "mapf_common.h"
#include "mapf_obs_bits.h"

namespace mapf {

// How phase 4 of obs_emit writes the observation (a template argument: OBS_PLAIN and OBS_NT are
// the former `bool NT`'s false and true).  OBS_BITS: `obs` is the packed uint32 [..][N][WPA] buffer
// (mapf_obs_bits.h) instead of float [..][N][C][F][F].
constexpr int OBS_PLAIN = 0, OBS_NT = 1, OBS_BITS = 2;

// LDS carve-up of an observing workgroup (E envs).  per_env: every env has its
// own word-aligned bit-stream (stride swe words) and its own copy of the map
// rows, so one wave can observe its env with no workgroup barrier.
struct ObsLds {
    int swe;                    // per-env stream stride in words (0: one stream for the workgroup)
    uint32_t *stream, *occ, *mapc, *spos, *sgoal, *shn, *shp;
    int32_t *shpn;
    uint8_t *idg;               // [E][H*W] agent index at each occupied cell (read only where occ is set)
    uint32_t *bfsw;             // BFS channel: [E*N][F][WD] dwords = 2*WD int16 cells of each FOV row's
    int32_t *bfsown;            //   bfsMap window, from column (tc & ~1); [E*N] bfsMap at the agent's cell
    const float4 *lut;          // optional [16] float4: nibble -> its 4 bits as 0.f / 1.f (obs_lut_init)
    int stream_words, rowsz;
    bool bfs_win;               // BFS channel read through the LDS windows (else straight from HBM per task)
};

__host__ __device__ inline int obs_stream_words(const DevEnv &e, int E) { return (E * e.N * e.C * e.F * e.F + 31) / 32 + 1; }

__host__ __device__ inline bool obs_bfs_windows(const DevEnv &e) { return e.C >= 7 && e.keep_bfs && (e.W & 1) == 0; }
__host__ __device__ inline int obs_bfs_wd(const DevEnv &e) { return (e.F + 2) >> 1; }   // dwords per window row

__host__ __device__ inline int obs_env_stream_words(const DevEnv &e) {
    return ((e.N * e.C * e.F * e.F + 31) / 32 + 1 + 3) & ~3;
}

__host__ __device__ inline size_t obs_lds_bytes(const DevEnv &e, int E, bool per_env = false) {
    const int rowsz = e.Hp * e.WW;
    const int nmap = (e.shared_map && !per_env) ? 1 : E;
    const size_t sw = per_env ? (size_t)E * obs_env_stream_words(e) : (size_t)((obs_stream_words(e, E) + 3) & ~3);
    const size_t words = sw + (size_t)E * rowsz + (size_t)nmap * rowsz +
                         2 * (size_t)E * e.N + E + (size_t)E * e.k_predict + E;
    const size_t bfs_words = obs_bfs_windows(e) ? (size_t)E * e.N * (e.F * obs_bfs_wd(e) + 1) : 0;
    return (words + bfs_words) * 4 + (((size_t)E * e.H * e.W + 3) & ~(size_t)3);
}

__device__ inline ObsLds obs_layout(const DevEnv &e, int E, char *smem, bool per_env = false) {
    ObsLds L;
    L.swe = per_env ? obs_env_stream_words(e) : 0;
    L.stream_words = per_env ? E * L.swe : obs_stream_words(e, E);
    L.rowsz = e.Hp * e.WW;
    const int nmap = (e.shared_map && !per_env) ? 1 : E;
    L.stream = reinterpret_cast<uint32_t *>(smem);
    L.occ = L.stream + ((L.stream_words + 3) & ~3);
    L.mapc = L.occ + E * L.rowsz;
    L.spos = L.mapc + nmap * L.rowsz;
    L.sgoal = L.spos + E * e.N;
    L.shn = L.sgoal + E * e.N;                  // [E] human next
    L.shp = L.shn + E;                          // [E][k_predict] human.path[1..K]
    L.shpn = reinterpret_cast<int32_t *>(L.shp + E * e.k_predict);   // [E] count
    L.bfsw = reinterpret_cast<uint32_t *>(L.shpn + E);
    L.bfsown = reinterpret_cast<int32_t *>(L.bfsw + (obs_bfs_windows(e) ? (size_t)E * e.N * e.F * obs_bfs_wd(e) : 0));
    L.idg = reinterpret_cast<uint8_t *>(L.bfsown + (obs_bfs_windows(e) ? E * e.N : 0));
    L.lut = nullptr;
    L.bfs_win = obs_bfs_windows(e);
    return L;
}

// the 16-entry nibble -> float4 table (256 B of LDS, 16-B aligned), filled by the
// first 16 threads; the caller synchronises before use
__device__ inline void obs_lut_init(float4 *lut) {
    const int t = (int)threadIdx.x;
    if (t < 16) lut[t] = make_float4((float)(t & 1), (float)((t >> 1) & 1), (float)((t >> 2) & 1), (float)(t >> 3));
}

namespace obsd {

__device__ inline uint32_t seg_at(const uint32_t *row, int WW, int off, int F) {
    const int w = off >> 5, s = off & 31;
    const uint64_t a = (uint64_t)row[w] | ((w + 1 < WW) ? ((uint64_t)row[w + 1] << 32) : 0ull);
    return (uint32_t)(a >> s) & ((1u << F) - 1u);
}

__device__ inline void or_bits(uint32_t *stream, int off, uint32_t seg, int F) {
    if (!seg) return;
    const int w = off >> 5, s = off & 31;
    atomicOr(&stream[w], seg << s);
    if (s + F > 32) {
        const uint32_t hi = seg >> (32 - s);
        if (hi) atomicOr(&stream[w + 1], hi);
    }
}

__device__ inline void set_bit(uint32_t *stream, int off) { atomicOr(&stream[off >> 5], 1u << (off & 31)); }

__device__ inline int isqrt_floor(int x) {
    int r = (int)sqrtf((float)x);
    while (r * r > x) --r;
    while ((r + 1) * (r + 1) <= x) ++r;
    return r;
}

}  // namespace obsd

// Zero the bit-stream and the occupancy maps.  Staging the obstacle rows is
// split so a caller can issue the loads early and store them later:
// obs_map_word() loads word k of the workgroup's maps, obs_init() stores the
// first blockDim.x words from `mreg` and loads+stores the rest itself.
__device__ inline uint32_t obs_map_word(const DevEnv &e, int b0, int nenv, int k) {
    const int rowsz = e.Hp * e.WW;
    const int nw = e.shared_map ? rowsz : nenv * rowsz;
    if (k >= nw) return 0u;
    return e.shared_map ? e.map_bits[k] : e.map_bits[(size_t)b0 * rowsz + k];
}

__device__ inline void obs_init(const DevEnv &e, const ObsLds &L, int E, int b0, int nenv, uint32_t mreg) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = tid; k < L.stream_words; k += nt) L.stream[k] = 0u;
    for (int k = tid; k < E * L.rowsz; k += nt) L.occ[k] = 0u;
    const int nw = e.shared_map ? L.rowsz : nenv * L.rowsz;
    if (tid < nw) L.mapc[tid] = mreg;
    for (int k = tid + nt; k < nw; k += nt) L.mapc[k] = obs_map_word(e, b0, nenv, k);
}

__device__ inline void obs_load_agents(const DevEnv &e, const ObsLds &L, int b0, int nenv, int tid, int nt) {
    const int N = e.N, K = nenv * N;
    for (int k = tid; k < K; k += nt) {
        L.spos[k] = e.pos[(size_t)b0 * N + k];
        L.sgoal[k] = e.goal[(size_t)b0 * N + k];
    }
    for (int k = tid; k < nenv; k += nt) {
        const int b = b0 + k;
        L.shn[k] = human_next(e, b);
        int cnt = 0;
        if (e.use_hp && e.C >= 6) {
            const int cur = e.hcur[b];
            const int len = e.hlen[b * 2 + cur];
            const uint32_t *path = human_path(e, b, cur);
            for (int q = 1; q <= e.k_predict && q < len; ++q) L.shp[k * e.k_predict + cnt++] = path[q];
        }
        L.shpn[k] = cnt;
    }
}
__device__ inline void obs_load_agents(const DevEnv &e, const ObsLds &L, int b0, int nenv) {
    obs_load_agents(e, L, b0, nenv, (int)threadIdx.x, (int)blockDim.x);
}

// The config-static zero band of an agent's [C][F][F] block: channel 5
// (human.path[1:K+1], mapf_gym.py:293-297) is written only when use_hp is on,
// so with use_hp off every one of its floats is 0 at every step.  Returns the
// band's float offsets [z0, z1) inside the block, or false if there is none.
__host__ __device__ inline bool obs_zero_band(const DevEnv &e, int &z0, int &z1) {
    if (e.use_hp || e.C < 6 || e.F * e.F > 124) return false;    // <= 31 whole float4s (32 lanes per agent)
    z0 = 5 * e.F * e.F;
    z1 = 6 * e.F * e.F;
    return true;
}

// The skip set of a slot-buffer rollout launched with MAPF_SLOTS_BAND_CLEAN (mapf.h): the caller
// guarantees that the zero band of every slot already holds zeros, so the band's whole `unit`-byte
// pieces (16, 64 or 128, at unit-aligned absolute addresses) need no store.  Float4 q of an env's
// observation, whose slice starts at byte address `off` (16-B aligned; only off % unit matters),
// is skipped iff the aligned unit around it lies wholly inside one agent's band -- never a byte
// outside the band.  The one function both the kernel and the host (mapf_obs_band_skip) evaluate.
__host__ __device__ inline bool obs_band_skip(const DevEnv &e, int unit, size_t off, int q) {
    int z0, z1;
    if (!obs_zero_band(e, z0, z1)) return false;
    const uint32_t ab = (uint32_t)(e.C * e.F * e.F) * 4u;              // bytes per agent
    const uint32_t o = (uint32_t)(off & (size_t)(unit - 1));
    const uint32_t u0 = (o + 16u * (uint32_t)q) & ~(uint32_t)(unit - 1);   // the unit, from the aligned base below off
    if (u0 < o) return false;                                          // it begins before the env's slice
    const uint32_t r0 = u0 - o, r1 = r0 + (uint32_t)unit;               // the unit within the env's slice
    const uint32_t k = r0 / ab;
    return r0 >= k * ab + 4u * (uint32_t)z0 && r1 <= k * ab + 4u * (uint32_t)z1;
}
// The wave store loop's iterations per env (lane l stores float4 l + 64k, k < obs_band_iters), and
// a lane's skip set as one bit per iteration (obs_emit<.., BAND>); a mask holds at most 32
__host__ __device__ inline int obs_band_iters(const DevEnv &e) { return ((e.N * e.C * e.F * e.F) / 4 + 63) / 64; }
__host__ __device__ inline uint32_t obs_band_skip_mask(const DevEnv &e, int unit, size_t off, int lane) {
    const int nq = (e.N * e.C * e.F * e.F) >> 2;
    uint32_t m = 0;
    for (int k = 0, q = lane; q < nq && k < 32; ++k, q += 64)
        if (obs_band_skip(e, unit, off, q)) m |= 1u << k;
    return m;
}
// The unit a flagged launch skips in: the measured choice (holes of whole
// 64-B pieces cost the store stream nothing, 16-B holes leave partial pieces and run slower than
// no holes at all).  An experiment build may pass another one of 16, 64, 128.
#ifndef MAPF_BAND_UNIT
#define MAPF_BAND_UNIT 64
#endif

// The band's whole float4s of agents [k0, k1) of `obs` (16-B aligned), written
// as zeros by `nt` threads numbered `t`: float4 q of the buffer belongs to the
// band iff 4q >= k*CFF + z0 and 4q + 4 <= k*CFF + z1 for its agent k.  The fused
// launch runs this in workgroups of their own while the step's latency-bound
// chains run in the others; obs_emit(skip_band) then skips exactly these float4s.
__device__ inline void obs_zero_band_store(const DevEnv &e, float *__restrict__ obs, size_t k0, size_t k1, size_t t,
                                           size_t nt) {
    int z0, z1;
    if (!obs_zero_band(e, z0, z1)) return;
    const size_t CFF = (size_t)e.C * e.F * e.F;
    float4 *o4 = reinterpret_cast<float4 *>(obs);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t idx = k0 * 32 + t; idx < k1 * 32; idx += nt) {      // 32 lanes per agent (a band has <= 31 float4s)
        const size_t k = idx >> 5, j = idx & 31;
        const size_t qa = (k * CFF + z0 + 3) >> 2, qb = (k * CFF + z1) >> 2;
        if (qa + j < qb) o4[qa + j] = zero;
    }
}

// ---- the sparse form of a slot-buffer rollout (obs_emit<.., OBS_SPARSE>; mapf.h: mapf_rollout_sparse) ----
// A piece is 16 consecutive floats (64 B) of an env's [N][C][F][F] slice; the caller's shadow holds
// one bit per piece of every env-slot, uint32 [slots][B][16]: bit p of the 16 words is 1 iff piece p
// holds a non-zero float.  A step whose slot the shadow describes stores exactly the pieces that were
// or become non-zero; the others hold zeros and stay.  The band's pieces are among those.
constexpr int OBS_BAND = 1, OBS_SPARSE = 2;        // obs_emit's BAND argument (0: every float stored)
constexpr int OBS_SPARSE_WORDS = 16, OBS_SPARSE_PIECE = 16;   // words per env-slot, floats per piece
// The form applies where an env's slice is a whole number of pieces that the 16 words can name and
// every slice starts on a 64-B line (holes finer than 64 B cost more than they save: DESIGN.md 9d).
__host__ __device__ inline bool obs_sparse_applies(int N, int C, int F, size_t obs_addr) {
    const int fl = N * C * F * F;
    return fl > 0 && fl % OBS_SPARSE_PIECE == 0 && fl / OBS_SPARSE_PIECE <= 32 * OBS_SPARSE_WORDS && (obs_addr & 63) == 0;
}
// The lane's share of an env-slot's old mask.  Lane l stores float4 l + 64k at iteration k: piece
// (l >> 2) + 16k, which is bit (k & 1) * 16 + (l >> 2) of word k >> 1.  Returned: bit j = iteration 2j,
// bit 16 + j = iteration 2j + 1.  `words` is wave-uniform and nothing in this launch has written it:
// read through the constant address space, the 16 words come by scalar loads, which wait on lgkmcnt
// and not, as a vector load would, behind the previous step's observation stores (vmcnt).
__device__ inline uint32_t obs_sparse_old(const uint32_t *words, int lane) {
    typedef const __attribute__((address_space(4))) uint32_t cu32;
    cu32 *w = (cu32 *)(uintptr_t)words;
    const int g = lane >> 2;
    uint32_t a = 0;
#pragma unroll
    for (int j = 0; j < OBS_SPARSE_WORDS; ++j) a |= ((w[j] >> g) & 0x10001u) << j;
    return a;
}
// The env-slot's new mask out of the wave's finished bit-stream (piece p = half-word p): lane l
// folds stream words [4l, 4l + 4) into 8 bits, four lanes make a word, lanes 0, 4, .. store the 16.
__device__ inline void obs_sparse_store(const uint32_t *stream, int swe, uint32_t *words, int lane) {
    uint32_t b = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = 4 * lane + i;
        const uint32_t w = idx < swe ? stream[idx] : 0u;
        b |= (((w & 0xFFFFu) ? 1u : 0u) | ((w >> 16) ? 2u : 0u)) << (2 * i);
    }
    b |= (uint32_t)__shfl_down((int)b, 1) << 8;
    b |= (uint32_t)__shfl_down((int)b, 2) << 16;
    if ((lane & 3) == 0) words[lane >> 2] = b;
}

// Phases 1-4.  Every thread of the workgroup calls it after a __syncthreads()
// that follows obs_init and the agents' staging.  skip_band: the zero band's
// whole float4s were written by obs_zero_band_store in this launch.
// BFSCH = false compiles the BFS channel (C = 7) out (the fused launch never
// has it: step_observe_fusable).  ST (OBS_*): OBS_NT, the table-driven store loop (L.lut) uses
// nontemporal stores; OBS_BITS, phase 4 writes the packed words instead of floats (`obs` is then
// the uint32 buffer; skip_band and band_mask are ignored: nothing else writes a packed buffer).  BAND: the one-wave table loop skips the stores of `band_mask`
// (bit k = this lane's iteration k, obs_band_skip_mask); BAND = 0 compiles the test out; BAND = OBS_SPARSE:
// `band_mask` is obs_sparse_old's word (all ones: store everything) and the loop stores the pieces that
// were non-zero by it or are non-zero now.  GN (with OBS_NT): OBS_NT_GROUP, the one-wave table loop runs in
// groups of that many stores (obs_store_wave_nt, below: the pair-lane kernels but PIBT's); 0, one store per trip.
// The threads that observe a run of the workgroup's envs together: the whole
// workgroup (workgroup barriers) or one wave observing its own env (per_env
// layout; wave-level ordering only).
struct ObsGroup {
    int tid, nt;                 // thread index in the group, group size
    int le0, nenv;               // first env (index within the workgroup) and env count
    uint32_t *stream;            // bit 0 = float 0 of env le0's observation
    const uint32_t *mapc;        // map rows: the shared map, or per-env maps at (le - le0) * rowsz
    bool wave;
#ifdef MAPF_STAMPS
    int diag = 0;                // stamps-build experiments: 2 no float stores, 3 stores only (no bit-stream)
#endif
};

__device__ inline void obs_sync(const ObsGroup &g) {
    if (g.wave) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

__device__ inline ObsGroup obs_workgroup(const ObsLds &L, int nenv) {
    return ObsGroup{(int)threadIdx.x, (int)blockDim.x, 0, nenv, L.stream, L.mapc, false};
}

// The map rows of env le that the wave holds in registers (lane k = word k), into its LDS copy
__device__ inline void obs_wave_map(const ObsLds &L, int le, uint32_t mreg) {
    const int lane = lane_id();
    if (lane < L.rowsz) L.mapc[le * L.rowsz + lane] = mreg;
}
// One wave observes env le of the workgroup (per_env layout): zero its stream
// and occupancy, copy the map rows.  copy_map = false: the caller stored the rows
// once before its step loop (obs_wave_map; the map does not change within a launch).
// zero16: the stream is zeroed in uint4s (swe is a multiple of 4 words and every env's
// stream starts 16-B aligned: obs_layout), a third of the word loop's trips.
__device__ inline ObsGroup obs_wave_init(const DevEnv &e, const ObsLds &L, int le, uint32_t mreg, bool copy_map = true,
                                         bool zero16 = false) {
    const int lane = lane_id();
    uint32_t *st = L.stream + (size_t)le * L.swe;
    if (zero16) {
        uint4 *st4 = reinterpret_cast<uint4 *>(st);
        for (int k = lane; k < (L.swe >> 2); k += 64) st4[k] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int k = lane; k < L.swe; k += 64) st[k] = 0u;
    }
    for (int k = lane; k < L.rowsz; k += 64) L.occ[le * L.rowsz + k] = 0u;
    uint32_t *mp = L.mapc + le * L.rowsz;
    if (copy_map) obs_wave_map(L, le, mreg);
    ObsGroup g{lane, 64, le, 1, st, mp, true};
    obs_sync(g);
    return g;
}

// ---- the one-wave table loop of phase 4 with streaming stores (obs_emit<.., OBS_NT, ..>) ----
// Lane l stores float4 l + 64k of the env's slice at iteration k (obs_emit's comment).  The slice has
// `q` float4s, a wave-uniform count, so the loop is counted in scalars and runs in groups of
// OBS_NT_GROUP iterations: the group's stream words are read first (constant LDS offsets, 32 B apart),
// then its skip tests and table reads, then its stores -- one LDS latency per kind and group instead
// of two per store.  The stores are buffer stores through a descriptor of the slice: base = the
// slice, num_records = its bytes, so the hardware's range check drops the lanes past the slice in the
// last iteration and nothing can land outside it; the lane's byte offset 16 l + 4096 g stays in one
// VGPR and the iteration's 1 KiB step is the instruction's immediate offset.  A skipped store (the
// clean band, a sparse piece of zeros over zeros) takes an offset out of range instead of a branch.
// The LDS reads are not predicated: in the last iteration the lanes past q read up to 7 words past the
// env's stream (the next env's stream or the occupancy words after it, inside the workgroup's LDS) and, in
// the sparse form, make a skip test of them.  That is harmless only because the range check drops those
// lanes' stores whatever the test says; the loop of one store per trip never touched those words.
// Cache bits sc1 nt: streamed AND not kept in the XCD's L2 (MI355X_MICROARCH: sc1 stores drop the
// line), so the lines the step outputs merge in stay resident.  A/B on one box: c2 slots 21.3 ->
// 20.3 us per step, c5 (446 MB in place) 89.1 -> 86.8 vs nt alone; plain 23.7, sc1 alone 21.0 (taken
// with the loop of one store per trip in every kernel: tools/ab_libs.sh, MAPF_SLOT_STORE in obs_emit).
constexpr int OBS_NT_GROUP = 4;                    // 4 x 1 KiB: the immediate offset's 12 bits
constexpr uint32_t OBS_NT_DROP = 0x80000000u;      // a byte offset no slice reaches (+ 3 KiB: no wrap)
constexpr int OBS_NT_AUX = 16 | 2;                 // raw buffer store's aux: sc1 (16), nt (2, the former slc)
// experiment build: MAPF_STORE_PRED=1 skips by EXEC (a branch around the store) instead
#ifndef MAPF_STORE_PRED
#define MAPF_STORE_PRED 0
#endif

// One group: iterations [0, cnt) from `swp` / `voff` on.  WHOLE: cnt == GN, known to the compiler.
// `mask`: the group's skip bits -- OBS_BAND bit j = iteration j; OBS_SPARSE obs_sparse_old's layout,
// bit (j & 1) * 16 + (j >> 1) = iteration j's old bit (0: the piece held zeros).
template <int BAND, bool WHOLE, int GN>
__device__ __forceinline__ void obs_nt_group(__amdgpu_buffer_rsrc_t rs, const float4 *lut, const uint32_t *swp, int sh,
                                             int hsh, uint32_t voff, uint32_t mask, int cnt) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    uint32_t sw[GN], vo[GN];
    float4 f[GN];
#pragma unroll
    for (int j = 0; j < GN; ++j) sw[j] = (WHOLE || j < cnt) ? swp[8 * j] : 0u;
#pragma unroll
    for (int j = 0; j < GN; ++j) {
        bool skip = false;
        if constexpr (BAND == OBS_BAND) skip = (mask >> j) & 1u;
        // the piece's 16 bits are the lane's half of the word
        if constexpr (BAND == OBS_SPARSE)
            skip = (__builtin_amdgcn_ubfe(sw[j], hsh, 16) | __builtin_amdgcn_ubfe(mask, (j & 1) * 16 + (j >> 1), 1)) == 0;
        vo[j] = skip ? OBS_NT_DROP : voff;
        // opaque: `+ 1024 j` below stays the store's immediate offset (the compiler would otherwise move
        // the addition into both arms of the select: a VALU add per store and four registers of constants)
        if constexpr (BAND != 0) asm("" : "+v"(vo[j]));
    }
#pragma unroll
    for (int j = 0; j < GN; ++j)
        if (WHOLE || j < cnt) f[j] = lut[__builtin_amdgcn_ubfe(sw[j], sh, 4)];
#pragma unroll
    for (int j = 0; j < GN; ++j) {
        if (!(WHOLE || j < cnt)) continue;
        const v4u d = {__float_as_uint(f[j].x), __float_as_uint(f[j].y), __float_as_uint(f[j].z), __float_as_uint(f[j].w)};
#if MAPF_STORE_PRED
        if (vo[j] != OBS_NT_DROP) __builtin_amdgcn_raw_buffer_store_b128(d, rs, voff + 1024u * j, 0, OBS_NT_AUX);
#else
        __builtin_amdgcn_raw_buffer_store_b128(d, rs, vo[j] + 1024u * j, 0, OBS_NT_AUX);
#endif
    }
}

// The whole slice: `dst` its first float (16-B aligned), `q` its float4s; every lane of the wave is
// active and holds the same `dst` and `q` (the wave's env).  `swp` / `sh` / `hsh`: the lane's stream
// word pointer, nibble shift and half-word shift; BAND and `band_mask` as obs_emit's.
template <int BAND, int GN>
__device__ __forceinline__ void obs_store_wave_nt(const float4 *lut, const uint32_t *swp, int sh, int hsh, float *dst, int q,
                                                  int lane, uint32_t band_mask) {
    // the descriptor out of values the compiler knows to be uniform (the env index comes from
    // threadIdx): otherwise every store is wrapped in a loop over the descriptor's values
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    q = __builtin_amdgcn_readfirstlane(q);
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uintptr_t)hi << 32) | lo), 0, q * 16, 0x00020000);
    const int iters = (q + 63) >> 6;
    uint32_t voff = (uint32_t)lane * 16u;
    static_assert(GN == OBS_NT_GROUP, "an even group (the sparse mask's layout) within the immediate offset");
    for (int g = 0; g < iters / GN; ++g) {
        obs_nt_group<BAND, true, GN>(rs, lut, swp, sh, hsh, voff, band_mask, GN);
        swp += 8 * GN;
        voff += 1024u * GN;
        band_mask >>= BAND == OBS_SPARSE ? GN / 2 : GN;
    }
    if (iters % GN) obs_nt_group<BAND, false, GN>(rs, lut, swp, sh, hsh, voff, band_mask, iters % GN);
}

// ---- phases 1-3 of obs_emit for one wave observing its own env (obs_emit<.., WV = true>: G.wave, G.nenv == 1,
// N <= 8, F <= 16, no BFS channel) ----
// The workgroup form below numbers its tasks k = tid, tid + nt, .. and divides by the run-time N and F to
// find the env, the agent and the FOV row of each: generic signed divisions, ~17 VALU instructions apiece,
// issued by the whole wave.  Here the env is G.le0 and lane l works for agent l >> 3: its FOV rows are
// (l & 7) and (l & 7) + 8 -- shifts, and at most two rows per lane for every accepted F -- and the agent's
// cell, window corner and stream offset are computed once per lane, not once per row task.  The agent's
// head lane (l & 7 == 0) does phase 1 and phase 3.  The same bits are ORed into the same stream words
// (or_bits / set_bit: atomic ORs, whose order does not matter), so the stream is the workgroup form's.
__device__ inline void obs_wave_occ(const DevEnv &e, const ObsLds &L, const ObsGroup &G, int KB) {
    const int k = G.tid >> 3;
    if ((G.tid & 7) == 0 && k < KB) {
        const uint32_t p = L.spos[G.le0 * e.N + k];
        const int r = prow(p), c = pcol(p);
        const int rr = r + e.P, cc = c + e.P;
        atomicOr(&L.occ[G.le0 * L.rowsz + rr * e.WW + (cc >> 5)], 1u << (cc & 31));
        L.idg[G.le0 * e.H * e.W + r * e.W + c] = (uint8_t)k;
    }
}

__device__ inline void obs_wave_rows(const DevEnv &e, const ObsLds &L, float *__restrict__ vec, const ObsGroup &G,
                                     int b, int KB) {
    using namespace obsd;
    const int k = G.tid >> 3, j = G.tid & 7;
    if (k >= KB) return;
    const int N = e.N, F = e.F, FF = F * F, half = F / 2;
    const int le = G.le0, kw = le * N;
    uint32_t *stream = G.stream;
    const uint32_t *occ = L.occ + le * L.rowsz;
    const uint8_t *idg = L.idg + le * e.H * e.W;
    const uint32_t p = L.spos[kw + k];
    const int pr = prow(p), pc = pcol(p);
    const int tr = pr - half, tc = pc - half;
    const int abase = k * (e.C * FF);                // the agent's block in the env's stream
    const int R2 = e.R * e.R;
    // ---- phase 2: the lane's FOV rows ----
    for (int y0 = 0; y0 < F; y0 += 8) {               // a scalar count: one trip for F <= 8, two above
        const int y = y0 + j;
        if (y >= F) continue;
        const int rr = tr + y;                       // map row of this FOV row
        const int prow_idx = rr + e.P;               // padded row (always inside)
        const uint32_t seg0 = seg_at(G.mapc + prow_idx * e.WW, e.WW, tc + e.P, F);
        const uint32_t segA = seg_at(occ + prow_idx * e.WW, e.WW, tc + e.P, F);
        const uint32_t self = (y == half) ? (1u << half) : 0u;
        const int base = abase + y * F;
        or_bits(stream, base, seg0 | self, F);
        or_bits(stream, base + FF, segA & ~self, F);
        // visibleAgents (the agents of this FOV row) -> their goals clamped to the FOV (ch3)
        for (uint32_t others = segA & ~self; others; others &= others - 1u) {
            const int cc = tc + __builtin_ctz(others);
            const uint32_t g = L.sgoal[kw + idg[rr * e.W + cc]];
            const int xr = min(max(prow(g), tr), tr + F - 1);
            const int xc = min(max(pcol(g), tc), tc + F - 1);
            set_bit(stream, abase + 3 * FF + (xr - tr) * F + (xc - tc));
        }
        if (e.use_da && rr >= 0 && rr < e.H) {      // ch4 danger area
            const uint32_t hn = L.shn[le];
            const int dy = prow(hn) - rr;
            if (dy * dy <= R2) {
                const int w = isqrt_floor(R2 - dy * dy);
                const int c0 = max(max(pcol(hn) - w, 0), tc), c1 = min(min(pcol(hn) + w, e.W - 1), tc + F - 1);
                if (c0 <= c1) or_bits(stream, base + 4 * FF, ((1u << (c1 - c0 + 1)) - 1u) << (c0 - tc), F);
            }
        }
    }
    if (j != 0) return;
    // ---- phase 3, on the agent's head lane: own goal (ch2), human next position (ch4), HP cells (ch5), vector ----
    const uint32_t gl = L.sgoal[kw + k];
    const int gr = prow(gl), gc = pcol(gl);
    if (tr <= gr && gr < tr + F && tc <= gc && gc < tc + F) set_bit(stream, abase + 2 * FF + (gr - tr) * F + (gc - tc));
    const uint32_t hn = L.shn[le];
    const int hr = prow(hn), hc = pcol(hn);
    if (tr <= hr && hr < tr + F && tc <= hc && hc < tc + F) set_bit(stream, abase + 4 * FF + (hr - tr) * F + (hc - tc));
    for (int q = 0; q < L.shpn[le]; ++q) {            // ch5: in-map cells inside the FOV
        const uint32_t cell = L.shp[le * e.k_predict + q];
        const int r = prow(cell), c = pcol(cell);
        if (tr <= r && r < tr + F && tc <= c && c < tc + F) set_bit(stream, abase + 5 * FF + (r - tr) * F + (c - tc));
    }
    // vector: obs_emit's phase 3 has the rule (float64 square root and divides, then float32)
    const int dx = gr - pr, dy = gc - pc;
    const int d2 = dx * dx + dy * dy;
    float4 v;
    if (d2 == 0) {
        v = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        const double d = __builtin_sqrt((double)d2);
        v = make_float4((float)((double)dx / d), (float)((double)dy / d), (float)d, 0.f);
    }
    reinterpret_cast<float4 *>(vec)[(size_t)b * N + k] = v;
}

// WV: the group is one wave observing one env (G.wave, G.nenv == 1) of at most 8 agents with no BFS channel:
// phases 1-3 take obs_wave_occ / obs_wave_rows above, without divisions.
template <bool BFSCH = true, int ST = OBS_PLAIN, int BAND = 0, int GN = 0, bool WV = false>
__device__ inline void obs_emit(const DevEnv &e, const ObsLds &L, float *__restrict__ obs, float *__restrict__ vec,
                                const ObsGroup &G, int b0, bool skip_band = false, uint32_t band_mask = 0) {
    using namespace obsd;
    const int N = e.N, F = e.F, C = e.C, FF = F * F, CFF = C * FF;
    const int K = G.nenv * N;                 // agents of the group; k below is group-relative
    const int kw = G.le0 * N;                 // first agent of the group within the workgroup
    const int rowsz = L.rowsz;
    const int tid = G.tid, nt = G.nt;
    uint32_t *stream = G.stream;
    b0 += G.le0;                              // first env of the group
    const int E = G.nenv;

    // ---- phase 1: worldWithAgents as a padded bitmap per env + agent index grid ----
    const int HW = e.H * e.W;
#ifdef MAPF_STAMPS
    const int KB = G.diag == 3 ? 0 : K;       // agents whose bits phases 1-3 build
#else
    const int KB = K;
#endif
    static_assert(!(WV && BFSCH), "the one-wave path has no BFS channel");
    if constexpr (WV) obs_wave_occ(e, L, G, KB);
    else
    for (int k = tid; k < KB; k += nt) {
        const int le = G.le0 + k / N;
        const int r = prow(L.spos[kw + k]), c = pcol(L.spos[kw + k]);
        const int rr = r + e.P, cc = c + e.P;
        atomicOr(&L.occ[le * rowsz + rr * e.WW + (cc >> 5)], 1u << (cc & 31));
        L.idg[le * HW + r * e.W + c] = (uint8_t)(k % N);
    }
    const int half = F / 2;
    const size_t bcells = bfs_cells(e.H, e.W);
    if (BFSCH && L.bfs_win) {
        // the BFS channel's bfsMap windows: every load of the workgroup issued here
        // at once (one HBM latency, not one per FOV-row task), as aligned dwords
        const int WD = obs_bfs_wd(e);
        for (int idx = tid; idx < KB * F * WD; idx += nt) {
            const int task = idx / WD, w = idx - task * WD;
            const int k = task / F, y = task - k * F;
            const int rr = min(max(prow(L.spos[kw + k]) - half + y, 0), e.H - 1);
            const int col = min(max(((pcol(L.spos[kw + k]) - half) & ~1) + 2 * w, 0), e.W - 2);
            const int16_t *bm = e.bfs + ((size_t)b0 * N + k) * bcells;
            L.bfsw[kw * F * WD + idx] = *reinterpret_cast<const uint32_t *>(bm + bfs_at(e.W, rr, col));   // col even
        }
        for (int k = tid; k < KB; k += nt)
            L.bfsown[kw + k] = e.bfs[((size_t)b0 * N + k) * bcells + bfs_at(e.W, prow(L.spos[kw + k]), pcol(L.spos[kw + k]))];
    }
    obs_sync(G);

    // ---- phase 2: (agent, FOV row) ----
    const int R2 = e.R * e.R;
    if constexpr (WV) obs_wave_rows(e, L, vec, G, b0, KB);      // phases 2 and 3
    else
    for (int task = tid; task < KB * F; task += nt) {
        const int k = task / F, y = task - k * F;
        const int le = G.le0 + k / N;
        const int pr = prow(L.spos[kw + k]), pc = pcol(L.spos[kw + k]);
        const int tr = pr - half, tc = pc - half;
        const int rr = tr + y;                       // map row of this FOV row
        const int prow_idx = rr + e.P;               // padded row (always inside)
        const uint32_t *mrow = G.mapc + (e.shared_map ? 0 : (le - G.le0) * rowsz) + prow_idx * e.WW;
        const uint32_t *orow = L.occ + le * rowsz + prow_idx * e.WW;
        uint32_t seg0 = seg_at(mrow, e.WW, tc + e.P, F);
        uint32_t segA = seg_at(orow, e.WW, tc + e.P, F);
        const uint32_t self = (y == half) ? (1u << half) : 0u;
        const int base = k * CFF + y * F;
        or_bits(stream, base, seg0 | self, F);
        or_bits(stream, base + FF, segA & ~self, F);
        // visibleAgents (the agents of this FOV row) -> their goals clamped to the FOV (ch3, :302-308)
        for (uint32_t others = segA & ~self; others; others &= others - 1u) {
            const int cc = tc + __builtin_ctz(others);
            const int kj = le * N + L.idg[le * HW + rr * e.W + cc];
            const int xr = min(max(prow(L.sgoal[kj]), tr), tr + F - 1);
            const int xc = min(max(pcol(L.sgoal[kj]), tc), tc + F - 1);
            set_bit(stream, k * CFF + 3 * FF + (xr - tr) * F + (xc - tc));
        }
        if (e.use_da && rr >= 0 && rr < e.H) {      // ch4 danger area (mapf_gym.py:289-290)
            const uint32_t hn = L.shn[le];
            const int dy = prow(hn) - rr;
            if (dy * dy <= R2) {
                const int w = isqrt_floor(R2 - dy * dy);
                int c0 = max(max(pcol(hn) - w, 0), tc), c1 = min(min(pcol(hn) + w, e.W - 1), tc + F - 1);
                if (c0 <= c1) {
                    const uint32_t m = ((1u << (c1 - c0 + 1)) - 1u) << (c0 - tc);
                    or_bits(stream, base + 4 * FF, m, F);
                }
            }
        }
        if (BFSCH && L.bfs_win && rr >= 0 && rr < e.H) {   // ch6 BFS descent (extension), from LDS
            const int own = L.bfsown[kw + k];
            const uint32_t *win = L.bfsw + ((size_t)kw * F + task) * obs_bfs_wd(e);
            const int c0 = tc & ~1;
            uint32_t m = 0;
            for (int x = 0; x < F; ++x) {
                const int cc = tc + x, wi = cc - c0;
                const int v = (int16_t)(win[wi >> 1] >> ((wi & 1) * 16));
                if (cc >= 0 && cc < e.W && v >= 0 && v < own) m |= 1u << x;
            }
            if (own < 0) m = 0;
            or_bits(stream, base + 6 * FF, m, F);
        } else if (BFSCH && C >= 7 && e.keep_bfs && rr >= 0 && rr < e.H) {   // ch6 BFS descent (extension)
            // the row's window straight from the tiled map: aligned dwords from column tc & ~1
            // (a dword never straddles a tile; columns past the edge read the tile padding's -1
            // or are masked), all loads issued before any is used
            const size_t ai = (size_t)b0 * N + k;
            const int16_t *bm = e.bfs + ai * bcells;
            const int own = bm[bfs_at(e.W, pr, pc)];
            const int c0 = tc & ~1, cmax = bfs_tw(e.W) * 8 - 2;
            uint32_t wv[9];
#pragma unroll
            for (int w = 0; w < 9; ++w)
                if (2 * w < F + 1)
                    wv[w] = *reinterpret_cast<const uint32_t *>(bm + bfs_at(e.W, rr, min(max(c0 + 2 * w, 0), cmax)));
            uint32_t m = 0;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int cc = tc + x, wi = cc - c0;
                if (x < F) {
                    const int v = (int16_t)(wv[wi >> 1] >> ((wi & 1) * 16));
                    if (cc >= 0 && cc < e.W && v >= 0 && v < own) m |= 1u << x;
                }
            }
            if (own < 0) m = 0;
            or_bits(stream, base + 6 * FF, m, F);
        }
    }

    // ---- phase 3: per agent: own goal (ch2), human next position (ch4), HP cells (ch5), vector ----
    if constexpr (!WV)
    for (int k = tid; k < KB; k += nt) {
        const int le = G.le0 + k / N;
        const int pr = prow(L.spos[kw + k]), pc = pcol(L.spos[kw + k]);
        const int tr = pr - half, tc = pc - half;
        const int base = k * CFF;
        const int gr = prow(L.sgoal[kw + k]), gc = pcol(L.sgoal[kw + k]);
        if (tr <= gr && gr < tr + F && tc <= gc && gc < tc + F) set_bit(stream, base + 2 * FF + (gr - tr) * F + (gc - tc));
        const uint32_t hn = L.shn[le];
        const int hr = prow(hn), hc = pcol(hn);
        if (tr <= hr && hr < tr + F && tc <= hc && hc < tc + F) set_bit(stream, base + 4 * FF + (hr - tr) * F + (hc - tc));
        for (int q = 0; q < L.shpn[le]; ++q) {         // ch5 (:293-297): in-map cells inside the FOV
            const uint32_t cell = L.shp[le * e.k_predict + q];
            const int r = prow(cell), c = pcol(cell);
            if (tr <= r && r < tr + F && tc <= c && c < tc + F) set_bit(stream, base + 5 * FF + (r - tr) * F + (c - tc));
        }
        // vector (:316-323): d = (dx^2 + dy^2) ** .5 in float64 -- the correctly
        // rounded sqrt equals Python's pow(x, .5) for every x >= 0 (no table load)
        const int dx = gr - pr, dy = gc - pc;
        const int d2 = dx * dx + dy * dy;
        float4 v;
        if (d2 == 0) {
            v = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const double d = __builtin_sqrt((double)d2);
            v = make_float4((float)((double)dx / d), (float)((double)dy / d), (float)d, 0.f);
        }
        reinterpret_cast<float4 *>(vec)[(size_t)b0 * N + k] = v;
    }
    obs_sync(G);
    TL_STAMP(4);
#ifdef MAPF_STAMPS
    if (G.diag == 2) return;
#endif

    // ---- phase 4, packed: the group's K * WPA words, agent-aligned out of the env-contiguous stream
    // (obs_bits_word), stored coalesced -- a packed slice is WPA / CFF of the float one, so a
    // float-sized write here would overrun the buffer 32 times: this branch never falls through ----
    if constexpr (ST == OBS_BITS) {
        const int WPA = obs_bits_words(C, F), nw = K * WPA;
        uint32_t *dw = reinterpret_cast<uint32_t *>(obs) + (size_t)b0 * N * WPA;
        if (((N * WPA) & 3) == 0 && ((uintptr_t)dw & 15) == 0) {     // every env's slice: whole, aligned uint4s
            for (int q = tid; q < (nw >> 2); q += nt) {
                int k = (4 * q) / WPA, w = 4 * q - k * WPA;
                uint32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = obs_bits_word(stream, CFF, k, w);
                    if (++w == WPA) { w = 0; ++k; }
                }
                reinterpret_cast<uint4 *>(dw)[q] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int i = tid; i < nw; i += nt) {
                const int k = i / WPA;
                dw[i] = obs_bits_word(stream, CFF, k, i - k * WPA);
            }
        }
        return;
    }
    // ---- phase 4: bit-stream -> float stores ----
    const size_t total = (size_t)K * CFF;
    float *dst = obs + (size_t)b0 * N * CFF;
    if (G.wave && L.lut && !skip_band && ((K * CFF) & 3) == 0) {
        // one wave, one env, whole float4s: lane l stores float4 q = l + 64k, whose 4 bits
        // are bits 4(l & 7).. of stream word (l >> 3) + 8k -- a lane-constant field (one
        // v_bfe), an 8-lane LDS broadcast -- and the float4 of that nibble comes from the
        // 16-entry LDS table L.lut: one 1 KiB store per wave instruction, constant step.
        const int sh = (tid & 7) * 4;
        const uint32_t *swp = stream + (tid >> 3);
        if constexpr (ST == OBS_NT && GN != 0) {
            obs_store_wave_nt<BAND, GN>(L.lut, swp, sh, (tid & 4) * 4, dst, (K * CFF) >> 2, tid, band_mask);
            return;
        }
        float4 *dp = reinterpret_cast<float4 *>(dst) + tid;
        [[maybe_unused]] int it = 0;          // OBS_SPARSE: the iteration
#pragma unroll 4
        for (int rem = ((K * CFF) >> 2) - tid; rem > 0; rem -= 64) {
            const uint32_t sw = *swp;
            const float4 f = L.lut[__builtin_amdgcn_ubfe(sw, sh, 4)];
            bool skip = false;
            if constexpr (BAND == OBS_BAND) skip = band_mask & 1u;
            // the piece's 16 bits are the lane's half of the word; its old bit: obs_sparse_old's layout
            if constexpr (BAND == OBS_SPARSE)
                skip = (__builtin_amdgcn_ubfe(sw, (tid & 4) * 4, 16) | __builtin_amdgcn_ubfe(band_mask, (it & 1) * 16 + (it >> 1), 1)) == 0;
            if (skip) {
                // inside the clean zero band, or a piece of zeros over zeros: nothing to store
            } else if constexpr (ST == OBS_NT) {   // streaming stores, one per trip (GN = 0: the wide and the PIBT kernels)
                // (an asm x4 store ends with s_nop 1: the compiler's next instruction may write the data registers)
                typedef float v4f __attribute__((ext_vector_type(4)));
#if defined(MAPF_SLOT_STORE) && MAPF_SLOT_STORE == 1     // store-policy experiment: nt only (round 2's)
                __builtin_nontemporal_store(v4f{f.x, f.y, f.z, f.w}, reinterpret_cast<v4f *>(dp));
#elif defined(MAPF_SLOT_STORE) && MAPF_SLOT_STORE == 2   // store-policy experiment: sc1 only
                asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dp), "v"(v4f{f.x, f.y, f.z, f.w}) : "memory");
#elif defined(MAPF_SLOT_STORE) && MAPF_SLOT_STORE == 3   // store-policy experiment: plain
                *dp = f;
#else
                // nt sc1 (obs_store_wave_nt's comment has the A/B; tools/ab_libs.sh, MAPF_SLOT_STORE: these arms
                // cover the kernels of this loop, c4 / c5 among them; the grouped loop's bits are OBS_NT_AUX)
                asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(dp), "v"(v4f{f.x, f.y, f.z, f.w}) : "memory");
#endif
            } else {
#if defined(MAPF_INPLACE_STORE) && MAPF_INPLACE_STORE == 1      // store-policy experiment: sc1
                typedef float v4f __attribute__((ext_vector_type(4)));
                asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dp), "v"(v4f{f.x, f.y, f.z, f.w}) : "memory");
#elif defined(MAPF_INPLACE_STORE) && MAPF_INPLACE_STORE == 2    // store-policy experiment: nt sc1
                typedef float v4f __attribute__((ext_vector_type(4)));
                asm volatile("global_store_dwordx4 %0, %1, off sc1 nt\n\ts_nop 1" ::"v"(dp), "v"(v4f{f.x, f.y, f.z, f.w}) : "memory");
#elif defined(MAPF_INPLACE_STORE) && MAPF_INPLACE_STORE == 3    // store-policy experiment: sc0 sc1
                typedef float v4f __attribute__((ext_vector_type(4)));
                asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(dp), "v"(v4f{f.x, f.y, f.z, f.w}) : "memory");
#else
                *dp = f;
#endif
            }
            if constexpr (BAND == OBS_BAND) band_mask >>= 1;
            if constexpr (BAND == OBS_SPARSE) ++it;
            swp += 8;
            dp += 64;
        }
    } else if (!G.wave && L.lut && !skip_band && ((E * N * CFF) & 3) == 0 && (nt & 7) == 0) {
        // the same table-driven expansion for a workgroup's stream: thread t's float4s
        // q = t + nt*k keep the bit field 4(t & 7) of words (t >> 3) + (nt / 8) k
        int tid = G.tid;
        asm volatile("" : "+v"(tid));      // opaque here: its pointers are not hoisted into the
                                           // persistent kernels' loop prologue (VGPR spills there)
        const int sh = (tid & 7) * 4;
        const uint32_t *swp = stream + (tid >> 3);
        float4 *dp = reinterpret_cast<float4 *>(dst) + tid;
        for (int rem = (int)(total >> 2) - tid; rem > 0; rem -= nt) {
            *dp = L.lut[__builtin_amdgcn_ubfe(*swp, sh, 4)];
            swp += nt >> 3;
            dp += nt;
        }
        for (size_t q = ((total >> 2) << 2) + tid; q < total; q += nt)
            dst[q] = (float)((stream[q >> 5] >> (q & 31)) & 1u);
    } else if (((E * N * CFF) & 3) == 0) {
        int tid = G.tid;
        asm volatile("" : "+v"(tid));      // (as above)
        const size_t n4 = total >> 2;
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        int z0 = 0, z1 = 0;
        if (!(skip_band && obs_zero_band(e, z0, z1))) z0 = z1 = 0;
        int off = (tid * 4) % CFF;                  // float offset of float4 q inside its agent's block
        const int step = (nt * 4) % CFF;
        for (size_t q = tid; q < n4; q += nt) {
            if (!(off >= z0 && off + 4 <= z1)) {
                const uint32_t bitpos = (uint32_t)(q << 2);
                const uint32_t nib = (stream[bitpos >> 5] >> (bitpos & 31)) & 15u;
                const float4 f = make_float4((float)(nib & 1u), (float)((nib >> 1) & 1u), (float)((nib >> 2) & 1u),
                                             (float)((nib >> 3) & 1u));
                d4[q] = f;
            }
            off += step;
            if (off >= CFF) off -= CFF;
        }
        for (size_t q = (n4 << 2) + tid; q < total; q += nt)
            dst[q] = (float)((stream[q >> 5] >> (q & 31)) & 1u);
    } else {
        int tid = G.tid;
        asm volatile("" : "+v"(tid));      // (as above)
        for (size_t q = tid; q < total; q += nt) dst[q] = (float)((stream[q >> 5] >> (q & 31)) & 1u);
    }
}

}  // namespace mapf
