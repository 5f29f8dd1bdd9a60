// tools/store_pattern.hip -- what the c2 slot-buffer rollout's store pattern costs.
//
// The rollout kernel's wave for env b writes env b's 23 KB observation slice as 1 KiB
// store instructions (64 lanes x 16 B), 4096 waves at once, into a fresh [B] slice every
// step.  This measures that pattern against an address-interleaved one (concurrent
// instructions of the waves hit adjacent KiB) with plain and nontemporal stores, at the
// same bytes per step, in persistent launches of S steps:
//     hipcc -O3 --offload-arch=gfx950 tools/store_pattern.hip -o tools/store_pattern
//     ./tools/store_pattern [waves kib_per_wave steps in_place waves_per_workgroup]
// (default: the c2 slot pattern, 4096 23 64 0 4; c4's observer pattern in place: 1024 32 256 1 1)
//
//     ./tools/store_pattern slice [steps reps]
// writes the real c2 slice instead -- 23,232 B per wave (8 agents x 6 x 11 x 11 floats), env b at
// b * 23232, so odd envs start mid-line -- with the rollout kernel's lane mapping (lane l stores
// float4 l + 64k, k < 23), fresh slices, 4096 waves, 16 per workgroup, and leaves out the whole
// 16 / 64 / 128-B units of every agent's zero band (channel 5: bytes [2420, 2904) of each 2904-B
// agent block) with the skipped lanes predicated off; "compact 16": the 1,216 float4s that remain
// at the 16-B unit as 19 full instructions.  Each form with plain and with `sc1 nt` stores; the
// full pattern is measured in the same run (min / median / max of the repeats).
// "aligned": odd envs (slice base % 128 = 64) use lane l -> float4 l - 4 + 64k instead, lanes whose
// index falls outside [0, 1452) off, so that every instruction of every env starts on a 128-B line
// (same bytes, same 64-B pieces, same 23 instructions; fewer lines touched per instruction).
// "scatter p": every 64-B piece of a slice is left out independently with probability p (seeded; 256
// hole sets, wave w uses set w % 256), same lane mapping and predication: what a store of only the
// pieces that changed would cost.  Comparable with the band form ("skip 64-B units") of the same run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef float v4f __attribute__((ext_vector_type(4)));

// CHUNK: per-wave contiguous KiB (the env's slice); else interleaved (KiB k of wave w at
// (k * waves + w)); NT: nontemporal
template <bool CHUNK, bool NT>
__global__ __launch_bounds__(1024) void stores(float *buf, int steps, int kib_per_wave, size_t step_floats) {
    const int lane = threadIdx.x & 63;
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int waves = (gridDim.x * blockDim.x) >> 6;
    for (int s = 0; s < steps; ++s) {
        float *base = buf + (size_t)s * step_floats;
        const v4f v = {(float)s, 1.f, 0.f, 1.f};
        for (int k = 0; k < kib_per_wave; ++k) {
            const size_t kib = CHUNK ? (size_t)w * kib_per_wave + k : (size_t)k * waves + w;
            v4f *p = reinterpret_cast<v4f *>(base + kib * 256) + lane;
            if (NT) __builtin_nontemporal_store(v, p);
            else *p = v;
        }
    }
}

// ---- the c2 slice with holes ----
constexpr int AGENTS = 8, AGENT_BYTES = 6 * 11 * 11 * 4, BAND0 = 5 * 11 * 11 * 4;   // band = [BAND0, AGENT_BYTES)
constexpr int ENV_BYTES = AGENTS * AGENT_BYTES, ENV_Q = ENV_BYTES / 16, ITERS = (ENV_Q + 63) / 64;   // 23232, 1452, 23
constexpr int COMPACT_ITERS = 19;

template <bool NT>
__device__ inline void store4(v4f *p, v4f v) {
    if (NT) asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(p), "v"(v) : "memory");
    else *p = v;
}

// masks: [nvar][64] per-lane skip bits (bit k = float4 lane + 64k), set w % nvar (nvar = 2: by env parity), or null (full);
// cidx: [COMPACT_ITERS][64] float4 indices of the compacted form, or null
// aligned: odd envs shift their lane mapping down by 4 float4s (the masks are then built for that mapping)
template <bool NT>
__global__ __launch_bounds__(1024) void slice_stores(float *buf, int steps, size_t step_floats, const uint32_t *masks,
                                                     const int *cidx, int aligned, int nvar) {
    const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = (int)(threadIdx.x & 63) - (aligned ? 4 * (w & 1) : 0);
    const uint32_t mask = masks ? masks[(w % nvar) * 64 + (threadIdx.x & 63)] : 0u;   // env offset % 128 = 64 * (w & 1)
    int idx[COMPACT_ITERS];
#pragma unroll
    for (int k = 0; k < COMPACT_ITERS; ++k) idx[k] = cidx ? cidx[k * 64 + (threadIdx.x & 63)] : 0;
    for (int s = 0; s < steps; ++s) {
        v4f *base = reinterpret_cast<v4f *>(buf + (size_t)s * step_floats + (size_t)w * (ENV_BYTES / 4));
        const v4f v = {(float)s, 1.f, 0.f, 1.f};
        if (cidx) {
#pragma unroll
            for (int k = 0; k < COMPACT_ITERS; ++k) store4<NT>(base + idx[k], v);
        } else {
            uint32_t m = mask;
#pragma unroll
            for (int k = 0; k < ITERS; ++k) {
                const int q = lane + 64 * k;
                if (q >= 0 && q < ENV_Q && !(m & 1u)) store4<NT>(base + q, v);      // never outside the env's slice
                m >>= 1;
            }
        }
    }
}

// float4 q of an env slice at byte offset `off` (mod 128) is skipped iff the aligned unit around
// it lies wholly inside one agent's band
static bool skip_q(int unit, int off, int q) {
    const int o = off & (unit - 1), u0 = (o + 16 * q) & ~(unit - 1);
    if (u0 < o) return false;
    const int r0 = u0 - o, r1 = r0 + unit, k = r0 / AGENT_BYTES;
    return r0 >= k * AGENT_BYTES + BAND0 && r1 <= (k + 1) * AGENT_BYTES;
}

static int slice_mode(int steps, int reps) {
    const int waves = 4096, wpg = 16;
    const size_t step_floats = (size_t)waves * ENV_BYTES / 4;
    printf("c2 slice: %d waves x %d B, %d steps, fresh slices, %d waves per workgroup, %d repeats\n", waves, ENV_BYTES,
           steps, wpg, reps);
    float *buf = nullptr;
    if (hipMalloc(&buf, step_floats * 4 * steps) != hipSuccess) return 1;
    uint32_t *dmask = nullptr;
    int *dcidx = nullptr;
    if (hipMalloc(&dmask, 4 * 2 * 64 * 4) != hipSuccess || hipMalloc(&dcidx, COMPACT_ITERS * 64 * 4) != hipSuccess) return 1;
    const int units[3] = {16, 64, 128};
    double skipped[3] = {0, 0, 0};
    std::vector<uint32_t> hm(4 * 2 * 64, 0u);      // [3]: the 64-B unit in the aligned lane mapping
    for (int u = 0; u < 3; ++u)
        for (int par = 0; par < 2; ++par)
            for (int q = 0; q < ENV_Q; ++q)
                if (skip_q(units[u], 64 * par, q)) {
                    hm[(u * 2 + par) * 64 + (q & 63)] |= 1u << (q >> 6);
                    skipped[u] += 16.0 / 2;
                }
    for (int par = 0; par < 2; ++par)
        for (int q = 0; q < ENV_Q; ++q)
            if (skip_q(64, 64 * par, q)) {
                const int j = q + 4 * par;              // lane (j & 63) holds float4 q at iteration j >> 6
                hm[(3 * 2 + par) * 64 + (j & 63)] |= 1u << (j >> 6);
            }
    std::vector<int> hc;
    for (int q = 0; q < ENV_Q; ++q)
        if (!skip_q(16, 0, q)) hc.push_back(q);
    if ((int)hc.size() != COMPACT_ITERS * 64) return 1;
    hipMemcpy(dmask, hm.data(), hm.size() * 4, hipMemcpyHostToDevice);
    // scattered holes: piece p = float4s [4p, 4p + 4), lane l holds float4 l + 64k at bit k
    constexpr int NPROB = 3, NVAR = 256, PIECES = ENV_Q / 4;
    const double probs[NPROB] = {0.55, 0.68, 0.80};
    double sc_skipped[NPROB] = {0, 0, 0};
    uint32_t *dscat = nullptr;
    if (hipMalloc(&dscat, NPROB * NVAR * 64 * 4) != hipSuccess) return 1;
    std::vector<uint32_t> hs(NPROB * NVAR * 64, 0u);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < NPROB; ++i)
        for (int v = 0; v < NVAR; ++v)
            for (int p = 0; p < PIECES; ++p) {
                rng = rng * 6364136223846793005ull + 1442695040888963407ull;
                if ((double)(rng >> 11) * (1.0 / 9007199254740992.0) >= probs[i]) continue;
                for (int q = 4 * p; q < 4 * p + 4; ++q) hs[(i * NVAR + v) * 64 + (q & 63)] |= 1u << (q >> 6);
                sc_skipped[i] += 64.0 / NVAR;
            }
    hipMemcpy(dscat, hs.data(), hs.size() * 4, hipMemcpyHostToDevice);
    hipMemcpy(dcidx, hc.data(), hc.size() * 4, hipMemcpyHostToDevice);
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    auto run = [&](const char *name, bool nt, const uint32_t *masks, const int *cidx, double bytes_env, int aligned = 0, int nvar = 2) {
        std::vector<float> us;
        for (int r = 0; r <= reps; ++r) {
            hipEventRecord(a);
            if (nt) hipLaunchKernelGGL(slice_stores<true>, dim3(waves / wpg), dim3(64 * wpg), 0, 0, buf, steps, step_floats, masks, cidx, aligned, nvar);
            else hipLaunchKernelGGL(slice_stores<false>, dim3(waves / wpg), dim3(64 * wpg), 0, 0, buf, steps, step_floats, masks, cidx, aligned, nvar);
            hipEventRecord(b);
            hipEventSynchronize(b);
            float ms;
            hipEventElapsedTime(&ms, a, b);
            if (r > 0) us.push_back(ms * 1e3f / steps);       // the first launch is warm-up
        }
        std::sort(us.begin(), us.end());
        const double med = us[us.size() / 2];
        printf("%-22s %-6s %7.0f B/env  %6.2f / %6.2f / %6.2f us/step (min / median / max)  %6.0f GB/s\n", name,
               nt ? "sc1 nt" : "plain", bytes_env, us.front(), med, us.back(), bytes_env * waves / (med * 1e-6) / 1e9);
    };
    for (int nt = 0; nt < 2; ++nt) {
        run("full", nt, nullptr, nullptr, ENV_BYTES);
        for (int u = 0; u < 3; ++u) {
            char name[32];
            snprintf(name, sizeof name, "skip %d-B units", units[u]);
            run(name, nt, dmask + u * 2 * 64, nullptr, ENV_BYTES - skipped[u]);
        }
        run("compact 16 (19 instr)", nt, nullptr, dcidx, ENV_BYTES - skipped[0]);
        run("full, aligned", nt, nullptr, nullptr, ENV_BYTES, 1);
        run("skip 64-B, aligned", nt, dmask + 3 * 2 * 64, nullptr, ENV_BYTES - skipped[1], 1);
        run("skip 64-B units (again)", nt, dmask + 1 * 2 * 64, nullptr, ENV_BYTES - skipped[1]);
        run("full (again)", nt, nullptr, nullptr, ENV_BYTES);
        for (int i = 0; i < NPROB; ++i) {
            char name[32];
            snprintf(name, sizeof name, "scatter %.2f, 64-B", probs[i]);
            run(name, nt, dscat + i * NVAR * 64, nullptr, ENV_BYTES - sc_skipped[i], 0, NVAR);
        }
        run("skip 64-B units (3rd)", nt, dmask + 1 * 2 * 64, nullptr, ENV_BYTES - skipped[1]);
    }
    hipFree(buf);
    hipFree(dmask);
    hipFree(dcidx);
    hipFree(dscat);
    return 0;
}

#include <cstdlib>
#include <cstring>
int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "slice"))
        return slice_mode(argc > 2 ? atoi(argv[2]) : 64, argc > 3 ? atoi(argv[3]) : 7);
    // c2: 4096 envs x ~23 KiB each per step, fresh slices
    const int waves = argc > 1 ? atoi(argv[1]) : 4096, kib = argc > 2 ? atoi(argv[2]) : 23;
    const int steps = argc > 3 ? atoi(argv[3]) : 64, inplace = argc > 4 ? atoi(argv[4]) : 0;
    const int wpg = argc > 5 ? atoi(argv[5]) : 4;
    const size_t slice = (size_t)waves * kib * 256;
    const size_t step_floats = inplace ? 0 : slice;
    printf("%d waves x %d KiB, %d steps, %s, %d waves per workgroup\n", waves, kib, steps,
           inplace ? "in place" : "fresh slices", wpg);
    float *buf = nullptr;
    if (hipMalloc(&buf, slice * 4 * (inplace ? 1 : steps)) != hipSuccess) return 1;
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    auto run = [&](const char *name, auto kern) {
        hipLaunchKernelGGL(kern, dim3(waves / wpg), dim3(64 * wpg), 0, 0, buf, steps, kib, step_floats);
        hipDeviceSynchronize();
        float best = 1e30f;
        for (int r = 0; r < 5; ++r) {
            hipEventRecord(a);
            hipLaunchKernelGGL(kern, dim3(waves / wpg), dim3(64 * wpg), 0, 0, buf, steps, kib, step_floats);
            hipEventRecord(b);
            hipEventSynchronize(b);
            float ms;
            hipEventElapsedTime(&ms, a, b);
            if (ms < best) best = ms;
        }
        const double bytes = (double)slice * 4 * steps;
        printf("%-34s %7.2f us/step  %6.0f GB/s\n", name, best * 1e3 / steps, bytes / (best * 1e-3) / 1e9);
    };
    run("env chunks, plain", stores<true, false>);
    run("env chunks, nontemporal", stores<true, true>);
    run("interleaved KiB, plain", stores<false, false>);
    run("interleaved KiB, nontemporal", stores<false, true>);
    hipFree(buf);
    return 0;
}
