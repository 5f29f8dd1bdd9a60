// primal-ppo_amd/csrc/mapf_obs_bits.hip -- mapf_unpack_obs: packed observations (mapf_obs_bits.h,
// uint32 [n][WPA]) -> the 0/1 floats a consumer without a packed reader wants, fp32 or fp16
// [n][C][F][F].
//
// A workgroup unpacks UNPACK_AGENTS consecutive agents: its indices stay 32-bit (the whole buffer
// may pass 2^31 elements: c2's 256 slots are 6.1e9), and the chunk starts on a 4-byte boundary of
// an fp16 destination whatever CFF is (an even number of agents).  Thread t writes 4-byte unit
// t + 256 i of the chunk -- one float, or two halves that may belong to two agents -- so a wave
// stores 256 contiguous bytes per instruction and dst needs 4-byte alignment only.
#include "mapf.h"
#include "mapf_common.h"
#include "mapf_obs_bits.h"

namespace mapf {

constexpr int UNPACK_AGENTS = 64;

template <bool F16>
__global__ __launch_bounds__(256) void unpack_obs_kernel(const uint32_t *__restrict__ bits, void *__restrict__ dst,
                                                        int64_t n, int CFF, int WPA) {
    const int64_t a0 = (int64_t)blockIdx.x * UNPACK_AGENTS;
    const int K = (int)min((int64_t)UNPACK_AGENTS, n - a0);
    const uint32_t *src = bits + (size_t)a0 * WPA;
    const int total = K * CFF;                                  // <= 64 * 64 * 64 * 64
    auto bit = [&](int q) {                                     // element q of the chunk
        const int k = q / CFF;
        return obs_bits_get(src + (size_t)k * WPA, q - k * CFF);
    };
    if constexpr (F16) {
        uint16_t *d = reinterpret_cast<uint16_t *>(dst) + (size_t)a0 * CFF;      // 4-byte aligned: a0 is even
        for (int u = (int)threadIdx.x; 2 * u + 1 < total; u += 256)
            reinterpret_cast<uint32_t *>(d)[u] = (bit(2 * u) ? 0x3C00u : 0u) | (bit(2 * u + 1) ? 0x3C000000u : 0u);
        if ((total & 1) && threadIdx.x == 0) d[total - 1] = bit(total - 1) ? (uint16_t)0x3C00 : (uint16_t)0;
    } else {
        float *d = reinterpret_cast<float *>(dst) + (size_t)a0 * CFF;
        for (int q = (int)threadIdx.x; q < total; q += 256) d[q] = (float)bit(q);
    }
}

}  // namespace mapf

using namespace mapf;

extern "C" int mapf_unpack_obs(const uint32_t *bits, void *dst, int64_t n_agents, int32_t C, int32_t F, int32_t dst_f16,
                               void *stream) {
    if (n_agents < 0 || C < 1 || F < 1 || C > 64 || F > 64) return MAPF_EINVAL;
    if (n_agents == 0) return MAPF_OK;                           // nothing launched
    if (!bits || !dst || ((uintptr_t)dst & 3) || ((uintptr_t)bits & 3)) return MAPF_EINVAL;
    const int64_t blocks = (n_agents + UNPACK_AGENTS - 1) / UNPACK_AGENTS;
    if (blocks > 0x7FFFFFFF) return MAPF_EINVAL;
    const int CFF = C * F * F, WPA = obs_bits_words(C, F);
    hipStream_t s = (hipStream_t)stream;
    if (dst_f16)
        hipLaunchKernelGGL(unpack_obs_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, bits, dst, n_agents, CFF, WPA);
    else
        hipLaunchKernelGGL(unpack_obs_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, bits, dst, n_agents, CFF, WPA);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_EDEVICE;
}
