// primal-ppo_amd/csrc/mapf_obs_bits.h -- the bit-packed observation format (mapf.h: "Packed
// observations"), one bit per cell: an agent's [C][F][F] block of 0/1 floats as
// WPA = ceil(C*F*F / 32) little-endian uint32 words, bit k % 32 of word k / 32 = float k, the padding
// bits of the last word 0.  The functions here are the format: the kernels that write it
// (obs_emit<.., OBS_BITS>), the kernels that read it (mapf_unpack_obs, mapf_conv_first_bits) and
// the host entry points (mapf_obs_pack_host / mapf_obs_unpack_host) all evaluate them.
#pragma once
#include <cstdint>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace mapf {

__host__ __device__ inline int obs_bits_words(int C, int F) { return (C * F * F + 31) >> 5; }

// Word w of agent k's packed block, from a contiguous bit-stream in which bit k*CFF + j is float j
// of agent k (the stream the observing kernels build in LDS): bits [k*CFF + 32w, k*CFF + 32w + 32)
// through a 64-bit funnel, masked to the min(32, CFF - 32w) bits that belong to the agent.  Reads
// stream words i and i + 1, i = (k*CFF + 32w) / 32: the stream keeps one spare word after its last
// (obs_stream_words / obs_env_stream_words reserve it).  k*CFF + 32w must fit 32 bits.
__host__ __device__ inline uint32_t obs_bits_word(const uint32_t *stream, int CFF, int k, int w) {
    const uint32_t bit = (uint32_t)k * (uint32_t)CFF + 32u * (uint32_t)w;
    const uint32_t i = bit >> 5, s = bit & 31u;
    const uint64_t a = (uint64_t)stream[i] | ((uint64_t)stream[i + 1] << 32);
    const int n = CFF - 32 * w;
    return (uint32_t)(a >> s) & (n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u));
}

// float j of a packed block as a bit
__host__ __device__ inline uint32_t obs_bits_get(const uint32_t *block, int j) { return (block[j >> 5] >> (j & 31)) & 1u; }

}  // namespace mapf
