// primal-ppo_amd/csrc/mapf_minibatch.hip -- PPO minibatches drawn from a whole device rollout:
// the epoch's permutation window (mapf_minibatch_rows) and the one-launch gather of the minibatch's
// rows from the t-major rollout buffers into the update's static inputs (mapf_gather_rows).
//
// The gather is a pure copy of a few MB (c3 minibatch: 256 rows x 15,552 B of observation plus
// eight arrays of 32..160 B per row).  Grid: per gathered row, one 256-lane workgroup per
// GATHER_CHUNK bytes of every "big" array (rows longer than GATHER_SMALL), so a long row is spread
// over several CUs; the "small" arrays ride with the row's first workgroup.  Each array moves in
// 16-byte accesses when its src, dst and row_bytes allow (bit a of vec16, set on the host), else in
// 4-byte ones.
#include <hip/hip_runtime.h>

#include "mapf.h"
#include "mapf_common.h"
#include "mapf_kernels.h"

namespace mapf {
namespace mb {

__global__ __launch_bounds__(256) void minibatch_rows_kernel(ShuffleKey key, uint64_t start, uint64_t count,
                                                             int64_t *rows) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (uint64_t)gridDim.x * 256)
        rows[j] = (int64_t)shuffle_index(key, start + j);
}

// bytes [off, off + len) of one row: 16-byte or 4-byte accesses, lane-contiguous
__device__ inline void copy_piece(const char *__restrict__ src, char *__restrict__ dst, int64_t len, bool vec16) {
    if (vec16) {
        for (int64_t i = (int64_t)threadIdx.x * 16; i < len; i += 256 * 16)
            *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    } else {
        for (int64_t i = (int64_t)threadIdx.x * 4; i < len; i += 256 * 4)
            *reinterpret_cast<uint32_t *>(dst + i) = *reinterpret_cast<const uint32_t *>(src + i);
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgs a) {
    const uint32_t cpr = (uint32_t)a.chunks_per_row;
    const int64_t j = blockIdx.x / cpr;
    const int c = (int)(blockIdx.x % cpr);
    const int64_t r = a.rows[j];
    const int64_t s = (r % a.T) * a.B + r / a.T;       // the row's place in a t-major [T][B] buffer
    if (c < a.chunk_begin[a.nbig]) {
        int k = 0;
        while (c >= a.chunk_begin[k + 1]) ++k;
        const int64_t rb = a.row_bytes[k], off = (int64_t)(c - a.chunk_begin[k]) * GATHER_CHUNK;
        const int64_t len = rb - off < GATHER_CHUNK ? rb - off : GATHER_CHUNK;
        copy_piece(a.src[k] + s * rb + off, a.dst[k] + j * rb + off, len, (a.vec16 >> k) & 1u);
    }
    if (c == 0)
        for (int k = a.nbig; k < a.count; ++k) {
            const int64_t rb = a.row_bytes[k];
            copy_piece(a.src[k] + s * rb, a.dst[k] + j * rb, rb, (a.vec16 >> k) & 1u);
        }
}

}  // namespace mb

void launch_minibatch_rows(const ShuffleKey &key, int64_t start, int64_t count, int64_t *rows, hipStream_t s) {
    const int64_t need = (count + 255) / 256;      // grid-stride beyond 65,536 workgroups
    hipLaunchKernelGGL(mb::minibatch_rows_kernel, dim3((unsigned)(need < 65536 ? need : 65536)), dim3(256), 0, s, key,
                       (uint64_t)start, (uint64_t)count, rows);
}

void launch_gather_rows(const GatherArgs &a, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(mb::gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

}  // namespace mapf
