// primal-ppo_amd/csrc/mapf_sym.hip -- mapf_gather_rows_sym: mapf_gather_rows (mapf_minibatch.hip) with
// one of the square's eight symmetries per gathered row (mapf_sym.h), and mapf_sym_draw, the draw of
// those symmetries.
//
// Grid: mapf_gather_rows' -- per gathered row, one 256-lane workgroup per GATHER_CHUNK bytes of the
// DESTINATION row of every big array, the short arrays with the row's first workgroup.  g is the
// row's, so every branch on it is uniform over the workgroup.
//
// Observations: the destination is the large side (c3: 15.5 KB of floats per row from 512 B of bits),
// so the lanes walk the destination -- lane t owns floats 4t..4t+3 of the piece, 16 B per store, a
// wave 1 KiB contiguous -- and each finds its source cell through the inverse map, an affine function
// of the destination (i, j) whose three coefficients the workgroup derives once from sym_cell_inv.
// Packed sources: the words of the agents under the piece are staged in LDS first (coalesced loads;
// at most SYM_LDS_WORDS), the bits are then LDS reads.  Float sources: an identity row is the plain
// 16-byte copy; any other row reads the permuted index directly -- a plane is F*F*4 <= 1 KiB, so a
// wave's reads stay inside the few lines its stores cover.
#include <hip/hip_runtime.h>

#include "mapf.h"
#include "mapf_common.h"
#include "mapf_kernels.h"
#include "mapf_obs_bits.h"
#include "mapf_sym.h"

namespace mapf {
namespace symk {

// mapf_minibatch.hip's copy_piece (kept there as it is, so gather_rows_kernel builds as before)
__device__ inline void copy_piece(const char *__restrict__ src, char *__restrict__ dst, int64_t len, bool vec16) {
    if (vec16) {
        for (int64_t i = (int64_t)threadIdx.x * 16; i < len; i += 256 * 16)
            *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
    } else {
        for (int64_t i = (int64_t)threadIdx.x * 4; i < len; i += 256 * 4)
            *reinterpret_cast<uint32_t *>(dst + i) = *reinterpret_cast<const uint32_t *>(src + i);
    }
}

// the inverse map as src cell = K + A i + B j
struct CellMap {
    int K, A, B;
};
__device__ inline CellMap cell_map(int g, int F) {
    int r, c;
    sym_cell_inv(g, F, 0, 0, r, c);
    CellMap m{r * F + c, 0, 0};
    if (F > 1) {
        sym_cell_inv(g, F, 1, 0, r, c);
        m.A = r * F + c - m.K;
        sym_cell_inv(g, F, 0, 1, r, c);
        m.B = r * F + c - m.K;
    }
    return m;
}

// Floats [q0, q0 + len) of one destination row [N][C][F][F] from the row's source: BITS ? packed
// uint32 [N][WPA] : float [N][C][F][F].  Called by the whole workgroup.
template <bool BITS>
__device__ inline void obs_piece(const char *__restrict__ src_row, float *__restrict__ dst_row, int q0, int len, int g,
                                 int C, int F, bool vec16, uint32_t *lds) {
    const int FF = F * F, CFF = C * FF, WPA = obs_bits_words(C, F);
    const CellMap m = cell_map(g, F);
    const int n0 = q0 / CFF;
    if constexpr (BITS) {
        const int n1 = (q0 + len - 1) / CFF;
        const int words = (n1 - n0 + 1) * WPA;                     // <= SYM_LDS_WORDS: checked on the host
        const uint32_t *w = reinterpret_cast<const uint32_t *>(src_row) + (size_t)n0 * WPA;
        __syncthreads();                                           // the previous piece's readers are done
        for (int i = (int)threadIdx.x; i < words; i += 256) lds[i] = w[i];
        __syncthreads();
    }
    const float *fsrc = reinterpret_cast<const float *>(src_row);
    auto value = [&](int n, int ch, int i, int j) -> float {
        const int cell = ch * FF + m.K + m.A * i + m.B * j;
        if constexpr (BITS) return (float)obs_bits_get(lds + (n - n0) * WPA, cell);
        return fsrc[(size_t)n * CFF + cell];
    };
    const int per = vec16 ? 4 : 1;
    for (int q = q0 + (int)threadIdx.x * per; q < q0 + len; q += 256 * per) {
        int n = q / CFF, rem = q - n * CFF;
        int ch = rem / FF;
        rem -= ch * FF;
        int i = rem / F, j = rem - i * F;
        if (!vec16) {
            dst_row[q] = value(n, ch, i, j);
            continue;
        }
        float v[4];                                                // q % 4 == 0 and the row is whole float4s
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = value(n, ch, i, j);
            if (++j == F) {
                j = 0;
                if (++i == F) {
                    i = 0;
                    if (++ch == C) ch = 0, ++n;
                }
            }
        }
        *reinterpret_cast<float4 *>(dst_row + q) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// Units [u0, u1) of a row of per-agent records: vec float[4], action int32 / int64, columns float[5]
__device__ inline void unit_piece(int kind, const char *__restrict__ src_row, char *__restrict__ dst_row, int u0, int u1,
                                  int g) {
    for (int u = u0 + (int)threadIdx.x; u < u1; u += 256) {
        if (kind == MAPF_GATHER_VEC) {
            float v[4], o[4];
            const float *s = reinterpret_cast<const float *>(src_row) + (size_t)u * 4;
            for (int e = 0; e < 4; ++e) v[e] = s[e];
            sym_vec(g, v, o);
            float *d = reinterpret_cast<float *>(dst_row) + (size_t)u * 4;
            for (int e = 0; e < 4; ++e) d[e] = o[e];
        } else if (kind == MAPF_GATHER_ACTION32) {
            const int32_t a = reinterpret_cast<const int32_t *>(src_row)[u];
            reinterpret_cast<int32_t *>(dst_row)[u] = (int32_t)sym_action(g, a);
        } else if (kind == MAPF_GATHER_ACTION64) {
            reinterpret_cast<int64_t *>(dst_row)[u] = sym_action(g, reinterpret_cast<const int64_t *>(src_row)[u]);
        } else {
            // sym_cols' rule, stored straight to its place: a lane-private array indexed by the permuted
            // action would live in scratch or LDS
            const float *s = reinterpret_cast<const float *>(src_row) + (size_t)u * NA;
            float *d = reinterpret_cast<float *>(dst_row) + (size_t)u * NA;
#pragma unroll
            for (int e = 0; e < NA; ++e) d[(int)sym_action(g, e)] = s[e];
        }
    }
}

__host__ __device__ inline int unit_bytes(int kind) {
    return kind == MAPF_GATHER_VEC ? 16 : kind == MAPF_GATHER_ACTION32 ? 4 : kind == MAPF_GATHER_ACTION64 ? 8 : 4 * NA;
}

// bytes [off, off + len) of array k's destination row j (a unit belongs to the piece its first byte is in)
__device__ inline void piece(const SymGatherArgs &a, int k, int64_t s, int64_t j, int64_t off, int64_t len, int g,
                             uint32_t *lds) {
    const int kind = a.kind[k];
    const bool vec16 = (a.vec16 >> k) & 1u;
    const char *src_row = a.src[k] + s * a.src_row_bytes[k];
    char *dst_row = a.dst[k] + j * a.dst_row_bytes[k];
    if (kind == MAPF_GATHER_PLAIN || (kind == MAPF_GATHER_OBS_F32 && g == 0)) {
        copy_piece(src_row + off, dst_row + off, len, vec16);
    } else if (kind == MAPF_GATHER_OBS_F32) {
        obs_piece<false>(src_row, reinterpret_cast<float *>(dst_row), (int)(off >> 2), (int)(len >> 2), g, a.C, a.F, vec16, lds);
    } else if (kind == MAPF_GATHER_OBS_BITS) {
        obs_piece<true>(src_row, reinterpret_cast<float *>(dst_row), (int)(off >> 2), (int)(len >> 2), g, a.C, a.F, vec16, lds);
    } else {
        const int64_t ub = unit_bytes(kind);
        unit_piece(kind, src_row, dst_row, (int)((off + ub - 1) / ub), (int)((off + len + ub - 1) / ub), g);
    }
}

__global__ __launch_bounds__(256) void gather_rows_sym_kernel(const SymGatherArgs a) {
    __shared__ uint32_t lds[SYM_LDS_WORDS];
    const uint32_t cpr = (uint32_t)a.chunks_per_row;
    const int64_t j = blockIdx.x / cpr;
    const int c = (int)(blockIdx.x % cpr);
    const int64_t r = a.rows[j];
    const int64_t s = (r % a.T) * a.B + r / a.T;       // the row's place in a t-major [T][B] buffer
    const int g = a.sym ? (int)(a.sym[j] & 7u) : 0;
    if (c < a.chunk_begin[a.nbig]) {
        int k = 0;
        while (c >= a.chunk_begin[k + 1]) ++k;
        const int64_t rb = a.dst_row_bytes[k], off = (int64_t)(c - a.chunk_begin[k]) * GATHER_CHUNK;
        piece(a, k, s, j, off, rb - off < GATHER_CHUNK ? rb - off : GATHER_CHUNK, g, lds);
    }
    if (c == 0)
        for (int k = a.nbig; k < a.count; ++k) piece(a, k, s, j, 0, a.dst_row_bytes[k], g, lds);
}

__global__ __launch_bounds__(256) void sym_draw_kernel(uint64_t seed, uint32_t epoch, uint64_t start, uint64_t count,
                                                       uint32_t allowed, uint8_t *out) {
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < count; j += (uint64_t)gridDim.x * 256)
        out[j] = (uint8_t)sym_draw(seed, epoch, start + j, allowed);
}

}  // namespace symk

void launch_gather_rows_sym(const SymGatherArgs &a, int64_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(symk::gather_rows_sym_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
}

void launch_sym_draw(uint64_t seed, uint32_t epoch, int64_t start, int64_t count, uint32_t allowed, uint8_t *out,
                     hipStream_t s) {
    const int64_t need = (count + 255) / 256;
    hipLaunchKernelGGL(symk::sym_draw_kernel, dim3((unsigned)(need < 65536 ? need : 65536)), dim3(256), 0, s, seed, epoch,
                       (uint64_t)start, (uint64_t)count, allowed, out);
}

}  // namespace mapf
