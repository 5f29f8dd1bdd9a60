// primal-ppo_amd/csrc/mapf_imitation.hip -- the behaviour-cloning loss of one minibatch update as
// one kernel, forward and backward together (the supervised twin of mapf_ppo.hip).
//
// Reference: model.py:205-231 (Model.imitation_train under autocast):
//   logits          = the policy layer's output, [rows][agents][A]                       :220
//   imitation_loss  = F.cross_entropy(swapaxes(logits, 1, 2), optimal_action)             :221-222
//                   = mean_r(logsumexp(l_r) - l_r[a_r])  over R = rows x agents elements
// cross_entropy autocasts to fp32: every row is read (fp32, or fp16 bit patterns widened exactly),
// its maximum subtracted, and exp / log / the sums taken in fp32, in torch's order: the
// log-probability (x - max) - log(sum exp(x - max)), the softmax its exp.  With fp16 logits torch's
// log_softmax returns the log-probabilities in fp16 (computed in fp32, rounded once; -inf past
// -65504) before nll_loss widens them again, and its backward takes exp of the rounded values: the
// kernel rounds them at the same point, so an fp16 update sees the reference's loss and gradient.
// terms[] are statistics of the policy itself and use the unrounded softmax.  In the same pass
//   grad_logits[r][k] = (softmax(l_r)[k] - [k == a_r]) / R
//   terms[0] = mean [argmax(l_r) == a_r]   (the smallest index among the maxima)
//   terms[1] = mean softmax(l_r)[a_r]
// An action outside 0..A-1 (F.cross_entropy would raise) makes the loss NaN, as mapf_ppo_loss does.
//
// One workgroup of 1024 threads walks the rows; each thread sums its rows in fp64 and the sums
// reduce in a fixed order (deterministic).  R is small (one minibatch: 256 x 8 rows); R = 2^20 is
// 1024 rows per thread.
#include <hip/hip_fp16.h>

#include "mapf.h"
#include "mapf_common.h"

namespace mapf {
namespace imitation {

struct Args {
    const void *logits, *action;
    float *loss, *terms, *grad;
    long R;
    int A;
};

__device__ inline float r16(float x) { return __half2float(__float2half_rn(x)); }

template <bool F16>
__device__ inline float logit(const void *p, long i) {
    if constexpr (F16) return __half2float(static_cast<const __half *>(p)[i]);
    else return static_cast<const float *>(p)[i];
}

template <bool F16, bool I64>
__global__ __launch_bounds__(1024) void imitation_loss_kernel(Args a) {
    constexpr int NS = 3;              // loss, agreement, expert probability
    double s[NS] = {0.0, 0.0, 0.0};
    const float invR = 1.f / (float)a.R;
    const int A = a.A;
    int bad = 0;
    for (long r = threadIdx.x; r < a.R; r += blockDim.x) {
        const long base = r * A;
        long act64 = I64 ? static_cast<const int64_t *>(a.action)[r] : (long)static_cast<const int32_t *>(a.action)[r];
        const bool ok = act64 >= 0 && act64 < A;
        if (!ok) bad = 1;              // F.cross_entropy would raise: poison the loss instead
        const int act = ok ? (int)act64 : -1;
        float m = logit<F16>(a.logits, base);
        int am = 0;
        for (int k = 1; k < A; ++k) {
            const float x = logit<F16>(a.logits, base + k);
            if (x > m) {               // strict: the smallest index among the maxima
                m = x;
                am = k;
            }
        }
        float z = 0.f;
        for (int k = 0; k < A; ++k) z += expf(logit<F16>(a.logits, base + k) - m);
        // log_softmax as torch takes it, (x - max) - log(sum), and softmax = exp of it
        const float lz = logf(z);
        float *g = a.grad + base;
        float oa = 0.f, pa = 0.f;
        for (int k = 0; k < A; ++k) {
            const float o32 = (logit<F16>(a.logits, base + k) - m) - lz;
            // fp16 logits: torch's log_softmax hands the log-probabilities back in the logits' dtype,
            // so the loss and the gradient's softmax see them rounded to fp16 (-inf past -65504)
            const float o = F16 ? r16(o32) : o32;
            if (k == act) {
                oa = o;
                pa = expf(o32);
            }
            g[k] = (expf(o) - (k == act ? 1.f : 0.f)) * invR;
        }
        s[0] -= (double)oa;
        s[1] += am == act ? 1.0 : 0.0;
        s[2] += (double)pa;
    }
    // fixed-order reduction: waves by xor shuffles, then thread 0 over the 16 wave sums
    __shared__ double part[16][NS];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        double v = s[q];
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) part[w][q] = v;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        double t[NS];
        for (int q = 0; q < NS; ++q) {
            t[q] = 0.0;
            for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t[q] += part[i][q];
        }
        const double R = (double)a.R;
        a.loss[0] = bad ? __builtin_nanf("") : (float)(t[0] / R);
        a.terms[0] = (float)(t[1] / R);
        a.terms[1] = (float)(t[2] / R);
    }
}

}  // namespace imitation
}  // namespace mapf

using namespace mapf;

extern "C" {

int mapf_imitation_loss(const void *logits, int32_t logits_f16, const void *action, int32_t action_i64, int64_t R,
                        int32_t A, float *loss, float *terms, float *grad_logits, void *stream) {
    if (!logits || !action || !loss || !terms || !grad_logits || R < 1 || A < 2 || A > 16) return MAPF_EINVAL;
    imitation::Args a{logits, action, loss, terms, grad_logits, (long)R, (int)A};
    const hipStream_t st = (hipStream_t)stream;
    if (logits_f16 && action_i64) hipLaunchKernelGGL((imitation::imitation_loss_kernel<true, true>), dim3(1), dim3(1024), 0, st, a);
    else if (logits_f16) hipLaunchKernelGGL((imitation::imitation_loss_kernel<true, false>), dim3(1), dim3(1024), 0, st, a);
    else if (action_i64) hipLaunchKernelGGL((imitation::imitation_loss_kernel<false, true>), dim3(1), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL((imitation::imitation_loss_kernel<false, false>), dim3(1), dim3(1024), 0, st, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_EDEVICE;
}

}  // extern "C"
