// attn_partials.h — what the attention kernels that cut a sequence's keys into chunks share (attn_decode.hip, attn_extend.hip): every chunk leaves
// fp32 partials — per (sequence, query head, chunk) Dh + 2 floats [max, sum, Dh accumulators] — in the caller's workspace, and a second launch merges a
// query head's chunks in chunk order.  ONE definition of the merge and of the exponential both sides of it use: a partial is only meaningful to the
// merge that rescales it.
#pragma once
#include "common.h"

namespace {

// exp(x) for x <= 0: the accurate expf in fp32 (parity mode), v_exp_f32 in the 16-bit types (far below the rounding of the probability)
template <typename T> __device__ inline float dec_exp(float x) {
    if constexpr (sizeof(T) == 4) return expf(x);
    else return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
}

// ---- merge: one workgroup per (sequence, query head), the chunks in chunk order ----------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(const float* __restrict__ ws, T* __restrict__ out, int nch, int H, int Dh) {
    const int64_t bh = blockIdx.x;                                     // b * H + h; out rows are H * Dh wide
    const float* part = ws + bh * nch * (Dh + 2);
    float M = -INFINITY;
    for (int c = 0; c < nch; ++c) M = fmaxf(M, part[(int64_t)c * (Dh + 2)]);
    float L = 0.f;
    for (int c = 0; c < nch; ++c) {
        const float mc = part[(int64_t)c * (Dh + 2)];
        L = fmaf(mc == -INFINITY ? 0.f : dec_exp<T>(mc - M), part[(int64_t)c * (Dh + 2) + 1], L);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    for (int d = threadIdx.x; d < Dh; d += 64) {
        float o = 0.f;
        for (int c = 0; c < nch; ++c) {
            const float mc = part[(int64_t)c * (Dh + 2)];
            o = fmaf(mc == -INFINITY ? 0.f : dec_exp<T>(mc - M), part[(int64_t)c * (Dh + 2) + 2 + d], o);
        }
        out[bh * Dh + d] = (T)(o * inv);
    }
}

}  // namespace
