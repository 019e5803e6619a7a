// gemm_fp8w.hip — fp8 weight-only storage for the Llama projections (include/setok_hip.h, "FP8 weight-only decode"):
//   setok_quantize_fp8_rows     W (N, K) -> q (N, K) OCP e4m3fn bytes + one int8 power-of-two exponent per row
//   setok_dequantize_fp8_rows   the exact inverse, into the element type (no rounding: value(q) * 2^e is representable in bf16, fp16 and fp32)
//   setok_linear_fp8w           C = A · W'^T (+ residual) for M <= 64, W'[n, k] = value(q[n, k]) * 2^e[n]
//
// The GEMM is the weight-streaming kernel of wstream.h (the band of 16 NT columns, the k-steps dealt to four waves, the merge in wave order, the
// band rule, the checks); this file holds what is fp8's own: the quantiser and its inverse, and the format trait — a step is 64 k, a lane's 16
// bytes are 16 e4m3fn codes that v_cvt_pk_f32_fp8 and a pack to the element type (both exact) turn into the B operands of two MFMAs, and the
// scale 2^e[n] is applied once, in fp32, in the epilogue.  DESIGN.md §7 f7 has the resource report and the measurements.
#include "common.h"
#include "fp8.h"
#include "wstream.h"
// (e4m3fn <-> fp32 and the row-exponent rule: fp8.h, shared with the fp8 KV cache of attn_decode.hip)

// ---- the quantiser: one workgroup per row, two passes, no atomics ------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void fp8w_quantize_kernel(const T* __restrict__ W, int64_t ldw, uint8_t* __restrict__ q, int64_t ldq,
                                                            int8_t* __restrict__ e, int K) {
    __shared__ float red[4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const T* w = W + (int64_t)n * ldw;
    float amax = 0.f;                                              // over the finite entries; a non-finite one becomes the NaN code below
    for (int k = tid; k < K; k += 256) {
        const float a = fabsf(Elem<T>::ld(w + k));
        if (a <= 3.402823466e38f) amax = fmaxf(amax, a);
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) red[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const int ex = fp8w_exponent(amax);                            // the smallest e with amax <= 448 * 2^e, clamped; 0 for a row of zeros
    if (tid == 0) e[n] = (int8_t)ex;
    const float inv = fp8w_scale(-ex);
    uint8_t* o = q + (int64_t)n * ldq;
    for (int k = tid; k < K; k += 256) {
        const float v = Elem<T>::ld(w + k);
        o[k] = (uint8_t)(fabsf(v) <= 3.402823466e38f ? fp8w_encode(v * inv) : 0x7fu);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void fp8w_dequantize_kernel(const uint8_t* __restrict__ q, int64_t ldq, const int8_t* __restrict__ e,
                                                              T* __restrict__ W, int64_t ldw, int K, bool quads) {
    const int n = blockIdx.x;
    const float sc = fp8w_scale(e[n]);
    const uint8_t* src = q + (int64_t)n * ldq;
    T* dst = W + (int64_t)n * ldw;
    if (quads) {                                                   // K % 4 == 0 and 4-element aligned rows on both sides: four bytes per lane
        for (int k = 4 * (blockIdx.y * 256 + threadIdx.x); k < K; k += 4 * 256 * gridDim.y) {
            const unsigned u = *reinterpret_cast<const unsigned*>(src + k);
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, false);
            const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)u, true);
            if constexpr (sizeof(T) == 4) {
                f32x4 v = {lo[0] * sc, lo[1] * sc, hi[0] * sc, hi[1] * sc};
                *reinterpret_cast<f32x4*>(dst + k) = v;
            } else {
                bf16x4 v = {(bf16)(lo[0] * sc), (bf16)(lo[1] * sc), (bf16)(hi[0] * sc), (bf16)(hi[1] * sc)};
                *reinterpret_cast<bf16x4*>(dst + k) = v;
            }
        }
    } else {
        for (int k = blockIdx.y * 256 + threadIdx.x; k < K; k += 256 * gridDim.y) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)src[k], false);
            Elem<T>::st(dst + k, lo[0] * sc);
        }
    }
}

// ---- the format of the M <= 64 GEMM (wstream.h) -----------------------------------------------------------------------------------------------
struct Fp8wFormat {
    static constexpr const char* NAME = "setok_linear_fp8w";
    static constexpr int K_PER_QBYTE = 1, K_F32 = 16, SCALE_K = 0;                          // one exponent per row: no scale stride
    static constexpr const char* KQ_TEXT = "K";
    static constexpr int U[4][3] = {{8, 0, 0}, {8, 4, 0}, {4, 4, 2}, {4, 4, 2}};           // [MT - 1][NT >> 1]: 8 weight loads in flight per lane where the registers allow
    static constexpr int STEP = 64;
    typedef int8_t scale_t;
    static constexpr unsigned NEUTRAL = 0u;                                                 // (no per-step scale: nothing is loaded)
    static constexpr bool ROW_SCALE = true;
    __device__ static const scale_t* lane_scales(const scale_t* e, int64_t, int, int) { return e; }
    __device__ static unsigned step_scale(const scale_t*, int) { return NEUTRAL; }
    __device__ static float row_scale(const scale_t* e, int n) { return fp8w_scale(e[n]); }
    __device__ static void decode(const u32x4& w, unsigned, float* f) { fp8w_decode16(w, f); }
    __device__ static void frags(const u32x4& w, unsigned, bf16x8* b) {
        float f[16];
        fp8w_decode16(w, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) { b[0][j] = (bf16)f[j]; b[1][j] = (bf16)f[8 + j]; }
    }
};

// ---- entry points -------------------------------------------------------------------------------------------------------------------------------
extern "C" int setok_quantize_fp8_rows(void* stream, int dtype, const void* W, int64_t ldw, uint8_t* q, int64_t ldq, int8_t* e, int N, int K) {
    SETOK_CHECK_ARG(W && q && e, "setok_quantize_fp8_rows: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_quantize_fp8_rows: bad dtype %d", dtype);
    SETOK_CHECK_ARG(N >= 0 && K >= 1, "setok_quantize_fp8_rows: bad shape N=%d K=%d", N, K);
    SETOK_CHECK_ARG(ldw >= K, "setok_quantize_fp8_rows: ldw=%lld < K=%d", (long long)ldw, K);
    SETOK_CHECK_ARG(ldq >= K, "setok_quantize_fp8_rows: ldq=%lld < K=%d", (long long)ldq, K);
    if (N == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T("setok_quantize_fp8_rows", (fp8w_quantize_kernel<bf16><<<N, 256, 0, s>>>((const bf16*)W, ldw, q, ldq, e, K)),
               (fp8w_quantize_kernel<float><<<N, 256, 0, s>>>((const float*)W, ldw, q, ldq, e, K)));
    SETOK_CHECK_LAUNCH("setok_quantize_fp8_rows");
    return SETOK_OK;
}

extern "C" int setok_dequantize_fp8_rows(void* stream, int dtype, const uint8_t* q, int64_t ldq, const int8_t* e, void* W, int64_t ldw, int N, int K) {
    SETOK_CHECK_ARG(W && q && e, "setok_dequantize_fp8_rows: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_dequantize_fp8_rows: bad dtype %d", dtype);
    SETOK_CHECK_ARG(N >= 0 && K >= 1, "setok_dequantize_fp8_rows: bad shape N=%d K=%d", N, K);
    SETOK_CHECK_ARG(ldw >= K, "setok_dequantize_fp8_rows: ldw=%lld < K=%d", (long long)ldw, K);
    SETOK_CHECK_ARG(ldq >= K, "setok_dequantize_fp8_rows: ldq=%lld < K=%d", (long long)ldq, K);
    if (N == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int esz = dtype == SETOK_F32 ? 4 : 2;
    const bool quads = K % 4 == 0 && ldq % 4 == 0 && ldw % 4 == 0 && ((uintptr_t)q & 3u) == 0 && ((uintptr_t)W & (uintptr_t)(4 * esz - 1)) == 0;
    const dim3 grid(N, (unsigned)(cdiv(K, 4096) < 8 ? cdiv(K, 4096) : 8));
    DISPATCH_T("setok_dequantize_fp8_rows", (fp8w_dequantize_kernel<bf16><<<grid, 256, 0, s>>>(q, ldq, e, (bf16*)W, ldw, K, quads)),
               (fp8w_dequantize_kernel<float><<<grid, 256, 0, s>>>(q, ldq, e, (float*)W, ldw, K, quads)));
    SETOK_CHECK_LAUNCH("setok_dequantize_fp8_rows");
    return SETOK_OK;
}

extern "C" int setok_linear_fp8w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                                 const void* residual, void* C, int64_t ldc, int M, int N, int K) {
    return wstream_linear<Fp8wFormat>(stream, dtype, A, lda, q, ldq, e, 0, residual, C, ldc, M, N, K, WS_MIN_WGS);
}

extern "C" int setok_linear_fp8w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                                     const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    return wstream_linear<Fp8wFormat>(stream, dtype, A, lda, q, ldq, e, 0, residual, C, ldc, M, N, K, min_wgs);
}
