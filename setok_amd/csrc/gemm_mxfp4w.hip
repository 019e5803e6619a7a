// gemm_mxfp4w.hip — OCP MXFP4 weight-only storage for the Llama projections (include/setok_hip.h, "MXFP4 weight-only decode"):
//   setok_quantize_mxfp4_rows     W (N, K) -> q (N, K/2) bytes of two e2m1 nibbles + s (N, K/32) e8m0 scale bytes, one per 32 elements of a row
//   setok_dequantize_mxfp4_rows   the exact inverse, into the element type (no rounding: value(nibble) * 2^(s-127) is representable in bf16, fp16, fp32)
//   setok_linear_mxfp4w           C = A · W'^T (+ residual) for M <= 64, W'[n, k] = value(nibble[n, k]) * 2^(s[n, k/32] - 127)
//
// The GEMM is the weight-streaming kernel of wstream.h (the band of 16 NT columns, the k-steps dealt to four waves, the merge in wave order, the
// band rule, the checks) at half fp8's bytes; this file holds what is MXFP4's own: the quantiser and its inverse, and the format trait.  A step is
// 128 k, and a lane's 16 bytes are exactly ONE MX block of ONE weight row — lane (column r, group g) holds block 4 step + g of row n0 + r.
// v_cvt_scalef32_pk_{bf16,f16}_fp4 turns the block, together with its scale, into 32 exact element-type values: dword j of the load is the B
// operand of MFMA j of the step, so lane group g of MFMA j holds k = 128 step + 32 g + 8 j + 0..7, and A's fragment uses the same permutation (a
// lane's four A fragments of a step are 64 contiguous bytes of one row of A).  The scale differs from block to block of a row, so it is applied at
// conversion, never in the epilogue.  DESIGN.md §7 f13 has the resource report and the measurements.
#include "common.h"
#include "wstream.h"
#include "mx4.h"

// ---- the quantiser: one thread per 32-element block, the block in registers, no atomics ---------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mx4_quantize_kernel(const T* __restrict__ W, int64_t ldw, uint8_t* __restrict__ q, int64_t ldq,
                                                           uint8_t* __restrict__ s, int64_t lds, int K) {
    const int n = blockIdx.x, b = blockIdx.y * 256 + threadIdx.x;
    if (b >= (K >> 5)) return;
    const T* w = W + (int64_t)n * ldw + 32 * b;
    float v[32];
    float amax = 0.f;
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        v[j] = Elem<T>::ld(w + j);
        const float a = fabsf(v[j]);
        if (!(a <= 3.402823466e38f)) finite = false;
        amax = fmaxf(amax, a);
    }
    const int e = finite ? mx4_exponent(amax) : 0;                 // (mx4.h: the rule)
    const float inv = mx4_inv_scale(e);
    uint8_t* o = q + (int64_t)n * ldq + 16 * b;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned lo = finite ? mx4_encode(v[2 * j] * inv) : 0u, hi = finite ? mx4_encode(v[2 * j + 1] * inv) : 0u;
        o[j] = (uint8_t)(lo | (hi << 4));
    }
    s[(int64_t)n * lds + b] = (uint8_t)(finite ? 127 + e : 0xff);
}

// packed: 4 bytes of q (8 elements, inside one block) per lane and 16-byte stores; otherwise one byte (2 elements) per lane.  The same
// converter with the same scale operand either way: the same bits.
template <typename T>
__global__ __launch_bounds__(256) void mx4_dequantize_kernel(const uint8_t* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ s, int64_t lds,
                                                             T* __restrict__ W, int64_t ldw, int K, bool packed) {
    const int n = blockIdx.x;
    const uint8_t* src = q + (int64_t)n * ldq;
    const uint8_t* srow = s + (int64_t)n * lds;
    T* dst = W + (int64_t)n * ldw;
    if (packed) {
        for (int i = blockIdx.y * 256 + threadIdx.x; i < (K >> 3); i += 256 * gridDim.y) {
            const unsigned u = *reinterpret_cast<const unsigned*>(src + 4 * i);
            const float sc = mx4_scale(srow[i >> 2]);
            if constexpr (sizeof(T) == 4) {
                float f[8];
                mx4_f32x8(u, sc, f);
                *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{f[4], f[5], f[6], f[7]};
            } else {
                *reinterpret_cast<bf16x8*>(dst + 8 * i) = mx4_frag(u, sc);
            }
        }
    } else {
        for (int i = blockIdx.y * 256 + threadIdx.x; i < (K >> 1); i += 256 * gridDim.y) {
            const unsigned u = src[i];
            const float sc = mx4_scale(srow[i >> 4]);
            if constexpr (sizeof(T) == 4) {
                const auto p = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(u, sc, 0);
                dst[2 * i] = p[0]; dst[2 * i + 1] = p[1];
            } else {
                const bf16x2 p = MX4_CVT_PK16(u, sc, 0);
                dst[2 * i] = p[0]; dst[2 * i + 1] = p[1];
            }
        }
    }
}

// ---- the format of the M <= 64 GEMM (wstream.h) -----------------------------------------------------------------------------------------------
// U: a step carries twice the k of an fp8 step in the same 16 weight bytes, so A's fragments take twice the registers per step.  Measured at the
// four 7B shapes: one row tile is fastest with 8 steps in flight, two with 4; from three row tiles on the A fragments bound
// the kernel, and one step in flight at two to five waves per SIMD beats two steps at one or two.
struct Mx4Format {
    static constexpr const char* NAME = "setok_linear_mxfp4w";
    static constexpr int K_PER_QBYTE = 2, K_F32 = 32, SCALE_K = 32;
    static constexpr const char* KQ_TEXT = "K/2";
    static constexpr int U[4][3] = {{8, 0, 0}, {4, 4, 0}, {1, 1, 1}, {1, 1, 1}};           // [MT - 1][NT >> 1]
    static constexpr int STEP = 128;                                                        // 4 lane groups x one 32-element block
    typedef uint8_t scale_t;
    static constexpr unsigned NEUTRAL = 127u;                                               // 2^0
    static constexpr bool ROW_SCALE = false;
    __device__ static const scale_t* lane_scales(const scale_t* s, int64_t lds, int n, int g) { return s + (int64_t)n * lds + g; }
    __device__ static unsigned step_scale(const scale_t* srow, int step) { return srow[step * 4]; }
    __device__ static void decode(const u32x4& w, unsigned sc, float* f) {
        const float scale = mx4_scale(sc);
        mx4_f32x8(w[0], scale, f); mx4_f32x8(w[1], scale, f + 8); mx4_f32x8(w[2], scale, f + 16); mx4_f32x8(w[3], scale, f + 24);
    }
    __device__ static void frags(const u32x4& w, unsigned sc, bf16x8* b) {
        const float scale = mx4_scale(sc);
        b[0] = mx4_frag(w[0], scale); b[1] = mx4_frag(w[1], scale); b[2] = mx4_frag(w[2], scale); b[3] = mx4_frag(w[3], scale);
    }
};

// ---- entry points -------------------------------------------------------------------------------------------------------------------------------
#define MX4_CHECK_ROWS(NAME)                                                                                                                       \
    SETOK_CHECK_ARG(W && q && s, NAME ": null operand");                                                                                           \
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, NAME ": bad dtype %d", dtype);                                                      \
    SETOK_CHECK_ARG(N >= 0 && K >= 32 && K % 32 == 0, NAME ": bad shape N=%d K=%d (K must be a positive multiple of 32, the MX block)", N, K);     \
    SETOK_CHECK_ARG(ldw >= K, NAME ": ldw=%lld < K=%d", (long long)ldw, K);                                                                        \
    SETOK_CHECK_ARG(ldq >= K / 2, NAME ": ldq=%lld < K/2=%d", (long long)ldq, K / 2);                                                              \
    SETOK_CHECK_ARG(lds >= K / 32, NAME ": lds=%lld < K/32=%d", (long long)lds, K / 32)

extern "C" int setok_quantize_mxfp4_rows(void* stream, int dtype, const void* W, int64_t ldw, uint8_t* q, int64_t ldq, uint8_t* s, int64_t lds,
                                         int N, int K) {
    MX4_CHECK_ROWS("setok_quantize_mxfp4_rows");
    if (N == 0) return SETOK_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(N, (unsigned)cdiv(K / 32, 256));
    DISPATCH_T("setok_quantize_mxfp4_rows", (mx4_quantize_kernel<bf16><<<grid, 256, 0, st>>>((const bf16*)W, ldw, q, ldq, s, lds, K)),
               (mx4_quantize_kernel<float><<<grid, 256, 0, st>>>((const float*)W, ldw, q, ldq, s, lds, K)));
    SETOK_CHECK_LAUNCH("setok_quantize_mxfp4_rows");
    return SETOK_OK;
}

extern "C" int setok_dequantize_mxfp4_rows(void* stream, int dtype, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds, void* W, int64_t ldw,
                                           int N, int K) {
    MX4_CHECK_ROWS("setok_dequantize_mxfp4_rows");
    if (N == 0) return SETOK_OK;
    hipStream_t st = (hipStream_t)stream;
    const int vec = dtype == SETOK_F32 ? 4 : 8;                    // elements per 16-byte store
    const bool packed = ldq % 4 == 0 && ((uintptr_t)q & 3u) == 0 && ldw % vec == 0 && aligned16(W);
    const int items = packed ? K / 8 : K / 2;
    const dim3 grid(N, (unsigned)(cdiv(items, 1024) < 8 ? cdiv(items, 1024) : 8));
    DISPATCH_T("setok_dequantize_mxfp4_rows", (mx4_dequantize_kernel<bf16><<<grid, 256, 0, st>>>(q, ldq, s, lds, (bf16*)W, ldw, K, packed)),
               (mx4_dequantize_kernel<float><<<grid, 256, 0, st>>>(q, ldq, s, lds, (float*)W, ldw, K, packed)));
    SETOK_CHECK_LAUNCH("setok_dequantize_mxfp4_rows");
    return SETOK_OK;
}

extern "C" int setok_linear_mxfp4w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                                   const void* residual, void* C, int64_t ldc, int M, int N, int K) {
    return wstream_linear<Mx4Format>(stream, dtype, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K, WS_MIN_WGS);
}

extern "C" int setok_linear_mxfp4w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                                       const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    return wstream_linear<Mx4Format>(stream, dtype, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K, min_wgs);
}
