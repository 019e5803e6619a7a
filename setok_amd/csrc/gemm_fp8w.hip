// gemm_fp8w.hip — fp8 weight-only storage for the Llama projections (include/setok_hip.h, "FP8 weight-only decode"):
//   setok_quantize_fp8_rows     W (N, K) -> q (N, K) OCP e4m3fn bytes + one int8 power-of-two exponent per row
//   setok_dequantize_fp8_rows   the exact inverse, into the element type (no rounding: value(q) * 2^e is representable in bf16, fp16 and fp32)
//   setok_linear_fp8w           C = A · W'^T (+ residual) for M <= 64, W'[n, k] = value(q[n, k]) * 2^e[n]
//
// The GEMM is a weight-streaming kernel: a workgroup owns a band of 16 NT output columns, its four waves take the 64-wide k-steps round robin
// (step s belongs to wave s % 4), and a lane's 16 fp8 bytes of ONE weight row go straight from global memory to registers — no LDS round trip for
// an operand that one wave uses once — where v_cvt_pk_f32_fp8 and a pack to the element type (both exact) turn them into the B operands of two
// 16x16x32 MFMAs.  The k-slots of a fragment are permuted (lane group g of MFMA j holds k = 16 g + 8 j + 0..7 of the step); A's fragment uses the
// same permutation, so the products pair up.  The four partial sums meet in LDS and are added in wave order: ONE summation order, fixed
// by K alone, so a row's bits depend on that row, q and e only — not on M, the strides or the rows around it.  The scale 2^e[n] is applied once,
// in fp32, in the epilogue.  No atomics, no hand-off between workgroups.
//
// Band width.  A (at most 64 x 11008 elements, L2-resident) is re-read by every workgroup as fragment-shaped loads, and with one column tile per
// workgroup that is 2 bytes of A per byte of q for every 16 rows of M: from two row tiles on the kernel is then bound by A, not by the weights.
// So a lane's A fragments of a step are loaded once and multiply NT weight fragments, which divides that ratio by NT; the price is the
// workgroup count, N / (16 NT), and below one workgroup per CU the lost parallelism costs more than the A traffic saved.  The host picks the
// widest band of 1, 2, 4 column tiles (at most 2 at two row tiles, 1 at one) that leaves every CU a workgroup (fp8w_dispatch).  DESIGN.md §7 f7
// has the resource report and the measurements.
#include "common.h"
#include "fp8.h"

constexpr int FP8W_BN = 16;          // output columns per column tile: one MFMA tile; a workgroup owns NT of them
constexpr int FP8W_WAVES = 4;        // waves per workgroup: the K split
constexpr int FP8W_MAX_M = 64;
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

// ---- the M <= 64 GEMM, 16-bit element types ---------------------------------------------------------------------------------------------------------
// MT = ceil(M / 16) row tiles, NT = column tiles per workgroup (the band is 16 NT columns), U = k-steps in flight per wave (their loads are
// all issued before the first conversion).  A lane's A fragments of a step are loaded once and multiply the NT weight fragments of the step.
template <int MT, int NT, int U>
__global__ __launch_bounds__(64 * FP8W_WAVES) void fp8w_linear_kernel(const bf16* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q, int64_t ldq,
                                                                      const int8_t* __restrict__ e, const bf16* residual, bf16* C, int64_t ldc,
                                                                      int M, int N, int K) {
    __shared__ f32x4 part[FP8W_WAVES][MT * NT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (FP8W_BN * NT) + r16;              // this lane's column of column tile 0; tile c adds 16 c
    const uint8_t* qrow[NT];
    bool n_ok[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        n_ok[c] = n0 + 16 * c < N;
        qrow[c] = q + (int64_t)(n_ok[c] ? n0 + 16 * c : 0) * ldq + 16 * g;
    }
    const int steps = K >> 6;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s0 = wave; s0 < steps; s0 += FP8W_WAVES * U) {
        u32x4 w[U][NT];
        u32x4 a[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = s0 + u * FP8W_WAVES;
            const bool k_ok = step < steps;
            const int kb = step * 64 + 16 * g;                     // this lane's 16 k of the step
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                w[u][c] = u32x4{0u, 0u, 0u, 0u};
                if (k_ok && n_ok[c]) w[u][c] = *reinterpret_cast<const u32x4*>(qrow[c] + (int64_t)step * 64);
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int m = t * 16 + r16;
                const bool ok = k_ok && m < M;
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    a[u][t][v] = u32x4{0u, 0u, 0u, 0u};
                    if (ok) a[u][t][v] = *reinterpret_cast<const u32x4*>(A + (int64_t)m * lda + kb + v * 8);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                float f[16];
                fp8w_decode16(w[u][c], f);
                bf16x8 b0, b1;
#pragma unroll
                for (int j = 0; j < 8; ++j) { b0[j] = (bf16)f[j]; b1[j] = (bf16)f[8 + j]; }
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][0]), b0, acc[t][c], 0, 0, 0);
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][1]), b1, acc[t][c], 0, 0, 0);
                }
            }
        }
    }

    // merge in wave order: the MT * NT output tiles are dealt to the waves round robin
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < NT; ++c) part[wave][t * NT + c][lane] = acc[t][c];
    __syncthreads();
    for (int tile = wave; tile < MT * NT; tile += FP8W_WAVES) {
        const int t = tile / NT, c = tile % NT;
        const int n = n0 + 16 * c;
        if (n >= N) continue;
        f32x4 v = part[0][tile][lane];
#pragma unroll
        for (int w2 = 1; w2 < FP8W_WAVES; ++w2) v += part[w2][tile][lane];
        const float sc = fp8w_scale(e[n]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // C/D layout of the 16x16 MFMAs: column = lane & 15, row = 4 * (lane >> 4) + r
            const int m = t * 16 + g * 4 + r;
            if (m < M) {
                float x = v[r] * sc;
                if (residual) x += (float)residual[(int64_t)m * ldc + n];
                C[(int64_t)m * ldc + n] = (bf16)x;
            }
        }
    }
}

template <int MT, int NT, int U>
static void fp8w_launch(hipStream_t s, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e, const void* residual, void* C,
                        int64_t ldc, int M, int N, int K) {
    fp8w_linear_kernel<MT, NT, U><<<cdiv(N, FP8W_BN * NT), 64 * FP8W_WAVES, 0, s>>>((const bf16*)A, lda, q, ldq, e, (const bf16*)residual, (bf16*)C, ldc, M, N, K);
}

// The band: the widest of 1, 2, 4 column tiles (at most 2 at two row tiles, 1 at one) that still leaves `min_wgs` workgroups.  Sharing A's
// fragment among NT weight fragments divides the A bytes per q byte by NT, but below one workgroup per CU the lost parallelism costs more than
// the A traffic saved, so setok_linear_fp8w passes the CU count of the part this library is built for; setok_linear_fp8w_wgs
// takes the floor from its caller.  U keeps 8 weight loads in flight per lane where the registers allow.
// The choice changes which workgroup computes a column, never a bit: every (row, column) is summed over its wave's steps in step order and
// the four waves in wave order, whatever MT, NT and U are (tests/test_fp8w_bands_gpu.py holds every variant to that).
constexpr int FP8W_MIN_WGS = 256;                                  // MI355X: 256 CUs
static int fp8w_band(int mt, int N, int min_wgs) {                 // NT: column tiles per workgroup
    int nt = mt == 1 ? 1 : (mt == 2 ? 2 : 4);
    while (nt > 1 && cdiv(N, FP8W_BN * nt) < min_wgs) nt >>= 1;
    return nt;
}
static bool fp8w_dispatch(hipStream_t s, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e, const void* residual, void* C,
                          int64_t ldc, int M, int N, int K, int min_wgs) {
    const int mt = cdiv(M, 16), nt = fp8w_band(mt, N, min_wgs);
#define FP8W_CASE(MT, NT, U) if (mt == MT && nt == NT) { fp8w_launch<MT, NT, U>(s, A, lda, q, ldq, e, residual, C, ldc, M, N, K); return true; }
    FP8W_CASE(1, 1, 8);
    FP8W_CASE(2, 1, 8); FP8W_CASE(2, 2, 4);
    FP8W_CASE(3, 1, 4); FP8W_CASE(3, 2, 4); FP8W_CASE(3, 4, 2);
    FP8W_CASE(4, 1, 4); FP8W_CASE(4, 2, 4); FP8W_CASE(4, 4, 2);
#undef FP8W_CASE
    return false;                                                  // a band rule that names a variant not listed above: an error, never a silent no-op
}

// ---- the M <= 64 GEMM, fp32 (parity mode) -------------------------------------------------------------------------------------------------------------
// Plain fp32 arithmetic with the rounding errors carried along (error-free product by fma, error-free sum by Knuth's two-sum): every output is
// the fp32 value next to the exact dot product, give or take a second-order term — a short fp32 chain and a k-ordered one of another length differ
// by a few ulps either way, which no "no further from fp64 than the reference" bound survives at K = 64.  Not built for speed: wave t owns rows
// 16 t .. 16 t + 15 for the workgroup's 16 columns, lane (column, k-quarter) walks every 64-wide step; the four k-quarters meet by two shuffles.
// One order, fixed by K: a row's bits depend on that row, q and e only.
__device__ inline void fp8w_two_sum(float a, float b, float& s, float& err) {
#pragma clang fp contract(off)
    s = a + b;
    const float bp = s - a;
    err = (a - (s - bp)) + (b - bp);
}
__device__ inline void fp8w_add_product(float a, float b, float& hi, float& lo) {       // (hi, lo) += a * b
#pragma clang fp contract(off)
    const float p = a * b;
    const float ep = __builtin_fmaf(a, b, -p);
    float s, es;
    fp8w_two_sum(hi, p, s, es);
    hi = s;
    lo += es + ep;
}
__device__ inline void fp8w_add_pair(float bh, float bl, float& hi, float& lo) {         // (hi, lo) += (bh, bl)
#pragma clang fp contract(off)
    float s, es;
    fp8w_two_sum(hi, bh, s, es);
    hi = s;
    lo += es + bl;
}

__global__ __launch_bounds__(64 * FP8W_WAVES) void fp8w_linear_f32_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q,
                                                                          int64_t ldq, const int8_t* __restrict__ e, const float* residual, float* C,
                                                                          int64_t ldc, int M, int N, int K) {
    const int lane = threadIdx.x & 63, m0 = (threadIdx.x >> 6) * 16;
    const int r16 = lane & 15, g = lane >> 4;
    const int n = blockIdx.x * FP8W_BN + r16;
    const bool n_ok = n < N;
    const uint8_t* qrow = q + (int64_t)(n_ok ? n : 0) * ldq + 16 * g;
    const int steps = (K + 63) >> 6;
    float hi[16], lo[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[r] = lo[r] = 0.f;
    for (int s = 0; s < steps; ++s) {
        const int kb = s * 64 + 16 * g;                            // this lane's 16 k of the step; K % 16 == 0: inside K or all outside
        if (kb < K) {
            u32x4 w = u32x4{0u, 0u, 0u, 0u};
            if (n_ok) w = *reinterpret_cast<const u32x4*>(qrow + (int64_t)s * 64);
            float f[16];
            fp8w_decode16(w, f);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (m0 + r < M) {
                    const f32x4* ar = reinterpret_cast<const f32x4*>(A + (int64_t)(m0 + r) * lda + kb);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const f32x4 a = ar[v];
#pragma unroll
                        for (int j = 0; j < 4; ++j) fp8w_add_product(a[j], f[4 * v + j], hi[r], lo[r]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float oh = __shfl_xor(hi[r], off, 64), ol = __shfl_xor(lo[r], off, 64);
            fp8w_add_pair(oh, ol, hi[r], lo[r]);
        }
    }
    if (g == 0 && n_ok) {
        const float sc = fp8w_scale(e[n]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + r;
            if (m < M) {
                const float x = hi[r] * sc, y = lo[r] * sc;
                float out = x + y;
                if (residual) {
                    float s2, t2;
                    fp8w_two_sum(x, residual[(int64_t)m * ldc + n], s2, t2);
                    out = s2 + (t2 + y);
                }
                C[(int64_t)m * ldc + n] = out;
            }
        }
    }
}

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

static int fp8w_linear(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                       const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    SETOK_CHECK_ARG(A && q && e && C, "setok_linear_fp8w: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_linear_fp8w: bad dtype %d", dtype);
    const int kq = dtype == SETOK_F32 ? 16 : 64, vec = dtype == SETOK_F32 ? 4 : 8;
    SETOK_CHECK_ARG(M >= 1 && M <= FP8W_MAX_M, "setok_linear_fp8w: M=%d is outside 1..%d (dequantise and call setok_linear for more rows)", M, FP8W_MAX_M);
    SETOK_CHECK_ARG(N >= 1, "setok_linear_fp8w: N=%d must be at least 1", N);
    SETOK_CHECK_ARG(K >= kq && K % kq == 0, "setok_linear_fp8w: K=%d must be a positive multiple of %d", K, kq);
    SETOK_CHECK_ARG(lda >= K, "setok_linear_fp8w: lda=%lld < K=%d", (long long)lda, K);
    SETOK_CHECK_ARG(ldq >= K, "setok_linear_fp8w: ldq=%lld < K=%d", (long long)ldq, K);
    SETOK_CHECK_ARG(ldc >= N, "setok_linear_fp8w: ldc=%lld < N=%d", (long long)ldc, N);
    SETOK_CHECK_ARG(lda % vec == 0, "setok_linear_fp8w: lda=%lld must be a multiple of %d (16-byte pieces of A's rows)", (long long)lda, vec);
    SETOK_CHECK_ARG(ldq % 16 == 0, "setok_linear_fp8w: ldq=%lld must be a multiple of 16 (16-byte pieces of q's rows)", (long long)ldq);
    SETOK_CHECK_ARG(aligned16(A) && aligned16(q), "setok_linear_fp8w: A and q must be 16-byte aligned");
    SETOK_CHECK_ARG(min_wgs >= 1, "setok_linear_fp8w: min_wgs=%d must be at least 1", min_wgs);
    hipStream_t s = (hipStream_t)stream;
    bool launched = true;
    DISPATCH_T("setok_linear_fp8w", (launched = fp8w_dispatch(s, A, lda, q, ldq, e, residual, C, ldc, M, N, K, min_wgs)),
               (fp8w_linear_f32_kernel<<<cdiv(N, FP8W_BN), 64 * cdiv(M, 16), 0, s>>>((const float*)A, lda, q, ldq, e, (const float*)residual, (float*)C, ldc, M, N, K)));
    SETOK_CHECK_ARG(launched, "setok_linear_fp8w: no kernel variant for M=%d N=%d min_wgs=%d", M, N, min_wgs);
    SETOK_CHECK_LAUNCH("setok_linear_fp8w");
    return SETOK_OK;
}

extern "C" int setok_linear_fp8w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                                 const void* residual, void* C, int64_t ldc, int M, int N, int K) {
    return fp8w_linear(stream, dtype, A, lda, q, ldq, e, residual, C, ldc, M, N, K, FP8W_MIN_WGS);
}

extern "C" int setok_linear_fp8w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                                     const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    return fp8w_linear(stream, dtype, A, lda, q, ldq, e, residual, C, ldc, M, N, K, min_wgs);
}
