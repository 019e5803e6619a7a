// gemm_mxfp4w.hip — OCP MXFP4 weight-only storage for the Llama projections (include/setok_hip.h, "MXFP4 weight-only decode"):
//   setok_quantize_mxfp4_rows     W (N, K) -> q (N, K/2) bytes of two e2m1 nibbles + s (N, K/32) e8m0 scale bytes, one per 32 elements of a row
//   setok_dequantize_mxfp4_rows   the exact inverse, into the element type (no rounding: value(nibble) * 2^(s-127) is representable in bf16, fp16, fp32)
//   setok_linear_mxfp4w           C = A · W'^T (+ residual) for M <= 64, W'[n, k] = value(nibble[n, k]) * 2^(s[n, k/32] - 127)
//
// The GEMM is gemm_fp8w.hip's weight-streaming kernel at half the bytes: a workgroup owns a band of 16 NT output columns, its four waves take the
// 128-wide k-steps round robin (step s belongs to wave s % 4), and a lane's 16 bytes are exactly ONE MX block of ONE weight row — lane (column r,
// group g) holds block 4 step + g of row n0 + r.  v_cvt_scalef32_pk_{bf16,f16}_fp4 turns the block, together with its scale, into 32 exact
// element-type values: dword j of the load is the B operand of MFMA j of the step, so lane group g of MFMA j holds k = 128 step + 32 g + 8 j + 0..7,
// and A's fragment uses the same permutation (a lane's four A fragments of a step are 64 contiguous bytes of one row of A).  The scale differs from
// block to block of a row, so it is applied at conversion, never in the epilogue.  The four partial sums meet in LDS and are added in wave order:
// ONE summation order, fixed by K alone, so a row's bits depend on that row, q and s only — not on M, the strides, the variant or the rows around it.
// No atomics, no hand-off between workgroups.  The band rule is fp8w's (the widest of 1, 2, 4 column tiles that leaves every CU a workgroup).
// DESIGN.md §7 f13 has the resource report and the measurements.
#include "common.h"
#include "fp8.h"                     // u32x4

constexpr int MX4_BN = 16;           // output columns per column tile: one MFMA tile; a workgroup owns NT of them
constexpr int MX4_WAVES = 4;         // waves per workgroup: the K split
constexpr int MX4_MAX_M = 64;
constexpr int MX4_STEP = 128;        // k per step of the 16-bit kernel: 4 lane groups x one 32-element block

#ifdef SETOK_HALF
#define MX4_CVT_PK16 __builtin_amdgcn_cvt_scalef32_pk_f16_fp4
#else
#define MX4_CVT_PK16 __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4
#endif

// The converter's scale operand: an fp32 whose exponent field IS the e8m0 byte.  0xFF (the block is NaN) also sets a mantissa bit, so the operand
// is a NaN both as e8m0 and as fp32.
__device__ inline float mx4_scale(unsigned s) { return __builtin_bit_cast(float, (s << 23) | (s == 0xffu ? 0x400000u : 0u)); }

// the 8 values of one dword (elements 0..7: byte b holds element 2b in its low nibble, 2b + 1 in its high one), scaled, in the 16-bit element type
__device__ inline bf16x8 mx4_frag(unsigned w, float sc) {
    const bf16x2 p0 = MX4_CVT_PK16(w, sc, 0), p1 = MX4_CVT_PK16(w, sc, 1), p2 = MX4_CVT_PK16(w, sc, 2), p3 = MX4_CVT_PK16(w, sc, 3);
    return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
// ... and in fp32
__device__ inline void mx4_f32x8(unsigned w, float sc, float* f) {
    const auto p0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 0), p1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 1);
    const auto p2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 2), p3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc, 3);
    f[0] = p0[0]; f[1] = p0[1]; f[2] = p1[0]; f[3] = p1[1]; f[4] = p2[0]; f[5] = p2[1]; f[6] = p3[0]; f[7] = p3[1];
}

// round-to-nearest, ties to the even code, to e2m1 (0, 0.5, 1, 1.5, 2, 3, 4, 6), saturating at +-6; v is finite.  The sign bit is v's own.
__device__ inline unsigned mx4_encode(float v) {
    const unsigned sign = (__builtin_bit_cast(unsigned, v) >> 28) & 0x8u;
    const float a = fabsf(v);
    const unsigned code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
    return sign | code;
}

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
    int e = 0;                                                     // floor(log2(amax)) - 2 by exponent arithmetic (an fp32 subnormal reads as -127: clamped); 0 for zeros
    if (finite && amax > 0.f) {
        e = (int)(__builtin_bit_cast(unsigned, amax) >> 23) - 127 - 2;
        e = e < -13 ? -13 : (e > 13 ? 13 : e);
    }
    const float inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);      // 2^-e exactly
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

// ---- the M <= 64 GEMM, 16-bit element types ---------------------------------------------------------------------------------------------------------
// MT = ceil(M / 16) row tiles, NT = column tiles per workgroup (the band is 16 NT columns), U = k-steps in flight per wave (their loads — the
// block, its scale byte, A's fragments — are all issued before the first conversion).  A lane's A fragments of a step are loaded once and multiply
// the NT weight blocks of the step.
template <int MT, int NT, int U>
__global__ __launch_bounds__(64 * MX4_WAVES) void mx4_linear_kernel(const bf16* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q, int64_t ldq,
                                                                    const uint8_t* __restrict__ sb, int64_t lds, const bf16* residual, bf16* C,
                                                                    int64_t ldc, int M, int N, int K) {
    __shared__ f32x4 part[MX4_WAVES][MT * NT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (MX4_BN * NT) + r16;               // this lane's column of column tile 0; tile c adds 16 c
    const uint8_t* qrow[NT];
    const uint8_t* srow[NT];
    bool n_ok[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        n_ok[c] = n0 + 16 * c < N;
        qrow[c] = q + (int64_t)(n_ok[c] ? n0 + 16 * c : 0) * ldq + 16 * g;
        srow[c] = sb + (int64_t)(n_ok[c] ? n0 + 16 * c : 0) * lds + g;
    }
    const int steps = K / MX4_STEP;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s0 = wave; s0 < steps; s0 += MX4_WAVES * U) {
        u32x4 w[U][NT];
        unsigned sc[U][NT];
        u32x4 a[U][MT][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = s0 + u * MX4_WAVES;
            const bool k_ok = step < steps;
            const int kb = step * MX4_STEP + 32 * g;               // this lane's 32 k of the step
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                w[u][c] = u32x4{0u, 0u, 0u, 0u};
                sc[u][c] = 127u;
                if (k_ok && n_ok[c]) {
                    w[u][c] = *reinterpret_cast<const u32x4*>(qrow[c] + (int64_t)step * 64);
                    sc[u][c] = srow[c][step * 4];
                }
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int m = t * 16 + r16;
                const bool ok = k_ok && m < M;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    a[u][t][v] = u32x4{0u, 0u, 0u, 0u};
                    if (ok) a[u][t][v] = *reinterpret_cast<const u32x4*>(A + (int64_t)m * lda + kb + v * 8);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const float scale = mx4_scale(sc[u][c]);
                const bf16x8 b0 = mx4_frag(w[u][c][0], scale), b1 = mx4_frag(w[u][c][1], scale);
                const bf16x8 b2 = mx4_frag(w[u][c][2], scale), b3 = mx4_frag(w[u][c][3], scale);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][0]), b0, acc[t][c], 0, 0, 0);
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][1]), b1, acc[t][c], 0, 0, 0);
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][2]), b2, acc[t][c], 0, 0, 0);
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][3]), b3, acc[t][c], 0, 0, 0);
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
    for (int tile = wave; tile < MT * NT; tile += MX4_WAVES) {
        const int t = tile / NT, c = tile % NT;
        const int n = n0 + 16 * c;
        if (n >= N) continue;
        f32x4 v = part[0][tile][lane];
#pragma unroll
        for (int w2 = 1; w2 < MX4_WAVES; ++w2) v += part[w2][tile][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // C/D layout of the 16x16 MFMAs: column = lane & 15, row = 4 * (lane >> 4) + r
            const int m = t * 16 + g * 4 + r;
            if (m < M) {
                float x = v[r];
                if (residual) x += (float)residual[(int64_t)m * ldc + n];
                C[(int64_t)m * ldc + n] = (bf16)x;
            }
        }
    }
}

template <int MT, int NT, int U>
static void mx4_launch(hipStream_t s, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* sb, int64_t lds, const void* residual,
                       void* C, int64_t ldc, int M, int N, int K) {
    mx4_linear_kernel<MT, NT, U><<<cdiv(N, MX4_BN * NT), 64 * MX4_WAVES, 0, s>>>((const bf16*)A, lda, q, ldq, sb, lds, (const bf16*)residual, (bf16*)C, ldc, M, N, K);
}

// The band: fp8w's rule — the widest of 1, 2, 4 column tiles (at most 2 at two row tiles, 1 at one) that still leaves `min_wgs` workgroups.
// U: a step of this kernel carries twice the k of an fp8w step in the same 16 weight bytes, so A's fragments take twice the registers per step.
// Measured at the four 7B shapes: one row tile is fastest with 8 steps in flight, two with 4; from three row tiles on the
// A fragments bound the kernel, and one step in flight at two to five waves per SIMD beats two steps at one or two.  The choice changes which workgroup computes a column, never a bit:
// every (row, column) is summed over its wave's steps in step order and the four waves in wave order, whatever MT, NT and U are.
constexpr int MX4_MIN_WGS = 256;                                   // MI355X: 256 CUs
static int mx4_band(int mt, int N, int min_wgs) {                  // NT: column tiles per workgroup
    int nt = mt == 1 ? 1 : (mt == 2 ? 2 : 4);
    while (nt > 1 && cdiv(N, MX4_BN * nt) < min_wgs) nt >>= 1;
    return nt;
}
static bool mx4_dispatch(hipStream_t s, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* sb, int64_t lds, const void* residual,
                         void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    const int mt = cdiv(M, 16), nt = mx4_band(mt, N, min_wgs);
#define MX4_CASE(MT, NT, U) if (mt == MT && nt == NT) { mx4_launch<MT, NT, U>(s, A, lda, q, ldq, sb, lds, residual, C, ldc, M, N, K); return true; }
    MX4_CASE(1, 1, 8);
    MX4_CASE(2, 1, 4); MX4_CASE(2, 2, 4);
    MX4_CASE(3, 1, 1); MX4_CASE(3, 2, 1); MX4_CASE(3, 4, 1);
    MX4_CASE(4, 1, 1); MX4_CASE(4, 2, 1); MX4_CASE(4, 4, 1);
#undef MX4_CASE
    return false;                                                  // a band rule that names a variant not listed above: an error, never a silent no-op
}

// ---- the M <= 64 GEMM, fp32 (parity mode) -------------------------------------------------------------------------------------------------------------
// fp8w_linear_f32_kernel's compensated arithmetic (error-free product by fma, error-free sum by two-sum) for the reason DESIGN.md §7 f7 gives: every
// output is the fp32 value next to the exact dot product.  Wave t owns rows 16 t .. 16 t + 15 for the workgroup's 16 columns, lane (column,
// k-quarter g) walks block 4 step + g of every 128-wide step (K % 32 == 0: a block is inside K or all outside); the four k-quarters meet by two
// shuffles.  One order, fixed by K: a row's bits depend on that row, q and s only.
__device__ inline void mx4_two_sum(float a, float b, float& s, float& err) {
#pragma clang fp contract(off)
    s = a + b;
    const float bp = s - a;
    err = (a - (s - bp)) + (b - bp);
}
__device__ inline void mx4_add_product(float a, float b, float& hi, float& lo) {        // (hi, lo) += a * b
#pragma clang fp contract(off)
    const float p = a * b;
    const float ep = __builtin_fmaf(a, b, -p);
    float s, es;
    mx4_two_sum(hi, p, s, es);
    hi = s;
    lo += es + ep;
}
__device__ inline void mx4_add_pair(float bh, float bl, float& hi, float& lo) {          // (hi, lo) += (bh, bl)
#pragma clang fp contract(off)
    float s, es;
    mx4_two_sum(hi, bh, s, es);
    hi = s;
    lo += es + bl;
}

__global__ __launch_bounds__(64 * MX4_WAVES) void mx4_linear_f32_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q,
                                                                        int64_t ldq, const uint8_t* __restrict__ sb, int64_t lds, const float* residual,
                                                                        float* C, int64_t ldc, int M, int N, int K) {
    const int lane = threadIdx.x & 63, m0 = (threadIdx.x >> 6) * 16;
    const int r16 = lane & 15, g = lane >> 4;
    const int n = blockIdx.x * MX4_BN + r16;
    const bool n_ok = n < N;
    const uint8_t* qrow = q + (int64_t)(n_ok ? n : 0) * ldq + 16 * g;
    const uint8_t* srow = sb + (int64_t)(n_ok ? n : 0) * lds + g;
    const int steps = (K + MX4_STEP - 1) / MX4_STEP;
    float hi[16], lo[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[r] = lo[r] = 0.f;
    for (int s = 0; s < steps; ++s) {
        const int kb = s * MX4_STEP + 32 * g;                      // this lane's block of the step
        if (kb < K) {
            u32x4 w = u32x4{0u, 0u, 0u, 0u};
            unsigned sc = 127u;
            if (n_ok) {
                w = *reinterpret_cast<const u32x4*>(qrow + (int64_t)s * 64);
                sc = srow[s * 4];
            }
            const float scale = mx4_scale(sc);
            float f[32];
            mx4_f32x8(w[0], scale, f); mx4_f32x8(w[1], scale, f + 8); mx4_f32x8(w[2], scale, f + 16); mx4_f32x8(w[3], scale, f + 24);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (m0 + r < M) {
                    const f32x4* ar = reinterpret_cast<const f32x4*>(A + (int64_t)(m0 + r) * lda + kb);
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const f32x4 a = ar[v];
#pragma unroll
                        for (int j = 0; j < 4; ++j) mx4_add_product(a[j], f[4 * v + j], hi[r], lo[r]);
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
            mx4_add_pair(oh, ol, hi[r], lo[r]);
        }
    }
    if (g == 0 && n_ok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + r;
            if (m < M) {
                const float x = hi[r], y = lo[r];
                float out = x + y;
                if (residual) {
                    float s2, t2;
                    mx4_two_sum(x, residual[(int64_t)m * ldc + n], s2, t2);
                    out = s2 + (t2 + y);
                }
                C[(int64_t)m * ldc + n] = out;
            }
        }
    }
}

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

static int mx4_linear(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                      const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    SETOK_CHECK_ARG(A && q && s && C, "setok_linear_mxfp4w: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_linear_mxfp4w: bad dtype %d", dtype);
    const int kq = dtype == SETOK_F32 ? 32 : MX4_STEP, vec = dtype == SETOK_F32 ? 4 : 8;
    SETOK_CHECK_ARG(M >= 1 && M <= MX4_MAX_M, "setok_linear_mxfp4w: M=%d is outside 1..%d (dequantise and call setok_linear for more rows)", M, MX4_MAX_M);
    SETOK_CHECK_ARG(N >= 1, "setok_linear_mxfp4w: N=%d must be at least 1", N);
    SETOK_CHECK_ARG(K >= kq && K % kq == 0, "setok_linear_mxfp4w: K=%d must be a positive multiple of %d", K, kq);
    SETOK_CHECK_ARG(lda >= K, "setok_linear_mxfp4w: lda=%lld < K=%d", (long long)lda, K);
    SETOK_CHECK_ARG(ldq >= K / 2, "setok_linear_mxfp4w: ldq=%lld < K/2=%d", (long long)ldq, K / 2);
    SETOK_CHECK_ARG(lds >= K / 32, "setok_linear_mxfp4w: lds=%lld < K/32=%d", (long long)lds, K / 32);
    SETOK_CHECK_ARG(ldc >= N, "setok_linear_mxfp4w: ldc=%lld < N=%d", (long long)ldc, N);
    SETOK_CHECK_ARG(lda % vec == 0, "setok_linear_mxfp4w: lda=%lld must be a multiple of %d (16-byte pieces of A's rows)", (long long)lda, vec);
    SETOK_CHECK_ARG(ldq % 16 == 0, "setok_linear_mxfp4w: ldq=%lld must be a multiple of 16 (16-byte pieces of q's rows)", (long long)ldq);
    SETOK_CHECK_ARG(aligned16(A) && aligned16(q), "setok_linear_mxfp4w: A and q must be 16-byte aligned");
    SETOK_CHECK_ARG(min_wgs >= 1, "setok_linear_mxfp4w: min_wgs=%d must be at least 1", min_wgs);
    hipStream_t st = (hipStream_t)stream;
    bool launched = true;
    DISPATCH_T("setok_linear_mxfp4w", (launched = mx4_dispatch(st, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K, min_wgs)),
               (mx4_linear_f32_kernel<<<cdiv(N, MX4_BN), 64 * cdiv(M, 16), 0, st>>>((const float*)A, lda, q, ldq, s, lds, (const float*)residual, (float*)C, ldc, M, N, K)));
    SETOK_CHECK_ARG(launched, "setok_linear_mxfp4w: no kernel variant for M=%d N=%d min_wgs=%d", M, N, min_wgs);
    SETOK_CHECK_LAUNCH("setok_linear_mxfp4w");
    return SETOK_OK;
}

extern "C" int setok_linear_mxfp4w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                                   const void* residual, void* C, int64_t ldc, int M, int N, int K) {
    return mx4_linear(stream, dtype, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K, MX4_MIN_WGS);
}

extern "C" int setok_linear_mxfp4w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                                       const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    return mx4_linear(stream, dtype, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K, min_wgs);
}
