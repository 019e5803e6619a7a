// wstream.h — the weight-streaming M <= 64 GEMM shared by the weight-only storage formats (gemm_fp8w.hip, gemm_mxfp4w.hip):
//   C = A · W'^T (+ residual), W' the values a format's codes stand for.
//
// A workgroup owns a band of 16 NT output columns, its four waves take the k-steps round robin (step s belongs to wave s % 4), and a lane's 16
// weight bytes of ONE weight row go straight from global memory to registers — no LDS round trip for an operand that one wave uses once — where the
// format's converter turns them into the B operands of NF 16x16x32 MFMAs.  The k-slots of a fragment are permuted (lane group g of MFMA j holds
// k = STEP / 4 * g + 8 j + 0..7 of the step); A's fragment uses the same permutation, so the products pair up.  The four partial sums meet in LDS
// and are added in wave order: ONE summation order, fixed by K alone, so a row's bits depend on that row and its codes only — not on M, the
// strides, the variant or the rows around it.  No atomics, no hand-off between workgroups.
//
// Band width.  A (at most 64 x 11008 elements, L2-resident) is re-read by every workgroup as fragment-shaped loads, and with one column tile per
// workgroup that is 2 bytes of A per byte of fp8 weights for every 16 rows of M: from two row tiles on the kernel is then bound by A, not by the
// weights.  So a lane's A fragments of a step are loaded once and multiply NT weight fragments, which divides that ratio by NT; the price is the
// workgroup count, N / (16 NT), and below one workgroup per CU the lost parallelism costs more than the A traffic saved.  The host picks the
// widest band of 1, 2, 4 column tiles (at most 2 at two row tiles, 1 at one) that leaves every CU a workgroup (wstream_band).  DESIGN.md §7 f7
// and f13 have the resource reports and the measurements.
//
// A format is a trait F that provides only what differs:
//   NAME, K_PER_QBYTE, KQ_TEXT, K_F32, SCALE_K   host: the entry point's name in messages; k per byte of q and how "K over that" is spelled; the
//                                                K granule in fp32 (the 16-bit types': STEP); k per scale of a row (0: one scale per row, no stride)
//   U[MT - 1][NT >> 1]                           k-steps in flight per wave (measured per format; 0: the band rule never names that variant)
//   STEP, NF = STEP / 32                         k per step, MFMAs per step; a lane holds STEP / 4 of them in its 16 bytes
//   scale_t, lane_scales, step_scale, NEUTRAL    the scale operand: a row's per-lane pointer, a step's scale and the value that stands in off the edge
//   frags(w, scale, bf16x8[NF])                  16 bytes -> the step's B fragments, in the 16-bit element type
//   decode(w, scale, float[STEP / 4])            ... -> fp32 values in k order (the parity kernel)
//   ROW_SCALE, row_scale(sp, n)                  whether a row scale multiplies in the epilogue, and its value
#pragma once
#include "common.h"
#include "fp8.h"                     // u32x4

constexpr int WS_BN = 16;            // output columns per column tile: one MFMA tile; a workgroup owns NT of them
constexpr int WS_WAVES = 4;          // waves per workgroup: the K split
constexpr int WS_MAX_M = 64;
constexpr int WS_MIN_WGS = 256;      // MI355X: 256 CUs

// ---- the 16-bit element types ---------------------------------------------------------------------------------------------------------------------
// MT = ceil(M / 16) row tiles, NT = column tiles per workgroup (the band is 16 NT columns), U = k-steps in flight per wave (their loads — the
// weight bytes, the scale, A's fragments — are all issued before the first conversion).  A lane's A fragments of a step are loaded once and
// multiply the NT weight fragments of the step.  `lds` is the scale operand's row stride (unused where a row has one scale).
template <class F, int MT, int NT, int U>
__global__ __launch_bounds__(64 * WS_WAVES) void wstream_linear_kernel(const bf16* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q, int64_t ldq,
                                                                       const typename F::scale_t* __restrict__ sp, int64_t lds, const bf16* residual,
                                                                       bf16* C, int64_t ldc, int M, int N, int K) {
    constexpr int NF = F::STEP / 32;
    static_assert(NF == 2 || NF == 4, "the MFMAs of a step are written out for 2 or 4 fragments");
    __shared__ f32x4 part[WS_WAVES][MT * NT][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (WS_BN * NT) + r16;                // this lane's column of column tile 0; tile c adds 16 c
    const uint8_t* qrow[NT];
    const typename F::scale_t* srow[NT];
    bool n_ok[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        n_ok[c] = n0 + 16 * c < N;
        qrow[c] = q + (int64_t)(n_ok[c] ? n0 + 16 * c : 0) * ldq + 16 * g;
        srow[c] = F::lane_scales(sp, lds, n_ok[c] ? n0 + 16 * c : 0, g);
    }
    const int steps = K >> __builtin_ctz(F::STEP);                 // K / STEP: K > 0 (checked on the host), STEP a power of two

    f32x4 acc[MT][NT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s0 = wave; s0 < steps; s0 += WS_WAVES * U) {
        u32x4 w[U][NT];
        unsigned sc[U][NT];
        u32x4 a[U][MT][NF];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int step = s0 + u * WS_WAVES;
            const bool k_ok = step < steps;
            const int kb = step * F::STEP + F::STEP / 4 * g;       // this lane's k of the step
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                w[u][c] = u32x4{0u, 0u, 0u, 0u};
                sc[u][c] = F::NEUTRAL;
                if (k_ok && n_ok[c]) {
                    w[u][c] = *reinterpret_cast<const u32x4*>(qrow[c] + (int64_t)step * 64);
                    sc[u][c] = F::step_scale(srow[c], step);
                }
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int m = t * 16 + r16;
                const bool ok = k_ok && m < M;
#pragma unroll
                for (int v = 0; v < NF; ++v) {
                    a[u][t][v] = u32x4{0u, 0u, 0u, 0u};
                    if (ok) a[u][t][v] = *reinterpret_cast<const u32x4*>(A + (int64_t)m * lda + kb + v * 8);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                bf16x8 b[NF];
                F::frags(w[u][c], sc[u][c], b);
                // (fragment by constant index, not in a loop over NF: `b` indexed by a loop variable stays an array in memory until the loop is
                // unrolled, and the conversions then end up serialised behind each other's MFMA — 1 to 3 % at NT = 1 in fp8)
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][0]), b[0], acc[t][c], 0, 0, 0);
                    acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][1]), b[1], acc[t][c], 0, 0, 0);
                    if constexpr (NF == 4) {
                        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][2]), b[2], acc[t][c], 0, 0, 0);
                        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[u][t][3]), b[3], acc[t][c], 0, 0, 0);
                    }
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
    for (int tile = wave; tile < MT * NT; tile += WS_WAVES) {
        const int t = tile / NT, c = tile % NT;
        const int n = n0 + 16 * c;
        if (n >= N) continue;
        f32x4 v = part[0][tile][lane];
#pragma unroll
        for (int w2 = 1; w2 < WS_WAVES; ++w2) v += part[w2][tile][lane];
        float rs = 1.f;
        if constexpr (F::ROW_SCALE) rs = F::row_scale(sp, n);      // once, in fp32
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // C/D layout of the 16x16 MFMAs: column = lane & 15, row = 4 * (lane >> 4) + r
            const int m = t * 16 + g * 4 + r;
            if (m < M) {
                float x = v[r];
                if constexpr (F::ROW_SCALE) x *= rs;
                if (residual) x += (float)residual[(int64_t)m * ldc + n];
                C[(int64_t)m * ldc + n] = (bf16)x;
            }
        }
    }
}

// ---- fp32 (parity mode) -----------------------------------------------------------------------------------------------------------------------------
// Plain fp32 arithmetic with the rounding errors carried along (error-free product by fma, error-free sum by Knuth's two-sum): every output is
// the fp32 value next to the exact dot product, give or take a second-order term — a short fp32 chain and a k-ordered one of another length differ
// by a few ulps either way, which no "no further from fp64 than the reference" bound survives at K = 64.  Not built for speed: wave t owns rows
// 16 t .. 16 t + 15 for the workgroup's 16 columns, lane (column, k-quarter g) walks its STEP / 4 k of every step (K is a multiple of that: they
// are inside K or all outside); the four k-quarters meet by two shuffles.  One order, fixed by K: a row's bits depend on that row and its codes only.
__device__ inline void ws_two_sum(float a, float b, float& s, float& err) {
#pragma clang fp contract(off)
    s = a + b;
    const float bp = s - a;
    err = (a - (s - bp)) + (b - bp);
}
__device__ inline void ws_add_product(float a, float b, float& hi, float& lo) {         // (hi, lo) += a * b
#pragma clang fp contract(off)
    const float p = a * b;
    const float ep = __builtin_fmaf(a, b, -p);
    float s, es;
    ws_two_sum(hi, p, s, es);
    hi = s;
    lo += es + ep;
}
__device__ inline void ws_add_pair(float bh, float bl, float& hi, float& lo) {           // (hi, lo) += (bh, bl)
#pragma clang fp contract(off)
    float s, es;
    ws_two_sum(hi, bh, s, es);
    hi = s;
    lo += es + bl;
}

template <class F>
__global__ __launch_bounds__(64 * WS_WAVES) void wstream_linear_f32_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ q,
                                                                           int64_t ldq, const typename F::scale_t* __restrict__ sp, int64_t lds,
                                                                           const float* residual, float* C, int64_t ldc, int M, int N, int K) {
    constexpr int LK = F::STEP / 4;                                // k per lane per step
    const int lane = threadIdx.x & 63, m0 = (threadIdx.x >> 6) * 16;
    const int r16 = lane & 15, g = lane >> 4;
    const int n = blockIdx.x * WS_BN + r16;
    const bool n_ok = n < N;
    const uint8_t* qrow = q + (int64_t)(n_ok ? n : 0) * ldq + 16 * g;
    const typename F::scale_t* srow = F::lane_scales(sp, lds, n_ok ? n : 0, g);
    const int steps = (K + F::STEP - 1) / F::STEP;
    float hi[16], lo[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) hi[r] = lo[r] = 0.f;
    for (int s = 0; s < steps; ++s) {
        const int kb = s * F::STEP + LK * g;                       // this lane's k of the step
        if (kb < K) {
            u32x4 w = u32x4{0u, 0u, 0u, 0u};
            unsigned sc = F::NEUTRAL;
            if (n_ok) {
                w = *reinterpret_cast<const u32x4*>(qrow + (int64_t)s * 64);
                sc = F::step_scale(srow, s);
            }
            float f[LK];
            F::decode(w, sc, f);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (m0 + r < M) {
                    const f32x4* ar = reinterpret_cast<const f32x4*>(A + (int64_t)(m0 + r) * lda + kb);
#pragma unroll
                    for (int v = 0; v < LK / 4; ++v) {
                        const f32x4 a = ar[v];
#pragma unroll
                        for (int j = 0; j < 4; ++j) ws_add_product(a[j], f[4 * v + j], hi[r], lo[r]);
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
            ws_add_pair(oh, ol, hi[r], lo[r]);
        }
    }
    if (g == 0 && n_ok) {
        float rs = 1.f;
        if constexpr (F::ROW_SCALE) rs = F::row_scale(sp, n);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + r;
            if (m < M) {
                float x = hi[r], y = lo[r];
                if constexpr (F::ROW_SCALE) { x *= rs; y *= rs; }
                float out = x + y;
                if (residual) {
                    float s2, t2;
                    ws_two_sum(x, residual[(int64_t)m * ldc + n], s2, t2);
                    out = s2 + (t2 + y);
                }
                C[(int64_t)m * ldc + n] = out;
            }
        }
    }
}

// ---- the host path ------------------------------------------------------------------------------------------------------------------------------
// The band: the widest of 1, 2, 4 column tiles (at most 2 at two row tiles, 1 at one) that still leaves `min_wgs` workgroups.  Sharing A's
// fragment among NT weight fragments divides the A bytes per weight byte by NT, but below one workgroup per CU the lost parallelism costs more
// than the A traffic saved, so the public entry points pass the CU count of the part this library is built for; the _wgs
// entry points take the floor from their caller.  U keeps 8 weight loads in flight per lane where the registers allow and the format gains.
// The choice changes which workgroup computes a column, never a bit: every (row, column) is summed over its wave's steps in step order and
// the four waves in wave order, whatever MT, NT and U are (tests/test_fp8w_bands_gpu.py and tests/test_mxfp4_gpu.py hold every variant to that).
static int wstream_band(int mt, int N, int min_wgs) {              // NT: column tiles per workgroup
    int nt = mt == 1 ? 1 : (mt == 2 ? 2 : 4);
    while (nt > 1 && cdiv(N, WS_BN * nt) < min_wgs) nt >>= 1;
    return nt;
}

template <class F>
static bool wstream_dispatch(hipStream_t s, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const typename F::scale_t* sp, int64_t lds,
                             const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    const int mt = cdiv(M, 16), nt = wstream_band(mt, N, min_wgs);
#define WS_CASE(MT, NT)                                                                                                              \
    if (mt == MT && nt == NT) {                                                                                                      \
        wstream_linear_kernel<F, MT, NT, F::U[MT - 1][NT >> 1]><<<cdiv(N, WS_BN * NT), 64 * WS_WAVES, 0, s>>>(                        \
            (const bf16*)A, lda, q, ldq, sp, lds, (const bf16*)residual, (bf16*)C, ldc, M, N, K);                                    \
        return true;                                                                                                                 \
    }
    WS_CASE(1, 1);
    WS_CASE(2, 1); WS_CASE(2, 2);
    WS_CASE(3, 1); WS_CASE(3, 2); WS_CASE(3, 4);
    WS_CASE(4, 1); WS_CASE(4, 2); WS_CASE(4, 4);
#undef WS_CASE
    return false;                                                  // a band rule that names a variant not listed above: an error, never a silent no-op
}

// what both entry points of a format are: the checks, then one launch
template <class F>
static int wstream_linear(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const typename F::scale_t* sp, int64_t lds,
                          const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs) {
    const char* name = F::NAME;
    SETOK_CHECK_ARG(A && q && sp && C, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    const int kq = dtype == SETOK_F32 ? F::K_F32 : F::STEP, vec = dtype == SETOK_F32 ? 4 : 8;
    SETOK_CHECK_ARG(M >= 1 && M <= WS_MAX_M, "%s: M=%d is outside 1..%d (dequantise and call setok_linear for more rows)", name, M, WS_MAX_M);
    SETOK_CHECK_ARG(N >= 1, "%s: N=%d must be at least 1", name, N);
    SETOK_CHECK_ARG(K >= kq && K % kq == 0, "%s: K=%d must be a positive multiple of %d", name, K, kq);
    SETOK_CHECK_ARG(lda >= K, "%s: lda=%lld < K=%d", name, (long long)lda, K);
    SETOK_CHECK_ARG(ldq >= K / F::K_PER_QBYTE, "%s: ldq=%lld < %s=%d", name, (long long)ldq, F::KQ_TEXT, K / F::K_PER_QBYTE);
    if constexpr (F::SCALE_K != 0) SETOK_CHECK_ARG(lds >= K / F::SCALE_K, "%s: lds=%lld < K/%d=%d", name, (long long)lds, F::SCALE_K, K / F::SCALE_K);
    SETOK_CHECK_ARG(ldc >= N, "%s: ldc=%lld < N=%d", name, (long long)ldc, N);
    SETOK_CHECK_ARG(lda % vec == 0, "%s: lda=%lld must be a multiple of %d (16-byte pieces of A's rows)", name, (long long)lda, vec);
    SETOK_CHECK_ARG(ldq % 16 == 0, "%s: ldq=%lld must be a multiple of 16 (16-byte pieces of q's rows)", name, (long long)ldq);
    SETOK_CHECK_ARG(aligned16(A) && aligned16(q), "%s: A and q must be 16-byte aligned", name);
    SETOK_CHECK_ARG(min_wgs >= 1, "%s: min_wgs=%d must be at least 1", name, min_wgs);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_F32) {
        wstream_linear_f32_kernel<F><<<cdiv(N, WS_BN), 64 * cdiv(M, 16), 0, s>>>((const float*)A, lda, q, ldq, sp, lds, (const float*)residual, (float*)C,
                                                                                ldc, M, N, K);
    } else {
        SETOK_CHECK_ARG(wstream_dispatch<F>(s, A, lda, q, ldq, sp, lds, residual, C, ldc, M, N, K, min_wgs),
                        "%s: no kernel variant for M=%d N=%d min_wgs=%d", name, M, N, min_wgs);
    }
    SETOK_CHECK_LAUNCH(name);
    return SETOK_OK;
}
