// gemm_skinny.hip — C[M, N] = alpha * A[M, K] · W[N, K]^T for a NARROW output (N <= SETOK_SKINNY_MAX_N): the GEMMs of a LoRA adapter, whose
// one small dimension is the rank r.  (include/setok_hip.h: setok_linear_skinny.)
//
// An (M x r) output gives the tiled kernels of gemm.hip / gemm_persist.hip cdiv(M, 128) workgroups that each walk the whole K.  Here K is cut
// into slices of SETOK_SKINNY_KSLICE columns counted from column 0 and the grid is (row blocks, slices): every workgroup writes the fp32 partial
// of its rows over its slice to the caller's workspace, and a second launch sums a row's partials in slice order, multiplies by alpha and
// rounds once.  No atomics, no hand-off between workgroups; the slicing is a rule in K alone, so a row's bits depend on that row of A, W, K
// and alpha — not on M, the strides or the rows around it.
//
//  * 16-bit path: a workgroup of 4 waves owns 128 rows, a wave 32 of them across all of N (NT tiles of v_mfma_f32_32x32x16, fp32 accumulate).
//    W's slice goes through LDS, N x 64 columns per K step (<= 32 KB, double-buffered, the 16-byte-slot XOR swizzle of gemm.hip); A's rows are
//    streamed from global memory straight into MFMA fragments (a lane holds 8 consecutive k of row lane & 31), one K step ahead.
//  * fp32 path (parity mode): one thread per (row, column, slice), a plain k-ordered fmaf chain.  Not fast.
#include "common.h"

constexpr int SK_BM = 128, SK_BK = 64;

__device__ inline int sk_lds_off(int row, int chunk) {        // byte offset of a 16-byte chunk (8 elements) of a 128-byte LDS row
    return row * (SK_BK * 2) + ((chunk ^ (row & 7)) << 4);
}

struct SkinnyArgs {
    const void* A; const void* W; float* ws;
    int64_t lda, ldw;
    int M, N, K;
};

// NT: 32-column MFMA tiles per wave; 32 * NT >= N.  W rows >= N are read as row N - 1 and their columns never stored.
template <int NT>
__global__ __launch_bounds__(256) void skinny_bf16_kernel(SkinnyArgs g) {
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];
    constexpr int STAGE = NT * 32 * SK_BK * 2;                 // one W tile: (32 NT) rows x 64 columns

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * SK_BM + wave * 32;
    const int slice = blockIdx.y;
    const int k_begin = slice * SETOK_SKINNY_KSLICE;
    const int k_end = min(g.K, k_begin + SETOK_SKINNY_KSLICE);
    const int nk = (k_end - k_begin) / SK_BK;
    const bf16* A = (const bf16*)g.A;
    const bf16* W = (const bf16*)g.W;

    // W staging map: chunk c = tid + 256 p -> row = c >> 3, 16-byte piece = c & 7
    const bf16* w_src[NT]; int st_off[NT];
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int c = tid + 256 * p, row = c >> 3, kc = c & 7;
        w_src[p] = W + (int64_t)min(row, g.N - 1) * g.ldw + k_begin + kc * 8;
        st_off[p] = sk_lds_off(row, kc);
    }
    // this lane's A fragment source: row m0 + (lane & 31) (clamped: rows >= M are computed and dropped), k-group lane >> 5
    const bf16* a_src = A + (int64_t)min(m0 + (lane & 31), g.M - 1) * g.lda + k_begin + (lane >> 5) * 8;

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // registers of the NEXT K step: W's pieces on their way to LDS, A's fragments.  The step after the last one re-reads the last (in range) and
    // its LDS store lands in the buffer nobody reads any more: no branch around the loads.
    uint4 rw[NT]; bf16x8 ra[4];
#pragma unroll
    for (int p = 0; p < NT; ++p) rw[p] = *reinterpret_cast<const uint4*>(w_src[p]);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ra[ks] = *reinterpret_cast<const bf16x8*>(a_src + ks * 16);
#pragma unroll
    for (int p = 0; p < NT; ++p) *reinterpret_cast<uint4*>(sk_smem + st_off[p]) = rw[p];
    __syncthreads();

    const int frow = lane & 31, fk = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        const char* Wb = sk_smem + buf * STAGE;
        const int kn = min(kt + 1, nk - 1) * SK_BK;
        bf16x8 af[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) af[ks] = ra[ks];
#pragma unroll
        for (int p = 0; p < NT; ++p) rw[p] = *reinterpret_cast<const uint4*>(w_src[p] + kn);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) ra[ks] = *reinterpret_cast<const bf16x8*>(a_src + kn + ks * 16);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const bf16x8 wf = *reinterpret_cast<const bf16x8*>(Wb + sk_lds_off(j * 32 + frow, ks * 2 + fk));
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], wf, acc[j], 0, 0, 0);
            }
#pragma unroll
        for (int p = 0; p < NT; ++p) *reinterpret_cast<uint4*>(sk_smem + (buf ^ 1) * STAGE + st_off[p]) = rw[p];
        __syncthreads();
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    float* P = g.ws + (int64_t)slice * g.M * g.N;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = j * 32 + (lane & 31);
        if (col >= g.N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < g.M) P[(int64_t)row * g.N + col] = acc[j][r];
        }
    }
}

// fp32 parity mode: one (row, column) per thread, the slice's products in ascending k
__global__ __launch_bounds__(256) void skinny_f32_kernel(SkinnyArgs g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)g.M * g.N) return;
    const int row = (int)(e / g.N), col = (int)(e % g.N);
    const int slice = blockIdx.y;
    const int k_begin = slice * SETOK_SKINNY_KSLICE, k_end = min(g.K, k_begin + SETOK_SKINNY_KSLICE);
    const float* a = (const float*)g.A + (int64_t)row * g.lda;
    const float* w = (const float*)g.W + (int64_t)col * g.ldw;
    float acc = 0.f;
    for (int k = k_begin; k < k_end; ++k) acc = fmaf(a[k], w[k], acc);
    g.ws[(int64_t)slice * g.M * g.N + e] = acc;
}

// C[row, 4 c .. 4 c + 3] = round(alpha * (partial 0 + partial 1 + ...)): slice order, alpha once in fp32, one rounding
template <typename TO>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* ws, TO* C, int64_t ldc, int M, int N, int slices, float alpha) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;         // one group of 4 columns
    const int nq = N >> 2;
    if (q >= (int64_t)M * nq) return;
    const int row = (int)(q / nq), col = (int)(q % nq) * 4;
    const int64_t MN = (int64_t)M * N;
    const float* p = ws + (int64_t)row * N + col;
    f32x4 s = *reinterpret_cast<const f32x4*>(p);
    for (int i = 1; i < slices; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + i * MN);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2]; s[3] += v[3];
    }
    TO* o = C + (int64_t)row * ldc + col;
    if constexpr (sizeof(TO) == 4) {
        f32x4 v = {s[0] * alpha, s[1] * alpha, s[2] * alpha, s[3] * alpha};
        *reinterpret_cast<f32x4*>(o) = v;
    } else {
        bf16x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (bf16)(s[i] * alpha);
        *reinterpret_cast<bf16x4*>(o) = v;
    }
}

extern "C" int64_t setok_linear_skinny_workspace(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (int64_t)((K + SETOK_SKINNY_KSLICE - 1) / SETOK_SKINNY_KSLICE) * M * N;
}

template <int NT>
static bool skinny_launch_bf16(hipStream_t s, const SkinnyArgs& g, dim3 grid) {
    constexpr int lds = 2 * NT * 32 * SK_BK * 2;               // <= 64 KB at NT = 8
    static SetokDeviceOnce once;
    if (!once.run([&] { return hipFuncSetAttribute((const void*)skinny_bf16_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess; }))
        return false;
    skinny_bf16_kernel<NT><<<grid, 256, lds, s>>>(g);
    return true;
}

extern "C" int setok_linear_skinny(void* stream, int dtype, int out_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C,
                                   int64_t ldc, int M, int N, int K, float alpha, float* ws, int64_t ws_floats) {
    SETOK_CHECK_ARG(A && W && C, "setok_linear_skinny: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_linear_skinny: bad dtype %d", dtype);
    SETOK_CHECK_ARG(out_dtype == dtype || out_dtype == SETOK_F32, "setok_linear_skinny: out_dtype %d must be dtype (%d) or fp32", out_dtype, dtype);
    SETOK_CHECK_ARG(M >= 0 && K > 0, "setok_linear_skinny: bad shape M=%d K=%d", M, K);
    SETOK_CHECK_ARG(N >= 1 && N <= SETOK_SKINNY_MAX_N && N % 16 == 0,
                    "setok_linear_skinny: N=%d must be a multiple of 16 in [16, %d] (wider outputs are setok_linear's)", N, SETOK_SKINNY_MAX_N);
    const int kg = dtype == SETOK_F32 ? 16 : 64, pin = dtype == SETOK_F32 ? 4 : 8, pout = out_dtype == SETOK_F32 ? 4 : 8;
    SETOK_CHECK_ARG(K % kg == 0, "setok_linear_skinny: K=%d must be a multiple of %d", K, kg);
    SETOK_CHECK_ARG(lda >= K && lda % pin == 0, "setok_linear_skinny: lda=%lld must be >= K=%d and a multiple of %d", (long long)lda, K, pin);
    SETOK_CHECK_ARG(ldw >= K && ldw % pin == 0, "setok_linear_skinny: ldw=%lld must be >= K=%d and a multiple of %d", (long long)ldw, K, pin);
    SETOK_CHECK_ARG(ldc >= N && ldc % pout == 0, "setok_linear_skinny: ldc=%lld must be >= N=%d and a multiple of %d", (long long)ldc, N, pout);
    SETOK_CHECK_ARG(aligned16(A) && aligned16(W) && aligned16(C), "setok_linear_skinny: A, W and C must be 16-byte aligned");
    const int64_t need = setok_linear_skinny_workspace(M, N, K);
    SETOK_CHECK_ARG(ws_floats >= need && (ws || need == 0),
                    "setok_linear_skinny: workspace of %lld floats is shorter than setok_linear_skinny_workspace(M, N, K) = %lld", (long long)ws_floats,
                    (long long)need);
    SETOK_CHECK_ARG(need == 0 || aligned16(ws), "setok_linear_skinny: the workspace must be 16-byte aligned");
    if (M == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int slices = cdiv(K, SETOK_SKINNY_KSLICE);
    const SkinnyArgs g{A, W, ws, lda, ldw, M, N, K};
    if (dtype == SETOK_BF16) {
        const dim3 grid(cdiv(M, SK_BM), slices);
        bool ok;
        if (N <= 32) ok = skinny_launch_bf16<1>(s, g, grid);
        else if (N <= 64) ok = skinny_launch_bf16<2>(s, g, grid);
        else if (N <= 128) ok = skinny_launch_bf16<4>(s, g, grid);
        else ok = skinny_launch_bf16<8>(s, g, grid);
        if (!ok) return setok_fail(SETOK_ELAUNCH, "setok_linear_skinny: hipFuncSetAttribute failed");
    } else {
        const dim3 grid((unsigned)(((int64_t)M * N + 255) / 256), slices);
        skinny_f32_kernel<<<grid, 256, 0, s>>>(g);
    }
    SETOK_CHECK_LAUNCH("setok_linear_skinny (partials)");
    const unsigned rb = (unsigned)(((int64_t)M * (N >> 2) + 255) / 256);
    if (out_dtype == SETOK_F32) skinny_reduce_kernel<float><<<rb, 256, 0, s>>>(ws, (float*)C, ldc, M, N, slices, alpha);
    else skinny_reduce_kernel<bf16><<<rb, 256, 0, s>>>(ws, (bf16*)C, ldc, M, N, slices, alpha);
    SETOK_CHECK_LAUNCH("setok_linear_skinny (sum)");
    return SETOK_OK;
}
