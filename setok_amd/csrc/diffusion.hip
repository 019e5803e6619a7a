// diffusion.hip — the glue of the DiffLoss image head (src/model/loss/diffloss.py, src/model/diffusion/): everything of one sampler step
// that is not a Linear.
//   setok_timestep_embedding   sinusoidal embedding of the timesteps (once per sample() call, for all steps)
//   setok_add_silu             SiLU(t_emb + c_emb): the operand of the fused adaLN_modulation GEMM
//   setok_adaln_modulate       [x <- x + gate * h;]  y = LayerNorm(x) * (1 + scale) + shift, shift / scale / gate read in place from that GEMM's output
//   setok_ddpm_step            p_mean_variance + p_sample on the net's output: the fp32 state's update and the next step's 16-bit operand
// All of them: one wave per row, four rows per block, 16-byte accesses, fp32 arithmetic, one rounding per stored value, no atomics, no LDS.  At the
// head's sizes (M <= 256 rows of 1024-4096 elements) each is a few microseconds of memory traffic: what they cost is their launch.
#include "common.h"

#define DF_DISPATCH(NAME, CALL_BF16, CALL_F32) DISPATCH_T(NAME, CALL_BF16, CALL_F32)

static inline bool aligned_elems(int64_t n, int dtype) { return n % (dtype == SETOK_F32 ? 4 : 8) == 0; }      // a row stride that keeps 16-byte alignment

// ---- timestep embedding ------------------------------------------------------------------------------------------------------------------
// torch's arithmetic, operation by operation (diffloss.py:83-88): freqs = exp(-ln(max_period) * j / half) with the product and the quotient rounded
// to fp32 separately, args = t * freqs in fp32, then the accurate cosf / sinf — at 999 rad one fp32 ulp of the argument is 6e-5 rad, and a fast
// intrinsic's range reduction would add far more than that.  For the same reason exp is evaluated in double and rounded once: an expf that is one ulp
// off moves cos / sin at t = 999 by those 6e-5 (measured: 5.6e-5 of the 1e-4 bar with expf, against torch's CPU exp).  dim / 2 values per row, once per
// sample() call: the double-precision exp costs nothing that shows.
template <typename T>
__global__ __launch_bounds__(256) void timestep_embedding_kernel(const float* __restrict__ t, T* emb, int rows, int half, float neg_log_period) {
    constexpr int V = Elem<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float tr = t[row];
    T* er = emb + (int64_t)row * (2 * half);
    for (int j0 = lane * V; j0 < half; j0 += 64 * V) {
        float c[V], s[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
#pragma clang fp contract(off)
            const float f = (float)exp((double)(neg_log_period * (float)(j0 + i) / (float)half));
            const float a = tr * f;
            c[i] = cosf(a);
            s[i] = sinf(a);
        }
        st_vec<T>(er + j0, c);
        st_vec<T>(er + half + j0, s);
    }
}

extern "C" int setok_timestep_embedding(void* stream, int dtype, const float* t, void* emb, int rows, int dim, float max_period) {
    SETOK_CHECK_ARG(t && emb, "setok_timestep_embedding: null operand");
    SETOK_CHECK_ARG(rows >= 0 && dim > 0 && dim % 16 == 0, "setok_timestep_embedding: dim=%d must be a positive multiple of 16 (two halves of 16-byte vectors)", dim);
    SETOK_CHECK_ARG(max_period > 0.f, "setok_timestep_embedding: max_period=%g", (double)max_period);
    SETOK_CHECK_ARG(aligned16(emb), "setok_timestep_embedding: emb must be 16-byte aligned");
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const float nl = (float)(-log((double)max_period));          // the reference's rounding point: the double -math.log(max_period), rounded to fp32 once
    DF_DISPATCH("setok_timestep_embedding", (timestep_embedding_kernel<bf16><<<cdiv(rows, 4), 256, 0, s>>>(t, (bf16*)emb, rows, dim / 2, nl)),
                (timestep_embedding_kernel<float><<<cdiv(rows, 4), 256, 0, s>>>(t, (float*)emb, rows, dim / 2, nl)));
    SETOK_CHECK_LAUNCH("setok_timestep_embedding");
    return SETOK_OK;
}

// ---- SiLU(a + b) ---------------------------------------------------------------------------------------------------------------------------
__device__ inline float silu_f(float v) { return v / (1.0f + expf(-v)); }

template <typename T>
__global__ __launch_bounds__(256) void add_silu_kernel(const T* a, const T* b, int64_t ldb, T* y, int rows, int C) {
    constexpr int V = Elem<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* ar = a + (int64_t)row * C;
    const T* br = b + (int64_t)row * ldb;
    T* yr = y + (int64_t)row * C;
    for (int c = lane * V; c < C; c += 64 * V) {
        float av[V], bv[V];
        ld_vec<T>(ar + c, av);
        ld_vec<T>(br + c, bv);
#pragma unroll
        for (int i = 0; i < V; ++i) av[i] = silu_f(av[i] + bv[i]);
        st_vec<T>(yr + c, av);
    }
}

extern "C" int setok_add_silu(void* stream, int dtype, const void* a, const void* b, int64_t ldb, void* y, int rows, int C) {
    SETOK_CHECK_ARG(a && b && y, "setok_add_silu: null operand");
    SETOK_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0, "setok_add_silu: C=%d must be a positive multiple of 8", C);
    SETOK_CHECK_ARG(ldb == 0 || (ldb >= C && aligned_elems(ldb, dtype)), "setok_add_silu: ldb=%lld must be 0 (one broadcast row) or a 16-byte aligned row stride >= C", (long long)ldb);
    SETOK_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(y), "setok_add_silu: operands must be 16-byte aligned");
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DF_DISPATCH("setok_add_silu", (add_silu_kernel<bf16><<<cdiv(rows, 4), 256, 0, s>>>((const bf16*)a, (const bf16*)b, ldb, (bf16*)y, rows, C)),
                (add_silu_kernel<float><<<cdiv(rows, 4), 256, 0, s>>>((const float*)a, (const float*)b, ldb, (float*)y, rows, C)));
    SETOK_CHECK_LAUNCH("setok_add_silu");
    return SETOK_OK;
}

// ---- [gated residual +] LayerNorm + modulate --------------------------------------------------------------------------------------------------
// Three passes over the row by the wave that owns it, as setok_layernorm's generic kernel (mean, centred variance, apply): pass 1 also applies the
// previous block's gated residual and stores the new x, and every lane re-reads in passes 2 and 3 exactly the elements IT stored (program order, no
// fence needed), so the statistics are those of the stored, rounded x.  The re-reads hit L1 / L2.
template <typename T>
__global__ __launch_bounds__(256) void adaln_modulate_kernel(T* x, const T* h, const T* gate, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const T* shift, const T* scale, int64_t ldm, T* y, int rows, int C, float eps) {
    constexpr int V = Elem<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    T* xr = x + (int64_t)row * C;
    T* yr = y + (int64_t)row * C;
    float buf[V];
    float s = 0.f;
    if (h) {
        const T* hr = h + (int64_t)row * C;
        const T* gr = gate + (int64_t)row * ldm;
        for (int c = lane * V; c < C; c += 64 * V) {
            float hv[V], gv[V];
            ld_vec<T>(xr + c, buf);
            ld_vec<T>(hr + c, hv);
            ld_vec<T>(gr + c, gv);
#pragma unroll
            for (int i = 0; i < V; ++i) buf[i] = (float)(T)fmaf(gv[i], hv[i], buf[i]);          // rounded as stored: the statistics below are of these values
            st_vec<T>(xr + c, buf);
#pragma unroll
            for (int i = 0; i < V; ++i) s += buf[i];
        }
    } else {
        for (int c = lane * V; c < C; c += 64 * V) {
            ld_vec<T>(xr + c, buf);
#pragma unroll
            for (int i = 0; i < V; ++i) s += buf[i];
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane * V; c < C; c += 64 * V) {
        ld_vec<T>(xr + c, buf);
#pragma unroll
        for (int i = 0; i < V; ++i) { const float d = buf[i] - mean; q = fmaf(d, d, q); }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    const T* shr = shift + (int64_t)row * ldm;
    const T* scr = scale + (int64_t)row * ldm;
    for (int c = lane * V; c < C; c += 64 * V) {
        float sh[V], sc[V];
        ld_vec<T>(xr + c, buf);
        ld_vec<T>(shr + c, sh);
        ld_vec<T>(scr + c, sc);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float n = (buf[i] - mean) * rstd;
            if (gamma) n = fmaf(n, gamma[c + i], beta[c + i]);
            buf[i] = fmaf(n, 1.0f + sc[i], sh[i]);
        }
        st_vec<T>(yr + c, buf);
    }
}

extern "C" int setok_adaln_modulate(void* stream, int dtype, void* x, const void* h, const void* gate, const float* gamma, const float* beta,
                                    const void* shift, const void* scale, int64_t ldm, void* y, int rows, int C, float eps) {
    SETOK_CHECK_ARG(x && shift && scale && y, "setok_adaln_modulate: null operand");
    SETOK_CHECK_ARG((h == nullptr) == (gate == nullptr), "setok_adaln_modulate: h and gate go together (both NULL: no residual)");
    SETOK_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "setok_adaln_modulate: gamma and beta go together (both NULL: no affine)");
    SETOK_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0, "setok_adaln_modulate: C=%d must be a positive multiple of 8", C);
    SETOK_CHECK_ARG(ldm >= C && aligned_elems(ldm, dtype), "setok_adaln_modulate: ldm=%lld must be a 16-byte aligned row stride >= C", (long long)ldm);
    SETOK_CHECK_ARG(x != y, "setok_adaln_modulate: y must not alias x");
    SETOK_CHECK_ARG(aligned16(x) && aligned16(h) && aligned16(gate) && aligned16(shift) && aligned16(scale) && aligned16(y),
                    "setok_adaln_modulate: operands must be 16-byte aligned");
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DF_DISPATCH("setok_adaln_modulate",
                (adaln_modulate_kernel<bf16><<<cdiv(rows, 4), 256, 0, s>>>((bf16*)x, (const bf16*)h, (const bf16*)gate, gamma, beta, (const bf16*)shift, (const bf16*)scale,
                                                                          ldm, (bf16*)y, rows, C, eps)),
                (adaln_modulate_kernel<float><<<cdiv(rows, 4), 256, 0, s>>>((float*)x, (const float*)h, (const float*)gate, gamma, beta, (const float*)shift,
                                                                           (const float*)scale, ldm, (float*)y, rows, C, eps)));
    SETOK_CHECK_LAUNCH("setok_adaln_modulate");
    return SETOK_OK;
}

// ---- one reverse step of the DDPM ---------------------------------------------------------------------------------------------------------------
struct DdpmCoef { float cfg_scale, sqrt_recip, sqrt_recipm1, coef1, coef2, min_log, max_log, nonzero, temperature; };

// One wave per state row r (all `rows` of them: under cfg the second half keeps a state of its own, as in the reference, although the net never reads it).
// The operations are the reference's, in its order, in fp32; nothing is contracted across its rounding points except inside one product-sum.
template <int V> __device__ inline void ld_f32n(const float* p, float* o) {
#pragma unroll
    for (int j = 0; j < V; j += 4) ld_vec<float>(p + j, o + j);
}
template <int V> __device__ inline void st_f32n(float* p, const float* o) {
#pragma unroll
    for (int j = 0; j < V; j += 4) st_vec<float>(p + j, o + j);
}
template <typename T, int V> __device__ inline void st_elems(T* p, const float* o) {           // V elements of T: 16 bytes, or 8 when a 16-bit row is written 4 at a time
    if constexpr (V == Elem<T>::VEC) st_vec<T>(p, o);
    else {
        static_assert(sizeof(T) == 2 && V == 4, "half a 16-byte vector of the 16-bit type");
        bf16x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (bf16)o[i];
        *reinterpret_cast<bf16x4*>(p) = v;
    }
}

template <typename T, typename TO>
__global__ __launch_bounds__(256) void ddpm_step_kernel(const TO* out, int64_t ldo, float* x, const float* noise, int noise_rows, T* x_in, int rows, int C, int half,
                                                        DdpmCoef k) {
    constexpr int V = Elem<TO>::VEC;                                     // elements per lane and trip: one 16-byte vector of the net's output
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int rc = half > 0 ? row % half : row;                          // the conditional row this row's eps comes from
    const TO* oc = out + (int64_t)rc * ldo;
    const TO* ou = out + (int64_t)(rc + half) * ldo;                     // (half == 0: not read)
    const TO* ov = out + (int64_t)row * ldo + C;
    float* xr = x + (int64_t)row * C;
    const float* nr = noise + (int64_t)(row % noise_rows) * C;
    for (int c = lane * V; c < C; c += 64 * V) {
        float eps[V], u[V], v[V], xt[V], nz[V];
        ld_vec<TO>(oc + c, eps);
        if (half > 0) ld_vec<TO>(ou + c, u);
        ld_vec<TO>(ov + c, v);
        ld_f32n<V>(xr + c, xt);
        ld_f32n<V>(nr + c, nz);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float e = half > 0 ? u[i] + k.cfg_scale * (eps[i] - u[i]) : eps[i];
            const float x0 = k.sqrt_recip * xt[i] - k.sqrt_recipm1 * e;
            const float mean = k.coef1 * x0 + k.coef2 * xt[i];
            const float f = (v[i] + 1.0f) * 0.5f;
            const float logvar = f * k.max_log + (1.0f - f) * k.min_log;
            xt[i] = mean + k.nonzero * expf(0.5f * logvar) * nz[i] * k.temperature;
        }
        st_f32n<V>(xr + c, xt);
        if (half == 0 || row < half) st_elems<T, V>(x_in + (int64_t)row * C + c, xt);
        if (half > 0 && row < half) st_elems<T, V>(x_in + (int64_t)(row + half) * C + c, xt);
    }
}

extern "C" int setok_ddpm_step(void* stream, int dtype, int out_dtype, const void* out, int64_t ldo, float* x, const float* noise, int noise_rows, void* x_in,
                               int rows, int C, int half, float cfg_scale, float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, float min_log,
                               float max_log, float nonzero, float temperature) {
    SETOK_CHECK_ARG(out && x && noise && x_in, "setok_ddpm_step: null operand");
    SETOK_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0, "setok_ddpm_step: C=%d must be a positive multiple of 8", C);
    SETOK_CHECK_ARG(half >= 0 && (half == 0 || rows == 2 * half), "setok_ddpm_step: rows=%d must be 2 * half (half=%d) under classifier-free guidance", rows, half);
    SETOK_CHECK_ARG(noise_rows == rows || (half > 0 && noise_rows == half), "setok_ddpm_step: noise_rows=%d must be rows (%d) or half (%d)", noise_rows, rows, half);
    SETOK_CHECK_ARG(out_dtype == dtype || out_dtype == SETOK_F32, "setok_ddpm_step: out_dtype %d must be dtype (%d) or fp32", out_dtype, dtype);
    SETOK_CHECK_ARG(ldo >= 2 * (int64_t)C && aligned_elems(ldo, out_dtype), "setok_ddpm_step: ldo=%lld must be a 16-byte aligned row stride >= 2 C", (long long)ldo);
    SETOK_CHECK_ARG(aligned16(out) && aligned16(x) && aligned16(noise) && aligned16(x_in), "setok_ddpm_step: operands must be 16-byte aligned");
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const DdpmCoef k{cfg_scale, sqrt_recip, sqrt_recipm1, coef1, coef2, min_log, max_log, nonzero, temperature};
    const dim3 grid(cdiv(rows, 4));
    if (dtype == SETOK_BF16 && out_dtype == SETOK_F32)
        ddpm_step_kernel<bf16, float><<<grid, 256, 0, s>>>((const float*)out, ldo, x, noise, noise_rows, (bf16*)x_in, rows, C, half, k);
    else
        DF_DISPATCH("setok_ddpm_step", (ddpm_step_kernel<bf16, bf16><<<grid, 256, 0, s>>>((const bf16*)out, ldo, x, noise, noise_rows, (bf16*)x_in, rows, C, half, k)),
                    (ddpm_step_kernel<float, float><<<grid, 256, 0, s>>>((const float*)out, ldo, x, noise, noise_rows, (float*)x_in, rows, C, half, k)));
    SETOK_CHECK_LAUNCH("setok_ddpm_step");
    return SETOK_OK;
}
