// llama_bwd.hip — the dX chain through the FROZEN Llama (stage 2 of the reference's recipe trains mm_in_projector through the LLM loss:
// scripts/pretrain_mm_proj.sh, src/train/train_setokim.py:335-339).  The Linears' dX are setok_linear calls against transposed weights;
// these are the backward twins of llama.hip's other pieces.  No weight gradient is formed anywhere.
//   setok_lm_loss_bwd               d loss / d logits of setok_lm_loss
//   setok_rmsnorm_bwd               dx of LlamaRMSNorm (+ the residual branch's gradient in the same pass)
//   setok_rope_bwd_gqa              the transpose of setok_rope_gqa, in place on [dq | dk | dv]
//   setok_swiglu_pairs_bwd          d (gate_j, up_j) pairs from the pre-activation pairs and dout
//   setok_attention_causal_bwd_gqa  backward of setok_attention_causal_gqa: a 16-bit MFMA pair for head dim 128 (attn_causal_bwd.hip), a generic
//                                   wave-per-row pair (here) for everything else
// No atomics, every sum in a fixed order: two runs give the same bits, and a sequence's gradients do not depend on its neighbours in the batch.
#include "common.h"

#include <stdlib.h>

namespace {

template <typename T> __device__ inline float rnd(float v) { return (float)(T)v; }

// ---- d loss / d logits ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (sequence, position).  A position the forward did not count (last of its sequence, next token padded or ignored) gets a
// row of exact zeros without its logits being read; the others get upstream * (softmax(row) - onehot(target)) / n with n = loss_out[1], the
// forward's count, read on the device.  Element accesses are scalar: rows of a resized vocabulary (32003) start at any 2- / 4-byte boundary.
template <typename T>
__global__ __launch_bounds__(256) void lm_loss_bwd_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                          const uint8_t* __restrict__ amask, int Tn, int V, int ignore_index,
                                                          const float* __restrict__ loss_out, const float* __restrict__ upstream,
                                                          T* __restrict__ dlogits, int64_t ldd) {
    const int row = blockIdx.x, t = row % Tn, tid = threadIdx.x;
    __shared__ float red[4];
    bool valid = t + 1 < Tn;
    int64_t target = 0;
    if (valid) {
        target = labels[row + 1];
        valid = (!amask || amask[row + 1] != 0) && target != (int64_t)ignore_index;
    }
    T* d = dlogits + (int64_t)row * ldd;
    if (!valid) {
        for (int c = tid; c < V; c += 256) d[c] = (T)0.0f;
        return;
    }
    const T* x = logits + (int64_t)row * ld;
    float m = -INFINITY;
    for (int c = tid; c < V; c += 256) m = fmaxf(m, (float)x[c]);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = tid; c < V; c += 256) sum += expf((float)x[c] - m);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float tot = (red[0] + red[1]) + (red[2] + red[3]);
    const float g = (upstream ? upstream[0] : 1.0f) / loss_out[1];       // (a counted row exists, so n >= 1)
    const float inv = 1.0f / tot;
    for (int c = tid; c < V; c += 256) {
        const float p = expf((float)x[c] - m) * inv;
        d[c] = (T)(g * (p - ((int64_t)c == target ? 1.0f : 0.0f)));
    }
}

// ---- RMSNorm dx ------------------------------------------------------------------------------------------------------------------------------
// y = w * (x * rstd).to(T), w rounded to T (setok_rmsnorm).  g = (dy * w).to(T) — the gradient at the forward's rounding point, as the eager
// 16-bit graph forms it — then in fp32: dx = rstd * (g - xhat * mean(g * xhat)), xhat = x * rstd, rounded to T; `dres` (the residual branch's
// gradient) is added to the rounded value.  One wave per row, statistics recomputed.
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const T* dy, const T* dres, T* dx, int rows,
                                                          int C, float eps) {            // (dx may alias dy or dres: a lane rewrites what it has read)
    constexpr int V = Elem<T>::VEC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (int64_t)row * C;
    const T* gr = dy + (int64_t)row * C;
    float xb[V], gb[V], s = 0.f, dot = 0.f;
    for (int c = lane * V; c < C; c += 64 * V) {
        ld_vec<T>(xr + c, xb); ld_vec<T>(gr + c, gb);
#pragma unroll
        for (int i = 0; i < V; ++i) { s += xb[i] * xb[i]; dot += rnd<T>(gb[i] * rnd<T>(w[c + i])) * xb[i]; }
    }
    const float rstd = rsqrtf(wave_sum(s) / (float)C + eps);
    const float k = wave_sum(dot) * rstd * rstd / (float)C;               // mean(g * xhat) * rstd, per unit of x
    for (int c = lane * V; c < C; c += 64 * V) {
        float rb[V];
        ld_vec<T>(xr + c, xb); ld_vec<T>(gr + c, gb);
        if (dres) ld_vec<T>(dres + (int64_t)row * C + c, rb);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float v = rnd<T>(rstd * (rnd<T>(gb[i] * rnd<T>(w[c + i])) - xb[i] * k));
            gb[i] = dres ? v + rb[i] : v;
        }
        st_vec<T>(dx + (int64_t)row * C + c, gb);
    }
}

// ---- rotary embedding, transposed: [dq | dk] rotated back by the same tables ---------------------------------------------------------------------
// forward: o1 = x1 c - x2 s, o2 = x2 c + x1 s  =>  dx1 = do1 c + do2 s, dx2 = do2 c - do1 s (tables and roundings as setok_rope_gqa's)
template <typename T>
__global__ void rope_bwd_kernel(T* __restrict__ dqkv, const int64_t* __restrict__ pos, int rows, int H, int Hkv, int Dh, float log2_theta) {
    const int half = Dh >> 1;
    const int HR = H + Hkv;
    const int64_t total = (int64_t)rows * half;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % half);
        const int64_t r = i / half;
        const float ang = (float)pos[r] * (1.0f / exp2f(log2_theta * (float)(2 * d) / (float)Dh));
        const float c = rnd<T>(cosf(ang)), s = rnd<T>(sinf(ang));
        T* p = dqkv + r * (int64_t)((H + 2 * Hkv) * Dh) + d;
        for (int hh = 0; hh < HR; ++hh, p += Dh) {
            const float g1 = (float)p[0], g2 = (float)p[half];
            p[0] = (T)(rnd<T>(g1 * c) + rnd<T>(g2 * s));
            p[half] = (T)(rnd<T>(g2 * c) + rnd<T>(-g1 * s));
        }
    }
}

// ---- SwiGLU on interleaved pairs, backward -------------------------------------------------------------------------------------------------------
// out_j = silu(gate_j) * up_j  =>  d gate_j = dout_j up_j s (1 + gate_j (1 - s)), d up_j = dout_j silu(gate_j), s = sigmoid(gate_j); fp32, one rounding
template <typename T>
__global__ __launch_bounds__(256) void swiglu_pairs_bwd_kernel(const T* gu, const T* __restrict__ dout, T* dgu, int64_t rows, int F) {      // (dgu may alias gu)
    constexpr int V = Elem<T>::VEC;
    const int chunks = F / V;
    const int64_t total = rows * chunks;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / chunks; const int c = (int)(i % chunks) * V;
        float a[V], b[V], g[V];
        ld_vec<T>(gu + r * 2 * F + 2 * c, a); ld_vec<T>(gu + r * 2 * F + 2 * c + V, b); ld_vec<T>(dout + r * F + c, g);
#pragma unroll
        for (int e = 0; e < V / 2; ++e) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                float* p = hf ? b : a;
                const float gate = p[2 * e], up = p[2 * e + 1], go = g[hf * (V / 2) + e];
                const float s = 1.0f / (1.0f + expf(-gate));
                p[2 * e] = go * up * s * (1.0f + gate * (1.0f - s));
                p[2 * e + 1] = go * gate * s;
            }
        }
        st_vec<T>(dgu + r * 2 * F + 2 * c, a); st_vec<T>(dgu + r * 2 * F + 2 * c + V, b);
    }
}

// ---- generic causal attention backward: one wave per (query row, head), then one per (key row, key / value head) -----------------------------------
// s_ij = scale q_i.k_j over the keys query i sees (j <= i, key_mask[j]); p = softmax; D_i = do_i.o_i; ds_ij = p_ij (do_i.v_j - D_i);
// dq_i = scale sum_j ds_ij k_j; dk_j = scale sum_i ds_ij q_i; dv_j = sum_i p_ij do_i — for a shared key / value head summed over its H / Hkv query
// heads in head order.  The query kernel leaves lse_i and D_i in the workspace for the key kernel.  Head dim <= 64 * VEC * AT_MAXC.
template <typename T>
__device__ inline float cdot(const T* base, const float (&a)[AT_MAXC][Elem<T>::VEC], int lane, int Dh) {
    constexpr int V = Elem<T>::VEC;
    float acc = 0.f, buf[V];
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) {
        const int d = (c * 64 + lane) * V;
        if (d < Dh) {
            ld_vec<T>(base + d, buf);
#pragma unroll
            for (int i = 0; i < V; ++i) acc = fmaf(a[c][i], buf[i], acc);
        }
    }
    return wave_sum(acc);
}

template <typename T>
__global__ __launch_bounds__(64) void attn_causal_bwd_q_kernel(const T* __restrict__ qkv, const uint8_t* __restrict__ kmask, const T* __restrict__ o,
                                                               const T* __restrict__ dout, T* __restrict__ dqkv, int Tn, int H, int Hkv, int Dh,
                                                               float scale, float* __restrict__ lse, float* __restrict__ dsum) {
    constexpr int V = Elem<T>::VEC;
    const int row = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int b = row / Tn, i = row % Tn;
    const int64_t C = (int64_t)H * Dh, ld = (int64_t)(H + 2 * Hkv) * Dh;
    const int hk = h / (H / Hkv);
    const T* kb = qkv + (int64_t)b * Tn * ld + C + (int64_t)hk * Dh;
    const T* vb = kb + (int64_t)Hkv * Dh;
    const uint8_t* km = kmask ? kmask + (int64_t)b * Tn : nullptr;
    float qr[AT_MAXC][V], dO[AT_MAXC][V], dqr[AT_MAXC][V], buf[V];
    float D = 0.f;
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) {
        const int d = (c * 64 + lane) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) { qr[c][e] = 0.f; dO[c][e] = 0.f; dqr[c][e] = 0.f; }
        if (d < Dh) {
            ld_vec<T>(qkv + (int64_t)row * ld + (int64_t)h * Dh + d, qr[c]);
            ld_vec<T>(dout + (int64_t)row * C + (int64_t)h * Dh + d, dO[c]);
            ld_vec<T>(o + (int64_t)row * C + (int64_t)h * Dh + d, buf);
#pragma unroll
            for (int e = 0; e < V; ++e) D += dO[c][e] * buf[e];
        }
    }
    D = wave_sum(D);
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j <= i; ++j) {
        if (km && !km[j]) continue;
        const float s = cdot<T>(kb + (int64_t)j * ld, qr, lane, Dh) * scale;
        const float mn = fmaxf(m, s);
        l = l * expf(m - mn) + expf(s - mn);
        m = mn;
    }
    const float L = l > 0.f ? m + logf(l) : 0.f;                       // (a query that sees no key: nothing below runs, dq = 0)
    for (int j = 0; j <= i; ++j) {
        if (km && !km[j]) continue;
        const T* kp = kb + (int64_t)j * ld;
        const float p = expf(cdot<T>(kp, qr, lane, Dh) * scale - L);
        const float ds = p * (cdot<T>(vb + (int64_t)j * ld, dO, lane, Dh) - D) * scale;
#pragma unroll
        for (int c = 0; c < AT_MAXC; ++c) {
            const int d = (c * 64 + lane) * V;
            if (d < Dh) {
                ld_vec<T>(kp + d, buf);
#pragma unroll
                for (int e = 0; e < V; ++e) dqr[c][e] = fmaf(ds, buf[e], dqr[c][e]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) {
        const int d = (c * 64 + lane) * V;
        if (d < Dh) st_vec<T>(dqkv + (int64_t)row * ld + (int64_t)h * Dh + d, dqr[c]);
    }
    if (lane == 0) { lse[(int64_t)row * H + h] = L; dsum[(int64_t)row * H + h] = D; }
}

template <typename T>
__global__ __launch_bounds__(64) void attn_causal_bwd_kv_kernel(const T* __restrict__ qkv, const uint8_t* __restrict__ kmask, const T* __restrict__ dout,
                                                                T* __restrict__ dqkv, int Tn, int H, int Hkv, int Dh, float scale,
                                                                const float* __restrict__ lse, const float* __restrict__ dsum) {
    constexpr int V = Elem<T>::VEC;
    const int row = blockIdx.x, hk = blockIdx.y, lane = threadIdx.x;
    const int b = row / Tn, j = row % Tn;
    const int G = H / Hkv;
    const int64_t C = (int64_t)H * Dh, ld = (int64_t)(H + 2 * Hkv) * Dh;
    const int64_t ko = (int64_t)row * ld + C + (int64_t)hk * Dh, vo = ko + (int64_t)Hkv * Dh;
    float kr[AT_MAXC][V], vr[AT_MAXC][V], dkr[AT_MAXC][V], dvr[AT_MAXC][V], qb[AT_MAXC][V], ob[AT_MAXC][V];
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) {
        const int d = (c * 64 + lane) * V;
#pragma unroll
        for (int e = 0; e < V; ++e) { kr[c][e] = 0.f; vr[c][e] = 0.f; dkr[c][e] = 0.f; dvr[c][e] = 0.f; qb[c][e] = 0.f; ob[c][e] = 0.f; }
        if (d < Dh) { ld_vec<T>(qkv + ko + d, kr[c]); ld_vec<T>(qkv + vo + d, vr[c]); }
    }
    const bool seen = !kmask || kmask[row] != 0;                        // a padded key is seen by no query: zeros
    if (seen) {
        for (int h = hk * G; h < hk * G + G; ++h) {
            for (int i = j; i < Tn; ++i) {
                const int64_t r = (int64_t)b * Tn + i;
                float a = 0.f, bb = 0.f;
#pragma unroll
                for (int c = 0; c < AT_MAXC; ++c) {
                    const int d = (c * 64 + lane) * V;
                    if (d < Dh) {
                        ld_vec<T>(qkv + r * ld + (int64_t)h * Dh + d, qb[c]);
                        ld_vec<T>(dout + r * C + (int64_t)h * Dh + d, ob[c]);
#pragma unroll
                        for (int e = 0; e < V; ++e) { a = fmaf(qb[c][e], kr[c][e], a); bb = fmaf(ob[c][e], vr[c][e], bb); }
                    }
                }
                const float s = wave_sum(a) * scale, dp = wave_sum(bb);
                const float p = expf(s - lse[r * H + h]);
                const float ds = p * (dp - dsum[r * H + h]) * scale;
#pragma unroll
                for (int c = 0; c < AT_MAXC; ++c) {
#pragma unroll
                    for (int e = 0; e < V; ++e) { dkr[c][e] = fmaf(ds, qb[c][e], dkr[c][e]); dvr[c][e] = fmaf(p, ob[c][e], dvr[c][e]); }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < AT_MAXC; ++c) {
        const int d = (c * 64 + lane) * V;
        if (d < Dh) { st_vec<T>(dqkv + ko + d, dkr[c]); st_vec<T>(dqkv + vo + d, dvr[c]); }
    }
}

inline int grid_for(int64_t total) { return (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536); }

}  // namespace

extern "C" int setok_lm_loss_bwd(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels, const uint8_t* attention_mask,
                                 int B, int T, int V, int ignore_index, const float* loss_out, const float* upstream, void* dlogits, int64_t ldd) {
    SETOK_CHECK_ARG(logits && labels && loss_out && dlogits, "setok_lm_loss_bwd: null operand");
    SETOK_CHECK_ARG(B >= 0 && T > 0 && V > 0 && ld >= V && ldd >= V, "setok_lm_loss_bwd: bad shape B=%d T=%d V=%d", B, T, V);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int rows = B * T;
    DISPATCH_T("setok_lm_loss_bwd",
               (lm_loss_bwd_kernel<bf16><<<rows, 256, 0, s>>>((const bf16*)logits, ld, labels, attention_mask, T, V, ignore_index, loss_out, upstream, (bf16*)dlogits, ldd)),
               (lm_loss_bwd_kernel<float><<<rows, 256, 0, s>>>((const float*)logits, ld, labels, attention_mask, T, V, ignore_index, loss_out, upstream, (float*)dlogits, ldd)));
    SETOK_CHECK_LAUNCH("setok_lm_loss_bwd");
    return SETOK_OK;
}

extern "C" int setok_rmsnorm_bwd(void* stream, int dtype, const void* x, const float* weight, const void* dy, const void* dres, void* dx, int rows,
                                 int C, float eps) {
    SETOK_CHECK_ARG(x && weight && dy && dx, "setok_rmsnorm_bwd: null operand");
    SETOK_CHECK_ARG(rows >= 0 && C > 0 && C % 8 == 0, "setok_rmsnorm_bwd: C=%d must be a positive multiple of 8", C);
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T("setok_rmsnorm_bwd",
               (rmsnorm_bwd_kernel<bf16><<<cdiv(rows, 4), 256, 0, s>>>((const bf16*)x, weight, (const bf16*)dy, (const bf16*)dres, (bf16*)dx, rows, C, eps)),
               (rmsnorm_bwd_kernel<float><<<cdiv(rows, 4), 256, 0, s>>>((const float*)x, weight, (const float*)dy, (const float*)dres, (float*)dx, rows, C, eps)));
    SETOK_CHECK_LAUNCH("setok_rmsnorm_bwd");
    return SETOK_OK;
}

extern "C" int setok_rope_bwd_gqa(void* stream, int dtype, void* dqkv, const int64_t* position_ids, int rows, int H, int Hkv, int Dh, float theta) {
    SETOK_CHECK_ARG(dqkv && position_ids, "setok_rope_bwd: null operand");
    SETOK_CHECK_ARG(rows >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && Dh > 0 && Dh % 2 == 0 && theta > 0.f, "setok_rope_bwd: bad shape (H=%d Hkv=%d Dh=%d)", H, Hkv, Dh);
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const float l2 = log2f(theta);
    const int grid = grid_for((int64_t)rows * (Dh / 2));
    DISPATCH_T("setok_rope_bwd", (rope_bwd_kernel<bf16><<<grid, 256, 0, s>>>((bf16*)dqkv, position_ids, rows, H, Hkv, Dh, l2)),
               (rope_bwd_kernel<float><<<grid, 256, 0, s>>>((float*)dqkv, position_ids, rows, H, Hkv, Dh, l2)));
    SETOK_CHECK_LAUNCH("setok_rope_bwd");
    return SETOK_OK;
}

extern "C" int setok_swiglu_pairs_bwd(void* stream, int dtype, const void* gate_up_pairs, const void* dout, void* dpairs, int64_t rows, int F) {
    SETOK_CHECK_ARG(gate_up_pairs && dout && dpairs, "setok_swiglu_pairs_bwd: null operand");
    SETOK_CHECK_ARG(rows >= 0 && F > 0 && F % 8 == 0, "setok_swiglu_pairs_bwd: bad shape (F=%d must be a positive multiple of 8)", F);
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = grid_for(rows * (F / (dtype == SETOK_BF16 ? 8 : 4)));
    DISPATCH_T("setok_swiglu_pairs_bwd",
               (swiglu_pairs_bwd_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)gate_up_pairs, (const bf16*)dout, (bf16*)dpairs, rows, F)),
               (swiglu_pairs_bwd_kernel<float><<<grid, 256, 0, s>>>((const float*)gate_up_pairs, (const float*)dout, (float*)dpairs, rows, F)));
    SETOK_CHECK_LAUNCH("setok_swiglu_pairs_bwd");
    return SETOK_OK;
}

int setok_attention_causal_bwd_mfma(hipStream_t s, const bf16* qkv, const uint8_t* key_mask, const bf16* out, const bf16* dout, bf16* dqkv, int B, int T,
                                    int H, int Hkv, float scale, float* lse, float* dsum);   // attn_causal_bwd.hip

extern "C" int setok_attention_causal_bwd_gqa(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, const void* out, const void* dout,
                                              void* dqkv, int B, int T, int H, int Hkv, int Dh, float scale, float* ws) {
    SETOK_CHECK_ARG(qkv && out && dout && dqkv && ws, "setok_attention_causal_bwd: null operand");
    SETOK_CHECK_ARG(B >= 0 && T > 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && Dh > 0 && Dh % 8 == 0,
                    "setok_attention_causal_bwd: bad shape B=%d T=%d H=%d Hkv=%d Dh=%d", B, T, H, Hkv, Dh);
    SETOK_CHECK_ARG(Dh <= 64 * AT_MAXC * (dtype == SETOK_F32 ? 4 : 8), "setok_attention_causal_bwd: head dim %d too large", Dh);
    SETOK_CHECK_ARG(dtype == SETOK_F32 || dtype == SETOK_BF16, "setok_attention_causal_bwd: bad dtype %d", dtype);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    float* lse = ws;
    float* dsum = ws + (int64_t)B * T * H;
    if (dtype == SETOK_BF16 && Dh == 128) {
        const char* e = getenv("SETOK_LLAMA_ATTN_BWD_GENERIC");          // A/B in one process: force the wave-per-row pair
        if (!(e && e[0] == '1'))
            return setok_attention_causal_bwd_mfma(s, (const bf16*)qkv, key_mask, (const bf16*)out, (const bf16*)dout, (bf16*)dqkv, B, T, H, Hkv, scale, lse, dsum);
    }
    const dim3 gq(B * T, H), gkv(B * T, Hkv);
    auto launch = [&](auto elem) {
        using E = decltype(elem);
        attn_causal_bwd_q_kernel<E><<<gq, 64, 0, s>>>((const E*)qkv, key_mask, (const E*)out, (const E*)dout, (E*)dqkv, T, H, Hkv, Dh, scale, lse, dsum);
        attn_causal_bwd_kv_kernel<E><<<gkv, 64, 0, s>>>((const E*)qkv, key_mask, (const E*)dout, (E*)dqkv, T, H, Hkv, Dh, scale, lse, dsum);
    };
    if (dtype == SETOK_BF16) launch(bf16{});
    else launch(float{});
    SETOK_CHECK_LAUNCH("setok_attention_causal_bwd");
    return SETOK_OK;
}

extern "C" int setok_attention_causal_bwd(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, const void* out, const void* dout,
                                          void* dqkv, int B, int T, int H, int Dh, float scale, float* ws) {
    return setok_attention_causal_bwd_gqa(stream, dtype, qkv, key_mask, out, dout, dqkv, B, T, H, H, Dh, scale, ws);
}
