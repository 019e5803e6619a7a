// attn_decode.hip — KV-cached greedy generation: what one decoding step of HuggingFace Llama needs beyond the prefill's entries
// (SetokimLlamaForCausalLM.generate, src/model/language_model/setokim_llama.py:329-396, decodes with `past_key_values`, :99,133,189).
//   setok_kv_append             the post-rotary k / v columns of a fused [q | k | v] buffer -> slots [pos0, pos0 + T) of a (B, Hkv, cap, Dh) cache
//   setok_attention_decode_gqa  one query row per (sequence, query head) against the cached keys / values: eager_attention_forward for one new token
//   setok_argmax_rows           greedy selection on the device (lowest index of the row maximum)
//   setok_kv_append_fp8, setok_attention_decode_gqa_fp8kv   the same two over a cache stored as e4m3fn rows with a power-of-two exponent per row
//                               (second half of this file)
//
// The decode attention is bound by the K / V bytes it reads.  Its structure:
//   - work is cut over (key chunk of SETOK_DECODE_CHUNK slots, key / value head, sequence); the chunk length is a constant, so the partition of a
//     sequence's keys — and with it every summation order — depends on `len` alone, never on the batch or on the cache's capacity;
//   - a workgroup (4 waves) owns one chunk; each wave streams 32 consecutive K rows and the same V rows straight into registers with 16-byte
//     loads, all issued before the first use (no LDS staging of the streamed operand: each byte is used by exactly one wave);
//   - a row of the cache is spread over LPR = Dh / (elements per 16 bytes) lanes, so one load instruction covers 64 / LPR keys; the G = H / Hkv
//     query heads of the group are scored against the SAME registers (K / V are read once per group, not once per query head);
//   - scores and softmax in fp32; in the 16-bit types exp(s - m) is rounded to the element type before it multiplies V (HF's rounding point,
//     as in the prefill kernels), the normaliser sums the unrounded values;
//   - every chunk writes fp32 partials (max, sum, Dh accumulators per query head) to the caller's workspace; a second launch merges a query
//     head's chunks in chunk order.  No atomics, no hand-off between workgroups inside a launch.
// A key counts iff its slot is < len and its mask byte is non-zero; a sequence without such a key gets zeros (the prefill kernel's convention).
#include "common.h"
#include "fp8.h"
#include "attn_partials.h"

namespace {

template <typename T> __device__ inline float rnd(float v) { return (float)(T)v; }

template <typename T> struct Raw16;
template <> struct Raw16<float> { typedef f32x4 type; };
template <> struct Raw16<bf16> { typedef bf16x8 type; };

constexpr int DEC_CHUNK = SETOK_DECODE_CHUNK;
constexpr int DEC_WAVES = 4;
constexpr int DEC_WKEYS = DEC_CHUNK / DEC_WAVES;          // keys per wave
static_assert(DEC_WKEYS == 32, "the wave's slice is 32 keys: NSTEP = LPR / 2 below");

// Sum over aligned groups of N lanes (N a power of two), every lane of a group ending with the same bits: an xor butterfly.  Inside a row of 16 lanes the
// exchanges are DPP modifiers on the add (quad_perm for xor 1 and 2; once a quad's lanes agree, row_half_mirror and row_mirror pair the same partial sums
// as xor 4 and xor 8) instead of ds_bpermute round trips through the LDS crossbar.
template <int CTRL> __device__ inline float dpp_add(float a) {
    return a + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), CTRL, 0xf, 0xf, false));
}
template <int N> __device__ inline float row_sum(float a) {
    if constexpr (N >= 2) a = dpp_add<0xB1>(a);          // quad_perm [1, 0, 3, 2]
    if constexpr (N >= 4) a = dpp_add<0x4E>(a);          // quad_perm [2, 3, 0, 1]
    if constexpr (N >= 8) a = dpp_add<0x141>(a);         // row_half_mirror
    if constexpr (N >= 16) a = dpp_add<0x140>(a);        // row_mirror
#pragma unroll
    for (int o = 16; o < N; o <<= 1) a += __shfl_xor(a, o, 64);
    return a;
}

// ---- kv_append ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void kv_append_kernel(const T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc, int B, int Tn, int H, int Hkv,
                                                        int Dh, int cap, int pos0) {
    constexpr int VEC = Elem<T>::VEC;
    typedef typename Raw16<T>::type V16;
    const int vpr = Dh / VEC;                                          // 16-byte pieces per head row
    const int64_t per_row = (int64_t)2 * Hkv * vpr, total = (int64_t)B * Tn * per_row;
    const int64_t ld = (int64_t)(H + 2 * Hkv) * Dh;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / per_row;
        const int rem = (int)(i % per_row);
        const int which = rem / (Hkv * vpr), hk = (rem / vpr) % Hkv, p = rem % vpr;      // which: 0 = k, 1 = v
        const int b = (int)(row / Tn), t = (int)(row % Tn);
        const V16 v = *reinterpret_cast<const V16*>(qkv + row * ld + (int64_t)(H + which * Hkv + hk) * Dh + p * VEC);
        T* dst = (which ? vc : kc) + (((int64_t)b * Hkv + hk) * cap + pos0 + t) * Dh + p * VEC;
        *reinterpret_cast<V16*>(dst) = v;
    }
}

// ---- decode attention, a cache row spread over LPR lanes -------------------------------------------------------------------------------------
// grid (chunks, Hkv * (G / GT), B); GT query heads of one group per workgroup (G itself for G in {1, 2, 4, 8}).  ws: per (sequence, query head,
// chunk) Dh + 2 floats [max, sum, accumulators].
template <typename T, int LPR, int GT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kc, const T* __restrict__ vc,
                                                          const uint8_t* __restrict__ kmask, float* __restrict__ ws, int cap, int len, int H,
                                                          int Hkv, float scale) {
    constexpr int VEC = Elem<T>::VEC, DH = LPR * VEC, KPS = 64 / LPR, NSTEP = DEC_WKEYS / KPS;
    typedef typename Raw16<T>::type V16;
    __shared__ float red[DEC_WAVES][GT][DH + 2];
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int G = H / Hkv, npass = G / GT;
    const int hk = blockIdx.y / npass, h0 = hk * G + (blockIdx.y % npass) * GT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane / LPR, cc = lane % LPR;
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    const int jw = c * DEC_CHUNK + wave * DEC_WKEYS;                   // the wave's first key

    if (jw >= len) {                                                   // the whole slice lies past len (the last chunk): no key, nothing to load
        if (r == 0) {
#pragma unroll
            for (int g = 0; g < GT; ++g) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wave][g][2 + cc * VEC + e] = 0.f;
                if (cc == 0) { red[wave][g][0] = -INFINITY; red[wave][g][1] = 0.f; }
            }
        }
    } else {
        // every K and V load of the wave's slice is issued here, before the first use; a slot at or past len is read as slot len - 1 (in bounds) and masked
        // (the mask bytes first: loads return in order, and a score must not have to wait for the V rows issued behind its K row)
        V16 kr[NSTEP], vr[NSTEP];
        uint8_t mb[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            mb[i] = kmask[(int64_t)b * cap + jc];                         // (unconditional: a load behind a branch is waited for on the spot)
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            kr[i] = *reinterpret_cast<const V16*>(kc + (rowbase + jc) * DH + cc * VEC);
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            vr[i] = *reinterpret_cast<const V16*>(vc + (rowbase + jc) * DH + cc * VEC);
        }
        float qf[GT][VEC];
#pragma unroll
        for (int g = 0; g < GT; ++g) ld_vec<T>(q + (int64_t)b * ldq + (int64_t)(h0 + g) * DH + cc * VEC, qf[g]);
        __builtin_amdgcn_sched_barrier(0);                                // all of the above in flight before the first wait: hipcc otherwise sinks the loads to their uses
        bool ok[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) ok[i] = (jw + i * KPS + r < len) & (mb[i] != 0);

        float s[NSTEP][GT], m[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) m[g] = -INFINITY;
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            float kf[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) kf[e] = (float)kr[i][e];
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) a = fmaf(qf[g][e], kf[e], a);
                a = row_sum<LPR>(a);                                              // over the row's LPR lanes: every lane ends with the same bits
                s[i][g] = ok[i] ? a * scale : -INFINITY;
                m[g] = fmaxf(m[g], s[i][g]);
            }
        }
        float l[GT], acc[GT][VEC];
#pragma unroll
        for (int g = 0; g < GT; ++g) {
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) m[g] = fmaxf(m[g], __shfl_xor(m[g], o, 64));   // one maximum per wave and query head
            l[g] = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[g][e] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            float vf[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) vf[e] = ok[i] ? (float)vr[i][e] : 0.f;      // (a masked slot may hold anything, NaN included)
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                const float p = m[g] == -INFINITY ? 0.f : dec_exp<T>(s[i][g] - m[g]);
                l[g] += p;
                const float pr = rnd<T>(p);                                           // probabilities cast to the element type (HF)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[g][e] = fmaf(pr, vf[e], acc[g][e]);
            }
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) {
                l[g] += __shfl_xor(l[g], o, 64);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[g][e] += __shfl_xor(acc[g][e], o, 64);
            }
            if (r == 0) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wave][g][2 + cc * VEC + e] = acc[g][e];
                if (cc == 0) { red[wave][g][0] = m[g]; red[wave][g][1] = l[g]; }
            }
        }
    }
    __syncthreads();
    // the chunk's partial: the four waves in wave order
    for (int idx = tid; idx < GT * DH; idx += 256) {
        const int g = idx / DH, d = idx % DH;
        float M = red[0][g][0];
#pragma unroll
        for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, red[w][g][0]);
        float L = 0.f, val = 0.f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float f = red[w][g][0] == -INFINITY ? 0.f : dec_exp<T>(red[w][g][0] - M);
            L = fmaf(f, red[w][g][1], L);
            val = fmaf(f, red[w][g][2 + d], val);
        }
        float* part = ws + (((int64_t)b * H + h0 + g) * nch + c) * (DH + 2);
        part[2 + d] = val;
        if (d == 0) { part[0] = M; part[1] = L; }
    }
}

// ---- decode attention, any head dim (Dh % 8 == 0): one wave per (chunk, query head, sequence), a key per lane -----------------------------------
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_any_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kc, const T* __restrict__ vc,
                                                             const uint8_t* __restrict__ kmask, float* __restrict__ ws, int cap, int len, int H,
                                                             int Hkv, int Dh, float scale) {
    __shared__ float ps[DEC_CHUNK];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, nch = gridDim.x, lane = threadIdx.x;
    const int hk = h / (H / Hkv), j0 = c * DEC_CHUNK;
    const T* qr = q + (int64_t)b * ldq + (int64_t)h * Dh;
    const T* kb = kc + ((int64_t)b * Hkv + hk) * cap * Dh;
    const T* vb = vc + ((int64_t)b * Hkv + hk) * cap * Dh;
    float mx = -INFINITY;
    for (int jj = lane; jj < DEC_CHUNK; jj += 64) {
        const int j = j0 + jj;
        float sc = -INFINITY;
        if (j < len && kmask[(int64_t)b * cap + j]) {
            float a = 0.f;
            for (int d = 0; d < Dh; ++d) a = fmaf((float)qr[d], (float)kb[(int64_t)j * Dh + d], a);
            sc = a * scale;
        }
        ps[jj] = sc;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int jj = lane; jj < DEC_CHUNK; jj += 64) {
        const float e = mx == -INFINITY ? 0.f : dec_exp<T>(ps[jj] - mx);
        ps[jj] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float* part = ws + (((int64_t)b * H + h) * nch + c) * (Dh + 2);
    if (lane == 0) { part[0] = mx; part[1] = sum; }
    for (int d = lane; d < Dh; d += 64) {
        float o = 0.f;
        for (int jj = 0; jj < DEC_CHUNK; ++jj)
            if (ps[jj] != 0.f) o = fmaf(rnd<T>(ps[jj]), (float)vb[(int64_t)(j0 + jj) * Dh + d], o);      // (a non-zero weight: slot < len and unmasked)
        part[2 + d] = o;
    }
}

// ---- argmax over the rows of a matrix: lowest index of the maximum (a NaN counts as the maximum, like torch.argmax) ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void argmax_rows_kernel(const T* __restrict__ x, int64_t ld, int V, int64_t* __restrict__ out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const T* row = x + (int64_t)blockIdx.x * ld;
    float best = -INFINITY;
    int at = V;                                                        // "nothing yet": any index beats it on a tie
    for (int i = threadIdx.x; i < V; i += 256) {                       // ascending: a strict comparison keeps the lowest index
        const float v = (float)row[i];
        const bool nan_v = v != v, nan_b = best != best;
        if (at == V || (!nan_b && (nan_v || v > best))) { best = v; at = i; }
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = at;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float v = bv[threadIdx.x + o], w = bv[threadIdx.x];
            const int iv = bi[threadIdx.x + o], iw = bi[threadIdx.x];
            const bool nan_v = v != v, nan_w = w != w;
            bool take;
            if (iv == V) take = false;
            else if (iw == V) take = true;
            else if (nan_v || nan_w) take = nan_v && (!nan_w || iv < iw);
            else take = v > w || (v == w && iv < iw);
            if (take) { bv[threadIdx.x] = v; bi[threadIdx.x] = iv; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = bi[0];
}

template <typename T, int LPR>
int launch_decode(hipStream_t s, const T* q, int64_t ldq, const T* kc, const T* vc, const uint8_t* km, float* ws, int B, int H, int Hkv, int cap,
                  int len, float scale) {
    const int G = H / Hkv, nch = cdiv(len, DEC_CHUNK);
    const int GT = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
    dim3 grid(nch, Hkv * (G / GT), B);
    switch (GT) {
        case 8: attn_decode_kernel<T, LPR, 8><<<grid, 256, 0, s>>>(q, ldq, kc, vc, km, ws, cap, len, H, Hkv, scale); break;
        case 4: attn_decode_kernel<T, LPR, 4><<<grid, 256, 0, s>>>(q, ldq, kc, vc, km, ws, cap, len, H, Hkv, scale); break;
        case 2: attn_decode_kernel<T, LPR, 2><<<grid, 256, 0, s>>>(q, ldq, kc, vc, km, ws, cap, len, H, Hkv, scale); break;
        default: attn_decode_kernel<T, LPR, 1><<<grid, 256, 0, s>>>(q, ldq, kc, vc, km, ws, cap, len, H, Hkv, scale); break;
    }
    return 0;
}

template <typename T>
int decode_t(hipStream_t s, const T* q, int64_t ldq, const T* kc, const T* vc, const uint8_t* km, T* out, float* ws, int B, int H, int Hkv, int Dh,
             int cap, int len, float scale) {
    const int nch = cdiv(len, DEC_CHUNK);
    switch (Dh % Elem<T>::VEC == 0 ? Dh / Elem<T>::VEC : 0) {
        case 2: launch_decode<T, 2>(s, q, ldq, kc, vc, km, ws, B, H, Hkv, cap, len, scale); break;
        case 4: launch_decode<T, 4>(s, q, ldq, kc, vc, km, ws, B, H, Hkv, cap, len, scale); break;
        case 8: launch_decode<T, 8>(s, q, ldq, kc, vc, km, ws, B, H, Hkv, cap, len, scale); break;
        case 16: launch_decode<T, 16>(s, q, ldq, kc, vc, km, ws, B, H, Hkv, cap, len, scale); break;       // head dim 128 in the 16-bit types
        case 32: launch_decode<T, 32>(s, q, ldq, kc, vc, km, ws, B, H, Hkv, cap, len, scale); break;
        default: attn_decode_any_kernel<T><<<dim3(nch, H, B), 64, 0, s>>>(q, ldq, kc, vc, km, ws, cap, len, H, Hkv, Dh, scale); break;
    }
    SETOK_CHECK_LAUNCH("setok_attention_decode(chunks)");
    attn_decode_merge_kernel<T><<<B * H, 64, 0, s>>>(ws, out, nch, H, Dh);
    SETOK_CHECK_LAUNCH("setok_attention_decode(merge)");
    return SETOK_OK;
}

// ==== the fp8 KV cache (include/setok_hip.h, "FP8 KV cache") =====================================================================================
// A cache row is Dh e4m3fn bytes + one int8 exponent and means value(q[d]) * 2^e (fp8.h: the rule of the weight path).
constexpr int F8_CHUNK = SETOK_DECODE_CHUNK_FP8KV;
constexpr int F8_WKEYS = F8_CHUNK / DEC_WAVES;             // keys per wave: 64
constexpr int F8_VEC = 16;                                 // cache elements per 16-byte load

// Maximum over aligned groups of N lanes of non-negative values, every lane of a group ending with the same bits: row_sum's exchanges.
template <int CTRL> __device__ inline float dpp_max(float a) {
    return fmaxf(a, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), CTRL, 0xf, 0xf, false)));
}
template <int N> __device__ inline float row_max(float a) {
    if constexpr (N >= 2) a = dpp_max<0xB1>(a);
    if constexpr (N >= 4) a = dpp_max<0x4E>(a);
    if constexpr (N >= 8) a = dpp_max<0x141>(a);
    if constexpr (N >= 16) a = dpp_max<0x140>(a);
#pragma unroll
    for (int o = 16; o < N; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    return a;
}

// ---- kv_append with the quantiser: one pass, a row in the registers of GL lanes (8 elements each; GL = the power of two >= Dh / 8) -------------
// Rows are numbered ((b * T + t) * 2 + which) * Hkv + hk; a workgroup takes 256 / GL of them per trip, every wave makes the same number of trips
// (the exchanges of row_max need the whole wave), lanes without a piece carry zeros and write nothing.
template <typename T, int GL>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const T* __restrict__ qkv, uint8_t* __restrict__ kq, int8_t* __restrict__ ke,
                                                            uint8_t* __restrict__ vq, int8_t* __restrict__ ve, int B, int Tn, int H, int Hkv, int Dh,
                                                            int cap, int pos0) {
    constexpr int RPB = 256 / GL;                                      // rows per workgroup and trip
    const int vpr = Dh / 8, sub = threadIdx.x % GL;
    const int64_t rows = (int64_t)B * Tn * 2 * Hkv, ld = (int64_t)(H + 2 * Hkv) * Dh;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = r0 + threadIdx.x / GL;
        const bool live = row < rows && sub < vpr;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.f;
        int which = 0;
        int64_t slot = 0;
        if (live) {
            const int hk = (int)(row % Hkv);
            which = (int)((row / Hkv) & 1);                            // 0 = k, 1 = v
            const int64_t bt = row / (2 * Hkv);
            const T* src = qkv + bt * ld + (int64_t)(H + which * Hkv + hk) * Dh + sub * 8;
#pragma unroll
            for (int u = 0; u < 8 / Elem<T>::VEC; ++u) ld_vec<T>(src + u * Elem<T>::VEC, f + u * Elem<T>::VEC);
            slot = ((bt / Tn) * Hkv + hk) * cap + pos0 + bt % Tn;
        }
        float amax = 0.f;                                              // over the finite entries; a non-finite one becomes the NaN code below
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = fabsf(f[e]);
            if (a <= 3.402823466e38f) amax = fmaxf(amax, a);
        }
        amax = row_max<GL>(amax);
        const int ex = fp8w_exponent(amax);
        const float inv = fp8w_scale(-ex);
        if (live) {
            unsigned w[2] = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned code = fabsf(f[e]) <= 3.402823466e38f ? fp8w_encode(f[e] * inv) : 0x7fu;
                w[e >> 2] |= code << (8 * (e & 3));
            }
            *reinterpret_cast<uint2*>((which ? vq : kq) + slot * Dh + sub * 8) = make_uint2(w[0], w[1]);
            if (sub == 0) (which ? ve : ke)[slot] = (int8_t)ex;
        }
    }
}

template <typename T>
void launch_append_fp8(hipStream_t s, const T* qkv, uint8_t* kq, int8_t* ke, uint8_t* vq, int8_t* ve, int B, int Tn, int H, int Hkv, int Dh, int cap,
                       int pos0) {
    const int vpr = Dh / 8;
    const int64_t rows = (int64_t)B * Tn * 2 * Hkv;
#define F8_APPEND(GL)                                                                                                          \
    if (vpr <= GL) {                                                                                                           \
        const int64_t wgs = (rows + 256 / GL - 1) / (256 / GL);                                                                \
        kv_append_fp8_kernel<T, GL><<<(int)(wgs > 65536 ? 65536 : wgs), 256, 0, s>>>(qkv, kq, ke, vq, ve, B, Tn, H, Hkv, Dh, cap, pos0); \
        return;                                                                                                                \
    }
    F8_APPEND(1) F8_APPEND(2) F8_APPEND(4) F8_APPEND(8) F8_APPEND(16) F8_APPEND(32) F8_APPEND(64)
#undef F8_APPEND
}

// ---- decode attention over the fp8 cache, a cache row spread over LPR = Dh / 16 lanes -------------------------------------------------------------
// attn_decode_kernel with fp8 rows: the same cut over (chunk, key / value head, sequence), the same order of loads (mask and exponent bytes,
// unconditionally, ahead of the K rows, ahead of the V rows, ahead of q; a sched_barrier before the first wait), the same partials.  A lane
// holds 16 elements of a row, so a load instruction covers 64 / LPR keys and a wave's slice is 64 keys: 8 + 8 loads of 16 bytes per lane at
// head dim 128, what the 16-bit kernel has in flight.  Conversion is v_cvt_pk_f32_fp8 (exact).  Scaling: 2^e of a K row multiplies the
// FINISHED dot product (before `scale`), 2^e of a V row is folded into the ROUNDED probability — both exact, so every product and sum equals
// the one over K', V'.  A slot that does not count is discarded by selection: its exponent byte is replaced by 0 before a scale is built.
template <typename T, int LPR, int GT>
__global__ __launch_bounds__(256) void attn_decode_fp8kv_kernel(const T* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ kq,
                                                                const int8_t* __restrict__ ke, const uint8_t* __restrict__ vq,
                                                                const int8_t* __restrict__ ve, const uint8_t* __restrict__ kmask,
                                                                float* __restrict__ ws, int cap, int len, int H, int Hkv, float scale) {
    constexpr int VEC = F8_VEC, DH = LPR * VEC, KPS = 64 / LPR, NSTEP = F8_WKEYS / KPS, QV = Elem<T>::VEC;
    __shared__ float red[DEC_WAVES][GT][DH + 2];
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int G = H / Hkv, npass = G / GT;
    const int hk = blockIdx.y / npass, h0 = hk * G + (blockIdx.y % npass) * GT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane / LPR, cc = lane % LPR;
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    const int jw = c * F8_CHUNK + wave * F8_WKEYS;                     // the wave's first key

    if (jw >= len) {                                                   // the whole slice lies past len: no key, nothing to load
        if (r == 0) {
#pragma unroll
            for (int g = 0; g < GT; ++g) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wave][g][2 + cc * VEC + e] = 0.f;
                if (cc == 0) { red[wave][g][0] = -INFINITY; red[wave][g][1] = 0.f; }
            }
        }
    } else {
        u32x4 kr[NSTEP], vr[NSTEP];
        uint8_t mb[NSTEP];
        int8_t ek[NSTEP], ev[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {                              // a slot at or past len is read as slot len - 1 (in bounds) and discarded
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            mb[i] = kmask[(int64_t)b * cap + jc];
            ek[i] = ke[rowbase + jc];
            ev[i] = ve[rowbase + jc];
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            kr[i] = *reinterpret_cast<const u32x4*>(kq + (rowbase + jc) * DH + cc * VEC);
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            vr[i] = *reinterpret_cast<const u32x4*>(vq + (rowbase + jc) * DH + cc * VEC);
        }
        float qf[GT][VEC];
        int cq = cc;
        if constexpr (LPR == 1) asm volatile("" : "+v"(cq));           // (head dim 16: q's address is uniform, and 16 GT scalar registers of q spill at GT = 8; keep it a vector load)
#pragma unroll
        for (int g = 0; g < GT; ++g)
#pragma unroll
            for (int u = 0; u < VEC / QV; ++u) ld_vec<T>(q + (int64_t)b * ldq + (int64_t)(h0 + g) * DH + cq * VEC + u * QV, qf[g] + u * QV);
        __builtin_amdgcn_sched_barrier(0);                             // all of the above in flight before the first wait
        bool ok[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) ok[i] = (jw + i * KPS + r < len) & (mb[i] != 0);

        float s[NSTEP][GT], m[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) m[g] = -INFINITY;
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            float kf[VEC];
            fp8w_decode16(kr[i], kf);
            const float sk = fp8w_scale(ok[i] ? (int)ek[i] : 0);       // (a dead slot's exponent byte may hold anything)
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) a = fmaf(qf[g][e], kf[e], a);
                a = row_sum<LPR>(a);
                s[i][g] = ok[i] ? a * sk * scale : -INFINITY;          // (and its codes too, the NaN code included)
                m[g] = fmaxf(m[g], s[i][g]);
            }
        }
        float l[GT], acc[GT][VEC];
#pragma unroll
        for (int g = 0; g < GT; ++g) {
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) m[g] = fmaxf(m[g], __shfl_xor(m[g], o, 64));
            l[g] = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[g][e] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            float vf[VEC];
            fp8w_decode16(vr[i], vf);
#pragma unroll
            for (int e = 0; e < VEC; ++e) vf[e] = ok[i] ? vf[e] : 0.f;
            const float sv = fp8w_scale(ok[i] ? (int)ev[i] : 0);
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                const float p = m[g] == -INFINITY ? 0.f : dec_exp<T>(s[i][g] - m[g]);
                l[g] += p;
                const float pr = rnd<T>(p) * sv;                       // the rounded probability times 2^e of the V row
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[g][e] = fmaf(pr, vf[e], acc[g][e]);
            }
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) {
                l[g] += __shfl_xor(l[g], o, 64);
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[g][e] += __shfl_xor(acc[g][e], o, 64);
            }
            if (r == 0) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) red[wave][g][2 + cc * VEC + e] = acc[g][e];
                if (cc == 0) { red[wave][g][0] = m[g]; red[wave][g][1] = l[g]; }
            }
        }
    }
    __syncthreads();
    // the chunk's partial: the four waves in wave order
    for (int idx = tid; idx < GT * DH; idx += 256) {
        const int g = idx / DH, d = idx % DH;
        float M = red[0][g][0];
#pragma unroll
        for (int w = 1; w < DEC_WAVES; ++w) M = fmaxf(M, red[w][g][0]);
        float L = 0.f, val = 0.f;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float f = red[w][g][0] == -INFINITY ? 0.f : dec_exp<T>(red[w][g][0] - M);
            L = fmaf(f, red[w][g][1], L);
            val = fmaf(f, red[w][g][2 + d], val);
        }
        float* part = ws + (((int64_t)b * H + h0 + g) * nch + c) * (DH + 2);
        part[2 + d] = val;
        if (d == 0) { part[0] = M; part[1] = L; }
    }
}

// ---- decode attention over the fp8 cache, any head dim (Dh % 8 == 0): one wave per (chunk, query head, sequence), a key per lane -----------------
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_fp8kv_any_kernel(const T* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ kq,
                                                                   const int8_t* __restrict__ ke, const uint8_t* __restrict__ vq,
                                                                   const int8_t* __restrict__ ve, const uint8_t* __restrict__ kmask,
                                                                   float* __restrict__ ws, int cap, int len, int H, int Hkv, int Dh, float scale) {
    __shared__ float ps[F8_CHUNK];
    const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, nch = gridDim.x, lane = threadIdx.x;
    const int hk = h / (H / Hkv), j0 = c * F8_CHUNK;
    const T* qr = q + (int64_t)b * ldq + (int64_t)h * Dh;
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    float mx = -INFINITY;
    for (int jj = lane; jj < F8_CHUNK; jj += 64) {
        const int j = j0 + jj;
        float sc = -INFINITY;
        if (j < len && kmask[(int64_t)b * cap + j]) {                  // (only a slot that counts is decoded and scaled)
            const uint8_t* kb = kq + (rowbase + j) * Dh;
            float a = 0.f;
            for (int d = 0; d < Dh; ++d) a = fmaf((float)qr[d], __builtin_amdgcn_cvt_pk_f32_fp8((int)kb[d], false)[0], a);
            sc = a * fp8w_scale(ke[rowbase + j]) * scale;
        }
        ps[jj] = sc;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int jj = lane; jj < F8_CHUNK; jj += 64) {
        const float e = mx == -INFINITY ? 0.f : dec_exp<T>(ps[jj] - mx);
        ps[jj] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float* part = ws + (((int64_t)b * H + h) * nch + c) * (Dh + 2);
    if (lane == 0) { part[0] = mx; part[1] = sum; }
    for (int d = lane; d < Dh; d += 64) {
        float o = 0.f;
        for (int jj = 0; jj < F8_CHUNK; ++jj)
            if (ps[jj] != 0.f)                                         // (a non-zero weight: slot < len and unmasked)
                o = fmaf(rnd<T>(ps[jj]) * fp8w_scale(ve[rowbase + j0 + jj]), __builtin_amdgcn_cvt_pk_f32_fp8((int)vq[(rowbase + j0 + jj) * Dh + d], false)[0], o);
        part[2 + d] = o;
    }
}

template <typename T, int LPR>
void launch_decode_fp8kv(hipStream_t s, const T* q, int64_t ldq, const uint8_t* kq, const int8_t* ke, const uint8_t* vq, const int8_t* ve,
                         const uint8_t* km, float* ws, int B, int H, int Hkv, int cap, int len, float scale) {
    const int G = H / Hkv, nch = cdiv(len, F8_CHUNK);
    const int GT = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
    dim3 grid(nch, Hkv * (G / GT), B);
    switch (GT) {
        case 8: attn_decode_fp8kv_kernel<T, LPR, 8><<<grid, 256, 0, s>>>(q, ldq, kq, ke, vq, ve, km, ws, cap, len, H, Hkv, scale); break;
        case 4: attn_decode_fp8kv_kernel<T, LPR, 4><<<grid, 256, 0, s>>>(q, ldq, kq, ke, vq, ve, km, ws, cap, len, H, Hkv, scale); break;
        case 2: attn_decode_fp8kv_kernel<T, LPR, 2><<<grid, 256, 0, s>>>(q, ldq, kq, ke, vq, ve, km, ws, cap, len, H, Hkv, scale); break;
        default: attn_decode_fp8kv_kernel<T, LPR, 1><<<grid, 256, 0, s>>>(q, ldq, kq, ke, vq, ve, km, ws, cap, len, H, Hkv, scale); break;
    }
}

template <typename T>
int decode_fp8kv_t(hipStream_t s, const T* q, int64_t ldq, const uint8_t* kq, const int8_t* ke, const uint8_t* vq, const int8_t* ve, const uint8_t* km,
                   T* out, float* ws, int B, int H, int Hkv, int Dh, int cap, int len, float scale) {
    const int nch = cdiv(len, F8_CHUNK);
    switch (Dh) {
        case 16: launch_decode_fp8kv<T, 1>(s, q, ldq, kq, ke, vq, ve, km, ws, B, H, Hkv, cap, len, scale); break;
        case 32: launch_decode_fp8kv<T, 2>(s, q, ldq, kq, ke, vq, ve, km, ws, B, H, Hkv, cap, len, scale); break;
        case 64: launch_decode_fp8kv<T, 4>(s, q, ldq, kq, ke, vq, ve, km, ws, B, H, Hkv, cap, len, scale); break;
        case 128: launch_decode_fp8kv<T, 8>(s, q, ldq, kq, ke, vq, ve, km, ws, B, H, Hkv, cap, len, scale); break;
        default: attn_decode_fp8kv_any_kernel<T><<<dim3(nch, H, B), 64, 0, s>>>(q, ldq, kq, ke, vq, ve, km, ws, cap, len, H, Hkv, Dh, scale); break;
    }
    SETOK_CHECK_LAUNCH("setok_attention_decode_fp8kv(chunks)");
    attn_decode_merge_kernel<T><<<B * H, 64, 0, s>>>(ws, out, nch, H, Dh);      // the native merge: the partials have the same layout
    SETOK_CHECK_LAUNCH("setok_attention_decode_fp8kv(merge)");
    return SETOK_OK;
}

}  // namespace

extern "C" int setok_kv_append_fp8(void* stream, int dtype, const void* qkv, uint8_t* k_q, int8_t* k_e, uint8_t* v_q, int8_t* v_e, int B, int T, int H,
                                   int Hkv, int Dh, int cap, int pos0) {
    SETOK_CHECK_ARG(qkv && k_q && k_e && v_q && v_e, "setok_kv_append_fp8: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_kv_append_fp8: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "setok_kv_append_fp8: bad shape B=%d T=%d H=%d Hkv=%d", B, T, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0 && Dh <= 512, "setok_kv_append_fp8: unsupported head dim %d (a multiple of 8, at most 512)", Dh);
    SETOK_CHECK_ARG(cap > 0 && pos0 >= 0 && (int64_t)pos0 + T <= cap, "setok_kv_append_fp8: slots [%d, %d + %d) exceed the cache (len > cap = %d)", pos0, pos0, T, cap);
    SETOK_CHECK_ARG(aligned16(qkv) && aligned16(k_q) && aligned16(v_q), "setok_kv_append_fp8: qkv, k_q and v_q must be 16-byte aligned");
    if (B == 0 || T == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T("setok_kv_append_fp8", (launch_append_fp8<bf16>(s, (const bf16*)qkv, k_q, k_e, v_q, v_e, B, T, H, Hkv, Dh, cap, pos0)),
               (launch_append_fp8<float>(s, (const float*)qkv, k_q, k_e, v_q, v_e, B, T, H, Hkv, Dh, cap, pos0)));
    SETOK_CHECK_LAUNCH("setok_kv_append_fp8");
    return SETOK_OK;
}

extern "C" int setok_attention_decode_gqa_fp8kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const int8_t* k_e,
                                                const uint8_t* v_q, const int8_t* v_e, const uint8_t* key_mask, void* out, int B, int H, int Hkv,
                                                int Dh, int cap, int len, float scale, float* ws, int64_t ws_floats) {
    SETOK_CHECK_ARG(q && k_q && k_e && v_q && v_e && key_mask && out && ws, "setok_attention_decode_fp8kv: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_attention_decode_fp8kv: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && Hkv > 0 && H % Hkv == 0, "setok_attention_decode_fp8kv: bad shape B=%d H=%d Hkv=%d", B, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0, "setok_attention_decode_fp8kv: unsupported head dim %d (a multiple of 8)", Dh);
    SETOK_CHECK_ARG(cap > 0 && len >= 1 && len <= cap, "setok_attention_decode_fp8kv: len = %d outside [1, cap = %d] (len > cap)", len, cap);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_q) && aligned16(v_q),
                    "setok_attention_decode_fp8kv: q rows (stride %lld) and the code caches must be 16-byte aligned", (long long)ldq);
    const int64_t need = (int64_t)B * H * cdiv(len, F8_CHUNK) * (Dh + 2);
    SETOK_CHECK_ARG(ws_floats >= need, "setok_attention_decode_fp8kv: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return decode_fp8kv_t<bf16>(s, (const bf16*)q, ldq, k_q, k_e, v_q, v_e, key_mask, (bf16*)out, ws, B, H, Hkv, Dh, cap, len, scale);
    return decode_fp8kv_t<float>(s, (const float*)q, ldq, k_q, k_e, v_q, v_e, key_mask, (float*)out, ws, B, H, Hkv, Dh, cap, len, scale);
}

extern "C" int setok_kv_append(void* stream, int dtype, const void* qkv, void* k_cache, void* v_cache, int B, int T, int H, int Hkv, int Dh, int cap,
                               int pos0) {
    SETOK_CHECK_ARG(qkv && k_cache && v_cache, "setok_kv_append: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_kv_append: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "setok_kv_append: bad shape B=%d T=%d H=%d Hkv=%d", B, T, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0, "setok_kv_append: unsupported head dim %d (a multiple of 8)", Dh);
    SETOK_CHECK_ARG(cap > 0 && pos0 >= 0 && (int64_t)pos0 + T <= cap, "setok_kv_append: slots [%d, %d + %d) exceed the cache (len > cap = %d)", pos0, pos0, T, cap);
    SETOK_CHECK_ARG(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache), "setok_kv_append: operands must be 16-byte aligned");
    if (B == 0 || T == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)B * T * 2 * Hkv * (Dh / (dtype == SETOK_F32 ? 4 : 8));
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    DISPATCH_T("setok_kv_append",
               (kv_append_kernel<bf16><<<blocks, 256, 0, s>>>((const bf16*)qkv, (bf16*)k_cache, (bf16*)v_cache, B, T, H, Hkv, Dh, cap, pos0)),
               (kv_append_kernel<float><<<blocks, 256, 0, s>>>((const float*)qkv, (float*)k_cache, (float*)v_cache, B, T, H, Hkv, Dh, cap, pos0)));
    SETOK_CHECK_LAUNCH("setok_kv_append");
    return SETOK_OK;
}

extern "C" int setok_attention_decode_gqa(void* stream, int dtype, const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                          const uint8_t* key_mask, void* out, int B, int H, int Hkv, int Dh, int cap, int len, float scale, float* ws,
                                          int64_t ws_floats) {
    SETOK_CHECK_ARG(q && k_cache && v_cache && key_mask && out && ws, "setok_attention_decode: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_attention_decode: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && Hkv > 0 && H % Hkv == 0, "setok_attention_decode: bad shape B=%d H=%d Hkv=%d", B, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0, "setok_attention_decode: unsupported head dim %d (a multiple of 8)", Dh);
    SETOK_CHECK_ARG(cap > 0 && len >= 1 && len <= cap, "setok_attention_decode: len = %d outside [1, cap = %d] (len > cap)", len, cap);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_cache) && aligned16(v_cache),
                    "setok_attention_decode: q rows (stride %lld) and the caches must be 16-byte aligned", (long long)ldq);
    const int64_t need = (int64_t)B * H * cdiv(len, DEC_CHUNK) * (Dh + 2);
    SETOK_CHECK_ARG(ws_floats >= need, "setok_attention_decode: workspace of %lld floats, %lld needed", (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return decode_t<bf16>(s, (const bf16*)q, ldq, (const bf16*)k_cache, (const bf16*)v_cache, key_mask, (bf16*)out, ws, B, H, Hkv, Dh, cap, len, scale);
    return decode_t<float>(s, (const float*)q, ldq, (const float*)k_cache, (const float*)v_cache, key_mask, (float*)out, ws, B, H, Hkv, Dh, cap, len, scale);
}

extern "C" int setok_argmax_rows(void* stream, int dtype, const void* x, int64_t ld, int rows, int V, int64_t* out) {
    SETOK_CHECK_ARG(x && out, "setok_argmax_rows: null operand");
    SETOK_CHECK_ARG(rows >= 0 && V > 0 && ld >= V, "setok_argmax_rows: bad shape rows=%d V=%d ld=%lld", rows, V, (long long)ld);
    hipStream_t s = (hipStream_t)stream;
    if (rows == 0) {
        SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_argmax_rows: bad dtype %d", dtype);
        return SETOK_OK;
    }
    DISPATCH_T("setok_argmax_rows", (argmax_rows_kernel<bf16><<<rows, 256, 0, s>>>((const bf16*)x, ld, V, out)),
               (argmax_rows_kernel<float><<<rows, 256, 0, s>>>((const float*)x, ld, V, out)));
    SETOK_CHECK_LAUNCH("setok_argmax_rows");
    return SETOK_OK;
}
