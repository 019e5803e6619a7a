// attn_decode.hip — KV-cached greedy generation: what one decoding step of HuggingFace Llama needs beyond the prefill's entries
// (SetokimLlamaForCausalLM.generate, src/model/language_model/setokim_llama.py:329-396, decodes with `past_key_values`, :99,133,189).
//   setok_kv_append             the post-rotary k / v columns of a fused [q | k | v] buffer -> slots [pos0, pos0 + T) of a (B, Hkv, cap, Dh) cache
//   setok_attention_decode_gqa  one query row per (sequence, query head) against the cached keys / values: eager_attention_forward for one new token
//   setok_argmax_rows           greedy selection on the device (lowest index of the row maximum)
//   setok_kv_append_fp8, setok_attention_decode_gqa_fp8kv   the same two over a cache stored as e4m3fn rows with a power-of-two exponent per row
//                               (the same decode kernel over the KvFp8 format of attn_partials.h)
//   setok_kv_append_mxfp4, setok_attention_decode_gqa_mxfp4kv   and over a cache stored as OCP MXFP4 rows: e2m1 nibbles with one e8m0 scale byte per
//                               32 elements (the same decode kernel over the KvMxfp4 format)
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
#include "mx4.h"
#include "attn_partials.h"
#include <type_traits>

namespace {

constexpr int DEC_CHUNK = SETOK_DECODE_CHUNK;
constexpr int DEC_WAVES = 4;                              // a wave's slice is CHUNK / 4 keys: 32 native (NSTEP = LPR / 2 below), 64 over e4m3 rows

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
// chunk) Dh + 2 floats [max, sum, accumulators].  F is the cache's format (attn_partials.h): a lane holds F::VEC elements of a row, so a load
// instruction covers 64 / LPR keys and a wave's slice is F::CHUNK / 4 keys — 32 native, 64 over e4m3 rows: 8 + 8 loads of 16 bytes per lane at head
// dim 128 either way; over nibble rows 64 keys again, 8 + 8 loads of 8 bytes and as many scale bytes (the lane budget: DESIGN.md §7 f16).  Scaling of an e4m3 row: 2^e of a K row multiplies the FINISHED dot product (before `scale`), 2^e of a V row is folded into
// the ROUNDED probability — both exact, so every product and sum equals the one over K', V'.  A slot that does not count is discarded by selection:
// its exponent byte is replaced by 0 before a scale is built.
template <typename T, typename F, int LPR, int GT>
__global__ __launch_bounds__(256) void attn_decode_kernel(const T* __restrict__ q, int64_t ldq, F kv, const uint8_t* __restrict__ kmask,
                                                          float* __restrict__ ws, int cap, int len, int H, int Hkv, float scale) {
    constexpr int VEC = F::VEC, DH = LPR * VEC, KPS = 64 / LPR, WKEYS = F::CHUNK / DEC_WAVES, NSTEP = WKEYS / KPS, QV = Elem<T>::VEC;
    static_assert(WKEYS % KPS == 0 && NSTEP >= 1, "a wave's slice is a whole number of load steps");
    typedef typename F::Raw V16;
    __shared__ float red[DEC_WAVES][GT][DH + 2];
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int G = H / Hkv, npass = G / GT;
    const int hk = blockIdx.y / npass, h0 = hk * G + (blockIdx.y % npass) * GT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane / LPR, cc = lane % LPR;
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    const int jw = c * F::CHUNK + wave * WKEYS;                        // the wave's first key

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
        // (the mask and exponent bytes first: loads return in order, and a score must not have to wait for the V rows issued behind its K row)
        V16 kr[NSTEP], vr[NSTEP];
        uint8_t mb[NSTEP];
        int8_t ek[NSTEP], ev[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            mb[i] = kmask[(int64_t)b * cap + jc];                         // (unconditional: a load behind a branch is waited for on the spot)
            if constexpr (F::SCALED) {
                ek[i] = kv.ke[rowbase + jc];
                ev[i] = kv.ve[rowbase + jc];
            }
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            kr[i] = F::load(kv.k, (rowbase + jc) * DH + cc * VEC);
        }
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            const int j = jw + i * KPS + r, jc = j < len ? j : len - 1;
            vr[i] = F::load(kv.v, (rowbase + jc) * DH + cc * VEC);
        }
        float qf[GT][VEC];
        int cq = cc;
        if constexpr (LPR == 1) asm volatile("" : "+v"(cq));           // (head dim 16 over e4m3 rows: q's address is uniform, and 16 GT scalar registers of q spill at GT = 8; keep it a vector load)
#pragma unroll
        for (int g = 0; g < GT; ++g)
#pragma unroll
            for (int u = 0; u < VEC / QV; ++u) ld_vec<T>(q + (int64_t)b * ldq + (int64_t)(h0 + g) * DH + cq * VEC + u * QV, qf[g] + u * QV);
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
            F::decode(kr[i], kf);
            float sk = 0.f;
            if constexpr (F::SCALED) sk = fp8w_scale(ok[i] ? (int)ek[i] : 0);      // (a dead slot's exponent byte may hold anything)
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) a = fmaf(qf[g][e], kf[e], a);
                a = row_sum<LPR>(a);                                              // over the row's LPR lanes: every lane ends with the same bits
                if constexpr (F::SCALED) s[i][g] = ok[i] ? a * sk * scale : -INFINITY;      // (and its codes too, the NaN code included)
                else s[i][g] = ok[i] ? a * scale : -INFINITY;
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
            F::decode(vr[i], vf);
#pragma unroll
            for (int e = 0; e < VEC; ++e) vf[e] = ok[i] ? vf[e] : 0.f;                // (a masked slot may hold anything, NaN included)
            float sv = 0.f;
            if constexpr (F::SCALED) sv = fp8w_scale(ok[i] ? (int)ev[i] : 0);
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                const float p = m[g] == -INFINITY ? 0.f : dec_exp<T>(s[i][g] - m[g]);
                l[g] += p;
                float pr = rnd<T>(p);                                                 // probabilities cast to the element type (HF)
                if constexpr (F::SCALED) pr = pr * sv;                                // the rounded probability times 2^e of the V row
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

template <typename T, typename F, int LPR>
void launch_decode(hipStream_t s, const T* q, int64_t ldq, F kv, const uint8_t* km, float* ws, int B, int H, int Hkv, int cap, int len, float scale) {
    const int G = H / Hkv, nch = cdiv(len, F::CHUNK);
    const int GT = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
    dim3 grid(nch, Hkv * (G / GT), B);
    switch (GT) {
        case 8: attn_decode_kernel<T, F, LPR, 8><<<grid, 256, 0, s>>>(q, ldq, kv, km, ws, cap, len, H, Hkv, scale); break;
        case 4: attn_decode_kernel<T, F, LPR, 4><<<grid, 256, 0, s>>>(q, ldq, kv, km, ws, cap, len, H, Hkv, scale); break;
        case 2: attn_decode_kernel<T, F, LPR, 2><<<grid, 256, 0, s>>>(q, ldq, kv, km, ws, cap, len, H, Hkv, scale); break;
        default: attn_decode_kernel<T, F, LPR, 1><<<grid, 256, 0, s>>>(q, ldq, kv, km, ws, cap, len, H, Hkv, scale); break;
    }
}

// Both entry points (`name`: the entry point's, for its messages).  A head dim with a lane layout takes the chunk kernel — over e4m3 rows head dims
// 16 / 32 / 64 / 128, over nibble rows 32 / 64 / 128, native every LPR = Dh / VEC in {2, ..., 32} — and every other one the wave-per-chunk kernel
// of attn_partials.h.
template <typename T, typename F>
int decode_t(const char* name, hipStream_t s, const T* q, int64_t ldq, F kv, const uint8_t* km, T* out, float* ws, int B, int H, int Hkv, int Dh, int cap,
             int len, float scale) {
    const int nch = cdiv(len, F::CHUNK);
    auto any = [&] { attn_chunk_any_kernel<T, F, F::CHUNK, false><<<dim3(nch, H, B), 64, 0, s>>>(q, ldq, kv, km, ws, 1, H, Hkv, Dh, cap, len - 1, scale); };
#define DEC_LPR(N) launch_decode<T, F, N>(s, q, ldq, kv, km, ws, B, H, Hkv, cap, len, scale); break
    if constexpr (std::is_same<F, KvMxfp4>::value) {                   // 16 elements per lane
        switch (Dh) {
            case 32: DEC_LPR(2);
            case 64: DEC_LPR(4);
            case 128: DEC_LPR(8);
            default: any(); break;
        }
    } else if constexpr (F::SCALED) {
        switch (Dh) {
            case 16: DEC_LPR(1);
            case 32: DEC_LPR(2);
            case 64: DEC_LPR(4);
            case 128: DEC_LPR(8);
            default: any(); break;
        }
    } else {
        switch (Dh % F::VEC == 0 ? Dh / F::VEC : 0) {
            case 2: DEC_LPR(2);
            case 4: DEC_LPR(4);
            case 8: DEC_LPR(8);
            case 16: DEC_LPR(16);                                      // head dim 128 in the 16-bit types
            case 32: DEC_LPR(32);
            default: any(); break;
        }
    }
#undef DEC_LPR
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(chunks): %s", name, hipGetErrorString(e));
    attn_decode_merge_kernel<T><<<B * H, 64, 0, s>>>(ws, out, nch, H, Dh);      // one merge: the partials have the same layout in both formats
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(merge): %s", name, hipGetErrorString(e));
    return SETOK_OK;
}

// What both decode entry points require of their arguments; `caches` is how the entry point's alignment message calls its K / V operands.
int check_decode(const char* name, const char* caches, bool operands, bool aligned, int dtype, int64_t ldq, int B, int H, int Hkv, int Dh, int cap, int len,
                 int chunk, int64_t ws_floats) {
    SETOK_CHECK_ARG(operands, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && Hkv > 0 && H % Hkv == 0, "%s: bad shape B=%d H=%d Hkv=%d", name, B, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0, "%s: unsupported head dim %d (a multiple of 8)", name, Dh);
    SETOK_CHECK_ARG(cap > 0 && len >= 1 && len <= cap, "%s: len = %d outside [1, cap = %d] (len > cap)", name, len, cap);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned, "%s: q rows (stride %lld) and the %s must be 16-byte aligned", name, (long long)ldq,
                    caches);
    const int64_t need = (int64_t)B * H * cdiv(len, chunk) * (Dh + 2);
    SETOK_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed", name, (long long)ws_floats, (long long)need);
    return SETOK_OK;
}

// ==== filling the fp8 KV cache (include/setok_hip.h, "FP8 KV cache") ==============================================================================
// A cache row is Dh e4m3fn bytes + one int8 exponent and means value(q[d]) * 2^e (fp8.h: the rule of the weight path).

// ---- kv_append with the quantiser: one pass, a row in the registers of GL lanes (8 elements each; GL = the power of two >= Dh / 8) -------------
// Rows are numbered ((b * T + t) * 2 + which) * Hkv + hk; a workgroup takes 256 / GL of them per trip, every wave makes the same number of trips
// (the exchanges of row_max — attn_partials.h — need the whole wave), lanes without a piece carry zeros and write nothing.  The MXFP4 quantiser,
// which the paged cache shares, is kv_append_mxfp4_kernel in attn_partials.h.
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
    const char* name = "setok_attention_decode_fp8kv";
    if (int e = check_decode(name, "code caches", q && k_q && k_e && v_q && v_e && key_mask && out && ws, aligned16(q) && aligned16(k_q) && aligned16(v_q),
                             dtype, ldq, B, H, Hkv, Dh, cap, len, KvFp8::CHUNK, ws_floats))
        return e;
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const KvFp8 kv{k_q, k_e, v_q, v_e};
    if (dtype == SETOK_BF16) return decode_t<bf16>(name, s, (const bf16*)q, ldq, kv, key_mask, (bf16*)out, ws, B, H, Hkv, Dh, cap, len, scale);
    return decode_t<float>(name, s, (const float*)q, ldq, kv, key_mask, (float*)out, ws, B, H, Hkv, Dh, cap, len, scale);
}

extern "C" int setok_kv_append_mxfp4(void* stream, int dtype, const void* qkv, uint8_t* k_q, uint8_t* k_s, uint8_t* v_q, uint8_t* v_s, int B, int T, int H,
                                     int Hkv, int Dh, int cap, int pos0) {
    SETOK_CHECK_ARG(qkv && k_q && k_s && v_q && v_s, "setok_kv_append_mxfp4: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_kv_append_mxfp4: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0, "setok_kv_append_mxfp4: bad shape B=%d T=%d H=%d Hkv=%d", B, T, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 32 == 0 && Dh <= 512, "setok_kv_append_mxfp4: unsupported head dim %d (a multiple of 32, the MX block, at most 512)", Dh);
    SETOK_CHECK_ARG(cap > 0 && pos0 >= 0 && (int64_t)pos0 + T <= cap, "setok_kv_append_mxfp4: slots [%d, %d + %d) exceed the cache (len > cap = %d)", pos0, pos0, T, cap);
    SETOK_CHECK_ARG(aligned16(qkv) && aligned16(k_q) && aligned16(v_q), "setok_kv_append_mxfp4: qkv, k_q and v_q must be 16-byte aligned");
    if (B == 0 || T == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T("setok_kv_append_mxfp4", (launch_append_mxfp4<bf16>(s, (const bf16*)qkv, k_q, k_s, v_q, v_s, B, T, H, Hkv, Dh, Mx4ToDense{cap, pos0})),
               (launch_append_mxfp4<float>(s, (const float*)qkv, k_q, k_s, v_q, v_s, B, T, H, Hkv, Dh, Mx4ToDense{cap, pos0})));
    SETOK_CHECK_LAUNCH("setok_kv_append_mxfp4");
    return SETOK_OK;
}

extern "C" int setok_attention_decode_gqa_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                                  const uint8_t* v_q, const uint8_t* v_s, const uint8_t* key_mask, void* out, int B, int H, int Hkv,
                                                  int Dh, int cap, int len, float scale, float* ws, int64_t ws_floats) {
    const char* name = "setok_attention_decode_mxfp4kv";
    SETOK_CHECK_ARG(Dh > 0 && Dh % 32 == 0, "%s: unsupported head dim %d (a multiple of 32, the MX block)", name, Dh);
    if (int e = check_decode(name, "nibble caches", q && k_q && k_s && v_q && v_s && key_mask && out && ws, aligned16(q) && aligned16(k_q) && aligned16(v_q),
                             dtype, ldq, B, H, Hkv, Dh, cap, len, KvMxfp4::CHUNK, ws_floats))
        return e;
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const KvMxfp4 kv{{k_q, k_s}, {v_q, v_s}};
    if (dtype == SETOK_BF16) return decode_t<bf16>(name, s, (const bf16*)q, ldq, kv, key_mask, (bf16*)out, ws, B, H, Hkv, Dh, cap, len, scale);
    return decode_t<float>(name, s, (const float*)q, ldq, kv, key_mask, (float*)out, ws, B, H, Hkv, Dh, cap, len, scale);
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
    const char* name = "setok_attention_decode";
    if (int e = check_decode(name, "caches", q && k_cache && v_cache && key_mask && out && ws, aligned16(q) && aligned16(k_cache) && aligned16(v_cache), dtype,
                             ldq, B, H, Hkv, Dh, cap, len, DEC_CHUNK, ws_floats))
        return e;
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return decode_t<bf16>(name, s, (const bf16*)q, ldq, KvNative<bf16>{(const bf16*)k_cache, (const bf16*)v_cache}, key_mask, (bf16*)out, ws, B, H, Hkv, Dh,
                              cap, len, scale);
    return decode_t<float>(name, s, (const float*)q, ldq, KvNative<float>{(const float*)k_cache, (const float*)v_cache}, key_mask, (float*)out, ws, B, H, Hkv,
                           Dh, cap, len, scale);
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
