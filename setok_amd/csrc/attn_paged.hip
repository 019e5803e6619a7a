// attn_paged.hip — the paged KV cache: one layer's keys / values live in pools of pages and a sequence is a row of a block table (entry p: the
// page that holds its slots [128 p, 128 p + 128)) plus a length of its own.  Two pool formats (attn_partials.h): the element type — two pools
// (num_pages, Hkv, SETOK_KV_PAGE, Dh) — and MXFP4 — nibble pools (…, Dh / 2) and scale pools (…, Dh / 32), a row meaning what a row of the dense
// MXFP4 cache means.
//   setok_kv_append_paged                     the post-rotary k / v columns of a fused [q | k | v] buffer -> slots [slot0[b], slot0[b] + T) of sequence b
//   setok_attention_decode_gqa_paged          one query row per (sequence, query head) against the sequence's own lens[b] slots, found through the table
//   setok_kv_append_paged_mxfp4, setok_attention_decode_gqa_paged_mxfp4kv     the same two over MXFP4 pools
//
// The kernel below is attn_decode_kernel (attn_decode.hip) over the format F with two things replaced — where a wave's rows start (a table entry
// instead of b * Hkv * cap) and where `len` comes from (lens[b] instead of an argument) — and no mask bytes: the same wave slices, row_sum,
// rounding point of the probabilities, wave-order reduction and (attn_partials.h: merge_chunks) merge.  So a sequence's output bits are those of
// the dense entry of the same format on its slots gathered into a dense cache with an all-ones mask, wherever its pages lie.
//
// A chunk of the decode attention is F::CHUNK slots: one page in the native format (SETOK_KV_PAGE == SETOK_DECODE_CHUNK), TWO over nibble rows
// (SETOK_DECODE_CHUNK_MXFP4KV = 256).  Either way a wave's slice — a quarter of the chunk, 32 or 64 keys — lies inside one page, so the page is
// looked up per wave: over nibble rows waves 0-1 of chunk c read table entry 2c, waves 2-3 entry 2c + 1.  A wave reads its entry only if its slice
// starts below the sequence's length and the entry lies inside the table row (entry 2c + 1 may not, at an odd max_pages).
//
// A page id outside [0, num_pages) means "no page": the append writes nothing for such a row, the attention counts no key of such a page, and
// neither forms an address from the id.
#include "common.h"
#include "attn_partials.h"
#include <type_traits>

static_assert(SETOK_KV_PAGE == SETOK_DECODE_CHUNK, "native pools: a page is one chunk of the decode attention, a chunk's workgroup reads exactly one page");
static_assert(SETOK_DECODE_CHUNK_MXFP4KV == 2 * SETOK_KV_PAGE, "MXFP4 pools: a chunk's workgroup covers two pages, a wave's slice of 64 slots lies in one");

namespace {

constexpr int PAGE = SETOK_KV_PAGE;
constexpr int DEC_WAVES = 4;                              // as in attn_decode.hip: a wave's slice is F::CHUNK / 4 keys, 32 native and 64 over nibble rows

// ---- kv_append through the table --------------------------------------------------------------------------------------------------------------
// kv_append_kernel's enumeration of 16-byte pieces; the destination row is page table[b][slot / PAGE], row slot % PAGE.  Nothing is written for a
// sequence with slot0[b] < 0, for a slot past the table's max_pages entries and for a page id outside [0, num_pages).
template <typename T>
__global__ __launch_bounds__(256) void kv_append_paged_kernel(const T* __restrict__ qkv, T* __restrict__ kp, T* __restrict__ vp,
                                                              const int* __restrict__ table, int max_pages, int num_pages,
                                                              const int* __restrict__ slot0, int B, int Tn, int H, int Hkv, int Dh) {
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
        const int s0 = slot0[b];
        if (s0 < 0) continue;                                          // an idle row of the running batch
        const int64_t slot = (int64_t)s0 + t, pi = slot / PAGE;
        if (pi >= max_pages) continue;
        const int page = table[(int64_t)b * max_pages + pi];
        if (page < 0 || page >= num_pages) continue;                   // no page: nothing is written, no address is formed
        const V16 v = *reinterpret_cast<const V16*>(qkv + row * ld + (int64_t)(H + which * Hkv + hk) * Dh + p * VEC);
        T* dst = (which ? vp : kp) + (((int64_t)page * Hkv + hk) * PAGE + (int)(slot % PAGE)) * Dh + p * VEC;
        *reinterpret_cast<V16*>(dst) = v;
    }
}

// ---- decode attention, a chunk of F::CHUNK slots per workgroup, a row spread over LPR lanes ---------------------------------------------------
// grid (chunks of max_len, Hkv * (G / GT), B).  kv: the pools in the format F, a pool row where a cache row was.  The slice of wave w of chunk c — slots
// [jw, jw + WKEYS), jw = c * F::CHUNK + w * WKEYS, inside page entry jw / PAGE — holds keys iff jw < lens[b] and that entry lies in the table row and is a
// page; otherwise the wave writes the empty partial, loads nothing from the pools and — a slice at or past the sequence's length, or an entry at or
// past max_pages — does not read the table either.
template <typename T, typename F, int LPR, int GT>
__global__ __launch_bounds__(256) void attn_decode_paged_kernel(const T* __restrict__ q, int64_t ldq, F kv, const int* __restrict__ table, int max_pages,
                                                                int num_pages, const int* __restrict__ lens, float* __restrict__ ws, int H, int Hkv,
                                                                float scale) {
    constexpr int VEC = F::VEC, DH = LPR * VEC, KPS = 64 / LPR, WKEYS = F::CHUNK / DEC_WAVES, NSTEP = WKEYS / KPS, QV = Elem<T>::VEC;
    static_assert(WKEYS % KPS == 0 && NSTEP >= 1, "a wave's slice is a whole number of load steps");
    static_assert(!F::SCALED && F::CHUNK % PAGE == 0 && PAGE % WKEYS == 0, "no exponent per row; a chunk is whole pages and a wave's slice lies in one page");
    typedef typename F::Raw V16;
    __shared__ float red[DEC_WAVES][GT][DH + 2];
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int G = H / Hkv, npass = G / GT;
    const int hk = blockIdx.y / npass, h0 = hk * G + (blockIdx.y % npass) * GT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane / LPR, cc = lane % LPR;
    const int jw = c * F::CHUNK + wave * WKEYS;                        // the wave's first key
    const int pi = jw / PAGE;                                          // (wave-uniform) the table entry of the wave's slice: c natively, 2c + wave / 2 over nibble rows
    int len = lens[b], page = 0;
    if (jw < len) {
        page = pi < max_pages ? table[(int64_t)b * max_pages + pi] : -1;               // an entry at or past max_pages is not read: no page
        if (page < 0 || page >= num_pages) { page = 0; len = 0; }      // no page: no key of this slice counts
    }
    const int64_t rowbase = ((int64_t)page * Hkv + hk) * PAGE - (int64_t)pi * PAGE;    // slot j of the wave's page is row rowbase + j of the pool

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
        // every K and V load of the wave's slice is issued here, before the first use; a slot at or past len is read as slot len - 1 (the same page: jw < len) and discarded
        V16 kr[NSTEP], vr[NSTEP];
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
#pragma unroll
        for (int g = 0; g < GT; ++g)
#pragma unroll
            for (int u = 0; u < VEC / QV; ++u) ld_vec<T>(q + (int64_t)b * ldq + (int64_t)(h0 + g) * DH + cc * VEC + u * QV, qf[g] + u * QV);
        __builtin_amdgcn_sched_barrier(0);                                // all of the above in flight before the first wait: hipcc otherwise sinks the loads to their uses
        bool ok[NSTEP];
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) ok[i] = jw + i * KPS + r < len;

        float s[NSTEP][GT], m[GT];
#pragma unroll
        for (int g = 0; g < GT; ++g) m[g] = -INFINITY;
#pragma unroll
        for (int i = 0; i < NSTEP; ++i) {
            float kf[VEC];
            F::decode(kr[i], kf);
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
            F::decode(vr[i], vf);
#pragma unroll
            for (int e = 0; e < VEC; ++e) vf[e] = ok[i] ? vf[e] : 0.f;                // (a slot past len may hold anything, NaN included)
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

// ---- merge: the dense merge's loop over the sequence's own ceil(lens[b] / chunk) chunks (at most the launch's nch: lens[b] <= max_len is the caller's promise) ----
template <typename T>
__global__ __launch_bounds__(64) void attn_decode_merge_paged_kernel(const float* __restrict__ ws, T* __restrict__ out, const int* __restrict__ lens,
                                                                     int nch, int chunk, int H, int Dh) {
    const int64_t bh = blockIdx.x;                                     // b * H + h; out rows are H * Dh wide
    const int len = lens[bh / H];
    int n = len <= 0 ? 0 : (len - 1) / chunk + 1;
    n = n < nch ? n : nch;
    merge_chunks<T>(ws + bh * nch * (Dh + 2), out + bh * Dh, n, Dh);
}

template <typename T, typename F, int LPR>
void launch_decode_paged(hipStream_t s, const T* q, int64_t ldq, F kv, const int* table, int max_pages, int num_pages, const int* lens, float* ws, int B,
                         int H, int Hkv, int nch, float scale) {
    const int G = H / Hkv;
    const int GT = G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
    dim3 grid(nch, Hkv * (G / GT), B);
#define PAGED_GT(N) attn_decode_paged_kernel<T, F, LPR, N><<<grid, 256, 0, s>>>(q, ldq, kv, table, max_pages, num_pages, lens, ws, H, Hkv, scale); break
    switch (GT) {
        case 8: PAGED_GT(8);
        case 4: PAGED_GT(4);
        case 2: PAGED_GT(2);
        default: PAGED_GT(1);
    }
#undef PAGED_GT
}

// Both decode entries (`name`: the entry's, for its messages).  The head dim has a lane layout in F: the entry checked it (paged_head_dim, paged_mxfp4_head_dim).
template <typename T, typename F>
int decode_paged_t(const char* name, hipStream_t s, const T* q, int64_t ldq, F kv, const int* table, int max_pages, int num_pages, const int* lens, T* out,
                   float* ws, int B, int H, int Hkv, int Dh, int max_len, float scale) {
    const int nch = cdiv(max_len, F::CHUNK);
    if (nch > 0) {                                                     // (max_len == 0: every sequence is empty, the merge alone writes the zeros)
#define PAGED_LPR(N) launch_decode_paged<T, F, N>(s, q, ldq, kv, table, max_pages, num_pages, lens, ws, B, H, Hkv, nch, scale); break
        if constexpr (std::is_same<F, KvMxfp4>::value) {               // 16 elements per lane: attn_decode.hip's three lane layouts over nibble rows
            switch (Dh) {
                case 32: PAGED_LPR(2);
                case 64: PAGED_LPR(4);
                default: PAGED_LPR(8);
            }
        } else {
            switch (Dh / F::VEC) {
                case 2: PAGED_LPR(2);
                case 4: PAGED_LPR(4);
                case 8: PAGED_LPR(8);
                case 16: PAGED_LPR(16);                                // head dim 128 in the 16-bit types
                default: PAGED_LPR(32);
            }
        }
#undef PAGED_LPR
        if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(chunks): %s", name, hipGetErrorString(e));
    }
    attn_decode_merge_paged_kernel<T><<<B * H, 64, 0, s>>>(ws, out, lens, nch, F::CHUNK, H, Dh);
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(merge): %s", name, hipGetErrorString(e));
    return SETOK_OK;
}

}  // namespace

extern "C" int setok_kv_append_paged(void* stream, int dtype, const void* qkv, void* k_pool, void* v_pool, const int32_t* block_table, int max_pages,
                                     int num_pages, const int32_t* slot0, int B, int T, int H, int Hkv, int Dh) {
    SETOK_CHECK_ARG(qkv && k_pool && v_pool && block_table && slot0, "setok_kv_append_paged: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_kv_append_paged: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "setok_kv_append_paged: bad shape B=%d T=%d H=%d Hkv=%d max_pages=%d num_pages=%d", B, T, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(paged_head_dim(dtype, Dh), "setok_kv_append_paged: unsupported head dim %d (16-byte pieces per row in {2, 4, 8, 16, 32})", Dh);
    SETOK_CHECK_ARG(aligned16(qkv) && aligned16(k_pool) && aligned16(v_pool), "setok_kv_append_paged: qkv and the pools must be 16-byte aligned");
    if (B == 0 || T == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)B * T * 2 * Hkv * (Dh / (dtype == SETOK_F32 ? 4 : 8));
    const int blocks = (int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    DISPATCH_T("setok_kv_append_paged",
               (kv_append_paged_kernel<bf16><<<blocks, 256, 0, s>>>((const bf16*)qkv, (bf16*)k_pool, (bf16*)v_pool, block_table, max_pages, num_pages, slot0,
                                                                   B, T, H, Hkv, Dh)),
               (kv_append_paged_kernel<float><<<blocks, 256, 0, s>>>((const float*)qkv, (float*)k_pool, (float*)v_pool, block_table, max_pages, num_pages,
                                                                    slot0, B, T, H, Hkv, Dh)));
    SETOK_CHECK_LAUNCH("setok_kv_append_paged");
    return SETOK_OK;
}

extern "C" int setok_attention_decode_gqa_paged(void* stream, int dtype, const void* q, int64_t ldq, const void* k_pool, const void* v_pool,
                                                const int32_t* block_table, int max_pages, int num_pages, const int32_t* lens, void* out, int B, int H,
                                                int Hkv, int Dh, int max_len, float scale, float* ws, int64_t ws_floats) {
    const char* name = "setok_attention_decode_paged";
    SETOK_CHECK_ARG(q && k_pool && v_pool && block_table && lens && out && ws, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "%s: bad shape B=%d H=%d Hkv=%d max_pages=%d num_pages=%d", name, B, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(paged_head_dim(dtype, Dh), "%s: unsupported head dim %d (16-byte pieces per row in {2, 4, 8, 16, 32}: no paged twin of the generic kernel)",
                    name, Dh);
    SETOK_CHECK_ARG(max_len >= 0 && (int64_t)max_len <= (int64_t)max_pages * PAGE, "%s: max_len = %d outside [0, max_pages = %d * %d slots] (beyond the table)",
                    name, max_len, max_pages, PAGE);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_pool) && aligned16(v_pool),
                    "%s: q rows (stride %lld) and the pools must be 16-byte aligned", name, (long long)ldq);
    const int64_t need = (int64_t)B * H * cdiv(max_len, PAGE) * (Dh + 2);
    SETOK_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed", name, (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return decode_paged_t<bf16>(name, s, (const bf16*)q, ldq, KvNative<bf16>{(const bf16*)k_pool, (const bf16*)v_pool}, block_table, max_pages, num_pages,
                                    lens, (bf16*)out, ws, B, H, Hkv, Dh, max_len, scale);
    return decode_paged_t<float>(name, s, (const float*)q, ldq, KvNative<float>{(const float*)k_pool, (const float*)v_pool}, block_table, max_pages,
                                 num_pages, lens, (float*)out, ws, B, H, Hkv, Dh, max_len, scale);
}

extern "C" int setok_kv_append_paged_mxfp4(void* stream, int dtype, const void* qkv, uint8_t* k_q, uint8_t* k_s, uint8_t* v_q, uint8_t* v_s,
                                           const int32_t* block_table, int max_pages, int num_pages, const int32_t* slot0, int B, int T, int H, int Hkv,
                                           int Dh) {
    const char* name = "setok_kv_append_paged_mxfp4";
    SETOK_CHECK_ARG(qkv && k_q && k_s && v_q && v_s && block_table && slot0, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && T >= 0 && H > 0 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "%s: bad shape B=%d T=%d H=%d Hkv=%d max_pages=%d num_pages=%d", name, B, T, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(paged_mxfp4_head_dim(Dh), "%s: unsupported head dim %d (32, 64 or 128: the lane layouts of the decode attention over nibble rows)", name, Dh);
    SETOK_CHECK_ARG(aligned16(qkv) && aligned16(k_q) && aligned16(v_q), "%s: qkv and the nibble pools must be 16-byte aligned", name);
    if (B == 0 || T == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const Mx4ToPages dest{block_table, slot0, max_pages, num_pages};
    DISPATCH_T("setok_kv_append_paged_mxfp4", (launch_append_mxfp4<bf16>(s, (const bf16*)qkv, k_q, k_s, v_q, v_s, B, T, H, Hkv, Dh, dest)),
               (launch_append_mxfp4<float>(s, (const float*)qkv, k_q, k_s, v_q, v_s, B, T, H, Hkv, Dh, dest)));
    SETOK_CHECK_LAUNCH(name);
    return SETOK_OK;
}

extern "C" int setok_attention_decode_gqa_paged_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                                        const uint8_t* v_q, const uint8_t* v_s, const int32_t* block_table, int max_pages, int num_pages,
                                                        const int32_t* lens, void* out, int B, int H, int Hkv, int Dh, int max_len, float scale, float* ws,
                                                        int64_t ws_floats) {
    const char* name = "setok_attention_decode_paged_mxfp4kv";
    SETOK_CHECK_ARG(q && k_q && k_s && v_q && v_s && block_table && lens && out && ws, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && H > 0 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "%s: bad shape B=%d H=%d Hkv=%d max_pages=%d num_pages=%d", name, B, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(paged_mxfp4_head_dim(Dh), "%s: unsupported head dim %d (32, 64 or 128: no paged twin of the generic kernel)", name, Dh);
    SETOK_CHECK_ARG(max_len >= 0 && (int64_t)max_len <= (int64_t)max_pages * PAGE, "%s: max_len = %d outside [0, max_pages = %d * %d slots] (beyond the table)",
                    name, max_len, max_pages, PAGE);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_q) && aligned16(v_q),
                    "%s: q rows (stride %lld) and the nibble pools must be 16-byte aligned", name, (long long)ldq);
    const int64_t need = (int64_t)B * H * cdiv(max_len, KvMxfp4::CHUNK) * (Dh + 2);
    SETOK_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed", name, (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const KvMxfp4 kv{{k_q, k_s}, {v_q, v_s}};
    if (dtype == SETOK_BF16)
        return decode_paged_t<bf16>(name, s, (const bf16*)q, ldq, kv, block_table, max_pages, num_pages, lens, (bf16*)out, ws, B, H, Hkv, Dh, max_len, scale);
    return decode_paged_t<float>(name, s, (const float*)q, ldq, kv, block_table, max_pages, num_pages, lens, (float*)out, ws, B, H, Hkv, Dh, max_len, scale);
}
