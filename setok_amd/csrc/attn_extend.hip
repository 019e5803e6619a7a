// attn_extend.hip — extending a filled KV cache by Tn >= 1 tokens per sequence (include/setok_hip.h, "Extending a cache"): chunked prefill, a
// second turn of a conversation, scoring several candidate tokens in one pass.  HF LlamaAttention.forward with `past_key_values` on a Tn-token input.
//   setok_attention_extend_gqa   Tn query rows per (sequence, query head) against the cached keys / values, causal inside the new rows
// Query i of sequence b counts slot j iff j <= len0 + i and key_mask[b][j] != 0; a query with no counted key gets zeros.
//
// What attn_decode.hip established carries over:
//   - the keys are cut into chunks of SETOK_EXTEND_CHUNK slots counted from slot 0; every chunk writes fp32 partials (max, sum, Dh accumulators) per
//     (sequence, query row, query head, chunk) and the decode path's merge launch (attn_partials.h) combines them in chunk order with (b * Tn + i)
//     as its "sequence".  No atomics, no hand-off between workgroups; a row's summation order depends on len0, Tn, i and the mask alone.  With
//     more than 32 stacked rows (G * Tn > 32: a chunked prefill, a turn) a workgroup of the MFMA kernel carries its online softmax across
//     XSPAN consecutive chunks before it writes a partial — a rule in G * Tn alone: the partials, Dh + 2 floats per row and chunk, are otherwise the
//     call's largest traffic once a sequence brings hundreds of rows (measured at Tn = 512: DESIGN.md §7 f10);
//   - K / V are read once per group: the G = H / Hkv query heads of a group and the Tn query rows are stacked into the M dimension (row m = i * G + g,
//     so that a row's causal limit len0 + m / G grows with m and whole key tiles can be skipped per wave).
// Head dim 128 in the 16-bit type is attn_causal_kernel's arrangement (llama.hip) read from the cache: 32-key tiles of contiguous 256-byte rows go to
// LDS by LDS-DMA (K XOR-swizzled through the source address, V row-major for the transposing reads), a wave keeps 32 (group x query) rows in
// registers across the chunk, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_32x32x16 with the online softmax per lane.  The probabilities are
// rounded to the element type by the operand pack, the normaliser sums the unrounded values.  A slot that counts for no query may hold anything:
// its scores are replaced by selection and its V row is zeroed in LDS before the tile is used (0 * NaN would reach the accumulators otherwise).
// Everything else (fp32, other head dims) is one wave per (query row, query head, chunk) on a grid (B * Tn, H, chunks): attn_chunk_any_kernel of
// attn_partials.h, the decode path's fallback, with the row's own limit len0 + i + 1.
//   setok_attention_extend_gqa_mxfp4kv   the same over a cache stored as MXFP4 rows (include/setok_hip.h, "MXFP4 KV cache"), with the native call's
//                                        dispatch.  Head dim 128 in the 16-bit type: the MFMA kernel, the same text, under the staging policy
//                                        StageMx4 (attn_partials.h) — a thread loads MX blocks (16 bytes of nibbles + the e8m0 byte) of tile
//                                        kt + 1 into registers before tile kt's MFMAs and, after them, converts them with the hardware converter
//                                        (v_cvt_scalef32_pk_*_fp4: exact, the scale applied) and writes the 64 bytes into the LDS image the native
//                                        staging fills by LDS-DMA; the V rows of slots that cannot count are written as zeros there, which saves
//                                        the native staging's extra pass and barrier.  Everything from S^T = K Q^T to the partial is the native
//                                        kernel's, operation for operation: the output bits are setok_attention_extend_gqa's over a cache that
//                                        holds K', V' (DESIGN.md §7 f16).  Everything else: that wave-per-chunk kernel over the KvMxfp4 format.
#include "common.h"
#include "lds_mma.h"
#include "attn_partials.h"

namespace {

constexpr int EXT_CHUNK = SETOK_EXTEND_CHUNK;
constexpr int XD = 128;                  // head dim of the MFMA kernel
constexpr int XROW = XD * 2;             // bytes per K / V row, in the cache and in LDS
constexpr int XT = 32;                   // keys per tile
constexpr int XSPAN = SETOK_EXTEND_SPAN;  // chunks per partial of the MFMA kernel when G * Tn > 32
static_assert(EXT_CHUNK % XT == 0, "a chunk is a whole number of key tiles");

typedef __attribute__((ext_vector_type(2))) float f32x2;

// ---- 16-bit MFMA kernel, head dim 128 -------------------------------------------------------------------------------------------------------------
// grid (spans, Hkv * mblocks, B), NW waves of 32 M rows each (mblocks = ceil(G * Tn / (32 NW))); NW = 1 serves a verify-shaped call (G * Tn <= 32).
// A workgroup owns `span` slots (EXT_CHUNK, or XSPAN chunks) counted from slot 0 and writes one partial per row.
// S (attn_partials.h): how a tile reaches LDS — StageDma from native rows kc / vc, StageMx4 from MXFP4 rows (nibbles, scales) through registers.
template <int NW, typename S>
__global__ __launch_bounds__(NW * 64) void attn_extend_kernel(const bf16* __restrict__ q, int64_t ldq, typename S::Rows kc, typename S::Rows vc,
                                                              const uint8_t* __restrict__ kmask, float* __restrict__ ws, int Tn, int H, int Hkv, int cap,
                                                              int len0, int span, float scale_log2e) {
    constexpr int NT = NW * 64, PP = (XT * 16) / NT;                     // a tile is 512 pieces of 16 B: PP per thread
    __shared__ __attribute__((aligned(16))) char Ks[2][XT * XROW];       // K tile, 16-byte slots XOR-swizzled by (row & 15)
    __shared__ __attribute__((aligned(16))) char Vs[2][XT * XROW];       // V tile, row-major (hardware-transposing reads)
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int G = H / Hkv, MR = G * Tn, mblocks = (MR + NW * 32 - 1) / (NW * 32);
    const int hk = (int)blockIdx.y / mblocks, mb = (int)blockIdx.y % mblocks;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, hi = lane >> 5;
    const int m0 = (mb * NW + wave) * 32;                                // this wave's first row of the stacked (query, group head) rows
    const bool live = m0 < MR;                                           // (wave-uniform) a wave without rows still stages and meets the barriers
    const int m = min(m0 + qi, MR - 1), i = m / G, h = hk * G + m % G;
    const int lim = len0 + i;                                            // the last slot this row may count
    const int lim_lo = len0 + min(m0, MR - 1) / G, lim_hi = len0 + min(m0 + 31, MR - 1) / G;        // of the wave's first and last row
    const int lim_wg = len0 + min(mb * NW * 32 + NW * 32 - 1, MR - 1) / G;                           // of the workgroup's last row
    const int top = len0 + Tn;                                           // slots below `top` hold keys (<= cap); nothing at or above it is ever read
    const int kbeg = c * span, kend = min(kbeg + span, lim_wg + 1);
    const int nkt = kend > kbeg ? (kend - kbeg + XT - 1) / XT : 0;       // (workgroup-uniform) 0: the span lies wholly above this workgroup's rows
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    const uint8_t* km = kmask + (int64_t)b * cap;

    const bf16* qp = q + ((int64_t)b * Tn + i) * ldq + (int64_t)h * XD + hi * 8;
    bf16x8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
    f32x16 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    constexpr float NEG = -1.0e30f;                                      // finite sentinel: a row may meet only slots that do not count first
    float m_run = NEG, l_run = 0.f;                                      // the running maximum in units of log2 (scores * scale * log2 e)
    const int g16 = lane >> 4, i16 = lane & 15;
    const int tr_row = (i16 >> 2) + 4 * (g16 >> 1);
    const int tr_col = (g16 & 1) * 16 + (i16 & 3) * 4;
    const unsigned klds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)&Ks[0][0]) + wave * 1024;
    const unsigned vlds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)&Vs[0][0]) + wave * 1024;
    unsigned koffs[PP], voffs[PP];
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int p = u * NT + tid, row = p >> 4, pc = p & 15;
        koffs[u] = (unsigned)(row * XROW + ((pc ^ (row & 15)) << 4));    // physical slot pc of a row holds logical piece pc ^ (row & 15)
        voffs[u] = (unsigned)(row * XROW + (pc << 4));
    }
    // the tile's slots that can count at all, as a 32-bit set (bit j: slot k0 + j lies below `top` and is attended): the same in every wave
    auto countable = [&](int k0) { return (unsigned)__ballot(lane < 32 && k0 + lane < top && km[min(k0 + lane, top - 1)] != 0); };
    Mx4Tile<NT> tile = {};                                               // (StageMx4) the requested tile in registers, the mask byte of its slot
    unsigned kmb = 0u, kb_next = 0u;                                     // (lane & 31) as it was loaded, and — from commit() on — its set of slots
    auto stage = [&](int k0, int buf) {                                  // K and V rows [k0, k0 + 32) of the (sequence, key / value head) -> LDS buffer buf
        if constexpr (S::MX4) {                                          // requested into registers; commit() puts them into the image
            tile.request(kc, vc, rowbase + k0, min(XT, top - k0) - 1, tid);              // k0 < top always (k0 < kend <= lim_wg + 1 <= top)
            kmb = km[min(k0 + (lane & 31), top - 1)];                    // no use before commit(): nothing waits for these loads until then
        } else {
            if (k0 + XT <= top) {                                        // (uniform) all 32 slots lie below `top`
                const char* kb = reinterpret_cast<const char*>(kc + (rowbase + k0) * XD);
                const char* vb = reinterpret_cast<const char*>(vc + (rowbase + k0) * XD);
#pragma unroll
                for (int u = 0; u < PP; ++u) {
                    lds_dma16_sbase(kb, koffs[u], klds + buf * (XT * XROW) + u * (NT * 16));
                    lds_dma16_sbase(vb, voffs[u], vlds + buf * (XT * XROW) + u * (NT * 16));
                }
                return;
            }
#pragma unroll
            for (int u = 0; u < PP; ++u) {                               // a slot at or above `top` is read as slot top - 1 (in bounds) and discarded
                const int p = u * NT + tid, row = p >> 4, pc = p & 15;
                const int64_t src = (rowbase + min(k0 + row, top - 1)) * XD;
                lds_dma16(kc + src + ((pc ^ (row & 15)) << 3), klds + buf * (XT * XROW) + u * (NT * 16));
                lds_dma16(vc + src + (pc << 3), vlds + buf * (XT * XROW) + u * (NT * 16));
            }
        }
    };
    auto commit = [&](int k0, int buf) {                                 // (StageMx4) the requested tile k0 -> LDS buffer buf, the V rows of dead slots as zeros
        if constexpr (S::MX4) {
            kb_next = (unsigned)__ballot(lane < 32 && k0 + lane < top && kmb != 0u);     // countable(k0)
            tile.commit(&Ks[buf][0], &Vs[buf][0], kb_next, true, tid);
        }
    };
    if (nkt > 0) { stage(kbeg, 0); commit(kbeg, 0); }
    // (StageMx4) vmcnt(0), as an instruction the compiler's own wait counting sees: q has arrived on every path into the loop, so no wait for a q
    // fragment inside it also waits for the tile loads that were just requested.
    if constexpr (S::MX4) __builtin_amdgcn_s_waitcnt(0x0f70);
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        if constexpr (!S::MX4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this thread's pieces of tile kt (StageMx4: the barrier waits for its LDS writes)
        __syncthreads();                                                 // everyone's; everyone is done with the other buffer
        const int k0 = kbeg + kt * XT;
        const unsigned kb_cur = kb_next;                                 // (StageMx4) this tile's set, found when it was requested
        const bool more = kt + 1 < nkt;
        if (more) stage(k0 + XT, buf ^ 1);
        unsigned kbits;
        if constexpr (S::MX4) {
            kbits = kb_cur;                                              // commit() wrote zeros for the V rows of the other slots
        } else {
            kbits = countable(k0);
            if (kbits != 0xffffffffu) {                                  // (workgroup-uniform) zero the V rows of the other slots: they may hold anything
#pragma unroll
                for (int u = 0; u < PP; ++u) {
                    const int p = u * NT + tid;
                    if (!((kbits >> (p >> 4)) & 1u)) *reinterpret_cast<f32x4*>(&Vs[buf][p * 16]) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                __syncthreads();
            }
        }
        if (!live || k0 > lim_hi) {                                      // wave-uniform: no rows, or the whole tile lies in this wave's future
            if (more) commit(k0 + XT, buf ^ 1);
            continue;
        }
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const char* Kb = &Ks[buf][0];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kb + qi * XROW + (((ks * 2 + hi) ^ (qi & 15)) << 4));
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
        }
        float t[16];
        float mx = NEG;
        const bool diag = k0 + XT - 1 > lim_lo;                          // some slot of the tile may lie after some row of the wave
        const bool plain = !diag && kbits == 0xffffffffu;                // (wave-uniform) every slot of the tile counts for every row of the wave
        if (plain) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { t[r] = s[r] * scale_log2e; mx = fmaxf(mx, t[r]); }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;          // slot index inside the tile
                t[r] = (((kbits >> kj) & 1u) && k0 + kj <= lim) ? s[r] * scale_log2e : NEG;       // by selection: a discarded score may be NaN
                mx = fmaxf(mx, t[r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        if (!__all(m_new == m_run)) {
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            l_run *= alpha;
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
            m_run = m_new;
        }
        float ls = 0.f;
        if (plain) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { t[r] = __builtin_amdgcn_exp2f(t[r] - m_run); ls += t[r]; }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) { t[r] = t[r] <= NEG ? 0.f : __builtin_amdgcn_exp2f(t[r] - m_run); ls += t[r]; }
        }
        l_run += ls;
        const bf16x8 p0 = pack8(t), p1 = pack8(t + 8);                   // the probabilities rounded to the element type (HF's rounding point)
        const char* Vb = &Vs[buf][0];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                const char* va = Vb + (k2 * 16 + tr_row) * XROW + (d * 32 + tr_col) * 2;
                o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_read_tr16(va, va + 8 * XROW), k2 == 0 ? p0 : p1, o[d], 0, 0, 0);
            }
        }
        if (more) commit(k0 + XT, buf ^ 1);                                       // after this tile's MFMAs: the loads had their time
    }
    // the chunk's partial of every row: [max (natural-log units, what the merge rescales by), sum, 128 accumulators]; a row that counted no slot of the
    // chunk writes (-inf, 0, zeros)
    if (m0 + qi < MR) {
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const bool any = m_run > NEG;
        float* part = ws + ((((int64_t)b * Tn + i) * H + h) * nch + c) * (XD + 2);
        if (hi == 0) *reinterpret_cast<f32x2*>(part) = f32x2{any ? m_run * 0.69314718055994530942f : -INFINITY, any ? l_tot : 0.f};
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                float* dst = part + 2 + d * 32 + 8 * r4 + 4 * hi;
                *reinterpret_cast<f32x2*>(dst) = f32x2{any ? o[d][r4 * 4] : 0.f, any ? o[d][r4 * 4 + 1] : 0.f};
                *reinterpret_cast<f32x2*>(dst + 2) = f32x2{any ? o[d][r4 * 4 + 2] : 0.f, any ? o[d][r4 * 4 + 3] : 0.f};
            }
    }
}

static_assert(XD == 128 && XSPAN * EXT_CHUNK == SETOK_EXTEND_SPAN * SETOK_EXTEND_CHUNK, "extend_span (attn_partials.h) states this kernel's span rule");

// The MFMA kernel's launch for either staging: NW = 1 serves G * Tn <= 32 stacked rows, NW = 4 everything else; `nch` partials per row.
template <typename S>
void launch_extend_mfma(hipStream_t s, const bf16* q, int64_t ldq, typename S::Rows kc, typename S::Rows vc, const uint8_t* km, float* ws, int B, int Tn,
                        int H, int Hkv, int cap, int len0, int span, int nch, float scale) {
    const int MR = (H / Hkv) * Tn;
    const float sl = scale * 1.44269504088896340736f;
    if (MR <= 32) attn_extend_kernel<1, S><<<dim3(nch, Hkv, B), 64, 0, s>>>(q, ldq, kc, vc, km, ws, Tn, H, Hkv, cap, len0, span, sl);
    else attn_extend_kernel<4, S><<<dim3(nch, Hkv * cdiv(MR, 128), B), 256, 0, s>>>(q, ldq, kc, vc, km, ws, Tn, H, Hkv, cap, len0, span, sl);
}

template <typename T>
int extend_t(hipStream_t s, const T* q, int64_t ldq, const T* kc, const T* vc, const uint8_t* km, T* out, float* ws, int B, int Tn, int H, int Hkv, int Dh,
             int cap, int len0, float scale) {
    const int span = extend_span(sizeof(T) == 2, Tn, H, Hkv, Dh), nch = cdiv(len0 + Tn, span);
    if (sizeof(T) == 2 && Dh == XD) {
        launch_extend_mfma<StageDma>(s, (const bf16*)q, ldq, (const bf16*)kc, (const bf16*)vc, km, ws, B, Tn, H, Hkv, cap, len0, span, nch, scale);
    } else {
        attn_chunk_any_kernel<T, KvNative<T>, EXT_CHUNK, true><<<dim3(B * Tn, H, nch), 64, 0, s>>>(q, ldq, KvNative<T>{kc, vc}, km, ws, Tn, H, Hkv, Dh, cap, len0,
                                                                                               scale);
    }
    SETOK_CHECK_LAUNCH("setok_attention_extend(chunks)");
    attn_decode_merge_kernel<T><<<B * Tn * H, 64, 0, s>>>(ws, out, nch, H, Dh);      // the decode path's merge with (b * Tn + i) as its sequence
    SETOK_CHECK_LAUNCH("setok_attention_extend(merge)");
    return SETOK_OK;
}

// Over an MXFP4 cache: the native call's dispatch and partition.  16-bit at head dim 128: the MFMA kernel staged from nibbles, `span` slots per
// partial (a prefix of the workspace, whose rule stays one partial per chunk); everything else the wave-per-chunk kernel, one partial per chunk.
template <typename T>
int extend_mxfp4_t(hipStream_t s, const T* q, int64_t ldq, KvMxfp4 kv, const uint8_t* km, T* out, float* ws, int B, int Tn, int H, int Hkv, int Dh, int cap,
                   int len0, float scale) {
    const int span = extend_span(sizeof(T) == 2, Tn, H, Hkv, Dh), nch = cdiv(len0 + Tn, span);
    if (sizeof(T) == 2 && Dh == XD) {
        launch_extend_mfma<StageMx4>(s, (const bf16*)q, ldq, kv.k, kv.v, km, ws, B, Tn, H, Hkv, cap, len0, span, nch, scale);
    } else {
        attn_chunk_any_kernel<T, KvMxfp4, EXT_CHUNK, true><<<dim3(B * Tn, H, nch), 64, 0, s>>>(q, ldq, kv, km, ws, Tn, H, Hkv, Dh, cap, len0, scale);
    }
    SETOK_CHECK_LAUNCH("setok_attention_extend_mxfp4kv(chunks)");
    attn_decode_merge_kernel<T><<<B * Tn * H, 64, 0, s>>>(ws, out, nch, H, Dh);
    SETOK_CHECK_LAUNCH("setok_attention_extend_mxfp4kv(merge)");
    return SETOK_OK;
}

}  // namespace

extern "C" int64_t setok_attention_extend_workspace(int dtype, int B, int Tn, int H, int Hkv, int Dh, int len0) {
    if (B < 0 || Tn < 1 || H < 1 || Hkv < 1 || H % Hkv != 0 || Dh < 1 || len0 < 0) return 0;
    return (int64_t)B * Tn * H * (((int64_t)len0 + Tn + extend_span(dtype == SETOK_BF16, Tn, H, Hkv, Dh) - 1) / extend_span(dtype == SETOK_BF16, Tn, H, Hkv, Dh)) * (Dh + 2);
}

extern "C" int setok_attention_extend_gqa(void* stream, int dtype, const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                                          const uint8_t* key_mask, void* out, int B, int Tn, int H, int Hkv, int Dh, int cap, int len0, float scale,
                                          float* workspace, int64_t workspace_floats) {
    SETOK_CHECK_ARG(q && k_cache && v_cache && key_mask && out && workspace, "setok_attention_extend: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_attention_extend: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && Tn >= 1 && H > 0 && H <= 65535 && Hkv > 0 && H % Hkv == 0,
                    "setok_attention_extend: bad shape B=%d Tn=%d H=%d Hkv=%d", B, Tn, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 8 == 0, "setok_attention_extend: unsupported head dim %d (a multiple of 8)", Dh);
    SETOK_CHECK_ARG(cap > 0 && len0 >= 0 && (int64_t)len0 + Tn <= cap, "setok_attention_extend: slots [%d, %d + %d) exceed the cache (len0 + Tn > cap = %d)",
                    len0, len0, Tn, cap);
    SETOK_CHECK_ARG((int64_t)B * Tn * H <= 0x7fffffffll && (int64_t)Hkv * cdiv((H / Hkv) * Tn, 128) <= 65535 && cdiv(len0 + Tn, EXT_CHUNK) <= 65535,
                    "setok_attention_extend: B=%d Tn=%d H=%d len0=%d exceed the launch grid", B, Tn, H, len0);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_cache) && aligned16(v_cache),
                    "setok_attention_extend: q rows (stride %lld) and the caches must be 16-byte aligned", (long long)ldq);
    SETOK_CHECK_ARG(((uintptr_t)workspace & 7u) == 0, "setok_attention_extend: the workspace must be 8-byte aligned");
    const int64_t need = setok_attention_extend_workspace(dtype, B, Tn, H, Hkv, Dh, len0);
    SETOK_CHECK_ARG(workspace_floats >= need, "setok_attention_extend: workspace of %lld floats, %lld needed", (long long)workspace_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return extend_t<bf16>(s, (const bf16*)q, ldq, (const bf16*)k_cache, (const bf16*)v_cache, key_mask, (bf16*)out, workspace, B, Tn, H, Hkv, Dh, cap, len0,
                              scale);
    return extend_t<float>(s, (const float*)q, ldq, (const float*)k_cache, (const float*)v_cache, key_mask, (float*)out, workspace, B, Tn, H, Hkv, Dh, cap, len0,
                           scale);
}

extern "C" int64_t setok_attention_extend_mxfp4kv_workspace(int B, int Tn, int H, int Dh, int len0) {
    if (B < 0 || Tn < 1 || H < 1 || Dh < 1 || len0 < 0) return 0;
    return (int64_t)B * Tn * H * (((int64_t)len0 + Tn + EXT_CHUNK - 1) / EXT_CHUNK) * (Dh + 2);
}

extern "C" int setok_attention_extend_gqa_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                                  const uint8_t* v_q, const uint8_t* v_s, const uint8_t* key_mask, void* out, int B, int Tn, int H,
                                                  int Hkv, int Dh, int cap, int len0, float scale, float* workspace, int64_t workspace_floats) {
    SETOK_CHECK_ARG(q && k_q && k_s && v_q && v_s && key_mask && out && workspace, "setok_attention_extend_mxfp4kv: null operand");
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_attention_extend_mxfp4kv: bad dtype %d", dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && Tn >= 1 && H > 0 && H <= 65535 && Hkv > 0 && H % Hkv == 0,
                    "setok_attention_extend_mxfp4kv: bad shape B=%d Tn=%d H=%d Hkv=%d", B, Tn, H, Hkv);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 32 == 0, "setok_attention_extend_mxfp4kv: unsupported head dim %d (a multiple of 32, the MX block)", Dh);
    SETOK_CHECK_ARG(cap > 0 && len0 >= 0 && (int64_t)len0 + Tn <= cap,
                    "setok_attention_extend_mxfp4kv: slots [%d, %d + %d) exceed the cache (len0 + Tn > cap = %d)", len0, len0, Tn, cap);
    SETOK_CHECK_ARG((int64_t)B * Tn <= 0x7fffffffll && cdiv(len0 + Tn, EXT_CHUNK) <= 65535,
                    "setok_attention_extend_mxfp4kv: B=%d Tn=%d H=%d len0=%d exceed the launch grid", B, Tn, H, len0);
    SETOK_CHECK_ARG(!(dtype == SETOK_BF16 && Dh == XD) || ((int64_t)(H / Hkv) * Tn + 127) / 128 * Hkv <= 65535,
                    "setok_attention_extend_mxfp4kv: Tn=%d H=%d Hkv=%d exceed the launch grid of the MFMA kernel (Hkv * ceil(G * Tn / 128) <= 65535)", Tn, H, Hkv);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_q) && aligned16(v_q),
                    "setok_attention_extend_mxfp4kv: q rows (stride %lld) and the nibble caches must be 16-byte aligned", (long long)ldq);
    const int64_t need = setok_attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0);
    SETOK_CHECK_ARG(workspace_floats >= need, "setok_attention_extend_mxfp4kv: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                    (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const KvMxfp4 kv{{k_q, k_s}, {v_q, v_s}};
    if (dtype == SETOK_BF16) return extend_mxfp4_t<bf16>(s, (const bf16*)q, ldq, kv, key_mask, (bf16*)out, workspace, B, Tn, H, Hkv, Dh, cap, len0, scale);
    return extend_mxfp4_t<float>(s, (const float*)q, ldq, kv, key_mask, (float*)out, workspace, B, Tn, H, Hkv, Dh, cap, len0, scale);
}
