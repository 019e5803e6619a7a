// attn_extend_paged.hip — extending sequences of the paged KV cache by Tn >= 1 tokens each (include/setok_hip.h, "Paged extend attention"): a request
// that starts behind a shared prefix, and what a verify pass or a prefill window over pages will need.
//   setok_attention_extend_gqa_paged          Tn query rows per (sequence, query head) against the sequence's own len0[b] + Tn slots, found through the table
//   setok_attention_extend_gqa_paged_mxfp4kv  the same over MXFP4 pools (attn_paged.hip), with the native call's dispatch: head dim 128 in the 16-bit
//                                             type is the MFMA kernel below under the staging policy StageMx4 (attn_partials.h; attn_extend.hip says
//                                             what it does), everything else (every Dh % 32 == 0, fp32) the wave-per-chunk kernel over KvMxfp4
// Query i of sequence b counts slot j iff j <= len0[b] + i and table[b][j / SETOK_KV_PAGE] is a page; len0[b] < 0 is an idle sequence (zeros).
//
// These are attn_extend.hip's two kernels with two things replaced, as attn_decode_paged_kernel did it for decode — where a tile's rows start (a table
// entry and (page * Hkv + hk) * PAGE + k0 % PAGE instead of (b * Hkv + hk) * cap + k0) and where len0 comes from (len0[b] instead of an argument) —
// and no mask bytes: a page that is "no page" is what a mask that is zero on its 128 slots is to the dense kernel.  The dense kernel's key tiles are
// 32 slots counted from slot 0, its chunks 256 and its spans 1024, so a tile never straddles a page and chunks and spans are whole pages: the same
// partition into partials, the same online softmax per tile, the same merge in chunk order (attn_partials.h).  So a sequence's output bits are those
// of setok_attention_extend_gqa (over MXFP4 pools: of setok_attention_extend_gqa_mxfp4kv, whose partition is the same on either of its paths) at B = 1,
// len0 = len0[b], on its slots gathered into a dense cache, wherever its pages lie.
//
// No address is formed from a page id outside [0, num_pages), nor from a table index at or past max_pages: such a tile is not staged and no key of
// it counts.  With that, every pool address lies inside a page the table names and every table address inside the sequence's row.
#include "common.h"
#include "lds_mma.h"
#include "attn_partials.h"

static_assert(SETOK_KV_PAGE % 32 == 0 && SETOK_EXTEND_CHUNK % SETOK_KV_PAGE == 0, "a key tile lies in one page; chunks and spans are whole pages");

namespace {

constexpr int PAGE = SETOK_KV_PAGE;
constexpr int EXT_CHUNK = SETOK_EXTEND_CHUNK;
constexpr int XD = 128;                  // head dim of the MFMA kernel
constexpr int XROW = XD * 2;             // bytes per K / V row, in the pools and in LDS
constexpr int XT = 32;                   // keys per tile

typedef __attribute__((ext_vector_type(2))) float f32x2;

// ---- 16-bit MFMA kernel, head dim 128: attn_extend_kernel<NW> over pages ---------------------------------------------------------------------------
// grid (spans of max_len0 + Tn, Hkv * mblocks, B).  An idle sequence and a span at or above the sequence's own top write nothing: the merge reads
// neither.  Every other workgroup writes one partial per row, exactly the dense kernel's.
// S (attn_partials.h): how a tile reaches LDS — StageDma from native pools kp / vp, StageMx4 from MXFP4 pools (nibbles, scales) through registers.
template <int NW, typename S>
__global__ __launch_bounds__(NW * 64) void attn_extend_paged_kernel(const bf16* __restrict__ q, int64_t ldq, typename S::Rows kp, typename S::Rows vp,
                                                                    const int* __restrict__ table, int max_pages, int num_pages,
                                                                    const int* __restrict__ lens0, float* __restrict__ ws, int Tn, int H, int Hkv, int span,
                                                                    float scale_log2e) {
    constexpr int NT = NW * 64, PP = (XT * 16) / NT;                     // a tile is 512 pieces of 16 B: PP per thread
    __shared__ __attribute__((aligned(16))) char Ks[2][XT * XROW];       // K tile, 16-byte slots XOR-swizzled by (row & 15)
    __shared__ __attribute__((aligned(16))) char Vs[2][XT * XROW];       // V tile, row-major (hardware-transposing reads)
    const int c = blockIdx.x, b = blockIdx.z, nch = gridDim.x;
    const int len0 = lens0[b];
    if (len0 < 0 || c * span >= len0 + Tn) return;                       // (workgroup-uniform) idle, or a span past the sequence: nothing is read or written
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
    const int top = len0 + Tn;                                           // slots below `top` hold keys; nothing at or above it is ever read
    const int kbeg = c * span, kend = min(kbeg + span, lim_wg + 1);
    const int nkt = kend > kbeg ? (kend - kbeg + XT - 1) / XT : 0;       // (workgroup-uniform) 0: the span lies wholly above this workgroup's rows
    const int* trow = table + (int64_t)b * max_pages;

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
    // K and V rows [k0, k0 + 32) of the (sequence, key / value head) -> LDS buffer buf; false, with nothing requested, if the tile's page is no page.
    // k0 < top always (k0 < kend <= lim_wg + 1 <= top), and the tile lies in ONE page (k0 % 32 == 0, PAGE % 32 == 0): row j of the tile is row
    // (page * Hkv + hk) * PAGE + k0 % PAGE + j of the pool, below the page's PAGE rows.
    // the tile's slots that can count at all, as a 32-bit set (bit j: slot k0 + j lies below `top`; none without a page): the same in every wave
    auto countable = [&](int k0, bool paged) { return paged ? (unsigned)__ballot(lane < 32 && k0 + lane < top) : 0u; };
    Mx4Tile<NT> tile = {};                                               // (StageMx4) the requested tile in registers and, from commit() on, its set of slots
    unsigned kb_next = 0u;
    auto stage = [&](int k0, int buf) -> bool {
        const int pi = k0 / PAGE;                                        // (workgroup-uniform, like everything up to the requests)
        const int page = pi < max_pages ? trow[pi] : -1;                 // one uniform load per tile; an index past the row is no page
        if (page < 0 || page >= num_pages) {                             // no page: no address is formed from the id
            return false;
        }
        const int64_t tilebase = ((int64_t)page * Hkv + hk) * PAGE + k0 % PAGE;
        if constexpr (S::MX4) {                                          // requested into registers; commit() puts them into the image.  Tile rows
            tile.request(kp, vp, tilebase, min(XT, top - k0) - 1, tid);  // above slot top - 1 are read as that slot of THIS tile: inside its page
            return true;
        } else {
            if (k0 + XT <= top) {                                        // (uniform) all 32 slots lie below `top`
                const char* kb = reinterpret_cast<const char*>(kp + tilebase * XD);
                const char* vb = reinterpret_cast<const char*>(vp + tilebase * XD);
#pragma unroll
                for (int u = 0; u < PP; ++u) {
                    lds_dma16_sbase(kb, koffs[u], klds + buf * (XT * XROW) + u * (NT * 16));
                    lds_dma16_sbase(vb, voffs[u], vlds + buf * (XT * XROW) + u * (NT * 16));
                }
                return true;
            }
            // a slot at or above `top` is read as slot top - 1 and discarded.  k0 < top <= k0 + 31 here, so slot top - 1 is a slot of THIS tile: the
            // clamped read stays inside the tile's own page, which is what keeps every address in bounds.
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const int p = u * NT + tid, row = p >> 4, pc = p & 15;
                const int64_t src = (tilebase + min(row, top - 1 - k0)) * XD;
                lds_dma16(kp + src + ((pc ^ (row & 15)) << 3), klds + buf * (XT * XROW) + u * (NT * 16));
                lds_dma16(vp + src + (pc << 3), vlds + buf * (XT * XROW) + u * (NT * 16));
            }
            return true;
        }
    };
    bool paged_next = false;                                             // (workgroup-uniform) was the tile about to be used staged from a page?
    auto commit = [&](int k0, int buf) {                                 // (StageMx4) the requested tile k0 -> LDS buffer buf, the V rows of dead slots as zeros
        if constexpr (S::MX4) {
            kb_next = countable(k0, paged_next);
            tile.commit(&Ks[buf][0], &Vs[buf][0], kb_next, paged_next, tid);
        }
    };
    if (nkt > 0) { paged_next = stage(kbeg, 0); commit(kbeg, 0); }
    // (StageMx4) vmcnt(0), as an instruction the compiler's own wait counting sees: q has arrived on every path into the loop, so no wait for a q
    // fragment inside it also waits for the tile loads that were just requested.
    if constexpr (S::MX4) __builtin_amdgcn_s_waitcnt(0x0f70);
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        const bool paged = paged_next;
        if constexpr (!S::MX4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this thread's pieces of tile kt (StageMx4: the barrier waits for its LDS writes)
        __syncthreads();                                                 // everyone's; everyone is done with the other buffer
        const int k0 = kbeg + kt * XT;
        const unsigned kb_cur = kb_next;                                 // (StageMx4) this tile's set, found when it was requested
        const bool more = kt + 1 < nkt;
        if (more) paged_next = stage(k0 + XT, buf ^ 1);
        unsigned kbits;
        if constexpr (S::MX4) {
            kbits = kb_cur;                                              // commit() wrote zeros for the V rows of the other slots
        } else {
            kbits = countable(k0, paged);
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
    // the span's partial of every row, as the dense kernel writes it; a row that counted no slot of the span writes (-inf, 0, zeros)
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

// ---- every other case: attn_chunk_any_kernel (attn_partials.h) over pages, one wave per (query row, query head, chunk), a key per lane -------------
// grid (B * Tn, H, chunks of max_len0 + Tn).  Only a slot that counts is read: below the row's own limit, in a page.  A chunk is EXT_CHUNK / PAGE
// whole pages, whose ids the wave loads once.  kv: the pools in the format F (attn_partials.h), read an element at a time as attn_chunk_any_kernel does.
template <typename T, typename F>
__global__ __launch_bounds__(64) void attn_chunk_paged_kernel(const T* __restrict__ q, int64_t ldq, F kv, const int* __restrict__ table, int max_pages,
                                                              int num_pages, const int* __restrict__ lens0, float* __restrict__ ws, int Tn, int H, int Hkv,
                                                              int Dh, float scale) {
    constexpr int CHUNK = EXT_CHUNK, NPG = CHUNK / PAGE;
    static_assert(!F::SCALED, "no exponent per row: the e4m3 format has no extend attention");
    __shared__ float ps[CHUNK];
    const int row = blockIdx.x, h = blockIdx.y, c = blockIdx.z, nch = gridDim.z, lane = threadIdx.x;
    const int b = row / Tn, len0 = lens0[b];
    const int j0 = c * CHUNK;
    if (len0 < 0 || j0 >= len0 + Tn) return;                           // idle, or a chunk past the sequence: the merge reads no partial of it
    const int len = len0 + row % Tn + 1;                               // this row counts slots below len
    const int hk = h / (H / Hkv);
    const T* qr = q + (int64_t)row * ldq + (int64_t)h * Dh;
    int64_t pbase[NPG];                                                // first pool row of the chunk's pages for this key / value head; -1: no page
#pragma unroll
    for (int u = 0; u < NPG; ++u) {
        const int pi = j0 / PAGE + u;
        const int page = pi < max_pages && pi * PAGE < len ? table[(int64_t)b * max_pages + pi] : -1;
        pbase[u] = page >= 0 && page < num_pages ? ((int64_t)page * Hkv + hk) * PAGE : -1;
    }
    auto rowof = [&](int jj) -> int64_t {                              // pool row of slot j0 + jj, or -1
        int64_t base = pbase[0];
#pragma unroll
        for (int u = 1; u < NPG; ++u) base = jj / PAGE == u ? pbase[u] : base;
        return base < 0 ? -1 : base + jj % PAGE;
    };
    float mx = -INFINITY;
    for (int jj = lane; jj < CHUNK; jj += 64) {
        const int j = j0 + jj;
        float sc = -INFINITY;
        const int64_t r = rowof(jj);
        if (j < len && r >= 0) {
            float a = 0.f;
            for (int d = 0; d < Dh; ++d) a = fmaf((float)qr[d], F::at(kv.k, r * Dh + d), a);
            sc = a * scale;
        }
        ps[jj] = sc;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int jj = lane; jj < CHUNK; jj += 64) {
        const float e = mx == -INFINITY ? 0.f : dec_exp<T>(ps[jj] - mx);
        ps[jj] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    __syncthreads();
    float* part = ws + (((int64_t)row * H + h) * nch + c) * (Dh + 2);
    if (lane == 0) { part[0] = mx; part[1] = sum; }
    for (int d = lane; d < Dh; d += 64) {
        float o = 0.f;
        for (int jj = 0; jj < CHUNK; ++jj)
            if (ps[jj] != 0.f) {                                       // (a non-zero weight: the slot counts for this row, so it lies in a page)
                const float pr = rnd<T>(ps[jj]);
                o = fmaf(pr, F::at(kv.v, rowof(jj) * Dh + d), o);
            }
        part[2 + d] = o;
    }
}

// ---- merge: the dense merge's loop over the sequence's own ceil((len0[b] + Tn) / span) partials (at most the launch's nch); idle: none, so zeros ----
template <typename T>
__global__ __launch_bounds__(64) void attn_extend_merge_paged_kernel(const float* __restrict__ ws, T* __restrict__ out, const int* __restrict__ lens0,
                                                                     int nch, int span, int Tn, int H, int Dh) {
    const int64_t bh = blockIdx.x;                                     // (b * Tn + i) * H + h; out rows are H * Dh wide
    const int len0 = lens0[bh / ((int64_t)Tn * H)];
    int n = len0 < 0 ? 0 : (len0 + Tn - 1) / span + 1;
    n = n < nch ? n : nch;
    merge_chunks<T>(ws + bh * nch * (Dh + 2), out + bh * Dh, n, Dh);
}

// The MFMA kernel's launch for either staging: NW = 1 serves G * Tn <= 32 stacked rows, NW = 4 everything else; `nch` partials per row.
template <typename S>
void launch_extend_paged_mfma(hipStream_t s, const bf16* q, int64_t ldq, typename S::Rows kp, typename S::Rows vp, const int* table, int max_pages,
                              int num_pages, const int* lens0, float* ws, int B, int Tn, int H, int Hkv, int span, int nch, float scale) {
    const int MR = (H / Hkv) * Tn;
    const float sl = scale * 1.44269504088896340736f;
    if (MR <= 32)
        attn_extend_paged_kernel<1, S><<<dim3(nch, Hkv, B), 64, 0, s>>>(q, ldq, kp, vp, table, max_pages, num_pages, lens0, ws, Tn, H, Hkv, span, sl);
    else
        attn_extend_paged_kernel<4, S><<<dim3(nch, Hkv * cdiv(MR, 128), B), 256, 0, s>>>(q, ldq, kp, vp, table, max_pages, num_pages, lens0, ws, Tn, H, Hkv,
                                                                                         span, sl);
}

template <typename T>
int extend_paged_t(const char* name, hipStream_t s, const T* q, int64_t ldq, const T* kp, const T* vp, const int* table, int max_pages, int num_pages,
                   const int* lens0, T* out, float* ws, int B, int Tn, int H, int Hkv, int Dh, int max_len0, float scale) {
    const int span = extend_span(sizeof(T) == 2, Tn, H, Hkv, Dh), nch = cdiv(max_len0 + Tn, span);       // the dense call's partition at len0 = max_len0
    if (sizeof(T) == 2 && Dh == XD) {
        launch_extend_paged_mfma<StageDma>(s, (const bf16*)q, ldq, (const bf16*)kp, (const bf16*)vp, table, max_pages, num_pages, lens0, ws, B, Tn, H, Hkv, span,
                                           nch, scale);
    } else {
        attn_chunk_paged_kernel<T, KvNative<T>><<<dim3(B * Tn, H, nch), 64, 0, s>>>(q, ldq, KvNative<T>{kp, vp}, table, max_pages, num_pages, lens0, ws, Tn, H,
                                                                                  Hkv, Dh, scale);
    }
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(chunks): %s", name, hipGetErrorString(e));
    attn_extend_merge_paged_kernel<T><<<B * Tn * H, 64, 0, s>>>(ws, out, lens0, nch, span, Tn, H, Dh);
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(merge): %s", name, hipGetErrorString(e));
    return SETOK_OK;
}

// Over MXFP4 pools: the native call's dispatch and partition (the dense MXFP4 extend's).  16-bit at head dim 128: the MFMA kernel staged from
// nibbles, `span` slots per partial (a prefix of the workspace, whose rule stays one partial per chunk); everything else the wave-per-chunk kernel.
template <typename T>
int extend_paged_mxfp4_t(const char* name, hipStream_t s, const T* q, int64_t ldq, KvMxfp4 kv, const int* table, int max_pages, int num_pages,
                         const int* lens0, T* out, float* ws, int B, int Tn, int H, int Hkv, int Dh, int max_len0, float scale) {
    const int span = extend_span(sizeof(T) == 2, Tn, H, Hkv, Dh), nch = cdiv(max_len0 + Tn, span);
    if (sizeof(T) == 2 && Dh == XD) {
        launch_extend_paged_mfma<StageMx4>(s, (const bf16*)q, ldq, kv.k, kv.v, table, max_pages, num_pages, lens0, ws, B, Tn, H, Hkv, span, nch, scale);
    } else {
        attn_chunk_paged_kernel<T, KvMxfp4><<<dim3(B * Tn, H, nch), 64, 0, s>>>(q, ldq, kv, table, max_pages, num_pages, lens0, ws, Tn, H, Hkv, Dh, scale);
    }
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(chunks): %s", name, hipGetErrorString(e));
    attn_extend_merge_paged_kernel<T><<<B * Tn * H, 64, 0, s>>>(ws, out, lens0, nch, span, Tn, H, Dh);
    if (hipError_t e = hipGetLastError()) return setok_fail(SETOK_ELAUNCH, "%s(merge): %s", name, hipGetErrorString(e));
    return SETOK_OK;
}

}  // namespace

extern "C" int64_t setok_attention_extend_paged_workspace(int dtype, int B, int Tn, int H, int Hkv, int Dh, int max_len0) {
    return setok_attention_extend_workspace(dtype, B, Tn, H, Hkv, Dh, max_len0);      // the dense rule at len0 = max_len0: the same partition into partials
}

extern "C" int setok_attention_extend_gqa_paged(void* stream, int dtype, const void* q, int64_t ldq, const void* k_pool, const void* v_pool,
                                                const int32_t* block_table, int max_pages, int num_pages, const int32_t* len0, void* out, int B, int Tn,
                                                int H, int Hkv, int Dh, int max_len0, float scale, float* ws, int64_t ws_floats) {
    const char* name = "setok_attention_extend_paged";
    SETOK_CHECK_ARG(q && k_pool && v_pool && block_table && len0 && out && ws, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && Tn >= 1 && H > 0 && H <= 65535 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "%s: bad shape B=%d Tn=%d H=%d Hkv=%d max_pages=%d num_pages=%d", name, B, Tn, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(paged_head_dim(dtype, Dh), "%s: unsupported head dim %d (16-byte pieces per row in {2, 4, 8, 16, 32}: no paged twin of the generic kernel)",
                    name, Dh);
    SETOK_CHECK_ARG(max_len0 >= 0 && (int64_t)max_len0 + Tn <= (int64_t)max_pages * PAGE,
                    "%s: slots [%d, %d + %d) outside [0, max_pages = %d * %d slots] (beyond the table)", name, max_len0, max_len0, Tn, max_pages, PAGE);
    SETOK_CHECK_ARG((int64_t)B * Tn * H <= 0x7fffffffll && (int64_t)Hkv * cdiv((H / Hkv) * Tn, 128) <= 65535 && cdiv(max_len0 + Tn, EXT_CHUNK) <= 65535,
                    "%s: B=%d Tn=%d H=%d max_len0=%d exceed the launch grid", name, B, Tn, H, max_len0);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_pool) && aligned16(v_pool),
                    "%s: q rows (stride %lld) and the pools must be 16-byte aligned", name, (long long)ldq);
    SETOK_CHECK_ARG(((uintptr_t)ws & 7u) == 0, "%s: the workspace must be 8-byte aligned", name);
    const int64_t need = setok_attention_extend_paged_workspace(dtype, B, Tn, H, Hkv, Dh, max_len0);
    SETOK_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed", name, (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16)
        return extend_paged_t<bf16>(name, s, (const bf16*)q, ldq, (const bf16*)k_pool, (const bf16*)v_pool, block_table, max_pages, num_pages, len0,
                                    (bf16*)out, ws, B, Tn, H, Hkv, Dh, max_len0, scale);
    return extend_paged_t<float>(name, s, (const float*)q, ldq, (const float*)k_pool, (const float*)v_pool, block_table, max_pages, num_pages, len0,
                                 (float*)out, ws, B, Tn, H, Hkv, Dh, max_len0, scale);
}

extern "C" int64_t setok_attention_extend_paged_mxfp4kv_workspace(int B, int Tn, int H, int Dh, int max_len0) {
    return setok_attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, max_len0);          // the dense MXFP4 rule at len0 = max_len0: one partial per chunk
}

extern "C" int setok_attention_extend_gqa_paged_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                                        const uint8_t* v_q, const uint8_t* v_s, const int32_t* block_table, int max_pages, int num_pages,
                                                        const int32_t* len0, void* out, int B, int Tn, int H, int Hkv, int Dh, int max_len0, float scale,
                                                        float* ws, int64_t ws_floats) {
    const char* name = "setok_attention_extend_paged_mxfp4kv";
    SETOK_CHECK_ARG(q && k_q && k_s && v_q && v_s && block_table && len0 && out && ws, "%s: null operand", name);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "%s: bad dtype %d", name, dtype);
    SETOK_CHECK_ARG(B >= 0 && B <= 65535 && Tn >= 1 && H > 0 && H <= 65535 && Hkv > 0 && H % Hkv == 0 && max_pages > 0 && num_pages > 0,
                    "%s: bad shape B=%d Tn=%d H=%d Hkv=%d max_pages=%d num_pages=%d", name, B, Tn, H, Hkv, max_pages, num_pages);
    SETOK_CHECK_ARG(Dh > 0 && Dh % 32 == 0, "%s: unsupported head dim %d (a multiple of 32, the MX block)", name, Dh);
    SETOK_CHECK_ARG(max_len0 >= 0 && (int64_t)max_len0 + Tn <= (int64_t)max_pages * PAGE,
                    "%s: slots [%d, %d + %d) outside [0, max_pages = %d * %d slots] (beyond the table)", name, max_len0, max_len0, Tn, max_pages, PAGE);
    SETOK_CHECK_ARG((int64_t)B * Tn <= 0x7fffffffll && cdiv(max_len0 + Tn, EXT_CHUNK) <= 65535, "%s: B=%d Tn=%d H=%d max_len0=%d exceed the launch grid", name,
                    B, Tn, H, max_len0);
    SETOK_CHECK_ARG(!(dtype == SETOK_BF16 && Dh == XD) || ((int64_t)(H / Hkv) * Tn + 127) / 128 * Hkv <= 65535,
                    "%s: Tn=%d H=%d Hkv=%d exceed the launch grid of the MFMA kernel (Hkv * ceil(G * Tn / 128) <= 65535)", name, Tn, H, Hkv);
    SETOK_CHECK_ARG(ldq >= (int64_t)H * Dh && ldq % 8 == 0 && aligned16(q) && aligned16(k_q) && aligned16(v_q),
                    "%s: q rows (stride %lld) and the nibble pools must be 16-byte aligned", name, (long long)ldq);
    const int64_t need = setok_attention_extend_paged_mxfp4kv_workspace(B, Tn, H, Dh, max_len0);
    SETOK_CHECK_ARG(ws_floats >= need, "%s: workspace of %lld floats, %lld needed", name, (long long)ws_floats, (long long)need);
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const KvMxfp4 kv{{k_q, k_s}, {v_q, v_s}};
    if (dtype == SETOK_BF16)
        return extend_paged_mxfp4_t<bf16>(name, s, (const bf16*)q, ldq, kv, block_table, max_pages, num_pages, len0, (bf16*)out, ws, B, Tn, H, Hkv, Dh, max_len0,
                                          scale);
    return extend_paged_mxfp4_t<float>(name, s, (const float*)q, ldq, kv, block_table, max_pages, num_pages, len0, (float*)out, ws, B, Tn, H, Hkv, Dh, max_len0,
                                       scale);
}
