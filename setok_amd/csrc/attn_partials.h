// attn_partials.h — what the attention kernels that cut a sequence's keys into chunks share (attn_decode.hip, attn_paged.hip, attn_extend.hip, attn_extend_paged.hip): every chunk leaves
// fp32 partials — per (sequence, query head, chunk) Dh + 2 floats [max, sum, Dh accumulators] — in the caller's workspace, and a second launch merges a
// query head's chunks in chunk order.  ONE definition of the merge and of the exponential both sides of it use: a partial is only meaningful to the
// merge that rescales it.  Also here, once: the cache formats (native, fp8, MXFP4) as the kernels see them, and the wave-per-chunk kernel every head dim without a
// lane layout falls back to, whichever entry point it came through; and row_sum, the lane-group reduction of the lane-layout kernels (dense and paged).
// And the MXFP4 quantiser of kv_append, once for the dense cache and the pages (kv_append_mxfp4_kernel, with row_max).
#pragma once
#include "common.h"
#include "fp8.h"
#include "mx4.h"

namespace {

// exp(x) for x <= 0: the accurate expf in fp32 (parity mode), v_exp_f32 in the 16-bit types (far below the rounding of the probability)
template <typename T> __device__ inline float dec_exp(float x) {
    if constexpr (sizeof(T) == 4) return expf(x);
    else return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f);
}

template <typename T> __device__ inline float rnd(float v) { return (float)(T)v; }

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

template <typename T> struct Raw16;
template <> struct Raw16<float> { typedef f32x4 type; };
template <> struct Raw16<bf16> { typedef bf16x8 type; };

// ---- the cache formats: one layer's cache as a kernel argument (by value) and what a kernel must know to read it ------------------------------
// VEC elements per lane and load (16 bytes of a native or e4m3 row, 8 bytes of a nibble row), CHUNK slots per decode chunk, Raw the lane's piece in
// registers, load() elements [i, i + VEC) of the K or V operand -> Raw, decode() Raw -> VEC floats, at() one element (the fallback's read).  SCALED:
// a row carries a power-of-two exponent byte (ke / ve), whose 2^e multiplies the finished dot product and the rounded probability.
template <typename T> struct KvNative {
    static constexpr int VEC = Elem<T>::VEC, CHUNK = SETOK_DECODE_CHUNK;
    static constexpr bool SCALED = false;
    typedef typename Raw16<T>::type Raw;
    const T *k, *v;
    __device__ static inline Raw load(const T* p, int64_t i) { return *reinterpret_cast<const Raw*>(p + i); }
    __device__ static inline void decode(const Raw& r, float* f) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = (float)r[e];
    }
    __device__ static inline float at(const T* p, int64_t i) { return (float)p[i]; }
};
struct KvFp8 {                                                         // e4m3fn rows + one int8 exponent per row (fp8.h)
    static constexpr int VEC = 16, CHUNK = SETOK_DECODE_CHUNK_FP8KV;
    static constexpr bool SCALED = true;
    typedef u32x4 Raw;
    const uint8_t* k;
    const int8_t* ke;
    const uint8_t* v;
    const int8_t* ve;
    __device__ static inline Raw load(const uint8_t* p, int64_t i) { return *reinterpret_cast<const Raw*>(p + i); }
    __device__ static inline void decode(const Raw& r, float* f) { fp8w_decode16(r, f); }      // v_cvt_pk_f32_fp8: exact
    __device__ static inline float at(const uint8_t* p, int64_t i) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)p[i], false)[0]; }
};
// OCP MXFP4 rows (include/setok_hip.h, "MXFP4 KV cache"): Dh / 2 bytes of e2m1 nibbles + Dh / 32 e8m0 scale bytes per row.  An operand is the pair
// (nibbles, scales); element i of it is nibble i under scale byte i / 32 (Dh % 32 == 0, so blocks never straddle rows).  A lane holds 16
// elements — 8 nibble bytes and the scale byte it shares with its neighbour — and the hardware converter applies the scale, so decode() gives
// exactly K', V' and nothing is left to scale afterwards.  A 0xFF scale byte makes the operand a NaN: 16 NaNs, which a slot that does not count
// loses by selection like any other value.
struct Mx4Rows {
    const uint8_t* q;
    const uint8_t* s;
};
struct Mx4Piece {
    uint2 w;
    unsigned s;
};
struct KvMxfp4 {
    static constexpr int VEC = 16, CHUNK = SETOK_DECODE_CHUNK_MXFP4KV;
    static constexpr bool SCALED = false;
    typedef Mx4Piece Raw;
    Mx4Rows k, v;
    __device__ static inline Raw load(const Mx4Rows& p, int64_t i) { return Raw{*reinterpret_cast<const uint2*>(p.q + (i >> 1)), p.s[i >> 5]}; }
    __device__ static inline void decode(const Raw& r, float* f) {
        const float sc = mx4_scale(r.s);
        mx4_f32x8(r.w.x, sc, f);
        mx4_f32x8(r.w.y, sc, f + 8);
    }
    __device__ static inline float at(const Mx4Rows& p, int64_t i) {
        return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4((unsigned)p.q[i >> 1], mx4_scale(p.s[i >> 5]), 0)[i & 1];
    }
};

// ---- how a 32-key tile of the MFMA extend kernels (attn_extend.hip, attn_extend_paged.hip) reaches LDS: the staging policy S -------------------
// Both kernels read ONE LDS image — 256-byte rows of the 16-bit type, K in 16-byte slots XOR-swizzled by (row & 15), V row-major for the
// transposing reads — and state the tile arithmetic once each; S says what a cache operand is (Rows) and whether the image is filled by LDS-DMA
// from native rows (StageDma: the request IS the fill, nothing to commit) or from MXFP4 rows through registers (StageMx4: request = loads into an
// Mx4Tile, commit = convert and write after the previous tile's MFMAs).
struct StageDma {
    static constexpr bool MX4 = false;
    typedef const bf16* __restrict__ Rows;
};
struct StageMx4 {
    static constexpr bool MX4 = true;
    typedef Mx4Rows Rows;
};

// A tile of MXFP4 rows at head dim 128 on its way to LDS: 128 MX blocks of K, then 128 of V (a block: 16 bytes of nibbles + its e8m0 byte = 32
// elements = 64 bytes of the image), 256 / NT per thread of a workgroup of NT threads; block p & 127 is block (p & 3) of tile row (p & 127) >> 2,
// so a wave's loads are consecutive in memory, and p < 128 (K or V) is wave-uniform.
template <int NT> struct Mx4Tile {
    static constexpr int NB = 256 / NT;
    u32x4 w[NB];
    unsigned s[NB];

    // row0: the operands' row of the tile's slot 0; tile rows above `last` (the last slot below `top`) are read as row `last` and discarded
    __device__ inline void request(const Mx4Rows& k, const Mx4Rows& v, int64_t row0, int last, int tid) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int p = u * NT + tid;
            const Mx4Rows& src = p < 128 ? k : v;
            const int64_t blk = (row0 + min((p & 127) >> 2, last)) * 4 + (p & 3);       // the block's index in the operand
            w[u] = *reinterpret_cast<const u32x4*>(src.q + blk * 16);
            s[u] = src.s[blk];
        }
    }

    // out[j] = x[(j + r) & 3]: a lane writes its block's four 16-byte pieces in an order rotated by r, which costs selects on the nibble dwords only
    __device__ static inline u32x4 rot4(u32x4 x, int r) {
        if (r & 1) x = u32x4{x[1], x[2], x[3], x[0]};
        if (r & 2) x = u32x4{x[2], x[3], x[0], x[1]};
        return x;
    }

    // Convert (v_cvt_scalef32_pk_*_fp4: exact, the scale applied) and write the tile into the image Kb / Vb.  kbits: the tile's slots that can count;
    // the V row of every other slot is written as zeros (its nibbles and scale byte may be anything, 0xFF -> NaN included, and 0 * NaN would reach the
    // accumulators), its K row as it is (the score is replaced by selection).  !staged: nothing was requested (no page) — kbits is 0, V becomes
    // zeros, K stays whatever the buffer held.  ds_write_b128 is served in groups of 8 consecutive lanes over 32 banks: the rotation makes the 8
    // pieces of a group distinct modulo 128 bytes (V: r = (p >> 1) & 3; K: r = p & 2, the swizzle's row bit does the rest).
    __device__ inline void commit(char* Kb, char* Vb, unsigned kbits, bool staged, int tid) const {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int p = u * NT + tid, row = (p & 127) >> 2, c0 = (p & 3) * 4;
            if (p < 128) {
                if (!staged) continue;
                const int r = p & 2;
                const u32x4 x = rot4(w[u], r);
                const float sc = mx4_scale(s[u]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<bf16x8*>(Kb + row * 256 + (((c0 + ((j + r) & 3)) ^ (row & 15)) << 4)) = mx4_frag(x[j], sc);
            } else {
                const bool on = (kbits >> row) & 1u;
                const int r = (p >> 1) & 3;
                const u32x4 x = rot4(on ? w[u] : u32x4{0u, 0u, 0u, 0u}, r);            // nibble 0 under scale byte 127 is +0.0
                const float sc = mx4_scale(on ? s[u] : 127u);
#pragma unroll
                for (int j = 0; j < 4; ++j) *reinterpret_cast<bf16x8*>(Vb + row * 256 + ((c0 + ((j + r) & 3)) << 4)) = mx4_frag(x[j], sc);
            }
        }
    }
};

// ---- any head dim (Dh % 8 == 0): one wave per (query row, query head, chunk of CHUNK slots), a key per lane ------------------------------------
// Row b * Tn + i counts slot j iff j <= len0 + i and its mask byte is non-zero (a decode call: Tn = 1, len0 = len - 1).  Only a slot that counts is
// read.  grid (rows, H, chunks) with ROWS_X, else (chunks, H, rows): each caller keeps the grid its entry point's limits were written for.
template <typename T, typename F, int CHUNK, bool ROWS_X>
__global__ __launch_bounds__(64) void attn_chunk_any_kernel(const T* __restrict__ q, int64_t ldq, F kv, const uint8_t* __restrict__ kmask,
                                                            float* __restrict__ ws, int Tn, int H, int Hkv, int Dh, int cap, int len0, float scale) {
    __shared__ float ps[CHUNK];
    const int row = ROWS_X ? blockIdx.x : blockIdx.z;
    const int h = blockIdx.y, c = ROWS_X ? blockIdx.z : blockIdx.x, nch = ROWS_X ? gridDim.z : gridDim.x, lane = threadIdx.x;
    const int b = row / Tn, len = len0 + row % Tn + 1;                 // this row counts slots below len
    const int hk = h / (H / Hkv), j0 = c * CHUNK;
    const T* qr = q + (int64_t)row * ldq + (int64_t)h * Dh;
    const int64_t rowbase = ((int64_t)b * Hkv + hk) * cap;
    float mx = -INFINITY;
    for (int jj = lane; jj < CHUNK; jj += 64) {
        const int j = j0 + jj;
        float sc = -INFINITY;
        if (j < len && kmask[(int64_t)b * cap + j]) {
            float a = 0.f;
            for (int d = 0; d < Dh; ++d) a = fmaf((float)qr[d], F::at(kv.k, (rowbase + j) * Dh + d), a);
            if constexpr (F::SCALED) sc = a * fp8w_scale(kv.ke[rowbase + j]) * scale;
            else sc = a * scale;
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
            if (ps[jj] != 0.f) {                                       // (a non-zero weight: the slot counts for this row)
                float pr = rnd<T>(ps[jj]);
                if constexpr (F::SCALED) pr = pr * fp8w_scale(kv.ve[rowbase + j0 + jj]);
                o = fmaf(pr, F::at(kv.v, (rowbase + j0 + jj) * Dh + d), o);
            }
        part[2 + d] = o;
    }
}

// ---- merge: one workgroup per (sequence, query head), the chunks in chunk order ----------------------------------------------------------------
// `part`: the query head's partials, chunk c at c * (Dh + 2); `n` of them count (0: zeros).  The ONE loop behind the dense merge, where n is the launch's
// chunk count, and the paged one (attn_paged.hip), where n comes from the sequence's own length.
template <typename T>
__device__ inline void merge_chunks(const float* __restrict__ part, T* __restrict__ out, int n, int Dh) {
    float M = -INFINITY;
    for (int c = 0; c < n; ++c) M = fmaxf(M, part[(int64_t)c * (Dh + 2)]);
    float L = 0.f;
    for (int c = 0; c < n; ++c) {
        const float mc = part[(int64_t)c * (Dh + 2)];
        L = fmaf(mc == -INFINITY ? 0.f : dec_exp<T>(mc - M), part[(int64_t)c * (Dh + 2) + 1], L);
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    for (int d = threadIdx.x; d < Dh; d += 64) {
        float o = 0.f;
        for (int c = 0; c < n; ++c) {
            const float mc = part[(int64_t)c * (Dh + 2)];
            o = fmaf(mc == -INFINITY ? 0.f : dec_exp<T>(mc - M), part[(int64_t)c * (Dh + 2) + 2 + d], o);
        }
        out[d] = (T)(o * inv);
    }
}

// ---- host rules the dense and the paged entries share ---------------------------------------------------------------------------------------------
// Slots per partial on the path an extend call takes: the MFMA kernel (16-bit, head dim 128) with more than 32 stacked rows spans SETOK_EXTEND_SPAN
// chunks, everything else one.  `low`: the call's element type is the build's 16-bit type.
static inline int extend_span(bool low, int Tn, int H, int Hkv, int Dh) {
    return low && Dh == 128 && (H / Hkv) * Tn > 32 ? SETOK_EXTEND_SPAN * SETOK_EXTEND_CHUNK : SETOK_EXTEND_CHUNK;
}

// The head dims the paged entries take, those with a lane layout in the native format: Dh / VEC in {2, 4, 8, 16, 32} (16 ... 256 in 16 bits, 8 ... 128 in fp32).
static inline bool paged_head_dim(int dtype, int Dh) {
    const int vec = dtype == SETOK_F32 ? 4 : 8;
    if (Dh <= 0 || Dh % vec != 0) return false;
    const int lpr = Dh / vec;
    return lpr == 2 || lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32;
}

// The head dims the paged MXFP4 entries take: those with a lane layout over nibble rows (16 elements per lane; attn_decode.hip's decode_t has the
// same three), so that a paged sequence's bits are the dense lane-layout kernel's.  The paged extend alone would serve every Dh % 32 == 0.
static inline bool paged_mxfp4_head_dim(int Dh) { return Dh == 32 || Dh == 64 || Dh == 128; }

template <typename T>
__global__ __launch_bounds__(64) void attn_decode_merge_kernel(const float* __restrict__ ws, T* __restrict__ out, int nch, int H, int Dh) {
    const int64_t bh = blockIdx.x;                                     // b * H + h; out rows are H * Dh wide
    merge_chunks<T>(ws + bh * nch * (Dh + 2), out + bh * Dh, nch, Dh);
}

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

// ==== filling an MXFP4 KV cache, dense (attn_decode.hip) or paged (attn_paged.hip): ONE quantiser, the destination a parameter ====================
// A cache row is Dh / 2 bytes of e2m1 nibbles + Dh / 32 e8m0 scale bytes and means value(nibble[d]) * 2^(s[d / 32] - 127) (mx4.h: the rule of
// the weight path).  kv_append_fp8_kernel's arrangement: one pass, a row in the registers of GL lanes, 8 elements each, so a block of 32 is an
// aligned quad of lanes and its amax two quad_perm exchanges; a lane writes its 8 nibbles as one dword, the quad's first lane the scale byte.
// Dh % 32 == 0, so a row is a whole number of quads and a lane without a piece shares a quad with no live lane.
//
// D says where the row of (sequence b, new token t, key / value head hk) goes: row(b, t, hk, Hkv) is its row in the (…, Dh / 2) and (…, Dh / 32)
// operands, or < 0 for "nowhere".  A row that goes nowhere is skipped by predication — its lanes load nothing, carry zeros through the exchanges
// (which need every lane of a quad) and store nothing —, never by leaving the loop.
struct Mx4ToDense {                                                    // slot pos0 + t of a (B, Hkv, cap, ·) cache
    int cap, pos0;
    __device__ inline int64_t row(int b, int t, int hk, int Hkv) const { return ((int64_t)b * Hkv + hk) * cap + pos0 + t; }
};
struct Mx4ToPages {                                                    // slot slot0[b] + t of sequence b, through its row of the block table
    const int* table;
    const int* slot0;
    int max_pages, num_pages;
    __device__ inline int64_t row(int b, int t, int hk, int Hkv) const {
        const int s0 = slot0[b];
        if (s0 < 0) return -1;                                         // an idle row of the running batch
        const int64_t slot = (int64_t)s0 + t, pi = slot / SETOK_KV_PAGE;
        if (pi >= max_pages) return -1;
        const int page = table[(int64_t)b * max_pages + pi];
        if (page < 0 || page >= num_pages) return -1;                  // no page: nothing is written, no address is formed
        return ((int64_t)page * Hkv + hk) * SETOK_KV_PAGE + slot % SETOK_KV_PAGE;
    }
};

// Rows are numbered ((b * T + t) * 2 + which) * Hkv + hk; a workgroup takes 256 / GL of them per trip, every wave makes the same number of trips.
template <typename T, int GL, typename D>
__global__ __launch_bounds__(256) void kv_append_mxfp4_kernel(const T* __restrict__ qkv, uint8_t* __restrict__ kq, uint8_t* __restrict__ ks,
                                                              uint8_t* __restrict__ vq, uint8_t* __restrict__ vs, int B, int Tn, int H, int Hkv, int Dh,
                                                              D dest) {
    constexpr int RPB = 256 / GL;                                      // rows per workgroup and trip
    const int vpr = Dh / 8, sub = threadIdx.x % GL;
    const int64_t rows = (int64_t)B * Tn * 2 * Hkv, ld = (int64_t)(H + 2 * Hkv) * Dh;
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < rows; r0 += (int64_t)gridDim.x * RPB) {
        const int64_t row = r0 + threadIdx.x / GL;
        bool live = row < rows && sub < vpr;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = 0.f;
        int which = 0;
        int64_t slot = 0;
        if (live) {
            const int hk = (int)(row % Hkv);
            which = (int)((row / Hkv) & 1);                            // 0 = k, 1 = v
            const int64_t bt = row / (2 * Hkv);
            slot = dest.row((int)(bt / Tn), (int)(bt % Tn), hk, Hkv);
            live = slot >= 0;                                          // (the same for all lanes of the row, so for all lanes of a quad)
            if (live) {
                const T* src = qkv + bt * ld + (int64_t)(H + which * Hkv + hk) * Dh + sub * 8;
#pragma unroll
                for (int u = 0; u < 8 / Elem<T>::VEC; ++u) ld_vec<T>(src + u * Elem<T>::VEC, f + u * Elem<T>::VEC);
            }
        }
        float amax = 0.f, bad = 0.f;                                   // bad: the block holds a non-finite entry (it becomes scale byte 0xFF, nibbles 0)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = fabsf(f[e]);
            if (a <= 3.402823466e38f) amax = fmaxf(amax, a);
            else bad = 1.f;
        }
        amax = row_max<4>(amax);
        bad = row_max<4>(bad);
        const int ex = mx4_exponent(amax);
        const float inv = mx4_inv_scale(ex);
        if (live) {
            unsigned w = 0u;
#pragma unroll
            for (int e = 0; e < 8; ++e) w |= mx4_encode(f[e] * inv) << (4 * e);
            *reinterpret_cast<unsigned*>((which ? vq : kq) + slot * (Dh / 2) + sub * 4) = bad != 0.f ? 0u : w;
            if ((sub & 3) == 0) (which ? vs : ks)[slot * (Dh / 32) + (sub >> 2)] = (uint8_t)(bad != 0.f ? 0xff : 127 + ex);
        }
    }
}

template <typename T, typename D>
void launch_append_mxfp4(hipStream_t s, const T* qkv, uint8_t* kq, uint8_t* ks, uint8_t* vq, uint8_t* vs, int B, int Tn, int H, int Hkv, int Dh, D dest) {
    const int vpr = Dh / 8;
    const int64_t rows = (int64_t)B * Tn * 2 * Hkv;
#define MX4_APPEND(GL)                                                                                                          \
    if (vpr <= GL) {                                                                                                            \
        const int64_t wgs = (rows + 256 / GL - 1) / (256 / GL);                                                                 \
        kv_append_mxfp4_kernel<T, GL, D><<<(int)(wgs > 65536 ? 65536 : wgs), 256, 0, s>>>(qkv, kq, ks, vq, vs, B, Tn, H, Hkv, Dh, dest); \
        return;                                                                                                                 \
    }
    MX4_APPEND(4) MX4_APPEND(8) MX4_APPEND(16) MX4_APPEND(32) MX4_APPEND(64)
#undef MX4_APPEND
}

}  // namespace
