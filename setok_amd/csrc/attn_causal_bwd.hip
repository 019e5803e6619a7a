// attn_causal_bwd.hip — backward of the causal + key-padding-masked attention of the LLM prefill (llama.hip, attn_causal_kernel) for head dim 128
// in the library's 16-bit element type: two MFMA kernels (v_mfma_f32_32x32x16), fp32 accumulation, P and dS rounded to the element type for the
// second products.
//
//   dQ kernel     one workgroup = 4 waves = 128 queries of one (sequence, query head), a wave = 32 queries kept in registers (q, dO fragments, the
//                 dQ^T accumulators).  Key tiles of 32 stream through LDS up to the block's diagonal, TWICE: a first walk recomputes the forward's
//                 log-sum-exp (S^T = K Q^T only) and D = dO.O, left in the workspace for the other kernel; the second forms
//                 S^T, dP^T = V dO^T, dS^T = P^T (dP^T - D) and dQ^T += K^T dS^T.
//   dK/dV kernel  one workgroup = 128 keys of one (sequence, key / value head), a wave = 32 keys in registers (k, v fragments, the dK^T and dV^T
//                 accumulators).  Query tiles of 32 (q, dO, lse, D) stream through LDS from the block's diagonal to T, for each query head of the
//                 group in head order: S = Q K^T, dP = dO V^T with the key on the lane, dV^T += dO^T P, dK^T += Q^T dS.  No sum crosses a
//                 workgroup, so there are no atomics and the result is a fixed-order sum.
// In both kernels the products that need their streamed operand transposed read it from the SAME LDS image as the row reads, with the
// hardware-transposing LDS read; the image keeps 256-byte rows whose 16-byte chunks are XOR-permuted per row (`sw`) so that both kinds of read
// spread over the banks.  The accumulator of the first products is the B operand of the second ones without any lane movement (the contraction
// index sits in the registers).  Causality is in the loop bounds; only tiles on a wave's diagonal, tiles with padded keys and the last partial
// tile apply the per-element mask.  exp2 with the scale and the lse pre-multiplied by log2(e).
#include "lds_mma.h"

namespace {

constexpr int BD = 128;                  // head dim
constexpr int BROW = BD * 2;             // bytes per row of an LDS image
constexpr int BQ = 128;                  // rows per workgroup (4 waves x 32)
constexpr int TILE = 32 * BROW;          // one streamed tile: 32 rows

__device__ inline int sw(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }      // chunk permutation of a row: physical chunk = logical ^ sw(row)

// A 32-row tile of 128-element rows (row stride ldb bytes from `base`, first row r0, rows clamped to Tn - 1) -> the swizzled image at LDS byte
// address `dst` (wave-uniform: image base + wave * 1024): 512 pieces of 16 bytes, 2 per thread.  offs[i]: this thread's constant source offsets.
__device__ inline void stage_tile(const char* base, size_t ldb, int r0, int Tn, int tid, const unsigned (&offs)[2], unsigned dst) {
    if (r0 + 32 <= Tn) {                                                 // (uniform) all 32 rows exist
        const char* tb = base + (size_t)r0 * ldb;
#pragma unroll
        for (int i = 0; i < 2; ++i) lds_dma16_sbase(tb, offs[i], dst + i * 4096);
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = i * 256 + tid, row = p >> 4, c = p & 15;
        lds_dma16(base + (size_t)min(r0 + row, Tn - 1) * ldb + ((c ^ sw(row)) << 4), dst + i * 4096);
    }
}

// A operand of `X^T . acc` for the 32 columns d*32.. of the image and the 16 rows k2*16..: two transposing reads (rows +0 and +8); toff = the lane's
// offsets for (d, row group) computed once (tr_offsets)
__device__ inline bf16x8 tr_frag(const char* img, int k2, unsigned o0, unsigned o1) {
    const char* a = img + k2 * 16 * BROW;
    return lds_read_tr16(a + o0, a + o1);
}
// lane 4q+p of a 16-lane group supplies row q, columns 4p..4p+3 of its block; group g: rows 4 (g >> 1).., columns 16 (g & 1)..  (+ 8 rows for e = 1)
__device__ inline void tr_offsets(int lane, unsigned (&toff)[4][2]) {
    const int g16 = lane >> 4, i16 = lane & 15;
    const int row = (i16 >> 2) + 4 * (g16 >> 1);
    const int col = (g16 & 1) * 16 + (i16 & 3) * 4;                      // element column inside the 32-column block
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int r = row + 8 * e, ch = d * 4 + (col >> 3);
            toff[d][e] = (unsigned)(r * BROW + ((ch ^ sw(r)) << 4) + (col & 7) * 2);
        }
}

// ---- dQ (+ lse, D) ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_causal_bwd_dq_kernel(const bf16* __restrict__ qkv, const uint8_t* __restrict__ kmask, const bf16* __restrict__ out,
                                                                 const bf16* __restrict__ dout, bf16* __restrict__ dqkv, int Tn, int H, int Hkv,
                                                                 float scale, float scale_log2e, float* __restrict__ lse2, float* __restrict__ dsum) {
    __shared__ __attribute__((aligned(16))) char smem[2][2][TILE];       // [buffer][K, V] images
    const int qb = (int)gridDim.x - 1 - (int)blockIdx.x;                 // heavy (late) query blocks first
    const int h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qi = lane & 31, hi = lane >> 5;
    const int64_t C = (int64_t)H * BD, ld = (int64_t)(H + 2 * Hkv) * BD;
    const int hk = h / (H / Hkv);
    const bf16* seq = qkv + (int64_t)b * Tn * ld;
    const char* kbase = reinterpret_cast<const char*>(seq + C + (int64_t)hk * BD);
    const char* vbase = kbase + (int64_t)Hkv * BD * 2;
    const uint8_t* km = kmask ? kmask + (int64_t)b * Tn : nullptr;
    const int q0 = qb * BQ + wave * 32;
    const int q = q0 + qi;
    const int64_t qrow = (int64_t)b * Tn + min(q, Tn - 1);
    bf16x8 qf[8], dof[8];
    float D = 0.f;
    {
        const bf16* qp = qkv + qrow * ld + (int64_t)h * BD + hi * 8;
        const bf16* dp = dout + qrow * C + (int64_t)h * BD + hi * 8;
        const bf16* op = out + qrow * C + (int64_t)h * BD + hi * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
            dof[ks] = *reinterpret_cast<const bf16x8*>(dp + ks * 16);
            const bf16x8 ov = *reinterpret_cast<const bf16x8*>(op + ks * 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) D = fmaf((float)dof[ks][j], (float)ov[j], D);
        }
        D += __shfl_xor(D, 32, 64);
    }
    constexpr float NEG = -1.0e30f;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)&smem[0][0][0]) + wave * 1024;
    const int kend = min(qb * BQ + BQ, Tn);
    const int nkt = (kend + 31) >> 5;
    unsigned offs[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = i * 256 + tid, row = p >> 4, c = p & 15;
        offs[i] = (unsigned)row * (unsigned)(ld * 2) + (unsigned)((c ^ sw(row)) << 4);
    }
    unsigned toff[4][2];
    tr_offsets(lane, toff);
    const int rsw = sw(qi);
    auto stage = [&](int kt, int buf) {
        stage_tile(kbase, (size_t)ld * 2, kt * 32, Tn, tid, offs, lds0 + buf * (2 * TILE));
        stage_tile(vbase, (size_t)ld * 2, kt * 32, Tn, tid, offs, lds0 + buf * (2 * TILE) + TILE);
    };
    // key-padding / range mask of a tile as a 32-bit set
    auto tile_bits = [&](int k0) {
        unsigned kbits = 0xffffffffu;
        if (km) kbits = (unsigned)__ballot(lane < 32 && k0 + lane < Tn && km[min(k0 + lane, Tn - 1)] != 0);
        else if (k0 + 32 > Tn) kbits = (unsigned)__ballot(lane < 32 && k0 + lane < Tn);
        return kbits;
    };
    auto scores = [&](const char* Kb, const bf16x8 (&bf)[8]) {           // image rows (on the MFMA row index) x the wave's register fragments
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Kb + qi * BROW + (((ks * 2 + hi) ^ rsw) << 4));
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, bf[ks], s, 0, 0, 0);
        }
        return s;
    };
    // ---- first walk: the forward's running maximum and sum -> lse (log2 domain) ----
    float m_run = NEG, l_run = 0.f;
    stage(0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nkt) stage(kt + 1, buf ^ 1);
        const int k0 = kt * 32;
        if (k0 > q0 + 31) continue;                                      // wave-uniform: the tile lies in this wave's future
        const unsigned kbits = tile_bits(k0);
        const f32x16 s = scores(&smem[buf][0][0], qf);
        const bool diag = k0 + 31 > q0;
        float t[16], mx = NEG;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
            t[r] = s[r];
            if (!((kbits >> kj) & 1u) || (diag && k0 + kj > q)) t[r] = NEG;
            mx = fmaxf(mx, t[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        l_run *= __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);
        m_run = m_new;
        const float mc = m_run * scale_log2e;
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) ls += t[r] <= NEG ? 0.f : __builtin_amdgcn_exp2f(fmaf(t[r], scale_log2e, -mc));
        l_run += ls;
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float L2 = l_tot > 0.f ? fmaf(m_run, scale_log2e, __builtin_amdgcn_logf(l_tot)) : 0.f;      // (v_log_f32 is log2)
    if (q < Tn && hi == 0) {
        lse2[((int64_t)b * H + h) * Tn + q] = L2;
        dsum[((int64_t)b * H + h) * Tn + q] = D;
    }
    // ---- second walk: dQ^T += K^T dS^T ----
    f32x16 acc[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[d][r] = 0.f;
    __syncthreads();                                                     // every wave is done with the first walk's last tile
    stage(0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nkt) stage(kt + 1, buf ^ 1);
        const int k0 = kt * 32;
        if (k0 > q0 + 31) continue;
        const unsigned kbits = tile_bits(k0);
        const char* Kb = &smem[buf][0][0];
        const f32x16 s = scores(Kb, qf);
        const f32x16 dp = scores(&smem[buf][1][0], dof);
        const bool diag = k0 + 31 > q0;
        const bool plain = !diag && kbits == 0xffffffffu;                // (wave-uniform) every key of the tile is a token every query of the wave sees
        float t[16];
        if (plain) {
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -L2)) * (dp[r] - D);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kj = (r & 3) + 8 * (r >> 2) + 4 * hi;
                const bool off = !((kbits >> kj) & 1u) || (diag && k0 + kj > q);
                t[r] = off ? 0.f : __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -L2)) * (dp[r] - D);
            }
        }
        const bf16x8 p0 = pack8(t), p1 = pack8(t + 8);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2)
                acc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Kb, k2, toff[d][0], toff[d][1]), k2 == 0 ? p0 : p1, acc[d], 0, 0, 0);
        }
    }
    if (q < Tn) {
        bf16* op = dqkv + ((int64_t)b * Tn + q) * ld + (int64_t)h * BD;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                bf16x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (bf16)(acc[d][r4 * 4 + j] * scale);
                *reinterpret_cast<bf16x4*>(op + d * 32 + 8 * r4 + 4 * hi) = v;
            }
    }
}

// ---- dK, dV ------------------------------------------------------------------------------------------------------------------------------------------
constexpr int KV_LDS = 2 * (2 * TILE + 256);                            // [buffer][Q image | dO image | lse (32 floats) | D (32 floats)]

__global__ __launch_bounds__(256, 2) void attn_causal_bwd_dkv_kernel(const bf16* __restrict__ qkv, const uint8_t* __restrict__ kmask, const bf16* __restrict__ dout,
                                                                  bf16* __restrict__ dqkv, int Tn, int H, int Hkv, float scale, float scale_log2e,
                                                                  const float* __restrict__ lse2, const float* __restrict__ dsum) {
    __shared__ __attribute__((aligned(16))) char smem[KV_LDS];
    const int kb = blockIdx.x;                                           // key block 0 meets every query: the heaviest blocks already come first
    const int hk = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ki = lane & 31, hi = lane >> 5;
    const int G = H / Hkv;
    const int64_t C = (int64_t)H * BD, ld = (int64_t)(H + 2 * Hkv) * BD;
    const int k0w = kb * BQ + wave * 32;                                 // this wave's first key
    const int key = k0w + ki;
    const int64_t krow = (int64_t)b * Tn + min(key, Tn - 1);
    const bool key_ok = key < Tn && (!kmask || kmask[krow] != 0);        // a padded key is seen by no query: zeros
    bf16x8 kf[8], vf[8];
    {
        const bf16* kp = qkv + krow * ld + C + (int64_t)hk * BD + hi * 8;
        const bf16* vp = kp + (int64_t)Hkv * BD;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            kf[ks] = *reinterpret_cast<const bf16x8*>(kp + ks * 16);
            vf[ks] = *reinterpret_cast<const bf16x8*>(vp + ks * 16);
        }
    }
    f32x16 dk[4], dv[4];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[d][r] = 0.f; dv[d][r] = 0.f; }
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) char*)&smem[0]);
    const unsigned lds0 = lds_base + wave * 1024;
    unsigned qoffs[2], ooffs[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = i * 256 + tid, row = p >> 4, c = p & 15;
        qoffs[i] = (unsigned)row * (unsigned)(ld * 2) + (unsigned)((c ^ sw(row)) << 4);
        ooffs[i] = (unsigned)row * (unsigned)(C * 2) + (unsigned)((c ^ sw(row)) << 4);
    }
    unsigned toff[4][2];
    tr_offsets(lane, toff);
    const int rsw = sw(ki);
    const int qt0 = (kb * BQ) >> 5, nqt = (Tn + 31) >> 5;
    const int nq = nqt - qt0;                                            // query tiles per head: from the block's diagonal to T
    const int nit = G * nq;
    const char* qseq = reinterpret_cast<const char*>(qkv + (int64_t)b * Tn * ld);
    const char* oseq = reinterpret_cast<const char*>(dout + (int64_t)b * Tn * C);
    auto stage = [&](int it, int buf) {
        const int h = hk * G + it / nq, r0 = (qt0 + it % nq) * 32;
        const unsigned dst = buf * (2 * TILE + 256);
        stage_tile(qseq + (size_t)h * BD * 2, (size_t)ld * 2, r0, Tn, tid, qoffs, lds0 + dst);
        stage_tile(oseq + (size_t)h * BD * 2, (size_t)C * 2, r0, Tn, tid, ooffs, lds0 + dst + TILE);
        if (wave == 0) {                                                 // lanes 0-31: lse of the tile's queries, lanes 32-63: their D
            const int64_t i = ((int64_t)b * H + h) * Tn + min(r0 + (lane & 31), Tn - 1);
            lds_dma4((lane < 32 ? lse2 : dsum) + i, lds_base + dst + 2 * TILE);
        }
    };
    auto scores = [&](const char* img, const bf16x8 (&bf)[8]) {
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(img + ki * BROW + (((ks * 2 + hi) ^ rsw) << 4));
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[ks], s, 0, 0, 0);
        }
        return s;
    };
    if (nit > 0) stage(0, 0);
    for (int it = 0; it < nit; ++it) {
        const int buf = it & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (it + 1 < nit) stage(it + 1, buf ^ 1);
        const int r0 = (qt0 + it % nq) * 32;                             // first query of the tile
        if (r0 + 31 < k0w) continue;                                     // wave-uniform: every query of the tile precedes this wave's keys
        const char* Qi = &smem[buf * (2 * TILE + 256)];
        const char* Oi = Qi + TILE;
        const float* row_l = reinterpret_cast<const float*>(Qi + 2 * TILE);
        const f32x16 s = scores(Qi, kf);                                 // [query in the registers][key on the lane]
        const f32x16 dp = scores(Oi, vf);
        const bool plain = r0 >= k0w + 31 && r0 + 32 <= Tn;              // (wave-uniform) every query of the tile exists and sees every key of the wave
        float p[16], ds[16];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(row_l + 8 * r4 + 4 * hi);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(row_l + 32 + 8 * r4 + 4 * hi);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = r4 * 4 + j;
                float pv = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -l4[j]));
                if (!plain) {
                    const int qq = r0 + 8 * r4 + 4 * hi + j;
                    if (qq < key || qq >= Tn) pv = 0.f;
                }
                p[r] = pv;
                ds[r] = pv * (dp[r] - d4[j]);
            }
        }
        const bf16x8 p0 = pack8(p), p1 = pack8(p + 8), s0 = pack8(ds), s1 = pack8(ds + 8);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) {
                dv[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Oi, k2, toff[d][0], toff[d][1]), k2 == 0 ? p0 : p1, dv[d], 0, 0, 0);
                dk[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag(Qi, k2, toff[d][0], toff[d][1]), k2 == 0 ? s0 : s1, dk[d], 0, 0, 0);
            }
        }
    }
    if (key < Tn) {
        bf16* kp = dqkv + ((int64_t)b * Tn + key) * ld + C + (int64_t)hk * BD;
        bf16* vp = kp + (int64_t)Hkv * BD;
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                bf16x4 a, c;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = key_ok ? (bf16)(dk[d][r4 * 4 + j] * scale) : (bf16)0.0f;
                    c[j] = key_ok ? (bf16)dv[d][r4 * 4 + j] : (bf16)0.0f;
                }
                *reinterpret_cast<bf16x4*>(kp + d * 32 + 8 * r4 + 4 * hi) = a;
                *reinterpret_cast<bf16x4*>(vp + d * 32 + 8 * r4 + 4 * hi) = c;
            }
    }
}

}  // namespace

// lse / dsum: B * H * T floats each, indexed [sequence][query head][position] (this pair's own layout; the caller only provides the room)
int setok_attention_causal_bwd_mfma(hipStream_t s, const bf16* qkv, const uint8_t* key_mask, const bf16* out, const bf16* dout, bf16* dqkv, int B, int T,
                                    int H, int Hkv, float scale, float* lse, float* dsum) {
    const float c = scale * 1.44269504088896340736f;
    attn_causal_bwd_dq_kernel<<<dim3(cdiv(T, BQ), H, B), 256, 0, s>>>(qkv, key_mask, out, dout, dqkv, T, H, Hkv, scale, c, lse, dsum);
    SETOK_CHECK_LAUNCH("setok_attention_causal_bwd(dq, mfma)");
    attn_causal_bwd_dkv_kernel<<<dim3(cdiv(T, BQ), Hkv, B), 256, 0, s>>>(qkv, key_mask, dout, dqkv, T, H, Hkv, scale, c, lse, dsum);
    SETOK_CHECK_LAUNCH("setok_attention_causal_bwd(dk dv, mfma)");
    return SETOK_OK;
}
