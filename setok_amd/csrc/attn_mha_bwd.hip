// attn_mha_bwd.hip — backward of the reconstruction decoder's attentions and of its pixel loss (include/setok_hip.h: setok_mha_bwd,
// setok_pixel_loss_bwd).
//
// setok_mha_bwd serves both shapes of the decoder with strided operands, the operand layout of the forward setok_cross_attention
// (attn_vit.hip): query rows in groups of q_len, one group per segment; the segment's key / value rows either uniform (kv_offsets == NULL,
// max_kv rows per segment: self-attention passes max_kv = q_len and the three column windows of one fused qkv buffer) or ragged
// (kv_offsets, the Q-Former's cross-attention to each image's tokens).  dq, dk, dv go to row views of their own strides: the three windows
// of one dqkv buffer, or dq plus the [dk | dv] halves of the buffer the fused k|v weight's linear backward takes as dY.
//
// The forward kernels are not changed, so nothing is saved from them: the log-sum-exp and delta_i = do_i . o_i are recomputed here.
//   s_ij = scale q_i.k_j,  p_ij = exp(s_ij - lse_i),  ds_ij = p_ij (do_i.v_j - delta_i)
//   dq_i = scale sum_j ds_ij k_j,  dk_j = scale sum_i ds_ij q_i,  dv_j = sum_i p_ij do_i
// Head dims 48 and 64 in the 16-bit type run the MFMA kernels below.  Every other shape, fp32, and SETOK_ATTN_BWD_GENERIC=1 run the generic
// wave-per-(row, head) pair that setok_attention_bwd uses too (norm_attn.hip, setok_attention_bwd_generic).  In both forms a query kernel
// computes lse_i, delta_i (kept in `ws`) and dq_i, then a key kernel dk_j and dv_j by a loop over its segment's query rows in row order.
// No atomics; every sum runs in a fixed order, so two runs give the same bits, and a segment's result does not depend on its neighbours.
#include "common.h"

int setok_attention_bwd_generic(const char* what, hipStream_t s, int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                                const void* o, int64_t ldo, const void* dout, int64_t lddo, void* dq, int64_t lddq, void* dk, void* dv, int64_t lddkv,
                                const int32_t* seg_offsets, int n_segs, int seg_len, int q_len, int rows, int H, int Dh, float scale,
                                float* lse, float* dsum, int skip_long);                                     // norm_attn.hip

namespace {

// the key rows [k0, k1) of group s (the rule of norm_attn.hip's attn_rows)
__device__ inline void kv_range(const int32_t* kv_offsets, int s, int max_kv, int& k0, int& k1) {
    if (kv_offsets) { k0 = kv_offsets[s]; k1 = kv_offsets[s + 1]; if (k1 - k0 > max_kv) k1 = k0 + max_kv; }
    else { k0 = s * max_kv; k1 = k0 + max_kv; }
}

// ---- d(pixel loss) / d(patch rows): the backward of setok_pixel_loss and setok_unpatchify in one pass ---------------------------------------
// One thread per element of the (B gh gw, ld) patch-row matrix; column c < 3 p^2 is (pi, qi, ch) = (c / 3p, (c / 3) % p, c % 3) of the
// 'n (h w) (p q c) -> n c (h p) (w q)' rearrangement, columns [3 p^2, ld) are the GEMM's pad and get zeros.
template <typename T>
__global__ __launch_bounds__(256) void pixel_loss_bwd_kernel(const T* __restrict__ pred, const T* __restrict__ gold, const float* __restrict__ upstream,
                                                             int kind, T* __restrict__ dpatch, int64_t ld, int B, int gh, int gw, int p) {
    const int64_t rows = (int64_t)B * gh * gw;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * ld) return;
    const int64_t r = e / ld;
    const int c = (int)(e - r * ld);
    float g = 0.f;
    if (c < 3 * p * p) {
        const int b = (int)(r / (gh * gw)), hw = (int)(r % (gh * gw)), hh = hw / gw, w = hw % gw;
        const int pi = c / (3 * p), qi = (c / 3) % p, ch = c % 3;
        const int64_t W = (int64_t)gw * p, Hh = (int64_t)gh * p;
        const int64_t i = (((int64_t)b * 3 + ch) * Hh + (int64_t)hh * p + pi) * W + (int64_t)w * p + qi;
        const float up = upstream[0];
        const float x = Elem<T>::ld(pred + i);
        if (kind == 2) {
            g = x * up;
        } else {
            const float d = x - Elem<T>::ld(gold + i);
            const float inv_n = 1.0f / (float)(rows * 3 * p * p);
            const float sg = d != d ? d : (float)((d > 0.f) - (d < 0.f));        // torch.sign: NaN stays NaN, sign(0) = 0
            g = kind == 0 ? 2.0f * d * inv_n * up : sg * inv_n * up;
        }
    }
    Elem<T>::st(dpatch + r * ld + c, g);
}

// ---- MFMA form: head dims 48 and 64, 16-bit elements (v_mfma_f32_16x16x32, fp32 accumulation) ---------------------------------------------
// Fragments (attn_vit.hip's convention): A lane = row l & 15, k-slots 8 (l >> 4) .. + 7; B lane = column l & 15, the same k-slots; D lane = rows
// 4 (l >> 4) .. + 3 of column l & 15.  Every tile starts at its segment's first query / key row, so a segment's bits do not depend on the others.
//
// Kernel A (dQ): one wave per 16 query rows, the keys streamed in 32-row steps from L2.
//   S^T tile (16 keys x 16 queries) = K Q^T and dP^T = V dO^T: A = K / V rows, B = Q / dO rows — each lane owns ONE query, so its log-sum-exp
//   and delta = do.o are per-lane values (a meeting of the four lanes of a query; two passes over the keys: the exact lse first).
//   dQ^T (d x queries) += K^T dS^T over 32 keys: B = dS^T of two adjacent key tiles packed in place (slots 0-3: keys 4 g + i of the first tile,
//   slots 4-7: of the second) — no LDS round trip; A = K^T read as 8 scalars per lane whose keys are exactly that permutation.
// Kernel B (dK, dV): one wave per 16 key rows, the segment's queries streamed in 32-row steps.
//   S tile (16 queries x 16 keys) = Q K^T, dP = dO V^T; P = exp(scale s - lse_q), dS = P (dP - delta_q) with lse / delta from kernel A;
//   dV^T += dO^T P and dK^T += Q^T dS over 32 queries, P / dS packed the same way, dO^T / Q^T as permuted scalar reads.
// P and dS are rounded to the 16-bit type for the second products (fp32 accumulation throughout).
constexpr int MM_WAVES = 4;                     // waves per workgroup; each owns 16 rows

__device__ inline bf16x8 ld_frag(const bf16* p, bool ok) {
    if (ok) return *reinterpret_cast<const bf16x8*>(p);
    bf16x8 z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z[i] = (bf16)0.f;
    return z;
}
__device__ inline float quad_sum(float x) { x += __shfl_xor(x, 16); return x + __shfl_xor(x, 32); }        // over lanes {l, l^16, l^32, l^48}
__device__ inline float quad_max(float x) { x = fmaxf(x, __shfl_xor(x, 16)); return fmaxf(x, __shfl_xor(x, 32)); }
__device__ inline int perm32(int g, int j) { return j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4); }          // k-slot j of lane group g -> row of a 32-row step
__device__ inline f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

template <int DH>
__global__ __launch_bounds__(64 * MM_WAVES) void mha_bwd_q_mfma(const bf16* __restrict__ q, int64_t ldq, const bf16* __restrict__ k,
                                                               const bf16* __restrict__ v, int64_t ldkv, const int32_t* __restrict__ kv_offsets,
                                                               int q_len, int max_kv, const bf16* __restrict__ o, int64_t ldo,
                                                               const bf16* __restrict__ dout, int64_t lddo, bf16* __restrict__ dq, int64_t lddq,
                                                               float* __restrict__ lse_ws, float* __restrict__ dsum_ws, int H, float scale, int qblocks) {
    constexpr int NT = DH / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = blockIdx.x / qblocks, h = blockIdx.y;
    const int ql0 = (blockIdx.x % qblocks) * 16 * MM_WAVES + wave * 16;
    if (ql0 >= q_len) return;
    int k0, k1;
    kv_range(kv_offsets, seg, max_kv, k0, k1);
    const int c = lane & 15, g = lane >> 4;
    const bool qok = ql0 + c < q_len;
    const int64_t row = (int64_t)seg * q_len + (qok ? ql0 + c : ql0);
    const int64_t hc = (int64_t)h * DH;
    bf16x8 qf[2], df[2];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int d = ks * 32 + g * 8;
        const bool ok = qok && d < DH;
        qf[ks] = ld_frag(q + row * ldq + hc + d, ok);
        df[ks] = ld_frag(dout + row * lddo + hc + d, ok);
        const bf16x8 of = ld_frag(o + row * ldo + hc + d, ok);
#pragma unroll
        for (int i = 0; i < 8; ++i) dl = fmaf((float)df[ks][i], (float)of[i], dl);
    }
    const float delta = quad_sum(dl);
    // pass 1: the exact log-sum-exp of this lane's query
    float m = -INFINITY, l = 0.f;
    for (int kb = k0; kb < k1; kb += 16) {
        const bool kok = kb + c < k1;
        const int64_t kr = kok ? kb + c : k0;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int d = ks * 32 + g * 8;
            s = mfma16(ld_frag(k + kr * ldkv + hc + d, kok && d < DH), qf[ks], s);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (kb + 4 * g + i >= k1) continue;
            const float x = s[i] * scale;
            const float mn = fmaxf(m, x);
            l = l * expf(m - mn) + expf(x - mn);
            m = mn;
        }
    }
    const float M = quad_max(m);
    const float lse = M + logf(quad_sum(m == -INFINITY ? 0.f : l * expf(m - M)));
    // pass 2: dS^T tiles and dQ^T
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = {0.f, 0.f, 0.f, 0.f};
    for (int kb = k0; kb < k1; kb += 32) {
        bf16x8 dsp;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int kt = kb + 16 * t;
            const bool kok = kt + c < k1;
            const int64_t kr = kok ? kt + c : k0;
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int d = ks * 32 + g * 8;
                const bool ok = kok && d < DH;
                s = mfma16(ld_frag(k + kr * ldkv + hc + d, ok), qf[ks], s);
                dp = mfma16(ld_frag(v + kr * ldkv + hc + d, ok), df[ks], dp);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = kt + 4 * g + i < k1 ? expf(s[i] * scale - lse) : 0.f;
                dsp[4 * t + i] = (bf16)(p * (dp[i] - delta));
            }
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            bf16x8 kt8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = kb + perm32(g, j);
                kt8[j] = key < k1 ? k[(int64_t)key * ldkv + hc + 16 * n + c] : (bf16)0.f;
            }
            acc[n] = mfma16(kt8, dsp, acc[n]);
        }
    }
    if (!qok) return;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[row * lddq + hc + 16 * n + 4 * g + i] = (bf16)(acc[n][i] * scale);
    if (g == 0) { lse_ws[row * H + h] = lse; dsum_ws[row * H + h] = delta; }
}

template <int DH>
__global__ __launch_bounds__(64 * MM_WAVES) void mha_bwd_kv_mfma(const bf16* __restrict__ q, int64_t ldq, const bf16* __restrict__ k,
                                                                const bf16* __restrict__ v, int64_t ldkv, const int32_t* __restrict__ kv_offsets,
                                                                int q_len, int max_kv, const bf16* __restrict__ dout, int64_t lddo,
                                                                bf16* __restrict__ dk, bf16* __restrict__ dv, int64_t lddkv,
                                                                const float* __restrict__ lse_ws, const float* __restrict__ dsum_ws, int H, float scale,
                                                                int kblocks) {
    constexpr int NT = DH / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg = blockIdx.x / kblocks, h = blockIdx.y;
    int k0, k1;
    kv_range(kv_offsets, seg, max_kv, k0, k1);
    const int j0 = k0 + (blockIdx.x % kblocks) * 16 * MM_WAVES + wave * 16;
    if (j0 >= k1) return;
    const int c = lane & 15, g = lane >> 4;
    const bool kok = j0 + c < k1;
    const int64_t key = kok ? j0 + c : j0;
    const int64_t hc = (int64_t)h * DH;
    const int64_t r0 = (int64_t)seg * q_len;
    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int d = ks * 32 + g * 8;
        kf[ks] = ld_frag(k + key * ldkv + hc + d, kok && d < DH);
        vf[ks] = ld_frag(v + key * ldkv + hc + d, kok && d < DH);
    }
    f32x4 adk[NT], adv[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) { adk[n] = {0.f, 0.f, 0.f, 0.f}; adv[n] = {0.f, 0.f, 0.f, 0.f}; }
    for (int qb = 0; qb < q_len; qb += 32) {
        bf16x8 pp, dsp;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qt = qb + 16 * t;
            const bool qok = qt + c < q_len;
            const int64_t qr = r0 + (qok ? qt + c : 0);
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int d = ks * 32 + g * 8;
                const bool ok = qok && d < DH;
                s = mfma16(ld_frag(q + qr * ldq + hc + d, ok), kf[ks], s);
                dp = mfma16(ld_frag(dout + qr * lddo + hc + d, ok), vf[ks], dp);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qq = qt + 4 * g + i;
                float p = 0.f, dl = 0.f;
                if (qq < q_len) {
                    p = expf(s[i] * scale - lse_ws[(r0 + qq) * H + h]);
                    dl = dsum_ws[(r0 + qq) * H + h];
                }
                pp[4 * t + i] = (bf16)p;
                dsp[4 * t + i] = (bf16)(p * (dp[i] - dl));
            }
        }
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            bf16x8 qt8, dt8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int qq = qb + perm32(g, j);
                const bool ok = qq < q_len;
                qt8[j] = ok ? q[(r0 + qq) * ldq + hc + 16 * n + c] : (bf16)0.f;
                dt8[j] = ok ? dout[(r0 + qq) * lddo + hc + 16 * n + c] : (bf16)0.f;
            }
            adv[n] = mfma16(dt8, pp, adv[n]);
            adk[n] = mfma16(qt8, dsp, adk[n]);
        }
    }
    if (!kok) return;
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dk[key * lddkv + hc + 16 * n + 4 * g + i] = (bf16)(adk[n][i] * scale);
            dv[key * lddkv + hc + 16 * n + 4 * g + i] = (bf16)adv[n][i];
        }
}

// SETOK_ATTN_BWD_GENERIC=1: the wave-per-row kernels for every shape (A/B runs; read per call so one process can compare the forms)
inline bool mfma_forced_off() {
    const char* e = getenv("SETOK_ATTN_BWD_GENERIC");
    return e && e[0] == '1';
}

template <int DH>
void launch_mfma(hipStream_t s, const bf16* q, int64_t ldq, const bf16* k, const bf16* v, int64_t ldkv, const int32_t* kv_offsets, int n_segs,
                 int q_len, int max_kv, const bf16* out, int64_t ldo, const bf16* dout, int64_t lddo, bf16* dq, int64_t lddq, bf16* dk, bf16* dv,
                 int64_t lddkv, int H, float scale, float* lse, float* dsum) {
    const int rows_per_wg = 16 * MM_WAVES;
    const int qblocks = cdiv(q_len, rows_per_wg), kblocks = cdiv(max_kv, rows_per_wg);
    mha_bwd_q_mfma<DH><<<dim3(n_segs * qblocks, H), 64 * MM_WAVES, 0, s>>>(q, ldq, k, v, ldkv, kv_offsets, q_len, max_kv, out, ldo, dout, lddo, dq,
                                                                          lddq, lse, dsum, H, scale, qblocks);
    mha_bwd_kv_mfma<DH><<<dim3(n_segs * kblocks, H), 64 * MM_WAVES, 0, s>>>(q, ldq, k, v, ldkv, kv_offsets, q_len, max_kv, dout, lddo, dk, dv,
                                                                           lddkv, lse, dsum, H, scale, kblocks);
}

}  // namespace

extern "C" int setok_mha_bwd(void* stream, int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                             const int32_t* kv_offsets, int n_segs, int q_len, int max_kv, const void* out, int64_t ldo, const void* dout,
                             int64_t lddo, void* dq, int64_t lddq, void* dk, void* dv, int64_t lddkv, int H, int Dh, float scale, float* ws) {
    SETOK_CHECK_ARG(q && k && v && out && dout && dq && dk && dv && ws, "setok_mha_bwd: null operand");
    const int V = dtype == SETOK_BF16 ? 8 : 4;
    SETOK_CHECK_ARG(n_segs >= 0 && q_len > 0 && max_kv > 0 && H > 0 && Dh > 0 && Dh % 8 == 0 && Dh <= 64 * V * AT_MAXC,
                    "setok_mha_bwd: bad shape n_segs=%d q_len=%d max_kv=%d H=%d Dh=%d", n_segs, q_len, max_kv, H, Dh);
    const int64_t C = (int64_t)H * Dh;
    SETOK_CHECK_ARG(ldq >= C && ldkv >= C && ldo >= C && lddo >= C && lddq >= C && lddkv >= C, "setok_mha_bwd: a row stride is below H*Dh");
    SETOK_CHECK_ARG(ldq % V == 0 && ldkv % V == 0 && ldo % V == 0 && lddo % V == 0 && lddq % V == 0 && lddkv % V == 0 &&
                    aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) && aligned16(dq) && aligned16(dk) && aligned16(dv),
                    "setok_mha_bwd: operands and row strides must be 16-byte aligned");
    SETOK_CHECK_ARG((int64_t)n_segs * q_len <= INT32_MAX && (int64_t)n_segs * max_kv <= INT32_MAX, "setok_mha_bwd: too many rows");
    if (n_segs == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int rows = n_segs * q_len;
    float* lse = ws; float* dsum = ws + (int64_t)rows * H;
    if (dtype == SETOK_BF16 && (Dh == 48 || Dh == 64) && !mfma_forced_off()) {
        if (Dh == 48)
            launch_mfma<48>(s, (const bf16*)q, ldq, (const bf16*)k, (const bf16*)v, ldkv, kv_offsets, n_segs, q_len, max_kv, (const bf16*)out, ldo,
                            (const bf16*)dout, lddo, (bf16*)dq, lddq, (bf16*)dk, (bf16*)dv, lddkv, H, scale, lse, dsum);
        else
            launch_mfma<64>(s, (const bf16*)q, ldq, (const bf16*)k, (const bf16*)v, ldkv, kv_offsets, n_segs, q_len, max_kv, (const bf16*)out, ldo,
                            (const bf16*)dout, lddo, (bf16*)dq, lddq, (bf16*)dk, (bf16*)dv, lddkv, H, scale, lse, dsum);
        SETOK_CHECK_LAUNCH("setok_mha_bwd");
        return SETOK_OK;
    }
    return setok_attention_bwd_generic("setok_mha_bwd", s, dtype, q, ldq, k, v, ldkv, out, ldo, dout, lddo, dq, lddq, dk, dv, lddkv, kv_offsets,
                                       n_segs, max_kv, q_len, rows, H, Dh, scale, lse, dsum, 0);
}

extern "C" int setok_pixel_loss_bwd(void* stream, int dtype, const void* pred, const void* gold, int kind, const float* upstream, void* dpatches,
                                    int64_t ld, int B, int gh, int gw, int p) {
    SETOK_CHECK_ARG(pred && upstream && dpatches && (gold || kind == 2), "setok_pixel_loss_bwd: null operand");
    SETOK_CHECK_ARG(kind >= 0 && kind <= 2, "setok_pixel_loss_bwd: bad kind %d", kind);
    SETOK_CHECK_ARG(B >= 0 && gh > 0 && gw > 0 && p > 0 && ld >= 3 * p * p, "setok_pixel_loss_bwd: bad shape B=%d gh=%d gw=%d p=%d ld=%lld", B, gh, gw, p,
                    (long long)ld);
    const int64_t n = (int64_t)B * gh * gw * ld;
    if (n == 0) return SETOK_OK;
    SETOK_CHECK_ARG(n / 256 < INT32_MAX, "setok_pixel_loss_bwd: too many elements");
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)((n + 255) / 256);
    DISPATCH_T("setok_pixel_loss_bwd",
        (pixel_loss_bwd_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)pred, (const bf16*)gold, upstream, kind, (bf16*)dpatches, ld, B, gh, gw, p)),
        (pixel_loss_bwd_kernel<float><<<grid, 256, 0, s>>>((const float*)pred, (const float*)gold, upstream, kind, (float*)dpatches, ld, B, gh, gw, p)));
    SETOK_CHECK_LAUNCH("setok_pixel_loss_bwd");
    return SETOK_OK;
}
