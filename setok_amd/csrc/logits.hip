// logits.hip — the logits processors of generate() (include/setok_hip.h, "Logits processors").
//   setok_logits_process   a step's logits -> fp32 scores with HuggingFace's repetition penalty, n-gram bans, minimum-length eos ban and token
//                          suppression applied, for B * n rows whose row (b, i) sees sequence b's history plus i tail tokens.  One workgroup per row.
//   setok_history_append   the emitted tokens -> the histories.  One workgroup per sequence, a launch of its own.
// No atomics.  Several writers can aim at one output column (the copy, the penalty of every history position that holds the token, every ban);
// the stored bits do not depend on which of them runs last:
//   - the kernel runs in three phases - copy, penalty, bans - with a __syncthreads() between them: the barrier carries a workgroup-scope
//     release / acquire, so every global store of a phase is ordered before every global store of the next one, whichever wave issues it;
//   - inside the penalty phase every value is computed from the INPUT row, which nothing writes (out may not overlap it: refused on the host),
//     so two history positions that hold the same token store identical bits;
//   - inside the ban phase every store is the same -inf.
#include "common.h"

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_ROWS = 64;                            // n: K + 1 rows per sequence, the bound of setok_spec_accept
constexpr int LP_MAX_NGRAM = 8;                            // the bound of setok_ngram_propose
constexpr int LP_MAX_IDS = 64;                             // eos / suppressed ids: one thread each
constexpr int LP_MAX_V = 1 << 20;                          // the bound of setok_sample_rows
constexpr int HA_THREADS = 64;                             // n_emit <= 64: one thread per appended entry

template <typename T> struct lp_vec;
template <> struct lp_vec<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct lp_vec<bf16> { typedef bf16x8 type; static constexpr int N = 8; };

// Hs of a row: the sequence's history followed by the row's tail.  `tail` is only read at p >= hl, which needs i >= 1 and therefore n > 1.
struct lp_history {
    const int64_t* hist;
    const int64_t* tail;
    int hl;
    __device__ int64_t at(int p) const { return p < hl ? hist[p] : tail[p - hl]; }
};

template <typename T>
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(const T* __restrict__ logits, int64_t ld, int n, int V,
                                                                      const int64_t* __restrict__ hist, const int32_t* __restrict__ hist_len,
                                                                      const int32_t* __restrict__ prompt_len, int cap_h,
                                                                      const int64_t* __restrict__ tail, float penalty, int g, int min_new,
                                                                      const int64_t* __restrict__ eos, int n_eos, const int64_t* __restrict__ suppress,
                                                                      int n_suppress, float* __restrict__ out, int64_t ld_out) {
    typedef typename lp_vec<T>::type VT;
    constexpr int N = lp_vec<T>::N;
    const int tid = threadIdx.x, b = blockIdx.x / n, i = blockIdx.x % n;
    const T* x = logits + (int64_t)blockIdx.x * ld;
    float* o = out + (int64_t)blockIdx.x * ld_out;

    // ---- phase 1, the copy: scalar up to the row's first 16-byte boundary, 16-byte loads behind it, a scalar rest
    const int head = min((int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) / sizeof(T)), V);
    const int nvec = (V - head) / N;
    const bool out16 = (((uintptr_t)(o + head)) & 15u) == 0;                // workgroup-uniform
    if (tid < head) o[tid] = (float)x[tid];
    const VT* xv = reinterpret_cast<const VT*>(x + head);
    for (int k = tid; k < nvec; k += LP_THREADS) {
        const VT v = xv[k];
        float* d = o + head + k * N;
        if (out16) {
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                f32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = (float)v[4 * q + e];
                reinterpret_cast<f32x4*>(d)[q] = w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) d[e] = (float)v[e];
        }
    }
    for (int c = head + nvec * N + tid; c < V; c += LP_THREADS) o[c] = (float)x[c];

    const int hl = min(max(hist_len[b], 0), cap_h);
    const int L = hl + i;
    const lp_history hs{hist + (int64_t)b * cap_h, tail + (int64_t)b * (n - 1), hl};
    __syncthreads();

    // ---- phase 2, the penalty: one history position per thread and stride; the value comes from the input row
    if (penalty != 1.0f) {
        for (int p = tid; p < L; p += LP_THREADS) {
            const int64_t v = hs.at(p);
            if (v >= 0 && v < V) {
                const float xf = (float)x[v];
                o[v] = xf < 0.0f ? xf * penalty : xf / penalty;
            }
        }
    }
    __syncthreads();

    // ---- phase 3, the bans
    if (g >= 1 && L + 1 >= g) {
        int64_t suf[LP_MAX_NGRAM - 1];                                      // suf[t] = Hs[L - 1 - t], t < g - 1: the window that is compared
        bool ok = true;
#pragma unroll
        for (int t = 0; t < LP_MAX_NGRAM - 1; ++t) {
            suf[t] = t < g - 1 ? hs.at(L - 1 - t) : 0;
            ok = ok && suf[t] >= 0 && suf[t] < V;
        }
        if (ok) {
            for (int j = tid; j <= L - g; j += LP_THREADS) {                // Hs[j .. j + g - 1) against the suffix: Hs[j + g - 2 - t] == suf[t]
                bool eq = true;
#pragma unroll
                for (int t = 0; t < LP_MAX_NGRAM - 1; ++t)
                    if (t < g - 1 && eq) eq = hs.at(j + g - 2 - t) == suf[t];
                if (eq) {
                    const int64_t v = hs.at(j + g - 1);
                    if (v >= 0 && v < V) o[v] = -INFINITY;
                }
            }
        }
    }
    if (min_new > 0 && L - prompt_len[b] < min_new && tid < n_eos) {
        const int64_t v = eos[tid];
        if (v >= 0 && v < V) o[v] = -INFINITY;
    }
    if (tid < n_suppress) {
        const int64_t v = suppress[tid];
        if (v >= 0 && v < V) o[v] = -INFINITY;
    }
}

extern "C" int setok_logits_process(void* stream, int dtype, const void* logits, int64_t ld, int B, int n, int V, const int64_t* hist,
                                    const int32_t* hist_len, const int32_t* prompt_len, int cap_h, const int64_t* tail, float penalty, int ngram,
                                    int min_new, const int64_t* eos, int n_eos, const int64_t* suppress, int n_suppress, float* out, int64_t ld_out) {
    SETOK_CHECK_ARG(logits && hist && hist_len && prompt_len && out && (tail || n <= 1) && (eos || n_eos <= 0) && (suppress || n_suppress <= 0),
                    "setok_logits_process: null operand");
    SETOK_CHECK_ARG(B >= 0 && n >= 1 && n <= LP_MAX_ROWS && V >= 1 && V <= LP_MAX_V && ld >= V && ld_out >= V && cap_h >= 1,
                    "setok_logits_process: bad shape B=%d n=%d (1 .. 64) V=%d (1 .. 2^20) ld=%lld ld_out=%lld cap_h=%d", B, n, V, (long long)ld,
                    (long long)ld_out, cap_h);
    SETOK_CHECK_ARG(ngram >= 0 && ngram <= LP_MAX_NGRAM, "setok_logits_process: bad ngram %d (0 .. 8)", ngram);
    SETOK_CHECK_ARG(min_new >= 0, "setok_logits_process: bad min_new %d (>= 0)", min_new);
    SETOK_CHECK_ARG(n_eos >= 0 && n_eos <= LP_MAX_IDS && n_suppress >= 0 && n_suppress <= LP_MAX_IDS,
                    "setok_logits_process: bad id count n_eos=%d n_suppress=%d (0 .. 64)", n_eos, n_suppress);
    SETOK_CHECK_ARG(penalty == penalty && penalty > 0.0f && penalty < INFINITY, "setok_logits_process: bad penalty %g (finite, > 0)", (double)penalty);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_logits_process: bad dtype %d", dtype);
    const int64_t rows = (int64_t)B * n;
    if (rows == 0) return SETOK_OK;
    const uintptr_t a0 = (uintptr_t)logits, a1 = a0 + (uintptr_t)((rows - 1) * ld + V) * (dtype == SETOK_F32 ? 4u : 2u);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((rows - 1) * ld_out + V) * 4u;
    SETOK_CHECK_ARG(a1 <= o0 || o1 <= a0, "setok_logits_process: out overlaps logits");
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_T("setok_logits_process",
               (logits_process_kernel<bf16><<<(int)rows, LP_THREADS, 0, s>>>((const bf16*)logits, ld, n, V, hist, hist_len, prompt_len, cap_h, tail, penalty,
                                                                             ngram, min_new, eos, n_eos, suppress, n_suppress, out, ld_out)),
               (logits_process_kernel<float><<<(int)rows, LP_THREADS, 0, s>>>((const float*)logits, ld, n, V, hist, hist_len, prompt_len, cap_h, tail, penalty,
                                                                              ngram, min_new, eos, n_eos, suppress, n_suppress, out, ld_out)));
    SETOK_CHECK_LAUNCH("setok_logits_process");
    return SETOK_OK;
}

// One workgroup per sequence; a thread per appended entry.  The length is read by every thread before the barrier and written by one behind it.
__global__ __launch_bounds__(HA_THREADS) void history_append_kernel(int64_t* __restrict__ hist, int32_t* __restrict__ hist_len, int cap_h,
                                                                      const int64_t* __restrict__ emitted, const int32_t* __restrict__ m_in, int n_emit) {
    const int tid = threadIdx.x, b = blockIdx.x;
    const int L0 = min(max(hist_len[b], 0), cap_h);
    int mb = m_in ? min(max(m_in[b], 0), n_emit) : n_emit;
    mb = min(mb, cap_h - L0);                                               // (the host refused a history that cannot take it; never past the row)
    if (tid < mb) hist[(int64_t)b * cap_h + L0 + tid] = emitted[(int64_t)b * n_emit + tid];
    __syncthreads();
    if (tid == 0 && mb > 0) hist_len[b] = L0 + mb;
}

extern "C" int setok_history_append(void* stream, int64_t* hist, int32_t* hist_len, int B, int cap_h, int len_max, const int64_t* emitted,
                                    const int32_t* m, int n_emit) {
    SETOK_CHECK_ARG(hist && hist_len && (emitted || n_emit <= 0), "setok_history_append: null operand");
    SETOK_CHECK_ARG(B >= 0 && cap_h >= 1, "setok_history_append: bad shape B=%d cap_h=%d", B, cap_h);
    SETOK_CHECK_ARG(n_emit >= 0 && n_emit <= HA_THREADS, "setok_history_append: bad n_emit %d (0 .. 64)", n_emit);
    SETOK_CHECK_ARG(len_max >= 0 && len_max <= cap_h,
                    "setok_history_append: hist_len + m > cap_h (the history may reach %d entries, a row holds %d)", len_max, cap_h);
    if (B == 0 || n_emit == 0) return SETOK_OK;
    history_append_kernel<<<B, HA_THREADS, 0, (hipStream_t)stream>>>(hist, hist_len, cap_h, emitted, m, n_emit);
    SETOK_CHECK_LAUNCH("setok_history_append");
    return SETOK_OK;
}
