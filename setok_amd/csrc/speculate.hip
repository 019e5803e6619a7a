// speculate.hip — the two integer kernels of draft-and-verify decoding (include/setok_hip.h, "Speculative decoding").
//   setok_spec_accept     after one `extend` over (pending, K drafted tokens): which of the selected tokens each sequence emits, and the cache
//                         mask / positions / loop state that follow from it.  One launch, one workgroup.
//   setok_ngram_propose   the built-in drafter: append the emitted tokens to each sequence's history, then propose the continuation of the most
//                         recent earlier occurrence of the history's trailing n-gram.  One workgroup per sequence.
// Integer arithmetic only, no atomics: every result is a pure function of the inputs, the same bits in every run.
#include "common.h"

constexpr int SPEC_THREADS = 256;
constexpr int SPEC_WAVES = SPEC_THREADS / WAVE;
constexpr int SPEC_MAX_K = 63;                              // K + 1 rows per sequence <= 64: one wave writes a proposal, a round fits FP8W_MAX_M at B = 1
constexpr int NGRAM_MAX_N = 8;

__device__ inline int spec_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline int spec_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_accept_kernel(const int64_t* __restrict__ draft, const int64_t* __restrict__ sel, int B, int K,
                                                                     const int64_t* __restrict__ eos, int n_eos, int max_new,
                                                                     int64_t* __restrict__ seq, int32_t* __restrict__ count,
                                                                     uint8_t* __restrict__ finished, int64_t* __restrict__ pending,
                                                                     uint8_t* __restrict__ key_mask, int64_t* __restrict__ next_pos, int cap, int len0,
                                                                     int64_t* __restrict__ emitted, int32_t* __restrict__ m_out,
                                                                     int32_t* __restrict__ summary) {
    __shared__ int s_max[SPEC_WAVES], s_live[SPEC_WAVES], s_bad[SPEC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int my_max = 0, my_live = 0, my_bad = 0;
    for (int b = tid; b < B; b += SPEC_THREADS) {
        const int64_t* d = draft + (int64_t)b * K;
        const int64_t* e = sel + (int64_t)b * (K + 1);
        int64_t* em = emitted + (int64_t)b * (K + 1);
        uint8_t* km = key_mask + (int64_t)b * cap + len0;
        const int c = count[b];
        int m = 0;
        if (finished[b] == 0 && c >= 0 && c < max_new) {            // (a count outside [0, max_new) cannot emit: the row is handled as finished)
            int n = 0, nd = 0;                                         // leading accepted drafts; leading non-negative drafts (the rows `extend` attended)
            while (nd < K && d[nd] >= 0) ++nd;
            while (n < nd && d[n] == e[n]) ++n;
            m = min(n + 1, max_new - c);
            bool done = false;
            for (int i = 0; i < m && !done; ++i)
                for (int j = 0; j < n_eos; ++j)
                    if (e[i] == eos[j]) { m = i + 1; done = true; break; }
            if (c + m == max_new) done = true;
            int64_t* row = seq + (int64_t)b * max_new + c;
            for (int i = 0; i < m; ++i) {
                const int64_t t = e[i];
                row[i] = t;
                em[i] = t;
                if (t < 0) my_bad = 1;
            }
            count[b] = c + m;
            pending[b] = e[m - 1];
            next_pos[b] = next_pos[b] - (1 + nd) + m;
            if (done) finished[b] = 1;
            else my_live += 1;
        }
        for (int i = m; i <= K; ++i) em[i] = -1;
        for (int i = 0; i <= K; ++i) km[i] = i < m ? 1 : 0;
        m_out[b] = m;
        my_max = max(my_max, m);
    }
    my_max = spec_wave_max(my_max);
    my_live = spec_wave_sum(my_live);
    my_bad = spec_wave_max(my_bad);
    if (lane == 0) { s_max[wave] = my_max; s_live[wave] = my_live; s_bad[wave] = my_bad; }
    __syncthreads();
    if (tid == 0) {
        int mx = 0, live = 0, bad = 0;
#pragma unroll
        for (int w = 0; w < SPEC_WAVES; ++w) { mx = max(mx, s_max[w]); live += s_live[w]; bad |= s_bad[w]; }
        summary[0] = mx; summary[1] = live; summary[2] = bad;
    }
}

extern "C" int setok_spec_accept(void* stream, const int64_t* draft, const int64_t* sel, int B, int K, const int64_t* eos, int n_eos, int max_new,
                                 int64_t* seq, int32_t* count, uint8_t* finished, int64_t* pending, uint8_t* key_mask, int64_t* next_pos, int cap,
                                 int len0, int64_t* emitted, int32_t* m_out, int32_t* summary) {
    SETOK_CHECK_ARG(sel && seq && count && finished && pending && key_mask && next_pos && emitted && m_out && summary && (draft || K == 0) &&
                    (eos || n_eos <= 0), "setok_spec_accept: null operand");
    SETOK_CHECK_ARG(B >= 0, "setok_spec_accept: bad B %d (>= 0)", B);
    SETOK_CHECK_ARG(K >= 0 && K <= SPEC_MAX_K, "setok_spec_accept: bad K %d (0 .. 63)", K);
    SETOK_CHECK_ARG(max_new >= 1, "setok_spec_accept: bad max_new %d (>= 1)", max_new);
    SETOK_CHECK_ARG(n_eos >= 0, "setok_spec_accept: bad n_eos %d (>= 0)", n_eos);
    SETOK_CHECK_ARG(len0 >= 0 && cap >= 1 && (int64_t)len0 + K + 1 <= (int64_t)cap,
                    "setok_spec_accept: slots [len0, len0 + K] = [%d, %d + %d] exceed the cache (cap = %d)", len0, len0, K, cap);
    if (B == 0) return SETOK_OK;
    spec_accept_kernel<<<1, SPEC_THREADS, 0, (hipStream_t)stream>>>(draft, sel, B, K, eos, n_eos, max_new, seq, count, finished, pending, key_mask,
                                                                     next_pos, cap, len0, emitted, m_out, summary);
    SETOK_CHECK_LAUNCH("setok_spec_accept");
    return SETOK_OK;
}

// One workgroup per sequence.  The append comes first; the search then reads the history as it stands after it.  Threads test strided start
// indices j, every thread keeps its largest match, the largest of all meets by a wave max and an LDS max over the waves, and wave 0 writes the
// continuation.  The n-gram loop and its exits are workgroup-uniform.
__global__ __launch_bounds__(SPEC_THREADS) void ngram_propose_kernel(int64_t* hist, int32_t* hist_len, int cap_h,
                                                                       const int64_t* __restrict__ emitted, const int32_t* __restrict__ m_in, int n_emit,
                                                                       int K, int max_ngram, int min_ngram, int64_t* __restrict__ out) {
    __shared__ int s_best[SPEC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    int64_t* h = hist + (int64_t)b * cap_h;
    int64_t* o = out + (int64_t)b * K;
    const int L0 = min(max(hist_len[b], 0), cap_h);
    int mb = 0;
    if (n_emit > 0) mb = min(min(max(m_in[b], 0), n_emit), cap_h - L0);     // (the host refused a history that cannot take it; never past the row)
    if (tid < mb) h[L0 + tid] = emitted[(int64_t)b * n_emit + tid];         // n_emit <= 64 < SPEC_THREADS
    const int L = L0 + mb;
    __syncthreads();                                                        // the appended ids are visible to the whole workgroup; every thread has read L0
    if (tid == 0 && mb > 0) hist_len[b] = L;
    int64_t suf[NGRAM_MAX_N];                                               // suf[t] = h[L - 1 - t]
#pragma unroll
    for (int t = 0; t < NGRAM_MAX_N; ++t) suf[t] = (t < max_ngram && t < L) ? h[L - 1 - t] : -1;
    for (int n = max_ngram; n >= min_ngram; --n) {
        if (L <= n) continue;
        bool neg = false;
#pragma unroll
        for (int t = 0; t < NGRAM_MAX_N; ++t) neg = neg || (t < n && suf[t] < 0);
        if (neg) continue;
        int best = -1;
        for (int j = tid; j <= L - n - 1; j += SPEC_THREADS) {              // h[j .. j + n) against h[L - n .. L): h[j + n - 1 - t] == suf[t]
            bool eq = true;
#pragma unroll
            for (int t = 0; t < NGRAM_MAX_N; ++t)
                if (t < n && eq) eq = h[j + n - 1 - t] == suf[t];
            if (eq) best = j;                                               // ascending j: the last one stays
        }
        best = spec_wave_max(best);
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        best = -1;
#pragma unroll
        for (int w = 0; w < SPEC_WAVES; ++w) best = max(best, s_best[w]);
        __syncthreads();                                                    // the next n overwrites s_best
        if (best >= 0) {
            if (tid < K) { const int idx = best + n + tid; o[tid] = idx < L ? h[idx] : -1; }
            return;
        }
    }
    if (tid < K) o[tid] = -1;
}

extern "C" int setok_ngram_propose(void* stream, int64_t* hist, int32_t* hist_len, int B, int cap_h, int len_max, const int64_t* emitted,
                                   const int32_t* m, int n_emit, int K, int max_ngram, int min_ngram, int64_t* out) {
    SETOK_CHECK_ARG(hist && hist_len && out && (n_emit <= 0 || (emitted && m)), "setok_ngram_propose: null operand");
    SETOK_CHECK_ARG(B >= 0 && cap_h >= 1, "setok_ngram_propose: bad shape B=%d cap_h=%d", B, cap_h);
    SETOK_CHECK_ARG(K >= 1 && K <= SPEC_MAX_K, "setok_ngram_propose: bad K %d (1 .. 63)", K);
    SETOK_CHECK_ARG(n_emit >= 0 && n_emit <= SPEC_MAX_K + 1, "setok_ngram_propose: bad n_emit %d (0 .. 64)", n_emit);
    SETOK_CHECK_ARG(min_ngram >= 1 && min_ngram <= max_ngram && max_ngram <= NGRAM_MAX_N,
                    "setok_ngram_propose: bad n-gram range [%d, %d] (1 <= min_ngram <= max_ngram <= 8)", min_ngram, max_ngram);
    SETOK_CHECK_ARG(len_max >= 0 && len_max <= cap_h,
                    "setok_ngram_propose: hist_len + m > cap_h (the history may reach %d entries, a row holds %d)", len_max, cap_h);
    if (B == 0) return SETOK_OK;
    ngram_propose_kernel<<<B, SPEC_THREADS, 0, (hipStream_t)stream>>>(hist, hist_len, cap_h, emitted, m, n_emit, K, max_ngram, min_ngram, out);
    SETOK_CHECK_LAUNCH("setok_ngram_propose");
    return SETOK_OK;
}
