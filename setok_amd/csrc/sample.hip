// sample.hip — sampled token selection for the decode loop: temperature, top-k and top-p in ONE launch per step (include/setok_hip.h, "Sampling").
//   setok_sample_rows        out[r] = the token row r of the logits draws with the uniform u[r]
//   setok_sample_rows_each   the same launch with (temperature, top_k, top_p) per row; a row with temperature 0 takes the argmax instead
//
// The draw is a pure function of (logits row, u, temperature, top_k, top_p): the uniform is an input, every sum is an INTEGER sum of the
// fixed-point weights w_i = rint(exp(s_i - max s) * 2^32), so no result depends on the order in which lanes or waves arrive (LDS integer atomics
// are exact in any association) and two runs give the same bits.
//
// One workgroup of 1024 threads per row.  The row is read from memory once (16-byte pieces), scaled to s_i = logit_i / temperature in fp32 and kept
// in LDS (V <= SAMPLE_LDS_MAX_V; a longer row, V = 128256, is re-read through L2 by every pass).  Each filter's threshold is found by a select on
// the order-preserving 32-bit key of s_i with a 256-bin LDS histogram of (count, integer mass) per bin: the count decides top-k, the mass top-p.
// The first round buckets by VALUE (1/8 nat below the row maximum per bin): the high byte of a float key is sign + 7 exponent bits and would put
// nearly the whole vocabulary into two or three bins, i.e. into 64-way same-address atomics; the value buckets spread it.  Four 8-bit radix rounds
// on the key then run inside the chosen bucket only (a few hundred elements at most in a decode row), which makes the threshold exact.
// The inverse CDF is a scan in index order: every wave owns a contiguous index range and sums it, the wave whose range holds the target scans it.
#include "common.h"
#include <math.h>

typedef unsigned long long u64;

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / WAVE;
constexpr int SAMPLE_LDS_MAX_V = 36864;                  // 144 KiB of fp32 scores + the static block below stays inside the CU's 160 KiB
constexpr int SAMPLE_MAX_V = 1 << 20;                    // V * 2^32 < 2^52: every mass fits a uint64 and is exact in a double

struct SampleShared {
    unsigned cnt[256];
    u64 mass[256];
    u64 wtot[SAMPLE_WAVES];
    float wmax[SAMPLE_WAVES];
    int wflag[SAMPLE_WAVES];
    int sel_digit;
    unsigned sel_cnt_above;
    u64 sel_mass_above, sel_mass_at;
};

// s -> a uint32 whose unsigned order is the order of the floats (-0 and +0 share a key: they compare equal)
__device__ inline unsigned sample_key(float s) {
    unsigned u = __builtin_bit_cast(unsigned, s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the fixed-point weight: 2^32 for the row maximum, 0 below 2^-33 of it (and for -inf)
__device__ inline u64 sample_weight(float s, float m) { return (u64)rintf(expf(s - m) * 4294967296.0f); }
// round 0 of a select: 8 bins per nat below the maximum, everything 31.875 nats or more below it (weight exactly 0) in bin 0; monotone in s
__device__ inline int sample_vbin(float s, float m) { return 255 - (int)fminf((m - s) * 8.0f, 255.0f); }

__device__ inline u64 shfl_down_u64(u64 v, int o) {
    const unsigned lo = __shfl_down((unsigned)v, o, 64), hi = __shfl_down((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 shfl_up_u64(u64 v, int o) {
    const unsigned lo = __shfl_up((unsigned)v, o, 64), hi = __shfl_up((unsigned)(v >> 32), o, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 shfl_u64(u64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// The scaled scores of one row: out of LDS, or (a row too long for it) recomputed from the logits, which gives the same bits.
template <typename T, bool IN_LDS>
struct SampleRow {
    const T* g;
    const float* l;
    float temperature;
    __device__ inline float s(int i) const {
        if constexpr (IN_LDS) return l[i];
        else return (float)g[i] / temperature;
    }
};

// Wave 0, after a histogram round: the digit the threshold lies in.  BY_MASS = false: the largest digit d with #{digit >= d} >= kk (top-k);
// BY_MASS = true: the smallest non-empty digit d with (above + mass of the digits > d) < P (top-p).  Lane L owns bins 4L .. 4L + 3.
template <bool BY_MASS>
__device__ inline void sample_pick_digit(SampleShared& sh, unsigned kk, u64 above, double P) {
    const int lane = threadIdx.x;
    unsigned c[4], lc = 0;
    u64 ms[4], lm = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { c[e] = sh.cnt[4 * lane + e]; ms[e] = sh.mass[4 * lane + e]; lc += c[e]; lm += ms[e]; }
    unsigned sc = lc;
    u64 sm = lm;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                                 // inclusive suffix sums over the lanes
        const unsigned tc = __shfl_down(sc, o, 64);
        const u64 tm = shfl_down_u64(sm, o);
        if (lane + o < 64) { sc += tc; sm += tm; }
    }
    unsigned ca = sc - lc;                                             // strictly above this lane's bins
    u64 ma = sm - lm;
    int cand = BY_MASS ? 256 : -1;
    unsigned cand_ca = 0;
    u64 cand_ma = 0, cand_at = 0;
#pragma unroll
    for (int e = 3; e >= 0; --e) {                                     // descending digits
        bool ok;
        if constexpr (BY_MASS) ok = ms[e] > 0 && (double)(above + ma) < P;
        else ok = ca + c[e] >= kk;
        if (ok && (BY_MASS || cand < 0)) { cand = 4 * lane + e; cand_ca = ca; cand_ma = ma; cand_at = ms[e]; }
        ca += c[e]; ma += ms[e];
    }
    int best = cand;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(best, o, 64);
        best = BY_MASS ? min(best, t) : max(best, t);
    }
    if (best < 0 || best > 255) {                                      // cannot happen (the row maximum always qualifies); stay defined
        if (lane == 0) { sh.sel_digit = BY_MASS ? 255 : 0; sh.sel_cnt_above = 0; sh.sel_mass_above = 0; sh.sel_mass_at = 0; }
    } else if (cand == best) {
        sh.sel_digit = best; sh.sel_cnt_above = cand_ca; sh.sel_mass_above = cand_ma; sh.sel_mass_at = cand_at;
    }
}

// The threshold key of one filter among the elements with key >= floor_key.  BY_MASS = false: the kk-th largest key.  BY_MASS = true: the smallest
// key t whose mass of strictly larger keys is < P.  *w_ge = the mass of the eligible keys >= the result.  Called by the whole workgroup.
template <bool BY_MASS, class Row>
__device__ inline unsigned sample_select(const Row& row, int V, float m, unsigned floor_key, unsigned kk, double P, SampleShared& sh, u64* w_ge) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0;
    u64 above = 0;
    int vb = 0;
    for (int round = 0; round < 5; ++round) {
        const int shift = 32 - 8 * round;                              // rounds 1-4: key bits [shift, shift + 8)
        const unsigned hi_mask = round <= 1 ? 0u : ~0u << (shift + 8);
        if (tid < 256) { sh.cnt[tid] = 0; sh.mass[tid] = 0; }
        __syncthreads();
        for (int base = 0; base < V; base += SAMPLE_THREADS) {         // wave-uniform trip count: the ballot below sees whole waves
            const int i = base + tid;
            bool act = i < V;
            float s = 0.f;
            unsigned key = 0;
            int bin = 0;
            if (act) {
                s = row.s(i);
                key = sample_key(s);
                bin = sample_vbin(s, m);
                act = key >= floor_key;
                if (round > 0) { act = act && bin == vb && (key & hi_mask) == prefix; bin = (key >> shift) & 255u; }
            }
            if (round == 0) {                                          // bin 0 of the value round holds every far-away token, weight 0: one counted add per wave
                const bool far = act && bin == 0;
                const u64 fb = __ballot(far);
                if (fb != 0 && lane == __ffsll((long long)fb) - 1) atomicAdd(&sh.cnt[0], (unsigned)__popcll(fb));
                act = act && !far;
            }
            if (act) {
                atomicAdd(&sh.cnt[bin], 1u);
                const u64 w = sample_weight(s, m);
                if (w) atomicAdd(&sh.mass[bin], w);
            }
        }
        __syncthreads();
        if (tid < 64) sample_pick_digit<BY_MASS>(sh, kk, above, P);
        __syncthreads();
        const int d = sh.sel_digit;
        kk -= sh.sel_cnt_above;
        above += sh.sel_mass_above;
        if (round == 0) vb = d;
        else prefix |= (unsigned)d << shift;
        if (round == 4) *w_ge = above + sh.sel_mass_at;
        __syncthreads();                                               // the next round zeroes the histogram and the pick overwrites sel_*
    }
    return prefix;
}

// Where a row's three parameters come from.  Both sources give every thread of a workgroup the same values, so the kernel's branches on them are
// workgroup-uniform.  setok_sample_rows: the launch's scalars, validated on the host - every row is drawn from.
struct SampleScalars {
    float temperature;
    int top_k;
    float top_p;
    static constexpr bool PER_ROW = false;
    __device__ inline float t(int) const { return temperature; }
    __device__ inline int k(int) const { return top_k; }
    __device__ inline float p(int) const { return top_p; }
};
// setok_sample_rows_each: (rows) arrays, nothing validated on the host - the kernel classifies the row before it uses a value.
struct SampleArrays {
    const float* temperature;
    const int* top_k;
    const float* top_p;
    static constexpr bool PER_ROW = true;
    __device__ inline float t(int r) const { return temperature[r]; }
    __device__ inline int k(int r) const { return top_k[r]; }
    __device__ inline float p(int r) const { return top_p[r]; }
};

// f(i, float(g[i])) for every i < V, each element once: 16-byte pieces between the row's first 16-byte boundary and its last whole piece.
template <typename T, class F>
__device__ inline void sample_read_row(const T* g, int V, F&& f) {
    constexpr int VEC = Elem<T>::VEC;
    const int tid = threadIdx.x;
    int head = (int)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) / sizeof(T));          // elements before the first 16-byte boundary
    if (head > V) head = V;
    const int nvec = (V - head) / VEC, tail0 = head + nvec * VEC;
    if (tid < head) f(tid, (float)g[tid]);
    for (int v = tid; v < nvec; v += SAMPLE_THREADS) {
        float x[VEC];
        ld_vec<T>(g + head + v * VEC, x);
#pragma unroll
        for (int e = 0; e < VEC; ++e) f(head + v * VEC + e, x[e]);
    }
    if (tail0 + tid < V) f(tail0 + tid, (float)g[tail0 + tid]);                            // fewer than VEC elements
}

// A greedy row (temperature 0): setok_argmax_rows' rule - the lowest index of the maximum of the logits as they are, a NaN counting as the maximum,
// -0 == +0 - as one integer maximum of (order key of the value, V's complement of the index): exact in any association.  probs: one-hot.
template <typename T>
__device__ inline void sample_greedy_row(const T* g, int V, SampleShared& sh, int64_t* out_r, float* probs_r) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr u64 LOW = (u64)SAMPLE_MAX_V - 1;                         // i <= 2^20 - 1: 20 bits under a 33-bit key
    u64 best = 0;                                                      // below every element's word (a key is never 0 ... and V >= 1)
    sample_read_row(g, V, [&](int i, float x) {
        const u64 key = x != x ? 0x100000000ull : (u64)sample_key(x);
        const u64 word = (key << 20) | (LOW - (u64)i);
        best = word > best ? word : best;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)best, o, 64), hi = __shfl_xor((unsigned)(best >> 32), o, 64);
        const u64 t = ((u64)hi << 32) | lo;
        best = t > best ? t : best;
    }
    if (lane == 0) sh.wtot[wave] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) best = sh.wtot[w] > best ? sh.wtot[w] : best;
    const int at = (int)(LOW - (best & LOW));
    if (tid == 0) *out_r = at;
    if (probs_r)
        for (int i = tid; i < V; i += SAMPLE_THREADS) probs_r[i] = i == at ? 1.f : 0.f;
}

template <typename T, bool IN_LDS, class Params>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const T* __restrict__ logits, int64_t ld, int V, const float* __restrict__ u,
                                                                       Params params, int64_t* __restrict__ out, float* __restrict__ probs,
                                                                       int64_t ld_probs) {
    extern __shared__ __attribute__((aligned(16))) float srow[];
    __shared__ SampleShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const T* g = logits + (int64_t)r * ld;
    const float temperature = params.t(r), top_p = params.p(r);
    const int top_k = params.k(r);
    if constexpr (Params::PER_ROW) {                                   // workgroup-uniform: every thread read the same three words
        if (temperature == 0.0f) {
            sample_greedy_row(g, V, sh, out + r, probs ? probs + (int64_t)r * ld_probs : nullptr);
            return;
        }
        // the host checks of setok_sample_rows, per row: nothing below sees a value outside them (the comparisons are false for a NaN)
        if (!(temperature > 0.0f && temperature < INFINITY && top_k >= 0 && top_p > 0.0f && top_p <= 1.0f)) {
            if (tid == 0) out[r] = -1;
            if (probs)
                for (int i = tid; i < V; i += SAMPLE_THREADS) probs[(int64_t)r * ld_probs + i] = 0.f;
            return;
        }
    }

    // ---- pass 1: the only read of the row from memory; maximum and the bad-row flags --------------------------------------------------------
    float mx = -INFINITY;
    int flag = 0;                                                      // 1: NaN, 2: +inf
    auto see = [&](int i, float x) {
        const float s = x / temperature;
        if (s != s) flag |= 1;
        else { if (s == INFINITY) flag |= 2; mx = fmaxf(mx, s); }
        if constexpr (IN_LDS) srow[i] = s;
    };
    sample_read_row(g, V, see);
    mx = wave_max(mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) flag |= __shfl_xor(flag, o, 64);
    if (lane == 0) { sh.wmax[wave] = mx; sh.wflag[wave] = flag; }
    __syncthreads();
    float m = -INFINITY;
    flag = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) { m = fmaxf(m, sh.wmax[w]); flag |= sh.wflag[w]; }
    if (flag != 0 || m == -INFINITY) {                                 // workgroup-uniform: NaN, +inf or no finite entry
        if (tid == 0) out[r] = -1;
        if (probs)
            for (int i = tid; i < V; i += SAMPLE_THREADS) probs[(int64_t)r * ld_probs + i] = 0.f;
        return;
    }
    const SampleRow<T, IN_LDS> row{g, srow, temperature};

    // ---- the filters: thr = the smallest kept key ----------------------------------------------------------------------------------------------
    unsigned thr = 0;
    u64 w_set = 0;
    const bool by_k = top_k > 0 && top_k < V, by_p = top_p < 1.0f;
    if (by_k) thr = sample_select<false>(row, V, m, 0u, (unsigned)top_k, 0.0, sh, &w_set);
    if (by_p) {
        if (!by_k) {                                                   // the normaliser of top-p: the mass of the whole row
            u64 part = 0;
            for (int i = tid; i < V; i += SAMPLE_THREADS) part += sample_weight(row.s(i), m);
            part = wave_sum_u64(part);
            if (lane == 0) sh.wtot[wave] = part;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < SAMPLE_WAVES; ++w) w_set += sh.wtot[w];
            __syncthreads();
        }
        u64 unused;
        thr = sample_select<true>(row, V, m, thr, 0u, (double)top_p * (double)w_set, sh, &unused);
    }

    // ---- inverse CDF in index order: wave w owns indices [w * per, (w + 1) * per) ----------------------------------------------------------------
    const int per = ((V + SAMPLE_WAVES - 1) / SAMPLE_WAVES + 63) & ~63;
    const int lo = min(V, wave * per), hi = min(V, lo + per);
    {
        u64 part = 0;
        for (int i = lo + lane; i < hi; i += 64) {
            const float s = row.s(i);
            if (sample_key(s) >= thr) part += sample_weight(s, m);
        }
        part = wave_sum_u64(part);
        if (lane == 0) sh.wtot[wave] = part;
    }
    __syncthreads();
    u64 W = 0, before = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) { if (w < wave) before += sh.wtot[w]; W += sh.wtot[w]; }
    const u64 mine = sh.wtot[wave];
    const float uc = fminf(fmaxf(u[r], 0.0f), 1.0f - 5.9604644775390625e-8f);
    const u64 u24 = (u64)(unsigned)(uc * 16777216.0f);
    const u64 target = (__umul64hi(W, u24) << 40) | ((W * u24) >> 24);           // floor(W * u24 / 2^24) < W through the 128-bit product
    if (before <= target && target < before + mine) {                  // exactly one wave (wave-uniform)
        u64 run = before;
        for (int base = lo; base < hi; base += 64) {
            const int i = base + lane;
            u64 w = 0;
            if (i < hi) {
                const float s = row.s(i);
                if (sample_key(s) >= thr) w = sample_weight(s, m);
            }
            u64 inc = w;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 t = shfl_up_u64(inc, o);
                if (lane >= o) inc += t;
            }
            const bool hit = run + inc - w <= target && target < run + inc;      // w = 0 can never hit
            if (hit) out[r] = i;
            if (__ballot(hit) != 0) break;
            run += shfl_u64(inc, 63);
        }
    }
    if (probs) {
        const double inv = 1.0 / (double)W;
        for (int i = tid; i < V; i += SAMPLE_THREADS) {
            const float s = row.s(i);
            const u64 w = sample_key(s) >= thr ? sample_weight(s, m) : 0;
            probs[(int64_t)r * ld_probs + i] = (float)((double)w * inv);
        }
    }
}

template <typename T, class Params>
static int sample_launch(const char* who, hipStream_t s, const T* logits, int64_t ld, int rows, int V, const float* u, Params params, int64_t* out,
                         float* probs, int64_t ld_probs) {
    if (V <= SAMPLE_LDS_MAX_V) {
        static SetokDeviceOnce once;
        if (!once.run([] { return hipFuncSetAttribute((const void*)sample_rows_kernel<T, true, Params>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      SAMPLE_LDS_MAX_V * (int)sizeof(float)) == hipSuccess; }))
            return setok_fail(SETOK_ELAUNCH, "%s: cannot raise the dynamic LDS limit", who);
        const size_t lds = ((size_t)V * sizeof(float) + 15) & ~(size_t)15;
        sample_rows_kernel<T, true, Params><<<rows, SAMPLE_THREADS, lds, s>>>(logits, ld, V, u, params, out, probs, ld_probs);
    } else {
        sample_rows_kernel<T, false, Params><<<rows, SAMPLE_THREADS, 0, s>>>(logits, ld, V, u, params, out, probs, ld_probs);
    }
    return SETOK_OK;
}

template <class Params>
static int sample_dispatch(const char* who, void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, const float* u, Params params,
                           int64_t* out, float* probs, int64_t ld_probs) {
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SETOK_BF16) return sample_launch<bf16>(who, s, (const bf16*)logits, ld, rows, V, u, params, out, probs, ld_probs);
    return sample_launch<float>(who, s, (const float*)logits, ld, rows, V, u, params, out, probs, ld_probs);
}

extern "C" int setok_sample_rows(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, const float* u, float temperature,
                                 int top_k, float top_p, int64_t* out, float* probs, int64_t ld_probs) {
    SETOK_CHECK_ARG(logits && u && out, "setok_sample_rows: null operand");
    SETOK_CHECK_ARG(rows >= 0 && V >= 1 && V <= SAMPLE_MAX_V && ld >= V && (!probs || ld_probs >= V),
                    "setok_sample_rows: bad shape rows=%d V=%d (1 .. 2^20) ld=%lld ld_probs=%lld", rows, V, (long long)ld, (long long)ld_probs);
    SETOK_CHECK_ARG(isfinite(temperature) && temperature > 0.0f, "setok_sample_rows: bad temperature %g (finite and > 0)", (double)temperature);
    SETOK_CHECK_ARG(top_k >= 0, "setok_sample_rows: bad top_k %d (>= 0; 0 = no filter)", top_k);
    SETOK_CHECK_ARG(top_p > 0.0f && top_p <= 1.0f, "setok_sample_rows: bad top_p %g (a probability in (0, 1]; 1 = no filter)", (double)top_p);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_sample_rows: bad dtype %d", dtype);
    if (rows == 0) return SETOK_OK;
    const int rc = sample_dispatch("setok_sample_rows", stream, dtype, logits, ld, rows, V, u, SampleScalars{temperature, top_k, top_p}, out, probs,
                                   ld_probs);
    if (rc != SETOK_OK) return rc;
    SETOK_CHECK_LAUNCH("setok_sample_rows");
    return SETOK_OK;
}

extern "C" int setok_sample_rows_each(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, const float* u,
                                      const float* temperature, const int* top_k, const float* top_p, int64_t* out, float* probs,
                                      int64_t ld_probs) {
    SETOK_CHECK_ARG(logits && u && out && temperature && top_k && top_p, "setok_sample_rows_each: null operand");
    SETOK_CHECK_ARG(rows >= 0 && V >= 1 && V <= SAMPLE_MAX_V && ld >= V && (!probs || ld_probs >= V),
                    "setok_sample_rows_each: bad shape rows=%d V=%d (1 .. 2^20) ld=%lld ld_probs=%lld", rows, V, (long long)ld, (long long)ld_probs);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_sample_rows_each: bad dtype %d", dtype);
    if (rows == 0) return SETOK_OK;
    const int rc = sample_dispatch("setok_sample_rows_each", stream, dtype, logits, ld, rows, V, u, SampleArrays{temperature, top_k, top_p}, out,
                                   probs, ld_probs);
    if (rc != SETOK_OK) return rc;
    SETOK_CHECK_LAUNCH("setok_sample_rows_each");
    return SETOK_OK;
}
