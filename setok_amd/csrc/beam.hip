// beam.hip — the three device-side pieces of beam search in the decode loop (include/setok_hip.h, "Beam search").
//   setok_beam_topk      per sequence, the C best of its n_in * V accumulated log-probabilities running[j] + log_softmax(row j)[v]: one workgroup per
//                        logits row keeps that row's best 64, a second launch merges a sequence's n_in lists.
//   setok_beam_advance   HuggingFace's bookkeeping of running and finished hypotheses on the C candidates, one wave per sequence in ONE workgroup
//                        (the termination test is an any / all over the whole batch), hypotheses kept as back-pointers.
//   setok_kv_reorder     row r's generated slots of every cache tensor of every layer become what row src_row[r] held: gather into a scratch
//                        region, then copy back (two launches for the whole cache; the tensors come from a device pointer table).
// No atomics anywhere: every selection is a rank in a total order (value descending, then index ascending), so every result is a pure function of
// the inputs and a sequence's bits do not depend on its neighbours in the batch.
#include "common.h"
#include <math.h>

constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_WAVES = BEAM_THREADS / WAVE;
constexpr int BEAM_MAX_C = 64;                           // candidates per sequence: one wave holds them, one per lane
constexpr int BEAM_MAX_N = 16;                           // beams per sequence: n_in * 64 partial candidates fill one workgroup
constexpr int BEAM_MAX_V = 1 << 20;
constexpr int BEAM_EMPTY = 0x7fffffff;                   // the index of a list slot that holds no candidate (value -inf): it loses against every real one

// the total order of candidates: a beats b
__device__ inline bool beam_beats(float av, int64_t ai, float bv, int64_t bi) { return av > bv || (av == bv && ai < bi); }

// The two lane moves of a list insert, without a trip through the LDS crossbar: the value of a wave-uniform lane (v_readlane) and the value of the
// lane below (DPP wave_shr:1; lane 0 keeps its own, which no caller uses).
__device__ inline int beam_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ inline float beam_lane(float v, int src) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src)); }
__device__ inline int beam_lane_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ inline float beam_lane_below(float v) { return __builtin_bit_cast(float, beam_lane_below(__builtin_bit_cast(int, v))); }

// ---- setok_beam_topk, launch 1: one workgroup per logits row -----------------------------------------------------------------------------------
// Thread t owns the elements [(k * 1024 + t) * VEC, + VEC) for k = 0, 1, ..: read as one 16-byte piece when the row allows it, else one by one — the
// same elements in the same order either way, so the sums below do not depend on the row's alignment or stride, only on V.
template <typename T>
struct BeamRow {
    const T* g;
    int V;
    bool vec;
    static constexpr int VEC = Elem<T>::VEC;
    __device__ inline void load(int i0, float* x) const {                 // elements i0 .. i0 + VEC - 1; those at or behind V are not read (x = -inf)
        if (vec && i0 + VEC <= V) { ld_vec<T>(g + i0, x); return; }
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = i0 + e < V ? (float)g[i0 + e] : -INFINITY;
    }
};

template <typename T>
__global__ __launch_bounds__(BEAM_THREADS) void beam_row_topk_kernel(const T* __restrict__ logits, int64_t ld, int V, const float* __restrict__ running,
                                                                       float* __restrict__ part_val, int32_t* __restrict__ part_idx,
                                                                       int32_t* __restrict__ row_flag) {
    __shared__ float s_f[BEAM_WAVES];
    __shared__ int s_flag[BEAM_WAVES];
    __shared__ float s_val[BEAM_THREADS];
    __shared__ int s_idx[BEAM_THREADS];
    constexpr int VEC = Elem<T>::VEC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    const T* g = logits + (int64_t)r * ld;
    const BeamRow<T> row{g, V, ((uintptr_t)g & 15u) == 0};
    const int trips = (V + BEAM_THREADS * VEC - 1) / (BEAM_THREADS * VEC);        // workgroup-uniform

    // pass 1: the row maximum and the bad-row flag (NaN or +inf)
    float mx = -INFINITY;
    int flag = 0;
    for (int k = 0; k < trips; ++k) {
        float x[VEC];
        row.load((k * BEAM_THREADS + tid) * VEC, x);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (x[e] != x[e] || x[e] == INFINITY) flag = 1;
            else mx = fmaxf(mx, x[e]);
        }
    }
    mx = wave_max(mx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) flag |= __shfl_xor(flag, o, 64);
    if (lane == 0) { s_f[wave] = mx; s_flag[wave] = flag; }
    __syncthreads();
    float m = -INFINITY;
    flag = 0;
#pragma unroll
    for (int w = 0; w < BEAM_WAVES; ++w) { m = fmaxf(m, s_f[w]); flag |= s_flag[w]; }
    __syncthreads();                                                     // s_f is written again below
    const bool bad = flag != 0 || m == -INFINITY;                        // workgroup-uniform: NaN, +inf or no finite entry
    if (tid == 0) row_flag[r] = bad ? 1 : 0;

    // pass 2: sum exp(x - m): every thread in its own element order, then the wave butterfly, then the waves in order
    float lse = 0.f;
    if (!bad) {
        float part = 0.f;
        for (int k = 0; k < trips; ++k) {
            float x[VEC];
            row.load((k * BEAM_THREADS + tid) * VEC, x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) part += expf(x[e] - m);          // (-inf - m = -inf: exactly 0)
        }
        part = wave_sum(part);
        if (lane == 0) s_f[wave] = part;
        __syncthreads();
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < BEAM_WAVES; ++w) tot += s_f[w];
        lse = logf(tot);
    }
    const float run = running[r];

    // pass 3: every wave keeps the best 64 of its elements, sorted, one per lane; a new element enters by one ballot and one shift
    float lv = -INFINITY;
    int li = BEAM_EMPTY;
    if (!bad) {
        float thr_v = -INFINITY;
        int thr_i = BEAM_EMPTY;
        for (int k = 0; k < trips; ++k) {
            float x[VEC];
            const int i0 = (k * BEAM_THREADS + tid) * VEC;
            row.load(i0, x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int i = i0 + e;
                const float val = run + ((x[e] - m) - lse);                // torch's log_softmax, then HF's `+ running_beam_scores`
                unsigned long long todo = __ballot(i < V && beam_beats(val, i, thr_v, thr_i));
                if (todo == 0) continue;                                   // wave-uniform; the usual case once the list has filled
                while (todo != 0) {
                    const int src = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const float cv = beam_lane(val, src);
                    const int ci = beam_lane(i, src);
                    const int p = __popcll(__ballot(beam_beats(lv, li, cv, ci)));   // the list is sorted: lanes 0 .. p - 1 keep their entries
                    const float uv = beam_lane_below(lv);
                    const int ui = beam_lane_below(li);
                    if (lane > p) { lv = uv; li = ui; }
                    else if (lane == p) { lv = cv; li = ci; }
                }
                thr_v = beam_lane(lv, 63);
                thr_i = beam_lane(li, 63);
            }
        }
    }
    // the row's best 64 of the 16 lists: an entry's rank is its place in its own list plus, for every other list, the number of entries that beat it -
    // a binary search, the lists being sorted by the same order.  (Empty slots tie; those of equal rank write the same bytes.)
    s_val[tid] = lv;
    s_idx[tid] = li;
    __syncthreads();
    int rank = lane;
    for (int w = 0; w < BEAM_WAVES; ++w) {
        if (w == wave) continue;                                         // wave-uniform
        int lo = 0, hi = WAVE;
#pragma unroll
        for (int it = 0; it < 7; ++it) {                                 // 64 -> 0 in at most 7 halvings
            const int mid = min((lo + hi) >> 1, WAVE - 1);
            const bool ahead = lo < hi && beam_beats(s_val[w * WAVE + mid], s_idx[w * WAVE + mid], lv, li);
            if (lo < hi) { if (ahead) lo = mid + 1; else hi = mid; }
        }
        rank += lo;
    }
    if (rank < BEAM_MAX_C) {
        part_val[(int64_t)r * BEAM_MAX_C + rank] = lv;
        part_idx[(int64_t)r * BEAM_MAX_C + rank] = li;
    }
}

// ---- setok_beam_topk, launch 2: one workgroup per sequence merges its n_in lists (n_in * 64 <= 1024 entries) by the flat index j * V + v ------
__global__ __launch_bounds__(BEAM_THREADS) void beam_merge_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                                    const int32_t* __restrict__ row_flag, int n_in, int V, int C,
                                                                    float* __restrict__ cand_score, int64_t* __restrict__ cand_token,
                                                                    int32_t* __restrict__ cand_beam, int32_t* __restrict__ status) {
    __shared__ float s_val[BEAM_THREADS];
    __shared__ int64_t s_flat[BEAM_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int total = n_in * BEAM_MAX_C;
    float v = -INFINITY;
    int64_t flat = INT64_MAX;
    int tok = 0, beam = 0;
    bool real = false;
    if (tid < total) {
        const int j = tid / BEAM_MAX_C;
        const int64_t at = ((int64_t)b * n_in + j) * BEAM_MAX_C + (tid % BEAM_MAX_C);
        const int idx = part_idx[at];
        if (idx != BEAM_EMPTY) { v = part_val[at]; flat = (int64_t)j * V + idx; tok = idx; beam = j; real = true; }
    }
    s_val[tid] = v;
    s_flat[tid] = flat;
    __syncthreads();
    int rank = tid % BEAM_MAX_C;                                         // as above: every row's list is sorted, by the flat index as well
    for (int j = 0; j < n_in; ++j) {
        if (j == tid / BEAM_MAX_C) continue;
        int lo = 0, hi = BEAM_MAX_C;
#pragma unroll
        for (int it = 0; it < 7; ++it) {
            const int mid = min((lo + hi) >> 1, BEAM_MAX_C - 1);
            const bool ahead = lo < hi && beam_beats(s_val[j * BEAM_MAX_C + mid], s_flat[j * BEAM_MAX_C + mid], v, flat);
            if (lo < hi) { if (ahead) lo = mid + 1; else hi = mid; }
        }
        rank += lo;
    }
    if (tid < total && rank < C) {                                       // (an empty entry gets here only when a row of the sequence is bad)
        cand_score[(int64_t)b * C + rank] = v;
        cand_token[(int64_t)b * C + rank] = real ? tok : 0;
        cand_beam[(int64_t)b * C + rank] = real ? beam : 0;
    }
    if (tid == 0) {
        int bad = 0;
        for (int j = 0; j < n_in; ++j) bad |= row_flag[b * n_in + j];
        status[b] = bad;
    }
}

extern "C" int setok_beam_topk(void* stream, int dtype, const void* logits, int64_t ld, int B, int n_in, int V, const float* running, int C,
                               float* cand_score, int64_t* cand_token, int32_t* cand_beam, int32_t* status, void* ws, int64_t ws_bytes) {
    SETOK_CHECK_ARG(logits && running && cand_score && cand_token && cand_beam && status && ws, "setok_beam_topk: null operand");
    SETOK_CHECK_ARG(B >= 0 && n_in >= 1 && n_in <= BEAM_MAX_N && V >= 1 && V <= BEAM_MAX_V && ld >= V,
                    "setok_beam_topk: bad shape B=%d n_in=%d (1 .. 16) V=%d (1 .. 2^20) ld=%lld", B, n_in, V, (long long)ld);
    SETOK_CHECK_ARG(C >= 1 && C <= BEAM_MAX_C && (int64_t)C <= (int64_t)n_in * V, "setok_beam_topk: bad C %d (1 .. 64 and <= n_in * V)", C);
    SETOK_CHECK_ARG(dtype == SETOK_BF16 || dtype == SETOK_F32, "setok_beam_topk: bad dtype %d", dtype);
    const int64_t rows = (int64_t)B * n_in;
    SETOK_CHECK_ARG(ws_bytes >= rows * (BEAM_MAX_C * 8 + 4), "setok_beam_topk: workspace of %lld bytes, %lld needed (B * n_in * 516)",
                    (long long)ws_bytes, (long long)(rows * (BEAM_MAX_C * 8 + 4)));
    SETOK_CHECK_ARG(((uintptr_t)ws & 3u) == 0, "setok_beam_topk: the workspace must be 4-byte aligned");
    if (B == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    float* part_val = (float*)ws;
    int32_t* part_idx = (int32_t*)ws + rows * BEAM_MAX_C;
    int32_t* row_flag = (int32_t*)ws + 2 * rows * BEAM_MAX_C;
    if (dtype == SETOK_BF16)
        beam_row_topk_kernel<bf16><<<(int)rows, BEAM_THREADS, 0, s>>>((const bf16*)logits, ld, V, running, part_val, part_idx, row_flag);
    else
        beam_row_topk_kernel<float><<<(int)rows, BEAM_THREADS, 0, s>>>((const float*)logits, ld, V, running, part_val, part_idx, row_flag);
    SETOK_CHECK_LAUNCH("setok_beam_topk");
    beam_merge_kernel<<<B, BEAM_THREADS, 0, s>>>(part_val, part_idx, row_flag, n_in, V, C, cand_score, cand_token, cand_beam, status);
    SETOK_CHECK_LAUNCH("setok_beam_topk (merge)");
    return SETOK_OK;
}

// ---- setok_beam_advance ---------------------------------------------------------------------------------------------------------------------------
// One workgroup; wave w handles sequences w, w + 16, ..; lane c holds candidate c (c < C) and, in the merge with the finished set, lane i < n holds
// finished entry i as well.  Every `x + flag * -1e9` of the rule is the same fp32 addition here.
__global__ __launch_bounds__(BEAM_THREADS) void beam_advance_kernel(const float* __restrict__ cand_score, const int64_t* __restrict__ cand_token,
                                                                      const int32_t* __restrict__ cand_beam, const int32_t* __restrict__ topk_status,
                                                                      int B, int n, int C, const int64_t* __restrict__ eos, int n_eos, int step, int max_new,
                                                                      float fin_div, float heur_div, int early_stopping,
                                                                      float* __restrict__ run_score, float* __restrict__ fin_score,
                                                                      uint8_t* __restrict__ fin_flag, int32_t* __restrict__ fin_len,
                                                                      int32_t* __restrict__ fin_parent, int64_t* __restrict__ fin_token,
                                                                      uint8_t* __restrict__ heur, int64_t* __restrict__ bp_token,
                                                                      int32_t* __restrict__ bp_parent, int64_t* __restrict__ next_token,
                                                                      int32_t* __restrict__ src_row, int32_t* __restrict__ summary) {
    __shared__ int s_heur[BEAM_WAVES], s_allfin[BEAM_WAVES], s_allhit[BEAM_WAVES], s_bad[BEAM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float NEG = -1.0e9f;
    int any_heur = 0, all_fin = 1, all_hit = 1, any_bad = 0;             // wave-uniform
    for (int b = wave; b < B; b += BEAM_WAVES) {
        const bool have = lane < C;
        float sc = -INFINITY;
        int64_t tok = 0;
        int par = 0;
        if (have) {
            sc = cand_score[(int64_t)b * C + lane];
            tok = cand_token[(int64_t)b * C + lane];
            par = cand_beam[(int64_t)b * C + lane];
            if (par < 0 || par >= n) par = 0;                             // (never from setok_beam_topk; keeps src_row inside the group)
        }
        any_bad |= topk_status[b] != 0;
        bool hit = step + 1 >= max_new;
        for (int j = 0; j < n_eos; ++j) hit = hit || tok == eos[j];
        const unsigned long long hit_mask = __ballot(have && hit), have_mask = __ballot(have);
        all_hit &= hit_mask == have_mask;

        // the next running beams: the best n of score + hit * -1e9
        const float rsc = have ? sc + (hit ? NEG : 0.0f) : -INFINITY;
        int rank = 0;
        for (int j = 0; j < C; ++j) {
            const float ov = __shfl(rsc, j, 64);
            rank += beam_beats(ov, j, rsc, lane) ? 1 : 0;
        }
        if (have && rank < n) {
            const int at = b * n + rank;
            run_score[at] = rsc;
            next_token[at] = tok;
            src_row[at] = b * n + par;
            bp_token[(int64_t)step * B * n + at] = tok;
            bp_parent[(int64_t)step * B * n + at] = par;
        }
        const float best_running = __shfl(rsc, __ffsll((long long)__ballot(have && rank == 0)) - 1, 64);

        // the finished set: its n entries (lanes < n) merged with the C candidates, the best n stay
        float fs = -INFINITY;
        int ff = 0, fl = 0, fp = 0;
        int64_t ft = 0;
        if (lane < n) {
            fs = fin_score[b * n + lane]; ff = fin_flag[b * n + lane]; fl = fin_len[b * n + lane];
            fp = fin_parent[b * n + lane]; ft = fin_token[b * n + lane];
        }
        const bool full = __popcll(__ballot(lane < n && ff != 0)) == n;
        const bool open = heur[b] != 0;
        const bool did = have && hit && lane < n;
        float ns = sc / fin_div;
        ns = ns + ((full && early_stopping == 1) ? NEG : 0.0f);
        ns = ns + (!open ? NEG : 0.0f);
        ns = ns + (!did ? NEG : 0.0f);
        if (!have) ns = -INFINITY;
        // merged index: finished entry i -> i, candidate c -> n + c
        int rank_f = 0, rank_c = 0;
        for (int j = 0; j < n; ++j) {
            const float ov = __shfl(fs, j, 64);
            rank_f += beam_beats(ov, j, fs, lane) ? 1 : 0;
            rank_c += beam_beats(ov, j, ns, n + lane) ? 1 : 0;
        }
        for (int j = 0; j < C; ++j) {
            const float ov = __shfl(ns, j, 64);
            rank_f += beam_beats(ov, n + j, fs, lane) ? 1 : 0;
            rank_c += beam_beats(ov, n + j, ns, n + lane) ? 1 : 0;
        }
        // every lane has read the old entries: the survivors go to their new places
        if (lane < n && rank_f < n) {
            const int at = b * n + rank_f;
            fin_score[at] = fs; fin_flag[at] = (uint8_t)ff; fin_len[at] = fl; fin_parent[at] = fp; fin_token[at] = ft;
        }
        if (have && rank_c < n) {
            const int at = b * n + rank_c;
            fin_score[at] = ns; fin_flag[at] = did ? 1 : 0; fin_len[at] = step + 1; fin_parent[at] = par; fin_token[at] = tok;
        }
        // the new set's flags and worst score, from the registers (the stores above need not be visible)
        const bool f_keep = lane < n && rank_f < n, c_keep = have && rank_c < n;
        const int n_fin = __popcll(__ballot(f_keep && ff != 0)) + __popcll(__ballot(c_keep && did));
        float worst = INFINITY;
        if (f_keep) worst = fs;
        if (c_keep) worst = fminf(worst, ns);
        worst = wave_min(worst);
        // the early-stop heuristic: an unfinished entry compares against -1e9, a finished one against the set's minimum
        const float best_possible = best_running / heur_div;
        const bool improve = (n_fin < n && best_possible > NEG) || (n_fin > 0 && best_possible > worst);
        const bool still = open && improve;
        if (lane == 0) heur[b] = still ? 1 : 0;
        any_heur |= still ? 1 : 0;
        all_fin &= n_fin == n;
    }
    if (lane == 0) { s_heur[wave] = any_heur; s_allfin[wave] = all_fin; s_allhit[wave] = all_hit; s_bad[wave] = any_bad; }
    __syncthreads();
    if (tid == 0) {
        int h = 0, f = 1, a = 1, bad = 0;
#pragma unroll
        for (int w = 0; w < BEAM_WAVES; ++w) { h |= s_heur[w]; f &= s_allfin[w]; a &= s_allhit[w]; bad |= s_bad[w]; }
        summary[0] = (h && !(f && early_stopping == 1) && !a) ? 1 : 0;
        summary[1] = bad;
    }
}

extern "C" int setok_beam_advance(void* stream, const float* cand_score, const int64_t* cand_token, const int32_t* cand_beam,
                                  const int32_t* topk_status, int B, int n, int C, const int64_t* eos, int n_eos, int step, int max_new,
                                  double length_penalty, int early_stopping, float* run_score, float* fin_score, uint8_t* fin_flag, int32_t* fin_len,
                                  int32_t* fin_parent, int64_t* fin_token, uint8_t* heur, int64_t* bp_token, int32_t* bp_parent, int64_t* next_token,
                                  int32_t* src_row, int32_t* summary) {
    SETOK_CHECK_ARG(cand_score && cand_token && cand_beam && topk_status && run_score && fin_score && fin_flag && fin_len && fin_parent && fin_token &&
                    heur && bp_token && bp_parent && next_token && src_row && summary && (eos || n_eos <= 0), "setok_beam_advance: null operand");
    SETOK_CHECK_ARG(B >= 0 && n >= 1 && n <= BEAM_MAX_N, "setok_beam_advance: bad shape B=%d n=%d (1 .. 16)", B, n);
    SETOK_CHECK_ARG(C >= n && C <= BEAM_MAX_C, "setok_beam_advance: bad C %d (n .. 64)", C);
    SETOK_CHECK_ARG(n_eos >= 0, "setok_beam_advance: bad n_eos %d (>= 0)", n_eos);
    SETOK_CHECK_ARG(max_new >= 1 && step >= 0 && step < max_new, "setok_beam_advance: bad step %d of max_new %d", step, max_new);
    SETOK_CHECK_ARG(isfinite(length_penalty), "setok_beam_advance: bad length_penalty %g (finite)", length_penalty);
    SETOK_CHECK_ARG(early_stopping >= 0 && early_stopping <= 2, "setok_beam_advance: bad early_stopping %d (0 False, 1 True, 2 \"never\")", early_stopping);
    if (B == 0) return SETOK_OK;
    // Python's `int ** float` of the rule: a double power, rounded once to fp32 where torch divides an fp32 tensor by it
    const float fin_div = (float)pow((double)(step + 1), length_penalty);
    const int hyp = (early_stopping == 2 && length_penalty > 0.0) ? max_new : step + 1;
    const float heur_div = (float)pow((double)hyp, length_penalty);
    beam_advance_kernel<<<1, BEAM_THREADS, 0, (hipStream_t)stream>>>(cand_score, cand_token, cand_beam, topk_status, B, n, C, eos, n_eos, step, max_new,
                                                                      fin_div, heur_div, early_stopping, run_score, fin_score, fin_flag, fin_len,
                                                                      fin_parent, fin_token, heur, bp_token, bp_parent, next_token, src_row, summary);
    SETOK_CHECK_LAUNCH("setok_beam_advance");
    return SETOK_OK;
}

// ---- setok_kv_reorder -------------------------------------------------------------------------------------------------------------------------------
// Block (x = row * Hkv + head, y = tensor) moves the ns * row_bytes contiguous bytes of slots [slot0, slot1) of one (row, head) of one tensor:
// GATHER = true from row src_row[r] into the scratch, GATHER = false from the scratch back to row r.  Rows that keep their own data do nothing.
constexpr int REORDER_THREADS = 256;

__device__ inline int reorder_source(const int32_t* __restrict__ src_row, int r, int n, bool* bad) {
    const int s = src_row[r], g0 = r / n * n;
    *bad = s < g0 || s >= g0 + n;
    return *bad ? r : s;
}

template <bool GATHER>
__global__ __launch_bounds__(REORDER_THREADS) void kv_reorder_kernel(uint8_t* const* __restrict__ ptrs, const int32_t* __restrict__ row_bytes,
                                                                       const int64_t* __restrict__ scratch_unit, int n, int Hkv, int cap, int slot0,
                                                                       int ns, const int32_t* __restrict__ src_row, uint8_t* __restrict__ scratch,
                                                                       int32_t* __restrict__ status) {
    const int tid = threadIdx.x, t = blockIdx.y;
    const int r = blockIdx.x / Hkv, h = blockIdx.x % Hkv;
    bool bad;
    const int s = reorder_source(src_row, r, n, &bad);
    if (GATHER && t == 0 && h == 0 && tid == 0 && bad) status[r] = 1;   // the one writer of status[r]
    if (s == r || ns == 0) return;                                       // block-uniform
    const int64_t rb = row_bytes[t];
    const int64_t bytes = rb * ns;
    uint8_t* base = ptrs[t];
    const int64_t rows_heads = (int64_t)gridDim.x;
    uint8_t* sc = scratch + scratch_unit[t] * rows_heads * ns + (int64_t)blockIdx.x * (((rb + 15) & ~(int64_t)15) * ns);
    uint8_t* mine = base + (((int64_t)r * Hkv + h) * cap + slot0) * rb;
    const uint8_t* theirs = base + (((int64_t)s * Hkv + h) * cap + slot0) * rb;
    const uint8_t* from = GATHER ? theirs : sc;
    uint8_t* to = GATHER ? sc : mine;
    if ((((uintptr_t)from | (uintptr_t)to | (uintptr_t)bytes) & 15u) == 0) {
        const uint4* f4 = reinterpret_cast<const uint4*>(from);
        uint4* t4 = reinterpret_cast<uint4*>(to);
        for (int64_t i = tid; i < bytes / 16; i += REORDER_THREADS) t4[i] = f4[i];
    } else {
        for (int64_t i = tid; i < bytes; i += REORDER_THREADS) to[i] = from[i];
    }
}

extern "C" int setok_kv_reorder(void* stream, const void* const* ptrs, const int32_t* row_bytes, const int64_t* scratch_unit, int n_tensors,
                                int64_t unit_total, int rows, int n, int Hkv, int cap, int slot0, int slot1, const int32_t* src_row, void* scratch,
                                int64_t scratch_bytes, int32_t* status) {
    SETOK_CHECK_ARG(ptrs && row_bytes && scratch_unit && src_row && status, "setok_kv_reorder: null operand");
    SETOK_CHECK_ARG(n_tensors >= 1 && n_tensors <= 65535 && rows >= 0 && n >= 1 && rows % n == 0 && Hkv >= 1 && cap >= 1 && unit_total >= 16,
                    "setok_kv_reorder: bad shape n_tensors=%d rows=%d n=%d Hkv=%d cap=%d", n_tensors, rows, n, Hkv, cap);
    SETOK_CHECK_ARG(slot0 >= 0 && slot0 <= slot1 && slot1 <= cap, "setok_kv_reorder: slots [%d, %d) are not inside the cache (cap = %d)", slot0, slot1, cap);
    const int ns = slot1 - slot0;
    const int64_t need = unit_total * rows * Hkv * ns;
    SETOK_CHECK_ARG(ns == 0 || (scratch && scratch_bytes >= need && ((uintptr_t)scratch & 15u) == 0),
                    "setok_kv_reorder: scratch of %lld bytes (16-byte aligned), %lld needed", (long long)scratch_bytes, (long long)need);
    SETOK_CHECK_ARG((int64_t)rows * Hkv <= 0x7fffffff, "setok_kv_reorder: rows * Hkv = %lld exceeds the grid", (long long)rows * Hkv);
    if (rows == 0) return SETOK_OK;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* const* p = (uint8_t* const*)ptrs;
    const dim3 grid(rows * Hkv, ns == 0 ? 1 : n_tensors);
    kv_reorder_kernel<true><<<grid, REORDER_THREADS, 0, s>>>(p, row_bytes, scratch_unit, n, Hkv, cap, slot0, ns, src_row, (uint8_t*)scratch, status);
    SETOK_CHECK_LAUNCH("setok_kv_reorder (gather)");
    if (ns == 0) return SETOK_OK;
    kv_reorder_kernel<false><<<grid, REORDER_THREADS, 0, s>>>(p, row_bytes, scratch_unit, n, Hkv, cap, slot0, ns, src_row, (uint8_t*)scratch, status);
    SETOK_CHECK_LAUNCH("setok_kv_reorder (copy back)");
    return SETOK_OK;
}
