/*
 * setok_hip.h — C ABI of libsetok_hip.so, the MI355X (gfx950) implementation of the SeTok
 * `encode_images` hot path.
 *
 * The reference (ChocoWu/SeTok) has NO native / FFI interface for this path: it is 100 % Python
 * over stock torch ops.  The boundary a maintainer binds is therefore the
 * set of torch-op groups of the reference's hot path; each entry point below cites the reference
 * lines (relative to /root/reference/) whose arithmetic it replaces.  The Python host that mirrors
 * the reference's `SetokTokenizer` / `build_vision_tower` / `encode_images` surface
 * (setok_amd/) calls these through ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it, allocates
 *     nothing, and synchronises nothing — outputs and workspaces are caller-allocated (the context
 *     entry points are the documented exception: they own the weights; setok_encode synchronises only on request);
 *   - `dtype` selects the activation/weight element type: SETOK_F32 (parity mode; fp32 MFMA,
 *     exact fma chains), SETOK_BF16 (throughput mode; bf16 MFMA, fp32 accumulation) or — since ABI 9 —
 *     SETOK_F16 (IEEE half, fp16 MFMA at the bf16 rate, fp32 accumulation: what the reference's inference
 *     loader and its non-`--bf16` training launches cast the tower to, src/model/builder.py:43,135-136,
 *     src/train/train_setokim.py:326,348,374).  The 16-bit kernels are written ONCE against "a 16-bit float
 *     element with fp32 accumulation" and compiled twice: libsetok_hip.so serves SETOK_F32 + SETOK_BF16,
 *     libsetok_hip_f16.so (the same sources under -DSETOK_HALF, the same exported names) serves SETOK_F32 +
 *     SETOK_F16; each refuses the other's 16-bit code, a host binds the one(s) it needs (dlopen with
 *     RTLD_LOCAL: both export this header's names; the Python host routes by tensor dtype, setok_amd/_lib.py);
 *     biases, LayerNorm affine parameters, scores and distances are always fp32;
 *   - matrices are row-major and dense unless a leading dimension is given;
 *   - return value: 0 on success, a negative SETOK_E* code otherwise; setok_last_error() returns
 *     a thread-local human-readable message for the last failure.
 */
#ifndef SETOK_HIP_H
#define SETOK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SETOK_ABI_VERSION 9

enum { SETOK_F32 = 0, SETOK_BF16 = 1, SETOK_F16 = 2 };
enum { SETOK_ACT_NONE = 0, SETOK_ACT_QUICK_GELU = 1, SETOK_ACT_GELU_ERF = 2,
       SETOK_ACT_SILU = 3 /* x * sigmoid(x): setok_activation only; setok_linear / setok_linear_ln / setok_activation_dropout refuse it */ };
enum { SETOK_OK = 0, SETOK_EINVAL = -1, SETOK_ELAUNCH = -2, SETOK_EUNSUPPORTED = -3 };

int setok_abi_version(void);
const char* setok_last_error(void);
/* Name of the device the library sees ("" if none), its CU count; both cheap, host-side only. */
int setok_device_info(char* name_host, int name_cap, int* cu_count_host);

/* Launch profiler (measurement aid, off by default; process-wide): between start and stop every setok_linear / setok_linear_ln /
 * setok_cluster_dpc_knn call is timed by a pair of HIP events on its stream — attached to the call's first and last kernel dispatch
 * (hipExtLaunchKernelGGL: the dispatches' own start / end timestamps, no marker packets) where the call launches the LDS-DMA GEMM kernels or
 * the single-launch clustering, recorded as markers around the call otherwise.  stop waits for them and returns the number of records written:
 * kind 0 = bf16 GEMM, 1 = fp32 GEMM (work = FLOPs), 2 = clustering (work = Gram FLOPs); cls = act | residual << 2 | folded LayerNorm << 3;
 * bytes = algorithmic bytes of the call; ms = event duration.  Call start / stop while no other library call is in flight. */
int setok_profile_start(void);
int setok_profile_stop(int* kind, int* cls, double* work, double* bytes, float* ms, int cap);
/* Between start and stop: pause != 0 stops attaching events to launches (the records so far stay), 0 resumes.  An event pair per launch costs ~4 us of device
 * time: a caller timing many steps probes some of them. */
int setok_profile_pause(int pause);

/* ---- the whole path behind one call (host-language-neutral entry) -------------------------------------------------
 * `SetokTokenizer.forward` (src/model/setok/tokenizer.py:157-182): tower (clip_encoder.py:50-62, HF CLIP ViT hidden_states[select_layer],
 * feature_select :40-48) -> + PositionalEncoding2D (:164-168) -> cluster_dpc_knn (:174) -> group_encoding (:177-178) -> inter_encoder
 * (:179) -> out (:180).  A context owns device copies of the weights in compute layout; setok_encode runs the path on the caller's
 * stream into caller-allocated buffers.  These are the only entry points that allocate (create / load / ready); setok_encode itself is
 * asynchronous: the data-dependent shapes of the ragged stages (per-image token counts) are read on the DEVICE, the host reads them after the
 * call when it wants them (see below).
 * Contexts are independent: no global mutable state, one context per (device, stream) in use at a time. */
typedef struct setok_ctx setok_ctx;

typedef struct setok_config {
    /* tower: the HF CLIP vision config behind clip_encoder.py:35 */
    int image_size, patch_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads;
    float layer_norm_eps;
    int select_layer;            /* mm_vision_select_layer (clip_encoder.py:41): index into hidden_states, negative from the end */
    int select_cls_patch;        /* mm_vision_select_feature: 0 = 'patch' (drop the class token, :43), 1 = 'cls_patch' */
    /* head: ctor kwargs of SetokTokenizer (tokenizer.py:14-34); hidden_dim == tower hidden_size */
    int token_feat_dim, nheads, dim_feedforward, inner_cluster_layers, intra_cluster_layers, min_cluster_num;
    float threshold;
    int dtype;                   /* SETOK_BF16 / SETOK_F16 (throughput mode; F16 in libsetok_hip_f16.so) or SETOK_F32 (parity mode) */
    int fold_layernorm;          /* 16-bit modes only: fold layer_norm1 / layer_norm2 of the tower into the q|k|v / fc1 GEMMs */
} setok_config;

int setok_create(const setok_config* cfg, setok_ctx** out);
void setok_destroy(setok_ctx* ctx);
const char* setok_ctx_error(const setok_ctx* ctx);

/* One parameter by its name in the reference's state dict (`image_feature_encoder.vision_tower.` + HF CLIPVisionModel names, with or
 * without HF 4.x's `vision_model.`; `inner_encoder.*`, `inter_encoder.*`, `out.*`), plus `position_embedding.table`: the (N, C)
 * PositionalEncoding2D table of module.py:118-146 in the compute dtype (the reference builds it on the host in fp32 and casts; passing it
 * keeps it bit-identical to the host's).  `ptr` is a DEVICE pointer to a dense tensor of `dtype` and `shape`; the data is copied
 * (matrices to the compute dtype, vectors to fp32) on `stream`. */
int setok_load_weight(setok_ctx* ctx, void* stream, const char* name, const void* ptr, int dtype, const int64_t* shape, int ndim);

/* After the last setok_load_weight: checks that every parameter the configuration needs is there (the error names the first missing
 * one) and builds the fused q|k|v matrices, the padded patch matrix and the folded LayerNorm operands. */
int setok_weights_ready(setok_ctx* ctx, void* stream);

/* Bytes of 256-byte-aligned device workspace setok_encode needs for a batch of B images.
 * STREAM-ORDER CONTRACT of the workspace (and of every output buffer of setok_encode): the call's launches read and write it on `stream`, and
 * since ABI 8 the counts_host form RETURNS WHILE THE LAST OF THEM ARE STILL RUNNING.  The buffers therefore belong to `stream` until work enqueued
 * behind the call on that stream has run: reuse on the same stream needs nothing; reuse, reading (hipMemcpyAsync on another or a non-blocking
 * stream) or freeing from ANY OTHER stream or from the host needs an event recorded on `stream` after the call (or hipStreamSynchronize(stream)).
 * hipFree / hipFreeAsync on another stream without that order is a use-after-free, exactly as for any other asynchronous launch. */
int64_t setok_encode_workspace_bytes(const setok_ctx* ctx, int B);

/* images (B, 3, image_size, image_size) in the compute dtype -> tokens: packed (sum_b L_b, token_feat_dim) rows, image b owning rows
 * [sum_{b' < b} L_b', + L_b) (capacity B * N rows; rows past sum_b L_b are never written), counts (B) int32 on the device, idx_cluster (B, N)
 * int64, score (B, N) fp32, index_down (B, N) int64 (-1 padded).  k / threshold == 0 select the configured defaults (the reference's
 * truthiness rule, tokenizer.py:171-172); noise / token_mask as in setok_cluster_dpc_knn (NULL = none).  The optional stage_* outputs
 * receive pointers INTO the workspace (valid until its next use): x = features + positions (B*N, C), group (sum L, C), inter (sum L, C).
 *
 * ASYNCHRONOUS (since ABI 5): no host synchronisation between the stages — the ragged stages are launched at their worst-case
 * size and read the per-image token counts on the device — so with counts_host == NULL the call only enqueues work on `stream` (it can be
 * captured into a hipGraph) and the host reads `counts` whenever it needs shapes.  counts_host != NULL (B ints; total_tokens_host optional) is
 * the convenience form: ONE host wait at the END of the call fills them.  Since ABI 8 that wait is for the COUNTS only (they are final behind
 * the clustering stage and are copied to the host there): when the call returns, its remaining launches — the head, about 1 ms of device time at
 * batch 256 — may still be queued or running, so that the caller's next launches (the projector) queue up behind them and the device never
 * idles.  `tokens`, `idx_cluster`, `score`, `index_down` and the stage pointers are complete IN STREAM ORDER like the outputs of every other call
 * of this library: work enqueued on `stream` sees them; a host that reads them directly synchronises the stream first (a blocking hipMemcpy on
 * the null stream does). */
int setok_encode(setok_ctx* ctx, void* stream, const void* images, int B, int k, float threshold, const float* noise,
                 const float* token_mask, void* workspace, int64_t workspace_bytes, void* tokens, int32_t* counts,
                 int64_t* idx_cluster, float* score, int64_t* index_down, int32_t* counts_host, int64_t* total_tokens_host,
                 void** stage_x, void** stage_group, void** stage_inter);

/* ---- dense layers ------------------------------------------------------------------------ */

/* C[M,N] = act(A[M,K] · W[N,K]^T + bias[N]) + residual[M,N]          (bias, residual optional)
 * Replaces every nn.Linear on the path: module.py:40,43 (Mlp), :63,71 (Attention qkv/proj),
 * tokenizer.py:180 (`out`), multimodal_projector/builder.py:37-59 (mm_in_projector) and the HF CLIP
 * q/k/v/out_proj/fc1/fc2 linears reached from clip_encoder.py:59.  `act` fuses nn.GELU (exact erf,
 * module.py:41) or CLIP's quick_gelu.  A and W have element type `dtype`; C and residual have
 * `out_dtype` (C may alias residual): the 16-bit type of `dtype` or SETOK_F32 for 16-bit inputs, SETOK_F32 for
 * fp32 inputs (anything else is refused).  K % 64 == 0 (16-bit) or K % 16 == 0 (fp32).
 *
 * Strides, all in elements.  A, C and residual may be column windows of wider buffers — e.g. two column windows of
 * one fused projection buffer — the pointer names the window's first element; W is dense (row stride K):
 *   - lda >= K is A's row stride: a multiple of 8 (16-bit) or 4 (fp32) — A's rows are read in 16-byte pieces, so A
 *     itself is 16-byte aligned (not checked);
 *   - ldc >= N is the row stride of C AND of residual; any value is accepted.  C / residual rows that are 16-byte
 *     aligned (ldc % 8 == 0 for a 16-bit, ldc % 4 == 0 for an fp32 output) are what the fast kernels below need;
 *   - `batch` >= 1 runs independent problems: member b reads A + b * strideA and W + b * strideW and writes
 *     C + b * strideC; residual is read at the same b * strideC; the bias is shared by all members.  With batch > 1
 *     strideA and strideW are multiples of 8 (16-bit) or 4 (fp32); strideW = 0 (one weight for every member) is
 *     allowed, and so are strides larger than the matrices.  With batch == 1 the strides are ignored.
 * No element outside rows [0, M) x columns [0, K) of A is read and none outside [0, M) x [0, N) of C is written,
 * at any stride.
 *
 * Which bits a row gets.  fp32 inputs: always the same (a k-ordered chain that depends on neither M, the strides
 * nor the batch).  16-bit inputs: a 16-bit output with batch == 1, N % 64 == 0 and ldc % 8 == 0 is computed by the
 * LDS-DMA kernels, whose result for a row depends on nothing but that row, W and the bias — not on M, lda, ldc or
 * the rows around it (a sample alone equals the sample inside a batch of images).  Every other combination
 * (batch > 1, an fp32 output, N % 64 != 0 or ldc % 8 != 0) is computed by the 128 x 128 kernel — except fp32-out
 * problems without bias, activation and residual whose batch is large enough (split-K weight gradients).  These have another
 * summation order: a row's bits there are those of the same kernel at batch == 1, but not those of the LDS-DMA
 * kernels, and an activation is evaluated in its exact form for an fp32 output and in its fast form for a 16-bit one.
 * Within any one of these kernels a stride changes addresses only, never bits. */
int setok_linear(void* stream, int dtype, int out_dtype, const void* A, int64_t lda, const void* W,
                 const float* bias, const void* residual, void* C, int64_t ldc, int M, int N, int K,
                 int act, int batch, int64_t strideA, int64_t strideW, int64_t strideC);

/* y[r,:] = LayerNorm(x[r,:]) * gamma + beta   — nn.LayerNorm (module.py:81,83; HF CLIP
 * pre_layrnorm / layer_norm1 / layer_norm2).  Statistics in fp32.  x may alias y. */
int setok_layernorm(void* stream, int dtype, const void* x, const float* gamma, const float* beta,
                    void* y, int rows, int C, float eps);

/* y = act(x) elementwise (n elements) — nn.GELU placed after a LayerNorm in the `mlp{N}x_gelu_Norm`
 * projector (multimodal_projector/builder.py:48-58), where it cannot be fused into a GEMM epilogue; SETOK_ACT_SILU: the nn.SiLU inside
 * TimestepEmbedder.mlp and ResBlock.mlp of the DiffLoss head (loss/diffloss.py:67,115). */
int setok_activation(void* stream, int dtype, const void* x, void* y, int64_t n, int act);

/* Training-mode dropout of the head's Block: nn.Dropout(proj_drop) after the attention projection (module.py:59,72), after the Mlp's activation
 * and after its fc2 (module.py:36,44,45); proj_drop = 0.2 by default (tokenizer.py:26).
 *   y[i] = residual[i] + (keep_i ? x[i] / (1 - p) : 0),   c = offset + i,  keep_i = 16-bit slice (c & 3) of hash(seed, c >> 2) >= p * 2^16
 *   (residual may be NULL; y may alias x or residual; 16-byte aligned operands take the vector kernel, others an element-wise one: same mask)
 * The mask is a pure function of (seed, offset + i) (one SplitMix64 finaliser per four consecutive counters): the backward pass applies the same call to the
 * incoming gradient instead of storing masks, and a step is reproducible from its seed.  Bernoulli(1 - p) like the reference's masks, not
 * bit-equal to torch's Philox stream.  n elements of `dtype`. */
int setok_dropout(void* stream, int dtype, const void* x, const void* residual, void* y, int64_t n, float p, uint64_t seed, uint64_t offset);
/* y = drop(act(x)) in ONE pass: Mlp.forward's `self.drop(self.act(self.fc1(x)))` (module.py:41,44) in training mode.  The same mask as
 * setok_dropout(seed, offset); act(x) is rounded to `dtype` before the mask is applied, so the result is bit-identical to setok_activation
 * followed by setok_dropout in place.  ABI 6. */
int setok_activation_dropout(void* stream, int dtype, const void* x, void* y, int64_t n, int act, float p, uint64_t seed, uint64_t offset);

/* Block-diagonal ("varlen") multi-head self-attention over contiguous row segments.
 * qkv: (rows, 3*H*Dh) laid out [q | k | v], heads inside — the layout both the fused `qkv` Linear
 * of module.py:63 and a concatenated HF q/k/v projection produce.  Row r attends to the rows of
 * its own segment [seg_offsets[s], seg_offsets[s+1]) only:
 *   - ViT tower: segments = images (T rows each)                       clip_encoder.py:59 (HF eager attention)
 *   - inner_encoder: segments = clusters (member tokens only)          tokenizer.py:147-150, module.py:61-73
 *   - inter_encoder: segments = images (L_i cluster tokens each)       tokenizer.py:179
 * out: (rows, H*Dh) = softmax(q k^T * scale) v, heads concatenated (module.py:70).
 * seg_offsets: int32[n_segs+1] on the device; if NULL, uniform segments of `seg_len` rows. */
int setok_attention(void* stream, int dtype, const void* qkv, const int32_t* seg_offsets, int n_segs,
                    int seg_len, void* out, int rows, int H, int Dh, float scale);

/* Multi-head CROSS-attention of uniform query groups to ragged key/value segments — the Q-Former of the
 * reconstruction decoder (cfg 3): BertSelfAttention.forward's cross branch, module.py:283-286 (keys / values from the
 * encoder states), :303 (q k^T), :342 (/ sqrt(d_h), passed as `scale`), :343-345 (+ mask), :348 (softmax), :360-364.
 * The reference pads every image's L_i tokens to a common L and adds (1 - m) * -10000 (module.py:849, 962-973); exp of a
 * score lowered by 10000 is exactly 0 in fp32, so attending to the UNPADDED segment is the same arithmetic.
 * q:   (n_segs * q_len, >= H*Dh) rows, stride ldq; query row r belongs to segment r / q_len.
 * k,v: rows of stride ldkv (typically two column windows of one fused [k | v] projection buffer);
 *      segment s owns rows [kv_offsets[s], kv_offsets[s+1]), at most max_kv of them (int32[n_segs+1], device);
 *      kv_offsets == NULL means uniform segments of max_kv rows.
 * out: (n_segs * q_len, H*Dh) rows of stride ldo. */
int setok_cross_attention(void* stream, int dtype, const void* q, int64_t ldq, const void* k, const void* v,
                          int64_t ldkv, const int32_t* kv_offsets, int n_segs, int q_len, int max_kv, void* out,
                          int64_t ldo, int H, int Dh, float scale);

/* ---- ViT tower glue (HF CLIPVisionEmbeddings reached from clip_encoder.py:59) ------------ */

/* im2col for the stride-p patch conv: images (B,3,H,W) -> patches (B*g*g, Kpad) with column index
 * c*p*p + py*p + px (the flattening of conv weight (C,3,p,p)); columns >= 3*p*p are zero. */
int setok_patchify(void* stream, int dtype, const void* images, void* patches, int B, int H, int W,
                   int p, int Kpad);
/* tokens[b,0,:] = cls + pos[0]; tokens[b,1+i,:] = patch_embed[b,i,:] + pos[1+i]  (embeddings.forward) */
int setok_vit_assemble(void* stream, int dtype, const void* patch_embed, const void* cls, const void* pos,
                       void* tokens, int B, int N, int C);

/* ---- LayerNorm folded into the consuming Linear (bf16 throughput mode) ------------------------------------------------------
 * HF CLIP's encoder layer (reached from clip_encoder.py:59) computes q/k/v = Linear(layer_norm1(h)) and fc1(layer_norm2(h)); the
 * reference's Block does the same with norm1 / norm2 (module.py:88,98).  With W' = gamma * W (rounded to bf16), c = W' 1, b' = b + W beta:
 *     LN(h) W^T + b = rstd_r * (h W'^T - mean_r * c + b' / rstd_r)
 * so the GEMM reads the raw residual stream h and no normalised copy of it is ever written.  The fp32 parity mode keeps the separate
 * setok_layernorm. */

/* stats row r (8 floats): [0], [1] the compact activation-side MFMA fragment of (-mean_r, 1 / rstd_r) (two bf16 pairs: two-way splits),
 * [2] and [4] rstd_r = 1 / sqrt(var + eps), [5] mean_r, the rest 0.  Two-pass fp32 statistics in setok_layernorm's order; rows x C, `dtype`. */
int setok_row_stats(void* stream, int dtype, const void* x, float* stats, int rows, int C, float eps);

/* Once per weight load: W (N, K) bf16, gamma / beta (K) fp32, bias (N) fp32 or NULL ->
 * w_gamma (N, K) bf16, w_colsum (N) fp32, bias_folded (N) fp32, col_frag (N, 4) fp32-sized words: the weight-side MFMA fragment of
 * (w_colsum[n], bias_folded[n]) as 8 bf16. */
int setok_ln_fold(void* stream, const void* W, const float* gamma, const float* beta, const float* bias, void* w_gamma,
                  float* w_colsum, float* bias_folded, float* col_frag, int N, int K);

/* C[M,N] = act(LN(A)[M,K] . W[N,K]^T + bias) from w_gamma / col_frag of setok_ln_fold and the row statistics of A (bf16 in, bf16 out;
 * K % 64 == 0, N % 64 == 0, lda >= K and ldc >= N multiples of 8: A and C may be column windows of wider buffers as in setok_linear;
 * w_gamma, col_frag and row_stats are dense).  The kernel is the one setok_linear picks for the same 16-bit problem: a row's bits depend on
 * neither M nor the strides. */
int setok_linear_ln(void* stream, const void* A, int64_t lda, const void* w_gamma, const float* col_frag, const float* row_stats,
                    void* C, int64_t ldc, int M, int N, int K, int act);

/* ---- SeTok head glue --------------------------------------------------------------------- */

/* x[b,i,:] = hidden[b, i+skip, :] + pos2d[i,:] : feature_select's `[:, 1:]` (clip_encoder.py:43,
 * skip = 1 for 'patch', 0 for 'cls_patch') fused with the PositionalEncoding2D add
 * (tokenizer.py:164-168).  hidden: (B, N+skip, C); pos2d: (N, C) in `dtype`; the sum is rounded
 * once to `dtype`, as the reference's `x + pos_emb` is. */
int setok_select_add_pos(void* stream, int dtype, const void* hidden, const void* pos2d, void* x,
                         int B, int N, int C, int skip);

/* cluster_dpc_knn (tokenizer.py:78-121), batched over B images, each exactly as the reference's
 * per-image call:  D = cdist(x,x)/sqrt(C) (:82) [token_mask :84-86]; density from the k nearest
 * (self included) (:88-90) + noise*1e-6 (:91) [* token_mask :93-94]; delta with the row-j-max
 * quirk (:96-99); score = delta*density (:101); centres = {score > threshold} (:103) else the
 * min_cluster_num best scores, ascending by index (:104-107); idx_cluster = argmin over centre
 * rows, centres own themselves (:111-119).
 *   x:          (B, N, C) `dtype`                      noise, token_mask: (B, N) fp32 or NULL
 *   idx_cluster:(B, N) int64 out                       score: (B, N) fp32 out  (reference: (1,N) per image)
 *   index_down: (B, N) int64 out, first counts[b] entries valid, rest -1
 *   counts:     (B) int32 out  = L_b
 *   dist_ws:    fp32 workspace for the scaled distance matrix, vec_ws: fp32 workspace (density, row max, delta, spare) — sizes from
 *               setok_cluster_workspace; both may be NULL when it reports 0 (bf16, N <= 256, C % 64 == 0: the whole call is ONE launch,
 *               one workgroup per image, the distance matrix lives in MFMA accumulators and never reaches memory).
 * Requires N <= 1024, 1 <= k <= N, min_cluster_num <= N. */
int setok_cluster_dpc_knn(void* stream, int dtype, const void* x, int B, int N, int C, int k,
                          float threshold, int min_cluster_num, const float* noise,
                          const float* token_mask, int64_t* idx_cluster, float* score,
                          int64_t* index_down, int32_t* counts, float* dist_ws, float* vec_ws);

/* Workspace of setok_cluster_dpc_knn for a problem shape, in floats (0 = not needed). */
int setok_cluster_workspace(int dtype, int B, int N, int C, int64_t* dist_floats, int64_t* vec_floats);

/* Stable counting sort of each image's tokens by cluster id (`labels.unique()` order ==
 * ascending label, tokenizer.py:141-143) plus the segment tables the ragged stages need:
 *   perm:        (B*N) int32  — sorted position -> source row (b*N + i)
 *   seg_offsets: (total+1) int32, total = sum_b counts[b]: cluster segments in sorted-row space
 *   img_offsets: (B+1) int32 — prefix sum of counts (segments of the inter-encoder / ragged output)
 * Capacity of seg_offsets must be B*N+1. */
int setok_cluster_sort(void* stream, const int64_t* idx_cluster, const int32_t* counts, int B, int N,
                       int32_t* perm, int32_t* seg_offsets, int32_t* img_offsets);

/* out[p,:] = x[perm[p],:]   (the `x[m]` gathers of tokenizer.py:150, all clusters at once) */
int setok_gather_rows(void* stream, int dtype, const void* x, const int32_t* perm, void* out, int rows, int C);

/* out[s,:] = mean over rows [seg_offsets[s], seg_offsets[s+1]) of h   (tokenizer.py:151).
 * n_segs_dev: device int32 holding the segment count (= img_offsets[B]); max_segs = launch bound. */
int setok_segment_mean(void* stream, int dtype, const void* h, const int32_t* seg_offsets,
                       const int32_t* n_segs_dev, int max_segs, void* out, int C);

/* ---- after the path: prepare_inputs_labels_for_multimodal (setokim_arch.py:213-355) ------------------------------------
 * The reference walks the batch in Python: strips padding by the mask (:258-259), cuts every sequence at its
 * IMAGE_TOKEN_INDEX placeholders, embeds the text pieces, interleaves them with the images' (L_i, D) token matrices
 * (:273-303), truncates (:311-314) and pads to the batch maximum (:317-339).  Here it is three asynchronous steps on device
 * buffers; the host reads `seq_len` once in between to size the outputs (max over the batch, :317).
 *
 * img_offsets: int32[n_images + 1], row offsets of the packed image tokens (image i owns rows [off[i], off[i+1])).
 * Images are consumed in batch order, one per placeholder; a sequence WITHOUT a placeholder still consumes one (:264-271). */

/* Step 1.  seq_len[b] = tokens kept by the mask - placeholders + rows of the sequence's images, truncated to max_length
 * (<= 0: no limit); img_start[b] = index of its first image; status (int32[4]): [0] = 1 if the batch needs more than n_images
 * images (the reference raises IndexError at image_features[cur_image_idx]), [1] = images needed, [2] = 1 if a kept id other than
 * the placeholder lies outside [0, vocab) (the reference's embed_tokens raises IndexError, :273; vocab = 0 disables the check),
 * [3] = flat position b*T + t of the first such id (-1 if none).  attention_mask: uint8 (B,T), NULL = all kept (:250-251).
 * count_ws: int32[3*B] scratch. */
int setok_splice_lengths(void* stream, const int64_t* input_ids, const uint8_t* attention_mask, int B, int T,
                         int64_t image_token_index, int64_t vocab, const int32_t* img_offsets, int n_images, int max_length,
                         int32_t* seq_len, int32_t* img_start, int32_t* status, int32_t* count_ws);

/* Step 2.  For every output position (b, p), p < max_len: src (int32) = embedding-table row (token id) | -(image-token row + 1)
 * | INT32_MIN for a zero padding row; new_labels (NULL iff labels is NULL, :341-342): the token's label, ignore_index on
 * image rows (:293) and padding (:319), target_token_index mapped to ignore_index (:344); new_mask (uint8, optional);
 * new_position_ids (int64, optional; 0..len-1 inside the kept range, 0 in the padding, :321,337).  left_pad selects
 * tokenizer_padding_side == "left" (:324-330).  max_len = 0 (no sequence keeps anything): nothing is written and the outputs may be NULL. */
int setok_splice_plan(void* stream, const int64_t* input_ids, const uint8_t* attention_mask, const int64_t* labels, int B, int T,
                      int64_t image_token_index, int64_t ignore_index, int64_t target_token_index,
                      const int32_t* img_offsets, const int32_t* seq_len, const int32_t* img_start, int max_len, int left_pad,
                      int32_t* src, int64_t* new_labels, uint8_t* new_mask, int64_t* new_position_ids);

/* Step 3.  out[r, :] = embed_table[src[r]] | image_tokens[-(src[r] + 1)] | 0, r < rows = B * max_len: embed_tokens (:266,284)
 * fused with the concatenations and the zero padding (:296-303, 324-333).  D * sizeof(dtype) must be a multiple of 16.
 * A src the operands cannot serve (>= vocab; an image-token row >= image_token_rows or with image_tokens == NULL, e.g. an
 * IMAGE_TOKEN_INDEX in a text-only call) is never turned into an address: the row is zero-filled and, with `status` (int32[2], optional,
 * device), status[0] = 1 and status[1] = the first such row — where the reference's embed_tokens raises IndexError (:273).
 * rows = 0: src and out may be NULL (status is still initialised). */
int setok_splice_rows(void* stream, int dtype, const int32_t* src, const void* embed_table, int vocab, const void* image_tokens,
                      int64_t image_token_rows, void* out, int64_t rows, int D, int32_t* status);

/* Backward of step 3 (the reference gets it from autograd: stage 2 trains mm_in_projector THROUGH the splice, scripts/pretrain_mm_proj.sh:40,
 * setokim_arch.py:290-293): d_image_tokens[-(src[r] + 1)] = d_out[r] (rows no output position consumed — truncation — are zero);
 * d_embed (fp32 (vocab, D), optional, ACCUMULATED into: the caller zeroes it) += d_out[r] at src[r] >= 0 — hardware fp32 atomics, the
 * summation order over a repeated token id is not fixed.  Either output may be NULL. */
int setok_splice_rows_bwd(void* stream, int dtype, const int32_t* src, const void* d_out, int64_t rows, int D,
                          void* d_image_tokens, int64_t image_token_rows, float* d_embed, int vocab);

/* ---- reconstruction decoder: the output the reference never defines ---------------------------------------------
 * SetokDeTokenizer.forward ends at decoder_norm and returns None (src/model/setok/detokenizer.py:101-120) while SeTok.forward hands the result
 * to a pixel-space loss as an image (src/model/setok/model.py:75-76,91).  The pixel head = one setok_linear (decoder_embed_dim -> patch^2 * 3 per
 * query) + this rearrangement: image[b, c, h*p + pi, w*p + qi] = patches[(b*gh + h)*gw + w, (pi*p + qi)*3 + c]; ld = row stride of `patches`
 * in elements (>= 3 p^2: the GEMM output may be padded). */
int setok_unpatchify(void* stream, int dtype, const void* patches, int64_t ld, void* image, int B, int gh, int gw, int p);

/* out[0] = mean over the n elements of (pred - target)^2 (kind 0: WeightedMSELoss without a mask, src/model/loss/mse.py:9-19) or |pred - target|
 * (kind 1: the pixel term of the GAN loss, src/model/loss/discriminator.py:161,170).  fp32 accumulation in two fixed-order stages (no atomics).
 * ws: >= 1024 floats of scratch. */
int setok_pixel_loss(void* stream, int dtype, const void* pred, const void* target, int64_t n, int kind, float* ws, float* out);

/* ---- training step of the trainable head --------------------------------------------------------------
 * The reference trains through torch autograd (src/train/setok_trainer.py / train_setokim.py drive `loss.backward()`); the tower is
 * frozen (clip_encoder.py:50, unfreeze_mm_vision_tower=False) and cluster_dpc_knn is no_grad (tokenizer.py:79), so the backward
 * pass covers group_encoding / inter_encoder / out (tokenizer.py:147-180) and the Block / Attention / Mlp of module.py:29-100.
 * Its GEMMs are setok_linear calls (dX = dY W: A = dY, W = W^T;  dW = dY^T X: A = dY^T, W = X^T, fp32 out); the entry points below
 * are everything else.  All deterministic (no atomics).  `ws` arguments are caller-allocated fp32 scratch. */

/* out[c * ldo + r] = x[r * ldx + c] for r < rows, c < cols; out rows are zero-filled for r in [rows, ldo) (pads the contraction
 * dimension of the following GEMM to its K granule).  chunk > 0 (a divisor of ldo): the padded row range is cut into ldo / chunk
 * pieces stored one after the other, each a (cols, chunk) matrix — the operand layout of a split-K batched dW GEMM whose
 * fp32 partial products are then summed in a fixed order (setok_colsum over the batch).  colsum_partial (optional): fp32
 * [ceil(ldo / 64) * cols]; row b receives the column sums of x over rows [64 b, 64 b + 64) — summing these rows (setok_colsum, fp32)
 * gives the bias gradient without another pass over dY. */
int setok_transpose(void* stream, int dtype, const void* x, int64_t ldx, int rows, int cols, void* out, int64_t ldo, int chunk,
                    float* colsum_partial);

/* out[c] (+)= sum_r x[r, c] (bias gradients).  ws: fp32[ws_rows * cols], ws_rows >= 1 (more rows = more parallelism). */
int setok_colsum(void* stream, int dtype, const void* x, int rows, int cols, float* out, int accumulate, float* ws, int ws_rows);

/* Backward of nn.LayerNorm (module.py:81,83): dx = rstd (g - mean(g) - xhat mean(g xhat)) [+ res], g = dy * gamma;
 * dgamma (+)= sum_rows dy * xhat, dbeta (+)= sum_rows dy.  dx may be NULL (first layer: only the parameter gradients are needed);
 * `accumulate` serves the norm1 shared by a Block's attention sub-layers (module.py:87-88).  ws: fp32[ws_rows * C], ws_rows >= 2. */
int setok_layernorm_bwd(void* stream, int dtype, const void* x, const void* dy, const float* gamma, float eps, int rows, int C,
                        void* dx, const void* res, float* dgamma, float* dbeta, int accumulate, float* ws, int ws_rows);

/* Backward of nn.GELU (exact erf, module.py:41): dx = dy * (Phi(pre) + pre * phi(pre)). */
int setok_gelu_bwd(void* stream, int dtype, const void* pre, const void* dy, void* dx, int64_t n);
/* dx = gelu'(pre) * drop(dy): the backward of `drop(act(fc1 x))` in ONE pass — bit-identical to setok_dropout on the gradient (in place) followed by
 * setok_gelu_bwd.  ABI 6. */
int setok_gelu_bwd_dropout(void* stream, int dtype, const void* pre, const void* dy, void* dx, int64_t n, float p, uint64_t seed, uint64_t offset);

/* Backward of setok_attention (module.py:61-73) over the same segments: dqkv laid out [dq | dk | dv] like qkv.
 * out / dout: (rows, H*Dh).  ws: fp32[2 * rows * H] (log-sum-exp and do.o per row and head). */
int setok_attention_bwd(void* stream, int dtype, const void* qkv, const int32_t* seg_offsets, int n_segs, int seg_len,
                        const void* out, const void* dout, void* dqkv, int rows, int H, int Dh, float scale, float* ws);

/* Backward of setok_cross_attention (and of self-attention in the same operand layout) for the reconstruction decoder: n_segs groups of q_len query
 * rows; segment s attends to key / value rows [kv_offsets[s], kv_offsets[s+1]) (at most max_kv of them), or, with kv_offsets == NULL, to the
 * uniform rows [s * max_kv, (s+1) * max_kv) (self-attention: max_kv = q_len and q, k, v the three column windows of one qkv buffer).
 * q, out, dout, dq: (n_segs * q_len, >= H*Dh) rows of strides ldq, ldo, lddo, lddq; k, v: rows of stride ldkv; dk, dv: rows of stride lddkv
 * (the [dk | dv] halves of one buffer, or the dk / dv windows of a dqkv buffer).  Operands and strides 16-byte aligned, Dh % 8 == 0.
 * The log-sum-exp and do.o of every row are recomputed (nothing is saved by the forward).  Deterministic: no atomics, fixed summation order,
 * a segment's gradients do not depend on the other segments.  ws: fp32[2 * n_segs * q_len * H]. */
int setok_mha_bwd(void* stream, int dtype, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv,
                  const int32_t* kv_offsets, int n_segs, int q_len, int max_kv, const void* out, int64_t ldo, const void* dout,
                  int64_t lddo, void* dq, int64_t lddq, void* dk, void* dv, int64_t lddkv, int H, int Dh, float scale, float* ws);

/* Backward of setok_pixel_loss(setok_unpatchify(patches)) in one pass: dpatches (B*gh*gw, ld) receives d loss / d patch rows in the layout
 * the pixel head's GEMM produced (columns >= 3 p^2, the GEMM's pad, are zero), scaled by upstream[0] (fp32, device: the loss's incoming
 * gradient).  kind 0 (mse): 2 (pred - gold) / n;  kind 1 (l1): sign(pred - gold) / n with sign(0) = 0;  n = B * 3 * gh*p * gw*p.
 * kind 2: the backward of setok_unpatchify alone — `pred` is d loss / d image and `gold` is not read. */
int setok_pixel_loss_bwd(void* stream, int dtype, const void* pred, const void* gold, int kind, const float* upstream, void* dpatches,
                         int64_t ld, int B, int gh, int gw, int p);

/* Backward of setok_segment_mean (tokenizer.py:151): drows[r, :] = dseg[s, :] / n_s for every member row r of segment s. */
int setok_segment_mean_bwd(void* stream, int dtype, const void* dseg, const int32_t* seg_offsets, const int32_t* n_segs_dev,
                           int max_segs, void* drows, int C);

/* torch.optim.AdamW step on fp32 master parameters (decoupled weight decay, bias correction by `step` >= 1), gradient pre-scaled
 * by grad_scale (1 / world_size after a sum all-reduce); param_lp (optional, dtype lp_dtype) receives the rounded copy the next
 * forward uses. */
int setok_adamw(void* stream, int lp_dtype, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* param_lp,
                int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale);

/* ---- LLM prefill of BASELINE config 5 (last row) -------------------------------------------------------------
 * SetokimLlamaForCausalLM.forward (src/model/language_model/setokim_llama.py:130-143) hands the spliced embeddings to
 * `self.model` — HuggingFace `transformers` LlamaModel (third party, pinned 4.46.3 by the reference) — and `self.lm_head`.
 * Its Linears are setok_linear calls; these are the other pieces of LlamaDecoderLayer.forward (eager path). */

/* LlamaRMSNorm.forward: y = weight * (x * rsqrt(mean(x^2) + eps)).to(dtype) — statistics in fp32, the normalised value rounded
 * to the activation dtype before the weight multiply. */
int setok_rmsnorm(void* stream, int dtype, const void* x, const float* weight, void* y, int rows, int C, float eps);

/* apply_rotary_pos_emb (rotate_half convention, default rope: inv_freq = theta^(-2i/Dh), cos / sin in fp32 rounded to dtype) in
 * place on the q and k thirds of qkv: (rows, 3*H*Dh) laid out [q | k | v]; position_ids: int64[rows]. */
int setok_rope(void* stream, int dtype, void* qkv, const int64_t* position_ids, int rows, int H, int Dh, float theta);
/* ... with grouped-query attention (LlamaConfig.num_key_value_heads = Hkv < H, H % Hkv == 0: Llama-2-70B, Llama-3, Mistral): rows of
 * (H + 2*Hkv)*Dh elements [q: H heads | k: Hkv heads | v: Hkv heads]; the H + Hkv heads of q and k are rotated.  Hkv == H is setok_rope. */
int setok_rope_gqa(void* stream, int dtype, void* qkv, const int64_t* position_ids, int rows, int H, int Hkv, int Dh, float theta);

/* LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) on a fused (rows, 2*F) buffer [gate | up] -> (rows, F); act_fn = SiLU. */
int setok_swiglu(void* stream, int dtype, const void* gate_up, void* out, int64_t rows, int F);
/* ... on a buffer of INTERLEAVED pairs: gate_up_pairs (rows, 2 F) with (gate_j, up_j) in columns 2 j, 2 j + 1 — the output layout of a Linear whose weight
 * rows are interleaved the same way (setok_linear_swiglu's).  Same arithmetic, same bits as setok_swiglu on the de-interleaved buffer. */
int setok_swiglu_pairs(void* stream, int dtype, const void* gate_up_pairs, void* out, int64_t rows, int F);
/* out (M, F) = act_fn(A Wg^T) * (A Wu^T) in ONE launch: the gate|up Linear of LlamaMLP (HF modeling_llama.py LlamaMLP.forward, reached from
 * /root/reference/src/model/language_model/setokim_llama.py:130-143) with SwiGLU in the GEMM's epilogue — the (M, 2 F) intermediate is never written.
 * W_pairs (2 F, K): row 2 j = gate_proj.weight[j], row 2 j + 1 = up_proj.weight[j].  torch's 16-bit rounding points are kept (gate and up rounded to the
 * element type, the activation rounded, the product rounded), so the result equals setok_linear(W_pairs) followed by setok_swiglu_pairs bit for bit.
 * 16-bit element types; M % 256 == 0, (2 F) % 256 == 0, K % 64 == 0, K >= 128, else SETOK_EUNSUPPORTED (send those rows through the unfused pair).
 * lda >= K and ldo >= F are the row strides of A and out in elements, multiples of 8 (SETOK_EINVAL otherwise); a stride changes addresses only. */
int setok_linear_swiglu(void* stream, int dtype, const void* A, int64_t lda, const void* W_pairs, void* out, int64_t ldo, int M, int F, int K);

/* Causal self-attention of LlamaAttention (eager_attention_forward: softmax(q k^T * scale + mask) v, fp32 softmax) over B
 * sequences of T rows of a fused [q | k | v] buffer (num_key_value_heads == num_attention_heads).  Query i of a sequence sees key
 * j iff j <= i and key_mask[b*T + j] != 0 (key_mask NULL = all tokens): the causal + padding mask HF builds from attention_mask.
 * A query that sees no token at all (padding before a sequence's first token) gets zeros (HF gives such rows an arbitrary uniform
 * mix; they are padding and masked out of the loss, setokim_llama.py:149-152). */
int setok_attention_causal(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, void* out, int B, int T, int H, int Dh,
                           float scale);
/* ... with grouped-query attention (HF repeat_kv, modeling_llama.py: query head h reads key / value head h / (H / Hkv)): qkv rows of
 * (H + 2*Hkv)*Dh elements [q | k | v], out rows of H*Dh.  Hkv == H is setok_attention_causal (same kernels, same bits). */
int setok_attention_causal_gqa(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, void* out, int B, int T, int H, int Hkv, int Dh,
                               float scale);

/* The language-model loss of SetokimLlamaForCausalLM.forward (setokim_llama.py:145-160): logits (B*T rows of V, row stride ld) are read as
 * fp32; position t predicts labels[t + 1]; positions with attention_mask[t + 1] == 0 (NULL = none) or labels[t + 1] == ignore_index are left
 * out; out[0] = mean cross entropy over the rest (NaN if none), out[1] = their number.  row_ws: 2*B*T floats of workspace.  Deterministic. */
int setok_lm_loss(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels, const uint8_t* attention_mask, int B, int T,
                  int V, int ignore_index, float* row_ws, float* out);

/* ---- Backward through the FROZEN LLM (stage 2 of the reference's recipe trains mm_in_projector through the language-model loss:
 * scripts/pretrain_mm_proj.sh, src/train/train_setokim.py:335-339).  Only the dX chain exists: the Linears' dX are setok_linear calls against
 * transposed weights, these are the backward twins of the entries above; no weight gradient is formed.  All deterministic (no atomics). */

/* Backward of setok_lm_loss: dlogits[b, t, :] = upstream * (softmax(logits[b, t, :].float()) - onehot(labels[b, t + 1])) / n for the positions
 * the forward counted, exact zeros in every other row (every sequence's last position among them).  loss_out: the forward's `out` on the
 * device (n = loss_out[1] is read there: no host synchronisation); upstream: one float on the device (NULL = 1).  dlogits: B*T rows of V in
 * `dtype` with its own row stride ldd; logits / dlogits rows may start at any element boundary (resized vocabularies: 32003).  When the forward
 * counted no position every row is zero (nothing is divided by n). */
int setok_lm_loss_bwd(void* stream, int dtype, const void* logits, int64_t ld, const int64_t* labels, const uint8_t* attention_mask, int B, int T,
                      int V, int ignore_index, const float* loss_out, const float* upstream, void* dlogits, int64_t ldd);

/* dx of setok_rmsnorm (no weight gradient): statistics recomputed in fp32; g = (dy * weight).to(dtype) is the gradient at the forward's rounding
 * point, dx = rstd * (g - xhat * mean(g * xhat)) rounded to dtype, + dres (optional: the residual branch's gradient, added in the same pass).
 * dx may alias dy or dres. */
int setok_rmsnorm_bwd(void* stream, int dtype, const void* x, const float* weight, const void* dy, const void* dres, void* dx, int rows, int C,
                      float eps);

/* The transpose of setok_rope_gqa, in place on the dq and dk parts of a [dq | dk | dv] buffer: the same cos / sin tables (fp32, rounded to
 * dtype), the rotation reversed; dv is left untouched. */
int setok_rope_bwd_gqa(void* stream, int dtype, void* dqkv, const int64_t* position_ids, int rows, int H, int Hkv, int Dh, float theta);

/* Backward of setok_swiglu_pairs: from the pre-activation pairs (gate_j, up_j) (rows, 2 F) and dout (rows, F) to d (gate_j, up_j) in the same
 * interleaved layout — what the dX GEMM against the pair-interleaved weight consumes. */
int setok_swiglu_pairs_bwd(void* stream, int dtype, const void* gate_up_pairs, const void* dout, void* dpairs, int64_t rows, int F);

/* Backward of setok_attention_causal_gqa.  qkv: the forward's input (post-rotary, [q: H | k: Hkv | v: Hkv] heads), out: its output, dout:
 * d loss / d out; dqkv: the result in the layout of qkv.  The mask is the forward's (query i sees key j iff j <= i and key_mask[j] != 0): a query
 * that sees no key gets dq = 0, a key no query sees gets dk = dv = 0.  dk / dv of a shared key / value head are the sum over its H / Hkv query
 * heads in head order.  Nothing is saved by the forward: the log-sum-exp and do.o are recomputed into ws (2*B*T*H floats).  Two runs give the
 * same bits and a sequence's gradients do not depend on the other sequences of the batch.  Head dim 128 in the 16-bit element type runs an MFMA
 * pair (SETOK_LLAMA_ATTN_BWD_GENERIC=1 in the environment forces the generic pair), everything else a generic wave-per-row pair. */
int setok_attention_causal_bwd_gqa(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, const void* out, const void* dout, void* dqkv,
                                   int B, int T, int H, int Hkv, int Dh, float scale, float* ws);
/* ... Hkv == H */
int setok_attention_causal_bwd(void* stream, int dtype, const void* qkv, const uint8_t* key_mask, const void* out, const void* dout, void* dqkv,
                               int B, int T, int H, int Dh, float scale, float* ws);

/* ---- KV-cached greedy decoding (SetokimLlamaForCausalLM.generate, setokim_llama.py:329-396: encode, splice, prefill, then one token per
 * step against `past_key_values`, :99,133,189).  The step's Linears are setok_linear calls at M = B, its RMSNorm / rotary embedding / SwiGLU the
 * entries above on B rows; these are the rest.  Pure additions: the ABI version stays 9. */

/* Keys of one chunk of the decode attention: its work is cut over (chunk of this many cache slots, key / value head, sequence).  A constant, so
 * that how a sequence's keys are partitioned (and every summation order with it) depends on `len` alone. */
#define SETOK_DECODE_CHUNK 128

/* HF DynamicCache.update (reached from LlamaAttention.forward, modeling_llama.py, with `past_key_values` of setokim_llama.py:133): the post-rotary
 * k and v columns of B*T rows of a fused [q: H | k: Hkv | v: Hkv] buffer (what setok_rope_gqa leaves behind) are copied to slots
 * [pos0, pos0 + T) of every sequence of a per-layer cache.  k_cache, v_cache: (B, Hkv, cap, Dh) in `dtype` - the keys of one (sequence,
 * key / value head) are contiguous rows.  16-byte accesses (operands 16-byte aligned, Dh % 8 == 0); every other slot is left untouched. */
int setok_kv_append(void* stream, int dtype, const void* qkv, void* k_cache, void* v_cache, int B, int T, int H, int Hkv, int Dh, int cap, int pos0);

/* eager_attention_forward (HF modeling_llama.py: softmax(q k^T * scale + mask) v, fp32 softmax, repeat_kv) for ONE new token per sequence:
 * query row b of q (B rows of stride ldq elements, H heads of Dh - the q part of the step's fused qkv buffer is read in place) against the cached
 * keys / values of sequence b.  A key counts iff its slot is < len and key_mask[b * cap + slot] != 0 (key_mask: (B, cap) uint8); a sequence
 * without such a key gets zeros (setok_attention_causal's convention).  out: (B, H*Dh).
 * Each K / V byte of a (sequence, key / value head) is read once, for the H / Hkv query heads of its group together.  ws: fp32 workspace of
 * ws_floats >= B * H * ceil(len / SETOK_DECODE_CHUNK) * (Dh + 2) floats (per-chunk maximum, sum and Dh accumulators, merged in chunk order by a
 * second launch: no atomics).  A sequence's output bits depend only on its own q, keys, values, mask and `len`: not on B, not on cap, not on the run.
 * In the 16-bit types the probabilities are rounded to the element type before they multiply V (HF's rounding point).  Dh % 8 == 0; Dh = 128 in the
 * 16-bit type is the tuned shape; masked slots below len must hold initialised memory (they are read, then discarded). */
int setok_attention_decode_gqa(void* stream, int dtype, const void* q, int64_t ldq, const void* k_cache, const void* v_cache,
                               const uint8_t* key_mask, void* out, int B, int H, int Hkv, int Dh, int cap, int len, float scale, float* ws,
                               int64_t ws_floats);

/* Greedy selection (`do_sample=False` of HF GenerationMixin, reached from setokim_llama.py:381-396: torch.argmax(next_token_scores, dim=-1)):
 * out[r] (int64) = the LOWEST index of the maximum of row r of x (rows x V in `dtype`, row stride ld elements, any alignment, V = 32003 included);
 * a NaN counts as the maximum.  Deterministic. */
int setok_argmax_rows(void* stream, int dtype, const void* x, int64_t ld, int rows, int V, int64_t* out);

/* ---- Extending a cache (csrc/attn_extend.hip): Tn >= 1 new tokens per sequence against a cache that already holds len0 older slots — chunked
 * prefill, the next turn of a conversation, scoring several candidate tokens in one pass (HF LlamaAttention.forward with `past_key_values` on a
 * Tn-token input).  setok_kv_append with T = Tn, pos0 = len0 runs first, unchanged.  Pure additions: the ABI version stays 9. */

/* Keys of one chunk of the extend attention, counted from slot 0: its work is cut over (chunk, key / value head x tile of stacked query rows,
 * sequence).  A constant, so that how a row's keys are partitioned (and every summation order with it) depends on len0, Tn, the row and the mask
 * alone.  256 and not SETOK_DECODE_CHUNK: every (query row, query head, chunk) leaves Dh + 2 fp32 partials, and with Tn rows per sequence those are the
 * call's largest traffic and its workspace; 2048 cached slots still give 9 chunks x Hkv workgroups per sequence at Tn = 8. */
#define SETOK_EXTEND_CHUNK 256
/* Chunks a workgroup of the MFMA kernel (head dim 128 in the 16-bit type) carries its online softmax across before it writes a partial, when a group
 * brings more than 32 stacked rows (H / Hkv * Tn > 32): with hundreds of rows per sequence the partials are the call's largest traffic.  A rule in
 * H / Hkv * Tn alone, so what the bits depend on does not change. */
#define SETOK_EXTEND_SPAN 4

/* Floats of workspace setok_attention_extend_gqa needs for the same arguments: B * Tn * H * P * (Dh + 2), P partials per (query row, query head):
 * P = ceil((len0 + Tn) / SETOK_EXTEND_CHUNK), or — the MFMA kernel (this build's 16-bit `dtype`, Dh = 128) with H / Hkv * Tn > 32 —
 * P = ceil((len0 + Tn) / (SETOK_EXTEND_SPAN * SETOK_EXTEND_CHUNK)).  The ONE statement of that rule: hosts size their workspace by this call.  With
 * SETOK_F32 it is the first formula, which suffices for every dtype.  0 for shapes the entry point refuses. */
int64_t setok_attention_extend_workspace(int dtype, int B, int Tn, int H, int Hkv, int Dh, int len0);

/* eager_attention_forward for Tn new tokens per sequence.  q: rows b * Tn + i of the step's fused post-rotary [q | k | v] buffer, read in place with
 * row stride ldq elements (H heads of Dh).  k_cache, v_cache: (B, Hkv, cap, Dh) in `dtype`; they already hold the new tokens' keys and values in
 * slots [len0, len0 + Tn).  key_mask: (B, cap) uint8.  out: (B * Tn, H * Dh).
 * The rule for which keys count:
 *   - Query i of sequence b counts slot j iff j <= len0 + i and key_mask[b][j] != 0.
 *   - A query with no counted key gets zeros.  This is the convention of setok_attention_causal_gqa and setok_attention_decode_gqa.
 *   - Slots that do not count are never allowed to reach the output, whatever bytes they hold.  This covers slots >= len0 + Tn.  It also covers
 *     slots > len0 + i, which hold real keys of later queries.
 * Slots >= len0 + Tn are never read; a masked slot below len0 + Tn is read and discarded by selection (it may hold NaN).
 * Scores and softmax in fp32; in the 16-bit types exp(s - m) is rounded to the element type before it multiplies V, the normaliser sums the unrounded
 * values.  len0 = 0 is a causal prefill read from the cache; Tn = 1 agrees with setok_attention_decode_gqa to tolerance, not to the bit (another chunk
 * length, another summation order).  Each K / V byte of a (sequence, key / value head) is read once per 128 stacked (query row, group head) rows.
 * workspace: fp32, 8-byte aligned, workspace_floats >= setok_attention_extend_workspace(dtype, B, Tn, H, Hkv, Dh, len0): per (sequence, query row,
 * query head, chunk) the chunk's maximum, sum and Dh accumulators, merged in chunk order by a second launch: no atomics.  A row's output bits depend only on its sequence's
 * q, keys, values, mask, len0, Tn and i: not on B, not on cap, not on the run.  Dh % 8 == 0; Dh = 128 in the 16-bit type runs the MFMA kernel, everything
 * else a generic wave-per-(row, head, chunk) kernel.  Refused on the host (-1, setok_last_error): null operands, bad shapes, len0 + Tn > cap, a
 * workspace that is too small. */
int setok_attention_extend_gqa(void* stream, int dtype, const void* q, int64_t ldq, const void* k_cache, const void* v_cache, const uint8_t* key_mask,
                               void* out, int B, int Tn, int H, int Hkv, int Dh, int cap, int len0, float scale, float* workspace,
                               int64_t workspace_floats);

/* ---- Sampling (csrc/sample.hip): `do_sample=True` of HF GenerationMixin with TemperatureLogitsWarper, TopKLogitsWarper and TopPLogitsWarper in
 * HF's order, which is what SetokimLlamaForCausalLM.generate asks for (setokim_llama.py:341-356).  The draw itself is one uniform number per row,
 * and that number is an INPUT: out[r] is a pure function of (row r of the logits, u[r], temperature, top_k, top_p), the same bits in every run.
 * Pure addition: the ABI version stays 9.
 *
 * Per row (logits: rows x V in `dtype`, row stride ld >= V elements, any alignment; columns >= V are never read):
 *   1. s_i = float(logit_i) / temperature in fp32 (HF casts the step's logits to fp32 before its processors, for every model dtype).
 *   2. top-k (top_k > 0): keep i iff s_i >= the top_k-th largest value of the row; ties at the threshold are all kept.  top_k == 0 and
 *      top_k >= V mean no filter.
 *   3. top-p (top_p < 1): keep i iff the probability mass of the kept tokens with a STRICTLY LARGER score is < top_p, probabilities taken over the
 *      set that survived top-k.  Equal scores are kept or dropped together; the top token always survives.  (HF sorts and cuts inside a run of
 *      equal scores by sort position; on rows without ties at the cut the kept sets are identical.)
 *   4. Fixed-point weights: w_i = rint(exp(s_i - max s) * 2^32) as a 64-bit integer, 0 for a filtered token.  Every later sum - histogram masses,
 *      the normaliser W = sum of the kept w_i, the prefix - is an integer sum, exact in any association.  A token whose probability is below
 *      2^-33 of the maximum's has weight 0: it cannot be drawn and its `probs` entry is 0.
 *   5. The draw: u24 = (uint32)(clamp(u[r], 0, 1 - 2^-24) * 2^24); target = (W * u24) >> 24 through the 128-bit product; out[r] (int64) = the
 *      unique i, in INDEX order, with prefix_i <= target < prefix_i + w_i (prefix_i = the sum of w_j, j < i).
 *   6. A row that contains a NaN or +inf, or has no finite entry, is bad: out[r] = -1 and, when given, zeros in its `probs` row (HF raises
 *      "probability tensor contains either inf, nan or element < 0").  The other rows are unaffected.
 *   7. probs (may be NULL): (rows, V) fp32, row stride ld_probs >= V, receives w_i / W.
 * Refused on the host before any launch (-1, setok_last_error): a null logits / u / out, V < 1 or V > 2^20, ld < V, ld_probs < V with probs,
 * a temperature that is not finite or <= 0, top_k < 0, top_p outside (0, 1], a dtype the library does not serve.  rows == 0 launches nothing.
 * One workgroup of 1024 threads per row; the row is read from memory once and kept in LDS as fp32 (V <= 36864; a longer row is re-read through
 * L2 by every pass).  No float atomics and no float prefix sums anywhere. */
int setok_sample_rows(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, const float* u, float temperature, int top_k,
                      float top_p, int64_t* out, float* probs, int64_t ld_probs);

/* setok_sample_rows_each - the same launch (one workgroup per row, the same kernel text) with the three parameters PER ROW: temperature and top_p
 * are (rows) fp32 device arrays, top_k a (rows) int32 device array, and row r is selected under temperature[r], top_k[r], top_p[r].  It is what a
 * batch needs whose rows belong to different requests (ContinuousBatcher.submit(sampler=)): greedy rows sit next to sampled ones.  Every thread of
 * a row's workgroup reads the same three words, so each branch below is workgroup-uniform.  Pure addition: the ABI version stays 9.
 *   - Sampled row: temperature[r] finite and > 0, top_k[r] >= 0, top_p[r] in (0, 1].  out[r] and the `probs` row are, bit for bit, what
 *     setok_sample_rows writes for that row under those three scalars and the same u[r] (rules 1-7 above, bad rows included).
 *   - Greedy row: temperature[r] == 0; top_k[r], top_p[r] and u[r] are ignored.  out[r] is what setok_argmax_rows writes for the row: the lowest
 *     index of the maximum of the logits as they are, a NaN counting as the maximum.  The `probs` row, when given, is one-hot at that index.  This
 *     is NOT top_k = 1, which keeps tied maxima together and draws among them (16-bit logits tie).
 *   - Invalid row: anything else - a NaN, negative or infinite temperature, top_k < 0, top_p outside (0, 1] or NaN.  out[r] = -1 and zeros in the
 *     `probs` row.  The row is classified before any of the three values is used: no address and no loop bound is formed from one.
 * Refused on the host before any launch (-1, setok_last_error): a null logits / u / out / temperature / top_k / top_p, V < 1 or V > 2^20, ld < V,
 * ld_probs < V with probs, a dtype the library does not serve.  rows == 0 launches nothing. */
int setok_sample_rows_each(void* stream, int dtype, const void* logits, int64_t ld, int rows, int V, const float* u, const float* temperature,
                           const int* top_k, const float* top_p, int64_t* out, float* probs, int64_t ld_probs);

/* ---- Speculative decoding (csrc/speculate.hip): draft-and-verify on top of the extend above.  A round feeds K + 1 rows per sequence - the pending
 * token and K drafted ones - through one `extend`, selects a token from every row's logits (setok_argmax_rows or setok_sample_rows) and then keeps
 * the longest prefix of the drafts that the model itself would have produced, plus one more token: what the plain loop emits, in fewer passes
 * over the weights.  Both entries are integer-only, use no atomics, and are pure functions of their inputs.  Pure addition: the ABI stays 9.
 *
 * setok_spec_accept - one launch of one workgroup, a thread per sequence (looping for B above the block size).
 *   draft (B, K) int64, -1 = no proposal (everything behind a sequence's first negative entry counts as negative); sel (B, K + 1) int64: sel[b][i]
 *   is the token selected from the state that consumed the pending token and drafts 0 .. i - 1; eos (n_eos) int64 (NULL with n_eos == 0).
 *   Loop state, updated in place: seq (B, max_new) int64, count (B) int32, finished (B) uint8, pending (B) int64; the cache's key_mask (B, cap)
 *   uint8 and next_pos (B) int64; len0 = the first slot the round's extend filled.  Outputs: emitted (B, K + 1) int64, m_out (B) int32,
 *   summary (3) int32.
 *   For an unfinished sequence b (finished[b] == 0 and 0 <= count[b] < max_new):
 *     n  = the number of leading i < K with draft[b][i] >= 0 && draft[b][i] == sel[b][i];  the candidates are e_i = sel[b][i], i <= n;
 *     m  = min(n + 1, max_new - count[b]);  if some e_i with i < m is an eos id, m = (the first such i) + 1 and the sequence finishes;  it also
 *          finishes when count[b] + m == max_new;
 *     seq[b][count .. count + m) = e_0 .. e_{m-1};  count[b] += m;  emitted[b][i] = e_i for i < m, else -1;  m_out[b] = m;  pending[b] = e_{m-1};
 *     key_mask[b][len0 + i] = 1 for i < m and 0 for m <= i <= K  (slot len0 holds the old pending token, slot len0 + i draft i - 1: the accepted
 *          drafts ARE the emitted tokens e_0 .. e_{m-2}, and e_{m-1} is the new pending token, not yet in the cache);
 *     next_pos[b] = next_pos[b] - (1 + the number of leading non-negative drafts) + m: `extend` advanced it by the rows it attended, so this is its
 *          value before the round plus m.  With K == 0 and no extend before it (the loop's first token) the position is unchanged.
 *   A finished sequence: m = 0, emitted all -1, key_mask[b][len0 .. len0 + K] = 0, nothing else touched.
 *   summary = { max_b m, the number of sequences still unfinished after the round, 1 iff an emitted token is negative }.
 *   Refused on the host before any launch (-1, setok_last_error): a null operand (draft may be NULL with K == 0), B < 0, K outside [0, 63],
 *   max_new < 1, n_eos < 0, len0 + K + 1 > cap.  B == 0 launches nothing.
 *
 * setok_ngram_propose - the built-in drafter's one launch per round; one workgroup of 256 threads per sequence.
 *   hist (B, cap_h) int64 with hist_len (B) int32 valid entries per row, both updated in place; emitted (B, n_emit) int64 and m (B) int32 (NULL
 *   with n_emit == 0: propose only); out (B, K) int64.
 *   1. Append: hist[b][hist_len[b] ..] = emitted[b][0 .. m[b]) and hist_len[b] += m[b]  (m[b] is clamped to [0, n_emit]).  L = the new length.
 *   2. For n = max_ngram down to min_ngram: skip n when L <= n or when any of the last n entries is negative; find the LARGEST j <= L - n - 1 with
 *      hist[b][j .. j + n) == hist[b][L - n .. L)  (the match may overlap the suffix);  at the first n with a match
 *      out[b][i] = hist[b][j + n + i] if j + n + i < L, else -1, and the search ends.  With no match at any n, out[b] is all -1.
 *      A negative history entry (an image placeholder) matches nothing; one inside a continuation is copied and ends the proposal there.
 *   len_max is the caller's host-side bound on max_b (hist_len[b] + m[b]), the lengths themselves being on the device: the call is refused when
 *   len_max > cap_h ("hist_len + m > cap_h"), and the kernel never writes at or behind cap_h whatever the device values say.
 *   Refused as well: a null operand, B < 0, cap_h < 1, K outside [1, 63], n_emit outside [0, 64], 1 <= min_ngram <= max_ngram <= 8 violated.
 *   Threads test strided j and keep their largest match; the largest of all meets by a wave max and an LDS max over the waves; one wave writes the
 *   continuation. */
int setok_spec_accept(void* stream, const int64_t* draft, const int64_t* sel, int B, int K, const int64_t* eos, int n_eos, int max_new,
                      int64_t* seq, int32_t* count, uint8_t* finished, int64_t* pending, uint8_t* key_mask, int64_t* next_pos, int cap, int len0,
                      int64_t* emitted, int32_t* m_out, int32_t* summary);
int setok_ngram_propose(void* stream, int64_t* hist, int32_t* hist_len, int B, int cap_h, int len_max, const int64_t* emitted, const int32_t* m,
                        int n_emit, int K, int max_ngram, int min_ngram, int64_t* out);

/* ---- Beam search (csrc/beam.hip): HuggingFace's `GenerationMixin._beam_search` with do_sample=False and no logits processors, over B sequences of
 * n = num_beams running beams each (flat row b * n + i), the cache and the decode step running on B * n rows.  Pure addition: the ABI stays 9.
 *
 * The rule, per step `step` = 0, 1, .. (the step selects new token number step + 1), with C = max(2, 1 + n_eos) * n:
 *   1. the logits are taken as fp32, acc[j][v] = running[b][j] + log_softmax(row j)[v] in fp32, and the C largest acc of the sequence's n_in * V
 *      candidates are kept in descending order (setok_beam_topk).  Step 0 has n_in = 1: the prefill ran on B rows, the one row's running score is
 *      0 - HF replicates the prompt n times and starts beams 1 .. n - 1 at -1e9, which selects the same candidates as long as V >= C.
 *   2. candidate c "hits" when its token is an eos id or step + 1 == max_new.
 *   3. the next running beams are the n best candidates by acc + hit * -1e9; running beam i gets that score, the candidate's token, and the
 *      candidate's beam as its parent.
 *   4. the finished set holds n entries (score, finished?), initially (-1e9, no).  A candidate's entry score is
 *        acc / (step + 1) ** length_penalty  + (-1e9 if the set is full - all n finished - and early_stopping is True)
 *                                            + (-1e9 if the sequence's heuristic flag is already down)  + (-1e9 unless it hits and c < n),
 *      one fp32 addition each; its finished? bit is (hits and c < n).  The n best of (old entries, then candidates) form the new set.
 *   5. the heuristic flag (initially up) stays up while  running[0] / L ** length_penalty  >  (-1e9 for an entry that is not finished, the set's
 *      minimum score for one that is)  holds for some entry, with L = max_new when early_stopping is "never" and length_penalty > 0, else step + 1.
 *   6. the loop continues while some sequence's flag is up, and not (every entry of every sequence is finished and early_stopping is True), and
 *      not every candidate of every sequence hit.
 *   `x ** length_penalty` is Python's `int ** float`: a double power of the double length_penalty, rounded once to fp32 where the fp32 tensor is divided by it.  Every selection
 *   is by (value descending, index ascending), a total order; the fixtures keep every ordering the result depends on 1e-3 apart.
 *   At the end the entries of each sequence's finished set are its hypotheses in descending score.  A hypothesis is kept as back-pointers: per
 *   step the token and the parent of every running beam; a finished entry is (score, length, parent, last token).
 *
 * setok_beam_topk - step 1 of the rule.  logits: B * n_in rows of V columns, row stride ld elements, dtype = the build's 16-bit type or fp32; running
 *   (B, n_in) fp32.  Outputs cand_score (B, C) fp32, cand_token (B, C) int64, cand_beam (B, C) int32 (the j of the row), descending, ties to the lower
 *   flat index j * V + v; status (B) int32 = 1 iff a row of the sequence holds a NaN or +inf or no finite entry (such a row contributes no candidate;
 *   the other sequences are not affected), else 0.  -inf entries are legal and lose against every finite one.  ws: B * n_in * 516 bytes.
 *   Two launches: one workgroup of 1024 threads per row finds the row's maximum, sums exp(x - max) - every thread over the elements
 *   [(k * 1024 + t) * VEC, + VEC) in order of k, then the wave butterfly, then the 16 waves in order: the order depends on V alone - and keeps the row's
 *   best 64 acc (every wave a sorted list, one entry per lane; an entry's rank among the 16 lists is its place in its own plus a binary search in each other one); one workgroup per sequence then merges its n_in lists the same way.  No
 *   atomics; a sequence's result is the same bits alone and inside any batch.  Refused: a null operand, B < 0, n_in outside [1, 16], V outside
 *   [1, 2^20], ld < V, C outside [1, 64] or > n_in * V ("bad C"), another dtype, a workspace that is too small.
 *
 * setok_beam_advance - steps 2 to 6, one launch of one workgroup, one wave per sequence (looping above 16).  eos (n_eos) int64 (NULL with n_eos == 0);
 *   topk_status (B) int32 is setok_beam_topk's.  early_stopping: 0 False, 1 True, 2 "never".  State, updated in place: run_score (B, n) fp32;
 *   fin_score (B, n) fp32, fin_flag (B, n) uint8, fin_len (B, n) int32 (new tokens), fin_parent (B, n) int32 (the running beam of the step before
 *   that the entry's last token was selected from) and fin_token (B, n) int64; heur (B) uint8.  The caller initialises fin_score to -1e9, heur to 1 and
 *   everything else to 0.  bp_token (max_new, B * n) int64 and bp_parent (max_new, B * n) int32 receive row `step`.  Outputs next_token (B * n) int64,
 *   src_row (B * n) int32 = b * n + parent (what setok_kv_reorder takes), summary (2) int32 = { 1 iff the loop continues, 1 iff a status is set }.
 *   Refused: a null operand, B < 0, n outside [1, 16], C outside [n, 64] ("bad C"), n_eos < 0, step outside [0, max_new), a non-finite
 *   length_penalty, early_stopping outside {0, 1, 2}.
 *
 * setok_kv_reorder - for each of n_tensors cache tensors (rows, Hkv, cap, row_bytes[t] bytes), slots [slot0, slot1) of row r become what row
 *   src_row[r] held before the call.  ptrs (n_tensors) device pointers, row_bytes (n_tensors) int32 and scratch_unit (n_tensors) int64 - the sum of
 *   row_bytes rounded up to 16 over the tensors before t - are DEVICE tables built once per cache; unit_total is that sum over all tensors.  Two
 *   launches whatever the number of tensors: every (tensor, row, head) gathers its source's ns = slot1 - slot0 slots into the scratch
 *   (unit_total * rows * Hkv * ns bytes, 16-byte aligned), then copies them back, so any mapping inside a group is safe, several rows taking one
 *   parent included.  A row with src_row[r] == r moves nothing.  A src_row[r] outside r's own group [r / n * n, r / n * n + n) counts as r and sets
 *   status[r] = 1 (status (rows) int32 is otherwise left as it is: the caller zeroes it once).  Refused: a null operand, n_tensors outside
 *   [1, 65535], rows % n != 0, slots outside [0, cap], a scratch that is too small or misaligned. */
int setok_beam_topk(void* stream, int dtype, const void* logits, int64_t ld, int B, int n_in, int V, const float* running, int C,
                    float* cand_score, int64_t* cand_token, int32_t* cand_beam, int32_t* status, void* ws, int64_t ws_bytes);
int setok_beam_advance(void* stream, const float* cand_score, const int64_t* cand_token, const int32_t* cand_beam, const int32_t* topk_status,
                       int B, int n, int C, const int64_t* eos, int n_eos, int step, int max_new, double length_penalty, int early_stopping,
                       float* run_score, float* fin_score, uint8_t* fin_flag, int32_t* fin_len, int32_t* fin_parent, int64_t* fin_token,
                       uint8_t* heur, int64_t* bp_token, int32_t* bp_parent, int64_t* next_token, int32_t* src_row, int32_t* summary);
int setok_kv_reorder(void* stream, const void* const* ptrs, const int32_t* row_bytes, const int64_t* scratch_unit, int n_tensors,
                     int64_t unit_total, int rows, int n, int Hkv, int cap, int slot0, int slot1, const int32_t* src_row, void* scratch,
                     int64_t scratch_bytes, int32_t* status);

/* ---- Logits processors (csrc/logits.hip): HuggingFace's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
 * MinNewTokensLengthLogitsProcessor and SuppressTokensLogitsProcessor, in the order of `GenerationMixin._get_logits_processor`, applied to a
 * step's logits BEFORE a token is selected (setok_argmax_rows) and before the warpers that setok_sample_rows implements.  Pure addition: the ABI
 * version stays 9.
 *
 * A sequence b has a history hist[b][0 .. hist_len[b]) (hist (B, cap_h) int64, hist_len (B) int32) and a prompt_len[b] (int32).  The call works on
 * B * n rows; row (b, i) = b * n + i sees the virtual history
 *     Hs = hist[b][0 .. hist_len[b])  followed by  tail[b][0 .. i)        (tail (B, n - 1) int64, NULL with n == 1),   L = hist_len[b] + i.
 * n = 1 is the plain loop; n = K + 1 is a verify round of draft-and-verify whose tail holds the K drafts.
 * With x_v = float(logit_v) in fp32 (HF casts the step's logits to fp32 before its processors), for v in [0, V):
 *   1. out[v] = x_v.
 *   2. Penalty (penalty != 1): if v occurs in Hs, out[v] = x_v < 0 ? x_v * penalty : x_v / penalty - both in fp32, `penalty` rounded to fp32
 *      once, a true division (no reciprocal multiply); once, however often v occurs.
 *   3. N-gram ban (ngram = g >= 1 and L + 1 >= g): for every j in [0, L - g] with Hs[j .. j + g - 1) == Hs[L - g + 1 .. L) (g - 1 tokens;
 *      with g = 1 every occurring token), out[Hs[j + g - 1]] = -inf.  A window whose compared tokens or banned token include an id outside
 *      [0, V) bans nothing.
 *   4. Minimum length (min_new > 0 and L - prompt_len[b] < min_new): out[e] = -inf for every eos id e in [0, V).
 *   5. Suppression: out[s] = -inf for every suppressed id s in [0, V).
 * A ban wins over the penalty.  Ids outside [0, V) - image placeholders, everything behind a negative draft - match nothing and are never
 * dereferenced.  NaN and +-inf logits go through the arithmetic as IEEE gives them; what the selection kernels do with a bad row does not
 * change.  Slots at or behind hist_len[b] (a hist_len outside [0, cap_h] is clamped into it), logits columns >= V and out columns >= V are
 * never read or written.
 *
 * setok_logits_process - one workgroup of 256 threads per row.  logits: (B * n, V) in `dtype`, row stride ld >= V elements, any alignment (V =
 *   32003 included); out: (B * n, V) fp32, row stride ld_out >= V, must not overlap logits.  16-byte loads from the first 16-byte boundary of a row
 *   on, 16-byte stores where the out row then sits on one.  Threads stride over the history windows as in setok_ngram_propose.  No atomics.
 *   Up to three writers can aim at one column and several history positions can hold one token; the stored bits do not depend on timing:
 *   the copy, the penalty and the bans are three phases separated by workgroup barriers (a barrier orders the workgroup's global stores), every
 *   penalty value is computed from the untouched INPUT (duplicates store identical bits), and every ban stores the same -inf.
 *   eos (n_eos) and suppress (n_suppress) int64, NULL with a count of 0.
 *   Refused on the host before any launch (-1, setok_last_error): a null operand, B < 0, n outside [1, 64], V outside [1, 2^20], ld < V,
 *   ld_out < V, cap_h < 1, a null tail with n > 1, ngram outside [0, 8], min_new < 0, n_eos or n_suppress outside [0, 64], a penalty that is
 *   not finite or <= 0, an out that overlaps logits, a dtype the library does not serve.  B == 0 launches nothing.
 *
 * setok_history_append - one workgroup of 64 threads per sequence: hist[b][hist_len[b] ..] = emitted[b][0 .. m[b]) (emitted (B, n_emit) int64;
 *   m (B) int32 clamped to [0, n_emit], NULL = every row appends n_emit entries), then hist_len[b] += m[b].  A launch of its own: the rows of one
 *   sequence run in different workgroups of the process kernel, all of which read the history.  len_max is the caller's host-side bound on
 *   max_b (hist_len[b] + m[b]): the call is refused when len_max > cap_h ("hist_len + m > cap_h"), and the kernel never writes at or behind cap_h
 *   whatever the device values say.  Refused as well: a null operand, B < 0, cap_h < 1, n_emit outside [0, 64].  B == 0 or n_emit == 0 launches
 *   nothing. */
int setok_logits_process(void* stream, int dtype, const void* logits, int64_t ld, int B, int n, int V, const int64_t* hist, const int32_t* hist_len,
                         const int32_t* prompt_len, int cap_h, const int64_t* tail, float penalty, int ngram, int min_new, const int64_t* eos,
                         int n_eos, const int64_t* suppress, int n_suppress, float* out, int64_t ld_out);
int setok_history_append(void* stream, int64_t* hist, int32_t* hist_len, int B, int cap_h, int len_max, const int64_t* emitted, const int32_t* m,
                         int n_emit);

/* ---- FP8 weight-only decode (csrc/gemm_fp8w.hip; the M <= 64 GEMM it shares with MXFP4: csrc/wstream.h): the decode step streams every projection weight once per token, so the stack's Linear
 * weights may be STORED as OCP e4m3fn bytes with one power-of-two scale per output row.  A matrix W (N, K) becomes q (N, K) uint8 + e (N,) int8 and
 * means exactly
 *     W'[n, k] = value_e4m3fn(q[n, k]) * 2^e[n],      e[n] in [-15, 7].
 * Because the scale is a power of two inside that range, W' is exactly representable in bf16, in fp16 (2^-9 * 2^-15 is its smallest subnormal,
 * 448 * 2^7 < 65504) and in fp32: a quantised model is an ordinary model whose weights lie on a grid, and setok_linear on the dequantised W'
 * computes the same function.  Pure additions: the ABI version stays 9. */

/* The quantiser, per row n:  amax = max_k |W[n, k]| over the finite entries;  e[n] = the smallest integer with amax <= 448 * 2^e, clamped to
 * [-15, 7], and 0 for a row without a non-zero finite entry (exponent arithmetic, no log2);  q[n, k] = round-to-nearest-even_e4m3fn(W[n, k] * 2^-e[n]),
 * subnormals included, saturating at +-448 (reachable only where the clamp at 7 binds);  a non-finite W[n, k] becomes the NaN code 0x7f.
 * W: (N, K) in `dtype`, row stride ldw >= K elements;  q: row stride ldq >= K bytes;  any alignment, any K >= 1.  One workgroup per row, two
 * passes over the row, no atomics. */
int setok_quantize_fp8_rows(void* stream, int dtype, const void* W, int64_t ldw, uint8_t* q, int64_t ldq, int8_t* e, int N, int K);

/* The exact inverse: W[n, k] = value(q[n, k]) * 2^e[n] in `dtype` — no rounding happens, by the contract above.  Same strides. */
int setok_dequantize_fp8_rows(void* stream, int dtype, const uint8_t* q, int64_t ldq, const int8_t* e, void* W, int64_t ldw, int N, int K);

/* C[M, N] = A[M, K] · W'^T + residual[M, N]   (residual optional; C may alias it) for 1 <= M <= 64: the weight-streaming GEMM of a decode step.
 * A, residual and C have element type `dtype`; products of the exact element-type values of A and value(q), fp32 accumulation, the scale 2^e[n]
 * applied once in fp32, one rounding to `dtype`.  K % 64 == 0 (16-bit) or K % 16 == 0 (fp32), any N >= 1.
 * Strides as in setok_linear: lda >= K (A's row stride in elements, a multiple of 8 / 4: 16-byte pieces, A 16-byte aligned), ldc >= N (C AND
 * residual, any value), ldq >= K (q's row stride in bytes, a multiple of 16, q 16-byte aligned).  Anything else — M > 64 included: dequantise
 * and call setok_linear — is SETOK_EINVAL with a message naming the argument, before any launch.
 * No element outside A's [0, M) x [0, K) or q's [0, N) x [0, K) is read and none outside C's [0, M) x [0, N) is written, at any stride.
 * A row's bits depend on that row of A (and of residual), q and e alone — not on M, the strides or the rows around it: there is one summation
 * order, fixed by K.  It is NOT setok_linear's order: bit equality with setok_linear on the dequantised W' is not promised, only the same
 * function within fp32 accumulation error.  No atomics, no hand-off between workgroups.
 * SETOK_F32 is the parity mode and a DIFFERENT algorithm from the 16-bit MFMA path: plain fp32 arithmetic that carries its rounding errors
 * (error-free products and sums), so each output is the fp32 value next to the exact dot product — better than an fp32-accumulated chain.
 * Its agreement with fp64 says the layout, the scales and the bounds are right; it is no evidence for the accumulation of the 16-bit path. */
int setok_linear_fp8w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                      const void* residual, void* C, int64_t ldc, int M, int N, int K);

/* setok_linear_fp8w with the floor of its band rule as an argument.  A workgroup of the 16-bit path owns 16, 32 or 64 output columns — the widest
 * band (64 from three row tiles of 16 rows, 32 at two, 16 at one) that still leaves ceil(N / band) >= min_wgs workgroups; setok_linear_fp8w
 * passes 256, the CU count of an MI355X.  min_wgs >= 1: 1 always takes the widest band, a value above N / 32 always the narrowest.  The band
 * decides which workgroup computes a column and never a bit of C: this entry exists for parts with fewer active CUs, and so that the tests can
 * hold every band to that at small N.  SETOK_F32 ignores it. */
int setok_linear_fp8w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const int8_t* e,
                          const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs);

/* ---- MXFP4 weight-only decode (csrc/gemm_mxfp4w.hip; the M <= 64 GEMM it shares with fp8: csrc/wstream.h): the same idea at half the bytes again, in the OCP Microscaling format gfx950 converts in
 * hardware.  A matrix W (N, K), K % 32 == 0, is stored in two arrays:
 *     q (N, K/2) uint8     byte j of a row holds element 2j in its low nibble and element 2j+1 in its high nibble (torch's float4_e2m1fn_x2 order)
 *     s (N, K/32) uint8    e8m0 scale bytes, plain row-major: block b of a row covers k in [32 b, 32 b + 32)
 * and means exactly
 *     W'[n, k] = value_e2m1(nibble[n, k]) * 2^(s[n, k / 32] - 127);     a block whose scale byte is 0xFF is 32 NaNs.
 * A nibble's bit 3 is the sign; magnitude codes 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6.  The quantiser emits scale bytes in [114, 140] (and 0xFF), so
 * that 0.5 * 2^e and 6 * 2^e are normal numbers in fp16 as well: W' is exactly representable in bf16, fp16 and fp32, a quantised model is an ordinary
 * model whose weights lie on a grid, and setok_linear on the dequantised W' computes the same function.
 * Scale bytes the quantiser never emits are still accepted by the dequantiser and the GEMM: the byte is the exponent field of the hardware
 * converter's fp32 scale operand, the value is value_e2m1 * 2^(s - 127) formed in fp32 and rounded once to the element type (exact in fp32 and bf16
 * wherever the product is a normal number there; fp16 overflows and underflows as its range dictates).
 * Pure additions: the ABI version stays 9. */

/* The quantiser, per block of 32 elements of a row:  any non-finite entry -> scale byte 0xFF and nibbles 0 (a non-finite weight stays visible);
 * otherwise amax = max |W|;  a block of zeros gets scale byte 127;  any other block e = floor(log2(amax)) - 2 (the OCP MX v1.0 rule, by exponent
 * arithmetic, no log2), clamped to [-13, 13], scale byte e + 127;  nibble = round-to-nearest(W * 2^-e) saturating at +-6 (reachable where amax is
 * in (6, 8) * 2^e or the clamp at 13 binds), ties to the even code: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4;  the sign bit
 * is W's own sign bit, so -0.0 and a negative that rounds to zero store 0x8.
 * W: (N, K) in `dtype`, row stride ldw >= K elements;  q: row stride ldq >= K/2 bytes;  s: row stride lds >= K/32 bytes;  any alignment.  Each of
 * W, q, s may be a window of a wider buffer; nothing outside them is written.  One thread per block, no atomics. */
int setok_quantize_mxfp4_rows(void* stream, int dtype, const void* W, int64_t ldw, uint8_t* q, int64_t ldq, uint8_t* s, int64_t lds, int N, int K);

/* The exact inverse: W[n, k] = W'[n, k] in `dtype`.  Same strides.  Rows of q in 4-byte pieces and rows of W in 16-byte pieces take a packed path
 * (8 elements per lane), anything else a byte-wise one; both give the same bits. */
int setok_dequantize_mxfp4_rows(void* stream, int dtype, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds, void* W, int64_t ldw, int N, int K);

/* C[M, N] = A[M, K] · W'^T + residual[M, N]   (residual optional; C may alias it) for 1 <= M <= 64: the weight-streaming GEMM of a decode step on
 * the nibbles.  A, residual and C have element type `dtype`; products of the exact element-type values of A and W' (the block scale is applied
 * when the block is converted, by the hardware converter), fp32 accumulation, one rounding to `dtype`.  K % 128 == 0 (16-bit) or K % 32 == 0
 * (fp32), any N >= 1.
 * Strides: lda >= K (elements, a multiple of 8 / 4: 16-byte pieces, A 16-byte aligned), ldc >= N (C AND residual, any value), ldq >= K/2 (bytes, a
 * multiple of 16, q 16-byte aligned: a lane's 16-byte load is one block), lds >= K/32 (bytes, any value).  Anything else — M > 64 included:
 * dequantise and call setok_linear — is SETOK_EINVAL with a message naming the argument, before any launch.
 * No element outside A's [0, M) x [0, K), q's [0, N) x [0, K/2) or s's [0, N) x [0, K/32) is read and none outside C's [0, M) x [0, N) is written.
 * A row's bits depend on that row of A (and of residual), q and s alone — not on M, the strides, the band or the rows around it: there is one
 * summation order, fixed by K.  It is NOT setok_linear's order.  No atomics, no hand-off between workgroups.
 * SETOK_F32 is the parity mode, as in setok_linear_fp8w: compensated fp32 arithmetic, a different algorithm from the 16-bit MFMA path. */
int setok_linear_mxfp4w(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                        const void* residual, void* C, int64_t ldc, int M, int N, int K);

/* setok_linear_mxfp4w with the floor of its band rule as an argument (setok_linear_fp8w_wgs's rule: the widest band of 64 / 32 / 16 columns — 64 from
 * three row tiles, 32 at two, 16 at one — that leaves ceil(N / band) >= min_wgs workgroups; setok_linear_mxfp4w passes 256).  The band decides
 * which workgroup computes a column and never a bit of C.  SETOK_F32 ignores it. */
int setok_linear_mxfp4w_wgs(void* stream, int dtype, const void* A, int64_t lda, const uint8_t* q, int64_t ldq, const uint8_t* s, int64_t lds,
                            const void* residual, void* C, int64_t ldc, int M, int N, int K, int min_wgs);

/* ---- FP8 KV cache (csrc/attn_decode.hip): the decode attention is bound by the K / V bytes it reads, so the cache may be STORED by the rule
 * above, one cache row — the Dh post-rotary elements of one (sequence, key / value head, slot), of K or of V — taking the place of a weight row:
 * Dh e4m3fn bytes and one int8 exponent, meaning exactly value(q[d]) * 2^e with e in [-15, 7]; amax over the finite entries, e the smallest
 * exponent with amax <= 448 * 2^e (0 for a row of zeros), round-to-nearest-even including the subnormals, saturation at +-448, the NaN code for
 * a non-finite entry.  Per layer: k_q, v_q (B, Hkv, cap, Dh) uint8 and k_e, v_e (B, Hkv, cap) int8.  The stored K', V' are exactly
 * representable in fp32, bf16 and fp16, so an attention over the fp8 cache is an ordinary attention over K', V'.  Only the cache is
 * quantised: the prefill attends over its own unquantised q | k | v.  Pure additions: the ABI version stays 9. */

/* Keys of one chunk of the decode attention over the fp8 cache (what SETOK_DECODE_CHUNK is to setok_attention_decode_gqa): a wave streams 64
 * rows of 16-byte pieces, which keeps as many bytes in flight per wave as the 16-bit kernel has with 32 rows. */
#define SETOK_DECODE_CHUNK_FP8KV 256

/* setok_kv_append with the quantiser: the post-rotary k and v columns of B*T rows of a fused [q: H | k: Hkv | v: Hkv] buffer in `dtype` are
 * quantised row by row (the rule above) into slots [pos0, pos0 + T) of k_q / k_e and v_q / v_e.  One pass, a row in the registers of the
 * lanes that hold it; no atomics; no byte outside those slots is written.  Dh % 8 == 0 and Dh <= 512; qkv, k_q and v_q 16-byte aligned. */
int setok_kv_append_fp8(void* stream, int dtype, const void* qkv, uint8_t* k_q, int8_t* k_e, uint8_t* v_q, int8_t* v_e, int B, int T, int H,
                        int Hkv, int Dh, int cap, int pos0);

/* setok_attention_decode_gqa over the fp8 cache: q and out in `dtype`, the keys / values K', V' as stored.  Everything that call states holds
 * here — which keys count, zeros for a sequence without one, fp32 softmax, the probabilities rounded to the 16-bit element type before they
 * multiply V, one read of each cache byte per group of query heads, chunk partials merged in chunk order by a second launch, output bits that
 * depend on the sequence's own operands and `len` alone — with SETOK_DECODE_CHUNK_FP8KV in the place of SETOK_DECODE_CHUNK:
 * ws_floats >= B * H * ceil(len / SETOK_DECODE_CHUNK_FP8KV) * (Dh + 2).  2^e of a K row multiplies the finished dot product, 2^e of a V row the
 * rounded probability (both exact).  A slot that does not count (>= len, or masked) may hold ANY code and ANY exponent byte, values outside
 * [-15, 7] included: it is discarded by selection and no scale is ever built from its exponent.  Dh % 8 == 0; Dh in {16, 32, 64, 128} take the
 * lane-layout kernel, the others a generic one.  q, k_q and v_q 16-byte aligned. */
int setok_attention_decode_gqa_fp8kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const int8_t* k_e,
                                     const uint8_t* v_q, const int8_t* v_e, const uint8_t* key_mask, void* out, int B, int H, int Hkv, int Dh,
                                     int cap, int len, float scale, float* ws, int64_t ws_floats);

/* ---- MXFP4 KV cache (csrc/attn_decode.hip, csrc/attn_extend.hip): the cache STORED by the rule of "MXFP4 weight-only decode", one cache row —
 * the Dh post-rotary elements of one (sequence, key / value head, slot), of K or of V — taking the place of a weight row.  Per layer:
 *     k_q, v_q (B, Hkv, cap, Dh/2) uint8     element 2j of a row in the low nibble of byte j, element 2j+1 in the high one
 *     k_s, v_s (B, Hkv, cap, Dh/32) uint8    e8m0 scale bytes, one per 32 elements of a row
 * meaning exactly value_e2m1(nibble[d]) * 2^(s[d / 32] - 127).  The quantiser is setok_quantize_mxfp4_rows' rule per block of 32: a non-finite
 * entry -> scale byte 0xFF and nibbles 0; a block of zeros -> scale byte 127; otherwise e = floor(log2 amax) - 2 clamped to [-13, 13], nibbles
 * rounded to nearest with ties to the even code, saturating at +-6, the sign bit the value's own.  The stored K', V' are exactly representable in
 * fp32, bf16 and fp16, so an attention over the cache is an ordinary attention over K', V'.  Dh % 32 == 0 is required by every entry point
 * below; the cache takes 2 * layers * B * Hkv * cap * (Dh/2 + Dh/32) bytes (a row at Dh = 128: 68 bytes; an fp8 row 129, a bf16 row 256).
 * A slot that does not count (masked, or at / past `len`) may hold ANY nibbles and ANY scale byte, 0xFF included: it is discarded by selection.
 * A slot that counts and holds a 0xFF block gives NaN, as a NaN in a native cache would.  Only the cache is quantised: an unchunked prefill
 * attends over its own unquantised q | k | v, an extend (a window of a chunked prefill, a turn, a verify pass) over the stored slots.
 * Unlike the fp8 cache this format can be extended by several tokens.  Pure additions: the ABI version stays 9. */

/* Keys of one chunk of the decode attention over the MXFP4 cache.  A lane holds 16 elements of a row (8 nibble bytes and the scale byte it shares
 * with its neighbour), so at Dh = 128 a row is spread over 8 lanes as in the fp8 kernel and a wave streams 64 rows per chunk in 8 + 8 loads.
 * fp8's bytes-in-flight argument would ask for 512 (8-byte pieces: twice the rows for the same bytes), but the kernel keeps one fp32 score per
 * (load step, query head of the group) in registers until the wave's maximum is known, and at 8 query heads 16 steps of them do not fit next to
 * the group's q and accumulators without scratch.  256 keeps the fp8 kernel's register budget and its partition of a sequence's keys; the
 * constant depends on the format alone, so every summation order depends on `len` alone. */
#define SETOK_DECODE_CHUNK_MXFP4KV 256

/* setok_kv_append with the MXFP4 quantiser: the post-rotary k and v columns of B*T rows of a fused [q: H | k: Hkv | v: Hkv] buffer in `dtype`
 * are quantised block by block (the rule above) into slots [pos0, pos0 + T) of k_q / k_s and v_q / v_s; T >= 1 rows per sequence (a prefill
 * appends the whole prompt), T == 0 does nothing.  One pass, a row in the registers of the lanes that hold it (a block of 32 is four lanes); no
 * LDS, no atomics; no byte outside those slots is written.  Dh % 32 == 0 and Dh <= 512; qkv, k_q and v_q 16-byte aligned. */
int setok_kv_append_mxfp4(void* stream, int dtype, const void* qkv, uint8_t* k_q, uint8_t* k_s, uint8_t* v_q, uint8_t* v_s, int B, int T, int H,
                          int Hkv, int Dh, int cap, int pos0);

/* setok_attention_decode_gqa over the MXFP4 cache: q and out in `dtype`, the keys / values K', V' as stored.  Everything that call states holds
 * here — which keys count, zeros for a sequence without one, fp32 scores and softmax, the probabilities rounded to the 16-bit element type
 * before they multiply V, one read of each cache byte per group of query heads, chunk partials merged in chunk order by a second launch, output
 * bits that depend on the sequence's own operands and `len` alone — with SETOK_DECODE_CHUNK_MXFP4KV in the place of SETOK_DECODE_CHUNK:
 * ws_floats >= B * H * ceil(len / SETOK_DECODE_CHUNK_MXFP4KV) * (Dh + 2).  The block scale is applied by the hardware converter when a lane's
 * piece is decoded, so the decoded floats are exactly K', V' and the arithmetic from there on is the native kernel's.  Dh % 32 == 0; Dh in
 * {32, 64, 128} take the lane-layout kernel, the others (96, ...) a generic one.  q, k_q and v_q 16-byte aligned. */
int setok_attention_decode_gqa_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                       const uint8_t* v_q, const uint8_t* v_s, const uint8_t* key_mask, void* out, int B, int H, int Hkv, int Dh,
                                       int cap, int len, float scale, float* ws, int64_t ws_floats);

/* Floats of workspace setok_attention_extend_gqa_mxfp4kv needs: B * Tn * H * ceil((len0 + Tn) / SETOK_EXTEND_CHUNK) * (Dh + 2), whatever the
 * element type and head dim: one partial per chunk.  The MFMA path (below) partitions as setok_attention_extend_gqa does — a partial per span of
 * up to SETOK_EXTEND_SPAN chunks — and uses a prefix of these floats; the rule does not follow it.  0 for arguments the call would refuse. */
int64_t setok_attention_extend_mxfp4kv_workspace(int B, int Tn, int H, int Dh, int len0);

/* setok_attention_extend_gqa over the MXFP4 cache: Tn >= 1 query rows per (sequence, query head) against slots [0, len0 + Tn), which already
 * hold the new rows' quantised keys / values; query i of sequence b counts slot j iff j <= len0 + i and key_mask[b][j] != 0, a query without a
 * counted key gets zeros.  That call's semantics and refusals, with Dh % 32 == 0, and that call's dispatch:
 *   - the 16-bit type at Dh == 128: the MFMA kernel of setok_attention_extend_gqa — its partition into tiles, chunks and spans, its online
 *     softmax, its merge — whose 32-key tiles are converted from nibbles on their way to LDS (v_cvt_scalef32_pk_{bf16,f16}_fp4, the scale
 *     applied).  THE OUTPUT BITS ARE THOSE OF setok_attention_extend_gqa on the same q, key_mask, len0 and Tn over caches that hold K', V',
 *     provided K', V' are representable in the element type.  Every row setok_kv_append_mxfp4 writes is (block exponents in [-13, 13]: exact in
 *     bf16 and fp16); a hand-made scale byte outside that range is the caller's business here — the converter rounds or overflows as the type
 *     does — while the path below computes such a block in fp32.  Also needs Hkv * ceil((H / Hkv) * Tn / 128) <= 65535 (the launch grid);
 *   - everything else (fp32, the other head dims): one wave per (query row, query head, chunk of SETOK_EXTEND_CHUNK slots), a key per lane, then
 *     the shared merge in chunk order — a functional path that reads the cache once per query row and query head and uses no MFMA, as the native
 *     call's is for these shapes.
 * A slot that counts for no query may hold any nibbles and any scale byte (0xFF, the NaN block, included).  DESIGN.md §7 f16 has the
 * measurements.  q, k_q and v_q 16-byte aligned. */
int setok_attention_extend_gqa_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                       const uint8_t* v_q, const uint8_t* v_s, const uint8_t* key_mask, void* out, int B, int Tn, int H, int Hkv,
                                       int Dh, int cap, int len0, float scale, float* workspace, int64_t workspace_floats);

/* ---- Paged KV cache (csrc/attn_paged.hip): the native-format cache without a capacity per sequence.  One layer's keys / values live in two
 * pools, k_pool and v_pool (num_pages, Hkv, SETOK_KV_PAGE, Dh) in `dtype` - the rows of one (page, key / value head) are contiguous, as the rows
 * of one (sequence, key / value head) are in the dense cache.  A sequence is row b of block_table, (B, max_pages) int32 on the device - entry p
 * is the page that holds its slots [SETOK_KV_PAGE * p, SETOK_KV_PAGE * (p + 1)) - and an int32 length on the device: sequences of one batch
 * have lengths of their own, a compact sequence has no dead slots (there is no key_mask), and pages go back to a pool when a sequence ends.
 * A page id outside [0, num_pages) means "no page" to both entries: nothing is written to it, no key of it counts, and no address is formed from
 * it - a bad table is defined behaviour, never a fault.  These two entries take pools in the element type; MXFP4 pools have entries of their own
 * ("Paged MXFP4 KV cache" below); the extend attention over pages is the next section.  Pure additions: the ABI version stays 9. */

/* Slots per page.  Equal to SETOK_DECODE_CHUNK (a static_assert in csrc/attn_paged.hip): a chunk's workgroup reads exactly one page, so where a
 * page lies cannot change a bit of the output. */
#define SETOK_KV_PAGE 128

/* setok_kv_append through a block table: the post-rotary k and v columns of rows b * T + t of a fused [q: H | k: Hkv | v: Hkv] buffer go to slot
 * slot0[b] + t of sequence b - page block_table[b][slot / SETOK_KV_PAGE], row slot % SETOK_KV_PAGE of that page.  slot0: (B,) int32 on the
 * device; a sequence with slot0[b] < 0 is skipped entirely (an idle row of a running batch).  One call serves a prefill (T rows from slot 0; T may
 * cross page boundaries) and a decode step (T = 1).  Nothing is written for a slot past the table's max_pages entries or whose table entry is no
 * page; no other byte of the pools is written.  16-byte accesses (qkv and the pools 16-byte aligned); Dh as for the attention below. */
int setok_kv_append_paged(void* stream, int dtype, const void* qkv, void* k_pool, void* v_pool, const int32_t* block_table, int max_pages,
                          int num_pages, const int32_t* slot0, int B, int T, int H, int Hkv, int Dh);

/* setok_attention_decode_gqa over the pools: query row b of q (row stride ldq elements, H heads of Dh) against slots [0, lens[b]) of sequence b,
 * found through its row of the table.  lens: (B,) int32 on the device; slot j counts iff j < lens[b]; lens[b] == 0 gives zeros (the convention for
 * a sequence without a key).  max_len is the host's upper bound on lens (lens[b] <= max_len <= max_pages * SETOK_KV_PAGE): the grid's chunk
 * dimension and the workspace come from it, ws_floats >= B * H * ceil(max_len / SETOK_KV_PAGE) * (Dh + 2).  A chunk at or past a sequence's own
 * length writes the empty partial without loading from the pools or reading the table entry; the merge takes each sequence's chunk count from
 * lens[b].  Sequence b's output bits are those of setok_attention_decode_gqa at B = 1 on its slots gathered into a dense cache, with an
 * all-ones mask and len = lens[b]: the same arithmetic in the same order, so they depend on its own q, keys, values and length alone - not on the
 * table, the pool, B, max_len or the run.  Slots at or past lens[b] and pages no sequence owns may hold anything, NaN included.
 * Dh / (elements per 16 bytes) in {2, 4, 8, 16, 32} - Dh 16 ... 256 in the 16-bit type, 8 ... 128 in fp32 -; any other head dim is refused (the
 * generic wave-per-chunk kernel has no paged twin).  q and the pools 16-byte aligned, ldq % 8 == 0. */
int setok_attention_decode_gqa_paged(void* stream, int dtype, const void* q, int64_t ldq, const void* k_pool, const void* v_pool,
                                     const int32_t* block_table, int max_pages, int num_pages, const int32_t* lens, void* out, int B, int H, int Hkv,
                                     int Dh, int max_len, float scale, float* ws, int64_t ws_floats);

/* ---- Paged extend attention (csrc/attn_extend_paged.hip): setok_attention_extend_gqa over the pools of the paged KV cache above - Tn >= 1 query
 * rows per sequence against pages that are already filled.  What lets requests share a prompt prefix (whole pages, counted by reference on the host;
 * a request runs only its remainder), and what a verify pass or a prefill window over pages will call.  Pure additions: the ABI version stays 9. */

/* Floats of workspace setok_attention_extend_gqa_paged needs: setok_attention_extend_workspace's rule at len0 = max_len0 (the same partition into
 * partials, sized for the longest sequence of the call). */
int64_t setok_attention_extend_paged_workspace(int dtype, int B, int Tn, int H, int Hkv, int Dh, int max_len0);

/* Query row b * Tn + i of q (row stride ldq elements, H heads of Dh) against the slots of sequence b, found through its row of the table: it counts
 * slot j iff j <= len0[b] + i and block_table[b][j / SETOK_KV_PAGE] is a page.  The new rows' keys / values are already in slots [len0[b], len0[b] +
 * Tn) (setok_kv_append_paged with slot0 = len0).  len0: (B,) int32 on the device; len0[b] < 0 is an idle sequence - its Tn output rows are exact
 * zeros and nothing of the pools or the table is read for it.  max_len0 is the host's upper bound on len0 (len0[b] <= max_len0, max_len0 + Tn <=
 * max_pages * SETOK_KV_PAGE): the grid's span dimension and the workspace come from it.  A table entry outside [0, num_pages) is "no page", as
 * above: no key of that page counts, no address is formed from the id, nothing is loaded for it.  Slots at or above len0[b] + Tn and pages nobody
 * points at may hold anything, NaN included.
 * Sequence b's output bits are those of setok_attention_extend_gqa at B = 1, len0 = len0[b], on its slots gathered into a dense cache under an
 * all-ones mask (a missing page: a mask that is zero on its SETOK_KV_PAGE slots): the dense kernels' key tiles (32 slots from slot 0), chunks and
 * spans never straddle a page, so the partition into partials, the arithmetic and the merge order are the dense call's - the bits depend on the
 * sequence's own q, keys, values and length alone, not on the table, the pool, B, max_len0 or the run.  Both dense paths have a twin: the MFMA
 * kernel (this build's 16-bit dtype, Dh = 128; NW = 1 / 4 and the span rule on H / Hkv * Tn as there) and the wave-per-chunk kernel (everything
 * else).  Dh as for setok_attention_decode_gqa_paged; q and the pools 16-byte aligned, ldq % 8 == 0, ws 8-byte aligned,
 * ws_floats >= setok_attention_extend_paged_workspace(...).  B == 0 launches nothing. */
int setok_attention_extend_gqa_paged(void* stream, int dtype, const void* q, int64_t ldq, const void* k_pool, const void* v_pool,
                                     const int32_t* block_table, int max_pages, int num_pages, const int32_t* len0, void* out, int B, int Tn, int H,
                                     int Hkv, int Dh, int max_len0, float scale, float* ws, int64_t ws_floats);

/* ---- Paged MXFP4 KV cache (csrc/attn_paged.hip, csrc/attn_extend_paged.hip): the pools of "Paged KV cache" stored by the rule of "MXFP4 KV
 * cache" - the smallest rows in pages that go back to a pool.  One layer's pools are
 *     k_q, v_q (num_pages, Hkv, SETOK_KV_PAGE, Dh/2) uint8     e2m1 nibbles, element 2j of a row in the low nibble of byte j
 *     k_s, v_s (num_pages, Hkv, SETOK_KV_PAGE, Dh/32) uint8    e8m0 scale bytes, one per 32 elements of a row
 * and a row means what a row of the dense MXFP4 cache means.  block_table, lens / len0, slot0, max_pages, num_pages and max_len / max_len0 are
 * those of the native paged entries; a table entry outside [0, num_pages) is "no page" and never becomes an address.  The pools take
 * 2 * layers * num_pages * Hkv * SETOK_KV_PAGE * (Dh/2 + Dh/32) bytes: 68 per slot at Dh = 128 against 256 in 16 bits.  The kernels are the
 * dense MXFP4 kernels' arithmetic on the same partition of the keys, so a sequence's bits are the dense MXFP4 entries' on its gathered slots
 * (DESIGN.md §7 f19).  e4m3 pools are not built: that format has no extend attention.  Pure additions: the ABI version stays 9. */

/* setok_kv_append_mxfp4's quantiser with setok_kv_append_paged's destination: row b * T + t of the fused buffer goes, quantised block by block,
 * to page block_table[b][slot / SETOK_KV_PAGE], row slot % SETOK_KV_PAGE, slot = slot0[b] + t.  Nothing is written for a sequence with
 * slot0[b] < 0, for a slot past the table's max_pages entries or for a table entry that is no page (such a row's lanes load and store nothing but
 * still take part in the quantiser's lane exchanges); no other byte of the four pools is written.  The bytes written are exactly those
 * setok_kv_append_mxfp4 writes for the same source row, a block with a non-finite entry (scale byte 0xFF, nibbles 0) included.
 * Dh in {32, 64, 128}, as for the decode attention below; qkv, k_q and v_q 16-byte aligned. */
int setok_kv_append_paged_mxfp4(void* stream, int dtype, const void* qkv, uint8_t* k_q, uint8_t* k_s, uint8_t* v_q, uint8_t* v_s,
                                const int32_t* block_table, int max_pages, int num_pages, const int32_t* slot0, int B, int T, int H, int Hkv, int Dh);

/* setok_attention_decode_gqa_paged over MXFP4 pools: the same kernel over the nibble format.  A chunk is SETOK_DECODE_CHUNK_MXFP4KV = 256 slots,
 * TWO pages: a wave's slice is 64 slots and never straddles a page, waves 0-1 of chunk c read table entry 2c and waves 2-3 entry 2c + 1.  A wave
 * whose slice starts at or past lens[b] reads no table entry and loads nothing, and neither does one whose entry lies at or past max_pages (entry
 * 2c + 1 at an odd max_pages) or is no page: each writes the empty partial.  The grid's chunk dimension and the workspace come from
 * ceil(max_len / 256): ws_floats >= B * H * ceil(max_len / SETOK_DECODE_CHUNK_MXFP4KV) * (Dh + 2); the merge takes each sequence's chunk count
 * from lens[b].  Sequence b's output bits are those of setok_attention_decode_gqa_mxfp4kv at B = 1 on its slots gathered into a dense MXFP4 cache
 * with an all-ones mask and len = lens[b] (a missing page: a mask that is zero on its 128 slots).  Dh in {32, 64, 128}, the head dims with a lane
 * layout over nibble rows (16 elements per lane); any other is refused - the dense entry serves them with the generic kernel, which has no paged
 * twin, and a lane layout of its own for 256 or 512 would not give the dense call's bits.  q, k_q and v_q 16-byte aligned, ldq % 8 == 0. */
int setok_attention_decode_gqa_paged_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                             const uint8_t* v_q, const uint8_t* v_s, const int32_t* block_table, int max_pages, int num_pages,
                                             const int32_t* lens, void* out, int B, int H, int Hkv, int Dh, int max_len, float scale, float* ws,
                                             int64_t ws_floats);

/* Floats of workspace setok_attention_extend_gqa_paged_mxfp4kv needs: setok_attention_extend_mxfp4kv_workspace's rule at len0 = max_len0,
 * B * Tn * H * ceil((max_len0 + Tn) / SETOK_EXTEND_CHUNK) * (Dh + 2) (the MFMA path uses a prefix of it, as the dense call's does). */
int64_t setok_attention_extend_paged_mxfp4kv_workspace(int B, int Tn, int H, int Dh, int max_len0);

/* setok_attention_extend_gqa_paged over MXFP4 pools, with that call's meaning of every argument (len0[b] per sequence, < 0 idle; "no page";
 * only slots that count are read), and setok_attention_extend_gqa_mxfp4kv's dispatch.  The 16-bit type at Dh == 128: the MFMA kernel of
 * setok_attention_extend_gqa_paged — one table lookup per 32-key tile, a tile without a page is not staged — with its tiles converted from
 * nibbles on their way to LDS; THE OUTPUT BITS ARE THOSE OF setok_attention_extend_gqa_paged on the same q, block_table, len0 and Tn over pools
 * that hold K', V', provided K', V' are representable in the element type (every row setok_kv_append_paged_mxfp4 writes is; a hand-made scale
 * byte outside [-13, 13] + 127 is the caller's business); needs Hkv * ceil((H / Hkv) * Tn / 128) <= 65535.  Everything else (fp32, the other
 * Dh % 32 == 0): one wave per (query row, query head, chunk of SETOK_EXTEND_CHUNK = 256 slots, two pages), a key per lane with its page looked
 * up per key, then the merge in chunk order — the functional path.  On either path sequence b's output bits are those of
 * setok_attention_extend_gqa_mxfp4kv at B = 1, len0 = len0[b], on its gathered slots under an all-ones mask.  q, k_q and v_q 16-byte aligned,
 * ldq % 8 == 0, ws_floats >= setok_attention_extend_paged_mxfp4kv_workspace(...).  B == 0 launches nothing. */
int setok_attention_extend_gqa_paged_mxfp4kv(void* stream, int dtype, const void* q, int64_t ldq, const uint8_t* k_q, const uint8_t* k_s,
                                             const uint8_t* v_q, const uint8_t* v_s, const int32_t* block_table, int max_pages, int num_pages,
                                             const int32_t* len0, void* out, int B, int Tn, int H, int Hkv, int Dh, int max_len0, float scale,
                                             float* ws, int64_t ws_floats);

/* ---- The DiffLoss image head (src/model/loss/diffloss.py: SimpleMLPAdaLN driven by a respaced cosine DDPM with learned-range variance,
 * src/model/diffusion/).  Its Linears are setok_linear calls, its plain SiLUs setok_activation(SETOK_ACT_SILU); these are the rest
 * (csrc/diffusion.hip).  Every entry is asynchronous on `stream`, allocates nothing, synchronises nothing, accepts rows == 0, uses 16-byte
 * accesses (row lengths % 8 == 0, operands and row strides 16-byte aligned), one wave per row, fp32 arithmetic, no atomics; a row's bits depend
 * on that row's operands alone.  Pure additions: the ABI version stays 9. */

/* TimestepEmbedder.timestep_embedding (diffloss.py:73-91): emb[r, j] = cos(t[r] * f_j), emb[r, half + j] = sin(t[r] * f_j) for j < half = dim / 2,
 * f_j = exp(-ln(max_period) * j / half) — fp32 arguments and the accurate cosf / sinf (the arguments reach 999 rad), rounded to `dtype` once.
 * t: fp32 (rows,) on the device; emb: (rows, dim); dim % 16 == 0. */
int setok_timestep_embedding(void* stream, int dtype, const float* t, void* emb, int rows, int dim, float max_period);

/* y[r, :] = SiLU(a[r, :] + b[r * ldb + :]): the `y = t + c` of SimpleMLPAdaLN.forward (diffloss.py:229) with the nn.SiLU every adaLN_modulation
 * starts with (:120,140) applied once for all of them.  ldb = 0 broadcasts ONE row b (the sampler: one timestep for all rows). rows x C. */
int setok_add_silu(void* stream, int dtype, const void* a, const void* b, int64_t ldb, void* y, int rows, int C);

/* One launch per ResBlock boundary (diffloss.py:124-128,144-148):
 *     if h:  x[r, :] <- x[r, :] + gate[r, :] * h[r, :]                         (the previous block's gated residual, written back in place)
 *     y[r, :] = LayerNorm(x[r, :]; gamma, beta, eps) * (1 + scale[r, :]) + shift[r, :]     (modulate(in_ln(x), shift, scale))
 * gamma / beta: fp32 (C,), both NULL for a LayerNorm without affine (FinalLayer.norm_final).  shift, scale, gate: column windows of ONE wider
 * row-major buffer of `dtype` — each a pointer to its first column, with the buffer's row stride ldm (elements) — so the output of the fused
 * adaLN_modulation GEMM is consumed in place, without `chunk` copies.  h, gate: both NULL (no residual) or both given.  x, h, y: rows x C
 * contiguous; y must not alias x.  Two-pass fp32 statistics of the STORED (rounded) x; one rounding to `dtype` per output. */
int setok_adaln_modulate(void* stream, int dtype, void* x, const void* h, const void* gate, const float* gamma, const float* beta,
                         const void* shift, const void* scale, int64_t ldm, void* y, int rows, int C, float eps);

/* One reverse step of the sampler: GaussianDiffusion.p_mean_variance + p_sample (gaussian_diffusion.py:285-339,404-419; EPSILON mean type,
 * LEARNED_RANGE variance, clip_denoised = False) on the net's output `out` (rows x 2C, row stride ldo, element type out_dtype = `dtype` or SETOK_F32):
 *     eps    = out[r, :C]                                  (half == 0)
 *            = u + cfg_scale * (c - u),  c = out[r mod half, :C],  u = out[r mod half + half, :C]      (half > 0: rows == 2 * half, forward_with_cfg)
 *     v      = out[r, C:2C]
 *     x0     = sqrt_recip * x[r] - sqrt_recipm1 * eps;    mean = coef1 * x0 + coef2 * x[r]
 *     logvar = f * max_log + (1 - f) * min_log,  f = (v + 1) / 2
 *     x[r]  <- mean + nonzero * exp(0.5 * logvar) * noise[r mod noise_rows] * temperature
 * x: fp32 (rows, C), updated in place — the sampler's state stays fp32 in every dtype mode; noise: fp32 (noise_rows, C), noise_rows = rows or, with one draw
 * shared by both halves, half.  nonzero = 0 at the last step makes the noise term exactly 0 for finite noise.  x_in: (rows, C) in `dtype`, the next
 * evaluation's input_proj operand: row r gets the new x[r] (half == 0) or the new x[r mod half] (the conditional half duplicated). */
int setok_ddpm_step(void* stream, int dtype, int out_dtype, const void* out, int64_t ldo, float* x, const float* noise, int noise_rows, void* x_in,
                    int rows, int C, int half, float cfg_scale, float sqrt_recip, float sqrt_recipm1, float coef1, float coef2, float min_log,
                    float max_log, float nonzero, float temperature);

/* ---- The skinny GEMM of a LoRA adapter (csrc/gemm_skinny.hip).  Every adapter GEMM has one dimension equal to the rank r; with r as the
 * OUTPUT width the tiled kernels of setok_linear get cdiv(M, 128) workgroups that each walk the whole K.  Pure additions: the ABI version stays 9. */

/* Widest output setok_linear_skinny takes, and the columns of one K slice (counted from column 0; a multiple of 64). */
#define SETOK_SKINNY_MAX_N 256
#ifndef SETOK_SKINNY_KSLICE
#define SETOK_SKINNY_KSLICE 512
#endif

/* Floats of workspace setok_linear_skinny needs: ceil(K / SETOK_SKINNY_KSLICE) * M * N (0 for an empty problem). */
int64_t setok_linear_skinny_workspace(int M, int N, int K);

/* C[M, N] = alpha * A[M, K] · W[N, K]^T   for 1 <= N <= SETOK_SKINNY_MAX_N, N % 16 == 0, any M >= 0.  A, W in `dtype` (the build's 16-bit type
 * or SETOK_F32), C in out_dtype = `dtype` or SETOK_F32.  K % 64 == 0 (16-bit) or K % 16 == 0 (fp32).  Strides as in setok_linear, in elements:
 * lda >= K, ldw >= K (multiples of 8 / 4: 16-byte pieces), ldc >= N (a multiple of 8 for a 16-bit C, of 4 for fp32); A, W, C and ws 16-byte
 * aligned; a stride changes addresses only.  No element outside A's [0, M) x [0, K) or W's [0, N) x [0, K) is read, none outside C's
 * [0, M) x [0, N) is written.
 * Split-K by a rule in K alone: grid (blocks of 128 rows, slices of SETOK_SKINNY_KSLICE columns); every workgroup writes the fp32 partial of its
 * rows over its slice to ws[slice][M][N], and a second launch sums a row's partials in slice order, multiplies by alpha once in fp32 and rounds
 * once.  No atomics, no hand-off between workgroups.  A row's bits depend on that row of A, W, K and alpha alone — not on M, the strides or the
 * rows around it.  It is NOT setok_linear's summation order.  16-bit: v_mfma_f32_32x32x16, W's slice tile through LDS (N x 64 columns per K
 * step), A's rows streamed.  SETOK_F32 is the parity mode: a plain k-ordered fmaf chain per slice.
 * ws: ws_floats >= setok_linear_skinny_workspace(M, N, K) floats, the caller's.  A shorter workspace, and every other bad argument, is
 * SETOK_EINVAL with a message naming it, before any launch. */
int setok_linear_skinny(void* stream, int dtype, int out_dtype, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                        int M, int N, int K, float alpha, float* ws, int64_t ws_floats);

#ifdef __cplusplus
}
#endif
#endif /* SETOK_HIP_H */
