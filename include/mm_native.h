/*
 * mm_native.h — C ABI of libmm_native.so: MI355X (gfx950) interaction-scoring kernels for
 * matchmaker's re-ranking forward pass.
 *
 * The reference (sebastian-hofstaetter/matchmaker) is pure Python: it has no FFI of its own.
 * Its "operator API" for this path is the nn.Module protocol of SURVEY.md §8(b).  Each entry
 * point below replaces the arithmetic of one reference method; the Python host side
 * (the .py modules of matchmaker_amd/) mirrors the method signatures and binds these symbols with ctypes
 * (INTEGRATION.md shows the stub a matchmaker maintainer would add).
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HBM) unless stated; tensors are dense, row-major,
 *     innermost dimension contiguous, 16-byte aligned base;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work;
 *   - return 0 on success, a negative MM_E* code otherwise; mm_last_error() gives a
 *     thread-local message.  Nothing is allocated, retained or synchronised by the library.
 */
#ifndef MM_NATIVE_H
#define MM_NATIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM_ABI_VERSION 4 /* 4: mm_kernel_pool_ex_fwd2 / mm_kernel_pool_ex_bwd2 (the forward hands its pooled kernel sums to the backward),
                          *    mm_maxsim_fwd_batched (several eval.py-sized batches per launch).
                          * 3: 2: `flags` on the MaxSim forwards (the reference's 16-bit dtype flow); mm_tkl_fwd's ascending chunk_slot
                            contract and workspace layout.  3: + mm_tkl_fwd_peaks (the region search's three peak indices) */

/* element types of the embedding tensors */
#define MM_F32 0
#define MM_F16 1
#define MM_BF16 2

/* how a mask argument is encoded (the reference passes int64 HF attention masks to ColBERT —
 * colbert.py:69,73 — and float {0,1} masks to TK/TKL — neuralIR_encoder.py:35-37) */
#define MM_MASK_NONE 0    /* pointer ignored: every position is a real token              */
#define MM_MASK_LEN_I32 1 /* int32[rows]: positions >= len are padding (prefix masks)      */
#define MM_MASK_U8 2      /* uint8/bool[rows, L], nonzero = real token                     */
#define MM_MASK_I64 3     /* int64[rows, L]   (HF tokenizer attention_mask)                */
#define MM_MASK_F32 4     /* float[rows, L]   (matchmaker embedding-model masks)           */

/* error codes */
#define MM_OK 0
#define MM_EINVAL -1       /* bad argument (null pointer, non-positive size, bad enum)     */
#define MM_EUNSUPPORTED -2 /* shape/dtype outside what the kernels implement               */
#define MM_EWORKSPACE -3   /* workspace missing or too small                               */
#define MM_ELAUNCH -4      /* HIP reported a launch error                                  */

/* `flags` of the MaxSim forwards: the reference's dtype flow for 16-bit inputs.  In the reference the similarity matrix has
 * the dtype of the token vectors: under torch.cuda.amp.autocast(enabled=use_fp16) — config/train/defaults.yaml:21
 * `use_fp16: True`, colbert.py:60 — `bmm` returns fp16 (fp32 accumulation, ONE rounding per element), the -1000 fill and
 * `max` stay fp16 and only `sum` is promoted to fp32 (colbert.py:68-75).  Rounding is monotone, so rounding the per-token
 * maximum reproduces that arithmetic exactly.
 *   MM_SIM_ROUND  every per-query-token maximum is rounded (RNE) to the element type of q / d before the fp32 sum:
 *                 ColBERT.forward / forward_aggregation under autocast (colbert.py:60-75, indexing_heads.py:49-56)
 *   MM_SUM_ROUND  the pair's sum is rounded to that type as well: 16-bit tensors OUTSIDE autocast, where `sum` is a 16-bit op
 *                 too (fp32 accumulation, one rounding) — the dynamic teacher's all-pairs call, dynamic_teacher.py:245-246
 * Both are no-ops for MM_F32 inputs.  0 = fp32 accumulators through max and sum (the fp32 contract of `use_fp16: False`). */
#define MM_SIM_ROUND 1
#define MM_SUM_ROUND 2

int mm_abi_version(void);
const char* mm_last_error(void);

/* ------------------------------------------------------------------------------------------
 * ColBERT late-interaction MaxSim.
 *
 *   out[p] = sum_{i < Q, q_mask[i]}  max_{j < D} ( d_mask[p, j] ? <q[i,:], d[p,j,:]> : -1000 )
 *
 * Replaces: ColBERT.forward scoring block            matchmaker/models/colbert.py:68-75
 *           ColBERT.forward_aggregation (no masks)   matchmaker/models/colbert.py:100-112
 *
 *   q   [n_queries, Q, E]   n_queries = ceil(n_pairs / pairs_per_query)
 *   d   [n_pairs,   D, E]   pair p uses query p / pairs_per_query
 *   out [n_pairs] float32
 *
 * pairs_per_query = 1 is the reference's pair-per-row layout (query replicated per pair,
 * eval.py:108); pairs_per_query = C is the "1 query x C candidates" re-ranking layout in which
 * the query tile is read once per candidate list.
 * q_mask rows follow q (n_queries rows), d_mask rows follow d (n_pairs rows).
 * flags: MM_SIM_ROUND / MM_SUM_ROUND above (0 = fp32 through max and sum).
 * workspace: mm_maxsim_workspace_bytes() bytes of device scratch (may be 0 -> NULL allowed).  It holds the packed masks;
 *   calls whose int64 masks the kernel reads itself (the pair-per-row layout, and long queries when every wavefront scores
 *   one pair: eval.py's 512-pair batches) leave it untouched.
 */
size_t mm_maxsim_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int Q, int D,
                                 int q_mask_kind, int d_mask_kind);

int mm_maxsim_fwd(const void* q, const void* d,
                  const void* q_mask, int q_mask_kind,
                  const void* d_mask, int d_mask_kind,
                  float* out,
                  int64_t n_pairs, int64_t pairs_per_query,
                  int Q, int D, int E, int dtype, int flags,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Several pair-per-row batches of ONE shape scored by ONE launch: the scoring block of ColBERT.forward (colbert.py:68-75) as
 * eval.py:82-108 drives it — `batch_size_eval: 512` pairs per model.forward (config/train/defaults.yaml:115) — for a caller that
 * holds the token vectors of several batches (matchmaker_amd/rerank.py evaluate_batches(score_group=...)).  A 512-pair call at
 * dim 128 is 3.6 us of HBM time behind a ~9 us launch chain; the group pays the chain once.
 *   batches[i]: q [n_pairs, Q, E], d [n_pairs, D, E] (16-bit vectors, 16-byte aligned), q_mask [n_pairs, Q] / d_mask [n_pairs, D]
 *   (int64 tokenizer masks, or NULL for all of them), out [n_pairs] float32; the descriptors are HOST memory (read during the call).
 *   Shapes the pair-per-row kernel takes (Q <= 32, E in {128, 256, 384, 512, 768}, even Q and D <= 256 with masks); anything
 *   else returns MM_EUNSUPPORTED and the caller scores batch by batch with mm_maxsim_fwd.  n_batches <= MM_MAXSIM_MAX_BATCHES.
 * Scores: bit-equal to mm_maxsim_fwd on each batch alone (same kernel body; flags as there). */
#define MM_MAXSIM_MAX_BATCHES 16
typedef struct {
  const void* q;
  const void* d;
  const void* q_mask;
  const void* d_mask;
  float* out;
  int64_t n_pairs;
} mm_maxsim_batch_t;
int mm_maxsim_fwd_batched(const mm_maxsim_batch_t* batches, int n_batches, int q_mask_kind, int d_mask_kind,
                          int Q, int D, int E, int dtype, int flags, void* stream);

/* All-pairs MaxSim: out[i, j] over query i x document j.
 * Replaces ColBERT.forward_inbatch_aggregation       matchmaker/models/colbert.py:154-162
 * bug_compatible != 0 reproduces the reference's mask expansion (:158), which masks
 * score[i, j] with document i's mask and requires Bq == Bd (MM_EINVAL otherwise).
 *   q [Bq, Q, E], d [Bd, D, E], out [Bq, Bd] float32 */
size_t mm_maxsim_inbatch_workspace_bytes(int64_t Bq, int64_t Bd, int Q, int D,
                                         int q_mask_kind, int d_mask_kind);

int mm_maxsim_inbatch_fwd(const void* q, const void* d,
                          const void* q_mask, int q_mask_kind,
                          const void* d_mask, int d_mask_kind,
                          float* out,
                          int64_t Bq, int64_t Bd, int Q, int D, int E, int dtype,
                          int bug_compatible, int flags,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Ragged (CSR) MaxSim over a resident token store: document p = rows [doc_begin[p], doc_end[p]) of
 * `tokens` [T, E]; no padding, no document mask (every stored row is a real token: zero rows were
 * stripped when the store was written, dense_retrieval.py:244).  One launch replaces the
 * per-candidate Python loop of the ColBERT retrieval aggregate
 *   matchmaker/dense_retrieval.py:398-412   (doc_infos[seq_id] = (file, start, end) -> storage[file][start:end])
 *   ColBERT.forward_aggregation             matchmaker/models/colbert.py:100-112
 * q [n_queries, Q, E] in the store's dtype, pair p uses query p / pairs_per_query; q_mask as for
 * mm_maxsim_fwd (MM_MASK_NONE reproduces forward_aggregation exactly).  An empty range scores like
 * a fully padded document (-1000 per query token).  out [n_pairs] float32. */
size_t mm_maxsim_ragged_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int Q, int q_mask_kind);

int mm_maxsim_ragged_fwd(const void* q, const void* tokens, const int64_t* doc_begin, const int64_t* doc_end,
                         const void* q_mask, int q_mask_kind, float* out,
                         int64_t n_pairs, int64_t pairs_per_query, int Q, int E, int dtype, int flags,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Calibration, not scoring: mm_maxsim_fwd's HBM read stream with the arithmetic removed (same launch geometry, LDS-DMA
 * blocks, ring and counted waits; no MFMA, no maximum) over `bytes` of `src` (16-byte aligned, a multiple of 8192 bytes).
 * bench.py times it over the headline's document tensor and prints the headline kernel's rate as a fraction of it, so
 * that a slow box and a slow kernel can be told apart from the benchmark line alone.  nt != 0: non-temporal loads, as
 * the headline kernel issues them. */
int mm_hbm_stream_probe(const void* src, int64_t bytes, int nt, void* stream);

/* Backward of the paired MaxSim (pair-per-row layout, the one train.py uses: train.py:347-348,
 * loss.backward() :503-524).  Recomputes the similarities and routes grad_out[p] to the FIRST
 * arg-max document position of every real query token (torch.max's rule); nothing flows through
 * the -1000 sentinel (colbert.py:69) or padded query tokens (:73).
 *   grad_out [n_pairs] float32; grad_q [n_pairs, Q, E], grad_d [n_pairs, D, E] of element type grad_dtype: MM_F32, or the
 *   token vectors' own 16-bit type (what autograd hands back to an fp16 / bf16 encoder: summed in fp32, rounded once).
 *   Both are fully written by the call (rows without gradient are zeros: no memset needed in front of it).
 *   q/d/masks exactly as given to the forward. */
size_t mm_maxsim_bwd_workspace_bytes(int64_t n_pairs, int Q, int D, int q_mask_kind, int d_mask_kind);

int mm_maxsim_bwd(const void* q, const void* d,
                  const void* q_mask, int q_mask_kind,
                  const void* d_mask, int d_mask_kind,
                  const float* grad_out, void* grad_q, void* grad_d, int grad_dtype,
                  int64_t n_pairs, int Q, int D, int E, int dtype,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the all-pairs MaxSim (mm_maxsim_inbatch_fwd): autograd through matchmaker/models/colbert.py:154-162, the
 * [Bq, Bd] score matrix of in-batch-negative training (train.py:434-467 builds it, loss.backward() train.py:503-524).
 *   j*(i, j, t) = the FIRST arg-max over the document positions of <q[i, t], d[j, .]> with masked positions at -1000 (mask row
 *   j, or row i with bug_compatible != 0, which needs Bq == Bd: MM_EINVAL otherwise); no gradient for a padded query token
 *   or when the arg-max is a masked position.  The arg-max is taken on the recomputed fp32-accumulated similarities (the
 *   rule of mm_maxsim_bwd; the forward's MM_SIM_ROUND plays no part).
 *     grad_q[i, t, :] = sum_j grad_out[i, j] d[j, j*(i, j, t), :]
 *     grad_d[j, p, :] = sum_i sum_{t : j*(i, j, t) = p} grad_out[i, j] q[i, t, :]
 *   grad_out [Bq, Bd] float32; grad_q [Bq, Q, E], grad_d [Bd, D, E] of element type grad_dtype: MM_F32, or the token vectors'
 *   own 16-bit type (summed in fp32, rounded once).  Every byte of both is written by the call (zeros where nothing flows).
 *   grad_q or grad_d may be NULL: that gradient is not needed (a frozen encoder) and its pass is not run.
 *   No floating-point atomics: sums run in a fixed order (ascending j; ascending (i, t)), two calls give the same bits.
 *   One stream, no host synchronisation, no allocation: the call can be captured into a graph.
 *   q/d/masks exactly as given to the forward.  The workspace holds the packed masks and the int16 [Bq, Bd, Q] arg-max table.
 *   MM_EUNSUPPORTED: E rows that are not 16-byte multiples, D > 14336 (the LDS accumulator of grad_d; the table holds 32767). */
size_t mm_maxsim_inbatch_bwd_workspace_bytes(int64_t Bq, int64_t Bd, int Q, int D, int E, int q_mask_kind, int d_mask_kind);

int mm_maxsim_inbatch_bwd(const void* q, const void* d,
                          const void* q_mask, int q_mask_kind,
                          const void* d_mask, int d_mask_kind,
                          const float* grad_out, void* grad_q, void* grad_d, int grad_dtype,
                          int64_t Bq, int64_t Bd, int Q, int D, int E, int dtype, int bug_compatible,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * TK kernel pooling (cosine match matrix + K RBF kernels + log-sum pooling + bin weights).
 *
 *   cos[i,j]  = <q_i, d_j> / ((|q_i| + 1e-13)(|d_j| + 1e-13))
 *   pkq[i,k]  = sum_j d_mask[j] * exp(-(cos[i,j] - mu[k])^2 / (2 sigma[k]^2))
 *   out[p]    = sum_k w[k] * sum_i q_mask[i] * log(max(pkq[i,k] * alpha[k], 1e-10))
 *
 * Replaces: ECAI20_TK.forward pooling block   matchmaker/models/published/ecai20_tk.py:105-124
 *           (cosine = allennlp CosineMatrixAttention, call site ecai20_tk.py:105)
 *
 *   q [n_queries, Q, E], d [n_pairs, D, E] float32 contextualised embeddings
 *   mu, sigma, alpha, w: float32[K] device pointers, K <= 32 (K = 11, the reference configs, takes the
 *          streaming kernels; any other count the generic kernel)
 *   per_kernel: optional float32 [n_pairs, K] (the reference's secondary output), may be NULL
 *   masks: float {0,1} as the reference passes them (MM_MASK_F32) or any other mm mask kind;
 *          nonzero = real token.  workspace as for mm_maxsim_fwd.
 */
size_t mm_kernel_pool_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int Q, int D,
                                      int q_mask_kind, int d_mask_kind);

int mm_kernel_pool_fwd(const void* q, const void* d,
                       const void* q_mask, int q_mask_kind,
                       const void* d_mask, int d_mask_kind,
                       const float* mu, const float* sigma, const float* alpha, const float* w,
                       float* out, float* per_kernel,
                       int64_t n_pairs, int64_t pairs_per_query,
                       int Q, int D, int E, int K, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Variants of the pooling block that share its arithmetic:
 *   d_gate     optional float32 [n_pairs, D], >= 0: every activation of document token j is multiplied by
 *              d_gate[p, j] on top of d_mask — TK-Sparse's learned stop-word vector
 *              (matchmaker/models/published/cikm20_tk_sparse.py:133-135; negative values count as 0, the
 *              reference's gate is a ReLU output).  NULL = no gate (= mm_kernel_pool_fwd).
 *   clamp_min  the floor inside the log: 1e-10 for TK / TK-Sparse (ecai20_tk.py:121, cikm20_tk_sparse.py:142),
 *              1e-4 for the IDCM passage sampler (matchmaker/models/published/sigir21_idcm.py:182-186, whose
 *              pre-normalised vectors make the cosine's own normalisation a no-op).  Must be > 0.
 *   pair_query optional int32 [n_pairs]: the query row of every pair, for ragged groups — IDCM scores a
 *              different number of passages per document against the document's query (the reference
 *              materialises one query copy per passage, sigir21_idcm.py:143-144).  With it q / q_mask have
 *              n_queries rows and pairs_per_query is ignored; NULL = the uniform pairs_per_query layout.
 *              Consecutive equal entries reuse the query tile already in registers.  The workspace then packs
 *              n_queries query-mask rows: size it with
 *              mm_kernel_pool_workspace_bytes(max(n_pairs, n_queries), 1, Q, D, kinds).
 * Everything else as mm_kernel_pool_fwd (which calls this with NULL, NULL, 0, ..., 1e-10). */
int mm_kernel_pool_ex_fwd(const void* q, const void* d,
                          const void* q_mask, int q_mask_kind,
                          const void* d_mask, int d_mask_kind,
                          const float* d_gate,
                          const int32_t* pair_query, int64_t n_queries,
                          const float* mu, const float* sigma, const float* alpha, const float* w,
                          float clamp_min,
                          float* out, float* per_kernel,
                          int64_t n_pairs, int64_t pairs_per_query,
                          int Q, int D, int E, int K, int dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

/* mm_kernel_pool_ex_fwd with one more optional output, for training (train.py:347-348 forward, :503-524 backward):
 *   pooled [n_pairs, Q, K] float32 or NULL: the pooled kernel sums pkq[i][k] = sum_j mask_j gate_j exp(-(cos_ij - mu_k)^2 / (2 sigma_k^2))
 *   (ecai20_tk.py:120, before kernel_alpha_scaler / clamp / log), one row per query token.  Every position of the document
 *   enters each of them, so the backward cannot form a gradient before it has them; handed to mm_kernel_pool_ex_bwd2 they
 *   save its pooling pre-pass — the document's second trip through HBM.  Rows of padded / masked query tokens are unspecified. */
int mm_kernel_pool_ex_fwd2(const void* q, const void* d,
                           const void* q_mask, int q_mask_kind,
                           const void* d_mask, int d_mask_kind,
                           const float* d_gate,
                           const int32_t* pair_query, int64_t n_queries,
                           const float* mu, const float* sigma, const float* alpha, const float* w,
                           float clamp_min,
                           float* out, float* per_kernel, float* pooled,
                           int64_t n_pairs, int64_t pairs_per_query,
                           int Q, int D, int E, int K, int dtype,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Several (query tensor, document tensor) combinations pooled in ONE launch and summed: Conv-KNRM scores every
 * n-gram width of the query against every n-gram width of the document (n_grams^2 match matrices,
 * matchmaker/models/conv_knrm.py:130-132) and its dense layer (:137) is a weighted sum over all of them:
 *   out[p] = sum_{i < n_q, t < n_d} kernel_pool(q_list[i], d_list[t]; bin weights w[(i * n_d + t) * K ...])[p]
 * (summed in (i, t) order: deterministic).  q_list[i] [n_queries, Q, E], d_list[t] [n_pairs, D, E] float32, one mask
 * pair for all of them (the n-gram tensors share the token masks).  1 <= n_q, n_d <= 4, K = 11.
 * Workspace: mm_kernel_pool_multi_workspace_bytes (mask packing + the n_q * n_d partial score rows). */
size_t mm_kernel_pool_multi_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int n_q, int n_d, int Q, int D,
                                            int q_mask_kind, int d_mask_kind);
int mm_kernel_pool_multi_fwd(const void* const* q_list, int n_q, const void* const* d_list, int n_d,
                             const void* q_mask, int q_mask_kind, const void* d_mask, int d_mask_kind,
                             const float* mu, const float* sigma, const float* alpha, const float* w,
                             float clamp_min, float* out, int64_t n_pairs, int64_t pairs_per_query, int Q, int D,
                             int E, int K, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of mm_kernel_pool_fwd in the pair-per-row layout (training: train.py:347-348, loss.backward()
 * :503-524; the embedding model is called from neuralIR_encoder.py:86-87).  Gradients of the score w.r.t.
 * the contextualised embeddings and the two trainable pooling parameters (kernel_alpha_scaler
 * ecai20_tk.py:85, kernel_bin_weights :81); mu / sigma are buffers.
 *   grad_out [n_pairs]; grad_q [n_pairs, Q, E], grad_d [n_pairs, D, E] float32;
 *   grad_alpha, grad_w [n_pairs, K]: per-pair contributions (sum over pairs on the host side:
 *   deterministic, no atomics). */
size_t mm_kernel_pool_bwd_workspace_bytes(int64_t n_pairs, int Q, int D, int q_mask_kind, int d_mask_kind);
/* ... plus the partial grad_q buffers of a small batch (<= 128 pairs: several workgroups share a pair's document blocks and a
 * combine kernel finishes grad_q).  Optional: with the smaller workspace above each pair gets one workgroup. */
size_t mm_kernel_pool_bwd_workspace_bytes2(int64_t n_pairs, int Q, int D, int E, int q_mask_kind, int d_mask_kind);

int mm_kernel_pool_bwd(const void* q, const void* d,
                       const void* q_mask, int q_mask_kind,
                       const void* d_mask, int d_mask_kind,
                       const float* mu, const float* sigma, const float* alpha, const float* w,
                       const float* grad_out, float* grad_q, float* grad_d, float* grad_alpha, float* grad_w,
                       int64_t n_pairs, int Q, int D, int E, int K,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Backward of mm_kernel_pool_ex_fwd: as mm_kernel_pool_bwd, plus grad_gate [n_pairs, D] (may be NULL;
 * needs d_gate), the gradient w.r.t. the gate values (training of TK-Sparse's stop-word MLP,
 * cikm20_tk_sparse.py:133-135). */
int mm_kernel_pool_ex_bwd(const void* q, const void* d,
                          const void* q_mask, int q_mask_kind,
                          const void* d_mask, int d_mask_kind,
                          const float* d_gate,
                          const float* mu, const float* sigma, const float* alpha, const float* w,
                          float clamp_min,
                          const float* grad_out, float* grad_q, float* grad_d, float* grad_gate,
                          float* grad_alpha, float* grad_w,
                          int64_t n_pairs, int Q, int D, int E, int K,
                          void* workspace, size_t workspace_bytes, void* stream);

/* mm_kernel_pool_ex_bwd with the forward's pooled kernel sums: pooled [n_pairs, Q, K] as written by mm_kernel_pool_ex_fwd2 on
 * the SAME inputs, or NULL (then the backward pools them itself first and needs the workspace
 * mm_kernel_pool_bwd_workspace_bytes reports).  Same gradients either way (the sums are the same arithmetic). */
int mm_kernel_pool_ex_bwd2(const void* q, const void* d,
                           const void* q_mask, int q_mask_kind,
                           const void* d_mask, int d_mask_kind,
                           const float* d_gate,
                           const float* mu, const float* sigma, const float* alpha, const float* w,
                           float clamp_min, const float* pooled,
                           const float* grad_out, float* grad_q, float* grad_d, float* grad_gate,
                           float* grad_alpha, float* grad_w,
                           int64_t n_pairs, int Q, int D, int E, int K,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * TKL: match + RBF kernels per document position, sliding-window (30, stride 2) pooling with
 * learned saturation, per-window score; then top-3 non-overlapping region scoring.
 *
 * Replaces: TKL_sigir20.forward   matchmaker/models/published/sigir20_tkl.py:180-252 (windows)
 *                                 matchmaker/models/published/sigir20_tkl.py:254-286 (regions)
 *
 *   q_ctx        [B, Q, E]   contextualised query, already multiplied by its mask (:306)
 *   chunks       [P, 50, E]  contextualised packed chunks (output of :172); the 40 centre
 *                            tokens of each are used (:174)
 *   chunk_mask   [P, 50]     float {0,1} (padding_packed, :163)
 *   chunk_slot   [P] int32   flat slot b*C + c of each packed chunk (packed_indices :159, as indices), ASCENDING — the order
 *                            boolean-mask packing (:160-162) and torch.nonzero produce; the kernels rely on a document's
 *                            chunks being adjacent and on its last kept chunk coming last
 *   q_mask       [B, Q]      float {0,1}
 *   params       float32[MM_TKL_NPARAMS(K, E)] device, packed as (matchmaker_amd/tkl.py pack_params()):
 *                  mu[K] sigma[K] dense.weight[K] kernel_mult[0][K]
 *                  saturation_linear{w[2], b}  saturation_linear2{w[2], b}  saturation_linear3{w[2], b}
 *                  sat_normer{weight[2], bias[2]}  chunk_scoring[15]  sat_emb_reduce1.weight[E]
 *   saturation   0 = "embedding" (:224-234), 1 = "log" (:245-246)
 *   win_scores   [B, W] float32 out (W = (max(C*40,30) - 30)/2 + 1), may be NULL if workspace given
 *   out          [B] float32
 *   workspace    mm_tkl_workspace_bytes() bytes of device scratch: the slot -> packed-chunk map, the hand-off between the
 *                match stage and the window stage (the scaled, masked cosines of the real query tokens, 4 B per document
 *                position and token; behind the exact-f32 and the generic match kernels the pair sums of round 2), packed
 *                masks, the live window tiles per document, and the partial window scores of the query-token groups.
 *                Nothing in it survives the call.
 */
#define MM_TKL_NPARAMS(K, E) (4 * (K) + 13 + 15 + (E))
#define MM_TKL_SAT_EMBEDDING 0
#define MM_TKL_SAT_LOG 1
size_t mm_tkl_workspace_bytes(int64_t B, int64_t P, int C, int Q, int K);

int mm_tkl_fwd(const void* q_ctx, const void* chunks, const float* chunk_mask,
               const int32_t* chunk_slot, const float* q_mask, const float* params,
               float* win_scores, float* out,
               int64_t B, int64_t P, int C, int Q, int E, int K, int saturation,
               void* workspace, size_t workspace_bytes, void* stream);

/* mm_tkl_fwd + the region search's own result (ABI 3): top_idx [B, 3] int32 out (may be NULL) receives, per document, the
 * three arg-max window indices in round order — the reference's `top_non_overlapping_idx` (sigir20_tkl.py:266-271, returned
 * under output_secondary_output :290).  With win_scores they give `top_k_non_overlapping` (:276-282) by a gather of 15
 * values per document (matchmaker_amd/tkl.py does that), and they are what a rank-parity check needs to tell "the device
 * picked another region of equal score" from "the device scored a region wrongly" (tie policy). */
int mm_tkl_fwd_peaks(const void* q_ctx, const void* chunks, const float* chunk_mask,
                     const int32_t* chunk_slot, const float* q_mask, const float* params,
                     float* win_scores, float* out, int32_t* top_idx,
                     int64_t B, int64_t P, int C, int Q, int E, int K, int saturation,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Backward of mm_tkl_fwd (training: train.py:503-524 through sigir20_tkl.py:180-286).  The document score is a weighted
 * sum of at most 15 window scores whose indices are piecewise constant, so the exact gradient involves only those windows:
 * they are recomputed from the contextualised vectors and differentiated on the device.
 *   win_scores [B, W]  the forward's window scores (selects the windows; 0 = empty window = constant)
 *   grad_out [B];  grad_q [B, Q, E];  grad_chunks [P, 50, E] (zeroed by the call; only rows of selected windows are non-zero);
 *   grad_params [B, MM_TKL_NPARAMS(K, E)]: per-document gradients in the layout of `params` (mu / sigma columns are 0) —
 *   sum over the documents on the host side (deterministic, no atomics).  Q <= 32.
 * Exact zeros: every row of grad_chunks that none of the document's 15 selected windows reads (the 5 + 5 overlap rows of every
 *   chunk among them) is +0.0 bit for bit, on every kernel below; so is a padding row inside a selected window.
 * Kernels (the same gradients within fp32 rounding; Q > 32 or K != 11: MM_EUNSUPPORTED, nothing written):
 *   E <= 320        tiled kernel, five 16-byte chunks of a block of rows per thread    } E % 4 == 0, q_ctx / chunks / params /
 *   320 < E <= 512  tiled kernel, eight chunks per thread                              } grad_q / grad_chunks 16-byte aligned, and
 *                   the tiles fit 150 KiB of LDS (Q = 32 at E = 512 does not; Q = 12 does)
 *   anything else   the per-element kernel, one workgroup per document (E > 512, or MM_KP_BWD_UNTILED=1 in the environment)
 *   The tiled kernels run three workgroups per document while 3 B <= the device's CUs and the workspace has
 *   mm_tkl_bwd_workspace_bytes2 bytes, else (or with MM_TKL_BWD_NOSPLIT=1) one: grad_chunks bit-equal between the two.
 * Workspace: mm_tkl_bwd_workspace_bytes(B, C). */
size_t mm_tkl_bwd_workspace_bytes(int64_t B, int C);
/* ... plus the per-region shares of grad_q and of the parameter rows of a small batch (3 B <= 256: three workgroups per document,
 * one per arg-max region).  Optional: with the smaller workspace above every document gets one workgroup. */
size_t mm_tkl_bwd_workspace_bytes2(int64_t B, int C, int Q, int E);
int mm_tkl_bwd(const void* q_ctx, const void* chunks, const float* chunk_mask, const int32_t* chunk_slot,
               const float* q_mask, const float* params, const float* win_scores, const float* grad_out,
               float* grad_q, float* grad_chunks, float* grad_params,
               int64_t B, int64_t P, int C, int Q, int E, int K, int saturation,
               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Brute-force inner-product top-k over one GPU's shard of the collection (dense retrieval).
 *
 * Replaces: FaissIdIndexer / FaissBaseIndexer.search   matchmaker/retrieval/faiss_indices.py:22-36, 49-74
 *           (IndexIDMap(IndexFlatIP) sharded over the GPUs, useFloat16; faiss-gpu==1.7.0 is a
 *           third-party dependency, conda-requirements.txt:1), call site dense_retrieval.py:391;
 *           score = BERT_DOT dot product               matchmaker/models/bert_dot.py:62
 *
 *   queries [nq, E], corpus [n_docs, E]  float16 / bfloat16, E in {128, 256, 384, 512, 768}
 *   out_scores [nq, k] float32 descending; out_idx [nq, k] int64 = row of `corpus` (-1 and -inf pad
 *   a shard with fewer than k documents, as faiss does); ties: lower row first.
 *   status [nq] int32: 0 = exact top-k delivered; 1 / 2 = the sampled threshold of that query let
 *   too few / too many candidates through — call again for those queries with m_scale x4 / x0.25
 *   (matchmaker_amd/retrieval.py does).  m_scale = 1 on the first call.
 *   workspace: mm_dot_topk_workspace_bytes(n_docs, nq, k) bytes.  k <= 4096. */
size_t mm_dot_topk_workspace_bytes(int64_t n_docs, int nq, int k);

int mm_dot_topk_fwd(const void* queries, const void* corpus, int64_t n_docs, int nq, int E, int dtype, int k,
                    float m_scale, float* out_scores, int64_t* out_idx, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Final merge of a sharded index: in [nq, n_in] (score, id) rows (e.g. the all-gathered per-shard
 * top-k lists, ids < 0 = padding) -> the k best per row, score descending, input order on ties.
 * n_in <= 16384. */
int mm_topk_merge(const float* in_scores, const int64_t* in_ids, int nq, int n_in, int k,
                  float* out_scores, int64_t* out_ids, void* stream);

/* ------------------------------------------------------------------------------------------
 * IVF list scan: exact inner-product top-k over the inverted lists a query probes (dense retrieval,
 * faiss_index_type: ivf).
 *
 * Replaces: the list scan of FaissIVFIndexer.search      matchmaker/retrieval/faiss_indices.py:106-145
 *           (an inner-product IVF index cloned to the GPUs with co.shard and useFloat16); the coarse
 *           quantiser (centroid assignment, probe selection) is mm_dot_topk_fwd over the centroids.
 *
 *   queries [nq, E], vectors [n_vectors, E]  float16 / bfloat16, E in {128, 256, 384, 512, 768}; the
 *   vectors are stored list by list: list l is the rows list_begin[l] .. list_begin[l + 1] (list_begin
 *   [nlist + 1] int64, non-decreasing; lists may be empty).
 *   probes [nq, nprobe] int32 list numbers, -1 = no list; a list named twice in one row is an error
 *   (the row then never holds more than n_vectors candidates: the surplus is dropped).
 *   out_scores [nq, k] float32 descending = fp32-accumulated inner products of the 16-bit values;
 *   out_rows [nq, k] int64 = row of `vectors`; (-inf, -1) pads a probed union of fewer than k vectors.
 *   The result is the EXACT top-k of the union of the probed lists; equal scores: lower row first.
 *   k <= 4096, nprobe <= 4096, n_vectors and nq * nprobe below 2^31.  Every launch goes to `stream`,
 *   nothing is read back or allocated: the call can be captured into a graph.
 *   workspace: mm_ivf_scan_workspace_bytes(...) bytes = min(nq n_vectors, max(2^28, 2 n_vectors))
 *   floats of candidate scores (at most 1 GiB below 2^27 vectors; the queries are scored in rounds
 *   that fit) + 12 bytes per (query, probe) pair + 20 per query + 12 per list + 4 per 32 vectors. */
size_t mm_ivf_scan_workspace_bytes(int64_t n_vectors, int nlist, int nq, int nprobe, int k);

int mm_ivf_scan_fwd(const void* queries, const void* vectors, const int64_t* list_begin, const int32_t* probes,
                    int64_t n_vectors, int nlist, int nq, int nprobe, int E, int dtype, int k,
                    float* out_scores, int64_t* out_rows, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * k-means building blocks: maximum-inner-product assignment against a centroid table, and the
 * per-list sums of rows (IVF training, TAS-Balanced query clustering).
 *
 * Replaces: FaissDynamicIndexer.prepare / .search_single   matchmaker/retrieval/faiss_indices.py:323-352, 401-428
 *           (faiss k-means over the query vectors; the quantizer's nearest centroid with nprobe = 1)
 *           and the per-query assignment loop               matchmaker/distillation/query_clusterer.py:218-221
 *
 * mm_kmeans_assign
 *   x [n, E], centroids [nlist, E]  float16 / bfloat16 of one dtype, E in {128, 256, 384, 512, 768}.
 *   out_list [n] int32 = the centroid of maximum inner product, out_score [n] float32 = that product
 *   (fp32-accumulated products of the 16-bit values).  Equal scores: the LOWEST centroid number wins
 *   (the "lower row first" rule of mm_dot_topk_fwd); an all-zero row goes to centroid 0.
 *   1 <= nlist <= 65536, 0 <= n < 2^31 (else MM_EUNSUPPORTED, before any launch); n = 0 succeeds
 *   without a launch.  One launch on `stream`: a workgroup reads its 128 rows of x once, walks the
 *   centroid table in blocks of 32 and keeps a running (max, arg) per row in registers; no [n, nlist]
 *   score matrix, no workspace, no status word.  Graph-capturable.
 *
 * mm_kmeans_segment_sum
 *   x [n, E] as above; order [n] int64 = the rows of x list by list; list_begin [nlist + 1] int64,
 *   non-decreasing, lists may be empty (values are clamped to [0, n]).
 *   sums [nlist, E] float32: sums[l] = sum of x[order[j]], list_begin[l] <= j < list_begin[l + 1], in
 *   fp32; a row of zeros for an empty list.  order[j] outside [0, n) is skipped.
 *   Every element of sums is written exactly once, without atomics, and the result is a pure function
 *   of the inputs (bit-equal run to run): a list is cut into chunks of 512 rows, a chunk is summed by
 *   one workgroup in a fixed order, the chunks of a list are added in ascending order.
 *   workspace: mm_kmeans_segment_sum_workspace_bytes(n, nlist, E) bytes = 4 (nlist + 1) + 4 E
 *   (n / 512 + nlist), each rounded up to 256.  Same limits as above.  Three launches on `stream`,
 *   nothing read back: graph-capturable. */
int mm_kmeans_assign(const void* x, const void* centroids, int64_t n, int nlist, int E, int dtype,
                     int32_t* out_list, float* out_score, void* stream);

size_t mm_kmeans_segment_sum_workspace_bytes(int64_t n, int nlist, int E);

int mm_kmeans_segment_sum(const void* x, const int64_t* order, const int64_t* list_begin, int64_t n, int nlist, int E,
                          int dtype, float* sums, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quantized index: anisotropic 4-bit encoder, scan of the codes, exact re-score (dense retrieval,
 * faiss_index_type: scann).
 *
 * Replaces: ScaNNIndexer.index / .search                   matchmaker/retrieval/scann_index.py:24-47
 *           (scann builder .tree(...).score_ah(2, anisotropic_quantization_threshold=0.2)
 *           .reorder(top_n): leaves, 4-bit codes of 2-dimensional blocks, exact re-score).  ScaNN is a
 *           third-party CPU library that is not part of the reference tree: what follows is this
 *           library's restatement, not ScaNN's code path; INTEGRATION.md lists the differences.
 *
 * Common: E in {128, 256, 384, 512, 768}, dtype float16 / bfloat16; S = E / 2 blocks of 2 dimensions;
 *   codebook [S, 16, 2] of the vectors' dtype; codes [n, E / 4] uint8, byte i of a row = the code of
 *   block 2 i in the LOW nibble and of block 2 i + 1 in the high nibble.
 *   decode(codes[i]) = the concatenation of codebook[s][code_s], s = 0 .. S - 1.
 *
 * mm_ah_encode                                              scann_index.py:32-35 (score_ah)
 *   x [n, E], list [n] int32 (the row's leaf; outside [0, nlist): a zero centre), centroids [nlist, E].
 *   Per row, every step ONE rounded fp32 operation, in this order (16-bit values widen exactly):
 *     r_s = x_s - centroids[list]_s per element.
 *     |x|^2: sixteen partial sums, partial c = blocks c, c + 16, ... ascending, per block + x0 x0 then
 *       + x1 x1; the partials are combined by the butterfly t_c += t_(c ^ 8), then ^ 4, ^ 2, ^ 1.
 *       inv = 1 / sqrt(|x|^2), xhat = x inv per element; an all-zero row: xhat = 0 and eta = 1.
 *     per block s and codeword k:  e = (r_s - codebook[s][k]) per element,
 *       n_k = e0 e0 + e1 e1,  t_k = e0 xhat0 + e1 xhat1.
 *     start: blocks ascending, code_s = the k of least n_k (lowest k on equal n_k); p = p + t_code_s,
 *       from p = 0.
 *     then `passes` sweeps, blocks ascending: po = p - t_code_s; u_k = po + t_k;
 *       cost_k = n_k + (eta - 1) (u_k u_k)  (u_k u_k first, then x (eta - 1), then + n_k);
 *       code_s = the k of least cost_k (lowest k on equal cost); p = po + t_code_s.
 *   This is coordinate descent on L = sum_s |e_s|^2 + (eta - 1) (sum_s <e_s, xhat_s>)^2 with the other
 *   blocks' parallel error held fixed; eta = 1 or passes = 0 is plain nearest-codeword quantisation.
 *   eta finite and >= 0, 0 <= passes <= 64.  The result is a pure function of the inputs: no atomics,
 *   one launch on `stream`, no workspace: graph-capturable.  n = 0 succeeds without a launch; n < 2^35 (one workgroup
 *   per 16 rows; more returns MM_EUNSUPPORTED before any launch).
 *
 * mm_ah_scan_fwd                                            scann_index.py:44 (search_batched, AH stage)
 *   queries [nq, E]; codes stored list by list as the vectors of mm_ivf_scan_fwd are (list_begin
 *   [nlist + 1] int64); probes [nq, nprobe] int32, -1 = no list; probe_scores [nq, nprobe] float32.
 *   score(q, i) = probe_scores[q, j] + <queries[q], decode(codes[i])> for row i of the list probes[q, j]
 *   (products of 16-bit values accumulated in fp32, the probe score added last).
 *   out_scores / out_rows [nq, k]: the EXACT top-k of those scores over the probed union, descending,
 *   lower row first on equal scores, (-inf, -1) padded.  Limits, workspace formula and launch
 *   behaviour are mm_ivf_scan_fwd's (k <= 4096, nprobe <= 4096; no read-back, no allocation:
 *   graph-capturable); queries and codes 16-byte aligned.
 *
 * mm_gather_dot                                             scann_index.py:35 (reorder)
 *   queries [nq, E], vectors [n_vectors, E], rows [nq, R] int64.  out [nq, R] float32 =
 *   <queries[q], vectors[rows[q, j]]>, products of 16-bit values accumulated in fp32; -inf where the
 *   row is -1 (or outside [0, n_vectors)).  One launch on `stream`: graph-capturable. */
int mm_ah_encode(const void* x, const int32_t* list, const void* centroids, const void* codebook, int64_t n, int nlist,
                 int E, int dtype, float eta, int passes, uint8_t* codes, void* stream);

size_t mm_ah_scan_workspace_bytes(int64_t n_vectors, int nlist, int nq, int nprobe, int k);

int mm_ah_scan_fwd(const void* queries, const uint8_t* codes, const void* codebook, const int64_t* list_begin,
                   const int32_t* probes, const float* probe_scores, int64_t n_vectors, int nlist, int nq, int nprobe,
                   int E, int dtype, int k, float* out_scores, int64_t* out_rows, void* workspace, size_t workspace_bytes,
                   void* stream);

int mm_gather_dot(const void* queries, const void* vectors, const int64_t* rows, int64_t n_vectors, int nq, int R, int E,
                  int dtype, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Graph search: beam search over a fixed-degree neighbour graph (dense retrieval,
 * faiss_index_type: hnsw).
 *
 * Replaces: FaissHNSWIndexer.search (a CPU index)         matchmaker/retrieval/faiss_indices.py
 *           The graph has ONE level and is built exactly from the shard's k-NN lists
 *           (matchmaker_amd.retrieval.GraphIPIndexer); recall figures are this graph's, not HNSW's.
 *
 *   queries [nq, E], vectors [n, E]  float16 / bfloat16 of one dtype, E in {128, 256, ..., 768};
 *   neighbors [n, M] int32 rows of `vectors`, -1 = no neighbour; entry_rows [nq, n_entry] int32.
 *   Per query: the candidate list L starts as the entry rows (-1, rows outside [0, n) and duplicates
 *   are ignored), scored; they form the visited set; L keeps the best ef entries, score descending,
 *   lower row first on equal scores.  At most max_iters times: the `width` best entries of L that
 *   have not been expanded are marked expanded (none left: stop); each of their neighbours that is
 *   not -1 and not visited is marked visited and scored; the new pairs are merged into L, and L is
 *   cut to ef.  out_scores / out_rows [nq, k] = the first k entries of L (fp32-accumulated inner
 *   products of the 16-bit values; (-inf, -1) where L is shorter).  stats [nq, 2] int32 (may be
 *   NULL) = (iterations run, rows scored).  The visited set is exact (full row numbers, no false
 *   positives), so the result is a function of the inputs alone.
 *   Envelope: 1 <= ef <= 2048, 1 <= k <= ef, 1 <= width <= 8, 1 <= n_entry <= ef, M even in
 *   2 .. 128, 1 <= max_iters <= 65536, n < 2^31; anything else is MM_EUNSUPPORTED before any launch.
 *   The visited table is open-addressed in LDS when 2 (n_entry + max_iters width M) <= 16384
 *   slots; otherwise it is a slice of the workspace per workgroup (at most 1024 workgroups), which
 *   the kernel clears itself.  workspace: mm_graph_search_workspace_bytes(...) (256 bytes for the LDS
 *   placement).  One launch on `stream`, nothing read back or allocated: graph-capturable. */
size_t mm_graph_search_workspace_bytes(int64_t n, int nq, int M, int ef, int width, int n_entry, int max_iters);

int mm_graph_search_fwd(const void* queries, const void* vectors, const int32_t* neighbors, const int32_t* entry_rows,
                        int64_t n, int nq, int E, int dtype, int M, int n_entry, int ef, int width, int max_iters, int k,
                        float* out_scores, int64_t* out_rows, int32_t* stats /* [nq,2] or NULL */,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * PACRR: cosine match matrix -> n-gram convolutions + channel max -> per-row k-max pooling, fused.
 *
 *   cos[i,j]  = <q_i, d_j> / ((|q_i| + 1e-13)(|d_j| + 1e-13))            (allennlp cosine, pacrr.py:78)
 *   path 0    = top-k of cos[i, :]                                         (pacrr.py:86)
 *   path n    = top-k of max_c (b_n[c] + sum_{a,b < n} W_n[c][a][b] cos[i + a, j + b]), n = 2 .. N, with cos = 0 past
 *               the matrix (ConstantPad2d n - 1 columns right, n - 1 rows below; Conv2d; MaxPool3d over the C channels;
 *               pacrr.py:53-58, :88-91)
 *   out[p, i, :] = path 0, path 2, .., path N, k values each, sorted descending   (per_query_results, pacrr.py:97)
 *
 * Replaces: PACRR.forward up to per_query_results   matchmaker/models/pacrr.py:68-97
 *           (the dense layers of :101-112 stay torch; no mask enters, as in the reference)
 *
 *   q [n_queries, Q, E], d [n_pairs, D, E] float32, E a multiple of 4 (16-byte rows); pair p uses query p / pairs_per_query
 *   conv_w    float32, the Conv2d weights of widths n = 2 .. N packed in width order, [C, n, n] each (convolutions.<n-2>.1.weight
 *             without its in-channel axis): C * (4 + 9 + .. + N^2) floats; conv_b [N - 1, C] the biases in the same order.
 *             Both may be NULL when N = 1.
 *   out       [n_pairs, Q, k N] float32
 *   saved_idx optional int32 [n_pairs, Q, k N]: for every output value its document column, | winning channel << 16 on the
 *             conv paths — what mm_pacrr_bwd needs; NULL for inference (same values, bit for bit)
 *   Ties: among equal values the lower column comes first (tie policy); the channel max picks the lowest channel.
 *   Limits: 1 <= Q <= 64, k <= D <= 2048, 4 <= E <= 1024, 1 <= C <= 64, 1 <= N <= 5, 1 <= k <= 32; anything else returns
 *   MM_EUNSUPPORTED before any launch.  The forward needs no workspace (workspace may be NULL); the backward needs
 *   mm_pacrr_workspace_bytes() bytes (0 when N = 1).
 */
size_t mm_pacrr_workspace_bytes(int64_t n_pairs, int Q, int D, int C, int N, int k);

int mm_pacrr_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* out, int32_t* saved_idx,
                 int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Backward of mm_pacrr_fwd (training: train.py:503-524 through pacrr.py:78-97).  The output values are piecewise a linear
 * function of at most k (1 + 4 + .. + N^2) cosines per query row, selected by saved_idx: the backward recomputes those cosines
 * (one dot product each) and pushes grad_out through the convolutions and the cosine's normalisation (the + 1e-13 included).
 *   saved_idx   as written by mm_pacrr_fwd on the SAME inputs; grad_out [n_pairs, Q, k N]
 *   grad_q      [n_pairs, Q, E]: per PAIR (with pairs_per_query > 1 the caller sums each query's rows)
 *   grad_d      [n_pairs, D, E]; both fully written (rows without gradient are zeros)
 *   grad_w      [n_pairs, C * (4 + .. + N^2)], grad_b [n_pairs, (N - 1) C]: per-pair contributions in conv_w / conv_b's packing
 *               (sum over pairs on the host side: deterministic, no atomics); NULL allowed when N = 1
 *   workspace   mm_pacrr_workspace_bytes(n_pairs, Q, D, C, N, k) bytes: the recomputed window cosines */
int mm_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx, const float* grad_out,
                 float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                 int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CO-PACRR: PACRR's cosine -> n-gram convolutions + channel max -> per-row k-max, at four nested document views, with the
 * context similarity of every selected column.
 *
 *   cos, path 0 .. path N    as mm_pacrr_fwd (co_pacrr.py:90, :110-136)
 *   ctx[j]    = cosine(mean_i q_i, (1/6) sum_{t = j .. j+5, t < D} d_t)          (co_pacrr.py:98-101: mean over ALL Q rows;
 *               ConstantPad1d((0, 5)) + AvgPool1d(6, stride 1), :65-68)
 *   view i    = the first min(v_i, D) columns of a path, v_i = int(U * f_i), f = 0.25 / 0.5 / 0.75 / 1 (:74), computed by the
 *               caller with Python's int(); columns at or past min(v_3, D) enter no list but still feed the conv halo and the
 *               context windows of earlier columns
 *   out[p, i, path, :] = top-k of view 0, .., view 3 (k values each, sorted descending), then ctx[column] of those 4k slots
 *               in slot order (:111-126, :148-151); paths 0, 2, .., N                 (per_query_results, co_pacrr.py:158)
 *
 * Replaces: CO_PACRR.forward up to per_query_results   matchmaker/models/co_pacrr.py:79-158
 *           (the idf softmax and the query shuffle of :160-166 are dead code there; the dense layers of :168-179 stay torch)
 *
 *   q, d, conv_w, conv_b  as mm_pacrr_fwd
 *   view0..view3          the four view sizes, ascending (MM_EINVAL otherwise)
 *   out       [n_pairs, Q, 8 k N] float32
 *   saved_idx optional int32 [n_pairs, Q, N, 4 k]: document column | winning channel << 16 of every VALUE slot (the context
 *             slots share them) — what mm_co_pacrr_bwd needs; NULL for inference (same values, bit for bit)
 *   Ties: descending, lower column first, lowest channel: among equal values this also decides which
 *   ctx[column] is gathered.
 *   Limits: 1 <= Q <= 64, k <= D <= 2048, 4 <= E <= 1024 (a multiple of 4), 1 <= C <= 64, 1 <= N <= 5, 1 <= k <= 8,
 *   view0 >= k (torch.topk raises in the reference otherwise); anything else returns MM_EUNSUPPORTED before any launch.
 *   The forward needs no workspace.
 */
size_t mm_co_pacrr_workspace_bytes(int64_t n_pairs, int Q, int D, int E, int C, int N, int k);

int mm_co_pacrr_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* out, int32_t* saved_idx,
                    int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                    int view0, int view1, int view2, int view3, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of mm_co_pacrr_fwd (training: train.py:503-524 through co_pacrr.py:90-158), one launch.
 *   value slots    as mm_pacrr_bwd over the 4k slots of every (row, path); a column chosen by several views adds up
 *   context slots  d(loss)/d(ctx[col]) through the cosine Jacobian of (qctx, dctx[col]): every query row receives 1/Q of
 *                  d(loss)/d(qctx), document rows col .. min(col + 5, D - 1) 1/6 of d(loss)/d(dctx[col])
 *   saved_idx, grad_out [n_pairs, Q, 8 k N]; grad_q [n_pairs, Q, E] per PAIR; grad_d [n_pairs, D, E]; grad_w / grad_b per-pair
 *   contributions as mm_pacrr_bwd (NULL allowed when N = 1)
 *   workspace   mm_co_pacrr_workspace_bytes(n_pairs, Q, D, E, C, N, k) bytes (never 0 for n_pairs > 0) */
int mm_co_pacrr_bwd(const float* q, const float* d, const float* conv_w, const int32_t* saved_idx, const float* grad_out,
                    float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                    int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int C, int N, int k,
                    int view0, int view1, int view2, int view3, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * DRMM: cosine match matrix -> per query token a histogram of its cosines over the document -> (optionally) the scoring head.
 *
 *   cos[i,j]   = <q_i, d_j> / ((|q_i| + 1e-13)(|d_j| + 1e-13))               (allennlp cosine, drmm.py:66; exact-fp32 MFMA)
 *   hist[p,i,:] = torch.histc(cos[i, :], bins, min = -1, max = 1)             (drmm.py:71-74): an element with cos < -1 or
 *                cos > 1 is dropped, otherwise it counts in bin min(int((cos + 1) / 2 * bins), bins - 1), evaluated in fp32.
 *                No mask enters: zero rows (padding, OOV) give cos = 0 and count in bin bins / 2.
 *   score[p]   = sum_i gate[g, i] * tanh(w2 . tanh(W1 log1p(hist[p,i,:]) + b1) + b2)   (drmm.py:77, :88; the head is
 *                matching_classifier, the gate the masked softmax of query_gate, computed by the caller)
 *
 * Replaces: DRMM.forward   matchmaker/models/drmm.py:66-91   (cosine, the .cpu() copy, the per-row histc loop, the copy back,
 *           log1p + matching_classifier + the gated sum; the query gate of :82-83 stays torch)
 *
 *   q [n_queries, Q, E], d [n_pairs, D, E] float32, E a multiple of 4; pair p uses query p / pairs_per_query
 *   d_len    optional int32 [n_pairs]: document rows at or past d_len[p] are taken as zero rows without being read (their
 *            count goes to bin bins / 2); NULL = every row is read.  Bit-equal to the full computation when those rows are zero.
 *   hist     optional float32 [n_pairs, Q, bins] (raw counts); score optional float32 [n_pairs]; at least one of the two
 *   gate     float32 [n_pairs, Q] when gate_per_pair = 1, else [n_queries, Q]; W1 [bins, bins] row-major (Linear.weight),
 *            b1 [bins], w2 [bins], b2 [1]: needed with score only
 *   clamp    0 = the reference (cosines that round above 1 are dropped, as histc does); 1 = clamp the cosine into [-1, 1]
 *            before binning (a deliberate deviation: exact matches always count in the last bin)
 *   No gradient: the histogram is piecewise constant in q and d.  Deterministic (no atomics).
 *   Limits: 1 <= Q <= 64, 1 <= D <= 65535, 4 <= E <= 1024 (a multiple of 4), 1 <= bins <= 16; anything else returns
 *   MM_EUNSUPPORTED before any launch; NULL or inconsistent arguments return MM_EINVAL.  No workspace is needed
 *   (mm_drmm_workspace_bytes returns 0; workspace may be NULL).
 */
size_t mm_drmm_workspace_bytes(int64_t n_pairs, int Q, int D, int E, int bins);

int mm_drmm_fwd(const float* q, const float* d, const int32_t* d_len, float* hist, float* score, const float* gate,
                int gate_per_pair, const float* W1, const float* b1, const float* w2, const float* b2,
                int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int bins, int clamp,
                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * MatchPyramid: cosine match matrix -> L x (zero pad, Conv2d, ReLU, AdaptiveMaxPool2d) -> flattened features, one launch.
 *
 *   x_0[0,i,j]  = <q_i, d_j> / ((|q_i| + 1e-13)(|d_j| + 1e-13))           (allennlp cosine, matchpyramid.py:74; a zero row
 *                 gives exactly 0; no mask enters: padded document columns are convolved and pooled like real ones)
 *   layer l     : x_l [C_{l-1}, H, W] is padded with k0 - 1 zero COLUMNS on the right and k1 - 1 zero ROWS below
 *                 (ConstantPad2d((0, k[0] - 1, 0, k[1] - 1)), :50) and convolved with a k0-row x k1-column kernel
 *                 (Conv2d(kernel_size = k), :51): the conv output is (H + k1 - k0) x (W + k0 - k1); the bias is added at
 *                 every output position; ReLU (:52); AdaptiveMaxPool2d((ph, pw)) (:53): output i of an axis of length n
 *                 covers [floor(i n / ph), ceil((i + 1) n / ph)) (windows overlap, ph > n is legal)
 *   features[p] = x_L flattened channel-major, C_L ph_L pw_L floats             (conv_result.view(B, -1), :92)
 *
 * Replaces: MatchPyramid.forward up to conv_result_flat   matchmaker/models/matchpyramid.py:74-92
 *           (the three dense layers of :99-101 stay torch).  Forward only.
 *
 *   q [n_queries, Q, E], d [n_pairs, D, E] float32, E a multiple of 4; pair p uses query p / pairs_per_query
 *   layers    HOST array int32 [n_layers, 5]: (C_l, k0, k1, ph, pw) per layer
 *   conv_w    float32, the Conv2d weights [C_l, C_{l-1}, k0, k1] of the layers packed in order (C_0's input is 1 channel);
 *             conv_b the biases packed in the same order
 *   features  [n_pairs, C_L ph_L pw_L] float32
 *   workspace mm_matchpyramid_workspace_bytes(n_pairs, Q, D, n_layers, layers) bytes (0 when every activation plane fits the
 *             LDS): one slot per resident workgroup for the planes that do not fit, at most 256 MiB however large n_pairs is
 *             (the workgroups walk the batch).  Returns 0 for an unsupported shape as well.
 *   Exact fp32 (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32), no atomics, bit-reproducible; a pair's result does not
 *   depend on the rest of the batch.  MM_MP_GENERIC=1 runs the generic kernel at the reference config too (same bits).
 *   Limits: 1 <= Q <= 64, 1 <= D <= 2048, 4 <= E <= 1024 (a multiple of 4), 1 <= n_layers <= 8, 1 <= C_l <= 32, kernel
 *   sides 1 .. 5, 1 <= ph <= 64, 1 <= pw <= 256, every conv output at least 1 x 1; anything else returns MM_EUNSUPPORTED
 *   before any launch; NULL pointers or pairs_per_query < 1 return MM_EINVAL.
 */
size_t mm_matchpyramid_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers);

int mm_matchpyramid_fwd(const float* q, const float* d, const float* conv_w, const float* conv_b, float* features,
                        int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int n_layers, const int32_t* layers,
                        void* workspace, size_t workspace_bytes, void* stream);

/* MatchPyramid, training.  mm_matchpyramid_fwd_save is the forward above (the same instruction sequence for the values, in both
 * kernel instantiations: `features` has the bits mm_matchpyramid_fwd gives) that additionally writes the state the backward
 * routes through, so that no conv output is ever recomputed:
 *
 *   pooled  [n_pairs, S] float32, S = sum_l C_l ph_l pw_l: per pair, layer after layer, the layer's pooled output
 *           [C_l, ph_l, pw_l] (the next layer's input; the last layer's block equals features[p])
 *   argmax  [n_pairs, S] int32, the same layout: for every pooled element the flat index row * Wo + col into its channel's
 *           conv-output plane (Ho x Wo = (H + k1 - k0) x (W + k0 - k1)), the convention of
 *           F.adaptive_max_pool2d(return_indices=True).
 *   Tie rule: the FIRST maximum in row-major order of the window, i.e. among equal candidates the lowest flat index, as torch
 *           does on CPU and GPU.  The maximum is taken after ReLU, so a window without a positive value reports its first
 *           element (and carries no gradient).  Exact ties are routine: conv windows that see only zeros equal the bias.
 *   workspace mm_matchpyramid_fwd_save_workspace_bytes(..) bytes (its own size query: the kernel keeps one row-index tile per
 *           wavefront in LDS, which can move a plane from the LDS to the workspace; that changes no bit).
 *
 * mm_matchpyramid_bwd: the gradients of sum(features * grad_features) from that state.
 *
 *   q, d, conv_w, layers   as in the forward (conv_b is not needed)
 *   pooled, argmax         as written by mm_matchpyramid_fwd_save on the same inputs (an index outside its plane is clamped)
 *   grad_features          [n_pairs, C_L ph_L pw_L] float32
 *   grad_q  [n_pairs, Q, E] PER PAIR (the caller adds the pairs of a query when pairs_per_query > 1), grad_d [n_pairs, D, E]
 *   grad_w, grad_b         in the packed layout of conv_w / conv_b, summed over the batch
 *   Per pair from the last layer down: the conv-output gradient has one entry per pooled element (g_e at argmax_e where
 *   pooled_e > 0: ReLU's backward, 0 at 0; entries that share a position add); grad_b[c] += sum_e g_e;
 *   grad_w[c, k] += sum_e g_e In[argmax_e + k], In the saved pooled output of the layer below (the recomputed cosine plane for
 *   layer 0) with the forward's zero padding; the input gradient is the transposed convolution, computed as a gather; then the
 *   cosine's backward through x / (|x| + 1e-13) (a zero row takes only g / (|x| + 1e-13): torch's zero subgradient of the norm).
 *   Exact fp32 (fma chains in fixed orders), NO floating-point atomics: two calls give the same bits, and grad_q / grad_d of a
 *   pair do not depend on the rest of the batch.  A persistent grid; the weight / bias gradients accumulate per workgroup
 *   over its pairs in pair order and a second small launch adds the workgroups' partials in workgroup order.
 *   workspace mm_matchpyramid_bwd_workspace_bytes(..) bytes: one slot per resident workgroup, at most 256 MiB however large
 *   n_pairs is.  The size queries return 0 for an unsupported shape.
 *   Limits and errors: the forward's envelope; anything else returns MM_EUNSUPPORTED before any launch; NULL pointers or
 *   pairs_per_query < 1 return MM_EINVAL; n_pairs = 0 writes nothing.
 */
size_t mm_matchpyramid_fwd_save_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers);

int mm_matchpyramid_fwd_save(const float* q, const float* d, const float* conv_w, const float* conv_b, float* features,
                             float* pooled, int32_t* argmax, int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E,
                             int n_layers, const int32_t* layers, void* workspace, size_t workspace_bytes, void* stream);

size_t mm_matchpyramid_bwd_workspace_bytes(int64_t n_pairs, int Q, int D, int n_layers, const int32_t* layers);

int mm_matchpyramid_bwd(const float* q, const float* d, const float* conv_w, const float* pooled, const int32_t* argmax,
                        const float* grad_features, float* grad_q, float* grad_d, float* grad_w, float* grad_b,
                        int64_t n_pairs, int64_t pairs_per_query, int Q, int D, int E, int n_layers, const int32_t* layers,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * ColBERT retrieval, candidate generation: token hits -> per query the documents that own a hit, with their row ranges.
 *
 * Replaces: the step between the token search and the aggregate of the ColBERT retrieval branch
 *           matchmaker/dense_retrieval.py:391-412 (`current_ids`, read there before it is assigned, is meant to be the set
 *           of documents of the token hits); the ranges feed mm_maxsim_ragged_fwd = forward_aggregation,
 *           matchmaker/models/colbert.py:100-112.
 *
 *   hit_rows         [nq, H] int64 rows of the token matrix (the out_idx / out_rows of the token search); -1 = no hit
 *   doc_begin_sorted, doc_end_sorted [n_docs] int64: the documents' row ranges sorted by (begin, end); non-empty ranges are
 *                    disjoint; a zero-length range may share its begin with a document but not lie inside one
 *   doc_of_sorted    [n_docs] int32: the document index (position in the store's seq_ids) of every sorted range, a permutation
 *   A hit belongs to document j when begin[j] <= row < end[j]; hits of -1, rows outside [0, T) and rows no document owns are
 *   dropped; a zero-length document owns nothing.
 *   cand_doc   [nq, C_cap] int32: the distinct owning documents of the query, ASCENDING by document index, then -1
 *   cand_begin, cand_end [nq, C_cap] int64: their row ranges, then (0, 0): with pairs_per_query = C_cap they are the doc_begin /
 *              doc_end of mm_maxsim_ragged_fwd (an empty range costs nothing there)
 *   cand_count [nq] int32: candidates of the query
 *   One workgroup per query: binary search per hit, two int32 bitonic sorts in LDS, prefix sum, compaction.  Every output
 *   element is written exactly once; no atomics, nothing read back or allocated: graph-capturable and bit-reproducible.
 *   Limits: 1 <= H <= 16384, 1 <= n_docs < 2^31, T >= 0, C_cap >= min(H, n_docs); anything else returns MM_EUNSUPPORTED before
 *   any launch; NULL pointers or nq < 0 return MM_EINVAL.  Whatever the hit values are, memory accesses stay in bounds.
 *   workspace: mm_colbert_candidates_workspace_bytes(nq, H) bytes = 4 bytes per hit slot of the queries in flight.
 */
size_t mm_colbert_candidates_workspace_bytes(int nq, int H);

int mm_colbert_candidates(const int64_t* hit_rows, const int64_t* doc_begin_sorted, const int64_t* doc_end_sorted,
                          const int32_t* doc_of_sorted, int64_t n_docs, int64_t T, int nq, int H, int C_cap,
                          int32_t* cand_doc, int64_t* cand_begin, int64_t* cand_end, int32_t* cand_count,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp8 ColBERT token store: row quantiser and ragged MaxSim over the quantised rows (additive: MM_ABI_VERSION unchanged).
 *
 * Format: codes [T, E] uint8 = OCP e4m3fn bytes (not the MI300 fnuz encoding), scales [T] float32 = one power of two per
 *   token row.  For a row x taken as float32 values with a = max_k |x_k|:
 *     s      = 2^clamp(floor(log2 a) - 7, -126, 120), or 1.0 when a == 0
 *     code_k = RNE_e4m3fn(x_k * (1 / s))            (the multiply is exact; the scaled maximum lies in [128, 256), so
 *                                                    nothing saturates and the NaN patterns 0x7f / 0xff never appear)
 *   and the row's value is deq(code_k) * s, an exact product.  |deq * s - x| <= 2^-4 |x| + 2^-10 s per element.  Both
 *   zeros (0x00, 0x80) are one value.  Non-finite input is the caller's error: the codes and scale of such a row are
 *   unspecified.
 *
 * mm_fp8_quantize_rows: x [n_rows, E] of `dtype` (MM_F32 / MM_F16 / MM_BF16) -> codes, scales.  One 16-lane group per row:
 *   row maximum, then convert and store.  No atomics, every output byte is written, two calls give the same bits.
 *   E % 16 != 0 returns MM_EUNSUPPORTED; x and codes 16-byte aligned; n_rows = 0 succeeds.  n_rows <= 2^35 - 16 (one
 *   workgroup per 16 rows, at most 2^31 - 1 of them; more returns MM_EUNSUPPORTED before any launch); every offset is
 *   64-bit, so the input and the codes may cross 2^32 bytes.
 *
 * mm_maxsim_ragged_fp8_fwd: mm_maxsim_ragged_fwd over such a store,
 *     out[p] = sum_{i, q_mask} max_{t in [doc_begin[p], doc_end[p])} ( scales[t] * sum_k q[i,k] * deq(codes[t,k]) )
 *   q [n_queries, Q, E] is MM_F16 or MM_BF16 (MM_F32 returns MM_EUNSUPPORTED) and is NOT quantised: the codes are
 *   converted to q's type in registers (exact) and multiplied on the 16-bit MFMA, so every product is exact, the
 *   similarities accumulate in fp32 and the scale multiplies the finished dot product in fp32 (exact) before the maximum.
 *   pair p uses query p / pairs_per_query; q_mask as for mm_maxsim_fwd; an empty range scores -1000 per live query token;
 *   flags MM_SIM_ROUND / MM_SUM_ROUND round to q's type exactly as in mm_maxsim_ragged_fwd.  out [n_pairs] float32.
 *   E in {128, 256, 384, 512, 768} with Q <= 64 streams the rows through LDS; other E % 16 == 0 or larger Q take a
 *   one-wavefront-per-pair kernel; E % 16 != 0 returns MM_EUNSUPPORTED.  The ranges must lie inside [0, T): the kernels do
 *   not know T.
 */
int mm_fp8_quantize_rows(const void* x, int64_t n_rows, int E, int dtype, uint8_t* codes, float* scales, void* stream);

size_t mm_maxsim_ragged_fp8_workspace_bytes(int64_t n_pairs, int64_t pairs_per_query, int Q, int q_mask_kind);

int mm_maxsim_ragged_fp8_fwd(const void* q, const uint8_t* codes, const float* scales, const int64_t* doc_begin,
                             const int64_t* doc_end, const void* q_mask, int q_mask_kind, float* out,
                             int64_t n_pairs, int64_t pairs_per_query, int Q, int E, int q_dtype, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp8 token search: mm_dot_topk_fwd over an fp8 store (additive: MM_ABI_VERSION unchanged).
 *
 * Replaces, for a store held as codes + scales, the same reference lines as mm_dot_topk_fwd: the flat inner-product index
 *           FaissBaseIndexer.search                      matchmaker/retrieval/faiss_indices.py:22-36
 *           called per query batch at                    matchmaker/dense_retrieval.py:391
 *
 *   score[q, t] = scales[t] * sum_k queries[q, k] * deq(codes[t, k])
 *   queries [nq, E] MM_F16 or MM_BF16 (MM_F32 returns MM_EUNSUPPORTED) and NOT quantised; codes [n_rows, E] uint8 (OCP
 *   e4m3fn) + scales [n_rows] float32 as mm_fp8_quantize_rows writes them; E in {128, 256, 384, 512, 768}.  The codes are
 *   converted to the query's type in registers (exact) and multiplied on the 16-bit MFMA: every product is exact, the sum
 *   is fp32, and the power-of-two scale multiplies the finished dot product (exact) before the threshold test.
 *   out_scores / out_idx / the tie rule (score descending, lower row first) / the (-inf, -1) padding when n_rows < k /
 *   status 0, 1, 2 with m_scale / k <= 4096 / n_rows < 2^31 are mm_dot_topk_fwd's.  The sample pass and the filter pass
 *   give the same bits for one (query, row) pair.  queries and codes 16-byte aligned, scales 4-byte aligned.  No load uses
 *   a row index >= n_rows.
 *   workspace: mm_dot_topk_fp8_workspace_bytes(n_rows, nq, k) bytes. */
size_t mm_dot_topk_fp8_workspace_bytes(int64_t n_rows, int nq, int k);

int mm_dot_topk_fp8_fwd(const void* queries, const uint8_t* codes, const float* scales, int64_t n_rows, int nq, int E,
                        int q_dtype, int k, float m_scale, float* out_scores, int64_t* out_idx, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * fp8 IVF list scan: mm_ivf_scan_fwd over lists held as an fp8 store (additive: MM_ABI_VERSION unchanged).
 *
 * Replaces, for lists held as codes + scales, the same reference lines as mm_ivf_scan_fwd:
 *           the list scan of FaissIVFIndexer.search      matchmaker/retrieval/faiss_indices.py:106-145
 *           (the coarse quantiser stays mm_dot_topk_fwd over the 16-bit centroids).
 *
 *   score(q, t) = scales[t] * sum_k queries[q, k] * deq(codes[t, k])   for every row t of the lists named in probes[q, :]
 *   codes [n_rows, E] uint8 (OCP e4m3fn) + scales [n_rows] float32 powers of two as mm_fp8_quantize_rows writes them,
 *   stored list by list: list l is the rows list_begin[l] .. list_begin[l + 1] (list_begin [nlist + 1] int64, non-decreasing;
 *   lists may be empty).  queries [nq, E] MM_F16 or MM_BF16 (MM_F32 returns MM_EUNSUPPORTED) and NOT quantised;
 *   E in {128, 256, 384, 512, 768}.  The codes are converted to the query's type in registers (exact) and multiplied on
 *   the 16-bit MFMA: every product is exact, the sum is fp32, and the row's scale multiplies the finished dot product
 *   (exact) before the score is written.
 *   probes / out_scores / out_rows (rows of `codes`) / the EXACT top-k of the probed union / the tie rule (score
 *   descending, lower row first) / the (-inf, -1) padding / k <= 4096, nprobe <= 4096, n_rows and nq * nprobe below 2^31 /
 *   one enqueue on `stream` with no read-back and no allocation (graph-capturable as a single chain) are
 *   mm_ivf_scan_fwd's.  queries and codes 16-byte aligned, scales 4-byte aligned.  No load uses a row index >= n_rows:
 *   rows past the end of a list's partial last 32-row block are clamped into the list, codes and scale alike, and never
 *   written.  No floating-point atomics in scoring: two calls give the same bits.
 *   workspace: mm_ivf_scan_fp8_workspace_bytes(...) = mm_ivf_scan_workspace_bytes(n_rows, nlist, nq, nprobe, k) bytes; one
 *   byte less returns MM_EWORKSPACE with nothing written. */
size_t mm_ivf_scan_fp8_workspace_bytes(int64_t n_rows, int nlist, int nq, int nprobe, int k);

int mm_ivf_scan_fp8_fwd(const void* queries, const uint8_t* codes, const float* scales,
                        const int64_t* list_begin, const int32_t* probes,
                        int64_t n_rows, int nlist, int nq, int nprobe, int E, int q_dtype, int k,
                        float* out_scores, int64_t* out_rows,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * ColBERT store writer: a batch of encoder output -> its token rows appended to a resident store (additive:
 * MM_ABI_VERSION unchanged).
 *
 * Replaces: the host half of the encode loop, matchmaker/dense_retrieval.py:232-265 — the copy of the padded batch to the
 *           CPU (:232), the per-document removal of all-zero rows (:244), the copy into the memmap (:259-261) and
 *           doc_infos[seq_id] = (file, start, end) (:264) — for a store that stays on the device.
 *
 *   x [n_docs, D, E] of `dtype` (MM_F32 / MM_F16 / MM_BF16), contiguous, 16-byte aligned.
 *   Row (b, j) is KEPT iff one of its elements has a non-zero magnitude (bits & ~sign != 0: -0.0 counts as zero).  For
 *   finite input that is the reference's `abs().sum(-1) > 0` in the store's dtype.  Non-finite input is the caller's error,
 *   as for mm_fp8_quantize_rows (a row holding NaN is dropped by the reference and kept here).
 *   flags & MM_STORE_KEEP_ZERO_ROWS keeps every row: the reference's one-vector-per-document case (dim_count == 1,
 *   :243-246), called with D = 1.
 *   Kept rows are written back to back in document order, then token order, from store row fill[0] on:
 *     doc_begin[b] = fill_in + (kept rows of the documents < b),  doc_end[b] = doc_begin[b] + kept(b)
 *   (an empty range for a document without a kept row), and fill[0] becomes fill_in + the batch's kept rows.
 *   rows_out [capacity, E] of out_dtype (or NULL): out_dtype == dtype copies the bits; MM_F32 -> MM_F16 / MM_BF16 rounds to
 *     nearest even with overflow to +-inf (numpy's and torch's cast); MM_F16 / MM_BF16 -> MM_F32 widens exactly;
 *     MM_F16 <-> MM_BF16 returns MM_EUNSUPPORTED.
 *   codes_out [capacity, E] + scales_out [capacity] (or both NULL): exactly mm_fp8_quantize_rows of the kept rows in `dtype`
 *     (one copy of the device code serves both).  Either output or both may be given; neither returns MM_EINVAL.
 *   Capacity is all or nothing per batch: if fill_in + kept > capacity the call writes no row and no doc_begin / doc_end,
 *   leaves fill[0] unchanged and sets status[0] = 1.  status is sticky: when it is non-zero on entry the call does nothing.
 *   No store uses a row index >= capacity, no load reads outside x.  Store rows below fill_in and from the new fill[0] on are
 *   left as they were (rows_out, codes_out and scales_out alike): the call owns rows fill_in .. fill_in + kept - 1 only.
 *   fill [1] int64, status [1] int32, doc_begin / doc_end [n_docs] int64 are DEVICE memory: appends chain through fill with
 *   no read-back.  Three launches on `stream` (row flags by wavefront ballot; a one-workgroup scan with the capacity test;
 *   scatter), no allocation, no host synchronisation, no atomics and no workgroup waiting on another: graph-capturable as a
 *   single chain, and two runs give the same bits.
 *   Limits: E * sizeof(dtype) % 16 != 0, or an fp8 output with E % 16 != 0, returns MM_EUNSUPPORTED; n_docs * D < 2^31 (the
 *   kernels have no separate limit for D or n_docs; the scan is one workgroup, so its time grows with n_docs * D / 64);
 *   n_docs = 0 succeeds and changes nothing.
 *   workspace: mm_store_append_workspace_bytes(n_docs, D) bytes (12 bytes per 64 rows of the batch); one byte less returns
 *   MM_EWORKSPACE with nothing written.
 */
#define MM_STORE_KEEP_ZERO_ROWS 1

size_t mm_store_append_workspace_bytes(int n_docs, int D);

int mm_store_append(const void* x, int n_docs, int D, int E, int dtype, int flags,
                    void* rows_out, int out_dtype, uint8_t* codes_out, float* scales_out, int64_t capacity,
                    int64_t* fill, int64_t* doc_begin, int64_t* doc_end, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ranking and IR metrics: scores on the device -> rank order -> the per-query quantities of the reference's metric
 * dicts (additive: MM_ABI_VERSION unchanged).  None of the three entries needs a workspace, so there is no size query.
 * All run on `stream` with no allocation, no read-back and no atomics: graph-capturable, two calls give the same bits.
 *
 * Segments: seg_begin [nq + 1] int64, ascending, DEVICE memory; query s owns rows [seg_begin[s], seg_begin[s + 1]).
 * Every bound is clamped into [0, n_rows] on the device, so no load or store uses a row outside [0, n_rows) whatever
 * seg_begin (or, for the metric entries, `order`) holds.  Empty segments are legal anywhere.  n_rows < 2^31.
 *
 * mm_segment_rank_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/utils/core_metrics.py:502-511 (unrolled_to_ranked_result: `sorted(..., key=score, reverse=True)`
 *           per query), as called from eval.py:264-320, 395-407 and dense_retrieval.py:447-448.
 *   scores [n_rows] of `dtype` (MM_F32 / MM_F16 / MM_BF16; 16-bit scores are widened exactly to fp32 before comparison).
 *   order [n_rows] int32: order[seg_begin[s] + r] = the global row with rank r + 1 in query s.
 *   Rule: higher score first; equal scores keep arrival order (the sort is stable); -0.0 == +0.0.  STATED CHOICE: every
 *   NaN ranks after everything else, -inf included, NaNs among themselves in arrival order (Python's sorted() gives an
 *   order that depends on the arrival positions there; the reference never scores NaN on purpose).
 *   max_len: the caller's upper bound on the segment lengths, 0 .. MM_RANK_MAX_LEN.  max_len > MM_RANK_MAX_LEN returns
 *   MM_EUNSUPPORTED before any launch (8,192 rows: 64 KiB of 64-bit keys in LDS, two workgroups per CU beside it).  A
 *   segment that is longer than max_len all the same is written in arrival order.
 *   Segments of <= 64 rows take one wavefront each (four per workgroup), longer ones one workgroup each.
 *   nq = 0 or n_rows = 0 succeeds and writes nothing.
 */
#define MM_RANK_MAX_LEN 8192
#define MM_RANK_MAX_CUTOFFS 8
#define MM_RANK_NOT_JUDGED (-2147483647 - 1)   /* grade of a row whose document is not in the query's qrels (INT32_MIN) */

int mm_segment_rank_fwd(const void* scores, int dtype, const int64_t* seg_begin, int64_t n_rows, int nq, int max_len,
                        int32_t* order, void* stream);

/* mm_rank_metrics_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: the per-query body of calculate_metrics_plain (core_metrics.py:380-461; threshold = INT32_MAX, cand_pos =
 *           NULL) and of calculate_metrics_single_candidate_threshold (:228-327; cand_pos + threshold).
 *   Per row (DEVICE): order [n_rows] int32 (mm_segment_rank_fwd's); grade [n_rows] int32 = the qrels grade of the row's
 *   document for its query, MM_RANK_NOT_JUDGED when it is not in the query's qrels; cand_pos [n_rows] int32 or NULL = the
 *   1-based first-stage rank.  Rows with cand_pos > threshold are dropped and the rest renumbered 1, 2, ... (merged_ranks,
 *   :252-254).  A row is binary-relevant when it is judged and grade >= binarization_point.
 *   Cutoffs (HOST arrays, read before the launch): mrr_cutoffs [n_mrr], ndcg_cutoffs [n_ndcg], each 0 .. 8 entries >= 1;
 *   map_cutoff >= 1.
 *   Per query (DEVICE, computed from the qrels alone): binary_num_relevant [nq] int32; idcg [nq, n_ndcg] float64 = the
 *   reference's `idcg.sum()` (:447 / :318 / :164); log2_table [n_log2] float64, log2_table[r] = numpy's log2(1 + r), n_log2 >
 *   every nDCG cutoff (so the divisors are the reference's bits and the device evaluates no logarithm).
 *   Outputs per query (DEVICE): first_rank [nq] int32 = the rank of the first surviving binary-relevant row, 0 without one;
 *   hits [nq, n_mrr] int32 = surviving binary-relevant rows with rank <= cutoff; ap [nq] float64 (:405-407 / :271-273;
 *   0 when no row of the list is binary-relevant); ndcg [nq, n_ndcg] float64 (:444-461; 0 when no row of the list is
 *   judged, NaN exactly where the reference divides 0 by 0: a list with a judged row for a query whose judged documents
 *   all have grade 0).  RR, recall and the rank at a cutoff follow from first_rank, hits and binary_num_relevant.
 *   One wavefront per query; float64 sums of correctly rounded terms, added in rank order.
 */
int mm_rank_metrics_fwd(const int32_t* order, const int64_t* seg_begin, const int32_t* grade, const int32_t* cand_pos,
                        int64_t n_rows, int nq, int threshold, double binarization_point,
                        const int32_t* mrr_cutoffs, int n_mrr, const int32_t* ndcg_cutoffs, int n_ndcg, int map_cutoff,
                        const int32_t* binary_num_relevant, const double* idcg, const double* log2_table, int n_log2,
                        int32_t* first_rank, int32_t* hits, double* ap, double* ndcg, void* stream);

/* mm_rank_metrics_depth_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: the per-query body of calculate_metrics_along_candidate_depth (core_metrics.py:42-173) for every candidate
 *           threshold t = 1 .. hi at once, without its [hi, hi] mask (:40, :88-92).
 *   Inputs as mm_rank_metrics_fwd, cand_pos required; 1 <= hi <= MM_RANK_MAX_LEN (more returns MM_EUNSUPPORTED before any
 *   launch).  Outputs first_rank [nq, hi] int32, hits [nq, hi, n_mrr] int32, ap [nq, hi] float64, ndcg [nq, hi, n_ndcg]
 *   float64: entry t - 1 is what mm_rank_metrics_fwd gives with threshold = t (sums in rank order).
 *   A list shorter than hi behaves as padded (:58-85).  The reference refuses a list longer than hi (a broadcast error) and
 *   so must the caller: the kernel reads the first hi rows of such a list only.
 *   One lane per (query, threshold) walks the query's (cand_pos, grade) pairs, staged in LDS in rank order.
 */
int mm_rank_metrics_depth_fwd(const int32_t* order, const int64_t* seg_begin, const int32_t* grade, const int32_t* cand_pos,
                              int64_t n_rows, int nq, int hi, double binarization_point,
                              const int32_t* mrr_cutoffs, int n_mrr, const int32_t* ndcg_cutoffs, int n_ndcg, int map_cutoff,
                              const int32_t* binary_num_relevant, const double* idcg, const double* log2_table, int n_log2,
                              int32_t* first_rank, int32_t* hits, double* ap, double* ndcg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training losses: the reduced loss and its gradient with respect to the scores in ONE call, so that autograd's backward
 * is a single multiply by grad_output (additive: MM_ABI_VERSION unchanged).  Both entries run on `stream` with no
 * allocation, no read-back and no atomics, vector stores only, one linear chain of launches: graph-capturable, two calls
 * give the same bits.  Scores are MM_F32 / MM_F16 / MM_BF16 and are widened exactly to fp32; labels are fp32.  Per-element
 * terms of the list kinds are fp32 with the accurate library functions (expf, log1pf, logf, exp2f), those of the pair kinds
 * float64 (sigmoid(x) - y and KLDiv's terms cancel: fp32 terms miss one 16-bit ulp of the gradient / four fp32 ulps of the
 * loss there); every sum is float64 in a fixed order, rounded once to fp32; each gradient is rounded once to the scores' dtype.  STATED CHOICE: 16-bit
 * scores are computed from their exact widened values (the reference rounds pos - neg to 16 bits first).  STATED CHOICE:
 * inputs are never modified (lambdarank.py:66-67 writes -inf into y_pred / y_true in place).  Every output element is
 * written on every successful call, zeros for padded entries and for lists with no counted pair included.
 *
 * mm_pair_loss_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/losses/ranknet.py:15-16, matchmaker/losses/all.py:48, matchmaker/losses/msmargin.py:13,
 *           matchmaker/losses/teacher_mse_pointwise.py:13-14, matchmaker/losses/teacher_kldiv_pointwise.py:13-14,
 *           matchmaker/losses/teacher_ranknetweighted.py:16-18, matchmaker/losses/teacher_mse_ranknet.py:13-15
 *   pos, neg [n] of `dtype`; a, b [n] fp32 labels (b is not read by MM_PAIR_RANKNET and MM_PAIR_MARGIN and may be NULL
 *   there); loss [1] fp32 = the MEAN over n of the per-element loss; grad_pos, grad_neg [n] of `dtype` = d loss / d pos,
 *   d loss / d neg (the 1 / n included).  With x = pos - neg, sg = sigmoid, sp(x) = max(x, 0) + log1p(exp(-|x|)):
 *     MM_PAIR_RANKNET          a = target y.  sp(x) - x y;  dx = sg(x) - y                      (BCEWithLogitsLoss)
 *     MM_PAIR_MARGIN           a = label y.   max(0, 1 - y x);  dx = -y where 1 - y x >= 0, else 0
 *                              (MarginRankingLoss(margin=1); torch's clamp_min backward: the kink passes the gradient)
 *     MM_PAIR_MARGIN_MSE       (x - (a - b))^2;  dx = 2 (x - (a - b))
 *     MM_PAIR_MSE_POINTWISE    ((pos - a)^2 + (neg - b)^2) / 2;  gpos = pos - a, gneg = neg - b
 *     MM_PAIR_KLDIV_POINTWISE  (xlogy(a, a) - a pos + xlogy(b, b) - b neg) / 2;  gpos = -a / 2, gneg = -b / 2
 *                              (KLDivLoss() fed raw scores, reproduced as it is; a negative label gives a NaN loss as in torch)
 *     MM_PAIR_RANKNET_TEACHER  (a - b) (sp(x) - x);  dx = (a - b)(sg(x) - 1)
 *     MM_PAIR_MSE_RANKNET      the MM_PAIR_MSE_POINTWISE term + sp(x) - x;  the sum of both gradients
 *   For the kinds written with dx: gpos = dx, gneg = -dx.
 *   0 <= n <= 2^31.  n = 0 writes loss = NaN (torch.mean of an empty tensor) and launches nothing else.
 *   A grid that is a function of n alone strides over the elements; n <= 4,096 is one workgroup and one launch.  Larger n:
 *   one float64 partial per workgroup in the workspace (mm_pair_loss_workspace_bytes(n), 0 up to 4,096 elements, at most
 *   8 KiB), added by a second one-workgroup launch in a fixed order.
 *   MM_EINVAL: NULL where required, n < 0, unknown kind or dtype.  MM_EUNSUPPORTED: n > 2^31.  MM_EWORKSPACE: short workspace.
 */
#define MM_PAIR_RANKNET 0
#define MM_PAIR_MARGIN 1
#define MM_PAIR_MARGIN_MSE 2
#define MM_PAIR_MSE_POINTWISE 3
#define MM_PAIR_KLDIV_POINTWISE 4
#define MM_PAIR_RANKNET_TEACHER 5
#define MM_PAIR_MSE_RANKNET 6

size_t mm_pair_loss_workspace_bytes(int64_t n);
int mm_pair_loss_fwd(const void* pos, const void* neg, int dtype, const float* a, const float* b, int64_t n, int kind,
                     float* loss, void* grad_pos, void* grad_neg, void* workspace, size_t workspace_bytes, void* stream);

/* mm_list_loss_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/losses/listnet.py:27-33, matchmaker/losses/teacher_kldiv_list.py:13,
 *           matchmaker/losses/loss_smooth_mrr.py:11-33, matchmaker/losses/lambdarank.py:65-119 and :131-134
 *   scores [B, L] of `dtype`, labels [B, L] fp32; loss [1] fp32; per_list [B] fp32 = the list's own term before the batch
 *   reduction (what SmoothMRRLoss(agg=False) returns); grad [B, L] of `dtype` = d loss / d scores.  p = softmax(scores),
 *   T = softmax(labels), both per list:
 *     MM_LIST_LISTNET     per list -sum_i T_i log(p_i + 1e-6); mean over B.
 *                         grad_k = -(1 / B) sum_i T_i p_i (d_ik - p_k) / (p_i + 1e-6)
 *     MM_LIST_KLDIV       sum_i (xlogy(T_i, T_i) - T_i p_i), summed over the lists, divided by B (KLDivLoss("batchmean") fed
 *                         probabilities, reproduced as it is).  grad_k = -(1 / B) sum_i T_i p_i (d_ik - p_k)
 *     MM_LIST_SMOOTH_MRR  rank_i = 0.5 + sum_j sg(s_j - s_i), j = i included; rr_i = [label_i > 0] / rank_i; per list
 *                         1 - max_i rr_i; mean over B.  The gradient flows through the arg-max only.  STATED CHOICE: the
 *                         lowest index on ties.
 *     MM_LIST_LAMBDA_NDCG2  LambdaLoss("ndcgLoss2_scheme") with padded_value_indicator=-1, eps=1e-6, k=None, sigma=1,
 *                         reduction="sum", reduction_log="binary".  Entries with label == -1 are padded: score and label
 *                         count as -inf and their gradient is 0.  Stable descending order of the scores; t = the labels in
 *                         that order; D[m] = log2(2 + m); maxDCG = max(sum_m (2^max(label, 0) - 1) / D[m] over the labels in
 *                         descending order, eps); G_i = (2^max(t_i, 0) - 1) / maxDCG.  For every ordered pair (i, j) of sorted
 *                         positions with t_i, t_j finite and t_i > t_j:  w = |1 / D[|i - j| - 1] - 1 / D[|i - j|]| |G_i - G_j|,
 *                         x = clamp(s_i - s_j, +-1e4), p = sg(x), term = -log2(max(max(p, eps)^w, eps)).  Loss = the sum over
 *                         all lists, NOT divided by B.  d term / d x = -w (1 - p) / ln 2 when p >= eps and p^w >= eps, else 0;
 *                         it is added to the score at sorted position i and subtracted from the one at j.  (The discount
 *                         differences are formed in float64 and rounded once: two reciprocals that agree in ever more digits.
 *                         The term is evaluated as min(w softplus(-x) / ln 2, -log2(eps)) where p >= eps: the same value
 *                         without p^w and log(p) next to 1, where fp32 keeps a handful of the term's bits.)
 *     MM_LIST_LAMBDA_NDCG2_TEACHER  labels <- softmax(labels) in fp32, then + 2 where > 0.001, on the device; then as above.
 *                         Nothing is padded.
 *   STATED CHOICE for the order: stable, as mm_segment_rank_fwd (equal scores in arrival order, -0 == +0); torch.sort on the
 *   GPU leaves the order of ties open.  The loss depends on it only when non-padded scores tie exactly.
 *   Lists of <= 64 entries take one wavefront each (four per workgroup, no LDS), longer ones one workgroup each; ranks come
 *   from counting the keys below one's own; the pair loop is O(L^2) per list.  L > MM_LOSS_MAX_LIST returns MM_EUNSUPPORTED
 *   before any launch.  A second one-workgroup launch adds per_list in a fixed order.  No workspace.
 *   B = 0: loss = NaN for the mean kinds, 0 for the Lambda kinds.  L = 0: every per_list term is its empty sum (1 for
 *   MM_LIST_SMOOTH_MRR).
 *   MM_EINVAL: NULL where required, B < 0, L < 0, unknown kind or dtype.
 */
#define MM_LIST_LISTNET 0
#define MM_LIST_KLDIV 1
#define MM_LIST_SMOOTH_MRR 2
#define MM_LIST_LAMBDA_NDCG2 3
#define MM_LIST_LAMBDA_NDCG2_TEACHER 4
#define MM_LOSS_MAX_LIST 1024

int mm_list_loss_fwd(const void* scores, int dtype, const float* labels, int B, int L, int kind, float* loss,
                     float* per_list, void* grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * mm_distinct_hits_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/dense_retrieval.py:414-429 (the `maxP->bert_dot` branch of the search loop: per query a Python loop
 *           over the passage hits with a `set` of ids, the first hit of every id kept until top_n documents are found), on
 *           an index whose external ids repeat per passage (dense_retrieval.py:237-265, `current_ids[start:end] = len(seq_ids)`).
 *   hit_scores [nq, K] fp32, hit_ids [nq, K] int64, contiguous, in the order the search returned them (score descending, ties
 *   in the search's own order).  The list is NOT re-sorted by score: per query the first occurrence of every id IN LIST ORDER
 *   is kept, which is the reference's loop and, for a descending list, the document's maximum passage score.
 *   Every id < 0 is "no hit" and dropped (-1 is not the only such value); every id >= 0 is valid, INT64_MAX included (ids are
 *   ordered as unsigned numbers, so the sign bit is the valid bit and no id value is reserved).  Scores are payload: copied bit
 *   for bit (NaN, +-inf, -0.0) and never compared.
 *   out_scores fp32, out_ids int64, out_pos int32, each [nq, top_n]: the first min(distinct, top_n) kept hits in list order,
 *   out_pos = the hit's position in the list (the caller recovers the winning passage row from it); behind them -inf / -1 / -1.
 *   n_distinct [nq] int32 = distinct valid ids of the WHOLE list (not capped at top_n); n_valid [nq] int32 = ids >= 0.
 *   Certificate: when the list is the exact top-K in descending order, a document with no passage in it scores <= the K-th
 *   hit, so the kept hits are the exact document ranking as far as they go; n_distinct >= top_n or n_valid < K (the index was
 *   exhausted) means out_* is the exact top_n of all documents.
 *   1 <= K <= MM_DISTINCT_MAX_HITS, 1 <= top_n <= K, else MM_EUNSUPPORTED before any launch; nq < 0 or a NULL pointer with
 *   nq > 0: MM_EINVAL; nq = 0 succeeds without a launch (its pointers are not looked at); nq < 2^31 by its type.
 *   One workgroup per query in grid.x.  LDS: 16 bytes per key for the next power of two >= K, K flag bytes, 64 bytes of scan
 *   scratch: 136 KiB at K = 8,192 (one workgroup per CU), 2.2 KiB at K = 128.  Every output element is stored exactly once,
 *   nothing else is written, whatever the ids hold every access stays inside the arrays.  No workspace, no atomics, no
 *   read-back: graph-capturable, two calls give the same bits.
 */
#define MM_DISTINCT_MAX_HITS 8192

int mm_distinct_hits_fwd(const float* hit_scores, const int64_t* hit_ids, int nq, int K, int top_n,
                         float* out_scores, int64_t* out_ids, int32_t* out_pos,
                         int32_t* n_distinct, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * In-batch negatives of dense-retriever training: from the vectors (or the [B, B] score matrices) to the in-batch loss, its
 * statistics and every gradient, in one fixed linear chain of launches (additive: MM_ABI_VERSION unchanged).  Both entries
 * run on `stream` with no allocation, no read-back and no atomics, vector stores only: graph-capturable, two calls give the
 * same bits.  Every output element is written on every successful call.
 *
 *   sp [B] = the paired score of (query i, its positive); Sp[i, j] = <Q_i, Dp_j>, Sn[i, j] = <Q_i, Dn_j>; Tp, Tn [B, B] fp32
 *   teacher scores of the same pairs or both NULL; M = B (B - 1); "off" = every (i, j) with i != j.
 *   family MM_INBATCH_PAIR, kind = an MM_PAIR_* value:
 *     loss = (mean_off l(sp_i, Sp_ij; a_i, b_ij) + mean_off l(sp_i, Sn_ij; a_i, b'_ij)) / 2, l = the per-element term of
 *     mm_pair_loss_fwd with sp in the `pos` role and the in-batch score in the `neg` role (ONE device function serves both
 *     entries and mm_pair_loss_fwd: float64 terms).  With a teacher a_i = Tp_ii, b_ij = Tp_ij, b'_ij = Tn_ij (every kind with
 *     two labels); without one the label is 1 (MM_PAIR_RANKNET, MM_PAIR_MARGIN).  A kind with two labels and no teacher, or a
 *     one-label kind with a teacher, is MM_EINVAL.  The diagonal takes no part; its gradient is written as 0.
 *   family MM_INBATCH_LIST, kind = an MM_LIST_* value: mm_list_loss_fwd's loss of the lists cat([Sp, Sn], 1) [B, 2B] against
 *     cat([Tp, Tn], 1), the diagonal included, sp not used (grad_sp = 0); the teacher is required; the same device code as
 *     mm_list_loss_fwd, reading the two matrices in place.  2B <= MM_LOSS_MAX_LIST, else MM_EUNSUPPORTED before any launch.
 *   stats [3] fp32, for every kind:
 *     [0] accuracy    (mean_off [sp_i > Sp_ij] + mean_off [sp_i > Sn_ij]) / 2      (a tie counts as not greater)
 *     [1] score_diff  (mean_off (sp_i - Sp_ij) + mean_off (sp_i - Sn_ij)) / 2
 *     [2] teacher accuracy (mean_off [Tp_ii > Tp_ij] + mean_off [Tp_ii > Tn_ij]) / 2 for the pair family with a teacher, else NaN
 *   Every sum is float64 in a fixed order: per lane, per wavefront, per workgroup, then one workgroup over the workgroups'
 *   partials; loss and statistics are rounded once to fp32.  B = 0: loss (0 for the Lambda list kinds, as mm_list_loss_fwd) and
 *   statistics are NaN, one launch, nothing else is written.  B = 1 in the pair family: loss and statistics NaN (means of empty
 *   sets, as torch), gradients 0.
 *
 * mm_inbatch_select_loss_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/train.py:434-438 and :443-472 (the selection of the off-diagonal pairs, the loss calls and the three
 *           statistics, on score matrices the caller has: train.py:439-440, or ColBERT's forward_inbatch_aggregation)
 *   sp [B], Sp, Sn [B, B] of `dtype` (MM_F32 / MM_F16 / MM_BF16, widened exactly).  grad_sp [B], grad_Sp, grad_Sn [B, B] of
 *   `dtype` = d loss / d sp, d Sp, d Sn, each rounded once.  Two launches (three for the list family): the selection kernel
 *   (32 x 32 tiles, one per wavefront), [the list kernel,] the one-workgroup finish.  0 <= B <= 1024.
 *   Workspace: mm_inbatch_select_loss_workspace_bytes(B, family) (float64 partials, per-list terms).
 *
 * mm_inbatch_dot_loss_fwd (additive: MM_ABI_VERSION unchanged)
 * Replaces: matchmaker/train.py:434-472 (the two torch.mm included) and the backward of that block in loss.backward()
 *           (train.py:503-524): two mm, twelve masked indexings with their host synchronisations, three expand copies, two loss calls
 *   Q, Dp, Dn [B, E] of `dtype`; sp [B] of `sp_dtype` (under autocast 16-bit, else fp32).  grad_Q, grad_Dp, grad_Dn [B, E] of
 *   `dtype`, grad_sp [B] of `sp_dtype`; each of the four may be NULL and is then not computed; all of grad_Q, grad_Dp, grad_Dn NULL
 *   skips the gradient launch (loss and statistics only, the same bits).
 *   1. Scores: Sp = Q Dp^T and Sn = Q Dn^T on the matrix cores, v_mfma_f32_32x32x16_{bf16,f16} for 16-bit vectors (every
 *      product exact in fp32) and v_mfma_f32_32x32x2_f32 for fp32 vectors (no rounding of the inputs), fp32 accumulation in a
 *      fixed order inside blocks of 64 k, the blocks added in float64 and S rounded once to fp32.  STATED CHOICE: S stays fp32; it is not rounded to 16 bits as an autocast torch.mm rounds it.  The
 *      pair-family epilogue runs in the same launch on the accumulator registers: term, statistics, G = d loss / d S (fp32,
 *      the 1 / (2M) included), one float64 partial set per workgroup, float64 row sums for grad_sp.
 *   2. List family only: the list kernel on S, writing G.
 *   3. Finish: one workgroup adds the partials in a fixed order and writes loss, stats and grad_sp.
 *   4. Gradients, one launch: grad_Q = Gp Dp + Gn Dn, grad_Dp = Gp^T Q, grad_Dn = Gn^T Q with v_mfma_f32_32x32x2_f32 on the
 *      exactly widened vectors; G is not rounded to 16 bits; each gradient is rounded once to `dtype`.
 *   The select entry fed this entry's Sp, Sn (the workspace begins with them) gives the same loss, stats and grad_sp bits: both
 *   walk the elements in the same order.
 *   1 <= B <= 1024 (list family: 2B <= MM_LOSS_MAX_LIST), 8 <= E <= 1024, rows of 16 bytes (E % 8 == 0 for 16-bit vectors,
 *   E % 4 == 0 for fp32), else MM_EUNSUPPORTED before any launch; Q, Dp and Dn 16-byte aligned (the
 *   rows are loaded 16 bytes per lane), else MM_EINVAL.
 *   Workspace: mm_inbatch_dot_loss_workspace_bytes(B, E, family).  It begins with Sp, Sn [2][B][B] fp32, followed at the next
 *   multiple of 256 bytes by Gp, Gn [2][B][B] fp32; then the float64 partials and row sums and the per-list terms.
 *   MM_EINVAL: NULL where required, B < 0, unknown family, kind or dtype, a teacher that does not fit the kind.
 *   MM_EWORKSPACE: short workspace.
 */
#define MM_INBATCH_PAIR 0
#define MM_INBATCH_LIST 1

size_t mm_inbatch_select_loss_workspace_bytes(int B, int family);
int mm_inbatch_select_loss_fwd(const void* sp, const void* Sp, const void* Sn, int dtype, const float* Tp, const float* Tn,
                               int B, int family, int kind, float* loss, float* stats, void* grad_sp, void* grad_Sp,
                               void* grad_Sn, void* workspace, size_t workspace_bytes, void* stream);
size_t mm_inbatch_dot_loss_workspace_bytes(int B, int E, int family);
int mm_inbatch_dot_loss_fwd(const void* Q, const void* Dp, const void* Dn, int dtype, const void* sp, int sp_dtype,
                            const float* Tp, const float* Tn, int B, int E, int family, int kind, float* loss, float* stats,
                            void* grad_Q, void* grad_Dp, void* grad_Dn, void* grad_sp, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * mm_self_attention_fwd, mm_self_attention_supported (additive: MM_ABI_VERSION unchanged)
 * Replaces: the attention core of the contextualiser's encoder layers, matchmaker/models/published/ecai20_tk.py:138,
 *           sigir20_tkl.py:296-308 and sigir21_idcm.py:174-175 (nn.TransformerEncoder, batch_first=False, with
 *           src_key_padding_mask: per layer F.multi_head_attention_forward -> scaled_dot_product_attention with a float mask).
 *           The projections, LayerNorm and the feed-forward block stay torch's; there is no backward.
 *   out[b, i, h dh + d] = sum_j softmax_j(q[b,i,h] . k[b,j,h] / sqrt(dh) + (mask[b,j] ? 0 : -inf)) v[b,j,h,d]
 *   qkv [B, L, 3 E] of `dtype` (MM_F32 / MM_F16 / MM_BF16), contiguous, E = H dh: what F.linear(x, in_proj_weight, in_proj_bias)
 *   returns.  Q in columns [0, E), K in [E, 2E), V in [2E, 3E); head h at column offset h dh.  qkv and out aligned to their
 *   element type, nothing more: every global access is made in chunks of the largest of 16 / 8 / 4 / 2 bytes that divides both
 *   addresses, E and dh in bytes, and the result does not depend on it.
 *   mask [B, L] (or [B] lengths) of mask_kind MM_MASK_*: nonzero = token.  An arbitrary pattern, not a length.  Only KEYS are
 *   masked: all L query rows are computed and written.  A sequence with no unmasked key gets +0 in every row (torch 2.10's
 *   safe softmax gives the same).
 *   out [B, L, E] of `dtype`: heads concatenated, ready for out_proj.
 *   Arithmetic: q k^T by v_mfma_f32_32x32x2_f32 for fp32 inputs and by v_mfma_f32_32x32x16_{f16,bf16} for 16-bit ones (every
 *   product exact in fp32), the weighted sum of v by v_mfma_f32_32x32x2_f32 on the exactly widened v for every type (no rounding
 *   of an operand or of a weight, fp32 accumulation in a fixed order), scores scaled by log2(e) / sqrt(dh) with the mask added in one fma, softmax on v_exp_f32 in
 *   fp32, the weighted sum divided by the weights' sum, one rounding to `dtype` at the store.
 *   mm_self_attention_supported(dtype, L, H, dh) -> 1 / 0, a pure host function: 1 <= L <= 256, 1 <= dh <= 64, dh even for
 *   the 16-bit types, H >= 1.  Anything else: MM_EUNSUPPORTED from mm_self_attention_fwd before any launch.
 *   One workgroup per (sequence, head) in grid.x (B H < 2^31), K and V of the head in LDS (at most 76 KiB for dh <= 32, 138 KiB beyond).  One launch, no
 *   workspace, no atomics, no read-back, vector stores only, every element of out stored exactly once: graph-capturable, two
 *   calls give the same bits.  B = 0 succeeds without a launch.
 *   MM_EINVAL: NULL where required, B < 0, unknown dtype or mask kind, misaligned qkv / out.
 */
int mm_self_attention_supported(int dtype, int L, int H, int dh);
int mm_self_attention_fwd(const void* qkv, int dtype, const void* mask, int mask_kind, int B, int L, int H, int dh, void* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MM_NATIVE_H */
