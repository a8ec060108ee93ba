/*
 * ssi_hip.h — C ABI of libssi_hip.so: the MI355X (gfx950) kernels under the speech-integration training hot path.
 *
 * The reference (anilkeshwani/speech-integration) reaches its GPU arithmetic only through Python:
 * ssi/trainer.py -> ssi/loss.py -> torchtune 0.5.0 modules -> ATen.  It has no FFI of its own, so the drop-in boundary
 * is the Python API (speech-integration_amd/ssi mirrors it); THIS header is the native seam underneath it, one entry per
 * vendor op the reference hits.  Each entry cites the reference call site it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named host_*; the caller (PyTorch's allocator) owns all buffers,
 *     including workspaces; the library allocates nothing persistent and never synchronises the device.
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered.  Compute entries keep no per-call host state and may
 *     be called from any host thread (autograd runs backward on another thread than forward); their one-time set-up (LDS size
 *     attribute, CU count) is done under C++ thread-safe static initialisation.
 *   - PROCESS-GLOBAL state, stated here because it is not per call: (1) ssi_set_impl, (2) ssi_set_gemm_tile_order and (4) ssi_set_attn_impl
 *     are switches for the whole process (atomics; meant to be set once at start-up — tests, A/B runs, the data-parallel trainer — not
 *     flipped while another thread is launching; (4) takes its initial values from the environment variables SSI_ATTN_DQ / SSI_ATTN_DKV,
 *     read ONCE at first use, never on the launch path; the kernel choice moves results at the 1e-4 level — another summation order);
 *     (5) ssi_attn_last_dispatch reports the choice of the most recent attention backward of the process (diagnostic);
 *     (3) with SSI_TILES_DYNAMIC the persistent GEMM draws tiles from 16 scheduler slots in
 *     device memory handed out round-robin per launch, shared by all streams of the process: more than 16 persistent GEMMs in
 *     flight at once on one device would share a slot (the trainer has at most two).
 *   - return 0 on success; SSI_ERR_* otherwise (never throws).  ssi_last_error() gives a thread-local message.
 *   - dtype: SSI_F32 or SSI_BF16 selects the storage type of activations/weights; reductions, softmax, norms and
 *     accumulators are always fp32 (the reference's rounding points).
 *   - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef SSI_HIP_H
#define SSI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSI_ABI_VERSION 30 /* 30: + ssi_bpe_pair_count, ssi_bpe_train_workspace_bytes, ssi_bpe_train_begin, ssi_bpe_merge, ssi_bpe_encode (byte-pair encoding over discrete speech units: a trainer whose state stays on the device, and an encoder for many sequences per launch; opt-in)
                           * 29: + ssi_edit_distance, ssi_edit_distance_workspace_bytes (edit distance with substitution, deletion and insertion counts between spans of int32 ids, many pairs per launch: error rates and minimum-Bayes-risk selection; opt-in)
                           * 28: + ssi_decode_sample_rows, ssi_decode_sample_pen_rows (the two sampling entries with the step and the draw parameters per row, from device arrays: rows of different ages and requests in one launch; opt-in)
                           * 27: + ssi_weight_quant_fp8, ssi_gemm_skinny_w8, ssi_gemm_skinny_rope_w8, ssi_gemm_skinny_swiglu_w8 (weight matrices as e4m3 codes with one power-of-two exponent per row, and the skinny GEMMs over them: FP8 weights for small-batch decoding; opt-in)
                           * 26: + ssi_kv_store_fp8, ssi_attn_decode_fp8, ssi_attn_decode_beam_fp8, ssi_attn_decode_split_fp8, ssi_attn_decode_beam_split_fp8 (a K/V cache of e4m3 codes with one power-of-two exponent per line, and decode attention over it; opt-in)
                           * 25: + ssi_attn_decode_split, ssi_attn_decode_beam_split, ssi_attn_decode_split_span, ssi_attn_decode_split_workspace (split-KV decode attention: the keys of a row over several workgroups, a merge launch behind them; opt-in)
                           * 24: + ssi_gemm_skinny, ssi_gemm_skinny_rope, ssi_gemm_skinny_swiglu (weight-streaming bf16 GEMMs for 1 to 64 rows: small-batch decoding; opt-in)
                           * 23: + ssi_sumsq_groups, ssi_adamw_step_seg_gscale (per-group gradient norms of the flat buffer in one pass, a per-segment device gradient scale in the segmented AdamW; opt-in)
                           * 22: + ssi_decode_select_pen, ssi_decode_sample_pen (repetition, frequency and presence penalties inside the two selection kernels; opt-in)
                           * 21: + ssi_decode_sample (sampled decoding: temperature, top-k, top-p and a seeded Gumbel-max draw of a row's token in one launch; opt-in)
                           * 20: + ssi_attn_decode_beam, ssi_topk_logprob (beam search: decode attention through an ancestry table, the k best allowed columns of a row; opt-in)
                           * 19: + ssi_decode_select (constrained greedy decoding: the allowed argmax of a row, its log-probability and its rank in one pass; opt-in)
                           * 18: + ssi_kv_store, ssi_attn_decode (greedy generation: a K/V cache and single-query attention over it; nothing else calls them)
                           * 17: + ssi_ema_update (fp32 exponential moving average of the flat parameter buffer, one pass chained to AdamW; opt-in)
                           * 16: + ssi_adamw_step_seg (AdamW over segments of the flat buffers with their own lr, weight decay and frozen flag; opt-in)
                           * 15: + ssi_ce_fwd_kl (KL against a frozen teacher's logits inside the cross-entropy kernels; opt-in)
                           * 14: + ssi_ce_fwd_smooth (label smoothing inside the cross-entropy kernels, beside the z-loss; opt-in)
                           * 13: + ssi_seq_score_reduce (per-sequence sums of what ssi_ce_fwd_metrics wrote: likelihood scoring of packed rows)
                           * 12: + ssi_ce_fwd_z (cross-entropy with the auxiliary z-loss z * log^2 Z in its gradient; opt-in)
                           * 11: + ssi_adamw_step_sr, ssi_round_bf16_sr (bf16 AdamW whose three stores round stochastically, counter-based)
                           * 10: + ssi_ce_fwd_metrics, ssi_ce_metrics_reduce (dev-set loss and top-k accuracy per token type)
                           * 9: ssi_adamw_step takes its hyper-parameters in double (the coefficients of torch's fused AdamW)
                           * 8: + ssi_ce_fwd_weighted (per-row loss weights: an accumulation window run as ONE batch keeps the reference's
                           *    per-micro-batch normalisation, ssi/data/window.py)
                           * 7: + ssi_set_attn_impl, ssi_attn_last_dispatch (no getenv on the launch path), ssi_attn_plan_* and ssi_attn_varlen_bwd_plan
                           *    (packed rows on the pipelined backward kernels, host-built work plan)
                           * 6: + ssi_attn_bwd_workspace_bytes, ssi_attn_varlen_bwd_ws (attention backward with a caller-owned workspace)
                           * 5: ssi_doc_ranges takes n_clamped (out-of-table positions are counted, not only clamped)
                           * 4: + ssi_gemm_batched
                           * 2: + ssi_attn_varlen_fwd/bwd(_rope), ssi_set_gemm_tile_order, NN form of ssi_gemm_swiglu_bwd
                           * 3: ssi_ce_reduce takes `vocab` and reports out-of-range labels in out[3]; + ssi_doc_ranges; ssi_rmsnorm_bwd takes accumulate_dscale; + ssi_lmhead_ce_fwd/bwd */

enum { SSI_F32 = 0, SSI_BF16 = 1 };
enum { SSI_OK = 0, SSI_ERR_ARG = 1, SSI_ERR_UNSUPPORTED = 2, SSI_ERR_WORKSPACE = 3, SSI_ERR_HIP = 1000 /* + hipError_t */ };
/* GEMM operand layouts (row-major storage):
 *   NT: A[M,K]  B[N,K]   C = A * B^T   forward linear  y = x W^T      (F.linear, torchtune nn.Linear / TiedLinear)
 *   NN: A[M,K]  B[K,N]   C = A * B     data gradient   dx = dy W
 *   TN: A[K,M]  B[K,N]   C = A^T * B   weight gradient dW = dy^T x                                                  */
enum { SSI_GEMM_NT = 0, SSI_GEMM_NN = 1, SSI_GEMM_TN = 2 };
/* which implementation ssi_gemm may use: AUTO picks the MFMA kernel when shape/dtype allow, else the generic one */
/* Order in which the workgroups of the persistent MFMA GEMM take output tiles.  STATIC (default): tile b, b+G, ... — optimal
 * when the GEMM has the GPU to itself.  DYNAMIC: tiles are drawn from per-XCD counters, so a workgroup that starts late because
 * another kernel holds its CU (RCCL during the data-parallel gradient exchange) costs its share of tiles instead of a round. */
enum { SSI_TILES_STATIC = 0, SSI_TILES_DYNAMIC = 1 };
int ssi_set_gemm_tile_order(int mode);

enum { SSI_IMPL_AUTO = 0, SSI_IMPL_GENERIC = 1, SSI_IMPL_MFMA = 2,
       SSI_IMPL_MFMA_WG8 = 3 /* debug / A-B runs: MFMA paths, but the NT GEMM restricted to the 8-wave LDS-DMA kernel */ };

int ssi_abi_version(void);
const char* ssi_last_error(void);
/* force an implementation for kernels that have both a generic and an MFMA path (tests); returns previous value */
int ssi_set_impl(int impl);

/* ---- K1  nn.Embedding (torchtune TransformerDecoder.tok_embeddings; called from ssi/loss.py:8) ------------------- */
/* out[t,:] = table[tokens[t],:] */
int ssi_embed_fwd(const int64_t* tokens, const void* table, void* out, int64_t n_tok, int64_t dim, int64_t vocab,
                  int dtype, void* stream);
/* dtable[v,:] += sum_{t: tokens[t]==v} dout[t,:]   (deterministic: sorted segmented sum, fp32 accumulate, no atomics) */
int64_t ssi_embed_bwd_workspace_bytes(int64_t vocab);
int ssi_embed_bwd(const int64_t* tokens, const void* dout, void* dtable, int64_t n_tok, int64_t dim, int64_t vocab,
                  int dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- K2  RMSNorm (torchtune.modules.RMSNorm; sa_norm / mlp_norm / norm) ------------------------------------------- */
/* y = (x32 * rsqrt(mean(x32^2)+eps)).to(dtype) * scale ; rstd[row] saved for backward */
int ssi_rmsnorm_fwd(const void* x, const void* scale, void* y, float* rstd, int64_t rows, int64_t dim, float eps,
                    int dtype, void* stream);
/* dx = d(rmsnorm)/dx . dy (+ dres if non-null);  dscale (+)= sum_rows dy * xhat  (two-stage deterministic reduce; accumulate_dscale
 * == 0 overwrites: the first micro-batch of an accumulation window writes the gradients, nothing zeroes them beforehand).
 * partials: fp32 workspace of ssi_rmsnorm_bwd_workspace_bytes(rows, dim) bytes. */
int64_t ssi_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t dim);
int ssi_rmsnorm_bwd(const void* dy, const void* x, const void* scale, const float* rstd, const void* dres, void* dx,
                    void* dscale, int accumulate_dscale, int64_t rows, int64_t dim, int dtype, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- K4  Llama3ScaledRoPE (adjacent-pair rotation, fp32 math; torchtune MultiHeadAttention.pos_embeddings) -------- */
/* x: [rows, ld] rows = b*seq_len + s; rotates heads [0, n_heads_rot) of width head_dim in place; position of a row is
 * positions[row] if positions != NULL else row % seq_len.  table: [table_len, head_dim/2, 2] fp32 (cos, sin).
 * inverse != 0 applies the transpose rotation (the backward of the forward rotation). */
int ssi_rope_inplace(void* x, int64_t ld, int64_t rows, int64_t seq_len, int n_heads_rot, int head_dim,
                     const float* table, int64_t table_len, const int32_t* positions, int inverse, int dtype,
                     void* stream);

/* C[M, N] = A[M, K] B[N, K]^T followed by ssi_rope_inplace(C, heads [0, n_heads_rot)): the QKV projection (K3) with the rotation
 * (K4) in the GEMM epilogue on the MFMA path (bf16, head_dim 64, n_heads_rot * 64 a multiple of 256), two launches otherwise. */
int ssi_gemm_rope(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                  int64_t seq_len, int n_heads_rot, int head_dim, const float* rope_table, int64_t table_len,
                  const int32_t* positions, int dtype, void* stream);

/* ---- K5  causal GQA attention (F.scaled_dot_product_attention(is_causal=True) inside torchtune MultiHeadAttention) -- */
/* qkv: [B*S, ld] with q heads at column 0, k heads at n_heads*head_dim, v heads at (n_heads+n_kv)*head_dim.
 * out: [B*S, n_heads*head_dim].  lse: [B, n_heads, S] fp32 (natural-log sum-exp of scaled scores). */
int ssi_attn_fwd(const void* qkv, int64_t ld, void* out, float* lse, int64_t batch, int64_t seq, int n_heads,
                 int n_kv, int head_dim, int dtype, void* stream);
/* dqkv (same layout as qkv) is fully overwritten. delta: fp32 workspace [B, n_heads, S]. */
int ssi_attn_bwd(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                 float* delta, int64_t batch, int64_t seq, int n_heads, int n_kv, int head_dim, int dtype,
                 void* stream);

/* Packed rows (several documents per row; SURVEY.md §8f rank 1, the block-causal mask torchtune's padded_collate_packed builds
 * from `seq_lens`, reference stub ssi/data/__init__.py:66-73,202-205): doc_start / doc_end are int32 [B*S]; for position s of
 * row b, doc_start[b*S+s] is the first position and doc_end[b*S+s] one past the last position of the document holding s (both
 * relative to the row, non-decreasing along it).  A query sees the keys doc_start <= key <= query.  Both NULL = plain causal
 * attention (= ssi_attn_fwd / ssi_attn_bwd).  Key tiles outside the documents of a query block are skipped, not masked. */
int ssi_attn_varlen_fwd(const void* qkv, int64_t ld, void* out, float* lse, const int32_t* doc_start, const int32_t* doc_end,
                        int64_t batch, int64_t seq, int n_heads, int n_kv, int head_dim, int dtype, void* stream);
int ssi_attn_varlen_bwd(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                        float* delta, const int32_t* doc_start, const int32_t* doc_end, int64_t batch, int64_t seq,
                        int n_heads, int n_kv, int head_dim, int dtype, void* stream);

/* input_pos [batch, seq] (int64; restarts at 0 with every document of a packed row) -> the int32 [batch*seq] arrays the varlen entries
 * take: positions (clamped to [0, max_pos]: the RoPE table is never indexed past its end), doc_start, doc_end.  Position 0 of a row
 * always starts a document.  n_clamped (may be NULL): one int32 the kernel ADDS the number of positions outside [0, max_pos] to — the
 * caller zeroes it and reads it with whatever it reads back anyway, so that a data bug is reported instead of silently clamped.
 * One launch (the reference has no packed path: ssi/data/__init__.py:66-73 raises). */
int ssi_doc_ranges(const int64_t* input_pos, int64_t batch, int64_t seq, int64_t max_pos, int32_t* positions, int32_t* doc_start,
                   int32_t* doc_end, int32_t* n_clamped, void* stream);

/* Same, followed by the backward of the RoPE rotation on the q and k heads of dqkv (= ssi_rope_inplace(dqkv, ..., inverse=1)): the
 * MFMA kernels apply it in their epilogues, which saves a pass over dqkv.  rope_table / table_len / positions as in ssi_rope_inplace. */
int ssi_attn_varlen_bwd_rope(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                             float* delta, const int32_t* doc_start, const int32_t* doc_end, const float* rope_table,
                             int64_t table_len, const int32_t* positions, int64_t batch, int64_t seq, int n_heads, int n_kv,
                             int head_dim, int dtype, void* stream);

/* The same backward with a caller-owned workspace (any of the forms above: doc_start / doc_end and rope_table may be NULL).
 * ssi_attn_bwd_workspace_bytes: what this shape can use, 0 = nothing.  With at least that many bytes (16-byte aligned), launches whose
 * workgroups cannot fill the chip — the reference's default micro-batch of 2 x 2048 rows gives dK / dV 256 workgroups, the heaviest as long as
 * the launch — run dK / dV as one workgroup per query head with fp32 partial rows in the workspace and a reduction over the heads in fixed
 * order (reproducible; the sums over the heads are taken in another order than without workspace). */
int64_t ssi_attn_bwd_workspace_bytes(int64_t batch, int64_t seq, int n_heads, int n_kv, int head_dim, int dtype);
int ssi_attn_varlen_bwd_ws(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                           float* delta, const int32_t* doc_start, const int32_t* doc_end, const float* rope_table,
                           int64_t table_len, const int32_t* positions, int64_t batch, int64_t seq, int n_heads, int n_kv,
                           int head_dim, int dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* Which kernels the attention backward may take (process-global, see "PROCESS-GLOBAL state" above).  `which`: SSI_ATTN_KERNEL_DQ or
 * SSI_ATTN_KERNEL_DKV.  `mode`: AUTO = the dispatcher's choice by shape; OLD = the round-1..3 kernels (attn_bwd_dq_kernel / the 128-key
 * attn_bwd_dkv_kernel); NEW = the pipelined one-wave-per-SIMD kernels wherever their shape rules allow, whatever the fill / balance;
 * NO_HEAD_SPLIT (dK / dV only) = AUTO without the per-query-head split of small launches.  Returns the previous mode (an invalid `mode`
 * only reads it; an invalid `which` returns -1).  Initial values: environment SSI_ATTN_DQ / SSI_ATTN_DKV = 0..3, read once. */
enum { SSI_ATTN_KERNEL_DQ = 0, SSI_ATTN_KERNEL_DKV = 1 };
enum { SSI_ATTN_MODE_AUTO = 0, SSI_ATTN_MODE_OLD = 1, SSI_ATTN_MODE_NEW = 2, SSI_ATTN_MODE_NO_HEAD_SPLIT = 3 };
int ssi_set_attn_impl(int which, int mode);
/* Kernels the most recent MFMA attention backward of this process launched (diagnostic; tests assert the dispatch with it, the secondary
 * bench lines name the path a number came from): bit 0 dQ pipelined (attn_bwd_dq2_kernel), bit 1 dK/dV pipelined (attn_bwd_dkv2_kernel),
 * bit 2 dK/dV split over the query heads, bit 3 the document-aware (plan) forms of the pipelined kernels; bits 8-11 query blocks per
 * persistent dQ workgroup.  0 before any call and after a call that took the generic kernels. */
enum { SSI_ATTN_USED_DQ2 = 1, SSI_ATTN_USED_DKV2 = 2, SSI_ATTN_USED_HEAD_SPLIT = 4, SSI_ATTN_USED_PLAN = 8 };
int ssi_attn_last_dispatch(void);

/* Work plan for packed rows on the pipelined backward kernels (the Trainer's default path: ssi/data/unpad.py turns every right-padded batch of
 * the reference's collate function, ssi/data/__init__.py:139-199, into one packed row; plans/Feature - Packed Dataset Support.md:1-96).  The
 * document bounds are known on the HOST wherever batches are collated, so the plan is built there (no device sync, in the prefetch thread)
 * and travels to the device with the batch: every document is cut into dK/dV items (up to 256 keys of ONE document) and dQ items (a
 * 64-query block of ONE document), sorted by work, the dQ items dealt to persistent workgroups of equal load.  Tiles outside an item's
 * document are not in its tile list at all (skipped, not masked); the heaviest items start first whatever their place in the row.
 *   host_doc_row / _start / _end: n_docs documents as (row b, first position, one past the last position) — they must tile every row.
 *   flags: SSI_ATTN_PLAN_FORCE = build the plan even where the round-1..3 kernels are expected to be faster (tests).
 *   ssi_attn_plan_words: upper bound of a plan's size in int32 words.  ssi_attn_plan_build: words written (> 0); 0 = the pipelined kernels
 *   do not take this batch (other than 4 query heads per kv head, a document longer than 16 384 tokens, mostly tiny documents) — pass no
 *   plan then; < 0 = bad arguments.  The first SSI_ATTN_PLAN_HEADER words are the header the launch
 *   reads on the host.  RoPE positions are taken to be (position - document start): build no plan for batches whose input_pos does
 *   anything else. */
enum { SSI_ATTN_PLAN_HEADER = 16, SSI_ATTN_PLAN_FORCE = 1, SSI_ATTN_PLAN_SPLIT_ALL = 2 /* tests: every dK/dV chunk split over the query heads */ };
int64_t ssi_attn_plan_words(int64_t batch, int64_t seq, int64_t n_docs);
/* dK/dV chunks whose work exceeds the chip's share per compute unit (long documents) are split over the query heads: fp32 partial sums in
 * the caller's workspace, added by a reduction pass over those chunks only.  ssi_attn_plan_workspace_bytes: what ssi_attn_varlen_bwd_plan needs
 * in `workspace` for this plan (0: nothing was split; -1: not a plan header). */
int64_t ssi_attn_plan_workspace_bytes(const int32_t* host_plan_header);
int64_t ssi_attn_plan_build(const int32_t* host_doc_row, const int32_t* host_doc_start, const int32_t* host_doc_end, int64_t n_docs,
                            int64_t batch, int64_t seq, int n_heads, int n_kv, int flags, int32_t* host_plan, int64_t plan_words);
/* ssi_attn_varlen_bwd_ws + a plan: plan = the plan in DEVICE memory, host_plan_header = its first SSI_ATTN_PLAN_HEADER words on the host
 * (both NULL = ssi_attn_varlen_bwd_ws).  doc_start / doc_end stay required for packed rows (kernels a mode switch sends back to the
 * round-1..3 forms read them); plain causal rows (doc_start = doc_end = positions = NULL) may bring a plan whose documents are the rows
 * themselves — the persistent dQ workgroups then get their query blocks by load instead of by a fixed pattern.  Results equal the plan-less
 * call's to the rounding of another summation order; reproducible for a given plan. */
int ssi_attn_varlen_bwd_plan(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                             float* delta, const int32_t* doc_start, const int32_t* doc_end, const float* rope_table,
                             int64_t table_len, const int32_t* positions, int64_t batch, int64_t seq, int n_heads, int n_kv,
                             int head_dim, int dtype, void* workspace, int64_t workspace_bytes, const int32_t* plan,
                             const int32_t* host_plan_header, void* stream);

/* ---- Generation (ABI v18; the reference generates with vLLM, scripts/generate.py): K/V cache and one decode step's attention -------------
 * The cache of one layer is two buffers of the model's dtype, k_cache and v_cache, each [n_slots, cap, n_kv * head_dim] row-major; K is
 * stored AFTER RoPE, as it sits in qkv.  Both entries: head_dim a multiple of 8 up to 128 and 1 to 8 query heads per kv head, anything
 * else SSI_ERR_UNSUPPORTED; qkv and the caches 16-byte aligned with ld * sizeof(element) a multiple of 16 (SSI_ERR_ARG otherwise). */
/* cache[dest[r]] = the k / v columns of qkv row r; dest[r] = slot * cap + position, -1 = skip the row.
 * A dest outside [0, n_dest) other than -1 is skipped and COUNTED into *n_bad (may be NULL), like n_clamped of ssi_doc_ranges.
 * Distinct rows must have distinct dest (caller's contract).  Bit-exact copy, 16 bytes per lane. */
int ssi_kv_store(const void* qkv, int64_t ld, const int64_t* dest, int64_t rows, int64_t n_dest, void* k_cache, void* v_cache,
                 int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream);

/* out[r, h, :] = softmax_j(q[r,h]·K[slot[r], j, h / g] / sqrt(head_dim)) · V[slot[r], j, h / g],  j < kv_len[r],  g = n_heads / n_kv.
 * q = columns [0, n_heads*head_dim) of qkv row r.  slot[r] < 0 or kv_len[r] <= 0: the out row is zeros, lse -inf.
 * kv_len is clamped to cap; slot >= n_slots is SSI_ERR-free on the device: the row is zeros and *n_bad (may be NULL) counts it once.
 * out: [rows, n_heads * head_dim].  lse (NULL ok): fp32 [rows, n_heads], natural log.
 * Arithmetic: the header's rule — scores, max, exp-sum and the P·V accumulation in fp32, ONE rounding on the store.  Unlike the training
 * kernels (ssi_attn_*), which feed P to the matrix cores in the storage type, P is NOT rounded to bf16 on the way.  The scores are taken in
 * base 2: q is multiplied by (float)(log2(e) / sqrt(head_dim)) once, exp is v_exp_f32.
 * One workgroup of 4 waves per (row, kv head); the g query heads of a group share every K / V line; no split over workgroups, no
 * workspace, no second pass.  A key's head_dim elements lie on LPK lanes of 16 bytes (LPK = head_dim * sizeof(element) / 16 rounded up to
 * a power of two), a wave holds 64 / LPK keys per load and takes chunks of 2 loads = 128 / LPK keys, chunk c going to wave c % 4
 * (bf16, head_dim 64: chunks of 16 keys, 64 keys per round of the workgroup; fp32, head_dim 64: 8 and 32).  Each lane keeps the running
 * (max, sum, acc) of its key slot; the key slots of a wave are merged by an xor tree with the lower slot first, the waves through LDS in
 * the order 0..3: the result for a row depends on that row's inputs only — not on rows, not on the row's place, not on other slots.
 * Dispatch: ONE kernel form, instantiated per dtype and for G = 1, 2, 4, 8 query-head registers (g = 3 runs G = 4, g = 5..7 run G = 8; the
 * surplus heads repeat the last one and are not stored).  There is no specialised head_dim form, so ssi_set_impl has nothing to choose here.
 * Traffic per row: kv_len * 2 * n_kv * head_dim elements, read once. */
int ssi_attn_decode(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap,
                    const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv,
                    int head_dim, int32_t* n_bad, int dtype, void* stream);

/* ssi_attn_decode over the concatenation of two key ranges (ABI v20, beam search): row r attends to
 *   keys j in [0, prompt_len[r])  of the PROMPT cache [n_pslots, cap_p, n_kv * head_dim], slot prompt_slot[r], then
 *   keys i in [0, gen_len[r])     of the BEAM cache   [n_bslots, cap_b, n_kv * head_dim], slot anc[r * ld_anc + i], position i
 * (anc: int32 [rows, ld_anc] on the device, the ancestry of the row's hypothesis: which beam slot holds its generated position i).  The beams
 * of a prompt share the prompt's K / V and every generated position before they diverged; nothing is copied after a reorder.
 * prompt_len is clamped to [0, cap_p], gen_len to [0, min(cap_b, ld_anc)].  prompt_slot[r] < 0, or no key at all: a zero row and lse -inf.
 * An index outside its cache — prompt_slot[r] >= n_pslots, anc[r, i] outside [0, n_bslots) — is checked BEFORE any address is formed from it:
 * the keys it names are skipped, and the row is counted ONCE into *n_bad (may be NULL); a row whose keys were all skipped is zeros, lse -inf.
 * Dtypes, geometries, alignment, arithmetic, lanes, chunks, wave assignment and the fixed merge order are ssi_attn_decode's, walked over the
 * concatenated key index 0 .. prompt_len + gen_len: the two kernels share the row body, and out and lse are BIT-EQUAL to ssi_attn_decode on a
 * cache in which the row's keys lie one behind the other.  One workgroup per (row, kv head): each beam of a prompt reads the prompt's K / V
 * itself.  Same 8 forms (dtype x G = 1, 2, 4, 8).  ssi_kv_store fills the beam cache unchanged (dest = r * cap_b + t). */
int ssi_attn_decode_beam(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                         const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                         const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                         int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream);

/* ---- Split-KV decode attention (ABI v25; few rows, long caches: one workgroup per (row, kv head) leaves most of the device idle) ---------------
 * ssi_attn_decode / ssi_attn_decode_beam with the keys of a (row, kv head) split over workgroups.  THE DEFINITION, for a row with n keys (the
 * slot form: min(kv_len, cap); the beam form: prompt_len + gen_len after their clamps, the concatenated index) and a span of `span` keys:
 *   walk   grid (rows, n_kv, n_splits).  Workgroup z walks the keys [z * span, min((z + 1) * span, n)) exactly as the plain kernel walks a
 *          cache that starts at key z * span — lanes, loads, chunks, waves, the xor tree and the four-wave merge placed relative to the split's
 *          first key — and writes its merged, UNNORMALISED fp32 state per query head to workspace[r, h, z, :] = (O[head_dim], M, L).  A
 *          workgroup with z * span >= n returns before it reads or writes anything.
 *   merge  grid (rows, n_kv), behind the walk on the same stream.  It reads the S = ceil(n / span) partials z = 0 .. S - 1 of the row and no
 *          other (the workspace is never zeroed), and applies the four-wave merge's formula in that order:
 *              M = max_z M_z;   e_z = (M_z == -inf ? 0 : exp2(M_z - M));   L = fma(L_z, e_z, L);   O_d = fma(O_{z,d}, e_z, O_d)
 *          then the plain kernel's finish: a row all of whose keys were skipped is zeros with lse -inf, otherwise out = O / L with ONE rounding
 *          and lse = (M + log2 L) ln 2.  Dead rows (slot < 0, n <= 0, the slot form's slot >= n_slots) are zeros and -inf, written here.
 * The kernel boundary is the only synchronisation between workgroups: no atomics on values, no ticket, no flag.
 * It follows: a row with n <= span equals the plain entry by VALUE in out and lse (a zero may differ in sign); a row's result is a function of
 * its own query, its own keys, n and span only (not of rows, its place, n_splits or its neighbours); with equal span the beam form equals the
 * slot form on a cache that holds the row's keys one behind the other.  Against the plain entry a row with n > span differs by the merge order.
 * span: a positive multiple of the form's ROUND of 8 loads = 512 / LPK keys (bf16, head_dim 64: 64; fp32, head_dim 64: 32; 16 to 512 over all
 * forms).  n_splits in [1, 65535] with n_splits * span >= cap (the beam form: >= cap_p + min(cap_b, ld_anc)): no key can be dropped.
 * workspace: caller-owned, 16-byte aligned, at least ssi_attn_decode_split_workspace bytes = rows * n_heads * n_splits * (head_dim + 2) * 4.
 * Any of these violated: SSI_ERR_ARG before any launch.  Geometries, dtypes, alignment and every other argument: the plain entries'.
 * Errors are counted as there, once per row: the slot outside the cache by the merge, an index outside its cache in the beam form by the
 * z = 0, kv head 0 workgroup of the walk (over the row's whole ancestry).
 * Forms: the walk per dtype x G = 1, 2, 4, 8 and per key source (16), the merge per dtype (2).  No LDS in the merge, no scratch anywhere. */
/* the default span in keys of a form: max(128, the form's round) — 128 by measurement (README, "Split-KV decode attention"); 0: unsupported */
int ssi_attn_decode_split_span(int head_dim, int dtype);
int64_t ssi_attn_decode_split_workspace(int64_t rows, int n_heads, int head_dim, int64_t n_splits);
int ssi_attn_decode_split(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap,
                          const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv,
                          int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype,
                          void* stream);
int ssi_attn_decode_beam_split(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                               const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                               const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                               int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits,
                               void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* ---- FP8 K/V cache (ABI v26; vLLM's kv_cache_dtype="fp8" is what the reference's users would reach for; opt-in, it changes values) -----------
 * THE DEFINITION.  A cached LINE is the head_dim elements of one (position, kv head) of K (after RoPE, as it sits in qkv) or of V, in the
 * model's dtype (a bf16 model's line is rounded twice, to bf16 and then to fp8: accepted).  It is stored as head_dim e4m3fn CODES (OCP: bias 7,
 * no infinity, NaN = S.1111.111, largest finite 448; not fnuz) and one biased EXPONENT BYTE b:
 *   exponent   a = the largest |x_i| over the line's FINITE elements.  a == 0 or no finite element: b = 127.  Otherwise a = m * 2^E with m in
 *              [1, 2), e = E - 8 if m <= 1.75 else E - 7 (the smallest e with a * 2^-e <= 448), b = clamp(e, -127, 127) + 127.  e comes from
 *              the bits of a (exponent field and mantissa), not from a logarithm; an fp32 subnormal a gives b = 0.
 *   codes      code_i = RNE_e4m3(x_i * 2^-e), the scaling exact (v_ldexp_f32) and nothing above 448, so saturation is never relied on; a NaN
 *              or infinite element stores the NaN code 0x7f (the store writes it itself, whatever the conversion would make of such an input).
 *   value      float(code) * 2^(b - 127): exact in fp32 for every line, and exact in bf16 (four significant bits times a power of two) for every
 *              line with a >= 2^-116 — below that, b - 127 < -124 can put the low bit of a code under bf16's smallest subnormal 2^-133.
 * One power of two per (position, kv head), for K and V separately: neither a per-tensor scale nor an unscaled cast — K after RoPE has outlier
 * channels and positions, and a per-line exponent keeps three mantissa bits on every line; a power of two keeps both directions exact.
 * Storage per layer: k_codes, v_codes uint8 [n_slots, cap, n_kv * head_dim] (16-byte aligned); k_exp, v_exp uint8 [n_slots, cap, n_kv] (no
 * alignment; 1.6 % on top of the codes at head_dim 64).
 *
 * ssi_kv_store_fp8 is ssi_kv_store's contract on these four arrays: dest = -1 skips the row, a dest outside [0, n_dest) is counted once into
 * *n_bad and writes nothing.  A line lies on LPK lanes (head_dim / VEC rounded up to a power of two; VEC = 8 for bf16, 4 for fp32) of 16 bytes
 * of qkv each; the absmax is an xor-shuffle maximum over them; every lane writes its VEC codes at once (8 bytes for bf16, 4 for fp32) and the
 * line's first lane the exponent byte.  No LDS, no atomics on values.  Prefill attention itself runs on the unquantised K / V of the packed
 * forward: only what decode steps read is quantised, the new token's own key included.
 *
 * ssi_attn_decode_fp8, ssi_attn_decode_beam_fp8, ssi_attn_decode_split_fp8 and ssi_attn_decode_beam_split_fp8 are the four entries above with
 * (k_codes, v_codes, k_exp, v_exp) wherever those take (k_cache, v_cache); the beam forms read BOTH caches as fp8.  qkv, out, lse, the workspace,
 * span, n_splits, slot, kv_len, anc and n_bad are unchanged, and so are the checks.  The walk is the plain kernels' (one source): a lane holds the
 * VEC codes of its key where the plain form holds VEC elements (an 8-byte load for bf16, 4 for fp32, plus the line's exponent byte), so lanes,
 * chunks, waves, the xor tree and every merge are the same, and the merge kernel of the split forms is the same kernel.  The value of a code is
 * made ELEMENT BY ELEMENT before the dot product (v_cvt_pk_f32_fp8, v_ldexp_f32: both exact) rather than as one factor on the score and on p:
 * the walk then computes on the very fp32 numbers a plain cache of the dequantised lines would hand it, overflow and subnormals included, for
 * 2 * VEC exact instructions a key beside 2 * G * VEC fmas.  THE CONTRACT: out and lse of an _fp8 entry are BIT-EQUAL to the plain entry's on a
 * cache that holds the dequantised values in the model's dtype (wherever those are exact in it: see "value"), and n_bad counts the same rows.
 * Forms: 8 per attention entry (dtype x G = 1, 2, 4, 8), 2 of the store; no scratch.  A form with more loads in flight would change the bits. */
int ssi_kv_store_fp8(const void* qkv, int64_t ld, const int64_t* dest, int64_t rows, int64_t n_dest, void* k_codes, void* v_codes,
                     void* k_exp, void* v_exp, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream);
int ssi_attn_decode_fp8(const void* qkv, int64_t ld, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                        int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows,
                        int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream);
int ssi_attn_decode_beam_fp8(const void* qkv, int64_t ld, const void* pk_codes, const void* pv_codes, const void* pk_exp, const void* pv_exp,
                             int64_t n_pslots, int64_t cap_p, const void* bk_codes, const void* bv_codes, const void* bk_exp,
                             const void* bv_exp, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len,
                             const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse, int64_t rows, int n_heads,
                             int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream);
int ssi_attn_decode_split_fp8(const void* qkv, int64_t ld, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                              int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows,
                              int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits, void* workspace,
                              int64_t workspace_bytes, int dtype, void* stream);
int ssi_attn_decode_beam_split_fp8(const void* qkv, int64_t ld, const void* pk_codes, const void* pv_codes, const void* pk_exp,
                                   const void* pv_exp, int64_t n_pslots, int64_t cap_p, const void* bk_codes, const void* bv_codes,
                                   const void* bk_exp, const void* bv_exp, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                   const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                                   int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits,
                                   void* workspace, int64_t workspace_bytes, int dtype, void* stream);

/* The k best allowed continuations of every row of logits [rows, ld] with their log-probabilities (ABI v20, beam search).  Logits read only.
 * mask: ssi_decode_select's bit mask (mask_words = ceil(vocab / 32) int32 words, bit c % 32 of word c / 32), or NULL with mask_words 0 = every
 * real column.
 *   idx[r, j], j < k : the columns of the k largest STORED values among the allowed columns below vocab, by value descending, the lower column
 *                      first among equal values (-0 equals +0); a NaN ranks below every number, -inf included.  Exact: values are compared as
 *                      stored, nothing is rounded.  Fewer than k allowed columns: the rest are -1.
 *   lse[r]           : log sum_{c < vocab} exp x[c] over ALL real columns, allowed or not (NULL ok) — ssi_decode_select's normaliser, term for
 *                      term: exp2(fma(x, log2 e, nm)), nm = fl(-max log2 e), lse = fl(max + logf(sum)).
 *   lp[r, j]         : fl(x[idx] - lse); -inf where idx is -1.  On a row holding NaN or an infinity lse and lp are unspecified; idx is not.
 * One workgroup of 256 threads per row, two walks (max and per-thread sorted lists of K = 1, 2, 4 or 8 candidates in registers; exp-sum), then k
 * rounds that pick the best list head by ssi_decode_select's fixed tree.  No workspace, no atomics; a row's result depends on that row and the
 * mask only.  idx[r, 0] is ssi_decode_select's token on the same inputs.
 * SSI_ERR_ARG before any launch: k outside 1..8, a NULL mask with mask_words != 0 or a mask with another length, null logits / idx / lp,
 * vocab < 1, ld < vocab, vocab or rows >= 2^31.  rows == 0 launches nothing. */
int ssi_topk_logprob(const void* logits, int64_t ld, int64_t rows, int64_t vocab, int k, const uint32_t* mask, int64_t mask_words,
                     int32_t* idx, float* lp, float* lse, int dtype, void* stream);

/* The token of a decode step under a constraint (ABI v19; vLLM's allowed_token_ids and min_tokens, which the reference's generation can set):
 * the greedy choice among the ALLOWED columns of every row of logits [rows, ld], with its log-probability and its rank under the row's
 * UNCONSTRAINED distribution.  The logits are read only.
 * allow / allow_early: bit masks of ceil(vocab / 32) words, bit c % 32 of word c / 32 set = column c may be chosen; either may be NULL = every
 * real column.  Row r uses allow_early when n_generated != NULL && n_generated[r] < min_new, else allow (the host builds allow_early as allow
 * without the stop tokens: a row cannot end before it holds min_new tokens).
 *   token[r]   = the smallest allowed c < vocab whose stored value is the maximum over the allowed columns (torch's first-occurrence argmax of
 *                the masked row);
 *   logprob[r] = x[token] - log sum_{c < vocab} exp x[c], the sum over ALL real columns, allowed or not: comparable across constraint settings,
 *                and what ssi_ce_fwd_metrics gives as -row_nll with the token as label;
 *   rank[r]    = #{c < vocab : x[c] > x[token]} + #{c < token : x[c] == x[token]} over all real columns, on the stored values: row_rank of
 *                ssi_ce_fwd_metrics with the token as label.  rank == 0 <=> the constraint did not change the choice.
 * logprob and rank may be NULL.  A row whose mask has no bit set below vocab: token = -1, logprob = 0, rank = -1.  token is ALWAYS an allowed
 * column or -1, also on a row with NaN or +-inf logits (it is the next step's embedding index); what else such a row returns is unspecified.
 * Pad columns [vocab, ld) never count, whatever they hold.
 * Arithmetic: the header's rule — max, exp-sum and log in fp32, ONE rounding on the store: a term of the sum is exp2(fma(x, log2 e, nm)) with
 * nm = fl(-max log2 e) (v_exp_f32), logprob = fl(x[token] - fl(max + logf(sum))).
 * One workgroup of 256 threads per row, no workspace, no atomics.  The row is walked twice (max and allowed argmax; exp-sum and rank), 16-byte
 * loads when logits and ld * sizeof(element) are 16-byte aligned and a scalar tail over the last vocab % (16 / sizeof(element)) columns, scalar
 * loads throughout otherwise.  (value, column) pairs are merged in a fixed order with the lower column winning: a thread meets its columns in
 * rising order, the threads of a wave by an xor tree, the four waves in the order 0..3; the exp-sum by the same trees.  A row's result depends
 * on that row and the masks only — not on rows, not on the row's place, not on other rows.
 * SSI_ERR_ARG: null logits or token, vocab < 1, ld < vocab, vocab >= 2^31, rows >= 2^31, min_new < 0.  rows == 0 launches nothing. */
int ssi_decode_select(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                      const int32_t* n_generated, int32_t min_new, int64_t* token, float* logprob, int32_t* rank, int dtype, void* stream);

/* The sampled token of a decode step (ABI v21; vLLM's temperature, top_k, top_p and seed): a draw from softmax(x / T) of every row of logits
 * [rows, ld], restricted by ssi_decode_select's masks, top-k and top-p, as a pure function of (seed, sequence[r], step) and the row.  The logits
 * are read only.  Per row, on the STORED values, with the mask the row takes (allow_early while n_generated[r] < min_new; NULL = every column):
 *   A  = the allowed columns below vocab.  Values are ordered as ssi_topk_logprob orders them: NaN below every number, -0 with +0.
 *   K  = {c in A : x_c >= tk}, tk the top_k-th largest value of A counted with multiplicity, when 0 < top_k < |A| (ties at the threshold all
 *        stay: vLLM's `logits < kth` mask); K = A when top_k <= 0 or top_k >= |A|.
 *   P  = {c in K : x_c >= tp} when top_p < 1: with w_c = exp((x_c - m) / T), m = max_K x, Z = sum_K w and M(v) = sum_{c in K, x_c >= v} w_c,
 *        tp is the largest value v occurring in K with M(v) >= top_p Z — the fewest whole value classes, from the top, that reach top_p, after
 *        top-k and renormalised over K (vLLM's order).  The class of the maximum is always kept.  P = K when top_p >= 1.
 *   token[r]   = argmax_{c in P} (x_c / T + G_c), the lowest column on a tie (Gumbel-max: exactly a draw from softmax(x / T) over P), with
 *                G_c = -ln(-ln u_c), u_c = (2 (w_c >> 9) + 1) 2^-24, w_c word c & 3 of Philox4x32-10 with counter (c >> 2, step, sequence[r],
 *                0x53414D50) and key (seed low word, seed high word).  u is an odd multiple of 2^-24, exact in fp32: G lies in [-2.82, 16.64].
 *                A NaN or -inf column is never drawn while a column of A holds a number above -inf; when none does, the token is the FIRST
 *                allowed column (ssi_decode_select's rule) and P is that column alone.
 *   logprob[r] = x[token] - log sum_{c < vocab} exp x[c] over ALL real columns at T = 1: ssi_decode_select's, term for term (NULL ok).
 *   n_kept[r]  = |P| (NULL ok).
 * A row with nothing allowed below vocab: token = -1, logprob = 0, n_kept = -1.  A +inf in an allowed column makes the masses of top-p
 * meaningless (P is then K); the token is still an allowed column.
 * Arithmetic: the score is fma(x, fl(1 / T), G) with -ln u = -logf(u) below 1/2 and -log1pf(u - 1) from there on (u - 1 is exact).  A mass is
 * exp2(fma(x, sc, nm)), sc = fl(log2 e / T), nm = fl(-m sc) (a NaN counts 0), times 2^40 and truncated to an integer; masses are summed as
 * 64-bit integers (LDS atomics: the order of arrival cannot matter), and M(v) >= top_p Z is the integer compare M >= ceil(top_p Z) with the
 * product in fp64.
 * One workgroup of 256 threads per row; no workspace.  Walks of the row: 2 (the maxima; exp-sum and draw) with top_k <= 0 and top_p >= 1; with
 * either, a radix select on the values' unsigned order adds 8-bit passes of LDS histograms (counts and masses): 2 passes per threshold for
 * bf16, 4 for fp32.  In the draw a column's logarithms are skipped where the largest G its word's leading ones allow cannot lift it above a score
 * already reached, which cannot change the result.  A row's outputs depend on that row, the masks and the scalars only.
 * SSI_ERR_ARG before any launch: temperature not finite or <= 0, top_p outside (0, 1], a NULL sequence, and everything ssi_decode_select
 * refuses.  rows == 0 launches nothing. */
int ssi_decode_sample(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                      const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed, uint32_t step,
                      const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept, int dtype, void* stream);

/* ssi_decode_select and ssi_decode_sample under vLLM's repetition, frequency and presence penalties (ABI v22; `apply_penalties`).  For row r
 *   H   = the token ids of the row's prompt and of its generated tokens so far,
 *   n_c = the number of times c occurs among the GENERATED tokens only,
 * and the penalised value of column c, formed in fp32 from the stored value x_c wherever it is used and never stored, is
 *   a_c = 1 for c outside H;  fl(1 / r), rounded once from the double quotient on the host, for c in H with x_c > 0;  fl(r) for c in H
 *         otherwise (0, the negatives and NaN: vLLM's where(x > 0, x / r, x * r));
 *   t_c = fma(f, (float)n_c, n_c > 0 ? p : 0)     (0 when n_c == 0);
 *   y_c = fma(x_c, a_c, -t_c)                     (a column outside H is not touched: y_c is x_c),
 * with r = repetition_penalty (finite, > 0), f = frequency_penalty and p = presence_penalty (both in [-2, 2]).  The two fmas are the only
 * roundings.  x fl(1 / r) differs from vLLM's x / r by at most one ulp of the factor (half an ulp from rounding 1 / r, half from the product
 * against the quotient).  With r = 1, f = 0, p = 0, y_c == x_c bit for bit.
 * Everything that SELECTS uses y in place of x, everything that REPORTS stays on x:
 *   ssi_decode_select_pen: token = the first maximum of y over the allowed columns (the first allowed column on a row without a number);
 *     logprob = x[token] - lse(x) over all real columns, term for term ssi_decode_select's; rank = the token's rank in the RAW row, 0
 *     exactly when neither the mask nor the penalties changed the choice.
 *   ssi_decode_sample_pen: A, K, P, the masses and the score fma(y, fl(1 / T), G) are on y (penalties come before temperature, top-k and
 *     top-p: vLLM's order); logprob stays on x at T = 1; n_kept = |P|; the Philox counter, tag and u are ssi_decode_sample's.  y is an fp32
 *     value whatever the storage, so the radix select runs on the 32-bit key: 4 passes per threshold for bf16 logits, too.
 * History: prompt_ids is int32 [n_prompts, ld_prompt]; row r reads the first prompt_len[line] ids (clamped to [0, ld_prompt]) of line
 * prompt_row ? prompt_row[r] : r — the n samples of a prompt share one line, as they share its K / V.  gen_ids is int64 [rows, ld_gen] (the
 * generation loop's output tensor); row r reads its first n_generated[r] entries (clamped to [0, ld_gen]), so n_generated is required here;
 * it also picks allow_early as in the plain entries.  An id outside [0, vocab), or a line outside [0, n_prompts), is tested BEFORE any
 * address is formed from it: it is skipped (the line: the whole prompt), and the row is counted ONCE in *n_bad (NULL ok) —
 * ssi_attn_decode_beam's rule.
 * Per workgroup (one row, 256 threads), before the first walk, in dynamic LDS: a bit mask of ceil(vocab / 32) words ("c is in H", LDS
 * atomicOr) and an open-addressing table of Hs (token + 1, count) pairs, slot = token mod Hs, linear probing, Hs = the smallest power of two
 * >= 2 ld_gen and >= 64 (LDS atomicCAS / atomicAdd: integer sums, no order).  A walk reads the bits of a 16-byte vector with one LDS load and
 * looks a column up (O(1) expected) only where its bit is set.  The dynamic LDS is
 *   ssi_decode_penalty_lds_bytes(vocab, ld_gen) = 4 ceil(vocab / 32) + 8 Hs      (20 768 bytes at vocab 133 376, ld_gen 256)
 * and at most SSI_DECODE_PENALTY_LDS_MAX (64 KB less 8 KB for the kernels' static LDS); more is SSI_ERR_UNSUPPORTED before the launch.
 * SSI_ERR_ARG before any launch: r not finite or <= 0; f or p not finite or outside [-2, 2]; a NULL n_generated or prompt_len; a NULL gen_ids
 * with ld_gen > 0 or a NULL prompt_ids with ld_prompt > 0; ld_gen < 0, ld_prompt < 0, n_prompts < 1; and everything the plain entry refuses.
 * rows == 0 launches nothing.  No workspace, no scratch; a row's outputs depend on that row, its history, the masks and the scalars only. */
#define SSI_DECODE_PENALTY_LDS_MAX 57344
int64_t ssi_decode_penalty_lds_bytes(int64_t vocab, int64_t ld_gen);
int ssi_decode_select_pen(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                          const int32_t* n_generated, int32_t min_new, int64_t* token, float* logprob, int32_t* rank,
                          const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len, const int32_t* prompt_row, int64_t n_prompts,
                          const int64_t* gen_ids, int64_t ld_gen, double repetition_penalty, double frequency_penalty, double presence_penalty,
                          int32_t* n_bad, int dtype, void* stream);
int ssi_decode_sample_pen(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                          const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed,
                          uint32_t step, const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept,
                          const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len, const int32_t* prompt_row, int64_t n_prompts,
                          const int64_t* gen_ids, int64_t ld_gen, double repetition_penalty, double frequency_penalty, double presence_penalty,
                          int32_t* n_bad, int dtype, void* stream);

/* ssi_decode_sample and ssi_decode_sample_pen with the step and the draw parameters PER ROW (ABI v28): rows of one launch that are at different
 * steps of their sequences (a refilled pool) or belong to requests with different settings.  Four device arrays of one entry per row:
 *   step              uint32, required;
 *   temperature_rows  double, NULL ok: the scalar `temperature` then holds for all rows;
 *   top_k_rows        int64,  NULL ok: the scalar `top_k`;
 *   top_p_rows        double, NULL ok: the scalar `top_p`.
 * THE DEFINITION: row r has the bits of row r of the scalar entry launched with (temperature[r], top_k[r], top_p[r], step[r]) — token, logprob
 * and n_kept.  fl(1 / T) and fl(log2 e / T) are formed on the device by the scalar entry's host expression, an IEEE fp64 quotient rounded once
 * to fp32.  One workgroup owns one row, so whether the radix passes run is uniform over it.
 * A row whose temperature is not finite and > 0, or whose top_p lies outside (0, 1], fails by itself: it writes what a row with nothing allowed
 * writes (token -1, logprob 0, n_kept -1) and, in the penalised form, builds no history and counts nothing into *n_bad; no other row changes.
 * SSI_ERR_ARG before any launch: a NULL step; a scalar outside its range where its array is NULL (with the array, the scalar is not read);
 * and everything the scalar entry refuses otherwise. */
int ssi_decode_sample_rows(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                           const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed,
                           const uint32_t* step, const double* temperature_rows, const int64_t* top_k_rows, const double* top_p_rows,
                           const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept, int dtype, void* stream);
int ssi_decode_sample_pen_rows(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                               const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed,
                               const uint32_t* step, const double* temperature_rows, const int64_t* top_k_rows, const double* top_p_rows,
                               const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept,
                               const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len, const int32_t* prompt_row, int64_t n_prompts,
                               const int64_t* gen_ids, int64_t ld_gen, double repetition_penalty, double frequency_penalty, double presence_penalty,
                               int32_t* n_bad, int dtype, void* stream);

/* ---- K7  SwiGLU elementwise (torchtune FeedForward: w2(silu(w1 x) * w3 x)) ------------------------------------------ */
/* gu: [rows, 2*inter] = [gate | up]; act[rows, inter] = silu(gate) * up */
int ssi_swiglu_fwd(const void* gu, void* act, int64_t rows, int64_t inter, int dtype, void* stream);
int ssi_swiglu_bwd(const void* dact, const void* gu, void* dgu, int64_t rows, int64_t inter, int dtype, void* stream);

/* ---- K3/K6/K7/K8/K10  dense GEMMs (F.linear and its autograd) ------------------------------------------------------- */
/* C = (accumulate ? C : 0) + alpha * (alpha_dev ? *alpha_dev : 1) * op(A) op(B) + (R ? R : 0)
 * A, B, C, R share `dtype`; accumulation is fp32.  R (residual) has C's shape and ldc.  The bf16 MFMA path needs
 * dtype == SSI_BF16, M % 256 == 0, N % 256 == 0, K % 64 == 0 and 16-byte aligned rows.  The fp32 MFMA path (fp32-input
 * matrix instruction, exact fp32) needs dtype == SSI_F32 and N % 128 == 0; M and K are arbitrary, and it returns the
 * same bits as the generic path: one fmaf chain per element, k ascending from 0.  Otherwise the generic path runs (or
 * SSI_ERR_UNSUPPORTED if SSI_IMPL_MFMA / SSI_IMPL_MFMA_WG8 was forced). */
int ssi_gemm(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
             void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev, int accumulate, int dtype,
             void* stream);

/* Split-K variant for long-K / small-output contractions (weight gradients): `splits` K-slices into fp32 slabs in
 * `workspace` (ssi_gemm_splitk_workspace_bytes), then one reduction pass with the same epilogue as ssi_gemm. */
int64_t ssi_gemm_splitk_workspace_bytes(int64_t M, int64_t N, int splits);
int ssi_gemm_splitk(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                    void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev, int accumulate, int dtype,
                    int splits, void* workspace, int64_t workspace_bytes, void* stream);

/* `batch` GEMMs of one shape in ONE launch: problem b works on A + b strideA, B + b strideB, C + b strideC (strides in elements, no
 * residual).  For contractions whose output grid cannot fill the 256 CUs but which come in independent copies: the weight gradients
 * of the square projections (F.linear's autograd for attn.output_proj: 64 output tiles, fused q/k/v_proj: 96) of several LAYERS,
 * which the model defers until a group of layers has finished its backward — at full K, with no fp32 partials and no reduction pass.
 * MFMA path: SSI_GEMM_TN, bf16, ssi_gemm's shape rules, K % 128 == 0; anything else runs as `batch` ssi_gemm calls (same results). */
int ssi_gemm_batched(int layout, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t strideA, const void* B,
                     int64_t ldb, int64_t strideB, void* C, int64_t ldc, int64_t strideC, float alpha, const float* alpha_dev,
                     int accumulate, int dtype, void* stream);

/* Fused SwiGLU GEMMs (torchtune FeedForward and its autograd): the elementwise stage rides in the GEMM epilogue on the MFMA
 * path (bf16, M % 256 == 0, I % 256 == 0, K % 64 == 0); otherwise the unfused kernels run.  Same rounding points either way.
 *   fwd: GU[M, 2I] = X[M, K] W13[2I, K]^T  (W13 = [gate rows | up rows]),  ACT[M, I] = silu(gate) * up
 *   bwd: DGU[M, 2I] = swiglu_backward(DY[M, K] W2, GU);  W2 as [I, K] (layout SSI_GEMM_NT) or [K, I] (SSI_GEMM_NN);
 *        dact_ws: [M, I] scratch used only by the unfused fallback. */
int ssi_gemm_swiglu_fwd(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw, void* GU,
                        int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream);
int ssi_gemm_swiglu_bwd(int layout, int64_t M, int64_t inter, int64_t K, const void* DY, int64_t lddy, const void* W2, int64_t ldw,
                        const void* GU, int64_t ldgu, void* DGU, int64_t lddgu, void* dact_ws, int dtype, void* stream);

/* ---- Skinny GEMMs (ABI v24; small-batch decoding: one prompt, n samples, a few beams) -----------------------------------------------------
 * C[M, N] = A[M, K] W[N, K]^T (the NT layout), bf16 in and out, fp32 accumulation on v_mfma_f32_16x16x32_bf16, for 1 <= M <= 64: W is
 * streamed once, no 256-row tile is filled.  A workgroup owns 16 weight rows (64 from N = 8192; SwiGLU: 32 gate + the 32 matching
 * up rows) and every row of A, so A is read from L2 M / 16 (M / 64) times as often as W from HBM; its 8 or 4 waves share K in chunks of
 * 64 and their partial sums are added in LDS in a fixed order — no atomics, no workspace, one launch.  The split depends on N alone: row r of C is BIT-EQUAL whatever M is and wherever r lies among the rows, and equal in every launch.  Rows >= M of A, R and positions are never read; nothing outside [M, N] of the outputs is written.
 * Epilogues, with the rounding points of the 256-tile kernels they stand in for (on exactly representable data the results are bit-equal):
 *   ssi_gemm_skinny         bf16(sum);  R != NULL ([M, N] at ldc): bf16(float(bf16(sum)) + R)                      = ssi_gemm(NT, ..., R)
 *   ssi_gemm_skinny_rope    ssi_rope_inplace's rotation of heads [0, n_heads_rot) of the bf16-rounded row by positions[row] = ssi_gemm_rope;
 *                           positions is required and clamped to [0, table_len - 1] ON THE DEVICE (no read-back, nothing indexed past the table)
 *   ssi_gemm_skinny_swiglu  W13 = [gate rows | up rows]: ACT[M, I] = bf16(float(bf16(silu(gate))) * up) on the bf16-rounded gate and up
 *                           = ssi_gemm_swiglu_fwd; GU[M, 2 I] = [gate | up] is written only when GU != NULL (a decode step reads it nowhere)
 * SSI_ERR_UNSUPPORTED before any launch: dtype != SSI_BF16, M outside 0..64, N % 64, K % 64 (SwiGLU: I % 64), head_dim != 64, rotated
 * columns beyond N.  SSI_ERR_ARG: a null pointer, a leading dimension below the row length, a base or a leading dimension that leaves rows
 * off 16-byte boundaries.  M == 0 launches nothing. */
#define SSI_GEMM_SKINNY_MAX_ROWS 64
int ssi_gemm_skinny(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                    const void* R, int dtype, void* stream);
int ssi_gemm_skinny_rope(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                         int n_heads_rot, int head_dim, const float* rope_table, int64_t table_len, const int32_t* positions, int dtype,
                         void* stream);
int ssi_gemm_skinny_swiglu(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw, void* GU,
                           int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream);

/* ---- FP8 weights (ABI v27; vLLM's quantization="fp8" is what the reference's users would reach for; small-batch decoding only; opt-in, it
 * changes values) ----------------------------------------------------------------------------------------------------------------------------
 * THE DEFINITION is the "FP8 K/V cache" rule above with "line" read as ROW OF A WEIGHT MATRIX W[N, K], the K elements of one output channel:
 * K e4m3fn codes and one biased exponent byte b per row, the exponent, the codes and the value of a code exactly as that section says (and as
 * one copy of device code, csrc/q8_codes.h, computes them for both).  Storage: codes uint8 [N, ld_codes] (rows on 16-byte boundaries),
 * exps uint8 [N] (no alignment).  A dequantised weight has four significant bits, so it is EXACTLY a bf16 number whenever it is a normal bf16
 * number or zero; rows whose non-zero values fall below the bf16 normal range (2^-126) are outside the guarantee below.
 *
 * ssi_weight_quant_fp8: bf16 W[N, K] at ldw -> codes, exps.  One wave per row: a pass for the row's absmax, a pass (from L2) for the codes.
 * Nothing behind column K of a code row is written.  SSI_ERR_UNSUPPORTED: dtype != SSI_BF16, K % 64; SSI_ERR_ARG: a null pointer, a leading
 * dimension below K, rows of W or of the codes off 16-byte boundaries.  N == 0 launches nothing.
 *
 * ssi_gemm_skinny_w8, ssi_gemm_skinny_rope_w8 and ssi_gemm_skinny_swiglu_w8 are the three skinny entries with (codes, ld_codes, exps) where
 * those take (W, ldw); every other argument, the epilogues' rounding points, the refusals (ld_codes in place of ldw: >= K, 16-byte rows) and
 * "row r has the same bits whatever M is" are unchanged.  THE CONTRACT: the output is BIT-EQUAL to the matching plain entry called on the
 * dequantised matrix stored as bf16.  So the k of a lane slot, the wave of a 64-wide chunk, the order of the matrix instructions within a wave
 * and the LDS merge are skinny_kernel's (the merge, the epilogues and the refusals are one copy of code, csrc/gemm_skinny.h); a lane's 16 codes of a chunk and row come in ONE 16-byte
 * load and become the two bf16x8 operands by v_cvt_pk_f32_fp8, v_ldexp_f32 and v_cvt_pk_bf16_f32, all exact: the row's exponent is applied AT
 * THE CONVERSION, not to the fp32 sums.  Free, and used: two of a wave's chunks are in flight, which keeps the bf16 kernel's bytes in flight
 * per lane.  exps is read at rows [0, N) only (SwiGLU: [0, 2 I)).  Forms: 12, as skinny_kernel's; no scratch.  The bf16 weights are not
 * freed by anything here, and prefill and the 256-row tile path never read the codes. */
int ssi_weight_quant_fp8(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ld_codes, void* exps, int dtype, void* stream);
int ssi_gemm_skinny_w8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* codes, int64_t ld_codes, const void* exps,
                       void* C, int64_t ldc, const void* R, int dtype, void* stream);
int ssi_gemm_skinny_rope_w8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* codes, int64_t ld_codes, const void* exps,
                            void* C, int64_t ldc, int n_heads_rot, int head_dim, const float* rope_table, int64_t table_len,
                            const int32_t* positions, int dtype, void* stream);
int ssi_gemm_skinny_swiglu_w8(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* codes13, int64_t ld_codes,
                              const void* exps13, void* GU, int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream);

/* dst[c][r] = src[r][c] for a [rows, cols] matrix (both dims multiples of 8).  Keeps [in, out] copies of the projection
 * weights so that the data-gradient GEMMs use the k-contiguous operand form (refreshed once per optimizer step). */
int ssi_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols, int dtype,
                  void* stream);

/* ---- K9  CEWithChunkedOutputLoss (ssi/trainer.py:300; F.cross_entropy(logits.float(), reduction="sum")) -------------- */
/* logits: [rows, ld] (columns [0, vocab) are real, [vocab, ld) padding).  labels: already shifted (ssi/loss.py:16).
 * row_loss[r] = lse(logits[r]) - logits[r, label] (0 if ignored).  If write_grad: logits[r, :] is OVERWRITTEN by
 * softmax(logits[r]) - onehot(label) (0 for ignored rows and for padding columns) — the unscaled d(sum NLL)/dlogits. */
int ssi_ce_fwd(void* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t vocab, int64_t ignore_index,
               float* row_loss, float* row_lse, int write_grad, int dtype, void* stream);
/* bf16 rows of up to 196 608 columns are held in registers by one workgroup per CU: the log-sum-exp and the gradient come from ONE
 * read of the row (2 passes over the logits, not 3).  A label that is neither `ignore_index` nor inside [0, vocab) gives a zero
 * loss and a zero gradient row here and is COUNTED by ssi_ce_reduce (out[3]): the caller raises when it next reads back.
 * All five ssi_ce_fwd* entries move the rows 16 bytes at a time in either form: `logits` (and the `teacher` of ssi_ce_fwd_kl) must be
 * 16-byte aligned, SSI_ERR_ARG otherwise and nothing is launched (ld % 8 == 0 then aligns every row). */
/* out[0] = sum(row_loss) / n_valid (NaN if n_valid == 0, as the reference), out[1] = sum(row_loss), out[2] = n_valid (labels that
 * are not ignored and lie in [0, vocab) — the predicate ssi_ce_fwd uses), out[3] = number of out-of-range labels.  out: 4 floats. */
int ssi_ce_reduce(const float* row_loss, const int64_t* labels, int64_t rows, int64_t vocab, int64_t ignore_index, float* out,
                  void* stream);
/* ssi_ce_fwd with a weight per row (NULL: all 1, and then bit-identical to ssi_ce_fwd): row_loss[r] = w[r] (lse - logit[label]), gradient row
 * w[r] (softmax - onehot); w >= 0.  The reference normalises every micro-batch of an accumulation window by ITS OWN count of shifted labels and
 * weights it by its own count of unshifted ones (ssi/trainer.py:385-395 with ssi/loss.py:16-22); a window that runs as one batch carries that
 * ratio per row here.  In the register-resident bf16 kernel the weight is an additive term of the exponent: no cost per element. */
int ssi_ce_fwd_weighted(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                        int64_t ignore_index, float* row_loss, float* row_lse, int write_grad, int dtype, void* stream);
/* ssi_ce_fwd_weighted with the auxiliary z-loss z_coeff * log^2 Z (ABI v12; not in the reference, off by default: the trainer's z_loss_coeff).
 * With lse = logsumexp(logits[r, 0:vocab]), p = softmax and w = row_weight[r] (NULL: 1), for a row with a valid label:
 *   row_loss[r] = w (lse - logit[label])      what ssi_ce_fwd_weighted writes, bit for bit (row_lse too, NULL ok): the same form is chosen by the
 *                                             same predicate, with the same order of max, exp-sum and lse;
 *   row_z[r]    = w (lse lse)                 fp32, in this order, WITHOUT z_coeff (required);
 *   gradient    = w (f p - onehot(label)),    f = 1 + 2 z_coeff lse   (if write_grad; over the logits, pad columns 0).
 * A row whose label is ignored or outside [0, vocab): row_loss = row_z = 0 and a zero gradient row.  The batch objective is
 * (sum row_loss + z_coeff sum row_z) / n_valid: run ssi_ce_reduce on row_loss and again on row_z (out[1] is the fixed-order sum).
 * z_coeff must be finite and >= 0 (SSI_ERR_ARG otherwise); z_coeff == 0 gives the gradient of ssi_ce_fwd_weighted bit for bit (row_z is still
 * written).  f may be zero or negative (lse < -1 / (2 z_coeff)): in the register-resident bf16 kernel |f| is an additive term of the exponent,
 * like the weight, and the sign is one XOR per packed register — one store per row and four integer operations per 8 columns more. */
int ssi_ce_fwd_z(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab, int64_t ignore_index,
                 float z_coeff, float* row_loss, float* row_lse, float* row_z, int write_grad, int dtype, void* stream);
/* ssi_ce_fwd_z with label smoothing (ABI v14; not in the reference, off by default: the trainer's label_smoothing): the target distribution is
 * (1 - e) onehot(label) + e / vocab, e = smoothing.  With lse, p, w as above, f = 1 + 2 z_coeff lse, and sx = the fp32 sum of logit[c] over
 * c < vocab in a fixed order, for a row with a valid label:
 *   row_loss[r], row_lse[r]  what ssi_ce_fwd_weighted writes, bit for bit (row_lse NULL ok);
 *   row_z[r]    = w (lse lse)                     what ssi_ce_fwd_z writes; may be NULL only when z_coeff == 0;
 *   row_u[r]    = w (lse - sx / (float)vocab)     the uniform part, WITHOUT the coefficient (required);
 *   gradient    = w (f p[c] - (1 - e) [c == label]) - wu  on the real columns, wu = w * (smoothing / (float)vocab) and 1 - e = 1.f - smoothing
 *                 in fp32 in this order (a column whose p underflows holds exactly the rounding of -wu); pad columns stay 0.
 * A row whose label is ignored or outside [0, vocab): row_loss = row_u = row_z = 0 and a zero gradient row.  The batch objective is
 * ((1 - e) sum row_loss + e sum row_u + z_coeff sum row_z) / n_valid, the loss of torch's cross_entropy(label_smoothing = e) plus the z part: one
 * ssi_ce_reduce per sum.  smoothing must be finite and in [0, 1), z_coeff finite and >= 0 (SSI_ERR_ARG otherwise).  smoothing == 0 gives the
 * buffer, row_loss, row_lse and row_z of ssi_ce_fwd_z(z_coeff) bit for bit (minus an exact 0, times an exact 1: no branch), and with
 * z_coeff == 0 as well the buffer of ssi_ce_fwd_weighted.  In the register-resident bf16 kernel: one plain sum over the row registers beside
 * the exp-sum, one more block reduction per row, and one subtract per column. */
int ssi_ce_fwd_smooth(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                      int64_t ignore_index, float smoothing, float z_coeff, float* row_loss, float* row_lse, float* row_u, float* row_z,
                      int write_grad, int dtype, void* stream);
/* ssi_ce_fwd_weighted with a penalty kl_coeff * KL(teacher || student) on the row's distribution (ABI v15; not in the reference, off by default:
 * the trainer's teacher_kl_coeff).  `teacher` is a second [rows, ld_teacher] buffer of the same dtype, the logits of a frozen model on the same
 * rows; it is read only and must not be `logits`.  `teacher_lse[r]` is its log-sum-exp over [0, vocab): an INPUT, what
 * ssi_ce_fwd(teacher, ..., write_grad = 0, row_lse = teacher_lse) writes with the same labels (0 on a row without a valid label, skipped here).
 * With x, lse, p, w as above, t the teacher row, q = exp(t - teacher_lse[r]), k = row_kl_weight[r] (NULL: w) and b = kl_coeff, for a row with
 * a valid label:
 *   row_loss[r], row_lse[r]  what ssi_ce_fwd_weighted writes, bit for bit (row_lse NULL ok): the same statements for max, exp-sum and lse;
 *   row_kl[r]   = k sum_c q[c] ((t[c] - x[c]) - (teacher_lse[r] - lse))     = k KL(q || p), fp32, WITHOUT kl_coeff (required);
 *   gradient    = (w + b k) p[c] - w [c == label] - b k q[c]                (if write_grad; over the logits, pad columns [vocab, ld) exactly 0).
 * A row whose label is ignored or outside [0, vocab): row_loss = row_kl = 0 and a zero gradient row — the KL term lives on labelled rows only,
 * so one n_valid divides every part.  The batch objective is (sum row_loss + kl_coeff sum row_kl) / n_valid: one ssi_ce_reduce per sum.
 * kl_coeff must be finite and >= 0; NULL teacher, teacher_lse or row_kl, teacher == logits, ld_teacher < vocab or not a multiple of 8:
 * SSI_ERR_ARG.  kl_coeff == 0 gives the buffer of ssi_ce_fwd_weighted bit for bit (minus an exact 0; row_kl is still written).  The pad columns
 * of either buffer may hold anything.  bf16 buffers that both meet the register form's conditions, with ld_teacher == ld, take it: the student
 * row lives in registers as before, and with both lse known ONE pass over the teacher row (16 bytes per lane and chunk, three chunks in
 * flight) gives row_kl and the gradient — no second row in registers, no online rescaling.  Everything else takes the generic form, which sums
 * row_kl in fp64 and takes the rounding of the two fp32 lse out of it: with Q = exp(t - teacher_lse[r]), S = sum Q and SP = sum exp(x - lse) (both 1
 * up to that rounding), row_kl = k (sum_c Q[c] (t[c] - x[c]) / S - (teacher_lse[r] - lse) - log S + log SP), rounded to fp32 once.  Traffic:
 * student read + write, teacher read twice (once by the lse launch, once here). */
int ssi_ce_fwd_kl(void* logits, int64_t ld, const void* teacher, int64_t ld_teacher, const float* teacher_lse, const int64_t* labels,
                  const float* row_weight, const float* row_kl_weight, int64_t rows, int64_t vocab, int64_t ignore_index, float kl_coeff,
                  float* row_loss, float* row_lse, float* row_kl, int write_grad, int dtype, void* stream);
/* Forward-only ssi_ce_fwd_weighted that also ranks the label (ABI v10; the dev set's loss and accuracy per token type, ssi/eval.py).  The logits
 * are read only.  row_loss and row_lse (NULL ok) are what ssi_ce_fwd_weighted(..., write_grad = 0) writes on the same inputs, bit for bit: the
 * same form (register-resident bf16 rows or the generic kernel) is chosen by the same predicate, with the same order of max, exp-sum and lse.
 *   row_nll[r]  = lse - logit[label], WITHOUT row_weight (per-type metrics are plain token-level sums);
 *   row_rank[r] = #{c < vocab : x[c] > x[label]} + #{c < label : x[c] == x[label]}: the label's position in a stable descending sort of
 *                 the row, compared on the stored values (an exact integer).  rank == 0 <=> argmax(row) == label with torch's
 *                 first-occurrence rule; rank < k <=> top-k.
 * A row whose label is ignored or outside [0, vocab): row_nll = 0, row_rank = -1.  Pad columns [vocab, ld) never count.  The rank of a row
 * with NaN logits is unspecified (its loss is NaN).  One compare-and-count pass over the row registers and an integer block sum per row. */
int ssi_ce_fwd_metrics(const void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                       int64_t ignore_index, float* row_loss, float* row_lse, float* row_nll, int32_t* row_rank, int dtype, void* stream);
/* Per-type sums of what ssi_ce_fwd_metrics wrote.  ranges: n_ranges (<= 8) inclusive [lo, hi] pairs as in ssi_count_tokens, matched against
 * the LABEL.  out: double [n_ranges + 1][4] = {n_labels, sum nll, n(rank == 0), n(rank < topk)}; rows 0..n_ranges-1 are the ranges, the last
 * row is every valid label (also those in no range).  A row counts iff row_rank >= 0.  fp64 sums in a fixed order, no atomics: bitwise
 * reproducible.  accumulate != 0 adds to what out holds (one device accumulator per dev set, one read-back); 0 overwrites.  One workgroup. */
int ssi_ce_metrics_reduce(const float* row_nll, const int32_t* row_rank, const int64_t* labels, int64_t rows, const int64_t* ranges,
                          int n_ranges, int topk, int accumulate, double* out, void* stream);
/* Per-sequence sums of what ssi_ce_fwd_metrics wrote.  Sequence i covers the flat positions [seq_start[i], seq_end[i]) of row_nll / row_rank
 * (device arrays of n_seq int64 each; the kernel clamps seq_end to [0, rows] and seq_start to [0, seq_end]).  Sequences need not tile the
 * rows, may overlap and need not be sorted.  out: double [n_seq][4] = {n_labels, sum nll, n(rank == 0), n(rank < topk)}, overwritten; a
 * position counts iff row_rank >= 0 (the predicate of ssi_ce_metrics_reduce); an empty sequence gives four zeros.  One wave per sequence,
 * four per workgroup: fp64 per lane in position order, one fixed xor tree over the 64 lanes, no atomics, no LDS — bitwise reproducible and
 * independent of n_seq and of where the sequence lies.  n_seq == 0 launches nothing.  SSI_ERR_ARG: topk < 1, rows >= 2^31, n_seq >= 2^31,
 * a null pointer beside a non-zero size. */
int ssi_seq_score_reduce(const float* row_nll, const int32_t* row_rank, int64_t rows, const int64_t* seq_start, const int64_t* seq_end,
                         int64_t n_seq, int topk, double* out, void* stream);

/* ---- Edit distance between integer sequences (ABI v29; what the reference's scripts/wer.py gets from `evaluate`'s wer, and what picks
 * among samples or beams by minimum Bayes risk; opt-in, nothing else calls it) ----
 * THE DEFINITION.  For a reference r[0..m) and a hypothesis h[0..n) of int32 ids — compared by equality only, so any int32 value is an id —
 * the cell (i, j), 0 <= i <= m, 0 <= j <= n, holds (cost, S, D, I):
 *   row 0 is (j, 0, 0, j); column 0 is (i, 0, i, 0);
 *   for i, j >= 1 there are three candidates, taken in this order, a later one replacing an earlier one only on STRICTLY lower cost:
 *     1. the diagonal, from (i-1, j-1): + 0 if r[i-1] == h[j-1], else + 1 cost and + 1 S;
 *     2. up, from (i-1, j): + 1 cost and + 1 D (a reference id the hypothesis lacks);
 *     3. left, from (i, j-1): + 1 cost and + 1 I.
 * The result is the cell (m, n), written as int32[4] = {dist, S, D, I}.  It follows that dist == S + D + I, that m - S - D == n - S - I >= 0
 * (the hits), and that dist is symmetric in its two arguments (the counts are not).
 *
 * Sequences are spans of ONE flat device buffer tokens[n_tokens]: pair p compares tokens[ref_start[p] .. + ref_len[p]) with
 * tokens[hyp_start[p] .. + hyp_len[p]).  Spans may overlap, repeat and lie in any order; the four span arrays are device arrays of n_pairs
 * entries that the host never reads.  max_len is the caller's bound on every length, at most SSI_EDIT_MAX_LEN (more: SSI_ERR_UNSUPPORTED
 * before any launch).  A span is BAD if its length is negative or above max_len, its start negative, or start + len > n_tokens; the kernel
 * checks this before it forms any address from the span, and a pair with a bad span gets {-1, -1, -1, -1} while every other pair is
 * unaffected (as ssi_attn_decode_beam treats an ancestry index outside its cache).
 * One wave per pair, four per workgroup: the hypothesis columns in strips of SSI_EDIT_COLS per lane, the reference rows as a wavefront
 * through the lanes, hypotheses beyond 64 * SSI_EDIT_COLS columns in column blocks whose boundary column stays in LDS.  Integers only, no
 * atomics: a pair's four numbers depend on its two spans alone — not on n_pairs, not on where the pair lies, not on its neighbours.
 * ssi_edit_distance_workspace_bytes is 0 (nothing needs a workspace) and the entry accepts workspace == NULL; a workspace_bytes below it
 * would be SSI_ERR_WORKSPACE.  n_pairs == 0 launches nothing.  SSI_ERR_ARG: a null pointer beside a non-zero size, a negative size,
 * n_pairs >= 2^31. */
#define SSI_EDIT_MAX_LEN 4096 /* the RoPE table of the benchmark model: no generation is longer */
#define SSI_EDIT_COLS 4       /* hypothesis columns per lane */
size_t ssi_edit_distance_workspace_bytes(int64_t n_pairs, int32_t max_len);
int ssi_edit_distance(const int32_t* tokens, int64_t n_tokens, const int64_t* ref_start, const int32_t* ref_len, const int64_t* hyp_start,
                      const int32_t* hyp_len, int64_t n_pairs, int32_t max_len, int32_t* out /* [n_pairs][4] */, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- Byte-pair encoding over discrete speech units (ABI v30; produces the "compressed speech representations obtained using BPE" of the
 * reference's plans/MASTER PLAN.md; opt-in, nothing else calls it) ----
 * THE DEFINITION (restated in plain Python in tests/unit_bpe_ref.py).
 * Corpus: one flat int32 buffer of symbols in [0, V); sequences are divided by the in-band separator SSI_BPE_SEP (-1).  A PAIR is two
 *   neighbouring symbols of one sequence; a pair never includes a separator.  c(a, b) is the number of positions i with
 *   (x[i], x[i+1]) == (a, b); overlapping positions count: a a a holds two (a, a).
 * Merge m: the pair with the largest count, ties broken by the smallest a, then the smallest b; it gets the id n_base + m.  Training stops
 *   before merge m if the largest count is below min_frequency (>= 1, default 2) or m == n_merges.
 * Applying (a, b) -> z: within each sequence from left to right, where (x[i], x[i+1]) == (a, b) write z and continue at i + 2; for a == b a
 *   run of k equal symbols becomes k / 2 times z, followed by one a if k is odd.  Then the buffer is closed up; separators stay.
 * Encoding a sequence with a merge list applies merges 0, 1, ... in order.  Equivalently: repeatedly apply the lowest-numbered merge that has
 *   an adjacent pair present — the same, because a merge that contains n_base + r is numbered above r: applying merge r creates only pairs
 *   that hold n_base + r, which no merge numbered r or below contains, so the lowest number present never decreases.  Decoding expands ids
 *   >= n_base recursively; decode(encode(u)) == u.
 * Bad ids: an id outside [0, V) other than -1 is checked before any address is formed from it and acts as a separator (as ssi_attn_decode_beam
 *   treats an index outside its cache).  ssi_bpe_pair_count and ssi_bpe_train_begin count each once into *n_bad; ssi_bpe_train_begin writes the
 *   separator in its place into the working buffer; ssi_bpe_encode leaves it where it is.
 *
 * ssi_bpe_pair_count ADDS c(a, b) of ids[0..n) to table[a * stride + b] (uint32; the caller clears it; stride >= V, at most
 * SSI_BPE_MAX_VOCAB) with integer atomics, equal addresses combined within a wave first: integer adds commute, so the table is exact whatever
 * the order.  n_bad may be NULL.
 *
 * The trainer keeps its state on the device: two id buffers of n ids that swap roles per merge (merge m reads buffer m & 1), the table
 * uint32[v_cap * v_cap] with v_cap = n_base + n_merges <= SSI_BPE_MAX_VOCAB (16 384: 1 GiB; more is SSI_ERR_UNSUPPORTED before any launch),
 * the merge list int32[n_merges][3] = {a, b, count}, and int32 state[SSI_BPE_STATE_WORDS] (indices SSI_BPE_ST_*: done, merges made, the last
 * pair and its count, n_bad, and at SSI_BPE_ST_LEN + (m & 1) the length of buffer m & 1).  ssi_bpe_train_begin clears the table, copies the
 * corpus into buf0 with bad ids replaced, counts, and sets the state.  ssi_bpe_merge launches merge m: best pair (reads (n_base + m)^2
 * entries), mark, scan, close up and an INCREMENTAL count update (only pairs beside a merged window change; a pair is owned by its right-hand
 * position).  Its kernels read the pair and `done` from the state, and after done they do nothing: the host launches merge after merge and
 * reads the state back at a cadence of its choice; the result is in buffer state[SSI_BPE_ST_M] & 1.  n_upper is the host's bound on the current
 * length (the last length it read; the grid).  Whether a position of a run of a starts an (a, a) merge depends on the parity of its offset from
 * the run's start, which may lie any number of SSI_BPE_TILE-id tiles to the left: it is carried as a prefix maximum through the same three
 * launches that compute the closed-up offsets.  The kernel boundary is the only synchronisation between workgroups.  n < 2^31.
 *
 * ssi_bpe_encode: sequences are spans of one flat buffer (as ssi_edit_distance), one workgroup per sequence with the sequence and its pair
 * ranks in LDS (three int32 arrays: 4096 ids is 51 KiB of the 64 KiB a workgroup may declare, hence SSI_BPE_ENCODE_MAX_LEN; a larger max_len
 * is SSI_ERR_UNSUPPORTED).  rank_table is int32[V * V], -1 meaning no merge, built by the host from the merge list; V = n_base + n_merges.
 * Sequence s is written to out[seq_start[s] .. + out_len[s]); a bad span (negative, longer than max_len, outside tokens) gives out_len -1 for
 * that sequence alone.  A sequence's result depends on that sequence and the table only. */
#define SSI_BPE_SEP (-1)
#define SSI_BPE_TILE 4096           /* ids per workgroup of the trainer's tile kernels */
#define SSI_BPE_MAX_VOCAB 16384     /* n_base + n_merges */
#define SSI_BPE_ENCODE_MAX_LEN 4096
#define SSI_BPE_STATE_WORDS 8
enum { SSI_BPE_ST_DONE = 0, SSI_BPE_ST_M = 1, SSI_BPE_ST_A = 2, SSI_BPE_ST_B = 3, SSI_BPE_ST_COUNT = 4, SSI_BPE_ST_NBAD = 5, SSI_BPE_ST_LEN = 6 };
int ssi_bpe_pair_count(const int32_t* ids, int64_t n, int32_t V, int32_t stride, uint32_t* table, int32_t* n_bad, void* stream);
size_t ssi_bpe_train_workspace_bytes(int64_t n);
int ssi_bpe_train_begin(const int32_t* ids, int64_t n, int32_t n_base, int32_t v_cap, int32_t* buf0, uint32_t* table, int32_t* state, void* stream);
int ssi_bpe_merge(int32_t* buf0, int32_t* buf1, int64_t n_cap, int64_t n_upper, int32_t n_base, int32_t v_cap, int32_t m, int32_t min_frequency,
                  uint32_t* table, int32_t* merges, int32_t* state, void* workspace, size_t workspace_bytes, void* stream);
int ssi_bpe_encode(const int32_t* tokens, int64_t n_tokens, const int64_t* seq_start, const int32_t* seq_len, int64_t n_seq, int32_t max_len,
                   const int32_t* rank_table, int32_t V, int32_t n_base, int32_t* out, int32_t* out_len, void* stream);

/* ---- K8 + K9 as one entry per direction: tied LM head (TiedLinear over tok_embeddings, ssi/loss.py:8-14) + chunked CE (trainer.py:300) ----
 * fwd: logits_ws[rows, vocab_pad] = hidden[rows, dim] table[vocab_pad, dim]^T (table rows >= vocab are zero padding), then ssi_ce_fwd
 *      on it (write_grad: logits_ws becomes softmax - onehot in place) and ssi_ce_reduce into stats[4].  Equals the reference's
 *      CEWithChunkedOutputLoss(model(tokens), shifted_labels) for any chunk count.
 * bwd: d_hidden = alpha * dlogits table;  d_table (+)= alpha * dlogits^T hidden   (alpha_dev: device scalar = upstream grad / n_valid).
 * The [rows, vocab_pad] logits stay in HBM between the two calls (the caller's workspace, 4.37 GB at T = 16 384): recomputing the logit
 * tiles in backward instead costs another 2 rows vocab_pad dim flop (8.95 TFLOP = 6 ms per step at 1.5 PFLOP/s) to save the 1.8 ms the
 * register-resident CE kernel takes — measured and decided in DESIGN.md §4. */
int ssi_lmhead_ce_fwd(const void* hidden, int64_t ldh, const void* table, int64_t ldt, const int64_t* labels, int64_t rows,
                      int64_t dim, int64_t vocab, int64_t vocab_pad, int64_t ignore_index, void* logits_ws, int64_t ldl,
                      float* row_loss, float* stats, int write_grad, int dtype, void* stream);
int ssi_lmhead_ce_bwd(const void* dlogits, int64_t ldl, const void* hidden, int64_t ldh, const void* table, int64_t ldt,
                      const float* alpha_dev, int64_t rows, int64_t dim, int64_t vocab_pad, void* d_hidden, int64_t lddh,
                      void* d_table, int64_t lddt, int accumulate_d_table, int dtype, void* stream);

/* ---- K14 count_token_types + valid-label count (ssi/train_utils.py:150-165, ssi/trainer.py:388,391) ---------------- */
/* ranges: n_ranges inclusive [lo, hi] pairs (device int64).  out[0..n_ranges) = per-range counts,
 * out[n_ranges] = count(tokens != pad_id), out[n_ranges+1] = count(labels != ignore_index).  One launch, no host sync. */
int ssi_count_tokens(const int64_t* tokens, const int64_t* labels, int64_t n, const int64_t* ranges, int n_ranges,
                     int64_t pad_id, int64_t ignore_index, int64_t* out, void* stream);

/* ---- K11-K13 scale_grads / clip_grad_norm_ / AdamW (ssi/trainer.py:404-409, ssi/optimizer.py:8-17) ----------------- */
int ssi_scale_inplace(void* x, int64_t n, float scale, const float* scale_dev, int dtype, void* stream);
/* out[0] = sum(x^2) in fp32, deterministic two-stage; workspace >= ssi_sumsq_workspace_bytes(n) */
int64_t ssi_sumsq_workspace_bytes(int64_t n);
int ssi_sumsq(const void* x, int64_t n, int dtype, float* out, void* workspace, int64_t workspace_bytes, void* stream);
/* Decoupled-weight-decay Adam on flat buffers, fp32 op-math, one rounding on store (torch fused AdamW semantics; the coefficients 1-lr*wd,
 * 1-b1, b2, 1-b2, lr/bc1, 1/sqrt(bc2) computed in double, then rounded to fp32, as torch does):
 *   g = grad * (grad_scale_dev ? *grad_scale_dev : 1);  p *= 1-lr*wd;  m = m + (1-b1)(g-m);  v = b2 v + (1-b2) g g;
 *   p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),  bc1 = 1-b1^step, bc2 = 1-b2^step.  zero_grad bit 0: grad <- 0; bit 1 (ABI v7): the
 *   launch changes nothing when *grad_scale_dev is inf or NaN (1 / 0 label tokens of an accumulation window: the reference skips that window's
 *   optimizer step, ssi/trainer.py:399-403; an update issued before the host has read the count back skips by itself). */
int ssi_adamw_step(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1,
                   double beta2, double eps, double weight_decay, int64_t step, const float* grad_scale_dev, int zero_grad,
                   int dtype, void* stream);
/* ssi_adamw_step with STOCHASTIC rounding of the three bf16 stores (ABI v11; not in the reference, off by default: HipAdamW's
 * stochastic_rounding).  Same arguments, coefficients, fp32 arithmetic, flag bits and tail handling; dtype must be SSI_BF16, step < 2^32,
 * elem_offset % 8 == 0.  The rounding, on the bit pattern u of the fp32 value x with 16 random bits r:
 *   exponent of u all ones (inf, NaN): the round-to-nearest conversion;  otherwise t = u + r and the result is t >> 16, or u >> 16 where t
 *   would have an all-ones exponent (a finite value is never carried into inf).
 * So a value bf16 holds exactly (+-0 included) never changes, anything else becomes one of its two bf16 neighbours, the one away from zero
 * with probability (u & 0xFFFF) / 65536.  The bits are stateless: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9,
 * 0xBB67AE85) with key (seed & 0xFFFFFFFF, seed >> 32) and counter (j & 0xFFFFFFFF, j >> 32, step, tensor), where e = elem_offset + i is
 * the GLOBAL index of element i (its place in the model's flat buffer, not in the slice of this launch), j = e >> 3, and tensor is 0 for
 * param, 1 for exp_avg, 2 for exp_avg_sq; with output words w0..w3 and k = e & 7, r = (w[k >> 1] >> 16 (k & 1)) & 0xFFFF.  The same (seed,
 * step, e, tensor) gives the same bits in every launch: a buffer updated in slices, on any rank, before or after a resume, comes out the
 * same bit for bit. */
int ssi_adamw_step_sr(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int64_t step, const float* grad_scale_dev, int zero_grad, int dtype,
                      uint64_t seed, int64_t elem_offset, void* stream);
/* The rounding of ssi_adamw_step_sr on its own, an fp32 -> bf16 cast: dst[i] = sr_bf16(src[i], bits of (seed, step, elem_offset + i, tensor)).
 * src and dst 16-byte aligned, 0 <= step < 2^32, tensor >= 0, elem_offset % 8 == 0. */
int ssi_round_bf16_sr(const float* src, void* dst, int64_t n, uint64_t seed, int64_t step, int tensor, int64_t elem_offset, void* stream);
/* AdamW over SEGMENTS of the flat buffers in one launch (ABI v16; not in the reference, opt-in: HipAdamW's param_segments).  Segment s covers
 * the local elements [seg_end[s-1], seg_end[s]) with seg_end[-1] = 0 and has its own lr, weight decay and frozen flag.  seg_end, seg_lr,
 * seg_weight_decay and seg_frozen are HOST arrays of n_segs entries, read during the call only: the table travels in the kernel arguments,
 * the library allocates nothing on the device and enqueues no copy.  The ends are strictly ascending, every end but the last is a multiple of
 * 8 (a 16-byte vector lies in one segment), the last equals n: anything else is SSI_ERR_ARG.  n_segs > SSI_ADAMW_MAX_SEGS is
 * SSI_ERR_UNSUPPORTED (the caller splits the launch at a segment end), as is n >= 2^35 - 8.
 *   A non-frozen element comes out bit for bit as the plain entry would leave it (the _sr one when stochastic != 0) when launched on that
 * segment's slice alone with seg_lr[s], seg_weight_decay[s] and elem_offset + seg_end[s-1]: (float)(1 - lr wd) and (float)(lr / bc1) are
 * computed per segment in double, and the random bits are a function of the global element index.  A FROZEN element is neither read nor
 * written in any of the four buffers (its gradient may hold NaN; zero_grad bit 0 leaves it alone); frozen segments at either end of the slice
 * are not launched over, an all-frozen table launches nothing.  zero_grad bit 1 makes the whole launch a no-op on a non-finite scale.
 * stochastic != 0 needs SSI_BF16, step < 2^32 and elem_offset % 8 == 0; otherwise seed and elem_offset are not used. */
#define SSI_ADAMW_MAX_SEGS 128
int ssi_adamw_step_seg(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const int64_t* seg_end, const double* seg_lr,
                       const double* seg_weight_decay, const int32_t* seg_frozen, int n_segs, double beta1, double beta2, double eps,
                       int64_t step, const float* grad_scale_dev, int zero_grad, int dtype, int stochastic, uint64_t seed,
                       int64_t elem_offset, void* stream);
/* ssi_adamw_step_seg with one more gradient factor per segment, read on the DEVICE (ABI v23; not in the reference, opt-in: HipAdamW's
 * grad_groups with a clip rule).  seg_scale_dev is a device array of n_segs floats, never NULL (NULL is SSI_ERR_ARG).  For a non-frozen
 * segment s the effective factor is
 *     gs_s = grad_scale_dev ? fl(*grad_scale_dev * seg_scale_dev[s]) : seg_scale_dev[s]
 * one correctly rounded fp32 product, computed once per segment, and every element of the segment comes out BIT FOR BIT as ssi_adamw_step
 * (ssi_adamw_step_sr when stochastic != 0) would leave it when launched on that segment's slice alone with grad_scale_dev = &gs_s, seg_lr[s],
 * seg_weight_decay[s] and elem_offset + seg_end[s-1].  A segment whose gs_s is not finite -- the test of zero_grad bit 1, !(fabsf(gs_s) <
 * INFINITY) -- is treated as frozen for this launch: neither read nor written in any of the four buffers (a group whose norm overflowed skips
 * its step and nobody else's).  zero_grad bit 1 still makes the whole launch a no-op on a non-finite *grad_scale_dev.  Everything else is
 * ssi_adamw_step_seg's: the host arrays, the frozen flag, frozen segments at either end not launched over, SSI_ADAMW_MAX_SEGS, the tail. */
int ssi_adamw_step_seg_gscale(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const int64_t* seg_end, const double* seg_lr,
                              const double* seg_weight_decay, const int32_t* seg_frozen, int n_segs, double beta1, double beta2, double eps,
                              int64_t step, const float* grad_scale_dev, int zero_grad, int dtype, int stochastic, uint64_t seed,
                              int64_t elem_offset, const float* seg_scale_dev, void* stream);
/* Sums of squares of GROUPS of segments of a flat buffer in one pass (ABI v23; not in the reference, opt-in: HipAdamW's grad_groups).
 * Segment s covers the elements [seg_end[s-1], seg_end[s]) with seg_end[-1] = 0 and belongs to group seg_group[s] in [0, n_groups), or to
 * none (-1).  seg_end and seg_group are HOST arrays of n_segs entries, read during the call only, with ssi_adamw_step_seg's conventions:
 * ends strictly ascending, every end but the last a multiple of 8, the last equal to n; the table travels in the kernel arguments, the
 * library allocates nothing on the device and enqueues no copy.
 *   out[g] (device, n_groups floats) = sum over the elements of all segments of group g of (float)x * (float)x, accumulated in fp32; a
 * group without a segment gets 0.  out is written, not accumulated into.  A segment with group -1 is NOT READ at all (a frozen range of the
 * gradient buffer is unspecified and may hold NaN).  n == 0 (one segment with end 0) and an all-skipped table succeed with out zeroed.
 *   n_segs > SSI_SUMSQ_MAX_SEGS or n_groups > SSI_SUMSQ_MAX_GROUPS is SSI_ERR_UNSUPPORTED (as is n >= 2^35 - 8); a group id outside
 * [-1, n_groups) or bad ends SSI_ERR_ARG; workspace_bytes < ssi_sumsq_groups_workspace_bytes(n, n_segs, n_groups) SSI_ERR_WORKSPACE.
 *   Properties (tests/test_sumsq_groups_gpu.py):
 *   1. Reproducible: the same inputs give the same bits in every launch.  No float atomics: each block owns a contiguous run of 256-vector
 *      tiles, keeps per-thread sums, reduces them by a fixed tree per group, writes one slot per group to the workspace, and a second
 *      kernel adds the slots in ascending block order.
 *   2. Isolated: out[g] depends only on the elements of group g's segments and on the table.  No other element -- NaN and inf included, and
 *      whatever a skipped segment holds -- changes a bit of it.
 *   3. Bounded: against the sum in float64 of the same stored values, |out[g] - ref[g]| <= B ref[g] with B = D u / (1 - D u), u = 2^-24,
 *      D = 1 + (T E + 1) + n_segs + 12 + 1 + 12: the square, the longest per-thread chain (T = ceil(ceil((n / E) / 256) / 2048) tiles per
 *      block, E = 8 (bf16) or 4 (fp32) elements per 16-byte vector, + 1 for the ragged tail), the adds of a block's reduced sums into its
 *      group slot (at most one per segment), the block tree (6 + 6 levels), the pairing of two slots and the final tree. */
#define SSI_SUMSQ_MAX_SEGS 256
#define SSI_SUMSQ_MAX_GROUPS 64
int64_t ssi_sumsq_groups_workspace_bytes(int64_t n, int n_segs, int n_groups);
int ssi_sumsq_groups(const void* x, int64_t n, int dtype, const int64_t* seg_end, const int32_t* seg_group, int n_segs, int n_groups,
                     float* out /* device, [n_groups] */, void* workspace, int64_t workspace_bytes, void* stream);
/* Exponential moving average of the parameters, kept in fp32 (ABI v17; not in the reference, opt-in: HipAdamW's ema_decay).  Per element, in
 * fp32, with p = (float)param[i] (exact for bf16):
 *     ema[i] = __builtin_fmaf(decay, ema[i] - p, p)
 * the subtraction correctly rounded, then ONE fused multiply-add.  decay == 0 gives ema = p exactly, and ema == p is an exact fixed point: the
 * average of a frozen or converged weight never drifts by rounding.  ema is fp32 whatever `dtype`, which is that of param (SSI_BF16 or
 * SSI_F32).  0 <= decay < 1, anything else (NaN included) is SSI_ERR_ARG.  guard_dev may be NULL; otherwise the launch changes nothing when
 * *guard_dev is inf or NaN — the test of zero_grad bit 1 in ssi_adamw_step, !(fabsf(g) < INFINITY): pass AdamW's grad_scale_dev, and an
 * accumulation window without a label moves neither the parameters nor their average.  ema and param 16-byte aligned; n is arbitrary (the
 * tail after the last vector of 8 is handled in the kernel); n == 0 is success without a launch.  One pure HBM pass: per element 2 B (bf16)
 * or 4 B read of param, 4 B read and 4 B written of ema. */
int ssi_ema_update(void* ema /* fp32 */, const void* param, int64_t n, float decay, const float* guard_dev,
                   int dtype /* of param: SSI_BF16 | SSI_F32 */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSI_HIP_H */
