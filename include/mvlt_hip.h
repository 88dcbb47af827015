/* mvlt_hip.h -- C-ABI of the MI355X (gfx950) kernels for the MVLT hot path.
 *
 * The reference (Control-xl/Medical-Vision-Langauge-Transformer) has no
 * FFI/plugin seam: its hot path is eager PyTorch.  This
 * header is therefore the boundary a maintainer would bind (ctypes stub in
 * INTEGRATION.md): one entry point per fused op, each citing the reference
 * lines whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    marked host; the caller owns every buffer (inputs, outputs, saved
 *    tensors, workspace) -- the library allocates nothing.
 *  - `stream` is a hipStream_t passed as void*; every launch goes on it.
 *  - return 0 on success, a negative MVLT_ERR_* otherwise; no exceptions.
 *  - re-entrant, no global mutable state; one process per GPU.
 *  - `dtype` selects storage/MFMA input type of activations and of the
 *    compute copies of weight matrices: MVLT_F32 (exact f32 MFMA,
 *    v_mfma_f32_16x16x4_f32) or MVLT_BF16 (v_mfma_f32_16x16x32_bf16, f32
 *    accumulate).  Biases, LayerNorm affine parameters, the relative position
 *    bias table, statistics and gradients of parameters are always f32.
 */
#ifndef MVLT_HIP_H
#define MVLT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MVLT_F32 = 0, MVLT_BF16 = 1 };
enum { MVLT_OK = 0, MVLT_ERR_ARG = -1, MVLT_ERR_LAUNCH = -2, MVLT_ERR_UNSUPPORTED = -3 };

/* loader checks.  MVLT_ABI_VERSION is bumped on EVERY change of a struct layout or of an entry point's
 * signature; a binding compiles / hard-codes the value it was written against and compares it with what the
 * loaded library returns.  mvlt_sizeof(MVLT_STRUCT_*) lets a binding that mirrors the structs by hand (ctypes,
 * cgo, JNI) prove that its mirror has the size the library was compiled with (0 for an unknown id). */
#define MVLT_ABI_VERSION 17
int mvlt_version(void);            /* MVLT_ABI_VERSION of the loaded library */
const char* mvlt_arch(void);       /* "gfx950" */
enum { MVLT_STRUCT_GEMM = 0, MVLT_STRUCT_LAYERNORM = 1, MVLT_STRUCT_LAYERNORM_BWD = 2, MVLT_STRUCT_LN_REDUCE_ITEM = 3,
       MVLT_STRUCT_ATTN = 4, MVLT_STRUCT_SWIN_WMSA = 5, MVLT_STRUCT_EMBED = 6, MVLT_STRUCT_ATTN_CACHED = 7,
       MVLT_STRUCT_ZERO_ITEM = 8, MVLT_STRUCT_RANGE = 9, MVLT_STRUCT_MLM_MASK = 10, MVLT_STRUCT_GREEDY_STATE = 11, MVLT_STRUCT_SWIN_DBIAS_ITEM = 12,
       MVLT_STRUCT_SAMPLE_STATE = 13, MVLT_STRUCT_SAMPLE_FILTER = 14, MVLT_STRUCT_BEAM_CAND = 15, MVLT_STRUCT_ATTN_CACHED_BEAM = 16,
       MVLT_STRUCT_HEAD_CE = 17, MVLT_STRUCT_RETRIEVAL_HEAD = 18, MVLT_STRUCT_BEAM_STEP = 19,
       MVLT_STRUCT_LOGIT_RULES = 20, MVLT_STRUCT_COUNT = 21 };
size_t mvlt_sizeof(int struct_id);

/* ------------------------------------------------------------------ GEMM
 * C[M,N] = epilogue(A[M,K] * B[K,N]).  Replaces every nn.Linear on the path:
 * qkv/proj (visual_feature_extractor.py:231,252), Mlp fc1/fc2 (:135-141),
 * PatchMerging.reduction (:443), PatchEmbed.proj as im2col GEMM (:562), HF
 * BERT query/key/value/dense (modeling_bert.py:175-177,289,337,348), pooler,
 * MLM transform/decoder (:466-506) and all their dgrad/wgrad products.
 *   a_kmajor = 0: A[m*lda + k]          1: A[k*lda + m]   (wgrad: A = dY^T)
 *   b_kmajor = 0: B[n*ldb + k] (torch Linear weight [N,K])   1: B[k*ldb + n]
 * Epilogue, in this order (v = accumulator, m' = rowmap ? rowmap[m] : m):
 *   BIAS      v += bias[n]
 *   GELU      (SAVE_PRE: pre[m',n] = v)  v = gelu_erf(v)
 *   DROPOUT   v = keep(seed,tag,m*N+n) ? v/(1-p) : 0
 *   ROWSCALE  v *= rowscale[m' / rows_per_scale]            (DropPath)
 *   MUL_GELU_GRAD  v *= gelu'(aux[m',n])
 *   RESIDUAL  v += residual[m'*ldr + n]
 *   ACCUM     v += C[m',n]
 *   store C[m'*ldc + n]  (dtype, or f32 when OUT_F32)
 * TAIL (with m_dev, a_kmajor = 0): rows m >= *m_dev do NOT leave; they run the epilogue above on a ZERO accumulator and are
 *   stored like every other row (their rows of A are never read and may hold anything).  With ROWSCALE 0 and RESIDUAL that is
 *   (0 + bias) * 0 + residual = the residual row, bit for bit; with no bias and no residual, zeros.  A tile entirely beyond
 *   the count skips its K loop.  Honoured by the tile kernels (gemm_glds_kernel, gemm_kernel); k-slices refuse it
 *   (MVLT_ERR_UNSUPPORTED: pass split_k = 1), the skinny, row-streaming and 8-wave routes hand the product to the tile kernels.
 * split_k > 1 computes K-slices into `workspace` (f32 slabs) and a second
 * kernel reduces them and applies the epilogue (deterministic, no atomics). */
enum {
    MVLT_EPI_BIAS = 1, MVLT_EPI_GELU = 2, MVLT_EPI_SAVE_PRE = 4, MVLT_EPI_DROPOUT = 8,
    MVLT_EPI_ROWSCALE = 16, MVLT_EPI_RESIDUAL = 32, MVLT_EPI_ROWMAP = 64,
    MVLT_EPI_MUL_GELU_GRAD = 128, MVLT_EPI_OUT_F32 = 256, MVLT_EPI_ACCUM = 512, MVLT_EPI_TAIL = 1024
};
typedef struct MvltGemm {
    int dtype, M, N, K;
    const void* A; int64_t lda; int a_kmajor;
    const void* B; int64_t ldb; int b_kmajor;
    void* C; int64_t ldc;
    int epilogue;
    const float* bias;
    void* pre;                       /* ldc */
    const void* residual; int64_t ldr;
    const void* aux;                 /* ldc */
    const float* rowscale; int rows_per_scale;
    const int32_t* rowmap;
    float dropout_p; uint64_t seed; uint32_t tag;
    int split_k; void* workspace; size_t workspace_bytes;
    float* a_colsum;                 /* optional (a_kmajor only): a_colsum[m] = sum_k A[k*lda+m], i.e. the bias
                                        gradient colsum(dY) fused into the wgrad GEMM dW = dY^T X */
    void* event_after_main;          /* optional hipEvent_t recorded on `stream` right after the main GEMM kernel
                                        (before the split-K reduce): lets a benchmark time that kernel alone */
    const int32_t* m_dev;            /* optional, DEVICE int: the number of valid storage rows of A, read by the kernel
                                        (ragged batches planned on the GPU, mvlt_pack_plan: no host sync).  a_kmajor=0:
                                        rows of A / C beyond it are neither read nor written (M is the upper bound the
                                        launch is sized for); a_kmajor=1 (weight gradients): the reduction stops there
                                        (K is the upper bound) */
    const void* prefetch; int64_t prefetch_bytes;
                                     /* optional: a read-only byte range (the weight matrix of the NEXT nn.Linear of the
                                        layer) that this launch pulls towards the caches while it runs -- every thread
                                        reads and drops one dword of a few of its 128-byte lines.  The optimizer's sweep
                                        evicts all weights from the Infinity Cache once per step; a product whose weight
                                        panel is already on its way runs 10-20 % faster (profiles/r2_weight_prefetch.txt) */
} MvltGemm;
int mvlt_gemm(const MvltGemm* p, void* stream);
size_t mvlt_gemm_workspace_bytes(const MvltGemm* p);
/* introspection: tile (= kernel instantiation gemm_kernel<dtype,bm,bn,a_kmajor,b_kmajor>) and split-K chosen for p */
int mvlt_gemm_plan(const MvltGemm* p, int* bm, int* bn, int* split_k);
/* The kernel family mvlt_gemm / mvlt_gemm_group would launch for these arguments (and the environment switches the dispatch
 * reads per call), without launching anything: the dispatch itself runs in a no-launch mode, so the answer cannot drift from
 * what a call does.  Returns MVLT_GEMM_ROUTE_KIND (an MvltGemmRoute) in the low bits and the number of k-slices
 * (MVLT_GEMM_ROUTE_SLICES, >= 1) above them, or the negative MVLT_ERR_* the call itself would answer.  For tests that must
 * know which kernel they check (the plan says tile and split, not LDS-DMA / register-staged / row streaming / 8-wave). */
enum MvltGemmRoute {
    MVLT_GEMM_ROUTE_SKINNY = 1,               /* skinny.hip, M <= 64 */
    MVLT_GEMM_ROUTE_ROWSTREAM_0 = 2,          /* rowstream.hip, + the shape's bit of MVLT_ROWSTREAM (0 .. 8) */
    MVLT_GEMM_ROUTE_ROWSTREAM_8 = 10,
    MVLT_GEMM_ROUTE_G8_22_NARROW = 11,        /* gemm8.hip forward / dgrad: 256 x 256 or 128 x 256 tiles, 8- or 16-byte epilogue */
    MVLT_GEMM_ROUTE_G8_22_WIDE = 12,
    MVLT_GEMM_ROUTE_G8_12_NARROW = 13,
    MVLT_GEMM_ROUTE_G8_12_WIDE = 14,
    MVLT_GEMM_ROUTE_GLDS = 15,                /* gemm_glds_kernel at the planned tile (split-K: + splitk_reduce_kernel) */
    MVLT_GEMM_ROUTE_REG = 16,                 /* gemm_kernel (register-staged) at the planned tile */
    MVLT_GEMM_ROUTE_GROUP_GLDS_128x128 = 17,  /* gemm_group_glds_kernel<128, 128, 2> */
    MVLT_GEMM_ROUTE_GROUP_GLDS_64x128_S3 = 18,
    MVLT_GEMM_ROUTE_GROUP_GLDS_64x128_S2 = 19,
    MVLT_GEMM_ROUTE_GROUP_REG_128x128 = 20,   /* gemm_group_kernel, no k-slices (bf16 or f32) */
    MVLT_GEMM_ROUTE_GROUP_REG_64x128 = 21,
    MVLT_GEMM_ROUTE_GROUP_REG_64x96 = 22,
    MVLT_GEMM_ROUTE_GROUP_ATOMIC = 23,        /* gemm_group_kernel, k-slices that meet through atomicAdd in the zeroed output */
    MVLT_GEMM_ROUTE_GROUP_G8_22 = 24,         /* gemm8.hip group form: 256 x 256 / 128 x 256 / 128 x 128 tiles, slices through slabs */
    MVLT_GEMM_ROUTE_GROUP_G8_12 = 25,
    MVLT_GEMM_ROUTE_GROUP_G8_11 = 26
};
#define MVLT_GEMM_ROUTE_KIND_BITS 8
#define MVLT_GEMM_ROUTE_KIND(r) ((r) & ((1 << MVLT_GEMM_ROUTE_KIND_BITS) - 1))
#define MVLT_GEMM_ROUTE_SLICES(r) ((r) >> MVLT_GEMM_ROUTE_KIND_BITS)
int mvlt_gemm_route(const MvltGemm* p);
int mvlt_gemm_group_route(const MvltGemm* items, int n);
/* n (<= 8) independent products in ONE launch -- the weight gradients of one layer (dW_i = dY_i^T X_i, the
 * backward of the nn.Linear calls of one SwinTransformerBlock / BertLayer).  All items must have both operands
 * k-major, the same dtype and output widths that are all multiples of 128 or all multiples of 96; the tile
 * lists are concatenated (gemm_group_kernel<dtype,64,bn>), no split-K, no workspace.
 * MVLT_ERR_UNSUPPORTED if the items do not qualify (launch them one by one then). */
int mvlt_gemm_group(const MvltGemm* items, int n, void* stream);
/* Optional workspace of a grouped launch: put it into items[0].workspace / workspace_bytes.  With it, groups with fewer
 * output tiles than CUs (every weight-gradient group of the B = 32 step) are cut into k-slices that meet through f32
 * slabs inside the one launch (the last arriver of a tile sums the slices in slice order: deterministic, no atomics). */
size_t mvlt_gemm_group_workspace_bytes(const MvltGemm* items, int n);
/* Last-row MLM head fused with the greedy pick (model.py:896-900): out_idx[m] = argmax_n (A W^T + bias)[m, n]
 * (first index on ties), out_val[m] = that maximum (f32, may be NULL); the logits are never stored.  M <= 64,
 * both operands k-contiguous (MVLT_ERR_UNSUPPORTED otherwise); only MVLT_EPI_BIAS is honoured; C is unused.
 * part_val / part_idx: scratch, M * ceil(N / 16) elements each. */
int mvlt_gemm_argmax(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_val,
                     void* stream);
/* The same product with the per-token bookkeeping of greedy_search (model.py:896-913) in the finishing launch, all on the
 * device: next = argmax; samples that have finished emit pad_id; unfinished[m] &= (next != eos_id); ids[m, *col] = next;
 * scores[m, *col] = the maximum logit; new_ids[m, 0] = next (the first of the two ids the next cached step feeds);
 * alive[*col] is raised to 1 by every sample that is still unfinished (the caller zeroes `alive` when a decode starts);
 * *past += 1 (optional); *col += 1.  One launch (a workgroup per row; the last one to arrive -- `ticket`, an int32 the caller
 * zeroes once -- advances col / past) instead of the argmax finish + ten one-line kernels per replayed decode step.
 * has_eos = 0: no EOS handling (unfinished / alive unused). */
typedef struct MvltGreedyState {
    int64_t* unfinished; int64_t eos_id, pad_id; int has_eos;
    int64_t* col; int32_t* past;
    int64_t* ids; int64_t ld_ids; float* scores; int64_t ld_scores; int64_t* alive; int64_t* new_ids; int64_t ld_new;
    int32_t* ticket;
} MvltGreedyState;
int mvlt_gemm_argmax_greedy(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltGreedyState* g, void* stream);
/* Last-row MLM head fused with the SAMPLED pick (model.py:901-906, sample_mode = 'sample'): multinomial(softmax(x)) drawn as
 * argmax_n (x_n + G_n) with i.i.d. standard Gumbel noise (Gumbel-max); the logits are never stored.  Per element, in f32:
 *   x = (A W^T + bias)[m, n] * inv_temperature
 *   u = rng_u32(seed, tag, m * N + n)              (the counter hash of the dropout masks; N = p->N, not a padded width)
 *   u01 = ((u >> 8) + 0.5) * 2^-24,  G = -log(-log(u01))     (finite; |G_f32 - G| <= 2^-22 (3 + |G|): mvlt_gumbel_noise)
 *   out_idx[m] = first argmax_n (x + G),  out_logprob[m] = x[out_idx[m]] - logsumexp_n x
 * Same preconditions and error codes as mvlt_gemm_argmax_greedy (M <= 64, K a whole number of k-blocks, k-contiguous 16-byte
 * aligned operands, only MVLT_EPI_BIAS; C unused), M * N < 2^32, 0 < inv_temperature < inf.
 * part_val: scratch, 4 * M * ceil(N / 16) floats; part_idx: M * ceil(N / 16). */
int mvlt_gemm_sample(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_logprob,
                     uint64_t seed, uint32_t tag, float inv_temperature, void* stream);
/* The graph form: the bookkeeping of mvlt_gemm_argmax_greedy with the sampled pick; scores[m, *col] = the log-probability of
 * the DRAWN token (also for a finished sample, whose id becomes pad_id: the reference gathers the score first).  The noise of
 * the token in output column c uses seed = *seed and tag = tag0 + c, both read on the device: one captured graph serves every
 * call and every token.  A decode of max_length tokens uses the tags tag0 .. tag0 + max_length - 1. */
typedef struct MvltSampleState {
    int64_t* unfinished; int64_t eos_id, pad_id; int has_eos;
    int64_t* col; int32_t* past;
    int64_t* ids; int64_t ld_ids; float* scores; int64_t ld_scores; int64_t* alive; int64_t* new_ids; int64_t ld_new;
    int32_t* ticket;
    const uint64_t* seed; uint32_t tag0; float inv_temperature;
} MvltSampleState;
int mvlt_gemm_sample_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleState* g, void* stream);
/* The sampled pick behind a top-k / top-p filter (HF TopKLogitsWarper, then TopPLogitsWarper; sample_mode = 'sample' with
 * top_k / top_p).  A filter is a set function of a whole row, so the product writes x (as above, bit for bit) into the caller's
 * workspace `x` ([M, ldx] f32, ldx >= N) and a second launch, one workgroup per row, selects and draws.  Per row m:
 *   top-k  (1 <= top_k < N; 0 or >= N: off)  tau_k = the k-th largest x counted with multiplicity, K1 = {n : x_n >= tau_k}:
 *          ties at the threshold are ALL kept (HF's `scores < kth` rule), |K1| >= k
 *   top-p  (0 < top_p < 1; >= 1: off), applied after top-k: w_n = exp(x_n - max x), S = sum_K1 w, A(v) = sum_{j in K1, x_j > v} w_j,
 *          K = {n in K1 : A(x_n) < top_p S} -- a token is kept while the mass strictly above it has not reached top_p.  HF's
 *          nucleus rule without a dependence on the sort order: tie-inclusive, the row maximum is always kept
 *          (min_tokens_to_keep = 1).  K = {x_n >= tau} for one threshold per row.
 *   G_n = the Gumbel noise of mvlt_gemm_sample at index (row0 + m) * N + n (row0: the call's first row within a larger batch,
 *         so a batch issued in row chunks draws what one call would), y_n = x_n + G_n (f32)
 *   out_idx[m] = first argmax_{n in K} y_n,  out_logprob[m] = x[out_idx[m]] - log sum_{n in K} exp(x_n)   (renormalised)
 * With both filters off the token is mvlt_gemm_sample's, bit for bit.  Deterministic: integer histograms, masses as 64-bit fixed
 * point (rint(2^32 w), relative error of a mass sum <= E_MASS(N) = (3 ln N + 4) 2^-24 + N 2^-33 + 2^-51, csrc/skinny.hip),
 * no float atomics -- the same operands give the same set, token and score.
 * Refusals: those of mvlt_gemm_sample (part_val / part_idx are checked like there; this version keeps the row in `x` and leaves
 * them unwritten), and MVLT_ERR_ARG for filter or filter->x NULL, ldx < N, top_k < 0, top_p <= 0 or NaN,
 * (row0 + M) * N >= 2^32.  A refused call launches nothing and writes nothing. */
typedef struct MvltSampleFilter { int32_t top_k; float top_p; float* x; int64_t ldx; uint32_t row0; } MvltSampleFilter;
int mvlt_gemm_sample_filtered(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                              int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, float inv_temperature,
                              void* stream);
/* The graph form: mvlt_gemm_sample_step (same state, same seed / tag0 + column convention) with the filtered pick. */
int mvlt_gemm_sample_filtered_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                   const MvltSampleState* g, void* stream);
/* Logit rules of constrained decoding (HF RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, MinLengthLogitsProcessor),
 * applied to the raw logits inside the head kernels, before temperature and top-k / top-p.  Per row m: c = *col tokens generated so
 * far, h = ids[m, 0 .. c-1] exactly as stored (PAD of a finished row included), x = acc + bias in f32.
 *   seen(n)    n occurs in h.  x' = x < 0 ? x * penalty : x / penalty, applied once however often n occurs (penalty > 0; 1.0: off)
 *   banned(n)  n-grams (g = ngram >= 1 and c + 1 >= g): some i <= c - g has h[i .. i+g-2] == h[c-g+1 .. c-1] and h[i+g-1] == n
 *              (g = 1 bans every seen token); min length (has_eos and c < min_length): n == eos_id
 * A banned column takes part in nothing -- not in the maximum, the log-sum-exp, the Gumbel draw or the top-k / top-p sets -- and
 * is never returned; the filtered route stores -inf for it.  The recorded scores follow the processed logits.  At most c + 1
 * columns of a row are banned: the caller keeps N > the longest history so that a row always has a column left.
 * Two launches share the struct.  The PLAN (one workgroup per row, M <= 64) rebuilds `seen` and `banned` from ids / col: bitmaps of
 * ld_words >= ceil(V / 32) uint32 words per row, bit n & 31 of word n >> 5 = column n.  The rebuild is stateless (clear, then set):
 * nothing carries over between tokens or calls, so a replayed graph has nothing to reset.  ids outside [0, V) set no bit.
 * The _rules HEADS are the six head entry points above with the bitmaps and `penalty` applied in their epilogues; they read
 * seen / banned / ld_words / penalty only (the caller runs the plan first, on the same stream).
 * Refusals (MVLT_ERR_ARG, nothing launched, nothing written), ahead of the base entry point's own: rules, seen or banned NULL,
 * ld_words < ceil(N / 32), penalty <= 0 or NaN, ngram < 0, M > 64 (M < 1); the plan also refuses ids or col NULL, ld_ids < 1,
 * V < 1, min_length < 0. */
typedef struct MvltLogitRules {
    uint32_t* seen; uint32_t* banned; int64_t ld_words;       /* [M, ld_words] each */
    float penalty;
    const int64_t* ids; int64_t ld_ids; const int64_t* col;   /* the plan's history: ids[m, 0 .. *col - 1] */
    int32_t ngram, min_length; int64_t eos_id; int32_t has_eos;
} MvltLogitRules;
int mvlt_decode_rules_plan(const MvltLogitRules* rules, int M, int V, void* stream);
int mvlt_gemm_argmax_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_val,
                           const MvltLogitRules* rules, void* stream);
int mvlt_gemm_argmax_greedy_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltGreedyState* g,
                                  const MvltLogitRules* rules, void* stream);
int mvlt_gemm_sample_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_logprob,
                           uint64_t seed, uint32_t tag, float inv_temperature, const MvltLogitRules* rules, void* stream);
int mvlt_gemm_sample_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleState* g,
                                const MvltLogitRules* rules, void* stream);
int mvlt_gemm_sample_filtered_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                    int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, float inv_temperature,
                                    const MvltLogitRules* rules, void* stream);
int mvlt_gemm_sample_filtered_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                         const MvltSampleState* g, const MvltLogitRules* rules, void* stream);
/* Last-row MLM head with a PER-ROW pick over any number of rows R = p->M (K sampled reports per image next to a greedy row in one
 * decode pass).  Two device tables of R entries say what row r does:
 *   noise_row[r] (int32)  >= 0: sampled, y = x + G with G the noise of mvlt_gemm_sample at index (uint32)noise_row[r] * N + n
 *                         < 0 : greedy, y = x
 *   inv_t[r] (f32)        the row's inverse temperature; the caller guarantees 0 < inv_t[r] < inf (device data: not checked)
 * Per element, in f32 with no fused multiply-add: x = (A W^T + bias)[r, n] * inv_t[r] -- the two rounded operations of
 * mvlt_gemm_sample; the _rules forms apply the penalty to the raw logit ahead of inv_t and drop banned columns, as there.
 * Every row, sampled or greedy, has the same outputs:
 *   out_idx[r] = first argmax_n y,  out_logprob[r] = x[out_idx[r]] - logsumexp_n x
 * so the score of a GREEDY row is the log-probability of its token at inv_t[r], NOT the raw maximum logit that mvlt_gemm_argmax /
 * mvlt_gemm_argmax_greedy record.  The noise index wraps in uint32: a bad noise_row selects other noise and never an address;
 * nothing is read at a table index >= R.  Rows go in groups of 64 inside the call, each group streaming the weights once; the
 * finish is one workgroup per row.  A row's result depends on its own A row, noise_row and inv_t only -- not on R, not on the
 * other rows.  Bit for bit by construction: noise_row[r] = r and a uniform inv_t (R <= 64) give the tokens and scores of
 * mvlt_gemm_sample; noise_row < 0 and inv_t = 1 the tokens of mvlt_gemm_argmax's wide form; the _rules form on rows r0 .. r0 + 63 with
 * noise_row[r] = r - r0 what mvlt_gemm_sample_rules gives for that chunk (its bitmaps at row r0).
 * part_val: scratch, 4 * R * ceil(N / 16) floats; part_idx: R * ceil(N / 16).  The _rules forms read bitmaps of R rows
 * (mvlt_decode_rules_plan fills them 64 rows at a time).
 * Refusals (nothing is launched, nothing written).  MVLT_ERR_ARG: p, A, B, part_val, part_idx, noise_row, inv_t or (stand-alone)
 * out_idx / out_logprob NULL, bias NULL with MVLT_EPI_BIAS, R < 1, N / K / lda / ldb < 1, R * N >= 2^32; the _rules forms: the
 * refusals of the other _rules heads without their M <= 64.  MVLT_ERR_UNSUPPORTED: K not a whole number of k-blocks, operands
 * not k-contiguous or not 16-byte aligned (every 64-row group is checked), an epilogue bit other than MVLT_EPI_BIAS. */
int mvlt_gemm_pick_rows(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                        int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, void* stream);
int mvlt_gemm_pick_rows_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                              int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, const MvltLogitRules* rules,
                              void* stream);
/* The graph form: the bookkeeping of mvlt_gemm_sample_step over the R rows of `g` (ids, scores, new_ids, unfinished of R rows;
 * one ticket per row; col and past advance once per call), seed = *g->seed and tag = g->tag0 + *col read on the device.
 * g->inv_temperature is not read: the table is the temperature.  Also MVLT_ERR_ARG: g, g->seed or a state pointer
 * mvlt_gemm_sample_step requires NULL. */
int mvlt_gemm_pick_rows_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                             const MvltSampleState* g, void* stream);
int mvlt_gemm_pick_rows_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                                   const MvltSampleState* g, const MvltLogitRules* rules, void* stream);
/* Last-row MLM head fused with the candidate step of beam search (model.py:700-720: log_softmax + beam score, top 2 * beams over
 * (beam, token)).  The M = G * num_beams rows of the product are the hypotheses of G samples, rows g * num_beams .. + num_beams
 * the beams of sample g.  Per row m, all in f32 with no fused multiply-add:
 *   x = (A W^T + bias)[m, n]                       bit for bit the x of mvlt_gemm_sample_filtered at inv_temperature = 1
 *   lse_m = max_n x + logf(sum_n expf(x - max))    a fixed summation shape (csrc/skinny.hip beam_candidates_kernel)
 *   s[m, n] = (x - lse_m) + beam_scores[m]         the two roundings log_softmax followed by `+` make
 * Per sample g: the n_cand largest s over its num_beams * N entries, sorted descending, ties broken by the LOWER flat index
 * beam * N + n (torch.topk leaves ties unspecified) -> cand_score (f32), cand_beam, cand_tok (int32), all [G, n_cand]; lse
 * (f32 [M], optional).  The product writes x into the caller's workspace `x` ([M, ldx] f32, ldx >= N) in row chunks of at most 64
 * (M may exceed 64); the selection is one launch, a workgroup per sample.  The selection compares integers only and uses no
 * float atomics: the same operands give the same lists run to run.
 * Preconditions of the product: those of mvlt_gemm_sample_filtered (K a whole number of k-blocks, k-contiguous 16-byte aligned
 * operands, only MVLT_EPI_BIAS; C, m_dev unused) without its M <= 64.
 * Refusals (nothing is launched, nothing written): MVLT_ERR_ARG for a NULL p / c / operand / beam_scores / x / output,
 * num_beams < 1, n_cand < 1, M % num_beams != 0, ldx < N, n_cand > num_beams * N, num_beams * N >= 2^31; then
 * MVLT_ERR_UNSUPPORTED for num_beams > 8, n_cand > 16 or a product the wide head kernels refuse. */
typedef struct MvltBeamCand {
    int32_t num_beams, n_cand;
    const float* beam_scores;           /* [M] */
    float* x; int64_t ldx;              /* logits workspace [M, ldx] */
    float* cand_score; int32_t* cand_beam; int32_t* cand_tok;       /* [M / num_beams, n_cand] */
    float* lse;                         /* [M] or NULL */
} MvltBeamCand;
int mvlt_gemm_beam_candidates(const MvltGemm* p, const MvltBeamCand* c, void* stream);
/* The logit rules in beam search (HF 4.16 beam_search: the processors act on the LOG-PROBABILITIES, before the beam score is
 * added -- not on the raw logits, where the six picks above apply them).  Row m = g * num_beams + b is one live hypothesis; c = *col
 * tokens generated so far, the same for every row; h = the hypothesis' own c tokens after the beam reorder of the previous token
 * (no [MASK] placeholder; empty at step 0).  All in f32 with no fused multiply-add:
 *   x, lse_m   as in mvlt_gemm_beam_candidates, lse over ALL N columns of the unprocessed row
 *   lp = x - lse_m;  seen(n): lp' = lp < 0 ? lp * penalty : lp / penalty (once, however often n occurs);  s = lp' + beam_scores[m]
 *   banned(n)  the n-gram rule and the min-length rule exactly as worded for MvltLogitRules above
 * Per sample g: the n_cand largest s over its UNBANNED entries, sorted descending, ties by the lower flat index beam * N + n.  A
 * banned entry is never returned and changes nothing else (it stays inside lse).  With no bit set and penalty 1 the lists are
 * those of mvlt_gemm_beam_candidates bit for bit.  A sample with fewer than n_cand unbanned entries gets (-inf, beam 0, token 0)
 * in the remaining slots; nothing is read or written out of bounds.  Integer comparisons only, no float atomics: the same
 * operands give the same lists run to run.
 * mvlt_beam_rules_plan is the PLAN of mvlt_decode_rules_plan over int32 histories seq[m, 0 .. *rules->col - 1], row stride ld_seq
 * (the layout of MvltBeamStep.seq; *col is clamped into [0, ld_seq]), one workgroup per row, ANY rows >= 1; rules->ids and ld_ids
 * are ignored.  Stateless like that plan (clear, then set).  Refusals (MVLT_ERR_ARG, nothing launched, nothing written): those of
 * mvlt_decode_rules_plan without its 64 rows and its ids / ld_ids, and seq NULL, ld_seq < 1.
 * mvlt_gemm_beam_candidates_rules: the plain product (in row chunks of 64), then the rule-aware selection, which reads
 * seen / banned / ld_words / penalty only ([M, ld_words] bitmaps; the caller runs the plan first, on the same stream).  Refusals
 * (nothing launched, nothing written): those of the _rules heads above without their M <= 64 (M = G * num_beams, any size),
 * ahead of those of mvlt_gemm_beam_candidates. */
int mvlt_beam_rules_plan(const MvltLogitRules* rules, const int32_t* seq, int64_t ld_seq, int rows, int V, void* stream);
int mvlt_gemm_beam_candidates_rules(const MvltGemm* p, const MvltBeamCand* c, const MvltLogitRules* rules, void* stream);
/* MLM decoder product with the forward of F.cross_entropy(ignore_index = -100) in its epilogue (csrc/headce.hip): the training
 * loss and per-token log-probabilities without a pass over stored logits, and with C == NULL without any logits at all.
 * p: A = the transformed hidden rows [M, K], B = W [N = V, K] (torch-Linear layout), bias f32 [V] (MVLT_EPI_BIAS, the only epilogue
 * bit honoured), dtype bf16 or f32, m_dev optional (only the first *m_dev rows exist), C optional ([M, ldc >= V], storage dtype).
 * Per element x = round_to_dtype(acc + bias[n]) -- the value the plain product stores, and the value every statistic below is
 * computed from, so exp(x - lse) in mvlt_ce_bwd_ragged sees the numbers the forward saw.  Per row m < min(M, *m_dev):
 *   lse[m] = max_n x + logf(sum_n __expf(x - max)) over n < V    (f32; every row, labelled or not)
 *   x_label[m] = x[m, labels[m]]                                 (f32; written only for 0 <= labels[m] < V)
 *   acc[0] = sum of (lse[m] - x_label[m]) over rows with labels[m] >= 0,  acc[1] = their number
 * (the layout mvlt_ce_fwd_ragged fills: acc[0] / acc[1] is the mean, mvlt_ce_bwd_ragged takes lse and acc + 1 unchanged).  A label
 * >= V makes acc[0] NaN.  Rows at or beyond *m_dev leave lse / x_label / C unwritten; *m_dev = 0 gives acc = (0, 0).
 * Summation shape (fixed: the same operands give the same bits, no float atomics): 64 x 128 tiles of the register-staged main
 * loop; per row and wave (max, sum) over its 64 columns -- 16 per lane in column order, then across the 4 lane groups by
 * xor-16 / xor-32 exchanges --, the two waves of a row meet in LDS, one (max, sum) pair per row and column tile goes to
 * `workspace`; a second launch (one wave per row) folds the ceil(V / 128) pairs, lane-strided in tile order and then by a
 * butterfly; a third, single-workgroup launch adds the rows' terms: thread t rows t, t + 1024, ..., then a tree in LDS.
 * workspace: mvlt_mlm_head_ce_workspace_bytes(M, V) bytes, 16-byte aligned.
 * Refusals (MVLT_ERR_ARG, nothing launched, nothing written): NULL p / h / A / B / bias / labels / lse / x_label / acc / workspace,
 * M, V or K < 1, ldc < V with C given, a workspace that is too small, a k-major operand, an epilogue bit other than
 * BIAS; operands the loop and the epilogue read or write in vectors: A / B / C / workspace not 16-byte aligned, lda or ldb not a
 * multiple of 16 bytes, ldc not a multiple of 4, bias / lse / x_label / acc not 4-byte and labels not 8-byte aligned.
 * MVLT_ERR_UNSUPPORTED: a dtype other than bf16 / f32. */
typedef struct MvltHeadCE {
    const int64_t* labels;              /* [M]; negative = ignored */
    float* lse; float* x_label;         /* [M] */
    float* acc;                         /* [2] */
    void* workspace; size_t workspace_bytes;
} MvltHeadCE;
int mvlt_mlm_head_ce(const MvltGemm* p, const MvltHeadCE* h, void* stream);
size_t mvlt_mlm_head_ce_workspace_bytes(int M, int V);
/* Sequence-level loss on decoded id rows (csrc/seqloss.hip): the loss of self-critical / reward-weighted fine-tuning,
 *   L = - sum_b sum_{t < len_b} w[b, t] log p(seq[b, t] | image, seq[b, :t]) / N,   N = sum_b len_b
 * (the reference's --scst path, run_report_generation.py:315-361, names a RewardCriterion it never defines: the definition is
 * this project's).  len_b = 1 + the index of the first id equal to eos in row b ([END] is itself scored); without one, the index
 * of the first id <= 0 (PAD); with neither, T.  Scalar and pointer arguments only: the struct registry and MVLT_ABI_VERSION stay.
 *
 * mvlt_seq_loss_plan: ids int64 [B, ld >= T], eos (negative: none), weights f32 read at weights[b * w_stride_b + t * w_stride_t]
 * (element strides, either may be 0), row0 / row_step: the encoder row of position (b, t) is row0 + b * row_step + t.  One
 * launch, one workgroup, no host sync, stateless (everything below is written on every call):
 *   len int32 [B];  tf_ids int64 [B, T] = ids for t < len_b, 0 behind (the teacher-forcing input: the encoder masks the tail as
 *   padding);  rows_dev int32 [1] = N;  and the packed plan in the layout mvlt_label_plan gives for labels = ids on the scored
 *   positions and -100 elsewhere: slot off_b + t (off = exclusive prefix sum of len) holds position (b, t), t < len_b:
 *   gather_row int32 [B T] = its encoder row, sel_labels int64 [B T] = ids[b, t], row_weight f32 [B T] = its weight; the
 *   positions behind the ends follow from slot N on in (b, t) order with their encoder row, label -100 and weight 0.
 *   A negative id ahead of an [END] has no token: its slot carries label -100 and weight 0 and its tf_ids entry is 0 (it keeps
 *   its place in the prefix and counts in N: the one case in which the packing is not mvlt_label_plan's).
 *   Two things the plan does not judge.  A PAD (id 0) ahead of an [END] lies inside the prefix: it is scored as label 0 with
 *   its weight, while the encoder treats the position as it treats any PAD inside a caption.  Ids must be below the vocabulary size V of the head that
 *   follows: mvlt_mlm_head_ce leaves x_label unwritten for a label >= V, so mvlt_seq_loss_fwd would add an undefined term for
 *   that row (nothing here knows V, and checking it needs a read-back: the caller's contract, as for the caption ids of the
 *   CE route).
 * Refusals (MVLT_ERR_ARG, nothing launched, nothing written): a NULL pointer, B outside 1 .. 4096, T outside 1 .. 512, ld < T,
 * a negative stride / row0 / row_step, a last row beyond INT32_MAX, int64 operands not 8-byte or the others not 4-byte aligned.
 *
 * mvlt_seq_loss_fwd: acc[0] = sum over i < n of row_weight[i] * (lse[i] - x_label[i]), acc[1] = (float)n, n = min(rows,
 * *rows_dev) (rows_dev NULL: rows), from the lse / x_label mvlt_mlm_head_ce wrote.  A row of weight 0 adds nothing and its lse /
 * x_label are not read.  One workgroup; summation shape (fixed, no float atomics, the same operands give the same bits): thread
 * t adds its terms fl(w * fl(lse - x_label)) of rows t, t + 1024, ... in order, then a binary tree over the 1024 partial sums
 * in LDS (t += t + 512, t += t + 256, ...).  *rows_dev = 0 gives (0, 0).
 * Refusals (MVLT_ERR_ARG, nothing launched): NULL lse / x_label / row_weight / acc, rows outside 1 .. 4096 * 512, a pointer
 * not 4-byte aligned.
 *
 * mvlt_ce_bwd_weighted: mvlt_ce_bwd_ragged with a coefficient per row.  For rows i < min(rows, *rows_dev) with labels[i] >= 0
 *   dlogits[i, n] = c_i * (__expf(x[i, n] - lse[i]) - [n == labels[i]])   n < V,
 *   c_i = fl(fl(fl(grad_scale * *grad_scale_dev) / max(*count, 1)) * row_weight[i])
 * -- the scalar first, so row_weight == 1 gives the bits of mvlt_ce_bwd_ragged.  Columns V .. ld - 1 and rows with a negative
 * label are zero-filled; a row with row_weight == 0 is zero-filled without reading its logits or its lse (a non-finite logit
 * there cannot leak); rows at or beyond *rows_dev are neither read nor written.  dlogits == logits (in place) is allowed;
 * bf16 and f32.  When ld is a multiple of 16 bytes (8 bf16 / 4 f32 elements) rows move as 16-byte vectors, two in flight per
 * thread; any other ld takes an element-wise loop.  Grid: rows x column slices, at most 2048 workgroups, rows beyond it strided.
 * Refusals (MVLT_ERR_ARG, nothing launched, nothing written): NULL logits / labels / lse / row_weight / count / dlogits, rows or
 * V < 1, ld < V or ld > INT32_MAX, logits / dlogits not 16-byte aligned when ld is a multiple of 16 bytes (not element-aligned
 * otherwise), labels not 8-byte and the f32 / int32 operands not 4-byte aligned.  MVLT_ERR_UNSUPPORTED: another dtype. */
int mvlt_seq_loss_plan(const int64_t* ids, int64_t ld, int B, int T, int64_t eos, const float* weights, int64_t w_stride_b,
                       int64_t w_stride_t, int row0, int row_step, int32_t* len, int64_t* tf_ids, int32_t* gather_row,
                       int64_t* sel_labels, float* row_weight, int32_t* rows_dev, void* stream);
int mvlt_seq_loss_fwd(const float* lse, const float* x_label, const float* row_weight, int rows, const int32_t* rows_dev,
                      float* acc, void* stream);
int mvlt_ce_bwd_weighted(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels, const float* lse,
                         const float* row_weight, const float* count, float grad_scale, const float* grad_scale_dev,
                         void* dlogits, const int32_t* rows_dev, void* stream);

/* ------------------------------------------------------------------ retrieval (csrc/retrieval.hip)
 * Scoring head of MVLBertForRetrieval (model.py:444-476) on the packed output of one encoder pass over P (image, caption)
 * pairs, in ONE launch: the [CLS] gather, BertPooler (dense + tanh, modeling_bert.py:451-463), BertPredictionHeadTransform
 * (dense + erf-GELU + LayerNorm), Linear(H, 2), the softmax over the two classes and the scatter of the class-1 probability
 * into a score matrix.  Per pair p < min(P, *p_dev), with x = hidden[row_start[p], :]:
 *   pooled = round_dtype(tanh(x Wp^T + bp))                     f32 accumulate, ONE rounding to the compute dtype
 *   t1     = round_dtype(gelu_erf(pooled Wt^T + bt))            f32 accumulate, ONE rounding to the compute dtype
 *   everything below is f32 and is never rounded to the compute dtype:
 *   mean = sum_n t1 / H,  var = sum_n (t1 - mean)^2 / H  (two passes),  y_n = (t1_n - mean) rsqrt(var + eps) gamma_n + beta_n
 *   logit_c = sum_n y_n Wo[c, n] + bo[c]  (c = 0, 1),  scores[out_index[p]] = e_1 / (e_0 + e_1),  e_c = expf(logit_c - max logit)
 * (the unfused route rounds the pooler product before tanh, t2 = LayerNorm(t1) and the logits to the compute dtype as well.)
 * A workgroup owns 16 pairs; their gathered rows and the block's `pooled` / `t1` stay in LDS between the two H x H MFMA
 * products (2 x 16 x (H + 8) elements: 66 KB at H = 1024), the weights stream from L2.  Fixed summation shapes: no atomics,
 * the same operands give the same bits.  Optional outputs (written when non-NULL, rows p < min(P, *p_dev) only):
 * pooled [P, H], t1 [P, H] in the compute dtype, logits f32 [P, 2].  Entries of `scores` no out_index names are not touched.
 * MVLT_ERR_ARG: a NULL required pointer, P < 1, ld_hidden < H, operands the kernel reads in 16-byte vectors (hidden, w_pool,
 * w_tr, pooled, t1) not 16-byte aligned or ld_hidden not a multiple of 8.  MVLT_ERR_UNSUPPORTED: whatever
 * mvlt_retrieval_head_supported refuses (bf16 only, H a multiple of 64, H <= 1024); callers then issue the separate launches. */
typedef struct MvltRetrievalHead {
    int dtype, P, H;
    const void* hidden; int64_t ld_hidden;      /* packed encoder output [R, ld_hidden >= H] */
    const int32_t* row_start;                   /* [P]: the [CLS] row of every pair */
    const int32_t* p_dev;                       /* optional, DEVICE int: the number of valid pairs (<= P) */
    const void* w_pool; const float* b_pool;    /* BertPooler.dense [H, H] (compute dtype), [H] */
    const void* w_tr; const float* b_tr;        /* transform.dense [H, H] (compute dtype), [H] */
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    const void* w_out; const float* b_out;      /* final Linear [2, H] (compute dtype), [2] */
    const int64_t* out_index;                   /* [P]: flat position of pair p in `scores` */
    float* scores;
    void* pooled; void* t1; float* logits;      /* optional outputs */
} MvltRetrievalHead;
int mvlt_retrieval_head_supported(int dtype, int H);
int mvlt_retrieval_head(const MvltRetrievalHead* p, void* stream);
/* Recall ranks of a score matrix (compute_ranks of run_retrieval.py:220-249 without the N x N label matrix and with the ties
 * decided): scores f32 [Ni, ld >= Nc], pair (i, j) matches iff image_group[i] == caption_group[j] (int64 ids).  Order: the
 * stable ascending sort reversed -- (score, index) lexicographic, among equal scores the HIGHER index first; NaN is smaller
 * than every number (and than -inf), -0 equals +0.  For row i let (s*, j*) be the lexicographic maximum over its matching
 * columns: i2t_rank[i] = the number of columns j with (scores[i, j], j) > (s*, j*), or Nc when the row has no match;
 * t2i_rank[j] likewise down column j over the rows (Ni without a match).  Two passes per line (maximum, then count), integer
 * compares on an order-preserving key, no atomics.  Rows: a workgroup per row, threads along it.  Columns: a workgroup per 64
 * columns, its threads run along a row of `scores` (coalesced) and its four waves take every fourth row.
 * MVLT_ERR_ARG: NULL pointers, Ni or Nc < 1, ld < Nc. */
int mvlt_recall_ranks(const float* scores, int64_t ld, int Ni, int Nc, const int64_t* image_group, const int64_t* caption_group,
                      int32_t* i2t_rank, int32_t* t2i_rank, void* stream);
/* counts[k] = |{i < n : rank[i] < ks[k]}| for the nk (1 .. 8) thresholds of the HOST array ks (recall@k = counts / n); counts is
 * a DEVICE int32 [nk], overwritten.  One workgroup, fixed order. */
int mvlt_recall_counts(const int32_t* rank, int n, const int32_t* ks, int nk, int32_t* counts, void* stream);

/* Report metrics (compute_scores of run_report_generation_cxr.py:274-312 -- BLEU-1..4, ROUGE-L, CIDEr -- on WordPiece id rows in
 * place of the strings that test() :335-349 builds on the host).  A row int64 [T <= 512] ends before its first id that is one of
 * the n_stop (0 .. 8) ids of the HOST array stop_ids, or at T.  flags: DEVICE uint8 [V], bit 1 CONT (the piece glues to the
 * previous one, "##..."), bit 2 JOIN ("-", the .replace(' - ', '-') of :346), bit 4 BREAK (".", the .replace('.', ' .') of
 * :290-291); NULL: every id is a word.  An id outside [0, V) has flags 0 and never indexes the table.  With n pieces left,
 * JOIN piece i glues to its left when 0 < i < n - 1, piece i + 1 is not CONT and piece i was not itself pulled by a gluing
 * piece i - 1; it then pulls piece i + 1.  Piece i starts a word when i == 0, else when it is BREAK, else not when it is CONT,
 * pulled or gluing, else it does.  A word is its sequence of piece ids, an n-gram its sequence of words; both are compared
 * through 64-bit keys: mix = the splitmix64 finaliser, fold(h, v) = mix(h + 0x9E3779B97F4A7C15 + v), a word = fold over its ids
 * from 0x243F6A8885A308D3, an n-gram of order n = fold over its word keys from 0x13198A2E03707344 + n, read as int64;
 * INT64_MAX is "no key" (a key equal to it becomes INT64_MAX - 1).  Two different n-grams among K collide with probability
 * about K^2 / 2^65.
 *
 * mvlt_report_ngram_keys: one workgroup per row of ids [rows, ld >= T]; keys int64 [rows, 4, T]: slot j of order n holds the key
 * of the row's j-th n-gram when it is the first occurrence in the row, INT64_MAX otherwise (duplicates, unused slots);
 * n_words int32 [rows].  Sorting all keys and counting equal neighbours gives the document frequency of CiderScorer.compute_doc_freq.
 *
 * mvlt_report_stats: one workgroup per row of hyp [rows, ldh >= Th], scored against row index[row] (int32, NULL: row itself,
 * rows <= N) of ref [N, ldr >= Tr]; an index outside [0, N) scores against an empty reference and reports its length as -1.
 * stats int32 [rows, 11] = hypothesis words, reference words, correct[4] (sum over the distinct hypothesis n-grams of min(count
 * in hypothesis, count in reference)), guess[4] (max(0, words - n + 1)), LCS length over words.  cider f64 [rows] follows
 * CiderScorer.compute_cider with one reference: tf-idf = count * (log N - log max(1, df)), df from the sorted table df_keys int64
 * [K] / df_counts int32 [K] by binary search (absent: 0); per order sum over the distinct hypothesis n-grams of min(h, r) * r,
 * divided by sqrt(sum h^2) * sqrt(sum r^2) when both are non-zero, times exp(-d^2 / 72) with d the difference of the two bigram
 * counts; the mean of the four orders times 10.  f64 throughout, every sum in a fixed order (no atomics): two runs agree bit
 * for bit.  All pointers but stop_ids are device memory.  Scalar arguments only: the struct registry and MVLT_ABI_VERSION stay.
 * MVLT_ERR_ARG (nothing launched): a NULL required pointer, rows or N < 1, T outside 1 .. 512, ld < T, n_stop outside 0 .. 8,
 * flags with V < 1, K < 0, K > 0 without tables, index NULL with rows > N, misaligned pointers. */
int mvlt_report_ngram_keys(const int64_t* ids, int64_t ld, int rows, int T, const uint8_t* flags, int V, const int64_t* stop_ids,
                           int n_stop, int64_t* keys, int32_t* n_words, void* stream);
int mvlt_report_stats(const int64_t* hyp, int64_t ldh, int rows, int Th, const int64_t* ref, int64_t ldr, int N, int Tr,
                      const int32_t* index, const uint8_t* flags, int V, const int64_t* stop_ids, int n_stop, const int64_t* df_keys,
                      const int32_t* df_counts, int K, int32_t* stats, double* cider, void* stream);

/* Decode step (model.py:82-108: 2 new tokens per sample): skinny product with the reduction split over workgroups:
 * acc[s][M][N] (f32, k_splits slabs) = A[:, k-slice s] B[:, k-slice s]^T, M <= 64, both operands k-contiguous, no epilogue;
 * k_splits workgroups share every 16-column tile, each WRITES the slab of its slice (plain stores: no float atomics, nothing
 * to zero, bit-reproducible).  Pair it with mvlt_layernorm_acc_fwd(nsplit = k_splits), which adds the slabs in slice order
 * and applies bias + residual + LayerNorm (the BertSelfOutput / BertOutput tail, modeling_bert.py:282-293,340-351).
 * Slice rule (pinned by tests/test_decode_tail_gpu.py): with nkb = K / k-block (k-block = 32 elements in bf16, 16 in f32) and
 * per = ceil(nkb / k_splits), slice s covers the k-blocks [s * per, min(nkb, (s + 1) * per)); a slice with no blocks is
 * written as zeros (the consumer sums ALL k_splits slabs); exactly [k_splits][M][N] floats are written, nothing behind them.
 * MVLT_ERR_ARG: NULL pointers, k_splits outside 1 .. 64.  MVLT_ERR_UNSUPPORTED: M > 64, a k-major operand, a non-zero
 * epilogue, K not a multiple of the k-block, lda / ldb not a multiple of 8 (bf16) / 4 (f32) elements or A / B not 16-byte
 * aligned.  A refused call writes nothing. */
int mvlt_gemm_skinny_accum(const MvltGemm* p, float* acc, int k_splits, void* stream);

/* column sums: out[n] = sum_m x[m*ld + n]  (bias gradients), f32 out.
 * workspace: f32 [mvlt_colsum_workspace_rows(M)][N]. */
int mvlt_colsum(int dtype, const void* x, int64_t ld, int M, int N, float* out, int accumulate,
                float* workspace, void* stream);
int mvlt_colsum_workspace_rows(int M);

/* ------------------------------------------------------------------ LayerNorm
 * y = LN(x)*gamma + beta over the last dim C (nn.LayerNorm at
 * visual_feature_extractor.py:308,314,422,553,653 eps 1e-5; HF BERT
 * LayerNorm eps 1e-12, modeling_bert.py:287,346,480).
 *  - merge_H/W != 0: input row r = (b,i,j) is the PatchMerging gather
 *    cat(x[2i,2j], x[2i+1,2j], x[2i,2j+1], x[2i+1,2j+1]) of x:[B,H*W,C/4]
 *    (visual_feature_extractor.py:435-440).
 *  - out_rowmap: y row = out_rowmap[r] (fuses roll(-s)+window_partition,
 *    :360-367, into the store).
 *  - gelu: y = gelu(LN(x)) (Swin final norm + Conv_layer nn.GELU, model.py:232-235);
 *    y_pre (optional) receives LN(x) for the backward pass.
 *  - mean/rstd (optional, f32 [rows]) are saved for the backward pass. */
typedef struct MvltLayerNorm {
    int dtype, rows, C; float eps;
    const void* x; const float* gamma; const float* beta;
    void* y; void* y_pre; float* mean; float* rstd;
    const int32_t* out_rowmap; int merge_H, merge_W; int gelu;
    const int32_t* rows_dev;         /* optional, DEVICE int: valid rows (<= rows); see MvltGemm.m_dev */
} MvltLayerNorm;
int mvlt_layernorm_fwd(const MvltLayerNorm* p, void* stream);

/* backward: dx (+= dres) ; dgamma/dbeta f32 [C].
 *  - dy_rowmap: dy row for logical row r is dy[dy_rowmap[r]].
 *  - gelu: dy is the gradient of gelu(LN(x)); y_pre must be given.
 *  - merge_H/W: dx is scattered back to x:[B,H*W,C/4].
 * workspace: f32 [2][mvlt_layernorm_bwd_workspace_rows()][C]. */
typedef struct MvltLayerNormBwd {
    int dtype, rows, C;
    const void* dy; const int32_t* dy_rowmap;
    const void* x; const float* mean; const float* rstd; const float* gamma;
    const void* y_pre; int gelu;
    const void* dres; void* dx;
    int merge_H, merge_W;
    float* dgamma; float* dbeta; int accumulate;
    float* workspace;
    /* optional second output, the gradient entering the residual BRANCH that produced x's summand:
     * dz[dz_rowmap ? dz_rowmap[r] : r] = dropout_mask(dx[r]; p, seed, tag, idx r*C+c) * dz_rowscale[r / rows_per_scale]
     * (Swin: window-order scatter + DropPath scale; BERT: hidden-dropout backward) */
    void* dz; const int32_t* dz_rowmap; const float* dz_rowscale; int dz_rows_per_scale;
    float dz_dropout_p; uint64_t seed; uint32_t tag;
    int defer_param_reduce;          /* 1: leave the partial rows in `workspace`; reduce them later, batched */
    const int32_t* rows_dev;         /* optional, DEVICE int: valid rows (<= rows); see MvltGemm.m_dev */
    /* optional: dy is the SUM of dy_parts (2 .. 4) tensors of the same shape, dy_part_stride elements apart, starting at `dy` (the
     * partial qkv-dgrad products of mvlt_swin_wmsa2_bwd): added in f32 while the rows are loaded, the sum rounded to bf16 once.
     * bf16, C = 4 * lanes * chunks widths (96 .. 1024), no gelu / merge; else MVLT_ERR_UNSUPPORTED.  0 / 1: plain dy. */
    int dy_parts; int64_t dy_part_stride;
} MvltLayerNormBwd;
int mvlt_layernorm_bwd(const MvltLayerNormBwd* p, void* stream);
int mvlt_layernorm_bwd_workspace_rows(void);
/* y[r,:] = LayerNorm(sum_s acc[s][r,:] + bias + residual[r,:]) * gamma + beta, rows <= a few hundred, C <= 2048; acc = the
 * nsplit slabs [nsplit][rows][C] (f32) of mvlt_gemm_skinny_accum (read only).  residual may be NULL.  The row is formed in
 * f32: slabs in slice order, then bias, then residual; mean and variance are two passes over it.
 * MVLT_ERR_ARG (nothing written): nsplit outside 1 .. 64, rows < 1, C < 1, C % 4 != 0 or C > 2048, a NULL pointer. */
int mvlt_layernorm_acc_fwd(int dtype, const float* acc, int nsplit, const float* bias, const void* residual, const float* gamma,
                           const float* beta, float eps, int rows, int C, void* y, void* stream);
/* deferred parameter-gradient reduction: one launch per 96 LayerNorms instead of one per LayerNorm.
 * items is a HOST array; workspace = the buffer given to mvlt_layernorm_bwd, nparts = mvlt_layernorm_bwd_nparts(rows, C). */
typedef struct MvltLnReduceItem { const float* workspace; int nparts, C; float* dgamma; float* dbeta; } MvltLnReduceItem;
int mvlt_layernorm_bwd_nparts(int rows, int C);
int mvlt_layernorm_param_reduce_batch(const MvltLnReduceItem* items, int n, void* stream);

/* ------------------------------------------------------------------ attention
 * One (sequence, head) problem per workgroup; Q,K,V come from a fused
 * projection buffer qkv[rows, 3*nH*hd] laid out [3][nH][hd] per row.
 * mode MVLT_ATTN_SWIN  : WindowAttention core (visual_feature_extractor.py:234-251):
 *      softmax(q*scale @ k^T + table[relidx(q,k)][h] + shift_mask) @ v, N=49,
 *      relidx and the 0/-100 shift mask (:318-344) computed in-kernel from
 *      (win_res, shift); sequences are windows, nW per image.
 * mode MVLT_ATTN_BIDIR : HF eager attention (modeling_bert.py:111-136) with the
 *      MVLBert bidirectional key mask cat(1,image_mask,1,text>0) (model.py:125-128)
 *      rebuilt in-kernel from text_ids (int64 [B,T]) and optional image_mask (u8 [B,n_img]);
 *      masked keys get -10000 (model.py:182).
 * mode MVLT_ATTN_SEQ2SEQ : key allowed iff k<=q or k<=obj_end (model.py:118-123).
 * Dropout on the probabilities (attention_probs_dropout_prob) uses the counter RNG.
 * lse (f32 [nseq,nH,L]) is saved for the backward pass. */
enum { MVLT_ATTN_SWIN = 0, MVLT_ATTN_BIDIR = 1, MVLT_ATTN_SEQ2SEQ = 2 };
typedef struct MvltAttn {
    int dtype, mode;
    int nseq, L, nH, hd;
    const void* qkv; void* out;          /* out: [nseq*L, nH*hd] */
    float* lse;
    float scale;
    /* swin */
    const float* bias_table; int nW, win_res, shift;
    /* bert */
    const int64_t* text_ids; int T; const uint8_t* image_mask; int obj_end;
    float dropout_p; uint64_t seed; uint32_t tag;
    /* backward only */
    const void* dout; void* dqkv; float* dbias_table; float* delta_ws;
    /* packed rows (optional, MVLBert modes): sequence s occupies rows [row_start[s], row_start[s]+seq_len[s])
     * of qkv/out/dout/dqkv, seq_len[s] <= L; trailing zero-padded caption positions are simply absent
     * (they are masked keys in BIDIR mode and lie above the causal diagonal in SEQ2SEQ mode, so no kept
     * row ever reads them).  lse / delta_ws keep the [nseq,nH,L] layout.  NULL = dense [nseq*L] rows.
     * Rows outside every sequence are neither read (qkv / dout) nor written (out / dqkv), and neither are the lse
     * entries at q >= seq_len[s]. */
    const int32_t* row_start; const int32_t* seq_len;
    /* backward only, MVLT_ATTN_SWIN only (optional): the output projection's dgrad inside the launch.  When non-NULL, `dout`
     * is the gradient of the PROJECTION's output ([nseq*L, nH*hd], window order) and dout_weight the projection weight
     * [nH*hd (out), nH*hd (in)] row-major in the compute dtype (WindowAttention.proj, visual_feature_extractor.py:252):
     * the kernel forms dO_h = dout . W[:, hd*h .. hd*h + hd - 1] per head itself (rounded to the compute dtype, as the
     * separate product would).  bf16, hd 32, nH 3 / 6 / 12, no attention dropout, shift 0 or 3; anything else:
     * MVLT_ERR_UNSUPPORTED. */
    const void* dout_weight;
    /* backward only (optional; honoured by the bf16 Swin launch, ignored elsewhere): a byte range a LATER kernel will stream,
     * same contract as MvltGemm.prefetch (one dword of every 128-byte line is read and dropped) */
    const void* prefetch; int64_t prefetch_bytes;
} MvltAttn;
int mvlt_attn_fwd(const MvltAttn* p, void* stream);
int mvlt_attn_bwd(const MvltAttn* p, void* stream);   /* delta_ws: f32 [nseq,nH,L] */
/* The same, and `event` (a hipEvent_t of the caller) completes with the call's LAST kernel: it rides on that dispatch as its
 * stop event instead of a marker packet behind it (an event record costs the recording stream ~5 us, this form ~2.5 us:
 * scripts/event_cost.hip).  For the fork of the weight-gradient stream, which follows the attention backward of every
 * BertLayer / Swin block (modeling_bert.py:282-293 backward; visual_feature_extractor.py:224-254 backward): the caller
 * then hipStreamWaitEvent()s on it.  Nothing is recorded when the call fails. */
int mvlt_attn_bwd_ev(const MvltAttn* p, void* stream, void* event);
/* The kernel mvlt_attn_fwd (bwd = 0) / mvlt_attn_bwd (bwd != 0) would launch for *p, without launching anything:
 * an MvltAttnRoute, or MVLT_ERR_ARG when the call itself would answer that.  For tests that must know which kernel they
 * check; the launch takes its route from the same function. */
enum MvltAttnRoute {
    MVLT_ATTN_ROUTE_UNSUPPORTED = 0,       /* the call answers MVLT_ERR_UNSUPPORTED */
    MVLT_ATTN_ROUTE_SWIN_FWD = 1,          /* attn_fwd_kernel<T, 32, 4, SWIN> */
    MVLT_ATTN_ROUTE_BERT_FWD_KT5 = 2,      /* KT = 5 / 9 / 13 key tiles, L <= 80 / 144 / 208: bf16 bert_attn_fwd_kernel<KT, NW> (one
                                            * query tile per wave), f32 attn_fwd_kernel<float, 64, KT> */
    MVLT_ATTN_ROUTE_BERT_FWD_KT9 = 3,
    MVLT_ATTN_ROUTE_BERT_FWD_KT13 = 4,
    MVLT_ATTN_ROUTE_SWIN_BWD_KS0 = 5,      /* swin_attn_bwd2_kernel (scores once; bf16, no dropout, shift 0 / 3) */
    MVLT_ATTN_ROUTE_SWIN_BWD_KS3 = 6,      /* ... with dout_weight, 3 / 6 / 12 heads */
    MVLT_ATTN_ROUTE_SWIN_BWD_KS6 = 7,
    MVLT_ATTN_ROUTE_SWIN_BWD_KS12 = 8,
    MVLT_ATTN_ROUTE_SWIN_BWD = 9,          /* attn_bwd_kernel<T, 32, 4, SWIN> (f32, dropout, other shifts) */
    MVLT_ATTN_ROUTE_BERT_BWD2_NW5 = 10,    /* bert_attn_bwd2_kernel, one launch: bf16, L <= 160 (NW5: 10 key tiles per launch, one
                                            * wave each) / 192 (NW6: 12 key tiles) */
    MVLT_ATTN_ROUTE_BERT_BWD2_NW6 = 11,
    MVLT_ATTN_ROUTE_BERT_BWD_SPLIT_KT5 = 12,   /* attn_bwd_split_kernel, two launches through delta_ws */
    MVLT_ATTN_ROUTE_BERT_BWD_SPLIT_KT9 = 13,
    MVLT_ATTN_ROUTE_BERT_BWD_SPLIT_KT13 = 14,
    MVLT_ATTN_ROUTE_BERT_BWD_KT5 = 15,     /* attn_bwd_kernel<T, 64, KT>: no delta_ws, L <= 144 */
    MVLT_ATTN_ROUTE_BERT_BWD_KT9 = 16
};
int mvlt_attn_route(const MvltAttn* p, int bwd);
/* 1 exactly when mvlt_attn_bwd of a MVLT_ATTN_SWIN call (L 49, no dropout) with dout_weight set would take
 * MVLT_ATTN_ROUTE_SWIN_BWD_KS3 / 6 / 12, answered by that same route function: callers ask before they choose between
 * dout_weight and a separate projection dgrad. */
int mvlt_swin_bwd_proj_supported(int dtype, int nseq, int nH, int hd, int shift);
/* Attention maps (MVLBert modes): the probabilities mvlt_attn_fwd never materialises, recomputed from the call's qkv and the lse
 * it wrote (HF BertSelfAttention's attention_probs, modeling_bert.py:130, what output_attentions returns), eval mode:
 *     out[s, h, i, j] = exp(scale * q_{q0+i} . k_{k0+j} + bias(q0+i, k0+j) - lse[s, h, q0+i])        f32 [nseq, nH, nq, nk]
 * for the queries [q0, q0 + nq) and the keys [k0, k0 + nk) of every sequence; bias is the additive term of the forward (BIDIR:
 * -10000 on padded text keys and on image_mask == 0; SEQ2SEQ: -10000 unless k <= q or k <= obj_end), so masked entries are
 * exactly 0.  *p is the descriptor of that layer's forward call: dtype, mode, nseq, L, nH, hd, qkv, scale, text_ids / T /
 * image_mask / obj_end, row_start / seq_len are read, and lse (written by the forward); out, the dropout and the backward
 * fields are ignored.  The forward's arithmetic: operands in the compute dtype, f32 accumulation over hd, __expf.
 * Packed rows: keys >= seq_len[s] are exactly 0, query rows >= seq_len[s] are rows of zeros (their lse is not read), activation
 * rows outside every sequence are not read.
 * flags: MVLT_ATTNMAP_HEAD_MEAN -- out is [nseq, 1, nq, nk], the mean over heads (summed in head order inside one workgroup);
 *        MVLT_ATTNMAP_RENORM    -- every OUTPUT row (after the head mean, if both are set) is divided by its own sum over the
 *                                  selected keys: the attention within the key range; a row whose sum is 0 stays 0.
 * One launch, no atomics.  The arguments are scalars and an existing struct: the struct registry and MVLT_ABI_VERSION stay.
 * MVLT_ERR_ARG (nothing launched): a NULL p / qkv / lse / out, unknown flag bits, a range outside [0, L], nq <= 0 or nk <= 0,
 * the mode checks of mvlt_attn_fwd, qkv not 16-byte aligned.  MVLT_ERR_UNSUPPORTED: MVLT_ATTN_SWIN, hd != 64, nk > 208 (the
 * forward's own L range), a dtype other than bf16 / f32. */
enum { MVLT_ATTNMAP_HEAD_MEAN = 1, MVLT_ATTNMAP_RENORM = 2 };
int mvlt_attn_probs(const MvltAttn* p, int q0, int nq, int k0, int nk, int flags, float* out, void* stream);

/* ------------------------------------------------------------------ fused Swin (S)W-MSA (SURVEY.md 8b `swin_wmsa`)
 * The attention half of SwinTransformerBlock.forward in ONE launch (visual_feature_extractor.py:356-384 around
 * WindowAttention.forward :224-254):
 *   y = x + rowscale[b] * proj( softmax(q k^T * scale + rel_pos_bias + shift_mask) v ),  q,k,v = qkv(norm1(x))
 * with roll(-shift) + window_partition on the way in and window_reverse + roll(+shift) on the way out expressed
 * by the row map w2n (window-order row -> token row, the INT tables of SURVEY 8a2/8a3); window 7, head_dim 32.
 * x, y: [B*res*res, C] token order (y may not alias x).  The qkv tensor and the attention output never make an
 * HBM round trip.  Training: the optional pointers receive what the backward pass needs, as write-only outputs:
 *   xn_win   [B*res*res, C]  norm1(x), window order (A operand of the qkv weight gradient)
 *   attn_out [B*res*res, C]  attention output, window order (A operand of the proj weight gradient)
 *   lse      f32 [B*nW, nH, 49], mean / rstd f32 [B*res*res] (token order) */
typedef struct MvltSwinWmsa {
    int dtype, B, res, C, nH, shift;
    const void* x; void* y; const int32_t* w2n;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    const void* wqkv; const float* bqkv; const void* wproj; const float* bproj;
    const float* bias_table; float scale;
    const float* rowscale;             /* optional DropPath keep/(1-p), f32 [B] */
    void* xn_win; void* attn_out; float* lse; float* mean; float* rstd;
    /* backward only (mvlt_swin_wmsa2_bwd, see there) */
    const void* dy_win; void* dqkv; void* dxn_win;
    /* optional, training: q,k,v in the [B*res*res, 3C] window-order layout MvltAttn uses (forward: write-only
     * output, so the unfused mvlt_attn_bwd can run on a fused forward; backward: read instead of recomputed) */
    void* qkv_win;
    /* mvlt_swin_wmsa_fwd only: 1 = one workgroup per (window, head group) and NO output projection: attn_out [B*res*res, C]
     * (window order, required) is the result, y / wproj / bproj / rowscale are unused; follow with mvlt_gemm
     * (bias, DropPath row scale, window-reverse row map, residual).  For launches with too few windows to fill the chip. */
    int head_split;
    /* mvlt_swin_wmsa2_bwd only: per-workgroup sums of the relative-position-bias gradient (see there), or NULL */
    float* dbias_ws;
} MvltSwinWmsa;
int mvlt_swin_wmsa_supported(int dtype, int C, int nH);   /* 1 when the fused kernels cover this width */
int mvlt_swin_wmsa_fwd(const MvltSwinWmsa* p, void* stream);

/* Second design of the fused forward (csrc/wmsa2.hip, bf16): a workgroup owns TWO windows (98 rows share every weight
 * fragment) and a GROUP of heads; the head groups of a window pair run in different workgroups and meet through
 * attn_out (write-through stores, one arrival flag per head group, sc1 loads) before each computes its own output columns of the
 * projection -- still ONE launch, and 256 workgroups at stage 2 of a B = 32 step where the first design has 128.
 * Same MvltSwinWmsa fields as mvlt_swin_wmsa_fwd (head_split ignored) with two differences: attn_out is REQUIRED (it is
 * the exchange buffer; eval callers pass scratch), and sync_ws is an int32 workspace of mvlt_swin_wmsa2_sync_words(B, res)
 * words that the caller zeroes ONCE when it allocates it: every launch leaves its counters zeroed.  Layout (independent
 * of B, so one workspace serves every launch of a stream): word 0 = STICKY ERROR COUNT, words 1..15 unused, then
 * {arrivals, readers done} per window pair.  One workspace per stream (launches that may overlap must not share counters).
 * Failure mode: the groups of a window pair wait for each other inside the launch, which needs them co-resident (the
 * launch is persistent with at most one workgroup per CU, grid <= #CUs and a multiple of the group count).  A wait is
 * bounded (2 s by default, mvlt_swin_wmsa2_set_timeout_ms); when it runs out the kernel adds 1 to word 0 AND writes NaN
 * into that unit's rows of y, so the failure reaches the loss even when nobody reads the word.  Callers read word 0 where
 * they synchronise anyway (PretrainStep does, one step late, without a sync) and raise.
 * Replaces visual_feature_extractor.py:224-254, 356-384 exactly like mvlt_swin_wmsa_fwd. */
int mvlt_swin_wmsa2_supported(int dtype, int B, int res, int C, int nH);
int mvlt_swin_wmsa2_sync_words(int B, int res);
int mvlt_swin_wmsa2_fwd(const MvltSwinWmsa* p, int32_t* sync_ws, void* stream);
/* The backward of the same block half in ONE launch, in the second design's shape (round 6): output-projection dgrad +
 * attention backward + qkv dgrad (visual_feature_extractor.py:224-254 backward); unit = (two windows, 3 heads), window order
 * throughout.  Reads dy_win [B*res*res, C] (gradient of the projection's output, rowscale applied), qkv_win, lse, wproj, wqkv,
 * bias_table, scale, shift; writes dqkv [B*res*res, 3C] and -- because the qkv dgrad sums over the heads and the head groups
 * are different workgroups that never meet -- nparts = mvlt_swin_wmsa2_bwd_parts() PARTIAL products
 *   dxn_win [nparts][B*res*res, C],  sum over the parts (f32) = dqkv Wqkv,
 * which mvlt_layernorm_bwd adds while it loads them (MvltLayerNormBwd.dy_parts); dbias_table f32 [169, nH] is ACCUMULATED.
 * bf16, C = 96 / 192 / 384 with nH = C / 32, shift 0 or 3, an even number of windows; else MVLT_ERR_UNSUPPORTED.
 * _ev: `event` completes with the kernel (as mvlt_attn_bwd_ev). */
int mvlt_swin_wmsa2_bwd_parts(int dtype, int B, int res, int C, int nH);    /* nH / 3, or 0 = shape not covered */
/* Relative-position-bias gradient of that launch: every workgroup stores the sums of its units' dS along the 169 diagonals for its
 * three heads into MvltSwinWmsa.dbias_ws, f32 [mvlt_swin_wmsa2_bwd_workgroups()][3 * 169] (plain stores: nothing to zero, no
 * atomics), and mvlt_swin_wmsa2_bwd_dbias ADDS the workgroups of up to any number of launches into their tables
 * (dbias_table f32 [169, nH]) in a fixed order -- one small launch for all Swin blocks of a step; items is a HOST array.
 * (dbias_ws may be NULL: no bias gradient.) */
typedef struct MvltSwinDbiasItem { const float* ws; int nwg; int nH; float* dbias_table; } MvltSwinDbiasItem;
int mvlt_swin_wmsa2_bwd_workgroups(int dtype, int B, int res, int C, int nH);
int mvlt_swin_wmsa2_bwd_dbias(const MvltSwinDbiasItem* items, int n, void* stream);
int mvlt_swin_wmsa2_bwd(const MvltSwinWmsa* p, void* stream);
int mvlt_swin_wmsa2_bwd_ev(const MvltSwinWmsa* p, void* stream, void* event);
int mvlt_swin_wmsa2_set_timeout_ms(int ms);    /* bound of the hand-off wait, process-wide; 0 restores the default (2000) */
/* Diagnostic: `blocks` workgroups of 256 threads, each holding lds_bytes of LDS, spin for `usec` microseconds (100 MHz
 * real-time clock) and exit.  The tests use it to take CUs away from a launch that needs its workgroups co-resident. */
int mvlt_debug_hold_cus(int blocks, int lds_bytes, int usec, void* stream);
/* Diagnostic: copy `bytes` (multiple of 16, 16-byte aligned; dst may equal src) with `blocks` persistent workgroups of 256
 * threads and `inflight` (1..4) 16-byte loads in flight per thread -- the launch geometry of a ring collective's kernel,
 * i.e. a few hundred GB/s for milliseconds.  bench.py's one-GPU rehearsal of the data-parallel step issues it where the
 * all-reduce of a gradient bucket would run (MVLT_DDP_REHEARSE, mvlt_amd.ddp).  No reference counterpart (the reference
 * has no distributed code). */
int mvlt_debug_stream_copy(void* dst, const void* src, int64_t bytes, int blocks, int inflight, void* stream);

/* ------------------------------------------------------------------ data movement / embeddings
 * PatchEmbed im2col (visual_feature_extractor.py:562): img f32 NCHW [B,3,S,S]
 * -> cols [B*(S/P)^2, 3*P*P] in (c,dy,dx) order = Conv2d weight.view(96,-1). */
int mvlt_im2col_patch(int dtype, const float* img, void* cols, int B, int Cin, int S, int P, void* stream);

/* MVLBert.get_embedding (model.py:133-158): out[b,pos] = src(pos) + type_emb[pos<=obj_end] + pos_emb[pos]
 * with src = word_emb[cls] | image_feature | word_emb[sep] | word_emb[text];
 * NO LayerNorm/dropout.  Tables are f32 masters. */
typedef struct MvltEmbed {
    int dtype, B, n_img, T, H;
    const int64_t* text_ids;            /* [B,T] or NULL when T==0 */
    const void* image_feature;          /* [B,n_img,H] dtype */
    const float* word_emb; const float* pos_emb; const float* type_emb;
    int cls_id, sep_id, pos_offset, type_override;  /* cached step: pos_offset=past, type_override=0, n_img=-1 */
    void* out;                          /* [B, L, H] */
    /* backward */
    const void* dout; void* dimage; float* dword; float* dpos; float* dtype_emb;
    /* packed rows (optional): sequence b is written to / read from rows row_start[b] + pos, pos < seq_len[b] */
    const int32_t* row_start; const int32_t* seq_len;
    const int32_t* pos_offset_dev;      /* optional (forward): added to pos_offset, read on the device (replayed decode step) */
    /* backward: rows of the position / token-type tables (0 = unknown).  mvlt_embed_bwd OVERWRITES dpos rows
     * [pos_offset, pos_offset + L) and the dtype_emb rows in use with batch sums in a fixed order (no atomics,
     * bit-reproducible); with the row counts given it also zeroes every other row of the two tables, so the caller
     * clears only dword (which is accumulated with float atomics: a scatter-add over the batch's token ids). */
    int pos_rows, type_rows;
} MvltEmbed;
/* Packing plan of a ragged caption batch, computed ON THE DEVICE (no host sync): sample b keeps the sequence
 * positions [0, n_img + 2 + len_b) where len_b = 1 + the last caption position t with text_ids[b,t] != 0 or
 * (labels != NULL and labels[b,t] >= 0); the zero-padded tail beyond it is a masked key in the bidirectional mode
 * (model.py:125-128), lies above the causal diagonal in the seq2seq mode (:118-123) and carries no label, so no
 * kept row ever reads it.  Outputs: seq_len[b] = n_img + 2 + len_b, row_start[b] = exclusive prefix sum,
 * total_rows[0] = sum (feeds MvltGemm.m_dev / MvltLayerNorm.rows_dev), row_start64 = the same as int64 (index
 * tensors), text_row[b*T + t] = int64 packed row of caption position t (row_start[b] -- the [CLS] row, finite
 * data -- for positions beyond len_b: their label is -100 by construction).  B <= 65536. */
int mvlt_pack_plan(const int64_t* text_ids, const int64_t* labels, int B, int T, int n_img,
                   int32_t* row_start, int32_t* seq_len, int32_t* total_rows, int64_t* row_start64, int64_t* text_row,
                   void* stream);
/* MLM head on the labelled rows (F.cross_entropy(ignore_index=-100), model.py:410, only reads them): stable partition
 * of the N caption positions, labelled ones first.  gather_row[slot] = text_row[i] (the packed row of position i;
 * i itself when text_row is NULL), sel_labels[slot] = labels[i], count[0] = number of labelled positions (feeds
 * MvltGemm.m_dev).  One launch, no host sync; N <= 2^20. */
int mvlt_label_plan(const int64_t* labels, const int64_t* text_row, int N, int32_t* gather_row, int64_t* sel_labels,
                    int32_t* count, void* stream);
/* out[rowmap[i], :] = in[i, :] for i < min(rows, *count): backward of a row gather with unique source rows */
int mvlt_rows_scatter(int dtype, const void* in, void* out, int rows, int C, const int32_t* rowmap,
                      const int32_t* count, void* stream);
int mvlt_embed_fwd(const MvltEmbed* p, void* stream);
/* mvlt_embed_fwd with the position of batch row b shifted by row_shift[b] (int32 [B], device): position row
 * pos + pos_offset (+ *pos_offset_dev) + row_shift[b], clamped into [0, pos_rows).  Meant for the cached-step layout (n_img = -1,
 * type_override = 0) of a decode whose rows carry prompts of different lengths.  The same sums in the same order: an all-zero
 * table is bit for bit mvlt_embed_fwd.  MVLT_ERR_ARG: what mvlt_embed_fwd refuses, a NULL row_shift, pos_rows <= 0 (the clamp
 * needs the table's size) or pos_offset outside [0, pos_rows).  An existing struct plus a pointer: the struct registry and
 * MVLT_ABI_VERSION stay as they are. */
int mvlt_embed_fwd_rows(const MvltEmbed* p, const int32_t* row_shift, void* stream);
/* backward: ONLY dword is accumulated (float atomics over the batch's token ids, the [CLS] / [SEP] rows included): zero it
 * first.  dpos / dtype_emb are OVERWRITTEN with ordered batch sums -- a second call does not add to the first -- and rows
 * outside the range in use are zeroed only when pos_rows / type_rows are given (see the struct). */
int mvlt_embed_bwd(const MvltEmbed* p, void* stream);

/* out[i,:] = scale[i_src / rows_per_scale] * mask(in[src,:]) where src = rowmap ? rowmap[i] : i;
 * dropout mask (p>0) indexed by src*C + c.  Used for DropPath / dropout backward
 * and window-order gathers of gradients. */
int mvlt_rows_transform(int dtype, const void* in, void* out, int rows, int C, const int32_t* rowmap,
                        const float* rowscale, int rows_per_scale,
                        float dropout_p, uint64_t seed, uint32_t tag, void* stream);

/* elementwise helpers */
int mvlt_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream);
int mvlt_gelu_fwd(int dtype, const void* x, void* y, int64_t n, void* stream);
int mvlt_gelu_bwd(int dtype, const void* x, const void* dy, void* dx, int64_t n, void* stream); /* dx = dy*gelu'(x) */
int mvlt_softmax_rows(int dtype, const void* x, int64_t ld, int rows, int V, float* out, void* stream); /* f32 [rows,V] */
int mvlt_tanh_fwd(int dtype, const void* x, void* y, int64_t n, void* stream);
int mvlt_tanh_bwd(int dtype, const void* y, const void* dy, void* dx, int64_t n, void* stream);
int mvlt_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, uint32_t tag, void* stream);
/* the Gumbel noise of mvlt_gemm_sample as its kernel computes it: out[m * N + n] (f32, rows * N < 2^32) for one (seed, tag) */
int mvlt_gumbel_noise(uint64_t seed, uint32_t tag, int rows, int N, float* out, void* stream);
int mvlt_droppath_scale(float* scale, int B, float p, uint64_t seed, uint32_t tag, void* stream);
/* every DropPath scale of a forward pass in one launch (visual_feature_extractor.py:30-44 for each of the 2 x 24 residual
 * branches): scale [rows, B] f32, row r keeps sample b with probability 1 - probs[r] (device f32 [rows], each < 1) and
 * holds 1 / (1 - probs[r]) or 0; row r draws with tag + r */
int mvlt_droppath_scales(float* scale, const float* probs, int rows, int B, uint64_t seed, uint32_t tag, void* stream);
/* Row plans of the Swin blocks that run their Mlp branch only on the samples DropPath keeps, all blocks in one launch and with
 * nothing read back: block i reads row row0 + i * row_step of `scale` ([*, B] f32; the tensor of mvlt_droppath_scales holds
 * block i's Mlp branch in row 2 i + 1: row0 = 1, row_step = 2); a sample is kept iff its scale is not 0.  lt = DEVICE int32
 * [nblk], the tokens per sample of block i (0, or rows_i = B * lt[i] > ld: the block takes no plan and its outputs are left
 * alone).  For every other block:
 *   perm[i * ld + j]  position j of the compact order -> logical row b * lt + t: the kept samples first, in sample order, the
 *                     dropped ones behind them, tokens of a sample in order -- a full permutation of 0 .. rows_i - 1
 *   inv[i * ld + r]   its inverse
 *   count[i]          kept samples * lt[i] (the m_dev of the block's Mlp products)
 * MVLT_ERR_ARG: a NULL pointer, nblk < 1, B < 1 or B > 4096, ld < 1, row0 < 0, row_step < 0. */
int mvlt_droppath_plan(const float* scale, int row0, int row_step, const int32_t* lt, int nblk, int B, int64_t ld,
                       int32_t* perm, int32_t* inv, int32_t* count, void* stream);

/* ------------------------------------------------------------------ losses
 * F.cross_entropy(logits, labels, ignore_index=-100) (model.py:410,418):
 * logits [rows, ld>=V] dtype; loss_sum/count are f32 scalars (device),
 * lse f32 [rows].  bwd writes dlogits = scale*(softmax - onehot) for valid
 * rows and 0 for ignored rows, where scale = grad_scale / max(count,1)
 * (mean reduction), in place over logits when dlogits == logits. */
int mvlt_ce_fwd(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels,
                float* lse, float* loss_sum, float* count, void* stream);
int mvlt_ce_bwd(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels,
                const float* lse, const float* count, float grad_scale, const float* grad_scale_dev,
                void* dlogits, void* stream);   /* grad_scale_dev (optional): upstream dL/dloss on the device */
/* the same with the number of valid rows on the DEVICE (rows = upper bound; see MvltGemm.m_dev): rows beyond
 * *rows_dev are neither read nor written */
int mvlt_ce_fwd_ragged(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels,
                       float* lse, float* loss_sum, float* count, const int32_t* rows_dev, void* stream);
int mvlt_ce_bwd_ragged(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels,
                       const float* lse, const float* count, float grad_scale, const float* grad_scale_dev,
                       void* dlogits, const int32_t* rows_dev, void* stream);

/* ------------------------------------------------------------------ optimizer
 * torch.optim.AdamW step (run_pretrain.py:165-166: lr 4e-5, betas (0.9,0.999),
 * eps 1e-6, weight_decay 1e-4) over one flat f32 segment; also refreshes the
 * bf16 compute copy (shadow, may be NULL).  grad_scale multiplies g first
 * (1/world_size for DDP averaging). */
int mvlt_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
               int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
               int step, float grad_scale, void* stream);
/* Global-norm gradient clipping and non-finite step skip, without a host round trip (three plain-argument entry points, no struct).
 * mvlt_grad_sumsq: sum of squares of g[0..n) in f64 -- every element is widened before it is squared, so the squares are exact
 * and 3e19 does not overflow -- over a FIXED grid of mvlt_grad_sumsq_parts() workgroups: workgroup b stores its sum to partial[b],
 * or adds it to what is there when accumulate != 0.  Consecutive calls on one stream add the ranges of a step in a fixed order:
 * no float atomics, bit-reproducible.  g 16-byte aligned, n >= 1, partial holds mvlt_grad_sumsq_parts() doubles. */
int mvlt_grad_sumsq_parts(void);
int mvlt_grad_sumsq(const float* g, int64_t n, double* partial, int accumulate, void* stream);
/* sum = partial[0] + ... + partial[nparts - 1] (f64, index order);
 *   out[0]   = norm = (float)(fabs(grad_scale) * sqrt(sum))
 *   out[1]   = coef = min(1, max_norm / (norm + 1e-6f)) in f32 (torch.nn.utils.clip_grad_norm_; a NaN norm gives a NaN coef);
 *                     1 when max_norm <= 0 (no clipping)
 *   flags[0] = skip = skip_nonfinite && !isfinite(sum);   flags[1] += skip (running count) */
int mvlt_grad_norm_finish(const double* partial, int nparts, float grad_scale, float max_norm, int skip_nonfinite,
                          float* out, int32_t* flags, void* stream);
/* mvlt_adamw with the gradient scale grad_scale * *coef_dev (one f32 product); writes NOTHING when *skip_dev != 0.  The element
 * arithmetic is mvlt_adamw's own: with *coef_dev == 1 and *skip_dev == 0 the results are bit-identical. */
int mvlt_adamw_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16,
                       int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int step, float grad_scale, const float* coef_dev, const int32_t* skip_dev, void* stream);
/* The sweep with parameter groups resolved inside the launch (plain arguments, no struct): a contiguous range stays ONE launch
 * however many groups it crosses.
 *   block_group[b]   (uint8)  group of elements [64 b, 64 b + 64) of THIS range: it points at the byte of the range's first block
 *                             and spans n / 64 bytes.  Every id must be < ngroups (the caller guarantees it; an id in
 *                             [ngroups, 256) reads an unset table slot, never out of bounds).
 *   group_lr_scale[g], group_weight_decay[g]   (f32 [ngroups], device)   group g runs with lr_g = lr * group_lr_scale[g] (one f32
 *                             product) and its own weight decay; otherwise the element arithmetic is mvlt_adamw's own: a table of
 *                             (1, wd) gives mvlt_adamw's results bit for bit.
 *   lr               stays an argument: a schedule moves it every step, the tables are static.
 *   coef_dev / skip_dev       both NULL: plain.  Both set: mvlt_adamw_guarded's semantics (gradient scale grad_scale * *coef_dev,
 *                             nothing written when *skip_dev != 0).
 * MVLT_ERR_ARG before any launch: a NULL required pointer (shadow_bf16 alone may be NULL), n < 64 or n % 64 != 0, ngroups outside
 * 1..256, step < 1, param / grad / exp_avg / exp_avg_sq not 16-byte aligned, exactly one of coef_dev / skip_dev set.
 * mvlt_adamw_groups_block(): the block size of the map (64 elements); a binding checks it against its arena alignment. */
int mvlt_adamw_groups_block(void);
int mvlt_adamw_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t n,
                      const uint8_t* block_group, const float* group_lr_scale, const float* group_weight_decay, int ngroups,
                      float lr, float beta1, float beta2, float eps, int step, float grad_scale,
                      const float* coef_dev, const int32_t* skip_dev, void* stream);

/* ------------------------------------------------------------------ decode (greedy, KV cache)
 * 2-token cached step attention (model.py:82-108): q rows = n_new new tokens,
 * keys = cache[0..past) + new; causal over the new tokens. */
typedef struct MvltAttnCached {
    int dtype, B, nH, hd, past, n_new, cache_cap;
    const void* qkv_new;                /* [B*n_new, 3*nH*hd] */
    void* k_cache; void* v_cache;       /* [B, nH, cache_cap, hd]; new K/V appended at `past` */
    void* out;                          /* [B*n_new, nH*hd] */
    float scale;
    const int32_t* past_dev;            /* optional: `past` read from device memory instead (a decode loop that
                                           is replayed without host involvement keeps its position on the GPU) */
} MvltAttnCached;
int mvlt_attn_cached(const MvltAttnCached* p, void* stream);
/* The same step for a batch whose rows sit at DIFFERENT positions (ragged text prompts in front of a decode): batch row b is at
 *   past_b = past + row_shift[b]          (row_shift: int32 [B], device; <= 0 in the decode loops; past = p->past or *p->past_dev)
 * It appends its n_new K/V rows at past_b .. past_b + n_new - 1 of its OWN cache row and attends to the keys [0, past_b) of the
 * cache plus the new rows, causal over the new rows.  The kernel is mvlt_attn_cached's (one copy of the loop, a template
 * parameter): the walk over the key blocks, the online softmax and the 4-wave merge for bf16 are functions of the row's own key
 * count, so row b's output is bit for bit what mvlt_attn_cached gives for that row alone at past_b, and an all-zero table
 * reproduces mvlt_attn_cached bit for bit.
 * Cache slots of a row at and beyond past_b + n_new are never read: whatever a dense prefill left there is harmless.
 * past_b is clamped on the device into [0, cache_cap - n_new]: a bad table gives wrong attention, never an access outside the
 * row's cache (the convention of mvlt_attn_cached_beam).
 * MVLT_ERR_ARG: NULL pointers (row_shift included), n_new > cache_cap, and with a host `past`: past < 0 or past + n_new >
 * cache_cap.  MVLT_ERR_UNSUPPORTED: hd != 64, n_new > 4, operands not 16-byte aligned (there is no serial form).
 * An existing struct plus a pointer: the struct registry (MVLT_STRUCT_COUNT) and MVLT_ABI_VERSION stay as they are. */
int mvlt_attn_cached_rows(const MvltAttnCached* p, const int32_t* row_shift, void* stream);
/* The same step for beam search, with a cache that is NEVER reordered: the rows are the hypotheses of rows / num_beams samples
 * (rows g * num_beams .. + num_beams the beams of sample g) and a table says in which cache row each generated position of each
 * hypothesis lives.  Key position k of row r, g = r / num_beams:
 *   k < prefix            cache row g * num_beams            (the image prefix is stored once per sample, in its first row)
 *   prefix <= k < past    cache row g * num_beams + slot[r, k - prefix]
 *   k >= past             qkv_new of row r; also appended to row r's OWN cache row at position k, as mvlt_attn_cached does
 * Every (row, position) cell is written by one launch and only read by later ones.  Slot values are clamped into
 * [0, num_beams) and the column into [0, ld_slot): a bad table gives wrong attention, never a read outside the sample's rows.
 * The walk over the keys, the online softmax and the 4-wave merge for bf16 are mvlt_attn_cached's; only the row address of a key
 * differs, so with slot[r, :] = r % num_beams and the prefix present in every row the output is bit for bit mvlt_attn_cached's.
 * MVLT_ERR_ARG: NULL pointers, rows % num_beams != 0, prefix < 0, ld_slot < 1, and with a host `past`: past < prefix,
 * past + n_new > cache_cap, past - prefix > ld_slot (with past_dev the caller guarantees them).  MVLT_ERR_UNSUPPORTED:
 * hd != 64, n_new > 4, operands not 16-byte aligned (there is no serial form). */
typedef struct MvltAttnCachedBeam {
    int dtype, rows, nH, hd, past, n_new, cache_cap;
    const void* qkv_new;                /* [rows*n_new, 3*nH*hd] */
    void* k_cache; void* v_cache;       /* [rows, nH, cache_cap, hd] */
    void* out;                          /* [rows*n_new, nH*hd] */
    float scale;
    const int32_t* past_dev;            /* optional, as in MvltAttnCached */
    int num_beams, prefix;
    const int32_t* slot; int64_t ld_slot;       /* [rows, ld_slot] */
} MvltAttnCachedBeam;
int mvlt_attn_cached_beam(const MvltAttnCachedBeam* p, void* stream);
/* The hypothesis bookkeeping of one beam-search token on the device (csrc/beam.hip): HF transformers 4.16
 * BeamSearchScorer.process (decode.BeamScorer.process: length_penalty 1, early stopping off) and the three lines beam_search runs
 * behind it (model.py:722-763: beam scores / tokens / indices, the input_ids update, the beam reorder -- here of the slot table of
 * mvlt_attn_cached_beam, not of the cache).  One launch, a workgroup per sample; the walk over the candidates runs on one lane in
 * f64 (the host scorer works in Python floats on f32 inputs, and no comparison may differ by a rounding), the row copies on all
 * lanes; no float atomics.  rows = G * num_beams; c = *col, the number of tokens generated so far; L = max(1, c) (at step 0 the
 * host scorer is handed [[mask_id]]: a hypothesis that finishes there is the one-token list [mask_id]).
 * Inputs: the sorted candidate lists of mvlt_gemm_beam_candidates (cand_score f32, cand_beam, cand_tok, [G, n_cand]); src_beams =
 * the num_beams of the candidate call that made them (1 at step 0, where one row per sample was scored; cand_beam is clamped
 * into [0, src_beams)); the parent row of a candidate is g * num_beams + cand_beam.
 * State per sample, caller-allocated: the pool of finished hypotheses in insertion order -- hyp_score f64 [G, num_beams + 1],
 * hyp_len [G, num_beams + 1], hyp_tokens [G, num_beams + 1, max_length] (entries at and beyond a hypothesis' length are
 * unspecified) --, n_hyp [G], worst f64 [G] (the caller starts it at 1e9), done [G]; the live sequences seq [rows, max_length];
 * the slot table [rows, ld_slot >= max_length].  Counters: col (int64), past (int32, optional), ticket (int32, zeroed once by the
 * caller), alive int64 [max_length] (zeroed when a decode starts).
 * Sample g, when done[g] == 0: walk the candidates in rank order until num_beams are kept.  A candidate with token eos_id (has_eos
 * != 0 only) at rank < num_beams offers its parent's sequence (the first L tokens of seq[parent] as they were BEFORE this launch;
 * [mask_id] at c = 0) to the pool with score (double)cand_score / (double)L; at rank >= num_beams it is skipped.  The offer is
 * taken when n_hyp < num_beams or score > worst; the pool then grows, and beyond num_beams entries the one with the lowest (score,
 * insertion index) leaves (later entries move up) and worst = the second lowest score, else worst = min(score, worst).  Any other
 * candidate is kept as the next live beam k = 0, 1, ...:  beam_scores[g nb + k] = its score (bit for bit), new_ids[g nb + k] =
 * [token, mask_id] (int64 [rows, 2]), beam_idx[g nb + k] = its parent row (int32, global), seq[g nb + k] = seq[parent] with the
 * token at column c, slot[g nb + k] = slot[parent] with column c = k (the position the next forward appends lives in the row's own
 * cache row; that forward reads only columns below c, so writing the column before it equals writing it after).  Both
 * permutations are in place, staged through LDS.  Then done[g] |= n_hyp >= num_beams && worst >= (double)cand_score[g, 0] / L.
 * (At most num_beams of 2 num_beams distinct (beam, token) candidates carry EOS, so num_beams are always kept; with fewer
 * candidates the missing beams are filled with pad_id, score 0, parent 0.)
 * Sample g, when done[g] != 0: beam_scores 0, new_ids [pad_id, mask_id], beam_idx 0; its seq, slot rows and pool stay untouched.
 * Every launch: alive[c] is raised to 1 by every sample that is still not done; cand_log (optional, int32 [max_length, G, 3,
 * n_cand]) receives the consumed lists at index c (score bits, beam, token); the last workgroup to arrive advances *col and *past
 * by one and re-arms the ticket.  A launch that finds c outside [0, max_length) writes nothing and advances nothing.
 * Refusals (nothing launched, nothing written): MVLT_ERR_ARG for a NULL b or required pointer (all but past and cand_log), G < 1,
 * num_beams < 1, n_cand < num_beams, src_beams not in {1, num_beams}, max_length < 1, ld_slot < max_length; then
 * MVLT_ERR_UNSUPPORTED for num_beams > 8, n_cand > 16, num_beams * max_length > 8192 (the staging area in LDS). */
typedef struct MvltBeamStep {
    int32_t G, num_beams, n_cand, src_beams, max_length, has_eos;
    int64_t eos_id, pad_id, mask_id;
    const float* cand_score; const int32_t* cand_beam; const int32_t* cand_tok;        /* [G, n_cand] */
    double* hyp_score; int32_t* hyp_len; int32_t* hyp_tokens;                          /* the pool */
    int32_t* n_hyp; double* worst; int32_t* done;                                      /* [G] */
    int32_t* seq;                                                                      /* [rows, max_length] */
    int32_t* slot; int64_t ld_slot;                                                    /* [rows, ld_slot] */
    int64_t* col; int32_t* past; int32_t* ticket; int64_t* alive;
    float* beam_scores; int64_t* new_ids; int32_t* beam_idx;                           /* outputs: [rows], [rows, 2], [rows] */
    int32_t* cand_log;                                                                 /* optional */
} MvltBeamStep;
int mvlt_beam_step(const MvltBeamStep* b, void* stream);
/* argmax over V of logits [rows, ld] -> int64 ids (greedy_search, model.py:896-900) */
int mvlt_argmax(int dtype, const void* logits, int64_t ld, int rows, int V, int64_t* out, void* stream);

/* zero up to 32 small f32 buffers in ONE launch (the relative-position-bias gradients of all Swin blocks are
 * accumulated with atomics and must start from zero; items is a HOST array) */
typedef struct MvltZeroItem { float* ptr; int64_t n; } MvltZeroItem;
int mvlt_zero_batch(const MvltZeroItem* items, int n, void* stream);

/* Pull up to 8 read-only byte ranges (the weight matrices of the layer about to run) towards the GPU's caches: one
 * dword of every 128-byte line is read and dropped.  The optimizer's sweep over 6 GB of state evicts every weight from
 * the 256 MB Infinity Cache once per step, so each nn.Linear of the reference (model.py / visual_feature_extractor.py
 * forward passes) would otherwise stream its weight panels from HBM at one miss latency per k-tile.  items is a HOST
 * array; nothing is written. */
typedef struct MvltRange { const void* ptr; int64_t bytes; } MvltRange;
int mvlt_prefetch(const MvltRange* items, int n, void* stream);

/* ------------------------------------------------------------------ input pipeline
 * The reference prepares every sample on the host (run_pretrain_rgc_roco_medicat.py:94-212); these two entry
 * points move the per-step arithmetic of that code to the GPU for pre-resized / pre-tokenised shards.
 *
 * Image normalisation (:107-110, :127-130): HWC uint8 RGB [B,H,W,3] -> CHW f32 [B,3,H,W] with, per image and
 * channel, (x - mean_c) / var_c -- the reference divides by np.var (population VARIANCE, not the standard
 * deviation); a constant channel gives 0/0 = NaN exactly as numpy does.  Sums are exact integers. */
int mvlt_image_normalize(const uint8_t* hwc, float* chw, int B, int H, int W, void* stream);
/* MLM masking, _random_mask_word (:188-212) + the truncation of :170-176, on already truncated id rows:
 * n = min(10, max(1, round(0.2 * full_len[b]))) distinct token positions drawn uniformly from [0, full_len[b]);
 * each: 80 % -> mask_id, 10 % -> uniform random id in [0, vocab_size), 10 % unchanged; label = original id.
 * Position i of the untruncated caption lives at column i (i < T-1 or full_len <= T), the last token ([END]) at
 * column T-1 when full_len > T; other positions were cut off and their masks are dropped, like the reference.
 * Rows with itm_label[b] == 0 are left unmasked (:160-164).  Counter RNG (seed, row, position): statistically
 * equivalent to the reference's Python `random`, not bit-identical.  ids_in/ids_out/labels: int64 [B,T]. */
typedef struct MvltMlmMask {
    int B, T, vocab_size, mask_id;
    const int64_t* ids_in; const int32_t* full_len; const int64_t* itm_label;   /* itm_label may be NULL */
    int64_t* ids_out; int64_t* labels;
    uint64_t seed;
} MvltMlmMask;
int mvlt_mlm_mask(const MvltMlmMask* p, void* stream);

/* Fused fine-tuning image transform: Pillow-exact resize evaluated at the pixels of an O x O crop only, optional horizontal
 * flip, and ToTensor + Normalize as a table lookup -- the torchvision pipelines of run_report_generation_cxr.py:24-36 and
 * run_retrieval_iuxray.py:52-65 and the PIL resize of run_pretrain_rgc_roco_medicat.py:103-106, one launch per batch of B
 * ragged uint8 HWC RGB sources.  Image b is the hw[2b] x hw[2b+1] x 3 bytes at src + src_off[b].  Per image and axis
 * (0 = horizontal, 1 = vertical) and per output index t < O the host supplies Pillow's tap table: bounds [B,2,O,2] =
 * (first source index, tap count in 1 .. kmax) and coef [B,2,O,kmax] (22-bit fixed point; taps past the count MUST be 0), already restricted to
 * the crop's columns and rows.  With X = flip[b] ? O-1-x : x:
 *     H[r][X]   = clip8((2^21 + sum_i coef[b][0][X][i] * src_b[r][first_X + i]) >> 22)       (rounded to uint8, as Pillow does)
 *     v[y][x]   = clip8((2^21 + sum_j coef[b][1][y][j] * H[first_y + j][X]) >> 22)
 *     MVLT_IMGXF_F32_CHW: out f32 [B,3,O,O] = lut[c][v]     (lut f32 [3,256], e.g. (k/255 - mean_c) / std_c built by the caller)
 *     MVLT_IMGXF_U8_HWC:  out uint8 [B,O,O,3] = v           (lut unused, may be NULL)
 * Integer arithmetic throughout: the result is bit-identical to Pillow's Image.resize + crop + flip (and to torch's own
 * arithmetic through the table).  All pointers are device memory.  The kernel TRUSTS the tables: first + count must not pass the
 * source axis and count must not pass kmax -- the caller checks that before it uploads them (data.py: plan_image_transform).
 * The arguments are scalars, not a struct: the struct registry (MVLT_STRUCT_COUNT) and MVLT_ABI_VERSION stay as they are.
 * MVLT_ERR_ARG (nothing launched): a NULL pointer (lut only for MVLT_IMGXF_F32_CHW), B outside 1 .. 65535, kmax outside
 * 1 .. 65, out_size outside 8 .. 224 or not a multiple of 8, an unknown mode, out not 16-byte aligned. */
enum { MVLT_IMGXF_F32_CHW = 0, MVLT_IMGXF_U8_HWC = 1 };
int mvlt_image_transform(const uint8_t* src, const int64_t* src_off, const int32_t* hw, const int32_t* bounds, const int32_t* coef,
                         const uint8_t* flip, const float* lut, void* out, int B, int out_size, int kmax, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVLT_HIP_H */
