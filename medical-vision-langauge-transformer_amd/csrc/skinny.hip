// Everything the decode path runs at M <= 64 (see include/mvlt_hip.h): the skinny product behind mvlt_gemm, its K-split form
// (mvlt_gemm_skinny_accum), and the MLM head fused with the pick of the next token -- greedy (mvlt_gemm_argmax,
// mvlt_gemm_argmax_greedy), sampled (mvlt_gemm_sample, mvlt_gemm_sample_step), sampled behind a top-k / top-p filter
// (mvlt_gemm_sample_filtered, mvlt_gemm_sample_filtered_step) and greedy or sampled per row over any number of rows
// (mvlt_gemm_pick_rows, mvlt_gemm_pick_rows_step) -- and the candidate step of beam search
// (mvlt_gemm_beam_candidates: log-softmax + beam score + top-n per sample).  The six picks also come with the logit rules of
// constrained decoding in their epilogues (mvlt_gemm_*_rules, fed by mvlt_decode_rules_plan); the beam candidates apply them to the
// log-probabilities in their selection (mvlt_gemm_beam_candidates_rules, fed by mvlt_beam_rules_plan).  No LDS staging in the
// products: the weight matrix is read once and nothing is reused inside a workgroup, so every wave loads its MFMA fragments
// straight from global memory.
// Same argument block as the tile kernels of gemm.hip (gemm_dev.h); gemm.hip reaches the plain product through mvlt_skinny_try.
#include "common.h"
#include "gemm_dev.h"
#include "gemm_host.h"

namespace {

// (value, index) picks: the candidate (ov, oi) replaces the best so far (v, i) when it is larger, or equal with a LOWER index -- the
// first index of the maximum is what the greedy tests pin, and this is the one place the rule is written.  A macro, not a
// function: hipcc schedules every kernel below differently as soon as the comparison sits behind a call, inlined or not
// (profiles/skinny_split_isa.md).
#define BEATS(ov, oi, v, i) ((ov) > (v) || ((ov) == (v) && (oi) < (i)))

// Skinny products (M <= 64: the 2-token decode step, poolers, classifier heads): the weight matrix is read once
// and nothing is reused inside a workgroup, so there is no LDS staging -- every wave loads its MFMA fragments
// straight from global memory (16 B per lane, k-contiguous rows).  Workgroup = 16 output columns x all rows;
// its 8 waves split K (3 k-blocks in flight per wave: the loop is latency bound, so memory-level parallelism is
// what matters), partial accumulators meet in LDS, wave i < 4 finishes row tile i.
constexpr int SKINNY_WAVES = 8, SKINNY_UNROLL = 3;
// ARGMAX (greedy decoding, model.py:896-900): instead of storing the logits, every workgroup reduces its 16
// columns to (max, first index of the max) per row -> part_val/part_idx [M][gridDim.x]; argmax_parts_kernel
// finishes the rows.  The maximum is taken over the f32 accumulators (+ bias).
struct ArgmaxOut { float* part_val; int* part_idx; };
// Weight fragments of the skinny products: every workgroup reads ITS 16 (or 128) weight rows exactly once, and in decoding the
// 217 MB of weights + ~150 MB of K / V rows per step cycle through a 256 MB Infinity Cache -- non-temporal loads
// (MI355X_MICROARCH.md "nt-weights": once-read streamed weights, 5-10 % per decode layer).  -DMVLT_SKINNY_NT=0 restores the
// default cache policy (A/B builds).
#ifndef MVLT_SKINNY_NT
#define MVLT_SKINNY_NT 1
#endif
template <typename F> MVLT_DEV F skinny_wload(const F* q) {
#if MVLT_SKINNY_NT
    return __builtin_nontemporal_load(q);
#else
    return *q;
#endif
}
template <typename T, bool ARGMAX = false>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_skinny_kernel(const GemmDev p_in, const ArgmaxOut am) {
    const GemmDev p = effective<false>(p_in);          // ragged row counts (m_dev): rows beyond it are neither read nor written
    if (p.M <= 0) return;
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E;
    __shared__ f32x4 red[SKINNY_WAVES][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r15 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    const T* brow = B + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the finishing waves fetch their bias / residual values now, so the epilogue does not start with a
    // dependent memory round trip (the decode step is a chain of ~100 such kernels)
    constexpr int FASTMASK = MVLT_EPI_BIAS | MVLT_EPI_GELU | MVLT_EPI_RESIDUAL;
    const bool fast_epi = !ARGMAX && (p.epi & ~FASTMASK) == 0 && p.epi_vec && n0 + 16 <= p.N && wave < 4 && 16 * wave + r15 < p.M;
    f32x4 pre_bias{0.f, 0.f, 0.f, 0.f}, pre_res{0.f, 0.f, 0.f, 0.f};
    if (fast_epi) {
        if (p.epi & MVLT_EPI_BIAS) pre_bias = *reinterpret_cast<const f32x4*>(p.bias + n0 + 4 * g);
        if (p.epi & MVLT_EPI_RESIDUAL)
            pre_res = load4f(reinterpret_cast<const T*>(p.residual) + (long)(16 * wave + r15) * p.ldr + n0 + 4 * g);
    }
    const int nkb = p.K / KB;
    for (int kb0 = wave; kb0 < nkb; kb0 += SKINNY_WAVES * SKINNY_UNROLL) {
        Frag fb[SKINNY_UNROLL], fa[SKINNY_UNROLL][4];
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) {
            const int kb = kb0 + u * SKINNY_WAVES;
            const int k = (kb < nkb ? kb : kb0) * KB;          // past the end: reload a valid block, never multiplied
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) {
            if (kb0 + u * SKINNY_WAVES < nkb) {
#pragma unroll
                for (int i = 0; i < 4; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    const int i = wave;                                  // row tile finished by this wave
    if (i < 4 && 16 * i < p.M) {
        f32x4 v = red[0][i][lane];
#pragma unroll
        for (int w = 1; w < SKINNY_WAVES; ++w) v += red[w][i][lane];
        // acc[r] <-> n = n0 + 4*g + r, m = 16*i + (lane & 15)   (same orientation as gemm_body)
        if (!ARGMAX) {
            if (fast_epi) {
                f32x4 o = v + pre_bias;
                if (p.epi & MVLT_EPI_GELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = gelu_f(o[r]);
                }
                o += pre_res;
                store4f(reinterpret_cast<T*>(p.C) + (long)(16 * i + r15) * p.ldc + n0 + 4 * g, o);
            } else {
                epilogue4<T>(p, 16 * i + r15, n0 + 4 * g, v);
            }
        } else {
            float best = -3.0e38f; int bi = 0x7fffffff;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * g + r;
                if (n < p.N) {
                    const float x = v[r] + ((p.epi & MVLT_EPI_BIAS) ? p.bias[n] : 0.f);
                    if (x > best) { best = x; bi = n; }          // ascending n: ties keep the first index
                }
            }
#pragma unroll
            for (int o = 16; o < 64; o <<= 1) {
                const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
                if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; }
            }
            const int m = 16 * i + r15;
            if (g == 0 && m < p.M) { am.part_val[(long)m * gridDim.x + blockIdx.x] = best; am.part_idx[(long)m * gridDim.x + blockIdx.x] = bi; }
        }
    }
}

// Skinny product with K split over workgroups (decode: M = 2B rows, N = 768, K = 768 / 3072).  The plain skinny kernel
// gives every 16-column workgroup the WHOLE activation matrix to read (N/16 x M x K bytes through L2: 48 x 393 KB for
// the FFN-out product, 10 us per workgroup at the ~50 GB/s a CU takes in); here workgroup (j, s) reads only k-slice s
// of it and writes its partial 64x16 tile into the slab of its slice.  No epilogue: the consumer
// (mvlt_layernorm_acc_fwd: sum of the slices + bias + residual, LayerNorm) is the launch that follows anyway.
template <typename T>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_skinny_accum_kernel(const GemmDev p, float* accout) {
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E;
    __shared__ f32x4 red[SKINNY_WAVES][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r15 = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    const T* brow = B + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.K / KB;
    const int per = (nkb + (int)gridDim.y - 1) / (int)gridDim.y;
    const int kb_lo = blockIdx.y * per, kb_hi = min(nkb, kb_lo + per);
    for (int kb0 = kb_lo + wave; kb0 < kb_hi; kb0 += SKINNY_WAVES * SKINNY_UNROLL) {
        Frag fb[SKINNY_UNROLL], fa[SKINNY_UNROLL][4];
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) {
            const int kb = kb0 + u * SKINNY_WAVES;
            const int k = (kb < kb_hi ? kb : kb0) * KB;
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < 4; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < SKINNY_UNROLL; ++u) {
            if (kb0 + u * SKINNY_WAVES < kb_hi) {
#pragma unroll
                for (int i = 0; i < 4; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = acc[i];
    __syncthreads();
    const int i = wave;
    if (i < 4 && 16 * i + r15 < p.M) {
        f32x4 v = red[0][i][lane];
#pragma unroll
        for (int w = 1; w < SKINNY_WAVES; ++w) v += red[w][i][lane];
        // slab of this k-slice: [gridDim.y][M][N] f32, written once with plain stores; the consumer (ln_acc_fwd_kernel) adds the
        // slices in slice order -- no float atomics, no zeroing pass, bit-reproducible (round 5; the atomic form cost ~1 us more)
        float* c = accout + ((long)blockIdx.y * p.M + 16 * i + r15) * p.N + n0 + 4 * g;
        if (n0 + 4 * g + 4 <= p.N) store4f(c, v);
        else
#pragma unroll
            for (int r = 0; r < 4; ++r) if (n0 + 4 * g + r < p.N) c[r] = v[r];
    }
}

// one wave per row: (max, first index) over the workgroup partials
__global__ __launch_bounds__(64) void argmax_parts_kernel(const float* part_val, const int* part_idx, int nparts,
                                                          int64_t* out_idx, float* out_val) {
    const long base = (long)blockIdx.x * nparts;
    float best = -3.0e38f; int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < nparts; i += 64) {
        const float v = part_val[base + i]; const int idx = part_idx[base + i];
        if (BEATS(v, idx, best, bi)) { best = v; bi = idx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (threadIdx.x == 0) { out_idx[blockIdx.x] = bi; if (out_val) out_val[blockIdx.x] = best; }
}

// LOGIT RULES (mvlt_hip.h MvltLogitRules: repetition penalty, no-repeat n-grams, min length).  Two bitmaps per row, `seen` and
// `banned`, one bit per vocabulary column; decode_rules_plan_kernel rebuilds them from the generated history before every pick and
// the three wide head kernels read them in their epilogues.  A head kernel is rule-aware when it is instantiated with a trailing
// RulesDev argument (the pack R): the instantiations without one have the argument list, and the code, they had before the rules
// existed (two main-loop copies are scheduled differently as soon as anything around them moves: profiles/skinny_split_isa.md,
// profiles/decode_rules.md holds the register table of both forms).
struct RulesDev { const uint32_t* seen; const uint32_t* banned; long ld_words; float penalty; };
MVLT_DEV const RulesDev& rules_arg(const RulesDev& r) { return r; }
// A lane's four columns n0 + 4 g + r are 4-aligned and n0 is a multiple of 16, so they sit in ONE 32-bit word of a row's map, the
// word of n0 (n0 < N: inside the row): bits (seen | banned << 4) of the four columns of row m, bit r = column n0 + 4 g + r.
// Rows past M read row M - 1 (their result is dropped).
MVLT_DEV uint32_t rules_bits(const RulesDev& rd, const int m, const int M, const int n) {
    const long w = (long)min(m, M - 1) * rd.ld_words + (n >> 5);
    const int sh = n & 31;
    return ((rd.seen[w] >> sh) & 15u) | (((rd.banned[w] >> sh) & 15u) << 4);
}
// HF's repetition penalty on a seen column, two rounded operations
MVLT_DEV float rules_penalise(const float x, const float penalty) { return x < 0.f ? __fmul_rn(x, penalty) : __fdiv_rn(x, penalty); }

// The plan: one workgroup per row m rebuilds seen[m] and banned[m] from h = ids[m, 0 .. c-1], c = *col read on the device like
// the pick kernels read it.  Stateless: both maps are cleared and set again every call (global atomicOr; a workgroup touches only
// its own row), so a replayed graph carries nothing from token to token.  The n-gram rule is a scan over the start i of every
// earlier g-gram, one thread per i: h[i .. i+g-2] == the last g-1 tokens bans h[i+g-1].  ids outside [0, V) set no bit.
// The body is one template over the history's integer type: int64 ids of the greedy loops, int32 live sequences of beam search
// (mvlt_beam_rules_plan: row m = one hypothesis, h = MvltBeamStep.seq[m, 0 .. c-1], any number of rows).
template <typename I>
MVLT_DEV void rules_plan_row(uint32_t* seen, uint32_t* banned, const I* h, const long ld, const int64_t* col, const int g, const int min_length,
                             const int64_t eos, const int has_eos, const int V) {
    const int tid = threadIdx.x, nw = (V + 31) >> 5;
    const long c64 = col[0];
    const int c = (int)(c64 < 0 ? 0 : (c64 > ld ? ld : c64));          // never past the row of ids
    for (int w = tid; w < nw; w += 256) { seen[w] = 0u; banned[w] = 0u; }
    __syncthreads();
    for (int i = tid; i < c; i += 256) {
        const I t = h[i];
        if (t >= 0 && t < V) atomicOr(seen + (t >> 5), 1u << (t & 31));
        if (g >= 1 && i + g <= c) {          // the g-gram starting at i ends before column c
            bool same = true;
            for (int j = 0; j < g - 1; ++j) same = same && h[i + j] == h[c - g + 1 + j];
            const I b = h[i + g - 1];
            if (same && b >= 0 && b < V) atomicOr(banned + (b >> 5), 1u << (b & 31));
        }
    }
    if (tid == 0 && has_eos && c64 < min_length && eos >= 0 && eos < V) atomicOr(banned + (eos >> 5), 1u << (eos & 31));
}
struct RulesPlan {
    uint32_t* seen; uint32_t* banned; long ld_words; const int64_t* ids; long ld_ids; const int64_t* col;
    int ngram, min_length; int64_t eos; int has_eos, V;
};
__global__ __launch_bounds__(256) void decode_rules_plan_kernel(const RulesPlan f) {
    const int m = blockIdx.x;
    rules_plan_row(f.seen + (long)m * f.ld_words, f.banned + (long)m * f.ld_words, f.ids + (long)m * f.ld_ids, f.ld_ids, f.col, f.ngram,
                   f.min_length, f.eos, f.has_eos, f.V);
}
struct BeamRulesPlan {
    uint32_t* seen; uint32_t* banned; long ld_words; const int32_t* seq; long ld_seq; const int64_t* col;
    int ngram, min_length; int64_t eos; int has_eos, V;
};
__global__ __launch_bounds__(256) void beam_rules_plan_kernel(const BeamRulesPlan f) {
    const int m = blockIdx.x;
    rules_plan_row(f.seen + (long)m * f.ld_words, f.banned + (long)m * f.ld_words, f.seq + (long)m * f.ld_seq, f.ld_seq, f.col, f.ngram,
                   f.min_length, f.eos, f.has_eos, f.V);
}

// Decoder GEMM of the last-row MLM head fused with the greedy pick, wide form (round 5): a workgroup = 128 vocabulary columns,
// wave w = columns 16 w .. +16 over the WHOLE reduction -- no k-split across waves, so no LDS reduction and no barrier; the
// 47 MB weight matrix is streamed once by 239 workgroups (one per CU) with UNR k-blocks in flight per wave, the 32-64
// activation rows come from L1 / L2.  The 16-column form above launches 1,908 workgroups that each re-read the whole
// activation matrix and meet in LDS: 29 us for a product whose bytes take 9 us.  Same partial layout (one (max, index) per row
// and 16 columns), so the finishing kernel is shared.
template <typename T, int NRT, typename... R>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_argmax128_kernel(const GemmDev p, const ArgmaxOut am, int nparts, const R... rules) {
    constexpr bool RULES = sizeof...(R) > 0;
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E, UNR = NRT <= 2 ? 12 : 8;          // k-blocks in flight per wave (12 KB of weights; K = 768 in two rounds)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r15 = lane & 15, g = lane >> 4;
    const int n0 = (blockIdx.x * SKINNY_WAVES + wave) * 16;
    if (n0 >= p.N) return;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* brow = reinterpret_cast<const T*>(p.B) + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.K / KB;
    for (int kb0 = 0; kb0 < nkb; kb0 += UNR) {
        Frag fb[UNR], fa[UNR][NRT];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int k = min(kb0 + u, nkb - 1) * KB;          // past the end: reload the last block, never multiplied
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < NRT; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (kb0 + u < nkb) {
#pragma unroll
                for (int i = 0; i < NRT; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
    // acc[i][r] <-> n = n0 + 4 g + r, m = 16 i + r15
    f32x4 bias4{0.f, 0.f, 0.f, 0.f};
    if (p.epi & MVLT_EPI_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = p.bias[min(n0 + 4 * g + r, p.N - 1)];
    }
    const int part = blockIdx.x * SKINNY_WAVES + wave;
#pragma unroll
    for (int i = 0; i < NRT; ++i) {
        float best = -3.0e38f; int bi = 0x7fffffff;
        uint32_t bits = 0u;          // RULES: seen (bits 0-3) and banned (bits 4-7) of this lane's four columns
        if constexpr (RULES) bits = rules_bits(rules_arg(rules...), 16 * i + r15, p.M, n0 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * g + r;
            float x = acc[i][r] + bias4[r];
            if constexpr (RULES) {
                if ((bits >> r) & 1u) x = rules_penalise(x, rules_arg(rules...).penalty);
                if ((bits >> (4 + r)) & 1u) continue;          // a banned column is skipped like a column n >= N
            }
            if (n < p.N && x > best) { best = x; bi = n; }          // ascending n: ties keep the first index
        }
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; }
        }
        const int m = 16 * i + r15;
        if (g == 0 && m < p.M) { am.part_val[(long)m * nparts + part] = best; am.part_idx[(long)m * nparts + part] = bi; }
    }
}

// Finish of the greedy pick for ALL rows in one workgroup, with the per-token bookkeeping of greedy_search (model.py:896-913)
// folded in: next = argmax; finished samples emit PAD; unfinished &= (next != EOS); ids[:, col] = next; scores[:, col] = max
// logit; new_ids[:, 0] = next (the first of the two tokens the next cached step feeds); alive[col] = any sample unfinished;
// past += 1 (the cache position the NEXT forward reads: the previous step's [MASK] slot is overwritten); col += 1.
// Replaces argmax_parts_kernel + ten one-line torch kernels per replayed decode step.  M <= 64; 16 waves, wave w = rows w, w + 16, ...
struct GreedyState {
    int64_t* unfinished; int64_t eos, pad; int has_eos;
    int64_t* col; int32_t* past;
    int64_t* ids; long ld_ids; float* scores; long ld_scores; int64_t* alive; int64_t* new_ids; long ld_new;
    int32_t* ticket;
};
// The per-token bookkeeping both pick kernels end with (one thread per row): `tok` is the row's pick, `score` what goes into
// scores[:, col] -- of the PICKED token also for a finished row (the reference gathers the score before PAD replaces the token).
MVLT_DEV void pick_bookkeeping(const GreedyState& st, const int m, const int M, const long col, const int tok, const float score) {
    int64_t nxt = tok;
    if (st.has_eos) {
        const int64_t unf = st.unfinished[m];
        nxt = nxt * unf + st.pad * (1 - unf);
        const int64_t unf2 = unf * (nxt != st.eos ? 1 : 0);
        st.unfinished[m] = unf2;
        if (unf2) atomicMax(reinterpret_cast<unsigned long long*>(st.alive + col), 1ULL);
    }
    st.ids[(long)m * st.ld_ids + col] = nxt;
    st.scores[(long)m * st.ld_scores + col] = score;
    st.new_ids[(long)m * st.ld_new] = nxt;
    __threadfence();
    if (atomicAdd(st.ticket, 1) == M - 1) {
        *st.ticket = 0;
        st.col[0] = col + 1;
        if (st.past) st.past[0] += 1;
    }
}
// One workgroup per row (256 threads: ~8 partials per thread, one memory round trip; a single workgroup walking all rows took
// 26 us).  alive[col] is raised with an atomic max by the rows that are still unfinished (the caller zeroes `alive` when a
// decode starts); the LAST workgroup to arrive (ticket) advances col and past and re-arms the ticket.  Every workgroup reads
// col before it draws its ticket, and col is written only after all tickets are drawn.
__global__ __launch_bounds__(256) void greedy_pick_kernel(const float* part_val, const int* part_idx, int nparts, int M, const GreedyState st) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    const long col = st.col[0];
    const long base = (long)m * nparts;
    float best = -3.0e38f; int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float v = part_val[base + i]; const int idx = part_idx[base + i];
        if (BEATS(v, idx, best, bi)) { best = v; bi = idx; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = s_val[w]; const int oi = s_idx[w];
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; }
        }
        pick_bookkeeping(st, m, M, col, bi, best);
    }
}

// SAMPLED pick (greedy_search 'sample' mode, model.py:901-906): multinomial(softmax(x)) is argmax_n (x_n + G_n) with i.i.d.
// standard Gumbel noise G (Gumbel-max), so the sampled step is the greedy product with a noise term in the epilogue and an online
// log-sum-exp beside the running maximum (the score is the log-probability of the drawn token).  Sibling of
// gemm_argmax128_kernel: the same main loop (two copies: behind a shared helper hipcc schedules both differently, profiles/skinny_split_isa.md); epilogue
// per element (m, n), all in f32, no fused multiply-add:
//     x = (acc + bias[n]) * inv_temperature;   y = x + gumbel_noise(seed, tag0 + step, m N + n)      (common.h)
// seed = *seed_dev and step = *col are read from device memory (one captured graph serves every call and every token).
// Per row and 16-column part it writes five values, part_val[j][m][part]: j = 0 max y, 1 x at that index, 2 max x,
// 3 sum exp(x - max x); part_idx[m][part] = first index of max y.  Columns n >= N take part in neither.
struct SampleIn { const uint64_t* seed_dev; uint64_t seed; const int64_t* col; uint32_t tag0; float inv_t; };
template <typename T, int NRT, typename... R>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_sample128_kernel(const GemmDev p, float* part_val, int* part_idx, int nparts, const SampleIn si,
                                                                           const R... rules) {
    constexpr bool RULES = sizeof...(R) > 0;
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E, UNR = NRT <= 2 ? 12 : 8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r15 = lane & 15, g = lane >> 4;
    const int n0 = (blockIdx.x * SKINNY_WAVES + wave) * 16;
    if (n0 >= p.N) return;
    const uint64_t seed = si.seed_dev ? si.seed_dev[0] : si.seed;
    const uint32_t tag = si.tag0 + (si.col ? (uint32_t)si.col[0] : 0u);
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* brow = reinterpret_cast<const T*>(p.B) + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.K / KB;
    for (int kb0 = 0; kb0 < nkb; kb0 += UNR) {
        Frag fb[UNR], fa[UNR][NRT];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int k = min(kb0 + u, nkb - 1) * KB;          // past the end: reload the last block, never multiplied
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < NRT; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (kb0 + u < nkb) {
#pragma unroll
                for (int i = 0; i < NRT; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
    // acc[i][r] <-> n = n0 + 4 g + r, m = 16 i + r15
    f32x4 bias4{0.f, 0.f, 0.f, 0.f};
    if (p.epi & MVLT_EPI_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = p.bias[min(n0 + 4 * g + r, p.N - 1)];
    }
    const int part = blockIdx.x * SKINNY_WAVES + wave;
    const long plane = (long)p.M * nparts;
#pragma unroll
    for (int i = 0; i < NRT; ++i) {
        const int m = 16 * i + r15;
        float x[4];
        float best = -3.0e38f, bx = 0.f, xm = -3.0e38f; int bi = 0x7fffffff;
        uint32_t bits = 0u;          // RULES: seen (bits 0-3) and banned (bits 4-7) of this lane's four columns
        if constexpr (RULES) bits = rules_bits(rules_arg(rules...), m, p.M, n0 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * g + r;
            if constexpr (RULES) {          // the rules act on the raw logit, ahead of the temperature
                float raw = __fadd_rn(acc[i][r], bias4[r]);
                if ((bits >> r) & 1u) raw = rules_penalise(raw, rules_arg(rules...).penalty);
                x[r] = __fmul_rn(raw, si.inv_t);
            } else {
                x[r] = __fmul_rn(__fadd_rn(acc[i][r], bias4[r]), si.inv_t);
            }
            const float y = __fadd_rn(x[r], gumbel_noise(seed, tag, (uint32_t)m * (uint32_t)p.N + (uint32_t)n));
            if (n < p.N && !(RULES && ((bits >> (4 + r)) & 1u))) {
                if (y > best) { best = y; bi = n; bx = x[r]; }          // ascending n: ties keep the first index
                xm = fmaxf(xm, x[r]);
            }
        }
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float ov = __shfl_xor(best, o, 64), ox = __shfl_xor(bx, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = ox; }
            xm = fmaxf(xm, __shfl_xor(xm, o, 64));
        }
        // (n0 < N: every part has a valid column, so xm is a logit; __expf of a non-positive argument: v_exp_f32 of x log2 e)
        // RULES: a part whose 16 columns are all banned keeps xm = -3e38 and a zero sum, and the finish weighs it with exp(-3e38 - max) = 0
        float se = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) se += (n0 + 4 * g + r < p.N && !(RULES && ((bits >> (4 + r)) & 1u))) ? __expf(x[r] - xm) : 0.f;
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        if (g == 0 && m < p.M) {
            const long o = (long)m * nparts + part;
            part_val[o] = best; part_val[plane + o] = bx; part_val[2 * plane + o] = xm; part_val[3 * plane + o] = se;
            part_idx[o] = bi;
        }
    }
}

// Finish of the sampled pick, one workgroup per row like greedy_pick_kernel: the parts reduce to the token (first index of the
// largest y), lse = M + log(sum_parts s_p exp(m_p - M)) with M the row's largest logit, score = x_token - lse (logf: <= 2 ulp).
// STEP: then the bookkeeping of greedy_pick_kernel; else the stand-alone outputs out_idx / out_logprob.
template <bool STEP>
__global__ __launch_bounds__(256) void sample_pick_kernel(const float* part_val, const int* part_idx, int nparts, int M, const GreedyState st,
                                                          int64_t* out_idx, float* out_logprob) {
    __shared__ float s_val[4], s_x[4], s_max[4], s_sum[4];
    __shared__ int s_idx[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = blockIdx.x;
    const long col = STEP ? st.col[0] : 0;
    const long base = (long)m * nparts, plane = (long)M * nparts;
    float best = -3.0e38f, bx = 0.f, xm = -3.0e38f; int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float v = part_val[base + i]; const int idx = part_idx[base + i];
        if (BEATS(v, idx, best, bi)) { best = v; bi = idx; bx = part_val[plane + base + i]; }
        xm = fmaxf(xm, part_val[2 * plane + base + i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64), ox = __shfl_xor(bx, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = ox; }
        xm = fmaxf(xm, __shfl_xor(xm, o, 64));
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; s_x[wave] = bx; s_max[wave] = xm; }
    __syncthreads();
    xm = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    float se = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) se += part_val[3 * plane + base + i] * __expf(part_val[2 * plane + base + i] - xm);
    se = wave_sum(se);
    if (lane == 0) s_sum[wave] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = s_val[w]; const int oi = s_idx[w];
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = s_x[w]; }
        }
        const float lse = __fadd_rn(xm, logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])));
        const float score = __fadd_rn(bx, -lse);
        if (STEP) pick_bookkeeping(st, m, M, col, bi, score);
        else { out_idx[m] = bi; out_logprob[m] = score; }
    }
}

// PER-ROW pick (mvlt_gemm_pick_rows / _step: K sampled reports per image next to a greedy row, any number of rows).  A SIBLING of
// gemm_sample128_kernel (a fourth copy of the main loop, for the reason given there; gemm_sample128_kernel itself is untouched):
// the same loads and MFMAs in the same order, and per element (m, n) of the launch, all in f32 with no fused multiply-add,
//     x = (acc + bias[n]) * inv_t[row0 + m];   y = noise_row[row0 + m] >= 0 ? x + gumbel_noise(seed, tag, noise_row * N + n) : x
// so a greedy row is the sampled pick without its noise term and every row has one definition of token (first index of the
// largest y) and score (x_token - logsumexp x).  A launch covers the <= 64 rows row0 .. row0 + p.M of a call over `rows` rows
// (p.A and the rule bitmaps already point at row row0); the two tables and the parts are indexed by the row of the CALL:
// part_val[j][rows][nparts] in the layout sample_pick_kernel finishes, one workgroup per row for any number of rows.  Rows of a
// partial tile read the tables at the launch's last row, like they read A; the noise index wraps in uint32.
struct PickRows { const int32_t* noise_row; const float* inv_t; int row0, rows; };
template <typename T, int NRT, typename... R>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_pick_rows128_kernel(const GemmDev p, float* part_val, int* part_idx, int nparts, const SampleIn si,
                                                                              const PickRows pr, const R... rules) {
    constexpr bool RULES = sizeof...(R) > 0;
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E, UNR = NRT <= 2 ? 12 : 8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r15 = lane & 15, g = lane >> 4;
    const int n0 = (blockIdx.x * SKINNY_WAVES + wave) * 16;
    if (n0 >= p.N) return;
    const uint64_t seed = si.seed_dev ? si.seed_dev[0] : si.seed;
    const uint32_t tag = si.tag0 + (si.col ? (uint32_t)si.col[0] : 0u);
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* brow = reinterpret_cast<const T*>(p.B) + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.K / KB;
    for (int kb0 = 0; kb0 < nkb; kb0 += UNR) {
        Frag fb[UNR], fa[UNR][NRT];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int k = min(kb0 + u, nkb - 1) * KB;          // past the end: reload the last block, never multiplied
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < NRT; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (kb0 + u < nkb) {
#pragma unroll
                for (int i = 0; i < NRT; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
    // acc[i][r] <-> n = n0 + 4 g + r, m = 16 i + r15
    f32x4 bias4{0.f, 0.f, 0.f, 0.f};
    if (p.epi & MVLT_EPI_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = p.bias[min(n0 + 4 * g + r, p.N - 1)];
    }
    const int part = blockIdx.x * SKINNY_WAVES + wave;
    const long plane = (long)pr.rows * nparts;
#pragma unroll
    for (int i = 0; i < NRT; ++i) {
        const int m = 16 * i + r15;
        const int mt = pr.row0 + min(m, p.M - 1);          // the table row, clamped like the A row: < pr.rows
        const int nr = pr.noise_row[mt];
        const float inv_t = pr.inv_t[mt];
        const uint32_t idx0 = (uint32_t)nr * (uint32_t)p.N;
        float x[4];
        float best = -3.0e38f, bx = 0.f, xm = -3.0e38f; int bi = 0x7fffffff;
        uint32_t bits = 0u;          // RULES: seen (bits 0-3) and banned (bits 4-7) of this lane's four columns
        if constexpr (RULES) bits = rules_bits(rules_arg(rules...), m, p.M, n0 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * g + r;
            if constexpr (RULES) {          // the rules act on the raw logit, ahead of the temperature
                float raw = __fadd_rn(acc[i][r], bias4[r]);
                if ((bits >> r) & 1u) raw = rules_penalise(raw, rules_arg(rules...).penalty);
                x[r] = __fmul_rn(raw, inv_t);
            } else {
                x[r] = __fmul_rn(__fadd_rn(acc[i][r], bias4[r]), inv_t);
            }
            float y = x[r];          // a greedy row: y = x
            if (nr >= 0) y = __fadd_rn(x[r], gumbel_noise(seed, tag, idx0 + (uint32_t)n));
            if (n < p.N && !(RULES && ((bits >> (4 + r)) & 1u))) {
                if (y > best) { best = y; bi = n; bx = x[r]; }          // ascending n: ties keep the first index
                xm = fmaxf(xm, x[r]);
            }
        }
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float ov = __shfl_xor(best, o, 64), ox = __shfl_xor(bx, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = ox; }
            xm = fmaxf(xm, __shfl_xor(xm, o, 64));
        }
        float se = 0.f;          // (the notes of gemm_sample128_kernel on xm and on all-banned parts hold here)
#pragma unroll
        for (int r = 0; r < 4; ++r) se += (n0 + 4 * g + r < p.N && !(RULES && ((bits >> (4 + r)) & 1u))) ? __expf(x[r] - xm) : 0.f;
        se += __shfl_xor(se, 16, 64);
        se += __shfl_xor(se, 32, 64);
        if (g == 0 && m < p.M) {
            const long o = (long)(pr.row0 + m) * nparts + part;
            part_val[o] = best; part_val[plane + o] = bx; part_val[2 * plane + o] = xm; part_val[3 * plane + o] = se;
            part_idx[o] = bi;
        }
    }
}

// FILTERED sampled pick (top-k / top-p, mvlt_gemm_sample_filtered / _step).  A filter is a set function of a whole row of x, so
// the row has to exist: the product writes x[m, n] (f32, [M, ldx]) into a workspace and a finishing kernel per row selects the
// threshold and draws.  The product is a SIBLING of gemm_sample128_kernel (a third copy of the main loop, for the reason given
// there; gemm_sample128_kernel itself is untouched): the same loads and MFMAs in the same order and the same two rounded
// epilogue operations, so x is bit for bit the value that kernel forms.  It computes no noise.
// vec: ldx % 4 == 0 and a 16-byte aligned workspace (whole 4-column groups go out as one 16-byte store).
// RULES: x is the processed logit (penalty ahead of the temperature) and -inf in a banned column; sample_filter_pick_kernel needs
// no change for that: -inf is below every finite key, weighs exp(-inf) = 0 in the masses and the sums, and y = -inf + G never beats
// the initial best of the draw -- also when top_k exceeds the number of unbanned columns and the threshold falls to -inf.
template <typename T, int NRT, typename... R>
__global__ __launch_bounds__(64 * SKINNY_WAVES) void gemm_logits128_kernel(const GemmDev p, float* xout, long ldx, int vec, float inv_t, const R... rules) {
    constexpr bool RULES = sizeof...(R) > 0;
    using M_ = Mma<T>;
    using Frag = typename M_::Frag;
    constexpr int KB = M_::KB, E = TypeInfo<T>::E, UNR = NRT <= 2 ? 12 : 8;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), r15 = lane & 15, g = lane >> 4;
    const int n0 = (blockIdx.x * SKINNY_WAVES + wave) * 16;
    if (n0 >= p.N) return;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* brow = reinterpret_cast<const T*>(p.B) + (long)min(n0 + r15, p.N - 1) * p.ldb + g * E;
    const T* arow[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) arow[i] = A + (long)min(16 * i + r15, p.M - 1) * p.lda + g * E;
    f32x4 acc[NRT];
#pragma unroll
    for (int i = 0; i < NRT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = p.K / KB;
    for (int kb0 = 0; kb0 < nkb; kb0 += UNR) {
        Frag fb[UNR], fa[UNR][NRT];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int k = min(kb0 + u, nkb - 1) * KB;          // past the end: reload the last block, never multiplied
            fb[u] = skinny_wload(reinterpret_cast<const Frag*>(brow + k));
#pragma unroll
            for (int i = 0; i < NRT; ++i) fa[u][i] = *reinterpret_cast<const Frag*>(arow[i] + k);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (kb0 + u < nkb) {
#pragma unroll
                for (int i = 0; i < NRT; ++i) M_::mma(acc[i], fb[u], fa[u][i]);
            }
        }
    }
    // acc[i][r] <-> n = n0 + 4 g + r, m = 16 i + r15
    f32x4 bias4{0.f, 0.f, 0.f, 0.f};
    if (p.epi & MVLT_EPI_BIAS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) bias4[r] = p.bias[min(n0 + 4 * g + r, p.N - 1)];
    }
#pragma unroll
    for (int i = 0; i < NRT; ++i) {
        const int m = 16 * i + r15, n = n0 + 4 * g;
        if (m >= p.M) continue;
        f32x4 x;
        if constexpr (RULES) {
            const uint32_t bits = rules_bits(rules_arg(rules...), m, p.M, n);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float raw = __fadd_rn(acc[i][r], bias4[r]);
                if ((bits >> r) & 1u) raw = rules_penalise(raw, rules_arg(rules...).penalty);
                x[r] = ((bits >> (4 + r)) & 1u) ? -__builtin_inff() : __fmul_rn(raw, inv_t);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = __fmul_rn(__fadd_rn(acc[i][r], bias4[r]), inv_t);
        }
        float* o = xout + (long)m * ldx + n;
        if (vec && n + 4 <= p.N) store4f(o, x);
        else
#pragma unroll
            for (int r = 0; r < 4; ++r) if (n + r < p.N) o[r] = x[r];
    }
}

// Finish of the filtered pick, one workgroup of 1024 threads per row (thread t owns the columns t, t + 1024, ...: a fixed map).
//   key(x)   the order-preserving 32-bit image of x (-0 counts as +0), so every comparison below is an integer one
//   tau_k    k-th largest key: exact radix select, four 8-bit digits from the top.  A digit pass histograms the candidates (keys
//            that match the digits chosen so far) by integer LDS adds and one wave walks the 256 bins from the top:
//            tau = the largest v with #{key >= v} >= k.  Ties at tau are all kept.
//   tau_p    over K1 = {key >= tau_k}: the SAME select with the count replaced by the mass q_n = rint(2^32 exp(x_n - max x)), a
//            64-bit integer, and k by P = ceil(top_p S), S = sum_K1 q: the largest v whose inclusive mass C(v) = sum_{key >= v} q
//            reaches P.  Then the mass strictly above tau_p is < P (tau_p is kept: A(x_n) < top_p S) and every smaller value has
//            A >= C(tau_p) >= P (not kept), which is the issue's rule K = {n in K1 : A(x_n) < top_p S}; the row maximum has
//            A = 0 and is always kept.
//   pick     over {key >= max(tau_k, tau_p)} only: y = x + gumbel_noise(seed, tag, (row0 + m) N + n), first index of the largest y,
//            and the kept sum of exp(x - max x) in f32 by a fixed tree (per thread four accumulators over its own columns in
//            ascending order, the wave's xor tree, the 16 wave sums in wave order) -> score = x_tok - (max x + logf(sum)).
// Determinism: histograms are integer adds (order-free), the f32 sum has a fixed shape, no float atomics; the same operands
// give the same set, token and score run to run and graph against eager.
// The row is RE-READ from the workspace in every pass (up to ten: max, 4 + 4 digits, pick) instead of being held in LDS: 64 rows
// x 119 KiB stay in L2 after the first pass, a pass is 30 coalesced dword loads per thread, and nothing caps N -- an LDS copy
// needs a > 64 KiB dynamic allocation that stops at N = 40 K and ties the launch to one vocabulary size.
// Mass arithmetic, relative to a sum that holds the row maximum (q = 2^32; every S, P, A(v) != 0 and C(v) does):
//   __expf(d), d = x - max <= 0: rounding of d (2^-24 |d|), d log2 e with a rounded constant (1.5 2^-24 |d|), v_exp_f32 <= 1 ulp
//   (2^-23) -> (2.5 |d| + 2) 2^-24 per term, taken as (3 |d| + 4) 2^-24; mass-weighted, mean |d| <= ln N (entropy <= ln N and the
//   sum is >= 1), so (3 ln N + 4) 2^-24 for the sum.  Quantisation: <= 1/2 per term against a sum >= 2^32: N 2^-33.  Summation:
//   integers, exact (N < 2^32 terms <= 2^32 fit 64 bits).  P = ceil(top_p S) in f64 with S converted once: 2^-51.
//       E_MASS(N) = (3 ln N + 4) 2^-24 + N 2^-33 + 2^-51          (5.6e-6 at N = 30522; tests/sample_filter_ref.py restates it)
constexpr int FILT_THREADS = 1024, FILT_COPIES = 16;
MVLT_DEV uint32_t filt_key(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
MVLT_DEV unsigned long long filt_mass(float x, float xmax) {
    return (unsigned long long)__float2ull_rn(__expf(__fadd_rn(x, -xmax)) * 4294967296.0f);
}
struct FilterIn { const float* x; long ldx; int top_k; float top_p; uint32_t row0; };
template <bool STEP>
__global__ __launch_bounds__(FILT_THREADS) void sample_filter_pick_kernel(const FilterIn f, int M, int N, const SampleIn si, const GreedyState st,
                                                                           int64_t* out_idx, float* out_logprob) {
    __shared__ unsigned long long hist[256 * FILT_COPIES];          // [bin][copy]: the copies of a bin lie in different banks
    __shared__ unsigned long long s_above;
    __shared__ int s_bin;
    __shared__ float s_val[16], s_x[16], s_f[16];
    __shared__ int s_idx[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
    const long col = STEP ? st.col[0] : 0;
    const uint64_t seed = si.seed_dev ? si.seed_dev[0] : si.seed;
    const uint32_t tag = si.tag0 + (si.col ? (uint32_t)si.col[0] : 0u);
    const float* x = f.x + (long)m * f.ldx;
    // ---- row maximum
    float xmax = -3.0e38f;
    for (int n = tid; n < N; n += FILT_THREADS) xmax = fmaxf(xmax, x[n]);
    xmax = wave_max(xmax);
    if (lane == 0) s_f[wave] = xmax;
    __syncthreads();
    xmax = s_f[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) xmax = fmaxf(xmax, s_f[w]);
    __syncthreads();          // (s_f is written again by the pick)
    // ---- the two selects: mode 0 = top-k (weight 1, target k), mode 1 = top-p over key >= tau_k (weight q, target ceil(top_p S))
    uint32_t tau = 0u;          // keep key >= tau; 0 keeps everything
    const bool use_k = f.top_k >= 1 && f.top_k < N, use_p = f.top_p < 1.0f;
    for (int mode = use_k ? 0 : 1; mode < (use_p ? 2 : 1); ++mode) {
        const uint32_t floor_key = tau;
        uint32_t prefix = 0u;
        unsigned long long above = 0ull, target = (unsigned long long)f.top_k;          // (target: wave 0 only)
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = tid; i < 256 * FILT_COPIES; i += FILT_THREADS) hist[i] = 0ull;
            __syncthreads();
            const uint32_t pmask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
            for (int n = tid; n < N; n += FILT_THREADS) {
                const float v = x[n];
                const uint32_t key = filt_key(v);
                if ((key & pmask) == prefix && key >= floor_key) {
                    const unsigned long long w = mode == 0 ? 1ull : filt_mass(v, xmax);
                    atomicAdd(&hist[((key >> shift) & 255u) * FILT_COPIES + (tid & (FILT_COPIES - 1))], w);
                }
            }
            __syncthreads();
            if (wave == 0) {          // lane l: bins 4 l .. 4 l + 3; higher lanes hold higher bins
                unsigned long long t[4], s = 0ull;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t[j] = 0ull;
#pragma unroll
                    for (int c = 0; c < FILT_COPIES; ++c) t[j] += hist[(4 * lane + j) * FILT_COPIES + c];
                    s += t[j];
                }
                unsigned long long inc = s;          // -> sum over the lanes >= this one
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned long long v = __shfl_down(inc, o, 64);
                    if (lane + o < 64) inc += v;
                }
                if (mode == 1 && shift == 24) {          // S = the mass of K1; P = ceil(top_p S) (top_p <= 1 - 2^-24 and S >= 2^32: P <= S)
                    const unsigned long long S = __shfl(inc, 0, 64);
                    target = (unsigned long long)ceil((double)f.top_p * (double)S);
                    if (target < 1ull) target = 1ull;
                    if (target > S) target = S;
                }
                const unsigned long long hi = above + (inc - s);          // weight of everything above this lane's bins
                if (hi < target && hi + s >= target) {          // exactly one lane: above < target <= above + the candidates' total
                    unsigned long long a = hi; int b = 4 * lane;
#pragma unroll
                    for (int j = 3; j >= 1; --j) {
                        if (b == 4 * lane) { if (a + t[j] >= target) b = 4 * lane + j; else a += t[j]; }
                    }
                    s_bin = b; s_above = a;
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_bin << shift;
            above = s_above;
            __syncthreads();
        }
        tau = prefix;
    }
    // ---- the pick over the kept columns
    float best = -3.0e38f, bx = 0.f, se[4] = {0.f, 0.f, 0.f, 0.f}; int bi = 0x7fffffff;
    const uint32_t idx0 = (f.row0 + (uint32_t)m) * (uint32_t)N;
    int j = 0;
    for (int n = tid; n < N; n += FILT_THREADS, ++j) {
        const float v = x[n];
        if (filt_key(v) >= tau) {
            const float y = __fadd_rn(v, gumbel_noise(seed, tag, idx0 + (uint32_t)n));
            if (y > best) { best = y; bi = n; bx = v; }          // ascending n: ties keep the first index
            se[j & 3] += __expf(__fadd_rn(v, -xmax));
        }
    }
    float sum = (se[0] + se[1]) + (se[2] + se[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64), ox = __shfl_xor(bx, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = ox; }
        sum += __shfl_xor(sum, o, 64);
    }
    if (lane == 0) { s_val[wave] = best; s_idx[wave] = bi; s_x[wave] = bx; s_f[wave] = sum; }
    __syncthreads();
    if (tid == 0) {
        sum = s_f[0];
        for (int w = 1; w < 16; ++w) {
            const float ov = s_val[w]; const int oi = s_idx[w];
            if (BEATS(ov, oi, best, bi)) { best = ov; bi = oi; bx = s_x[w]; }
            sum += s_f[w];
        }
        const float lse = __fadd_rn(xmax, logf(sum));
        const float score = __fadd_rn(bx, -lse);
        if (STEP) pick_bookkeeping(st, m, M, col, bi, score);
        else { out_idx[m] = bi; out_logprob[m] = score; }
    }
}

// BEAM candidates (mvlt_gemm_beam_candidates): the step of beam search between the head and the host scorer.  The product is
// gemm_logits128_kernel at inv_t = 1 (a multiplication by 1 is exact: x is the value the sampled kernels form), issued in row
// chunks of 64 into one workspace; then ONE workgroup of 1024 threads per sample g (thread t owns the columns t, t + 1024, ... of
// every beam row: a fixed map) reads its num_beams rows three times:
//   1  per thread and beam the largest x of its own columns, then the row maxima (wave tree, 16 wave values in LDS)
//   2  per row sum expf(x - max) by the fixed tree of sample_filter_pick_kernel (four accumulators over the thread's columns in
//      ascending order, (a0 + a1) + (a2 + a3), the wave's xor tree, the 16 wave sums in wave order) -> lse = max + logf(sum)
//   3  s = (x - lse) + beam_score; every entry with key(s) >= tau goes into an LDS list as key << 32 | ~flat (flat = beam N + n):
//      a larger word is a larger score or, at equal score, a lower flat index
// tau is a lower bound of the n_cand-th largest key: rounding is monotone, so the largest s among a thread's entries of a row is
// s(its largest x) -- known after pass 1 without a read -- and the n_cand-th largest of the 1024 thread maxima (exact rank by
// counting in LDS) has at least n_cand entries at or above it.  The list holds the n_cand winners and a few more (every entry a
// thread owns above tau); its rank order (count of larger words: words are distinct) gives the sorted output.  The order in which
// the list is filled is the only thing that varies run to run and the ranks do not depend on it.
// More than BEAM_LIST entries at or above tau (thousands of tied scores): n_cand rounds of "the largest word below the previous
// winner" over the rows instead -- slow, exact, the same answer.
// A workgroup per sample leaves most of the chip idle at small G (measured: profiles/beam_fused.md); splitting a sample over
// several workgroups needs a second launch for the merge and was not built.
// With LOGIT RULES (a trailing RulesDev in the pack R, as in the head kernels: the instantiation without one keeps the argument list
// and the code it had) the processors act where HF 4.16 beam_search puts them, on lp = x - lse ahead of the beam score: a seen entry
// is penalised once (rules_penalise on lp), a banned entry enters nothing but lse -- not tau, not the list, not the slow rounds.
// The thread maxima of the processed scores come from two more maxima per beam in pass 1 -- over the thread's unbanned unseen and
// over its unbanned seen columns: the penalty is monotone inside a class, not across them, and a banned maximum must not decide
// tau -- so the rows are still read three times; a thread without an unbanned entry holds 0.  Fewer than n_cand unbanned entries in the sample: tau = 0
// lists them all and the remaining slots are filled with (-inf, 0, 0).
constexpr int BEAM_THREADS = 1024, BEAM_MAXB = 8, BEAM_MAXC = 16, BEAM_LIST = 1024;
struct BeamIn {
    const float* x; long ldx; const float* beam_scores; int num_beams, n_cand, N;
    float* cand_score; int32_t* cand_beam; int32_t* cand_tok; float* lse;
};
MVLT_DEV unsigned long long beam_word(float x, float lse, float bs, uint32_t flat) {
    return ((unsigned long long)filt_key(__fadd_rn(__fadd_rn(x, -lse), bs)) << 32) | (unsigned long long)(0xFFFFFFFFu - flat);
}
// the rule-aware word of an unbanned entry: HF's beam_search hands its processors the log-probability, so the penalty acts on
// lp = x - lse (lse over ALL columns, unprocessed) and the beam score is added behind it
MVLT_DEV unsigned long long beam_word_seen(float x, float lse, float bs, uint32_t flat, bool seen, float penalty) {
    float lp = __fadd_rn(x, -lse);
    if (seen) lp = rules_penalise(lp, penalty);
    return ((unsigned long long)filt_key(__fadd_rn(lp, bs)) << 32) | (unsigned long long)(0xFFFFFFFFu - flat);
}
// a slot no unbanned entry is left for (fewer than n_cand of them in the sample): (-inf, beam 0, token 0)
MVLT_DEV void beam_emit_none(const BeamIn& f, const long o) {
    f.cand_score[o] = -__builtin_inff(); f.cand_beam[o] = 0; f.cand_tok[o] = 0;
}
MVLT_DEV void beam_emit(const BeamIn& f, const long o, const unsigned long long w) {
    const uint32_t key = (uint32_t)(w >> 32), flat = 0xFFFFFFFFu - (uint32_t)w;
    f.cand_score[o] = __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    f.cand_beam[o] = (int32_t)(flat / (uint32_t)f.N);
    f.cand_tok[o] = (int32_t)(flat % (uint32_t)f.N);
}
template <typename... R>
__global__ __launch_bounds__(BEAM_THREADS) void beam_candidates_kernel(const BeamIn f, const R... rules) {
    constexpr bool RULES = sizeof...(R) > 0;
    __shared__ float s_f[BEAM_MAXB][16];
    __shared__ float s_lse[BEAM_MAXB], s_bs[BEAM_MAXB];
    __shared__ uint32_t s_tmax[BEAM_THREADS];
    __shared__ unsigned long long s_list[BEAM_LIST], s_w[16];
    __shared__ uint32_t s_tau;
    __shared__ int s_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = blockIdx.x, nb = f.num_beams, N = f.N;
    const float* x0 = f.x + (long)g * nb * f.ldx;
    // ---- 1: thread and row maxima
    float tmax[BEAM_MAXB], rmax[BEAM_MAXB];
    // RULES: per thread and beam also the largest x among its unbanned UNSEEN and among its unbanned SEEN columns (-inf: none).
    // x -> lp -> penalised lp -> s is monotone inside either class, so the largest processed s of a class is that of its largest x
    [[maybe_unused]] float umax[BEAM_MAXB], smax[BEAM_MAXB];
#pragma unroll
    for (int b = 0; b < BEAM_MAXB; ++b) {
        tmax[b] = -3.0e38f;
        if constexpr (RULES) { umax[b] = -__builtin_inff(); smax[b] = -__builtin_inff(); }
        if (b < nb) {
            const float* x = x0 + (long)b * f.ldx;
            if constexpr (RULES) {
                const RulesDev& rd = rules_arg(rules...);
                const long w0 = ((long)g * nb + b) * rd.ld_words;
                for (int n = tid; n < N; n += BEAM_THREADS) {
                    const float v = x[n];
                    const uint32_t bit = 1u << (n & 31), bw = rd.banned[w0 + (n >> 5)], sw = rd.seen[w0 + (n >> 5)];
                    tmax[b] = fmaxf(tmax[b], v);          // the row maximum and lse are those of the unprocessed row
                    if (!(bw & bit)) {
                        if (sw & bit) smax[b] = fmaxf(smax[b], v);
                        else umax[b] = fmaxf(umax[b], v);
                    }
                }
            } else {
                for (int n = tid; n < N; n += BEAM_THREADS) tmax[b] = fmaxf(tmax[b], x[n]);
            }
            const float wm = wave_max(tmax[b]);
            if (lane == 0) s_f[b][wave] = wm;
        }
    }
    if (tid == 0) s_count = 0;
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BEAM_MAXB; ++b) {
        rmax[b] = -3.0e38f;
        if (b < nb) {
            rmax[b] = s_f[b][0];
#pragma unroll
            for (int w = 1; w < 16; ++w) rmax[b] = fmaxf(rmax[b], s_f[b][w]);
        }
    }
    __syncthreads();          // (s_f is written again by the sums)
    // ---- 2: sum expf(x - max) per row, fixed shape
#pragma unroll
    for (int b = 0; b < BEAM_MAXB; ++b) {
        if (b < nb) {
            const float* x = x0 + (long)b * f.ldx;
            float se[4] = {0.f, 0.f, 0.f, 0.f};
            int j = 0;
            for (int n = tid; n < N; n += BEAM_THREADS, ++j) se[j & 3] += __expf(__fadd_rn(x[n], -rmax[b]));
            float sum = (se[0] + se[1]) + (se[2] + se[3]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (lane == 0) s_f[b][wave] = sum;
        }
    }
    __syncthreads();
    if (tid < nb) {
        float sum = s_f[tid][0];
        for (int w = 1; w < 16; ++w) sum += s_f[tid][w];
        float mx = 0.f;          // (rmax[] lives in registers, indexed by a compile-time b)
#pragma unroll
        for (int b = 0; b < BEAM_MAXB; ++b) if (b == tid) mx = rmax[b];
        const float lse = __fadd_rn(mx, logf(sum));
        s_lse[tid] = lse;
        s_bs[tid] = f.beam_scores[(long)g * nb + tid];
        if (f.lse) f.lse[(long)g * nb + tid] = lse;
    }
    __syncthreads();
    // ---- tau: the n_cand-th largest of the thread maxima (threads without a column hold 0, below every key)
    uint32_t mine = 0u;
    if constexpr (RULES) {
        // the penalty breaks "largest s = s of the largest x" across the two classes and a banned entry may decide nothing: the
        // largest PROCESSED key of the thread's unbanned entries, from the two class maxima of pass 1 (a thread without an
        // unbanned entry holds 0, below every key; with fewer than n_cand threads above 0, tau = 0 admits every unbanned entry)
        const float penalty = rules_arg(rules...).penalty;
#pragma unroll
        for (int b = 0; b < BEAM_MAXB; ++b) {
            if (b < nb) {
                const float lse = s_lse[b], bs = s_bs[b];
                if (umax[b] > -__builtin_inff()) mine = max(mine, (uint32_t)(beam_word_seen(umax[b], lse, bs, 0u, false, penalty) >> 32));
                if (smax[b] > -__builtin_inff()) mine = max(mine, (uint32_t)(beam_word_seen(smax[b], lse, bs, 0u, true, penalty) >> 32));
            }
        }
    } else if (tid < N) {
#pragma unroll
        for (int b = 0; b < BEAM_MAXB; ++b)
            if (b < nb) mine = max(mine, filt_key(__fadd_rn(__fadd_rn(tmax[b], -s_lse[b]), s_bs[b])));
    }
    s_tmax[tid] = mine;
    __syncthreads();
    {
        int above = 0;
        for (int j = 0; j < BEAM_THREADS; ++j) {
            const uint32_t o = s_tmax[j];
            above += (o > mine || (o == mine && j < tid)) ? 1 : 0;
        }
        if (above == f.n_cand - 1) s_tau = mine;
    }
    __syncthreads();
    const uint32_t tau = s_tau;
    // ---- 3: the list of entries at or above tau
#pragma unroll
    for (int b = 0; b < BEAM_MAXB; ++b) {
        if (b < nb) {
            const float* x = x0 + (long)b * f.ldx;
            const float lse = s_lse[b], bs = s_bs[b];
            for (int n = tid; n < N; n += BEAM_THREADS) {
                unsigned long long w;
                if constexpr (RULES) {
                    const RulesDev& rd = rules_arg(rules...);
                    const long wi = ((long)g * nb + b) * rd.ld_words + (n >> 5);
                    const uint32_t bit = 1u << (n & 31);
                    if (rd.banned[wi] & bit) continue;          // a banned entry never enters the list
                    w = beam_word_seen(x[n], lse, bs, (uint32_t)b * (uint32_t)N + (uint32_t)n, (rd.seen[wi] & bit) != 0u, rd.penalty);
                } else {
                    w = beam_word(x[n], lse, bs, (uint32_t)b * (uint32_t)N + (uint32_t)n);
                }
                if ((uint32_t)(w >> 32) >= tau) {
                    const int pos = atomicAdd(&s_count, 1);
                    if (pos < BEAM_LIST) s_list[pos] = w;
                }
            }
        }
    }
    __syncthreads();
    const int count = s_count;
    const long out0 = (long)g * f.n_cand;
    if (count <= BEAM_LIST) {          // (count >= n_cand: tau is a lower bound of the n_cand-th largest key)
        if (tid < count) {
            const unsigned long long w = s_list[tid];
            int rank = 0;
            for (int j = 0; j < count; ++j) rank += s_list[j] > w ? 1 : 0;
            if (rank < f.n_cand) beam_emit(f, out0 + rank, w);
        }
        if constexpr (RULES) {          // fewer unbanned entries than n_cand (tau = 0 listed them all): the rest of the list is empty
            if (tid >= count && tid < f.n_cand) beam_emit_none(f, out0 + tid);
        }
        return;
    }
    unsigned long long prev = ~0ull;
    for (int c = 0; c < f.n_cand; ++c) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int b = 0; b < BEAM_MAXB; ++b) {
            if (b < nb) {
                const float* x = x0 + (long)b * f.ldx;
                const float lse = s_lse[b], bs = s_bs[b];
                for (int n = tid; n < N; n += BEAM_THREADS) {
                    unsigned long long w;
                    if constexpr (RULES) {
                        const RulesDev& rd = rules_arg(rules...);
                        const long wi = ((long)g * nb + b) * rd.ld_words + (n >> 5);
                        const uint32_t bit = 1u << (n & 31);
                        if (rd.banned[wi] & bit) continue;
                        w = beam_word_seen(x[n], lse, bs, (uint32_t)b * (uint32_t)N + (uint32_t)n, (rd.seen[wi] & bit) != 0u, rd.penalty);
                    } else {
                        w = beam_word(x[n], lse, bs, (uint32_t)b * (uint32_t)N + (uint32_t)n);
                    }
                    if (w < prev && w > best) best = w;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ow = __shfl_xor(best, o, 64);
            if (ow > best) best = ow;
        }
        if (lane == 0) s_w[wave] = best;
        __syncthreads();
        best = s_w[0];
        for (int w = 1; w < 16; ++w) if (s_w[w] > best) best = s_w[w];
        if constexpr (RULES) {          // no unbanned entry below the previous winner: this slot and every later one stay empty
            if (tid == 0) { if (best != 0ull) beam_emit(f, out0 + c, best); else beam_emit_none(f, out0 + c); }
        } else {
            if (tid == 0) beam_emit(f, out0 + c, best);
        }
        prev = best;
        __syncthreads();          // (s_w is written again by the next round)
    }
}

// --------------------------------------------------------------------------------------------------------------- host
// run f(T{}) for the product's element type
template <typename F> int by_dtype(const int dtype, F&& f) {
    if (dtype == MVLT_BF16) return f(bf16_t{});
    if (dtype == MVLT_F32) return f(float{});
    return MVLT_ERR_UNSUPPORTED;
}

// the one precondition of every kernel in this file
template <typename T> bool skinny_ok(const MvltGemm* p) { return is_skinny<T>(p) && skinny_loads_ok<T>(p); }

// The kernel argument block of the head products and the K-split product: they read only M N K A lda B ldb epi bias (m_dev); the
// rest stays zero.
GemmDev skinny_dev(const MvltGemm* p) {
    GemmDev d{};
    d.M = p->M; d.N = p->N; d.K = p->K; d.A = p->A; d.lda = p->lda; d.B = p->B; d.ldb = p->ldb;
    d.epi = p->epilogue; d.bias = p->bias; d.m_dev = p->m_dev;
    return d;
}

// kernel<T, NRT> for the NRT = ceil(M / 16) row tiles of the wide products
#define LAUNCH_NRT(kernel, T, M, grid, block, s, ...)                                                     \
    do {                                                                                                  \
        if ((M) <= 16) hipLaunchKernelGGL((kernel<T, 1>), grid, block, 0, s, __VA_ARGS__);                \
        else if ((M) <= 32) hipLaunchKernelGGL((kernel<T, 2>), grid, block, 0, s, __VA_ARGS__);           \
        else if ((M) <= 48) hipLaunchKernelGGL((kernel<T, 3>), grid, block, 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<T, 4>), grid, block, 0, s, __VA_ARGS__);                          \
    } while (0)

int parts_of(const MvltGemm* p) { return ceil_div(p->N, 16); }          // one part per row and 16 columns

// the (max, index) partials per row and 16 columns: wide streaming form for big vocabularies, else the 16-column skinny kernel
// (`r`: the logit rules or nullptr; with rules always the wide form, which takes any N -- the 16-column kernel has no rule-aware sibling)
int argmax_products(const MvltGemm* p, float* part_val, int32_t* part_idx, hipStream_t s, const RulesDev* r = nullptr) {
    MVLT_CHECK((p->epilogue & ~(MVLT_EPI_BIAS)) == 0, MVLT_ERR_UNSUPPORTED);
    return by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        MVLT_CHECK(skinny_ok<T>(p), MVLT_ERR_UNSUPPORTED);
        const GemmDev d = skinny_dev(p);
        const int nblk = parts_of(p);
        const ArgmaxOut am{part_val, part_idx};
        const dim3 block(64 * SKINNY_WAVES);
        if (r) LAUNCH_NRT(gemm_argmax128_kernel, T, p->M, dim3(ceil_div(nblk, SKINNY_WAVES)), block, s, d, am, nblk, *r);
        else if (p->N >= 4096) LAUNCH_NRT(gemm_argmax128_kernel, T, p->M, dim3(ceil_div(nblk, SKINNY_WAVES)), block, s, d, am, nblk);
        else hipLaunchKernelGGL((gemm_skinny_kernel<T, true>), dim3(nblk), block, 0, s, d, am);
        return (int)MVLT_OK;
    });
}

// the sampled partials: always the wide streaming form (it handles any N; the 16-column skinny kernel has no sampled sibling)
int sample_products(const MvltGemm* p, float* part_val, int32_t* part_idx, const SampleIn& si, hipStream_t s, const RulesDev* r = nullptr) {
    return by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        MVLT_CHECK(skinny_ok<T>(p), MVLT_ERR_UNSUPPORTED);
        const GemmDev d = skinny_dev(p);
        const int nblk = parts_of(p);
        const dim3 grid(ceil_div(nblk, SKINNY_WAVES)), block(64 * SKINNY_WAVES);
        if (r) LAUNCH_NRT(gemm_sample128_kernel, T, p->M, grid, block, s, d, part_val, part_idx, nblk, si, *r);
        else LAUNCH_NRT(gemm_sample128_kernel, T, p->M, grid, block, s, d, part_val, part_idx, nblk, si);
        return (int)MVLT_OK;
    });
}

// what mvlt_gemm_argmax_greedy, mvlt_gemm_sample and mvlt_gemm_sample_step ask of the product and the scratch
int head_check(const MvltGemm* p, const float* part_val, const int32_t* part_idx) {
    MVLT_CHECK(p && p->A && p->B && part_val && part_idx, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->M <= 64 && p->N > 0 && p->K > 0 && p->lda > 0 && p->ldb > 0, MVLT_ERR_ARG);
    MVLT_CHECK(!p->a_kmajor && !p->b_kmajor && (p->epilogue & ~(MVLT_EPI_BIAS)) == 0, MVLT_ERR_UNSUPPORTED);
    if (p->epilogue & MVLT_EPI_BIAS) MVLT_CHECK(p->bias, MVLT_ERR_ARG);
    return MVLT_OK;
}
int sample_check(const MvltGemm* p, const float* part_val, const int32_t* part_idx, float inv_temperature) {
    { const int rc = head_check(p, part_val, part_idx); if (rc != MVLT_OK) return rc; }
    MVLT_CHECK((long)p->M * p->N < (1L << 32) && inv_temperature > 0.f && inv_temperature < 3.0e38f, MVLT_ERR_ARG);
    return MVLT_OK;
}

// MvltGreedyState / MvltSampleState (the same bookkeeping fields) -> the pick kernels' argument
template <typename S> int greedy_state(const S* g, GreedyState& st) {
    MVLT_CHECK(g->col && g->ticket && g->ids && g->scores && g->new_ids && g->ld_ids > 0 && g->ld_scores > 0 && g->ld_new > 0, MVLT_ERR_ARG);
    if (g->has_eos) MVLT_CHECK(g->unfinished && g->alive, MVLT_ERR_ARG);
    st = GreedyState{g->unfinished, g->eos_id, g->pad_id, g->has_eos, g->col, g->past, g->ids, g->ld_ids, g->scores, g->ld_scores, g->alive,
                     g->new_ids, g->ld_new, g->ticket};
    return MVLT_OK;
}

// MvltLogitRules -> what the rule-aware heads read, for a product of M rows and N columns (the refusals of mvlt_hip.h);
// max_rows: 64 for the six picks (one tile of rows), none for the beam candidates, whose product goes in row chunks
int rules_dev(const MvltLogitRules* r, const int M, const int N, RulesDev& rd, const int max_rows = 64) {
    MVLT_CHECK(r && r->seen && r->banned && M >= 1 && M <= max_rows && N >= 1, MVLT_ERR_ARG);
    MVLT_CHECK(r->ld_words >= (long)ceil_div(N, 32) && r->penalty > 0.f && r->ngram >= 0, MVLT_ERR_ARG);          // (a NaN penalty fails > 0)
    rd = RulesDev{r->seen, r->banned, (long)r->ld_words, r->penalty};
    return MVLT_OK;
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) int mvlt_skinny_try(const MvltGemm* p, const void* dev_block, void* stream, int* route) {
    const GemmDev& d = *reinterpret_cast<const GemmDev*>(dev_block);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        if (!skinny_ok<T>(p)) return 0;
        if (p->epilogue & MVLT_EPI_TAIL) return 0;          // rows beyond *m_dev leave this kernel: the tile kernels honour the bit
        if (route) { *route = gemm_route_code(MVLT_GEMM_ROUTE_SKINNY, 1); return 1; }
        hipLaunchKernelGGL((gemm_skinny_kernel<T, false>), dim3(ceil_div(p->N, 16)), dim3(64 * SKINNY_WAVES), 0, s, d, ArgmaxOut{nullptr, nullptr});
        return hipGetLastError() == hipSuccess ? 1 : -1;
    });
    return rc == MVLT_ERR_UNSUPPORTED ? 0 : rc;
}

// The head entry points come in pairs: the plain form and its _rules form (the same checks and launches with the rule-aware
// product, `r` = the checked rules; nullptr: none).
namespace {
int argmax_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_val, const RulesDev* r, void* stream) {
    MVLT_CHECK(p && p->A && p->B && part_val && part_idx && out_idx, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->N > 0 && p->K > 0 && p->lda > 0 && p->ldb > 0, MVLT_ERR_ARG);
    if (p->epilogue & MVLT_EPI_BIAS) MVLT_CHECK(p->bias, MVLT_ERR_ARG);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    { const int rc = argmax_products(p, part_val, part_idx, s, r); if (rc != MVLT_OK) return rc; }
    hipLaunchKernelGGL(argmax_parts_kernel, dim3(p->M), dim3(64), 0, s, part_val, part_idx, parts_of(p), out_idx, out_val);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
int argmax_greedy_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltGreedyState* g, const RulesDev* r, void* stream) {
    MVLT_CHECK(g, MVLT_ERR_ARG);
    { const int rc = head_check(p, part_val, part_idx); if (rc != MVLT_OK) return rc; }
    GreedyState st;
    { const int rc = greedy_state(g, st); if (rc != MVLT_OK) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    { const int rc = argmax_products(p, part_val, part_idx, s, r); if (rc != MVLT_OK) return rc; }
    hipLaunchKernelGGL(greedy_pick_kernel, dim3(p->M), dim3(256), 0, s, part_val, part_idx, parts_of(p), p->M, st);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
int sample_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag,
                 float inv_temperature, const RulesDev* r, void* stream) {
    { const int rc = sample_check(p, part_val, part_idx, inv_temperature); if (rc != MVLT_OK) return rc; }
    MVLT_CHECK(out_idx && out_logprob, MVLT_ERR_ARG);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const SampleIn si{nullptr, seed, nullptr, tag, inv_temperature};
    { const int rc = sample_products(p, part_val, part_idx, si, s, r); if (rc != MVLT_OK) return rc; }
    hipLaunchKernelGGL(sample_pick_kernel<false>, dim3(p->M), dim3(256), 0, s, part_val, part_idx, parts_of(p), p->M, GreedyState{}, out_idx, out_logprob);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
int sample_step_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleState* g, const RulesDev* r, void* stream) {
    MVLT_CHECK(g, MVLT_ERR_ARG);
    { const int rc = sample_check(p, part_val, part_idx, g->inv_temperature); if (rc != MVLT_OK) return rc; }
    MVLT_CHECK(g->seed, MVLT_ERR_ARG);
    GreedyState st;
    { const int rc = greedy_state(g, st); if (rc != MVLT_OK) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const SampleIn si{g->seed, 0, g->col, g->tag0, g->inv_temperature};
    { const int rc = sample_products(p, part_val, part_idx, si, s, r); if (rc != MVLT_OK) return rc; }
    hipLaunchKernelGGL(sample_pick_kernel<true>, dim3(p->M), dim3(256), 0, s, part_val, part_idx, parts_of(p), p->M, st, (int64_t*)nullptr, (float*)nullptr);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
// The per-row pick: every check ahead of the first launch (a refused call launches nothing), then one product launch per group
// of 64 rows -- each streams the weights once, with the 1-4 row-tile instantiation of its row count -- and ONE finish over all
// rows (sample_pick_kernel: a workgroup per row, the ticket counts p->M rows).  `g`: the step form's state, nullptr: stand-alone.
int pick_rows_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t, int64_t* out_idx,
                    float* out_logprob, uint64_t seed, uint32_t tag, const MvltSampleState* g, const bool step, const RulesDev* r, void* stream) {
    MVLT_CHECK(p && p->A && p->B && part_val && part_idx && noise_row && inv_t, MVLT_ERR_ARG);
    MVLT_CHECK(p->M >= 1 && p->N > 0 && p->K > 0 && p->lda > 0 && p->ldb > 0 && (long)p->M * p->N < (1L << 32), MVLT_ERR_ARG);
    if (p->epilogue & MVLT_EPI_BIAS) MVLT_CHECK(p->bias, MVLT_ERR_ARG);
    GreedyState st{};
    SampleIn si{nullptr, seed, nullptr, tag, 1.0f};
    if (step) {
        MVLT_CHECK(g && g->seed, MVLT_ERR_ARG);
        { const int rc = greedy_state(g, st); if (rc != MVLT_OK) return rc; }
        si = SampleIn{g->seed, 0, g->col, g->tag0, 1.0f};
    } else {
        MVLT_CHECK(out_idx && out_logprob, MVLT_ERR_ARG);
    }
    MVLT_CHECK(!p->a_kmajor && !p->b_kmajor && (p->epilogue & ~(MVLT_EPI_BIAS)) == 0, MVLT_ERR_UNSUPPORTED);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nblk = parts_of(p);
    const int rc = by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        for (int pass = 0; pass < 2; ++pass) {          // 0: check every group, 1: launch
            for (int r0 = 0; r0 < p->M; r0 += 64) {
                MvltGemm q = *p;
                q.M = p->M - r0 < 64 ? p->M - r0 : 64;
                q.A = reinterpret_cast<const T*>(p->A) + (long)r0 * p->lda;
                q.m_dev = nullptr;
                if (pass == 0) { MVLT_CHECK(skinny_ok<T>(&q), MVLT_ERR_UNSUPPORTED); continue; }
                const GemmDev d = skinny_dev(&q);
                const PickRows pr{noise_row, inv_t, r0, p->M};
                const dim3 grid(ceil_div(nblk, SKINNY_WAVES)), block(64 * SKINNY_WAVES);
                if (r) {
                    const RulesDev rg{r->seen + (long)r0 * r->ld_words, r->banned + (long)r0 * r->ld_words, r->ld_words, r->penalty};
                    LAUNCH_NRT(gemm_pick_rows128_kernel, T, q.M, grid, block, s, d, part_val, part_idx, nblk, si, pr, rg);
                } else {
                    LAUNCH_NRT(gemm_pick_rows128_kernel, T, q.M, grid, block, s, d, part_val, part_idx, nblk, si, pr);
                }
            }
        }
        return (int)MVLT_OK;
    });
    if (rc != MVLT_OK) return rc;
    if (step) hipLaunchKernelGGL(sample_pick_kernel<true>, dim3(p->M), dim3(256), 0, s, part_val, part_idx, nblk, p->M, st, (int64_t*)nullptr, (float*)nullptr);
    else hipLaunchKernelGGL(sample_pick_kernel<false>, dim3(p->M), dim3(256), 0, s, part_val, part_idx, nblk, p->M, GreedyState{}, out_idx, out_logprob);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
// the rules of a _rules call, checked ahead of everything else: rc != MVLT_OK refuses the call
#define RULES_OF(rd, rules, p)                                                                 \
    RulesDev rd;                                                                                \
    { MVLT_CHECK(p, MVLT_ERR_ARG); const int rc_ = rules_dev(rules, (p)->M, (p)->N, rd); if (rc_ != MVLT_OK) return rc_; }
}  // namespace

extern "C" int mvlt_decode_rules_plan(const MvltLogitRules* r, int M, int V, void* stream) {
    MVLT_CHECK(r && r->seen && r->banned && r->ids && r->col, MVLT_ERR_ARG);
    MVLT_CHECK(M >= 1 && M <= 64 && V >= 1 && r->ld_ids >= 1 && r->ld_words >= (long)ceil_div(V, 32), MVLT_ERR_ARG);
    MVLT_CHECK(r->penalty > 0.f && r->ngram >= 0 && r->min_length >= 0, MVLT_ERR_ARG);
    const RulesPlan f{r->seen, r->banned, (long)r->ld_words, r->ids, (long)r->ld_ids, r->col, r->ngram, r->min_length, r->eos_id, r->has_eos, V};
    hipLaunchKernelGGL(decode_rules_plan_kernel, dim3(M), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), f);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_gemm_argmax(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_val,
                                void* stream) {
    return argmax_entry(p, part_val, part_idx, out_idx, out_val, nullptr, stream);
}
extern "C" int mvlt_gemm_argmax_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_val,
                                      const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return argmax_entry(p, part_val, part_idx, out_idx, out_val, &rd, stream);
}

extern "C" int mvlt_gemm_argmax_greedy(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltGreedyState* g, void* stream) {
    return argmax_greedy_entry(p, part_val, part_idx, g, nullptr, stream);
}
extern "C" int mvlt_gemm_argmax_greedy_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltGreedyState* g,
                                             const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return argmax_greedy_entry(p, part_val, part_idx, g, &rd, stream);
}

extern "C" int mvlt_gemm_sample(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_logprob,
                                uint64_t seed, uint32_t tag, float inv_temperature, void* stream) {
    return sample_entry(p, part_val, part_idx, out_idx, out_logprob, seed, tag, inv_temperature, nullptr, stream);
}
extern "C" int mvlt_gemm_sample_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, int64_t* out_idx, float* out_logprob,
                                      uint64_t seed, uint32_t tag, float inv_temperature, const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return sample_entry(p, part_val, part_idx, out_idx, out_logprob, seed, tag, inv_temperature, &rd, stream);
}

extern "C" int mvlt_gemm_sample_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleState* g, void* stream) {
    return sample_step_entry(p, part_val, part_idx, g, nullptr, stream);
}
extern "C" int mvlt_gemm_sample_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleState* g,
                                           const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return sample_step_entry(p, part_val, part_idx, g, &rd, stream);
}

// the per-row pick and its rules: the bitmaps cover all p->M rows (RULES_OF without its 64 rows)
#define RULES_OF_ROWS(rd, rules, p)                                                                  \
    RulesDev rd;                                                                                     \
    { MVLT_CHECK(p, MVLT_ERR_ARG); const int rc_ = rules_dev(rules, (p)->M, (p)->N, rd, 0x7FFFFFFF); if (rc_ != MVLT_OK) return rc_; }
extern "C" int mvlt_gemm_pick_rows(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                                   int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, void* stream) {
    return pick_rows_entry(p, part_val, part_idx, noise_row, inv_t, out_idx, out_logprob, seed, tag, nullptr, false, nullptr, stream);
}
extern "C" int mvlt_gemm_pick_rows_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                                         int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, const MvltLogitRules* rules,
                                         void* stream) {
    RULES_OF_ROWS(rd, rules, p);
    return pick_rows_entry(p, part_val, part_idx, noise_row, inv_t, out_idx, out_logprob, seed, tag, nullptr, false, &rd, stream);
}
extern "C" int mvlt_gemm_pick_rows_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row, const float* inv_t,
                                        const MvltSampleState* g, void* stream) {
    return pick_rows_entry(p, part_val, part_idx, noise_row, inv_t, nullptr, nullptr, 0, 0, g, true, nullptr, stream);
}
extern "C" int mvlt_gemm_pick_rows_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const int32_t* noise_row,
                                              const float* inv_t, const MvltSampleState* g, const MvltLogitRules* rules, void* stream) {
    RULES_OF_ROWS(rd, rules, p);
    return pick_rows_entry(p, part_val, part_idx, noise_row, inv_t, nullptr, nullptr, 0, 0, g, true, &rd, stream);
}

// the two launches of the filtered pick: x = the product (bit for bit gemm_sample128_kernel's), then a workgroup per row
namespace {
int filter_check(const MvltGemm* p, const MvltSampleFilter* f) {
    MVLT_CHECK(f && f->x && f->ldx >= p->N && f->top_k >= 0 && f->top_p > 0.f, MVLT_ERR_ARG);          // (a NaN top_p fails > 0)
    MVLT_CHECK(((long)f->row0 + p->M) * p->N < (1L << 32), MVLT_ERR_ARG);
    return MVLT_OK;
}
template <bool STEP>
int filtered_launch(const MvltGemm* p, const MvltSampleFilter* f, const SampleIn& si, const GreedyState& st, int64_t* out_idx, float* out_logprob,
                    const RulesDev* r, hipStream_t s) {
    const int rc = by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        MVLT_CHECK(skinny_ok<T>(p), MVLT_ERR_UNSUPPORTED);
        const GemmDev d = skinny_dev(p);
        const int vec = (f->ldx % 4 == 0 && aligned16(f->x)) ? 1 : 0;
        const dim3 grid(ceil_div(parts_of(p), SKINNY_WAVES)), block(64 * SKINNY_WAVES);
        if (r) LAUNCH_NRT(gemm_logits128_kernel, T, p->M, grid, block, s, d, f->x, (long)f->ldx, vec, si.inv_t, *r);
        else LAUNCH_NRT(gemm_logits128_kernel, T, p->M, grid, block, s, d, f->x, (long)f->ldx, vec, si.inv_t);
        return (int)MVLT_OK;
    });
    if (rc != MVLT_OK) return rc;
    const FilterIn fi{f->x, (long)f->ldx, f->top_k, f->top_p, f->row0};
    hipLaunchKernelGGL(sample_filter_pick_kernel<STEP>, dim3(p->M), dim3(FILT_THREADS), 0, s, fi, p->M, p->N, si, st, out_idx, out_logprob);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
int filtered_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter, int64_t* out_idx, float* out_logprob,
                   uint64_t seed, uint32_t tag, float inv_temperature, const RulesDev* r, void* stream) {
    { const int rc = sample_check(p, part_val, part_idx, inv_temperature); if (rc != MVLT_OK) return rc; }
    { const int rc = filter_check(p, filter); if (rc != MVLT_OK) return rc; }
    MVLT_CHECK(out_idx && out_logprob, MVLT_ERR_ARG);
    const SampleIn si{nullptr, seed, nullptr, tag, inv_temperature};
    return filtered_launch<false>(p, filter, si, GreedyState{}, out_idx, out_logprob, r, reinterpret_cast<hipStream_t>(stream));
}
int filtered_step_entry(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter, const MvltSampleState* g,
                        const RulesDev* r, void* stream) {
    MVLT_CHECK(g, MVLT_ERR_ARG);
    { const int rc = sample_check(p, part_val, part_idx, g->inv_temperature); if (rc != MVLT_OK) return rc; }
    { const int rc = filter_check(p, filter); if (rc != MVLT_OK) return rc; }
    MVLT_CHECK(g->seed, MVLT_ERR_ARG);
    GreedyState st;
    { const int rc = greedy_state(g, st); if (rc != MVLT_OK) return rc; }
    const SampleIn si{g->seed, 0, g->col, g->tag0, g->inv_temperature};
    return filtered_launch<true>(p, filter, si, st, nullptr, nullptr, r, reinterpret_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" int mvlt_gemm_sample_filtered(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter, int64_t* out_idx,
                                         float* out_logprob, uint64_t seed, uint32_t tag, float inv_temperature, void* stream) {
    return filtered_entry(p, part_val, part_idx, filter, out_idx, out_logprob, seed, tag, inv_temperature, nullptr, stream);
}
extern "C" int mvlt_gemm_sample_filtered_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                               int64_t* out_idx, float* out_logprob, uint64_t seed, uint32_t tag, float inv_temperature,
                                               const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return filtered_entry(p, part_val, part_idx, filter, out_idx, out_logprob, seed, tag, inv_temperature, &rd, stream);
}

extern "C" int mvlt_gemm_sample_filtered_step(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                              const MvltSampleState* g, void* stream) {
    return filtered_step_entry(p, part_val, part_idx, filter, g, nullptr, stream);
}
extern "C" int mvlt_gemm_sample_filtered_step_rules(const MvltGemm* p, float* part_val, int32_t* part_idx, const MvltSampleFilter* filter,
                                                    const MvltSampleState* g, const MvltLogitRules* rules, void* stream) {
    RULES_OF(rd, rules, p);
    return filtered_step_entry(p, part_val, part_idx, filter, g, &rd, stream);
}

// The beam candidates: the product in row chunks of <= 64 into the one workspace, then the selection (`r` = the checked rules of
// the _rules form: the product stays the plain one, the selection is the rule-aware instantiation).  Every chunk is checked
// before the first launch: a refused call launches nothing.
namespace {
int beam_candidates_entry(const MvltGemm* p, const MvltBeamCand* c, const RulesDev* r, void* stream) {
    MVLT_CHECK(p && c && p->A && p->B && c->beam_scores && c->x && c->cand_score && c->cand_beam && c->cand_tok, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->N > 0 && p->K > 0 && p->lda > 0 && p->ldb > 0, MVLT_ERR_ARG);
    MVLT_CHECK(c->num_beams >= 1 && c->n_cand >= 1 && p->M % c->num_beams == 0 && c->ldx >= p->N, MVLT_ERR_ARG);
    MVLT_CHECK((long)c->num_beams * p->N < (1L << 31) && (long)c->n_cand <= (long)c->num_beams * p->N, MVLT_ERR_ARG);
    if (p->epilogue & MVLT_EPI_BIAS) MVLT_CHECK(p->bias, MVLT_ERR_ARG);
    MVLT_CHECK(c->num_beams <= BEAM_MAXB && c->n_cand <= BEAM_MAXC, MVLT_ERR_UNSUPPORTED);
    MVLT_CHECK(!p->a_kmajor && !p->b_kmajor && (p->epilogue & ~(MVLT_EPI_BIAS)) == 0, MVLT_ERR_UNSUPPORTED);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int vec = (c->ldx % 4 == 0 && aligned16(c->x)) ? 1 : 0;
    const int rc = by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        for (int pass = 0; pass < 2; ++pass) {          // 0: check every chunk, 1: launch
            for (int r0 = 0; r0 < p->M; r0 += 64) {
                MvltGemm q = *p;
                q.M = p->M - r0 < 64 ? p->M - r0 : 64;
                q.A = reinterpret_cast<const T*>(p->A) + (long)r0 * p->lda;
                q.m_dev = nullptr;
                if (pass == 0) { MVLT_CHECK(skinny_ok<T>(&q), MVLT_ERR_UNSUPPORTED); continue; }
                LAUNCH_NRT(gemm_logits128_kernel, T, q.M, dim3(ceil_div(parts_of(&q), SKINNY_WAVES)), dim3(64 * SKINNY_WAVES), s, skinny_dev(&q),
                           c->x + (long)r0 * c->ldx, (long)c->ldx, vec, 1.0f);
            }
        }
        return (int)MVLT_OK;
    });
    if (rc != MVLT_OK) return rc;
    const BeamIn bi{c->x, (long)c->ldx, c->beam_scores, c->num_beams, c->n_cand, p->N, c->cand_score, c->cand_beam, c->cand_tok, c->lse};
    if (r) hipLaunchKernelGGL(beam_candidates_kernel<RulesDev>, dim3(p->M / c->num_beams), dim3(BEAM_THREADS), 0, s, bi, *r);
    else hipLaunchKernelGGL(beam_candidates_kernel<>, dim3(p->M / c->num_beams), dim3(BEAM_THREADS), 0, s, bi);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
}  // namespace

extern "C" int mvlt_gemm_beam_candidates(const MvltGemm* p, const MvltBeamCand* c, void* stream) {
    return beam_candidates_entry(p, c, nullptr, stream);
}
extern "C" int mvlt_gemm_beam_candidates_rules(const MvltGemm* p, const MvltBeamCand* c, const MvltLogitRules* rules, void* stream) {
    RulesDev rd;          // RULES_OF without its 64 rows: M = G * num_beams, any size
    { MVLT_CHECK(p, MVLT_ERR_ARG); const int rc_ = rules_dev(rules, p->M, p->N, rd, 0x7FFFFFFF); if (rc_ != MVLT_OK) return rc_; }
    return beam_candidates_entry(p, c, &rd, stream);
}

extern "C" int mvlt_beam_rules_plan(const MvltLogitRules* r, const int32_t* seq, int64_t ld_seq, int rows, int V, void* stream) {
    MVLT_CHECK(r && r->seen && r->banned && r->col && seq, MVLT_ERR_ARG);
    MVLT_CHECK(rows >= 1 && V >= 1 && ld_seq >= 1 && r->ld_words >= (long)ceil_div(V, 32), MVLT_ERR_ARG);
    MVLT_CHECK(r->penalty > 0.f && r->ngram >= 0 && r->min_length >= 0, MVLT_ERR_ARG);
    const BeamRulesPlan f{r->seen, r->banned, (long)r->ld_words, seq, (long)ld_seq, r->col, r->ngram, r->min_length, r->eos_id, r->has_eos, V};
    hipLaunchKernelGGL(beam_rules_plan_kernel, dim3(rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), f);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_gemm_skinny_accum(const MvltGemm* p, float* acc, int k_splits, void* stream) {
    MVLT_CHECK(p && p->A && p->B && acc && k_splits >= 1 && k_splits <= 64, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->M <= 64 && p->N > 0 && p->K > 0 && !p->a_kmajor && !p->b_kmajor && p->epilogue == 0, MVLT_ERR_UNSUPPORTED);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = by_dtype(p->dtype, [&](auto t) -> int {
        using T = decltype(t);
        MVLT_CHECK(skinny_loads_ok<T>(p), MVLT_ERR_UNSUPPORTED);          // (split_k / a_colsum of the product are not looked at here)
        hipLaunchKernelGGL((gemm_skinny_accum_kernel<T>), dim3(ceil_div(p->N, 16), k_splits), dim3(64 * SKINNY_WAVES), 0, s, skinny_dev(p), acc);
        return (int)MVLT_OK;
    });
    if (rc != MVLT_OK) return rc;
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
