// Retrieval: the scoring head behind one encoder pass over a chunk of (image, caption) pairs, and the recall ranks of the score
// matrix (mvlt_retrieval_head, mvlt_recall_ranks, mvlt_recall_counts; include/mvlt_hip.h).
//
// Head.  A workgroup (8 waves) owns RB = 16 pairs -- one MFMA row tile.  The row block is small on purpose: a chunk is a few
// hundred pairs, so 16 rows give every chunk tens of workgroups, and the two H x H weight matrices (2.4 MB at H = 768) stay in L2
// for all of them.  LDS holds the gathered [CLS] rows and the block's intermediate, 2 x 16 x (H + 8) bf16 (66 KB at H = 1024 of the
// 160 KB a CU has); the 8-element row padding moves consecutive rows by one 16-byte slot, so the 16 lanes of a ds_read_b128 group
// (one row each, the same k) cover the 256-byte bank row once.  Wave w computes an eighth of the output columns in groups of NT = 3
// column tiles that share every activation fragment; a trip of the k loop issues the 6 weight loads of two k-blocks before their MFMAs
// (the loop waits on L2, not on the MFMA).  Weight fragments are read straight from global memory (lane 16 g + r: row n0 + r of
// W, k-slots 8 g .. 8 g + 7, the layout of v_mfma_f32_16x16x32_bf16) -- a row block reads each weight once,
// there is nothing to reuse through LDS.  With the weight as the FIRST MFMA operand, accumulator element q of lane 16 g + r is
// pair r, column n0 + 4 g + q: four consecutive columns per lane, one 8-byte store.
// Rounding points (the header states them): pooled and t1 once to bf16; LayerNorm, the two dot products and the softmax in f32.
//
// Ranks.  (score, index) pairs are compared as one 64-bit integer: an order-preserving 32-bit key of the score (NaN -> 0, below
// -inf; -0 -> +0) above the index, plus one so that 0 can stand for "no match".
#include "common.h"
#include <cmath>

namespace {

constexpr int RB = 16, NW = 8, NT = 3, PADE = 8;          // pairs per workgroup, waves, column tiles a wave keeps in flight

struct RHDev {
    int P, H; const int* p_dev;
    const bf16_t* hidden; int64_t ld; const int32_t* row_start;
    const bf16_t* w_pool; const float* b_pool; const bf16_t* w_tr; const float* b_tr;
    const float* gamma; const float* beta; float eps;
    const bf16_t* w_out; const float* b_out;
    const int64_t* out_index; float* scores;
    bf16_t* pooled; bf16_t* t1; float* logits;
};

// sOut[r][n] = round_bf16(act(sum_k sIn[r][k] W[n][k] + bias[n])) for the block's 16 rows and all H columns
template <bool GELU>
MVLT_DEV void head_product(const bf16_t* sIn, bf16_t* sOut, const bf16_t* W, const float* bias, bf16_t* gout, int H, int lds,
                           int p0, int P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int tiles = H / 16, per = (tiles + NW - 1) / NW;   // column tiles: wave w owns [w per, min((w + 1) per, tiles))
    const int first = wave * per, tpw = min(per, tiles - first);          // (<= 0: a wave without columns, H = 64)
    const bf16_t* xrow = sIn + r * lds + 8 * g;
    for (int t0 = 0; t0 < tpw; t0 += NT) {
        f32x4 acc[NT];
        const bf16_t* wp[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int tile = first + min(t0 + j, tpw - 1);          // past the wave's last tile: that tile again, result dropped
            wp[j] = W + (int64_t)(tile * 16 + r) * H + 8 * g;
        }
        for (int k0 = 0; k0 < H; k0 += 64) {                    // H % 64 == 0: two k-blocks per trip, all their loads issued first
            bf16x8 xa[2], wb[2][NT];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                xa[u] = *reinterpret_cast<const bf16x8*>(xrow + k0 + 32 * u);
#pragma unroll
                for (int j = 0; j < NT; ++j) wb[u][j] = *reinterpret_cast<const bf16x8*>(wp[j] + k0 + 32 * u);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < NT; ++j) Mma<bf16_t>::mma(acc[j], wb[u][j], xa[u]);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (t0 + j < tpw) {
                const int n = (first + t0 + j) * 16 + 4 * g;
                f32x4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float s = acc[j][q] + bias[n + q];
                    v[q] = GELU ? gelu_f(s) : tanhf(s);
                }
                store4f(sOut + r * lds + n, v);
                if (gout && p0 + r < P) store4f(gout + (int64_t)(p0 + r) * H + n, v);
            }
        }
    }
}

__global__ __launch_bounds__(64 * NW) void retrieval_head_kernel(const RHDev a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int H = a.H, lds = H + PADE;
    bf16_t* sX = reinterpret_cast<bf16_t*>(smem_raw);          // gathered [CLS] rows, then t1
    bf16_t* sP = sX + RB * lds;                                 // pooled
    const int P = a.p_dev ? min(a.P, max(*a.p_dev, 0)) : a.P;
    const int p0 = blockIdx.x * RB;
    if (p0 >= P) return;
    const int cpr = H / 8;                                      // 16-byte chunks per row
    for (int c = threadIdx.x; c < RB * cpr; c += 64 * NW) {
        const int r = c / cpr, k = (c - r * cpr) * 8;
        bf16x8 v = zero_vec<bf16_t>();                          // rows past the last pair: zeros (computed, never stored)
        if (p0 + r < P) v = *reinterpret_cast<const bf16x8*>(a.hidden + (int64_t)a.row_start[p0 + r] * a.ld + k);
        *reinterpret_cast<bf16x8*>(sX + r * lds + k) = v;
    }
    __syncthreads();
    head_product<false>(sX, sP, a.w_pool, a.b_pool, a.pooled, H, lds, p0, P);
    __syncthreads();
    head_product<true>(sP, sX, a.w_tr, a.b_tr, a.t1, H, lds, p0, P);
    __syncthreads();
    // f32 tail: a wave per row (RB / NW rows each), lane l takes the 4-column groups l, l + 64, ... (at most 4: H <= 1024)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int rr = 0; rr < RB / NW; ++rr) {
        const int r = wave * (RB / NW) + rr, p = p0 + r;
        if (p >= P) break;
        f32x4 x[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 4 * lane + 256 * i;
            x[i] = n < H ? load4f(sX + r * lds + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            s += (x[i][0] + x[i][1]) + (x[i][2] + x[i][3]);
        }
        const float mean = wave_sum(s) / (float)H;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * lane + 256 * i >= H) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) { x[i][q] -= mean; ss += x[i][q] * x[i][q]; }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)H + a.eps);
        float l0 = 0.f, l1 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = 4 * lane + 256 * i;
            if (n >= H) continue;
            const f32x4 w0 = load4f(a.w_out + n), w1 = load4f(a.w_out + H + n);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y = x[i][q] * rstd * a.gamma[n + q] + a.beta[n + q];
                l0 += y * w0[q];
                l1 += y * w1[q];
            }
        }
        l0 = wave_sum(l0) + a.b_out[0];
        l1 = wave_sum(l1) + a.b_out[1];
        if (lane == 0) {
            const float m = fmaxf(l0, l1);
            const float e0 = expf(l0 - m), e1 = expf(l1 - m);
            a.scores[a.out_index[p]] = e1 / (e0 + e1);
            if (a.logits) { a.logits[2 * p] = l0; a.logits[2 * p + 1] = l1; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- ranks
MVLT_DEV uint32_t score_key(float s) {
    if (s != s) return 0u;                                      // NaN: below everything, -inf (key 0x007fffff) included
    const uint32_t b = __float_as_uint(s + 0.0f);               // -0 + +0 = +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
MVLT_DEV unsigned long long packed(float s, int idx) {          // never 0: 0 = "no match"
    return (((unsigned long long)score_key(s) << 32) | (uint32_t)idx) + 1ull;
}
MVLT_DEV unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const unsigned long long u = ((unsigned long long)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return v;
}
MVLT_DEV int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a workgroup per row i: threads along the row
__global__ __launch_bounds__(256) void rank_rows_kernel(const float* scores, int64_t ld, int Nc, const int64_t* ig, const int64_t* cg,
                                                        int32_t* rank) {
    __shared__ unsigned long long best_s[4];
    __shared__ int cnt_s[4];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = scores + (int64_t)i * ld;
    const int64_t grp = ig[i];
    unsigned long long best = 0ull;
    for (int j = threadIdx.x; j < Nc; j += 256)
        if (cg[j] == grp) { const unsigned long long v = packed(row[j], j); best = v > best ? v : best; }
    best = wave_max_u64(best);
    if (lane == 0) best_s[wave] = best;
    __syncthreads();
    best = best_s[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = best_s[w] > best ? best_s[w] : best;
    if (best == 0ull) { if (threadIdx.x == 0) rank[i] = Nc; return; }
    int c = 0;
    for (int j = threadIdx.x; j < Nc; j += 256) c += packed(row[j], j) > best ? 1 : 0;
    c = wave_sum_i(c);
    if (lane == 0) cnt_s[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) rank[i] = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
}

// a workgroup per 64 columns: lane = column (a wave reads 256 contiguous bytes of a row), wave w takes the rows w, w + 4, ...
__global__ __launch_bounds__(256) void rank_cols_kernel(const float* scores, int64_t ld, int Ni, int Nc, const int64_t* ig,
                                                        const int64_t* cg, int32_t* rank) {
    __shared__ unsigned long long best_s[4][64];
    __shared__ int cnt_s[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const bool live = j < Nc;
    const int64_t grp = live ? cg[j] : 0;
    unsigned long long best = 0ull;
    if (live)
        for (int i = wave; i < Ni; i += 4)
            if (ig[i] == grp) { const unsigned long long v = packed(scores[(int64_t)i * ld + j], i); best = v > best ? v : best; }
    best_s[wave][lane] = best;
    __syncthreads();
    best = best_s[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = best_s[w][lane] > best ? best_s[w][lane] : best;
    int c = 0;
    if (live && best != 0ull)
        for (int i = wave; i < Ni; i += 4) c += packed(scores[(int64_t)i * ld + j], i) > best ? 1 : 0;
    cnt_s[wave][lane] = c;
    __syncthreads();
    if (wave == 0 && live) rank[j] = best == 0ull ? Ni : cnt_s[0][lane] + cnt_s[1][lane] + cnt_s[2][lane] + cnt_s[3][lane];
}

struct Ks { int32_t k[8]; };
__global__ __launch_bounds__(1024) void recall_counts_kernel(const int32_t* rank, int n, Ks ks, int nk, int32_t* counts) {
    __shared__ int red[8][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int r = rank[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) c[k] += (k < nk && r < ks.k[k]) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int s = wave_sum_i(c[k]); if (lane == 0) red[k][wave] = s; }
    __syncthreads();
    if ((int)threadIdx.x < nk) {
        int s = 0;
        for (int w = 0; w < 16; ++w) s += red[threadIdx.x][w];
        counts[threadIdx.x] = s;
    }
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int mvlt_retrieval_head_supported(int dtype, int H) {
    return dtype == MVLT_BF16 && H >= 64 && H <= 1024 && H % 64 == 0;
}

extern "C" int mvlt_retrieval_head(const MvltRetrievalHead* p, void* stream) {
    MVLT_CHECK(p && p->hidden && p->row_start && p->w_pool && p->b_pool && p->w_tr && p->b_tr && p->ln_gamma && p->ln_beta &&
               p->w_out && p->b_out && p->out_index && p->scores, MVLT_ERR_ARG);
    MVLT_CHECK(p->P > 0 && p->H > 0 && p->ld_hidden >= p->H, MVLT_ERR_ARG);
    MVLT_CHECK(mvlt_retrieval_head_supported(p->dtype, p->H), MVLT_ERR_UNSUPPORTED);
    MVLT_CHECK(aligned16(p->hidden) && p->ld_hidden % 8 == 0 && aligned16(p->w_pool) && aligned16(p->w_tr) && aligned_to(p->w_out, 8) &&
               (!p->pooled || aligned16(p->pooled)) && (!p->t1 || aligned16(p->t1)), MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(p->row_start, 4) && aligned_to(p->out_index, 8) && aligned_to(p->scores, 4) && aligned_to(p->b_pool, 4) &&
               aligned_to(p->b_tr, 4) && aligned_to(p->ln_gamma, 4) && aligned_to(p->ln_beta, 4) && aligned_to(p->b_out, 4) &&
               (!p->logits || aligned_to(p->logits, 4)) && (!p->p_dev || aligned_to(p->p_dev, 4)), MVLT_ERR_ARG);
    RHDev a;
    a.P = p->P; a.H = p->H; a.p_dev = p->p_dev;
    a.hidden = static_cast<const bf16_t*>(p->hidden); a.ld = p->ld_hidden; a.row_start = p->row_start;
    a.w_pool = static_cast<const bf16_t*>(p->w_pool); a.b_pool = p->b_pool;
    a.w_tr = static_cast<const bf16_t*>(p->w_tr); a.b_tr = p->b_tr;
    a.gamma = p->ln_gamma; a.beta = p->ln_beta; a.eps = p->ln_eps;
    a.w_out = static_cast<const bf16_t*>(p->w_out); a.b_out = p->b_out;
    a.out_index = p->out_index; a.scores = p->scores;
    a.pooled = static_cast<bf16_t*>(p->pooled); a.t1 = static_cast<bf16_t*>(p->t1); a.logits = p->logits;
    const size_t sh = (size_t)2 * RB * (p->H + PADE) * sizeof(bf16_t);
    static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(retrieval_head_kernel),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)((size_t)2 * RB * (1024 + PADE) * sizeof(bf16_t))) == hipSuccess;
    MVLT_CHECK(attr_ok || sh <= 64 * 1024, MVLT_ERR_LAUNCH);
    hipLaunchKernelGGL(retrieval_head_kernel, dim3(ceil_div(p->P, RB)), dim3(64 * NW), sh, reinterpret_cast<hipStream_t>(stream), a);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_recall_ranks(const float* scores, int64_t ld, int Ni, int Nc, const int64_t* image_group,
                                 const int64_t* caption_group, int32_t* i2t_rank, int32_t* t2i_rank, void* stream) {
    MVLT_CHECK(scores && image_group && caption_group && i2t_rank && t2i_rank, MVLT_ERR_ARG);
    MVLT_CHECK(Ni > 0 && Nc > 0 && ld >= Nc, MVLT_ERR_ARG);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rank_rows_kernel, dim3(Ni), dim3(256), 0, s, scores, ld, Nc, image_group, caption_group, i2t_rank);
    MVLT_LAUNCH_CHECK();
    hipLaunchKernelGGL(rank_cols_kernel, dim3(ceil_div(Nc, 64)), dim3(256), 0, s, scores, ld, Ni, Nc, image_group, caption_group,
                       t2i_rank);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_recall_counts(const int32_t* rank, int n, const int32_t* ks, int nk, int32_t* counts, void* stream) {
    MVLT_CHECK(rank && ks && counts && n > 0 && nk >= 1 && nk <= 8, MVLT_ERR_ARG);
    Ks k{};
    for (int i = 0; i < nk; ++i) k.k[i] = ks[i];
    hipLaunchKernelGGL(recall_counts_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), rank, n, k, nk, counts);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
