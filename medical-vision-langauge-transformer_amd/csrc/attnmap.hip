// Attention maps of the MVLBert encoder (mvlt_attn_probs in include/mvlt_hip.h): the probabilities the fused
// attention never materialises, recomputed from the layer's qkv and the lse its forward saved -- the recomputation
// the backward kernels of attn.hip do internally, as a kernel of its own with a (query range) x (key range)
// selection, a mean over heads and a renormalisation over the selected keys.
//
// One workgroup of 4 waves = one (sequence, head or all heads, 64 selected queries); wave w owns queries
// 16 w .. 16 w + 15 of the tile.  The selected K rows of a head go through LDS once per workgroup ([key][d], padded
// rows, zeros past the range or the sequence); a wave reads the Q fragments of its 16 queries straight from global
// memory.  Scores are formed as in the forward (first operand = K rows, second = Q rows: a lane owns 4 keys per
// key tile of ONE query), so a row sum is in-register plus two xor-shuffles and every output row is finished by
// the wave that owns it: no atomics, no second launch.  With MVLT_ATTNMAP_HEAD_MEAN the workgroup walks the heads
// in order and sums their probabilities in registers.
//
// Arithmetic: the forward's own -- operands in the compute dtype, f32 MFMA accumulation over hd, scale and the additive
// mask term in f32, __expf(s - lse).  exp(-10000 + ...) and exp(-1e30) are exactly 0 in f32, so masked entries and
// keys a packed sequence does not have come out as 0.0f.
#include "common.h"
#include "attn_frag.h"

namespace {
using namespace mvlt_attn;

struct MapDev {
    int mode, nseq, L, nH;
    const void* qkv; const float* lse; float scale;
    const int64_t* text_ids; int T; const uint8_t* image_mask; int obj_end;
    const int* row_start; const int* seq_len;   // packed rows, or null
    int q0, nq, k0, nk, flags;
    float* out;
};

constexpr int MAP_KT_MAX = 13;                  // key tiles per launch: nk <= 208, the forward's own L range

template <typename T> constexpr int map_ld() { return 64 + (sizeof(T) == 2 ? 8 : 4); }     // LDS row stride (elements)
static size_t map_smem(int nk, size_t es, int ld) {
    const size_t rows = 16 * (size_t)ceil_div(nk, 16);
    return rows * ld * es + rows * sizeof(float);
}

template <typename T, int KT>
__global__ __launch_bounds__(256) void attn_probs_kernel(const MapDev p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using M = Mma<T>;
    using Vec = typename TypeInfo<T>::Vec;
    constexpr int E = TypeInfo<T>::E, CPR = 64 / E, KBD = 64 / M::KB, LD = map_ld<T>();
    const int nt = (p.nk + 15) >> 4, rows = 16 * nt;                 // key tiles in use (<= KT), LDS rows
    T* kimg = reinterpret_cast<T*>(smem_raw);
    float* kmask = reinterpret_cast<float*>(smem_raw + (size_t)rows * LD * sizeof(T));
    const int seq = blockIdx.x;
    const bool mean = (p.flags & MVLT_ATTNMAP_HEAD_MEAN) != 0, renorm = (p.flags & MVLT_ATTNMAP_RENORM) != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c15 = lane & 15;
    const int C = p.nH * 64;
    const long rs = p.row_start ? (long)p.row_start[seq] : (long)seq * p.L;
    const int Ls = p.seq_len ? p.seq_len[seq] : p.L;
    const int qi = 64 * blockIdx.z + 16 * wave + c15;               // this lane's query, as an index into the selection
    const int q = p.q0 + qi;
    const bool qok = qi < p.nq && q < Ls;                            // a query the sequence has: otherwise a row of zeros
    const T* base = reinterpret_cast<const T*>(p.qkv) + rs * 3 * C;

    // additive key term of the selected keys: 0, -10000 (BIDIR: padded text, image_mask == 0) or NEG_BIG (past the range / the sequence)
    for (int r = threadIdx.x; r < rows; r += 256) {
        const int k = p.k0 + r;
        float m = 0.0f;
        if (r >= p.nk || k >= Ls) m = NEG_BIG;
        else if (p.mode == MVLT_ATTN_BIDIR) {
            const int n_img = p.obj_end - 1;
            bool ok = true;
            if (k >= 1 && k <= n_img) ok = p.image_mask ? p.image_mask[(long)seq * n_img + k - 1] != 0 : true;
            else if (k > p.obj_end) ok = p.text_ids[(long)seq * p.T + (k - p.obj_end - 1)] > 0;
            m = ok ? 0.0f : -10000.0f;
        }
        kmask[r] = m;
    }

    f32x4 tot[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) tot[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int h0 = mean ? 0 : (int)blockIdx.y, h1 = mean ? p.nH : h0 + 1;
    for (int h = h0; h < h1; ++h) {
        // this lane's query: Q fragments and lse (the lse of a query the sequence does not have is never read)
        typename M::Frag fq[KBD];
#pragma unroll
        for (int kb = 0; kb < KBD; ++kb)
            fq[kb] = qok ? *reinterpret_cast<const Vec*>(base + (long)q * 3 * C + h * 64 + kb * M::KB + g * E) : zero_vec<T>();
        const float lse_q = qok ? p.lse[((long)seq * p.nH + h) * p.L + q] : 0.0f;
        __syncthreads();                                            // the previous head's K image has been read
        for (int idx = threadIdx.x; idx < rows * CPR; idx += 256) {
            const int r = idx / CPR, ch = idx % CPR, k = p.k0 + r;
            Vec v = zero_vec<T>();
            if (r < p.nk && k < Ls) v = *reinterpret_cast<const Vec*>(base + (long)k * 3 * C + C + h * 64 + ch * E);
            *reinterpret_cast<Vec*>(kimg + r * LD + ch * E) = v;
        }
        __syncthreads();
        f32x4 acc[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < nt) {
#pragma unroll
                for (int kb = 0; kb < KBD; ++kb)
                    M::mma(acc[t], frag_rowmajor<T>(kimg, LD, 16 * t, kb * M::KB), fq[kb]);
            }
        }
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pr = 0.0f;
                if (t < nt && qok) {
                    const int r = 16 * t + 4 * g + j, k = p.k0 + r;
                    float b = kmask[r];
                    if (p.mode == MVLT_ATTN_SEQ2SEQ && !(k <= q || k <= p.obj_end)) b += -10000.0f;
                    pr = __expf(acc[t][j] * p.scale + b - lse_q);
                }
                tot[t][j] += pr;                                     // one head, or the heads summed in head order
            }
    }
    float sum = 0.f;
    const float nheads = (float)p.nH;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (mean) tot[t][j] = tot[t][j] / nheads;
            sum += tot[t][j];
        }
    if (renorm) {                                                    // the four lanes of a query hold its whole row
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
    }
    if (qi < p.nq) {
        float* orow = p.out + (((long)seq * gridDim.y + blockIdx.y) * p.nq + qi) * p.nk;
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = 16 * t + 4 * g + j;
                if (t < nt && r < p.nk) orow[r] = (renorm && sum > 0.f) ? tot[t][j] / sum : tot[t][j];
            }
    }
}

template <typename T, int KT>
int launch_map(const MapDev& d, hipStream_t s) {
    const dim3 grid(d.nseq, (d.flags & MVLT_ATTNMAP_HEAD_MEAN) ? 1 : d.nH, ceil_div(d.nq, 64));
    hipLaunchKernelGGL((attn_probs_kernel<T, KT>), grid, dim3(256), map_smem(d.nk, sizeof(T), map_ld<T>()), s, d);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

template <typename T>
int dispatch_map(const MapDev& d, hipStream_t s) {
    const int nt = ceil_div(d.nk, 16);
    if (nt <= 5) return launch_map<T, 5>(d, s);
    if (nt <= 9) return launch_map<T, 9>(d, s);
    return launch_map<T, MAP_KT_MAX>(d, s);
}

}  // namespace

extern "C" int mvlt_attn_probs(const MvltAttn* p, int q0, int nq, int k0, int nk, int flags, float* out, void* stream) {
    MVLT_CHECK(p && p->qkv && p->lse && out, MVLT_ERR_ARG);
    MVLT_CHECK((flags & ~(MVLT_ATTNMAP_HEAD_MEAN | MVLT_ATTNMAP_RENORM)) == 0, MVLT_ERR_ARG);
    MVLT_CHECK(p->nseq > 0 && p->L > 0 && p->nH > 0 && p->nH <= 65535, MVLT_ERR_ARG);
    if (p->mode == MVLT_ATTN_SWIN) return MVLT_ERR_UNSUPPORTED;
    if (p->mode == MVLT_ATTN_BIDIR) MVLT_CHECK((p->T == 0 || p->text_ids) && p->T >= 0 && p->obj_end >= 1 && p->obj_end + 1 + p->T == p->L, MVLT_ERR_ARG);
    else if (p->mode == MVLT_ATTN_SEQ2SEQ) MVLT_CHECK(p->obj_end < p->L, MVLT_ERR_ARG);
    else return MVLT_ERR_ARG;
    MVLT_CHECK(q0 >= 0 && nq > 0 && (long)q0 + nq <= p->L && k0 >= 0 && nk > 0 && (long)k0 + nk <= p->L, MVLT_ERR_ARG);
    MVLT_CHECK(aligned16(p->qkv), MVLT_ERR_ARG);
    MVLT_CHECK((p->row_start == nullptr) == (p->seq_len == nullptr), MVLT_ERR_ARG);
    if (p->hd != 64 || nk > 16 * MAP_KT_MAX) return MVLT_ERR_UNSUPPORTED;
    MapDev d{};
    d.mode = p->mode; d.nseq = p->nseq; d.L = p->L; d.nH = p->nH;
    d.qkv = p->qkv; d.lse = p->lse; d.scale = p->scale;
    d.text_ids = p->text_ids; d.T = p->T; d.image_mask = p->image_mask; d.obj_end = p->obj_end;
    d.row_start = p->row_start; d.seq_len = p->seq_len;
    d.q0 = q0; d.nq = nq; d.k0 = k0; d.nk = nk; d.flags = flags; d.out = out;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (p->dtype == MVLT_F32) return dispatch_map<float>(d, s);
    if (p->dtype == MVLT_BF16) return dispatch_map<bf16_t>(d, s);
    return MVLT_ERR_UNSUPPORTED;
}
