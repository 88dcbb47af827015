// MLM decoder product with the cross-entropy forward in its epilogue (mvlt_mlm_head_ce, include/mvlt_hip.h).
//
// The product is the register-staged 64 x 128 tile loop of gemm_dev.h (gemm_mainloop: both dtypes, any K); this file is the epilogue
// and the two small launches behind it.  Nothing here reads logits back: the tile's accumulators get their bias, are rounded to
// the storage dtype (and optionally stored), and the (max, sum exp) statistics of a row's 128 columns are taken from those rounded
// values while they are still in registers.
//
// Accumulator layout (gemm_mainloop): wave (wm, wn) of the 2 x 2 owns rows wm 32 .. + 32 and columns wn 64 .. + 64 of the tile;
// acc[i][j][r] is row 16 i + (lane & 15), column 16 j + 4 (lane >> 4) + r of that quadrant.  A row of a quadrant therefore lives in
// the four lanes {l, l + 16, l + 32, l + 48}, 16 values each: the lane folds its 16 in (j, r) order, xor-16 / xor-32 exchanges fold
// the four lanes (every lane ends with the same bits), and the wn = 1 wave hands its pair to the wn = 0 wave through 512 bytes of
// LDS.  Every step has one fixed order, so the same operands give the same bits.
#include "common.h"
#include "gemm_dev.h"
#include "gemm_host.h"
#include <cmath>

namespace {

constexpr int HBM = 64, HBN = 128;

struct HeadCEDev {
    const int64_t* labels; float* lse; float* x_label; float* acc;
    f32x2* part;          // [M][nct]: (max, sum exp(x - max)) of row m over column tile t
    float* nll;           // [M]: the row's term of acc[0]
    int nct;
};

// (m, s) with m = -inf, s = 0 stands for "no column": exp(-inf - 0) = 0 keeps it out of every sum without a NaN
MVLT_DEV float finite_or_zero(float m) { return m == -INFINITY ? 0.f : m; }

template <typename T>
__global__ __launch_bounds__(256, 3) void headce_kernel(const GemmDev p_in, const HeadCEDev h) {
    constexpr int FM = HBM / 32, FN = HBN / 32;
    __shared__ __attribute__((aligned(16))) T sA[TileGeom<T, HBM, false>::ELEMS];
    __shared__ __attribute__((aligned(16))) T sB[TileGeom<T, HBN, false>::ELEMS];
    __shared__ f32x2 meet[HBM];
    const GemmDev p = effective<false>(p_in);          // ragged rows: tiles at or beyond *m_dev leave here, before any access
    const int gx = gridDim.x;
    const int gy = min((int)gridDim.y, (p.M + HBM - 1) / HBM);
    const int orig = blockIdx.y * gx + blockIdx.x;
    if (orig >= gx * gy) return;
    int by, bx;
    tile_coords(xcd_remap(orig, gx * gy), gx, gy, p.xcs, by, bx);
    f32x4 acc[FM][FN];
    gemm_mainloop<T, HBM, HBN, false, false, false>(p, bx, by, 0, sA, sB, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int mr = lane & 15, nq = 4 * (lane >> 4);
    const int V = p.N;
    const int nb = bx * HBN + wn * (HBN / 2) + nq;          // this lane's first column of fragment 0
    f32x4 bias_v[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int n = nb + 16 * j + r; bias_v[j][r] = n < V ? p.bias[n] : 0.f; }
    T* const C = reinterpret_cast<T*>(p.C);
    float row_m[FM], row_s[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int lr = wm * (HBM / 2) + 16 * i + mr;
        const int m = by * HBM + lr;
        const bool live = m < p.M;
        const int64_t lab = live ? h.labels[m] : -1;
        f32x4 x[FN];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n = nb + 16 * j;
            f32x4 xr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xr[r] = to_f(from_f<T>(acc[i][j][r] + bias_v[j][r]));          // what is stored is what is summed
                x[j][r] = n + r < V ? xr[r] : -INFINITY;
                mx = fmaxf(mx, x[j][r]);
                if (n + r < V && lab == (int64_t)(n + r)) h.x_label[m] = xr[r];
            }
            if (C && live && n < V) {
                T* o = C + (long)m * p.ldc + n;
                if (n + 4 <= V) store4f(o, xr);
                else for (int r = 0; r < 4; ++r) if (n + r < V) o[r] = from_f<T>(xr[r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float ms = finite_or_zero(mx);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += __expf(x[j][r] - ms);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        row_m[i] = mx; row_s[i] = s;
        if (wn == 1 && lane < 16) meet[lr] = f32x2{mx, s};
    }
    __syncthreads();
    if (wn == 0 && lane < 16) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int lr = wm * (HBM / 2) + 16 * i + mr;
            const int m = by * HBM + lr;
            const f32x2 o = meet[lr];
            const float mx = fmaxf(row_m[i], o[0]), ms = finite_or_zero(mx);
            const float s = row_s[i] * __expf(row_m[i] - ms) + o[1] * __expf(o[0] - ms);
            if (m < p.M) h.part[(long)m * h.nct + bx] = f32x2{mx, s};
        }
    }
}

MVLT_DEV int valid_rows(int M, const int* m_dev) { return m_dev ? min(M, max(*m_dev, 0)) : M; }

// one wave per row: the row's column-tile pairs, lane-strided in tile order, then a butterfly
__global__ __launch_bounds__(256) void headce_rows_kernel(const HeadCEDev h, int M, int V, const int* m_dev) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= valid_rows(M, m_dev)) return;
    const f32x2* pr = h.part + (long)row * h.nct;
    float mx = -INFINITY;
    for (int t = lane; t < h.nct; t += 64) mx = fmaxf(mx, pr[t][0]);
    mx = wave_max(mx);
    const float ms = finite_or_zero(mx);
    float s = 0.f;
    for (int t = lane; t < h.nct; t += 64) { const f32x2 v = pr[t]; s += v[1] * __expf(v[0] - ms); }
    s = wave_sum(s);
    if (lane == 0) {
        const float l = mx + logf(s);
        h.lse[row] = l;
        const int64_t lab = h.labels[row];
        h.nll[row] = lab < 0 ? 0.f : (lab < V ? l - h.x_label[row] : NAN);          // a label outside the vocabulary poisons the loss
    }
}

// acc = (sum of the labelled rows' terms, their number): thread t takes rows t, t + 1024, ... in order, then a tree in LDS
__global__ __launch_bounds__(1024) void headce_sum_kernel(const HeadCEDev h, int M, const int* m_dev) {
    __shared__ float red_s[1024], red_c[1024];
    const int rows = valid_rows(M, m_dev);
    float s = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < rows; r += 1024)
        if (h.labels[r] >= 0) { s += h.nll[r]; c += 1.f; }
    red_s[threadIdx.x] = s; red_c[threadIdx.x] = c;
    for (int o = 512; o > 0; o >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < o) { red_s[threadIdx.x] += red_s[threadIdx.x + o]; red_c[threadIdx.x] += red_c[threadIdx.x + o]; }
    }
    if (threadIdx.x == 0) { h.acc[0] = red_s[0]; h.acc[1] = red_c[0]; }
}

size_t part_bytes(int M, int V) { return ((size_t)M * ceil_div(V, HBN) * sizeof(f32x2) + 15) & ~(size_t)15; }
bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" size_t mvlt_mlm_head_ce_workspace_bytes(int M, int V) {
    if (M < 1 || V < 1) return 0;
    return part_bytes(M, V) + (size_t)M * sizeof(float);
}

extern "C" int mvlt_mlm_head_ce(const MvltGemm* p, const MvltHeadCE* h, void* stream) {
    MVLT_CHECK(p && h && p->A && p->B && p->bias, MVLT_ERR_ARG);
    MVLT_CHECK(h->labels && h->lse && h->x_label && h->acc && h->workspace, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->N > 0 && p->K > 0 && p->lda >= p->K && p->ldb >= p->K, MVLT_ERR_ARG);
    MVLT_CHECK(!p->a_kmajor && !p->b_kmajor && p->epilogue == MVLT_EPI_BIAS, MVLT_ERR_ARG);
    MVLT_CHECK(p->M <= 65535 * HBM, MVLT_ERR_ARG);
    MVLT_CHECK(!p->C || (p->ldc >= p->N && p->ldc % 4 == 0 && aligned16(p->C)), MVLT_ERR_ARG);
    MVLT_CHECK(p->dtype == MVLT_F32 || p->dtype == MVLT_BF16, MVLT_ERR_UNSUPPORTED);
    const int E = p->dtype == MVLT_BF16 ? 8 : 4;          // elements per 16-byte operand chunk
    MVLT_CHECK(aligned16(p->A) && aligned16(p->B) && p->lda % E == 0 && p->ldb % E == 0, MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(p->bias, 4) && aligned_to(h->lse, 4) && aligned_to(h->x_label, 4) && aligned_to(h->acc, 4) &&
               aligned_to(h->labels, 8) && (!p->m_dev || aligned_to(p->m_dev, 4)), MVLT_ERR_ARG);
    MVLT_CHECK(aligned16(h->workspace) && h->workspace_bytes >= mvlt_mlm_head_ce_workspace_bytes(p->M, p->N), MVLT_ERR_ARG);
    const int bke = 128 / (p->dtype == MVLT_BF16 ? 2 : 4);
    GemmDev d{};
    d.M = p->M; d.N = p->N; d.K = p->K;
    d.A = p->A; d.lda = p->lda; d.B = p->B; d.ldb = p->ldb; d.C = p->C; d.ldc = p->ldc;
    d.epi = MVLT_EPI_BIAS; d.bias = p->bias;
    d.split_k = 1; d.k_per_split = ceil_div(p->K, bke) * bke;
    d.a_vec = d.b_vec = 1;
    d.m_dev = p->m_dev;
    d.xcs = gemm_pick_xcs(p->M, p->N, HBM, HBN);
    HeadCEDev hd;
    hd.labels = h->labels; hd.lse = h->lse; hd.x_label = h->x_label; hd.acc = h->acc;
    hd.part = reinterpret_cast<f32x2*>(h->workspace);
    hd.nll = reinterpret_cast<float*>(reinterpret_cast<char*>(h->workspace) + part_bytes(p->M, p->N));
    hd.nct = ceil_div(p->N, HBN);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(hd.nct, ceil_div(p->M, HBM));
    if (p->dtype == MVLT_BF16) hipLaunchKernelGGL(headce_kernel<bf16_t>, grid, dim3(256), 0, s, d, hd);
    else hipLaunchKernelGGL(headce_kernel<float>, grid, dim3(256), 0, s, d, hd);
    MVLT_LAUNCH_CHECK();
    hipLaunchKernelGGL(headce_rows_kernel, dim3(ceil_div(p->M, 4)), dim3(256), 0, s, hd, p->M, p->N, p->m_dev);
    MVLT_LAUNCH_CHECK();
    hipLaunchKernelGGL(headce_sum_kernel, dim3(1), dim3(1024), 0, s, hd, p->M, p->m_dev);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
