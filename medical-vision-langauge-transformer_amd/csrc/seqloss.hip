// Sequence-level loss on decoded id rows (self-critical / reward-weighted fine-tuning; include/mvlt_hip.h):
//   mvlt_seq_loss_plan     id rows -> lengths, teacher-forcing ids and the packed labelled-row plan with a weight per row
//   mvlt_seq_loss_fwd      sum of weight * (lse - x_label) over the packed rows, fixed order
//   mvlt_ce_bwd_weighted   dlogits = c_i * (softmax - onehot) with a coefficient per row
//
// The plan is one workgroup (B * T <= 2 M positions, a few microseconds at the workload's 32 x 150): every position is looked at
// independently and the first [END] / first PAD of a row meet in LDS by integer atomicMin (order-free, so stateless and
// reproducible); a scored row is a prefix, so its slots are off_b + t and nothing has to be partitioned.
//
// The backward streams the logits once in and once out (0.3 GB each way at 4800 x 30528 bf16): 16 bytes per lane and access, two
// independent vectors in flight per thread and trip, lse / coefficient / label uniform over the workgroup's row, no LDS, 30
// VGPRs (28 in f32), so a CU holds 8 workgroups of 256 threads; the grid is rows x column slices capped at 2048 workgroups
// (8 per CU), the rows beyond it are taken by striding.  With few rows the columns are sliced so that every CU still gets work.
#include "common.h"

namespace {

constexpr int PLAN_T = 1024, PLAN_MAXB = 4096, PLAN_MAXT = 512;

__global__ __launch_bounds__(PLAN_T) void seq_plan_kernel(const int64_t* ids, long ld, int B, int T, long eos, const float* w,
                                                          long ws_b, long ws_t, int row0, int row_step, int* len,
                                                          int64_t* tf_ids, int* gather_row, int64_t* sel_labels,
                                                          float* row_weight, int* rows_dev) {
    __shared__ int first_eos[PLAN_MAXB];           // later: off_b, the exclusive prefix sum of len
    __shared__ int first_pad[PLAN_MAXB];           // later: len_b
    __shared__ int part[PLAN_T];
    __shared__ int total;
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += PLAN_T) { first_eos[b] = T; first_pad[b] = T; }
    __syncthreads();
    const long n = (long)B * T;
    for (long i = tid; i < n; i += PLAN_T) {
        const int b = (int)(i / T), t = (int)(i - (long)b * T);
        const int64_t id = ids[(long)b * ld + t];
        if (eos >= 0 && id == eos) atomicMin(&first_eos[b], t);
        if (id <= 0) atomicMin(&first_pad[b], t);
    }
    __syncthreads();
    // len_b, then its exclusive prefix sum: every thread owns `per` consecutive samples, thread 0 scans the 1024 partial sums
    const int per = (B + PLAN_T - 1) / PLAN_T;
    const int lo = min(tid * per, B), hi = min(lo + per, B);
    int c = 0;
    for (int b = lo; b < hi; ++b) {
        const int l = first_eos[b] < T ? first_eos[b] + 1 : first_pad[b];
        first_pad[b] = l;
        len[b] = l;
        c += l;
    }
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int t = 0; t < PLAN_T; ++t) { const int v = part[t]; part[t] = acc; acc += v; }
        total = acc;
        rows_dev[0] = acc;
    }
    __syncthreads();
    int off = part[tid];
    for (int b = lo; b < hi; ++b) { first_eos[b] = off; off += first_pad[b]; }
    __syncthreads();
    const int N = total;
    for (long i = tid; i < n; i += PLAN_T) {
        const int b = (int)(i / T), t = (int)(i - (long)b * T);
        const int l = first_pad[b], o = first_eos[b];
        const int row = row0 + b * row_step + t;
        if (t < l) {
            // scored: slot off_b + t.  A negative id inside the prefix (only possible ahead of an [END]) has no token to score:
            // it keeps its slot with an ignored label and weight 0 and enters the encoder as PAD.
            const int64_t id = ids[(long)b * ld + t];
            const int slot = o + t;
            gather_row[slot] = row;
            sel_labels[slot] = id >= 0 ? id : -100;
            row_weight[slot] = id >= 0 ? w[(long)b * ws_b + (long)t * ws_t] : 0.f;
            tf_ids[i] = id >= 0 ? id : 0;
        } else {
            // behind the end: after all N scored slots, in (b, t) order -- (b T + t) - (off_b + len_b) unscored positions precede it
            const int slot = N + (int)(i - (long)(o + l));
            gather_row[slot] = row;
            sel_labels[slot] = -100;
            row_weight[slot] = 0.f;
            tf_ids[i] = 0;
        }
    }
}

__global__ __launch_bounds__(1024) void seq_loss_fwd_kernel(const float* lse, const float* x_label, const float* row_weight,
                                                            int rows, const int* rows_dev, float* acc) {
    __shared__ float red[1024];
    const int n = rows_dev ? max(0, min(rows, *rows_dev)) : rows;
    float s = 0.f;
    // every operation rounds on its own (no contraction into an fma): the sum is a stated sequence of f32 operations
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float w = row_weight[i];
        if (w != 0.f) s = __fadd_rn(s, __fmul_rn(w, __fsub_rn(lse[i], x_label[i])));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { acc[0] = red[0]; acc[1] = (float)n; }
}

template <typename T> struct Vec16;
template <> struct Vec16<float>  { using V = f32x4;  static constexpr int E = 4; };
template <> struct Vec16<bf16_t> { using V = bf16x8; static constexpr int E = 8; };

// E consecutive gradient elements from E logits: the expression of ce_bwd_kernel with the row's coefficient in place of its scale
template <typename T>
MVLT_DEV typename Vec16<T>::V ce_vec(const typename Vec16<T>::V x, int c, int V, float l, float ci, long lab) {
    typename Vec16<T>::V g;
#pragma unroll
    for (int e = 0; e < Vec16<T>::E; ++e)
        g[e] = from_f<T>((c + e < V) ? ci * (__expf(to_f(x[e]) - l) - ((long)(c + e) == lab ? 1.f : 0.f)) : 0.f);
    return g;
}

// grid (row slots, column slices); VEC: ld is a multiple of 16 bytes and both pointers are 16-byte aligned
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void ce_bwd_weighted_kernel(const T* logits, long ld, int rows, int V, const int64_t* labels,
                                                             const float* lse, const float* row_weight, const float* count,
                                                             float gscale, const float* gscale_dev, T* dl, const int* rows_dev) {
    using VT = typename Vec16<T>::V;
    constexpr int E = Vec16<T>::E;
    const int n = rows_dev ? max(0, min(rows, *rows_dev)) : rows;     // rows at or beyond it: neither read nor written
    if (gscale_dev) gscale *= gscale_dev[0];
    const float sc = gscale / fmaxf(count[0], 1.0f);                  // the scalar of ce_bwd_kernel, formed the same way
    const int stride = gridDim.y * 256;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const long lab = labels[r];
        const float w = row_weight[r];
        const bool live = lab >= 0 && w != 0.f;                        // otherwise the row is zeros and its logits are not read
        const float ci = sc * w;
        const float l = live ? lse[r] : 0.f;
        const T* x = logits + (long)r * ld;
        T* d = dl + (long)r * ld;
        if (VEC) {
            const int nv = (int)(ld / E);
            const VT z = zero_vec<T>();
            for (int v = blockIdx.y * 256 + threadIdx.x; v < nv; v += 2 * stride) {
                const int v1 = v + stride;
                const bool two = v1 < nv;
                VT a = z, b = z;
                if (live) {
                    a = reinterpret_cast<const VT*>(x)[v];
                    if (two) b = reinterpret_cast<const VT*>(x)[v1];
                    a = ce_vec<T>(a, v * E, V, l, ci, lab);
                    if (two) b = ce_vec<T>(b, v1 * E, V, l, ci, lab);
                }
                reinterpret_cast<VT*>(d)[v] = a;
                if (two) reinterpret_cast<VT*>(d)[v1] = b;
            }
        } else {
            for (long c = blockIdx.y * 256 + threadIdx.x; c < ld; c += stride) {
                float g = 0.f;
                if (live && c < V) g = ci * (__expf(to_f(x[c]) - l) - (c == lab ? 1.f : 0.f));
                d[c] = from_f<T>(g);
            }
        }
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int mvlt_seq_loss_plan(const int64_t* ids, int64_t ld, int B, int T, int64_t eos, const float* weights,
                                  int64_t w_stride_b, int64_t w_stride_t, int row0, int row_step, int32_t* len, int64_t* tf_ids,
                                  int32_t* gather_row, int64_t* sel_labels, float* row_weight, int32_t* rows_dev, void* stream) {
    MVLT_CHECK(ids && weights && len && tf_ids && gather_row && sel_labels && row_weight && rows_dev, MVLT_ERR_ARG);
    MVLT_CHECK(B >= 1 && B <= PLAN_MAXB && T >= 1 && T <= PLAN_MAXT && ld >= T, MVLT_ERR_ARG);
    MVLT_CHECK(w_stride_b >= 0 && w_stride_t >= 0 && row0 >= 0 && row_step >= 0, MVLT_ERR_ARG);
    MVLT_CHECK((int64_t)row0 + (int64_t)(B - 1) * row_step + (T - 1) <= INT32_MAX, MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(ids, 8) && aligned_to(tf_ids, 8) && aligned_to(sel_labels, 8) && aligned_to(weights, 4) &&
               aligned_to(len, 4) && aligned_to(gather_row, 4) && aligned_to(row_weight, 4) && aligned_to(rows_dev, 4), MVLT_ERR_ARG);
    hipLaunchKernelGGL(seq_plan_kernel, dim3(1), dim3(PLAN_T), 0, STREAM(stream), ids, (long)ld, B, T, (long)eos, weights,
                       (long)w_stride_b, (long)w_stride_t, row0, row_step, len, tf_ids, gather_row, sel_labels, row_weight, rows_dev);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_seq_loss_fwd(const float* lse, const float* x_label, const float* row_weight, int rows,
                                 const int32_t* rows_dev, float* acc, void* stream) {
    MVLT_CHECK(lse && x_label && row_weight && acc && rows >= 1 && rows <= PLAN_MAXB * PLAN_MAXT, MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(lse, 4) && aligned_to(x_label, 4) && aligned_to(row_weight, 4) && aligned_to(acc, 4) &&
               aligned_to(rows_dev, 4), MVLT_ERR_ARG);
    hipLaunchKernelGGL(seq_loss_fwd_kernel, dim3(1), dim3(1024), 0, STREAM(stream), lse, x_label, row_weight, rows, rows_dev, acc);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

template <typename T>
static int launch_ce_bwd_weighted(const void* logits, int64_t ld, int rows, int V, const int64_t* labels, const float* lse,
                                  const float* row_weight, const float* count, float grad_scale, const float* grad_scale_dev,
                                  void* dlogits, const int32_t* rows_dev, void* stream) {
    constexpr int E = Vec16<T>::E;
    MVLT_CHECK(aligned_to(logits, sizeof(T)) && aligned_to(dlogits, sizeof(T)), MVLT_ERR_ARG);
    const bool vec = ld % E == 0;
    // a leading dimension of whole 16-byte vectors is the vector route's: there a misaligned base is refused, not demoted
    if (vec) MVLT_CHECK(aligned16(logits) && aligned16(dlogits), MVLT_ERR_ARG);
    // 8 workgroups per CU on 256 CUs; few rows: slice the columns (a slice = 256 threads x 2 vectors per trip) to fill them
    const int gx = rows < 2048 ? rows : 2048;
    const long trips = vec ? ceil_div(ld / E, 512) : ceil_div(ld, 256);
    long gy = 2048 / gx;
    if (gy > trips) gy = trips;
    if (gy < 1) gy = 1;
    const dim3 grid(gx, (unsigned)gy);
    if (vec)
        hipLaunchKernelGGL((ce_bwd_weighted_kernel<T, true>), grid, dim3(256), 0, STREAM(stream), (const T*)logits, (long)ld, rows, V,
                           labels, lse, row_weight, count, grad_scale, grad_scale_dev, (T*)dlogits, rows_dev);
    else
        hipLaunchKernelGGL((ce_bwd_weighted_kernel<T, false>), grid, dim3(256), 0, STREAM(stream), (const T*)logits, (long)ld, rows, V,
                           labels, lse, row_weight, count, grad_scale, grad_scale_dev, (T*)dlogits, rows_dev);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_ce_bwd_weighted(int dtype, const void* logits, int64_t ld, int rows, int V, const int64_t* labels,
                                    const float* lse, const float* row_weight, const float* count, float grad_scale,
                                    const float* grad_scale_dev, void* dlogits, const int32_t* rows_dev, void* stream) {
    MVLT_CHECK(logits && labels && lse && row_weight && count && dlogits, MVLT_ERR_ARG);
    MVLT_CHECK(rows >= 1 && V >= 1 && ld >= V && ld <= INT32_MAX, MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(labels, 8) && aligned_to(lse, 4) && aligned_to(row_weight, 4) && aligned_to(count, 4) &&
               aligned_to(grad_scale_dev, 4) && aligned_to(rows_dev, 4), MVLT_ERR_ARG);
    if (dtype == MVLT_F32)
        return launch_ce_bwd_weighted<float>(logits, ld, rows, V, labels, lse, row_weight, count, grad_scale, grad_scale_dev, dlogits,
                                             rows_dev, stream);
    if (dtype == MVLT_BF16)
        return launch_ce_bwd_weighted<bf16_t>(logits, ld, rows, V, labels, lse, row_weight, count, grad_scale, grad_scale_dev, dlogits,
                                              rows_dev, stream);
    return MVLT_ERR_UNSUPPORTED;
}
