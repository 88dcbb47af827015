// Host-side pieces shared by gemm.hip (which routes) and skinny.hip (which runs the M <= 64 products); gemm_dev.h stays device-only.
#pragma once
#include "common.h"

// M <= 64, both operands k-contiguous, whole k-blocks, no split requested -> gemm_skinny_kernel (alignment permitting)
template <typename T>
static bool is_skinny(const MvltGemm* p) {
    return p->M <= 64 && !p->a_kmajor && !p->b_kmajor && p->K % Mma<T>::KB == 0 && p->split_k <= 1 && !p->a_colsum;
}

// The skinny kernels walk whole k-blocks with 16-byte fragment loads straight from global memory: a K that is not a multiple of
// the k-block would silently lose its tail, an unaligned base or row stride would fault.
template <typename T>
static bool skinny_loads_ok(const MvltGemm* p) {
    constexpr int E = TypeInfo<T>::E;
    return p->K % Mma<T>::KB == 0 && p->lda % E == 0 && p->ldb % E == 0 && aligned16(p->A) && aligned16(p->B);
}

// Route probe (mvlt_gemm_route / mvlt_gemm_group_route): every launcher of the GEMM dispatch takes an `int* route`.  Null: it
// launches.  Non-null: it takes exactly the same decisions, writes the MvltGemmRoute it WOULD launch (k-slice count in the bits
// above MVLT_GEMM_ROUTE_KIND_BITS) instead of launching, touches neither the device nor the stream, and returns as if it had
// launched.  One decision, two uses: there is no second copy of any eligibility condition.
static inline int gemm_route_code(int kind, int slices) { return kind | ((slices > 1 ? slices : 1) << MVLT_GEMM_ROUTE_KIND_BITS); }

// skinny.hip: launches gemm_skinny_kernel<T, false> on the filled kernel argument block when the product is skinny and its
// operands can be loaded 16 bytes at a time; 1 = taken, 0 = not eligible (the tile kernels run), -1 = launch error
extern "C" __attribute__((visibility("hidden"))) int mvlt_skinny_try(const MvltGemm* p, const void* dev_block, void* stream, int* route);
