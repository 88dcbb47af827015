// Host-side pieces shared by gemm.hip (which routes) and skinny.hip (which runs the M <= 64 products); gemm_dev.h stays device-only.
#pragma once
#include "common.h"
#include <cstdlib>

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

// Tile order (tile_coords, gemm_dev.h): the number of column groups that minimises what the eight L2s pull over the fabric,
// M * xcs (rows of A, every group re-reads its row band) + 8 N / xcs (columns of B); MVLT_XCD_CS = 1 turns it off, 2 / 4 / 8 force it
static inline int gemm_pick_xcs(int M, int N, int bm, int bn) {
    static const int xcs_env = [] { const char* e = getenv("MVLT_XCD_CS"); return e ? atoi(e) : 0; }();
    int xcs = 1;
    const int gx = ceil_div(N, bn), gy = ceil_div(M, bm);
    if (xcs_env > 1) { if (gx >= xcs_env) xcs = xcs_env; }
    else if (xcs_env == 0 && gx * gy >= 128) {
        long best = (long)M + 8L * N;
        for (int cs = 2; cs <= 8; cs *= 2)
            if (gx >= 2 * cs && gy >= 2 * (8 / cs)) {
                const long c = (long)M * cs + 8L * N / cs;
                if (c < best) { best = c; xcs = cs; }
            }
    }
    return xcs;
}
