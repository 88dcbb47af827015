// MFMA GEMM for gfx950 with fused epilogues (see include/mvlt_hip.h, MvltGemm).
//
// Structure: 256 threads = 4 waves (2 x 2), workgroup tile BM x BN, k-tile of
// 128 bytes per row (64 bf16 / 32 f32 = two MFMA k-blocks), register-staged
// double-buffered LDS (global loads for tile t+1 are issued before the MFMAs
// of tile t and written to the other LDS buffer after them: one barrier per
// k-tile).  k-contiguous operands use an XOR-swizzled [row][128 B] image read
// with ds_read_b128 (conflict-free); k-strided operands (dgrad weights, both
// wgrad operands) are staged as they lie in memory ([k][row], padded rows) and
// transposed for free by ds_read_b64_tr_b16 (bf16) when the fragment is read.
// The MFMA is issued as (B-fragment, A-fragment) so each lane owns 4
// consecutive n of one output row -> 8/16-byte epilogue loads and stores.
#include "common.h"
#include "gemm_dev.h"
#include "gemm_host.h"
#include <cstdio>
#include <cstdlib>

// gemm8.hip: 8-wave ping-pong kernel; takes the filled kernel argument block, returns 1 if it launched
extern "C" __attribute__((visibility("hidden"))) int mvlt_gemm8_try(const void* dev_blocks, int n, int a_kmajor, int b_kmajor, int big_only,
                                                                    float* const* colsum, void* ws, size_t ws_bytes, void* stream, int* route);
extern "C" __attribute__((visibility("hidden"))) size_t mvlt_gemm8_group_workspace(const void* dev_blocks, int n);
// row-streaming kernel for the HBM-bound Swin stage-0 / 1 products (rowstream.hip): 1 = taken, 0 = not eligible, -1 = error
extern "C" __attribute__((visibility("hidden"))) int mvlt_rowstream_try(const void* dev_block, int b_kmajor, void* stream, int* route);
// MVLT_G8: unset / 2 = automatic (single products that fill the chip with 256 x 256 tiles: MLM decoder, large batches),
// 0 = never, 1 = wherever it is eligible, weight-gradient groups included (experiments: slower than the 4-wave kernels on
// the B=32 step's mid-size products)
static int g8_mode() { const char* e = getenv("MVLT_G8"); return e ? atoi(e) : 2; }

namespace {

// What the tile epilogues (gemm_dev.h) do not take, fragment by fragment: k-slices (f32 slabs in the workspace for splitk_reduce_kernel, or
// with ATOMIC and p.atomic_out straight into the zeroed f32 output) and rows the vector epilogue cannot address (epilogue4).
// acc[i][j][r] <-> n = n_base + 16 j + 4 (lane >> 4) + r, m = m_base + 16 i + (lane & 15).  ATOMIC is compile time: the LDS-DMA
// kernel is never launched with atomic_out and does not test it.
template <typename T, bool ATOMIC, int FM, int FN>
MVLT_DEV void slow_tail(const GemmDev& p, const int m_base, const int n_base, const int bz, const f32x4 (&acc)[FM][FN]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int m = m_base + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n = n_base + j * 16 + 4 * (lane >> 4);
            if (ATOMIC && p.atomic_out) {
                // k-slices of one output tile meet in the f32 output itself (zeroed by the launcher): no slabs, no
                // reduce launch; the order of the 2..8 additions per element is not fixed (last-bit differences)
                if (m < p.M) {
                    float* c = reinterpret_cast<float*>(p.C) + (long)m * p.ldc + n;
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (n + r < p.N) atomicAdd(c + r, acc[i][j][r]);
                }
            } else if (p.split_k > 1) {
                if (m < p.M && n < p.N) {
                    float* w = p.ws + ((long)bz * p.M + m) * p.N + n;
                    if ((p.N & 3) == 0) store4f(w, acc[i][j]);
                    else for (int r = 0; r < 4; ++r) if (n + r < p.N) w[r] = acc[i][j][r];
                }
            } else {
                // MVLT_EPI_TAIL: rows at or beyond the count run the epilogue on a zero accumulator (gemm_dev.h tail_rows_zero)
                const bool dead = (p.epi & MVLT_EPI_TAIL) && m >= p.m_valid;
                epilogue4<T>(p, m, n, dead ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[i][j]);
            }
        }
    }
}

// one output tile (bx, by) of one k-split bz
template <typename T, int BM, int BN, bool AK, bool BK_, bool PF2, int DEEP = 0, bool WIDE = false>
MVLT_DEV void gemm_body(const GemmDev& p_in, const int bx, const int by, const int bz, T* sA, T* sB) {
    constexpr int FM = BM / 32, FN = BN / 32;
    const GemmDev& p = p_in;                     // (already the effective problem: see gemm_kernel / gemm_group_kernel)
    const int m0 = by * BM, n0 = bx * BN;
    if (m0 >= p.M) return;                       // (uniform per workgroup; only with m_dev)
    const int wm = (threadIdx.x >> 6) >> 1, wn = (threadIdx.x >> 6) & 1;
    f32x4 acc[FM][FN];
    if (!AK && m0 >= p.m_valid) {                // MVLT_EPI_TAIL only: a tile beyond the rows of A that exist skips its K loop
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        GemmDev pl = p;                          // the loop reads the rows of A that exist (m_valid == M without MVLT_EPI_TAIL)
        if (!AK) pl.M = p.m_valid;
        gemm_mainloop<T, BM, BN, AK, BK_, PF2, DEEP>(pl, bx, by, bz, sA, sB, acc);          // gemm_dev.h
    }

    if (!p.atomic_out && p.split_k <= 1 && p.epi_vec && (p.N & 3) == 0) {
        if constexpr (WIDE && sizeof(T) == 2 && FN % 2 == 0) tile_epilogue_wide<T, FM, FN>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), acc);
        else tile_epilogue<T, FM, FN>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), acc);          // loads hoisted out of the store sequence
    } else slow_tail<T, true>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), bz, acc);
}

// ---------------------------------------------------------------------------------------------------------------
// Both operands k-contiguous (every forward nn.Linear), bf16, K a multiple of 64: the tiles go global -> LDS by
// `global_load_lds_dwordx4` (LDS-DMA: no staging registers, no ds_write pass -- the register-staged loop spends
// about as long in ds_write_b128 as in MFMA), two LDS buffers, ONE barrier per k-tile: the DMA of tile t+1 is in
// flight while tile t is multiplied.  An LDS-DMA instruction writes wave-uniform base + lane * 16 bytes, so the
// XOR swizzle of the [row][128 B] image is applied to the per-lane SOURCE address (chunk' = chunk ^ (row & 7), the
// same involution tile_frag applies on the read side).
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

template <int R>
MVLT_DEV void glds_fill(const bf16_t* const (&src)[R / 32], bf16_t* lds_tile, int wave, long koff) {
#pragma unroll
    for (int j = 0; j < R / 32; ++j) {
        bf16_t* dst = lds_tile + (wave * (R / 32) + j) * 8 * 64;          // 8 rows x 64 elements = 1 KB per instruction
        __builtin_amdgcn_global_load_lds((glb_void_t*)(src[j] + koff), (lds_void_t*)dst, 16, 0, 0);
    }
}

// BKM: the B operand is k-major (dgrad: dx = dy W reads the [N_out, K_in] weight along its rows).  Its tile image is
// [64 k][BN] with the 32-byte units XOR-swizzled by kswz<BN>(k) (the layout tile_frag<T, BN, true> transposes out of with
// ds_read_b64_tr_b16); one LDS-DMA instruction covers 1 KB = 8 (BN = 64) / 4 (BN = 128) k-rows, the swizzle again on the
// source side.  With transposing reads in the loop the DMA is issued through inline asm (glds16, common.h).
template <int BM, int BN, bool BKM, bool WIDE, int NST = 2>
__global__ __launch_bounds__(256, 2) void gemm_glds_kernel(const GemmDev p_in) {
    using T = bf16_t;
    constexpr int BKE = 64, FM = BM / 32, FN = BN / 32;
    static_assert(!BKM || BN == 64 || BN == 128, "k-major B tiles: 64 or 128 columns");
    static_assert(NST >= 2 && NST <= 5 && (NST - 2) * (BM / 32 + BN / 32) < 64, "two to five LDS stages (counted vmcnt: 6 bits)");
    // NST stages; beyond the 64 KB a static array may have (160 x 128 tiles: 72 KB) the launcher passes dynamic LDS
    constexpr bool DYN = NST * (BM + BN) * BKE * sizeof(T) > 65536;
    extern __shared__ __attribute__((aligned(16))) char glds_dyn[];
    __shared__ __attribute__((aligned(16))) T glds_static[DYN ? 8 : NST * (BM + BN) * BKE];
    T* const smem = DYN ? reinterpret_cast<T*>(glds_dyn) : glds_static;
    const GemmDev p = effective<false>(p_in);
    const unsigned pfv = prefetch_lines(p_in);
    const int gx = gridDim.x;
    const int gy = min((int)gridDim.y, (p.M + BM - 1) / BM);
    const int orig = blockIdx.y * gx + blockIdx.x;
    if (orig >= gx * gy) return;
    int by, bx;
    tail_tile_order(orig, gx, gy, BM, p, by, bx);
    const int bz = blockIdx.z;
    const int m0 = by * BM, n0 = bx * BN;
    const int ks = bz * p.k_per_split;
    const int ke = min(p.K, ks + p.k_per_split);
    // MVLT_EPI_TAIL (m_valid < M): a tile beyond the rows of A that exist skips its K loop, one that straddles the count reads
    // clamped copies of the last valid row; the epilogue zeroes those accumulators (gemm_dev.h tail_rows_zero)
    const int nkt = m0 < p.m_valid ? (ke - ks) / BKE : 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wm = wave >> 1, wn = wave & 1;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    constexpr int STAGE = (BM + BN) * BKE;            // elements per LDS stage: A tile, then B tile
    // per-lane source pointers: instruction j of this wave covers tile rows 8 (wave R/32 + j) .. +8; lane = (row_in, chunk')
    const int rin = lane >> 3, chs = (lane & 7) ^ rin;
    const T* srcA[BM / 32];
    const T* srcB[BN / 32];
#pragma unroll
    for (int j = 0; j < BM / 32; ++j) {
        const int row = min(m0 + (wave * (BM / 32) + j) * 8 + rin, max(p.m_valid, 1) - 1);
        srcA[j] = A + (long)row * p.lda + ks + chs * 8;
    }
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) {
        if constexpr (BKM) {
            constexpr int KPI = 512 / BN;                                    // k-rows per instruction (1 KB / (BN * 2 B))
            constexpr int XM = BN / 8 - 1;                                   // 16-byte positions per k-row - 1
            const int krow = (wave * (BN / 32) + j) * KPI + lane / (BN / 8), x = lane & XM;
            const int ch = (((x >> 1) ^ kswz<BN>(krow)) << 1) | (x & 1);
            srcB[j] = B + (long)(ks + krow) * p.ldb + min(n0 + ch * 8, max(p.N - 8, 0));
        } else {
            const int row = min(n0 + (wave * (BN / 32) + j) * 8 + rin, p.N - 1);
            srcB[j] = B + (long)row * p.ldb + ks + chs * 8;
        }
    }
    const long kstep_b = BKM ? (long)BKE * p.ldb : (long)BKE;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) T*)smem;
    auto fill = [&](int stage, int kt) {
        const unsigned sa = lds0 + (unsigned)(stage * STAGE) * 2u, sb = sa + (unsigned)(BM * BKE) * 2u;
#pragma unroll
        for (int j = 0; j < BM / 32; ++j) glds16(srcA[j] + (long)kt * BKE, sa + (wave * (BM / 32) + j) * 1024);
#pragma unroll
        for (int j = 0; j < BN / 32; ++j) glds16(srcB[j] + kt * kstep_b, sb + (wave * (BN / 32) + j) * 1024);
    };
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < NST - 1; ++st) if (st < nkt) fill(st, st);
    constexpr int PER = BM / 32 + BN / 32;               // LDS-DMA requests per wave and K-tile
    for (int kt = 0; kt < nkt; ++kt) {
        // this wave's share of tile kt has landed (NST stages: the requests of the next NST - 2 tiles may still be in flight --
        // vmcnt completes in order, so a COUNTED wait leaves exactly those outstanding; fewer near the end of the reduction)
        const int ahead = min(NST - 2, nkt - 1 - kt);
        if (NST >= 5 && ahead >= 3) wait_vmcnt<(NST >= 5 ? 3 : 0) * PER>();
        else if (NST >= 4 && ahead == 2) wait_vmcnt<(NST >= 4 ? 2 : 0) * PER>();
        else if (NST >= 3 && ahead == 1) wait_vmcnt<(NST >= 3 ? 1 : 0) * PER>();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // everybody's has; everybody is done reading tile kt-1
        if (kt + NST - 1 < nkt) fill((kt + NST - 1) % NST, kt + NST - 1);
        const T* a = smem + (kt % NST) * STAGE;
        const T* b = a + BM * BKE;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            typename Mma<T>::Frag fa[FM], fb[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) fa[i] = tile_frag<T, BM, false>(a, wm * (BM / 2) + i * 16, kb);
#pragma unroll
            for (int j = 0; j < FN; ++j) fb[j] = tile_frag<T, BN, BKM>(b, wn * (BN / 2) + j * 16, kb);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) Mma<T>::mma(acc[i][j], fb[j], fa[i]);
        }
    }
    if (p.split_k <= 1 && p.epi_vec && (p.N & 3) == 0) {
        if constexpr (WIDE && sizeof(T) == 2 && FN % 2 == 0) tile_epilogue_wide<T, FM, FN>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), acc);
        else tile_epilogue<T, FM, FN>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), acc);          // loads hoisted out of the store sequence
    } else slow_tail<T, false>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), bz, acc);
    asm volatile("" :: "v"(pfv));
}

template <typename T, int BM, int BN, bool AK, bool BK_, bool PF2, bool WIDE = false>
__global__ __launch_bounds__(256, 3) void gemm_kernel(const GemmDev p) {
    __shared__ __attribute__((aligned(16))) T sA[TileGeom<T, BM, AK>::ELEMS];
    __shared__ __attribute__((aligned(16))) T sB[TileGeom<T, BN, BK_>::ELEMS];
    // ragged batches (m_dev): the tile list is the EFFECTIVE one -- the XCD remap deals contiguous chunks of it to the
    // XCDs, so remapping the upper-bound list would leave the XCDs that own the empty tail idle
    const GemmDev q = effective<AK>(p);
    const unsigned pfv = prefetch_lines(p);
    const int gx = gridDim.x;
    const int gy = AK ? (int)gridDim.y : min((int)gridDim.y, (q.M + BM - 1) / BM);
    const int orig = blockIdx.y * gx + blockIdx.x;
    if (orig < gx * gy) {
        int by, bx;
        tail_tile_order(orig, gx, gy, BM, q, by, bx);
        gemm_body<T, BM, BN, AK, BK_, PF2, 0, WIDE>(q, bx, by, blockIdx.z, sA, sB);
    }
    asm volatile("" :: "v"(pfv));
}

// ---------------------------------------------------------------------------------------------------------------
// Weight-gradient tile with BOTH operands k-major through LDS-DMA (round 6): dW[m, n] = sum_k dY[k, m] X[k, n].
// The register-staged form (gemm_body, DEEP = 2) keeps two register sets of the next tiles beside 64 accumulators: 243 VGPRs
// at 128 x 128, i.e. two waves per SIMD and NOTHING else resident on a CU that holds two such workgroups
// (profiles/r6_ln_bwd.md).  Here the tiles go global -> LDS by LDS-DMA in the k-major image the transposing fragment reads
// expect ([64 k][R] with the 32-byte units XOR-swizzled by kswz<R>(k), the swizzle applied to the per-lane SOURCE address
// exactly as gemm_glds_kernel<.., BKM> does for its B tile): no staging registers, no ds_write pass.
//   * K tail / ragged reductions (m_dev): k-rows at or beyond the reduction length are fetched from a page of
//     zeros (g_zero_page) instead of the operand (a per-lane pointer select per request), for BOTH operands (0 x NaN of an unwritten
//     tail row would poison the sum);
//   * bias gradient db[m] = sum_k dY[k, m]: on the matrix pipe, dY^T . 1 (one extra MFMA per A fragment and k-block in the
//     wn = 0 waves of the first column tile of every tile row; accumulator column 0 holds the sum) -- the staging registers
//     the register form sums from do not exist here;
//   * two LDS stages, one barrier per k-tile, counted by hand (the DMA is inline asm: common.h).
// The library's one page of device zeros (a request reads 16 lanes x 16 bytes of it); gemm8.hip takes its address from the
// host through mvlt_gemm_zero_page below.
__device__ __attribute__((aligned(256))) unsigned char g_zero_page[512];

template <int BM, int BN, int NST>
MVLT_DEV void wgrad_glds_tile(const GemmDev& p, const int bx, const int by, bf16_t* smem) {
    using T = bf16_t;
    constexpr int BKE = 64, FM = BM / 32, FN = BN / 32;
    static_assert((BM == 64 || BM == 128) && (BN == 64 || BN == 128), "k-major LDS-DMA tiles: 64 or 128 wide");
    const int m0 = by * BM, n0 = bx * BN;
    const int ke = p.K;
    const int nkt = (ke + BKE - 1) / BKE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wm = wave >> 1, wn = wave & 1;
    const T* A = reinterpret_cast<const T*>(p.A);
    const T* B = reinterpret_cast<const T*>(p.B);
    constexpr int STAGE = (BM + BN) * BKE;            // elements per LDS stage: A image [64][BM], then B image [64][BN]
    const T* srcA[BM / 32];
    const T* srcB[BN / 32];
    int krowA[BM / 32], krowB[BN / 32];
#pragma unroll
    for (int j = 0; j < BM / 32; ++j) {
        constexpr int KPI = 512 / BM, XM = BM / 8 - 1;
        const int krow = (wave * (BM / 32) + j) * KPI + lane / (BM / 8), x = lane & XM;
        const int ch = (((x >> 1) ^ kswz<BM>(krow)) << 1) | (x & 1);
        krowA[j] = krow;
        srcA[j] = A + (long)krow * p.lda + min(m0 + ch * 8, max(p.M - 8, 0));
    }
#pragma unroll
    for (int j = 0; j < BN / 32; ++j) {
        constexpr int KPI = 512 / BN, XM = BN / 8 - 1;
        const int krow = (wave * (BN / 32) + j) * KPI + lane / (BN / 8), x = lane & XM;
        const int ch = (((x >> 1) ^ kswz<BN>(krow)) << 1) | (x & 1);
        krowB[j] = krow;
        srcB[j] = B + (long)krow * p.ldb + min(n0 + ch * 8, max(p.N - 8, 0));
    }
    const T* zero = reinterpret_cast<const T*>(g_zero_page) + (lane & 15) * 8;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) T*)smem;
    auto fill = [&](int stage, int kt) {
        const unsigned sa = lds0 + (unsigned)(stage * STAGE) * 2u, sb = sa + (unsigned)(BM * BKE) * 2u;
        const int k0 = kt * BKE;
#pragma unroll
        for (int j = 0; j < BM / 32; ++j)
            glds16(k0 + krowA[j] < ke ? srcA[j] + (long)k0 * p.lda : zero, sa + (wave * (BM / 32) + j) * 1024);
#pragma unroll
        for (int j = 0; j < BN / 32; ++j)
            glds16(k0 + krowB[j] < ke ? srcB[j] + (long)k0 * p.ldb : zero, sb + (wave * (BN / 32) + j) * 1024);
    };
    f32x4 acc[FM][FN], cacc[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        cacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_colsum = p.a_colsum != nullptr && bx == 0 && wn == 0;          // (wave-uniform)
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.0f;
    static_assert(NST >= 2 && NST <= 4, "two to four LDS stages (four measured slower than three: not instantiated)");
    constexpr int PER = BM / 32 + BN / 32;                     // LDS-DMA requests per wave and k-tile
#pragma unroll
    for (int st = 0; st < NST - 1; ++st) if (st < nkt) fill(st, st);
    for (int kt = 0; kt < nkt; ++kt) {
        // this wave's share of tile kt has landed (NST stages: the requests of the next NST - 2 tiles may still be in flight -- counted)
        const int ahead = min(NST - 2, nkt - 1 - kt);
        if (NST >= 4 && ahead >= 2) wait_vmcnt<(NST >= 4 ? 2 : 0) * PER>();
        else if (NST >= 3 && ahead == 1) wait_vmcnt<(NST >= 3 ? 1 : 0) * PER>();
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // everybody's has; everybody is done reading tile kt - 1
        if (kt + NST - 1 < nkt) fill((kt + NST - 1) % NST, kt + NST - 1);
        const T* a = smem + (kt % NST) * STAGE;
        const T* b = a + BM * BKE;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            Mma<T>::Frag fa[FM], fb[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) fa[i] = tile_frag<T, BM, true>(a, wm * (BM / 2) + i * 16, kb);
#pragma unroll
            for (int j = 0; j < FN; ++j) fb[j] = tile_frag<T, BN, true>(b, wn * (BN / 2) + j * 16, kb);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) Mma<T>::mma(acc[i][j], fb[j], fa[i]);
            if (do_colsum) {
#pragma unroll
                for (int i = 0; i < FM; ++i) Mma<T>::mma(cacc[i], ones, fa[i]);
            }
        }
    }
    if (do_colsum && lane < 16) {
        // cacc[i][r] = sum_k A[k, m] for m = m0 + wm BM/2 + 16 i + lane (every r: the first operand's rows are all ones)
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int m = m0 + wm * (BM / 2) + i * 16 + lane;
            if (m < p.M) p.a_colsum[m] = (p.epi & MVLT_EPI_ACCUM) ? p.a_colsum[m] + cacc[i][0] : cacc[i][0];
        }
    }
    tile_epilogue<T, FM, FN>(p, m0 + wm * (BM / 2), n0 + wn * (BN / 2), acc);
    __syncthreads();                                           // (persistent callers refill stage 0)
}

// Several independent products in one launch (the weight gradients of one layer): the tile lists of the
// items are concatenated, a workgroup finds its item by a scan of the (<= 8) prefix counts.
constexpr int GROUP_MAX = 8;
struct GemmGroupDev { int n; int split; int start[GROUP_MAX + 1]; GemmDev g[GROUP_MAX]; };   // start[]: in (tile, k-slice) units

template <typename T, int BM, int BN, bool AK, bool BK_, int DEEP>
__global__ __launch_bounds__(256, 2) void gemm_group_kernel(const GemmGroupDev gp) {
    __shared__ __attribute__((aligned(16))) T sA[(DEEP == 2 ? 2 : 1) * TileGeom<T, BM, AK>::ELEMS];
    __shared__ __attribute__((aligned(16))) T sB[(DEEP == 2 ? 2 : 1) * TileGeom<T, BN, BK_>::ELEMS];
    // persistent: the grid may be smaller than the tile list (the launcher caps the workgroups per CU so the
    // dgrad chain on the main stream keeps most of every CU); gemm_body ends on a barrier, so LDS is reusable
    const int total = gp.start[gp.n];
    for (int t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
        const int t = xcd_remap(t0, total);
        int i = 0;
        while (i + 1 < gp.n && t >= gp.start[i + 1]) ++i;
        const GemmDev p = effective<AK>(gp.g[i]);
        const int gx = (p.N + BN - 1) / BN, gy = (p.M + BM - 1) / BM;
        const int local = t - gp.start[i];
        const int bz = local / (gx * gy), tile = local - bz * gx * gy;          // k-slice bz of output tile `tile`
        // the list runs along the SHORTER side of the tile grid first: the contiguous chunk of it that lands on one XCD (xcd_remap)
        // is then a block, not a sliver of a few rows x all columns -- a [768, 3072] gradient: 6 + 9 operand bands per L2 instead of 3 + 24
        int by, bx;
        if (gx > gy) { bx = tile / gy; by = tile - bx * gy; }
        else { by = tile / gx; bx = tile - by * gx; }
        gemm_body<T, BM, BN, AK, BK_, false, DEEP>(p, bx, by, bz, sA, sB);
    }
}

// the same list walked by the LDS-DMA tile (bf16, both operands k-major, no k-slices): ~150 instead of 243 VGPRs at 128 x 128
template <int BM, int BN, int NST>
__global__ __launch_bounds__(256, 2) void gemm_group_glds_kernel(const GemmGroupDev gp) {
    constexpr bool DYN = NST * (BM + BN) * 64 * 2 > 65536;
    extern __shared__ __attribute__((aligned(16))) char wg_dyn[];
    __shared__ __attribute__((aligned(16))) bf16_t wg_static[DYN ? 8 : NST * (BM + BN) * 64];
    bf16_t* const smem = DYN ? reinterpret_cast<bf16_t*>(wg_dyn) : wg_static;
    const int total = gp.start[gp.n];
    for (int t0 = blockIdx.x; t0 < total; t0 += gridDim.x) {
        const int t = xcd_remap(t0, total);
        int i = 0;
        while (i + 1 < gp.n && t >= gp.start[i + 1]) ++i;
        const GemmDev p = effective<true>(gp.g[i]);
        const int gx = (p.N + BN - 1) / BN, gy = (p.M + BM - 1) / BM;
        const int tile = t - gp.start[i];
        int by, bx;
        if (gx > gy) { bx = tile / gy; by = tile - bx * gy; }
        else { by = tile / gx; bx = tile - by * gx; }
        wgrad_glds_tile<BM, BN, NST>(p, bx, by, smem);
    }
}

// slabs -> output: 64 output quads per block, the slabs are shared out over 4 waves and combined in LDS
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmDev p_in) {
    __shared__ f32x4 red[4][64];
    GemmDev p = p_in;
    // m_dev counts the rows of a k-contiguous A (= rows of the output): slab rows beyond it were never written.  For a k-major
    // A (weight gradients) it is the reduction length and the output keeps all M rows.
    if (p.m_dev && !p.a_kmajor) p.M = min(p.M, max(*p.m_dev, 0));
    const int nq = (p.N + 3) / 4;
    const long total = (long)p.M * nq;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (long base = (long)blockIdx.x * 64; base < total; base += (long)gridDim.x * 64) {
        const long idx = base + lane;
        const bool ok = idx < total;
        const int m = ok ? (int)(idx / nq) : 0, n = ok ? (int)(idx % nq) * 4 : 0;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (ok) {
            if ((p.N & 3) == 0) {
                // eight slabs per round trip (a plain loop waits out one load latency per slab: 30 us for the 96 slices of
                // the patch-embedding weight gradient, at the very end of the backward pass), summed in slice order
                const long sstride = (long)p.M * p.N;
                const float* ws0 = p.ws + (long)m * p.N + n;
                for (int s = w; s < p.split_k; s += 32) {
                    f32x4 t[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int sj = s + 4 * j;
                        t[j] = sj < p.split_k ? load4f(ws0 + sj * sstride) : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) v += t[j];
                }
            } else {
                for (int s = w; s < p.split_k; s += 4) {
                    const float* ws = p.ws + ((long)s * p.M + m) * p.N + n;
                    for (int r = 0; r < 4; ++r) if (n + r < p.N) v[r] += ws[r];
                }
            }
        }
        red[w][lane] = v;
        __syncthreads();
        if (w == 0 && ok) epilogue4<T>(p, m, n, red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane]);
        __syncthreads();
    }
    if (p.a_colsum) {
        for (int m = blockIdx.x * 256 + threadIdx.x; m < p.M; m += gridDim.x * 256) {
            float s0 = 0.f;
            for (int z = 0; z < p.split_k; z += 8) {
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = z + j < p.split_k ? p.ws_colsum[(long)(z + j) * p.M + m] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) s0 += t[j];
            }
            p.a_colsum[m] = (p.epi & MVLT_EPI_ACCUM) ? p.a_colsum[m] + s0 : s0;
        }
    }
}

template <typename T, int BM, int BN, bool PF2>
int launch_layout2(const GemmDev& d, bool ak, bool bk, dim3 grid, hipStream_t s) {
    if constexpr (sizeof(T) == 2) {          // bf16 rows out, 16 bytes per lane (GemmDev.wide): forward / dgrad products only
        if (d.wide && !ak) {
            if (bk) hipLaunchKernelGGL((gemm_kernel<T, BM, BN, false, true, PF2, true>), grid, dim3(256), 0, s, d);
            else hipLaunchKernelGGL((gemm_kernel<T, BM, BN, false, false, PF2, true>), grid, dim3(256), 0, s, d);
            return 0;
        }
    }
    if (!ak && !bk) hipLaunchKernelGGL((gemm_kernel<T, BM, BN, false, false, PF2>), grid, dim3(256), 0, s, d);
    else if (!ak && bk) hipLaunchKernelGGL((gemm_kernel<T, BM, BN, false, true, PF2>), grid, dim3(256), 0, s, d);
    else if (ak && bk) hipLaunchKernelGGL((gemm_kernel<T, BM, BN, true, true, PF2>), grid, dim3(256), 0, s, d);
    else hipLaunchKernelGGL((gemm_kernel<T, BM, BN, true, false, PF2>), grid, dim3(256), 0, s, d);
    return 0;
}
template <typename T, int BM, int BN>
int launch_layout(const GemmDev& d, bool ak, bool bk, dim3 grid, hipStream_t s) {
    // deeper prefetch only for the small tiles (cheap in registers) and long reductions
    const int bke = 128 / (int)sizeof(T);
    const bool pf2 = BM == 64 && BN == 64 && d.k_per_split >= 12 * bke;
    if (pf2) return launch_layout2<T, BM, BN, (BM == 64 && BN == 64)>(d, ak, bk, grid, s);
    return launch_layout2<T, BM, BN, false>(d, ak, bk, grid, s);
}

struct Plan { int bm, bn, split; };

// 160 x 128 tiles exist only as the LDS-DMA kernel with the 16-byte epilogue (gemm_glds_kernel<160, 128, *, true>): every
// condition of that path is checked here, at PLAN time (the grid is sized for the planned tile)
bool tile160_ok(const MvltGemm* p) {
    const int epi = p->epilogue;
    if (p->dtype != MVLT_BF16 || p->a_kmajor || p->split_k > 1 || p->a_colsum) return false;
    if (p->K % 64 || p->N % 8 || p->lda % 8 || p->ldb % 8 || p->ldc % 8) return false;
    if (!aligned16(p->A) || !aligned16(p->B) || !aligned16(p->C)) return false;
    if (epi & (MVLT_EPI_OUT_F32 | MVLT_EPI_ACCUM)) return false;
    if ((epi & MVLT_EPI_RESIDUAL) && (p->ldr % 8 || !aligned16(p->residual))) return false;
    if ((epi & MVLT_EPI_SAVE_PRE) && !aligned16(p->pre)) return false;
    if ((epi & MVLT_EPI_MUL_GELU_GRAD) && !aligned16(p->aux)) return false;
    if ((epi & MVLT_EPI_BIAS) && !aligned16(p->bias)) return false;
    return true;
}

Plan choose_plan(const MvltGemm* p) {
    // tile: BN = 128 when N is a multiple of 128 (or large), else 96 (all model
    // widths are multiples of 96), 64 for tiny N.  BM = 128 unless that leaves
    // the 256 CUs under-filled.  split-K only when requested (>1) or auto (0).
    Plan pl;
    pl.bn = (p->N % 128 == 0) ? 128 : (p->N % 96 == 0 || p->N > 512) ? 96 : (p->N <= 64 ? 64 : (p->N <= 96 ? 96 : 128));
    if (p->N > 512 && p->N % 128 != 0 && p->N % 96 != 0) pl.bn = 128;
    long tiles128 = (long)ceil_div(p->M, 128) * ceil_div(p->N, pl.bn);
    pl.bm = (tiles128 >= 384 || p->M > 64 * 1024) ? 128 : 64;
    if (pl.bn == 64) pl.bm = 64;
    // narrow outputs (N = C of a Swin stage / 768): 64x128 tiles leave most of the 1024 resident slots
    // empty; 64x64 tiles quadruple the workgroup count (measured 10-25 % faster on those shapes)
    if (pl.bm == 64 && pl.bn == 128 && p->N % 64 == 0 &&
        (long)ceil_div(p->M, 64) * ceil_div(p->N, 128) < 512 && !(p->a_kmajor && p->b_kmajor)) pl.bn = 64;
    // wide outputs with a short reduction (BertLayer qkv / FFN-in forward, FFN-out dgrad: N >= 2304, K = 768): 64 x 128 tiles
    // put four to five workgroups on a CU instead of three and hide more of the operand latency: 27.6 vs 29.4 us stand-alone
    // on 3090 x 3072 x 768, +0.35 % pairs/s in the step (5 interleaved runs each)
    if (pl.bm == 128 && pl.bn == 128 && p->N >= 2304 && p->K <= 1024 && !(p->a_kmajor && p->b_kmajor)) pl.bm = 64;
    // forward products (x W^T) of the stage-2 / BertLayer size with a short reduction: 64 x 64 tiles are as fast as the wide ones
    // stand-alone (6272 x 1536 x 384: 19.8 vs 20.3 us, 3090 x 2304 x 768: 22.9 vs 23.1) and finish more evenly inside the forward
    // pass, a serial chain of ~250 launches where every tail is exposed: +0.55 % pairs/s (6 interleaved runs each)
    if (!p->a_kmajor && !p->b_kmajor && p->N % 64 == 0 && p->M <= 8192 && p->K <= 768 && p->N <= 2304) { pl.bm = 64; pl.bn = 64; }
    // ONE round of 160 x 128 tiles (two workgroups per CU: 512 slots) where that fills 2/3 .. all of the chip: 71 FLOP per byte of
    // L2 -> LDS traffic against 32-43 for the 64-row tiles (stand-alone 3150 x 3072 x 768 + GELU 27.1 vs 29.9 us, 3150 x 2304 x 768
    // 21.5 vs 23.7, 6272 x 1536 x 384 22.1 vs 24.5, 4192 x 2304 x 768 22.0 vs 28.3; scripts/tile160_sweep.sh)
    // Forward products only: for the dgrads of the same shapes the 72-KB workgroups share a CU badly with the weight-gradient stream
    // (step 11.66 -> 11.90 ms with them, 11.71 -> 11.64 ms with the forward products alone; profiles/r5_tile160_ab.txt).
    static const bool t160 = [] { const char* e = getenv("MVLT_TILE160"); return !e || atoi(e) != 0; }();
    if (t160 && p->N % 128 == 0 && p->N >= 1536 && p->K <= 1024 && !p->b_kmajor && tile160_ok(p)) {
        const long t = (long)ceil_div(p->M, 160) * (p->N / 128);
        // ragged batches (m_dev): M is the dense upper bound; the tiles beyond the packed row count leave at once, so the EFFECTIVE
        // count is ~3/4 of t (BertLayer FFN-in: 648 launched, ~480 with work).  Round 6: accepted up to 680 launched tiles -- at
        // worst (every caption at full length) that is a second, quarter-full round: 2 x 13.5 us against 33.6 us on 64 x 128 tiles.
        static const bool ragged160 = [] { const char* e = getenv("MVLT_TILE160_RAGGED"); return !e || atoi(e) != 0; }();
        const long tmax = (p->m_dev && ragged160) ? 680 : 512;
        if (t > 340 && t <= tmax) { pl.bm = 160; pl.bn = 128; }
    }
    if (const char* ov = getenv("MVLT_TILE")) {          // experiments: MVLT_TILE=bm,bn
        int a = 0, b = 0;
        if (sscanf(ov, "%d,%d", &a, &b) == 2 && (a == 128 || a == 64) && (b == 128 || b == 96 || b == 64) &&
            !(a == 128 && b == 64)) { pl.bm = a; pl.bn = b; }
        if (a == 160 && b == 128 && tile160_ok(p)) { pl.bm = 160; pl.bn = 128; }
    }
    long tiles = (long)ceil_div(p->M, pl.bm) * ceil_div(p->N, pl.bn);
    int split = p->split_k;
    if (split == 0) {
        split = 1;
        const int bke = (p->dtype == MVLT_BF16) ? 64 : 32;
        const int nkt = ceil_div(p->K, bke);
        if (tiles < 200 && nkt >= 16 && pl.bm != 160) {          // small outputs with a long reduction only (wgrads)
            split = (int)((768 + tiles - 1) / tiles);
            if (split > nkt / 8) split = nkt / 8;
            if (split > 96) split = 96;
            if (split < 1) split = 1;
        }
    }
    pl.split = split;
    return pl;
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) const void* mvlt_gemm_zero_page() {
    static const void* ptr = [] { void* q = nullptr; return hipGetSymbolAddress(&q, HIP_SYMBOL(g_zero_page)) == hipSuccess ? q : nullptr; }();
    return ptr;
}

static bool is_skinny_any(const MvltGemm* p) {
    return p->dtype == MVLT_BF16 ? is_skinny<bf16_t>(p) : (p->dtype == MVLT_F32 && is_skinny<float>(p));
}

extern "C" size_t mvlt_gemm_workspace_bytes(const MvltGemm* p) {
    if (!p) return 0;
    if (is_skinny_any(p)) return 0;
    Plan pl = choose_plan(p);
    return pl.split > 1 ? (size_t)pl.split * p->M * ((size_t)p->N + 1) * sizeof(float) : 0;
}

extern "C" int mvlt_gemm_plan(const MvltGemm* p, int* bm, int* bn, int* split_k) {
    if (!p || !bm || !bn || !split_k) return MVLT_ERR_ARG;
    if (is_skinny_any(p)) {      // (alignment permitting)
        *bm = 64; *bn = 16; *split_k = 1;
        return MVLT_OK;
    }
    Plan pl = choose_plan(p);
    *bm = pl.bm; *bn = pl.bn; *split_k = pl.split;
    return MVLT_OK;
}

// MvltGemm -> kernel argument block for a given plan
template <typename T>
static int fill_dev(const MvltGemm* p, const Plan& pl, GemmDev& d) {
    d.M = p->M; d.N = p->N; d.K = p->K;
    d.A = p->A; d.lda = p->lda; d.B = p->B; d.ldb = p->ldb; d.C = p->C; d.ldc = p->ldc;
    d.epi = p->epilogue; d.bias = p->bias; d.pre = p->pre; d.residual = p->residual; d.ldr = p->ldr;
    d.aux = p->aux; d.rowscale = p->rowscale; d.rps = p->rows_per_scale > 0 ? p->rows_per_scale : 1;
    d.rowmap = p->rowmap;
    double th = (double)p->dropout_p * 4294967296.0;
    d.drop_thresh = th >= 4294967295.0 ? 4294967295u : (uint32_t)th;
    d.drop_scale = p->dropout_p < 1.0f ? 1.0f / (1.0f - p->dropout_p) : 0.0f;
    d.seed = p->seed; d.tag = p->tag;
    constexpr int E = TypeInfo<T>::E;
    const int bke = 128 / (int)sizeof(T);
    d.split_k = pl.split;
    int kps = ceil_div(ceil_div(p->K, bke), pl.split) * bke;
    d.k_per_split = pl.split > 1 ? kps : ((p->K + bke - 1) / bke) * bke;
    if (pl.split > 1) {
        // drop empty trailing splits
        d.split_k = ceil_div(p->K, kps);
        size_t need = (size_t)d.split_k * p->M * ((size_t)p->N + 1) * sizeof(float);
        MVLT_CHECK(p->workspace && p->workspace_bytes >= need, MVLT_ERR_ARG);
        if (d.split_k == 1) d.k_per_split = ((p->K + bke - 1) / bke) * bke;
    }
    d.ws = reinterpret_cast<float*>(p->workspace);
    d.a_colsum = p->a_colsum;
    d.pf = (p->prefetch && p->prefetch_bytes >= 128) ? reinterpret_cast<const char*>(p->prefetch) : nullptr;
    d.pf_lines = d.pf ? (long)(p->prefetch_bytes >> 7) : 0;
    d.m_dev = p->m_dev;
    d.a_kmajor = p->a_kmajor != 0;
    d.atomic_out = 0;
    d.ws_colsum = d.ws ? d.ws + (size_t)d.split_k * p->M * p->N : nullptr;
    d.a_vec = (p->lda % E == 0) && aligned16(p->A);
    d.b_vec = (p->ldb % E == 0) && aligned16(p->B);
    const int epi = p->epilogue;
    bool ev = (p->ldc % 4 == 0) && aligned16(p->C);
    if (epi & MVLT_EPI_RESIDUAL) ev = ev && (p->ldr % 4 == 0) && aligned16(p->residual);
    if (epi & MVLT_EPI_SAVE_PRE) ev = ev && aligned16(p->pre);
    if (epi & MVLT_EPI_MUL_GELU_GRAD) ev = ev && aligned16(p->aux);
    d.epi_vec = ev;
    // 16-byte row operands (tile_epilogue_wide): bf16 rows out, every row operand in 8-column chunks that are 16-byte aligned;
    // tiles of 64 / 128 columns only (fragment PAIRS)
    d.wide = sizeof(T) == 2 && ev && !(epi & (MVLT_EPI_OUT_F32 | MVLT_EPI_ACCUM)) && p->N % 8 == 0 && p->ldc % 8 == 0 && pl.split <= 1 &&
             pl.bn != 96 && (!(epi & MVLT_EPI_RESIDUAL) || p->ldr % 8 == 0) && (!(epi & MVLT_EPI_BIAS) || aligned16(p->bias));
    d.xcs = gemm_pick_xcs(p->M, p->N, pl.bm, pl.bn);          // tile order (tile_coords)
    d.m_valid = p->M;                                         // (the kernels take it from effective())
    return MVLT_OK;
}

// route (gemm_host.h): null = launch; non-null = the same decisions, *route = the kernel family that would run, nothing launched
template <typename T>
static int gemm_dispatch(const MvltGemm* p, hipStream_t s, int* route = nullptr) {
    Plan pl = choose_plan(p);
    // MVLT_EPI_TAIL lives in the tile epilogues of this file (gemm_dev.h tail_rows_zero, slow_tail).  k-slices cannot honour it
    // (the slabs of the rows beyond the count are never written): refused, the caller asks for split_k = 1.  The skinny kernels,
    // the row-streaming kernel and the 8-wave engine refuse it themselves (their *_try answer 0) and the tile kernels run.
    if ((p->epilogue & MVLT_EPI_TAIL) && pl.split > 1) return MVLT_ERR_UNSUPPORTED;
    const bool skinny = is_skinny<T>(p);
    if (skinny) pl.split = 1;          // (no workspace was requested for it)
    GemmDev d;
    { const int rc = fill_dev<T>(p, pl, d); if (rc != MVLT_OK) return rc; }
    if (skinny) {          // M <= 64: skinny.hip, unless the operands cannot be loaded 16 bytes at a time
        const int rcs = mvlt_skinny_try(p, &d, s, route);
        if (rcs < 0) return MVLT_ERR_LAUNCH;
        if (rcs > 0) {
            if (route) return MVLT_OK;
            if (p->event_after_main) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(p->event_after_main), s);
            return MVLT_OK;
        }
    }
    dim3 grid(ceil_div(p->N, pl.bn), ceil_div(p->M, pl.bm), d.split_k);
    const bool ak = p->a_kmajor != 0, bk = p->b_kmajor != 0;
    if constexpr (sizeof(T) == 2) {
        // weight-stationary row streaming for the HBM-bound Swin stage-0 / 1 products (100 k / 25 k rows, K, N <= 384)
        if (!ak && d.split_k <= 1 && p->M >= 16384 && p->N <= 768 && p->K <= 384) {
            const int rcs = mvlt_rowstream_try(&d, bk ? 1 : 0, s, route);
            if (rcs < 0) return MVLT_ERR_LAUNCH;
            if (rcs > 0) {
                if (route) return MVLT_OK;
                if (p->event_after_main) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(p->event_after_main), s);
                return MVLT_OK;
            }
        }
        // 8-wave ping-pong engine (gemm8.hip) for wide outputs: MVLT_G8 = 0 never / 1 wherever it is eligible
        const int g8m = g8_mode();
        if (g8m && !ak && d.split_k <= 1) {
            const int rc8 = mvlt_gemm8_try(&d, 1, 0, bk ? 1 : 0, g8m == 2, nullptr, nullptr, 0, s, route);
            if (rc8 < 0) return MVLT_ERR_LAUNCH;
            if (rc8 > 0) {
                if (route) return MVLT_OK;
                if (p->event_after_main) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(p->event_after_main), s);
                return MVLT_OK;
            }
        }
        // LDS-DMA loop: 64-row tiles only.  Standalone the LDS-DMA loop is 5-12 %
        // faster on 128x128 tiles and 18-24 % on 64x64; inside the training step the 128x128 form (64 KB of LDS, two
        // workgroups per CU) is SLOWER than the register-staged one (three per CU, shares the CU better with the
        // weight-gradient stream): 16.5 vs 16.1 ms per step.
        const bool glds_on = pl.bm == 64 || pl.bm == 160;          // LDS-DMA loop for the 64-row tiles (comment above) and the 160-row ones
        const int kspan = d.split_k > 1 ? d.k_per_split : p->K;
        const bool bkm_ok = !bk || ((pl.bn == 64 || pl.bn == 128) && p->N % 8 == 0 && p->N >= 8);
        if (glds_on && !ak && bkm_ok && p->K % 64 == 0 && kspan % 64 == 0 && d.a_vec && d.b_vec) {
            bool done = true;
            // (route probe: every branch below launches through one of these two macros, which report instead)
#define GLDS_GO(BM_, BN_, BKM_) do { if (route) break; if (d.wide) hipLaunchKernelGGL((gemm_glds_kernel<BM_, BN_, BKM_, true>), grid, dim3(256), 0, s, d); \
                                     else hipLaunchKernelGGL((gemm_glds_kernel<BM_, BN_, BKM_, false>), grid, dim3(256), 0, s, d); } while (0)
            // 160-row tiles (72 KB of dynamic LDS, two workgroups per CU): wide epilogue only
#define GLDS_GO_DYN(BM_, BN_, BKM_) do { if (route) break; constexpr int sh_ = 2 * (BM_ + BN_) * 64 * 2; \
                static const bool ok_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_glds_kernel<BM_, BN_, BKM_, true>), \
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, sh_) == hipSuccess; \
                if (!ok_) return MVLT_ERR_LAUNCH; \
                hipLaunchKernelGGL((gemm_glds_kernel<BM_, BN_, BKM_, true>), grid, dim3(256), sh_, s, d); } while (0)
            // Three LDS stages (two K-tiles in flight per workgroup, counted vmcnt) where a launch has so few 64 x 64 tiles that a CU
            // holds one or two workgroups and every K-tile waits out a full L2 -> LDS latency: 1568 x 768 x 3072 26.8 -> 21.6 us.
            // With three workgroups per CU the loop is bound by the CU's L2 -> LDS bandwidth and the third stage only costs
            // (3150 x 768 x 3072: 32.3 vs 29.8 us; profiles/r5_glds_stages.txt).  MVLT_GLDS_STAGES=0 off, 2 = every 64 x 64 product.
            static const int st3 = [] { const char* e = getenv("MVLT_GLDS_STAGES"); return e ? atoi(e) : 1; }();
            const long tiles64 = (long)grid.x * grid.y;
            if (pl.bm == 160) {
                if (bk) GLDS_GO_DYN(160, 128, true); else GLDS_GO_DYN(160, 128, false);
            }
            else if (st3 && pl.bm == 64 && pl.bn == 64 && d.wide && kspan >= 768 && (st3 == 2 || (!bk && tiles64 <= 400))) {
                if (route) {}
                else if (bk) hipLaunchKernelGGL((gemm_glds_kernel<64, 64, true, true, 3>), grid, dim3(256), 0, s, d);
                else hipLaunchKernelGGL((gemm_glds_kernel<64, 64, false, true, 3>), grid, dim3(256), 0, s, d);
            }
            else if (bk) {
                if (pl.bm == 128 && pl.bn == 128) GLDS_GO(128, 128, true);
                else if (pl.bm == 64 && pl.bn == 128) GLDS_GO(64, 128, true);
                else if (pl.bm == 64 && pl.bn == 64) GLDS_GO(64, 64, true);
                else done = false;
            }
            else if (pl.bm == 128 && pl.bn == 128) GLDS_GO(128, 128, false);
            else if (pl.bm == 128 && pl.bn == 96) GLDS_GO(128, 96, false);
            else if (pl.bm == 64 && pl.bn == 128) GLDS_GO(64, 128, false);
            else if (pl.bm == 64 && pl.bn == 96) GLDS_GO(64, 96, false);
            else if (pl.bm == 64 && pl.bn == 64) GLDS_GO(64, 64, false);
            else done = false;
#undef GLDS_GO
#undef GLDS_GO_DYN
            if (done && route) { *route = gemm_route_code(MVLT_GEMM_ROUTE_GLDS, d.split_k); return MVLT_OK; }
            if (done) {
                MVLT_LAUNCH_CHECK();
                if (p->event_after_main) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(p->event_after_main), s);
                if (d.split_k > 1) {
                    long total = (long)p->M * ((p->N + 3) / 4);
                    int blocks = (int)((total + 63) / 64);
                    if (blocks > 8192) blocks = 8192;
                    hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3(blocks), dim3(256), 0, s, d);
                    MVLT_LAUNCH_CHECK();
                }
                return MVLT_OK;
            }
        }
    }
    if (pl.bm == 160) return MVLT_ERR_UNSUPPORTED;          // (tile160_ok and the conditions above disagree: never launch a mis-sized grid)
    if (route) { *route = gemm_route_code(MVLT_GEMM_ROUTE_REG, d.split_k); return MVLT_OK; }
    if (pl.bm == 128 && pl.bn == 128) launch_layout<T, 128, 128>(d, ak, bk, grid, s);
    else if (pl.bm == 128 && pl.bn == 96) launch_layout<T, 128, 96>(d, ak, bk, grid, s);
    else if (pl.bm == 64 && pl.bn == 128) launch_layout<T, 64, 128>(d, ak, bk, grid, s);
    else if (pl.bm == 64 && pl.bn == 96) launch_layout<T, 64, 96>(d, ak, bk, grid, s);
    else launch_layout<T, 64, 64>(d, ak, bk, grid, s);
    MVLT_LAUNCH_CHECK();
    if (p->event_after_main) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(p->event_after_main), s);
    if (d.split_k > 1) {
        long total = (long)p->M * ((p->N + 3) / 4);
        int blocks = (int)((total + 63) / 64);
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL((splitk_reduce_kernel<T>), dim3(blocks), dim3(256), 0, s, d);
        MVLT_LAUNCH_CHECK();
    }
    return MVLT_OK;
}

static int check_gemm_args(const MvltGemm* p) {
    MVLT_CHECK(p && p->A && p->B && p->C, MVLT_ERR_ARG);
    MVLT_CHECK(p->M > 0 && p->N > 0 && p->K > 0, MVLT_ERR_ARG);
    MVLT_CHECK(p->lda > 0 && p->ldb > 0 && p->ldc >= p->N, MVLT_ERR_ARG);
    MVLT_CHECK((long)p->M * p->N < (1L << 32) || !(p->epilogue & MVLT_EPI_DROPOUT), MVLT_ERR_ARG);
    const int e = p->epilogue;
    if (e & MVLT_EPI_BIAS) MVLT_CHECK(p->bias, MVLT_ERR_ARG);
    if (e & MVLT_EPI_SAVE_PRE) MVLT_CHECK(p->pre && (e & MVLT_EPI_GELU), MVLT_ERR_ARG);
    if (e & MVLT_EPI_RESIDUAL) MVLT_CHECK(p->residual && p->ldr >= p->N, MVLT_ERR_ARG);
    if (e & MVLT_EPI_ROWSCALE) MVLT_CHECK(p->rowscale, MVLT_ERR_ARG);
    if (e & MVLT_EPI_ROWMAP) MVLT_CHECK(p->rowmap, MVLT_ERR_ARG);
    if (e & MVLT_EPI_MUL_GELU_GRAD) MVLT_CHECK(p->aux, MVLT_ERR_ARG);
    if (e & MVLT_EPI_DROPOUT) MVLT_CHECK(p->dropout_p >= 0.f && p->dropout_p < 1.f, MVLT_ERR_ARG);
    if (p->a_colsum) MVLT_CHECK(p->a_kmajor, MVLT_ERR_ARG);
    if (e & MVLT_EPI_TAIL) MVLT_CHECK(p->m_dev && !p->a_kmajor, MVLT_ERR_ARG);
    return MVLT_OK;
}

// Grouped launch: weight gradients only (both operands k-major), 64-row tiles, no split-K.
template <typename T>
static int gemm_group_dispatch(const MvltGemm* items, int n, hipStream_t s, int* route = nullptr) {
    GemmGroupDev g{};
    g.n = n;
    bool all128 = true, all96 = true;
    for (int i = 0; i < n; ++i) { all128 = all128 && items[i].N % 128 == 0; all96 = all96 && items[i].N % 96 == 0; }
    const int bn = all128 ? 128 : (all96 ? 96 : 0);
    MVLT_CHECK(bn != 0, MVLT_ERR_UNSUPPORTED);
    for (int i = 0; i < n; ++i) {
        const MvltGemm* p = items + i;
        MVLT_CHECK(p->a_kmajor && p->b_kmajor && p->dtype == items[0].dtype, MVLT_ERR_UNSUPPORTED);
        Plan pl{64, bn, 1};
        { const int rc = fill_dev<T>(p, pl, g.g[i]); if (rc != MVLT_OK) return rc; }
    }
    // 128-row tiles when they still give every CU a workgroup (half the LDS fragment traffic per MFMA)
    int bm = 64;
    if (bn == 128) {
        long t128 = 0;
        for (int i = 0; i < n; ++i) t128 += (long)ceil_div(items[i].M, 128) * ceil_div(items[i].N, 128);
        if (t128 >= 256) bm = 128;
        // MVLT_WGRAD_BM=64: 64 x 128 tiles for every group (162 instead of 243 VGPRs per wave: two such workgroups leave a third
        // of a SIMD's registers to the dgrad chain's kernels; A/B switch, profiles/r6_ln_bwd.md)
        static const int env_bm = [] { const char* e = getenv("MVLT_WGRAD_BM"); return e ? atoi(e) : 0; }();
        if (env_bm == 64) bm = 64;
    }
    long tiles = 0;
    int kmin = items[0].K;
    for (int i = 0; i < n; ++i) { tiles += (long)ceil_div(items[i].M, bm) * ceil_div(items[i].N, bn); kmin = items[i].K < kmin ? items[i].K : kmin; }
    // In-launch split-K: groups with fewer than 200 tiles (Swin stages 0/1: 21 / 72 tiles, 100k / 25k reduction rows) are
    // cut into k-slices: on the 8-wave engine below (f32 slabs, deterministic) when it takes the group, otherwise here, where the
    // slices meet in the zeroed f32 output through atomicAdd.  Groups with >= 200 tiles are never split: measured on the B=32 step it does not shorten
    // the stage-2 groups in situ and the zeroing launch + atomics cost 1 ms per step (17.1 vs 15.9 ms).
    const int bke = 128 / (int)sizeof(T);
    int split = 1;
    // the k-slices meet through f32 atomicAdd: the order of the 7-24 additions per element is not fixed, so the result is
    // not bit-reproducible run to run.  Never in the exact-f32 mode (the parity path), never under MVLT_DETERMINISTIC=1.
    static const bool deterministic = [] { const char* e = getenv("MVLT_DETERMINISTIC"); return e && e[0] == '1'; }();
    if (tiles < 200 && sizeof(T) == 2 && !deterministic) {
        split = (int)((512 + tiles - 1) / tiles);
        const int nkt = ceil_div(kmin, bke);
        if (split > nkt / 8) split = nkt / 8;
        if (split > 64) split = 64;
        if (split < 1) split = 1;
    }
    // 8-wave ping-pong engine (gemm8.hip) for the groups this kernel would cut into ATOMIC k-slices (few tiles, tens of
    // thousands of reduction rows: Swin stages 0 / 1): one persistent launch of 128 x 128 tiles, k-slices that meet through
    // f32 slabs (the last arriver of a tile sums them in slice order: deterministic, no float atomics), bias gradients as
    // dY^T . 1 on the matrix pipe -- 100 vs 137 us (stage 0) and 78 vs 91 us (stage 1) per group.  MVLT_G8=1 sends every
    // group there (tests / experiments: the BertLayer / stage-2 groups tie with this kernel), MVLT_G8=0 none.
    if constexpr (sizeof(T) == 2) {
        const int g8m = g8_mode();
        if (g8m && (g8m == 1 || split > 1 || tiles < 200)) {
            GemmDev tmp[GROUP_MAX];
            float* outs[GROUP_MAX];
            bool ok = true;
            for (int i = 0; i < n; ++i) {
                tmp[i] = g.g[i]; outs[i] = tmp[i].a_colsum; tmp[i].a_colsum = nullptr;
                ok = ok && tmp[i].epi == MVLT_EPI_OUT_F32;
            }
            if (ok) {
                const int rc8 = mvlt_gemm8_try(tmp, n, 1, 1, 0, outs, items[0].workspace, items[0].workspace_bytes, s, route);
                if (rc8 < 0) return MVLT_ERR_LAUNCH;
                if (rc8 > 0) return MVLT_OK;
            }
        }
    }
    g.split = split;
    for (int i = 0; i < n; ++i) {
        g.start[i] = i == 0 ? 0 : g.start[i];
        g.start[i + 1] = g.start[i] + ceil_div(items[i].M, bm) * ceil_div(items[i].N, bn) * split;
        if (split > 1) {
            GemmDev& d = g.g[i];
            d.split_k = split;
            d.k_per_split = ceil_div(ceil_div(items[i].K, bke), split) * bke;
            d.atomic_out = 1;
        }
    }
    if (split > 1) {
        for (int i = 0; i < n; ++i) MVLT_CHECK(items[i].ldc == items[i].N, MVLT_ERR_UNSUPPORTED);          // contiguous outputs (gradient arena views)
        if (route) { *route = gemm_route_code(MVLT_GEMM_ROUTE_GROUP_ATOMIC, split); return MVLT_OK; }
        MvltZeroItem z[2 * GROUP_MAX];
        int nz = 0;
        for (int i = 0; i < n; ++i) {
            z[nz++] = MvltZeroItem{reinterpret_cast<float*>(items[i].C), (int64_t)items[i].M * items[i].N};
            if (items[i].a_colsum) z[nz++] = MvltZeroItem{items[i].a_colsum, (int64_t)items[i].M};
        }
        const int rc = mvlt_zero_batch(z, nz, s);
        if (rc != MVLT_OK) return rc;
    }
    // at most 2 workgroups per CU (of the 3 that fit): the group runs on the side stream beside the dgrad
    // chain, which should keep a share of every CU (16.8 vs 17.1 ms/step uncapped; 1 / 3 per CU measured equal or worse)
    int total = g.start[n];
    // (MVLT_WGRAD_PER_CU=1|2|3: A/B switch; round 6 re-ran 1 against 2 with the low-footprint LayerNorm backward beside it)
    static const int per_cu = [] { const char* e = getenv("MVLT_WGRAD_PER_CU"); const int v = e ? atoi(e) : 2; return v >= 1 && v <= 3 ? v : 2; }();
    if (total > per_cu * 256) total = per_cu * 256;
    // bf16: two LDS stages + two register sets, one barrier per k-tile (the single-stage form measured 1.3 % slower in the step)
    const int reg_route = gemm_route_code(bn == 96 ? MVLT_GEMM_ROUTE_GROUP_REG_64x96
                                                   : (bm == 128 ? MVLT_GEMM_ROUTE_GROUP_REG_128x128 : MVLT_GEMM_ROUTE_GROUP_REG_64x128), 1);
#define GROUP_LAUNCH(BM_, BN_, D_) hipLaunchKernelGGL((gemm_group_kernel<T, BM_, BN_, true, true, D_>), dim3(total), dim3(256), 0, s, g)
    if constexpr (sizeof(T) == 2) {
        // LDS-DMA form (round 6; MVLT_WGRAD_GLDS=0: the register-staged kernel): bf16, no k-slices, 128-wide column tiles, every
        // operand row 16-byte aligned in 8-element chunks, f32 output through the vector epilogue
        static const bool glds_wg = [] { const char* e = getenv("MVLT_WGRAD_GLDS"); return !e || atoi(e) != 0; }();
        // 128 x 128 tiles (BertLayer and stage-3 groups, two stages, two workgroups per CU): 62.2 against 77.1 us and 36.3 against 43.9 us
        // stand-alone.  64 x 128 tiles (stage 2: 216 tiles, ONE workgroup per CU): a lone workgroup needs the deeper pipeline -- two
        // stages 88 us, three stages (72 KB of dynamic LDS, two k-tiles in flight) 75 us, four 89 us, against 62 us for the
        // register-staged form stand-alone; INSIDE the step the order turns round, because the dgrad chain's kernels run beside
        // 128-register waves instead of 162-register ones: 11.45 / 11.45 / 11.36 ms per step with three stages against 11.55 / 11.50 /
        // 11.57 with the register-staged kernels (two stages 11.53 / 11.51 / 11.51; profiles/r6_wgrad_glds.md).
        // MVLT_WGRAD_GLDS: 0 = register-staged kernels, 1 = 128 x 128 groups only, 2 = 64 x 128 with two stages, 3 (default) = three.
        static const int glds_mode = [] { const char* e = getenv("MVLT_WGRAD_GLDS"); return e ? atoi(e) : 3; }();
        bool ok = glds_wg && split == 1 && bn == 128 && (bm == 128 || glds_mode >= 2);
        for (int i = 0; i < n && ok; ++i) {
            const GemmDev& d = g.g[i];
            ok = d.a_vec && d.b_vec && d.epi_vec && (d.M % 8 == 0) && (d.N % 8 == 0) && d.M >= 8 && d.N >= 8 &&
                 (d.epi & ~(MVLT_EPI_OUT_F32 | MVLT_EPI_ACCUM)) == 0 && (d.epi & MVLT_EPI_OUT_F32) && !d.atomic_out && d.split_k <= 1;
        }
        if (ok && route) {
            *route = gemm_route_code(bm == 128 ? MVLT_GEMM_ROUTE_GROUP_GLDS_128x128
                                               : (glds_mode == 3 ? MVLT_GEMM_ROUTE_GROUP_GLDS_64x128_S3 : MVLT_GEMM_ROUTE_GROUP_GLDS_64x128_S2), 1);
            return MVLT_OK;
        }
        if (ok) {
            if (bm == 128) hipLaunchKernelGGL((gemm_group_glds_kernel<128, 128, 2>), dim3(total), dim3(256), 0, s, g);
            else if (glds_mode == 3) {          // 64 x 128 with three stages (72 KB of dynamic LDS: two k-tiles in flight for a lone workgroup)
                constexpr int sh3 = 3 * (64 + 128) * 64 * 2;
                static const bool ok3 = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_group_glds_kernel<64, 128, 3>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, sh3) == hipSuccess;
                if (!ok3) return MVLT_ERR_LAUNCH;
                hipLaunchKernelGGL((gemm_group_glds_kernel<64, 128, 3>), dim3(total), dim3(256), sh3, s, g);
            }
            else hipLaunchKernelGGL((gemm_group_glds_kernel<64, 128, 2>), dim3(total), dim3(256), 0, s, g);
            MVLT_LAUNCH_CHECK();
            return MVLT_OK;
        }
        if (route) { *route = reg_route; return MVLT_OK; }
        if (bn == 128 && bm == 128) GROUP_LAUNCH(128, 128, 2); else if (bn == 128) GROUP_LAUNCH(64, 128, 2); else GROUP_LAUNCH(64, 96, 2);
    } else {
        if (route) { *route = reg_route; return MVLT_OK; }
        if (bn == 128 && bm == 128) GROUP_LAUNCH(128, 128, 0); else if (bn == 128) GROUP_LAUNCH(64, 128, 0); else GROUP_LAUNCH(64, 96, 0);
    }
#undef GROUP_LAUNCH
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

// Workspace a grouped launch can use (items[0].workspace / workspace_bytes; 0 = none needed): room for the k-slice slabs of
// the 8-wave engine.  Without it the group still runs (unsliced, or on the 4-wave grouped kernel).
extern "C" size_t mvlt_gemm_group_workspace_bytes(const MvltGemm* items, int n) {
    if (!items || n < 1 || n > GROUP_MAX || items[0].dtype != MVLT_BF16) return 0;
    GemmDev tmp[GROUP_MAX];
    for (int i = 0; i < n; ++i) {
        if (check_gemm_args(items + i) != MVLT_OK || !items[i].a_kmajor || !items[i].b_kmajor) return 0;
        Plan pl{64, 128, 1};
        MvltGemm it = items[i];
        it.workspace = nullptr; it.workspace_bytes = 0;
        if (fill_dev<bf16_t>(&it, pl, tmp[i]) != MVLT_OK) return 0;
    }
    return mvlt_gemm8_group_workspace(tmp, n);
}

extern "C" int mvlt_gemm_group(const MvltGemm* items, int n, void* stream) {
    MVLT_CHECK(items && n >= 1 && n <= GROUP_MAX, MVLT_ERR_ARG);
    for (int i = 0; i < n; ++i) { const int rc = check_gemm_args(items + i); if (rc != MVLT_OK) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (items[0].dtype == MVLT_F32) return gemm_group_dispatch<float>(items, n, s);
    if (items[0].dtype == MVLT_BF16) return gemm_group_dispatch<bf16_t>(items, n, s);
    return MVLT_ERR_UNSUPPORTED;
}

// The routes, from the dispatch functions themselves in their no-launch mode
extern "C" int mvlt_gemm_route(const MvltGemm* p) {
    { const int rc = check_gemm_args(p); if (rc != MVLT_OK) return rc; }
    int route = 0;
    const int rc = p->dtype == MVLT_F32 ? gemm_dispatch<float>(p, nullptr, &route)
                                        : (p->dtype == MVLT_BF16 ? gemm_dispatch<bf16_t>(p, nullptr, &route) : MVLT_ERR_UNSUPPORTED);
    return rc != MVLT_OK ? rc : route;
}

extern "C" int mvlt_gemm_group_route(const MvltGemm* items, int n) {
    MVLT_CHECK(items && n >= 1 && n <= GROUP_MAX, MVLT_ERR_ARG);
    for (int i = 0; i < n; ++i) { const int rc = check_gemm_args(items + i); if (rc != MVLT_OK) return rc; }
    int route = 0;
    const int rc = items[0].dtype == MVLT_F32 ? gemm_group_dispatch<float>(items, n, nullptr, &route)
                                              : (items[0].dtype == MVLT_BF16 ? gemm_group_dispatch<bf16_t>(items, n, nullptr, &route) : MVLT_ERR_UNSUPPORTED);
    return rc != MVLT_OK ? rc : route;
}

extern "C" int mvlt_gemm(const MvltGemm* p, void* stream) {
    { const int rc = check_gemm_args(p); if (rc != MVLT_OK) return rc; }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (p->dtype == MVLT_F32) return gemm_dispatch<float>(p, s);
    if (p->dtype == MVLT_BF16) return gemm_dispatch<bf16_t>(p, s);
    return MVLT_ERR_UNSUPPORTED;
}
