// Fused Swin (S)W-MSA forward, second design (round 4): several windows per workgroup, heads split across workgroups.
// Same contract as wmsa.hip (MvltSwinWmsa, include/mvlt_hip.h): the attention half of a SwinTransformerBlock
// (visual_feature_extractor.py:224-254 and :356-384) in ONE launch, bf16 storage / f32 accumulation.
//
// Why a second design: with one window per workgroup (wmsa.hip) every workgroup streams all 8 C^2 bytes of projection
// weights for 49 rows, and a stage-2 launch of a B = 32 step has 128 windows for 256 CUs (profiles/r2_wmsa_pmc.md:
// 7.6 % MFMA busy).  Here a UNIT is (W consecutive windows) x (G heads):
//   * M = 49 W token rows share every weight fragment (W = 2: 98 rows = seven 16-row MFMA tiles, 12.5 % padding instead
//     of 23 %), so a weight element is fetched from L2 once per 98 rows;
//   * the nH / G head groups of a window set go to DIFFERENT workgroups: stage 2 at B = 32 is 64 sets x 4 groups = 256
//     workgroups, one per CU, each streaming its own 6 C x 32 G slice of Wqkv and 32 G x C slice of Wproj;
//   * the output projection needs all heads of a row: the groups meet through the attention-output tensor itself
//     (attn_out, which training saves anyway).  Each workgroup writes its [M, 32 G] slice WRITE-THROUGH (sc1), drains,
//     and adds to an arrival counter; when the counter shows all groups, it reads the full [M, C] rows back with sc1 loads
//     (cdna_hip_programming.md Guideline 16, counter form; no fence, L1 bypassed) and computes ITS 32 G output columns
//     of proj + bias + DropPath + shortcut.  Nothing depends on dispatch order or XCD placement; what the wait needs is
//     that the groups of a set are co-resident: the launch is persistent with at most one workgroup per CU
//     (grid <= 256, a multiple of the group count; LDS use forces one per CU), units dealt round-robin, so the groups
//     of a set are always in flight together.  Spins are bounded: when one runs out the unit's rows of y become NaN and
//     the sticky error count (word 0 of the sync workspace) is raised -- a failure is loud, never silent.
//   * counters clean up after themselves (the last group to finish READING resets them), so no memset per launch.
//
// Phases of a unit (8 waves):
//   0  gather M rows through the row map, LayerNorm (f32 statistics) -> LDS tile [16 MT][C], XOR-swizzled so that the
//      A fragments are conflict-free ds_read_b128 (scripts/lds_bank_model.py); group 0 also saves xn / mean / rstd
//   1  qkv projection of the group's heads: N tiles dealt to the waves, weight fragments straight from L2 into MFMA
//      operands through a register ring PD k-steps deep; q, k, v (+ bias) -> LDS tiles [part][head][row][32] with 64-byte
//      rows, chunk' = (chunk + 2 (row >> 2)) & 3 (conflict-free row AND transposed reads at any window offset)
//   2  attention: (window, head, query tile) units; scores transposed (keys on accumulator rows) so softmax is in-register;
//      the accumulators START at (bias + mask) / scale -- read from an LDS copy of the table through per-lane offsets with
//      the head as an immediate -- and exp2 folds scale and max into one fma: ~6 vector instructions per score
//   3  hand-off (above), then the projection slice with all its weight fragments prefetched before the wait
#include "common.h"
#include "attn_frag.h"
#include <stdlib.h>
#include <atomic>

namespace {
using namespace mvlt_attn;
typedef bf16_t T;
using Frag = bf16x8;

struct Wmsa2Dev {
    int nwin, nW, res, shift, nH, nunits;
    const T* x; T* y; const int* w2n;
    const float* gamma; const float* beta; float eps;
    const T* wqkv; const float* bqkv; const T* wproj; const float* bproj;
    const float* bias_table; float scale;
    const float* rowscale;
    T* xn; T* ao; T* qkv; float* lse; float* mean; float* rstd;
    int* sync;               // hand-off workspace (layout below)
    long long spin_ticks;    // bound of the hand-off wait in ticks of the 100 MHz real-time clock
};

// Hand-off workspace (int32 words).  The layout does not depend on the batch size, so one workspace serves every launch of a
// stream: word 0 = sticky error count (bounded waits that ran out since the words were last cleared), words 1..15 unused,
// then per window set 8 words: one ARRIVAL FLAG per head group (round 6: was one arrival counter) and the readers-done
// counter; all of them are back at 0 when a launch has finished.
#define W2_SYNC_ERROR 0
#define W2_SYNC_STRIDE 8     /* words per window set: arrival flag of head group g at +g (g < 7), readers-done counter at +7 */
#define W2_SYNC_FLAG(set, g) (16 + W2_SYNC_STRIDE * (set) + (g))
#define W2_SYNC_DONE(set) (16 + W2_SYNC_STRIDE * (set) + 7)
#define W2_TBL_FLAG 175      // pad entry of the LDS bias table (indices 170..175 are never addressed)

template <int C, int W, int G, int GS> struct W2Geom {
    static constexpr int M = 49 * W, MT = (M + 15) / 16, MR = MT * 16;
    static constexpr int NH = C / 32, NHG = NH / G, NSUB = G / GS;
    static constexpr int QR = (49 * (W - 1) + 64 + 3) / 4 * 4;            // rows of one (part, head) tile
    static constexpr int OC = G * 32;                                      // columns of the attention-output tile
    static constexpr int XB = MR * C * 2;
    // q/k/v tiles; for widths whose weights stream through LDS (C % 64 == 0) the same region first holds the two stages of the
    // weight ring ([96 GS rows][64 k] each) and, after the attention phase, the output-projection weights
    static constexpr int WROWS = 96 * GS, WSTAGE = WROWS * 64, WNBUF = 4;          // stage = one k-step (32 k = 64 bytes per row)
    static constexpr bool WLDS = C % 64 == 0 && NSUB == 1;          // (two sub-groups, C = 192: the LDS budget has no room for the ring)
    static constexpr int QB0 = 3 * GS * QR * 64;
    static constexpr int QB = (WLDS && WNBUF * WSTAGE > QB0) ? WNBUF * WSTAGE : QB0;
    static constexpr int TB = G * 176 * 4;
    static constexpr bool ALIAS_O = NSUB == 1 && NHG > 1 && (XB + QB + MR * OC * 2 + TB > 160 * 1024);
    static constexpr int OB = ALIAS_O ? 0 : MR * OC * 2;
    static constexpr int bytes = XB + QB + OB + TB;
    static_assert(bytes <= 160 * 1024, "LDS");
    static_assert(NH % G == 0 && G % GS == 0, "head groups");
};

// [rows][CC] bf16 tile: byte offset of 16-byte chunk `chunk` of row `row`; chunks XOR-swizzled with the row inside groups
// of 16 / 8 / 4 chunks (whatever divides the row) -- the A fragments of every k-step are then conflict-free for C = 384, 768
template <int CC> MVLT_DEV int xoff(int row, int chunk) {
    constexpr int CPR = CC / 8;
    constexpr int GRP = CPR % 16 == 0 ? 16 : (CPR % 8 == 0 ? 8 : 4);
    return row * (CC * 2) + (((chunk & ~(GRP - 1)) | ((chunk ^ row) & (GRP - 1))) << 4);
}
// [rows][32] bf16 tile with 64-byte rows
MVLT_DEV int hoff(int row, int chunk) { return row * 64 + (((chunk + 2 * (row >> 2)) & 3) << 4); }

MVLT_DEV void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// LDS-DMA (glds16, common.h): hipcc does not see the request, the callers wait for it with vm_drain before the barrier that
// publishes the bytes


// -DW2_TRACE (diagnostic build only): thread 0 of every workgroup stamps the 100 MHz real-time counter at the phase
// boundaries of its FIRST unit into a buffer set by mvlt_swin_wmsa2_trace_buffer (scripts/wmsa2_trace.py reads it)
#ifdef W2_TRACE
__device__ long long* g_w2_trace = nullptr;
#define W2_STAMP(k) do { if (threadIdx.x == 0 && g_w2_trace && unit < (int)gridDim.x) { g_w2_trace[blockIdx.x * 64 + (k)] = __builtin_amdgcn_s_memrealtime(); g_w2_trace[blockIdx.x * 64 + 32 + (k)] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define W2_STAMP(k) do { } while (0)
#endif

typedef __attribute__((address_space(3))) char lds_char;
MVLT_DEV uint32_t lds_addr(const void* q) { return (uint32_t)(uintptr_t)(lds_char*)q; }      // generic pointer into LDS -> LDS byte address
MVLT_DEV float lds_f32(uint32_t a) { return *reinterpret_cast<__attribute__((address_space(3))) float*>(a); }
MVLT_DEV Frag lds_frag(uint32_t a) { return *reinterpret_cast<__attribute__((address_space(3))) Frag*>(a); }
MVLT_DEV bf16x4 lds_tr(uint32_t a) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(reinterpret_cast<__attribute__((address_space(3))) bf16x4*>(a)); }
// sum over the 2 / 4 / 8 / 16 consecutive lanes of a row segment with DPP adds (no LDS round trips)
template <int LPR> MVLT_DEV float row_sum(float v) {
    static_assert(LPR <= 16, "row_sum: one DPP row");
    if (LPR >= 2) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    if (LPR >= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    if (LPR >= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
    if (LPR >= 16) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true)); // row_mirror
    return v;
}

template <int C, int W, int G, int GS, int NWV>
__global__ __launch_bounds__(64 * NWV) void wmsa2_fwd_kernel(const Wmsa2Dev p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using GM = W2Geom<C, W, G, GS>;
    constexpr int M = GM::M, MT = GM::MT, MR = GM::MR, NHG = GM::NHG, NSUB = GM::NSUB, QR = GM::QR, OC = GM::OC;
    constexpr int NT = 64 * NWV;
    constexpr int KSTEPS = C / 32;
    constexpr int NTQ = 6 * GS, NTQW = (NTQ + NWV - 1) / NWV;      // qkv N tiles of a head sub-group, per wave
    constexpr int NTP = (NHG > 1 ? OC : C) / 16, NTPW = (NTP + NWV - 1) / NWV;   // output-projection N tiles of this group
    constexpr int PD = KSTEPS < 4 ? KSTEPS : 4;
    // attention: W GS (window, head) pairs x 4 query tiles; wave = (pair group NG', query tile), UPW pairs per wave.  With as many
    // pair groups as heads (12 waves, 3 heads) a wave keeps ONE head (bias values in registers) and walks the windows; with as
    // many as windows (8 waves, 2 windows) it keeps one window and walks the heads
    constexpr int NG = NWV / 4;
    constexpr int UPW = W * GS / NG;
    constexpr bool HEAD_FIXED = NG == GS;
    static_assert(NWV % 4 == 0 && (W * GS) % NG == 0 && (HEAD_FIXED || NG == W), "attention units per wave");
    // output projection: NTP column tiles; when there are more waves than tiles the row tiles are split into MG groups
    constexpr int MG = NTP < NWV ? NWV / NTP : 1, MTW = (MT + MG - 1) / MG;
    constexpr bool PAIR = C % 64 == 0;
    constexpr int TILE = QR * 64;                                   // bytes of one (part, head) q/k/v tile
    static_assert(C % 32 == 0, "width");
    static_assert(W == 1 || W == 2, "windows per unit");

    char* xln = smem;                                   // [MR][C] LayerNorm tile; later the full attention output [MR][C]
    char* qkvt = smem + GM::XB;                         // [3][GS][QR][32]
    char* ot = GM::ALIAS_O ? smem : smem + GM::XB + GM::QB;        // [MR][OC] attention output of this group's heads
    float* tbl = reinterpret_cast<float*>(smem + GM::XB + GM::QB + GM::OB);     // [G][176] (bias / scale; 169.. = -1e30)

    const int nsets = p.nwin / W;
    const float cexp = p.scale * 1.4426950408889634f;   // exp(scale s) = exp2(cexp s)
    const float inv_scale = 1.0f / p.scale;
    const int nwx = p.res / 7;

    const __amdgpu_buffer_rsrc_t ao_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.ao, 0, (int)((long)p.nwin * 49 * C * 2), 0x00020000);
    // lse stores of invalid lanes (padded queries) and of eval launches (no lse) are dropped by the range check
    const __amdgpu_buffer_rsrc_t lse_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.lse, 0, p.lse ? (int)((long)p.nwin * p.nH * 49 * 4) : 0, 0x00020000);

    // unit order: blocks b and b + 8 share an XCD (observed round-robin placement; speed only), so the blocks of one XCD take a
    // CONTIGUOUS run of units: the head groups of a window set then share an L2 (its rows are fetched once instead of NHG
    // times).  (grid / 8) * 8 blocks are remapped, the rest keep their index; grid is a multiple of NHG either way.
    const int gpx = gridDim.x / 8;
    const int bid = ((int)blockIdx.x < gpx * 8 && gpx % NHG == 0) ? ((int)blockIdx.x & 7) * gpx + ((int)blockIdx.x >> 3) : (int)blockIdx.x;
#pragma unroll 1
    for (int unit = bid; unit < p.nunits; unit += gridDim.x) {
        // every per-lane quantity is derived INSIDE the loop from an opaque copy of the thread id: with one unit per
        // workgroup (the B = 32 case) loop-invariant hoisting only buys ~600 instructions and ~90 spilled registers up front
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, c15 = lane & 15;
        // element offset of a lane's 16 bytes at k-step kk inside a weight row / chunk index inside an activation row:
        // lane group g takes bytes [32 g, 32 g + 32) of every 128-byte line, first half at the even step (whole lines per pair)
        auto koff = [&](int kk) -> int { return PAIR ? (kk >> 1) * 64 + g * 16 + (kk & 1) * 8 : kk * 32 + g * 8; };
        auto kchunk = [&](int kk) -> int { return PAIR ? (kk >> 1) * 8 + 2 * g + (kk & 1) : kk * 4 + g; };
        const int qt = wave & 3, wg = wave >> 2;
        const int qrow = 16 * qt + c15;

        const int set = unit / NHG, hg = unit - set * NHG;
        const int win0 = set * W;
        const int head0 = hg * G;
        const long grow0 = (long)win0 * 49;                 // first window-order row of the set
        W2_STAMP(0);

        // token row of window-order row m of this unit: roll(-shift) + window_partition (visual_feature_extractor.py:144-156,
        // 360-367) evaluated directly -- the INT map of SURVEY 8a2 / 8a3 (mvlt_amd.indexing.window_token_map), no table read
        int wbase[W], wy7[W], wx7[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int win = win0 + w, b = win / p.nW, wi = win - b * p.nW, wy = wi / nwx;
            wbase[w] = b * p.res * p.res; wy7[w] = 7 * wy; wx7[w] = 7 * (wi - wy * nwx);
        }
        auto tok_of = [&](int m) -> int {
            const int w = (W == 2 && m >= 49) ? 1 : 0, slot = m - 49 * w, sy = div7(slot), sx = slot - 7 * sy;
            int h = wy7[w] + sy + p.shift, x = wx7[w] + sx + p.shift;
            h = h >= p.res ? h - p.res : h; x = x >= p.res ? x - p.res : x;
            return wbase[w] + h * p.res + x;
        };

        auto wq_ptr = [&](int hs, int t) -> const T* {      // weight row of qkv tile t (sub-group hs) for this lane
            const int tt = min(t, NTQ - 1);
            const int part = tt / (2 * GS), within = tt - part * 2 * GS;
            return p.wqkv + (long)(part * C + (head0 + hs * GS) * 32 + within * 16 + c15) * C;
        };
        Frag fb[PD][NTQW];
        uint32_t ridx[4], rowbits = 0, colbits = 0;
        // weight ring (WLDS): buffer kk % WNBUF <- k-step kk (columns 32 kk .. +32) of the qkv weight rows of sub-group hs.  A 1-KB
        // piece is 16 rows x 64 bytes (lane = (row, position); position pos of row r holds chunk (pos + 2 (r >> 2)) & 3, the
        // hoff placement); wave w issues pieces w, w + NWV, ... -- WPPW of them (the last ones may be missing: see WPC)
        constexpr int WNPC = GM::WROWS / 16, WPPW = (WNPC + NWV - 1) / NWV;
        const int wpc = (WNPC - wave + NWV - 1) / NWV;                           // pieces THIS wave issues per k-step
        auto wring_fill = [&](int hs, int kk) {
            if constexpr (GM::WLDS) {
                const uint32_t dst0 = lds_addr(qkvt) + (kk % GM::WNBUF) * GM::WSTAGE;
#pragma unroll
                for (int j = 0; j < WPPW; ++j) {
                    const int pc = wave + NWV * j;
                    if (pc < WNPC) {
                        const int r = 16 * pc + (lane >> 2), part = r / (32 * GS), rr = r - part * 32 * GS;
                        const int ch = ((lane & 3) + 2 * (r >> 2)) & 3;
                        glds16(p.wqkv + (long)(part * C + (head0 + hs * GS) * 32 + rr) * C + kk * 32 + ch * 8, dst0 + pc * 1024);
                    }
                }
            }
        };
        // wait until this wave's pieces of k-step kk have landed while `later` younger k-steps stay in flight
        auto wring_wait = [&](int later) {
            if (wpc == WPPW) {
                if (later >= 2) wait_vmcnt<2 * WPPW>();
                else if (later == 1) wait_vmcnt<WPPW>();
                else vm_drain();
            } else {
                if (later >= 2) wait_vmcnt<2 * (WPPW - 1)>();
                else if (later == 1) wait_vmcnt<WPPW - 1>();
                else vm_drain();
            }
        };
        // ---- gather the rows (token order -> window order), LayerNorm, normalised tile -> LDS
        {
            constexpr int CPR = C / 8;                                       // 16-byte chunks per row
            constexpr int LPR = CPR % 3 == 0 ? CPR / 3 : CPR / 2;             // lanes per row
            constexpr int CPL = CPR / LPR;
            constexpr int RPP = NT / LPR, NPASS = (MR + RPP - 1) / RPP;
            static_assert(LPR <= 16 && (LPR & (LPR - 1)) == 0 && NT % LPR == 0, "LayerNorm lanes per row");
            const int sub = tid % LPR, r0 = tid / LPR;
            bf16x8 xv[NPASS][CPL];
            int tok[NPASS];
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const int row = ps * RPP + r0;
                tok[ps] = row < M ? tok_of(row) : -1;
                const T* src = p.x + (long)max(tok[ps], 0) * C;
#pragma unroll
                for (int i = 0; i < CPL; ++i) xv[ps][i] = *reinterpret_cast<const bf16x8*>(src + (sub + LPR * i) * 8);
            }
            // gamma / beta of this lane's chunks: the same for every pass
            f32x4 ga[CPL][2], be[CPL][2];
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    ga[i][hf] = load4f(p.gamma + (sub + LPR * i) * 8 + 4 * hf);
                    be[i][hf] = load4f(p.beta + (sub + LPR * i) * 8 + 4 * hf);
                }
            bf16x2 ones; ones[0] = (T)1.0f; ones[1] = (T)1.0f;
#ifdef W2_TRACE
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            W2_STAMP(16);                                  // rows, gamma / beta, first weight fragments arrived
#endif
#pragma unroll
            for (int ps = 0; ps < NPASS; ++ps) {
                const int row = ps * RPP + r0;
                if (ps == 1 || NPASS == 1) {
                    asm volatile("" ::: "memory");         // (keeps the requests below behind the first pass's loads)
            // ---- behind the first rows' statistics: the first weight fragments, the pair facts and the tables.  Requested any
                    // earlier they queue IN FRONT of nothing but share the start-up burst (every CU fetching ~75 KB of rows at once runs at
                    // ~11 B/cycle/CU) and the rows, which everything waits for, arrive later
                    if constexpr (!GM::WLDS) {
#pragma unroll
                        for (int jj = 0; jj < NTQW; ++jj) {
                            const T* w = wq_ptr(0, wave + NWV * jj);
#pragma unroll
                            for (int d = 0; d < PD; ++d) fb[d][jj] = *reinterpret_cast<const Frag*>(w + koff(d));
                        }
                    }
                    // packed pair facts of this wave's query tile (relative-position indices, border bits): 5 registers carried to the
                    // attention phase, expanded there
                    if (p.shift == 0 || p.shift == 3) {
                        const int e = qt * 64 + lane;
#pragma unroll
                        for (int t = 0; t < 4; ++t) ridx[t] = SWIN_PAIRS.ridx[e][t];
                        const uint32_t bb = p.shift ? SWIN_PAIRS.bits3[e] : 0u;
                        rowbits = bb & 0xffffu; colbits = bb >> 16;
                    } else {
                        const int query = 16 * qt + c15, oc = min(query, 48), oy = div7(oc), ox = oc - 7 * oy;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            ridx[t] = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int key = 16 * t + 4 * g + j;
                                const bool valid = key < 49 && query < 49;
                                const int kc = min(key, 48), ky = div7(kc), kx = kc - 7 * ky;
                                ridx[t] |= (uint32_t)(valid ? rel_index(oc, kc) : 169) << (8 * j);
                                if (valid && ((ky < 7 - p.shift) != (oy < 7 - p.shift))) rowbits |= 1u << (4 * t + j);
                                if (valid && ((kx < 7 - p.shift) != (ox < 7 - p.shift))) colbits |= 1u << (4 * t + j);
                            }
                        }
                    }

                    // bias table of this group's heads -> LDS, divided by scale (the score accumulators start there)
                    for (int i = tid; i < G * 176; i += NT) {
                        const int h = i / 176, e = i - h * 176;
                        tbl[i] = e < 169 ? p.bias_table[e * p.nH + head0 + h] * inv_scale : NEG_BIG;
                    }
                    // the ring's first requests go out LAST: hipcc does not see them, so its wait for any load it issued earlier
                    // (the table values above are consumed at once) would otherwise wait for the ring too
                    asm volatile("" ::: "memory");
                    if constexpr (GM::WLDS) {
#pragma unroll
                        for (int kk = 0; kk < GM::WNBUF && kk < KSTEPS; ++kk) wring_fill(0, kk);      // the whole ring fills under the LayerNorm
                    }
                    asm volatile("" ::: "memory");
                }
                if (row >= M && row < MR) {
                    // padded rows of the last 16-row tile: zeros (finite values nobody reads) -- no statistics, no arithmetic
#pragma unroll
                    for (int i = 0; i < CPL; ++i) *reinterpret_cast<bf16x8*>(xln + xoff<C>(row, sub + LPR * i)) = zero_vec<T>();
                } else if (row < M) {
                    const bool rv = true;
                    // sum and sum of squares with the packed dot product (no conversions), reduced over the row's lanes by DPP
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int i = 0; i < CPL; ++i)
#pragma unroll
                        for (int e = 0; e < 8; e += 2) {
                            bf16x2 a; a[0] = xv[ps][i][e]; a[1] = xv[ps][i][e + 1];
                            s1 = __builtin_amdgcn_fdot2_f32_bf16(a, ones, s1, false);
                            s2 = __builtin_amdgcn_fdot2_f32_bf16(a, a, s2, false);
                        }
                    s1 = row_sum<LPR>(s1); s2 = row_sum<LPR>(s2);
                    const float mean = s1 * (1.0f / C);
                    const float var = fmaxf(s2 * (1.0f / C) - mean * mean, 0.0f);
                    const float rstd = __builtin_amdgcn_rsqf(var + p.eps);
                    const bool save = rv && hg == 0;
                    if (save && sub == 0 && p.mean) { p.mean[tok[ps]] = mean; p.rstd[tok[ps]] = rstd; }
                    T* xs = (p.xn && save) ? p.xn + (grow0 + row) * C : nullptr;
                    const float nm = -mean * rstd;
                    const f32x2 rs2{rstd, rstd}, nm2{nm, nm};
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        const int ch = sub + LPR * i;
                        bf16x8 o;
                        // ((x rstd + nm) gamma + beta) on element PAIRS: two v_pk_fma_f32 per pair instead of a multiply and two
                        // fmas per element (round 6: the LayerNorm phase is ~500 vector instructions per wave, all of them issue)
                        const u32x4 xw = __builtin_bit_cast(u32x4, xv[ps][i]);
#pragma unroll
                        for (int e = 0; e < 8; e += 2) {
                            const uint32_t w = xw[e >> 1];
                            f32x2 x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)};
                            const f32x2 g2{ga[i][e >> 2][e & 3], ga[i][e >> 2][(e & 3) + 1]}, b2{be[i][e >> 2][e & 3], be[i][e >> 2][(e & 3) + 1]};
                            f32x2 t = __builtin_elementwise_fma(x2, rs2, nm2);
                            t = __builtin_elementwise_fma(t, g2, b2);
                            o[e] = (T)t[0]; o[e + 1] = (T)t[1];
                        }
                        *reinterpret_cast<bf16x8*>(xln + xoff<C>(row, ch)) = o;
                        if (xs) *reinterpret_cast<bf16x8*>(xs + ch * 8) = o;
                    }
                }
            }
        }
        __syncthreads();
        W2_STAMP(1);                                       // LayerNorm tile ready

#pragma unroll
        for (int hs = 0; hs < NSUB; ++hs) {
            // ================= qkv projection of head sub-group hs: [MR, C] x [C, 96 GS]
            if constexpr (GM::WLDS) {
                // Weights through the LDS ring.  Tile assignment WITHOUT wave-dependent branches (a branch per tile keeps hipcc from
                // overlapping a k-step's fragment reads with the previous k-step's MFMAs): every wave owns FULL whole column tiles
                // (all MT row tiles each); the REM left-over column tiles are dealt out as single (row tile, column tile) pairs,
                // LPW per wave (a wave without a last pair repeats pair LQ - 1 into an accumulator nobody stores).
                constexpr int FULL = NTQ / NWV, REM = NTQ % NWV, LQ = REM * MT, LPW = (LQ + NWV - 1) / NWV;
                f32x4 acc[MT][FULL > 0 ? FULL : 1], lacc[LPW > 0 ? LPW : 1];
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int jj = 0; jj < FULL; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
                int lm[LPW > 0 ? LPW : 1], ln[LPW > 0 ? LPW : 1];
#pragma unroll
                for (int e = 0; e < LPW; ++e) {
                    const int q = min(wave + NWV * e, LQ - 1);
                    ln[e] = FULL * NWV + q / MT; lm[e] = q % MT;
                    lacc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                const uint32_t xa = lds_addr(xln), wa = lds_addr(qkvt);
                // (k-slots in plain order here: a stage row is the 64 contiguous bytes of one k-step.)  The loop is software-
                // pipelined ACROSS its barrier: the barrier in front of k-step kk's MFMAs certifies k-step kk + 1 (landed for every
                // wave; every wave has its k-step-kk fragments in registers), the fragments of kk + 1 are requested, and only then
                // are the MFMAs of kk issued -- the LDS latency and the LDS-DMA issue hide behind the matrix pipe
                auto frags = [&](int kk, Frag (&fa)[MT], Frag (&la)[LPW > 0 ? LPW : 1], Frag (&fw)[FULL > 0 ? FULL : 1], Frag (&lw)[LPW > 0 ? LPW : 1]) {
                    const uint32_t wst = wa + (kk % GM::WNBUF) * GM::WSTAGE;
#pragma unroll
                    for (int jj = 0; jj < FULL; ++jj) fw[jj] = lds_frag(wst + hoff(16 * (wave + NWV * jj) + c15, g));
#pragma unroll
                    for (int e = 0; e < LPW; ++e) lw[e] = lds_frag(wst + hoff(16 * ln[e] + c15, g));
#pragma unroll
                    for (int i = 0; i < MT; ++i) fa[i] = lds_frag(xa + xoff<C>(16 * i + c15, 4 * kk + g));
#pragma unroll
                    for (int e = 0; e < LPW; ++e) la[e] = lds_frag(xa + xoff<C>(16 * lm[e] + c15, 4 * kk + g));
                };
                Frag fa[2][MT], la[2][LPW > 0 ? LPW : 1], fw[2][FULL > 0 ? FULL : 1], lw[2][LPW > 0 ? LPW : 1];
                wring_wait(KSTEPS - 1 < GM::WNBUF - 1 ? KSTEPS - 1 : GM::WNBUF - 1);          // k-step 0 (the prologue filled the whole ring)
                __syncthreads();
                frags(0, fa[0], la[0], fw[0], lw[0]);
#pragma unroll
                for (int kk = 0; kk < KSTEPS; ++kk) {
                    const int cur = kk & 1, nxt = cur ^ 1;
                    if (kk + 1 < KSTEPS) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this wave's fragments of k-step kk are in registers
                        wring_wait(KSTEPS - 2 - kk < GM::WNBUF - 2 ? KSTEPS - 2 - kk : GM::WNBUF - 2);      // its pieces of k-step kk + 1 have landed
                        __syncthreads();
#ifndef W2_ABL_NODMA
                        if (kk + GM::WNBUF < KSTEPS) wring_fill(hs, kk + GM::WNBUF);           // into the buffer k-step kk just left
#endif
                        frags(kk + 1, fa[nxt], la[nxt], fw[nxt], lw[nxt]);
                    }
#ifdef W2_ABL_NOMMA
#pragma unroll
                    for (int jj = 0; jj < FULL; ++jj) asm volatile("" :: "v"(fw[cur][jj]));
#pragma unroll
                    for (int i = 0; i < MT; ++i) asm volatile("" :: "v"(fa[cur][i]));
#pragma unroll
                    for (int e = 0; e < LPW; ++e) { asm volatile("" :: "v"(lw[cur][e])); asm volatile("" :: "v"(la[cur][e])); }
#else
#pragma unroll
                    for (int jj = 0; jj < FULL; ++jj)
#pragma unroll
                        for (int i = 0; i < MT; ++i)
                            acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[cur][jj], fa[cur][i], acc[i][jj], 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < LPW; ++e)
                        lacc[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lw[cur][e], la[cur][e], lacc[e], 0, 0, 0);
#endif
                }
                W2_STAMP(12 + hs);                         // (wave 0) projection MFMAs issued
                __syncthreads();                           // the last stage has been read: the region becomes the q/k/v tiles
                // rows of the q/k/v tiles beyond the projected rows (read as padded keys of the last window): finite
                for (int i = tid; i < 3 * GS * (QR - MR) * 4; i += NT) {
                    const int ch = i & 3, r = (i >> 2) % (QR - MR), tl = (i >> 2) / (QR - MR);
                    *reinterpret_cast<bf16x8*>(qkvt + tl * TILE + hoff(MR + r, ch)) = zero_vec<T>();
                }
                // + bias, to the q/k/v LDS tiles [part][head][row][32]
                auto put = [&](int t, int i, const f32x4& v) {
                    const int part = t / (2 * GS), within = t - part * 2 * GS;
                    const f32x4 b4 = load4f(p.bqkv + part * C + (head0 + hs * GS) * 32 + within * 16 + 4 * g);
                    char* tile = qkvt + (part * GS + (within >> 1)) * TILE;
                    store4f(reinterpret_cast<T*>(tile + hoff(16 * i + c15, (within & 1) * 2 + (g >> 1)) + (g & 1) * 8), v + b4);
                };
#pragma unroll
                for (int jj = 0; jj < FULL; ++jj)
#pragma unroll
                    for (int i = 0; i < MT; ++i) put(wave + NWV * jj, i, acc[i][jj]);
#pragma unroll
                for (int e = 0; e < LPW; ++e)
                    if (wave + NWV * e < LQ) put(ln[e], lm[e], lacc[e]);
            } else
            {
                f32x4 acc[MT][NTQW];
                f32x4 b4[NTQW];
#pragma unroll
                for (int jj = 0; jj < NTQW; ++jj) {
                    const int t = min(wave + NWV * jj, NTQ - 1);
                    const int part = t / (2 * GS), within = t - part * 2 * GS;
                    b4[jj] = load4f(p.bqkv + part * C + (head0 + hs * GS) * 32 + within * 16 + 4 * g);
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                const T* wrow[NTQW];
#pragma unroll
                for (int jj = 0; jj < NTQW; ++jj) wrow[jj] = wq_ptr(hs, wave + NWV * jj);
#pragma unroll
                for (int kk = 0; kk < KSTEPS; ++kk) {
                    Frag fa[MT];
                    const int ch = kchunk(kk);
#pragma unroll
                    for (int i = 0; i < MT; ++i) fa[i] = *reinterpret_cast<const Frag*>(xln + xoff<C>(16 * i + c15, ch));
#pragma unroll
                    for (int jj = 0; jj < NTQW; ++jj) {
                        if (wave + NWV * jj < NTQ) {
#pragma unroll
                            for (int i = 0; i < MT; ++i)
                                acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[kk % PD][jj], fa[i], acc[i][jj], 0, 0, 0);
                        }
                        if constexpr (PAIR && PD % 2 == 0) {
                            // the two k-steps of a pair read the two halves of the same 128-byte lines: requested back to back
                            // (issued one k-step apart the line has left the 32-KB L1 again and crosses L2 -> L1 twice)
                            if (kk & 1) {
                                if (kk - 1 + PD < KSTEPS) fb[(kk - 1) % PD][jj] = *reinterpret_cast<const Frag*>(wrow[jj] + koff(kk - 1 + PD));
                                if (kk + PD < KSTEPS) fb[kk % PD][jj] = *reinterpret_cast<const Frag*>(wrow[jj] + koff(kk + PD));
                            }
                        } else {
                            if (kk + PD < KSTEPS) fb[kk % PD][jj] = *reinterpret_cast<const Frag*>(wrow[jj] + koff(kk + PD));
                        }
                    }
                }
                // rows of the q/k/v tiles beyond the projected rows (read as padded keys of the last window): finite
                for (int i = tid; i < 3 * GS * (QR - MR) * 4; i += NT) {
                    const int ch = i & 3, r = (i >> 2) % (QR - MR), tl = (i >> 2) / (QR - MR);
                    *reinterpret_cast<bf16x8*>(qkvt + tl * TILE + hoff(MR + r, ch)) = zero_vec<T>();
                }
                W2_STAMP(12 + hs);                         // (wave 0) projection MFMAs issued
                // + bias, to the q/k/v LDS tiles [part][head][row][32]
#pragma unroll
                for (int jj = 0; jj < NTQW; ++jj) {
                    const int t = wave + NWV * jj;
                    if (t < NTQ) {
                        const int part = t / (2 * GS), within = t - part * 2 * GS;
                        char* tile = qkvt + (part * GS + (within >> 1)) * TILE;
                        const int ch = (within & 1) * 2 + (g >> 1), sub8 = (g & 1) * 8;
#pragma unroll
                        for (int i = 0; i < MT; ++i)
                            store4f(reinterpret_cast<T*>(tile + hoff(16 * i + c15, ch) + sub8), acc[i][jj] + b4[jj]);
                    }
                }
            }
            // weight fragments of what comes next: the next sub-group's first k-steps
            if constexpr (!GM::WLDS) {
                if (hs + 1 < NSUB) {
#pragma unroll
                    for (int jj = 0; jj < NTQW; ++jj) {
                        const T* w = wq_ptr(hs + 1, wave + NWV * jj);
#pragma unroll
                        for (int d = 0; d < PD; ++d) fb[d][jj] = *reinterpret_cast<const Frag*>(w + koff(d));
                    }
                }
            }
            __syncthreads();
            W2_STAMP(2 + 2 * hs);                          // q, k, v tiles ready

            // ================= (training) q, k, v of the sub-group -> HBM in the [row, 3C] layout of the unfused kernels
            if (p.qkv) {
                T* qg = p.qkv + grow0 * 3 * C + (head0 + hs * GS) * 32;
                for (int idx = tid; idx < M * 3 * GS * 4; idx += NT) {
                    const int ch = idx & 3, ph = (idx >> 2) % (3 * GS), r = (idx >> 2) / (3 * GS);
                    const int part = ph / GS, hl = ph - part * GS;
                    *reinterpret_cast<bf16x8*>(qg + (long)r * 3 * C + part * C + hl * 32 + ch * 8) =
                        *reinterpret_cast<const bf16x8*>(qkvt + (part * GS + hl) * TILE + hoff(r, ch));
                }
            }

            // ================= window attention: this wave's query tile of UPW (window, head) pairs.  The pairs are written stage
            // by stage over u (straight-line code, no branches): independent chains for the scheduler
            {
                // pair u of this wave: (window, head inside the sub-group)
                auto pw = [&](int u) -> int { return HEAD_FIXED ? u : wg; };
                auto ph = [&](int u) -> int { return HEAD_FIXED ? wg : u; };
                const uint32_t qk0 = lds_addr(qkvt), tb0 = lds_addr(tbl) + hs * GS * 176 * 4;
                const float maskv = -100.0f * inv_scale;
                f32x4 sc[UPW][4];
                // scores start at (bias + mask) / scale
                uint32_t mbits[UPW];
#pragma unroll
                for (int u = 0; u < UPW; ++u) {
                    mbits[u] = 0;
                    if (p.shift != 0) {
                        const int wi = (win0 + pw(u)) % p.nW, wy = wi / nwx, wx = wi - wy * nwx;
                        mbits[u] = (wy == nwx - 1 ? rowbits : 0u) | (wx == nwx - 1 ? colbits : 0u);
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t a = tb0 + ((ridx[t] >> (8 * j)) & 255u) * 4;
                        if constexpr (HEAD_FIXED) {
                            const float bv = lds_f32(a + wg * 176 * 4);
#pragma unroll
                            for (int u = 0; u < UPW; ++u) sc[u][t][j] = (mbits[u] & (1u << (4 * t + j))) ? bv + maskv : bv;
                        } else {
                            const float mk = (mbits[0] & (1u << (4 * t + j))) ? maskv : 0.0f;
#pragma unroll
                            for (int u = 0; u < UPW; ++u) sc[u][t][j] = lds_f32(a + u * 176 * 4) + mk;
                        }
                    }
                Frag fq[UPW];
#pragma unroll
                for (int u = 0; u < UPW; ++u) fq[u] = lds_frag(qk0 + (0 * GS + ph(u)) * TILE + hoff(49 * pw(u) + 16 * qt + c15, g));
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int u = 0; u < UPW; ++u)
                        sc[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lds_frag(qk0 + (1 * GS + ph(u)) * TILE + hoff(49 * pw(u) + 16 * t + c15, g)),
                                                                            fq[u], sc[u][t], 0, 0, 0);
                W2_STAMP(17);                              // score MFMAs issued
                float mx[UPW], sum[UPW];
#pragma unroll
                for (int u = 0; u < UPW; ++u) {
                    float m = NEG_BIG;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int j = 0; j < 4; ++j) m = fmaxf(m, sc[u][t][j]);
                    mx[u] = m;
                }
#pragma unroll
                for (int u = 0; u < UPW; ++u) mx[u] = fmaxf(mx[u], __shfl_xor(mx[u], 16, 64));
#pragma unroll
                for (int u = 0; u < UPW; ++u) mx[u] = fmaxf(mx[u], __shfl_xor(mx[u], 32, 64));
#pragma unroll
                for (int u = 0; u < UPW; ++u) {
                    const float mxc = -mx[u] * cexp;
                    float sm = 0.f;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int j = 0; j < 4; ++j) { const float e = __builtin_amdgcn_exp2f(fmaf(sc[u][t][j], cexp, mxc)); sc[u][t][j] = e; sm += e; }
                    sum[u] = sm;
                }
#pragma unroll
                for (int u = 0; u < UPW; ++u) sum[u] += __shfl_xor(sum[u], 16, 64);
#pragma unroll
                for (int u = 0; u < UPW; ++u) sum[u] += __shfl_xor(sum[u], 32, 64);
                // lse (training); padded queries and eval launches fall outside the descriptor's range and are dropped
#pragma unroll
                for (int u = 0; u < UPW; ++u) {
                    const int h = head0 + hs * GS + ph(u);
                    const long off = (((long)(win0 + pw(u)) * p.nH + h) * 49 + qrow) * 4;
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, fmaf(__builtin_amdgcn_logf(sum[u]), 0.6931471805599453f, mx[u] * p.scale)),
                                                          lse_rsrc, (g == 0 && qrow < 49) ? (int)off : 0x7fffffff, 0, 0);
                }
                W2_STAMP(18);                              // softmax done
                f32x4 o[UPW][2];
#pragma unroll
                for (int u = 0; u < UPW; ++u) { o[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; o[u][1] = o[u][0]; }
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                    for (int td = 0; td < 2; ++td) {
#pragma unroll
                        for (int u = 0; u < UPW; ++u) {
                            // V^T fragment: features 16 td .. +15 on the rows, k-slots = keys 32 kb + 4 g + {0..3} and + 16
                            const int q4 = c15 >> 2, pp = c15 & 3;
                            const int row = 49 * pw(u) + 32 * kb + 4 * g + q4, el = 16 * td + 4 * pp;
                            const uint32_t vb = qk0 + (2 * GS + ph(u)) * TILE + (el & 7) * 2;
                            const bf16x4 lo = lds_tr(vb + hoff(row, el >> 3)), hi4 = lds_tr(vb + hoff(row + 16, el >> 3));
                            Frag fv;
                            fv[0] = lo[0]; fv[1] = lo[1]; fv[2] = lo[2]; fv[3] = lo[3];
                            fv[4] = hi4[0]; fv[5] = hi4[1]; fv[6] = hi4[2]; fv[7] = hi4[3];
                            o[u][td] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv, frag_acc<4>(sc[u], kb, T()), o[u][td], 0, 0, 0);
                        }
                    }
                }
                // normalised output -> attention-output tile; padded queries write the tile's last (unused) row
#pragma unroll
                for (int u = 0; u < UPW; ++u) {
                    const int orow = qrow < 49 ? 49 * pw(u) + qrow : MR - 1;
                    const float inv = __builtin_amdgcn_rcpf(sum[u]);
#pragma unroll
                    for (int td = 0; td < 2; ++td) {
                        const int el = (hs * GS + ph(u)) * 32 + 16 * td + 4 * g;
                        store4f(reinterpret_cast<T*>(ot + xoff<OC>(orow, el >> 3) + (el & 7) * 2), o[u][td] * inv);
                    }
                }
            }
            if (hs + 1 < NSUB) {
                __syncthreads();                          // the q/k/v tiles are rewritten by the next sub-group
                if constexpr (GM::WLDS) wring_fill(hs + 1, 0);
            }
        }

        // ================= output-projection operands that do not depend on the other groups: ALL weight fragments of this
        // wave's columns, bias, shortcut rows, DropPath scales -- requested before the hand-off so the wait hides them.
        // Wave -> (column tiles pt(jj), row tiles pm0 .. pm0 + MTW): more waves than column tiles split the row tiles
        const int pm0 = MG > 1 ? (wave / NTP) * MTW : 0;
        auto pt = [&](int jj) -> int { return MG > 1 ? wave % NTP : wave + NWV * jj; };
        const bool pact = MG > 1 ? wave < MG * NTP : true;
        // (PLDS: this group's rows of Wproj go to the q/k/v region by LDS-DMA once the attention phase has left it -- whole
        // cache lines, no fragment registers -- and land while the groups wait for each other)
        constexpr bool PLDS = GM::WLDS && NHG > 1 && OC * C * 2 <= GM::QB;
        Frag fpj[PLDS ? 1 : KSTEPS][NTPW];
        f32x4 pb4[NTPW];
        bf16x4 resid[MTW][NTPW];             // shortcut values, converted where they are used (a conversion here would wait for the load)
        int tokm[MTW];
        float rsm[MTW];
#pragma unroll
        for (int i = 0; i < MTW; ++i) {
            const int m = 16 * (pm0 + i) + c15;
            tokm[i] = m < M ? tok_of(m) : -1;
            rsm[i] = (p.rowscale && m < M) ? p.rowscale[(win0 + m / 49) / p.nW] : 1.0f;
        }
#pragma unroll
        for (int jj = 0; jj < NTPW; ++jj) {
            const int t = min(pt(jj), NTP - 1);
            const int n0 = (NHG > 1 ? hg * OC : 0) + 16 * t;
            const T* w = p.wproj + (long)(n0 + c15) * C;
            if constexpr (!PLDS) {
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) fpj[ks][jj] = *reinterpret_cast<const Frag*>(w + koff(ks));
            }
            pb4[jj] = load4f(p.bproj + n0 + 4 * g);
#pragma unroll
            for (int i = 0; i < MTW; ++i) resid[i][jj] = *reinterpret_cast<const bf16x4*>(p.x + (long)max(tokm[i], 0) * C + n0 + 4 * g);
        }
        W2_STAMP(19);                                      // (wave 0) attention units and prefetch requests issued
        __syncthreads();                                   // attention-output tile of the group complete
        W2_STAMP(6);

        const char* atile;                                 // A operand of the projection: [MR][C]
        int done_ticket = -1;
        bool poison = false;                               // the hand-off wait of this unit ran out
        if constexpr (NHG > 1) {
            // ---- this group's [M, OC] slice -> attn_out, write-through
            {
                constexpr int CH = OC / 8;
                for (int idx = tid; idx < M * CH; idx += NT) {
                    const int r = idx / CH, ch = idx - r * CH;
                    const u32x4 v = *reinterpret_cast<const u32x4*>(ot + xoff<OC>(r, ch));
                    __builtin_amdgcn_raw_buffer_store_b128(v, ao_rsrc, (int)(((grow0 + r) * C + hg * OC + ch * 8) * 2), 0, 16);
                }
            }
            if (tid == 0) tbl[W2_TBL_FLAG] = 0.0f;         // (a pad entry of the bias table: rewritten with the table per unit)
            vm_drain();
            __syncthreads();
            W2_STAMP(7);                                   // slice published
            if constexpr (PLDS) {
                // Wproj rows [hg OC, +OC) -> LDS image [OC][C] in the A-operand layout (xoff): piece = 1 KB of the image
                constexpr int NPC = OC * C * 2 / 1024;
                static_assert((OC * C * 2) % 1024 == 0, "projection weight image");
                const uint32_t dst0 = lds_addr(qkvt);
#pragma unroll
                for (int j = 0; j < (NPC + NWV - 1) / NWV; ++j) {
                    const int pc = wave + NWV * j;
                    if (pc < NPC) {
                        const int slot = pc * 64 + lane, r = slot / (C / 8), pos = slot - r * (C / 8);
                        constexpr int GRP = (C / 8) % 16 == 0 ? 16 : ((C / 8) % 8 == 0 ? 8 : 4);
                        const int ch = (pos & ~(GRP - 1)) | ((pos ^ r) & (GRP - 1));
                        glds16(p.wproj + (long)(hg * OC + r) * C + ch * 8, dst0 + pc * 1024);
                    }
                }
            }
            // ---- the exchange, ordered by ARRIVAL (round 6).  Every group raises its own flag once all its stores have
            // completed (one lane, after the workgroup's vmcnt(0) + barrier above: cdna_hip_programming.md Guideline 16, flag
            // form).  The waves of a reader split the NHG slices among themselves -- wave w takes slice slot w / NPART (slot 0 =
            // the workgroup's own slice: no wait) and part w % NPART of its rows -- and each wave polls ITS group's flag and
            // then loads that slice with sc1 loads (the wave that polled loads after its poll matched; another CU wrote the
            // bytes: L1 bypassed) straight into the A-operand tile: the slices of groups that arrived early are in LDS while
            // the wave of the last group is still waiting, there is no counter round trip (add -> poll) and one workgroup
            // barrier less than the wait-for-all form (stage 2, B = 32: 6.4 -> ~4 us between "published" and "rows in LDS").
            // Bounded (p.spin_ticks of the 100 MHz clock, ~2 s by default): when a wait runs out the sticky error word (word 0 of
            // the workspace, whatever the batch size) is raised and this unit's rows of y are written as NaN, so a caller that
            // never reads the word still sees a poisoned loss.
            // (an ADD, polled as "> 0": a flag that was mis-armed negative never reads as raised -- how the tests provoke a time-out)
            if (tid == 0) __hip_atomic_fetch_add(p.sync + W2_SYNC_FLAG(set, hg), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            {
                static_assert(NWV % NHG == 0 && NHG <= 7, "exchange: waves per slice");
                constexpr int NPART = NWV / NHG;
                constexpr int CHG = OC / 8;                                  // 16-byte chunks per row of one group's slice
                constexpr int RP = (M + NPART - 1) / NPART, TOTP = RP * CHG, PER = (TOTP + 63) / 64;
                const int slot = wave / NPART, part = wave - slot * NPART;
                const int gid = (hg + slot) % NHG;
                if (slot != 0) {
                    int ok = 1;
                    if (lane == 0) {
                        const long long t0 = __builtin_amdgcn_s_memrealtime();
                        while (__hip_atomic_load(p.sync + W2_SYNC_FLAG(set, gid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) {
                            __builtin_amdgcn_s_sleep(1);
                            if (__builtin_amdgcn_s_memrealtime() - t0 > p.spin_ticks) { ok = 0; break; }
                        }
                        if (!ok) tbl[W2_TBL_FLAG] = 1.0f;          // (several waves may write the same 1.0)
                    }
                    ok = __builtin_amdgcn_readfirstlane(ok);          // (also orders the wave's loads below behind lane 0's poll)
                    asm volatile("" ::: "memory");
                }
                u32x4 v[PER];
                const int r_lo = part * RP, r_hi = min(r_lo + RP, M);
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = min(lane + 64 * i, TOTP - 1), r = min(r_lo + idx / CHG, M - 1), ch = idx % CHG;
                    v[i] = __builtin_amdgcn_raw_buffer_load_b128(ao_rsrc, (int)(((grow0 + r) * C + gid * OC + ch * 8) * 2), 0, 16);
                }
#pragma unroll
                for (int i = 0; i < PER; ++i) {
                    const int idx = lane + 64 * i, r = r_lo + idx / CHG, ch = idx % CHG;
                    if (idx < TOTP && r < r_hi) *reinterpret_cast<u32x4*>(xln + xoff<C>(r, gid * CHG + ch)) = v[i];
                }
                // padded rows M..MR-1 of the tile keep the LayerNorm tile's zeros (the attention-output tile ends below them)
            }
            if constexpr (PLDS) vm_drain();                // (the projection weights were requested before these loads: landed)
            __syncthreads();
            poison = tbl[W2_TBL_FLAG] != 0.0f;
            if (poison && tid == 0)                        // ONE count per workgroup whose wait ran out
                __hip_atomic_fetch_add(p.sync + W2_SYNC_ERROR, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            W2_STAMP(9);                                   // full rows in LDS
            // every reader counts itself out (the add is issued here, its result is looked at after the projection)
            if (tid == NT - 64) done_ticket = __hip_atomic_fetch_add(p.sync + W2_SYNC_DONE(set), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atile = xln;
        } else {
            // all heads are here: (training) the attention output -> HBM for the proj weight gradient
            if (p.ao) {
                constexpr int CH = C / 8;
                for (int idx = tid; idx < M * CH; idx += NT) {
                    const int r = idx / CH, ch = idx - r * CH;
                    *reinterpret_cast<u32x4*>(p.ao + (grow0 + r) * C + ch * 8) = *reinterpret_cast<const u32x4*>(ot + xoff<OC>(r, ch));
                }
            }
            atile = ot;
        }

        // ================= output projection slice: y[M, cols of this group] = A[M, C] Wproj[cols, :]^T
        {
            f32x4 pacc[MTW][NTPW];
#pragma unroll
            for (int i = 0; i < MTW; ++i)
#pragma unroll
                for (int jj = 0; jj < NTPW; ++jj) pacc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (pact) {
                // fragments of k-step ks + 1 are requested before the MFMAs of k-step ks (two register sets)
                Frag fa[2][MTW], fw[2][NTPW];
                auto pfrags = [&](int ks, Frag (&a)[MTW], Frag (&w)[NTPW]) {
                    const int ch = kchunk(ks);
#pragma unroll
                    for (int i = 0; i < MTW; ++i) a[i] = *reinterpret_cast<const Frag*>(atile + xoff<C>(min(16 * (pm0 + i), MR - 16) + c15, ch));
#pragma unroll
                    for (int jj = 0; jj < NTPW; ++jj) {
                        if constexpr (PLDS) w[jj] = lds_frag(lds_addr(qkvt) + xoff<C>(16 * min(pt(jj), NTP - 1) + c15, ch));
                        else w[jj] = fpj[ks][jj];
                    }
                };
                pfrags(0, fa[0], fw[0]);
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) {
                    if (ks + 1 < KSTEPS) pfrags(ks + 1, fa[(ks + 1) & 1], fw[(ks + 1) & 1]);
#pragma unroll
                    for (int jj = 0; jj < NTPW; ++jj) {
                        if (pt(jj) < NTP) {
#pragma unroll
                            for (int i = 0; i < MTW; ++i)
                                pacc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ks & 1][jj], fa[ks & 1][i], pacc[i][jj], 0, 0, 0);
                        }
                    }
                }
            }
            W2_STAMP(10);                                  // projection MFMAs issued
            // ---- epilogue: + bias, DropPath scale, + shortcut, back to token order
#pragma unroll
            for (int jj = 0; jj < NTPW; ++jj) {
                const int t = pt(jj);
                if (pact && t < NTP) {
                    const int n = (NHG > 1 ? hg * OC : 0) + 16 * t + 4 * g;
#pragma unroll
                    for (int i = 0; i < MTW; ++i) {
                        if (tokm[i] >= 0) {
                            f32x4 v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = (pacc[i][jj][e] + pb4[jj][e]) * rsm[i] + (float)resid[i][jj][e];
                            if (poison) v = f32x4{NAN, NAN, NAN, NAN};
                            store4f(p.y + (long)tokm[i] * C + n, v);
                        }
                    }
                }
            }
        }
        if constexpr (NHG > 1) {
            // the last reader of the set re-arms its counters for the next launch
            if (tid == NT - 64 && done_ticket == NHG - 1) {
#pragma unroll
                for (int gq = 0; gq < NHG; ++gq) __hip_atomic_store(p.sync + W2_SYNC_FLAG(set, gq), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(p.sync + W2_SYNC_DONE(set), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();                                   // the LDS tiles are rewritten by the next unit
        W2_STAMP(11);
    }
}

template <int C, int W, int G, int GS, int NWV>
int launch2(Wmsa2Dev d, hipStream_t s) {
    using GM = W2Geom<C, W, G, GS>;
    if (d.nwin % W) return MVLT_ERR_UNSUPPORTED;
    const int nsets = d.nwin / W;
    d.nunits = nsets * GM::NHG;
    auto k = wmsa2_fwd_kernel<C, W, G, GS, NWV>;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, GM::bytes);
    (void)attr;
    static const int ncu = [] { int dev = 0, n = 256; if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n; }();
    // persistent, at most one workgroup per CU, a multiple of the group count: the groups of a set are in flight together
    int grid = d.nunits < ncu ? d.nunits : ncu / GM::NHG * GM::NHG;
    if (grid < GM::NHG) return MVLT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(k, dim3(grid), dim3(64 * NWV), GM::bytes, s, d);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

}  // namespace

#ifdef W2_TRACE
extern "C" int mvlt_swin_wmsa2_trace_buffer(void* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_w2_trace), &buf, sizeof(buf)) == hipSuccess ? MVLT_OK : MVLT_ERR_LAUNCH;
}
#endif

// which (W, G) the second design uses for a width / launch size; 0 = not covered (wmsa.hip or the unfused kernels run)
extern "C" int mvlt_swin_wmsa2_supported(int dtype, int B, int res, int C, int nH) {
    if (dtype != MVLT_BF16 || nH * 32 != C || res % 7) return 0;
    const int nwin = B * (res / 7) * (res / 7);
    if (nwin % 2) return 0;
    return C == 384 || C == 192 || C == 96;
}

// sync_ws: int32 [16 + 8 * (B nW / 2)], zeroed ONCE by the caller when it is allocated (every launch leaves its counters
// zeroed).  Word 0 is the sticky error count: a bounded hand-off wait ran out (never expected; the unit's rows of y are NaN).
// One workspace per stream: launches that may run concurrently must not share counters.
extern "C" int mvlt_swin_wmsa2_sync_words(int B, int res) { return 16 + W2_SYNC_STRIDE * (B * (res / 7) * (res / 7) / 2); }

// Bound of the hand-off wait (default 2000 ms; the tests shorten it to provoke the failure path).  Process-wide setting.
static std::atomic<long long> g_w2_spin_ticks{200000000LL};
extern "C" int mvlt_swin_wmsa2_set_timeout_ms(int ms) {
    MVLT_CHECK(ms >= 0, MVLT_ERR_ARG);
    g_w2_spin_ticks.store(ms > 0 ? (long long)ms * 100000LL : 200000000LL);
    return MVLT_OK;
}

extern "C" int mvlt_swin_wmsa2_fwd(const MvltSwinWmsa* p, int32_t* sync_ws, void* stream) {
    MVLT_CHECK(p && p->x && p->y && p->w2n && p->ln_gamma && p->ln_beta, MVLT_ERR_ARG);
    MVLT_CHECK(p->wqkv && p->bqkv && p->wproj && p->bproj && p->bias_table && p->attn_out && sync_ws, MVLT_ERR_ARG);
    MVLT_CHECK(p->B > 0 && p->res > 0 && p->res % 7 == 0 && p->shift >= 0 && p->shift < 7, MVLT_ERR_ARG);
    MVLT_CHECK(aligned16(p->x) && aligned16(p->y) && aligned16(p->wqkv) && aligned16(p->wproj) && aligned16(p->attn_out), MVLT_ERR_ARG);
    MVLT_CHECK(aligned16(p->ln_gamma) && aligned16(p->ln_beta) && aligned16(p->bqkv) && aligned16(p->bproj), MVLT_ERR_ARG);
    MVLT_CHECK((p->mean == nullptr) == (p->rstd == nullptr), MVLT_ERR_ARG);
    if (p->xn_win) MVLT_CHECK(aligned16(p->xn_win), MVLT_ERR_ARG);
    if (p->qkv_win) MVLT_CHECK(aligned16(p->qkv_win), MVLT_ERR_ARG);
    if (!mvlt_swin_wmsa2_supported(p->dtype, p->B, p->res, p->C, p->nH)) return MVLT_ERR_UNSUPPORTED;
    Wmsa2Dev d{};
    d.nW = (p->res / 7) * (p->res / 7);
    d.nwin = p->B * d.nW; d.res = p->res; d.shift = p->shift; d.nH = p->nH;
    d.x = reinterpret_cast<const T*>(p->x); d.y = reinterpret_cast<T*>(p->y); d.w2n = p->w2n;
    d.gamma = p->ln_gamma; d.beta = p->ln_beta; d.eps = p->ln_eps;
    d.wqkv = reinterpret_cast<const T*>(p->wqkv); d.bqkv = p->bqkv; d.wproj = reinterpret_cast<const T*>(p->wproj); d.bproj = p->bproj;
    d.bias_table = p->bias_table; d.scale = p->scale; d.rowscale = p->rowscale;
    d.xn = reinterpret_cast<T*>(p->xn_win); d.ao = reinterpret_cast<T*>(p->attn_out); d.qkv = reinterpret_cast<T*>(p->qkv_win);
    d.lse = p->lse; d.mean = p->mean; d.rstd = p->rstd;
    d.sync = sync_ws;
    d.spin_ticks = g_w2_spin_ticks.load();
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (p->C) {
        // 8 waves: 12 (three per SIMD, 168 registers) measured the same 30 us at stage 2 and spills
        case 384: return launch2<384, 2, 3, 3, 8>(d, s);    // stage 2: 12 heads in 4 groups
        case 192: return launch2<192, 2, 6, 3, 8>(d, s);    // stage 1: 6 heads in one workgroup, two passes of 3
        case 96:  return launch2<96, 2, 3, 3, 8>(d, s);     // stage 0
        default: return MVLT_ERR_UNSUPPORTED;
    }
}
