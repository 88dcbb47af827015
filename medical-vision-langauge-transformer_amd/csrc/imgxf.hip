// Fused image transform of the fine-tuning input pipeline (include/mvlt_hip.h: mvlt_image_transform).
//
// Pillow's 8-bit resize is two integer passes over tap tables (22-bit fixed point) that the host builds once per batch
// (data.py: plan_image_transform); torchvision's Resize -> RandomCrop -> RandomHorizontalFlip -> ToTensor -> Normalize only ever
// reads an O x O crop of the resized image.  The kernel evaluates the resize at the crop's pixels alone, straight from the
// source bytes: the tables hold just the crop's O columns and O rows, the resized image never exists.
//
// Design ("Image transform"): a workgroup owns a band of 8 output rows of one image; thread t < 3 * O owns table
// column tx = t / 3 and channel c = t % 3 of the band and walks the band's source rows r once.  Per row it runs the horizontal
// pass for its column (clip8 as Pillow rounds between the passes) and adds kv[y][r - ymin_y] * H to the register accumulator of
// every band row y whose vertical window holds r.  Nothing intermediate leaves the registers, there is no barrier in the loop,
// and the horizontal pass of a source row is redone only by the neighbouring band (1 + 2 * support / 8 times in all).
//  * lanes t = 3 * tx + c read src[r][(xmin_tx + i) * 3 + c]: the interleaved bytes of neighbouring columns, so a wave's 64 byte
//    loads of one tap fall into one or two runs of contiguous source bytes;
//  * the horizontal tables of the image sit in LDS as [tap][column] (lane-consecutive words; the three channel lanes of a column
//    read one word, a broadcast); the vertical coefficient of (y, r) is the same for the whole workgroup and comes in as a
//    scalar load;
//  * the band's result bytes go through LDS in the output's own order, so the stores are full 16-byte (f32 CHW, through the
//    [3, 256] normalisation table) or 4-byte (uint8 HWC) vectors of contiguous memory and the flip costs nothing.
#include "common.h"

namespace {

constexpr int IX_BAND = 8;                        // output rows per workgroup
constexpr int IX_MAX_O = 224;                     // output side: the kernel's thread count and staging area are sized for it
constexpr int IX_THREADS = 704;                   // 11 waves >= 3 * IX_MAX_O
constexpr int IX_ROWS = 4;                        // source rows in flight per thread
constexpr int IX_MAX_K = 65;                      // taps per output pixel and axis
constexpr int IX_STAGE = 3 * IX_BAND * IX_MAX_O;  // bytes of a band's result

struct ImgXf {
    const uint8_t* src; const int64_t* src_off; const int32_t* hw;
    const int32_t* bounds; const int32_t* coef; const uint8_t* flip; const float* lut;
    void* out; int O, kmax;
};

MVLT_DEV int clip8(int acc) { return min(max(acc >> 22, 0), 255); }

template <int MODE>
__global__ __launch_bounds__(IX_THREADS) void imgxf_kernel(const ImgXf a) {
    extern __shared__ __attribute__((aligned(16))) int smem[];
    int* kh = smem;                                                   // [kmax][O]: horizontal taps of this image; after the
    uint8_t* stage = reinterpret_cast<uint8_t*>(smem);                // passes the same bytes hold the band's result
    float* lut = reinterpret_cast<float*>(smem + IX_STAGE / 4);       // and the normalisation table
    const int O = a.O, kmax = a.kmax, tid = threadIdx.x;
    const int b = blockIdx.y, y0 = blockIdx.x * IX_BAND;
    const int32_t* hb = a.bounds + (long)b * 4 * O;                   // [2][O][2]
    const int32_t* vb = hb + 2 * O;
    const int32_t* hc = a.coef + (long)b * 2 * O * kmax;              // [2][O][kmax]
    const int32_t* vc = hc + (long)O * kmax;
    for (int i = tid; i < O * kmax; i += IX_THREADS) kh[(i % kmax) * O + i / kmax] = hc[i];
    __syncthreads();

    const int w = a.hw[2 * b + 1];
    const uint8_t* src = a.src + a.src_off[b];
    int ymn[IX_BAND], yn[IX_BAND], r0 = 0x7fffffff, r1 = 0;           // workgroup-uniform
#pragma unroll
    for (int q = 0; q < IX_BAND; ++q) {
        ymn[q] = vb[2 * (y0 + q)]; yn[q] = vb[2 * (y0 + q) + 1];
        r0 = min(r0, ymn[q]); r1 = max(r1, ymn[q] + yn[q]);
    }
    const int tx = tid / 3, c = tid - 3 * tx;
    const bool live = tid < 3 * O;
    const int xmin = live ? hb[2 * tx] : 0, xn = live ? hb[2 * tx + 1] : 0;
    // One trip count for the wave (its widest column): taps past a column's own count re-read its last pixel with the zero
    // coefficient the table is padded with, so the loop has no divergence and its byte loads can be issued ahead of the sums.
    int nmax = xn;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
    nmax = __builtin_amdgcn_readfirstlane(nmax);
    int acc[IX_BAND];
#pragma unroll
    for (int q = 0; q < IX_BAND; ++q) acc[q] = 1 << 21;
    if (live) {
        const uint8_t* col = src + (long)xmin * 3 + c;
        const int last = xn - 1;
        // IX_ROWS source rows per trip: their byte loads are independent, so a trip waits for memory once, not once per row.
        // A row past the band's last one re-reads that last row and lies in no vertical window, so it adds nothing.
        for (int r = r0; r < r1; r += IX_ROWS) {
            const uint8_t* px[IX_ROWS];
            int s[IX_ROWS];
#pragma unroll
            for (int u = 0; u < IX_ROWS; ++u) { px[u] = col + (long)min(r + u, r1 - 1) * w * 3; s[u] = 1 << 21; }
#pragma unroll 2
            for (int i = 0; i < nmax; ++i) {
                const int k = kh[i * O + tx], at = 3 * min(i, last);
#pragma unroll
                for (int u = 0; u < IX_ROWS; ++u) s[u] += k * (int)px[u][at];
            }
#pragma unroll
            for (int u = 0; u < IX_ROWS; ++u) {
                const int hv = clip8(s[u]);
#pragma unroll
                for (int q = 0; q < IX_BAND; ++q) {
                    const int j = r + u - ymn[q];
                    if (j >= 0 && j < yn[q]) acc[q] += vc[(long)(y0 + q) * kmax + j] * hv;
                }
            }
        }
    }
    __syncthreads();                                                  // every thread is done with kh
    if (MODE == MVLT_IMGXF_F32_CHW)
        for (int i = tid; i < 768; i += IX_THREADS) lut[i] = a.lut[i];
    if (live) {
        const int xo = a.flip[b] ? O - 1 - tx : tx;
#pragma unroll
        for (int q = 0; q < IX_BAND; ++q) {
            const uint8_t v = (uint8_t)clip8(acc[q]);
            if (MODE == MVLT_IMGXF_F32_CHW) stage[(c * IX_BAND + q) * O + xo] = v;
            else stage[(q * O + xo) * 3 + c] = v;
        }
    }
    __syncthreads();
    if (MODE == MVLT_IMGXF_F32_CHW) {
        const int per_c = IX_BAND * O / 4;                            // float4 per channel of the band (contiguous rows)
        float* out = reinterpret_cast<float*>(a.out);
        for (int i = tid; i < 3 * per_c; i += IX_THREADS) {
            const int cc = i / per_c, rem = i - cc * per_c;
            const uint32_t v = *reinterpret_cast<const uint32_t*>(stage + cc * IX_BAND * O + rem * 4);
            const float* t = lut + cc * 256;
            f32x4 o;
            o[0] = t[v & 255]; o[1] = t[(v >> 8) & 255]; o[2] = t[(v >> 16) & 255]; o[3] = t[v >> 24];
            store4f(out + (((long)b * 3 + cc) * O + y0) * O + rem * 4, o);
        }
    } else {
        uint32_t* out = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.out) + ((long)b * O + y0) * O * 3);
        for (int i = tid; i < IX_BAND * O * 3 / 4; i += IX_THREADS) out[i] = reinterpret_cast<const uint32_t*>(stage)[i];
    }
}

}  // namespace

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int mvlt_image_transform(const uint8_t* src, const int64_t* src_off, const int32_t* hw, const int32_t* bounds,
                                    const int32_t* coef, const uint8_t* flip, const float* lut, void* out, int B, int out_size,
                                    int kmax, int mode, void* stream) {
    MVLT_CHECK(src && src_off && hw && bounds && coef && flip && out, MVLT_ERR_ARG);
    MVLT_CHECK(B > 0 && B <= 65535 && kmax >= 1 && kmax <= IX_MAX_K, MVLT_ERR_ARG);
    MVLT_CHECK(out_size >= IX_BAND && out_size <= IX_MAX_O && out_size % IX_BAND == 0, MVLT_ERR_ARG);
    MVLT_CHECK(mode == MVLT_IMGXF_F32_CHW || mode == MVLT_IMGXF_U8_HWC, MVLT_ERR_ARG);
    MVLT_CHECK(mode != MVLT_IMGXF_F32_CHW || lut, MVLT_ERR_ARG);
    MVLT_CHECK(aligned16(out), MVLT_ERR_ARG);
    ImgXf a{src, src_off, hw, bounds, coef, flip, lut, out, out_size, kmax};
    const dim3 grid(out_size / IX_BAND, B);
    const size_t lds = max((size_t)kmax * out_size * sizeof(int), (size_t)IX_STAGE + 768 * sizeof(float));   // <= 58240 bytes
    if (mode == MVLT_IMGXF_F32_CHW) hipLaunchKernelGGL(imgxf_kernel<MVLT_IMGXF_F32_CHW>, grid, dim3(IX_THREADS), lds, STREAM(stream), a);
    else hipLaunchKernelGGL(imgxf_kernel<MVLT_IMGXF_U8_HWC>, grid, dim3(IX_THREADS), lds, STREAM(stream), a);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
