// Report metrics: the integers behind BLEU-1..4 and ROUGE-L, and the CIDEr score, of decoded WordPiece id rows against their
// reference reports, on the device (mvlt_report_ngram_keys, mvlt_report_stats; include/mvlt_hip.h).
//
// A workgroup (4 waves) owns one row (ngram_keys) or one (hypothesis, reference) pair (stats); a row holds at most 512 pieces.
//
// Segmentation.  The row ends before its first stop id.  Piece i carries three flag bits (CONT / JOIN / BREAK, 0 for an id outside
// the table).  Whether a JOIN piece glues to its left depends on its left neighbour only through a run of consecutive eligible JOIN
// pieces, in which every second one glues: the parity of the distance to the run's start decides, so every thread resolves its own
// piece (a run is one piece long in practice).  Word starts -> exclusive scan (two adjacent pieces per thread, wave shuffle scan,
// the four wave totals through LDS) -> the start piece of every word -> a thread per word folds its piece ids into a 64-bit key.
//
// Keys.  mix(x) is the splitmix64 finaliser (a bijection of 2^64); fold(h, v) = mix(h + 0x9E3779B97F4A7C15 + v).  A word is the fold
// of its piece ids from SEED_WORD, an n-gram the fold of its word keys from SEED_GRAM + n.  Keys travel as int64 bit patterns;
// INT64_MAX means "no key" (a key that happens to equal it becomes INT64_MAX - 1).
//
// Matching is all-pairs over the row (<= 512^2 compares per order, every thread reads the same LDS word: a broadcast), the LCS an
// anti-diagonal wavefront over three rolling diagonals, the document frequency a binary search in the sorted key table.  All
// floating-point work is f64 and every sum has a fixed order: a thread adds its positions in order, the wave adds by xor
// butterfly, the four wave totals are added as (0 + 1) + (2 + 3).  No atomics, no MFMA: this is integer compares and a few
// hundred f64 operations per pair, bound by LDS latency and barriers, not by any pipe's throughput.
//
// LDS per workgroup (static): ids 4 KB, flags 1 KB, word starts 2 KB, word keys 2 x 4 KB, n-gram keys 2 x 4 KB, three diagonals
// 6 KB: 29 KB of the 160 KB a CU has.
#include "common.h"
#include <cmath>

namespace {

constexpr int MAXP = 512, NT = 256;
constexpr int64_t NOKEY = INT64_MAX;
constexpr int F_CONT = 1, F_JOIN = 2, F_BREAK = 4;
constexpr uint64_t SEED_WORD = 0x243F6A8885A308D3ull, SEED_GRAM = 0x13198A2E03707344ull;

struct Stops { int64_t id[8]; int n; };

struct Seg {                       // scratch of one segmentation
    int64_t id[MAXP];
    uint8_t fl[MAXP], elig[MAXP];
    int wstart[MAXP];
    int red[4];
};

MVLT_DEV uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x;
}
MVLT_DEV uint64_t fold(uint64_t h, uint64_t v) { return mix64(h + 0x9E3779B97F4A7C15ull + v); }
MVLT_DEV int64_t as_key(uint64_t h) { const int64_t k = (int64_t)h; return k == NOKEY ? NOKEY - 1 : k; }

template <typename T> MVLT_DEV T wave_add(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the same total in every thread; `red` is 4 slots of LDS that nothing else uses
template <typename T> MVLT_DEV T block_add(T v, T* red) {
    v = wave_add(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
MVLT_DEV int block_min(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return min(min(red[0], red[1]), min(red[2], red[3]));
}

// JOIN piece i glues to its left: eligible, and at an even distance from the start of its run of eligible pieces
MVLT_DEV bool glues(const Seg& s, int i) {
    if (!s.elig[i]) return false;
    int b = i;
    while (b > 0 && s.elig[b - 1]) --b;
    return ((i - b) & 1) == 0;
}

// Words of row[0 .. T): their keys to wkey[0 .. nw), nw returned (the same in every thread).  Ends with a barrier.
MVLT_DEV int segment(const int64_t* row, int T, const uint8_t* flags, int V, const Stops& st, Seg& s, uint64_t* wkey) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int first_stop = T;
    for (int i = tid; i < T; i += NT) {
        const int64_t id = row[i];
        s.id[i] = id;
        bool stop = false;
        for (int q = 0; q < st.n; ++q) stop |= id == st.id[q];
        if (stop) first_stop = min(first_stop, i);
    }
    const int n = block_min(first_stop, s.red);
    for (int i = tid; i < MAXP; i += NT) {
        int f = 0;
        if (i < n && flags) { const int64_t id = s.id[i]; if (id >= 0 && id < (int64_t)V) f = flags[id]; }
        s.fl[i] = (uint8_t)f;
    }
    __syncthreads();
    for (int i = tid; i < MAXP; i += NT)
        s.elig[i] = (i > 0 && i < n - 1 && (s.fl[i] & F_JOIN) && !(s.fl[i + 1] & F_CONT)) ? 1 : 0;
    __syncthreads();
    int st2[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = 2 * tid + u;
        bool start = false;
        if (i < n) {
            const int f = s.fl[i];
            if (i == 0 || (f & F_BREAK)) start = true;
            else if (f & F_CONT) start = false;
            else start = !glues(s, i - 1) && !glues(s, i);
        }
        st2[u] = start ? 1 : 0;
    }
    const int mine = st2[0] + st2[1];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    __syncthreads();                                   // s.red free
    if (lane == 63) s.red[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += s.red[w];
    const int nw = s.red[0] + s.red[1] + s.red[2] + s.red[3];
    const int excl = base + incl - mine;
    if (st2[0]) s.wstart[excl] = 2 * tid;
    if (st2[1]) s.wstart[excl + st2[0]] = 2 * tid + 1;
    __syncthreads();
    for (int w = tid; w < nw; w += NT) {
        const int b = s.wstart[w], e = w + 1 < nw ? s.wstart[w + 1] : n;
        uint64_t h = SEED_WORD;
        for (int p = b; p < e; ++p) h = fold(h, (uint64_t)s.id[p]);
        wkey[w] = h;
    }
    __syncthreads();
    return nw;
}

// keys of the m = max(0, nw - k + 1) n-grams of order k; ends with a barrier
MVLT_DEV int gram_keys(const uint64_t* wkey, int nw, int k, int64_t* out) {
    const int m = max(0, nw - k + 1);
    for (int j = threadIdx.x; j < m; j += NT) {
        uint64_t h = SEED_GRAM + (uint64_t)k;
        for (int q = 0; q < k; ++q) h = fold(h, wkey[j + q]);
        out[j] = as_key(h);
    }
    __syncthreads();
    return m;
}

MVLT_DEV int count_of(const int64_t* keys, int m, int64_t key) {
    int c = 0;
    for (int j = 0; j < m; ++j) c += keys[j] == key ? 1 : 0;
    return c;
}
MVLT_DEV bool seen_before(const int64_t* keys, int j) {
    const int64_t key = keys[j];
    bool seen = false;
    for (int q = 0; q < j; ++q) seen |= keys[q] == key;
    return seen;
}

MVLT_DEV int df_lookup(const int64_t* keys, const int32_t* counts, int K, int64_t key) {
    int lo = 0, hi = K;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < K && keys[lo] == key) ? counts[lo] : 0;
}

__global__ __launch_bounds__(NT) void ngram_keys_kernel(const int64_t* ids, int64_t ld, int T, const uint8_t* flags, int V, Stops st,
                                                        int64_t* keys, int32_t* n_words) {
    __shared__ Seg seg;
    __shared__ uint64_t wkey[MAXP];
    __shared__ int64_t gk[MAXP];
    const int row = blockIdx.x;
    const int nw = segment(ids + (int64_t)row * ld, T, flags, V, st, seg, wkey);
    if (threadIdx.x == 0) n_words[row] = nw;
    for (int k = 1; k <= 4; ++k) {
        const int m = gram_keys(wkey, nw, k, gk);
        int64_t* out = keys + ((int64_t)row * 4 + (k - 1)) * T;
        for (int j = threadIdx.x; j < T; j += NT) out[j] = (j < m && !seen_before(gk, j)) ? gk[j] : NOKEY;
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void report_stats_kernel(const int64_t* hyp, int64_t ldh, int Th, const int64_t* ref, int64_t ldr,
                                                          int N, int Tr, const int32_t* index, const uint8_t* flags, int V, Stops st,
                                                          const int64_t* df_keys, const int32_t* df_counts, int K, int32_t* stats,
                                                          double* cider) {
    __shared__ Seg seg;
    __shared__ uint64_t hw[MAXP], rw[MAXP];
    __shared__ int64_t hk[MAXP], rk[MAXP];
    __shared__ int diag[3][MAXP + 4];
    __shared__ double redd[4];
    __shared__ int redi[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int r = index ? index[row] : row;
    const bool has_ref = r >= 0 && r < N;
    const int nh = segment(hyp + (int64_t)row * ldh, Th, flags, V, st, seg, hw);
    const int nr = has_ref ? segment(ref + (int64_t)r * ldr, Tr, flags, V, st, seg, rw) : 0;
    int32_t* out = stats + (int64_t)row * 11;
    if (tid == 0) { out[0] = nh; out[1] = has_ref ? nr : -1; }

    const double logN = log((double)N);
    const double delta = (double)(max(0, nh - 1) - max(0, nr - 1));          // the two bigram counts
    const double penalty = exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
    double score = 0.0;
    for (int k = 1; k <= 4; ++k) {
        const int mh = gram_keys(hw, nh, k, hk), mr = gram_keys(rw, nr, k, rk);
        int correct = 0;
        double dot = 0.0, h2 = 0.0, r2 = 0.0;
        for (int j = tid; j < mh; j += NT) {
            if (seen_before(hk, j)) continue;
            const int64_t key = hk[j];
            const int ch = count_of(hk, mh, key), cr = count_of(rk, mr, key);
            correct += min(ch, cr);
            const double idf = logN - log(fmax(1.0, (double)df_lookup(df_keys, df_counts, K, key)));
            const double vh = (double)ch * idf, vr = (double)cr * idf;
            dot += fmin(vh, vr) * vr;
            h2 += vh * vh;
        }
        for (int j = tid; j < mr; j += NT) {
            if (seen_before(rk, j)) continue;
            const int64_t key = rk[j];
            const double idf = logN - log(fmax(1.0, (double)df_lookup(df_keys, df_counts, K, key)));
            const double vr = (double)count_of(rk, mr, key) * idf;
            r2 += vr * vr;
        }
        correct = block_add(correct, redi);
        dot = block_add(dot, redd);
        h2 = block_add(h2, redd);
        r2 = block_add(r2, redd);
        if (h2 != 0.0 && r2 != 0.0) dot /= sqrt(h2) * sqrt(r2);
        score += dot * penalty;
        if (tid == 0) { out[1 + k] = correct; out[5 + k] = mh; }
        __syncthreads();                                // hk / rk are rewritten by the next order
    }
    if (tid == 0) cider[row] = score / 4.0 * 10.0;

    // LCS over words: cell (i, j), 1 <= i <= nh, 1 <= j <= nr, lies on diagonal d = i + j at index i; cells with i == 0 or j == 0 are 0
    int lcs = 0;
    if (nh > 0 && nr > 0) {
        for (int i = tid; i < 3 * (MAXP + 4); i += NT) (&diag[0][0])[i] = 0;
        __syncthreads();
        for (int d = 2; d <= nh + nr; ++d) {
            int* cur = diag[d % 3];
            const int* p1 = diag[(d + 2) % 3];
            const int* p2 = diag[(d + 1) % 3];
            const int lo = max(0, d - nr), hi = min(nh, d);
            for (int i = lo + tid; i <= hi; i += NT) {
                int v = 0;
                if (i != 0 && i != d) v = hw[i - 1] == rw[d - i - 1] ? p2[i - 1] + 1 : max(p1[i - 1], p1[i]);
                cur[i] = v;
            }
            __syncthreads();
        }
        lcs = diag[(nh + nr) % 3][nh];
    }
    if (tid == 0) out[10] = lcs;
}

Stops make_stops(const int64_t* stop_ids, int n) {
    Stops s{};
    s.n = n;
    for (int i = 0; i < n; ++i) s.id[i] = stop_ids[i];
    return s;
}

bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int mvlt_report_ngram_keys(const int64_t* ids, int64_t ld, int rows, int T, const uint8_t* flags, int V,
                                      const int64_t* stop_ids, int n_stop, int64_t* keys, int32_t* n_words, void* stream) {
    MVLT_CHECK(ids && keys && n_words && rows > 0 && T > 0 && T <= MAXP && ld >= T, MVLT_ERR_ARG);
    MVLT_CHECK(n_stop >= 0 && n_stop <= 8 && (n_stop == 0 || stop_ids) && (!flags || V > 0), MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(ids, 8) && aligned_to(keys, 8) && aligned_to(n_words, 4), MVLT_ERR_ARG);
    hipLaunchKernelGGL(ngram_keys_kernel, dim3(rows), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), ids, ld, T, flags, V,
                       make_stops(stop_ids, n_stop), keys, n_words);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}

extern "C" int mvlt_report_stats(const int64_t* hyp, int64_t ldh, int rows, int Th, const int64_t* ref, int64_t ldr, int N, int Tr,
                                 const int32_t* index, const uint8_t* flags, int V, const int64_t* stop_ids, int n_stop,
                                 const int64_t* df_keys, const int32_t* df_counts, int K, int32_t* stats, double* cider,
                                 void* stream) {
    MVLT_CHECK(hyp && ref && stats && cider && rows > 0 && N > 0, MVLT_ERR_ARG);
    MVLT_CHECK(Th > 0 && Th <= MAXP && Tr > 0 && Tr <= MAXP && ldh >= Th && ldr >= Tr, MVLT_ERR_ARG);
    MVLT_CHECK(index || rows <= N, MVLT_ERR_ARG);
    MVLT_CHECK(n_stop >= 0 && n_stop <= 8 && (n_stop == 0 || stop_ids) && (!flags || V > 0), MVLT_ERR_ARG);
    MVLT_CHECK(K >= 0 && (K == 0 || (df_keys && df_counts)), MVLT_ERR_ARG);
    MVLT_CHECK(aligned_to(hyp, 8) && aligned_to(ref, 8) && aligned_to(cider, 8) && aligned_to(stats, 4) && aligned_to(df_keys, 8) &&
               aligned_to(df_counts, 4) && aligned_to(index, 4), MVLT_ERR_ARG);
    hipLaunchKernelGGL(report_stats_kernel, dim3(rows), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), hyp, ldh, Th, ref, ldr, N,
                       Tr, index, flags, V, make_stops(stop_ids, n_stop), df_keys, df_counts, K, stats, cider);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
