// Order statistics and top-k means of anomaly maps: the robust frame scores between the mean of the map
// (a small defect barely moves it) and its maximum (one pixel) - the mean of the k largest pixels and the k-th largest pixel, for
// up to VAD_TOPK_MAX_RANKS ranks k per call.  The maps stay on the device; nothing is sorted and nothing is allocated.
//
// Semantics - specified so that numpy restates them (tests/map_topk_ref.py), kth to the bit:
//   order    pixels compare through the monotone key of their bits, key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), unsigned:
//            -inf < ... < -0.0 < +0.0 < ... < +inf;
//   kth      the pixel whose key is the k-th largest of the frame, its bits unchanged;
//   mean     (float)((S + (double)(k - c) * (double)v) / (double)k) with v = kth, c = the pixels with key > key(v), S = their float64
//            sum: every term of S is exact in double, so S is within c * 2^-53 * sum|x| of the exact sum in any order;
//   NaN      a frame with a NaN pixel gets 0x7FC00000 in every output (torch.amax's rule, frame_max's rule).
//
// A radix select over the key in three digit passes (11 / 11 / 10 bits), every pass one coalesced read of the frame by work-groups
// of 1024 threads; LDS holds one u32[2048] histogram per rank (NK * 8 KiB) and 1.1 KiB of scratch.
//   pass 1   histogram of key >> 21, shared by all ranks (one table); detects NaN.  Wave j then walks the table from the top and
//            picks rank j's digit: the highest bin at which the running count reaches the rank; the rank is reduced by the count
//            above the bin.
//   pass 2   per rank, histogram of (key >> 10) & 2047 over the pixels whose first digit is the rank's; pick as above.
//   pass 3   per rank, histogram of key & 1023 over the pixels whose first 22 bits are the rank's - a bin of this table is ONE key,
//            hence one value - and, in the same read, the float64 sum of the pixels whose first 22 bits are above the rank's: one
//            accumulator per thread and rank, folded by a butterfly over the wave and then over the 16 waves in wave order.
//   finish   wave j picks the last digit (the key is complete: kth), adds count[b] * value(b) over the bins b above it - exact
//            products, lanes strided over the bins, a butterfly - and then the partial sums in a fixed order: S.  c = k - (what is
//            left of the rank).  Lane 0 forms the mean and writes the outputs and the rank's record (value bits, c, S).
// Two paths by frame size (vad_topk_plan reports the boundary):
//   one work-group per frame, one launch (P <= TK_SPLIT_ABOVE): everything above in LDS;
//   split (larger frames, which one CU would read for milliseconds): the frame in slices of TK_SLICE pixels, one work-group each;
//            per pass a histogram launch - LDS tables flushed into the frame's tables in the workspace by integer atomics - and a
//            pick launch (one work-group per frame, which also clears the tables for the next pass); pass 3 leaves one float64
//            partial sum per slice and rank, which the finish adds in slice order.  Six launches and one memset.
// In both, thread t of a work-group reads pixels t, t + 1024, ... of its frame or slice: the assignment depends on nothing but the
// pixel's index in its frame, so a frame's partial sums - and with them every output word - are the same for any n, any position in
// the batch and any alignment of the frame.  Integer atomics on counters only; no float atomics.
#include <hip/hip_runtime.h>

#include <atomic>

#include "vad_args.h"
#include "vad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TK_THREADS = 1024, TK_WAVES = TK_THREADS / 64;
constexpr int TK_BINS = 2048;                                   // 11-bit digits (the last digit has 10 bits: half a table)
constexpr int TK_MAX = VAD_TOPK_MAX_RANKS;
constexpr unsigned TK_QNAN = 0x7FC00000u;
constexpr unsigned TK_SPLIT_ABOVE = 262144;                     // frames with more pixels take the split path
constexpr unsigned TK_SLICE = 32768;                            // pixels of one work-group of the split path

struct TopkRec { unsigned value_bits, above; double sum; };     // one per (frame, rank) in the workspace: 16 bytes
static_assert(sizeof(TopkRec) == 16, "the workspace holds 16 bytes per frame and rank");

struct TopkScratch {                                            // behind the histograms in LDS
    double part[TK_WAVES][TK_MAX];
    unsigned prefix[TK_MAX], rem[TK_MAX];
    unsigned nan;
};

struct TopkState { unsigned prefix[TK_MAX], rem[TK_MAX], nan, pad[3]; };   // split path: one per frame in the workspace
static_assert(sizeof(TopkState) == 80, "state records are 80 bytes");

struct TopkP {
    const float* maps;
    float* kth;                 // [frames, nk] or NULL
    float* mean;                // [frames, nk] or NULL
    TopkRec* rec;               // [frames, nk]
    unsigned pixels;
    unsigned ranks[TK_MAX];
    // split path only
    TopkState* state;           // [frames]
    unsigned* tables;           // [frames, nk, TK_BINS]
    double* part;               // [frames, slices, nk]
    unsigned slices;
};

// The workspace: records first (both paths), then - split path - states, tables and slice sums (byte offsets; [state, part) is
// zeroed before the first pass).
struct TopkCarve { size_t state, tables, part, total; unsigned slices; };
inline TopkCarve topk_carve(long long n, unsigned pixels, int nk) {
    TopkCarve c{};
    const size_t recs = (size_t)n * nk * sizeof(TopkRec);
    c.slices = pixels > TK_SPLIT_ABOVE ? (pixels + TK_SLICE - 1) / TK_SLICE : 0;
    c.state = recs;
    c.tables = c.state + (c.slices ? (size_t)n * sizeof(TopkState) : 0);
    c.part = c.tables + (c.slices ? (size_t)n * nk * TK_BINS * sizeof(unsigned) : 0);
    c.total = c.part + (size_t)n * c.slices * nk * sizeof(double);
    return c;
}

__device__ __forceinline__ unsigned topk_key(unsigned bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ unsigned topk_bits(unsigned key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

__device__ __forceinline__ double topk_wave_sum(double v) {     // butterfly: every lane ends with the same word
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// One wave walks a table of `bins` counters (a multiple of 64) from the top: -> the highest bin at which the count of this bin and
// all bins above reaches rem (1 <= rem <= the table's total); rem loses the count above that bin.  Same result in every lane.
__device__ __forceinline__ unsigned topk_pick(const unsigned* table, int bins, unsigned& rem, int lane) {
    unsigned run = 0;
    for (int top = bins - 1; top >= 0; top -= 64) {
        const unsigned cnt = table[top - lane];
        unsigned incl = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        const unsigned long long hit = __ballot(run + incl >= rem);
        if (hit) {
            const int l = __ffsll((long long)hit) - 1;
            rem -= run + __shfl(incl - cnt, l, 64);
            return (unsigned)(top - l);
        }
        run += __shfl(incl, 63, 64);
    }
    return 0;                                                   // not reached: the table holds at least rem keys
}

template <int NK> struct TopkPre { unsigned v[NK]; };         // the ranks' prefixes, by value: they stay in registers

// The streaming loop of every pass: pixels begin + tid, begin + tid + 1024, ... below end, four loads in flight per trip.
template <typename F>
__device__ __forceinline__ void topk_stream(const unsigned* __restrict__ src, unsigned begin, unsigned end, int tid, F&& each) {
    unsigned i = begin + tid;
    for (; i + 3 * TK_THREADS < end; i += 4 * TK_THREADS) {
        const unsigned b0 = src[i], b1 = src[i + TK_THREADS], b2 = src[i + 2 * TK_THREADS], b3 = src[i + 3 * TK_THREADS];
        each(b0);                                               // (spelled out: a loop over an array of four is not always unrolled
        each(b1);                                               // around a large body, and the array then lives in scratch)
        each(b2);
        each(b3);
    }
    for (; i < end; i += TK_THREADS) each(src[i]);
}

// pass 1 over [begin, end): the first digit into one table; -> did this thread see a NaN
__device__ __forceinline__ bool topk_pass1(const unsigned* __restrict__ src, unsigned begin, unsigned end, int tid, unsigned* hist) {
    bool nan = false;
    topk_stream(src, begin, end, tid, [&](unsigned b) __attribute__((always_inline)) {
        nan |= (b & 0x7FFFFFFFu) > 0x7F800000u;
        atomicAdd(&hist[topk_key(b) >> 21], 1u);
    });
    return nan;
}

// pass 2: per rank the second digit of the pixels whose first digit is pre[j]
template <int NK>
__device__ __forceinline__ void topk_pass2(const unsigned* __restrict__ src, unsigned begin, unsigned end, int tid, unsigned* hist,
                                           const TopkPre<NK> pre) {
    topk_stream(src, begin, end, tid, [&](unsigned b) __attribute__((always_inline)) {
        const unsigned k = topk_key(b);
#pragma unroll
        for (int j = 0; j < NK; ++j)
            if ((k >> 21) == pre.v[j]) atomicAdd(&hist[j * TK_BINS + ((k >> 10) & 2047u)], 1u);
    });
}

// pass 3: per rank the last digit of the pixels whose first 22 bits are pre[j] (tables `stride` apart), and the float64 sum of the
// pixels above; the wave sums go to sc.part[wave][rank]
template <int NK>
__device__ __forceinline__ void topk_pass3(const unsigned* __restrict__ src, unsigned begin, unsigned end, int tid, unsigned* hist, int stride,
                                           const TopkPre<NK> pre, TopkScratch& sc) {
    double acc[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) acc[j] = 0.0;
    topk_stream(src, begin, end, tid, [&acc, pre, hist, stride](unsigned b) __attribute__((always_inline)) {
        const unsigned k = topk_key(b), hi = k >> 10;
        const double x = (double)__uint_as_float(b);
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            if (hi == pre.v[j]) atomicAdd(&hist[j * stride + (k & 1023u)], 1u);
            if (hi > pre.v[j]) acc[j] = acc[j] + x;
        }
    });
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const double s = topk_wave_sum(acc[j]);
        if (lane == 0) sc.part[wv][j] = s;
    }
}

// The sum of a wave over the last digit's table: count[b] * value(b) for the bins above d.  Exact products: 23 + 24 bits.
__device__ __forceinline__ double topk_bins_above(const unsigned* table, unsigned hi, unsigned d, int lane) {
    double s = 0.0;
    for (unsigned b = lane; b < 1024u; b += 64u) {
        const unsigned cnt = table[b];
        if (b > d && cnt) s = s + (double)cnt * (double)__uint_as_float(topk_bits((hi << 10) | b));
    }
    return topk_wave_sum(s);
}

__device__ __forceinline__ void topk_write(const TopkP& p, size_t o, unsigned k, unsigned rem, unsigned key, double s) {
    const unsigned c = k - rem, vbits = topk_bits(key);
    if (p.kth) p.kth[o] = __uint_as_float(vbits);
    if (p.mean) p.mean[o] = (float)((s + (double)(k - c) * (double)__uint_as_float(vbits)) / (double)k);
    p.rec[o] = TopkRec{vbits, c, s};
}

__device__ __forceinline__ void topk_write_nan(const TopkP& p, size_t o) {
    if (p.kth) p.kth[o] = __uint_as_float(TK_QNAN);
    if (p.mean) p.mean[o] = __uint_as_float(TK_QNAN);
    p.rec[o] = TopkRec{TK_QNAN, 0u, __longlong_as_double(0x7FF8000000000000ll)};
}

// ---------------------------------------------------------------------------------------------- one work-group per frame
constexpr size_t topk_lds_bytes(int nk) { return (size_t)nk * TK_BINS * sizeof(unsigned) + sizeof(TopkScratch); }

template <int NK>
__global__ __launch_bounds__(TK_THREADS) void topk_kernel(TopkP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned tk_lds[];
    unsigned* hist = tk_lds;
    TopkScratch& sc = *(TopkScratch*)(tk_lds + NK * TK_BINS);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t frame = blockIdx.x;
    const unsigned* __restrict__ src = (const unsigned*)p.maps + frame * p.pixels;
    const unsigned P = p.pixels;

    // ---- pass 1: the first digit, one table for all ranks
    for (int i = tid; i < TK_BINS; i += TK_THREADS) hist[i] = 0;
    if (tid == 0) sc.nan = 0;
    __syncthreads();
    if (topk_pass1(src, 0, P, tid, hist)) sc.nan = 1;
    __syncthreads();
    if (sc.nan) {                                               // uniform over the work-group
        if (tid < NK) topk_write_nan(p, frame * NK + tid);
        return;
    }
    if (wv < NK) {
        unsigned rem = p.ranks[wv];
        const unsigned d = topk_pick(hist, TK_BINS, rem, lane);
        if (lane == 0) { sc.prefix[wv] = d; sc.rem[wv] = rem; }
    }
    __syncthreads();

    // ---- pass 2: the second digit, one table per rank
    TopkPre<NK> pre;
#pragma unroll
    for (int j = 0; j < NK; ++j) pre.v[j] = sc.prefix[j];
    for (int i = tid; i < NK * TK_BINS; i += TK_THREADS) hist[i] = 0;
    __syncthreads();
    topk_pass2<NK>(src, 0, P, tid, hist, pre);
    __syncthreads();
    if (wv < NK) {
        unsigned rem = sc.rem[wv];
        const unsigned d = topk_pick(hist + wv * TK_BINS, TK_BINS, rem, lane);
        if (lane == 0) { sc.prefix[wv] = (sc.prefix[wv] << 11) | d; sc.rem[wv] = rem; }
    }
    __syncthreads();

    // ---- pass 3: the last digit, and the sum of everything above the rank's 22-bit prefix
#pragma unroll
    for (int j = 0; j < NK; ++j) pre.v[j] = sc.prefix[j];
    for (int i = tid; i < NK * TK_BINS; i += TK_THREADS) hist[i] = 0;
    __syncthreads();
    topk_pass3<NK>(src, 0, P, tid, hist, TK_BINS, pre, sc);
    __syncthreads();

    // ---- finish: wave j completes rank j
    if (wv < NK) {
        unsigned rem = sc.rem[wv];
        const unsigned* table = hist + wv * TK_BINS;
        const unsigned d = topk_pick(table, 1024, rem, lane), hi = sc.prefix[wv];
        double s = topk_bins_above(table, hi, d, lane);
        for (int w = 0; w < TK_WAVES; ++w) s = s + sc.part[w][wv];
        if (lane == 0) topk_write(p, frame * NK + wv, p.ranks[wv], rem, (hi << 10) | d, s);
    }
}

// ---------------------------------------------------------------------------------------------- the split path
// LDS of the histogram launches: pass 1 one table, pass 2 NK tables (64 KiB at eight ranks: nothing else), pass 3 NK half tables
// and the scratch of the wave sums.
constexpr size_t topk_split_lds_bytes(int nk, int pass) {
    return pass == 1 ? TK_BINS * sizeof(unsigned) : pass == 2 ? (size_t)nk * TK_BINS * sizeof(unsigned) : (size_t)nk * 1024 * sizeof(unsigned) + sizeof(TopkScratch);
}

// grid (slices, frames): one slice of one frame into LDS tables, flushed into the frame's tables in the workspace.
template <int NK, int PASS>
__global__ __launch_bounds__(TK_THREADS) void topk_split_hist(TopkP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned tk_lds[];
    constexpr int STRIDE = PASS == 3 ? 1024 : TK_BINS, TABLES = PASS == 1 ? 1 : NK;
    unsigned* hist = tk_lds;
    const int tid = threadIdx.x;
    const size_t frame = blockIdx.y;
    const unsigned slice = blockIdx.x;
    TopkState* st = p.state + frame;
    if (PASS > 1 && st->nan) return;                            // uniform: written by the launch before this one
    const unsigned* __restrict__ src = (const unsigned*)p.maps + frame * p.pixels;
    const unsigned begin = slice * TK_SLICE, end = begin + TK_SLICE < p.pixels ? begin + TK_SLICE : p.pixels;
    for (int i = tid; i < TABLES * STRIDE; i += TK_THREADS) hist[i] = 0;
    __syncthreads();
    if (PASS == 1) {
        if (topk_pass1(src, begin, end, tid, hist)) atomicOr(&st->nan, 1u);
    } else {
        TopkPre<NK> pre;
#pragma unroll
        for (int j = 0; j < NK; ++j) pre.v[j] = st->prefix[j];
        if (PASS == 2) {
            topk_pass2<NK>(src, begin, end, tid, hist, pre);
        } else {
            TopkScratch& sc = *(TopkScratch*)(tk_lds + NK * 1024);
            topk_pass3<NK>(src, begin, end, tid, hist, STRIDE, pre, sc);
            __syncthreads();
            if (tid < NK) {
                double s = 0.0;
                for (int w = 0; w < TK_WAVES; ++w) s = s + sc.part[w][tid];
                p.part[(frame * p.slices + slice) * NK + tid] = s;
            }
        }
    }
    __syncthreads();
    unsigned* tables = p.tables + frame * NK * TK_BINS;
    for (int i = tid; i < TABLES * STRIDE; i += TK_THREADS) {
        const unsigned c = hist[i];
        if (c) atomicAdd(&tables[(i / STRIDE) * TK_BINS + (i % STRIDE)], c);
    }
}

// grid (frames): wave j picks rank j's digit of this pass from the frame's tables; passes 1 and 2 then clear the tables for the
// next histogram launch, pass 3 finishes the rank.
template <int NK, int PASS>
__global__ __launch_bounds__(TK_THREADS) void topk_split_pick(TopkP p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t frame = blockIdx.x;
    TopkState* st = p.state + frame;
    unsigned* tables = p.tables + frame * NK * TK_BINS;
    if (st->nan) {                                              // uniform; the tables are cleared by the next call's memset
        if (PASS == 3 && tid < NK) topk_write_nan(p, frame * NK + tid);
        return;
    }
    if (wv < NK) {
        unsigned rem = PASS == 1 ? p.ranks[wv] : st->rem[wv];
        const unsigned* table = tables + (PASS == 1 ? 0 : wv * TK_BINS);
        const unsigned d = topk_pick(table, PASS == 3 ? 1024 : TK_BINS, rem, lane);
        if (PASS < 3) {
            if (lane == 0) { st->prefix[wv] = PASS == 1 ? d : (st->prefix[wv] << 11) | d; st->rem[wv] = rem; }
        } else {
            const unsigned hi = st->prefix[wv];
            double s = topk_bins_above(table, hi, d, lane);
            const double* part = p.part + frame * p.slices * NK + wv;
            for (unsigned sl = 0; sl < p.slices; ++sl) s = s + part[(size_t)sl * NK];
            if (lane == 0) topk_write(p, frame * NK + wv, p.ranks[wv], rem, (hi << 10) | d, s);
        }
    }
    if (PASS < 3) {
        __syncthreads();                                        // every wave has read its table (pass 1: the one table)
        for (int i = tid; i < NK * TK_BINS; i += TK_THREADS) tables[i] = 0;
    }
}

typedef void (*TopkKernel)(TopkP);
#define TK_EACH_NK(K) {K<1>, K<2>, K<3>, K<4>, K<5>, K<6>, K<7>, K<8>}
#define TK_SPLIT_ROW(NK) {topk_split_hist<NK, 1>, topk_split_pick<NK, 1>, topk_split_hist<NK, 2>, topk_split_pick<NK, 2>, topk_split_hist<NK, 3>, topk_split_pick<NK, 3>}
const TopkKernel TOPK_KERNELS[TK_MAX] = TK_EACH_NK(topk_kernel);
const TopkKernel TOPK_SPLIT[TK_MAX][6] = {TK_SPLIT_ROW(1), TK_SPLIT_ROW(2), TK_SPLIT_ROW(3), TK_SPLIT_ROW(4),
                                          TK_SPLIT_ROW(5), TK_SPLIT_ROW(6), TK_SPLIT_ROW(7), TK_SPLIT_ROW(8)};

inline bool topk_n_ok(long long n) { return n <= (1ll << 56); }                     // n * nk * 16 bytes stay a size_t
inline bool topk_dims_ok(long long n, int h, int w, int nk) { return vad_map_dims_ok(n, h, w) && topk_n_ok(n) && nk >= 1 && nk <= TK_MAX; }
inline bool topk_apart(const void* a, size_t na, const void* b, size_t nb) {        // [a, a + na) and [b, b + nb) share no byte
    return (uintptr_t)a + na <= (uintptr_t)b || (uintptr_t)b + nb <= (uintptr_t)a;
}

// A launch with 64 KiB of dynamic LDS or more gets the attribute, once per process and kernel (setting it twice is harmless).
int topk_allow_lds(TopkKernel kernel, size_t lds, std::atomic<bool>& done) {
    if (lds >= 64 * 1024 && !done.load(std::memory_order_acquire)) {
        VAD_HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done.store(true, std::memory_order_release);
    }
    return VAD_OK;
}

}  // namespace

extern "C" int vad_topk_plan(int* split_above, int* slice_pixels) {
    if (split_above) *split_above = (int)TK_SPLIT_ABOVE;
    if (slice_pixels) *slice_pixels = (int)TK_SLICE;
    return VAD_OK;
}

extern "C" size_t vad_topk_workspace_bytes(long long n, int h, int w, int nk) {
    if (!topk_dims_ok(n, h, w, nk)) return 0;
    return topk_carve(n, (unsigned)(h * w), nk).total;
}

extern "C" int vad_map_topk(const float* maps, long long n, int h, int w, const unsigned* ranks, int nk, float* kth, float* topk_mean,
                            void* ws, size_t ws_bytes, void* stream) {
    const char* who = "map_topk";
    VAD_ARG(vad_req_map_dims(who, n, h, w));
    VAD_REQUIRE(topk_n_ok(n), "%s: n=%lld is out of range (at most 2^56 frames)", who, n);
    VAD_REQUIRE(nk >= 1 && nk <= TK_MAX, "%s: nk must be in 1..%d, got %d", who, TK_MAX, nk);
    VAD_ARG(vad_req_nonnull(who, "ranks", ranks));
    const unsigned pixels = (unsigned)(h * w);
    for (int j = 0; j < nk; ++j)
        VAD_REQUIRE(ranks[j] >= 1u && ranks[j] <= pixels, "%s: ranks[%d] must be in 1..%u (h * w), got %u", who, j, pixels, ranks[j]);
    VAD_REQUIRE(kth != nullptr || topk_mean != nullptr, "%s: kth and topk_mean are both NULL", who);
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_aligned(who, "kth", kth, 4));
    VAD_ARG(vad_req_aligned(who, "topk_mean", topk_mean, 4));
    const size_t map_bytes = (size_t)n * pixels * sizeof(float), out_bytes = (size_t)n * nk * sizeof(float);
    VAD_REQUIRE(kth == nullptr || topk_apart(maps, map_bytes, kth, out_bytes), "%s: kth overlaps maps", who);
    VAD_REQUIRE(topk_mean == nullptr || topk_apart(maps, map_bytes, topk_mean, out_bytes), "%s: topk_mean overlaps maps", who);
    const TopkCarve carve = topk_carve(n, pixels, nk);
    if (carve.total) {
        VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
        VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, carve.total, "vad_topk_workspace_bytes(%lld, %d, %d, %d)", n, h, w, nk);
    }
    if (n == 0) return VAD_OK;

    const hipStream_t s = (hipStream_t)stream;
    TopkP p{};
    p.pixels = pixels;
    for (int j = 0; j < TK_MAX; ++j) p.ranks[j] = j < nk ? ranks[j] : 1u;
    if (!carve.slices) {                                                            // one work-group per frame, one launch
        static std::atomic<bool> allowed;
        const size_t lds = topk_lds_bytes(nk);
        VAD_ARG(topk_allow_lds(TOPK_KERNELS[nk - 1], lds, allowed));
        for (long long f0 = 0; f0 < n; f0 += (1ll << 30)) {                         // frames in slices of gridDim.x
            const unsigned m = (unsigned)(n - f0 < (1ll << 30) ? n - f0 : (1ll << 30));
            p.maps = maps + (size_t)f0 * pixels;
            p.kth = kth ? kth + (size_t)f0 * nk : nullptr;
            p.mean = topk_mean ? topk_mean + (size_t)f0 * nk : nullptr;
            p.rec = (TopkRec*)ws + (size_t)f0 * nk;
            hipLaunchKernelGGL(TOPK_KERNELS[nk - 1], dim3(m), dim3(TK_THREADS), lds, s, p);
            VAD_LAUNCH_CHECK();
        }
        return VAD_OK;
    }

    // the split path: states and tables cleared, then histogram and pick launches pass by pass, frames in slices of gridDim.y
    char* base = (char*)ws;
    VAD_HIP_TRY(hipMemsetAsync(base + carve.state, 0, carve.part - carve.state, s));
    p.slices = carve.slices;
    for (int step = 0; step < 6; ++step) {
        const bool hist = (step & 1) == 0;
        const TopkKernel kernel = TOPK_SPLIT[nk - 1][step];
        const size_t lds = hist ? topk_split_lds_bytes(nk, step / 2 + 1) : 0;
        static std::atomic<bool> allowed;                                           // one kernel reaches 64 KiB: pass 2 at eight ranks
        VAD_ARG(topk_allow_lds(kernel, lds, allowed));
        for (long long f0 = 0; f0 < n; f0 += 65535) {
            const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
            p.maps = maps + (size_t)f0 * pixels;
            p.kth = kth ? kth + (size_t)f0 * nk : nullptr;
            p.mean = topk_mean ? topk_mean + (size_t)f0 * nk : nullptr;
            p.rec = (TopkRec*)ws + (size_t)f0 * nk;
            p.state = (TopkState*)(base + carve.state) + f0;
            p.tables = (unsigned*)(base + carve.tables) + (size_t)f0 * nk * TK_BINS;
            p.part = (double*)(base + carve.part) + (size_t)f0 * carve.slices * nk;
            hipLaunchKernelGGL(kernel, hist ? dim3(carve.slices, m) : dim3(m), dim3(TK_THREADS), lds, s, p);
            VAD_LAUNCH_CHECK();
        }
    }
    return VAD_OK;
}
