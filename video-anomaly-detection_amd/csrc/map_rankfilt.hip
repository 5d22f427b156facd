// Rank filters of anomaly maps with a rectangular window: the sliding-window median and its generalisation,
// the r-th smallest value of the window - the denoiser of impulsive residual noise (single hot pixels on edges, gloss, sensor
// noise) that neither a Gaussian (spreads an impulse) nor an opening (eats corners, biased low) is.  Erosion and dilation
// (map_morph.hip) are its two end ranks; this is the middle of the family.
//
// Semantics - scipy.ndimage.rank_filter(x, rank=r, size=(size_h, size_w), mode="reflect"); median_filter is r = n / 2 (n = size_h *
// size_w; the upper median of an even n), percentile_filter(p) is r = n - 1 for p == 100, else (int)((double)n * p / 100):
//   out[y][x] = the r-th smallest (0-based) of { x[R(y - size_h/2 + i, H)][R(x - size_w/2 + j, W)] : i < size_h, j < size_w }
//   R(i, L): m = i mod 2L (non-negative);  m < L ? m : 2L - 1 - m          (d c b a | a b c d | d c b a, periodic)
// Even sizes lean towards index 0, as VAD_MORPH_ERODE does.  A reflected pixel counts as often as it appears in the window - a rank,
// unlike a minimum, cannot clamp its window -, and a window larger than the frame reflects several times.  Rank 0 is grey_erosion
// at every size; rank n - 1 is grey_dilation at ODD sizes only (scipy's dilation mirrors the origin of an even element).
// Nothing is computed, only selected: the order is that of the monotone key of map_topk.hip (key = bits ^ (bits >> 31 ? 0xFFFFFFFF
// : 0x80000000), unsigned: -0 below +0, denormals and +-Inf ordinary values), the result is one of the window's values with its
// bits unchanged, and a window that holds a NaN gives NaN whatever the rank (as morph_maps does; scipy's answer there is an accident
// of its selection algorithm).  tests/rank_filter_ref.py restates it to the bit.
//
// Tiling: one work-group of 256 threads per RF_TH x RF_TW = 16 x 64 output tile, one launch.
//   stage   K[r][c] <- key of pixel (R(y0 - size_h/2 + r, H), R(x0 - size_w/2 + c, W)) for the tile and its halo (size - 1 rows /
//           columns), NaN as the key 0xFFFFFFFF that no other float has; lanes along x, a row per wave.  The reflection is resolved
//           here, so the selection never sees a border;
//   select  a thread owns the two vertically adjacent outputs (2q, lane), (2q + 1, lane) of row pair q - lanes along x, so the 64
//           lanes of every LDS read fall on consecutive banks at any pitch.  A bitwise binary search over the 32-bit key, most
//           significant bit first: with the bits above b decided (res), the candidate is res | 1 << b, one pass counts the window's
//           keys below it, and the bit is kept if that count is <= r: after 32 passes res is the largest v with #(key < v) <= r,
//           which is the r-th smallest key.  The two outputs share the size_h - 1 rows their windows have in common: a key read
//           once from LDS is compared with both candidates (size_h + 1 rows of reads for two outputs, n compares each).  One more
//           pass in front takes the maximum key of each window: 0xFFFFFFFF there means a NaN, which overrides the rank;
//   store   rows with lanes along x.
// Every pass is the same trip count for every lane (no divergence), the window's width is a template parameter (the reads of a
// row are unrolled: immediate offsets, all in flight together), its height a loop.  Cost per output: 33 n LDS-read-equivalents /
// 2 and 2 x 32 n + n VALU operations (compare, add-with-carry) - VALU-bound; section 4.26 has the estimate against the measurement.
// Registers hold two candidates and two counts, not the window: no scratch at any size.
#include <hip/hip_runtime.h>

#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int RF_TH = 16, RF_TW = 64;
constexpr int RF_THREADS = 256;
constexpr int RF_WAVES = RF_THREADS / 64;
constexpr int RF_MAX_ROWS = RF_TH + VAD_RANKFILT_MAX_SIZE - 1;
constexpr unsigned RF_NAN_KEY = 0xFFFFFFFFu;       // key(0x7FFFFFFF), a NaN: no number has it

__device__ __forceinline__ unsigned rf_key(unsigned bits) {
    const unsigned k = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return (bits & 0x7FFFFFFFu) > 0x7F800000u ? RF_NAN_KEY : k;
}
__device__ __forceinline__ unsigned rf_bits(unsigned key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// scipy's mode="reflect" of index i on an axis of length len (2 * len fits: len <= VAD_MAX_FRAME_PIXELS)
__device__ __forceinline__ int rf_reflect(int i, int len) {
    if ((unsigned)i < (unsigned)len) return i;
    const int p = 2 * len;
    int m = i % p;
    if (m < 0) m += p;
    return m < len ? m : p - 1 - m;
}

struct RankP {
    const float* maps;
    float* out;
    int h, w, sh, rank;
    int tiles_x;
};

template <int SW> __global__ __launch_bounds__(RF_THREADS) void rankfilt_kernel(RankP p) {
    constexpr int COLS = RF_TW + SW - 1;                       // the pitch of K
    __shared__ unsigned K[RF_MAX_ROWS * COLS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int y0 = ty * RF_TH, x0 = tx * RF_TW;
    const size_t frame = blockIdx.y;
    const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(p.maps) + frame * (size_t)p.h * p.w;
    float* __restrict__ dst = p.out + frame * (size_t)p.h * p.w;
    const int sh = p.sh, rows = RF_TH + sh - 1;

    // stage (every index is reflected into the frame: no load is out of bounds, whatever the tile)
    const int ay = y0 - sh / 2, ax = x0 - SW / 2;
    for (int c = lane; c < COLS; c += 64) {
        const unsigned* col = src + rf_reflect(ax + c, p.w);
#pragma unroll 4
        for (int r = wv; r < rows; r += RF_WAVES) K[r * COLS + c] = rf_key(col[(size_t)rf_reflect(ay + r, p.h) * p.w]);
    }
    __syncthreads();

    const unsigned rank = (unsigned)p.rank;
    const int gx = x0 + lane;
    for (int q = wv; q < RF_TH / 2; q += RF_WAVES) {
        const int gy = y0 + 2 * q;
        if (gy >= p.h) break;                                  // (uniform over the wave)
        // window of output 0: rows 2q .. 2q + sh - 1 of K, of output 1: one row further down; columns lane .. lane + SW - 1
        const unsigned* top = K + (2 * q) * COLS + lane;
        const unsigned* bot = top + sh * COLS;
        unsigned mt = 0u, mm = 0u, mb = 0u;                    // maxima of the first row, the shared rows, the last row
#pragma unroll
        for (int j = 0; j < SW; ++j) {
            mt = max(mt, top[j]);
            mb = max(mb, bot[j]);
        }
        for (int i = 1; i < sh; ++i) {
            const unsigned* row = top + i * COLS;
#pragma unroll
            for (int j = 0; j < SW; ++j) mm = max(mm, row[j]);
        }
        const bool nan0 = max(mt, mm) == RF_NAN_KEY, nan1 = max(mm, mb) == RF_NAN_KEY;

        unsigned res0 = 0u, res1 = 0u;
        for (int b = 31; b >= 0; --b) {
            const unsigned c0 = res0 | (1u << b), c1 = res1 | (1u << b);
            unsigned n0 = 0u, n1 = 0u;
#pragma unroll
            for (int j = 0; j < SW; ++j) {
                n0 += top[j] < c0 ? 1u : 0u;
                n1 += bot[j] < c1 ? 1u : 0u;
            }
            for (int i = 1; i < sh; ++i) {
                const unsigned* row = top + i * COLS;
#pragma unroll
                for (int j = 0; j < SW; ++j) {
                    const unsigned k = row[j];
                    n0 += k < c0 ? 1u : 0u;
                    n1 += k < c1 ? 1u : 0u;
                }
            }
            if (n0 <= rank) res0 = c0;
            if (n1 <= rank) res1 = c1;
        }
        if (gx < p.w) {
            dst[(size_t)gy * p.w + gx] = nan0 ? __uint_as_float(0x7FC00000u) : __uint_as_float(rf_bits(res0));
            if (gy + 1 < p.h) dst[(size_t)(gy + 1) * p.w + gx] = nan1 ? __uint_as_float(0x7FC00000u) : __uint_as_float(rf_bits(res1));
        }
    }
}

template <int SW> int rankfilt_launch(const RankP& base, long long n, void* stream) {
    RankP p = base;
    const size_t fs = (size_t)p.h * p.w;
    const long long tiles = (long long)((p.h + RF_TH - 1) / RF_TH) * p.tiles_x;
    for (long long f0 = 0; f0 < n; f0 += 65535) {                                               // frames in slices of gridDim.y
        const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
        p.maps = base.maps + (size_t)f0 * fs;
        p.out = base.out + (size_t)f0 * fs;
        hipLaunchKernelGGL(rankfilt_kernel<SW>, dim3((unsigned)tiles, m), dim3(RF_THREADS), 0, (hipStream_t)stream, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

}  // namespace

extern "C" int vad_rankfilt_tile(int size_h, int size_w, int* tile_h, int* tile_w) {
    VAD_REQUIRE(size_h >= 1 && size_h <= VAD_RANKFILT_MAX_SIZE && size_w >= 1 && size_w <= VAD_RANKFILT_MAX_SIZE,
                "rankfilt_tile: size must be in 1..%d per side, got %dx%d", VAD_RANKFILT_MAX_SIZE, size_h, size_w);
    if (tile_h) *tile_h = RF_TH;                                                                // one tile and one selection route
    if (tile_w) *tile_w = RF_TW;                                                                // for every size
    return VAD_OK;
}

extern "C" int vad_rankfilt_maps(const float* maps, long long n, int h, int w, int size_h, int size_w, int rank, float* out, void* stream) {
    VAD_REQUIRE(size_h >= 1 && size_h <= VAD_RANKFILT_MAX_SIZE && size_w >= 1 && size_w <= VAD_RANKFILT_MAX_SIZE,
                "rankfilt_maps: size must be in 1..%d per side, got %dx%d", VAD_RANKFILT_MAX_SIZE, size_h, size_w);
    VAD_REQUIRE(rank >= 0 && rank < size_h * size_w, "rankfilt_maps: rank must be in 0..%d (a window of %dx%d), got %d", size_h * size_w - 1,
                size_h, size_w, rank);
    VAD_ARG(vad_req_map_dims("rankfilt_maps", n, h, w));
    VAD_REQUIRE(maps != nullptr && out != nullptr, "rankfilt_maps: maps or out is NULL");
    VAD_REQUIRE(vad_aligned(maps, 4) && vad_aligned(out, 4), "rankfilt_maps: maps and out must be 4-byte aligned");
    VAD_REQUIRE(vad_disjoint(maps, out, (size_t)n * h * w * sizeof(float)),
                "rankfilt_maps: out overlaps maps (a pixel's window reads its neighbours: not in place)");
    if (n == 0) return VAD_OK;

    RankP p;
    p.maps = maps;
    p.out = out;
    p.h = h;
    p.w = w;
    p.sh = size_h;
    p.rank = rank;
    p.tiles_x = (w + RF_TW - 1) / RF_TW;
    switch (size_w) {
#define RF_CASE(S) case S: return rankfilt_launch<S>(p, n, stream)
        RF_CASE(1); RF_CASE(2); RF_CASE(3); RF_CASE(4); RF_CASE(5); RF_CASE(6); RF_CASE(7); RF_CASE(8);
        RF_CASE(9); RF_CASE(10); RF_CASE(11); RF_CASE(12); RF_CASE(13); RF_CASE(14);
#undef RF_CASE
        default: return rankfilt_launch<15>(p, n, stream);
    }
}
