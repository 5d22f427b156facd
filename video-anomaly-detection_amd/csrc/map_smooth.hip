// Gaussian smoothing of anomaly maps and the per-frame maximum of the smoothed map: the step every
// MVTec-style evaluation takes between the error map and the ranking metrics (scipy.ndimage.gaussian_filter, sigma = 4, then the
// image score = max of the map).  The maps stay on the device between score_all and the histograms.
//
// Arithmetic - specified so that numpy float32 restates it bit for bit (tests/map_smooth_ref.py):
//   taps     n = 2 r + 1 fp32 weights made on the host (metrics.gaussian_taps: scipy's, float64, normalised, rounded once); no exp here;
//   borders  scipy's mode="reflect" (d c b a | a b c d | d c b a): index -k -> k - 1, index n - 1 + k -> n - k; one reflection only,
//            so r <= min(H, W) (the host refuses anything else);
//   order    first along H, then along W; each pass  acc = fl(w[0] x[0]);  acc = fl(acc + fl(w[k] x[k]))  for k = 1 .. 2r ascending,
//            every product and every sum rounded to fp32 on its own: this file is compiled with contraction off (hip.py) and says
//            so itself (the pragma below); the first pass's result is fp32.
// Non-finite values need no code: a NaN makes exactly the pixels whose (reflected) window holds it NaN; every tap is > 0, so +Inf
// spreads as +Inf and creates no NaN.  The maximum is the IEEE `maximum` (vad_vmax): NaN if any smoothed pixel of the frame is.
//
// Tiling: one work-group of 256 threads per SM_TH x SM_TW = 32 x 64 output tile, both passes through LDS, one launch.
//   stage   A[32 + 2r][64 + 2r] <- the tile and its halo, the reflection resolved per row (wave-uniform) and per column (once per
//           lane); rows and columns of a ragged tile that only feed pixels outside the frame are clamped into it;
//   H pass  thread = (8-row strip, column PAIR 2p, 2p+1), strip-major so the items fill whole waves: an 8-row window of float2
//           slides down A (one 8-byte LDS read and 8 + 8 packed multiplies / adds per tap, consecutive lanes on consecutive
//           banks) -> B[32][64 + 2r];
//   W pass  thread = (row PAIR, 8 columns), the first 128 threads: an 8-column window of float2 (the two rows) slides along B
//           (two 4-byte reads and 8 + 8 packed multiplies / adds per tap; B's pitch is 1 mod 4, so the row pairs of a wave fall
//           on different banks and a read is 2-way conflicted at most) -> C[32][64] (over A, which is dead behind the barrier
//           that closes the H pass);
//   store   rows of C with lanes along x (256-byte runs), and the tile's maximum over the pixels inside the frame.
// The tile maxima go to the workspace (one float per tile) and smooth_max_kernel folds a frame's tiles: compare-only, so the
// result is the same for every batching, launch order and tiling.
#include <hip/hip_runtime.h>

#include <atomic>

#include "vad_args.h"
#include "vad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SM_TH = 32, SM_TW = 64;          // hip.py SMOOTH_TILE
constexpr int SM_THREADS = 256;
constexpr int SM_STRIP = 8;                    // outputs per thread and pass
constexpr int SM_CPITCH = SM_TW + 1;

struct SmoothGeo {
    int rows, cols;      // of A: SM_TH + 2r, SM_TW + 2r
    int pa, pb;          // pitches of A and B in floats
    size_t lds_bytes;
};

__host__ __device__ inline SmoothGeo smooth_geo(int r) {
    SmoothGeo g;
    g.rows = SM_TH + 2 * r;
    g.cols = SM_TW + 2 * r;
    g.pa = g.cols;                              // even: the H pass reads float2 at even columns
    g.pb = ((g.cols + 3) & ~3) + 1;
    g.lds_bytes = ((size_t)g.rows * g.pa + (size_t)SM_TH * g.pb) * sizeof(float);
    return g;
}

// scipy's "reflect" for one reflection; a coordinate further out (it can only feed pixels outside the frame) is clamped
__device__ __forceinline__ int smooth_reflect(int g, int n) {
    int i = g < 0 ? -g - 1 : (g >= n ? 2 * n - 1 - g : g);
    i = i < 0 ? 0 : i;
    return i > n - 1 ? n - 1 : i;
}

struct SmoothP {
    const float* maps;
    const float* taps;
    float* out;           // may be NULL
    float* tile_max;      // [frames][tiles], may be NULL
    int h, w, r;
    int tiles_x, tiles;
};

__global__ __launch_bounds__(SM_THREADS) void smooth_kernel(SmoothP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float wave_max[SM_THREADS / 64];
    const SmoothGeo g = smooth_geo(p.r);
    float* A = lds;
    float* B = lds + g.rows * g.pa;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: row indices and their reflection stay on the scalar unit
    const int tile = blockIdx.x, ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int y0 = ty * SM_TH, x0 = tx * SM_TW;
    const size_t frame = blockIdx.y;
    const float* __restrict__ src = p.maps + frame * (size_t)p.h * p.w;
    const float* __restrict__ taps = p.taps;
    const int ntaps = 2 * p.r + 1;

    for (int cx = lane; cx < g.cols; cx += 64) {
        const float* col = src + smooth_reflect(x0 - p.r + cx, p.w);
        float* a = A + cx;
#pragma unroll 8
        for (int ry = wv; ry < g.rows; ry += SM_THREADS / 64) {
            const int gy = smooth_reflect(y0 - p.r + ry, p.h);
            a[ry * g.pa] = col[gy * p.w];
        }
    }
    __syncthreads();

    const float w0 = taps[0];
    // H pass: work item = (8-row strip, column pair), strip-major over the threads, so that the items fill whole waves (96 columns:
    // three full waves and an idle one, not four waves at 48 lanes)
    const int pairs = g.cols >> 1;
    const int strip = (tid >= pairs) + (tid >= 2 * pairs) + (tid >= 3 * pairs);
    if (tid < (SM_TH / SM_STRIP) * pairs) {
        const int pair = tid - strip * pairs;
        const float* a = A + (strip * SM_STRIP) * g.pa + 2 * pair;
        f32x2 win[SM_STRIP], acc[SM_STRIP];
#pragma unroll
        for (int j = 0; j < SM_STRIP; ++j) {
            win[j] = *(const f32x2*)(a + j * g.pa);
            acc[j] = win[j] * w0;
        }
        const float* nxt = a + SM_STRIP * g.pa;
#pragma unroll 8
        for (int k = 1; k < ntaps; ++k) {
#pragma unroll
            for (int j = 0; j < SM_STRIP - 1; ++j) win[j] = win[j + 1];
            win[SM_STRIP - 1] = *(const f32x2*)nxt;
            nxt += g.pa;
            const float wk = taps[k];
#pragma unroll
            for (int j = 0; j < SM_STRIP; ++j) acc[j] = acc[j] + win[j] * wk;
        }
        float* b = B + (strip * SM_STRIP) * g.pb + 2 * pair;
#pragma unroll
        for (int j = 0; j < SM_STRIP; ++j) {
            b[j * g.pb] = acc[j][0];
            b[j * g.pb + 1] = acc[j][1];
        }
    }
    __syncthreads();

    // W pass: work item = (row PAIR, 8-column strip): the two rows are the halves of the packed operations, so a window element
    // is two 4-byte reads into one register pair and nothing has to be moved to form the packed operands
    if (tid < (SM_TH / 2) * (SM_TW / SM_STRIP)) {
        const int rp = tid >> 3, lx = tid & 7;
        const float* b0 = B + (2 * rp) * g.pb + SM_STRIP * lx;
        const float* b1 = b0 + g.pb;
        f32x2 win[SM_STRIP], acc[SM_STRIP];
#pragma unroll
        for (int j = 0; j < SM_STRIP; ++j) {
            win[j] = f32x2{b0[j], b1[j]};
            acc[j] = win[j] * w0;
        }
#pragma unroll 8
        for (int k = 1; k < ntaps; ++k) {
#pragma unroll
            for (int j = 0; j < SM_STRIP - 1; ++j) win[j] = win[j + 1];
            win[SM_STRIP - 1] = f32x2{b0[SM_STRIP - 1 + k], b1[SM_STRIP - 1 + k]};
            const float wk = taps[k];
#pragma unroll
            for (int j = 0; j < SM_STRIP; ++j) acc[j] = acc[j] + win[j] * wk;
        }
        float* c0 = A + (2 * rp) * SM_CPITCH + SM_STRIP * lx;
#pragma unroll
        for (int j = 0; j < SM_STRIP; ++j) {
            c0[j] = acc[j][0];
            c0[SM_CPITCH + j] = acc[j][1];
        }
    }
    __syncthreads();

    float m = -INFINITY;
    const int gx = x0 + lane;
    float* __restrict__ dst = p.out ? p.out + frame * (size_t)p.h * p.w : nullptr;
#pragma unroll
    for (int y = wv; y < SM_TH; y += SM_THREADS / 64) {
        const int gy = y0 + y;
        if (gx < p.w && gy < p.h) {
            const float v = A[y * SM_CPITCH + lane];
            m = vad_vmax(m, v);
            if (dst) dst[gy * p.w + gx] = v;
        }
    }
    if (p.tile_max) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = vad_vmax(m, __shfl_xor(m, off, 64));
        if (lane == 0) wave_max[wv] = m;
        __syncthreads();
        if (tid == 0) p.tile_max[frame * p.tiles + tile] = vad_vmax4(wave_max[0], wave_max[1], wave_max[2], wave_max[3]);
    }
}

// frame_max[f] = the maximum of the frame's tile maxima: one wave per frame.
__global__ __launch_bounds__(64) void smooth_max_kernel(const float* tile_max, int tiles, float* frame_max) {
    const size_t f = blockIdx.x;
    const float* t = tile_max + f * tiles;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < tiles; i += 64) m = vad_vmax(m, t[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = vad_vmax(m, __shfl_xor(m, off, 64));
    if (threadIdx.x == 0) frame_max[f] = m;
}

inline bool smooth_dims_ok(long long n, int h, int w, int radius) {
    return vad_map_dims_ok(n, h, w) && radius >= 1 && radius <= VAD_SMOOTH_MAX_RADIUS && radius <= h && radius <= w;
}

inline long long smooth_tiles(int h, int w) { return (long long)((h + SM_TH - 1) / SM_TH) * ((w + SM_TW - 1) / SM_TW); }

}  // namespace

extern "C" int vad_smooth_tile(int* tile_h, int* tile_w) {
    if (tile_h) *tile_h = SM_TH;
    if (tile_w) *tile_w = SM_TW;
    return VAD_OK;
}

extern "C" size_t vad_smooth_workspace_bytes(long long n, int h, int w, int radius) {
    if (!smooth_dims_ok(n, h, w, radius)) return 0;
    return (size_t)n * (size_t)smooth_tiles(h, w) * sizeof(float);
}

extern "C" int vad_smooth_maps(const float* maps, long long n, int h, int w, const float* taps_dev, int radius, float* out, float* frame_max,
                               void* ws, size_t ws_bytes, void* stream) {
    VAD_ARG(vad_req_map_n("smooth_maps", n));
    VAD_ARG(vad_req_map_hw("smooth_maps", h, w));
    VAD_REQUIRE(radius >= 1 && radius <= VAD_SMOOTH_MAX_RADIUS, "smooth_maps: radius must be in 1..%d, got %d", VAD_SMOOTH_MAX_RADIUS, radius);
    VAD_REQUIRE(radius <= h && radius <= w, "smooth_maps: radius %d exceeds min(h, w) of a %dx%d map (one reflection only)", radius, h, w);
    VAD_ARG(vad_req_map_total("smooth_maps", n, h, w));
    VAD_REQUIRE(out != nullptr || frame_max != nullptr, "smooth_maps: out and frame_max are both NULL");
    VAD_REQUIRE(maps != nullptr && taps_dev != nullptr, "smooth_maps: maps or taps is NULL");
    VAD_REQUIRE(vad_aligned(maps, 4) && vad_aligned(taps_dev, 4) && vad_aligned(out, 4) && vad_aligned(frame_max, 4) && vad_aligned(ws, 4),
                "smooth_maps: maps, taps, out, frame_max and ws must be 4-byte aligned");
    VAD_REQUIRE(out == nullptr || vad_disjoint(maps, out, (size_t)n * h * w * sizeof(float)),
                "smooth_maps: out overlaps maps (a pixel's window reads its neighbours: not in place)");
    const long long tiles = smooth_tiles(h, w);
    if (frame_max != nullptr) {
        const size_t need = vad_smooth_workspace_bytes(n, h, w, radius);
        if (need && (ws == nullptr || ws_bytes < need))
            return vad_fail(VAD_ERR_WS, "smooth_maps: workspace of %zu bytes needed, %zu given", need, ws ? ws_bytes : (size_t)0);
    }
    if (n == 0) return VAD_OK;

    const hipStream_t s = (hipStream_t)stream;
    const SmoothGeo g = smooth_geo(radius);
    if (g.lds_bytes > 64 * 1024) {                                                              // needs the attribute, once per process
        static std::atomic<bool> attr_set;                                                      // (setting it twice from two threads is harmless)
        if (!attr_set.load(std::memory_order_acquire)) {
            VAD_HIP_TRY(hipFuncSetAttribute((const void*)smooth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)smooth_geo(VAD_SMOOTH_MAX_RADIUS).lds_bytes));
            attr_set.store(true, std::memory_order_release);
        }
    }
    SmoothP p;
    p.taps = taps_dev;
    p.h = h;
    p.w = w;
    p.r = radius;
    p.tiles_x = (w + SM_TW - 1) / SM_TW;
    p.tiles = (int)tiles;
    for (long long f0 = 0; f0 < n; f0 += 65535) {                                               // frames in slices of gridDim.y
        const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
        p.maps = maps + (size_t)f0 * h * w;
        p.out = out ? out + (size_t)f0 * h * w : nullptr;
        p.tile_max = frame_max ? (float*)ws + (size_t)f0 * tiles : nullptr;
        hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)tiles, m), dim3(SM_THREADS), g.lds_bytes, s, p);
        VAD_LAUNCH_CHECK();
    }
    if (frame_max != nullptr) {
        for (long long f0 = 0; f0 < n; f0 += (1ll << 30)) {
            const unsigned m = (unsigned)(n - f0 < (1ll << 30) ? n - f0 : (1ll << 30));
            hipLaunchKernelGGL(smooth_max_kernel, dim3(m), dim3(64), 0, s, (const float*)ws + (size_t)f0 * tiles, (int)tiles, frame_max + f0);
            VAD_LAUNCH_CHECK();
        }
    }
    return VAD_OK;
}
