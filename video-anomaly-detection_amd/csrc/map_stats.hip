// Per-pixel calibration of anomaly maps: the mean and standard deviation of every pixel of the map over the
// normal (training) frames, and the z-score map z = (map - mean) / std that is ranked, thresholded and labelled in place of the raw
// map.  An autoencoder reconstructs edges, gloss and fine texture worse than flat background in EVERY normal frame of a fixed
// camera; one global threshold either fires there all day or misses a defect on the background.  The maps stay on the device.
//
// Arithmetic - specified so that numpy restates it bit for bit (tests/map_stats_ref.py) and no result depends on the batching:
//   state       K, S1, S2: float64 planes of h * w; n: a 64-bit frame count in the blob's header, on the device;
//   accumulate  per pixel, in frame order:  n == 0: K = (double)x[0];  then for every frame  d = (double)x - K,  S1 = S1 + d,
//               S2 = S2 + d * d;  the product and each sum rounded to float64 on their own (contraction off: hip.py and the pragma);
//   merge       dl = K_b - K_a;  S1 = S1_a + (S1_b + n_b dl);  S2 = S2_a + (S2_b + ((2 dl) S1_b + (n_b dl) dl));  K_a stays; an empty
//               side gives the other side;
//   finalize    mean = fl32(K + S1 / n);  var = (S2 - S1 (S1 / n)) / (n - ddof), var < 0 -> 0 (a NaN stays), std = sqrtf(fl32(var)):
//               the root is taken in fp32, where hipcc's sqrt and divide are correctly rounded by default;
//   normalize   z = (x - mean) / (std < min_std ? min_std : std), fp32, each operation rounded on its own, IEEE division.
// K is the pixel's first value, so S1 and S2 are sums of SHIFTED data: the cancellation in S2 - S1^2 / n is that of values the size
// of the pixel's spread, not of its level (a map of 1000 +- 1e-3 keeps its standard deviation).
// Non-finite values need no code: a NaN, or an Inf in the first frame (Inf - Inf), makes K-relative sums NaN; a later Inf makes S1
// and S2 infinite, so the variance is Inf - Inf = NaN and the mean is the infinity numpy's mean gives.  No other pixel is touched.
//
// Accumulate: one thread per pixel - the additions of one pixel are ordered, so its frames are never split over threads - with
// MS_FRAMES = 32 frames' loads in flight per thread and the next 32 issued before the current ones are added: 256 threads x 32 frames
// x 4 bytes = 32 KiB per work-group, what a streaming kernel needs per CU, and a 256 x 256 map has exactly one work-group per CU.
// Lanes run along x, so a wave's load is 256 contiguous bytes whatever the width or the base.
// The count is read by every thread before it touches its pixel, so it is advanced by a second, one-thread launch behind the first.
// Normalize: one work-group per NZ_CHUNK = 1024 pixels and NZ_FRAMES = 4 frames (mean and the floored std stay in registers across
// the frames; they are 512 KiB at 256 x 256 and stay in L2); chunk maxima go to the workspace and one wave per frame folds them -
// compare-only, the same for every batching and tiling, like map_smooth.hip's.
// Every loop has a bound known at launch.
#include <hip/hip_runtime.h>

#include <math.h>

#include "vad_args.h"
#include "vad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr unsigned MS_MAGIC = 0x4d444156u;     // "VADM"
constexpr size_t MS_HEADER_BYTES = 32;         // metrics.py _MS_HEADER_BYTES
constexpr int MS_THREADS = 256;
constexpr int MS_PIXELS_PER_THREAD = 1;
constexpr int MS_FRAMES = 32;                  // loads in flight per thread
constexpr int NZ_THREADS = 256;
constexpr int NZ_CHUNK = 1024;                 // pixels of one work-group: 4 per thread, 256 apart
constexpr int NZ_PER_THREAD = NZ_CHUNK / NZ_THREADS;
constexpr int NZ_FRAMES = 4;                   // frames of one work-group

struct MapStatHeader {
    unsigned magic, tag;
    int h, w;
    unsigned long long n, reserved;
};
static_assert(sizeof(MapStatHeader) == MS_HEADER_BYTES, "the header is 32 bytes");

__host__ __device__ inline unsigned ms_tag(void) { return (unsigned)VAD_ABI_VERSION << 16; }

// the header lives in device memory: every kernel compares it with the call's geometry and leaves a foreign blob alone
__device__ __forceinline__ bool ms_header_ok(const MapStatHeader* hd, int h, int w) {
    return hd->magic == MS_MAGIC && hd->tag == ms_tag() && hd->h == h && hd->w == w;
}

__device__ __forceinline__ double* ms_planes(void* state) { return (double*)((char*)state + MS_HEADER_BYTES); }

__global__ __launch_bounds__(MS_THREADS) void mapstat_reset_kernel(void* state, int h, int w) {
    const int pixels = h * w;
    const int p = blockIdx.x * MS_THREADS + threadIdx.x;
    if (p == 0) {
        MapStatHeader* hd = (MapStatHeader*)state;
        hd->magic = MS_MAGIC;
        hd->tag = ms_tag();
        hd->h = h;
        hd->w = w;
        hd->n = 0;
        hd->reserved = 0;
    }
    if (p < pixels) {
        double* k = ms_planes(state);
        k[p] = 0.0;
        k[pixels + p] = 0.0;
        k[2 * (size_t)pixels + p] = 0.0;
    }
}

// x[j] = frame f + j of the thread's pixel; FULL: all MS_FRAMES frames exist
template <bool FULL>
__device__ __forceinline__ void ms_load(float (&x)[MS_FRAMES], const float* __restrict__ src, size_t fs, long long f, long long n) {
#pragma unroll
    for (int j = 0; j < MS_FRAMES; ++j) x[j] = (FULL || f + j < n) ? src[(size_t)(f + j) * fs] : 0.f;
}

__device__ __forceinline__ void ms_add(float x, double k, double& s1, double& s2) {
    const double d = (double)x - k;
    s1 = s1 + d;
    s2 = s2 + d * d;
}

__global__ __launch_bounds__(MS_THREADS) void mapstat_accumulate_kernel(const float* __restrict__ maps, long long n, int h, int w, void* state) {
    const MapStatHeader* hd = (const MapStatHeader*)state;
    if (!ms_header_ok(hd, h, w)) return;
    const int pixels = h * w;
    const int p = blockIdx.x * MS_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const bool empty = hd->n == 0;
    double* K = ms_planes(state);
    double* S1 = K + pixels;
    double* S2 = S1 + pixels;
    const size_t fs = (size_t)pixels;
    const float* __restrict__ src = maps + p;

    float cur[MS_FRAMES], nxt[MS_FRAMES];
    if (n >= MS_FRAMES) ms_load<true>(cur, src, fs, 0, n);
    else ms_load<false>(cur, src, fs, 0, n);
    double k, s1, s2;
    if (empty) {
        k = (double)cur[0];
        s1 = 0.0;
        s2 = 0.0;
    } else {
        k = K[p];
        s1 = S1[p];
        s2 = S2[p];
    }
    for (long long f = 0; f < n; f += MS_FRAMES) {
        const long long g = f + MS_FRAMES;                       // the next group's loads go out before this group is added
        if (g + MS_FRAMES <= n) ms_load<true>(nxt, src, fs, g, n);
        else ms_load<false>(nxt, src, fs, g, n);
        if (g <= n) {
#pragma unroll
            for (int j = 0; j < MS_FRAMES; ++j) ms_add(cur[j], k, s1, s2);
        } else {
            const int m = (int)(n - f);
#pragma unroll
            for (int j = 0; j < MS_FRAMES; ++j)
                if (j < m) ms_add(cur[j], k, s1, s2);
        }
#pragma unroll
        for (int j = 0; j < MS_FRAMES; ++j) cur[j] = nxt[j];
    }
    K[p] = k;
    S1[p] = s1;
    S2[p] = s2;
}

// n += n_new, or += the count of `other` (merge); behind the kernel whose threads all read the old count
__global__ void mapstat_count_kernel(void* state, const void* other, long long n_new, int h, int w) {
    MapStatHeader* hd = (MapStatHeader*)state;
    if (!ms_header_ok(hd, h, w)) return;
    if (other != nullptr) {
        const MapStatHeader* ho = (const MapStatHeader*)other;
        if (!ms_header_ok(ho, h, w)) return;
        hd->n += ho->n;
    } else {
        hd->n += (unsigned long long)n_new;
    }
}

__global__ __launch_bounds__(MS_THREADS) void mapstat_merge_kernel(void* state, const void* other, int h, int w) {
    const MapStatHeader* ha = (const MapStatHeader*)state;
    const MapStatHeader* hb = (const MapStatHeader*)other;
    if (!ms_header_ok(ha, h, w) || !ms_header_ok(hb, h, w)) return;
    const int pixels = h * w;
    const int p = blockIdx.x * MS_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const unsigned long long na = ha->n, nb = hb->n;
    if (nb == 0) return;
    double* Ka = ms_planes(state);
    const double* Kb = (const double*)((const char*)other + MS_HEADER_BYTES);
    const double kb = Kb[p], s1b = Kb[pixels + p], s2b = Kb[2 * (size_t)pixels + p];
    if (na == 0) {
        Ka[p] = kb;
        Ka[pixels + p] = s1b;
        Ka[2 * (size_t)pixels + p] = s2b;
        return;
    }
    const double dl = kb - Ka[p];
    const double ndl = (double)nb * dl;
    Ka[pixels + p] = Ka[pixels + p] + (s1b + ndl);
    Ka[2 * (size_t)pixels + p] = Ka[2 * (size_t)pixels + p] + (s2b + ((2.0 * dl) * s1b + ndl * dl));
}

__global__ __launch_bounds__(MS_THREADS) void mapstat_finalize_kernel(const void* state, int h, int w, int ddof, float* __restrict__ mean,
                                                                       float* __restrict__ sd) {
    const MapStatHeader* hd = (const MapStatHeader*)state;
    const int pixels = h * w;
    const int p = blockIdx.x * MS_THREADS + threadIdx.x;
    if (p >= pixels) return;
    float m = NAN, s = NAN;                                      // a foreign blob, or no frame yet: NaN everywhere
    if (ms_header_ok(hd, h, w) && hd->n != 0) {
        const double* K = (const double*)((const char*)state + MS_HEADER_BYTES);
        const double k = K[p], s1 = K[pixels + p], s2 = K[2 * (size_t)pixels + p];
        const double n = (double)hd->n;
        const double q = s1 / n;
        m = (float)(k + q);
        if (hd->n > (unsigned long long)ddof) {                  // n - ddof <= 0: the standard deviation is NaN
            double var = (s2 - s1 * q) / (n - (double)ddof);
            var = var < 0.0 ? 0.0 : var;                         // written this way a NaN stays a NaN
            s = sqrtf((float)var);
        }
    }
    if (mean) mean[p] = m;
    if (sd) sd[p] = s;
}

struct NormP {
    const float* maps;
    const float* mean;
    const float* sd;
    float* out;          // may be NULL; may be maps
    float* chunk_max;    // [frames][chunks], may be NULL
    long long n;
    int pixels, chunks;
    float min_std;
};

__global__ __launch_bounds__(NZ_THREADS) void map_normalize_kernel(NormP p) {
    __shared__ float wave_max[NZ_FRAMES][NZ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = blockIdx.x;
    const long long f0 = (long long)blockIdx.y * NZ_FRAMES;
    const int base = chunk * NZ_CHUNK + tid;
    float mu[NZ_PER_THREAD], den[NZ_PER_THREAD];
#pragma unroll
    for (int i = 0; i < NZ_PER_THREAD; ++i) {
        const int px = base + i * NZ_THREADS;
        const bool in = px < p.pixels;
        mu[i] = in ? p.mean[px] : 0.f;
        const float s = in ? p.sd[px] : 1.f;
        den[i] = s < p.min_std ? p.min_std : s;                  // a NaN std stays NaN
    }
    float x[NZ_FRAMES][NZ_PER_THREAD];
#pragma unroll
    for (int j = 0; j < NZ_FRAMES; ++j) {
        const bool live = f0 + j < p.n;
        const float* src = p.maps + (size_t)(live ? f0 + j : f0) * p.pixels;     // no __restrict__: out may be maps
#pragma unroll
        for (int i = 0; i < NZ_PER_THREAD; ++i) {
            const int px = base + i * NZ_THREADS;
            x[j][i] = (live && px < p.pixels) ? src[px] : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < NZ_FRAMES; ++j) {
        const bool live = f0 + j < p.n;
        float* dst = (p.out && live) ? p.out + (size_t)(f0 + j) * p.pixels : nullptr;
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < NZ_PER_THREAD; ++i) {
            const int px = base + i * NZ_THREADS;
            if (live && px < p.pixels) {
                const float z = (x[j][i] - mu[i]) / den[i];
                m = vad_vmax(m, z);
                if (dst) dst[px] = z;
            }
        }
        if (p.chunk_max) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = vad_vmax(m, __shfl_xor(m, off, 64));
            if (lane == 0) wave_max[j][wv] = m;
        }
    }
    if (p.chunk_max) {
        __syncthreads();
        if (tid < NZ_FRAMES && f0 + tid < p.n)
            p.chunk_max[(size_t)(f0 + tid) * p.chunks + chunk] = vad_vmax4(wave_max[tid][0], wave_max[tid][1], wave_max[tid][2], wave_max[tid][3]);
    }
}

// frame_max[f] = the maximum of the frame's chunk maxima: one wave per frame
__global__ __launch_bounds__(64) void map_normalize_max_kernel(const float* chunk_max, int chunks, float* frame_max) {
    const size_t f = blockIdx.x;
    const float* t = chunk_max + f * chunks;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < chunks; i += 64) m = vad_vmax(m, t[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = vad_vmax(m, __shfl_xor(m, off, 64));
    if (threadIdx.x == 0) frame_max[f] = m;
}

inline unsigned ms_blocks(int h, int w) { return (unsigned)(((long long)h * w + MS_THREADS - 1) / MS_THREADS); }
inline long long nz_chunks(int h, int w) { return ((long long)h * w + NZ_CHUNK - 1) / NZ_CHUNK; }

}  // namespace

extern "C" int vad_mapstat_plan(int* pixels_per_thread, int* frames_in_flight, int* threads) {
    if (pixels_per_thread) *pixels_per_thread = MS_PIXELS_PER_THREAD;
    if (frames_in_flight) *frames_in_flight = MS_FRAMES;
    if (threads) *threads = MS_THREADS;
    return VAD_OK;
}

extern "C" size_t vad_mapstat_state_bytes(int h, int w) {
    if (!vad_map_hw_ok(h, w)) return 0;
    return MS_HEADER_BYTES + 3 * sizeof(double) * (size_t)h * w;
}

extern "C" int vad_mapstat_reset(void* state, int h, int w, void* stream) {
    VAD_ARG(vad_req_map_hw("mapstat_reset", h, w));
    VAD_ARG(vad_req_ptr("mapstat_reset", "state", state, 16));
    hipLaunchKernelGGL(mapstat_reset_kernel, dim3(ms_blocks(h, w)), dim3(MS_THREADS), 0, (hipStream_t)stream, state, h, w);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_mapstat_accumulate(const float* maps, long long n, int h, int w, void* state, void* stream) {
    VAD_ARG(vad_req_map_dims("mapstat_accumulate", n, h, w));
    VAD_ARG(vad_req_ptr("mapstat_accumulate", "maps", maps, 4));
    VAD_ARG(vad_req_ptr("mapstat_accumulate", "state", state, 16));
    if (n == 0) return VAD_OK;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mapstat_accumulate_kernel, dim3(ms_blocks(h, w)), dim3(MS_THREADS), 0, s, maps, n, h, w, state);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(mapstat_count_kernel, dim3(1), dim3(1), 0, s, state, (const void*)nullptr, n, h, w);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_mapstat_merge(void* state, const void* other, int h, int w, void* stream) {
    VAD_ARG(vad_req_map_hw("mapstat_merge", h, w));
    VAD_ARG(vad_req_ptr("mapstat_merge", "state", state, 16));
    VAD_ARG(vad_req_ptr("mapstat_merge", "other", other, 16));
    VAD_REQUIRE(vad_disjoint(state, other, vad_mapstat_state_bytes(h, w)), "mapstat_merge: other overlaps state");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mapstat_merge_kernel, dim3(ms_blocks(h, w)), dim3(MS_THREADS), 0, s, state, other, h, w);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(mapstat_count_kernel, dim3(1), dim3(1), 0, s, state, other, 0ll, h, w);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_mapstat_finalize(const void* state, int h, int w, int ddof, float* mean, float* std_out, void* stream) {
    VAD_ARG(vad_req_map_hw("mapstat_finalize", h, w));
    VAD_ARG(vad_req_ptr("mapstat_finalize", "state", state, 16));
    VAD_REQUIRE(ddof == 0 || ddof == 1, "mapstat_finalize: ddof must be 0 or 1, got %d", ddof);
    VAD_REQUIRE(mean != nullptr || std_out != nullptr, "mapstat_finalize: mean and std are both NULL");
    VAD_REQUIRE(vad_aligned(mean, 4) && vad_aligned(std_out, 4), "mapstat_finalize: mean and std must be 4-byte aligned");
    hipLaunchKernelGGL(mapstat_finalize_kernel, dim3(ms_blocks(h, w)), dim3(MS_THREADS), 0, (hipStream_t)stream, state, h, w, ddof, mean, std_out);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" size_t vad_map_normalize_workspace_bytes(long long n, int h, int w) {
    if (!vad_map_dims_ok(n, h, w)) return 0;
    return (size_t)n * (size_t)nz_chunks(h, w) * sizeof(float);
}

extern "C" int vad_map_normalize(const float* maps, long long n, int h, int w, const float* mean, const float* std_in, float min_std, float* out,
                                 float* frame_max, void* ws, size_t ws_bytes, void* stream) {
    VAD_ARG(vad_req_map_dims("map_normalize", n, h, w));
    VAD_REQUIRE(min_std > 0.f && min_std <= 3.402823466e38f, "map_normalize: min_std must be finite and greater than 0, got %g", (double)min_std);
    VAD_REQUIRE(out != nullptr || frame_max != nullptr, "map_normalize: out and frame_max are both NULL");
    VAD_REQUIRE(maps != nullptr && mean != nullptr && std_in != nullptr, "map_normalize: maps, mean or std is NULL");
    VAD_REQUIRE(vad_aligned(maps, 4) && vad_aligned(mean, 4) && vad_aligned(std_in, 4) && vad_aligned(out, 4) && vad_aligned(frame_max, 4) &&
                    vad_aligned(ws, 4),
                "map_normalize: maps, mean, std, out, frame_max and ws must be 4-byte aligned");
    VAD_REQUIRE(out == nullptr || out == maps || vad_disjoint(maps, out, (size_t)n * h * w * sizeof(float)),
                "map_normalize: out partly overlaps maps (out == maps, in place, is allowed)");
    const long long chunks = nz_chunks(h, w);
    if (frame_max != nullptr) {
        const size_t need = vad_map_normalize_workspace_bytes(n, h, w);
        if (need && (ws == nullptr || ws_bytes < need))
            return vad_fail(VAD_ERR_WS, "map_normalize: workspace of %zu bytes needed, %zu given", need, ws ? ws_bytes : (size_t)0);
    }
    if (n == 0) return VAD_OK;

    const hipStream_t s = (hipStream_t)stream;
    NormP p;
    p.mean = mean;
    p.sd = std_in;
    p.pixels = h * w;
    p.chunks = (int)chunks;
    p.min_std = min_std;
    const long long slice = 65535ll * NZ_FRAMES;                                                // frames in slices of gridDim.y
    for (long long f0 = 0; f0 < n; f0 += slice) {
        const long long m = n - f0 < slice ? n - f0 : slice;
        p.maps = maps + (size_t)f0 * p.pixels;
        p.out = out ? out + (size_t)f0 * p.pixels : nullptr;
        p.chunk_max = frame_max ? (float*)ws + (size_t)f0 * chunks : nullptr;
        p.n = m;
        hipLaunchKernelGGL(map_normalize_kernel, dim3((unsigned)chunks, (unsigned)((m + NZ_FRAMES - 1) / NZ_FRAMES)), dim3(NZ_THREADS), 0, s, p);
        VAD_LAUNCH_CHECK();
    }
    if (frame_max != nullptr) {
        for (long long f0 = 0; f0 < n; f0 += (1ll << 30)) {
            const unsigned m = (unsigned)(n - f0 < (1ll << 30) ? n - f0 : (1ll << 30));
            hipLaunchKernelGGL(map_normalize_max_kernel, dim3(m), dim3(64), 0, s, (const float*)ws + (size_t)f0 * chunks, (int)chunks, frame_max + f0);
            VAD_LAUNCH_CHECK();
        }
    }
    return VAD_OK;
}
