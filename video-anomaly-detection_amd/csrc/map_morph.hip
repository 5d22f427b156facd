// Grey morphology of anomaly maps with a flat rectangular structuring element: erode, dilate, open, close -
// the clean-up a deployed line applies to a map before it is thresholded and labelled (opening removes speckle no Gaussian removes
// without blurring real defects; closing fills pinholes and joins the fragments of one cracked defect).  The maps stay on the device
// between score_all / smooth_maps / MapStatistics.normalize and detect_regions / detect_events / EventTracker.
//
// Semantics - scipy.ndimage.grey_erosion / grey_dilation / grey_opening / grey_closing with size=(size_h, size_w), mode="reflect".
// For a flat element these are windows clamped to the image, with scipy's even-size convention; per axis of length L, size s:
//   erode   out[i] = min x[max(0, i - s/2)       .. min(L - 1, i + (s - 1)/2)]
//   dilate  out[i] = max x[max(0, i - (s - 1)/2) .. min(L - 1, i + s/2)]
//   open    = dilate(erode(x)),  close = erode(dilate(x)): the second step clamps its windows to the image ON THE INTERMEDIATE image,
//           which has no values outside the frame.
// Nothing is rounded: minimum and maximum are the IEEE-754-2019 `minimum` / `maximum` (vad_vmin / vad_vmax): NaN if any value of the
// window is NaN (for open / close: the windows of both steps), -0 below +0.  tests/map_morph_ref.py restates it to the bit.
//
// A clamped window is a full window over a frame surrounded by the step's identity (+Inf for a minimum, -Inf for a maximum): the
// identity changes no other operand, NaN and the zeros included.  That is how borders are handled here, and why a rectangle
// separates into a pass along H and one along W.  The first step's result is OVERWRITTEN with the second step's identity wherever
// it lies outside the frame, so the second step never sees a value computed from padding.
//
// Tiling: one work-group of 256 threads per MO_TH x MO_TW = 32 x 64 output tile, one launch per op, every pass through LDS.
//   stage   A[R0][C0] <- the tile and its halo (s - 1 rows / columns in all for one step, 2 (s - 1) for open / close), identity
//           outside the frame; lanes along x, the loads of 8 rows per wave in flight together;
//   V pass  work item = (8-row strip, column), lanes along the columns (consecutive banks): A -> B;
//   H pass  work item = (row, 8-column strip), lanes along the ROWS: the pitch of A and B is odd, so the 32 lanes of an LDS access
//           group fall on 32 different banks: B -> A (dead behind the barrier that closes the V pass); the first step of open /
//           close writes the second step's identity outside the frame here;
//   (open / close: V and H pass of the second step, A -> B -> A)
//   store   rows of A with lanes along x (256-byte runs).
// A strip's 8 outputs of window s share their inputs x[0 .. s + 6].  s < 8: a window of 8 registers slides over them (s compares
// per output).  s >= 8: x[7 .. s - 1] is in every one of the 8 windows, so its minimum is taken once, and output j adds the
// minimum of x[j .. 6] and of x[s .. s + j - 1] (running minima of the 7 first and 7 last inputs): s + 12 compares per 8 outputs
// instead of 8 s - what keeps size 31 near the small sizes.  The last strip of a pass is moved back to end at the last output
// (it recomputes a few outputs of its neighbour, same values), so no strip reads or writes outside its buffer.
#include <hip/hip_runtime.h>

#include <atomic>

#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int MO_TH = 32, MO_TW = 64;
constexpr int MO_THREADS = 256;
constexpr int MO_STRIP = 8;                    // outputs per work item and pass
constexpr int MO_BATCH = 8;                    // rows a wave has in flight while it stages the tile

struct MorphGeo {
    int steps;           // 1: erode / dilate, 2: open / close
    int r0, c0;          // of A as staged: MO_TH + steps (size_h - 1), MO_TW + steps (size_w - 1)
    int r1, c1;          // of the first step's result (two steps): MO_TH + size_h - 1, MO_TW + size_w - 1
    int pitch;           // of A and B in floats, odd
    int lo_h[2], lo_w[2];  // how far a step's window reaches towards index 0
    size_t lds_bytes;
};

__host__ __device__ inline bool morph_is_max(int op, int step) {
    return step == 0 ? (op == VAD_MORPH_DILATE || op == VAD_MORPH_CLOSE) : op == VAD_MORPH_OPEN;
}

__host__ __device__ inline MorphGeo morph_geo(int op, int sh, int sw) {
    MorphGeo g;
    g.steps = (op == VAD_MORPH_OPEN || op == VAD_MORPH_CLOSE) ? 2 : 1;
    for (int k = 0; k < 2; ++k) {
        const bool mx = morph_is_max(op, k);
        g.lo_h[k] = mx ? (sh - 1) / 2 : sh / 2;
        g.lo_w[k] = mx ? (sw - 1) / 2 : sw / 2;
    }
    g.r1 = MO_TH + sh - 1;
    g.c1 = MO_TW + sw - 1;
    g.r0 = MO_TH + g.steps * (sh - 1);
    g.c0 = MO_TW + g.steps * (sw - 1);
    g.pitch = g.c0 | 1;
    g.lds_bytes = ((size_t)g.r0 + (g.steps == 2 ? g.r1 : MO_TH)) * g.pitch * sizeof(float);
    return g;
}

template <bool MAX> __device__ __forceinline__ float morph_mm(float a, float b) { return MAX ? vad_vmax(a, b) : vad_vmin(a, b); }

// out[j] = min / max of a[j * stride .. (j + s - 1) * stride], j = 0 .. 7
template <bool MAX> __device__ __forceinline__ void morph_window8(const float* a, int stride, int s, float (&out)[MO_STRIP]) {
    if (s < MO_STRIP) {
        float win[MO_STRIP];
#pragma unroll
        for (int j = 0; j < MO_STRIP; ++j) out[j] = win[j] = a[j * stride];
#pragma unroll
        for (int k = 1; k < MO_STRIP - 1; ++k) {
            if (k >= s) break;
#pragma unroll
            for (int j = 0; j < MO_STRIP - 1; ++j) win[j] = win[j + 1];
            win[MO_STRIP - 1] = a[(MO_STRIP - 1 + k) * stride];
#pragma unroll
            for (int j = 0; j < MO_STRIP; ++j) out[j] = morph_mm<MAX>(out[j], win[j]);
        }
    } else {
        float lo[MO_STRIP - 1], hi[MO_STRIP - 1];
#pragma unroll
        for (int j = 0; j < MO_STRIP - 1; ++j) lo[j] = a[j * stride];
        const float* t = a + s * stride;
#pragma unroll
        for (int j = 0; j < MO_STRIP - 1; ++j) hi[j] = t[j * stride];
        const float* m = a + (MO_STRIP - 1) * stride;
        float core = *m;
#pragma unroll 8
        for (int k = MO_STRIP; k < s; ++k) {
            m += stride;
            core = morph_mm<MAX>(core, *m);
        }
#pragma unroll
        for (int j = MO_STRIP - 3; j >= 0; --j) lo[j] = morph_mm<MAX>(lo[j], lo[j + 1]);      // lo[j] = of x[j .. 6]
#pragma unroll
        for (int j = 1; j < MO_STRIP - 1; ++j) hi[j] = morph_mm<MAX>(hi[j], hi[j - 1]);      // hi[j] = of x[s .. s + j]
        out[0] = morph_mm<MAX>(core, lo[0]);
#pragma unroll
        for (int j = 1; j < MO_STRIP - 1; ++j) out[j] = morph_mm<MAX>(morph_mm<MAX>(core, lo[j]), hi[j - 1]);
        out[MO_STRIP - 1] = morph_mm<MAX>(core, hi[MO_STRIP - 2]);
    }
}

// dst[y][c] = min / max of src[y .. y + s - 1][c] for y < rows_out (>= 8), c < cols
template <bool MAX> __device__ __forceinline__ void morph_pass_v(const float* src, float* dst, int pitch, int rows_out, int cols, int s, int tid) {
    const int items = ((rows_out + MO_STRIP - 1) / MO_STRIP) * cols;
    for (int it = tid; it < items; it += MO_THREADS) {
        const int strip = it / cols, c = it - strip * cols;
        const int y = min(strip * MO_STRIP, rows_out - MO_STRIP);
        float o[MO_STRIP];
        morph_window8<MAX>(src + y * pitch + c, pitch, s, o);
        float* d = dst + y * pitch + c;
#pragma unroll
        for (int j = 0; j < MO_STRIP; ++j) d[j * pitch] = o[j];
    }
}

// dst[y][c] = min / max of src[y][c .. c + s - 1] for y < rows, c < cols_out (>= 8).  FILL: dst[0][0] is pixel (gy0, gx0) of the frame;
// what lies outside the h x w frame becomes `fill`
template <bool MAX, bool FILL>
__device__ __forceinline__ void morph_pass_h(const float* src, float* dst, int pitch, int rows, int cols_out, int s, int tid, int gy0, int gx0,
                                             int h, int w, float fill) {
    const int items = ((cols_out + MO_STRIP - 1) / MO_STRIP) * rows;
    for (int it = tid; it < items; it += MO_THREADS) {
        const int strip = it / rows, y = it - strip * rows;
        const int c = min(strip * MO_STRIP, cols_out - MO_STRIP);
        float o[MO_STRIP];
        morph_window8<MAX>(src + y * pitch + c, 1, s, o);
        float* d = dst + y * pitch + c;
        const bool row_in = (unsigned)(gy0 + y) < (unsigned)h;
#pragma unroll
        for (int j = 0; j < MO_STRIP; ++j) d[j] = (!FILL || (row_in && (unsigned)(gx0 + c + j) < (unsigned)w)) ? o[j] : fill;
    }
}

struct MorphP {
    const float* maps;
    float* out;
    int h, w, sh, sw;
    int tiles_x;
};

template <int OP> __global__ __launch_bounds__(MO_THREADS) void morph_kernel(MorphP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool TWO = OP == VAD_MORPH_OPEN || OP == VAD_MORPH_CLOSE;
    constexpr bool MAX0 = OP == VAD_MORPH_DILATE || OP == VAD_MORPH_CLOSE;       // morph_is_max(OP, 0)
    constexpr bool MAX1 = OP == VAD_MORPH_OPEN;                                  // morph_is_max(OP, 1)
    const MorphGeo g = morph_geo(OP, p.sh, p.sw);
    float* A = lds;
    float* B = lds + g.r0 * g.pitch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int y0 = ty * MO_TH, x0 = tx * MO_TW;
    const size_t frame = blockIdx.y;
    const float* __restrict__ src = p.maps + frame * (size_t)p.h * p.w;
    float* __restrict__ dst = p.out + frame * (size_t)p.h * p.w;

    // stage: A[r][c] = pixel (ay + r, ax + c), the first step's identity outside the frame
    const int ay = y0 - g.lo_h[0] - (TWO ? g.lo_h[1] : 0), ax = x0 - g.lo_w[0] - (TWO ? g.lo_w[1] : 0);
    const float id0 = MAX0 ? -INFINITY : INFINITY;
    // (rows in batches of MO_BATCH: every load is of a pixel clamped into the frame, all loads of a batch are issued before the
    // first is used, and the identity is selected afterwards - one memory latency per batch, not per row)
    constexpr int WAVES = MO_THREADS / 64;
    for (int c = lane; c < g.c0; c += 64) {
        const int gx = ax + c;
        const bool col_in = (unsigned)gx < (unsigned)p.w;
        const float* col = src + min(max(gx, 0), p.w - 1);
        float* a = A + c;
        for (int rb = wv; rb < g.r0; rb += MO_BATCH * WAVES) {
            float v[MO_BATCH];
#pragma unroll
            for (int k = 0; k < MO_BATCH; ++k) v[k] = col[min(max(ay + rb + k * WAVES, 0), p.h - 1) * p.w];
#pragma unroll
            for (int k = 0; k < MO_BATCH; ++k) {
                const int r = rb + k * WAVES;
                if (r < g.r0) a[r * g.pitch] = (col_in && (unsigned)(ay + r) < (unsigned)p.h) ? v[k] : id0;
            }
        }
    }
    __syncthreads();

    if (TWO) {
        morph_pass_v<MAX0>(A, B, g.pitch, g.r1, g.c0, p.sh, tid);
        __syncthreads();
        morph_pass_h<MAX0, true>(B, A, g.pitch, g.r1, g.c1, p.sw, tid, y0 - g.lo_h[1], x0 - g.lo_w[1], p.h, p.w, MAX1 ? -INFINITY : INFINITY);
        __syncthreads();
        morph_pass_v<MAX1>(A, B, g.pitch, MO_TH, g.c1, p.sh, tid);
        __syncthreads();
        morph_pass_h<MAX1, false>(B, A, g.pitch, MO_TH, MO_TW, p.sw, tid, 0, 0, 0, 0, 0.f);
    } else {
        morph_pass_v<MAX0>(A, B, g.pitch, MO_TH, g.c0, p.sh, tid);
        __syncthreads();
        morph_pass_h<MAX0, false>(B, A, g.pitch, MO_TH, MO_TW, p.sw, tid, 0, 0, 0, 0, 0.f);
    }
    __syncthreads();

    const int gx = x0 + lane;
#pragma unroll
    for (int y = wv; y < MO_TH; y += MO_THREADS / 64) {
        const int gy = y0 + y;
        if (gx < p.w && gy < p.h) dst[gy * p.w + gx] = A[y * g.pitch + lane];
    }
}

template <int OP> int morph_launch(const MorphP& base, long long n, void* stream) {
    const MorphGeo g = morph_geo(OP, base.sh, base.sw);
    if (g.lds_bytes > 64 * 1024) {                                                              // needs the attribute, once per process
        static std::atomic<bool> attr_set;                                                      // (setting it twice from two threads is harmless)
        if (!attr_set.load(std::memory_order_acquire)) {
            VAD_HIP_TRY(hipFuncSetAttribute((const void*)morph_kernel<OP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)morph_geo(OP, VAD_MORPH_MAX_SIZE, VAD_MORPH_MAX_SIZE).lds_bytes));
            attr_set.store(true, std::memory_order_release);
        }
    }
    MorphP p = base;
    const size_t fs = (size_t)p.h * p.w;
    const long long tiles = (long long)((p.h + MO_TH - 1) / MO_TH) * p.tiles_x;
    for (long long f0 = 0; f0 < n; f0 += 65535) {                                               // frames in slices of gridDim.y
        const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
        p.maps = base.maps + (size_t)f0 * fs;
        p.out = base.out + (size_t)f0 * fs;
        hipLaunchKernelGGL(morph_kernel<OP>, dim3((unsigned)tiles, m), dim3(MO_THREADS), g.lds_bytes, (hipStream_t)stream, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

}  // namespace

extern "C" int vad_morph_tile(int size_h, int size_w, int op, int* tile_h, int* tile_w) {
    VAD_REQUIRE(op >= VAD_MORPH_ERODE && op <= VAD_MORPH_CLOSE, "morph_tile: unknown op %d (0 erode, 1 dilate, 2 open, 3 close)", op);
    VAD_REQUIRE(size_h >= 1 && size_h <= VAD_MORPH_MAX_SIZE && size_w >= 1 && size_w <= VAD_MORPH_MAX_SIZE,
                "morph_tile: size must be in 1..%d per side, got %dx%d", VAD_MORPH_MAX_SIZE, size_h, size_w);
    if (tile_h) *tile_h = MO_TH;                                                                // one tile for every size class: the halo of
    if (tile_w) *tile_w = MO_TW;                                                                // open / close at 31 x 31 still leaves two groups a CU
    return VAD_OK;
}

extern "C" int vad_morph_maps(const float* maps, long long n, int h, int w, int op, int size_h, int size_w, float* out, void* stream) {
    VAD_REQUIRE(op >= VAD_MORPH_ERODE && op <= VAD_MORPH_CLOSE, "morph_maps: unknown op %d (0 erode, 1 dilate, 2 open, 3 close)", op);
    VAD_REQUIRE(size_h >= 1 && size_h <= VAD_MORPH_MAX_SIZE && size_w >= 1 && size_w <= VAD_MORPH_MAX_SIZE,
                "morph_maps: size must be in 1..%d per side, got %dx%d", VAD_MORPH_MAX_SIZE, size_h, size_w);
    VAD_ARG(vad_req_map_dims("morph_maps", n, h, w));
    VAD_REQUIRE(maps != nullptr && out != nullptr, "morph_maps: maps or out is NULL");
    VAD_REQUIRE(vad_aligned(maps, 4) && vad_aligned(out, 4), "morph_maps: maps and out must be 4-byte aligned");
    VAD_REQUIRE(vad_disjoint(maps, out, (size_t)n * h * w * sizeof(float)),
                "morph_maps: out overlaps maps (a pixel's window reads its neighbours: not in place)");
    if (n == 0) return VAD_OK;

    MorphP p;
    p.maps = maps;
    p.out = out;
    p.h = h;
    p.w = w;
    p.sh = size_h;
    p.sw = size_w;
    p.tiles_x = (w + MO_TW - 1) / MO_TW;
    switch (op) {
        case VAD_MORPH_ERODE: return morph_launch<VAD_MORPH_ERODE>(p, n, stream);
        case VAD_MORPH_DILATE: return morph_launch<VAD_MORPH_DILATE>(p, n, stream);
        case VAD_MORPH_OPEN: return morph_launch<VAD_MORPH_OPEN>(p, n, stream);
        default: return morph_launch<VAD_MORPH_CLOSE>(p, n, stream);
    }
}
