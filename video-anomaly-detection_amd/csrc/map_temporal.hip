// Temporal filters of anomaly maps: per pixel, causal, over the last k frames of a stream - minimum
// (temporal erosion: "high in each of the last k frames", removes noise that differs from frame to frame without any spatial
// blur), maximum (temporal dilation: holds a detection across a dropped frame), mean (lowers the noise floor of a fixed camera by
// about sqrt(k)) - and the exponential average.  The step between MapStatistics.normalize / morph_maps and the threshold.
//
// Semantics.  Frames of one stream are x[0], x[1], ...; frame 0 is the first after vad_tfilt_init, or the first of a clip.
//   min / max  y[t] = minimum / maximum of x[max(0, t - k + 1) .. t]      (IEEE-754-2019 minimum / maximum: vad_vmin / vad_vmax)
//              = scipy.ndimage.minimum_filter1d / maximum_filter1d(x, size=k, axis=0, mode="nearest", origin=(k - 1) // 2)
//   mean       y[t] = (float)(S / (double)c), c = min(t + 1, k), S = the float64 sum of the window added oldest to newest, formed
//              anew for every output (no sliding add / subtract: its rounding would depend on the stream's history)
//   ema        y[0] = x[0], y[t] = y[t-1] + a * (x[t] - y[t-1]), a = alpha as float32, every operation rounded to float32 on its
//              own (this file is compiled with -ffp-contract=off): a finite constant stream stays constant to the bit
// tests/map_temporal_ref.py restates all four to the bit.
//
// Frames that do not exist yet are the operation's identity: +Inf for a minimum, -Inf for a maximum (the identity changes no other
// operand, NaN and both zeros included), -0.0 for the mean's sum (x + -0.0 = x for every x, -0.0 + -0.0 = -0.0: a sum that starts
// at -0.0 and adds -0.0 for every missing frame has the bits of the sum of the frames that exist).  vad_tfilt_init fills the ring
// with it, the clip mode (state NULL) a register window - so the kernels know no "short window" case; the frame count only
// decides the mean's divisor and the EMA's first frame.
//
// Work: HBM-bound, one read and one write of the maps.  A work item owns 4 consecutive pixels of a stream (one pixel on the
// scalar path) and walks them along t with the window of the k - 1 earlier frames in REGISTERS.  The window length is a template
// argument (k = 1 .. 16 per op, 98 kernels of a few hundred bytes): every index into the window is a constant after unrolling,
// so nothing goes to scratch.  The alternative - re-reading the k - 1 earlier frames - costs k times the L2 traffic and works
// only while k frames of all resident work items stay in L2: at 256 CUs x 2048 threads x 16 bytes that is 8 MiB PER FRAME, above
// the 4 MiB of L2 at the first frame (reasoning from the sizes; that form was not built or measured).  Frames are loaded four at
// a time before the first is used, so a work item has 64 bytes in flight.
// Vector path (16-byte loads and stores): h * w a multiple of 4 and maps, out 16-byte aligned - then every frame of every stream
// is.  Anything else takes the scalar path for the whole call: with h * w not a multiple of 4 a pixel's alignment changes from
// frame to frame.  The state's planes are padded to 16 bytes, so they serve both.
//
// State, per stream (caller-owned, 16-byte aligned): 16 words of header - frames seen (saturates at 2^32 - 1), ring position (the
// plane the next frame goes to), ticket, 0, magic, op, k, h, w, zeros - and a ring of k - 1 planes of round_up(h * w, 4) floats
// (ema: one plane, y[t-1]).  A call of t frames writes its last min(t, k - 1) frames into the ring at (position + i) mod (k - 1);
// nothing is shifted.  The counters are advanced ON THE DEVICE by the last work-group of the stream to finish (a ticket: every
// work-group has read the header before it draws one), so a captured call can be replayed.  The header is compared with the
// call's op, k, h, w on the device: with a blob made for something else the kernel follows no offset of it and writes NaN.
#include <hip/hip_runtime.h>

#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_HEADER_WORDS = 16;
constexpr unsigned TF_MAGIC = 0x46444156u;     // "VADF"
constexpr int TF_BATCH = 4;                    // frames a work item has in flight

typedef double f64x4 __attribute__((ext_vector_type(4)));
template <typename V> struct TfLanes;
template <> struct TfLanes<float> { typedef double D; static constexpr int N = 1; };
template <> struct TfLanes<f32x4> { typedef f64x4 D; static constexpr int N = 4; };
__device__ __forceinline__ double tf_wide(float v) { return (double)v; }
__device__ __forceinline__ f64x4 tf_wide(f32x4 v) { return __builtin_convertvector(v, f64x4); }
__device__ __forceinline__ float tf_narrow(double v) { return (float)v; }
__device__ __forceinline__ f32x4 tf_narrow(f64x4 v) { return __builtin_convertvector(v, f32x4); }
template <typename V> __device__ __forceinline__ V tf_splat(float v) { return (V)(v); }
// vad_vmin / vad_vmax per lane: for four lanes the builtin those two wrap, applied to the vector (the IEEE-754-2019 minimum / maximum)
__device__ __forceinline__ float tf_vmin(float a, float b) { return vad_vmin(a, b); }
__device__ __forceinline__ float tf_vmax(float a, float b) { return vad_vmax(a, b); }
__device__ __forceinline__ f32x4 tf_vmin(f32x4 a, f32x4 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ f32x4 tf_vmax(f32x4 a, f32x4 b) { return __builtin_elementwise_maximum(a, b); }

__host__ __device__ inline float tf_identity(int op) { return op == VAD_TFILT_MIN ? INFINITY : op == VAD_TFILT_MAX ? -INFINITY : op == VAD_TFILT_MEAN ? -0.0f : 0.0f; }
__host__ __device__ inline unsigned tf_planes(int op, int k) { return op == VAD_TFILT_EMA ? 1u : (unsigned)(k - 1); }
__host__ __device__ inline size_t tf_plane_floats(int h, int w) { return ((size_t)h * w + 3) & ~(size_t)3; }
__host__ __device__ inline size_t tf_stream_words(int h, int w, int op, int k) { return TF_HEADER_WORDS + tf_planes(op, k) * tf_plane_floats(h, w); }

struct TfP {
    const float* maps;       // [b, t, h * w]
    float* out;
    unsigned* state;         // b streams of stream_words, or NULL: every clip is a fresh stream
    size_t stream_words, plane, fs;     // plane: floats between two planes of the ring; fs = h * w
    unsigned items;          // work items per stream: fs / lanes
    int t, h, w;
    float alpha;
};

// true: the blob is a state of this op, k, h, w
__device__ __forceinline__ bool tf_header_ok(const unsigned* hdr, int op, int k, int h, int w) {
    return hdr[4] == TF_MAGIC && hdr[5] == (unsigned)op && hdr[6] == (unsigned)(op == VAD_TFILT_EMA ? 0 : k) && hdr[7] == (unsigned)h && hdr[8] == (unsigned)w;
}

// the last work-group of a stream to arrive advances its counters; every work-group has read them before it arrives: its threads
// have branched on the header (the loads have returned) before the barrier.  The ticket orders nothing else - a work-group's pixels
// are its own, and the next call is the next kernel -, so it is a relaxed atomic: with release semantics at agent scope every
// work-group would write its L2 back (measured with ("min", 2): 64 streams of one new 256 x 256 map took 0.138 ms, 0.014 as it is)
__device__ __forceinline__ void tf_advance(unsigned* hdr, unsigned seen, unsigned pos, int t, unsigned ring) {
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned before = __hip_atomic_fetch_add(&hdr[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (before != gridDim.x - 1) return;
    const unsigned long long total = (unsigned long long)seen + (unsigned)t;
    hdr[0] = total > 0xffffffffull ? 0xffffffffu : (unsigned)total;
    hdr[1] = ring ? (unsigned)(((unsigned long long)pos + (unsigned)t) % ring) : 0u;
    hdr[2] = 0u;
}

template <int OP, int K, typename V> __global__ __launch_bounds__(TF_THREADS) void tfilt_kernel(TfP p) {
    typedef typename TfLanes<V>::D D;
    constexpr int W = K > 1 ? K - 1 : 1;       // registers of the window (K == 1: one, unused)
    constexpr unsigned RING = OP == VAD_TFILT_EMA ? 1u : (unsigned)(K - 1);
    const unsigned item = blockIdx.x * TF_THREADS + threadIdx.x;
    const size_t s = blockIdx.y;
    unsigned* hdr = p.state ? p.state + s * p.stream_words : nullptr;
    unsigned seen = 0, pos = 0;
    bool bad = false;
    if (hdr) {
        bad = !tf_header_ok(hdr, OP, K, p.h, p.w);
        if (!bad) {
            seen = hdr[0];
            pos = hdr[1] < (RING ? RING : 1u) ? hdr[1] : 0u;
        }
    }
    const size_t clip = s * (size_t)p.t * p.fs;
    const V* __restrict__ x = (const V*)(p.maps + clip) + item;
    V* __restrict__ y = (V*)(p.out + clip) + item;
    const size_t step = p.items;               // V elements between two frames
    if (bad) {                                 // not a state of this call: nothing of it is followed
        if (item < p.items)
            for (int i = 0; i < p.t; ++i) y[i * step] = tf_splat<V>(__builtin_nanf(""));
        return;
    }
    if (item < p.items) {
        V* ring = hdr ? (V*)(hdr + TF_HEADER_WORDS) + item : nullptr;
        const size_t pstep = p.plane / TfLanes<V>::N;
        V win[W];                              // win[j]: the frame j + 1 before the one being made
#pragma unroll
        for (int j = 0; j < W; ++j) win[j] = tf_splat<V>(tf_identity(OP));
        if (ring) {
            if (OP == VAD_TFILT_EMA) {
                win[0] = ring[0];
            } else {
#pragma unroll
                for (int j = 0; j < K - 1; ++j) win[j] = ring[((pos + RING - 1u - (unsigned)j) % (RING ? RING : 1u)) * pstep];
            }
        }
        const V a = tf_splat<V>(p.alpha);
        auto one = [&](V v, int i) {
            V r;
            if (OP == VAD_TFILT_EMA) {
                r = (seen == 0 && i == 0) ? v : win[0] + a * (v - win[0]);
                win[0] = r;
            } else {
                if (OP == VAD_TFILT_MEAN) {
                    D sum = tf_wide(tf_splat<V>(-0.0f));
#pragma unroll
                    for (int j = K - 2; j >= 0; --j) sum = sum + tf_wide(win[j]);
                    sum = sum + tf_wide(v);
                    const unsigned long long n = (unsigned long long)seen + (unsigned)i + 1ull;
                    const double c = (double)(n < (unsigned long long)K ? (int)n : K);
                    r = tf_narrow(sum / c);
                } else {
                    r = v;
#pragma unroll
                    for (int j = 0; j < K - 1; ++j)
                        r = OP == VAD_TFILT_MAX ? tf_vmax(r, win[j]) : tf_vmin(r, win[j]);
                }
#pragma unroll
                for (int j = K - 2; j >= 1; --j) win[j] = win[j - 1];
                if (K > 1) win[0] = v;
            }
            return r;
        };
        int i = 0;
        for (; i + TF_BATCH <= p.t; i += TF_BATCH) {
            V v[TF_BATCH];
#pragma unroll
            for (int q = 0; q < TF_BATCH; ++q) v[q] = x[(size_t)(i + q) * step];
#pragma unroll
            for (int q = 0; q < TF_BATCH; ++q) y[(size_t)(i + q) * step] = one(v[q], i + q);
        }
        for (; i < p.t; ++i) y[(size_t)i * step] = one(x[(size_t)i * step], i);
        if (ring) {
            if (OP == VAD_TFILT_EMA) {
                ring[0] = win[0];
            } else {
#pragma unroll
                for (int j = 0; j < K - 1; ++j)    // the call's frame t - 1 - j goes to plane (pos + t - 1 - j) mod (k - 1)
                    if (j < p.t) ring[(((unsigned long long)pos + (unsigned)(p.t - 1 - j)) % (RING ? RING : 1u)) * pstep] = win[j];
            }
        }
    }
    if (hdr) tf_advance(hdr, seen, pos, p.t, RING);
}

struct TfInitP {
    unsigned* state;
    size_t stream_words;
    int op, k, h, w;
};

__global__ __launch_bounds__(TF_THREADS) void tfilt_init_kernel(TfInitP p) {
    unsigned* st = p.state + (size_t)blockIdx.y * p.stream_words;
    const unsigned fill = __float_as_uint(tf_identity(p.op));
    for (size_t i = (size_t)blockIdx.x * TF_THREADS + threadIdx.x; i < p.stream_words; i += (size_t)gridDim.x * TF_THREADS) {
        unsigned v = fill;
        if (i < TF_HEADER_WORDS)
            v = i == 4 ? TF_MAGIC : i == 5 ? (unsigned)p.op : i == 6 ? (unsigned)(p.op == VAD_TFILT_EMA ? 0 : p.k) : i == 7 ? (unsigned)p.h : i == 8 ? (unsigned)p.w : 0u;
        st[i] = v;
    }
}

template <int OP, int K> int tfilt_launch(TfP p, long long b, bool vec, void* stream) {
    p.items = (unsigned)(p.fs / (vec ? 4 : 1));
    const unsigned gx = (p.items + TF_THREADS - 1) / TF_THREADS;
    const TfP base = p;
    for (long long s0 = 0; s0 < b; s0 += 65535) {                                               // streams in slices of gridDim.y
        const unsigned m = (unsigned)(b - s0 < 65535 ? b - s0 : 65535);
        p.maps = base.maps + (size_t)s0 * p.t * p.fs;
        p.out = base.out + (size_t)s0 * p.t * p.fs;
        p.state = base.state ? base.state + (size_t)s0 * p.stream_words : nullptr;
        if (vec)
            hipLaunchKernelGGL((tfilt_kernel<OP, K, f32x4>), dim3(gx, m), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((tfilt_kernel<OP, K, float>), dim3(gx, m), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

template <int OP> int tfilt_launch_k(const TfP& p, long long b, int k, bool vec, void* stream) {
    switch (k) {
#define TF_CASE(K) case K: return tfilt_launch<OP, K>(p, b, vec, stream);
        TF_CASE(1) TF_CASE(2) TF_CASE(3) TF_CASE(4) TF_CASE(5) TF_CASE(6) TF_CASE(7) TF_CASE(8)
        TF_CASE(9) TF_CASE(10) TF_CASE(11) TF_CASE(12) TF_CASE(13) TF_CASE(14) TF_CASE(15) TF_CASE(16)
#undef TF_CASE
    }
    return vad_fail(VAD_ERR_ARG, "tfilt_maps: k must be in 1..%d, got %d", VAD_TFILT_MAX_K, k);
}

bool tf_op_ok(int op) { return op >= VAD_TFILT_MIN && op <= VAD_TFILT_EMA; }
bool tf_k_ok(int op, int k) { return op == VAD_TFILT_EMA || (k >= 1 && k <= VAD_TFILT_MAX_K); }
bool tf_b_ok(long long b) { return b >= 0 && b <= (1ll << 20); }

// op, k, b, h, w: what vad_tfilt_init and vad_tfilt_maps share, in this order
int tf_req_shape(const char* who, long long b, int h, int w, int op, int k) {
    VAD_REQUIRE(tf_op_ok(op), "%s: unknown op %d (0 min, 1 max, 2 mean, 3 ema)", who, op);
    VAD_REQUIRE(tf_k_ok(op, k), "%s: k must be in 1..%d, got %d", who, VAD_TFILT_MAX_K, k);
    VAD_REQUIRE(tf_b_ok(b), "%s: b must be in 0..2^20, got %lld", who, b);
    return vad_req_map_hw(who, h, w);
}

}  // namespace

extern "C" size_t vad_tfilt_state_bytes(long long b, int h, int w, int op, int k) {
    if (!tf_op_ok(op) || !tf_k_ok(op, k) || !tf_b_ok(b) || !vad_map_hw_ok(h, w)) return 0;
    return (size_t)b * tf_stream_words(h, w, op, k) * 4;
}

extern "C" int vad_tfilt_plan(int* threads, int* vector_pixels) {
    VAD_REQUIRE(threads && vector_pixels, "tfilt_plan: an output pointer is NULL");
    *threads = TF_THREADS;
    *vector_pixels = 4;
    return VAD_OK;
}

extern "C" int vad_tfilt_init(void* state, long long b, int h, int w, int op, int k, void* stream) {
    VAD_ARG(tf_req_shape("tfilt_init", b, h, w, op, k));
    VAD_ARG(vad_req_ptr("tfilt_init", "state", state, 16));
    if (b == 0) return VAD_OK;
    TfInitP p;
    p.stream_words = tf_stream_words(h, w, op, k);
    p.op = op;
    p.k = k;
    p.h = h;
    p.w = w;
    const size_t blocks = (p.stream_words + TF_THREADS - 1) / TF_THREADS;
    for (long long s0 = 0; s0 < b; s0 += 65535) {
        const unsigned m = (unsigned)(b - s0 < 65535 ? b - s0 : 65535);
        p.state = (unsigned*)state + (size_t)s0 * p.stream_words;
        hipLaunchKernelGGL(tfilt_init_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), m), dim3(TF_THREADS), 0, (hipStream_t)stream, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

extern "C" int vad_tfilt_maps(const float* maps, long long b, int t, int h, int w, int op, int k, float alpha, void* state_or_null, float* out,
                              void* stream) {
    VAD_ARG(tf_req_shape("tfilt_maps", b, h, w, op, k));
    VAD_REQUIRE(op != VAD_TFILT_EMA || (alpha > 0.f && alpha < 1.f), "tfilt_maps: alpha must be a float32 in (0, 1), got %g", (double)alpha);   // false for NaN
    VAD_REQUIRE(t >= 0, "tfilt_maps: t=%d is negative", t);
    VAD_ARG(vad_req_map_total("tfilt_maps", b * (long long)t, h, w));
    VAD_REQUIRE(maps != nullptr && out != nullptr, "tfilt_maps: maps or out is NULL");
    VAD_REQUIRE(vad_aligned(maps, 4) && vad_aligned(out, 4), "tfilt_maps: maps and out must be 4-byte aligned");
    VAD_ARG(vad_req_aligned("tfilt_maps", "state", state_or_null, 16));
    VAD_REQUIRE(vad_disjoint(maps, out, (size_t)b * t * h * w * sizeof(float)), "tfilt_maps: out overlaps maps (not in place)");
    if (b == 0 || t == 0) return VAD_OK;

    TfP p;
    p.maps = maps;
    p.out = out;
    p.state = (unsigned*)state_or_null;
    p.stream_words = tf_stream_words(h, w, op, k);
    p.plane = tf_plane_floats(h, w);
    p.fs = (size_t)h * w;
    p.items = 0;
    p.t = t;
    p.h = h;
    p.w = w;
    p.alpha = alpha;
    const bool vec = p.fs % 4 == 0 && vad_aligned(maps, 16) && vad_aligned(out, 16);
    switch (op) {
        case VAD_TFILT_MIN: return tfilt_launch_k<VAD_TFILT_MIN>(p, b, k, vec, stream);
        case VAD_TFILT_MAX: return tfilt_launch_k<VAD_TFILT_MAX>(p, b, k, vec, stream);
        case VAD_TFILT_MEAN: return tfilt_launch_k<VAD_TFILT_MEAN>(p, b, k, vec, stream);
        default: return tfilt_launch<VAD_TFILT_EMA, 1>(p, b, vec, stream);
    }
}
