// PIL-exact antialiased bilinear Resize of uint8 NHWC frames (include/vad_hip.h: vad_resize_u8): what
// `transforms.Resize((S, S))` does to a PIL image before ToTensor / Normalize (reference utils/dataset.py:65-70,
// utils/video_dataset.py:62-66, 191-195, 356-360, main.py:209-218), so camera-resolution frames can be handed to the scoring
// entry points in their VAD_X_U8_NHWC form without a CPU resample.
//
// The resample is separable integer fixed point: out = clip((2^21 + sum_j in[lo + j] * k_j) >> 22) per channel, horizontal
// pass first, its result rounded to uint8, then the vertical pass (coefficients: vad_resize_plan, csrc/pack.cpp).  Integer
// sums have no rounding order, so the device bytes ARE the host bytes; a pixel is < 2^8, a coefficient <= 2^22 and the
// coefficients of one output sum to 2^22 +- count / 2, so a sum stays below 2^31 and the 24-bit multiply-add applies.
//
// Two launches:
//   horizontal  one block stages RB consecutive input rows of one frame - ONE contiguous byte range - into LDS with 16-byte
//               coalesced loads (interleaved RGB at a 3-byte stride never becomes per-lane byte loads from global memory), then
//               every lane owns one (row, output column): it walks its taps four at a time, 12 bytes = three aligned LDS
//               dwords funnel-shifted to the lane's byte phase, against one 16-byte load of four coefficients (table laid out
//               [tap / 4][column][4], so neighbouring lanes read neighbouring 16 bytes).  Taps per output come from the table
//               (17 for 1920 -> 256, 3 when up-scaling, 128-129 at the 64-fold cap), padded with zero coefficients to a multiple of
//               four.  Only the rows the vertical pass reads are produced, into the caller's workspace.
//   vertical    every lane owns four consecutive bytes of an output row (channels are independent, so a row is a flat byte
//               string) and walks the rows of its taps with dword loads; rows of a width that is not a multiple of 4 pixels, and
//               the BGR swap of a vertical-only geometry, take the byte-per-lane form of the same kernel.
// A pass whose lengths are equal is skipped; with both skipped the frames are copied (channel-swapped for BGR input).
// Every kernel checks the plan's header against the call's geometry ON THE DEVICE and writes zeros instead of pixels on a
// mismatch: a plan made for another geometry cannot pass as a result, and its offsets are never followed.
//
// vad_resize_u8_f (second half of this file) takes the other pixel layouts a decoder delivers - one byte per pixel (PIL mode
// L: grey images, MVTec's ground-truth masks) and four (RGBA / BGRA, the fourth byte ignored) - with the SAME plan blob: the
// coefficients depend on the axis lengths only and the resample treats channels independently, so `convert('RGB')` followed by
// the resize is the resize of the plane, replicated, resp. of the first three bytes.  Its kernels are separate ones; the
// 3-byte kernels above are what vad_resize_u8 launches, unchanged.
#include <atomic>

#include <hip/hip_runtime.h>

#include "vad_common.h"
#include "vad_layout.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int RZ_THREADS = 256;
constexpr int RZ_LDS_TARGET = 32768;     // bytes of staged rows per block (more rows per block while they fit)
constexpr int RZ_LDS_SLACK = 64;         // 15 bytes of alignment phase in front, zero-weight taps read behind the last row

struct Geo { int in_h, in_w, out_h, out_w; };

__device__ __forceinline__ bool plan_matches(const int* __restrict__ plan, Geo g) {
    return (unsigned)plan[RZ_MAGIC] == VAD_RESIZE_MAGIC && (unsigned)plan[RZ_TAG] == ((unsigned)VAD_ABI_VERSION << 16 | 1u) &&
           plan[RZ_IN_H] == g.in_h && plan[RZ_IN_W] == g.in_w && plan[RZ_OUT_H] == g.out_h && plan[RZ_OUT_W] == g.out_w;
}

__device__ __forceinline__ unsigned char rz_round(unsigned acc) {
    const unsigned v = (acc + (1u << 21)) >> 22;
    return (unsigned char)(v > 255u ? 255u : v);
}

// src [frames][in_h][in_w][3] -> out [frames][rows][out_w][3], rows = input rows [row0, row0 + rows).  grid (row chunks, frames).
// src_begin / src_end bound the whole source tensor: the 16-byte staging loads of the first and last chunk are trimmed to it.
__global__ __launch_bounds__(RZ_THREADS) void resize_h_kernel(const unsigned char* __restrict__ src, const unsigned char* src_begin,
                                                              const unsigned char* src_end, const int* __restrict__ plan, Geo g,
                                                              unsigned char* __restrict__ out, int row0, int rows, int rb, int swap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.y;
    const int r0 = blockIdx.x * rb;
    const int nr = rows - r0 < rb ? rows - r0 : rb;
    const int out_w = g.out_w;
    unsigned char* o_base = out + ((n * rows + r0) * (size_t)out_w) * 3;
    if (!plan_matches(plan, g) || plan[RZ_KPAD_H] <= 0) {
        for (int i = tid; i < nr * out_w * 3; i += RZ_THREADS) o_base[i] = 0;
        return;
    }
    const int row_bytes = g.in_w * 3;
    const unsigned char* a = src + (n * g.in_h + row0 + r0) * (size_t)row_bytes;
    const int phase = (int)((uintptr_t)a & 15);
    const unsigned char* a16 = a - phase;
    const int nvec = (phase + nr * row_bytes + 15) >> 4;
    for (int v = tid; v < nvec; v += RZ_THREADS) {
        const unsigned char* p = a16 + 16 * (size_t)v;
        u32x4 val;
        if (p >= src_begin && p + 16 <= src_end) {
            val = *(const u32x4*)p;
        } else {                                             // head / tail of the tensor: byte by byte, zeros outside
            unsigned w[4] = {0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b)
                if (p + b >= src_begin && p + b < src_end) w[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
            val = u32x4{w[0], w[1], w[2], w[3]};
        }
        *(u32x4*)(lds + 16 * v) = val;
    }
    __syncthreads();
    const int kpad = plan[RZ_KPAD_H];
    const int* lo_t = plan + plan[RZ_OFF_H];
    const int* cnt_t = lo_t + out_w;
    const i32x4* w_t = (const i32x4*)(lo_t + ((2 * out_w + 3) & ~3));
    const int c0 = swap ? 2 : 0, c2 = swap ? 0 : 2;          // input channel that feeds output channel 0 / 2
    for (int it = tid; it < nr * out_w; it += RZ_THREADS) {
        const int r = it / out_w, o = it - r * out_w;
        int lo = lo_t[o], cnt = cnt_t[o];
        lo = lo < 0 ? 0 : (lo > g.in_w - 1 ? g.in_w - 1 : lo);       // a damaged table cannot steer a read out of the staged rows
        cnt = cnt < 0 ? 0 : (cnt > g.in_w - lo ? g.in_w - lo : cnt);
        cnt = cnt > kpad ? kpad : cnt;
        const int p = phase + r * row_bytes + lo * 3;                // byte position of the first tap in LDS
        const unsigned* q = (const unsigned*)(lds + (p & ~3));
        const unsigned sh = (unsigned)(p & 3) * 8u;
        unsigned acc[3] = {0u, 0u, 0u};
        unsigned d0 = q[0];
        const int groups = (cnt + 3) >> 2;
        for (int gi = 0; gi < groups; ++gi) {
            const i32x4 k = w_t[(size_t)gi * out_w + o];
            const unsigned d1 = q[3 * gi + 1], d2 = q[3 * gi + 2], d3 = q[3 * gi + 3];
            // 12 bytes of four pixels at the lane's byte phase: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            const unsigned e0 = (unsigned)((((unsigned long long)d1 << 32) | d0) >> sh);
            const unsigned e1 = (unsigned)((((unsigned long long)d2 << 32) | d1) >> sh);
            const unsigned e2 = (unsigned)((((unsigned long long)d3 << 32) | d2) >> sh);
            d0 = d3;
            acc[0] += (e0 & 255u) * (unsigned)k[0] + (e0 >> 24) * (unsigned)k[1] + ((e1 >> 16) & 255u) * (unsigned)k[2] + ((e2 >> 8) & 255u) * (unsigned)k[3];
            acc[1] += ((e0 >> 8) & 255u) * (unsigned)k[0] + (e1 & 255u) * (unsigned)k[1] + (e1 >> 24) * (unsigned)k[2] + ((e2 >> 16) & 255u) * (unsigned)k[3];
            acc[2] += ((e0 >> 16) & 255u) * (unsigned)k[0] + ((e1 >> 8) & 255u) * (unsigned)k[1] + (e2 & 255u) * (unsigned)k[2] + (e2 >> 24) * (unsigned)k[3];
        }
        unsigned char* op = o_base + (size_t)it * 3;
        op[0] = rz_round(acc[c0]);
        op[1] = rz_round(acc[1]);
        op[2] = rz_round(acc[c2]);
    }
}

// src: rows [row0, row0 + rows) of every frame, [frames][rows][w][3] with frame stride src_fs bytes -> out [frames][out_h][w][3].
// V = bytes per lane (4: dword loads, needs w % 4 == 0 and 4-byte aligned bases; 1: any width, and the only form that can swap
// channels).  grid (items of one frame / 256, frames).
template <int V>
__global__ __launch_bounds__(RZ_THREADS) void resize_v_kernel(const unsigned char* __restrict__ src, size_t src_fs, const int* __restrict__ plan,
                                                              Geo g, unsigned char* __restrict__ out, int row0, int rows, int swap) {
    const int row_bytes = g.out_w * 3, rv = row_bytes / V;
    const long long item = (long long)blockIdx.x * RZ_THREADS + threadIdx.x;
    if (item >= (long long)g.out_h * rv) return;
    const size_t n = blockIdx.y;
    const int o = (int)(item / rv), xb = (int)(item - (long long)o * rv) * V;
    unsigned char* op = out + (n * g.out_h + o) * (size_t)row_bytes + xb;
    if (!plan_matches(plan, g) || plan[RZ_KPAD_V] <= 0) {
        for (int b = 0; b < V; ++b) op[b] = 0;
        return;
    }
    const int kpad = plan[RZ_KPAD_V];
    const int* lo_t = plan + plan[RZ_OFF_V];
    const int* cnt_t = lo_t + g.out_h;
    const i32x4* w_t = (const i32x4*)(lo_t + ((2 * g.out_h + 3) & ~3));
    int lo = lo_t[o] - row0, cnt = cnt_t[o];
    lo = lo < 0 ? 0 : (lo > rows - 1 ? rows - 1 : lo);
    cnt = cnt < 0 ? 0 : (cnt > rows - lo ? rows - lo : cnt);
    cnt = cnt > kpad ? kpad : cnt;
    const int sx = (V == 1 && swap) ? xb + 2 - 2 * (xb % 3) : xb;    // source byte of this output byte (R <-> B)
    const unsigned char* sp = src + n * src_fs + sx;
    unsigned acc[V];
    for (int b = 0; b < V; ++b) acc[b] = 0u;
    const int groups = (cnt + 3) >> 2;
    for (int gi = 0; gi < groups; ++gi) {
        const i32x4 k = w_t[(size_t)gi * g.out_h + o];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int row = lo + 4 * gi + t;
            row = row > rows - 1 ? rows - 1 : row;            // taps behind count have weight 0: read the last row again
            const unsigned char* rp = sp + (size_t)row * row_bytes;
            if (V == 4) {
                const unsigned d = *(const unsigned*)rp;
                acc[0] += (d & 255u) * (unsigned)k[t];
                acc[1 % V] += ((d >> 8) & 255u) * (unsigned)k[t];
                acc[2 % V] += ((d >> 16) & 255u) * (unsigned)k[t];
                acc[3 % V] += (d >> 24) * (unsigned)k[t];
            } else {
                acc[0] += (unsigned)rp[0] * (unsigned)k[t];
            }
        }
    }
    if (V == 4) {
        *(unsigned*)op = (unsigned)rz_round(acc[0]) | (unsigned)rz_round(acc[1 % V]) << 8 | (unsigned)rz_round(acc[2 % V]) << 16 |
                         (unsigned)rz_round(acc[3 % V]) << 24;
    } else {
        op[0] = rz_round(acc[0]);
    }
}

// identity geometry with BGR input: out[b] = src[b with R and B exchanged]
__global__ __launch_bounds__(RZ_THREADS) void swap_copy_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ out, size_t pixels) {
    const size_t i = (size_t)blockIdx.x * RZ_THREADS + threadIdx.x;
    if (i >= pixels) return;
    const unsigned char b = src[3 * i], gch = src[3 * i + 1], r = src[3 * i + 2];
    out[3 * i] = r; out[3 * i + 1] = gch; out[3 * i + 2] = b;
}

struct Rows { int row0, rows; };
Rows rows_needed(int in_h, int out_h) {
    if (in_h == out_h) return Rows{0, in_h};
    int row0, row1, unused;
    vad_resize_bounds(in_h, out_h, 0, &row0, &unused);
    vad_resize_bounds(in_h, out_h, out_h - 1, &unused, &row1);
    return Rows{row0, row1 - row0};
}

}  // namespace

extern "C" size_t vad_resize_workspace_bytes(long long n, int in_h, int in_w, int out_h, int out_w) {
    if (n < 0 || !vad_resize_axis_ok(in_h, out_h) || !vad_resize_axis_ok(in_w, out_w)) return 0;
    if (in_h == out_h || in_w == out_w) return 0;                        // at most one pass: it writes dst directly
    return (size_t)n * rows_needed(in_h, out_h).rows * out_w * 3;
}

extern "C" int vad_resize_u8(const void* src, long long n, int in_h, int in_w, int channel_order, const void* plan_dev, void* dst, int out_h,
                             int out_w, void* workspace, size_t workspace_bytes, void* stream) {
    VAD_REQUIRE(vad_resize_axis_ok(in_h, out_h) && vad_resize_axis_ok(in_w, out_w),
                "resize_u8: unsupported geometry %dx%d -> %dx%d (input sides 1..%d, output sides 1..%d, at most a %d-fold reduction per axis)",
                in_h, in_w, out_h, out_w, VAD_RESIZE_MAX_IN, VAD_RESIZE_MAX_OUT, VAD_RESIZE_MAX_RATIO);
    VAD_REQUIRE(n >= 0, "resize_u8: n=%lld is negative", n);
    VAD_REQUIRE(channel_order == 0 || channel_order == 1, "resize_u8: channel_order=%d must be 0 (RGB) or 1 (BGR)", channel_order);
    VAD_REQUIRE(src && dst && plan_dev, "resize_u8: null pointer");
    VAD_REQUIRE(((uintptr_t)plan_dev & 15) == 0, "resize_u8: the plan blob must be 16-B aligned");
    const size_t need = vad_resize_workspace_bytes(n, in_h, in_w, out_h, out_w);
    if (need && (!workspace || workspace_bytes < need))
        return vad_fail(VAD_ERR_WS, "resize_u8: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    if (n == 0) return VAD_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* s = (const unsigned char*)src;
    unsigned char* d = (unsigned char*)dst;
    const int* plan = (const int*)plan_dev;
    const Geo g{in_h, in_w, out_h, out_w};
    const bool hp = in_w != out_w, vp = in_h != out_h;
    const size_t in_fs = (size_t)in_h * in_w * 3;
    if (!hp && !vp) {
        if (!channel_order) {
            VAD_HIP_TRY(hipMemcpyAsync(d, s, (size_t)n * in_fs, hipMemcpyDeviceToDevice, st));
            return VAD_OK;
        }
        const size_t pixels = (size_t)n * in_h * in_w;
        VAD_REQUIRE((pixels + RZ_THREADS - 1) / RZ_THREADS < (1ull << 31), "resize_u8: grid out of range (n=%lld)", n);
        hipLaunchKernelGGL(swap_copy_kernel, dim3((unsigned)((pixels + RZ_THREADS - 1) / RZ_THREADS)), dim3(RZ_THREADS), 0, st, s, d, pixels);
        VAD_LAUNCH_CHECK();
        return VAD_OK;
    }
    const Rows R = rows_needed(in_h, out_h);
    const int row_bytes = in_w * 3;
    int rb = RZ_LDS_TARGET / row_bytes;
    rb = rb < 1 ? 1 : (rb > 16 ? 16 : rb);
    rb = rb > R.rows ? R.rows : rb;
    const size_t lds_bytes = (((size_t)rb * row_bytes + 15) & ~(size_t)15) + RZ_LDS_SLACK;      // <= 48 KB + slack at in_w = 16384
    unsigned char* mid = hp && vp ? (unsigned char*)workspace : d;                              // what the horizontal pass writes
    const size_t mid_fs = (size_t)R.rows * out_w * 3;
    const bool v4 = out_w % 4 == 0 && ((uintptr_t)d & 3) == 0 && (((uintptr_t)(hp ? mid : s)) & 3) == 0 && !(channel_order && !hp);
    const long long v_items = (long long)out_h * (out_w * 3 / (v4 ? 4 : 1));
    for (long long f0 = 0; f0 < n; f0 += 65535) {                                               // frames in slices of gridDim.y
        const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
        if (hp) {
            hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)((R.rows + rb - 1) / rb), m), dim3(RZ_THREADS), lds_bytes, st, s + f0 * in_fs, s,
                               s + (size_t)n * in_fs, plan, g, mid + f0 * mid_fs, R.row0, R.rows, rb, channel_order);
            VAD_LAUNCH_CHECK();
        }
        if (vp) {
            const unsigned char* vs = hp ? mid + f0 * mid_fs : s + f0 * in_fs + (size_t)R.row0 * row_bytes;
            const size_t vfs = hp ? mid_fs : in_fs;
            const dim3 grid((unsigned)((v_items + RZ_THREADS - 1) / RZ_THREADS), m);
            unsigned char* vd = d + f0 * (size_t)out_h * out_w * 3;
            if (v4) hipLaunchKernelGGL(resize_v_kernel<4>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, 0);
            else hipLaunchKernelGGL(resize_v_kernel<1>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, hp ? 0 : channel_order);
            VAD_LAUNCH_CHECK();
        }
    }
    return VAD_OK;
}

// ------------------------------------------------------------------------------------------------ other pixel formats
namespace {

// Stage nvec 16-byte vectors from a16 (16-B aligned, may start in front of / end behind the tensor) into LDS; ends with the barrier.
__device__ __forceinline__ void stage_rows(unsigned char* lds, const unsigned char* a16, int nvec, const unsigned char* src_begin,
                                           const unsigned char* src_end) {
    for (int v = threadIdx.x; v < nvec; v += RZ_THREADS) {
        const unsigned char* p = a16 + 16 * (size_t)v;
        u32x4 val;
        if (p >= src_begin && p + 16 <= src_end) {
            val = *(const u32x4*)p;
        } else {                                             // head / tail of the tensor: byte by byte, zeros outside
            unsigned w[4] = {0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b)
                if (p + b >= src_begin && p + b < src_end) w[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
            val = u32x4{w[0], w[1], w[2], w[3]};
        }
        *(u32x4*)(lds + 16 * v) = val;
    }
    __syncthreads();
}

// One tap: a byte times a coefficient.  Both are below 2^24 (a coefficient is at most 2^22), so the 24-bit multiply is exact and
// the sum of a tap group fuses into full-rate 24-bit multiply-adds.
__device__ __forceinline__ unsigned tap(unsigned byte, int k) { return __umul24(byte, (unsigned)k); }

__device__ __forceinline__ unsigned funnel(unsigned hi, unsigned lo, unsigned sh) {
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
}

// Horizontal pass of BPP-byte pixels: src [frames][in_h][in_w][BPP] -> out [frames][rows][out_w][oc], rows = input rows
// [row0, row0 + rows); grid (row chunks, frames), staging as resize_h_kernel.
//   BPP 1  four taps = four consecutive bytes: two LDS dwords funnel-shifted to the lane's phase (an odd-width frame starts every
//          row at another one).  The value is stored oc times: once into the workspace or a mask, 3 times as `convert('RGB')`.
//   BPP 4  four taps = 16 bytes; the fourth byte of a pixel is never multiplied.  oc = 3: 3-byte pixels, in output order (swap:
//          the source is BGRA).
template <int BPP>
__global__ __launch_bounds__(RZ_THREADS) void resize_hf_kernel(const unsigned char* __restrict__ src, const unsigned char* src_begin,
                                                               const unsigned char* src_end, const int* __restrict__ plan, Geo g,
                                                               unsigned char* __restrict__ out, int row0, int rows, int rb, int oc, int swap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.y;
    const int r0 = blockIdx.x * rb;
    const int nr = rows - r0 < rb ? rows - r0 : rb;
    const int out_w = g.out_w;
    unsigned char* o_base = out + ((n * rows + r0) * (size_t)out_w) * oc;
    if (!plan_matches(plan, g) || plan[RZ_KPAD_H] <= 0) {
        for (int i = tid; i < nr * out_w * oc; i += RZ_THREADS) o_base[i] = 0;
        return;
    }
    const int row_bytes = g.in_w * BPP;
    const unsigned char* a = src + (n * g.in_h + row0 + r0) * (size_t)row_bytes;
    const int phase = (int)((uintptr_t)a & 15);
    stage_rows(lds, a - phase, (phase + nr * row_bytes + 15) >> 4, src_begin, src_end);
    const int kpad = plan[RZ_KPAD_H];
    const int* lo_t = plan + plan[RZ_OFF_H];
    const int* cnt_t = lo_t + out_w;
    const i32x4* w_t = (const i32x4*)(lo_t + ((2 * out_w + 3) & ~3));
    for (int it = tid; it < nr * out_w; it += RZ_THREADS) {
        const int r = it / out_w, o = it - r * out_w;
        int lo = lo_t[o], cnt = cnt_t[o];
        lo = lo < 0 ? 0 : (lo > g.in_w - 1 ? g.in_w - 1 : lo);       // a damaged table cannot steer a read out of the staged rows
        cnt = cnt < 0 ? 0 : (cnt > g.in_w - lo ? g.in_w - lo : cnt);
        cnt = cnt > kpad ? kpad : cnt;
        const int p = phase + r * row_bytes + lo * BPP;              // byte position of the first tap in LDS
        const unsigned* q = (const unsigned*)(lds + (p & ~3));
        const unsigned sh = (unsigned)(p & 3) * 8u;
        const int groups = (cnt + 3) >> 2;
        unsigned d0 = q[0];
        unsigned char* op = o_base + (size_t)it * oc;
        if (BPP == 1) {
            unsigned acc = 0u;
            for (int gi = 0; gi < groups; ++gi) {
                const i32x4 k = w_t[(size_t)gi * out_w + o];
                const unsigned d1 = q[gi + 1];
                const unsigned e = funnel(d1, d0, sh);
                d0 = d1;
                acc += tap(e & 255u, k[0]) + tap((e >> 8) & 255u, k[1]) + tap((e >> 16) & 255u, k[2]) + tap(e >> 24, k[3]);
            }
            const unsigned char v = rz_round(acc);
            op[0] = v;
            if (oc == 3) { op[1] = v; op[2] = v; }
        } else {
            unsigned acc[3] = {0u, 0u, 0u};
            for (int gi = 0; gi < groups; ++gi) {
                const i32x4 k = w_t[(size_t)gi * out_w + o];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const unsigned d1 = q[4 * gi + t + 1];
                    const unsigned e = funnel(d1, d0, sh);           // one pixel: c0 c1 c2 x
                    d0 = d1;
                    acc[0] += tap(e & 255u, k[t]);
                    acc[1] += tap((e >> 8) & 255u, k[t]);
                    acc[2] += tap((e >> 16) & 255u, k[t]);
                }
            }
            op[0] = rz_round(acc[swap ? 2 : 0]);
            op[1] = rz_round(acc[1]);
            op[2] = rz_round(acc[swap ? 0 : 2]);
        }
    }
}

// Vertical pass of one channel: src = rows [row0, row0 + rows) of every frame, [frames][rows][w] with frame stride src_fs bytes ->
// out [frames][out_h][w][oc].  V = source bytes per lane (4: dword loads and stores, needs w % 4 == 0 and 4-byte aligned bases;
// 1: any width).  grid (items of one frame / 256, frames).
template <int V>
__global__ __launch_bounds__(RZ_THREADS) void resize_v1_kernel(const unsigned char* __restrict__ src, size_t src_fs, const int* __restrict__ plan,
                                                               Geo g, unsigned char* __restrict__ out, int row0, int rows, int oc) {
    const int w = g.out_w, rv = w / V;
    const long long item = (long long)blockIdx.x * RZ_THREADS + threadIdx.x;
    if (item >= (long long)g.out_h * rv) return;
    const size_t n = blockIdx.y;
    const int o = (int)(item / rv), xb = (int)(item - (long long)o * rv) * V;
    unsigned char* op = out + ((n * g.out_h + o) * (size_t)w + xb) * oc;
    if (!plan_matches(plan, g) || plan[RZ_KPAD_V] <= 0) {
        for (int b = 0; b < V * oc; ++b) op[b] = 0;
        return;
    }
    const int kpad = plan[RZ_KPAD_V];
    const int* lo_t = plan + plan[RZ_OFF_V];
    const int* cnt_t = lo_t + g.out_h;
    const i32x4* w_t = (const i32x4*)(lo_t + ((2 * g.out_h + 3) & ~3));
    int lo = lo_t[o] - row0, cnt = cnt_t[o];
    lo = lo < 0 ? 0 : (lo > rows - 1 ? rows - 1 : lo);
    cnt = cnt < 0 ? 0 : (cnt > rows - lo ? rows - lo : cnt);
    cnt = cnt > kpad ? kpad : cnt;
    const unsigned char* sp = src + n * src_fs + xb;
    unsigned acc[V];
    for (int b = 0; b < V; ++b) acc[b] = 0u;
    const int groups = (cnt + 3) >> 2;
    for (int gi = 0; gi < groups; ++gi) {
        const i32x4 k = w_t[(size_t)gi * g.out_h + o];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int row = lo + 4 * gi + t;
            row = row > rows - 1 ? rows - 1 : row;            // taps behind count have weight 0: read the last row again
            const unsigned char* rp = sp + (size_t)row * w;
            if (V == 4) {
                const unsigned d = *(const unsigned*)rp;
                acc[0] += tap(d & 255u, k[t]);
                acc[1 % V] += tap((d >> 8) & 255u, k[t]);
                acc[2 % V] += tap((d >> 16) & 255u, k[t]);
                acc[3 % V] += tap(d >> 24, k[t]);
            } else {
                acc[0] += tap((unsigned)rp[0], k[t]);
            }
        }
    }
    if (V == 4) {
        const unsigned v0 = rz_round(acc[0]), v1 = rz_round(acc[1 % V]), v2 = rz_round(acc[2 % V]), v3 = rz_round(acc[3 % V]);
        unsigned* o4 = (unsigned*)op;
        if (oc == 3) {                                        // v0 v0 v0 v1 | v1 v1 v2 v2 | v2 v3 v3 v3
            o4[0] = v0 * 0x010101u | v1 << 24;
            o4[1] = v1 * 0x0101u | v2 * 0x01010000u;
            o4[2] = v2 | v3 * 0x01010100u;
        } else {
            o4[0] = v0 | v1 << 8 | v2 << 16 | v3 << 24;
        }
    } else {
        const unsigned char v = rz_round(acc[0]);
        op[0] = v;
        if (oc == 3) { op[1] = v; op[2] = v; }
    }
}

// Vertical pass of 4-byte pixels whose horizontal pass is skipped: src = rows [row0, row0 + rows) of every frame,
// [frames][rows][w][4] with frame stride src_fs bytes -> out [frames][out_h][w][3].  A lane owns one pixel; A: src is 4-byte
// aligned (every row and frame stride is a multiple of 4), so a pixel is one dword load.  grid (pixels of one frame / 256, frames).
template <bool A>
__global__ __launch_bounds__(RZ_THREADS) void resize_v43_kernel(const unsigned char* __restrict__ src, size_t src_fs, const int* __restrict__ plan,
                                                                Geo g, unsigned char* __restrict__ out, int row0, int rows, int swap) {
    const int w = g.out_w;
    const long long item = (long long)blockIdx.x * RZ_THREADS + threadIdx.x;
    if (item >= (long long)g.out_h * w) return;
    const size_t n = blockIdx.y;
    const int o = (int)(item / w), x = (int)(item - (long long)o * w);
    unsigned char* op = out + ((n * g.out_h + o) * (size_t)w + x) * 3;
    if (!plan_matches(plan, g) || plan[RZ_KPAD_V] <= 0) {
        op[0] = 0; op[1] = 0; op[2] = 0;
        return;
    }
    const int kpad = plan[RZ_KPAD_V];
    const int* lo_t = plan + plan[RZ_OFF_V];
    const int* cnt_t = lo_t + g.out_h;
    const i32x4* w_t = (const i32x4*)(lo_t + ((2 * g.out_h + 3) & ~3));
    int lo = lo_t[o] - row0, cnt = cnt_t[o];
    lo = lo < 0 ? 0 : (lo > rows - 1 ? rows - 1 : lo);
    cnt = cnt < 0 ? 0 : (cnt > rows - lo ? rows - lo : cnt);
    cnt = cnt > kpad ? kpad : cnt;
    const unsigned char* sp = src + n * src_fs + (size_t)x * 4;
    unsigned acc[3] = {0u, 0u, 0u};
    const int groups = (cnt + 3) >> 2;
    for (int gi = 0; gi < groups; ++gi) {
        const i32x4 k = w_t[(size_t)gi * g.out_h + o];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int row = lo + 4 * gi + t;
            row = row > rows - 1 ? rows - 1 : row;            // taps behind count have weight 0: read the last row again
            const unsigned char* rp = sp + (size_t)row * w * 4;
            const unsigned d = A ? *(const unsigned*)rp : ((unsigned)rp[0] | (unsigned)rp[1] << 8 | (unsigned)rp[2] << 16);
            acc[0] += tap(d & 255u, k[t]);
            acc[1] += tap((d >> 8) & 255u, k[t]);
            acc[2] += tap((d >> 16) & 255u, k[t]);
        }
    }
    op[0] = rz_round(acc[swap ? 2 : 0]);
    op[1] = rz_round(acc[1]);
    op[2] = rz_round(acc[swap ? 0 : 2]);
}

// identity geometry: BPP 1: the byte oc times; BPP 4: the first three bytes of a pixel, R and B exchanged with swap
template <int BPP>
__global__ __launch_bounds__(RZ_THREADS) void convert_copy_kernel(const unsigned char* __restrict__ src, const int* __restrict__ plan, Geo g,
                                                                  unsigned char* __restrict__ out, size_t pixels, int oc, int swap) {
    const size_t i = (size_t)blockIdx.x * RZ_THREADS + threadIdx.x;
    if (i >= pixels) return;
    unsigned char* op = out + i * oc;
    const bool ok = plan_matches(plan, g);
    if (BPP == 1) {
        const unsigned char v = ok ? src[i] : (unsigned char)0;
        op[0] = v;
        if (oc == 3) { op[1] = v; op[2] = v; }
    } else {
        const unsigned char c0 = ok ? src[4 * i] : (unsigned char)0, c1 = ok ? src[4 * i + 1] : (unsigned char)0,
                            c2 = ok ? src[4 * i + 2] : (unsigned char)0;
        op[0] = swap ? c2 : c0; op[1] = c1; op[2] = swap ? c0 : c2;
    }
}

inline int bytes_per_pixel(int pixel_format) { return pixel_format == VAD_PIX_L ? 1 : (pixel_format == VAD_PIX_RGBA || pixel_format == VAD_PIX_BGRA ? 4 : 3); }
inline bool format_ok(int pixel_format, int out_channels) {
    return pixel_format >= VAD_PIX_RGB && pixel_format <= VAD_PIX_BGRA && (out_channels == 3 || (out_channels == 1 && pixel_format == VAD_PIX_L));
}

}  // namespace

extern "C" size_t vad_resize_workspace_bytes_f(long long n, int in_h, int in_w, int out_h, int out_w, int pixel_format, int out_channels) {
    if (!format_ok(pixel_format, out_channels)) return 0;
    // the intermediate of a one-byte format is one byte per pixel whatever out_channels is: the value is replicated on the last store
    return vad_resize_workspace_bytes(n, in_h, in_w, out_h, out_w) / (pixel_format == VAD_PIX_L ? 3 : 1);
}

extern "C" int vad_resize_u8_f(const void* src, long long n, int in_h, int in_w, int pixel_format, const void* plan_dev, void* dst, int out_h,
                               int out_w, int out_channels, void* workspace, size_t workspace_bytes, void* stream) {
    VAD_REQUIRE(vad_resize_axis_ok(in_h, out_h) && vad_resize_axis_ok(in_w, out_w),
                "resize_u8_f: unsupported geometry %dx%d -> %dx%d (input sides 1..%d, output sides 1..%d, at most a %d-fold reduction per axis)",
                in_h, in_w, out_h, out_w, VAD_RESIZE_MAX_IN, VAD_RESIZE_MAX_OUT, VAD_RESIZE_MAX_RATIO);
    VAD_REQUIRE(n >= 0, "resize_u8_f: n=%lld is negative", n);
    VAD_REQUIRE(pixel_format >= VAD_PIX_RGB && pixel_format <= VAD_PIX_BGRA,
                "resize_u8_f: pixel_format=%d must be VAD_PIX_RGB (0), _BGR (1), _L (2), _RGBA (3) or _BGRA (4)", pixel_format);
    VAD_REQUIRE(format_ok(pixel_format, out_channels), "resize_u8_f: out_channels=%d must be 3, or 1 with VAD_PIX_L (pixel_format=%d)", out_channels,
                pixel_format);
    if (pixel_format == VAD_PIX_RGB || pixel_format == VAD_PIX_BGR)
        return vad_resize_u8(src, n, in_h, in_w, pixel_format, plan_dev, dst, out_h, out_w, workspace, workspace_bytes, stream);
    VAD_REQUIRE(src && dst && plan_dev, "resize_u8_f: null pointer");
    VAD_REQUIRE(((uintptr_t)plan_dev & 15) == 0, "resize_u8_f: the plan blob must be 16-B aligned");
    const size_t need = vad_resize_workspace_bytes_f(n, in_h, in_w, out_h, out_w, pixel_format, out_channels);
    if (need && (!workspace || workspace_bytes < need))
        return vad_fail(VAD_ERR_WS, "resize_u8_f: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    if (n == 0) return VAD_OK;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* s = (const unsigned char*)src;
    unsigned char* d = (unsigned char*)dst;
    const int* plan = (const int*)plan_dev;
    const Geo g{in_h, in_w, out_h, out_w};
    const bool hp = in_w != out_w, vp = in_h != out_h, mono = pixel_format == VAD_PIX_L;
    const int bpp = bytes_per_pixel(pixel_format), swap = pixel_format == VAD_PIX_BGRA;
    const int mc = mono ? 1 : 3;                                                                // bytes per pixel behind the horizontal pass
    const size_t in_fs = (size_t)in_h * in_w * bpp;
    if (!hp && !vp) {
        const size_t pixels = (size_t)n * in_h * in_w;
        VAD_REQUIRE((pixels + RZ_THREADS - 1) / RZ_THREADS < (1ull << 31), "resize_u8_f: grid out of range (n=%lld)", n);
        const dim3 grid((unsigned)((pixels + RZ_THREADS - 1) / RZ_THREADS));
        if (mono) hipLaunchKernelGGL(convert_copy_kernel<1>, grid, dim3(RZ_THREADS), 0, st, s, plan, g, d, pixels, out_channels, 0);
        else hipLaunchKernelGGL(convert_copy_kernel<4>, grid, dim3(RZ_THREADS), 0, st, s, plan, g, d, pixels, 3, swap);
        VAD_LAUNCH_CHECK();
        return VAD_OK;
    }
    const Rows R = rows_needed(in_h, out_h);
    const int row_bytes = in_w * bpp;
    int rb = RZ_LDS_TARGET / row_bytes;
    rb = rb < 1 ? 1 : (rb > 16 ? 16 : rb);
    rb = rb > R.rows ? R.rows : rb;
    const size_t lds_bytes = (((size_t)rb * row_bytes + 15) & ~(size_t)15) + RZ_LDS_SLACK;      // <= 64 KB + slack: one row of 16384 4-byte pixels
    if (hp && lds_bytes > 64 * 1024) {                                                          // needs the attribute, once per process
        static std::atomic<bool> attr_set;                                                      // (setting it twice from two threads is harmless)
        if (!attr_set.load(std::memory_order_acquire)) {
            VAD_HIP_TRY(hipFuncSetAttribute((const void*)resize_hf_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024 + 2 * RZ_LDS_SLACK));
            attr_set.store(true, std::memory_order_release);
        }
    }
    unsigned char* mid = hp && vp ? (unsigned char*)workspace : d;                              // what the horizontal pass writes
    const int h_oc = vp ? mc : out_channels;                                                    // ... and how many bytes per pixel
    const size_t mid_fs = (size_t)R.rows * out_w * h_oc;
    const bool v4 = out_w % 4 == 0 && ((uintptr_t)d & 3) == 0 && (((uintptr_t)(hp ? mid : s)) & 3) == 0;
    for (long long f0 = 0; f0 < n; f0 += 65535) {                                               // frames in slices of gridDim.y
        const unsigned m = (unsigned)(n - f0 < 65535 ? n - f0 : 65535);
        if (hp) {
            const dim3 grid((unsigned)((R.rows + rb - 1) / rb), m);
            if (mono) hipLaunchKernelGGL(resize_hf_kernel<1>, grid, dim3(RZ_THREADS), lds_bytes, st, s + f0 * in_fs, s, s + (size_t)n * in_fs, plan, g,
                                         mid + f0 * mid_fs, R.row0, R.rows, rb, h_oc, 0);
            else hipLaunchKernelGGL(resize_hf_kernel<4>, grid, dim3(RZ_THREADS), lds_bytes, st, s + f0 * in_fs, s, s + (size_t)n * in_fs, plan, g,
                                    mid + f0 * mid_fs, R.row0, R.rows, rb, 3, swap);
            VAD_LAUNCH_CHECK();
        }
        if (vp) {
            const unsigned char* vs = hp ? mid + f0 * mid_fs : s + f0 * in_fs + (size_t)R.row0 * row_bytes;
            const size_t vfs = hp ? mid_fs : in_fs;
            unsigned char* vd = d + f0 * (size_t)out_h * out_w * out_channels;
            if (mono) {
                const dim3 grid((unsigned)(((long long)out_h * (out_w / (v4 ? 4 : 1)) + RZ_THREADS - 1) / RZ_THREADS), m);
                if (v4) hipLaunchKernelGGL(resize_v1_kernel<4>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, out_channels);
                else hipLaunchKernelGGL(resize_v1_kernel<1>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, out_channels);
            } else if (hp) {                                                                    // 3-byte rows in output order: the 3-byte kernel
                const dim3 grid((unsigned)(((long long)out_h * (out_w * 3 / (v4 ? 4 : 1)) + RZ_THREADS - 1) / RZ_THREADS), m);
                if (v4) hipLaunchKernelGGL(resize_v_kernel<4>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, 0);
                else hipLaunchKernelGGL(resize_v_kernel<1>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, 0);
            } else {
                const dim3 grid((unsigned)(((long long)out_h * out_w + RZ_THREADS - 1) / RZ_THREADS), m);
                if (((uintptr_t)s & 3) == 0) hipLaunchKernelGGL(resize_v43_kernel<true>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, swap);
                else hipLaunchKernelGGL(resize_v43_kernel<false>, grid, dim3(RZ_THREADS), 0, st, vs, vfs, plan, g, vd, R.row0, R.rows, swap);
            }
            VAD_LAUNCH_CHECK();
        }
    }
    return VAD_OK;
}
