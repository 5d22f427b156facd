// Frame bank -> batch: out[i] = bank[index[i]] for uint8 frames [h][w][3] that stay resident in HBM, either as the float32
// NCHW batch the models and trainers take (ToTensor + Normalize(0.5, 0.5) = vad_norm_u8, bit for bit) or as a plain uint8 NHWC
// copy for the scoring entry points' uint8 ingest.  The dataset's __getitem__ (T transforms + torch.stack per sequence,
// utils/video_dataset.py:136-152, 301-329) and the DataLoader collate become ONE launch per batch; overlapping sequences are
// index entries, not copies.  HBM-bound: 3 bytes read and 12 (3) written per pixel.
//
// Two kernels per output format, chosen per launch by the host from the addresses it was given:
//   vector  f32: a lane takes 4 consecutive pixels = 12 source bytes (one 12-byte load, 4-byte aligned) and writes one 16-byte
//           store per plane; consecutive lanes take consecutive pixel quads, so every wave instruction covers one contiguous
//           768-byte (load) / 1-KiB (store) run.  Needs h*w % 4 == 0 (every frame and plane then starts on the alignment the
//           bank / out pointer has), bank % 4 == 0 and out % 16 == 0.
//           u8: 16-byte loads and stores; needs 3*h*w % 16 == 0 and both pointers 16-byte aligned.
//   plain   one pixel (f32) or one byte (u8) per lane: any h, w >= 1 and any byte address.
// An index outside [0, bank_frames) skips its output frame: nothing is read, nothing is written.
#include <hip/hip_runtime.h>

#include "vad_common.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_UNROLL = 4;      // items per lane, GATHER_THREADS apart: 4 loads in flight before the first store

// vad_norm_u8 without the ten-instruction division sequence: q = v * RN(1/255) is within an ulp of v / 255, the residual
// e = v - 255 q is then exact in fp32 (one fma), and q + e * RN(1/255) rounds once more (the second fma).  That this equals the
// IEEE quotient is a finite statement - 256 inputs - and the exactness tests (tests/test_hip_frame_bank.py) check every one of
// them against vad_norm_u8's definition, through the vector and the plain kernel.
__device__ __forceinline__ float gather_norm(float v) {
    const float r = 1.0f / 255.0f;                       // constant-folded, correctly rounded
    float q = v * r;
    const float e = __builtin_fmaf(-q, 255.0f, v);
    q = __builtin_fmaf(e, r, q);
    return (q - 0.5f) * 2.0f;                            // (q - 0.5) / 0.5: both exact scalings of the rounded difference
}

struct __attribute__((packed, aligned(4))) Bytes12 { unsigned a, b, c; };

struct GatherP {
    const unsigned char* bank;
    const long long* index;
    void* out;
    long long bank_frames, n;
    unsigned plane;          // h * w
};

// The bank frame of output frame i, or -1 (skip) when index[i] is out of range.  Wave-uniform.
__device__ __forceinline__ long long gather_src(const GatherP& p, long long i) {
    const long long f = p.index[i];
    return (f >= 0 && f < p.bank_frames) ? f : -1;
}

// ------------------------------------------------------------------------------------------------ float32 NCHW
__global__ __launch_bounds__(GATHER_THREADS) void gather_f32_vec_kernel(GatherP p) {
    const unsigned quads = p.plane / 4;
    const unsigned q0 = blockIdx.x * (GATHER_THREADS * GATHER_UNROLL) + threadIdx.x;
    for (long long i = blockIdx.y; i < p.n; i += gridDim.y) {
        const long long f = gather_src(p, i);
        if (f < 0) continue;
        const unsigned char* src = p.bank + (size_t)f * 3 * p.plane;
        float* dst = (float*)p.out + (size_t)i * 3 * p.plane;
        Bytes12 v[GATHER_UNROLL];
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; ++u) {
            const unsigned q = q0 + u * GATHER_THREADS;
            if (q < quads) v[u] = *(const Bytes12*)(src + (size_t)q * 12);
        }
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; ++u) {
            const unsigned q = q0 + u * GATHER_THREADS;
            if (q >= quads) continue;
            // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian words a, b, c)
            const unsigned a = v[u].a, b = v[u].b, c = v[u].c;
            const f32x4 red = {gather_norm((float)(a & 255u)), gather_norm((float)(a >> 24)), gather_norm((float)((b >> 16) & 255u)),
                               gather_norm((float)((c >> 8) & 255u))};
            const f32x4 grn = {gather_norm((float)((a >> 8) & 255u)), gather_norm((float)(b & 255u)), gather_norm((float)(b >> 24)),
                               gather_norm((float)((c >> 16) & 255u))};
            const f32x4 blu = {gather_norm((float)((a >> 16) & 255u)), gather_norm((float)((b >> 8) & 255u)), gather_norm((float)(c & 255u)),
                               gather_norm((float)(c >> 24))};
            float* o = dst + (size_t)q * 4;
            *(f32x4*)o = red;
            *(f32x4*)(o + p.plane) = grn;
            *(f32x4*)(o + 2 * (size_t)p.plane) = blu;
        }
    }
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_f32_plain_kernel(GatherP p) {
    const unsigned q = blockIdx.x * GATHER_THREADS + threadIdx.x;      // pixel
    if (q >= p.plane) return;
    for (long long i = blockIdx.y; i < p.n; i += gridDim.y) {
        const long long f = gather_src(p, i);
        if (f < 0) continue;
        const unsigned char* src = p.bank + (size_t)f * 3 * p.plane + (size_t)q * 3;
        float* o = (float*)p.out + (size_t)i * 3 * p.plane + q;
        const unsigned r = src[0], g = src[1], b = src[2];
        o[0] = gather_norm((float)r);
        o[p.plane] = gather_norm((float)g);
        o[2 * (size_t)p.plane] = gather_norm((float)b);
    }
}

// ------------------------------------------------------------------------------------------------ uint8 NHWC (a copy)
__global__ __launch_bounds__(GATHER_THREADS) void gather_u8_vec_kernel(GatherP p) {
    const unsigned chunks = 3 * p.plane / 16;                          // plane <= 2^27: no overflow
    const unsigned c0 = blockIdx.x * (GATHER_THREADS * GATHER_UNROLL) + threadIdx.x;
    for (long long i = blockIdx.y; i < p.n; i += gridDim.y) {
        const long long f = gather_src(p, i);
        if (f < 0) continue;
        const u32x4* src = (const u32x4*)(p.bank + (size_t)f * 3 * p.plane);
        u32x4* dst = (u32x4*)((unsigned char*)p.out + (size_t)i * 3 * p.plane);
        u32x4 v[GATHER_UNROLL];
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; ++u) {
            const unsigned c = c0 + u * GATHER_THREADS;
            if (c < chunks) v[u] = src[c];
        }
#pragma unroll
        for (int u = 0; u < GATHER_UNROLL; ++u) {
            const unsigned c = c0 + u * GATHER_THREADS;
            if (c < chunks) dst[c] = v[u];
        }
    }
}

__global__ __launch_bounds__(GATHER_THREADS) void gather_u8_plain_kernel(GatherP p) {
    const size_t bytes = (size_t)3 * p.plane;
    const size_t k = (size_t)blockIdx.x * GATHER_THREADS + threadIdx.x;
    if (k >= bytes) return;
    for (long long i = blockIdx.y; i < p.n; i += gridDim.y) {
        const long long f = gather_src(p, i);
        if (f < 0) continue;
        ((unsigned char*)p.out)[(size_t)i * bytes + k] = p.bank[(size_t)f * bytes + k];
    }
}

}  // namespace

int vad_gather_frames_u8(const unsigned char* bank, long long bank_frames, const long long* index, long long n, int h, int w,
                         int out_format, void* out, void* stream) {
    VAD_REQUIRE(bank != nullptr, "gather_frames: bank is NULL");
    VAD_REQUIRE(index != nullptr, "gather_frames: index is NULL");
    VAD_REQUIRE(out != nullptr, "gather_frames: out is NULL");
    VAD_REQUIRE(n >= 0, "gather_frames: n must be >= 0, got %lld", n);
    VAD_REQUIRE(h > 0 && w > 0, "gather_frames: h and w must be positive, got %d x %d", h, w);
    VAD_REQUIRE(bank_frames > 0, "gather_frames: bank_frames must be positive, got %lld", bank_frames);
    VAD_REQUIRE(out_format == VAD_X_F32_NCHW || out_format == VAD_X_U8_NHWC,
                "gather_frames: out_format must be VAD_X_F32_NCHW (%d) or VAD_X_U8_NHWC (%d), got %d", VAD_X_F32_NCHW, VAD_X_U8_NHWC, out_format);
    const bool f32 = out_format == VAD_X_F32_NCHW;
    VAD_REQUIRE(!f32 || (uintptr_t)out % 4 == 0, "gather_frames: a float32 out must be 4-byte aligned");
    VAD_REQUIRE(((uintptr_t)index & 7) == 0, "gather_frames: index must be 8-byte aligned");
    // in-frame offsets are 32-bit: an output frame stays below 2^31 bytes
    VAD_REQUIRE((long long)h * w <= (1ll << 27), "gather_frames: h * w must not exceed 2^27 pixels, got %d x %d", h, w);
    if (n == 0) return VAD_OK;

    const unsigned plane = (unsigned)h * (unsigned)w;
    GatherP p{bank, index, out, bank_frames, n, plane};
    const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
    const hipStream_t s = (hipStream_t)stream;
    if (f32) {
        if (plane % 4 == 0 && (uintptr_t)bank % 4 == 0 && (uintptr_t)out % 16 == 0) {
            const unsigned per = GATHER_THREADS * GATHER_UNROLL, quads = plane / 4;
            hipLaunchKernelGGL(gather_f32_vec_kernel, dim3((quads + per - 1) / per, gy), dim3(GATHER_THREADS), 0, s, p);
        } else {
            hipLaunchKernelGGL(gather_f32_plain_kernel, dim3((plane + GATHER_THREADS - 1) / GATHER_THREADS, gy), dim3(GATHER_THREADS), 0, s, p);
        }
    } else {
        const size_t bytes = (size_t)3 * plane;
        if (bytes % 16 == 0 && (uintptr_t)bank % 16 == 0 && (uintptr_t)out % 16 == 0) {
            const unsigned per = GATHER_THREADS * GATHER_UNROLL, chunks = (unsigned)(bytes / 16);
            hipLaunchKernelGGL(gather_u8_vec_kernel, dim3((chunks + per - 1) / per, gy), dim3(GATHER_THREADS), 0, s, p);
        } else {
            hipLaunchKernelGGL(gather_u8_plain_kernel, dim3((unsigned)((bytes + GATHER_THREADS - 1) / GATHER_THREADS), gy), dim3(GATHER_THREADS), 0, s, p);
        }
    }
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
