// Recurrent-state plumbing of the stateful video path (include/vad_hip.h: vad_vid_score_s, vad_convlstm_seq).
//
// The kernels keep h and c as zero-padded NHWC [frames][pixels][cpad]; the reference's ConvLSTM.forward takes and returns
// NCHW tensors of the real width (models/video_autoencoder.py:127-166).  The two converters below move 32 pixels x 32
// channels at a time through LDS so that BOTH sides are accessed along their contiguous axis (pixels on the NCHW side,
// channels on the NHWC side); the tile is padded to 33 columns, so the transposed read walks 32 different banks.  Import
// writes exact zeros into the padded channels, export drops them.  vad_state_store gathers the last h of every layer's
// sequence and its cell state into the caller's blob in one launch.  HBM-bound copies of a few KB per stream.
#include <hip/hip_runtime.h>

#include "vad_common.h"
#include "vad_layout.h"

namespace {

// out[n][q][cpad] = in[n][ch][q] (ch < c), 0 (c <= ch < cpad).  grid (pixel tiles, channel tiles, frames), 32 x 8 threads.
__global__ __launch_bounds__(256) void nchw_to_nhwc_tile_kernel(const float* __restrict__ in, float* __restrict__ out, int plane, int c, int cpad) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int q0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const size_t n = blockIdx.z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ch = c0 + ty + 8 * k, q = q0 + tx;
        tile[ty + 8 * k][tx] = (ch < c && q < plane) ? in[(n * c + ch) * plane + q] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + ty + 8 * k, ch = c0 + tx;
        if (q < plane && ch < cpad) out[(n * plane + q) * cpad + ch] = tile[tx][ty + 8 * k];
    }
}

// out[n][ch][q] = in[n][q][ch] for ch < c (the padded channels are dropped)
__global__ __launch_bounds__(256) void nhwc_to_nchw_tile_kernel(const float* __restrict__ in, float* __restrict__ out, int plane, int c, int cpad) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int q0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const size_t n = blockIdx.z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int q = q0 + ty + 8 * k, ch = c0 + tx;
        tile[ty + 8 * k][tx] = (q < plane && ch < cpad) ? in[(n * plane + q) * cpad + ch] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ch = c0 + ty + 8 * k, q = q0 + tx;
        if (ch < c && q < plane) out[(n * c + ch) * plane + q] = tile[tx][ty + 8 * k];
    }
}

struct StoreP {
    const float* hs; const float* cs;     // layer 0's h sequence [nc][t][fs] and cell state [nc][fs] in the workspace
    long long hs_ls, cs_ls;               // floats between two layers' buffers
    float* out;                           // row 0 of this launch group in layer 0's h plane of the blob
    long long out_ls, out_c;              // floats between two layers of the blob; from a layer's h plane to its c plane
    int t, fs4, nc;                       // fs4: floats per stream / 4
};

// grid (blocks over one stream's plane, streams, layers): one f32x4 of h and one of c per thread
__global__ __launch_bounds__(256) void state_store_kernel(StoreP p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.fs4) return;
    const size_t n = blockIdx.y, l = blockIdx.z, fs = (size_t)p.fs4 * 4;
    const f32x4 hv = *(const f32x4*)(p.hs + l * p.hs_ls + (n * p.t + (p.t - 1)) * fs + 4 * (size_t)i);
    const f32x4 cv = *(const f32x4*)(p.cs + l * p.cs_ls + n * fs + 4 * (size_t)i);
    float* o = p.out + l * p.out_ls + n * fs + 4 * (size_t)i;
    *(f32x4*)o = hv;
    *(f32x4*)(o + p.out_c) = cv;
}

int launch_tile(bool to_nhwc, const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream, const char* who) {
    VAD_REQUIRE(in && out, "%s: null pointer", who);
    VAD_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && cpad >= c && cpad % 4 == 0, "%s: bad shape n=%lld %dx%d c=%d cpad=%d", who, n, h, w, c, cpad);
    const long long plane = (long long)h * w;
    VAD_REQUIRE(n < 65536 && (plane + 31) / 32 < (1ll << 31) && (cpad + 31) / 32 < 65536, "%s: grid out of range (n=%lld)", who, n);
    const dim3 grid((unsigned)((plane + 31) / 32), (unsigned)((cpad + 31) / 32), (unsigned)n);
    if (to_nhwc) hipLaunchKernelGGL(nchw_to_nhwc_tile_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, (int)plane, c, cpad);
    else hipLaunchKernelGGL(nhwc_to_nchw_tile_kernel, grid, dim3(256), 0, (hipStream_t)stream, in, out, (int)plane, c, cpad);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

}  // namespace

// frames in slices of at most 65535 (gridDim.z)
static int tile_frames(bool to_nhwc, const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream, const char* who) {
    VAD_REQUIRE(n > 0, "%s: no frames", who);
    const size_t fin = (size_t)h * w * (to_nhwc ? c : cpad), fout = (size_t)h * w * (to_nhwc ? cpad : c);
    for (long long f0 = 0; f0 < n; f0 += 65535) {
        const long long m = n - f0 < 65535 ? n - f0 : 65535;
        const int rc = launch_tile(to_nhwc, in ? in + f0 * fin : in, out ? out + f0 * fout : out, m, h, w, c, cpad, stream, who);
        if (rc != VAD_OK) return rc;
    }
    return VAD_OK;
}

extern "C" int vad_nchw_to_nhwc_padded(const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream) {
    return tile_frames(true, in, out, n, h, w, c, cpad, stream, "nchw_to_nhwc_padded");
}
extern "C" int vad_nhwc_padded_to_nchw(const float* in, float* out, long long n, int h, int w, int c, int cpad, void* stream) {
    return tile_frames(false, in, out, n, h, w, c, cpad, stream, "nhwc_padded_to_nchw");
}

extern "C" size_t vad_convlstm_state_floats(int b, int gh, int gw, int hid_p, int layers) {
    if (b <= 0 || gh <= 0 || gw <= 0 || hid_p <= 0 || hid_p % 64 || hid_p > vad_pad_up(VAD_MAX_WIDTH, 64) || layers < 1 || layers > 8) return 0;
    return (size_t)2 * layers * b * gh * gw * hid_p;
}
extern "C" size_t vad_vid_state_floats(int b, int h, int w, int hid, int layers) {
    if (h <= 0 || w <= 0 || h % 16 || w % 16 || !vad_frame_pixels_ok(h, w) || hid <= 0 || hid > VAD_MAX_WIDTH) return 0;   // (no model scores such frames)
    return vad_convlstm_state_floats(b, h / 16, w / 16, vad_pad_up(hid, 64), layers);
}

static int state_args(const char* who, const void* h, const void* c, const void* blob, int layer, int b, int gh, int gw, int hid, int hid_p, int layers) {
    VAD_REQUIRE(h && c && blob, "%s: null pointer", who);
    VAD_REQUIRE(vad_convlstm_state_floats(b, gh, gw, hid_p, layers) != 0, "%s: unsupported state shape b=%d grid=%dx%d hid_p=%d layers=%d", who, b, gh, gw, hid_p, layers);
    VAD_REQUIRE(layer >= 0 && layer < layers, "%s: layer=%d out of range [0,%d)", who, layer, layers);
    VAD_REQUIRE(hid > 0 && hid <= hid_p, "%s: hid=%d does not fit the padded width %d", who, hid, hid_p);
    VAD_REQUIRE(((uintptr_t)blob & 15) == 0, "%s: the state blob must be 16-B aligned", who);
    return VAD_OK;
}

extern "C" int vad_state_import(const float* h_nchw, const float* c_nchw, float* blob, int layer, int b, int gh, int gw, int hid, int hid_p, int layers,
                                void* stream) {
    const int rc = state_args("state_import", h_nchw, c_nchw, blob, layer, b, gh, gw, hid, hid_p, layers);
    if (rc != VAD_OK) return rc;
    const size_t plane = (size_t)b * gh * gw * hid_p;
    float* hp = blob + (size_t)2 * layer * plane;
    const int r1 = tile_frames(true, h_nchw, hp, b, gh, gw, hid, hid_p, stream, "state_import");
    return r1 != VAD_OK ? r1 : tile_frames(true, c_nchw, hp + plane, b, gh, gw, hid, hid_p, stream, "state_import");
}

extern "C" int vad_state_export(const float* blob, float* h_nchw, float* c_nchw, int layer, int b, int gh, int gw, int hid, int hid_p, int layers,
                                void* stream) {
    const int rc = state_args("state_export", h_nchw, c_nchw, blob, layer, b, gh, gw, hid, hid_p, layers);
    if (rc != VAD_OK) return rc;
    const size_t plane = (size_t)b * gh * gw * hid_p;
    const float* hp = blob + (size_t)2 * layer * plane;
    const int r1 = tile_frames(false, hp, h_nchw, b, gh, gw, hid, hid_p, stream, "state_export");
    return r1 != VAD_OK ? r1 : tile_frames(false, hp + plane, c_nchw, b, gh, gw, hid, hid_p, stream, "state_export");
}

// rows [row0, row0 + nc) of every layer of `state` (sized for b streams) <- last h of hs[l] ([nc][t][fs]) and cs[l] ([nc][fs])
int vad_state_store(const float* hs, long long hs_layer_stride, const float* cs, long long cs_layer_stride, float* state, long long b, long long row0,
                    int nc, int t, long long fs, int layers, void* stream) {
    VAD_REQUIRE(hs && cs && state && nc > 0 && t > 0 && fs > 0 && fs % 4 == 0 && layers >= 1 && row0 >= 0 && row0 + nc <= b, "state_store: bad arguments");
    VAD_REQUIRE(nc < 65536 && fs / 4 < (1ll << 31), "state_store: grid out of range");
    StoreP p{hs, cs, hs_layer_stride, cs_layer_stride, state + row0 * fs, 2 * b * fs, b * fs, t, (int)(fs / 4), nc};
    hipLaunchKernelGGL(state_store_kernel, dim3((unsigned)((p.fs4 + 255) / 256), (unsigned)nc, (unsigned)layers), dim3(256), 0, (hipStream_t)stream, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
