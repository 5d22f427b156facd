// Training-step kernels (reference train_video.py:44-65), gfx950, exact fp32.
//
// The reference's step is stock autograd over models/video_autoencoder.py in train() mode.  Here the same arithmetic
// is stated as explicit kernels on NHWC activations:
//   * train-mode BatchNorm2d (batch statistics over N*H*W, eps 1e-5, momentum 0.1, unbiased running variance):
//     per-channel sums with wave/LDS reductions and a fixed-order fp64 finalize, then ONE fused
//     normalise + activation (+ MaxPool2d) pass; backward in two passes (route the pooled gradient, apply act',
//     accumulate sum(dz), sum(dz*xhat); then dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)))
//   * conv / convT weight gradients as one MFMA GEMM (M = input channels, N = output channels, K = pixels) with a
//     deterministic split-K (partials + fixed-order reduce straight into the torch OIHW / IOHW layouts): csrc/wgrad.hip
//   * conv data gradients reuse the forward implicit-GEMM kernels on re-packed (rotated / transposed) weights;
//     convT data gradients are a 1x1 GEMM over the space-to-depth view that the BatchNorm backward writes directly
//   * ConvLSTM gate non-linearities + state update, forward and backward (BPTT), as pointwise kernels
//   * ConvTranspose2d(32->3) + Tanh + MSELoss forward AND backward in one pass over the last activation
//   * Adam with L2 weight decay folded into the gradient (torch.optim.Adam semantics) over ONE flat parameter buffer.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "vad_common.h"

namespace {

__device__ __forceinline__ long long view_frame(int n, int t, int b) { return t > 0 ? (long long)(n % t) * b + n / t : n; }

// Reduce two per-thread float4 channel accumulators over the pixel rows of a 256-thread block; thread = (row, c4).
__device__ __forceinline__ void block_chan_reduce(f32x4 s0, f32x4 s1, int c, float* dst /*[2][c]*/) {
    __shared__ f32x4 red[2][256];
    const int tid = threadIdx.x, cg = c >> 2, rows = 256 / cg;
    red[0][tid] = s0;
    red[1][tid] = s1;
    __syncthreads();
    if (tid < cg) {
        f32x4 a = red[0][tid], b = red[1][tid];
        for (int r = 1; r < rows; ++r) { a += red[0][r * cg + tid]; b += red[1][r * cg + tid]; }
        *(f32x4*)&dst[4 * tid] = a;
        *(f32x4*)&dst[c + 4 * tid] = b;
    }
}

// ------------------------------------------------------------------------------------------------ channel sums
// ws[block][0][c] = sum over the block's pixels of (v - pivot[c]), ws[block][1][c] = sum of (v - pivot[c])^2.
// pivot (nullable = 0) is a per-channel shift applied BEFORE squaring: BatchNorm statistics pass the channel's first
// sample, so the variance is not formed as E[x^2] - mean^2 of the raw values (that cancels catastrophically in fp32 when
// |mean| >> std: measured 5e-5 relative error in 1/std, enough to flip ReLU decisions in the layers that follow).
template <typename T>
__global__ __launch_bounds__(256) void chan_sums_kernel(const T* y, long long npix, int c, long long chunk, const float* pivot,
                                                        float* ws) {
    const int tid = threadIdx.x, cg = c >> 2, rows = 256 / cg, row = tid / cg, c4 = tid - row * cg;
    const long long p0 = (long long)blockIdx.x * chunk, p1 = (p0 + chunk < npix) ? p0 + chunk : npix;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (row < rows) {
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (pivot) pv = *(const f32x4*)&pivot[4 * c4];
        // four loads in flight per thread (same accumulation order): one at a time, a CU's 2048 threads keep 32 KB in flight and
        // the pass ran at 3.8 TB/s
        long long p = p0 + row;
        for (; p + 3 * rows < p1; p += 4 * rows) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = vad_io4<T>::ld(&y[(p + (long long)u * rows) * c + 4 * c4]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 d = v[u] - pv;
                s0 += d;
                s1 += d * d;
            }
        }
        for (; p < p1; p += rows) {
            const f32x4 v = vad_io4<T>::ld(&y[p * c + 4 * c4]) - pv;
            s0 += v;
            s1 += v * v;
        }
    }
    block_chan_reduce(s0, s1, c, ws + (size_t)blockIdx.x * 2 * c);
}

// mode 0: BatchNorm statistics -> stats[0][c] = mean, stats[1][c] = 1/sqrt(var_biased + eps); running stats updated
//         like torch (momentum; unbiased variance) when given
// mode 1: BatchNorm backward sums -> dgamma = sum(dz*xhat), dbeta = sum(dz), stats = {sum(dz)/M, sum(dz*xhat)/M}
// mode 2: plain sums -> dbeta[c] = sum (bias gradients)
__global__ __launch_bounds__(256) void chan_finalize_kernel(const float* ws, int nblocks, int c, double count, int mode,
                                                            float eps, float momentum, float* stats, float* running_mean,
                                                            float* running_var, float* dgamma, float* dbeta, const float* pivot) {
    // one work-group per channel: thread t adds partial blocks t, t+256, ... in fp64, then a fixed-shape tree over the
    // 256 threads (the result depends only on the data and the block count, never on scheduling)
    __shared__ double rs[256], rq[256];
    const int ch = blockIdx.x, tid = threadIdx.x;
    double s = 0.0, q = 0.0;
    for (int b = tid; b < nblocks; b += 256) {
        s += (double)ws[(size_t)b * 2 * c + ch];
        q += (double)ws[(size_t)b * 2 * c + c + ch];
    }
    rs[tid] = s;
    rq[tid] = q;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { rs[tid] += rs[tid + o]; rq[tid] += rq[tid + o]; }
        __syncthreads();
    }
    if (tid != 0) return;
    s = rs[0];
    q = rq[0];
    if (mode == 0) {
        const double sm = s / count;                     // mean of the shifted values
        const double mean = (pivot ? (double)pivot[ch] : 0.0) + sm;
        double var = q / count - sm * sm;
        if (var < 0.0) var = 0.0;
        stats[ch] = (float)mean;
        stats[c + ch] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
            const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            running_mean[ch] = (float)((1.0 - momentum) * (double)running_mean[ch] + momentum * mean);
            running_var[ch] = (float)((1.0 - momentum) * (double)running_var[ch] + momentum * unb);
        }
    } else if (mode == 1) {
        dbeta[ch] = (float)s;
        dgamma[ch] = (float)q;
        stats[ch] = (float)(s / count);
        stats[c + ch] = (float)(q / count);
    } else {
        dbeta[ch] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ BatchNorm forward
struct BnFwdP {     // y / out: fp32 or bf16 (the kernel's storage type)
    const void* y; const float* stats; const float* gamma; const float* beta;
    void* out; long long out_fs; int out_ps, t, b;
    int n, h, w, c, act, pool;
    long long total;      // n * oh * ow * c/4
};

// xhat and the BatchNorm output with every operation rounded on its own (no fma contraction): forward, backward pass A and
// backward pass B must take bit-identical branch decisions whatever code the compiler generates around them.
__device__ __forceinline__ float bn_xhat(float y, float mean, float invstd) { return __fmul_rn(__fsub_rn(y, mean), invstd); }
__device__ __forceinline__ float bn_value(float xhat, float gamma, float beta) { return __fadd_rn(__fmul_rn(xhat, gamma), beta); }

__device__ __forceinline__ f32x4 bn_apply(f32x4 y, f32x4 mean, f32x4 invstd, f32x4 gamma, f32x4 beta, int act) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = vad_act(bn_value(bn_xhat(y[e], mean[e], invstd[e]), gamma[e], beta[e]), act);
    return v;
}

// POOL / ACT are compile-time (host dispatch): with run-time flags every element paid the selects of both activations and the
// window loop's guards - VALU work these passes can no longer hide once the tensors are bf16.
template <typename T, int POOL, int ACT>
__global__ __launch_bounds__(256) void bn_act_pool_fwd_kernel(BnFwdP p) {
    typedef vad_io4<T> io;
    const int cg = p.c >> 2, oh = POOL ? p.h / 2 : p.h, ow = POOL ? p.w / 2 : p.w;
    // (32-bit index arithmetic, host-checked: three 64-bit divisions per item cost more than the item's memory traffic once
    // the tensors are bf16)
    const unsigned total = (unsigned)p.total, ucg = (unsigned)cg, uow = (unsigned)ow, uoh = (unsigned)oh;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned pix = idx / ucg, t_ = pix / uow, un = t_ / uoh;
        const int c4 = (int)(idx - pix * ucg);
        const int x = (int)(pix - t_ * uow);
        const int y = (int)(t_ - un * uoh);
        const int n = (int)un;
        const f32x4 mean = *(const f32x4*)&p.stats[4 * c4], invstd = *(const f32x4*)&p.stats[p.c + 4 * c4];
        const f32x4 gamma = *(const f32x4*)&p.gamma[4 * c4], beta = *(const f32x4*)&p.beta[4 * c4];
        const T* src = (const T*)p.y + (size_t)n * p.h * p.w * p.c + 4 * c4;
        f32x4 v;
        if constexpr (POOL) {
            const size_t o = ((size_t)(2 * y) * p.w + 2 * x) * p.c;
            v = bn_apply(io::ld(&src[o]), mean, invstd, gamma, beta, ACT);
            const f32x4 v1 = bn_apply(io::ld(&src[o + p.c]), mean, invstd, gamma, beta, ACT);
            const f32x4 v2 = bn_apply(io::ld(&src[o + (size_t)p.w * p.c]), mean, invstd, gamma, beta, ACT);
            const f32x4 v3 = bn_apply(io::ld(&src[o + (size_t)p.w * p.c + p.c]), mean, invstd, gamma, beta, ACT);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = vad_vmax4(v[e], v1[e], v2[e], v3[e]);
        } else {
            v = bn_apply(io::ld(&src[((size_t)y * p.w + x) * p.c]), mean, invstd, gamma, beta, ACT);
        }
        io::st((T*)p.out + view_frame(n, p.t, p.b) * p.out_fs + ((size_t)y * ow + x) * p.out_ps + 4 * c4, v);
    }
}

// bf16 tensors, EIGHT channels per thread (16-byte accesses: twice the bytes in flight per wave, half the index arithmetic);
// every element goes through the same bn_apply as above: identical results.  c % 8 == 0, strides % 8 == 0 (host-checked).
__device__ __forceinline__ void bf16_ld8(const vad_bf16* p, f32x4& a, f32x4& b) {
    const u32x4 r = *(const u32x4*)p;
    a = f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16), __uint_as_float(r[1] & 0xffff0000u)};
    b = f32x4{__uint_as_float(r[2] << 16), __uint_as_float(r[2] & 0xffff0000u), __uint_as_float(r[3] << 16), __uint_as_float(r[3] & 0xffff0000u)};
}
__device__ __forceinline__ void bf16_st8(vad_bf16* p, f32x4 a, f32x4 b) {
    *(u32x4*)p = u32x4{vad_pack_bf16(a[0], a[1]), vad_pack_bf16(a[2], a[3]), vad_pack_bf16(b[0], b[1]), vad_pack_bf16(b[2], b[3])};
}
template <int POOL, int ACT>
__global__ __launch_bounds__(256) void bn_act_pool_fwd8_kernel(BnFwdP p) {
    const int cg = p.c >> 3, oh = POOL ? p.h / 2 : p.h, ow = POOL ? p.w / 2 : p.w;
    const unsigned total = (unsigned)(p.total >> 1), ucg = (unsigned)cg, uow = (unsigned)ow, uoh = (unsigned)oh;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned pix = idx / ucg, t_ = pix / uow, un = t_ / uoh;
        const int c8 = (int)(idx - pix * ucg);
        const int x = (int)(pix - t_ * uow);
        const int y = (int)(t_ - un * uoh);
        const int n = (int)un;
        f32x4 mean[2], invstd[2], gamma[2], beta[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            mean[hf] = *(const f32x4*)&p.stats[8 * c8 + 4 * hf]; invstd[hf] = *(const f32x4*)&p.stats[p.c + 8 * c8 + 4 * hf];
            gamma[hf] = *(const f32x4*)&p.gamma[8 * c8 + 4 * hf]; beta[hf] = *(const f32x4*)&p.beta[8 * c8 + 4 * hf];
        }
        const vad_bf16* src = (const vad_bf16*)p.y + (size_t)n * p.h * p.w * p.c + 8 * c8;
        f32x4 v[2];
        if constexpr (POOL) {
            const size_t o = ((size_t)(2 * y) * p.w + 2 * x) * p.c;
            f32x4 w0[2], w1[2], w2[2], w3[2];
            bf16_ld8(&src[o], w0[0], w0[1]);
            bf16_ld8(&src[o + p.c], w1[0], w1[1]);
            bf16_ld8(&src[o + (size_t)p.w * p.c], w2[0], w2[1]);
            bf16_ld8(&src[o + (size_t)p.w * p.c + p.c], w3[0], w3[1]);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                v[hf] = bn_apply(w0[hf], mean[hf], invstd[hf], gamma[hf], beta[hf], ACT);
                const f32x4 v1 = bn_apply(w1[hf], mean[hf], invstd[hf], gamma[hf], beta[hf], ACT);
                const f32x4 v2 = bn_apply(w2[hf], mean[hf], invstd[hf], gamma[hf], beta[hf], ACT);
                const f32x4 v3 = bn_apply(w3[hf], mean[hf], invstd[hf], gamma[hf], beta[hf], ACT);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[hf][e] = vad_vmax4(v[hf][e], v1[e], v2[e], v3[e]);
            }
        } else {
            f32x4 w0[2];
            bf16_ld8(&src[((size_t)y * p.w + x) * p.c], w0[0], w0[1]);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) v[hf] = bn_apply(w0[hf], mean[hf], invstd[hf], gamma[hf], beta[hf], ACT);
        }
        bf16_st8((vad_bf16*)p.out + view_frame(n, p.t, p.b) * p.out_fs + ((size_t)y * ow + x) * p.out_ps + 8 * c8, v[0], v[1]);
    }
}

// ------------------------------------------------------------------------------------------------ BatchNorm backward
struct BnBwdP {     // y / dout / dy: fp32 or bf16 (the kernels' storage type)
    const void* y; const float* stats; const float* gamma; const float* beta;
    const void* dout; long long dout_fs; int dout_ps, t, b;
    float* ws;            // pass A: partial sums
    const float* k;       // pass B: {sum(dz)/M, sum(dz*xhat)/M}
    void* dy;             // pass B: gradient of the conv output, dense NHWC or space-to-depth
    int s2d;
    int n, h, w, c, act, pool;
    long long opix, chunk;   // pooled-resolution pixels (n*oh*ow), per block
    unsigned char* dec;   // debug (nullable): [opix][c] bytes, bits 0-1 = pooling argmax (window scan order), bit 2 = value > 0
    unsigned char* codes; // nullable: the same bytes as an OUTPUT of pass A (the routed first-layer weight gradient reads them)
};

__device__ __forceinline__ float act_grad(float v, int act) {
    if (act == VAD_ACT_LEAKY) return v > 0.f ? 1.f : 0.2f;
    if (act == VAD_ACT_RELU) return v > 0.f ? 1.f : 0.f;
    return 1.f;
}

// The routed gradient of one (pooled) output element: which window element receives it (first maximum in window scan
// order, like torch), its xhat, and dz = d(out) * act'(value).  Shared by both passes.
struct Routed { int am; float xh, gz, v; };
__device__ __forceinline__ Routed bn_route(const float y4[4], int nwin, float mean, float invstd, float gamma, float beta, float g, int act) {
    Routed r;
    float xh[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nwin) { xh[k] = bn_xhat(y4[k], mean, invstd); v[k] = vad_act(bn_value(xh[k], gamma, beta), act); }
    r.am = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < nwin && v[k] > v[r.am]) r.am = k;
    r.xh = xh[r.am];
    r.v = v[r.am];
    r.gz = g * act_grad(r.v, act);
    return r;
}

// pass A: per-channel partial sums of dz and dz*xhat (dz itself is never stored; pass B re-derives it)
template <typename T, int POOL, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(BnBwdP p) {
    typedef vad_io4<T> io;
    const T* py = (const T*)p.y;
    const T* pdout = (const T*)p.dout;
    const int tid = threadIdx.x, cg = p.c >> 2, rows = 256 / cg, row = tid / cg, c4 = tid - row * cg;
    const int oh = POOL ? p.h / 2 : p.h, ow = POOL ? p.w / 2 : p.w; constexpr int nwin = POOL ? 4 : 1;
    const long long p0 = (long long)blockIdx.x * p.chunk, p1 = (p0 + p.chunk < p.opix) ? p0 + p.chunk : p.opix;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (row < rows) {
        const f32x4 mean = *(const f32x4*)&p.stats[4 * c4], invstd = *(const f32x4*)&p.stats[p.c + 4 * c4];
        const f32x4 gamma = *(const f32x4*)&p.gamma[4 * c4], beta = *(const f32x4*)&p.beta[4 * c4];
        auto fetch = [&](long long q, f32x4& g, f32x4 (&yv)[4]) {
            const unsigned uq = (unsigned)q, t_ = uq / (unsigned)ow, un = t_ / (unsigned)oh;       // (opix < 2^31: host-checked)
            const int x = (int)(uq - t_ * (unsigned)ow), y = (int)(t_ - un * (unsigned)oh), n = (int)un;
            g = io::ld(&pdout[view_frame(n, p.t, p.b) * p.dout_fs + ((size_t)y * ow + x) * p.dout_ps + 4 * c4]);
            const size_t o0 = (size_t)n * p.h * p.w * p.c + 4 * c4 + (POOL ? ((size_t)(2 * y) * p.w + 2 * x) : ((size_t)y * p.w + x)) * p.c;
            yv[0] = io::ld(&py[o0]);
            if constexpr (POOL) { yv[1] = io::ld(&py[o0 + p.c]); yv[2] = io::ld(&py[o0 + (size_t)p.w * p.c]); yv[3] = io::ld(&py[o0 + (size_t)p.w * p.c + p.c]); }
        };
        auto add = [&](long long q, const f32x4& g, const f32x4 (&yv)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y4[4] = {yv[0][e], yv[1][e], yv[2][e], yv[3][e]};
                const Routed r = bn_route(y4, nwin, mean[e], invstd[e], gamma[e], beta[e], g[e], ACT);
                if (p.dec) p.dec[q * p.c + 4 * c4 + e] = (unsigned char)(r.am | (r.v > 0.f ? 4 : 0));
                if (p.codes) p.codes[q * p.c + 4 * c4 + e] = (unsigned char)(r.am | (r.v > 0.f ? 4 : 0));
                s0[e] += r.gz;
                s1[e] += r.gz * r.xh;
            }
        };
        // (two pixels per trip with all ten loads first measured SLOWER - 1.61 -> 2.0 ms per bf16 training step: the second
        // register set costs occupancy, and the pass is bound by its ~230 VALU instructions per pixel quad as much as by memory)
        for (long long q = p0 + row; q < p1; q += rows) {
            f32x4 ga, ya[4];
            fetch(q, ga, ya);
            add(q, ga, ya);
        }
    }
    block_chan_reduce(s0, s1, p.c, p.ws + (size_t)blockIdx.x * 2 * p.c);
}

// pass B: dy = gamma * invstd * (dz - k1 - xhat * k2) for every element of the window (dz = 0 off the routed element);
// s2d writes the space-to-depth view [n][h/2][w/2][4][c] (the operand layout of the transposed convolution's gradients)
template <typename T, int POOL, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdP p) {
    typedef vad_io4<T> io;
    const T* py = (const T*)p.y;
    const T* pdout = (const T*)p.dout;
    T* pdy = (T*)p.dy;
    const int cg = p.c >> 2, oh = POOL ? p.h / 2 : p.h, ow = POOL ? p.w / 2 : p.w; constexpr int nwin = POOL ? 4 : 1;
    const unsigned total = (unsigned)(p.opix * cg), ucg = (unsigned)cg;               // (< 2^31: host-checked)
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned q = idx / ucg, t_ = q / (unsigned)ow, un = t_ / (unsigned)oh;
        const int c4 = (int)(idx - q * ucg);
        const int x = (int)(q - t_ * (unsigned)ow), y = (int)(t_ - un * (unsigned)oh), n = (int)un;
        const f32x4 mean = *(const f32x4*)&p.stats[4 * c4], invstd = *(const f32x4*)&p.stats[p.c + 4 * c4];
        const f32x4 gamma = *(const f32x4*)&p.gamma[4 * c4], beta = *(const f32x4*)&p.beta[4 * c4];
        const f32x4 k1 = *(const f32x4*)&p.k[4 * c4], k2 = *(const f32x4*)&p.k[p.c + 4 * c4];
        const f32x4 g = io::ld(&pdout[view_frame(n, p.t, p.b) * p.dout_fs + ((size_t)y * ow + x) * p.dout_ps + 4 * c4]);
        const size_t fb = (size_t)n * p.h * p.w * p.c + 4 * c4;
        const size_t o0 = fb + (POOL ? ((size_t)(2 * y) * p.w + 2 * x) : ((size_t)y * p.w + x)) * p.c;
        const size_t off[4] = {o0, o0 + p.c, o0 + (size_t)p.w * p.c, o0 + (size_t)p.w * p.c + p.c};
        f32x4 yv[4], out[4];
        yv[0] = io::ld(&py[off[0]]);
        if constexpr (POOL) { yv[1] = io::ld(&py[off[1]]); yv[2] = io::ld(&py[off[2]]); yv[3] = io::ld(&py[off[3]]); }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float y4[4] = {yv[0][e], yv[1][e], yv[2][e], yv[3][e]};
            const Routed r = bn_route(y4, nwin, mean[e], invstd[e], gamma[e], beta[e], g[e], ACT);
            const float sc = gamma[e] * invstd[e];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nwin) {
                    const float xh = bn_xhat(y4[k], mean[e], invstd[e]);
                    out[k][e] = sc * ((k == r.am ? r.gz : 0.f) - k1[e] - xh * k2[e]);
                }
        }
        if (p.s2d) {          // no-pool layers only (checked on the host): pixel (y, x) of an h x w map
            const size_t o = (((size_t)n * (p.h / 2) + y / 2) * (p.w / 2) + x / 2) * 4 * p.c + ((y & 1) * 2 + (x & 1)) * p.c + 4 * c4;
            io::st(&pdy[o], out[0]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nwin) io::st(&pdy[off[k]], out[k]);
        }
    }
}

// pass B on bf16 tensors, eight channels per thread (see bn_act_pool_fwd8_kernel): the same bn_route / expressions per element
template <int POOL, int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply8_kernel(BnBwdP p) {
    const vad_bf16* py = (const vad_bf16*)p.y;
    const vad_bf16* pdout = (const vad_bf16*)p.dout;
    vad_bf16* pdy = (vad_bf16*)p.dy;
    const int cg = p.c >> 3, oh = POOL ? p.h / 2 : p.h, ow = POOL ? p.w / 2 : p.w; constexpr int nwin = POOL ? 4 : 1;
    const unsigned total = (unsigned)(p.opix * cg), ucg = (unsigned)cg;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < total; idx += gridDim.x * 256u) {
        const unsigned q = idx / ucg, t_ = q / (unsigned)ow, un = t_ / (unsigned)oh;
        const int c8 = (int)(idx - q * ucg);
        const int x = (int)(q - t_ * (unsigned)ow), y = (int)(t_ - un * (unsigned)oh), n = (int)un;
        f32x4 g[2];
        bf16_ld8(&pdout[view_frame(n, p.t, p.b) * p.dout_fs + ((size_t)y * ow + x) * p.dout_ps + 8 * c8], g[0], g[1]);
        const size_t fb = (size_t)n * p.h * p.w * p.c + 8 * c8;
        const size_t o0 = fb + (POOL ? ((size_t)(2 * y) * p.w + 2 * x) : ((size_t)y * p.w + x)) * p.c;
        const size_t off[4] = {o0, o0 + p.c, o0 + (size_t)p.w * p.c, o0 + (size_t)p.w * p.c + p.c};
        f32x4 yv[4][2], out[4][2];
        bf16_ld8(&py[off[0]], yv[0][0], yv[0][1]);
        if constexpr (POOL) { bf16_ld8(&py[off[1]], yv[1][0], yv[1][1]); bf16_ld8(&py[off[2]], yv[2][0], yv[2][1]); bf16_ld8(&py[off[3]], yv[3][0], yv[3][1]); }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int c4 = 2 * c8 + hf;
            const f32x4 mean = *(const f32x4*)&p.stats[4 * c4], invstd = *(const f32x4*)&p.stats[p.c + 4 * c4];
            const f32x4 gamma = *(const f32x4*)&p.gamma[4 * c4], beta = *(const f32x4*)&p.beta[4 * c4];
            const f32x4 k1 = *(const f32x4*)&p.k[4 * c4], k2 = *(const f32x4*)&p.k[p.c + 4 * c4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y4[4] = {yv[0][hf][e], yv[1][hf][e], yv[2][hf][e], yv[3][hf][e]};
                const Routed r = bn_route(y4, nwin, mean[e], invstd[e], gamma[e], beta[e], g[hf][e], ACT);
                const float sc = gamma[e] * invstd[e];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nwin) {
                        const float xh = bn_xhat(y4[k], mean[e], invstd[e]);
                        out[k][hf][e] = sc * ((k == r.am ? r.gz : 0.f) - k1[e] - xh * k2[e]);
                    }
            }
        }
        if (p.s2d) {          // no-pool layers only (checked on the host): pixel (y, x) of an h x w map
            const size_t o = (((size_t)n * (p.h / 2) + y / 2) * (p.w / 2) + x / 2) * 4 * p.c + ((y & 1) * 2 + (x & 1)) * p.c + 8 * c8;
            bf16_st8(&pdy[o], out[0][0], out[0][1]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nwin) bf16_st8(&pdy[off[k]], out[k][0], out[k][1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ ConvLSTM pointwise
struct LstmFwdP {   // z / h1 / h2: fp32 or bf16 (the kernel's storage type); the cell state is always fp32
    void* z;                  // [npix][4*hid]: pre-activations in, activated gates (i, f, g, o) out
    const float* c_prev;      // [npix][hid] or null (zeros)
    float* c_out;             // [npix][hid]
    void* h1; long long h1_fs; int h1_ps;      // destination 1 of h (frame b, pixel, channel) or null
    void* h2; long long h2_fs; int h2_ps;      // destination 2 or null
    int hw, hid;
    long long total;          // nb * hw * hid/4
};

template <typename T>
__global__ __launch_bounds__(256) void lstm_gates_fwd_kernel(LstmFwdP p) {
    typedef vad_io4<T> io;
    const int hg = p.hid >> 2;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += (long long)gridDim.x * 256) {
        const int j4 = (int)(idx % hg);
        const long long pix = idx / hg;
        T* zz = (T*)p.z + pix * 4 * p.hid + 4 * j4;
        f32x4 gi = io::ld(&zz[0]), gf = io::ld(&zz[p.hid]), gg = io::ld(&zz[2 * p.hid]), go = io::ld(&zz[3 * p.hid]);
        f32x4 cp = {0.f, 0.f, 0.f, 0.f};
        if (p.c_prev) cp = *(const f32x4*)&p.c_prev[pix * p.hid + 4 * j4];
        f32x4 cn, hn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // (bf16 storage: the state update uses the gate values AS STORED, the ones the backward will read)
            gi[e] = io::round(vad_sigmoid(gi[e])); gf[e] = io::round(vad_sigmoid(gf[e])); gg[e] = io::round(vad_tanh(gg[e])); go[e] = io::round(vad_sigmoid(go[e]));
            cn[e] = gf[e] * cp[e] + gi[e] * gg[e];
            hn[e] = go[e] * vad_tanh(cn[e]);
        }
        io::st(&zz[0], gi); io::st(&zz[p.hid], gf); io::st(&zz[2 * p.hid], gg); io::st(&zz[3 * p.hid], go);
        *(f32x4*)&p.c_out[pix * p.hid + 4 * j4] = cn;
        const long long b = pix / p.hw, q = pix - b * p.hw;
        if (p.h1) io::st((T*)p.h1 + b * p.h1_fs + q * p.h1_ps + 4 * j4, hn);
        if (p.h2) io::st((T*)p.h2 + b * p.h2_fs + q * p.h2_ps + 4 * j4, hn);
    }
}

struct LstmBwdP {   // gates / dh1 / dh2 / dz: fp32 or bf16 (the kernel's storage type); cell states and their gradients fp32
    const void* gates;        // [npix][4*hid] activated
    const float* c_prev;      // null = zeros
    const float* c;           // [npix][hid]
    const void* dh1; long long dh1_fs; int dh1_ps;    // gradient sources for h (either may be null)
    const void* dh2; long long dh2_fs; int dh2_ps;
    const float* dc_next;     // null = zeros
    void* dz;                 // [npix][4*hid]
    float* dc_prev;           // [npix][hid] (may alias dc_next)
    int hw, hid;
    long long total;
};

template <typename T>
__global__ __launch_bounds__(256) void lstm_gates_bwd_kernel(LstmBwdP p) {
    typedef vad_io4<T> io;
    const int hg = p.hid >> 2;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += (long long)gridDim.x * 256) {
        const int j4 = (int)(idx % hg);
        const long long pix = idx / hg, b = pix / p.hw, q = pix - b * p.hw;
        const T* gz = (const T*)p.gates + pix * 4 * p.hid + 4 * j4;
        const f32x4 gi = io::ld(&gz[0]), gf = io::ld(&gz[p.hid]), gg = io::ld(&gz[2 * p.hid]), go = io::ld(&gz[3 * p.hid]);
        const f32x4 c = *(const f32x4*)&p.c[pix * p.hid + 4 * j4];
        f32x4 cp = {0.f, 0.f, 0.f, 0.f}, dh = cp, dcn = cp;
        if (p.c_prev) cp = *(const f32x4*)&p.c_prev[pix * p.hid + 4 * j4];
        if (p.dh1) dh += io::ld((const T*)p.dh1 + b * p.dh1_fs + q * p.dh1_ps + 4 * j4);
        if (p.dh2) dh += io::ld((const T*)p.dh2 + b * p.dh2_fs + q * p.dh2_ps + 4 * j4);
        if (p.dc_next) dcn = *(const f32x4*)&p.dc_next[pix * p.hid + 4 * j4];
        f32x4 di, df, dg, dgo, dcp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float tc = vad_tanh(c[e]);
            const float dc = dcn[e] + dh[e] * go[e] * (1.f - tc * tc);
            dgo[e] = dh[e] * tc * go[e] * (1.f - go[e]);
            di[e] = dc * gg[e] * gi[e] * (1.f - gi[e]);
            df[e] = dc * cp[e] * gf[e] * (1.f - gf[e]);
            dg[e] = dc * gi[e] * (1.f - gg[e] * gg[e]);
            dcp[e] = dc * gf[e];
        }
        T* dzp = (T*)p.dz + pix * 4 * p.hid + 4 * j4;
        io::st(&dzp[0], di); io::st(&dzp[p.hid], df); io::st(&dzp[2 * p.hid], dg); io::st(&dzp[3 * p.hid], dgo);
        *(f32x4*)&p.dc_prev[pix * p.hid + 4 * j4] = dcp;
    }
}

// ------------------------------------------------------------------------------------------------ last layer + loss
// ConvTranspose2d(32->3, k2 s2) + Tanh + MSELoss, forward and backward in one pass (models/video_autoencoder.py:259-260,
// train_video.py:54-55): per input pixel the 4x3 outputs, their squared error against x, d(pre-activation) and the
// gradient with respect to the 32 input channels.  dpre is also written as the 32-column GEMM operand of the weight
// gradient (columns q*3+c, 12..31 zero).
struct To3P {         // in / din / dpre: fp32 or bf16 (the kernel's storage type)
    const void* in; const float* w; const float* bias; const float* x;
    float* recon; void* din; void* dpre; float* loss_parts;
    int n, h, w_;           // input resolution (output is 2h x 2w)
    float gscale;           // 2 / (n * 3 * 2h * 2w)
    long long total;
};

template <typename T>
__global__ __launch_bounds__(256) void convt_to3_mse_kernel(To3P p) {
    typedef vad_io4<T> io;
    __shared__ float ws[32 * 12], bs[3], red[4];
    for (int i = threadIdx.x; i < 384; i += 256) ws[i] = p.w[i];     // [ci][c][q]
    if (threadIdx.x < 3) bs[threadIdx.x] = p.bias[threadIdx.x];
    __syncthreads();
    float lsum = 0.f;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.total) {
        const int x = (int)(idx % p.w_), y = (int)((idx / p.w_) % p.h);
        const long long n = idx / ((long long)p.w_ * p.h);
        float r[32];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const f32x4 v = io::ld((const T*)p.in + idx * 32 + 4 * k);
            r[4 * k] = v[0]; r[4 * k + 1] = v[1]; r[4 * k + 2] = v[2]; r[4 * k + 3] = v[3];
        }
        float dp[12];       // index q*3 + c
        const int H2 = 2 * p.h, W2 = 2 * p.w_;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pre = bs[c];
#pragma unroll
                for (int ci = 0; ci < 32; ++ci) pre = fmaf(r[ci], ws[ci * 12 + c * 4 + q], pre);
                const float rec = vad_tanh(pre);
                const size_t xo = (((size_t)n * 3 + c) * H2 + 2 * y + (q >> 1)) * W2 + 2 * x + (q & 1);
                const float d = rec - p.x[xo];
                if (p.recon) p.recon[xo] = rec;
                lsum = fmaf(d, d, lsum);
                dp[q * 3 + c] = p.gscale * d * (1.f - rec * rec);
            }
        if (p.din) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = 0.f;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int c = 0; c < 3; ++c) s = fmaf(dp[q * 3 + c], ws[(4 * k + e) * 12 + c * 4 + q], s);
                    o[e] = s;
                }
                io::st((T*)p.din + idx * 32 + 4 * k, o);
            }
        }
        if (p.dpre) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (k < 3) o = f32x4{dp[4 * k], dp[4 * k + 1], dp[4 * k + 2], dp[4 * k + 3]};
                io::st((T*)p.dpre + idx * 32 + 4 * k, o);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) p.loss_parts[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss = sum(parts)/count (fixed order); optionally db[c] = sum_q colsum[q*3+c]
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* parts, int nparts, double count, float* loss,
                                                            const float* colsum32, float* dbias3) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += (double)parts[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / count);
    if (dbias3 && threadIdx.x < 3)
        dbias3[threadIdx.x] = (colsum32[threadIdx.x] + colsum32[3 + threadIdx.x]) + (colsum32[6 + threadIdx.x] + colsum32[9 + threadIdx.x]);
}

// The same layer as three launches, for criteria whose gradient is not a function of the pixel alone (SSIM: an 11x11
// neighbourhood): forward, the criterion on `recon` (csrc/ssim.hip), then the backward from an arbitrary d loss / d recon.
// A thread owns one input pixel = 2x2x3 outputs; per channel these are two rows of one adjacent float pair, so adjacent lanes
// touch contiguous 8-byte pieces of the NCHW planes.
struct To3FwdP { const void* in; const float* w; const float* bias; float* recon; int h, w_; long long total; };

// recon = tanh(convT(in) + b): the fmaf chain from the bias and vad_tanh of convt_to3_mse_kernel - the same bits.
template <typename T>
__global__ __launch_bounds__(256) void convt_to3_tanh_fwd_kernel(To3FwdP p) {
    typedef vad_io4<T> io;
    __shared__ float ws[32 * 12], bs[3];
    for (int i = threadIdx.x; i < 384; i += 256) ws[i] = p.w[i];     // [ci][c][q]
    if (threadIdx.x < 3) bs[threadIdx.x] = p.bias[threadIdx.x];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int x = (int)(idx % p.w_), y = (int)((idx / p.w_) % p.h);
    const long long n = idx / ((long long)p.w_ * p.h);
    float r[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const f32x4 v = io::ld((const T*)p.in + idx * 32 + 4 * k);
        r[4 * k] = v[0]; r[4 * k + 1] = v[1]; r[4 * k + 2] = v[2]; r[4 * k + 3] = v[3];
    }
    const int H2 = 2 * p.h, W2 = 2 * p.w_;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            f32x2 o;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int q = 2 * dy + dx;
                float pre = bs[c];
#pragma unroll
                for (int ci = 0; ci < 32; ++ci) pre = fmaf(r[ci], ws[ci * 12 + c * 4 + q], pre);
                o[dx] = vad_tanh(pre);
            }
            *(f32x2*)&p.recon[(((size_t)n * 3 + c) * H2 + 2 * y + dy) * W2 + 2 * x] = o;
        }
}

struct To3BwdP { const float* recon; const float* drecon; const float* w; void* din; void* dpre; int h, w_; float grad_mul; long long total; };

// dp[q*3+c] = grad_mul * drecon * (1 - recon^2); din = dp . W in convt_to3_mse_kernel's summation order; dpre = the 32-column
// weight-gradient operand.  Reads the reconstruction and its gradient only: neither the layer's input nor its forward.
template <typename T>
__global__ __launch_bounds__(256) void convt_to3_tanh_bwd_kernel(To3BwdP p) {
    typedef vad_io4<T> io;
    __shared__ float ws[32 * 12];
    for (int i = threadIdx.x; i < 384; i += 256) ws[i] = p.w[i];     // [ci][c][q]
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.total) return;
    const int x = (int)(idx % p.w_), y = (int)((idx / p.w_) % p.h);
    const long long n = idx / ((long long)p.w_ * p.h);
    const int H2 = 2 * p.h, W2 = 2 * p.w_;
    float dp[12];       // index q*3 + c
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const size_t o = (((size_t)n * 3 + c) * H2 + 2 * y + dy) * W2 + 2 * x;
            const f32x2 rec = *(const f32x2*)&p.recon[o], d = *(const f32x2*)&p.drecon[o];
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) dp[(2 * dy + dx) * 3 + c] = p.grad_mul * d[dx] * (1.f - rec[dx] * rec[dx]);
        }
    if (p.din) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) s = fmaf(dp[q * 3 + c], ws[(4 * k + e) * 12 + c * 4 + q], s);
                o[e] = s;
            }
            io::st((T*)p.din + idx * 32 + 4 * k, o);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (k < 3) o = f32x4{dp[4 * k], dp[4 * k + 1], dp[4 * k + 2], dp[4 * k + 3]};
        io::st((T*)p.dpre + idx * 32 + 4 * k, o);
    }
}

// db[c] = sum_q colsum[q*3+c], in loss_finalize_kernel's order
__global__ void to3_dbias_kernel(const float* colsum32, float* dbias3) {
    if (threadIdx.x < 3)
        dbias3[threadIdx.x] = (colsum32[threadIdx.x] + colsum32[3 + threadIdx.x]) + (colsum32[6 + threadIdx.x] + colsum32[9 + threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ optimiser
// torch.optim.Adam (train_video.py:175): g += wd*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
// p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, long long n, float lr, float b1,
                                                   float b2, float eps, float wd, float bc1, float sqrt_bc2, float gscale) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float pv = p[i];
        const float gv = g[i] * gscale + wd * pv;
        const float mv = b1 * m[i] + (1.f - b1) * gv;
        const float vv = b2 * v[i] + (1.f - b2) * gv * gv;
        m[i] = mv;
        v[i] = vv;
        p[i] = pv - (lr / bc1) * (mv / (sqrtf(vv) / sqrt_bc2 + eps));
    }
}

// ------------------------------------------------------------------------------------------------ operand packing
// torch layouts -> the kernels' MFMA operand orders, on the device (the parameters change every step)
// split != 0: the split-fp16 operand form of the same weights (csrc/pack.cpp, conv_pkernel.h): per 16 input channels and
// output channel, two halves h of [8 x hi | 8 x lo] fp16 with hi = fp16(w), lo = fp16((w - hi) * 2^11); same byte count.
// split == 2: bf16 operands in the same slots: hi = bf16(w), lo unused (conv_pkernel.h, PREC 2)
__device__ __forceinline__ void put_split(float* dst, size_t group16, int k, float v, int mode) {      // k = channel index inside the 16
    _Float16* o = (_Float16*)dst + (group16 * 2 + ((k >> 3) & 1)) * 16;
    if (mode == 2) {
        o[k & 7] = __builtin_bit_cast(_Float16, (__bf16)v);
        o[8 + (k & 7)] = (_Float16)0.f;
        return;
    }
    const _Float16 hi = (_Float16)v;
    o[k & 7] = hi;
    o[8 + (k & 7)] = (_Float16)((v - (float)hi) * 2048.0f);
}

__global__ __launch_bounds__(256) void scale_kernel(float* p, long long n, float mul) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] *= mul;
}

__global__ __launch_bounds__(256) void pack_conv3x3_kernel(const float* w, int cout, int cin, float* fwd, float* dgrad, int split) {
    const long long total = (long long)cout * cin * 9;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int tap = (int)(idx % 9), ci = (int)((idx / 9) % cin), co = (int)(idx / (9ll * cin));
        const float v = w[idx];
        // data gradient = the same convolution with the taps rotated by 180 degrees and the channel roles swapped
        if (split) {
            if (fwd) put_split(fwd, ((size_t)tap * (cin / 16) + ci / 16) * cout + co, ci & 15, v, split);
            if (dgrad) put_split(dgrad, ((size_t)(8 - tap) * (cout / 16) + co / 16) * cin + ci, co & 15, v, split);
        } else {
            if (fwd) fwd[(((size_t)tap * (cin / 8) + ci / 8) * cout + co) * 8 + (ci & 7)] = v;
            if (dgrad) dgrad[(((size_t)(8 - tap) * (cout / 8) + co / 8) * cin + ci) * 8 + (co & 7)] = v;
        }
    }
}

// Winograd F(2x2,3x3) forms of a Conv2d weight for the training step's VAD_PREC_WINO mode (csrc/conv_wino.hip): U = G g G^T per
// (output, input) channel pair in double, rounded once - the forward form [16][cin/8][cout][8] and the data-gradient form (taps
// rotated by 180 degrees, channel roles swapped) [16][cout/8][cin][8].  One thread per channel pair.
__global__ __launch_bounds__(256) void pack_conv3x3_wino_kernel(const float* w, int cout, int cin, float* fwd, float* dgrad) {
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const long long total = (long long)cout * cin;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int ci = (int)(idx % cin), co = (int)(idx / cin);
        double g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = (double)w[idx * 9 + a * 3 + b];
#pragma unroll
        for (int fr = 0; fr < 4; ++fr)
#pragma unroll
            for (int fc = 0; fc < 4; ++fc) {
                double u = 0.0, ur = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        u += G[fr][a] * g[a][b] * G[fc][b];
                        ur += G[fr][a] * g[2 - a][2 - b] * G[fc][b];
                    }
                const int f = fr * 4 + fc;
                if (fwd) fwd[(((size_t)f * (cin / 8) + ci / 8) * cout + co) * 8 + (ci & 7)] = (float)u;
                if (dgrad) dgrad[(((size_t)f * (cout / 8) + co / 8) * cin + ci) * 8 + (co & 7)] = (float)ur;
            }
    }
}

__global__ __launch_bounds__(256) void pack_convt2x2_kernel(const float* w, int cin, int cout, float* fwd, float* dgrad, int split, int dgrad16) {
    const long long total = (long long)cin * cout * 4;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int q = (int)(idx & 3), co = (int)((idx >> 2) % cout), ci = (int)(idx / (4ll * cout));
        const float v = w[idx];
        if (fwd) {
            if (split) put_split(fwd, ((size_t)q * (cin / 16) + ci / 16) * cout + co, ci & 15, v, split);
            else fwd[(((size_t)q * (cin / 8) + ci / 8) * cout + co) * 8 + (ci & 7)] = v;
        }
        // data gradient = 1x1 convolution over the space-to-depth gradient (K index q*cout+co, N index ci); that GEMM
        // runs in exact fp32 in either mode
        // (dgrad16: VAD_PREC_BF16S runs that GEMM on bf16 operands too - the gradient tensors are bf16 in memory)
        if (dgrad) {
            const int kk = q * cout + co;
            if (dgrad16) put_split(dgrad, (size_t)(kk / 16) * cin + ci, kk & 15, v, 2);
            else dgrad[(((size_t)(kk / 8)) * cin + ci) * 8 + (kk & 7)] = v;
        }
    }
}

__global__ __launch_bounds__(256) void pack_conv1x1_kernel(const float* w, int cout, int cin, float* fwd, float* dgrad, int bf16) {
    const long long total = (long long)cout * cin;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int ci = (int)(idx % cin), co = (int)(idx / cin);
        const float v = w[idx];
        if (bf16) {
            if (fwd) put_split(fwd, (size_t)(ci / 16) * cout + co, ci & 15, v, 2);
            if (dgrad) put_split(dgrad, (size_t)(co / 16) * cin + ci, co & 15, v, 2);
            continue;
        }
        if (fwd) fwd[(((size_t)(ci / 8)) * cout + co) * 8 + (ci & 7)] = v;          // K = ci, N = co
        if (dgrad) dgrad[(((size_t)(co / 8)) * cin + ci) * 8 + (co & 7)] = v;       // K = co, N = ci
    }
}

__global__ __launch_bounds__(256) void pack_conv3x3_c3_kernel(const float* w, int cout, float* fwd) {
    const int total = 28 * cout;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int co = idx % cout, k = idx / cout;
        fwd[idx] = k < 27 ? w[(size_t)co * 27 + k] : 0.f;
    }
}

// ------------------------------------------------------------------------------------ image autoencoder: last layer
// Conv2d(32->3, k3, p1) + Tanh (models/autoencoder.py:134-135) in train mode.  Forward = the scoring tail kernel on
// device-packed weights.  Backward: dpre = d(recon) * (1 - recon^2) as three NCHW planes; with the roles swapped the first
// layer's kernels do the rest - the data gradient is a 3->32 convolution of dpre with the rotated weights
// (vad_conv3x3_c3), the weight gradient is the first-layer weight gradient of (x := dpre, g := input activation), read back
// with taps mirrored.
__global__ __launch_bounds__(256) void pack_conv3x3_to3_train_kernel(const float* w, int cin, float* fwd, float* dgrad_c3) {
    const int total = 3 * cin * 9;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int tap = idx % 9, ci = (idx / 9) % cin, co = idx / (9 * cin);
        const float v = w[idx];
        if (fwd) fwd[(size_t)(ci / 4) * 108 + tap * 12 + (ci & 3) * 3 + co] = v;
        if (dgrad_c3) {
            dgrad_c3[(size_t)(co * 9 + (8 - tap)) * cin + ci] = v;           // row k = c*9 + tap' of the [28][cin] first-layer form
            if (co == 0 && tap == 0) dgrad_c3[(size_t)27 * cin + ci] = 0.f;  // padding row
        }
    }
}

// dpre[n][c][y][x] = g * (1 - recon^2), g = drecon (given) or gscale * (recon - x); per-block partial sums of dpre for the
// bias gradient: parts[(n*3 + c) * chunks + chunk]
__global__ __launch_bounds__(256) void tanh_bwd_planes_kernel(const float* recon, const float* x, const float* drecon, float gscale,
                                                              float gmul, float* dpre, float* parts, long long plane, int chunks) {
    __shared__ float red[4];
    const long long pl = blockIdx.y, base = pl * plane;
    const long long per = (plane + chunks - 1) / chunks, i0 = (long long)blockIdx.x * per, i1 = (i0 + per < plane) ? i0 + per : plane;
    float s = 0.f;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        const float r = recon[base + i];
        const float g = drecon ? drecon[base + i] * gmul : gscale * (r - x[base + i]);
        const float d = g * (1.f - r * r);
        dpre[base + i] = d;
        s += d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) parts[pl * chunks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void bias3_finalize_kernel(const float* parts, int n, int chunks, float* db3) {
    const int c = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n * chunks; i += 64) s += (double)parts[((size_t)(i / chunks) * 3 + c) * chunks + i % chunks];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) db3[c] = (float)s;
}

// dW[c][ci][tap] = tmp[ci][c][8 - tap]   (tmp = first-layer weight gradient of the swapped-role problem, OIHW (cin,3,3,3))
__global__ __launch_bounds__(256) void mirror_last_wgrad_kernel(const float* tmp, int cin, float* dw) {
    const int total = 3 * cin * 9;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int tap = idx % 9, ci = (idx / 9) % cin, c = idx / (9 * cin);
        dw[idx] = tmp[((size_t)ci * 3 + c) * 9 + (8 - tap)];
    }
}

unsigned grid_for(long long total) {
    long long b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

// ================================================================================================ host entry points
// pixels per work-group of the channel-reduction passes: short per-thread loops (memory-level parallelism comes from
// many resident groups), at most 16384 partial rows for the finalize
static long long stats_chunk(long long npix) {
    long long chunk = 512;
    if ((npix + chunk - 1) / chunk > 16384) chunk = (npix + 16383) / 16384;
    return chunk;
}

extern "C" size_t vad_chan_ws_floats(long long npix, int c) {
    if (npix <= 0 || c <= 0) return 0;
    const long long chunk = stats_chunk(npix);
    return (size_t)((npix + chunk - 1) / chunk) * 2 * c;
}

static bool chan_ok(int c) { return c >= 4 && c % 4 == 0 && c <= 1024; }

extern "C" int vad_bn_stats(const float* y, long long npix, int c, float eps, float momentum, float* stats,
                            float* running_mean, float* running_var, float* ws, void* stream) {
    VAD_REQUIRE(y && stats && ws && npix > 0 && chan_ok(c), "bn_stats: bad arguments (c=%d)", c);
    VAD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_stats: running_mean/var must come together");
    const long long chunk = stats_chunk(npix);
    const int nb = (int)((npix + chunk - 1) / chunk);
    // pivot = the first pixel's channel vector (y[0..c)): a sample of each channel
    hipLaunchKernelGGL(chan_sums_kernel<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, y, npix, c, chunk, y, ws);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(chan_finalize_kernel, dim3(c), dim3(256), 0, (hipStream_t)stream, (const float*)ws, nb, c,
                       (double)npix, 0, eps, momentum, stats, running_mean, running_var, (float*)nullptr, (float*)nullptr, y);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

// BatchNorm statistics from partial sums a producer kernel wrote ([nblocks][2][c], shifted by `pivot`): the finalize half of
// vad_bn_stats (internal: conv_mfma.hip's first-layer kernel is the producer).
int vad_bn_stats_from_partials(const float* partials, int nblocks, long long npix, int c, float eps, float momentum, float* stats,
                               float* running_mean, float* running_var, const float* pivot, void* stream) {
    VAD_REQUIRE(partials && stats && pivot && nblocks > 0 && npix > 0 && chan_ok(c), "bn_stats_from_partials: bad arguments (c=%d)", c);
    VAD_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "bn_stats_from_partials: running_mean/var must come together");
    hipLaunchKernelGGL(chan_finalize_kernel, dim3(c), dim3(256), 0, (hipStream_t)stream, partials, nblocks, c,
                       (double)npix, 0, eps, momentum, stats, running_mean, running_var, (float*)nullptr, (float*)nullptr, pivot);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_chan_sum(const float* g, long long npix, int c, float* out, float* ws, void* stream) {
    return vad_chan_sum_t(g, 0, npix, c, out, ws, stream);
}

// io16 != 0 (here and in the *_t forms below): the activation / gradient tensors are bf16 in memory (VAD_PREC_BF16S)
int vad_chan_sum_t(const void* g, int io16, long long npix, int c, float* out, float* ws, void* stream) {
    VAD_REQUIRE(g && out && ws && npix > 0 && chan_ok(c), "chan_sum: bad arguments (c=%d)", c);
    const long long chunk = stats_chunk(npix);
    const int nb = (int)((npix + chunk - 1) / chunk);
    if (io16) hipLaunchKernelGGL(chan_sums_kernel<vad_bf16>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const vad_bf16*)g, npix, c, chunk, (const float*)nullptr, ws);
    else hipLaunchKernelGGL(chan_sums_kernel<float>, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)g, npix, c, chunk, (const float*)nullptr, ws);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(chan_finalize_kernel, dim3(c), dim3(256), 0, (hipStream_t)stream, (const float*)ws, nb, c,
                       (double)npix, 2, 0.f, 0.f, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, out, (const float*)nullptr);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_bn_act_pool_fwd(const float* y, const float* stats, const float* gamma, const float* beta, float* out,
                                   long long out_fs, int out_ps, int remap_t, int remap_b, int n, int h, int w, int c,
                                   int act, int pool, void* stream) {
    return vad_bn_act_pool_fwd_t(y, 0, stats, gamma, beta, out, out_fs, out_ps, remap_t, remap_b, n, h, w, c, act, pool, stream);
}

static std::atomic<int> g_bn_wide{1};     // debug / A-B: 0 = the bf16 BatchNorm passes at four channels per thread
extern "C" int vad_debug_set_bn_wide(int on) { g_bn_wide = on; return VAD_OK; }
int vad_bn_act_pool_fwd_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, void* out,
                          long long out_fs, int out_ps, int remap_t, int remap_b, int n, int h, int w, int c,
                          int act, int pool, void* stream) {
    VAD_REQUIRE(y && stats && gamma && beta && out && n > 0 && h > 0 && w > 0 && chan_ok(c), "bn_act_pool_fwd: bad arguments");
    VAD_REQUIRE(act >= 0 && act <= 2 && (!pool || (h % 2 == 0 && w % 2 == 0)), "bn_act_pool_fwd: bad act/pool");
    VAD_REQUIRE(remap_t == 0 || (remap_b > 0 && n == remap_t * remap_b), "bn_act_pool_fwd: n must equal T*B with a frame remap");
    const int oh = pool ? h / 2 : h, ow = pool ? w / 2 : w;
    BnFwdP p{y, stats, gamma, beta, out, out_fs ? out_fs : (long long)oh * ow * (out_ps ? out_ps : c), out_ps ? out_ps : c,
             remap_t, remap_b, n, h, w, c, act, pool, (long long)n * oh * ow * (c / 4)};
    VAD_REQUIRE(p.out_ps % 4 == 0 && p.out_fs % 4 == 0, "bn_act_pool_fwd: strides must be multiples of 4 elements");
    VAD_REQUIRE(p.total < (1ll << 31), "bn_act_pool_fwd: %lld items are too many for the kernel's 32-bit index arithmetic", p.total);
#define BN_DISPATCH(KERNEL, GRID, STREAM)                                                                                   \
    {                                                                                                                      \
        const int v_ = (pool ? 3 : 0) + act;                                                                               \
        if (io16) switch (v_) {                                                                                            \
            case 0: hipLaunchKernelGGL((KERNEL<vad_bf16, 0, 0>), GRID, dim3(256), 0, STREAM, p); break;                    \
            case 1: hipLaunchKernelGGL((KERNEL<vad_bf16, 0, 1>), GRID, dim3(256), 0, STREAM, p); break;                    \
            case 2: hipLaunchKernelGGL((KERNEL<vad_bf16, 0, 2>), GRID, dim3(256), 0, STREAM, p); break;                    \
            case 3: hipLaunchKernelGGL((KERNEL<vad_bf16, 1, 0>), GRID, dim3(256), 0, STREAM, p); break;                    \
            case 4: hipLaunchKernelGGL((KERNEL<vad_bf16, 1, 1>), GRID, dim3(256), 0, STREAM, p); break;                    \
            default: hipLaunchKernelGGL((KERNEL<vad_bf16, 1, 2>), GRID, dim3(256), 0, STREAM, p); break;                   \
        } else switch (v_) {                                                                                               \
            case 0: hipLaunchKernelGGL((KERNEL<float, 0, 0>), GRID, dim3(256), 0, STREAM, p); break;                       \
            case 1: hipLaunchKernelGGL((KERNEL<float, 0, 1>), GRID, dim3(256), 0, STREAM, p); break;                       \
            case 2: hipLaunchKernelGGL((KERNEL<float, 0, 2>), GRID, dim3(256), 0, STREAM, p); break;                       \
            case 3: hipLaunchKernelGGL((KERNEL<float, 1, 0>), GRID, dim3(256), 0, STREAM, p); break;                       \
            case 4: hipLaunchKernelGGL((KERNEL<float, 1, 1>), GRID, dim3(256), 0, STREAM, p); break;                       \
            default: hipLaunchKernelGGL((KERNEL<float, 1, 2>), GRID, dim3(256), 0, STREAM, p); break;                      \
        }                                                                                                                  \
    }
#define BN8_DISPATCH(KERNEL, GRID, STREAM)                                                                                  \
    switch ((pool ? 3 : 0) + act) {                                                                                        \
        case 0: hipLaunchKernelGGL((KERNEL<0, 0>), GRID, dim3(256), 0, STREAM, p); break;                                  \
        case 1: hipLaunchKernelGGL((KERNEL<0, 1>), GRID, dim3(256), 0, STREAM, p); break;                                  \
        case 2: hipLaunchKernelGGL((KERNEL<0, 2>), GRID, dim3(256), 0, STREAM, p); break;                                  \
        case 3: hipLaunchKernelGGL((KERNEL<1, 0>), GRID, dim3(256), 0, STREAM, p); break;                                  \
        case 4: hipLaunchKernelGGL((KERNEL<1, 1>), GRID, dim3(256), 0, STREAM, p); break;                                  \
        default: hipLaunchKernelGGL((KERNEL<1, 2>), GRID, dim3(256), 0, STREAM, p); break;                                 \
    }
    if (io16 && c % 8 == 0 && p.out_ps % 8 == 0 && p.out_fs % 8 == 0 && g_bn_wide.load(std::memory_order_relaxed)) {
        BN8_DISPATCH(bn_act_pool_fwd8_kernel, dim3(grid_for(p.total / 2)), (hipStream_t)stream)
    } else
    BN_DISPATCH(bn_act_pool_fwd_kernel, dim3(grid_for(p.total)), (hipStream_t)stream)
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

// Debug: the next vad_bn_act_pool_bwd calls record their branch decisions (one byte per output pixel and channel, see
// BnBwdP::dec) consecutively into this buffer until it is full or reset with (NULL, 0).  Used by the decision-conditioned
// float64 oracle of tests/test_hip_train_step.py; vad_debug_train_decisions_used() tells how many bytes were written.
static unsigned char* g_dec_buf = nullptr;
static size_t g_dec_cap = 0, g_dec_used = 0;
extern "C" int vad_debug_set_train_decisions(void* buf, size_t bytes) { g_dec_buf = (unsigned char*)buf; g_dec_cap = buf ? bytes : 0; g_dec_used = 0; return VAD_OK; }
extern "C" size_t vad_debug_train_decisions_used(void) { return g_dec_used; }

extern "C" int vad_bn_act_pool_bwd(const float* y, const float* stats, const float* gamma, const float* beta, const float* dout,
                                   long long dout_fs, int dout_ps, int remap_t, int remap_b, float* dy, int s2d,
                                   float* dgamma, float* dbeta, float* ksums, float* ws, int n, int h, int w, int c, int act,
                                   int pool, void* stream) {
    return vad_bn_act_pool_bwd_t(y, 0, stats, gamma, beta, dout, dout_fs, dout_ps, remap_t, remap_b, dy, s2d, dgamma, dbeta, ksums, ws,
                                 n, h, w, c, act, pool, stream);
}

int vad_bn_act_pool_bwd_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, const void* dout,
                          long long dout_fs, int dout_ps, int remap_t, int remap_b, void* dy, int s2d,
                          float* dgamma, float* dbeta, float* ksums, float* ws, int n, int h, int w, int c, int act,
                          int pool, void* stream) {
    return vad_bn_act_pool_bwd_codes_t(y, io16, stats, gamma, beta, dout, dout_fs, dout_ps, remap_t, remap_b, dy, s2d, dgamma, dbeta, ksums, ws,
                                       n, h, w, c, act, pool, nullptr, stream);
}

// codes != NULL: pass A (the sums, dgamma / dbeta, k1 / k2) ONLY, and it also writes one routing byte per pooled element -
// argmax position | sign << 2 - to `codes` ([n * oh * ow][c]); dy is not touched (may be NULL).  For a layer whose dy has a
// single consumer that can work from the routed gradient: vad_conv_c3_wgrad_routed.
int vad_bn_act_pool_bwd_codes_t(const void* y, int io16, const float* stats, const float* gamma, const float* beta, const void* dout,
                                long long dout_fs, int dout_ps, int remap_t, int remap_b, void* dy, int s2d,
                                float* dgamma, float* dbeta, float* ksums, float* ws, int n, int h, int w, int c, int act,
                                int pool, unsigned char* codes, void* stream) {
    VAD_REQUIRE(y && stats && gamma && beta && dout && (dy || codes) && dgamma && dbeta && ksums && ws, "bn_act_pool_bwd: null pointer");
    VAD_REQUIRE(n > 0 && h > 0 && w > 0 && chan_ok(c) && act >= 0 && act <= 2, "bn_act_pool_bwd: bad arguments");
    VAD_REQUIRE(!pool || (h % 2 == 0 && w % 2 == 0), "bn_act_pool_bwd: pooling needs even H, W");
    VAD_REQUIRE(!s2d || (!pool && h % 2 == 0 && w % 2 == 0), "bn_act_pool_bwd: space-to-depth output is for un-pooled layers with even H, W");
    VAD_REQUIRE(dy != dout, "bn_act_pool_bwd: dy must not alias dout (pass B reads dout while writing dy)");
    VAD_REQUIRE(remap_t == 0 || (remap_b > 0 && n == remap_t * remap_b), "bn_act_pool_bwd: n must equal T*B with a frame remap");
    const int oh = pool ? h / 2 : h, ow = pool ? w / 2 : w;
    BnBwdP p{};
    p.y = y; p.stats = stats; p.gamma = gamma; p.beta = beta; p.dout = dout;
    p.dout_ps = dout_ps ? dout_ps : c;
    p.dout_fs = dout_fs ? dout_fs : (long long)oh * ow * p.dout_ps;
    p.t = remap_t; p.b = remap_b; p.ws = ws; p.k = ksums; p.dy = dy; p.s2d = s2d;
    p.n = n; p.h = h; p.w = w; p.c = c; p.act = act; p.pool = pool;
    p.opix = (long long)n * oh * ow;
    VAD_REQUIRE(p.opix * (c / 4) < (1ll << 31), "bn_act_pool_bwd: %lld items are too many for the kernels' 32-bit index arithmetic", p.opix * (c / 4));
    p.chunk = stats_chunk(p.opix);
    p.dec = nullptr;
    p.codes = codes;
    if (g_dec_buf) {
        const size_t need = (size_t)p.opix * c;
        VAD_REQUIRE(g_dec_used + need <= g_dec_cap, "bn_act_pool_bwd: decision buffer too small (%zu + %zu > %zu)", g_dec_used, need, g_dec_cap);
        p.dec = g_dec_buf + g_dec_used;
        g_dec_used += need;
    }
    VAD_REQUIRE(p.dout_ps % 4 == 0 && p.dout_fs % 4 == 0, "bn_act_pool_bwd: strides must be multiples of 4 floats");
    const int nb = (int)((p.opix + p.chunk - 1) / p.chunk);
    hipStream_t s = (hipStream_t)stream;
    BN_DISPATCH(bn_bwd_sums_kernel, dim3(nb), s)
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(chan_finalize_kernel, dim3(c), dim3(256), 0, s, (const float*)ws, nb, c,
                       (double)n * h * w, 1, 0.f, 0.f, ksums, (float*)nullptr, (float*)nullptr, dgamma, dbeta, (const float*)nullptr);
    VAD_LAUNCH_CHECK();
    p.dec = nullptr;
    if (codes) return VAD_OK;                     // pass A only
    if (io16 && c % 8 == 0 && p.dout_ps % 8 == 0 && p.dout_fs % 8 == 0 && g_bn_wide.load(std::memory_order_relaxed)) {
        BN8_DISPATCH(bn_bwd_apply8_kernel, dim3(grid_for(p.opix * (c / 8))), s)
    } else
    BN_DISPATCH(bn_bwd_apply_kernel, dim3(grid_for(p.opix * (c / 4))), s)
#undef BN_DISPATCH
#undef BN8_DISPATCH
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_lstm_gates_fwd(float* z, const float* c_prev, float* c_out, float* h1, long long h1_fs, int h1_ps,
                                  float* h2, long long h2_fs, int h2_ps, int nb, int hw, int hid, void* stream) {
    return vad_lstm_gates_fwd_t(z, 0, c_prev, c_out, h1, h1_fs, h1_ps, h2, h2_fs, h2_ps, nb, hw, hid, stream);
}

int vad_lstm_gates_fwd_t(void* z, int io16, const float* c_prev, float* c_out, void* h1, long long h1_fs, int h1_ps,
                         void* h2, long long h2_fs, int h2_ps, int nb, int hw, int hid, void* stream) {
    VAD_REQUIRE(z && c_out && nb > 0 && hw > 0 && hid > 0 && hid % 4 == 0, "lstm_gates_fwd: bad arguments");
    LstmFwdP p{z, c_prev, c_out, h1, h1_fs ? h1_fs : (long long)hw * (h1_ps ? h1_ps : hid), h1_ps ? h1_ps : hid,
               h2, h2_fs ? h2_fs : (long long)hw * (h2_ps ? h2_ps : hid), h2_ps ? h2_ps : hid, hw, hid, (long long)nb * hw * (hid / 4)};
    if (io16) hipLaunchKernelGGL(lstm_gates_fwd_kernel<vad_bf16>, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(lstm_gates_fwd_kernel<float>, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_lstm_gates_bwd(const float* gates, const float* c_prev, const float* c, const float* dh1, long long dh1_fs,
                                  int dh1_ps, const float* dh2, long long dh2_fs, int dh2_ps, const float* dc_next, float* dz,
                                  float* dc_prev, int nb, int hw, int hid, void* stream) {
    return vad_lstm_gates_bwd_t(gates, 0, c_prev, c, dh1, dh1_fs, dh1_ps, dh2, dh2_fs, dh2_ps, dc_next, dz, dc_prev, nb, hw, hid, stream);
}

int vad_lstm_gates_bwd_t(const void* gates, int io16, const float* c_prev, const float* c, const void* dh1, long long dh1_fs,
                         int dh1_ps, const void* dh2, long long dh2_fs, int dh2_ps, const float* dc_next, void* dz,
                         float* dc_prev, int nb, int hw, int hid, void* stream) {
    VAD_REQUIRE(gates && c && dz && dc_prev && nb > 0 && hw > 0 && hid > 0 && hid % 4 == 0, "lstm_gates_bwd: bad arguments");
    LstmBwdP p{gates, c_prev, c, dh1, dh1_fs ? dh1_fs : (long long)hw * (dh1_ps ? dh1_ps : hid), dh1_ps ? dh1_ps : hid,
               dh2, dh2_fs ? dh2_fs : (long long)hw * (dh2_ps ? dh2_ps : hid), dh2_ps ? dh2_ps : hid, dc_next, dz, dc_prev,
               hw, hid, (long long)nb * hw * (hid / 4)};
    if (io16) hipLaunchKernelGGL(lstm_gates_bwd_kernel<vad_bf16>, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(lstm_gates_bwd_kernel<float>, dim3(grid_for(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

// ws = [nb loss partials][64: column sums of dpre][partials of that column reduction]
extern "C" size_t vad_convt_to3_mse_ws_floats(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    const long long total = (long long)n * h * w;
    return (size_t)((total + 255) / 256) + 64 + vad_chan_ws_floats(total, 32);
}

extern "C" int vad_convt_to3_mse(const float* in_nhwc, const float* w_iohw, const float* bias3, const float* x_nchw, float* recon,
                                 float* din, float* dpre32, float* loss, float* dbias3, float* ws, int n, int h, int w,
                                 void* stream) {
    return vad_convt_to3_mse_t(in_nhwc, 0, w_iohw, bias3, x_nchw, recon, din, dpre32, loss, dbias3, ws, n, h, w, 1.f, stream);
}

int vad_convt_to3_mse_t(const void* in_nhwc, int io16, const float* w_iohw, const float* bias3, const float* x_nchw, float* recon,
                        void* din, void* dpre32, float* loss, float* dbias3, float* ws, int n, int h, int w, float grad_mul, void* stream) {
    VAD_REQUIRE(in_nhwc && w_iohw && bias3 && x_nchw && loss && ws && n > 0 && h > 0 && w > 0, "convt_to3_mse: bad arguments");
    VAD_REQUIRE(vad_is_pow2f(grad_mul), "convt_to3_mse: grad_mul=%g must be a power of two (an exact rescaling of every gradient)", (double)grad_mul);
    VAD_REQUIRE(!dbias3 || dpre32, "convt_to3_mse: the bias gradient needs the dpre buffer");
    const long long total = (long long)n * h * w;
    const long long nb = (total + 255) / 256;
    VAD_REQUIRE(nb < (1ll << 31), "convt_to3_mse: grid too large");
    const double count = (double)n * 3.0 * (2.0 * h) * (2.0 * w);
    To3P p{in_nhwc, w_iohw, bias3, x_nchw, recon, din, dpre32, ws, n, h, w, (float)(2.0 / count) * grad_mul, total};
    hipStream_t s = (hipStream_t)stream;
    if (io16) hipLaunchKernelGGL(convt_to3_mse_kernel<vad_bf16>, dim3((unsigned)nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(convt_to3_mse_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, p);
    VAD_LAUNCH_CHECK();
    float* colsum = ws + nb;
    if (dbias3) {
        const long long chunk = stats_chunk(total);
        const int cb = (int)((total + chunk - 1) / chunk);
        float* cws = ws + nb + 64;
        if (io16) hipLaunchKernelGGL(chan_sums_kernel<vad_bf16>, dim3(cb), dim3(256), 0, s, (const vad_bf16*)dpre32, total, 32, chunk, (const float*)nullptr, cws);
        else hipLaunchKernelGGL(chan_sums_kernel<float>, dim3(cb), dim3(256), 0, s, (const float*)dpre32, total, 32, chunk, (const float*)nullptr, cws);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(chan_finalize_kernel, dim3(32), dim3(256), 0, s, (const float*)cws, cb, 32, (double)total, 2, 0.f, 0.f,
                           (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, colsum, (const float*)nullptr);
        VAD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, (int)nb, count, loss,
                       (const float*)colsum, dbias3);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

// ws = [64: column sums of dpre][partials of that column reduction]
extern "C" size_t vad_convt_to3_tanh_bwd_ws_floats(int n, int h, int w) {
    if (n <= 0 || h <= 0 || w <= 0) return 0;
    return 64 + vad_chan_ws_floats((long long)n * h * w, 32);
}

int vad_convt_to3_tanh_fwd_t(const void* in_nhwc, int io16, const float* w_iohw, const float* bias3, float* recon, int n, int h, int w,
                             void* stream) {
    VAD_REQUIRE(in_nhwc && w_iohw && bias3 && recon && n > 0 && h > 0 && w > 0, "convt_to3_tanh_fwd: bad arguments");
    const long long total = (long long)n * h * w;
    const long long nb = (total + 255) / 256;
    VAD_REQUIRE(nb < (1ll << 31), "convt_to3_tanh_fwd: grid too large");
    To3FwdP p{in_nhwc, w_iohw, bias3, recon, h, w, total};
    hipStream_t s = (hipStream_t)stream;
    if (io16) hipLaunchKernelGGL(convt_to3_tanh_fwd_kernel<vad_bf16>, dim3((unsigned)nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(convt_to3_tanh_fwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

int vad_convt_to3_tanh_bwd_t(const float* recon, const float* drecon, const float* w_iohw, void* din, void* dpre32, int io16,
                             float* dbias3, float* ws, int n, int h, int w, float grad_mul, void* stream) {
    VAD_REQUIRE(recon && drecon && w_iohw && dpre32 && n > 0 && h > 0 && w > 0, "convt_to3_tanh_bwd: bad arguments");
    VAD_REQUIRE(vad_is_pow2f(grad_mul), "convt_to3_tanh_bwd: grad_mul=%g must be a power of two (an exact rescaling of every gradient)", (double)grad_mul);
    VAD_REQUIRE(!dbias3 || ws, "convt_to3_tanh_bwd: the bias gradient needs the workspace");
    const long long total = (long long)n * h * w;
    const long long nb = (total + 255) / 256;
    VAD_REQUIRE(nb < (1ll << 31), "convt_to3_tanh_bwd: grid too large");
    To3BwdP p{recon, drecon, w_iohw, din, dpre32, h, w, grad_mul, total};
    hipStream_t s = (hipStream_t)stream;
    if (io16) hipLaunchKernelGGL(convt_to3_tanh_bwd_kernel<vad_bf16>, dim3((unsigned)nb), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(convt_to3_tanh_bwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, s, p);
    VAD_LAUNCH_CHECK();
    if (dbias3) {       // the route of vad_convt_to3_mse_t: column sums of dpre, then the four positions of a channel
        const long long chunk = stats_chunk(total);
        const int cb = (int)((total + chunk - 1) / chunk);
        float *colsum = ws, *cws = ws + 64;
        if (io16) hipLaunchKernelGGL(chan_sums_kernel<vad_bf16>, dim3(cb), dim3(256), 0, s, (const vad_bf16*)dpre32, total, 32, chunk, (const float*)nullptr, cws);
        else hipLaunchKernelGGL(chan_sums_kernel<float>, dim3(cb), dim3(256), 0, s, (const float*)dpre32, total, 32, chunk, (const float*)nullptr, cws);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(chan_finalize_kernel, dim3(32), dim3(256), 0, s, (const float*)cws, cb, 32, (double)total, 2, 0.f, 0.f,
                           (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, colsum, (const float*)nullptr);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(to3_dbias_kernel, dim3(1), dim3(64), 0, s, (const float*)colsum, dbias3);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

extern "C" int vad_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int step, float grad_scale, void* stream) {
    VAD_REQUIRE(p && g && m && v && n > 0 && step >= 1, "adam_step: bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                       weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_scale_floats(float* p, long long n, float mul, void* stream) {
    VAD_REQUIRE(p && n > 0, "scale_floats: bad arguments");
    hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, n, mul);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_train_pack_conv3x3(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, int precision, void* stream) {
    VAD_REQUIRE(w_oihw && (fwd || dgrad) && cout > 0 && cin > 0 && cin % 8 == 0 && (!dgrad || cout % 8 == 0), "train_pack_conv3x3: bad arguments");
    if (precision == VAD_PREC_WINO) {     // Winograd forms (16 "taps": vad_pack_conv3x3_wino_floats of room each)
        hipLaunchKernelGGL(pack_conv3x3_wino_kernel, dim3(grid_for((long long)cout * cin)), dim3(256), 0, (hipStream_t)stream, w_oihw, cout, cin, fwd, dgrad);
        VAD_LAUNCH_CHECK();
        return VAD_OK;
    }
    VAD_REQUIRE(precision >= VAD_PREC_FP32 && precision <= VAD_PREC_BF16S, "train_pack_conv3x3: precision=%d must be 0 (fp32), 1 (split fp16), 2 or 3 (bf16) or 4 (Winograd)", precision);
    const int split = precision == VAD_PREC_BF16S ? 2 : precision;   // the packed layout follows the arithmetic mode, like the host packers (2 = bf16 in the hi slots)
    VAD_REQUIRE(!split || (cin % 16 == 0 && (!dgrad || cout % 16 == 0)), "train_pack_conv3x3: split precision needs channel counts in multiples of 16");
    hipLaunchKernelGGL(pack_conv3x3_kernel, dim3(grid_for(9ll * cout * cin)), dim3(256), 0, (hipStream_t)stream, w_oihw, cout, cin, fwd, dgrad, split);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_train_pack_convt2x2(const float* w_iohw, int cin, int cout, float* fwd, float* dgrad, int precision, void* stream) {
    VAD_REQUIRE(w_iohw && (fwd || dgrad) && cout > 0 && cin > 0 && cin % 8 == 0 && (!dgrad || (4 * cout) % 8 == 0), "train_pack_convt2x2: bad arguments");
    VAD_REQUIRE(precision >= VAD_PREC_FP32 && precision <= VAD_PREC_BF16S, "train_pack_convt2x2: precision=%d must be 0 (fp32), 1 (split fp16), 2 or 3 (bf16)", precision);
    const int split = precision == VAD_PREC_BF16S ? 2 : precision;
    VAD_REQUIRE(!split || cin % 16 == 0, "train_pack_convt2x2: split precision needs cin in multiples of 16");
    hipLaunchKernelGGL(pack_convt2x2_kernel, dim3(grid_for(4ll * cout * cin)), dim3(256), 0, (hipStream_t)stream, w_iohw, cin, cout, fwd, dgrad, split,
                       precision == VAD_PREC_BF16S ? 1 : 0);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_train_pack_conv1x1(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, void* stream) {
    return vad_train_pack_conv1x1_p(w_oihw, cout, cin, fwd, dgrad, VAD_PREC_FP32, stream);
}

// precision VAD_PREC_BF16S: bf16 operand forms ([K/16][N][half][8 x bf16 | unused]) for vad_conv1x1_p; anything else: fp32
int vad_train_pack_conv1x1_p(const float* w_oihw, int cout, int cin, float* fwd, float* dgrad, int precision, void* stream) {
    VAD_REQUIRE(w_oihw && (fwd || dgrad) && cout > 0 && cin > 0 && cin % 8 == 0 && (!dgrad || cout % 8 == 0), "train_pack_conv1x1: bad arguments");
    const int bf16 = precision == VAD_PREC_BF16S;
    VAD_REQUIRE(!bf16 || (cin % 16 == 0 && cout % 16 == 0), "train_pack_conv1x1: bf16 operands need channel counts in multiples of 16");
    hipLaunchKernelGGL(pack_conv1x1_kernel, dim3(grid_for((long long)cout * cin)), dim3(256), 0, (hipStream_t)stream, w_oihw, cout, cin, fwd, dgrad, bf16);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

extern "C" int vad_train_pack_conv3x3_c3(const float* w_oihw, int cout, float* fwd, void* stream) {
    VAD_REQUIRE(w_oihw && fwd && cout > 0, "train_pack_conv3x3_c3: bad arguments");
    hipLaunchKernelGGL(pack_conv3x3_c3_kernel, dim3(grid_for(28ll * cout)), dim3(256), 0, (hipStream_t)stream, w_oihw, cout, fwd);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

// ------------------------------------------------------------------------------------ image autoencoder: last layer (host)
extern "C" int vad_train_pack_conv3x3_to3(const float* w_oihw, int cin, float* fwd, float* dgrad_c3, void* stream) {
    VAD_REQUIRE(w_oihw && (fwd || dgrad_c3) && cin > 0 && cin % 4 == 0, "train_pack_conv3x3_to3: bad arguments");
    hipLaunchKernelGGL(pack_conv3x3_to3_train_kernel, dim3(grid_for(27ll * cin)), dim3(256), 0, (hipStream_t)stream, w_oihw, cin, fwd, dgrad_c3);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

static int to3_chunks(int h, int w) { const long long plane = (long long)h * w; return (int)((plane + 16383) / 16384); }

// ws = [bias partials n*3*chunks][64: zero bias for the data-gradient conv][tmp weight gradient cin*27][first-layer wgrad ws]
extern "C" size_t vad_conv3x3_to3_bwd_ws_floats(int n, int h, int w, int cin) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin % 32) return 0;
    return (size_t)n * 3 * to3_chunks(h, w) + 64 + (size_t)cin * 27 + vad_conv_c3_wgrad_ws_floats(n, h, cin);
}

extern "C" int vad_conv3x3_to3_tanh_bwd(const float* in_nhwc, const float* recon, const float* x, const float* drecon,
                                        const float* w_dgrad_c3, float* dpre, float* din, float* dw, float* db3, float* ws,
                                        int n, int h, int w, int cin, float grad_mul, void* stream) {
    VAD_REQUIRE(in_nhwc && recon && (x || drecon) && w_dgrad_c3 && dpre && din && dw && db3 && ws, "conv3x3_to3_tanh_bwd: null pointer");
    VAD_REQUIRE(vad_is_pow2f(grad_mul), "conv3x3_to3_tanh_bwd: grad_mul=%g must be a power of two", (double)grad_mul);
    VAD_REQUIRE(n > 0 && h > 0 && w > 0 && cin == 32, "conv3x3_to3_tanh_bwd: bad shape (the reference's last conv has 32 input channels)");
    hipStream_t s = (hipStream_t)stream;
    const int chunks = to3_chunks(h, w);
    float* parts = ws;
    float* zero_bias = ws + (size_t)n * 3 * chunks;
    float* tmp = zero_bias + 64;
    float* wws = tmp + (size_t)cin * 27;
    VAD_HIP_TRY(hipMemsetAsync(zero_bias, 0, 64 * sizeof(float), s));
    const double count = (double)n * 3.0 * h * w;
    hipLaunchKernelGGL(tanh_bwd_planes_kernel, dim3(chunks, n * 3), dim3(256), 0, s, recon, x, drecon, (float)(2.0 / count) * grad_mul, grad_mul, dpre, parts,
                       (long long)h * w, chunks);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(bias3_finalize_kernel, dim3(3), dim3(64), 0, s, (const float*)parts, n, chunks, db3);
    VAD_LAUNCH_CHECK();
    int rc = vad_conv3x3_c3(dpre, w_dgrad_c3, zero_bias, din, n, h, w, cin, VAD_ACT_NONE, 0, stream);      // data gradient
    if (rc != VAD_OK) return rc;
    rc = vad_conv_c3_wgrad(dpre, in_nhwc, tmp, wws, n, h, w, cin, stream);                                  // swapped-role weight gradient
    if (rc != VAD_OK) return rc;
    hipLaunchKernelGGL(mirror_last_wgrad_kernel, dim3(grid_for(27ll * cin)), dim3(256), 0, s, (const float*)tmp, cin, dw);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
