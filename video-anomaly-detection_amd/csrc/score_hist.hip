// Score histogram: the joint distribution of (score, label) as integer counters, the one thing a ranking metric (AUROC, ROC
// curve, average precision, a threshold at a false-positive rate) needs of a per-pixel error map / SSIM map and its ground-truth
// mask, or of frame scores and frame labels.  The reference plots the mask beside the map (evaluate.py:142-171) and sorts the
// frame scores on the host (evaluate_video.py:171-176); here the maps never leave the device: only the counters do, once.
//
// Quantiser, parameter m = mantissa_bits in 4..15: a finite v >= 0 (-0.0 counts as 0) has key = float_bits(v) >> (23 - m), the
// sign-less exponent and the top m mantissa bits - monotone in v, (255 << m) bins.  A negative value, a NaN or an infinity is not
// binned: it increments rejected[class].
//
// State blob (caller-owned, 16-byte aligned):  u32 header[4] = {magic "VADH", abi << 16 | m, m, 0};  u64 counts[2][nbins];
// u64 rejected[2].  Every kernel compares the header with its own m ON THE DEVICE and does nothing on a mismatch: a blob made for
// another m (a smaller allocation) is never indexed with this m's bins.
//
// Combining: integer atomics only, so the counters are exact and the same for every batching, launch order and sharding.  Error
// maps sit in a few exponents - one atomic per element would pile onto a few cache lines - so equal keys are combined on chip
// before they reach HBM, in two steps:
//   wave   when every active lane of a wave instruction holds the same (key, class) - a constant region, a saturated patch -, ONE
//          lane adds the lane count;
//   block  an LDS table of HIST_SLOTS (key, class) -> u32 count entries per work-group (one work-group per CU, 128 KiB), the slot
//          taken from the low bits of 2 * key + class with HIST_PROBES linear probes: a frame of a 256 x 256 error map populates
//          ~10 k bins at m = 11, which fit.  Lanes that find no slot add to the global counters directly, one add per distinct
//          bin among them (the overflow path: correct for any distribution, slower when more distinct bins than slots are live).
// The table and its overflow path live in score_hist_lds.h (region_overlap.hip counts its unweighted classes through them too).
// A work-group takes a contiguous run of the input (neighbouring pixels share bins) and at its end adds each live slot to its
// 64-bit global counter: at most HIST_SLOTS global atomics per work-group, to contiguous addresses, however many elements it
// has seen.  A launch covers at most 2^30 elements (the host splits longer calls), so a u32 slot cannot wrap.
//
// Loads: the values' 16-byte aligned body as one 16-byte load per lane (labels: 16 bytes of floats / 4 bytes of uint8 where
// their address allows, single elements otherwise); the up to 3 + 3 elements in front of and behind the body one per lane.
#include <hip/hip_runtime.h>

#include "score_hist_lds.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr unsigned HIST_MAGIC = 0x48444156u;   // "VADH"
constexpr long long HIST_LAUNCH_ELEMS = 1ll << 30;

__device__ __forceinline__ bool hist_header_ok(const unsigned* hdr, int m) {
    return hdr[0] == HIST_MAGIC && hdr[1] == hist_tag(m) && hdr[2] == (unsigned)m;
}

struct HistP {
    const float* values;
    const void* labels;
    unsigned* state;
    long long base;          // index of values[0] in the whole call (VAD_LBL_U8_GROUP: group = (base + i) / group_elems)
    long long group_elems;
    unsigned n;              // elements of this launch
    unsigned head;           // elements in front of the 16-byte aligned body
    unsigned quads;          // 16-byte groups of the body
    int fmt, m;
    int lab_vec;             // the labels of a quad can be loaded as one word (u8) / one 16-byte vector (f32)
};

// One element of every lane that calls (converged: all lanes of the caller's loop iteration).  rej0 / rej1: the lane's rejected
// counts per class.
__device__ __forceinline__ void hist_count(HistLds& s, u64* counts, unsigned nbins, int shift, float v, bool pos, unsigned& rej0,
                                           unsigned& rej1) {
    unsigned bits = __float_as_uint(v);
    if (bits == 0x80000000u) bits = 0u;                      // -0.0 is 0
    const bool ok = bits < 0x7f800000u;                      // finite and >= 0 (a set sign bit compares above)
    rej0 += (!ok && !pos) ? 1u : 0u;
    rej1 += (!ok && pos) ? 1u : 0u;
    const unsigned bin = ok ? (pos ? nbins : 0u) + (bits >> shift) : 0u;
    const u64 act = __ballot(ok);
    if (act == 0) return;                                    // wave-uniform
    const int lead = __builtin_ctzll(act);
    const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)bin, lead);
    if (__ballot(ok && bin == first) == act)                 // every binned lane holds the same bin: one add for the instruction
        hist_lds_add(s, counts, nbins, first, (unsigned)__builtin_popcountll(act), (int)(threadIdx.x & 63u) == lead);
    else
        hist_lds_add(s, counts, nbins, bin, 1u, ok);
}

__device__ __forceinline__ bool hist_label(const HistP& p, long long i) {    // element i of this launch, one at a time
    if (p.fmt == VAD_LBL_U8_ELEM) return ((const unsigned char*)p.labels)[i] >= 128;
    if (p.fmt == VAD_LBL_F32_ELEM) return ((const float*)p.labels)[i] > 0.5f;
    return ((const unsigned char*)p.labels)[(p.base + i) / p.group_elems] != 0;
}

__global__ __launch_bounds__(HIST_THREADS) void hist_accumulate_kernel(HistP p) {
    if (!hist_header_ok(p.state, p.m)) return;               // uniform over the grid: not this m's blob, nothing is touched
    __shared__ HistLds s;
    for (int i = threadIdx.x; i < HIST_SLOTS; i += HIST_THREADS) {
        s.tag[i] = 0u;
        s.cnt[i] = 0u;
    }
    if (threadIdx.x < 2) s.rej[threadIdx.x] = 0u;
    __syncthreads();

    const unsigned nbins = hist_nbins(p.m);
    const int shift = 23 - p.m;
    u64* counts = (u64*)(p.state + 4);
    unsigned rej0 = 0u, rej1 = 0u;

    const float* body = p.values + p.head;
    // a work-group takes one contiguous run of the body (a frame or a part of one: a map's neighbours share bins, so the table
    // sees the fewest distinct keys this way)
    const unsigned per = (p.quads + gridDim.x - 1) / gridDim.x;
    const unsigned q_lo = blockIdx.x * per, q_hi = q_lo + per < p.quads ? q_lo + per : p.quads;
    for (unsigned q = q_lo + threadIdx.x; q < q_hi; q += HIST_THREADS) {
        const f32x4 v = *(const f32x4*)(body + 4ull * q);
        const long long i0 = (long long)p.head + 4ll * q;
        bool pos[4];
        if (p.fmt == VAD_LBL_F32_ELEM) {
            const float* lp = (const float*)p.labels + i0;
            if (p.lab_vec) {
                const f32x4 l = *(const f32x4*)lp;
#pragma unroll
                for (int j = 0; j < 4; ++j) pos[j] = l[j] > 0.5f;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) pos[j] = lp[j] > 0.5f;
            }
        } else if (p.fmt == VAD_LBL_U8_ELEM) {
            const unsigned char* lp = (const unsigned char*)p.labels + i0;
            if (p.lab_vec) {
                const unsigned w = *(const unsigned*)lp;
#pragma unroll
                for (int j = 0; j < 4; ++j) pos[j] = ((w >> (8 * j)) & 255u) >= 128u;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) pos[j] = lp[j] >= 128;
            }
        } else {
            const unsigned char* lp = (const unsigned char*)p.labels;
            const u64 e = (u64)(p.base + i0), ge = (u64)p.group_elems;
            u64 g = e / ge, r = e - g * ge;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pos[j] = lp[g] != 0;
                if (++r == ge) {
                    r = 0;
                    ++g;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) hist_count(s, counts, nbins, shift, v[j], pos[j], rej0, rej1);
    }
    // the elements in front of and behind the body (at most 3 + 3), one per lane of the first work-group
    const unsigned edge = p.n - 4u * p.quads;
    if (blockIdx.x == 0 && threadIdx.x < edge) {
        const long long i = threadIdx.x < p.head ? (long long)threadIdx.x : (long long)threadIdx.x + 4ll * p.quads;
        hist_count(s, counts, nbins, shift, p.values[i], hist_label(p, i), rej0, rej1);
    }

    if (rej0) atomicAdd(&s.rej[0], rej0);
    if (rej1) atomicAdd(&s.rej[1], rej1);
    __syncthreads();
    for (int i = threadIdx.x; i < HIST_SLOTS; i += HIST_THREADS) {
        const unsigned t = s.tag[i];
        if (t != 0u) atomicAdd(&counts[t - 1u], (u64)s.cnt[i]);
    }
    if (threadIdx.x < 2 && s.rej[threadIdx.x] != 0u) atomicAdd(&counts[2ull * nbins + threadIdx.x], (u64)s.rej[threadIdx.x]);
}

__global__ void hist_header_kernel(unsigned* state, int m) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *(u32x4*)state = u32x4{HIST_MAGIC, hist_tag(m), (unsigned)m, 0u};
}

// dst += src over counts and rejected: (2 * nbins + 2) 64-bit words behind the headers, two per lane.
__global__ __launch_bounds__(256) void hist_merge_kernel(unsigned* dst, const unsigned* src, int m) {
    if (!hist_header_ok(dst, m) || !hist_header_ok(src, m)) return;
    const unsigned pairs = hist_nbins(m) + 1u;
    u64x2* d = (u64x2*)(dst + 4);
    const u64x2* s = (const u64x2*)(src + 4);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < pairs; i += gridDim.x * 256u) d[i] += s[i];
}

}  // namespace

size_t vad_hist_state_bytes(int m) {
    if (!vad_hist_m_ok(m)) return 0;
    return 16 + 8 * (2 * (size_t)hist_nbins(m) + 2);
}

int vad_hist_reset(void* state, int m, void* stream) {
    VAD_ARG(vad_req_mantissa("hist_reset", m));
    VAD_ARG(vad_req_ptr("hist_reset", "state", state, 16));
    const hipStream_t s = (hipStream_t)stream;
    VAD_HIP_TRY(hipMemsetAsync(state, 0, vad_hist_state_bytes(m), s));
    hipLaunchKernelGGL(hist_header_kernel, dim3(1), dim3(64), 0, s, (unsigned*)state, m);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

int vad_hist_accumulate(const float* values, long long n_groups, long long group_elems, const void* labels, int label_format,
                        void* state, int m, void* stream) {
    const char* who = "hist_accumulate";
    VAD_ARG(vad_req_mantissa(who, m));
    VAD_ARG(vad_req_nonnull(who, "values", values));
    VAD_ARG(vad_req_nonnull(who, "labels", labels));
    VAD_ARG(vad_req_nonnull(who, "state", state));
    VAD_REQUIRE(label_format == VAD_LBL_U8_ELEM || label_format == VAD_LBL_F32_ELEM || label_format == VAD_LBL_U8_GROUP,
                "hist_accumulate: label_format must be VAD_LBL_U8_ELEM (%d), VAD_LBL_F32_ELEM (%d) or VAD_LBL_U8_GROUP (%d), got %d",
                VAD_LBL_U8_ELEM, VAD_LBL_F32_ELEM, VAD_LBL_U8_GROUP, label_format);
    VAD_REQUIRE(n_groups >= 0, "hist_accumulate: n_groups must be >= 0, got %lld", n_groups);
    VAD_REQUIRE(group_elems > 0, "hist_accumulate: group_elems must be positive, got %lld", group_elems);
    long long total = 0;
    VAD_REQUIRE(!__builtin_mul_overflow(n_groups, group_elems, &total) && total <= (1ll << 60),
                "hist_accumulate: n_groups * group_elems is not representable (%lld x %lld)", n_groups, group_elems);
    VAD_ARG(vad_req_aligned(who, "values", values, 4));
    VAD_ARG(vad_req_float_labels(who, "labels", labels, label_format));
    VAD_ARG(vad_req_aligned(who, "state", state, 16));

    const hipStream_t s = (hipStream_t)stream;
    for (long long base = 0; base < total; base += HIST_LAUNCH_ELEMS) {
        const long long left = total - base;
        const unsigned n = (unsigned)(left < HIST_LAUNCH_ELEMS ? left : HIST_LAUNCH_ELEMS);
        HistP p;
        p.values = values + base;
        p.labels = label_format == VAD_LBL_U8_GROUP ? labels
                   : label_format == VAD_LBL_F32_ELEM ? (const void*)((const float*)labels + base)
                                                      : (const void*)((const unsigned char*)labels + base);
        p.state = (unsigned*)state;
        p.base = base;
        p.group_elems = group_elems;
        p.n = n;
        const unsigned to_aligned = (unsigned)((16 - ((uintptr_t)p.values & 15)) & 15) / 4;
        p.head = to_aligned < n ? to_aligned : n;
        p.quads = (n - p.head) / 4;
        p.fmt = label_format;
        p.m = m;
        p.lab_vec = 0;
        if (label_format == VAD_LBL_F32_ELEM) p.lab_vec = ((uintptr_t)((const float*)p.labels + p.head) % 16) == 0;
        if (label_format == VAD_LBL_U8_ELEM) p.lab_vec = ((uintptr_t)((const unsigned char*)p.labels + p.head) % 4) == 0;
        unsigned blocks = (p.quads + HIST_THREADS - 1) / HIST_THREADS;
        blocks = blocks < 1 ? 1 : (blocks > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : blocks);
        hipLaunchKernelGGL(hist_accumulate_kernel, dim3(blocks), dim3(HIST_THREADS), 0, s, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

int vad_hist_merge(void* dst, const void* src, int m, void* stream) {
    VAD_ARG(vad_req_mantissa("hist_merge", m));
    VAD_ARG(vad_req_nonnull("hist_merge", "dst", dst));
    VAD_ARG(vad_req_nonnull("hist_merge", "src", src));
    VAD_REQUIRE(vad_aligned(dst, 16) && vad_aligned(src, 16), "hist_merge: dst and src must be 16-byte aligned");
    VAD_REQUIRE(dst != src, "hist_merge: dst and src are the same state");
    const unsigned pairs = hist_nbins(m) + 1u;
    unsigned blocks = (pairs + 255u) / 256u;
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(hist_merge_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (unsigned*)dst, (const unsigned*)src, m);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
