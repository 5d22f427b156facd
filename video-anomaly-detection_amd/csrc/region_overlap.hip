// Per-region overlap (PRO): connected-component labelling of ground-truth masks and the region-weighted score histogram the
// AUPRO of MVTec-style evaluations is computed from.  The reference loads the masks and only plots them
// (evaluate.py:142-171); here masks, error maps, labels and region sizes stay on the device and only the counters are read.
//
// Labelling: label equivalence by a union-find on the label plane itself.  labels[p] holds 0 for a normal pixel and otherwise
// 1 + (the index of p's parent inside its image); parents only ever decrease, a root is its own parent.
//   init     labels[p] = p + 1 for an anomalous pixel (every pixel its own root), 0 otherwise; sizes[p] = 0; flags = 0
//   merge    every anomalous pixel unites itself with the neighbours that precede it in raster order: find both roots, atomicMin
//            the smaller into the larger's parent, carry on from whatever stood there if another thread came first.  8-connectivity
//            needs one or two links per pixel, not four: with the pixel above set, left / above-left / above-right are already
//            tied to it by their own links; without it, left (or else above-left) and above-right.
//   flatten  labels[p] = 1 + root (the smallest index of the region: canonical), sizes[root] += 1 (equal roots of a wave combined)
// Every walk is bounded by a number known at launch.  A root chase visits strictly decreasing indices; a union replaces one of
// its two indices by a smaller one in every step (a step of a chase, or the parent another thread wrote), so it ends within
// 2 * h * w steps whatever the other threads do.  A walk that runs out of its budget sets LABEL_FLAG_WALK in the workspace's
// flag word and leaves: a defect gives an error (the Python layer raises on a set flag), never a spin.
// The three kernels are also what csrc/map_regions.hip labels thresholded anomaly maps with (region_label.h: vad_label_launch and an
// internal third predicate of the init kernel, v >= threshold, which the public entry points refuse like any unknown format).
//
// Histogram: the state is {u32 header[4]; u64 wpos[nbins], pos[nbins], neg[nbins]; u64 regions, max_region, rejected[2], flags}.
// pos / neg are the counters of score_hist.hip (its quantiser, its rejection rules, its wave + LDS combining: score_hist_lds.h).
// An anomalous pixel of region r also adds W(r) = (2^44 + |r| / 2) / |r| (integer division) to wpos[key]: sum_t wpos / (R * 2^44)
// is the mean overlap.  Weights do not fit the u32 LDS slots: equal (key, region) are combined within a wave, then added with one
// 64-bit global atomic.  Integer atomics only - the counters are exact and the same for any batching, order or sharding.
#include <hip/hip_runtime.h>

#include "region_label.h"
#include "score_hist_lds.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr unsigned PRO_MAGIC = 0x50444156u;    // "VADP"
constexpr int PRO_TAIL_WORDS = 5;              // regions, max_region, rejected[2], flags
constexpr int LABEL_THREADS = 256;
constexpr unsigned LABEL_MAX_BLOCKS_X = 4096;
constexpr unsigned LABEL_FLAG_WALK = VAD_LABEL_FLAG_WALK;   // a root chase or a union ran out of its step budget
constexpr unsigned LABEL_FLAG_SIZE = 2u;       // an anomalous pixel's region has size 0 (the label planes are not a labelling)
constexpr size_t WS_HEAD_BYTES = VAD_LABEL_WS_HEAD_BYTES;
static_assert(LABEL_MAX_BLOCKS_X * LABEL_THREADS == VAD_LABEL_ROUND_PIXELS, "region_label.h reports the labeller's grid round");

__device__ __forceinline__ bool pro_header_ok(const unsigned* hdr, int m) {
    return hdr[0] == PRO_MAGIC && hdr[1] == hist_tag(m) && hdr[2] == (unsigned)m;
}

struct LabelP {
    const void* masks;
    int* labels;
    unsigned* sizes;         // may be NULL
    unsigned* flags;
    long long n;
    unsigned npix;           // h * w < 2^31 - 1
    int w, fmt, conn;
    float threshold;         // VAD_LABEL_FMT_F32_GE only
};

// label_load, label_find, label_union - the bounded walks - live in region_label.h: csrc/map_events.hip unites with them too

__global__ __launch_bounds__(LABEL_THREADS) void label_init_kernel(LabelP p) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.flags[0] = 0u;
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const long long off = img * (long long)p.npix;
        for (unsigned i = blockIdx.x * LABEL_THREADS + threadIdx.x; i < p.npix; i += gridDim.x * LABEL_THREADS) {
            bool fg;
            if (p.fmt == VAD_LBL_U8_ELEM) fg = ((const unsigned char*)p.masks)[off + i] >= 128;
            else if (p.fmt == VAD_LABEL_FMT_F32_GE) fg = ((const float*)p.masks)[off + i] >= p.threshold;   // false for a NaN value
            else fg = ((const float*)p.masks)[off + i] > 0.5f;
            p.labels[off + i] = fg ? (int)(i + 1u) : 0;
            if (p.sizes != nullptr) p.sizes[off + i] = 0u;
        }
    }
}

__global__ __launch_bounds__(LABEL_THREADS) void label_merge_kernel(LabelP p) {
    const unsigned w = (unsigned)p.w;
    const unsigned budget = 2u * p.npix + 2u;                // fits: npix < 2^31 - 1
    bool failed = false;
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        int* L = p.labels + img * (long long)p.npix;
        for (unsigned i = blockIdx.x * LABEL_THREADS + threadIdx.x; i < p.npix; i += gridDim.x * LABEL_THREADS) {
            if (L[i] == 0) continue;                         // whether a pixel is anomalous never changes after the init pass
            const unsigned y = i / w, x = i - y * w;
            const bool left = x > 0u && L[i - 1u] != 0;
            const bool up = y > 0u && L[i - w] != 0;
            if (p.conn == 4) {
                if (left) failed |= !label_union(L, i, i - 1u, budget);
                if (up) failed |= !label_union(L, i, i - w, budget);
            } else if (up) {
                failed |= !label_union(L, i, i - w, budget);
            } else {
                const bool upleft = y > 0u && x > 0u && L[i - w - 1u] != 0;
                const bool upright = y > 0u && x + 1u < w && L[i - w + 1u] != 0;
                if (left) failed |= !label_union(L, i, i - 1u, budget);
                else if (upleft) failed |= !label_union(L, i, i - w - 1u, budget);
                if (upright) failed |= !label_union(L, i, i - w + 1u, budget);
            }
        }
    }
    if (failed) atomicOr(p.flags, LABEL_FLAG_WALK);
}

__global__ __launch_bounds__(LABEL_THREADS) void label_flatten_kernel(LabelP p) {
    const int lane = (int)(threadIdx.x & 63u);
    bool failed = false;
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        int* L = p.labels + img * (long long)p.npix;
        unsigned* S = p.sizes != nullptr ? p.sizes + img * (long long)p.npix : nullptr;
        // the trip count is the same for every lane of the work-group: the ballots below run in converged control flow
        for (unsigned base = blockIdx.x * LABEL_THREADS; base < p.npix; base += gridDim.x * LABEL_THREADS) {
            const unsigned i = base + threadIdx.x;
            const bool fg = i < p.npix && L[i] != 0;
            unsigned root = 0u;
            if (fg) {
                unsigned budget = p.npix + 1u;
                root = label_find(L, i, budget);
                failed |= budget == 0u;
                // a root keeps its value; any other pixel gets an ancestor of its old parent, so concurrent chases stay valid
                __hip_atomic_store(L + i, (int)(root + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (S == nullptr) continue;                      // uniform
            bool pending = fg;
            u64 left = __ballot(pending);
            while (left != 0) {                              // wave-uniform; every round retires at least the leading lane
                const int lead = __builtin_ctzll(left);
                const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)root, lead);
                const u64 same = __ballot(pending && root == first);
                if (lane == lead) atomicAdd(S + first, (unsigned)__builtin_popcountll(same));
                if (root == first) pending = false;
                left &= ~same;
            }
        }
    }
    if (failed) atomicOr(p.flags, LABEL_FLAG_WALK);
}

struct ProP {
    const float* values;
    const int* labels;
    const unsigned* sizes;
    const unsigned* flags;
    unsigned* state;
    long long total;         // n * h * w
    unsigned npix;
    int m;
};

__global__ __launch_bounds__(HIST_THREADS) void pro_hist_kernel(ProP p) {
    if (!pro_header_ok(p.state, p.m)) return;                // uniform over the grid: not this m's blob, nothing is touched
    __shared__ HistLds s;
    __shared__ unsigned s_regions, s_max;
    for (int i = threadIdx.x; i < HIST_SLOTS; i += HIST_THREADS) {
        s.tag[i] = 0u;
        s.cnt[i] = 0u;
    }
    if (threadIdx.x < 2) s.rej[threadIdx.x] = 0u;
    if (threadIdx.x == 0) s_regions = s_max = 0u;
    __syncthreads();

    const unsigned nbins = hist_nbins(p.m);
    const int shift = 23 - p.m;
    u64* wpos = (u64*)(p.state + 4);
    u64* counts = wpos + nbins;                              // two rows of the LDS table's bins: anomalous, then normal
    u64* tail = wpos + 3ull * nbins;
    const int lane = (int)(threadIdx.x & 63u);
    unsigned rej_n = 0u, rej_p = 0u, regions = 0u, max_region = 0u;
    bool bad_size = false;

    // a work-group takes one contiguous run; the trip count is the same for all its lanes (converged ballots)
    const u64 total = (u64)p.total;
    const u64 per = (total + gridDim.x - 1) / gridDim.x;
    const u64 lo = blockIdx.x * per < total ? blockIdx.x * per : total;
    const u64 hi = lo + per < total ? lo + per : total;
    for (u64 base = lo; base < hi; base += HIST_THREADS) {
        const u64 i = base + threadIdx.x;
        const bool valid = i < hi;
        const float v = valid ? p.values[i] : 0.f;
        const int lab = valid ? p.labels[i] : 0;
        const bool pos = lab != 0;
        unsigned bits = __float_as_uint(v);
        if (bits == 0x80000000u) bits = 0u;                  // -0.0 is 0
        const bool ok = valid && bits < 0x7f800000u;         // finite and >= 0
        rej_n += (valid && !ok && !pos) ? 1u : 0u;
        rej_p += (valid && !ok && pos) ? 1u : 0u;
        const unsigned key = bits >> shift;

        // pos[key] / neg[key]: the unweighted counters, through the work-group's table
        const unsigned bin = ok ? (pos ? 0u : nbins) + key : 0u;
        const u64 act = __ballot(ok);
        if (act != 0) {                                      // wave-uniform
            const int lead = __builtin_ctzll(act);
            const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)bin, lead);
            if (__ballot(ok && bin == first) == act)         // every binned lane holds the same bin: one add for the instruction
                hist_lds_add(s, counts, nbins, first, (unsigned)__builtin_popcountll(act), lane == lead);
            else
                hist_lds_add(s, counts, nbins, bin, 1u, ok);
        }

        // the region of an anomalous pixel: its root's index in the whole batch, and the root's size
        u64 root = 0;
        unsigned size = 0u;
        if (pos) {
            const u64 img = i / p.npix;
            root = img * p.npix + (u64)(unsigned)(lab - 1);
            size = root < total ? p.sizes[root] : 0u;
            if (root == i) {                                 // a region is counted at its root, binned or not
                ++regions;
                max_region = size > max_region ? size : max_region;
            }
            bad_size |= size == 0u;
        }
        const unsigned root_lo = (unsigned)root, root_hi = (unsigned)(root >> 32);
        bool pending = ok && pos && size != 0u;
        u64 left = __ballot(pending);
        // W(r): a 64-bit division, done by all lanes at once in front of the loop - inside it, by one lane per round, the rounds
        // of a wave that crosses a region's row (as many as the row has distinct keys) ran one after the other
        u64 weight = 0;
        if (left != 0) {                                     // wave-uniform
            const unsigned d = pending ? size : 1u;
            weight = ((1ull << VAD_PRO_WEIGHT_BITS) + d / 2u) / d;
        }
        while (left != 0) {                                  // wave-uniform: one distinct (key, region) per round
            const int lead = __builtin_ctzll(left);
            const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)key, lead);
            const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)root_lo, lead);
            const unsigned r1 = (unsigned)__builtin_amdgcn_readlane((int)root_hi, lead);
            const bool mine = pending && key == k0 && root_lo == r0 && root_hi == r1;
            const u64 same = __ballot(mine);
            if (lane == lead) atomicAdd(wpos + k0, weight * (u64)__builtin_popcountll(same));
            if (mine) pending = false;
            left &= ~same;
        }
    }

    if (rej_n) atomicAdd(&s.rej[0], rej_n);
    if (rej_p) atomicAdd(&s.rej[1], rej_p);
    if (regions) atomicAdd(&s_regions, regions);
    if (max_region) atomicMax(&s_max, max_region);
    if (bad_size) atomicOr(tail + 4, (u64)LABEL_FLAG_SIZE);
    __syncthreads();
    for (int i = threadIdx.x; i < HIST_SLOTS; i += HIST_THREADS) {
        const unsigned t = s.tag[i];
        if (t != 0u) atomicAdd(&counts[t - 1u], (u64)s.cnt[i]);
    }
    if (threadIdx.x == 0) {
        if (s_regions != 0u) atomicAdd(tail + 0, (u64)s_regions);
        if (s_max != 0u) atomicMax(tail + 1, (u64)s_max);
        if (s.rej[0] != 0u) atomicAdd(tail + 2, (u64)s.rej[0]);
        if (s.rej[1] != 0u) atomicAdd(tail + 3, (u64)s.rej[1]);
        if (blockIdx.x == 0 && p.flags[0] != 0u) atomicOr(tail + 4, (u64)p.flags[0]);   // what the labelling passes reported
    }
}

__global__ void pro_header_kernel(unsigned* state, int m) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *(u32x4*)state = u32x4{PRO_MAGIC, hist_tag(m), (unsigned)m, 0u};
}

// dst (+)= src behind the headers: sums, the maximum for max_region, the union for flags.
__global__ __launch_bounds__(256) void pro_merge_kernel(unsigned* dst, const unsigned* src, int m) {
    if (!pro_header_ok(dst, m) || !pro_header_ok(src, m)) return;
    const unsigned nb3 = 3u * hist_nbins(m), words = nb3 + PRO_TAIL_WORDS;
    u64* d = (u64*)(dst + 4);
    const u64* s = (const u64*)(src + 4);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < words; i += gridDim.x * 256u) {
        if (i == nb3 + 1u) d[i] = d[i] > s[i] ? d[i] : s[i];
        else if (i == nb3 + 4u) d[i] |= s[i];
        else d[i] += s[i];
    }
}

// The checks the two labelling entry points share; *total = n * h * w.
int label_args(const char* fn, const void* masks, int label_format, long long n, int h, int w, int connectivity, long long* total) {
    VAD_ARG(vad_req_masks(fn, masks, "label_format", label_format));
    VAD_ARG(vad_req_label_n(fn, "n", n));
    VAD_ARG(vad_req_label_hw(fn, h, w));
    VAD_ARG(vad_req_connectivity(fn, connectivity));
    return vad_req_label_total(fn, n, h, w, total);
}

}  // namespace

int vad_label_launch(const void* masks, int fmt, float threshold, long long n, int h, int w, int conn, int* labels, unsigned* sizes,
                     unsigned* flags, hipStream_t s) {
    LabelP p;
    p.masks = masks;
    p.labels = labels;
    p.sizes = sizes;
    p.flags = flags;
    p.n = n;
    p.npix = (unsigned)h * (unsigned)w;
    p.w = w;
    p.fmt = fmt;
    p.conn = conn;
    p.threshold = threshold;
    unsigned bx = (p.npix + LABEL_THREADS - 1) / LABEL_THREADS;
    if (bx > LABEL_MAX_BLOCKS_X) bx = LABEL_MAX_BLOCKS_X;
    const dim3 grid(bx, (unsigned)(n < 65535 ? n : 65535));
    hipLaunchKernelGGL(label_init_kernel, grid, dim3(LABEL_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_merge_kernel, grid, dim3(LABEL_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(label_flatten_kernel, grid, dim3(LABEL_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

size_t vad_pro_state_bytes(int m) {
    if (!vad_hist_m_ok(m)) return 0;
    return 16 + 8 * (3 * (size_t)hist_nbins(m) + PRO_TAIL_WORDS);
}

int vad_pro_reset(void* state, int m, void* stream) {
    VAD_ARG(vad_req_mantissa("pro_reset", m));
    VAD_ARG(vad_req_ptr("pro_reset", "state", state, 16));
    const hipStream_t s = (hipStream_t)stream;
    VAD_HIP_TRY(hipMemsetAsync(state, 0, vad_pro_state_bytes(m), s));
    hipLaunchKernelGGL(pro_header_kernel, dim3(1), dim3(64), 0, s, (unsigned*)state, m);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

int vad_pro_merge(void* dst, const void* src, int m, void* stream) {
    VAD_ARG(vad_req_mantissa("pro_merge", m));
    VAD_ARG(vad_req_nonnull("pro_merge", "dst", dst));
    VAD_ARG(vad_req_nonnull("pro_merge", "src", src));
    VAD_REQUIRE(vad_aligned(dst, 16) && vad_aligned(src, 16), "pro_merge: dst and src must be 16-byte aligned");
    VAD_REQUIRE(dst != src, "pro_merge: dst and src are the same state");
    const unsigned words = 3u * hist_nbins(m) + PRO_TAIL_WORDS;
    unsigned blocks = (words + 255u) / 256u;
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(pro_merge_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (unsigned*)dst, (const unsigned*)src, m);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

size_t vad_pro_workspace_bytes(long long n, int h, int w) {
    long long total = 0;
    if (!vad_label_dims_ok(n, h, w, &total)) return 0;
    return WS_HEAD_BYTES + 8 * (size_t)total;                // the flag word; an int32 label and a uint32 size per pixel
}

int vad_label_regions(const void* masks, int label_format, long long n, int h, int w, int connectivity, int32_t* labels,
                      uint32_t* sizes_or_null, void* ws, size_t ws_bytes, void* stream) {
    long long total = 0;
    VAD_ARG(label_args("label_regions", masks, label_format, n, h, w, connectivity, &total));
    VAD_ARG(vad_req_nonnull("label_regions", "labels", labels));
    VAD_REQUIRE(vad_aligned(labels, 4) && vad_aligned(sizes_or_null, 4), "label_regions: labels and sizes must be 4-byte aligned");
    VAD_ARG(vad_req_ptr("label_regions", "ws", ws, 16));
    VAD_REQUIRE_WS(VAD_ERR_ARG, "label_regions", ws_bytes, vad_pro_workspace_bytes(n, h, w), "vad_pro_workspace_bytes(%lld, %d, %d)", n, h, w);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {                                            // nothing to label: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    return vad_label_launch(masks, label_format, 0.f, n, h, w, connectivity, labels, sizes_or_null, (unsigned*)ws, s);
}

int vad_pro_accumulate(const float* values, const void* masks, int label_format, long long n, int h, int w, int connectivity,
                       void* state, int m, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "pro_accumulate";
    VAD_ARG(vad_req_mantissa(who, m));
    VAD_ARG(vad_req_ptr(who, "values", values, 4));
    long long total = 0;
    VAD_ARG(label_args(who, masks, label_format, n, h, w, connectivity, &total));
    VAD_ARG(vad_req_ptr(who, "state", state, 16));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    VAD_REQUIRE_WS(VAD_ERR_ARG, who, ws_bytes, vad_pro_workspace_bytes(n, h, w), "vad_pro_workspace_bytes(%lld, %d, %d)", n, h, w);
    if (n == 0) return VAD_OK;
    const hipStream_t s = (hipStream_t)stream;
    unsigned* flags = (unsigned*)ws;
    int* labels = (int*)((char*)ws + WS_HEAD_BYTES);
    unsigned* sizes = (unsigned*)(labels + total);
    if (int rc = vad_label_launch(masks, label_format, 0.f, n, h, w, connectivity, labels, sizes, flags, s)) return rc;
    ProP p;
    p.values = values;
    p.labels = labels;
    p.sizes = sizes;
    p.flags = flags;
    p.state = (unsigned*)state;
    p.total = total;
    p.npix = (unsigned)h * (unsigned)w;
    p.m = m;
    long long blocks = (total + HIST_THREADS - 1) / HIST_THREADS;
    if (blocks > HIST_MAX_BLOCKS) blocks = HIST_MAX_BLOCKS;
    hipLaunchKernelGGL(pro_hist_kernel, dim3((unsigned)blocks), dim3(HIST_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
