// The labelling of a clip's volume [t, h, w] as the event kernels use it (csrc/map_events.hip, csrc/map_event_match.hip): one copy
// of what lies between the in-frame labelling of region_label.h and a table's slot pass - rebase, link, flatten, count -, of the
// launcher that runs them, and of the two argument checks that belong to a volume.  Any predicate the in-frame labeller takes goes
// through it: v >= threshold for the events, the mask formats for the ground-truth tracks.  Not part of the C ABI; the kernels have
// internal linkage, every file that includes this header launches its own.
//
//   rebase   labels of a frame -> parents inside the clip's volume (+ t * h * w); sizes and last frames cleared
//   link     every foreground pixel of a frame t > 0 unites with its counterparts of frame t - 1 (the walks of region_label.h, the
//            bound 2 * volume + 2).  temporal 1: the pixel behind it.  temporal 9 (8-connectivity): the pixel behind it when that
//            is set - its 3 x 3 is one set already -, otherwise one union per run of set pixels around the 3 x 3's ring (consecutive
//            ring pixels are neighbours inside their frame).  The union with the pixel behind is made on the two pixels' parents,
//            once per distinct pair of a wave: a blob over a blob costs a union per wave, not per pixel.
//   flatten  labels[p] = 1 + root (the smallest volume index of the component: canonical), sizes[root] += 1, last[root] = max t; a
//            lane gathers its pixels of one root over a run of EV_RUN pixels, equal roots of a wave are combined before the atomics
//            (wave_each_key of region_table.h)
//   count    a volume is cut into chunks of EV_CHUNK pixels; chunk c of clip b counts its kept roots (last - t0 + 1 >= min_duration
//            and sizes >= min_volume; t0 is the root's own frame) and its dropped roots into chunk_kept[b][c]
// Integer atomics, min and max only; no loop without a bound known at launch; a walk that runs out of its budget sets
// VAD_LABEL_FLAG_WALK in the flag word.
#pragma once
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int EV_THREADS = REGION_THREADS;
constexpr unsigned EV_CHUNK = REGION_CHUNK;
constexpr unsigned EV_RUN = 4096;               // pixels a work-group of the link, flatten and reduce / join passes takes at a time
constexpr unsigned EV_VOLUME_BLOCKS_X = 4096;    // rebase: 2^20 pixels of a clip per grid round
constexpr unsigned EV_SCAN_BLOCKS_X = 1024;      // count, slot: 2^20 pixels per round
constexpr unsigned EV_REDUCE_BLOCKS_X = 256;     // link, flatten, reduce / join: 2^20 pixels per round; the clips of a call fill the device
static_assert(EV_VOLUME_BLOCKS_X * EV_THREADS == EV_REDUCE_BLOCKS_X * EV_RUN, "the plans report one round for the passes over a volume");
constexpr int EV_MAX_EVENTS = 65536;

struct VolumeP {
    int* labels;             // [b][vol]: 0, or 1 + parent inside the clip's volume
    unsigned* sizes;         // [b][vol]: the volume at the root
    unsigned* aux;           // [b][vol]: the last frame at the root (a table's slot pass may put the root's slot in its place)
    unsigned* chunk_kept;    // [b][nchunks]
    unsigned* flags;
    long long b;
    unsigned vol, npix, nchunks, w, min_duration, min_volume;   // vol = t * npix < 2^31 - 1
    int temporal;
};

// per-frame labels -> parents inside the volume
__global__ __launch_bounds__(EV_THREADS) void events_rebase_kernel(VolumeP p) {
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const long long off = clip * (long long)p.vol;
        // i + the stride stays below 2^31 + 2^20: no wrap
        for (unsigned i = blockIdx.x * EV_THREADS + threadIdx.x; i < p.vol; i += gridDim.x * EV_THREADS) {
            const int lab = p.labels[off + i];
            const unsigned base = (i / p.npix) * p.npix;
            if (lab != 0) p.labels[off + i] = lab + (int)base;
            p.sizes[off + i] = 0u;
            p.aux[off + i] = 0u;
        }
    }
}

__global__ __launch_bounds__(EV_THREADS) void events_link_kernel(VolumeP p) {
    const unsigned w = p.w, npix = p.npix;
    const unsigned h = npix / w;
    const unsigned budget = 2u * p.vol + 2u;                 // fits: vol < 2^31 - 1
    const unsigned behind = p.vol - npix;                    // the pixels of the frames t > 0
    const unsigned nruns = (behind + EV_RUN - 1u) / EV_RUN;  // behind < 2^31: no wrap
    const unsigned lane = threadIdx.x & 63u;
    bool failed = false;
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        int* L = p.labels + clip * (long long)p.vol;
        unsigned seen_a = 0xffffffffu, seen_b = 0xffffffffu;   // the pair this lane met last: united by then (below)
        // the trip counts are the same for every lane of the work-group: the ballots below run in converged control flow
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x)
        for (unsigned j = 0; j < EV_RUN / EV_THREADS; ++j) {
            const u64 o = (u64)run * EV_RUN + j * EV_THREADS + threadIdx.x;
            const unsigned i = npix + (unsigned)o;           // read only where o < behind
            const bool fg = o < behind && L[i] != 0;         // whether a pixel is foreground never changes after the labelling
            const unsigned q = i - npix;                     // the same pixel of the frame before: the same clip, as i >= npix
            const bool direct = fg && L[q] != 0;
            // Uniting the two pixels' parents unites the pixels.  After the labelling a parent is the frame's root of the region, so
            // the lanes of a wave that sit in one region over one region hold the same pair: one union for the pair, by its first
            // lane.  wave_elect_pair only elects those lanes; the unions then run side by side.  A lane that meets the pair of its
            // previous pixel again - 256 pixels on in the same run, the same blob - skips it: that union was made, by this lane or
            // by the one elected for it, before the wave went on.
            const unsigned pa = direct ? (unsigned)label_load(L + i) - 1u : 0u, pb = direct ? (unsigned)label_load(L + q) - 1u : 0u;
            const bool pending = direct && (pa != seen_a || pb != seen_b);
            if (direct) {
                seen_a = pa;
                seen_b = pb;
            }
            if (wave_elect_pair(pending, pa, pb, lane)) {
                // the wave before may have made this union already: the same parent, or pb itself as pa's parent
                const unsigned ga = (unsigned)label_load(L + pa) - 1u, gb = (unsigned)label_load(L + pb) - 1u;
                if (ga != gb && ga != pb) failed |= !label_union(L, pa, pb, budget);
            }
            if (!fg || direct || p.temporal != 9) continue;
            const unsigned pix = i % npix;
            const unsigned y = pix / w, x = pix - y * w;
            // the set pixels of the ring of the 3 x 3 around q
            unsigned ring = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (ring_inside(y, x, h, w, k) && L[(int)q + ring_dy(k) * (int)w + ring_dx(k)] != 0) ring |= 1u << k;
            if (ring == 0xffu) ring = 1u;                    // a closed ring is one run
            else ring &= ~((ring << 1) | (ring >> 7));       // the first pixel of every run
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (ring & (1u << k)) failed |= !label_union(L, i, (unsigned)((int)q + ring_dy(k) * (int)w + ring_dx(k)), budget);
        }
    }
    if (failed) atomicOr(p.flags, VAD_LABEL_FLAG_WALK);
}

// Adds the lanes' gathered pixel counts and last frames to their roots: `pending` lanes hold a root, equal roots of the wave are
// combined first.
__device__ __forceinline__ void events_sizes_flush(bool pending, unsigned root, unsigned n, unsigned t, unsigned* S, unsigned* last,
                                                   unsigned lane) {
    wave_each_key(pending, root, lane, [&](unsigned first, bool mine, bool many, bool lead) {
        unsigned sum = mine ? n : 0u, latest = mine ? t : 0u;
        if (many) {
            sum = wave_sum(sum);
            latest = wave_max(latest);
        }
        if (lead) {
            atomicAdd(S + first, sum);
            atomicMax(last + first, latest);
        }
    });
}

__global__ __launch_bounds__(EV_THREADS) void events_flatten_kernel(VolumeP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;               // vol < 2^31 - 1: no wrap
    bool failed = false;
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        int* L = p.labels + clip * (long long)p.vol;
        unsigned* S = p.sizes + clip * (long long)p.vol;
        unsigned* last = p.aux + clip * (long long)p.vol;
        // a lane gathers the pixels of one root in registers: a run of 4096 pixels inside one event costs a wave two atomics
        unsigned acc_root = 0u, acc_n = 0u, acc_t = 0u;                  // acc_n == 0: nothing gathered
        // the trip counts are the same for every lane of the work-group: the ballots run in converged control flow
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {
            for (unsigned j = 0; j < EV_RUN / EV_THREADS; ++j) {
                const u64 i64 = (u64)run * EV_RUN + j * EV_THREADS + threadIdx.x;
                const unsigned i = (unsigned)i64;
                const bool fg = i64 < p.vol && L[i] != 0;
                unsigned root = 0u;
                if (fg) {
                    unsigned budget = p.vol + 1u;
                    root = label_find(L, i, budget);
                    failed |= budget == 0u;
                    // a root keeps its value; any other pixel gets an ancestor of its old parent, so concurrent chases stay valid
                    __hip_atomic_store(L + i, (int)(root + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                // another root than the one gathered so far: that one's pixels go out first
                const bool moved = fg && acc_n != 0u && root != acc_root;
                events_sizes_flush(moved, acc_root, acc_n, acc_t, S, last, lane);
                if (moved) acc_n = 0u;
                if (fg) {
                    acc_root = root;
                    ++acc_n;
                    acc_t = i / p.npix;                                  // a lane's pixels ascend: the latest frame is the largest
                }
            }
        }
        events_sizes_flush(acc_n != 0u, acc_root, acc_n, acc_t, S, last, lane);
    }
    if (failed) atomicOr(p.flags, VAD_LABEL_FLAG_WALK);
}

// is the root at volume index i, of `volume` pixels and last frame t1, kept?  (t0 is the root's own frame: it is the first voxel)
__device__ __forceinline__ bool events_kept(unsigned npix, unsigned min_duration, unsigned min_volume, unsigned i, unsigned volume, unsigned t1) {
    const unsigned t0 = i / npix;
    return volume >= min_volume && t1 - t0 + 1u >= min_duration;
}

// kept / dropped roots per chunk, packed into one word (a chunk holds at most EV_CHUNK of either)
static_assert(EV_CHUNK < 65536u, "kept and dropped roots of a chunk share a word");
__global__ __launch_bounds__(EV_THREADS) void events_count_kernel(VolumeP p) {
    __shared__ unsigned s_n[2];
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const int* L = p.labels + clip * (long long)p.vol;
        const unsigned* S = p.sizes + clip * (long long)p.vol;
        const unsigned* last = p.aux + clip * (long long)p.vol;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<2>(s_n);
            unsigned n[2] = {0u, 0u};                                    // kept, dropped
            for (unsigned j = 0; j < EV_CHUNK / EV_THREADS; ++j) {
                const unsigned i = c * EV_CHUNK + j * EV_THREADS + threadIdx.x;        // < 2^31 + 1024: no wrap
                if (i < p.vol && L[i] == (int)(i + 1u)) {
                    if (events_kept(p.npix, p.min_duration, p.min_volume, i, S[i], last[i])) ++n[0];
                    else ++n[1];
                }
            }
            block_sum(n, s_n);
            if (threadIdx.x == 0) p.chunk_kept[clip * (long long)p.nchunks + c] = n[0] | (n[1] << 16);
            __syncthreads();                                             // s_n is cleared again for the next chunk
        }
    }
}

// b >= 0, t, h, w >= 1, t * h * w < 2^31 - 1, b * t * h * w <= 2^38; *vol = t * h * w, *total = b * vol
inline bool events_dims_ok(long long b, int t, int h, int w, long long* vol, long long* total) {
    if (b < 0 || t < 1 || !vad_label_hw_ok(h, w)) return false;
    if (__builtin_mul_overflow((long long)t, (long long)h * w, vol) || *vol >= 2147483647ll) return false;
    return !__builtin_mul_overflow(b, *vol, total) && *total <= (1ll << 38);
}

// the two limits of a call's volumes, behind vad_req_label_n, vad_req_t and vad_req_label_hw
inline int events_req_volume(const char* who, long long b, int t, int h, int w, long long* vol, long long* total) {
    VAD_REQUIRE(!__builtin_mul_overflow((long long)t, (long long)h * w, vol) && *vol < 2147483647ll,
                "%s: t * h * w must be below 2^31 - 1 (%d x %d x %d)", who, t, h, w);
    VAD_REQUIRE(events_dims_ok(b, t, h, w, vol, total), "%s: b * t * h * w must be at most 2^38 (%lld x %d x %d x %d)", who, b, t, h, w);
    return VAD_OK;
}

// the link structure, behind vad_req_connectivity
inline int events_req_temporal(const char* who, int connectivity, int temporal) {
    VAD_REQUIRE(temporal == 1 || temporal == 9, "%s: temporal must be 1 or 9, got %d", who, temporal);
    VAD_REQUIRE(temporal == 1 || connectivity == 8, "%s: temporal 9 needs connectivity 8, got connectivity %d", who, connectivity);
    return VAD_OK;
}

inline unsigned events_grid_x(unsigned long long items, unsigned cap) { return (unsigned)(items < cap ? items : cap); }
inline unsigned events_grid_y(long long b) { return (unsigned)(b < 65535 ? b : 65535); }

// rebase, link, flatten, count on `s`, behind vad_label_launch on the b * t frames of p.labels: afterwards every foreground voxel
// holds 1 + its component's root, sizes and aux hold volume and last frame at the roots, chunk_kept the packed counts of the chunks
inline int events_volume_launch(const VolumeP& p, int t, hipStream_t s) {
    const unsigned gy = events_grid_y(p.b);
    const dim3 block(EV_THREADS);
    const dim3 volume_grid(events_grid_x(((unsigned long long)p.vol + EV_THREADS - 1) / EV_THREADS, EV_VOLUME_BLOCKS_X), gy);
    hipLaunchKernelGGL(events_rebase_kernel, volume_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    if (t > 1) {
        const unsigned long long behind = (unsigned long long)p.vol - p.npix;   // the pixels of the frames t > 0
        hipLaunchKernelGGL(events_link_kernel, dim3(events_grid_x((behind + EV_RUN - 1) / EV_RUN, EV_REDUCE_BLOCKS_X), gy), block, 0, s, p);
        VAD_LAUNCH_CHECK();
    }
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;
    hipLaunchKernelGGL(events_flatten_kernel, dim3(events_grid_x(nruns, EV_REDUCE_BLOCKS_X), gy), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(events_count_kernel, dim3(events_grid_x(p.nchunks, EV_SCAN_BLOCKS_X), gy), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

}  // namespace
