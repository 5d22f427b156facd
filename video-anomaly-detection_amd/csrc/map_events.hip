// Anomaly events of a clip: the connected components of {v >= threshold} in the volume [t, h, w] of every clip - regions linked
// across frames - as a table of records: root, volume, first and last frame, union box, peak and its position, coordinate sums, in
// ascending order of their first voxel.  A deployed line alarms on events that persist, not on the blob of
// one frame; the host route copies every map of the clip and runs scipy.ndimage label with a 3-D structure, find_objects and
// maximum_position.  Here the maps stay on the device and the table is what leaves it.
//
//   label    the union-find of csrc/region_overlap.hip through region_label.h on the b * t frames as it stands: every foreground
//            pixel then hangs directly under its frame's root, so the unions in time that follow are short
//   rebase   labels of a frame -> parents inside the clip's volume (+ t * h * w); sizes and last frames cleared
//   link     every foreground pixel of a frame t > 0 unites with its counterparts of frame t - 1 (the walks of region_label.h, the
//            bound 2 * volume + 2).  temporal 1: the pixel behind it.  temporal 9 (8-connectivity): the pixel behind it when that
//            is set - its 3 x 3 is one set already -, otherwise one union per run of set pixels around the 3 x 3's ring (consecutive
//            ring pixels are neighbours inside their frame).  The union with the pixel behind is made on the two pixels' parents,
//            once per distinct pair of a wave: a blob over a blob costs a union per wave, not per pixel.
//   flatten  labels[p] = 1 + root (the smallest volume index of the event: canonical), sizes[root] += 1, last[root] = max t; a lane
//            gathers its pixels of one root over a run of EV_RUN pixels, equal roots of a wave are combined before the atomics
//            (wave_each_key of region_table.h, as in every flush below)
//   count    a volume is cut into chunks of EV_CHUNK pixels; chunk c of clip b counts its kept roots (last - t0 + 1 >= min_duration
//            and sizes >= min_volume; t0 is the root's own frame) and its dropped roots into chunk_kept[b][c]
//   slot     the rank of a kept root = the kept roots of the chunks before it + those in front of it inside its chunk (block_sum,
//            chunk_rank_row of region_table.h): ascending
//            roots across the whole volume.  A root of rank r < max_events gets slot r + 1 and its record's first words and the
//            identities of the reductions; a kept root behind the table gets EV_SLOT_NO_RECORD (its pixels still count as kept);
//            any other root gets 0.  The slot takes the place of the root's last frame, which its record now holds.  The
//            work-group of a clip's last chunk has summed the whole clip: it writes counts[b][0 / 1].
//   reduce   every foreground pixel whose root has a record contributes x, y, t, (key(v) << 32 | ~index) to it - gathered per lane,
//            combined per wave, eight integer atomics per group - and every pixel counts into its frame's three words.
//   finish   the records in use get their peak word split into float bits and index; every other record of the table is zeroed.
// Integer atomics, min and max only: every output is the same words for any batching, launch order or tiling.  Every launch is
// asynchronous on the caller's stream, nothing is allocated, the host never waits.  No loop without a bound known at launch.
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int EV_THREADS = REGION_THREADS;
constexpr unsigned EV_CHUNK = REGION_CHUNK;
constexpr unsigned EV_RUN = 4096;               // pixels a work-group of the link, flatten and reduce passes takes at a time
constexpr unsigned EV_VOLUME_BLOCKS_X = 4096;    // rebase: 2^20 pixels of a clip per grid round
constexpr unsigned EV_SCAN_BLOCKS_X = 1024;      // count, slot: 2^20 pixels per round
constexpr unsigned EV_REDUCE_BLOCKS_X = 256;     // link, flatten, reduce: 2^20 pixels per round; the clips of a call fill the device
static_assert(EV_VOLUME_BLOCKS_X * EV_THREADS == EV_REDUCE_BLOCKS_X * EV_RUN, "vad_events_plan reports one round for the passes over a volume");
constexpr int EV_MAX_EVENTS = 65536;
constexpr unsigned EV_SLOT_NO_RECORD = 0xffffffffu;

struct EventP {
    const float* maps;
    int* labels;             // [b][vol]: 0, or 1 + parent inside the clip's volume
    unsigned* sizes;         // [b][vol]: the volume at the root
    unsigned* aux;           // [b][vol]: the last frame at the root; from the slot pass on, the root's slot
    unsigned* chunk_kept;    // [b][nchunks]
    unsigned* records;       // [b][max_events][VAD_EVENT_WORDS]
    unsigned* counts;        // [b][4]: kept, dropped, foreground pixels, NaN pixels
    unsigned* frame_counts;  // [b][t][3]: foreground pixels, pixels of kept events, NaN pixels
    unsigned* flags;
    long long b;
    unsigned vol, npix, nchunks, w, t, min_duration, min_volume, max_events;   // vol = t * npix < 2^31 - 1
    int conn, temporal;
};

// per-frame labels -> parents inside the volume
__global__ __launch_bounds__(EV_THREADS) void events_rebase_kernel(EventP p) {
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

__global__ __launch_bounds__(EV_THREADS) void events_link_kernel(EventP p) {
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

__global__ __launch_bounds__(EV_THREADS) void events_flatten_kernel(EventP p) {
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
__device__ __forceinline__ bool events_kept(const EventP& p, unsigned i, unsigned volume, unsigned t1) {
    const unsigned t0 = i / p.npix;
    return volume >= p.min_volume && t1 - t0 + 1u >= p.min_duration;
}

// kept / dropped roots per chunk, packed into one word (a chunk holds at most EV_CHUNK of either)
static_assert(EV_CHUNK < 65536u, "kept and dropped roots of a chunk share a word");
__global__ __launch_bounds__(EV_THREADS) void events_count_kernel(EventP p) {
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
                    if (events_kept(p, i, S[i], last[i])) ++n[0];
                    else ++n[1];
                }
            }
            block_sum(n, s_n);
            if (threadIdx.x == 0) p.chunk_kept[clip * (long long)p.nchunks + c] = n[0] | (n[1] << 16);
            __syncthreads();                                             // s_n is cleared again for the next chunk
        }
    }
}

// ranks of the kept roots in ascending order; the records' first words and the identities of the reductions
__global__ __launch_bounds__(EV_THREADS) void events_slot_kernel(EventP p) {
    __shared__ unsigned s_sum[2], s_wave[1][REGION_WAVES];
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const int* L = p.labels + clip * (long long)p.vol;
        const unsigned* S = p.sizes + clip * (long long)p.vol;
        unsigned* aux = p.aux + clip * (long long)p.vol;
        const unsigned* kept_of = p.chunk_kept + clip * (long long)p.nchunks;
        unsigned* rec = p.records + (u64)clip * p.max_events * VAD_EVENT_WORDS;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<2>(s_sum);
            // the clip's last chunk also sums the whole clip: its work-group writes the clip's kept / dropped counts, no atomics
            const bool last_chunk = c + 1u == p.nchunks;
            unsigned sum[2] = {0u, 0u};                                  // the kept roots in front of the chunk; the dropped ones
            for (unsigned k = threadIdx.x; k < c + (last_chunk ? 1u : 0u); k += EV_THREADS) {
                const unsigned v = kept_of[k];
                sum[0] += k < c ? v & 0xffffu : 0u;
                sum[1] += v >> 16;
            }
            block_sum(sum, s_sum);
            unsigned base = sum[0];
            if (last_chunk && threadIdx.x == 0) {
                p.counts[clip * 4] = base + (kept_of[c] & 0xffffu);
                p.counts[clip * 4 + 1] = sum[1];
            }
            for (unsigned j = 0; j < EV_CHUNK / EV_THREADS; ++j) {
                const unsigned i = c * EV_CHUNK + j * EV_THREADS + threadIdx.x;
                const bool root = i < p.vol && L[i] == (int)(i + 1u);
                const unsigned volume = root ? S[i] : 0u;
                const unsigned t1 = root ? aux[i] : 0u;
                const bool kept = root && events_kept(p, i, volume, t1);
                const unsigned rank = chunk_rank_row(kept, base, s_wave);
                if (kept && rank < p.max_events) {
                    aux[i] = rank + 1u;
                    unsigned* r = rec + (u64)rank * VAD_EVENT_WORDS;
                    *(u32x4*)r = u32x4{i, volume, i / p.npix, t1};                   // root, volume, t0, t1
                    *(u32x4*)(r + 4) = u32x4{0xffffffffu, 0xffffffffu, 0u, 0u};     // x0, y0 (min), x1, y1 (max)
                    *(u32x4*)(r + 8) = u32x4{0u, 0u, 0u, 0u};                       // the 64-bit peak word (max), sum x
                    *(u32x4*)(r + 12) = u32x4{0u, 0u, 0u, 0u};                      // sum y, sum t
                } else if (root) {
                    aux[i] = kept ? EV_SLOT_NO_RECORD : 0u;
                }
            }
        }
    }
}

// Adds the lanes' gathered values (sw: the sum of the frames) to their records: `pending` lanes hold a slot in 1 .. max_events,
// equal slots of the wave are combined first.
__device__ __forceinline__ void events_flush(bool pending, const RegionAcc<u64>& a, unsigned* rec, unsigned lane) {
    wave_each_key(pending, a.slot, lane, [&](unsigned first, bool mine, bool many, bool lead) {
        const RegionAcc<u64> c = a.combined(mine, many);
        if (lead) {
            unsigned* r = rec + (u64)(first - 1u) * VAD_EVENT_WORDS;
            c.commit(r, 4, 8, 10);
            atomicAdd((u64*)(r + 14), c.sw);
        }
    });
}

// Adds the lanes' counts of one frame each (`pending` lanes: frame < p.t) to frame_counts; equal frames of the wave are combined
// first.
__device__ __forceinline__ void events_frames_flush(bool pending, unsigned frame, unsigned nfg, unsigned nkept, unsigned nnan, unsigned* fc,
                                                    unsigned lane) {
    wave_each_key(pending, frame, lane, [&](unsigned first, bool mine, bool, bool lead) {
        const unsigned f = wave_sum(mine ? nfg : 0u), k = wave_sum(mine ? nkept : 0u), n = wave_sum(mine ? nnan : 0u);
        if (lead) {
            unsigned* r = fc + (u64)first * 3u;
            if (f) atomicAdd(r, f);
            if (k) atomicAdd(r + 1, k);
            if (n) atomicAdd(r + 2, n);
        }
    });
}

__global__ __launch_bounds__(EV_THREADS) void events_reduce_kernel(EventP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;               // vol < 2^31 - 1: no wrap
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const float* V = p.maps + clip * (long long)p.vol;
        const int* L = p.labels + clip * (long long)p.vol;
        const unsigned* slots = p.aux + clip * (long long)p.vol;
        unsigned* rec = p.records + (u64)clip * p.max_events * VAD_EVENT_WORDS;
        unsigned* fc = p.frame_counts + (u64)clip * p.t * 3u;
        RegionAcc<u64> acc;                                              // sw: the sum of the frames
        acc.clear();
        unsigned nfg = 0u, nnan = 0u;                                    // of the clip
        unsigned frame = 0u, ffg = 0u, fkept = 0u, fnan = 0u;            // of the frame this lane is in
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {  // uniform over the work-group
            for (unsigned j = 0; j < EV_RUN / EV_THREADS; ++j) {         // the same trip count for every lane: converged ballots
                const u64 i64 = (u64)run * EV_RUN + j * EV_THREADS + threadIdx.x;
                const bool valid = i64 < p.vol;
                const unsigned i = (unsigned)i64;
                const unsigned bits = valid ? __float_as_uint(V[i]) : 0u;
                const int lab = valid ? L[i] : 0;
                const unsigned t = valid ? i / p.npix : frame;
                const bool isnan = (bits & 0x7fffffffu) > 0x7f800000u;
                unsigned slot = 0u;
                if (lab != 0) {
                    const unsigned root = (unsigned)lab - 1u;
                    slot = root < p.vol ? slots[root] : 0u;              // a label is a root of this clip: always inside
                }
                // another frame than the one counted so far: that one's counts go out first
                const bool moved = t != frame;
                events_frames_flush(moved && (ffg | fkept | fnan) != 0u, frame, ffg, fkept, fnan, fc, lane);
                if (moved) {
                    frame = t;
                    ffg = fkept = fnan = 0u;
                }
                nnan += isnan ? 1u : 0u;
                nfg += lab != 0 ? 1u : 0u;
                fnan += isnan ? 1u : 0u;
                ffg += lab != 0 ? 1u : 0u;
                fkept += slot != 0u ? 1u : 0u;                           // kept, with a record or behind the table
                if (slot > p.max_events) slot = 0u;                      // no record: no address is formed from it
                // another event than the one gathered so far: that one goes to its record first
                events_flush(acc.slot != 0u && slot != 0u && slot != acc.slot, acc, rec, lane);
                if (slot != 0u) {
                    const unsigned pix = i - t * p.npix;
                    const unsigned y = pix / p.w, x = pix - y * p.w;
                    acc.add(slot, x, y, ((u64)order_key(bits) << 32) | (u64)(~i), (u64)t);
                }
            }
        }
        events_flush(acc.slot != 0u, acc, rec, lane);
        events_frames_flush((ffg | fkept | fnan) != 0u, frame, ffg, fkept, fnan, fc, lane);
        nfg = wave_sum(nfg);
        nnan = wave_sum(nnan);
        if (lane == 0u) {
            if (nfg) atomicAdd(p.counts + clip * 4 + 2, nfg);
            if (nnan) atomicAdd(p.counts + clip * 4 + 3, nnan);
        }
    }
}

// the peak word of a record in use -> float bits, index; every record behind the clip's last one -> zeros
__global__ __launch_bounds__(EV_THREADS) void events_finish_kernel(EventP p) {
    const u64 total = (u64)p.b * p.max_events;
    for (u64 k = (u64)blockIdx.x * EV_THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * EV_THREADS) {
        const u64 clip = k / p.max_events;
        const unsigned r = (unsigned)(k - clip * p.max_events);
        unsigned* rec = p.records + k * VAD_EVENT_WORDS;
        if (r < p.counts[clip * 4]) {                                    // kept may exceed max_events; r does not
            const unsigned not_index = rec[8], key = rec[9];
            rec[8] = order_key_inv(key);
            rec[9] = ~not_index;
        } else {
            *(u32x4*)rec = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(rec + 4) = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(rec + 8) = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(rec + 12) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

// b >= 0, t, h, w >= 1, t * h * w < 2^31 - 1, b * t * h * w <= 2^38; *vol = t * h * w, *total = b * vol
bool events_dims_ok(long long b, int t, int h, int w, long long* vol, long long* total) {
    if (b < 0 || t < 1 || !vad_label_hw_ok(h, w)) return false;
    if (__builtin_mul_overflow((long long)t, (long long)h * w, vol) || *vol >= 2147483647ll) return false;
    return !__builtin_mul_overflow(b, *vol, total) && *total <= (1ll << 38);
}

unsigned events_grid_x(unsigned long long items, unsigned cap) { return (unsigned)(items < cap ? items : cap); }

}  // namespace

size_t vad_events_workspace_bytes(long long b, int t, int h, int w, int labels_given) {
    long long vol = 0, total = 0;
    if (!events_dims_ok(b, t, h, w, &vol, &total) || (labels_given != 0 && labels_given != 1)) return 0;
    return region_head_bytes(b, vol, 1) + (size_t)(labels_given ? 8 : 12) * (size_t)total;   // [labels,] sizes, last / slots: 4 bytes each
}

int vad_events_plan(int* label_round, int* volume_round, int* scan_round, int* reduce_round, int* threads) {
    VAD_REQUIRE(label_round && volume_round && scan_round && reduce_round && threads, "events_plan: an output pointer is NULL");
    *label_round = (int)VAD_LABEL_ROUND_PIXELS;
    *volume_round = (int)(EV_VOLUME_BLOCKS_X * EV_THREADS);
    *scan_round = (int)(EV_SCAN_BLOCKS_X * EV_CHUNK);
    *reduce_round = (int)(EV_REDUCE_BLOCKS_X * EV_RUN);
    *threads = EV_THREADS;
    return VAD_OK;
}

int vad_detect_events(const float* maps, long long b, int t, int h, int w, float threshold, int connectivity, int temporal,
                      unsigned min_duration, unsigned min_volume, int max_events, int32_t* labels_or_null, uint32_t* records,
                      uint32_t* counts, uint32_t* frame_counts, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "detect_events";
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_label_n(who, "b", b));
    VAD_ARG(vad_req_t(who, t));
    VAD_ARG(vad_req_label_hw(who, h, w));
    long long vol = 0, total = 0;
    VAD_REQUIRE(!__builtin_mul_overflow((long long)t, (long long)h * w, &vol) && vol < 2147483647ll,
                "detect_events: t * h * w must be below 2^31 - 1 (%d x %d x %d)", t, h, w);
    VAD_REQUIRE(events_dims_ok(b, t, h, w, &vol, &total), "detect_events: b * t * h * w must be at most 2^38 (%lld x %d x %d x %d)", b, t, h, w);
    VAD_ARG(vad_req_threshold(who, threshold));
    VAD_ARG(vad_req_connectivity(who, connectivity));
    VAD_REQUIRE(temporal == 1 || temporal == 9, "detect_events: temporal must be 1 or 9, got %d", temporal);
    VAD_REQUIRE(temporal == 1 || connectivity == 8, "detect_events: temporal 9 needs connectivity 8, got connectivity %d", connectivity);
    VAD_ARG(vad_req_nonzero(who, "min_duration", min_duration));
    VAD_ARG(vad_req_nonzero(who, "min_volume", min_volume));
    VAD_ARG(vad_req_capacity(who, "max_events", max_events, EV_MAX_EVENTS));
    VAD_ARG(vad_req_aligned(who, "labels", labels_or_null, 4));
    VAD_ARG(vad_req_ptr(who, "records", records, 16));
    VAD_ARG(vad_req_ptr(who, "counts", counts, 4));
    VAD_ARG(vad_req_ptr(who, "frame_counts", frame_counts, 4));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    const int given = labels_or_null != nullptr ? 1 : 0;
    VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, vad_events_workspace_bytes(b, t, h, w, given), "vad_events_workspace_bytes(%lld, %d, %d, %d, %d)", b, t, h, w, given);
    const hipStream_t s = (hipStream_t)stream;
    if (b == 0) {                                            // nothing to detect: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, VAD_LABEL_WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    unsigned* flags = (unsigned*)ws;
    unsigned* planes = (unsigned*)((char*)ws + region_head_bytes(b, vol, 1));
    int* labels = given ? labels_or_null : (int*)planes;
    unsigned* sizes = given ? planes : planes + total;
    // inside the frames: the labeller as it stands, on b * t frames (its flatten pass leaves every pixel directly under its root)
    if (int rc = vad_label_launch(maps, VAD_LABEL_FMT_F32_GE, threshold, b * t, h, w, connectivity, labels, nullptr, flags, s)) return rc;

    EventP p;
    p.maps = maps;
    p.labels = labels;
    p.sizes = sizes;
    p.aux = sizes + total;
    p.chunk_kept = (unsigned*)((char*)ws + VAD_LABEL_WS_HEAD_BYTES);
    p.records = records;
    p.counts = counts;
    p.frame_counts = frame_counts;
    p.flags = flags;
    p.b = b;
    p.vol = (unsigned)vol;
    p.npix = (unsigned)h * (unsigned)w;
    p.nchunks = region_chunks(vol);
    p.w = (unsigned)w;
    p.t = (unsigned)t;
    p.min_duration = min_duration;
    p.min_volume = min_volume;
    p.max_events = (unsigned)max_events;
    p.conn = connectivity;
    p.temporal = temporal;
    VAD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)b * 16, s));
    VAD_HIP_TRY(hipMemsetAsync(frame_counts, 0, (size_t)b * (size_t)t * 12, s));
    const unsigned gy = (unsigned)(b < 65535 ? b : 65535);
    const dim3 block(EV_THREADS);
    const dim3 volume_grid(events_grid_x(((unsigned long long)vol + EV_THREADS - 1) / EV_THREADS, EV_VOLUME_BLOCKS_X), gy);
    hipLaunchKernelGGL(events_rebase_kernel, volume_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    if (t > 1) {
        const unsigned long long behind = (unsigned long long)vol - p.npix;   // the pixels of the frames t > 0
        hipLaunchKernelGGL(events_link_kernel, dim3(events_grid_x((behind + EV_RUN - 1) / EV_RUN, EV_REDUCE_BLOCKS_X), gy), block, 0, s, p);
        VAD_LAUNCH_CHECK();
    }
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;
    const dim3 run_grid(events_grid_x(nruns, EV_REDUCE_BLOCKS_X), gy);
    hipLaunchKernelGGL(events_flatten_kernel, run_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    const dim3 scan_grid(events_grid_x(p.nchunks, EV_SCAN_BLOCKS_X), gy);
    hipLaunchKernelGGL(events_count_kernel, scan_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(events_slot_kernel, scan_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(events_reduce_kernel, run_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned long long recs = (unsigned long long)b * p.max_events;
    hipLaunchKernelGGL(events_finish_kernel, dim3(events_grid_x((recs + EV_THREADS - 1) / EV_THREADS, 65536u)), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
