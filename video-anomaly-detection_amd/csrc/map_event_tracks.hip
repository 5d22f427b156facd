// Per-frame tracks of anomaly events: the cross-section of an event - its pixels in ONE frame - as a record
// of the region table's twelve words (smallest pixel, area, box, peak and its pixel, coordinate sums), for every event and frame of
// a clip behind csrc/map_events.hip, and for every open event in the newest frame of a live stream behind csrc/map_track.hip.  The
// event tables say that something persists and where it has ever been; a box that follows the object, "where is it now", a
// trajectory need the reduction per (event, frame).  The labellers are not touched: the label volume of vad_detect_events and the
// slot plane of the tracker already say which event a pixel belongs to.
//
//   init     every record of the table: the identities of the reductions where an event (kept and inside the table; open) stands
//            behind it, zeros everywhere else
//   reduce   clip: a foreground pixel's root is looked up among the clip's kept records - their roots ascend - by a 64-ary search
//            that the wave makes together, once per distinct root of the wave (wave_each_key of region_table.h) and only when a
//            lane's root differs from that of the pixel it saw before; live: the slot plane holds the slot itself.  The pixel then
//            contributes x, y, (key(v) << 32 | ~pixel), its index and a count to the record (event, frame) - gathered per lane over
//            its run of pixels (RegionAcc), combined per wave, nine integer atomics per group
//   finish   a record that gathered pixels gets its peak word split into float bits and pixel; one that gathered none (the event
//            is absent from the frame) becomes all-zero
// Integer atomics, min and max only: the table is the same words for any batching, launch order or tiling.  No workspace, no flag
// word, no union-find walk; every launch is asynchronous on the caller's stream, nothing is allocated, the host never waits, no
// loop without a bound known at launch.
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int ET_THREADS = REGION_THREADS;
constexpr unsigned ET_RUN = 1024;               // pixels a work-group of the reduce passes takes at a time
constexpr unsigned ET_REDUCE_BLOCKS_X = 256;    // reduce: 2^18 pixels of a clip (of a frame) per grid round
constexpr unsigned ET_TABLE_BLOCKS_X = 4096;    // init, finish: 2^20 records per round
constexpr int ET_MAX_EVENTS = 65536, ET_MAX_OPEN = 65536;
constexpr long long ET_MAX_RECORDS = 1ll << 26;
constexpr long long ET_MAX_PIXELS = 1ll << 24;  // the tracker's frames
// the tracker's state (include/vad_hip.h, csrc/map_track.hip): a header of 16 words - word 1 the open events, word 4 the magic,
// words 5-7 h, w, max_open -, the open table, the slot plane
constexpr unsigned ET_HEADER_WORDS = 16;
constexpr unsigned ET_MAGIC = 0x54444156u;      // "VADT"
constexpr unsigned ET_WORDS = VAD_REGION_WORDS;
static_assert(VAD_REGION_WORDS == 12, "the record layout below: word 0 min, 1 sum, 2-5 box, 6-7 peak word, 8-11 sums");

struct TracksP {
    const float* maps;       // clip: [b][vol]; live: the newest frame of stream s at maps + s * stride
    const int* labels;       // clip: [b][vol]: 0 or 1 + root
    const unsigned* records; // clip: [b][max_slots][VAD_EVENT_WORDS]
    const unsigned* counts;  // clip: [b][4]
    const unsigned* state;   // live: [b][state_words]
    unsigned* table;         // [b][max_slots][t][12] (live: t = 1)
    long long b, stride;
    size_t state_words;
    unsigned vol, npix, w, h, t, max_slots;
};

// the events of group g (a clip, a stream) that have records in the table: the kept ones inside it; the open ones of a state that
// is the tracker's own for this geometry (0 for any other blob: nothing of it is followed)
template <bool LIVE>
__device__ __forceinline__ unsigned tracks_used(const TracksP& p, long long g) {
    unsigned n;
    if (LIVE) {
        const unsigned* hd = p.state + (size_t)g * p.state_words;
        n = hd[4] == ET_MAGIC && hd[5] == p.h && hd[6] == p.w && hd[7] == p.max_slots ? hd[1] : 0u;
    } else {
        n = p.counts[g * 4];
    }
    return n < p.max_slots ? n : p.max_slots;
}

template <bool LIVE>
__global__ __launch_bounds__(ET_THREADS) void tracks_init_kernel(TracksP p) {
    const u64 per = (u64)p.max_slots * p.t, total = (u64)p.b * per;
    for (u64 k = (u64)blockIdx.x * ET_THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * ET_THREADS) {
        const u64 g = k / per;
        const unsigned e = (unsigned)((k - g * per) / p.t);
        unsigned* r = p.table + k * ET_WORDS;
        if (e < tracks_used<LIVE>(p, (long long)g)) {
            *(u32x4*)r = u32x4{0xffffffffu, 0u, 0xffffffffu, 0xffffffffu};      // smallest pixel (min), area, x0, y0 (min)
            *(u32x4*)(r + 4) = u32x4{0u, 0u, 0u, 0u};                           // x1, y1 (max), the 64-bit peak word (max)
        } else {
            *(u32x4*)r = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(r + 4) = u32x4{0u, 0u, 0u, 0u};
        }
        *(u32x4*)(r + 8) = u32x4{0u, 0u, 0u, 0u};                               // sum x, sum y
    }
}

// Adds the lanes' gathered values (sw: the pixel count; first: the lane's smallest pixel) to their records: `pending` lanes hold a
// record number + 1 inside the table, equal ones of the wave are combined first.
__device__ __forceinline__ void tracks_flush(bool pending, const RegionAcc<unsigned>& a, unsigned first, unsigned* table, unsigned lane) {
    wave_each_key(pending, a.slot, lane, [&](unsigned slot, bool mine, bool many, bool lead) {
        const RegionAcc<unsigned> c = a.combined(mine, many);
        unsigned not_first = mine ? ~first : 0u;
        if (many) not_first = wave_max(not_first);
        if (lead) {
            unsigned* r = table + (size_t)(slot - 1u) * ET_WORDS;
            c.commit(r, 2, 6, 8);
            atomicMin(r, ~not_first);
            atomicAdd(r + 1, c.sw);
        }
    });
}

// 1 + the index of the record whose root is `root` among the first n records of rec (their roots ascend), or 0: a 64-ary search of
// the whole wave, at most three rounds for 65536 records.  root and n are wave-uniform and the call sits in converged control flow.
// No index outside [0, n) is formed, whatever the words hold.
__device__ __forceinline__ unsigned tracks_locate(const unsigned* rec, unsigned n, unsigned root, unsigned lane) {
    unsigned lo = 0u;
    while (n > 64u) {
        const unsigned step = (n + 63u) / 64u;
        const bool le = lane * step < n && rec[(size_t)(lo + lane * step) * VAD_EVENT_WORDS] <= root;
        const unsigned k = (unsigned)__builtin_popcountll(__ballot(le));        // the lanes at or below the root: a prefix
        if (k == 0u) return 0u;
        lo += (k - 1u) * step;
        n -= (k - 1u) * step;
        n = n < step ? n : step;
    }
    const u64 hit = __ballot(lane < n && rec[(size_t)(lo + lane) * VAD_EVENT_WORDS] == root);
    return hit != 0ull ? lo + (unsigned)__builtin_ctzll(hit) + 1u : 0u;
}

__global__ __launch_bounds__(ET_THREADS) void tracks_reduce_kernel(TracksP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.vol + ET_RUN - 1u) / ET_RUN;                   // vol < 2^31 - 1: no wrap
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const unsigned nkept = tracks_used<false>(p, clip);
        if (nkept == 0u) continue;                                           // uniform over the work-group
        const float* V = p.maps + clip * (long long)p.vol;
        const int* L = p.labels + clip * (long long)p.vol;
        const unsigned* rec = p.records + (u64)clip * p.max_slots * VAD_EVENT_WORDS;
        unsigned* table = p.table + (u64)clip * p.max_slots * p.t * ET_WORDS;
        const unsigned root_lo = rec[0], root_hi = rec[(size_t)(nkept - 1u) * VAD_EVENT_WORDS];
        RegionAcc<unsigned> acc;                                             // sw: the pixel count
        acc.clear();
        unsigned acc_first = 0u;                                             // the first pixel gathered: a lane's pixels ascend
        unsigned seen_root = 0xffffffffu, seen_event = 0u;                   // the root this lane looked up last: 1 + its record, or 0
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {     // uniform over the work-group
            for (unsigned j = 0; j < ET_RUN / ET_THREADS; ++j) {             // the same trip count for every lane: converged ballots
                const u64 i64 = (u64)run * ET_RUN + j * ET_THREADS + threadIdx.x;
                const unsigned i = (unsigned)i64;
                const int lab = i64 < p.vol ? L[i] : 0;
                const unsigned root = (unsigned)lab - 1u;
                const bool inside = lab != 0 && root >= root_lo && root <= root_hi;
                // a root is looked up once per distinct root of the wave, and not again while a lane stays inside one event
                const bool search = inside && root != seen_root;
                unsigned found = 0u;
                wave_each_key(search, root, lane, [&](unsigned first, bool mine, bool, bool) {
                    const unsigned e = tracks_locate(rec, nkept, first, lane);
                    if (mine) found = e;
                });
                if (search) {
                    seen_root = root;
                    seen_event = found;
                }
                const unsigned event = inside ? seen_event : 0u;             // <= nkept <= max_slots
                const unsigned f = i / p.npix;
                const unsigned slot = event != 0u ? (event - 1u) * p.t + f + 1u : 0u;   // <= max_slots * t <= 2^26
                // another record than the one gathered so far: that one goes out first
                tracks_flush(acc.slot != 0u && slot != 0u && slot != acc.slot, acc, acc_first, table, lane);
                if (slot != 0u) {
                    const unsigned pix = i - f * p.npix;
                    const unsigned y = pix / p.w, x = pix - y * p.w;
                    if (slot != acc.slot) acc_first = pix;
                    acc.add(slot, x, y, ((u64)order_key(__float_as_uint(V[i])) << 32) | (u64)(~pix), 1u);
                }
            }
        }
        tracks_flush(acc.slot != 0u, acc, acc_first, table, lane);
    }
}

__global__ __launch_bounds__(ET_THREADS) void boxes_reduce_kernel(TracksP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.npix + ET_RUN - 1u) / ET_RUN;                  // npix <= 2^24
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        const unsigned nopen = tracks_used<true>(p, s);
        if (nopen == 0u) continue;                                           // uniform; a foreign blob's plane is never read
        const float* V = p.maps + s * p.stride;
        const unsigned* P = p.state + (size_t)s * p.state_words + ET_HEADER_WORDS + (size_t)p.max_slots * VAD_TRACK_WORDS;
        unsigned* table = p.table + (u64)s * p.max_slots * ET_WORDS;
        RegionAcc<unsigned> acc;
        acc.clear();
        unsigned acc_first = 0u;
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {
            for (unsigned j = 0; j < ET_RUN / ET_THREADS; ++j) {
                const unsigned i = run * ET_RUN + j * ET_THREADS + threadIdx.x;
                unsigned slot = i < p.npix ? P[i] : 0u;                      // 0, slot + 1, or 0xffffffff for a lost event
                if (slot - 1u >= nopen) slot = 0u;                           // no record: no address is formed from it
                tracks_flush(acc.slot != 0u && slot != 0u && slot != acc.slot, acc, acc_first, table, lane);
                if (slot != 0u) {
                    const unsigned y = i / p.w, x = i - y * p.w;
                    if (slot != acc.slot) acc_first = i;
                    acc.add(slot, x, y, ((u64)order_key(__float_as_uint(V[i])) << 32) | (u64)(~i), 1u);
                }
            }
        }
        tracks_flush(acc.slot != 0u, acc, acc_first, table, lane);
    }
}

// the peak word of a record that gathered pixels -> float bits, pixel; a record in use that gathered none -> zeros
template <bool LIVE>
__global__ __launch_bounds__(ET_THREADS) void tracks_finish_kernel(TracksP p) {
    const u64 per = (u64)p.max_slots * p.t, total = (u64)p.b * per;
    for (u64 k = (u64)blockIdx.x * ET_THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * ET_THREADS) {
        const u64 g = k / per;
        const unsigned e = (unsigned)((k - g * per) / p.t);
        if (e >= tracks_used<LIVE>(p, (long long)g)) continue;               // zeroed by the init pass
        unsigned* r = p.table + k * ET_WORDS;
        if (r[1] != 0u) {
            const unsigned not_pixel = r[6], key = r[7];
            r[6] = order_key_inv(key);
            r[7] = ~not_pixel;
        } else {
            *(u32x4*)r = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(r + 4) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

unsigned tracks_grid_x(unsigned long long items, unsigned cap) { return (unsigned)(items < cap ? (items ? items : 1) : cap); }

template <bool LIVE>
int tracks_launch(const TracksP& p, unsigned long long pixels, hipStream_t s) {
    const unsigned long long recs = (unsigned long long)p.b * p.max_slots * p.t;
    const unsigned gy = (unsigned)(p.b < 65535 ? p.b : 65535);
    const dim3 block(ET_THREADS);
    const dim3 table_grid(tracks_grid_x((recs + ET_THREADS - 1) / ET_THREADS, ET_TABLE_BLOCKS_X));
    hipLaunchKernelGGL(tracks_init_kernel<LIVE>, table_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    const dim3 reduce_grid(tracks_grid_x((pixels + ET_RUN - 1) / ET_RUN, ET_REDUCE_BLOCKS_X), gy);
    if (LIVE) hipLaunchKernelGGL(boxes_reduce_kernel, reduce_grid, block, 0, s, p);
    else hipLaunchKernelGGL(tracks_reduce_kernel, reduce_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(tracks_finish_kernel<LIVE>, table_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

}  // namespace

int vad_event_tracks_plan(int* reduce_round, int* threads) {
    VAD_REQUIRE(reduce_round && threads, "event_tracks_plan: an output pointer is NULL");
    *reduce_round = (int)(ET_REDUCE_BLOCKS_X * ET_RUN);
    *threads = ET_THREADS;
    return VAD_OK;
}

int vad_event_tracks(const float* maps, const int32_t* labels, const uint32_t* records, const uint32_t* counts, long long b, int t, int h,
                     int w, int max_events, uint32_t* tracks, void* stream) {
    const char* who = "event_tracks";
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_ptr(who, "labels", labels, 4));
    VAD_ARG(vad_req_ptr(who, "records", records, 16));
    VAD_ARG(vad_req_ptr(who, "counts", counts, 4));
    VAD_ARG(vad_req_label_n(who, "b", b));
    VAD_ARG(vad_req_t(who, t));
    VAD_ARG(vad_req_label_hw(who, h, w));
    long long vol = 0, total = 0, recs = 0;
    VAD_REQUIRE(!__builtin_mul_overflow((long long)t, (long long)h * w, &vol) && vol < 2147483647ll,
                "event_tracks: t * h * w must be below 2^31 - 1 (%d x %d x %d)", t, h, w);
    VAD_REQUIRE(!__builtin_mul_overflow(b, vol, &total) && total <= (1ll << 38), "event_tracks: b * t * h * w must be at most 2^38 (%lld x %d x %d x %d)",
                b, t, h, w);
    VAD_ARG(vad_req_capacity(who, "max_events", max_events, ET_MAX_EVENTS));
    VAD_REQUIRE(!__builtin_mul_overflow(b, (long long)max_events * t, &recs) && recs <= ET_MAX_RECORDS,
                "event_tracks: b * max_events * t must be at most 2^26 records (%lld x %d x %d)", b, max_events, t);
    VAD_ARG(vad_req_ptr(who, "tracks", tracks, 16));
    if (b == 0) return VAD_OK;
    TracksP p = {};
    p.maps = maps;
    p.labels = labels;
    p.records = records;
    p.counts = counts;
    p.table = tracks;
    p.b = b;
    p.vol = (unsigned)vol;
    p.npix = (unsigned)h * (unsigned)w;
    p.w = (unsigned)w;
    p.h = (unsigned)h;
    p.t = (unsigned)t;
    p.max_slots = (unsigned)max_events;
    return tracks_launch<false>(p, (unsigned long long)vol, (hipStream_t)stream);
}

int vad_track_boxes(const float* maps_newest, long long frame_stride, long long b, int h, int w, int max_open, const void* state,
                    uint32_t* boxes, void* stream) {
    const char* who = "track_boxes";
    VAD_ARG(vad_req_ptr(who, "maps_newest", maps_newest, 4));
    VAD_REQUIRE(b >= 0 && b <= (1ll << 20), "%s: b must be in 0..2^20, got %lld", who, b);
    VAD_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= ET_MAX_PIXELS, "%s: h and w must be >= 1 with h * w <= 2^24, got %d x %d", who, h, w);
    VAD_REQUIRE(frame_stride >= (long long)h * w && frame_stride <= (1ll << 38), "%s: frame_stride must be in h * w .. 2^38 floats, got %lld", who,
                frame_stride);
    VAD_ARG(vad_req_capacity(who, "max_open", max_open, ET_MAX_OPEN));
    VAD_ARG(vad_req_ptr(who, "state", state, 16));
    VAD_ARG(vad_req_ptr(who, "boxes", boxes, 16));
    if (b == 0) return VAD_OK;
    TracksP p = {};
    p.maps = maps_newest;
    p.state = (const unsigned*)state;
    p.table = boxes;
    p.b = b;
    p.stride = frame_stride;
    p.state_words = vad_track_state_bytes(1, h, w, max_open) / 4;            // one stream's blob, as the tracker lays it out
    p.npix = (unsigned)h * (unsigned)w;
    p.vol = p.npix;
    p.w = (unsigned)w;
    p.h = (unsigned)h;
    p.t = 1u;
    p.max_slots = (unsigned)max_open;
    return tracks_launch<true>(p, p.npix, (hipStream_t)stream);
}
