// Anomaly events of a clip: the connected components of {v >= threshold} in the volume [t, h, w] of every clip - regions linked
// across frames - as a table of records: root, volume, first and last frame, union box, peak and its position, coordinate sums, in
// ascending order of their first voxel.  A deployed line alarms on events that persist, not on the blob of
// one frame; the host route copies every map of the clip and runs scipy.ndimage label with a 3-D structure, find_objects and
// maximum_position.  Here the maps stay on the device and the table is what leaves it.
//
//   label    the union-find of csrc/region_overlap.hip through region_label.h on the b * t frames as it stands: every foreground
//            pixel then hangs directly under its frame's root, so the unions in time that follow are short
//   rebase, link, flatten, count
//            the labelling of the volume, shared with csrc/map_event_match.hip: event_volume.h describes the four passes.  After
//            them labels[p] = 1 + root (the smallest volume index of the event: canonical), sizes and last frames stand at the
//            roots, and chunk_kept[b][c] holds the kept and the dropped roots of chunk c of clip b (EV_CHUNK pixels a chunk).
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

#include "event_volume.h"

namespace {

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
};

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
                const bool kept = root && events_kept(p.npix, p.min_duration, p.min_volume, i, volume, t1);
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
    VAD_ARG(events_req_volume(who, b, t, h, w, &vol, &total));
    VAD_ARG(vad_req_threshold(who, threshold));
    VAD_ARG(vad_req_connectivity(who, connectivity));
    VAD_ARG(events_req_temporal(who, connectivity, temporal));
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
    VAD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)b * 16, s));
    VAD_HIP_TRY(hipMemsetAsync(frame_counts, 0, (size_t)b * (size_t)t * 12, s));
    const unsigned gy = events_grid_y(b);
    const dim3 block(EV_THREADS);
    VolumeP v;
    v.labels = p.labels;
    v.sizes = p.sizes;
    v.aux = p.aux;
    v.chunk_kept = p.chunk_kept;
    v.flags = p.flags;
    v.b = b;
    v.vol = p.vol;
    v.npix = p.npix;
    v.nchunks = p.nchunks;
    v.w = p.w;
    v.min_duration = min_duration;
    v.min_volume = min_volume;
    v.temporal = temporal;
    if (int rc = events_volume_launch(v, t, s)) return rc;
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;
    const dim3 run_grid(events_grid_x(nruns, EV_REDUCE_BLOCKS_X), gy);
    const dim3 scan_grid(events_grid_x(p.nchunks, EV_SCAN_BLOCKS_X), gy);
    hipLaunchKernelGGL(events_slot_kernel, scan_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(events_reduce_kernel, run_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned long long recs = (unsigned long long)b * p.max_events;
    hipLaunchKernelGGL(events_finish_kernel, dim3(events_grid_x((recs + EV_THREADS - 1) / EV_THREADS, 65536u)), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
