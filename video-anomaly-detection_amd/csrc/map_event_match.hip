// Events against ground-truth masks: the kept events of vad_detect_events joined with the connected tracks of the clip's mask volume
//  - the 3-D counterpart of csrc/map_match.hip.  What a debounced alarm is accepted on: how many labelled
// anomalies it still finds, how many false-alarm events it raises, how many frames after a defect appears it fires.  A host route
// copies every map and mask volume, labels both with a 3-D scipy.ndimage.label and runs sum_labels / minimum of one labelling under
// the other; here maps, masks and both labellings stay on the device.
//
//   label    the in-frame labeller of region_label.h twice, as it stands: the masks (their public formats) into labels_g, the maps
//            (predicate v >= threshold) into labels_p, on the b * t frames.  The labeller clears the flag word it is given, so the
//            masks' run reports into the second word of the head and the init pass folds it into the first.
//   volume   rebase, link, flatten, count of event_volume.h - the one copy csrc/map_events.hip runs - on both label planes: the
//            tracks with the filters (1, 1), so all of them count; the events with min_duration and min_volume
//   init     the six join words of every root of either labelling get their identities (0, 0xffffffff, 0)
//   join     one pass over the voxels.  P = the voxels of kept events (sizes and last frame at the root pass the filters), G = the
//            mask's voxels.  A voxel of both adds 1 to hit[root_g] and overlap[root_p] and its frame to the first / last shared frame
//            of both: a lane gathers a run of voxels with the same (track, event) pair in registers, equal pairs of a wave are
//            combined (wave_each_pair of region_table.h) and one lane issues the six integer atomics - a blob over a blob costs one
//            group of atomics per wave, not per voxel.  The classes P&G, P\G, G\P and the NaN voxels are counted per frame the same
//            way (equal frames of a wave combined first).
//   slot     the rank of a root = the roots of its table in the chunks before it + those in front of it inside its chunk: ascending
//            roots, scipy's 3-D numbering.  A root of rank r < max_events writes its record, which is final; every chunk adds its
//            tracks, detected tracks, kept, matched and dropped events, delays and immediate detections to the clip's counters.
//   finish   one work-group per clip: the voxel classes and the frame classes from frame_counts, the clip's one-hot class.
// The tables are zeroed in front of the kernels, so every record that is not written is all-zero.  Integer atomics, min and max only,
// and one IEEE double multiply and compare per root (-ffp-contract=off): every output is the same words for any batching, launch
// order or tiling.  Every launch is asynchronous on the caller's stream, nothing is allocated, the host never waits.  No loop
// without a bound known at launch.
#include <hip/hip_runtime.h>

#include "event_volume.h"

namespace {

constexpr int EM_PLANES = 12;   // labels, sizes, last frames of both volumes; hit, first, last shared frame of both: 4 bytes a voxel each

struct EvMatchP {
    const float* maps;
    const int* lab_p;        // [b][vol]: 0, or 1 + root
    const unsigned* size_p;  // at the roots: volume
    const unsigned* last_p;  // at the roots: last frame
    const int* lab_g;
    const unsigned* size_g;
    const unsigned* last_g;
    unsigned* hit;           // [b][vol] each, read and written at the roots of lab_g only
    unsigned* first_hit;
    unsigned* last_hit;
    unsigned* overlap;       // at the roots of lab_p only
    unsigned* first_ov;
    unsigned* last_ov;
    const unsigned* chunk_p; // [b][nchunks]: kept | dropped << 16 (event_volume.h)
    const unsigned* chunk_g;
    unsigned* gt_rec;        // [b][max_events][VAD_EVMATCH_WORDS]
    unsigned* pred_rec;
    u64* counts;             // [b][VAD_EVMATCH_COUNTS]
    unsigned* frame_counts;  // [b][t][4]
    unsigned* flags;         // [0] the call's flag word, [1] what the in-frame labelling of the masks reported
    double gt_fraction, pred_fraction;
    long long b;
    unsigned vol, npix, nchunks, t, min_duration, min_volume, max_events;
};

// shared >= 1 and (double)shared >= fraction * (double)volume: one multiply, one compare
__device__ __forceinline__ bool evmatch_passes(unsigned shared, unsigned volume, double fraction) {
    return shared >= 1u && (double)shared >= fraction * (double)volume;
}

__device__ __forceinline__ unsigned wave_min(unsigned v) { return ~wave_max(~v); }

// the identities of the join words at the roots of both labellings
__global__ __launch_bounds__(EV_THREADS) void evmatch_init_kernel(EvMatchP p) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const unsigned g = p.flags[1];                                   // the masks' in-frame labelling ran into its own word
        if (g != 0u) atomicOr(p.flags, g);
    }
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const long long off = clip * (long long)p.vol;
        // i + the stride stays below 2^31 + 2^20: no wrap
        for (unsigned i = blockIdx.x * EV_THREADS + threadIdx.x; i < p.vol; i += gridDim.x * EV_THREADS) {
            if (p.lab_g[off + i] == (int)(i + 1u)) {
                p.hit[off + i] = 0u;
                p.first_hit[off + i] = 0xffffffffu;
                p.last_hit[off + i] = 0u;
            }
            if (p.lab_p[off + i] == (int)(i + 1u)) {
                p.overlap[off + i] = 0u;
                p.first_ov[off + i] = 0xffffffffu;
                p.last_ov[off + i] = 0u;
            }
        }
    }
}

// Adds the lanes' gathered voxels of one (track, event) pair each to both roots: `pending` lanes hold a pair of labels (1 + root,
// both inside the volume), equal pairs of the wave are combined first.
__device__ __forceinline__ void evmatch_pair_flush(bool pending, unsigned key_g, unsigned key_p, unsigned cnt, unsigned tmin, unsigned tmax,
                                                   const EvMatchP& p, long long off, unsigned lane) {
    wave_each_pair(pending, key_g, key_p, lane, [&](unsigned g0, unsigned p0, bool mine, bool many, bool lead) {
        unsigned c = mine ? cnt : 0u, lo = mine ? tmin : 0xffffffffu, hi = mine ? tmax : 0u;
        if (many) {
            c = wave_sum(c);
            lo = wave_min(lo);
            hi = wave_max(hi);
        }
        if (lead) {
            const long long g = off + (g0 - 1u), q = off + (p0 - 1u);
            atomicAdd(p.hit + g, c);
            atomicMin(p.first_hit + g, lo);
            atomicMax(p.last_hit + g, hi);
            atomicAdd(p.overlap + q, c);
            atomicMin(p.first_ov + q, lo);
            atomicMax(p.last_ov + q, hi);
        }
    });
}

// Adds the lanes' counts of one frame each (`pending` lanes: frame < p.t) to frame_counts; equal frames of the wave are combined first.
__device__ __forceinline__ void evmatch_frames_flush(bool pending, unsigned frame, unsigned ntp, unsigned nfp, unsigned nfn, unsigned nnan,
                                                     unsigned* fc, unsigned lane) {
    wave_each_key(pending, frame, lane, [&](unsigned first, bool mine, bool, bool lead) {
        const unsigned a = wave_sum(mine ? ntp : 0u), b = wave_sum(mine ? nfp : 0u), c = wave_sum(mine ? nfn : 0u), d = wave_sum(mine ? nnan : 0u);
        if (lead) {
            unsigned* r = fc + (u64)first * 4u;
            if (a) atomicAdd(r, a);
            if (b) atomicAdd(r + 1, b);
            if (c) atomicAdd(r + 2, c);
            if (d) atomicAdd(r + 3, d);
        }
    });
}

__global__ __launch_bounds__(EV_THREADS) void evmatch_join_kernel(EvMatchP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;               // vol < 2^31 - 1: no wrap
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const long long off = clip * (long long)p.vol;
        const float* V = p.maps + off;
        const int* Lp = p.lab_p + off;
        const int* Lg = p.lab_g + off;
        const unsigned* Sp = p.size_p + off;
        const unsigned* Tp = p.last_p + off;
        unsigned* fc = p.frame_counts + (u64)clip * p.t * 4u;
        unsigned key_g = 0u, key_p = 0u, cnt = 0u, tmin = 0u, tmax = 0u;  // cnt == 0: nothing gathered
        unsigned frame = 0u, ftp = 0u, ffp = 0u, ffn = 0u, fnan = 0u;     // of the frame this lane is in
        int seen_lp = 0;                                                  // the event label this lane met last, and whether it is kept
        bool seen_kept = false;
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {  // uniform over the work-group
            for (unsigned j = 0; j < EV_RUN / EV_THREADS; ++j) {         // the same trip count for every lane: converged ballots
                const u64 i64 = (u64)run * EV_RUN + j * EV_THREADS + threadIdx.x;
                const bool valid = i64 < p.vol;
                const unsigned i = (unsigned)i64;
                const unsigned bits = valid ? __float_as_uint(V[i]) : 0u;
                const int lp = valid ? Lp[i] : 0;
                const int lg = valid ? Lg[i] : 0;
                const unsigned t = valid ? i / p.npix : frame;
                const bool isnan = (bits & 0x7fffffffu) > 0x7f800000u;
                if (lp != seen_lp) {
                    seen_lp = lp;
                    seen_kept = false;
                    const unsigned root = (unsigned)lp - 1u;
                    // a label is a root of this clip: always inside
                    if (lp != 0 && root < p.vol) seen_kept = events_kept(p.npix, p.min_duration, p.min_volume, root, Sp[root], Tp[root]);
                }
                const bool in_p = lp != 0 && seen_kept;
                const bool in_g = lg != 0 && (unsigned)lg - 1u < p.vol;  // never false for a label, short of a defect: no address from it
                const bool both = in_p && in_g;
                // another frame than the one counted so far: that one's counts go out first
                const bool moved = t != frame;
                evmatch_frames_flush(moved && (ftp | ffp | ffn | fnan) != 0u, frame, ftp, ffp, ffn, fnan, fc, lane);
                if (moved) {
                    frame = t;
                    ftp = ffp = ffn = fnan = 0u;
                }
                ftp += both ? 1u : 0u;
                ffp += in_p && !in_g ? 1u : 0u;
                ffn += in_g && !in_p ? 1u : 0u;
                fnan += isnan ? 1u : 0u;
                // another pair than the one gathered so far: that one goes to its roots first
                const bool changed = cnt != 0u && both && ((unsigned)lg != key_g || (unsigned)lp != key_p);
                evmatch_pair_flush(changed, key_g, key_p, cnt, tmin, tmax, p, off, lane);
                if (changed) cnt = 0u;
                if (both) {
                    if (cnt == 0u) {
                        key_g = (unsigned)lg;
                        key_p = (unsigned)lp;
                        tmin = t;                                        // a lane's voxels ascend: the first frame is the smallest
                    }
                    ++cnt;
                    tmax = t;
                }
            }
        }
        evmatch_pair_flush(cnt != 0u, key_g, key_p, cnt, tmin, tmax, p, off, lane);
        evmatch_frames_flush((ftp | ffp | ffn | fnan) != 0u, frame, ftp, ffp, ffn, fnan, fc, lane);
    }
}

// ranks of the roots of both tables in ascending order, their records, and the clip's track and event counters
__global__ __launch_bounds__(EV_THREADS) void evmatch_slot_kernel(EvMatchP p) {
    __shared__ unsigned s_base[2], s_n[6], s_wave[2][REGION_WAVES];
    const unsigned lane = threadIdx.x & 63u;
    for (long long clip = blockIdx.y; clip < p.b; clip += gridDim.y) {
        const long long off = clip * (long long)p.vol;
        const unsigned* cp = p.chunk_p + clip * (long long)p.nchunks;
        const unsigned* cg = p.chunk_g + clip * (long long)p.nchunks;
        unsigned* rec_p = p.pred_rec + (u64)clip * p.max_events * VAD_EVMATCH_WORDS;
        unsigned* rec_g = p.gt_rec + (u64)clip * p.max_events * VAD_EVMATCH_WORDS;
        u64* cnt = p.counts + clip * VAD_EVMATCH_COUNTS;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<2>(s_base);
            unsigned base[2] = {0u, 0u}, rank[2];                        // [0] kept events, [1] tracks: those in front of the chunk
            for (unsigned k = threadIdx.x; k < c; k += EV_THREADS) {
                base[0] += cp[k] & 0xffffu;
                base[1] += cg[k] & 0xffffu;
            }
            block_sum(base, s_base);
            block_sum_clear<6>(s_n);
            unsigned n[6] = {0u, 0u, 0u, 0u, 0u, 0u};                    // tracks, detected, kept, matched, dropped, immediate
            u64 delays = 0ull;
            for (unsigned j = 0; j < EV_CHUNK / EV_THREADS; ++j) {
                const unsigned i = c * EV_CHUNK + j * EV_THREADS + threadIdx.x;        // < 2^31 + 1024: no wrap
                const bool inside = i < p.vol;
                const bool root_p = inside && p.lab_p[off + i] == (int)(i + 1u);
                const bool root_g = inside && p.lab_g[off + i] == (int)(i + 1u);
                const unsigned t0 = i / p.npix;                          // a root is its component's first voxel
                const unsigned vol_p = root_p ? p.size_p[off + i] : 0u, t1_p = root_p ? p.last_p[off + i] : 0u;
                const unsigned vol_g = root_g ? p.size_g[off + i] : 0u, t1_g = root_g ? p.last_g[off + i] : 0u;
                const bool kept = root_p && events_kept(p.npix, p.min_duration, p.min_volume, i, vol_p, t1_p);
                const unsigned ov = kept ? p.overlap[off + i] : 0u, hit = root_g ? p.hit[off + i] : 0u;
                const bool matched = kept && evmatch_passes(ov, vol_p, p.pred_fraction);
                const bool detected = root_g && evmatch_passes(hit, vol_g, p.gt_fraction);
                const unsigned first_hit = hit ? p.first_hit[off + i] : 0xffffffffu, last_hit = hit ? p.last_hit[off + i] : 0xffffffffu;
                const bool preds[2] = {kept, root_g};
                chunk_rank_row(preds, base, rank, s_wave);
                if (kept && rank[0] < p.max_events) {
                    unsigned* r = rec_p + (u64)rank[0] * VAD_EVMATCH_WORDS;
                    *(u32x4*)r = u32x4{i, vol_p, t0, t1_p};
                    *(u32x4*)(r + 4) = u32x4{ov, ov ? p.first_ov[off + i] : 0xffffffffu, ov ? p.last_ov[off + i] : 0xffffffffu, matched ? 1u : 0u};
                }
                if (root_g && rank[1] < p.max_events) {
                    unsigned* r = rec_g + (u64)rank[1] * VAD_EVMATCH_WORDS;
                    *(u32x4*)r = u32x4{i, vol_g, t0, t1_g};
                    *(u32x4*)(r + 4) = u32x4{hit, first_hit, last_hit, detected ? 1u : 0u};
                }
                n[0] += root_g ? 1u : 0u;
                n[1] += detected ? 1u : 0u;
                n[2] += kept ? 1u : 0u;
                n[3] += matched ? 1u : 0u;
                n[4] += root_p && !kept ? 1u : 0u;
                n[5] += detected && first_hit == t0 ? 1u : 0u;
                delays += detected ? (u64)(first_hit - t0) : 0ull;       // a shared voxel lies in the track: first_hit >= t0
            }
            block_sum(n, s_n);
            delays = wave_sum(delays);
            if (lane == 0u && delays != 0ull) atomicAdd(cnt + 12, delays);
            if (threadIdx.x == 0) {
                if (n[0]) atomicAdd(cnt + 0, (u64)n[0]);
                if (n[1]) atomicAdd(cnt + 1, (u64)n[1]);
                if (n[2]) atomicAdd(cnt + 2, (u64)n[2]);
                if (n[3]) atomicAdd(cnt + 3, (u64)n[3]);
                if (n[2] - n[3]) atomicAdd(cnt + 4, (u64)(n[2] - n[3]));   // matched is a subset of kept
                if (n[4]) atomicAdd(cnt + 5, (u64)n[4]);
                if (n[5]) atomicAdd(cnt + 13, (u64)n[5]);
            }
        }
    }
}

// per clip: the voxel classes and the frame classes summed from frame_counts, and the clip's one-hot class
__global__ __launch_bounds__(EV_THREADS) void evmatch_finish_kernel(EvMatchP p) {
    __shared__ u64 s_part[REGION_WAVES][8];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long clip = blockIdx.x; clip < p.b; clip += gridDim.x) {   // uniform over the work-group
        const unsigned* fc = p.frame_counts + (u64)clip * p.t * 4u;
        u64 v[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};     // P&G, P\G, G\P, NaN voxels; frames of both, P only, G only, neither
        for (unsigned f = threadIdx.x; f < p.t; f += EV_THREADS) {
            const unsigned* r = fc + (u64)f * 4u;
            const unsigned tp = r[0], fp = r[1], fn = r[2];
            v[0] += tp;
            v[1] += fp;
            v[2] += fn;
            v[3] += r[3];
            const bool in_p = (tp | fp) != 0u, in_g = (tp | fn) != 0u;
            v[4 + (in_g ? (in_p ? 0 : 2) : (in_p ? 1 : 3))] += 1ull;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = wave_sum(v[q]);
        if (lane == 0u) {
#pragma unroll
            for (int q = 0; q < 8; ++q) s_part[wave][q] = v[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 s[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                s[q] = 0ull;
                for (unsigned k = 0; k < REGION_WAVES; ++k) s[q] += s_part[k][q];
            }
            u64* c = p.counts + clip * VAD_EVMATCH_COUNTS;
            c[6] = s[0];
            c[7] = s[1];
            c[8] = s[2];
            c[9] = (u64)p.vol - s[0] - s[1] - s[2];
            c[10] = s[3];
            c[11] = s[0] + s[2];
            c[14] = s[4];
            c[15] = s[5];
            c[16] = s[6];
            c[17] = s[7];
            const bool gt = c[0] != 0ull, pred = c[2] != 0ull;           // final: the slot pass ran before this kernel
            c[18 + (gt ? (pred ? 0 : 2) : (pred ? 1 : 3))] = 1ull;        // the other three words were zeroed in front of the kernels
        }
        __syncthreads();                                                 // s_part is written again for the next clip
    }
}

// the bytes in front of the planes: the flag words' 16, then the chunk words of the events and of the tracks, each padded to 16
size_t evmatch_head_bytes(long long b, long long vol) { return VAD_LABEL_WS_HEAD_BYTES + 2 * region_chunk_bytes(b, vol, 1); }

}  // namespace

size_t vad_event_match_workspace_bytes(long long b, int t, int h, int w) {
    long long vol = 0, total = 0;
    if (!events_dims_ok(b, t, h, w, &vol, &total)) return 0;
    return evmatch_head_bytes(b, vol) + (size_t)(4 * EM_PLANES) * (size_t)total;
}

int vad_event_match_plan(int* label_round, int* volume_round, int* scan_round, int* join_round, int* threads) {
    VAD_REQUIRE(label_round && volume_round && scan_round && join_round && threads, "event_match_plan: an output pointer is NULL");
    *label_round = (int)VAD_LABEL_ROUND_PIXELS;
    *volume_round = (int)(EV_VOLUME_BLOCKS_X * EV_THREADS);
    *scan_round = (int)(EV_SCAN_BLOCKS_X * EV_CHUNK);
    *join_round = (int)(EV_REDUCE_BLOCKS_X * EV_RUN);
    *threads = EV_THREADS;
    return VAD_OK;
}

int vad_match_events(const float* maps, const void* masks, int mask_format, long long b, int t, int h, int w, float threshold,
                     int connectivity, int temporal, unsigned min_duration, unsigned min_volume, double gt_fraction, double pred_fraction,
                     int max_events, uint32_t* gt_records, uint32_t* pred_records, uint64_t* counts, uint32_t* frame_counts, void* ws,
                     size_t ws_bytes, void* stream) {
    const char* who = "match_events";
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_masks(who, masks, "mask_format", mask_format));
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
    VAD_REQUIRE(gt_fraction >= 0.0 && gt_fraction <= 1.0, "match_events: gt_fraction must be in [0, 1], got %g", gt_fraction);
    VAD_REQUIRE(pred_fraction >= 0.0 && pred_fraction <= 1.0, "match_events: pred_fraction must be in [0, 1], got %g", pred_fraction);
    VAD_ARG(vad_req_capacity(who, "max_events", max_events, EV_MAX_EVENTS));
    VAD_ARG(vad_req_ptr(who, "gt_records", gt_records, 16));
    VAD_ARG(vad_req_ptr(who, "pred_records", pred_records, 16));
    VAD_ARG(vad_req_ptr(who, "counts", counts, 8));
    VAD_ARG(vad_req_ptr(who, "frame_counts", frame_counts, 4));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, vad_event_match_workspace_bytes(b, t, h, w), "vad_event_match_workspace_bytes(%lld, %d, %d, %d)", b, t, h, w);
    const hipStream_t s = (hipStream_t)stream;
    if (b == 0) {                                            // nothing to match: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, VAD_LABEL_WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    unsigned* flags = (unsigned*)ws;
    unsigned* chunk_p = (unsigned*)((char*)ws + VAD_LABEL_WS_HEAD_BYTES);
    unsigned* chunk_g = (unsigned*)((char*)chunk_p + region_chunk_bytes(b, vol, 1));
    unsigned* planes = (unsigned*)((char*)ws + evmatch_head_bytes(b, vol));

    VolumeP vp, vg;
    vp.labels = (int*)planes;
    vp.sizes = planes + total;
    vp.aux = planes + 2 * total;
    vp.chunk_kept = chunk_p;
    vp.flags = flags;
    vp.b = b;
    vp.vol = (unsigned)vol;
    vp.npix = (unsigned)h * (unsigned)w;
    vp.nchunks = region_chunks(vol);
    vp.w = (unsigned)w;
    vp.min_duration = min_duration;
    vp.min_volume = min_volume;
    vp.temporal = temporal;
    vg = vp;
    vg.labels = (int*)(planes + 3 * total);
    vg.sizes = planes + 4 * total;
    vg.aux = planes + 5 * total;
    vg.chunk_kept = chunk_g;
    vg.min_duration = 1u;                                    // every track counts
    vg.min_volume = 1u;

    EvMatchP p;
    p.maps = maps;
    p.lab_p = vp.labels;
    p.size_p = vp.sizes;
    p.last_p = vp.aux;
    p.lab_g = vg.labels;
    p.size_g = vg.sizes;
    p.last_g = vg.aux;
    p.hit = planes + 6 * total;
    p.first_hit = planes + 7 * total;
    p.last_hit = planes + 8 * total;
    p.overlap = planes + 9 * total;
    p.first_ov = planes + 10 * total;
    p.last_ov = planes + 11 * total;
    p.chunk_p = chunk_p;
    p.chunk_g = chunk_g;
    p.gt_rec = gt_records;
    p.pred_rec = pred_records;
    p.counts = (u64*)counts;
    p.frame_counts = frame_counts;
    p.flags = flags;
    p.gt_fraction = gt_fraction;
    p.pred_fraction = pred_fraction;
    p.b = b;
    p.vol = vp.vol;
    p.npix = vp.npix;
    p.nchunks = vp.nchunks;
    p.t = (unsigned)t;
    p.min_duration = min_duration;
    p.min_volume = min_volume;
    p.max_events = (unsigned)max_events;

    // inside the frames; the masks first, into the second flag word: the labeller clears the word it is given, and the maps' run
    // gets the first
    if (int rc = vad_label_launch(masks, mask_format, 0.f, b * t, h, w, connectivity, vg.labels, nullptr, flags + 1, s)) return rc;
    if (int rc = vad_label_launch(maps, VAD_LABEL_FMT_F32_GE, threshold, b * t, h, w, connectivity, vp.labels, nullptr, flags, s)) return rc;
    VAD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)b * VAD_EVMATCH_COUNTS * 8, s));
    VAD_HIP_TRY(hipMemsetAsync(frame_counts, 0, (size_t)b * (size_t)t * 16, s));
    const size_t table = (size_t)b * p.max_events * VAD_EVMATCH_WORDS * 4;
    VAD_HIP_TRY(hipMemsetAsync(gt_records, 0, table, s));
    VAD_HIP_TRY(hipMemsetAsync(pred_records, 0, table, s));
    if (int rc = events_volume_launch(vg, t, s)) return rc;
    if (int rc = events_volume_launch(vp, t, s)) return rc;
    const unsigned gy = events_grid_y(b);
    const dim3 block(EV_THREADS);
    const dim3 volume_grid(events_grid_x(((unsigned long long)vol + EV_THREADS - 1) / EV_THREADS, EV_VOLUME_BLOCKS_X), gy);
    hipLaunchKernelGGL(evmatch_init_kernel, volume_grid, block, 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned nruns = (p.vol + EV_RUN - 1u) / EV_RUN;
    hipLaunchKernelGGL(evmatch_join_kernel, dim3(events_grid_x(nruns, EV_REDUCE_BLOCKS_X), gy), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(evmatch_slot_kernel, dim3(events_grid_x(p.nchunks, EV_SCAN_BLOCKS_X), gy), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(evmatch_finish_kernel, dim3(events_grid_x((unsigned long long)b, 65535u)), block, 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
