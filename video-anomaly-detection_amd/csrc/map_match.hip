// Detections against ground-truth masks: the connected regions of {v >= threshold} of every frame joined with the connected regions
// of the frame's mask.  What a user accepts an operating point on - how many labelled defects it finds, how
// many false alarms it raises, which pixel IoU it reaches - as two tables of four words per region and sixteen counters per frame.
// A host route copies every map and every mask, labels both with scipy.ndimage.label and runs sum_labels of one labelling under the
// other; here maps, masks and both labellings stay on the device.
//
//   label    the union-find of csrc/region_overlap.hip through region_label.h, twice and as it stands: the masks (their public
//            formats) into labels_g / sizes_g, the maps (predicate v >= threshold) into labels_p / sizes_p.  The labeller clears the
//            flag word it is given, so the masks' run reports into the second word of the head and the join folds it into the first.
//   join     one pass over the pixels.  P = the pixels of predicted regions with sizes_p[root] >= min_area, G = the mask's pixels.
//            A pixel of both adds 1 to hit[root_g] and 1 to overlap[root_p]: a lane first gathers its own pixels of one region in
//            registers, equal roots of a wave are then combined (wave_each_key of region_table.h) and one lane issues the integer atomic - a frame that
//            is one region under one mask costs 8 atomics per work-group.  The classes P&G, P\G, G\P, the rest and the NaN pixels are
//            counted by ballot and popcount in wave-uniform registers, summed in LDS, and leave as one 64-bit atomic per class and
//            work-group.
//   count    a frame is cut into chunks of MT_CHUNK pixels; chunk c of frame f counts its kept predicted roots and its mask roots
//            into chunk_cnt[f][c][0 / 1], and adds regions, detected, kept, matched, false alarms and dropped to the frame's counters.
//   slot     the rank of a root = the roots of its table in the chunks before it + those in front of it inside its chunk (chunk_before,
//            chunk_rank_row of region_table.h): raster order across the frame, scipy.ndimage.label's numbering.  A root of rank r <
//            max_regions writes its record - root, area, hit or overlap, flag - which is final: nothing is reduced afterwards.
//   finish   one thread per frame: the one-hot frame class from the frame's two region counters.
// The tables are zeroed in front of the kernels, so every record that is not written is all-zero.  Integer atomics only, and one
// IEEE double multiply and compare per region (-ffp-contract=off): the outputs are the same words for any batching, launch order
// or tiling.  Every launch is asynchronous on the caller's stream, nothing is allocated, the host never waits.
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int MT_THREADS = REGION_THREADS;
constexpr unsigned MT_CHUNK = REGION_CHUNK;
constexpr unsigned MT_RUN = 4096;              // pixels a work-group of the join pass takes at a time
constexpr unsigned MT_SCAN_BLOCKS_X = 1024;     // count, slot: 2^20 pixels of a frame per grid round
constexpr unsigned MT_JOIN_BLOCKS_X = 256;      // join: 2^20 pixels of a frame per grid round; the frames of a call fill the device
constexpr int MT_MAX_REGIONS = 65536;
constexpr int MT_PLANES = 6;                    // labels_p, sizes_p, labels_g, sizes_g, hit, overlap: 4 bytes per pixel each

struct MatchP {
    const float* maps;
    const int* lab_p;
    const unsigned* size_p;
    const int* lab_g;
    const unsigned* size_g;
    unsigned* hit;           // [n][npix], read and written at the roots of lab_g only
    unsigned* overlap;       // [n][npix], at the roots of lab_p only
    unsigned* chunk_cnt;     // [n][nchunks][2]: kept predicted roots, mask roots
    unsigned* gt_rec;        // [n][max_regions][VAD_MATCH_WORDS]
    unsigned* pred_rec;
    u64* counts;             // [n][VAD_MATCH_COUNTS]
    unsigned* flags;         // [0] the call's flag word, [1] what the labelling of the masks reported
    double gt_fraction, pred_fraction;
    long long n;
    unsigned npix, nchunks, min_area, max_regions;
};

// hit >= 1 and (double)hit >= fraction * (double)area: one multiply, one compare
__device__ __forceinline__ bool match_passes(unsigned shared, unsigned area, double fraction) {
    return shared >= 1u && (double)shared >= fraction * (double)area;
}

// Adds the lanes' gathered counts to table[key - 1]: `pending` lanes hold a key != 0, equal keys of the wave are combined first.
__device__ __forceinline__ void match_flush(bool pending, unsigned key, unsigned cnt, unsigned* table, unsigned lane) {
    wave_each_key(pending, key, lane, [&](unsigned first, bool mine, bool many, bool lead) {
        unsigned c = mine ? cnt : 0u;
        if (many) c = wave_sum(c);
        if (lead) atomicAdd(table + (first - 1u), c);
    });
}

__global__ __launch_bounds__(MT_THREADS) void match_join_kernel(MatchP p) {
    __shared__ unsigned s_cls[5];                                        // P&G, P\G, G\P, NaN, pixels seen
    const unsigned lane = threadIdx.x & 63u;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const unsigned g = p.flags[1];                                   // the masks' labelling ran first, into its own word
        if (g != 0u) atomicOr(p.flags, g);
    }
    const unsigned nruns = (p.npix + MT_RUN - 1u) / MT_RUN;              // npix < 2^31 - 1: no wrap
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const long long off = img * (long long)p.npix;
        const float* V = p.maps + off;
        const int* Lp = p.lab_p + off;
        const int* Lg = p.lab_g + off;
        const unsigned* Sp = p.size_p + off;
        if (threadIdx.x < 5) s_cls[threadIdx.x] = 0u;
        __syncthreads();
        unsigned ntp = 0u, nfp = 0u, nfn = 0u, nnan = 0u, nseen = 0u;    // wave-uniform: below 2^31 per work-group and frame
        unsigned key_g = 0u, cnt_g = 0u, key_p = 0u, cnt_p = 0u;         // key = label = 1 + root; 0 = nothing gathered
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {  // uniform over the work-group
            for (unsigned j = 0; j < MT_RUN / MT_THREADS; ++j) {         // the same trip count for every lane: converged ballots
                const u64 i64 = (u64)run * MT_RUN + j * MT_THREADS + threadIdx.x;
                const bool valid = i64 < p.npix;
                const unsigned i = (unsigned)i64;
                const unsigned bits = valid ? __float_as_uint(V[i]) : 0u;
                const int lp = valid ? Lp[i] : 0;
                const int lg = valid ? Lg[i] : 0;
                bool in_p = false;
                if (lp != 0) {
                    const unsigned root = (unsigned)lp - 1u;
                    in_p = root < p.npix && Sp[root] >= p.min_area;      // a label is a root of this frame: always inside
                }
                const bool in_g = lg != 0;
                const bool both = in_p && in_g;
                ntp += (unsigned)__builtin_popcountll(__ballot(both));
                nfp += (unsigned)__builtin_popcountll(__ballot(in_p && !in_g));
                nfn += (unsigned)__builtin_popcountll(__ballot(in_g && !in_p));
                nnan += (unsigned)__builtin_popcountll(__ballot((bits & 0x7fffffffu) > 0x7f800000u));
                nseen += (unsigned)__builtin_popcountll(__ballot(valid));
                // never, short of a defect: a mask label that is no index of this frame forms no address
                const unsigned kg = both && (unsigned)lg - 1u < p.npix ? (unsigned)lg : 0u;
                const unsigned kp = both ? (unsigned)lp : 0u;
                // another region than the one gathered so far: that one goes to its counter first
                match_flush(key_g != 0u && kg != 0u && kg != key_g, key_g, cnt_g, p.hit + off, lane);
                match_flush(key_p != 0u && kp != 0u && kp != key_p, key_p, cnt_p, p.overlap + off, lane);
                if (kg != 0u) {
                    cnt_g = kg != key_g ? 1u : cnt_g + 1u;
                    key_g = kg;
                }
                if (kp != 0u) {
                    cnt_p = kp != key_p ? 1u : cnt_p + 1u;
                    key_p = kp;
                }
            }
        }
        match_flush(key_g != 0u, key_g, cnt_g, p.hit + off, lane);
        match_flush(key_p != 0u, key_p, cnt_p, p.overlap + off, lane);
        if (lane == 0u) {
            if (ntp) atomicAdd(&s_cls[0], ntp);
            if (nfp) atomicAdd(&s_cls[1], nfp);
            if (nfn) atomicAdd(&s_cls[2], nfn);
            if (nnan) atomicAdd(&s_cls[3], nnan);
            if (nseen) atomicAdd(&s_cls[4], nseen);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u64* c = p.counts + img * VAD_MATCH_COUNTS;
            const unsigned tp = s_cls[0], fp = s_cls[1], fn = s_cls[2];
            const unsigned tn = s_cls[4] - tp - fp - fn;
            if (tp) atomicAdd(c + 6, (u64)tp);
            if (fp) atomicAdd(c + 7, (u64)fp);
            if (fn) atomicAdd(c + 8, (u64)fn);
            if (tn) atomicAdd(c + 9, (u64)tn);
            if (s_cls[3]) atomicAdd(c + 10, (u64)s_cls[3]);
            if (tp + fn) atomicAdd(c + 11, (u64)tp + (u64)fn);
        }
        __syncthreads();                                                 // s_cls is cleared again for the next frame
    }
}

struct MatchRoots {
    bool kept, dropped, matched, gt, detected;
    unsigned area_p, area_g, overlap, hit;
};

// what pixel i is a root of, in either labelling
__device__ __forceinline__ MatchRoots match_roots(const MatchP& p, long long off, unsigned i) {
    MatchRoots r;
    const bool inside = i < p.npix;
    const bool root_p = inside && p.lab_p[off + i] == (int)(i + 1u);
    r.gt = inside && p.lab_g[off + i] == (int)(i + 1u);
    r.area_p = root_p ? p.size_p[off + i] : 0u;
    r.area_g = r.gt ? p.size_g[off + i] : 0u;
    r.kept = root_p && r.area_p >= p.min_area;
    r.dropped = root_p && !r.kept;
    r.overlap = r.kept ? p.overlap[off + i] : 0u;
    r.hit = r.gt ? p.hit[off + i] : 0u;
    r.matched = r.kept && match_passes(r.overlap, r.area_p, p.pred_fraction);
    r.detected = r.gt && match_passes(r.hit, r.area_g, p.gt_fraction);
    return r;
}

// roots per chunk, and the frame's region counters
__global__ __launch_bounds__(MT_THREADS) void match_count_kernel(MatchP p) {
    __shared__ unsigned s_n[5];                                          // kept, dropped, matched, mask regions, detected
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const long long off = img * (long long)p.npix;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<5>(s_n);
            unsigned n[5] = {0u, 0u, 0u, 0u, 0u};
            for (unsigned j = 0; j < MT_CHUNK / MT_THREADS; ++j) {
                const MatchRoots r = match_roots(p, off, c * MT_CHUNK + j * MT_THREADS + threadIdx.x);   // < 2^31 + 1024: no wrap
                n[0] += r.kept ? 1u : 0u;
                n[1] += r.dropped ? 1u : 0u;
                n[2] += r.matched ? 1u : 0u;
                n[3] += r.gt ? 1u : 0u;
                n[4] += r.detected ? 1u : 0u;
            }
            block_sum(n, s_n);
            if (threadIdx.x == 0) {
                unsigned* cc = p.chunk_cnt + (img * (long long)p.nchunks + c) * 2;
                cc[0] = n[0];
                cc[1] = n[3];
                u64* cnt = p.counts + img * VAD_MATCH_COUNTS;
                if (n[3]) atomicAdd(cnt + 0, (u64)n[3]);
                if (n[4]) atomicAdd(cnt + 1, (u64)n[4]);
                if (n[0]) atomicAdd(cnt + 2, (u64)n[0]);
                if (n[2]) atomicAdd(cnt + 3, (u64)n[2]);
                if (n[0] - n[2]) atomicAdd(cnt + 4, (u64)(n[0] - n[2]));   // matched is a subset of kept
                if (n[1]) atomicAdd(cnt + 5, (u64)n[1]);
            }
            __syncthreads();                                             // s_n is cleared again for the next chunk
        }
    }
}

// ranks of the roots of both tables in raster order, and their records
__global__ __launch_bounds__(MT_THREADS) void match_slot_kernel(MatchP p) {
    __shared__ unsigned s_before[2], s_wave[2][REGION_WAVES];
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const long long off = img * (long long)p.npix;
        unsigned* rec_p = p.pred_rec + (u64)img * p.max_regions * VAD_MATCH_WORDS;
        unsigned* rec_g = p.gt_rec + (u64)img * p.max_regions * VAD_MATCH_WORDS;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            unsigned base[2], rank[2];                                   // [0] kept predicted roots, [1] mask roots
            chunk_before(p.chunk_cnt + img * (long long)p.nchunks * 2, c, base, s_before);
            for (unsigned j = 0; j < MT_CHUNK / MT_THREADS; ++j) {
                const unsigned i = c * MT_CHUNK + j * MT_THREADS + threadIdx.x;
                const MatchRoots r = match_roots(p, off, i);
                const bool roots[2] = {r.kept, r.gt};
                chunk_rank_row(roots, base, rank, s_wave);
                if (r.kept && rank[0] < p.max_regions)
                    *(u32x4*)(rec_p + (u64)rank[0] * VAD_MATCH_WORDS) = u32x4{i, r.area_p, r.overlap, r.matched ? 1u : 0u};
                if (r.gt && rank[1] < p.max_regions)
                    *(u32x4*)(rec_g + (u64)rank[1] * VAD_MATCH_WORDS) = u32x4{i, r.area_g, r.hit, r.detected ? 1u : 0u};
            }
        }
    }
}

// the one-hot frame class: mask regions and kept predictions, predictions only, mask regions only, neither
__global__ __launch_bounds__(MT_THREADS) void match_finish_kernel(MatchP p) {
    for (u64 img = (u64)blockIdx.x * MT_THREADS + threadIdx.x; img < (u64)p.n; img += (u64)gridDim.x * MT_THREADS) {
        u64* c = p.counts + img * VAD_MATCH_COUNTS;
        const bool gt = c[0] != 0ull, pred = c[2] != 0ull;
        c[12 + (gt ? (pred ? 0 : 2) : (pred ? 1 : 3))] = 1ull;            // the other three words were zeroed in front of the kernels
    }
}

// the bytes in front of the planes: the flag words' 16, then chunk_cnt [n][nchunks][2], padded to 16
size_t match_head_bytes(long long n, int h, int w) { return region_head_bytes(n, (long long)h * w, 2); }

}  // namespace

size_t vad_match_workspace_bytes(long long n, int h, int w) {
    long long total = 0;
    if (!vad_label_dims_ok(n, h, w, &total)) return 0;
    return match_head_bytes(n, h, w) + (size_t)(4 * MT_PLANES) * (size_t)total;
}

int vad_match_plan(int* label_round, int* join_round, int* scan_round, int* threads) {
    VAD_REQUIRE(label_round && join_round && scan_round && threads, "match_plan: an output pointer is NULL");
    *label_round = (int)VAD_LABEL_ROUND_PIXELS;
    *join_round = (int)(MT_JOIN_BLOCKS_X * MT_RUN);
    *scan_round = (int)(MT_SCAN_BLOCKS_X * MT_CHUNK);
    *threads = MT_THREADS;
    return VAD_OK;
}

int vad_match_regions(const float* maps, const void* masks, int mask_format, long long n, int h, int w, float threshold,
                      int connectivity, unsigned min_area, double gt_fraction, double pred_fraction, int max_regions,
                      uint32_t* gt_records, uint32_t* pred_records, uint64_t* counts, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "match_regions";
    long long total = 0;
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_masks(who, masks, "mask_format", mask_format));
    VAD_ARG(vad_req_label_n(who, "n", n));
    VAD_ARG(vad_req_label_hw(who, h, w));
    VAD_ARG(vad_req_label_total(who, n, h, w, &total));
    VAD_ARG(vad_req_threshold(who, threshold));
    VAD_ARG(vad_req_connectivity(who, connectivity));
    VAD_ARG(vad_req_nonzero(who, "min_area", min_area));
    VAD_REQUIRE(gt_fraction >= 0.0 && gt_fraction <= 1.0, "match_regions: gt_fraction must be in [0, 1], got %g", gt_fraction);
    VAD_REQUIRE(pred_fraction >= 0.0 && pred_fraction <= 1.0, "match_regions: pred_fraction must be in [0, 1], got %g", pred_fraction);
    VAD_ARG(vad_req_capacity(who, "max_regions", max_regions, MT_MAX_REGIONS));
    VAD_ARG(vad_req_nonnull(who, "gt_records", gt_records));
    VAD_ARG(vad_req_nonnull(who, "pred_records", pred_records));
    VAD_REQUIRE(vad_aligned(gt_records, 16) && vad_aligned(pred_records, 16), "match_regions: records must be 16-byte aligned");
    VAD_ARG(vad_req_ptr(who, "counts", counts, 8));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, vad_match_workspace_bytes(n, h, w), "vad_match_workspace_bytes(%lld, %d, %d)", n, h, w);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {                                            // nothing to match: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, VAD_LABEL_WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    unsigned* planes = (unsigned*)((char*)ws + match_head_bytes(n, h, w));

    MatchP p;
    p.maps = maps;
    p.lab_p = (const int*)planes;
    p.size_p = planes + total;
    p.lab_g = (const int*)(planes + 2 * total);
    p.size_g = planes + 3 * total;
    p.hit = planes + 4 * total;
    p.overlap = planes + 5 * total;
    p.chunk_cnt = (unsigned*)((char*)ws + VAD_LABEL_WS_HEAD_BYTES);
    p.gt_rec = gt_records;
    p.pred_rec = pred_records;
    p.counts = (u64*)counts;
    p.flags = (unsigned*)ws;
    p.gt_fraction = gt_fraction;
    p.pred_fraction = pred_fraction;
    p.n = n;
    p.npix = (unsigned)h * (unsigned)w;
    p.nchunks = region_chunks((long long)h * w);
    p.min_area = min_area;
    p.max_regions = (unsigned)max_regions;

    // the masks first, into the second flag word: the labeller clears the word it is given, and the maps' run gets the first
    if (int rc = vad_label_launch(masks, mask_format, 0.f, n, h, w, connectivity, (int*)p.lab_g, (unsigned*)p.size_g, p.flags + 1, s)) return rc;
    if (int rc = vad_label_launch(maps, VAD_LABEL_FMT_F32_GE, threshold, n, h, w, connectivity, (int*)p.lab_p, (unsigned*)p.size_p, p.flags, s))
        return rc;
    VAD_HIP_TRY(hipMemsetAsync(p.hit, 0, (size_t)8 * (size_t)total, s)); // hit and overlap lie side by side
    VAD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * VAD_MATCH_COUNTS * 8, s));
    const size_t table = (size_t)n * p.max_regions * VAD_MATCH_WORDS * 4;
    VAD_HIP_TRY(hipMemsetAsync(gt_records, 0, table, s));
    VAD_HIP_TRY(hipMemsetAsync(pred_records, 0, table, s));
    const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
    const unsigned nruns = (p.npix + MT_RUN - 1u) / MT_RUN;
    hipLaunchKernelGGL(match_join_kernel, dim3(nruns < MT_JOIN_BLOCKS_X ? nruns : MT_JOIN_BLOCKS_X, gy), dim3(MT_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    const dim3 chunk_grid(p.nchunks < MT_SCAN_BLOCKS_X ? p.nchunks : MT_SCAN_BLOCKS_X, gy);
    hipLaunchKernelGGL(match_count_kernel, chunk_grid, dim3(MT_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_slot_kernel, chunk_grid, dim3(MT_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned long long fin = ((unsigned long long)n + MT_THREADS - 1) / MT_THREADS;
    hipLaunchKernelGGL(match_finish_kernel, dim3((unsigned)(fin < 1024ull ? fin : 1024ull)), dim3(MT_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
