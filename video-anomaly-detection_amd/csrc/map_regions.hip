// Defect regions of an anomaly map: the connected regions of {v >= threshold} of every frame as a table of records - root, area,
// bounding box, peak and its position, coordinate sums - in raster order of their first pixel.  The
// reference paints the map (evaluate.py:142-171, main.py:231-250) and compares one scalar with a constant (main.py:282-283); a
// host route copies every map and runs scipy.ndimage label / find_objects / maximum_position per frame.  Here the maps stay on the
// device and the table is what leaves it.
//
//   label    the union-find of csrc/region_overlap.hip through region_label.h (its init kernel with the predicate v >= threshold):
//            labels[p] = 0 or 1 + root, sizes[root] = area.  A NaN pixel is never foreground.
//   count    a frame is cut into chunks of REG_CHUNK pixels; chunk c of frame f counts its kept roots (sizes[root] >= min_area)
//            into chunk_kept[f][c], and adds kept / dropped roots to counts[f][0 / 1]
//   slot     the rank of a kept root = the kept roots of the chunks before it (a sum over chunk_kept[f][0 .. c)) + the kept roots in
//            front of it inside its chunk (chunk_before, chunk_rank_row of region_table.h): raster order across the whole frame.  A root of rank
//            r < max_regions gets slots[root] = r + 1 and its record's root, area and the identities of the reductions; any other
//            root gets slots[root] = 0.  Only roots' slots are ever written or read.
//   reduce   every foreground pixel whose root has a slot contributes x, y, (key(v) << 32 | ~index) to its record: min / max of
//            the box, max of the 64-bit peak word (the largest key and, among equals, the smallest index), sums of x and y.  A lane
//            first gathers its own pixels of one region in registers, then equal slots of a wave are combined, and one lane issues
//            the seven integer atomics (RegionAcc, wave_each_key of region_table.h): one region costs 28 atomics per 4096 pixels.  The same
//            pass counts foreground and NaN pixels into counts[f][2 / 3].
//   finish   the records in use get their peak word split into float bits and index; every other record of the table is zeroed.
// Integer atomics, min and max only: the table is the same words for any batching, launch order or tiling.  Every launch is
// asynchronous on the caller's stream, nothing is allocated, the host never waits.
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int REG_THREADS = REGION_THREADS;
constexpr unsigned REG_CHUNK = REGION_CHUNK;
constexpr unsigned REG_RUN = 4096;              // pixels a work-group of the reduce pass takes at a time
constexpr unsigned REG_MAX_BLOCKS_X = 4096;
constexpr int REG_MAX_REGIONS = 65536;

struct RegionP {
    const float* maps;
    const int* labels;
    const unsigned* sizes;
    unsigned* slots;
    unsigned* chunk_kept;    // [n][nchunks]
    unsigned* records;       // [n][max_regions][VAD_REGION_WORDS]
    unsigned* counts;        // [n][4]: kept, dropped for area, foreground pixels, NaN pixels
    long long n;
    unsigned npix, nchunks, w, min_area, max_regions;
};

// kept / dropped roots per chunk
__global__ __launch_bounds__(REG_THREADS) void regions_count_kernel(RegionP p) {
    __shared__ unsigned s_n[2];
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const int* L = p.labels + img * (long long)p.npix;
        const unsigned* S = p.sizes + img * (long long)p.npix;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<2>(s_n);
            unsigned n[2] = {0u, 0u};                                    // kept, dropped
            for (unsigned j = 0; j < REG_CHUNK / REG_THREADS; ++j) {
                const unsigned i = c * REG_CHUNK + j * REG_THREADS + threadIdx.x;      // < 2^31 + 1024: no wrap
                if (i < p.npix && L[i] == (int)(i + 1u)) {
                    if (S[i] >= p.min_area) ++n[0];
                    else ++n[1];
                }
            }
            block_sum(n, s_n);
            if (threadIdx.x == 0) {
                p.chunk_kept[img * (long long)p.nchunks + c] = n[0];
                if (n[0]) atomicAdd(p.counts + img * 4, n[0]);
                if (n[1]) atomicAdd(p.counts + img * 4 + 1, n[1]);
            }
            __syncthreads();                                             // s_n is cleared again for the next chunk
        }
    }
}

// ranks of the kept roots in raster order; the records' first words and the identities of the reductions
__global__ __launch_bounds__(REG_THREADS) void regions_slot_kernel(RegionP p) {
    __shared__ unsigned s_before[1], s_wave[1][REGION_WAVES];
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const int* L = p.labels + img * (long long)p.npix;
        const unsigned* S = p.sizes + img * (long long)p.npix;
        unsigned* slots = p.slots + img * (long long)p.npix;
        unsigned* rec = p.records + (u64)img * p.max_regions * VAD_REGION_WORDS;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            unsigned base[1];                                            // the kept roots of this frame in front of the chunk
            chunk_before(p.chunk_kept + img * (long long)p.nchunks, c, base, s_before);
            for (unsigned j = 0; j < REG_CHUNK / REG_THREADS; ++j) {
                const unsigned i = c * REG_CHUNK + j * REG_THREADS + threadIdx.x;
                const bool root = i < p.npix && L[i] == (int)(i + 1u);
                const unsigned area = root ? S[i] : 0u;
                const bool kept = root && area >= p.min_area;
                const unsigned rank = chunk_rank_row(kept, base[0], s_wave);
                if (kept && rank < p.max_regions) {
                    slots[i] = rank + 1u;
                    unsigned* r = rec + (u64)rank * VAD_REGION_WORDS;
                    *(u32x4*)r = u32x4{i, area, 0xffffffffu, 0xffffffffu};          // root, area, x0, y0 (min)
                    *(u32x4*)(r + 4) = u32x4{0u, 0u, 0u, 0u};                       // x1, y1 (max), the 64-bit peak word (max)
                    *(u32x4*)(r + 8) = u32x4{0u, 0u, 0u, 0u};                       // sum x, sum y
                } else if (root) {
                    slots[i] = 0u;
                }
            }
        }
    }
}

// Adds the lanes' gathered values to their records: `pending` lanes hold a slot != 0, equal slots of the wave are combined first.
__device__ __forceinline__ void regions_flush(bool pending, const RegionAcc<unsigned>& a, unsigned* rec, unsigned lane) {
    wave_each_key(pending, a.slot, lane, [&](unsigned first, bool mine, bool many, bool lead) {
        const RegionAcc<unsigned> c = a.combined(mine, many);
        if (lead) c.commit(rec + (u64)(first - 1u) * VAD_REGION_WORDS, 2, 6, 8);
    });
}

__global__ __launch_bounds__(REG_THREADS) void regions_reduce_kernel(RegionP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.npix + REG_RUN - 1u) / REG_RUN;            // npix < 2^31 - 1: no wrap
    for (long long img = blockIdx.y; img < p.n; img += gridDim.y) {
        const float* V = p.maps + img * (long long)p.npix;
        const int* L = p.labels + img * (long long)p.npix;
        const unsigned* slots = p.slots + img * (long long)p.npix;
        unsigned* rec = p.records + (u64)img * p.max_regions * VAD_REGION_WORDS;
        RegionAcc<unsigned> acc;                                         // no further sum
        acc.clear();
        unsigned nfg = 0u, nnan = 0u;
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {  // uniform over the work-group
            for (unsigned j = 0; j < REG_RUN / REG_THREADS; ++j) {       // the same trip count for every lane: converged ballots
                const u64 i64 = (u64)run * REG_RUN + j * REG_THREADS + threadIdx.x;
                const bool valid = i64 < p.npix;
                const unsigned i = (unsigned)i64;
                const unsigned bits = valid ? __float_as_uint(V[i]) : 0u;
                const int lab = valid ? L[i] : 0;
                nnan += (bits & 0x7fffffffu) > 0x7f800000u ? 1u : 0u;
                nfg += lab != 0 ? 1u : 0u;
                unsigned slot = 0u;
                if (lab != 0) {
                    const unsigned root = (unsigned)lab - 1u;
                    slot = root < p.npix ? slots[root] : 0u;            // a label is a root of this frame: always inside
                    if (slot > p.max_regions) slot = 0u;                 // never, short of a defect: no address is formed from it
                }
                // another region than the one gathered so far: that one goes to its record first
                regions_flush(acc.slot != 0u && slot != 0u && slot != acc.slot, acc, rec, lane);
                if (slot != 0u) {
                    const unsigned y = i / p.w, x = i - y * p.w;
                    acc.add(slot, x, y, ((u64)order_key(bits) << 32) | (u64)(~i), 0u);
                }
            }
        }
        regions_flush(acc.slot != 0u, acc, rec, lane);
        nfg = wave_sum(nfg);
        nnan = wave_sum(nnan);
        if (lane == 0u) {
            if (nfg) atomicAdd(p.counts + img * 4 + 2, nfg);
            if (nnan) atomicAdd(p.counts + img * 4 + 3, nnan);
        }
    }
}

// the peak word of a record in use -> float bits, index; every record behind the frame's last one -> zeros
__global__ __launch_bounds__(REG_THREADS) void regions_finish_kernel(RegionP p) {
    const u64 total = (u64)p.n * p.max_regions;
    for (u64 k = (u64)blockIdx.x * REG_THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * REG_THREADS) {
        const u64 img = k / p.max_regions;
        const unsigned r = (unsigned)(k - img * p.max_regions);
        unsigned* rec = p.records + k * VAD_REGION_WORDS;
        if (r < p.counts[img * 4]) {                                     // kept may exceed max_regions; r does not
            const unsigned not_index = rec[6], key = rec[7];
            rec[6] = order_key_inv(key);
            rec[7] = ~not_index;
        } else {
            *(u32x4*)rec = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(rec + 4) = u32x4{0u, 0u, 0u, 0u};
            *(u32x4*)(rec + 8) = u32x4{0u, 0u, 0u, 0u};
        }
    }
}

}  // namespace

size_t vad_regions_workspace_bytes(long long n, int h, int w, int labels_given) {
    long long total = 0;
    if (!vad_label_dims_ok(n, h, w, &total) || (labels_given != 0 && labels_given != 1)) return 0;
    return region_head_bytes(n, (long long)h * w, 1) + (size_t)(labels_given ? 8 : 12) * (size_t)total;   // [labels,] sizes, slots: 4 bytes each
}

int vad_detect_regions(const float* maps, long long n, int h, int w, float threshold, int connectivity, unsigned min_area,
                       int max_regions, int32_t* labels_or_null, uint32_t* records, uint32_t* counts, void* ws, size_t ws_bytes,
                       void* stream) {
    const char* who = "detect_regions";
    long long total = 0;
    VAD_ARG(vad_req_ptr(who, "maps", maps, 4));
    VAD_ARG(vad_req_label_n(who, "n", n));
    VAD_ARG(vad_req_label_hw(who, h, w));
    VAD_ARG(vad_req_label_total(who, n, h, w, &total));
    VAD_ARG(vad_req_threshold(who, threshold));
    VAD_ARG(vad_req_connectivity(who, connectivity));
    VAD_ARG(vad_req_nonzero(who, "min_area", min_area));
    VAD_ARG(vad_req_capacity(who, "max_regions", max_regions, REG_MAX_REGIONS));
    VAD_ARG(vad_req_aligned(who, "labels", labels_or_null, 4));
    VAD_ARG(vad_req_ptr(who, "records", records, 16));
    VAD_ARG(vad_req_ptr(who, "counts", counts, 4));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    const int given = labels_or_null != nullptr ? 1 : 0;
    VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, vad_regions_workspace_bytes(n, h, w, given), "vad_regions_workspace_bytes(%lld, %d, %d, %d)", n, h, w, given);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {                                            // nothing to detect: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, VAD_LABEL_WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    unsigned* flags = (unsigned*)ws;
    unsigned* planes = (unsigned*)((char*)ws + region_head_bytes(n, (long long)h * w, 1));
    int* labels = given ? labels_or_null : (int*)planes;
    unsigned* sizes = given ? planes : planes + total;
    if (int rc = vad_label_launch(maps, VAD_LABEL_FMT_F32_GE, threshold, n, h, w, connectivity, labels, sizes, flags, s)) return rc;

    RegionP p;
    p.maps = maps;
    p.labels = labels;
    p.sizes = sizes;
    p.slots = sizes + total;
    p.chunk_kept = (unsigned*)((char*)ws + VAD_LABEL_WS_HEAD_BYTES);
    p.records = records;
    p.counts = counts;
    p.n = n;
    p.npix = (unsigned)h * (unsigned)w;
    p.nchunks = region_chunks((long long)h * w);
    p.w = (unsigned)w;
    p.min_area = min_area;
    p.max_regions = (unsigned)max_regions;
    VAD_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * 16, s));
    const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
    const dim3 chunk_grid(p.nchunks < REG_MAX_BLOCKS_X ? p.nchunks : REG_MAX_BLOCKS_X, gy);
    hipLaunchKernelGGL(regions_count_kernel, chunk_grid, dim3(REG_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    hipLaunchKernelGGL(regions_slot_kernel, chunk_grid, dim3(REG_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned nruns = (p.npix + REG_RUN - 1u) / REG_RUN;
    hipLaunchKernelGGL(regions_reduce_kernel, dim3(nruns < REG_MAX_BLOCKS_X ? nruns : REG_MAX_BLOCKS_X, gy), dim3(REG_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    const unsigned long long recs = (unsigned long long)n * p.max_regions;
    const unsigned long long fin = (recs + REG_THREADS - 1) / REG_THREADS;
    hipLaunchKernelGGL(regions_finish_kernel, dim3((unsigned)(fin < 65536ull ? fin : 65536ull)), dim3(REG_THREADS), 0, s, p);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}
