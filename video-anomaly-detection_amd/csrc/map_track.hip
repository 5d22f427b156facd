// Anomaly events across the calls of a live stream: the events of csrc/map_events.hip - connected
// components of {v >= threshold} in the volume of a stream - continued frame by frame, with the state between calls in a
// caller-owned device blob: a header (the frame counter lives on the device, so a captured call can be replayed), the table of the
// events still open (slot r = the open event whose handle - its smallest pixel in the newest frame - has rank r in raster order) and
// the slot plane of the newest frame (0, slot + 1, or TR_NO_RECORD for an open event behind the table).  A call continues b streams
// by t new maps each and returns the events that closed, filtered and in ascending (t1, handle) order, and the causal alarm word of
// every new frame.
//
//   zero       counts, frame counts and the flag word (a kernel: no memset node in a captured call)
//   label      the labeller of region_label.h on the call's b * t frames, once; then, frame after frame:
//   begin      the frame counter advances, minroot[slot] = none
//   link-min   every foreground pixel looks behind it in the slot plane (the pixel behind it; under temporal 9 with that pixel
//              unset, the 3 x 3's ring) and writes atomicMin(minroot[slot], its frame root), once per distinct pair of a wave
//   link-union the same walk unites the pixel's root with minroot[slot]: the regions that share an open event are one set, whose
//              root - its smallest pixel - is the event's new handle
//   flatten    every pixel directly under its handle; the handles of every chunk of TR_CHUNK pixels are counted
//   slot       rank scan over the chunks (chunk_before, chunk_rank_row of region_table.h): handle of rank r < max_open -> slot r + 1 and a cleared working record; behind the table
//              -> TR_NO_RECORD, counted as lost
//   carry      one work-group per stream over the old table (in a call's first frame it zeroes the closed table first): an old
//              event whose minroot leads to a handle merges its record into that handle's working record (64-bit adds, a 64-bit min on (t0, root pixel), box min / max, the peak as a max on the
//              key followed - after a barrier - by a min on (frame, pixel) among the holders of that key); one without a link
//              closed: it is ranked among the closed of this frame by a scan over the slots, filtered and appended
//   reduce     the new frame's pixels into the working records (RegionAcc of region_table.h: gathered per lane, combined per wave), the frame's foreground and
//              NaN counts, the new slot plane
//   finish     working records -> the state's table (peak resolved: the new frame wins only with a larger key), unused records
//              zeroed, the causal alarm word, the header's open count
// Integer atomics, min and max only: every output and the state are the same words for any batching of streams and any split of
// the frames over calls.  Every launch is asynchronous on the caller's stream, nothing is allocated, the host never waits, no
// cooperative launch, no loop without a bound known at launch.
#include <hip/hip_runtime.h>

#include "region_table.h"
#include "vad_args.h"
#include "vad_common.h"

namespace {

constexpr int TR_THREADS = REGION_THREADS;
constexpr unsigned TR_CHUNK = REGION_CHUNK;
constexpr unsigned TR_RUN = 1024;               // pixels a work-group of the link and reduce passes takes at a time
constexpr unsigned TR_PIXEL_BLOCKS_X = 256;     // link-min, link-union, reduce: 2^18 pixels of a frame per grid round
constexpr unsigned TR_SCAN_BLOCKS_X = 256;      // flatten, slot: 2^18 pixels per round
constexpr unsigned TR_TABLE_BLOCKS_X = 64;      // begin, finish: 2^14 slots per round
constexpr int TR_MAX_OPEN = 65536, TR_MAX_CLOSED = 65536;
constexpr long long TR_MAX_PIXELS = 1ll << 24;  // (frame << 32 | pixel) and the 24-bit pixel index of the kernels
constexpr unsigned TR_NO_RECORD = 0xffffffffu;
constexpr unsigned TR_NONE = 0xffffffffu;
constexpr unsigned TR_HEADER_WORDS = 16;        // frames, open, lost in total, flags, magic, h, w, max_open, zeros
constexpr unsigned TR_MAGIC = 0x54444156u;      // "VADT"
constexpr unsigned TR_WORK_WORDS = 24;
// the working record of an open event while a frame is taken in (uint32 words)
constexpr unsigned WK_T0ROOT = 0;               // u64 min: t0 << 32 | root pixel
constexpr unsigned WK_HANDLE = 2, WK_NFRAME = 3, WK_X0 = 4, WK_Y0 = 5, WK_X1 = 6, WK_Y1 = 7;
constexpr unsigned WK_OLDKEY = 8;               // max over the merged old records' peak keys; 0 = none (no foreground value has key 0)
constexpr unsigned WK_OLDPOS = 10;              // u64 min: peak frame << 32 | peak pixel among the holders of WK_OLDKEY
constexpr unsigned WK_VOLUME = 12, WK_SX = 14, WK_SY = 16, WK_ST = 18;   // u64 sums
constexpr unsigned WK_NEWPEAK = 20;             // u64 max over the new frame: key << 32 | ~pixel
// the record of the C ABI (include/vad_hip.h)
constexpr unsigned RC_ROOT = 0, RC_T0 = 1, RC_T1 = 2, RC_HANDLE = 3, RC_X0 = 4, RC_PEAK = 8, RC_PEAK_PIXEL = 9, RC_PEAK_FRAME = 10;
constexpr unsigned RC_VOLUME = 12, RC_SX = 14, RC_SY = 16, RC_ST = 18;
static_assert(VAD_TRACK_WORDS == 20, "the record layout above");

struct TrackP {
    const float* maps;       // [b][t][npix]
    int* labels;             // [b][t][npix]: 0, or 1 + parent inside the frame
    unsigned* state;         // [b][state_words]: header, table [max_open][20], plane [npix]
    unsigned* minroot;       // [b][max_open]: link passes: the smallest frame root that touches the slot; carry: the slot's fate
    unsigned* chunk_n;       // [b][nchunks]: handles per chunk
    unsigned* newslot;       // [b][npix]: at a handle, its new slot + 1 or TR_NO_RECORD
    unsigned* work;          // [b][max_open][TR_WORK_WORDS]
    unsigned* nopen;         // [b]: open events with a record after this frame
    unsigned* closed;        // [b][max_closed][20]
    unsigned* counts;        // [b][6]
    unsigned* frame_counts;  // [b][t][3]
    unsigned* flags;
    long long b;
    size_t state_words;
    unsigned t, j, npix, w, h, nchunks, max_open, max_closed, min_duration, min_volume;
    int temporal, flush;
};

__device__ __forceinline__ unsigned* tr_header(const TrackP& p, long long s) { return p.state + (size_t)s * p.state_words; }
__device__ __forceinline__ unsigned* tr_table(const TrackP& p, long long s) { return tr_header(p, s) + TR_HEADER_WORDS; }
__device__ __forceinline__ unsigned* tr_plane(const TrackP& p, long long s) {
    return tr_table(p, s) + (size_t)p.max_open * VAD_TRACK_WORDS;
}
__device__ __forceinline__ int* tr_labels(const TrackP& p, long long s) { return p.labels + ((size_t)s * p.t + p.j) * p.npix; }

__device__ __forceinline__ void tr_fail(const TrackP& p, long long s) {
    atomicOr(p.flags, VAD_LABEL_FLAG_WALK);
    atomicOr(tr_header(p, s) + 3, VAD_LABEL_FLAG_WALK);
}

// init / reset, and the end of a flush: table and plane zeroed; with `header`, a fresh header
__global__ __launch_bounds__(TR_THREADS) void track_clear_kernel(TrackP p, int header) {
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        unsigned* st = tr_header(p, s);
        for (size_t i = (size_t)blockIdx.x * TR_THREADS + threadIdx.x; i < p.state_words; i += (size_t)gridDim.x * TR_THREADS) {
            unsigned v = 0u;
            if (i < TR_HEADER_WORDS) {
                if (!header && i != 1u) continue;                        // a flush keeps the counter and the sticky words
                v = i == 4u ? TR_MAGIC : i == 5u ? p.h : i == 6u ? p.w : i == 7u ? p.max_open : 0u;
            }
            st[i] = v;
        }
        if (!header && blockIdx.x == 0 && threadIdx.x == 0) p.counts[s * 6 + 4] = 0u;
    }
}

// the call's counts, frame counts and flag word.  A kernel, not memset nodes: the call is meant to be captured and replayed
__global__ __launch_bounds__(TR_THREADS) void track_zero_kernel(TrackP p) {
    const size_t nc = (size_t)p.b * 6u, nf = (size_t)p.b * p.t * 3u;
    for (size_t i = (size_t)blockIdx.x * TR_THREADS + threadIdx.x; i < nc + nf; i += (size_t)gridDim.x * TR_THREADS) {
        if (i < nc) p.counts[i] = 0u;
        else p.frame_counts[i - nc] = 0u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) p.flags[0] = 0u;
}

__global__ __launch_bounds__(TR_THREADS) void track_begin_kernel(TrackP p) {
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        unsigned* m = p.minroot + (size_t)s * p.max_open;
        for (unsigned r = blockIdx.x * TR_THREADS + threadIdx.x; r < p.max_open; r += gridDim.x * TR_THREADS) m[r] = TR_NONE;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            unsigned* hd = tr_header(p, s);
            if (hd[0] == 0xffffffffu) {                                  // the counter is at its end: sticky, and nothing advances
                hd[3] |= VAD_TRACK_FLAG_COUNTER;
                atomicOr(p.flags, VAD_TRACK_FLAG_COUNTER);
            } else {
                hd[0] += 1u;
            }
        }
    }
}

// the slot of the 3 x 3's ring pixel k around (y, x) in the plane before, or 0
__device__ __forceinline__ unsigned track_ring_slot(const unsigned* P, unsigned i, unsigned y, unsigned x, unsigned h, unsigned w, int k) {
    return ring_inside(y, x, h, w, k) ? P[(int)i + ring_dy(k) * (int)w + ring_dx(k)] : 0u;
}

// link-min (UNION = false) and link-union (UNION = true): the same walk over the new frame's foreground pixels
template <bool UNION>
__global__ __launch_bounds__(TR_THREADS) void track_link_kernel(TrackP p) {
    const unsigned npix = p.npix, w = p.w, h = p.h;
    const unsigned budget = 2u * npix + 2u;                              // npix <= 2^24
    const unsigned nruns = (npix + TR_RUN - 1u) / TR_RUN;
    const unsigned lane = threadIdx.x & 63u;
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        int* L = tr_labels(p, s);
        const unsigned* P = tr_plane(p, s);
        unsigned* M = p.minroot + (size_t)s * p.max_open;
        bool failed = false;
        // the trip counts are the same for every lane of the work-group: the ballots run in converged control flow
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x)
        for (unsigned j = 0; j < TR_RUN / TR_THREADS; ++j) {
            const unsigned i = run * TR_RUN + j * TR_THREADS + threadIdx.x;
            const int lab = i < npix ? L[i] : 0;
            const bool fg = lab != 0;
            // whether a pixel is foreground never changes; its parent after the labelling is its frame root, later an ancestor
            const unsigned root = fg ? (unsigned)label_load(L + i) - 1u : 0u;
            const unsigned centre = fg ? P[i] : 0u;
            const bool direct = centre - 1u < p.max_open;                // a slot with a record (0 and TR_NO_RECORD are not)
            if (wave_elect_pair(direct, centre, root, lane)) {
                if (!UNION) {
                    atomicMin(M + (centre - 1u), root);
                } else {
                    const unsigned m = M[centre - 1u];
                    if (m != root && m < npix) failed |= !label_union(L, root, m, budget);
                }
            }
            // Under temporal 9 a set pixel behind holds the one event of its 3 x 3 (8-connectivity); with a lost event behind, the
            // 3 x 3 holds lost pixels only.  With nothing behind, the ring: at most four distinct events.
            if (!fg || centre != 0u || p.temporal != 9) continue;
            const unsigned y = i / w, x = i - y * w;
            unsigned prev = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned slot = track_ring_slot(P, i, y, x, h, w, k);
                if (slot - 1u < p.max_open && slot != prev) {
                    if (!UNION) {
                        atomicMin(M + (slot - 1u), root);
                    } else {
                        const unsigned m = M[slot - 1u];
                        if (m != root && m < npix) failed |= !label_union(L, root, m, budget);
                    }
                }
                prev = slot;
            }
        }
        if (failed) tr_fail(p, s);
    }
}

// every pixel directly under its handle; handles per chunk
__global__ __launch_bounds__(TR_THREADS) void track_flatten_kernel(TrackP p) {
    __shared__ unsigned s_n[1];
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        int* L = tr_labels(p, s);
        bool failed = false;
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            block_sum_clear<1>(s_n);
            unsigned n[1] = {0u};
            for (unsigned j = 0; j < TR_CHUNK / TR_THREADS; ++j) {
                const unsigned i = c * TR_CHUNK + j * TR_THREADS + threadIdx.x;
                if (i < p.npix && L[i] != 0) {
                    unsigned budget = p.npix + 1u;
                    const unsigned root = label_find(L, i, budget);
                    failed |= budget == 0u;
                    // a root keeps its value; any other pixel gets an ancestor of its old parent, so concurrent chases stay valid
                    if (root != i) __hip_atomic_store(L + i, (int)(root + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else ++n[0];
                }
            }
            block_sum(n, s_n);
            if (threadIdx.x == 0) p.chunk_n[(size_t)s * p.nchunks + c] = n[0];
            __syncthreads();                                             // s_n is cleared again for the next chunk
        }
        if (failed) tr_fail(p, s);
    }
}

// ranks of the handles in raster order; the working records' identities
__global__ __launch_bounds__(TR_THREADS) void track_slot_kernel(TrackP p) {
    __shared__ unsigned s_before[1], s_wave[1][REGION_WAVES];
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        const int* L = tr_labels(p, s);
        const unsigned* n_of = p.chunk_n + (size_t)s * p.nchunks;
        unsigned* S = p.newslot + (size_t)s * p.npix;
        unsigned* work = p.work + (size_t)s * p.max_open * TR_WORK_WORDS;
        unsigned* hd = tr_header(p, s);
        const unsigned f = hd[0] - 1u;                                   // the frame's number: begin advanced the counter
        for (unsigned c = blockIdx.x; c < p.nchunks; c += gridDim.x) {   // uniform over the work-group
            unsigned base[1];                                            // the handles of this frame in front of the chunk
            chunk_before(n_of, c, base, s_before);
            // the frame's last chunk has summed the whole frame: its work-group writes the open and the lost count
            if (c + 1u == p.nchunks && threadIdx.x == 0) {
                const unsigned total = base[0] + n_of[c];
                const unsigned open = total < p.max_open ? total : p.max_open;
                p.nopen[s] = open;
                if (total > open) {
                    atomicAdd(p.counts + s * 6 + 5, total - open);
                    hd[2] += total - open;                               // sticky; no other thread touches the word in this launch
                }
            }
            for (unsigned j = 0; j < TR_CHUNK / TR_THREADS; ++j) {
                const unsigned i = c * TR_CHUNK + j * TR_THREADS + threadIdx.x;
                const bool handle = i < p.npix && L[i] == (int)(i + 1u);
                const unsigned rank = chunk_rank_row(handle, base[0], s_wave);
                if (handle && rank < p.max_open) {
                    S[i] = rank + 1u;
                    unsigned* r = work + (size_t)rank * TR_WORK_WORDS;
                    *(u32x4*)r = u32x4{i, f, i, 0u};                                 // (t0, root pixel) = (f, handle); handle; pixels of the frame
                    *(u32x4*)(r + 4) = u32x4{0xffffffffu, 0xffffffffu, 0u, 0u};     // x0, y0 (min), x1, y1 (max)
                    *(u32x4*)(r + 8) = u32x4{0u, 0u, 0xffffffffu, 0xffffffffu};     // old key (max), -, old position (min)
                    *(u32x4*)(r + 12) = u32x4{0u, 0u, 0u, 0u};                      // volume, sum x
                    *(u32x4*)(r + 16) = u32x4{0u, 0u, 0u, 0u};                      // sum y, sum t
                    *(u32x4*)(r + 20) = u32x4{0u, 0u, 0u, 0u};                      // new peak (max), -
                } else if (handle) {
                    S[i] = TR_NO_RECORD;
                }
            }
        }
    }
}

// the old table: merged into the handles' working records, or closed
__global__ __launch_bounds__(TR_THREADS) void track_carry_kernel(TrackP p) {
    __shared__ unsigned s_wave[TR_THREADS / 64][2];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (long long s = blockIdx.x; s < p.b; s += gridDim.x) {
        const unsigned* hd = tr_header(p, s);
        const unsigned* table = tr_table(p, s);
        unsigned* M = p.minroot + (size_t)s * p.max_open;
        unsigned* work = p.work + (size_t)s * p.max_open * TR_WORK_WORDS;
        const unsigned nold = hd[1] < p.max_open ? hd[1] : p.max_open;   // never more: no address past the table is formed
        unsigned* out = p.closed + (size_t)s * p.max_closed * VAD_TRACK_WORDS;
        bool failed = false;
        // the call's first frame: this work-group, the only one that writes the stream's closed table, zeroes it first (the barrier
        // between phases A and B lies before every record it writes)
        if (p.j == 0u)
            for (unsigned k = threadIdx.x; k < p.max_closed * (VAD_TRACK_WORDS / 4u); k += TR_THREADS) ((u32x4*)out)[k] = u32x4{0u, 0u, 0u, 0u};
        // phase A: the fate of every old slot (0 = closed, a new slot + 1, or TR_NO_RECORD: continued behind the table - lost);
        // sums, box, (t0, root) and the peak's key into the working record
        for (unsigned r = threadIdx.x; r < nold; r += TR_THREADS) {
            unsigned fate = 0u;
            if (!p.flush && M[r] != TR_NONE) {
                const int* L = tr_labels(p, s);
                unsigned budget = p.npix + 1u;
                const unsigned m = M[r];
                const unsigned handle = m < p.npix ? label_find(L, m, budget) : 0u;
                failed |= budget == 0u || m >= p.npix;
                fate = p.newslot[(size_t)s * p.npix + handle];
                if (fate - 1u >= p.max_open) fate = TR_NO_RECORD;
            }
            M[r] = fate;
            if (fate - 1u < p.max_open) {
                const unsigned* o = table + (size_t)r * VAD_TRACK_WORDS;
                unsigned* n = work + (size_t)(fate - 1u) * TR_WORK_WORDS;
                atomicMin((u64*)(n + WK_T0ROOT), ((u64)o[RC_T0] << 32) | o[RC_ROOT]);
                atomicMin(n + WK_X0, o[RC_X0]);
                atomicMin(n + WK_Y0, o[RC_X0 + 1]);
                atomicMax(n + WK_X1, o[RC_X0 + 2]);
                atomicMax(n + WK_Y1, o[RC_X0 + 3]);
                atomicMax(n + WK_OLDKEY, order_key(o[RC_PEAK]));
                atomicAdd((u64*)(n + WK_VOLUME), *(const u64*)(o + RC_VOLUME));
                atomicAdd((u64*)(n + WK_SX), *(const u64*)(o + RC_SX));
                atomicAdd((u64*)(n + WK_SY), *(const u64*)(o + RC_SY));
                atomicAdd((u64*)(n + WK_ST), *(const u64*)(o + RC_ST));
            }
        }
        if (failed) tr_fail(p, s);
        __threadfence();
        __syncthreads();
        // phase B: among the old records that hold the largest key, the earliest frame, then the smallest pixel
        for (unsigned r = threadIdx.x; r < nold; r += TR_THREADS) {
            const unsigned fate = M[r];
            if (fate - 1u < p.max_open) {
                const unsigned* o = table + (size_t)r * VAD_TRACK_WORDS;
                unsigned* n = work + (size_t)(fate - 1u) * TR_WORK_WORDS;
                if (order_key(o[RC_PEAK]) == __hip_atomic_load(n + WK_OLDKEY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    atomicMin((u64*)(n + WK_OLDPOS), ((u64)o[RC_PEAK_FRAME] << 32) | o[RC_PEAK_PIXEL]);
            }
        }
        // phase C: the closed events in slot order - the order of their handles in their last frame -, filtered, appended
        // The ballot scan is written out here, not through chunk_rank_row of region_table.h: this is the one work-group of the
        // stream and every round of the scan is on its critical path; through the helper the kernel measured 8 - 18 % slower on
        // frames of many small events (profiles/region_table_ab.json), so this call site keeps the form it had.
        unsigned kept_base = p.counts[s * 6], dropped_n = 0u;            // read by every thread before thread 0 writes it (barriers below)
        for (unsigned r0 = 0; r0 < nold; r0 += TR_THREADS) {             // uniform over the work-group
            const unsigned r = r0 + threadIdx.x;
            const bool closed = r < nold && M[r] == 0u;
            const unsigned* o = table + (size_t)(closed ? r : 0u) * VAD_TRACK_WORDS;
            const bool kept = closed && o[RC_T1] - o[RC_T0] + 1u >= p.min_duration && *(const u64*)(o + RC_VOLUME) >= (u64)p.min_volume;
            const u64 bk = __ballot(kept), bd = __ballot(closed && !kept);
            if (lane == 0u) {
                s_wave[wave][0] = (unsigned)__builtin_popcountll(bk);
                s_wave[wave][1] = (unsigned)__builtin_popcountll(bd);
            }
            __syncthreads();
            unsigned rank = kept_base + (unsigned)__builtin_popcountll(bk & ((1ull << lane) - 1ull));
            for (unsigned k = 0; k < TR_THREADS / 64; ++k) {
                if (k < wave) rank += s_wave[k][0];
                kept_base += s_wave[k][0];
                dropped_n += s_wave[k][1];
            }
            __syncthreads();                                             // s_wave is written again in the next round
            if (kept && rank < p.max_closed) {
                unsigned* d = out + (size_t)rank * VAD_TRACK_WORDS;
                for (unsigned k = 0; k < VAD_TRACK_WORDS; k += 4) *(u32x4*)(d + k) = *(const u32x4*)(o + k);
            }
        }
        if (threadIdx.x == 0) {
            p.counts[s * 6] = kept_base;
            p.counts[s * 6 + 1] += dropped_n;
        }
        __syncthreads();
    }
}

static_assert(WK_Y0 == WK_X0 + 1 && WK_X1 == WK_X0 + 2 && WK_Y1 == WK_X0 + 3 && WK_SY == WK_SX + 2, "the words RegionAcc::commit writes");

// Adds the lanes' gathered values (sw: the pixel count) to their working records: `pending` lanes hold a slot in 1 .. max_open,
// equal slots of the wave are combined first.
__device__ __forceinline__ void track_flush(bool pending, const RegionAcc<unsigned>& a, unsigned* work, unsigned f, unsigned lane) {
    wave_each_key(pending, a.slot, lane, [&](unsigned first, bool mine, bool many, bool lead) {
        const RegionAcc<unsigned> c = a.combined(mine, many);
        if (lead) {
            unsigned* r = work + (size_t)(first - 1u) * TR_WORK_WORDS;
            c.commit(r, WK_X0, WK_NEWPEAK, WK_SX);
            atomicAdd(r + WK_NFRAME, c.sw);
            atomicAdd((u64*)(r + WK_VOLUME), (u64)c.sw);
            atomicAdd((u64*)(r + WK_ST), (u64)c.sw * f);
        }
    });
}

__global__ __launch_bounds__(TR_THREADS) void track_reduce_kernel(TrackP p) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nruns = (p.npix + TR_RUN - 1u) / TR_RUN;
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        const float* V = p.maps + ((size_t)s * p.t + p.j) * p.npix;
        const int* L = tr_labels(p, s);
        const unsigned* S = p.newslot + (size_t)s * p.npix;
        unsigned* P = tr_plane(p, s);
        unsigned* work = p.work + (size_t)s * p.max_open * TR_WORK_WORDS;
        const unsigned f = tr_header(p, s)[0] - 1u;
        RegionAcc<unsigned> acc;                                         // sw: the pixel count
        acc.clear();
        unsigned nfg = 0u, nnan = 0u;
        for (unsigned run = blockIdx.x; run < nruns; run += gridDim.x) {  // uniform over the work-group
            for (unsigned j = 0; j < TR_RUN / TR_THREADS; ++j) {         // the same trip count for every lane: converged ballots
                const unsigned i = run * TR_RUN + j * TR_THREADS + threadIdx.x;
                const bool valid = i < p.npix;
                const unsigned bits = valid ? __float_as_uint(V[i]) : 0u;
                const int lab = valid ? L[i] : 0;
                unsigned slot = 0u;
                if (lab != 0) {
                    const unsigned handle = (unsigned)lab - 1u;
                    slot = handle < p.npix ? S[handle] : 0u;             // a label is a handle of this frame: always inside
                }
                if (valid) P[i] = slot;                                  // 0, slot + 1 or TR_NO_RECORD
                nnan += (bits & 0x7fffffffu) > 0x7f800000u ? 1u : 0u;
                nfg += lab != 0 ? 1u : 0u;
                if (slot - 1u >= p.max_open) slot = 0u;                  // no record: no address is formed from it
                // another event than the one gathered so far: that one goes to its record first
                track_flush(acc.slot != 0u && slot != 0u && slot != acc.slot, acc, work, f, lane);
                if (slot != 0u) {
                    const unsigned y = i / p.w, x = i - y * p.w;
                    acc.add(slot, x, y, ((u64)order_key(bits) << 32) | (u64)(~i), 1u);
                }
            }
        }
        track_flush(acc.slot != 0u, acc, work, f, lane);
        nfg = wave_sum(nfg);
        nnan = wave_sum(nnan);
        if (lane == 0u) {
            unsigned* fc = p.frame_counts + ((size_t)s * p.t + p.j) * 3u;
            if (nfg) {
                atomicAdd(p.counts + s * 6 + 2, nfg);
                atomicAdd(fc, nfg);
            }
            if (nnan) {
                atomicAdd(p.counts + s * 6 + 3, nnan);
                atomicAdd(fc + 2, nnan);
            }
        }
    }
}

// working records -> the state's table; the causal alarm word; the header's open count
__global__ __launch_bounds__(TR_THREADS) void track_finish_kernel(TrackP p) {
    for (long long s = blockIdx.y; s < p.b; s += gridDim.y) {
        unsigned* hd = tr_header(p, s);
        unsigned* table = tr_table(p, s);
        const unsigned* work = p.work + (size_t)s * p.max_open * TR_WORK_WORDS;
        const unsigned nopen = p.nopen[s];                               // <= max_open
        const unsigned f = hd[0] - 1u;                                   // no thread of this launch writes the counter
        unsigned alarm = 0u;
        for (unsigned r = blockIdx.x * TR_THREADS + threadIdx.x; r < p.max_open; r += gridDim.x * TR_THREADS) {
            unsigned* d = table + (size_t)r * VAD_TRACK_WORDS;
            if (r < nopen) {
                const unsigned* k = work + (size_t)r * TR_WORK_WORDS;
                const unsigned t0 = k[WK_T0ROOT + 1];
                const u64 volume = *(const u64*)(k + WK_VOLUME);
                const unsigned newkey = k[WK_NEWPEAK + 1], oldkey = k[WK_OLDKEY];
                const bool fresh = newkey > oldkey;                      // a tie goes to the earlier frame
                *(u32x4*)d = u32x4{k[WK_T0ROOT], t0, f, k[WK_HANDLE]};
                *(u32x4*)(d + 4) = *(const u32x4*)(k + WK_X0);
                *(u32x4*)(d + 8) = u32x4{order_key_inv(fresh ? newkey : oldkey), fresh ? ~k[WK_NEWPEAK] : k[WK_OLDPOS], fresh ? f : k[WK_OLDPOS + 1], 0u};
                *(u32x4*)(d + 12) = *(const u32x4*)(k + WK_VOLUME);
                *(u32x4*)(d + 16) = *(const u32x4*)(k + WK_SY);
                if (f - t0 + 1u >= p.min_duration && volume >= (u64)p.min_volume) alarm += k[WK_NFRAME];
            } else {
                for (unsigned q = 0; q < VAD_TRACK_WORDS; q += 4) *(u32x4*)(d + q) = u32x4{0u, 0u, 0u, 0u};
            }
        }
        alarm = wave_sum(alarm);
        if ((threadIdx.x & 63u) == 0u && alarm) atomicAdd(p.frame_counts + ((size_t)s * p.t + p.j) * 3u + 1u, alarm);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            hd[1] = nopen;
            p.counts[s * 6 + 4] = nopen;
        }
    }
}

bool track_dims_ok(long long b, int h, int w, int max_open) {
    return b >= 0 && b <= (1ll << 20) && h >= 1 && w >= 1 && (long long)h * w <= TR_MAX_PIXELS && max_open >= 1 && max_open <= TR_MAX_OPEN;
}

size_t track_state_words(int h, int w, int max_open) {
    const size_t words = TR_HEADER_WORDS + (size_t)max_open * VAD_TRACK_WORDS + (size_t)h * w;
    return (words + 3) & ~(size_t)3;                                     // every stream's blob 16-byte aligned
}

size_t track_pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

unsigned track_grid_x(unsigned long long items, unsigned cap) { return (unsigned)(items < cap ? (items ? items : 1) : cap); }

struct TrackWs {
    size_t labels, minroot, chunk_n, newslot, work, nopen, total;       // byte offsets
};

// one carve for the size and for the pointers; t = 0 (flush) needs no labels
TrackWs track_carve(long long b, int t, int h, int w, int max_open) {
    const size_t npix = (size_t)h * w;
    TrackWs c;
    size_t at = VAD_LABEL_WS_HEAD_BYTES;
    c.labels = at;
    at += track_pad16((size_t)b * t * npix * 4);
    c.minroot = at;
    at += track_pad16((size_t)b * max_open * 4);
    c.chunk_n = at;
    at += region_chunk_bytes(b, (long long)npix, 1);
    c.newslot = at;
    at += track_pad16((size_t)b * npix * 4);
    c.work = at;
    at += (size_t)b * max_open * TR_WORK_WORDS * 4;
    c.nopen = at;
    at += track_pad16((size_t)b * 4);
    c.total = at;
    return c;
}

int track_run(const char* who, const float* maps, long long b, int t, int h, int w, float threshold, int connectivity, int temporal,
              unsigned min_duration, unsigned min_volume, int max_open, int max_closed, void* state, uint32_t* closed, uint32_t* counts,
              uint32_t* frame_counts, void* ws, size_t ws_bytes, void* stream) {
    const bool flush = t == 0;
    if (!flush) VAD_ARG(vad_req_nonnull(who, "maps", maps));
    VAD_ARG(vad_req_aligned(who, "maps", maps, 4));
    VAD_REQUIRE(b >= 0 && b <= (1ll << 20), "%s: b must be in 0..2^20, got %lld", who, b);
    if (!flush) VAD_ARG(vad_req_t(who, t));
    VAD_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= TR_MAX_PIXELS, "%s: h and w must be >= 1 with h * w <= 2^24, got %d x %d", who, h, w);
    VAD_REQUIRE(flush || (long long)b * t * ((long long)h * w) <= (1ll << 38), "%s: b * t * h * w must be at most 2^38 (%lld x %d x %d x %d)", who,
                b, t, h, w);
    VAD_ARG(vad_req_threshold(who, threshold));
    VAD_ARG(vad_req_connectivity(who, connectivity));
    VAD_REQUIRE(temporal == 1 || temporal == 9, "%s: temporal must be 1 or 9, got %d", who, temporal);
    VAD_REQUIRE(temporal == 1 || connectivity == 8, "%s: temporal 9 needs connectivity 8, got connectivity %d", who, connectivity);
    VAD_ARG(vad_req_nonzero(who, "min_duration", min_duration));
    VAD_ARG(vad_req_nonzero(who, "min_volume", min_volume));
    VAD_ARG(vad_req_capacity(who, "max_open", max_open, TR_MAX_OPEN));
    VAD_ARG(vad_req_capacity(who, "max_closed", max_closed, TR_MAX_CLOSED));
    VAD_ARG(vad_req_ptr(who, "state", state, 16));
    VAD_ARG(vad_req_ptr(who, "closed", closed, 16));
    VAD_ARG(vad_req_ptr(who, "counts", counts, 4));
    if (!flush) VAD_ARG(vad_req_nonnull(who, "frame_counts", frame_counts));
    VAD_ARG(vad_req_aligned(who, "frame_counts", frame_counts, 4));
    VAD_ARG(vad_req_ptr(who, "ws", ws, 16));
    const TrackWs c = track_carve(b, t, h, w, max_open);
    VAD_REQUIRE_WS(VAD_ERR_WS, who, ws_bytes, c.total, "vad_track_workspace_bytes(%lld, %d, %d, %d, %d)", b, t, h, w, max_open);
    const hipStream_t s = (hipStream_t)stream;
    if (b == 0) {                                            // nothing to track: the flag word still reads "no defect"
        VAD_HIP_TRY(hipMemsetAsync(ws, 0, VAD_LABEL_WS_HEAD_BYTES, s));
        return VAD_OK;
    }
    char* base = (char*)ws;
    TrackP p;
    p.maps = maps;
    p.labels = (int*)(base + c.labels);
    p.state = (unsigned*)state;
    p.minroot = (unsigned*)(base + c.minroot);
    p.chunk_n = (unsigned*)(base + c.chunk_n);
    p.newslot = (unsigned*)(base + c.newslot);
    p.work = (unsigned*)(base + c.work);
    p.nopen = (unsigned*)(base + c.nopen);
    p.closed = closed;
    p.counts = counts;
    p.frame_counts = frame_counts;
    p.flags = (unsigned*)ws;
    p.b = b;
    p.state_words = track_state_words(h, w, max_open);
    p.t = (unsigned)t;
    p.j = 0u;
    p.npix = (unsigned)h * (unsigned)w;
    p.w = (unsigned)w;
    p.h = (unsigned)h;
    p.nchunks = region_chunks(p.npix);
    p.max_open = (unsigned)max_open;
    p.max_closed = (unsigned)max_closed;
    p.min_duration = min_duration;
    p.min_volume = min_volume;
    p.temporal = temporal;
    p.flush = flush ? 1 : 0;
    const unsigned gy = (unsigned)(b < 65535 ? b : 65535);
    const dim3 block(TR_THREADS);
    const dim3 carry_grid(gy);
    hipLaunchKernelGGL(track_zero_kernel, dim3(track_grid_x(((unsigned long long)b * (6 + 3 * (unsigned long long)t) + TR_THREADS - 1) / TR_THREADS, 1024u)),
                       block, 0, s, p);
    VAD_LAUNCH_CHECK();
    if (flush) {
        hipLaunchKernelGGL(track_carry_kernel, carry_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_clear_kernel, dim3(track_grid_x((p.state_words + TR_THREADS - 1) / TR_THREADS, 1024u), gy), block, 0, s, p, 0);
        VAD_LAUNCH_CHECK();
        return VAD_OK;
    }
    // inside the frames: the labeller as it stands, on b * t frames (its flatten pass leaves every pixel directly under its root);
    // its first kernel clears the flag word
    if (int rc = vad_label_launch(maps, VAD_LABEL_FMT_F32_GE, threshold, b * t, h, w, connectivity, p.labels, nullptr, p.flags, s)) return rc;
    const dim3 pixel_grid(track_grid_x((p.npix + TR_RUN - 1u) / TR_RUN, TR_PIXEL_BLOCKS_X), gy);
    const dim3 scan_grid(track_grid_x(p.nchunks, TR_SCAN_BLOCKS_X), gy);
    const dim3 table_grid(track_grid_x((p.max_open + TR_THREADS - 1u) / TR_THREADS, TR_TABLE_BLOCKS_X), gy);
    for (int j = 0; j < t; ++j) {
        p.j = (unsigned)j;
        hipLaunchKernelGGL(track_begin_kernel, table_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_link_kernel<false>, pixel_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_link_kernel<true>, pixel_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_flatten_kernel, scan_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_slot_kernel, scan_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_carry_kernel, carry_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_reduce_kernel, pixel_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
        hipLaunchKernelGGL(track_finish_kernel, table_grid, block, 0, s, p);
        VAD_LAUNCH_CHECK();
    }
    return VAD_OK;
}

}  // namespace

size_t vad_track_state_bytes(long long b, int h, int w, int max_open) {
    if (!track_dims_ok(b, h, w, max_open)) return 0;
    return (size_t)b * track_state_words(h, w, max_open) * 4;
}

size_t vad_track_workspace_bytes(long long b, int t, int h, int w, int max_open) {
    if (!track_dims_ok(b, h, w, max_open) || t < 0 || (long long)b * t * ((long long)h * w) > (1ll << 38)) return 0;
    return track_carve(b, t, h, w, max_open).total;
}

int vad_track_plan(int* label_round, int* pixel_round, int* scan_round, int* table_round, int* threads) {
    VAD_REQUIRE(label_round && pixel_round && scan_round && table_round && threads, "track_plan: an output pointer is NULL");
    *label_round = (int)VAD_LABEL_ROUND_PIXELS;
    *pixel_round = (int)(TR_PIXEL_BLOCKS_X * TR_RUN);
    *scan_round = (int)(TR_SCAN_BLOCKS_X * TR_CHUNK);
    *table_round = (int)(TR_TABLE_BLOCKS_X * TR_THREADS);
    *threads = TR_THREADS;
    return VAD_OK;
}

int vad_track_init(void* state, long long b, int h, int w, int max_open, void* stream) {
    VAD_ARG(vad_req_ptr("track_init", "state", state, 16));
    VAD_REQUIRE(b >= 0 && b <= (1ll << 20), "track_init: b must be in 0..2^20, got %lld", b);
    VAD_REQUIRE(h >= 1 && w >= 1 && (long long)h * w <= TR_MAX_PIXELS, "track_init: h and w must be >= 1 with h * w <= 2^24, got %d x %d", h, w);
    VAD_ARG(vad_req_capacity("track_init", "max_open", max_open, TR_MAX_OPEN));
    if (b == 0) return VAD_OK;
    TrackP p = {};
    p.state = (unsigned*)state;
    p.b = b;
    p.state_words = track_state_words(h, w, max_open);
    p.h = (unsigned)h;
    p.w = (unsigned)w;
    p.max_open = (unsigned)max_open;
    const unsigned gy = (unsigned)(b < 65535 ? b : 65535);
    hipLaunchKernelGGL(track_clear_kernel, dim3(track_grid_x((p.state_words + TR_THREADS - 1) / TR_THREADS, 1024u), gy), dim3(TR_THREADS), 0,
                       (hipStream_t)stream, p, 1);
    VAD_LAUNCH_CHECK();
    return VAD_OK;
}

int vad_track_events(const float* maps, long long b, int t, int h, int w, float threshold, int connectivity, int temporal,
                     unsigned min_duration, unsigned min_volume, int max_open, int max_closed, void* state, uint32_t* closed,
                     uint32_t* counts, uint32_t* frame_counts, void* ws, size_t ws_bytes, void* stream) {
    VAD_ARG(vad_req_t("track_events", t));
    return track_run("track_events", maps, b, t, h, w, threshold, connectivity, temporal, min_duration, min_volume, max_open, max_closed, state,
                     closed, counts, frame_counts, ws, ws_bytes, stream);
}

int vad_track_flush(long long b, int h, int w, unsigned min_duration, unsigned min_volume, int max_open, int max_closed, void* state,
                    uint32_t* closed, uint32_t* counts, void* ws, size_t ws_bytes, void* stream) {
    return track_run("track_flush", nullptr, b, 0, h, w, 0.0f, 8, 1, min_duration, min_volume, max_open, max_closed, state, closed, counts, nullptr,
                     ws, ws_bytes, stream);
}
