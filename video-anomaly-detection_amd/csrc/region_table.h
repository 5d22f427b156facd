// What the region consumers build behind the labeller of region_label.h (csrc/map_regions.hip, csrc/map_match.hip,
// csrc/map_events.hip, csrc/map_event_match.hip, csrc/map_track.hip): one copy of the wave-level election and combination, of the accumulator of a record's
// box, peak and coordinate sums, of the raster-order rank of roots over chunks, of the 3 x 3 ring, and of the host-side chunk
// arithmetic.  Not part of the C ABI; everything here is inlined into the kernels that use it.
//
// The contract of every wave_* function, of RegionAcc::combined and of wave_each_key / wave_each_pair: the call sits in converged
// control flow - every lane of the wave reaches it, in loops whose trip counts are the same for every lane, never under a branch
// that depends on the lane.  A lane with nothing to contribute passes pending = false (or the identity), it does not skip the call.
// The block_* and chunk_* functions hold barriers: every thread of the work-group reaches them, REGION_THREADS threads a group.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "region_label.h"

typedef unsigned long long u64;

constexpr int REGION_THREADS = 256;
constexpr unsigned REGION_WAVES = REGION_THREADS / 64;
constexpr unsigned REGION_CHUNK = 1024;   // pixels of one chunk of the count / slot passes: four rows of the work-group

// The order-preserving key of a float's bits: a < b as floats (with -0.0 < +0.0) iff key(a) < key(b) as unsigned.
__device__ __forceinline__ unsigned order_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ unsigned order_key_inv(unsigned key) { return (key & 0x80000000u) ? key & 0x7fffffffu : ~key; }

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned other = __shfl_xor(v, m);
        v = other > v ? other : v;
    }
    return v;
}

// Calls f(a0, b0, mine, many, lead) once for every distinct pair (a, b) among the `pending` lanes of the wave: a0, b0 the pair
// (wave-uniform), mine = this lane holds it, many = more than one lane does (wave-uniform: a butterfly can be skipped for a
// single holder), lead = this lane is the pair's first, the one to act for it.  The loop is wave-uniform and every round retires at
// least the leading lane, so f runs in converged control flow too and may itself combine across the wave.
template <class F>
__device__ __forceinline__ void wave_each_pair(bool pending, unsigned a, unsigned b, unsigned lane, F&& f) {
    u64 left = __ballot(pending);
    while (left != 0) {
        const int lead = __builtin_ctzll(left);
        const unsigned a0 = (unsigned)__builtin_amdgcn_readlane((int)a, lead), b0 = (unsigned)__builtin_amdgcn_readlane((int)b, lead);
        const bool mine = pending && a == a0 && b == b0;
        const u64 same = __ballot(mine);
        f(a0, b0, mine, (same & (same - 1ull)) != 0, lane == (unsigned)lead);
        if (mine) pending = false;
        left &= ~same;
    }
}

// The same for one word: f(first, mine, many, lead) once for every distinct key among the pending lanes.
template <class F>
__device__ __forceinline__ void wave_each_key(bool pending, unsigned key, unsigned lane, F&& f) {
    wave_each_pair(pending, key, 0u, lane, [&](unsigned first, unsigned, bool mine, bool many, bool lead) { f(first, mine, many, lead); });
}

// Whether this lane is the one elected for its pair (a, b): one lane for every distinct pair among the pending lanes.
__device__ __forceinline__ bool wave_elect_pair(bool pending, unsigned a, unsigned b, unsigned lane) {
    bool elected = false;
    wave_each_pair(pending, a, b, lane, [&](unsigned, unsigned, bool, bool, bool lead) { elected |= lead; });
    return elected;
}

// What a lane gathers of one record before it goes to memory: the box, the 64-bit peak word (key(v) << 32 | ~index: the largest
// key and, among equals, the smallest index), the coordinate sums of its own pixels of one slot, and one further sum `sw` of the
// table's own, in a type W of its choice (the frames of the events, the pixel count of the tracker).  A table without one adds 0
// and never reads it: after inlining nothing of it is left.
template <class W>
struct RegionAcc {
    unsigned slot;           // 0 = nothing gathered
    unsigned x0, y0, x1, y1;
    u64 peak, sx, sy;
    W sw;

    __device__ __forceinline__ void clear() {
        slot = 0u;
        x0 = y0 = 0xffffffffu;
        x1 = y1 = 0u;
        peak = sx = sy = 0ull;
        sw = 0;
    }

    // One pixel of slot s != 0, with w for the further sum.  The first pixel of another slot drops what was gathered before: the
    // caller has sent it to its record (the pending lanes of its flush are those with slot != 0 && s != 0 && s != slot).
    __device__ __forceinline__ void add(unsigned s, unsigned x, unsigned y, u64 pk, W w) {
        if (s != slot) {
            slot = s;
            x0 = x1 = x;
            y0 = y1 = y;
            peak = pk;
            sx = x;
            sy = y;
            sw = w;
        } else {
            x0 = x < x0 ? x : x0;
            y0 = y < y0 ? y : y0;
            x1 = x > x1 ? x : x1;
            y1 = y > y1 ? y : y1;
            peak = pk > peak ? pk : peak;
            sx += x;
            sy += y;
            sw += w;
        }
    }

    // Inside wave_each_key: the values of the lanes that hold the key (`mine`), combined over the wave by a butterfly - skipped
    // when the key has one holder (`many` is wave-uniform).  Every lane that holds the key gets the combined values.
    __device__ __forceinline__ RegionAcc combined(bool mine, bool many) const {
        RegionAcc c;
        c.slot = slot;
        c.x0 = mine ? x0 : 0xffffffffu;
        c.y0 = mine ? y0 : 0xffffffffu;
        c.x1 = mine ? x1 : 0u;
        c.y1 = mine ? y1 : 0u;
        c.peak = mine ? peak : 0ull;
        c.sx = mine ? sx : 0ull;
        c.sy = mine ? sy : 0ull;
        c.sw = mine ? sw : (W)0;
        if (many) {
            for (int m = 32; m >= 1; m >>= 1) {
                const unsigned ox0 = __shfl_xor(c.x0, m), oy0 = __shfl_xor(c.y0, m), ox1 = __shfl_xor(c.x1, m), oy1 = __shfl_xor(c.y1, m);
                const u64 opeak = __shfl_xor(c.peak, m);
                c.x0 = ox0 < c.x0 ? ox0 : c.x0;
                c.y0 = oy0 < c.y0 ? oy0 : c.y0;
                c.x1 = ox1 > c.x1 ? ox1 : c.x1;
                c.y1 = oy1 > c.y1 ? oy1 : c.y1;
                c.peak = opeak > c.peak ? opeak : c.peak;
                c.sx += __shfl_xor(c.sx, m);
                c.sy += __shfl_xor(c.sy, m);
                c.sw += __shfl_xor(c.sw, m);
            }
        }
        return c;
    }

    // The seven atomics of one record r: the box in the words box .. box + 3 (x0, y0 min, x1, y1 max), the peak word (max) at
    // `pk`, the sums of x and y at sums, sums + 2; where sw goes is the caller's.  Issued by one lane for a record it has checked
    // to lie inside the table.
    __device__ __forceinline__ void commit(unsigned* r, unsigned box, unsigned pk, unsigned sums) const {
        atomicMin(r + box, x0);
        atomicMin(r + box + 1, y0);
        atomicMax(r + box + 2, x1);
        atomicMax(r + box + 3, y1);
        atomicMax((u64*)(r + pk), peak);
        atomicAdd((u64*)(r + sums), sx);
        atomicAdd((u64*)(r + sums + 2), sy);
    }
};

// The sums over the work-group of N values per thread, through s_sum[N] in LDS, in two steps.  block_sum_clear comes before the
// threads gather their values: its barrier then follows the one that ended the round before and is met without a wait.  block_sum
// adds the waves' sums and hands the totals back to every thread in v.  Between its return and the next clear of the same s_sum
// lies a barrier (the rows of chunk_rank_row, or one of the caller's own): a slow thread may still be reading.
template <int N>
__device__ __forceinline__ void block_sum_clear(unsigned* s_sum) {
    if (threadIdx.x < N) s_sum[threadIdx.x] = 0u;
    __syncthreads();
}

template <int N>
__device__ __forceinline__ void block_sum(unsigned (&v)[N], unsigned* s_sum) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = wave_sum(v[q]);               // all of them before the branch: the butterflies overlap
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (v[q]) atomicAdd(&s_sum[q], v[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = s_sum[q];
}

// The roots of the chunks in front of chunk c: base[q] = the sum of cnt_of[k * N + q] over k < c, for N counters per chunk.
template <int N>
__device__ __forceinline__ void chunk_before(const unsigned* cnt_of, unsigned c, unsigned (&base)[N], unsigned* s_sum) {
    block_sum_clear<N>(s_sum);
#pragma unroll
    for (int q = 0; q < N; ++q) base[q] = 0u;
    for (unsigned k = threadIdx.x; k < c; k += REGION_THREADS) {
#pragma unroll
        for (int q = 0; q < N; ++q) base[q] += cnt_of[k * N + q];
    }
    block_sum(base, s_sum);
}

// One row of REGION_THREADS consecutive pixels, N predicates a pixel: rank[q] = base[q] + the pixels of the row in front of this
// one with pred[q] set (ballot and popcount inside the wave, the totals of the waves through s_wave), and base[q] moves past the
// row.  The first barrier publishes the waves' totals; the second keeps a fast wave from writing s_wave for the next row while a
// slow one still reads this row's.
template <int N>
__device__ __forceinline__ void chunk_rank_row(const bool (&pred)[N], unsigned (&base)[N], unsigned (&rank)[N], unsigned (*s_wave)[REGION_WAVES]) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 b[N];
    unsigned row[N];
#pragma unroll
    for (int q = 0; q < N; ++q) b[q] = __ballot(pred[q]);
    if (lane == 0u) {
#pragma unroll
        for (int q = 0; q < N; ++q) s_wave[q][wave] = (unsigned)__builtin_popcountll(b[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        rank[q] = base[q] + (unsigned)__builtin_popcountll(b[q] & ((1ull << lane) - 1ull));
        row[q] = 0u;
    }
    for (unsigned k = 0; k < REGION_WAVES; ++k) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            if (k < wave) rank[q] += s_wave[q][k];
            row[q] += s_wave[q][k];
        }
    }
#pragma unroll
    for (int q = 0; q < N; ++q) base[q] += row[q];
    __syncthreads();
}

// the same for one predicate
__device__ __forceinline__ unsigned chunk_rank_row(bool pred, unsigned& base, unsigned (*s_wave)[REGION_WAVES]) {
    const bool preds[1] = {pred};
    unsigned bases[1] = {base}, ranks[1];
    chunk_rank_row(preds, bases, ranks, s_wave);
    base = bases[0];
    return ranks[0];
}

// The ring of the 3 x 3 around a pixel, clockwise from above-left: consecutive ring pixels are neighbours inside their frame.
__device__ __forceinline__ int ring_dy(int k) { return k < 3 ? -1 : (k == 3 || k == 7) ? 0 : 1; }
__device__ __forceinline__ int ring_dx(int k) { return (k == 0 || k >= 6) ? -1 : (k == 1 || k == 5) ? 0 : 1; }
__device__ __forceinline__ bool ring_inside(unsigned y, unsigned x, unsigned h, unsigned w, int k) {
    const int dy = ring_dy(k), dx = ring_dx(k);
    return (dy >= 0 || y > 0u) && (dy <= 0 || y + 1u < h) && (dx >= 0 || x > 0u) && (dx <= 0 || x + 1u < w);
}

inline unsigned region_chunks(long long pixels) { return (unsigned)((pixels + REGION_CHUNK - 1) / REGION_CHUNK); }

// the bytes of `words` uint32 per chunk for n frames (or clips) of `pixels` pixels, padded to 16
inline size_t region_chunk_bytes(long long n, long long pixels, unsigned words) {
    return ((size_t)n * region_chunks(pixels) * words * 4 + 15) & ~(size_t)15;
}

// the bytes in front of a workspace's planes: the flag words' 16, then the per-chunk words
inline size_t region_head_bytes(long long n, long long pixels, unsigned words) {
    return VAD_LABEL_WS_HEAD_BYTES + region_chunk_bytes(n, pixels, words);
}
