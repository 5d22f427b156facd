// The on-chip half of the score histograms (score_hist.hip, region_overlap.hip): the quantiser's bin count and blob tag, and the
// work-group's LDS table of (bin -> u32 count) entries with its wave-combined overflow path.  See score_hist.hip for the design.
#pragma once
#include <hip/hip_runtime.h>

#include "vad_common.h"

namespace {

constexpr int HIST_THREADS = 1024;
constexpr int HIST_SLOTS = 16384;              // 2 x 64 KiB of the CU's 160 KiB of LDS: one work-group (16 waves) per CU
constexpr int HIST_PROBES = 8;
constexpr int HIST_MAX_BLOCKS = 256;           // one per CU

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline unsigned hist_tag(int m) { return ((unsigned)VAD_ABI_VERSION << 16) | (unsigned)m; }
__host__ __device__ inline unsigned hist_nbins(int m) { return 255u << m; }

struct HistLds {
    unsigned tag[HIST_SLOTS];   // 0 = free, else bin + 1 (bin = class * nbins + key)
    unsigned cnt[HIST_SLOTS];
    unsigned rej[2];
};

// One (bin, count) of every lane with `mine` set into the work-group's table.  Called in converged control flow: every ballot
// below names its predicate, none relies on which lanes a branch left active.  The slot is picked from the low bits of
// 2 * key + class: neighbouring bins sit in neighbouring slots, so the final flush adds to contiguous counters (two rows, one per
// class), and the two classes of one key never compete for a slot.  Lanes whose probes find no slot add to the global counters
// directly, one add per distinct bin among them (a hot bin that arrives after the table is full must not become one global atomic
// per element).
__device__ __forceinline__ void hist_lds_add(HistLds& s, u64* counts, unsigned nbins, unsigned bin, unsigned c, bool mine) {
    const unsigned want = bin + 1u;
    const unsigned h = bin >= nbins ? 2u * (bin - nbins) + 1u : 2u * bin;
    bool pending = mine;
#pragma unroll
    for (int p = 0; p < HIST_PROBES; ++p) {
        if (pending) {
            const unsigned slot = (h + 2u * p) & (HIST_SLOTS - 1);
            unsigned t = __hip_atomic_load(&s.tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (t == 0u) {
                t = atomicCAS(&s.tag[slot], 0u, want);
                if (t == 0u) t = want;
            }
            if (t == want) {
                atomicAdd(&s.cnt[slot], c);
                pending = false;
            }
        }
    }
    const int lane = (int)(threadIdx.x & 63u);
    u64 left = __ballot(pending);
    while (left != 0) {                                      // wave-uniform loop: one distinct bin of the lanes left over per round
        const int lead = __builtin_ctzll(left);
        const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)bin, lead);
        const u64 same = __ballot(pending && bin == first);
        // the lanes of `same` carry the same c: 1 each, or (wave-uniform caller) there is only the one lane
        if (lane == lead) atomicAdd(&counts[first], (u64)c * (u64)__builtin_popcountll(same));
        if (bin == first) pending = false;
        left &= ~same;
    }
}

}  // namespace
