// The union-find labeller of csrc/region_overlap.hip as the other kernels of the library use it (csrc/map_regions.hip,
// csrc/map_events.hip): one copy of the init / merge / flatten kernels, reached through this launcher, and one copy of the bounded
// find / union walks for the kernels that unite further (the links in time of map_events.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// A third predicate of the init kernel behind the two public label formats (VAD_LBL_U8_ELEM, VAD_LBL_F32_ELEM): float values,
// foreground iff v >= threshold (a NaN value never is).  Internal: vad_label_regions, vad_pro_accumulate and vad_hist_accumulate
// refuse it like every other number that is not one of theirs.
constexpr int VAD_LABEL_FMT_F32_GE = 3;
constexpr size_t VAD_LABEL_WS_HEAD_BYTES = 16;   // the flag word, padded so that the planes behind it are 16-byte aligned
constexpr unsigned VAD_LABEL_FLAG_WALK = 1u;     // flag word: a root chase or a union ran out of its step budget
constexpr unsigned VAD_LABEL_ROUND_PIXELS = 4096u * 256u;   // pixels of one frame that one grid round of the labelling kernels covers

// init, merge, flatten on `s`: labels int32 [n, h, w] (0, or 1 + the smallest y * w + x of the region), sizes (may be NULL)
// uint32 [n, h, w] (the pixel count at the root, 0 elsewhere), flags[0] cleared by the first kernel and set by a walk that ran out
// of its bound.  `threshold` is read under VAD_LABEL_FMT_F32_GE only.  The arguments are the caller's to check.
int vad_label_launch(const void* masks, int fmt, float threshold, long long n, int h, int w, int conn, int* labels, unsigned* sizes,
                     unsigned* flags, hipStream_t s);

__device__ __forceinline__ int label_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x (indices inside one image, or inside one clip's volume; L[x] = parent + 1).  At most `budget` steps, each to a smaller index.  A parent that is
// not a smaller index (the plane is not a union-find: never, short of a defect) ends the walk with the budget spent - no address
// is ever formed from it.
__device__ __forceinline__ unsigned label_find(const int* L, unsigned x, unsigned& budget) {
    while (budget != 0u) {
        const unsigned parent = (unsigned)label_load(L + x) - 1u;
        if (parent == x) break;
        if (parent > x) {
            budget = 0u;
            break;
        }
        x = parent;
        --budget;
    }
    return x;
}

// Unite the sets of a and b.  Returns false when the budget ran out.
__device__ __forceinline__ bool label_union(int* L, unsigned a, unsigned b, unsigned budget) {
    while (budget != 0u) {
        a = label_find(L, a, budget);
        b = label_find(L, b, budget);
        if (a == b) return budget != 0u;
        if (a < b) {
            const unsigned t = a;
            a = b;
            b = t;
        }
        if (budget == 0u) break;
        const unsigned old = (unsigned)atomicMin(L + a, (int)(b + 1u)) - 1u;
        if (old == a) return true;                           // a was a root and now hangs below b
        if (old > a) break;                                  // not a union-find plane (see label_find)
        a = old;                                            // another thread gave a a parent first (old < a): unite that with b
        --budget;
    }
    return false;
}
