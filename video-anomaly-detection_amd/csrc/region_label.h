// The union-find labeller of csrc/region_overlap.hip as the other kernels of the library use it (csrc/map_regions.hip): one copy of
// the init / merge / flatten kernels, reached through this launcher.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// A third predicate of the init kernel behind the two public label formats (VAD_LBL_U8_ELEM, VAD_LBL_F32_ELEM): float values,
// foreground iff v >= threshold (a NaN value never is).  Internal: vad_label_regions, vad_pro_accumulate and vad_hist_accumulate
// refuse it like every other number that is not one of theirs.
constexpr int VAD_LABEL_FMT_F32_GE = 3;
constexpr size_t VAD_LABEL_WS_HEAD_BYTES = 16;   // the flag word, padded so that the planes behind it are 16-byte aligned

// n >= 0, h, w >= 1, h * w < 2^31 - 1, n * h * w <= 2^38: the limits of vad_label_regions; *total = n * h * w.
bool vad_label_dims_ok(long long n, int h, int w, long long* total);

// init, merge, flatten on `s`: labels int32 [n, h, w] (0, or 1 + the smallest y * w + x of the region), sizes (may be NULL)
// uint32 [n, h, w] (the pixel count at the root, 0 elsewhere), flags[0] cleared by the first kernel and set by a walk that ran out
// of its bound.  `threshold` is read under VAD_LABEL_FMT_F32_GE only.  The arguments are the caller's to check.
int vad_label_launch(const void* masks, int fmt, float threshold, long long n, int h, int w, int conn, int* labels, unsigned* sizes,
                     unsigned* flags, hipStream_t s);
