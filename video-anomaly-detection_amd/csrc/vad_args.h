// Argument checks of the anomaly-map entry points (score_hist, region_overlap, map_regions, map_match, map_events, map_event_match, map_track,
// map_smooth, map_morph, map_stats): one copy of every check that three or more entry points word the same way; a check that one
// or two make stays written out where it is made.  Host code only, all of it runs before an entry point's first HIP call.  `who`
// is the entry point's name in the message, `name` the argument's.  A helper returns VAD_OK or what vad_fail returned (a ?: b:
// the first refusal wins); VAD_ARG is the call site.  The size queries (*_workspace_bytes, *_state_bytes) use the *_ok predicates
// and answer 0 silently, so a query and its entry point cannot disagree.
#pragma once
#include "vad_common.h"

#define VAD_ARG(call) do { if (int rc_ = (call)) return rc_; } while (0)
#define VAD_REQ(name, params, cond, ...) static inline int name params { VAD_REQUIRE(cond, __VA_ARGS__); return VAD_OK; }
static inline bool vad_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }
static inline bool vad_disjoint(const void* a, const void* b, size_t bytes) {   // [a, a + bytes) and [b, b + bytes) share no byte
    return (uintptr_t)a + bytes <= (uintptr_t)b || (uintptr_t)b + bytes <= (uintptr_t)a;
}

// ---- pointers.  vad_req_aligned alone is the form for a pointer that may be NULL (labels_or_null, frame_max, maps on a flush);
// float labels / masks (VAD_LBL_F32_ELEM) are read as floats, the uint8 formats have no alignment; vad_req_masks: ground-truth
// masks in one of the two per-element formats (`fmt_name`: the format argument's name).
VAD_REQ(vad_req_nonnull, (const char* who, const char* name, const void* p), p != nullptr, "%s: %s is NULL", who, name)
VAD_REQ(vad_req_aligned, (const char* who, const char* name, const void* p, int bytes), vad_aligned(p, (uintptr_t)bytes),
        "%s: %s must be %d-byte aligned", who, name, bytes)
VAD_REQ(vad_req_float_labels, (const char* who, const char* name, const void* p, int format), format != VAD_LBL_F32_ELEM || vad_aligned(p, 4),
        "%s: float %s must be 4-byte aligned", who, name)
static inline int vad_req_ptr(const char* who, const char* name, const void* p, int bytes) { return vad_req_nonnull(who, name, p) ?: vad_req_aligned(who, name, p, bytes); }
VAD_REQ(vad_req_mask_format, (const char* who, const char* fmt_name, int format), format == VAD_LBL_U8_ELEM || format == VAD_LBL_F32_ELEM,
        "%s: %s must be VAD_LBL_U8_ELEM (%d) or VAD_LBL_F32_ELEM (%d), got %d", who, fmt_name, VAD_LBL_U8_ELEM, VAD_LBL_F32_ELEM, format)
static inline int vad_req_masks(const char* who, const void* masks, const char* fmt_name, int format) {
    return vad_req_nonnull(who, "masks", masks) ?: vad_req_mask_format(who, fmt_name, format) ?: vad_req_float_labels(who, "masks", masks, format);
}

// ---- dims of the smoothing family (smooth_maps, morph_maps, mapstat_*, map_normalize): n maps of h x w, a frame within
// VAD_MAX_FRAME_PIXELS, n * h * w <= 2^60.  vad_req_map_dims: all three, for the entry points that check nothing in between.
static inline bool vad_map_hw_ok(int h, int w) { return h >= 1 && w >= 1 && vad_frame_pixels_ok(h, w); }
static inline bool vad_map_total_ok(long long n, int h, int w) { return n <= (1ll << 60) / ((long long)h * w); }   // (h, w checked)
static inline bool vad_map_dims_ok(long long n, int h, int w) { return n >= 0 && vad_map_hw_ok(h, w) && vad_map_total_ok(n, h, w); }
VAD_REQ(vad_req_map_n, (const char* who, long long n), n >= 0, "%s: n=%lld is negative", who, n)
VAD_REQ(vad_req_map_total, (const char* who, long long n, int h, int w), vad_map_total_ok(n, h, w), "%s: n * h * w is not representable (n=%lld)", who, n)
static inline int vad_req_map_hw(const char* who, int h, int w) {
    VAD_REQUIRE(h >= 1 && w >= 1, "%s: h and w must be positive, got %dx%d", who, h, w);
    VAD_REQUIRE_PIXELS(who, h, w);
    return VAD_OK;
}
static inline int vad_req_map_dims(const char* who, long long n, int h, int w) { return vad_req_map_n(who, n) ?: vad_req_map_hw(who, h, w) ?: vad_req_map_total(who, n, h, w); }

// ---- dims of the labelling family (label_regions, pro_accumulate, detect_regions, match_regions, detect_events, match_events): n >= 0 frames
// (`name`: n or b) of h x w < 2^31 - 1 pixels, n * h * w <= 2^38 (a work-group's run of a 256-group launch stays below 2^32);
// *total = n * h * w.  One helper per check: the entry points check other arguments between them.
static inline bool vad_label_hw_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * w < 2147483647ll; }
static inline bool vad_label_dims_ok(long long n, int h, int w, long long* total) {
    return n >= 0 && vad_label_hw_ok(h, w) && !__builtin_mul_overflow(n, (long long)h * w, total) && *total <= (1ll << 38);
}
VAD_REQ(vad_req_label_n, (const char* who, const char* name, long long n), n >= 0, "%s: %s must be >= 0, got %lld", who, name, n)
VAD_REQ(vad_req_label_hw, (const char* who, int h, int w), vad_label_hw_ok(h, w), "%s: h and w must be >= 1 with h * w < 2^31 - 1, got %d x %d", who, h, w)
VAD_REQ(vad_req_label_total, (const char* who, long long n, int h, int w, long long* total), vad_label_dims_ok(n, h, w, total),
        "%s: n * h * w must be at most 2^38 (%lld x %d x %d)", who, n, h, w)

// ---- the operating point (nonzero: min_area, min_duration, min_volume; capacity: max_regions, max_events, max_open, max_closed)
VAD_REQ(vad_req_threshold, (const char* who, float threshold), threshold == threshold, "%s: threshold is NaN", who)
VAD_REQ(vad_req_connectivity, (const char* who, int c), c == 4 || c == 8, "%s: connectivity must be 4 or 8, got %d", who, c)
VAD_REQ(vad_req_t, (const char* who, int t), t >= 1, "%s: t must be >= 1, got %d", who, t)
VAD_REQ(vad_req_nonzero, (const char* who, const char* name, unsigned v), v >= 1u, "%s: %s must be >= 1, got 0", who, name)
VAD_REQ(vad_req_capacity, (const char* who, const char* name, int v, int max), v >= 1 && v <= max, "%s: %s must be in 1..%d, got %d", who, name, max, v)

// ---- the mantissa bits of the score histograms (score_hist.hip, region_overlap.hip)
static inline bool vad_hist_m_ok(int m) { return m >= VAD_HIST_MIN_M && m <= VAD_HIST_MAX_M; }
VAD_REQ(vad_req_mantissa, (const char* who, int m), vad_hist_m_ok(m), "%s: m (mantissa_bits) must be in %d..%d, got %d", who, VAD_HIST_MIN_M, VAD_HIST_MAX_M, m)

// ---- a workspace shorter than its size query asks for.  `query` and the arguments behind it print the query as the caller would
// write it.  `code` is VAD_ERR_WS; label_regions and pro_accumulate have always answered VAD_ERR_ARG, and callers may test for it.
#define VAD_REQUIRE_WS(code, who, ws_bytes, need, query, ...) \
    do { if ((ws_bytes) < (need)) return vad_fail(code, "%s: ws_bytes %zu is less than " query " = %zu", who, ws_bytes, __VA_ARGS__, need); } while (0)
