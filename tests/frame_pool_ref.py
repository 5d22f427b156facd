"""A pool of P distinct frames (clips, streams) and the batches built from it by index: batch item i is pool[i % P].

The frame-count tests (tests/test_hip_frame_counts.py, tests/test_hip_large_offsets.py) hand the map kernels more frames than one
launch takes.  A per-frame restatement cannot run over 131,075 frames and does not have to: the operations treat every item on
its own, so the expected output of the batch is the expected output of the P pool items, expanded with the same index vector on
the device, and an additive state is the pool items' integer counts times each item's multiplicity in the batch.  P = 251 is
prime and divides none of the slice lengths, so a slice based one item off, or 65535 or 65536 items off, lands on another pool
entry.  tests/test_frame_count_plan.py checks this arithmetic and the pool's coverage without a GPU."""
import numpy as np

import map_stats_ref
import regions_ref

P = 251

#: frames (streams, clips) of one launch along gridDim.y / gridDim.z: the host loops `for (f0 = 0; f0 < n; f0 += 65535)` of
#: csrc/map_smooth.hip:255, map_morph.hip:235, map_temporal.hip:209 and :270, resize_u8.hip:250 and :567, state_io.hip:92,
#: map_topk.hip:446, and the `gy = min(n, 65535)` of the grid-stride kernels (map_regions.hip:231, map_match.hip:320,
#: region_overlap.hip:297, map_events.hip:463, map_event_tracks.hip:224, map_track.hip:564 and :640, frame_gather.hip:157)
SLICE = 65535
#: frames of one work-group of vad_map_normalize and the pixels of one (csrc/map_stats.hip:46-48); its slices are SLICE * NZ_FRAMES
NZ_FRAMES = 4
NZ_CHUNK = 1024
NZ_SLICE = SLICE * NZ_FRAMES
#: elements of one launch of vad_hist_accumulate (csrc/score_hist.hip:39)
HIST_LAUNCH_ELEMS = 1 << 30

N3 = 2 * SLICE + 5          # three slices / rounds; the third begins at 131070
N2 = SLICE + 6              # the second slice / round has six frames
NZ = 4 * SLICE + 5          # two normalize slices; the second has five frames

#: the threshold the pools are built around
T = np.float32(0.01)

#: what the first pool items are; the others are seeded signed log-normal maps
NOTHING, NONFINITE, TIES, TWO_REGIONS, THREE_REGIONS = 0, 1, 2, 3, 4

# Part B: (2050, 1024, 1024) float32 = 2^31 + 2^21 elements; item i is bigpool[i % BIG_P]
BIG_N, BIG_H, BIG_W, BIG_P = 2050, 1024, 1024, 7


def index(n: int, p: int = P) -> np.ndarray:
    """int64 [n]: the pool entry of batch item i."""
    return np.arange(n, dtype=np.int64) % p


def multiplicity(n: int, p: int = P) -> np.ndarray:
    """int64 [p]: how often every pool entry occurs among the n batch items."""
    return np.bincount(index(n, p), minlength=p).astype(np.int64)


def expand(per_item: np.ndarray, n: int) -> np.ndarray:
    """The batch of n items from per-item arrays [p, ...] (the host form of what the GPU tests do on the device)."""
    return per_item[index(n, len(per_item))]


def signed_lognormal(shape, seed):
    """The seeded signed log-normal maps the map tests share (`_maps` of tests/test_hip_map_smooth.py and its neighbours)."""
    rng = np.random.default_rng(seed)
    x = (np.exp(rng.standard_normal(shape) * 3.0) * 1e-3).astype(np.float32)
    return x * rng.choice(np.array([-1, 1], np.float32), shape)


def _below(x):
    """Nothing at or above T: the magnitudes, negated."""
    return -np.abs(x) - np.float32(1e-6)


def pool(tail, seed, p: int = P) -> np.ndarray:
    """float32 [p, *tail]: `tail` ends in H, W (H >= 2, W >= 5) and may begin with T (clips).  Entries NOTHING .. THREE_REGIONS
    are, in every frame of the entry: nothing at or above T; a NaN, a +Inf and a -Inf; pixels equal to T next to pixels one ulp
    below it; two regions and three regions (two pixels each, one above the other) of values >= T on a background below it."""
    h, w = tail[-2:]
    assert h >= 2 and w >= 5 and p > THREE_REGIONS
    x = signed_lognormal((p, *tail), seed)
    x[NOTHING] = _below(x[NOTHING])
    x[NONFINITE, ..., 0, 1] = np.nan
    x[NONFINITE, ..., h - 1, w - 1] = np.inf
    x[NONFINITE, ..., 1, 2] = -np.inf
    x[TIES] = _below(x[TIES])
    x[TIES, ..., 0, 0] = T
    x[TIES, ..., 0, 1] = np.nextafter(T, np.float32(0))
    x[TIES, ..., 1, 3] = T
    x[TIES, ..., 1, 4] = T
    for entry, cols in ((TWO_REGIONS, (0, 2)), (THREE_REGIONS, (0, 2, 4))):
        x[entry] = _below(x[entry])
        for c in cols:
            x[entry, ..., 0, c] = T * np.float32(1 + c)
            x[entry, ..., 1, c] = T
    return np.ascontiguousarray(x, np.float32)


def masks(tail, seed, p: int = P) -> np.ndarray:
    """bool [p, *tail] ground-truth masks for `pool(tail, ...)`: entry NOTHING is empty, TWO_REGIONS / THREE_REGIONS hold two and
    three mask regions (one of them on the map's first region), the others are seeded blobs of about a fifth of the frame."""
    rng = np.random.default_rng(seed)
    m = rng.random((p, *tail)) < 0.2
    m[NOTHING] = False
    for entry, cols in ((TWO_REGIONS, (0, 3)), (THREE_REGIONS, (0, 2, 4))):
        m[entry] = False
        for c in cols:
            m[entry, ..., 0, c] = True
    m[TIES] = False
    m[TIES, ..., 0, 0:2] = True
    return m


def kinds(x: np.ndarray, threshold=T) -> dict:
    """Which pool entries are of the required kinds: name -> list of entries.  Regions are counted 8-connected on the entry's first
    frame by the restatement the region tests use."""
    out = {"nothing": [], "nan_and_inf": [], "ties": [], "two_regions": [], "three_regions": []}
    t = np.float32(threshold)
    for i, item in enumerate(x):
        frame = item.reshape(-1, *item.shape[-2:])[0]
        with np.errstate(invalid="ignore"):
            fg = frame >= t
        if not fg.any():
            out["nothing"].append(i)
        if np.isnan(item).any() and np.isinf(item).any():
            out["nan_and_inf"].append(i)
        if (frame == t).any() and (frame == np.nextafter(t, np.float32(0))).any():
            out["ties"].append(i)
        count = int(regions_ref.detect(frame, t, 8, 1, 64)[1][0])
        if count == 2:
            out["two_regions"].append(i)
        if count == 3:
            out["three_regions"].append(i)
    return out


def weighted_counts(per_item: np.ndarray, n: int) -> np.ndarray:
    """Integer counts [p, ...] of the pool items -> their sum over the batch of n items, exactly (Python integers in an object
    array would be the general form; int64 holds every total of these tests)."""
    per_item = np.asarray(per_item)
    mult = multiplicity(n, len(per_item))
    assert per_item.dtype.kind in "iu"
    total = (per_item.astype(np.int64) * mult.reshape((-1,) + (1,) * (per_item.ndim - 1))).sum(axis=0)
    return total


def weighted_stats(x: np.ndarray, n: int) -> map_stats_ref.State:
    """The `map_stats_ref.State` of the batch of n items of pool `x` [p, H, W], accumulated with multiplicities in float64: K is the
    batch's first frame (pool entry 0), S1 = sum m_i (x_i - K), S2 = sum m_i (x_i - K)^2.  The item-by-item restatement rounds
    every one of its n additions, this sum every one of its p: the two agree to n 2^-53 relative to sum |d|, far inside the
    float32 unit `map_stats_ref.ulps32` measures the finalized mean and std in."""
    mult = multiplicity(n, len(x)).astype(np.float64)
    st = map_stats_ref.State(*x.shape[-2:])
    st.n = int(n)
    st.K = x[0].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x.astype(np.float64) - st.K
        st.S1 = (d * mult[:, None, None]).sum(axis=0)
        st.S2 = (d * d * mult[:, None, None]).sum(axis=0)
    return st


def stats_within_bound(got32: np.ndarray, want32_from64: np.ndarray, want64: np.ndarray, bound: float = 1.0) -> bool:
    """A finalized float32 plane against the float64 value it rounds: non-finite pixels as such, the finite ones within `bound`
    units in the last place (`map_stats_ref.ulps32`, the measure and the 1-ulp bound of tests/test_hip_map_stats.py::test_merge).
    Why one unit holds for an exact state: the mean is one rounding of K + S1 / n (half a unit); the std is sqrtf of fl32(var) -
    the rounding of var moves the root by at most 2^-25 relative, under half a unit, and sqrtf adds its own half."""
    fin = np.isfinite(want64)
    if not (np.array_equal(np.isnan(got32), np.isnan(want32_from64)) and np.array_equal(got32[~fin & ~np.isnan(want64)], want32_from64[~fin & ~np.isnan(want64)])):
        return False
    return (not fin.any()) or map_stats_ref.ulps32(got32[fin], want64[fin]) <= bound


def big_frames(seed: int = 4100) -> np.ndarray:
    """float32 [BIG_P, 1024, 1024]: sparse above T like the 1040 x 1040 frames of tests/test_hip_match.py - a positive background below T (a
    few per cent of it negative, which a score histogram rejects) and a few dozen seeded rectangles and single pixels at or above it."""
    rng = np.random.default_rng(seed)
    x = signed_lognormal((BIG_P, BIG_H, BIG_W), seed)
    x = np.where(np.abs(x) < np.float32(1e-4), x, np.minimum(np.abs(x), np.float32(0.009))).astype(np.float32)   # below T; few negative
    for i in range(BIG_P):
        for k in range(24):
            y0, x0 = int(rng.integers(0, BIG_H - 40)), int(rng.integers(0, BIG_W - 40))
            hh, ww = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            x[i, y0:y0 + hh, x0:x0 + ww] = T + np.abs(signed_lognormal((hh, ww), seed + 100 * i + k))
        ys, xs = rng.integers(0, BIG_H, 64), rng.integers(0, BIG_W, 64)
        x[i, ys, xs] = T
    x[0, 0, 0], x[0, BIG_H - 1, BIG_W - 1] = T, T                       # the corners of the frame that repeats at every boundary
    return np.ascontiguousarray(x, np.float32)


def big_masks(frames: np.ndarray, seed: int = 4200) -> np.ndarray:
    """bool [BIG_P, 1024, 1024] for `frames = big_frames()`: a few dozen seeded rectangles per frame, and the foreground of the upper
    half of the frame moved seven pixels to the right, so that some mask regions lie over predicted ones and some beside them."""
    rng = np.random.default_rng(seed)
    m = np.zeros((BIG_P, BIG_H, BIG_W), bool)
    for i in range(BIG_P):
        for _ in range(20):
            y0, x0 = int(rng.integers(0, BIG_H - 60)), int(rng.integers(0, BIG_W - 60))
            m[i, y0:y0 + int(rng.integers(1, 60)), x0:x0 + int(rng.integers(1, 60))] = True
    m[:, :BIG_H // 2, 7:] |= (frames >= T)[:, :BIG_H // 2, :-7]
    return m


#: Part A's batches: case -> (items, shape of one item, bytes of one element) of the largest input the case hands to one call
CASES = {
    "smooth_maps": (N3, (4, 6), 4), "smooth_maps_two_tiles": (N2, (2, 70), 4),
    "morph_maps": (N3, (4, 6), 4), "morph_maps_two_tiles": (N2, (2, 70), 4),
    "map_statistics": (NZ, (3, 5), 4), "map_statistics_two_chunks": (NZ, (5, 205), 4),
    "temporal_f32x4": (N3, (3, 2, 6), 4), "temporal_scalar": (N2, (3, 2, 5), 4), "temporal_filter": (N3, (2, 2, 6), 4),
    "resize_rgb": (N3, (5, 8, 3), 1), "resize_rgba": (N3, (5, 7, 4), 1), "resize_l": (N3, (5, 7), 1),
    "transpose_c3": (N3, (2, 3, 4), 4), "transpose_c5": (N3, (2, 3, 8), 4),
    "detect_regions": (N3, (5, 7), 4), "match_regions": (N2, (5, 7), 4), "pro_histogram": (N2, (5, 7), 4),
    "detect_events": (N2, (2, 4, 5), 4), "event_tracker": (N2, (1, 4, 5), 4),
    "frame_bank_vector": (N3, (3, 4, 4), 4), "frame_bank_plain": (N3, (3, 3, 5), 4),
    "map_topk": (N3, (3, 5), 4),
}


def case_bytes(name: str) -> int:
    n, shape, size = CASES[name]
    return n * int(np.prod(shape)) * size
