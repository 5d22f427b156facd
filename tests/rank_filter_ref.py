"""numpy restatement of the rank filter of csrc/map_rankfilt.hip: what the GPU tests compare the kernel
with, bit for bit, and what tests/test_rank_filter_plan.py holds against scipy's recorded results.

Window `size = (size_h, size_w)` of n = size_h * size_w values, 0-based ascending rank r in 0 .. n - 1; per frame of H x W:

    out[y][x] = the r-th smallest of { x[R(y - size_h // 2 + i, H)][R(x - size_w // 2 + j, W)] : 0 <= i < size_h, 0 <= j < size_w }
    R(i, L): m = i mod 2L (non-negative);  m < L ? m : 2L - 1 - m          scipy's mode="reflect": d c b a | a b c d | d c b a

Even sizes lean towards index 0; a reflected pixel counts as often as it appears; a window larger than the frame reflects several
times.  `scipy.ndimage.rank_filter(x, rank=r, size=size, mode="reflect")` is this on finite data; `median_filter` is r = n // 2,
`percentile_filter(p)` is r = `rank_of_percentile(n, p)`.

Nothing is computed, only selected - `sort(window)[r]` -, and the order is spelled out here instead of left to `np.sort`:
  * zeros: values are ordered on their bit patterns (`order_key`: a monotone map of the float32 bits to integers), so -0 < +0 by
    construction, denormals and +-Inf are ordinary values, and the result carries the bits of the selected element;
  * NaN: a window that holds a NaN gives NaN at EVERY rank (tracked as a mask beside the values; which NaN is not specified).
    scipy's answer there is an accident of its selection algorithm and is not followed.
All leading axes are batch axes: frames are processed one by one."""
import numpy as np

MAX_SIZE = 15


def order_key(x: np.ndarray) -> np.ndarray:
    """float32 -> int64, strictly monotone in the IEEE total order of the non-NaN values: ... < -0 (key -1) < +0 (key 0) < ..."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def from_key(k: np.ndarray) -> np.ndarray:
    b = np.where(k < 0, k ^ 0x7FFFFFFF, k)
    return b.astype(np.int32).view(np.float32)


def pair(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))


def reflect(i, length: int):
    """R(i, L) of the module's header, for an integer or an integer array."""
    m = np.mod(i, 2 * length)                                               # numpy's mod of a negative number is non-negative
    return np.where(m < length, m, 2 * length - 1 - m)


def window_index(length: int, size: int) -> np.ndarray:
    """[L, size]: the source index of element j of the window around position p of one axis."""
    return reflect(np.arange(length)[:, None] - size // 2 + np.arange(size)[None, :], length)


def windows(a: np.ndarray, size) -> np.ndarray:
    """a [..., H, W] -> [..., H, W, n]: every pixel's window, reflected pixels as often as they appear."""
    sh, sw = pair(size)
    h, w = a.shape[-2:]
    iy, ix = window_index(h, sh), window_index(w, sw)
    g = a[..., iy[:, None, :, None], ix[None, :, None, :]]                  # [..., H, W, sh, sw]
    return g.reshape(*a.shape[:-2], h, w, sh * sw)


def median_rank(size) -> int:
    sh, sw = pair(size)
    return (sh * sw) // 2


def rank_of_percentile(n: int, p) -> int:
    """scipy.ndimage.percentile_filter's rank: p += 100 if p < 0; n - 1 if p == 100, else int(float(n) * p / 100.0)."""
    p = float(p)
    if p < 0.0:
        p += 100.0
    if not 0.0 <= p <= 100.0:
        raise ValueError("percentile out of range")
    return n - 1 if p == 100.0 else int(float(n) * p / 100.0)


def rank_filter(x: np.ndarray, size, rank) -> np.ndarray:
    """The r-th smallest of every window; rank "median" = n // 2."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim < 2:
        raise ValueError("maps need the two dimensions H, W")
    sh, sw = pair(size)
    n = sh * sw
    r = n // 2 if isinstance(rank, str) and rank == "median" else int(rank)
    if not (1 <= sh <= MAX_SIZE and 1 <= sw <= MAX_SIZE and 0 <= r < n):
        raise ValueError(f"size {sh} x {sw} or rank {r} out of range")
    nan = np.isnan(x)
    key = order_key(np.where(nan, np.float32(0), x))
    out = from_key(np.sort(windows(key, (sh, sw)), axis=-1)[..., r]).copy()  # integers: no NaN, no signed zeros in the sort
    out[windows(nan, (sh, sw)).any(axis=-1)] = np.nan
    return out


def rank_filters(x: np.ndarray, size, ranks) -> dict:
    """{rank: rank_filter(x, size, rank)} for several ranks of one window: one gather and one sort."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sh, sw = pair(size)
    nan = np.isnan(x)
    srt = np.sort(windows(order_key(np.where(nan, np.float32(0), x)), (sh, sw)), axis=-1)
    hit = windows(nan, (sh, sw)).any(axis=-1)
    out = {}
    for r in ranks:
        if not 0 <= int(r) < sh * sw:
            raise ValueError(f"rank {r} out of range")
        y = from_key(srt[..., int(r)]).copy()
        y[hit] = np.nan
        out[int(r)] = y
    return out


def apply(x: np.ndarray, steps) -> np.ndarray:
    """x through normalised steps ((size_h, size_w), rank), as metrics.apply_rank_filter runs them."""
    for size, rank in steps:
        x = rank_filter(x, size, rank)
    return x


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal NaN positions, equal bits everywhere else (so -0 and +0 differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def nan_footprint(h: int, w: int, points, size) -> np.ndarray:
    """The pixels whose window holds one of `points` - from the definition, pixel by pixel, not from `windows`."""
    sh, sw = pair(size)
    pts = set(map(tuple, points))
    m = np.zeros((h, w), bool)
    for y in range(h):
        rows = {int(reflect(y - sh // 2 + i, h)) for i in range(sh)}
        for x in range(w):
            cols = {int(reflect(x - sw // 2 + j, w)) for j in range(sw)}
            m[y, x] = any(py in rows and px in cols for py, px in pts)
    return m


def loop(x: np.ndarray, size, rank: int) -> np.ndarray:
    """The definition again as a per-pixel Python loop over one finite 2-D frame (values only, Python's sort of floats): the
    independent check of the gathered form above on small frames."""
    sh, sw = pair(size)
    a = np.asarray(x, dtype=np.float32)
    h, w = a.shape
    out = np.empty_like(a)
    for y in range(h):
        for xx in range(w):
            win = []
            for i in range(sh):
                m = (y - sh // 2 + i) % (2 * h)
                yy = m if m < h else 2 * h - 1 - m
                for j in range(sw):
                    m = (xx - sw // 2 + j) % (2 * w)
                    win.append(a[yy, m if m < w else 2 * w - 1 - m])
            out[y, xx] = sorted(win)[rank]
    return out
