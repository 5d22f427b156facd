"""Numpy restatement of the Gaussian map smoothing (csrc/map_smooth.hip), written from its specification:
scipy's taps, scipy's "reflect" border for one reflection, first along H then along W, every product and every sum rounded to
float32 on its own in ascending tap order.  numpy float32 arithmetic is exactly that, so the device result is compared with
`torch.equal`."""
import numpy as np


def taps(sigma: float, truncate: float = 4.0):
    """(r, float32 [2r + 1]): w[k] = exp(-0.5 / sigma^2 * (k - r)^2) in float64, divided by their float64 sum, rounded once."""
    r = int(truncate * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    w = w / w.sum()
    return r, w.astype(np.float32)


def reflect_index(n: int, r: int) -> np.ndarray:
    """int64 [n + 2r]: the source index of padded position i (coordinate i - r) under scipy's mode="reflect"
    (d c b a | a b c d | d c b a): -k -> k - 1, n - 1 + k -> n - k.  One reflection: r <= n."""
    if not 0 <= r <= n:
        raise ValueError(f"one reflection needs r <= n, got r={r}, n={n}")
    g = np.arange(-r, n + r, dtype=np.int64)
    return np.where(g < 0, -g - 1, np.where(g >= n, 2 * n - 1 - g, g))


def _pass(x: np.ndarray, w: np.ndarray, r: int, axis: int) -> np.ndarray:
    """One float32 pass along `axis`: acc = fl(w[0] x[0]); acc = fl(acc + fl(w[k] x[k])), k ascending."""
    n = x.shape[axis]
    xp = np.take(x, reflect_index(n, r), axis=axis)
    acc = None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(2 * r + 1):
            term = np.float32(w[k]) * np.take(xp, np.arange(k, k + n), axis=axis)
            acc = term if acc is None else acc + term
    assert acc.dtype == np.float32
    return acc


def smooth(maps: np.ndarray, sigma: float, truncate: float = 4.0) -> np.ndarray:
    """float32 maps [..., H, W] -> smoothed float32 of the same shape."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim >= 2
    r, w = taps(sigma, truncate)
    return _pass(_pass(maps, w, r, -2), w, r, -1)


def frame_max(smoothed: np.ndarray) -> np.ndarray:
    """Maximum over the last two axes with torch.amax semantics: NaN if any pixel of the frame is NaN."""
    with np.errstate(invalid="ignore"):
        return np.max(smoothed, axis=(-2, -1))                   # np.max propagates NaN


def window(h: int, w: int, y: int, x: int, r: int) -> np.ndarray:
    """bool [h, w]: the output pixels whose reflected window holds input pixel (y, x)."""
    rows = np.zeros(h, bool)
    cols = np.zeros(w, bool)
    iy, ix = reflect_index(h, r), reflect_index(w, r)
    for o in range(h):
        rows[o] = (iy[o:o + 2 * r + 1] == y).any()
    for o in range(w):
        cols[o] = (ix[o:o + 2 * r + 1] == x).any()
    return rows[:, None] & cols[None, :]
