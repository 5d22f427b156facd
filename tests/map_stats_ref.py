"""Numpy restatement of the per-pixel map statistics and the z-score map (csrc/map_stats.hip), written from
their specification: float64 planes K, S1, S2 and a frame count; every frame added in order, every product and every sum rounded
on its own.  numpy float64 / float32 arithmetic is exactly that (IEEE add, multiply, divide and square root, no contraction), so
the device result is compared with `torch.equal`."""
import numpy as np


class State:
    """n frames seen; K, S1, S2 float64 [H, W]."""

    def __init__(self, h: int, w: int):
        self.n = 0
        self.K = np.zeros((h, w), np.float64)
        self.S1 = np.zeros((h, w), np.float64)
        self.S2 = np.zeros((h, w), np.float64)

    def copy(self) -> "State":
        s = State(*self.K.shape)
        s.n, s.K, s.S1, s.S2 = self.n, self.K.copy(), self.S1.copy(), self.S2.copy()
        return s

    def planes(self) -> np.ndarray:
        return np.stack([self.K, self.S1, self.S2])


def accumulate(state: State, maps: np.ndarray) -> State:
    """Add float32 maps [..., H, W] frame by frame, in row-major order of the leading dimensions: empty state -> K = (double)x[0],
    S1 = S2 = 0; per frame d = (double)x - K, S1 = S1 + d, S2 = S2 + d * d."""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.shape[-2:] == state.K.shape
    frames = maps.reshape(-1, *state.K.shape)
    if len(frames) == 0:
        return state
    with np.errstate(invalid="ignore", over="ignore"):
        if state.n == 0:
            state.K = frames[0].astype(np.float64)
            state.S1 = np.zeros_like(state.K)
            state.S2 = np.zeros_like(state.K)
        for x in frames:
            d = x.astype(np.float64) - state.K
            state.S1 = state.S1 + d
            state.S2 = state.S2 + d * d
    state.n += len(frames)
    return state


def merge(a: State, b: State) -> State:
    """a += b.  dl = K_b - K_a; S1 = S1_a + (S1_b + n_b dl); S2 = S2_a + (S2_b + ((2 dl) S1_b + (n_b dl) dl)); K_a is kept; an empty
    side gives the other side."""
    if b.n == 0:
        return a
    if a.n == 0:
        a.n, a.K, a.S1, a.S2 = b.n, b.K.copy(), b.S1.copy(), b.S2.copy()
        return a
    with np.errstate(invalid="ignore", over="ignore"):
        dl = b.K - a.K
        ndl = np.float64(b.n) * dl
        a.S1 = a.S1 + (b.S1 + ndl)
        a.S2 = a.S2 + (b.S2 + ((2.0 * dl) * b.S1 + ndl * dl))
    a.n += b.n
    return a


def finalize(state: State, ddof: int = 1):
    """(mean, std) float32 [H, W]: mean = fl32(K + S1 / n); var = (S2 - S1 (S1 / n)) / (n - ddof), var < 0 -> 0 (a NaN stays),
    std = sqrt in float32 of fl32(var).  n == 0: both NaN; n - ddof <= 0: std NaN."""
    assert ddof in (0, 1)
    nan = np.full(state.K.shape, np.nan, np.float32)
    if state.n == 0:
        return nan, nan.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = np.float64(state.n)
        q = state.S1 / n
        mean = (state.K + q).astype(np.float32)
        if state.n - ddof <= 0:
            return mean, nan
        var = (state.S2 - state.S1 * q) / (n - np.float64(ddof))
        var = np.where(var < 0.0, 0.0, var)
        std = np.sqrt(var.astype(np.float32))
    assert std.dtype == np.float32
    return mean, std


def normalize(maps: np.ndarray, mean: np.ndarray, std: np.ndarray, min_std: float) -> np.ndarray:
    """z = (x - mean) / (std < min_std ? min_std : std) in float32; a NaN std stays NaN."""
    maps = np.asarray(maps)
    assert maps.dtype == mean.dtype == std.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        den = np.where(std < np.float32(min_std), np.float32(min_std), std)
        z = (maps - mean) / den
    assert z.dtype == np.float32
    return z


def frame_max(z: np.ndarray) -> np.ndarray:
    """Maximum over the last two axes with torch.amax semantics: NaN if any pixel of the frame is NaN."""
    with np.errstate(invalid="ignore"):
        return np.max(z, axis=(-2, -1))


def ulps32(got: np.ndarray, want64: np.ndarray) -> float:
    """The largest distance of float32 `got` from float64 `want64` in units in the last place of float32 at `want64`."""
    want64 = np.asarray(want64, np.float64)
    unit = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want64) / unit))
