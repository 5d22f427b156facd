"""numpy restatement of the temporal filters of csrc/map_temporal.hip: what the GPU tests compare the
kernel with, bit for bit, and what tests/test_map_temporal_plan.py holds against scipy's recorded results.

Time is axis 0 of a stream `x[T, ...]`; every other axis is a pixel axis.  Per pixel, causal, over the frames that exist:

    min / max   y[t] = minimum / maximum of x[max(0, t - k + 1) .. t]
    mean        y[t] = float32(S / c), c = min(t + 1, k), S = the float64 sum of the window added OLDEST TO NEWEST - an explicit loop:
                np.sum adds pairwise -, the division in float64, one rounding to float32
    ema         y[0] = x[0], y[t] = y[t-1] + a * (x[t] - y[t-1]), a = float32(alpha), all of it float32 arrays: under NEP 50 a Python
                float times a float32 array stays float32, and so does np.float32 - every operation rounds to float32 on its own

Minimum and maximum are the IEEE-754-2019 `minimum` / `maximum`, ordered on bit patterns as tests/map_morph_ref.py does: a window
that holds a NaN gives NaN (a mask beside the keys), -0 < +0 by construction.

`Stream` is the stateful form: it takes the frames of a stream call by call and keeps, per step, what the kernel's state keeps -
the last k - 1 inputs, or the EMA's last output."""
import numpy as np

from map_morph_ref import from_key, order_key, same_bits  # noqa: F401  (same_bits: for the tests)

OPS = ("min", "max", "mean", "ema")
_BIG = np.int64(1) << 40


def _minmax(x: np.ndarray, k: int, is_max: bool) -> np.ndarray:
    nan = np.isnan(x)
    key = order_key(np.where(nan, np.float32(0), x)).reshape(x.shape)
    out_k = np.empty_like(key)
    out_m = np.empty_like(nan)
    for t in range(x.shape[0]):
        win = key[max(0, t - k + 1):t + 1]
        out_k[t] = win.max(axis=0) if is_max else win.min(axis=0)               # integers: no NaN, no zeros
        out_m[t] = nan[max(0, t - k + 1):t + 1].any(axis=0)
    out = from_key(out_k).reshape(x.shape).copy()
    out[out_m] = np.nan
    return out


def _mean(x: np.ndarray, k: int) -> np.ndarray:
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(x.shape[0]):
            lo = max(0, t - k + 1)
            s = x[lo].astype(np.float64)
            for j in range(lo + 1, t + 1):                                      # oldest to newest, one addition at a time
                s = s + x[j].astype(np.float64)
            out[t] = (s / np.float64(t + 1 - lo)).astype(np.float32)
    return out


def _ema(x: np.ndarray, alpha, y=None) -> np.ndarray:
    """`y`: the average before x[0] (float32), or None: x[0] starts it."""
    a = np.float32(alpha)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for t in range(x.shape[0]):
            if y is None:
                y = x[t].copy()
            else:
                d = x[t] - y
                p = a * d
                y = y + p
                assert d.dtype == p.dtype == y.dtype == np.float32
            out[t] = y
    return out


def temporal(op: str, x, param) -> np.ndarray:
    """One filter along axis 0 of a whole stream, frame 0 its first."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape[0] == 0:
        return x.copy()
    if op == "ema":
        return _ema(x, param)
    if op == "mean":
        return _mean(x, int(param))
    return _minmax(x, int(param), op == "max")


def apply(steps, x) -> np.ndarray:
    for op, param in steps:
        x = temporal(op, x, param)
    return np.ascontiguousarray(x, dtype=np.float32)


def clips(steps, x) -> np.ndarray:
    """`x[B, T, ...]`: every clip a fresh stream."""
    return np.stack([apply(steps, c) for c in np.asarray(x, dtype=np.float32)]) if len(x) else np.asarray(x, dtype=np.float32).copy()


class Stream:
    """One stream through `steps`, its frames arriving call by call: `update(x[T, ...])` -> the T filtered frames."""

    def __init__(self, steps):
        self.steps = tuple(steps)
        self.reset()

    def reset(self):
        self.seen = 0
        self.kept = [None] * len(self.steps)       # min / max / mean: the last min(seen, k - 1) inputs; ema: the last output

    def update(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = x.shape[0]
        if n == 0:
            return x.copy()
        for i, (op, param) in enumerate(self.steps):
            if op == "ema":
                y = _ema(x, param, self.kept[i])
                self.kept[i] = y[-1].copy()
            else:
                k = int(param)
                old = self.kept[i] if self.kept[i] is not None else x[:0]
                both = np.concatenate([old, x])                                # a short history IS the stream's beginning
                y = temporal(op, both, k)[len(old):]
                self.kept[i] = both[len(both) - min(len(both), k - 1):].copy()
            x = y
        self.seen += n
        return x
