"""numpy restatement of the grey morphology of csrc/map_morph.hip: what the GPU tests compare the kernel
with, bit for bit, and what tests/test_map_morph_plan.py holds against scipy's recorded results.

Flat rectangle `size = (size_h, size_w)`, windows clamped to the frame, scipy's even-size convention; per axis of length L, size s:

    erode   out[i] = min x[max(0, i - s // 2)       .. min(L - 1, i + (s - 1) // 2)]
    dilate  out[i] = max x[max(0, i - (s - 1) // 2) .. min(L - 1, i + s // 2)]
    open = dilate(erode(x)),  close = erode(dilate(x)), the second step on the intermediate IMAGE (clamped again)

Minimum and maximum are the IEEE-754-2019 `minimum` / `maximum`, spelled out here instead of left to `np.minimum`:
  * NaN: a window that holds a NaN gives NaN (tracked as a mask beside the values; which NaN is not specified);
  * zeros: values are ordered on their bit patterns (`order_key`: a monotone map of the float32 bits to integers), so -0 < +0
    by construction and the result carries the bits of the window's extreme element.
All leading axes are batch axes: frames are processed one by one."""
import numpy as np

OPS = ("erode", "dilate", "open", "close")
_BIG = np.int64(1) << 40                     # beyond every key: the identity of a clamped window


def order_key(x: np.ndarray) -> np.ndarray:
    """float32 -> int64, strictly monotone in the IEEE total order of the non-NaN values: ... < -0 (key -1) < +0 (key 0) < ..."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7FFFFFFF, b)


def from_key(k: np.ndarray) -> np.ndarray:
    b = np.where(k < 0, k ^ 0x7FFFFFFF, k)
    return b.astype(np.int32).view(np.float32)


def reach(size: int, is_max: bool):
    """(towards index 0, towards the end): how far the window of one axis reaches."""
    return ((size - 1) // 2, size // 2) if is_max else (size // 2, (size - 1) // 2)


def _axis(key: np.ndarray, nan: np.ndarray, size: int, axis: int, is_max: bool):
    """One axis of one step on (keys, NaN mask): the clamped window as a full window over an identity-padded line."""
    lo, hi = reach(size, is_max)
    n = key.shape[axis]
    pad = [(0, 0)] * key.ndim
    pad[axis] = (lo, hi)
    kp = np.pad(key, pad, constant_values=-_BIG if is_max else _BIG)
    mp = np.pad(nan, pad, constant_values=False)
    out_k, out_m = None, None
    for d in range(size):                                                   # the plain window: one shifted slice per element
        sl = [slice(None)] * key.ndim
        sl[axis] = slice(d, d + n)
        k, m = kp[tuple(sl)], mp[tuple(sl)]
        out_k = k if out_k is None else (np.maximum(out_k, k) if is_max else np.minimum(out_k, k))    # integers: no NaN, no zeros
        out_m = m if out_m is None else (out_m | m)
    return out_k, out_m


def _step(x: np.ndarray, size, is_max: bool) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim < 2:
        raise ValueError("maps need the two dimensions H, W")
    sh, sw = (size, size) if np.isscalar(size) else size
    nan = np.isnan(x)
    key = order_key(np.where(nan, np.float32(0), x))
    key, nan = _axis(key, nan, int(sh), x.ndim - 2, is_max)
    key, nan = _axis(key, nan, int(sw), x.ndim - 1, is_max)
    out = from_key(key).copy()
    out[nan] = np.nan
    return out


def erode(x, size):
    return _step(x, size, False)


def dilate(x, size):
    return _step(x, size, True)


def opening(x, size):
    return dilate(erode(x, size), size)


def closing(x, size):
    return erode(dilate(x, size), size)


def morph(op: str, x, size):
    return {"erode": erode, "dilate": dilate, "open": opening, "close": closing}[op](x, size)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Equal NaN positions, equal bits everywhere else (so -0 and +0 differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb]))


def loop(op: str, x: np.ndarray, size) -> np.ndarray:
    """The definition again as a per-pixel Python loop over one finite 2-D frame (values only): the independent check of the
    sliced form above on small frames."""
    sh, sw = (size, size) if np.isscalar(size) else size

    def step(a, is_max):
        h, w = a.shape
        (lh, hh), (lw, hw) = reach(sh, is_max), reach(sw, is_max)
        out = np.empty_like(a)
        for i in range(h):
            for j in range(w):
                win = a[max(0, i - lh):min(h - 1, i + hh) + 1, max(0, j - lw):min(w - 1, j + hw) + 1]
                out[i, j] = win.max() if is_max else win.min()
        return out

    a = np.asarray(x, dtype=np.float32)
    seq = {"erode": (False,), "dilate": (True,), "open": (False, True), "close": (True, False)}[op]
    for is_max in seq:
        a = step(a, is_max)
    return a
