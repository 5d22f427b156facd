"""numpy restatement of the score histogram (csrc/score_hist.hip) for the tests: the quantiser, the per-class bin counts with the
rejection rules, and q(v) = the value a score is quantised to."""
import numpy as np


def nbins(m):
    return 255 << m


def positive(labels, fmt):
    """Class of every label under a label format of vad_hist_accumulate: 'u8' >= 128, 'f32' > 0.5, 'group' non-zero."""
    labels = np.asarray(labels)
    if fmt == "u8":
        return labels >= 128
    if fmt == "f32":
        return labels > np.float32(0.5)
    if fmt == "group":
        return labels != 0
    raise ValueError(fmt)


def keys_of(values, m):
    """-> (key uint32, binned bool) per element: key = bits >> (23 - m) for a finite v >= 0 (-0.0 is 0); negatives, NaN and
    infinities are not binned."""
    bits = np.ascontiguousarray(values, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    return bits >> np.uint32(23 - m), bits < 0x7F800000


def ref_counts(values, pos, m):
    """values: float32, any shape; pos: bool, one per element (same size).  -> (counts int64 [2, nbins], rejected int64 [2])."""
    key, ok = keys_of(values, m)
    pos = np.asarray(pos, dtype=bool).reshape(-1)
    assert pos.size == key.size
    counts = np.stack([np.bincount(key[ok & (pos == c)], minlength=nbins(m)) for c in (False, True)]).astype(np.int64)
    rejected = np.array([np.sum(~ok & ~pos), np.sum(~ok & pos)], np.int64)
    return counts, rejected


def q(values, m):
    """Keep the top m mantissa bits (float32 in, float32 out; finite non-negative input)."""
    key, ok = keys_of(values, m)
    assert ok.all()
    return (key << np.uint32(23 - m)).view(np.float32).reshape(np.shape(values))
