"""numpy restatement of the defect-region table (csrc/map_regions.hip, metrics.detect_regions) for the tests, built on the reference
labeller of tests/pro_ref.py: the foreground predicate, the records in their exact layout and order, the min_area filter, truncation
with zero fill, the per-frame counts and the order key of the peak."""
import numpy as np

import pro_ref

WORDS = 12
ROOT, AREA, X0, Y0, X1, Y1, PEAK, PEAK_INDEX, SUM_X, SUM_Y = 0, 1, 2, 3, 4, 5, 6, 7, 8, 10


def foreground(frame, threshold):
    """v >= threshold: false for a NaN pixel, true for +Inf; a NaN threshold is not a threshold."""
    threshold = np.float32(threshold)
    assert not np.isnan(threshold)
    with np.errstate(invalid="ignore"):
        return np.asarray(frame, np.float32) >= threshold


def order_key(values):
    """uint32 keys with key(a) < key(b) iff a < b as floats, and key(-0.0) < key(+0.0)."""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def regions(frame, threshold, connectivity=8):
    """All foreground regions of one frame [h, w] in ascending root order -> (uint32 [K, 12] records, int32 [h, w] labels)."""
    frame = np.ascontiguousarray(frame, np.float32)
    h, w = frame.shape
    labels, _ = pro_ref.label(foreground(frame, threshold), connectivity)
    flat = labels.reshape(-1)
    idx = np.flatnonzero(flat).astype(np.int64)
    roots, inv = np.unique(flat[idx].astype(np.int64) - 1, return_inverse=True)
    k = len(roots)
    rec = np.zeros((k, WORDS), np.uint32)
    if k == 0:
        return rec, labels
    y, x = idx // w, idx % w
    big = np.iinfo(np.int64).max
    lo_x, lo_y, hi_x, hi_y = np.full(k, big), np.full(k, big), np.zeros(k, np.int64), np.zeros(k, np.int64)
    np.minimum.at(lo_x, inv, x)
    np.minimum.at(lo_y, inv, y)
    np.maximum.at(hi_x, inv, x)
    np.maximum.at(hi_y, inv, y)
    word = (order_key(frame.reshape(-1)[idx]).astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)
    best = np.zeros(k, np.uint64)
    np.maximum.at(best, inv, word)
    peak_index = ~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    sums = np.zeros((k, 2), np.uint64)
    np.add.at(sums[:, 0], inv, x.astype(np.uint64))
    np.add.at(sums[:, 1], inv, y.astype(np.uint64))
    rec[:, ROOT] = roots
    rec[:, AREA] = np.bincount(inv, minlength=k)
    rec[:, X0], rec[:, Y0], rec[:, X1], rec[:, Y1] = lo_x, lo_y, hi_x, hi_y
    rec[:, PEAK] = frame.reshape(-1)[peak_index.astype(np.int64)].view(np.uint32)
    rec[:, PEAK_INDEX] = peak_index
    rec[:, SUM_X:SUM_X + 2] = sums[:, 0].copy().view(np.uint32).reshape(k, 2)          # little-endian uint64 in two words
    rec[:, SUM_Y:SUM_Y + 2] = sums[:, 1].copy().view(np.uint32).reshape(k, 2)
    assert np.array_equal(roots, np.sort(roots)) and np.array_equal(flat[roots], roots + 1)
    return rec, labels


def detect(frame, threshold, connectivity=8, min_area=1, max_regions=64):
    """One frame -> (records uint32 [max_regions, 12], counts uint32 [4], labels int32 [h, w]): the regions with area >= min_area in
    root order, the first max_regions of them, zeros behind; counts = kept (all of them), dropped for area, foreground pixels, NaN
    pixels; labels of every foreground region."""
    assert min_area >= 1 and 1 <= max_regions <= 65536 and connectivity in (4, 8)
    rec, labels = regions(frame, threshold, connectivity)
    keep = rec[:, AREA] >= min_area
    kept = rec[keep]
    out = np.zeros((max_regions, WORDS), np.uint32)
    n = min(len(kept), max_regions)
    out[:n] = kept[:n]
    counts = np.array([len(kept), len(rec) - len(kept), int((labels != 0).sum()), int(np.isnan(np.asarray(frame, np.float32)).sum())], np.uint32)
    return out, counts, labels


def detect_batch(maps, threshold, connectivity=8, min_area=1, max_regions=64):
    """maps float32 [n, h, w], every frame on its own -> (records uint32 [n, max_regions, 12], counts uint32 [n, 4], labels int32
    [n, h, w])."""
    maps = np.asarray(maps, np.float32)
    assert maps.ndim == 3
    out = [detect(f, threshold, connectivity, min_area, max_regions) for f in maps]
    if not out:
        return (np.zeros((0, max_regions, WORDS), np.uint32), np.zeros((0, 4), np.uint32), np.zeros(maps.shape, np.int32))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])


def sums(records):
    """(sum_x, sum_y) int64 of records [..., 12]."""
    r = np.ascontiguousarray(records, np.uint32)
    s = r[..., SUM_X:SUM_X + 4].copy().view(np.uint64)
    return s[..., 0].astype(np.int64), s[..., 1].astype(np.int64)


def map_from_mask(rng, mask, threshold):
    """A float32 map whose foreground under `threshold` is exactly `mask`: seeded random values >= threshold on it (the threshold
    itself among them) and < threshold off it."""
    mask = np.asarray(mask, bool)
    t = np.float32(threshold)
    span = np.float32(max(abs(float(t)), 1.0))
    hi = (t + span * rng.random(mask.shape).astype(np.float32)).astype(np.float32)
    hi[rng.random(mask.shape) < 0.1] = t
    lo = (t - span * (np.float32(0.01) + rng.random(mask.shape).astype(np.float32))).astype(np.float32)
    out = np.where(mask, hi, lo).astype(np.float32)
    assert np.array_equal(foreground(out, t), mask)
    return out
