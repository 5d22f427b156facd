"""numpy restatement of the event table (csrc/map_events.hip, metrics.detect_events) for the tests, without scipy: the foreground
predicate of tests/regions_ref.py, a 3-D union-find with the three link rules, the records in their exact layout and order, the
duration and volume filters, truncation with zero fill, the per-clip counts, the per-frame counts and the label volume."""
import numpy as np

import regions_ref

WORDS = 16
ROOT, VOLUME, T0, T1, X0, Y0, X1, Y1, PEAK, PEAK_INDEX, SUM_X, SUM_Y, SUM_T = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14

foreground = regions_ref.foreground
order_key = regions_ref.order_key


def steps(connectivity, temporal):
    """The neighbours (dt, dy, dx) that precede a voxel in raster order: inside the frame those of the 2-D labeller, in the frame
    before the voxel behind it (temporal 1) or its 3 x 3 (temporal 9, 8-connectivity only)."""
    assert connectivity in (4, 8) and temporal in (1, 9) and (temporal == 1 or connectivity == 8)
    inside = ((0, 0, -1), (0, -1, -1), (0, -1, 0), (0, -1, 1)) if connectivity == 8 else ((0, 0, -1), (0, -1, 0))
    before = ((-1, 0, 0),) if temporal == 1 else tuple((-1, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return inside + before


def structure(connectivity, temporal):
    """The same connectivity as the 3 x 3 x 3 structure scipy.ndimage.label takes."""
    s = np.zeros((3, 3, 3), int)
    for dt, dy, dx in steps(connectivity, temporal):
        s[1 + dt, 1 + dy, 1 + dx] = s[1 - dt, 1 - dy, 1 - dx] = 1
    s[1, 1, 1] = 1
    return s


def label(mask, connectivity=8, temporal=9):
    """mask: bool [t, h, w] -> int32 [t, h, w]: 0, or 1 + the smallest t * h * w + y * w + x of the voxel's component.  Union-find
    in raster order, the larger root always hung below the smaller."""
    mask = np.asarray(mask, dtype=bool)
    t, h, w = mask.shape
    flat = mask.reshape(-1)
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    nb = steps(connectivity, temporal)
    idx = np.flatnonzero(flat).tolist()
    for i in idx:
        parent[i] = i
        f, p = divmod(i, h * w)
        y, x = divmod(p, w)
        for dt, dy, dx in nb:
            ff, yy, xx = f + dt, y + dy, x + dx
            if ff >= 0 and 0 <= yy < h and 0 <= xx < w:
                j = (ff * h + yy) * w + xx
                if flat[j]:
                    a, b = find(i), find(j)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    labels = np.zeros(t * h * w, np.int32)
    for i in idx:
        labels[i] = find(i) + 1
    return labels.reshape(t, h, w)


def events(volume, threshold, connectivity=8, temporal=9):
    """All events of one clip [t, h, w] in ascending root order -> (uint32 [K, 16] records, int32 [t, h, w] labels)."""
    volume = np.ascontiguousarray(volume, np.float32)
    t, h, w = volume.shape
    labels = label(foreground(volume, threshold), connectivity, temporal)
    flat = labels.reshape(-1)
    idx = np.flatnonzero(flat).astype(np.int64)
    roots, inv = np.unique(flat[idx].astype(np.int64) - 1, return_inverse=True)
    k = len(roots)
    rec = np.zeros((k, WORDS), np.uint32)
    if k == 0:
        return rec, labels
    f, p = idx // (h * w), idx % (h * w)
    y, x = p // w, p % w
    big = np.iinfo(np.int64).max
    lo = {name: np.full(k, big) for name in "xyt"}
    hi = {name: np.zeros(k, np.int64) for name in "xyt"}
    for name, v in (("x", x), ("y", y), ("t", f)):
        np.minimum.at(lo[name], inv, v)
        np.maximum.at(hi[name], inv, v)
    word = (order_key(volume.reshape(-1)[idx]).astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)
    best = np.zeros(k, np.uint64)
    np.maximum.at(best, inv, word)
    peak_index = ~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rec[:, ROOT] = roots
    rec[:, VOLUME] = np.bincount(inv, minlength=k)
    rec[:, T0], rec[:, T1] = lo["t"], hi["t"]
    rec[:, X0], rec[:, Y0], rec[:, X1], rec[:, Y1] = lo["x"], lo["y"], hi["x"], hi["y"]
    rec[:, PEAK] = volume.reshape(-1)[peak_index.astype(np.int64)].view(np.uint32)
    rec[:, PEAK_INDEX] = peak_index
    for col, v in ((SUM_X, x), (SUM_Y, y), (SUM_T, f)):
        s = np.zeros(k, np.uint64)
        np.add.at(s, inv, v.astype(np.uint64))
        rec[:, col:col + 2] = s.view(np.uint32).reshape(k, 2)             # little-endian uint64 in two words
    assert np.array_equal(flat[roots], roots + 1) and np.array_equal(rec[:, T0], roots // (h * w))
    # an event has no gaps in time: every frame of t0..t1 holds one of its pixels
    present = np.zeros((k, t), bool)
    present[inv, f] = True
    assert np.array_equal(present.sum(1), hi["t"] - lo["t"] + 1)
    return rec, labels


def detect(volume, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """One clip -> (records uint32 [max_events, 16], counts uint32 [4], frame_counts uint32 [t, 3], labels int32 [t, h, w]): the
    events with t1 - t0 + 1 >= min_duration and volume >= min_volume in root order, the first max_events of them, zeros behind;
    counts = kept (all of them), dropped by a filter, foreground pixels, NaN pixels; frame_counts = per frame foreground pixels,
    pixels of kept events (truncated or not), NaN pixels; labels of every foreground voxel."""
    assert min_duration >= 1 and min_volume >= 1 and 1 <= max_events <= 65536
    volume = np.ascontiguousarray(volume, np.float32)
    t = volume.shape[0]
    rec, labels = events(volume, threshold, connectivity, temporal)
    keep = (rec[:, T1].astype(np.int64) - rec[:, T0] + 1 >= min_duration) & (rec[:, VOLUME] >= min_volume)
    kept = rec[keep]
    out = np.zeros((max_events, WORDS), np.uint32)
    n = min(len(kept), max_events)
    out[:n] = kept[:n]
    nan = np.isnan(volume)
    counts = np.array([len(kept), len(rec) - len(kept), int((labels != 0).sum()), int(nan.sum())], np.uint32)
    in_kept = np.isin(labels, kept[:, ROOT].astype(np.int64) + 1) & (labels != 0)
    frame_counts = np.stack([(labels != 0).reshape(t, -1).sum(1), in_kept.reshape(t, -1).sum(1), nan.reshape(t, -1).sum(1)], axis=1).astype(np.uint32)
    return out, counts, frame_counts, labels


def detect_batch(maps, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """maps float32 [b, t, h, w], every clip on its own -> (records [b, max_events, 16], counts [b, 4], frame_counts [b, t, 3],
    labels [b, t, h, w])."""
    maps = np.asarray(maps, np.float32)
    assert maps.ndim == 4 and len(maps) >= 1
    out = [detect(v, threshold, connectivity, temporal, min_duration, min_volume, max_events) for v in maps]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def sums(records):
    """(sum_x, sum_y, sum_t) int64 of records [..., 16]."""
    r = np.ascontiguousarray(records, np.uint32)
    s = r[..., SUM_X:SUM_X + 6].copy().view(np.uint64)
    return s[..., 0].astype(np.int64), s[..., 1].astype(np.int64), s[..., 2].astype(np.int64)


map_from_mask = regions_ref.map_from_mask
