"""numpy restatement of the per-frame tracks of anomaly events (csrc/map_event_tracks.hip, metrics.event_tracks,
EventTracker.update(boxes=True)) for the tests, from the specification alone: a cross-section is the set of
one event's pixels in one frame, written as the twelve words of a region record.  Clip mode is built on tests/events_ref.py (the
label volume and the kept records say which event a pixel belongs to), live mode on tests/track_ref.py (the slot plane does)."""
import numpy as np

import events_ref
import regions_ref
import track_ref

WORDS = regions_ref.WORDS
ROOT, AREA, X0, Y0, X1, Y1, PEAK, PEAK_INDEX, SUM_X, SUM_Y = (regions_ref.ROOT, regions_ref.AREA, regions_ref.X0, regions_ref.Y0, regions_ref.X1,
                                                              regions_ref.Y1, regions_ref.PEAK, regions_ref.PEAK_INDEX, regions_ref.SUM_X,
                                                              regions_ref.SUM_Y)
MAX_RECORDS = 2 ** 26


def section(frame, pix):
    """One cross-section: frame float32 [h, w], pix = the flat indices y * w + x of the event's pixels in it -> uint32 [12]; all-zero
    for no pixel.  The peak is the largest order key, among equals the smallest index."""
    frame = np.ascontiguousarray(frame, np.float32)
    w = frame.shape[1]
    pix = np.asarray(pix, np.int64)
    rec = np.zeros(WORDS, np.uint32)
    if len(pix) == 0:
        return rec
    y, x = pix // w, pix % w
    values = frame.reshape(-1)
    best = max((int(regions_ref.order_key(values[i:i + 1])[0]), -int(i)) for i in pix)
    peak_index = -best[1]
    rec[ROOT], rec[AREA] = pix.min(), len(pix)
    rec[X0], rec[Y0], rec[X1], rec[Y1] = x.min(), y.min(), x.max(), y.max()
    rec[PEAK], rec[PEAK_INDEX] = values[peak_index:peak_index + 1].view(np.uint32)[0], peak_index
    for col, v in ((SUM_X, int(x.sum())), (SUM_Y, int(y.sum()))):
        rec[col], rec[col + 1] = v & 0xFFFFFFFF, v >> 32
    return rec


def tracks_of(volume, labels, records, kept):
    """One clip: volume float32 [t, h, w], labels int32 [t, h, w] (0 or 1 + root), records uint32 [max_events, 16] and kept = the
    clip's count of kept events -> uint32 [max_events, t, 12]: record (e, f) the cross-section of kept event e in frame f, zeros
    behind the kept events; a pixel whose root has no record among the first min(kept, max_events) contributes nothing."""
    volume = np.ascontiguousarray(volume, np.float32)
    t = volume.shape[0]
    max_events = len(records)
    out = np.zeros((max_events, t, WORDS), np.uint32)
    for e in range(min(int(kept), max_events)):
        label = int(records[e, events_ref.ROOT]) + 1
        for f in range(t):
            out[e, f] = section(volume[f], np.flatnonzero(labels[f].reshape(-1) == label))
    return out


def tracks(volume, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """One clip -> (tracks uint32 [max_events, t, 12], then what events_ref.detect returns: records, counts, frame_counts, labels)."""
    records, counts, frame_counts, labels = events_ref.detect(volume, threshold, connectivity, temporal, min_duration, min_volume, max_events)
    return tracks_of(volume, labels, records, counts[0]), records, counts, frame_counts, labels


def tracks_batch(maps, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """maps float32 [b, t, h, w], every clip on its own -> the five arrays of `tracks`, stacked."""
    maps = np.asarray(maps, np.float32)
    assert maps.ndim == 4 and len(maps) >= 1 and len(maps) * max_events * maps.shape[1] <= MAX_RECORDS
    out = [tracks(v, threshold, connectivity, temporal, min_duration, min_volume, max_events) for v in maps]
    return tuple(np.stack([o[k] for o in out]) for k in range(5))


def boxes(tracker, frame):
    """Live mode: tracker = a track_ref.Tracker after its update, frame = the newest map [h, w] it took in -> uint32 [max_open, 12]:
    record r the cross-section of the open event in slot r, from the slot plane (0, slot + 1, NO_RECORD for a lost event's pixels,
    which contribute nothing); zeros behind the open events."""
    out = np.zeros((tracker.max_open, WORDS), np.uint32)
    frame = np.ascontiguousarray(frame, np.float32).reshape(tracker.h, tracker.w)
    for r in range(len(tracker.table)):
        out[r] = section(frame, np.flatnonzero(tracker.plane == r + 1))
        assert out[r, ROOT] == tracker.table[r]["handle"] and out[r, AREA] > 0
    assert track_ref.NO_RECORD > tracker.max_open
    return out


def sums(records):
    """(sum_x, sum_y) int64 of cross-section records [..., 12]."""
    return regions_ref.sums(records)
