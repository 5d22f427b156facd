"""numpy restatement of the matched-event tables (csrc/map_event_match.hip, metrics.match_events) for the tests, built on the 3-D
union-find and the event table of tests/events_ref.py for both volumes: the kept events and the mask volume's tracks in root order,
hit and overlap as voxel counts of one labelling under the other's foreground with the first and last shared frame, the two
fraction tests as one float64 multiply and compare, truncation with zero fill, the 22 counters of a clip and the four of a frame."""
import numpy as np

import events_ref
import match_ref

WORDS = 8
COUNTS = 22
ROOT, VOLUME, T0, T1, SHARED, FIRST, LAST, FLAGS = range(8)
(GT_TRACKS, GT_DETECTED, PRED_EVENTS, PRED_MATCHED, FALSE_ALARMS, PRED_DROPPED, TP, FP, FN, TN, NAN_VOXELS, GT_VOXELS, DELAY_SUM, IMMEDIATE,
 F_BOTH, F_PRED_ONLY, F_GT_ONLY, F_NEITHER, C_BOTH, C_PRED_ONLY, C_GT_ONLY, C_NEITHER) = range(22)
NONE = 0xFFFFFFFF

passes = match_ref.passes


def components(mask, connectivity, temporal):
    """bool [t, h, w] -> (uint32 [K, 4] root, volume, t0, t1 in ascending root order, int32 labels [t, h, w])."""
    t, h, w = mask.shape
    labels = events_ref.label(mask, connectivity, temporal)
    flat = labels.reshape(-1)
    idx = np.flatnonzero(flat).astype(np.int64)
    roots, inv = np.unique(flat[idx].astype(np.int64) - 1, return_inverse=True)
    rec = np.zeros((len(roots), 4), np.uint32)
    if len(roots):
        f = idx // (h * w)
        last = np.zeros(len(roots), np.int64)
        np.maximum.at(last, inv, f)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = roots, np.bincount(inv, minlength=len(roots)), roots // (h * w), last
    return rec, labels


def _joined(rec, labels, other, fraction):
    """[K, 4] components and their labels -> [K, 8]: the voxels shared with the bool volume `other`, their first and last frame."""
    t, h, w = labels.shape
    out = np.zeros((len(rec), WORDS), np.uint32)
    out[:, :4] = rec
    out[:, FIRST] = out[:, LAST] = NONE
    frames = np.broadcast_to(np.arange(t)[:, None, None], labels.shape)
    for k, root in enumerate(rec[:, 0].astype(np.int64)):
        shared = (labels == root + 1) & other
        n = int(shared.sum())
        out[k, SHARED] = n
        if n:
            out[k, FIRST], out[k, LAST] = frames[shared].min(), frames[shared].max()
    out[:, FLAGS] = passes(out[:, SHARED], out[:, VOLUME], fraction)
    return out


def tables(volume, mask, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, gt_fraction=0.0, pred_fraction=0.0):
    """One clip [t, h, w] and its bool mask volume -> (gt uint32 [Kg, 8], pred uint32 [Kp, 8], P bool [t, h, w], dropped events)."""
    volume = np.ascontiguousarray(volume, np.float32)
    mask = np.asarray(mask, bool)
    assert volume.shape == mask.shape and volume.ndim == 3
    prec, plabels = components(events_ref.foreground(volume, threshold), connectivity, temporal)
    keep = (prec[:, 3].astype(np.int64) - prec[:, 2] + 1 >= min_duration) & (prec[:, 1] >= min_volume)
    kept = prec[keep]
    P = np.isin(plabels, kept[:, 0].astype(np.int64) + 1) & (plabels != 0)
    grec, glabels = components(mask, connectivity, temporal)
    return _joined(grec, glabels, P, gt_fraction), _joined(kept, plabels, mask, pred_fraction), P, len(prec) - len(kept)


def match(volume, mask, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, gt_fraction=0.0, pred_fraction=0.0, max_events=64):
    """One clip -> (gt_records uint32 [max_events, 8], pred_records uint32 [max_events, 8], counts uint64 [22], frame_counts uint32 [t, 4])."""
    assert 1 <= max_events <= 65536
    gt, pred, P, dropped = tables(volume, mask, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction)
    mask = np.asarray(mask, bool)
    t = mask.shape[0]
    out_g, out_p = np.zeros((max_events, WORDS), np.uint32), np.zeros((max_events, WORDS), np.uint32)
    out_g[:min(len(gt), max_events)] = gt[:max_events]
    out_p[:min(len(pred), max_events)] = pred[:max_events]
    nan = np.isnan(np.asarray(volume, np.float32))
    frames = np.stack([(P & mask).reshape(t, -1).sum(1), (P & ~mask).reshape(t, -1).sum(1), (~P & mask).reshape(t, -1).sum(1),
                       nan.reshape(t, -1).sum(1)], axis=1).astype(np.uint32)
    c = np.zeros(COUNTS, np.uint64)
    det = gt[:, FLAGS] == 1
    c[GT_TRACKS], c[GT_DETECTED] = len(gt), int(det.sum())
    c[PRED_EVENTS], c[PRED_MATCHED] = len(pred), int(pred[:, FLAGS].sum())
    c[FALSE_ALARMS], c[PRED_DROPPED] = len(pred) - int(pred[:, FLAGS].sum()), dropped
    c[TP], c[FP], c[FN], c[TN] = int((P & mask).sum()), int((P & ~mask).sum()), int((~P & mask).sum()), int((~P & ~mask).sum())
    c[NAN_VOXELS], c[GT_VOXELS] = int(nan.sum()), int(mask.sum())
    delays = gt[det, FIRST].astype(np.int64) - gt[det, T0].astype(np.int64)
    assert (delays >= 0).all()
    c[DELAY_SUM], c[IMMEDIATE] = int(delays.sum()), int((delays == 0).sum())
    in_p, in_g = P.reshape(t, -1).any(1), mask.reshape(t, -1).any(1)
    c[F_BOTH], c[F_PRED_ONLY], c[F_GT_ONLY], c[F_NEITHER] = (int((in_p & in_g).sum()), int((in_p & ~in_g).sum()), int((~in_p & in_g).sum()),
                                                               int((~in_p & ~in_g).sum()))
    c[C_BOTH + (0 if len(gt) and len(pred) else 1 if len(pred) else 2 if len(gt) else 3)] = 1
    return out_g, out_p, c, frames


def match_batch(maps, masks, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, gt_fraction=0.0, pred_fraction=0.0,
                max_events=64):
    """maps float32 [b, t, h, w], masks bool [b, t, h, w], every clip on its own -> (gt_records [b, max_events, 8], pred_records
    [b, max_events, 8], counts uint64 [b, 22], frame_counts uint32 [b, t, 4])."""
    maps = np.asarray(maps, np.float32)
    masks = np.asarray(masks, bool)
    assert maps.ndim == 4 and maps.shape == masks.shape and len(maps) >= 1
    out = [match(v, m, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction, max_events)
           for v, m in zip(maps, masks)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


# ---------------------------------------------------------------------- the cases by hand: 5 x 12 x 20 volumes
T = np.float32(1.0)
SHAPE = (5, 12, 20)


def case(name):
    """-> (maps float32 [b, 5, 12, 20], masks bool [b, 5, 12, 20], kwargs of match) of one hand-made case; foreground is 2.0."""
    fg = np.zeros((2,) + SHAPE, bool)
    gt = np.zeros((2,) + SHAPE, bool)
    nan = np.zeros((2,) + SHAPE, bool)
    kw = {}
    b = 1
    if name == "hit_in_the_last_frame":                        # a track of four frames, the event only on its last: delay 3
        gt[0, 0:4, 2:5, 2:6] = True
        fg[0, 3, 3:5, 4:9] = True
    elif name == "hit_by_a_dropped_event":                     # the only event lasts one frame: min_duration 2 drops it
        gt[0, 1:4, 2:5, 2:6] = True
        fg[0, 2, 2:5, 2:6] = True
        kw = {"min_duration": 2}
    elif name == "one_event_over_two_tracks":
        gt[0, 1:3, 2:4, 2:5] = gt[0, 1:3, 2:4, 10:13] = True
        fg[0, 2, 3, 1:15] = True
    elif name == "two_events_on_one_track":
        gt[0, 0:5, 5:8, 2:18] = True
        fg[0, 1, 6, 3:6] = fg[0, 3:5, 6, 12:15] = True
    elif name == "merge_and_split":                            # two tracks' worth of blobs joined by a bridge in frame 2 only
        gt[0, :, 2:5, 2:6] = gt[0, :, 2:5, 12:16] = True
        gt[0, 2, 3, 6:12] = True
        fg[0, 0:2, 3, 3:5] = fg[0, 3:5, 3, 13:15] = True       # two events, both inside the one track
    elif name == "consecutive_frames_only":                    # the same pixels, the event one frame after the mask: no overlap
        gt[0, 1, 4:7, 4:9] = True
        fg[0, 2, 4:7, 4:9] = True
    elif name == "diagonal_touch":
        gt[0, 2, 2:4, 2:4] = True
        fg[0, 2, 4:6, 4:6] = True
    elif name == "clips_never_link":                           # the last frame of clip 0 over the first frame of clip 1
        b = 2
        fg[0, 4, 3:6, 3:8] = True
        gt[1, 0, 3:6, 3:8] = True
    elif name == "nan_inside_a_track":
        gt[0, 1:3, 2:6, 2:8] = True
        fg[0, 1:3, 2:6, 2:8] = True
        nan[0, 2, 3, 4] = True
    elif name == "fraction_boundary_passes":                   # 15 of 60 at fraction 0.25, both ways
        gt[0, 1, 2:8, 2:12] = True                             # a track of 60 voxels ...
        fg[0, 1, 2:5, 2:7] = True                              # ... hit in 15
        fg[0, 1, 0:2, 2:7] = fg[0, 1, 2:9, 0:2] = True         # the event: 15 + 10 + 14 = 39 ... made 60 below
        fg[0, 1, 9:12, 0:7] = True                             # + 21 = 60 voxels, 15 of them on the mask
        kw = {"gt_fraction": 0.25, "pred_fraction": 0.25, "connectivity": 4, "temporal": 1}
    elif name == "fraction_boundary_fails":                    # 14 of 60
        gt[0, 1, 2:8, 2:12] = True
        fg[0, 1, 2:5, 2:7] = True
        fg[0, 1, 0:2, 2:7] = fg[0, 1, 2:9, 0:2] = True
        fg[0, 1, 9:12, 0:7] = True
        gt[0, 1, 4, 6] = False                                 # one shared voxel leaves the mask: a track of 59, 14 shared ...
        gt[0, 1, 7, 12] = True                                 # ... and back to 60 elsewhere
        kw = {"gt_fraction": 0.25, "pred_fraction": 0.25, "connectivity": 4, "temporal": 1}
    elif name == "truncation":                                 # five tracks and four events, tables of three
        for k in range(5):
            gt[0, k, 1:3, 1 + 3 * k:3 + 3 * k] = True
        for k in range(4):
            fg[0, k, 2:4, 2 + 3 * k:4 + 3 * k] = True
        kw = {"max_events": 3, "temporal": 1}
    else:
        raise KeyError(name)
    maps = np.where(fg, np.float32(2.0), np.float32(0.0)).astype(np.float32)
    maps[nan] = np.nan
    return maps[:b], gt[:b], kw


CASES = ("hit_in_the_last_frame", "hit_by_a_dropped_event", "one_event_over_two_tracks", "two_events_on_one_track", "merge_and_split",
         "consecutive_frames_only", "diagonal_touch", "clips_never_link", "nan_inside_a_track", "fraction_boundary_passes",
         "fraction_boundary_fails", "truncation")
