"""numpy restatement of the matched-region tables (csrc/map_match.hip, metrics.match_regions) for the tests, built on the reference
labeller of tests/pro_ref.py and the region table of tests/regions_ref.py: the kept predictions and the mask's regions in root order,
hit and overlap as pixel counts of one labelling under the other's foreground, the two fraction tests as one float64 multiply and
compare, truncation with zero fill, and the sixteen counters of a frame."""
import numpy as np

import pro_ref
import regions_ref

WORDS = 4
COUNTS = 16
ROOT, AREA, SHARED, FLAGS = 0, 1, 2, 3
(GT_REGIONS, GT_DETECTED, PRED_REGIONS, PRED_MATCHED, FALSE_ALARMS, PRED_DROPPED, TP, FP, FN, TN, NAN_PIXELS, GT_PIXELS, C_BOTH, C_PRED_ONLY,
 C_GT_ONLY, C_NEITHER) = range(16)


def passes(shared, area, fraction):
    """shared >= 1 and (double)shared >= fraction * (double)area - one IEEE multiply, one compare."""
    fraction = np.float64(fraction)
    assert 0.0 <= fraction <= 1.0
    return (shared >= 1) & (shared.astype(np.float64) >= fraction * area.astype(np.float64))


def tables(frame, mask, threshold, connectivity=8, min_area=1, gt_fraction=0.0, pred_fraction=0.0):
    """One frame [h, w] and its bool mask -> (gt uint32 [Kg, 4], pred uint32 [Kp, 4], P bool [h, w], all predicted regions [K, 12]):
    every mask region and every KEPT predicted region in ascending root order, and the pixels of the kept predictions."""
    frame = np.ascontiguousarray(frame, np.float32)
    mask = np.asarray(mask, bool)
    assert frame.shape == mask.shape and min_area >= 1 and connectivity in (4, 8)
    npix = frame.size
    rec, plabels = regions_ref.regions(frame, threshold, connectivity)
    kept = rec[rec[:, regions_ref.AREA] >= min_area]
    is_kept = np.zeros(npix + 1, bool)
    is_kept[kept[:, regions_ref.ROOT].astype(np.int64) + 1] = True
    P = is_kept[plabels]                                                       # label 0 is never kept
    glabels, gsizes = pro_ref.label(mask, connectivity)
    groots = np.flatnonzero(gsizes.reshape(-1))                                # ascending
    both = P & mask
    hit = np.bincount(glabels[both].astype(np.int64) - 1, minlength=npix)[groots]
    overlap = np.bincount(plabels[both].astype(np.int64) - 1, minlength=npix)[kept[:, regions_ref.ROOT].astype(np.int64)]
    gt = np.zeros((len(groots), WORDS), np.uint32)
    gt[:, ROOT], gt[:, AREA], gt[:, SHARED] = groots, gsizes.reshape(-1)[groots], hit
    gt[:, FLAGS] = passes(gt[:, SHARED], gt[:, AREA], gt_fraction)
    pred = np.zeros((len(kept), WORDS), np.uint32)
    pred[:, ROOT], pred[:, AREA], pred[:, SHARED] = kept[:, regions_ref.ROOT], kept[:, regions_ref.AREA], overlap
    pred[:, FLAGS] = passes(pred[:, SHARED], pred[:, AREA], pred_fraction)
    return gt, pred, P, rec


def match(frame, mask, threshold, connectivity=8, min_area=1, gt_fraction=0.0, pred_fraction=0.0, max_regions=64):
    """One frame -> (gt_records uint32 [max_regions, 4], pred_records uint32 [max_regions, 4], counts uint64 [16])."""
    assert 1 <= max_regions <= 65536
    gt, pred, P, rec = tables(frame, mask, threshold, connectivity, min_area, gt_fraction, pred_fraction)
    mask = np.asarray(mask, bool)
    out_g, out_p = np.zeros((max_regions, WORDS), np.uint32), np.zeros((max_regions, WORDS), np.uint32)
    out_g[:min(len(gt), max_regions)] = gt[:max_regions]
    out_p[:min(len(pred), max_regions)] = pred[:max_regions]
    c = np.zeros(COUNTS, np.uint64)
    c[GT_REGIONS], c[GT_DETECTED] = len(gt), int(gt[:, FLAGS].sum())
    c[PRED_REGIONS], c[PRED_MATCHED] = len(pred), int(pred[:, FLAGS].sum())
    c[FALSE_ALARMS], c[PRED_DROPPED] = len(pred) - int(pred[:, FLAGS].sum()), len(rec) - len(pred)
    c[TP], c[FP], c[FN], c[TN] = int((P & mask).sum()), int((P & ~mask).sum()), int((~P & mask).sum()), int((~P & ~mask).sum())
    c[NAN_PIXELS], c[GT_PIXELS] = int(np.isnan(np.asarray(frame, np.float32)).sum()), int(mask.sum())
    c[C_BOTH + (0 if len(gt) and len(pred) else 1 if len(pred) else 2 if len(gt) else 3)] = 1
    return out_g, out_p, c


def match_batch(maps, masks, threshold, connectivity=8, min_area=1, gt_fraction=0.0, pred_fraction=0.0, max_regions=64):
    """maps float32 [n, h, w], masks bool [n, h, w], every frame on its own -> (gt_records uint32 [n, max_regions, 4], pred_records
    uint32 [n, max_regions, 4], counts uint64 [n, 16])."""
    maps = np.asarray(maps, np.float32)
    masks = np.asarray(masks, bool)
    assert maps.ndim == 3 and maps.shape == masks.shape
    out = [match(f, m, threshold, connectivity, min_area, gt_fraction, pred_fraction, max_regions) for f, m in zip(maps, masks)]
    if not out:
        return np.zeros((0, max_regions, WORDS), np.uint32), np.zeros((0, max_regions, WORDS), np.uint32), np.zeros((0, COUNTS), np.uint64)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])

