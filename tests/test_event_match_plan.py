"""The host half of the matched-event tables (csrc/map_event_match.hip, metrics.match_events, metrics.EventCounts) on a machine
without a GPU: the numpy restatement (tests/event_match_ref.py) against scipy.ndimage - the 3-D label numbering of both volumes under
the three structures, sum_labels both ways, the first and last shared frame per label -, the cases by hand with their words written
out, the workspace size against its documented formula, the launch plan, every refusal the host makes before it launches anything,
and the arithmetic of the report."""
import importlib
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import event_match_ref as ref
import events_ref
import regions_ref

metrics = importlib.import_module("video-anomaly-detection_amd.metrics")
scoring = importlib.import_module("video-anomaly-detection_amd.scoring")
hip = importlib.import_module("video-anomaly-detection_amd.hip")
REPO = Path(__file__).resolve().parent.parent

MODES = ((4, 1), (8, 1), (8, 9))
SHAPES = ((4, 9, 11), (1, 7, 9), (3, 1, 13), (3, 13, 1), (1, 1, 1))
NONE = ref.NONE


@pytest.mark.parametrize("mode", MODES, ids=[f"c{c}t{t}" for c, t in MODES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_restatement_against_scipy(shape, mode):
    ndimage = pytest.importorskip("scipy.ndimage")
    connectivity, temporal = mode
    structure = events_ref.structure(connectivity, temporal)
    rng = np.random.default_rng(270 + sum(shape) + connectivity + temporal)
    t, h, w = shape
    thr = np.float32(0.5)
    frames = np.broadcast_to(np.arange(t)[:, None, None], shape)
    for density, min_duration, min_volume in ((0.25, 1, 1), (0.4, 2, 1), (0.55, 1, 3), (0.8, 2, 2)):
        fg = rng.random(shape) < density
        mask = rng.random(shape) < density
        vol = regions_ref.map_from_mask(rng, fg.reshape(t * h, w), thr).reshape(shape)
        for gt_fraction, pred_fraction in ((0.0, 0.0), (0.5, 0.25), (1.0, 1.0)):
            gt, pred, P, dropped = ref.tables(vol, mask, thr, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction)
            plab, pcount = ndimage.label(fg, structure=structure)
            glab, gcount = ndimage.label(mask, structure=structure)
            assert len(gt) == gcount and len(pred) + dropped == pcount
            # the kept events, by scipy: numbered in raster order of their first voxel, filtered by volume and duration
            pindex = np.arange(1, pcount + 1)
            volumes = ndimage.sum_labels(np.ones_like(plab), plab, pindex).astype(np.int64) if pcount else np.zeros(0, np.int64)
            durations = np.array([sl[0].stop - sl[0].start for sl in ndimage.find_objects(plab)], np.int64)
            keep = (volumes >= min_volume) & (durations >= min_duration) if pcount else np.zeros(0, bool)
            kept_ids = pindex[keep]
            want_P = np.isin(plab, kept_ids)
            assert np.array_equal(P, want_P)
            assert np.array_equal(plab.reshape(-1)[pred[:, ref.ROOT].astype(np.int64)], kept_ids)
            gindex = np.arange(1, gcount + 1)
            assert np.array_equal(glab.reshape(-1)[gt[:, ref.ROOT].astype(np.int64)], gindex)
            for table, lab, index, other in ((gt, glab, gindex, want_P), (pred, plab, kept_ids, mask)):
                if not len(index):
                    continue
                assert np.array_equal(table[:, ref.VOLUME], ndimage.sum_labels(np.ones_like(lab), lab, index).astype(np.int64))
                shared = ndimage.sum_labels(other, lab, index).astype(np.int64)
                assert np.array_equal(table[:, ref.SHARED], shared)
                objects = ndimage.find_objects(lab)
                assert [[objects[k - 1][0].start, objects[k - 1][0].stop - 1] for k in index] == table[:, ref.T0:ref.T1 + 1].tolist()
                # the first and last frame of a shared voxel: minimum / maximum of the frame index under label and the other volume
                both = np.where(other, lab, 0)
                first = ndimage.minimum(frames, both, index).astype(np.int64)
                last = ndimage.maximum(frames, both, index).astype(np.int64)
                assert np.array_equal(table[:, ref.FIRST], np.where(shared > 0, first, NONE))
                assert np.array_equal(table[:, ref.LAST], np.where(shared > 0, last, NONE))
                # a root is its component's first voxel
                for r in table:
                    assert r[ref.ROOT] == np.flatnonzero(lab.reshape(-1) == lab.reshape(-1)[r[ref.ROOT]])[0]
            for table, fraction in ((gt, gt_fraction), (pred, pred_fraction)):
                assert table[:, ref.FLAGS].tolist() == [int(s >= 1 and float(s) >= fraction * float(v)) for v, s in table[:, [ref.VOLUME, ref.SHARED]].tolist()]
            for max_events in (64, 1):
                out_g, out_p, c, f = ref.match(vol, mask, thr, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction, max_events)
                ng, np_ = min(len(gt), max_events), min(len(pred), max_events)
                assert np.array_equal(out_g[:ng], gt[:ng]) and not out_g[ng:].any() and np.array_equal(out_p[:np_], pred[:np_]) and not out_p[np_:].any()
                det = gt[:, ref.FLAGS] == 1
                detected, matched = int(det.sum()), int(pred[:, ref.FLAGS].sum())
                delays = gt[det, ref.FIRST].astype(np.int64) - gt[det, ref.T0]
                in_p, in_g = want_P.reshape(t, -1).any(1), mask.reshape(t, -1).any(1)
                assert c.dtype == np.uint64 and c.tolist() == [
                    gcount, detected, len(kept_ids), matched, len(kept_ids) - matched, pcount - len(kept_ids),
                    int((want_P & mask).sum()), int((want_P & ~mask).sum()), int((~want_P & mask).sum()), int((~want_P & ~mask).sum()), 0, int(mask.sum()),
                    int(delays.sum()), int((delays == 0).sum()),
                    int((in_p & in_g).sum()), int((in_p & ~in_g).sum()), int((~in_p & in_g).sum()), int((~in_p & ~in_g).sum()),
                    int(gcount > 0 and len(kept_ids) > 0), int(gcount == 0 and len(kept_ids) > 0), int(gcount > 0 and len(kept_ids) == 0),
                    int(gcount == 0 and len(kept_ids) == 0)]
                assert c[ref.TP:ref.TN + 1].sum() == t * h * w and gt[:, ref.SHARED].sum() == pred[:, ref.SHARED].sum() == c[ref.TP]
                assert f.dtype == np.uint32 and np.array_equal(f[:, :3].sum(0), c[ref.TP:ref.FN + 1]) and not f[:, 3].any()
                # the kept-voxel word of the event table's restatement
                kept_word = events_ref.detect(vol, thr, connectivity, temporal, min_duration, min_volume, 4)[2][:, 1]
                assert np.array_equal(f[:, 0] + f[:, 1], kept_word)
                r = metrics.event_report_from_counts(c)
                for key, num, den in (("voxel_iou", int((want_P & mask).sum()), int((want_P | mask).sum())), ("track_recall", detected, gcount),
                                      ("event_precision", matched, len(kept_ids)), ("mean_delay", int(delays.sum()), detected)):
                    assert r[key] == num / den if den else math.isnan(r[key]), key
                assert r["gt_tracks"] == gcount and r["frames"] == t and r["clips"] == 1


def test_one_frame_is_the_region_match():
    """T = 1: words 0-1, 4 and 7 of both tables and the counters they share are those of tests/match_ref.py."""
    import match_ref
    rng = np.random.default_rng(271)
    thr = np.float32(0.5)
    for connectivity in (4, 8):
        fg, mask = rng.random((23, 31)) < 0.45, rng.random((23, 31)) < 0.45
        frame = regions_ref.map_from_mask(rng, fg, thr)
        g2, p2, c2 = match_ref.match(frame, mask, thr, connectivity, 2, 0.5, 0.25, 64)
        g3, p3, c3, f3 = ref.match(frame[None], mask[None], thr, connectivity, 1, 1, 2, 0.5, 0.25, 64)
        assert np.array_equal(g3[:, [0, 1, 4, 7]], g2) and np.array_equal(p3[:, [0, 1, 4, 7]], p2)
        assert np.array_equal(c3[:12], c2[:12]) and np.array_equal(c3[18:], c2[12:]) and np.array_equal(c3[14:18], c2[12:])
        assert f3.tolist() == [[int(c2[6]), int(c2[7]), int(c2[8]), 0]]


#: name -> (gt records in use, pred records in use, counts), per clip; tables of four records (three for "truncation")
BY_HAND = {
    "hit_in_the_last_frame": [([[42, 48, 0, 3, 4, 3, 3, 1]], [[784, 10, 3, 3, 4, 3, 3, 1]],
                               [1, 1, 1, 1, 0, 0, 4, 6, 44, 1146, 0, 48, 3, 0, 1, 0, 3, 1, 1, 0, 0, 0])],
    "hit_by_a_dropped_event": [([[282, 36, 1, 3, 0, NONE, NONE, 0]], [],
                                [1, 0, 0, 0, 0, 1, 0, 0, 36, 1164, 0, 36, 0, 0, 0, 0, 3, 2, 0, 0, 1, 0])],
    "one_event_over_two_tracks": [([[282, 12, 1, 2, 3, 2, 2, 1], [290, 12, 1, 2, 3, 2, 2, 1]], [[541, 14, 2, 2, 6, 2, 2, 1]],
                                   [2, 2, 1, 1, 0, 0, 6, 8, 18, 1168, 0, 24, 2, 0, 1, 0, 1, 3, 1, 0, 0, 0])],
    "two_events_on_one_track": [([[102, 240, 0, 4, 9, 1, 4, 1]], [[363, 3, 1, 1, 3, 1, 1, 1], [852, 6, 3, 4, 6, 3, 4, 1]],
                                 [1, 1, 2, 2, 0, 0, 9, 0, 231, 960, 0, 240, 1, 0, 3, 0, 2, 0, 1, 0, 0, 0])],
    "merge_and_split": [([[42, 126, 0, 4, 8, 0, 4, 1]], [[63, 4, 0, 1, 4, 0, 1, 1], [793, 4, 3, 4, 4, 3, 4, 1]],
                         [1, 1, 2, 2, 0, 0, 8, 0, 118, 1074, 0, 126, 0, 1, 4, 0, 1, 0, 1, 0, 0, 0])],
    "consecutive_frames_only": [([[324, 15, 1, 1, 0, NONE, NONE, 0]], [[564, 15, 2, 2, 0, NONE, NONE, 0]],
                                 [1, 0, 1, 0, 1, 0, 0, 15, 15, 1170, 0, 15, 0, 0, 0, 1, 1, 3, 1, 0, 0, 0])],
    "diagonal_touch": [([[522, 4, 2, 2, 0, NONE, NONE, 0]], [[564, 4, 2, 2, 0, NONE, NONE, 0]],
                        [1, 0, 1, 0, 1, 0, 0, 4, 4, 1192, 0, 4, 0, 0, 1, 0, 0, 4, 1, 0, 0, 0])],
    "clips_never_link": [([], [[1023, 15, 4, 4, 0, NONE, NONE, 0]], [0, 0, 1, 0, 1, 0, 0, 15, 0, 1185, 0, 0, 0, 0, 0, 1, 0, 4, 0, 1, 0, 0]),
                         ([[63, 15, 0, 0, 0, NONE, NONE, 0]], [], [1, 0, 0, 0, 0, 0, 0, 0, 15, 1185, 0, 15, 0, 0, 0, 0, 1, 4, 0, 0, 1, 0])],
    "nan_inside_a_track": [([[282, 48, 1, 2, 47, 1, 2, 1]], [[282, 47, 1, 2, 47, 1, 2, 1]],
                            [1, 1, 1, 1, 0, 0, 47, 0, 1, 1152, 1, 48, 0, 1, 2, 0, 0, 3, 1, 0, 0, 0])],
    "fraction_boundary_passes": [([[282, 60, 1, 1, 15, 1, 1, 1]], [[242, 60, 1, 1, 15, 1, 1, 1]],
                                  [1, 1, 1, 1, 0, 0, 15, 45, 45, 1095, 0, 60, 0, 1, 1, 0, 0, 4, 1, 0, 0, 0])],
    "fraction_boundary_fails": [([[282, 60, 1, 1, 14, 1, 1, 0]], [[242, 60, 1, 1, 14, 1, 1, 0]],
                                 [1, 0, 1, 0, 1, 0, 14, 46, 46, 1094, 0, 60, 0, 0, 1, 0, 0, 4, 1, 0, 0, 0])],
    "truncation": [([[21, 4, 0, 0, 1, 0, 0, 1], [264, 4, 1, 1, 1, 1, 1, 1], [507, 4, 2, 2, 1, 2, 2, 1]],
                    [[42, 4, 0, 0, 1, 0, 0, 1], [285, 4, 1, 1, 1, 1, 1, 1], [528, 4, 2, 2, 1, 2, 2, 1]],
                    [5, 4, 4, 4, 0, 0, 4, 12, 16, 1168, 0, 20, 0, 4, 4, 0, 1, 0, 1, 0, 0, 0])],
}


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_on_the_cases_by_hand(name):
    maps, masks, kw = ref.case(name)
    assert maps.shape[1:] == ref.SHAPE and set(BY_HAND) == set(ref.CASES)
    g, p, c, f = ref.match_batch(maps, masks, ref.T, **{"max_events": 4, **kw})
    assert len(BY_HAND[name]) == len(maps)
    for clip, (want_g, want_p, want_c) in enumerate(BY_HAND[name]):
        assert g[clip, :len(want_g)].tolist() == want_g and not g[clip, len(want_g):].any()
        assert p[clip, :len(want_p)].tolist() == want_p and not p[clip, len(want_p):].any()
        assert c[clip].tolist() == want_c
        assert np.array_equal(f[clip, :, :3].sum(0), c[clip, ref.TP:ref.FN + 1]) and int(f[clip, :, 3].sum()) == want_c[ref.NAN_VOXELS]
    named = dict(zip(metrics.EVENT_COUNT_NAMES, c[0].tolist()))
    if name == "hit_in_the_last_frame":                                         # delay = duration - 1
        assert named["delay_sum"] == 3 and named["immediate_tracks"] == 0 and metrics.event_report_from_counts(c[0])["mean_delay"] == 3.0
    if name == "hit_by_a_dropped_event":
        assert named["pred_dropped"] == 1 and named["voxel_fn"] == named["gt_voxels"] == 36 and named["clips_gt_only"] == 1
    if name == "truncation":                                                    # the full counters stand behind tables of three
        assert named["gt_tracks"] == 5 and named["pred_events"] == 4 and g.shape[1] == 3


def test_workspace_bytes_and_the_plan_without_a_gpu():
    lib = hip.lib()
    assert hip.EVMATCH_WORDS == 8 and hip.EVMATCH_COUNTS == 22 and metrics.EVMATCH_WORDS == 8 and metrics.EVMATCH_COUNTS == 22
    assert len(metrics.EVENT_COUNT_NAMES) == 22 == ref.COUNTS and ref.WORDS == 8
    # 16 for the flag words, 4 per chunk of 1024 voxels of a clip for the events and again for the tracks (each padded to 16), 48 a voxel
    vol = 16 * 256 * 256
    assert lib.vad_event_match_workspace_bytes(32, 16, 256, 256) == 16 + 2 * 4 * 32 * 1024 + 48 * 32 * vol
    assert lib.vad_event_match_workspace_bytes(1, 3, 37, 53) == 16 + 2 * 32 + 48 * 3 * 37 * 53             # six chunks: 24 bytes, padded to 32
    assert lib.vad_event_match_workspace_bytes(3, 1, 1, 1) == 16 + 2 * 16 + 48 * 3
    assert lib.vad_event_match_workspace_bytes(0, 4, 4, 4) == 16
    for b, t, h, w in ((1, 5, 12, 20), (7, 3, 33, 65), (5, 2, 40, 70), (2, 17, 256, 256)):
        chunks = b * ((t * h * w + 1023) // 1024)
        assert lib.vad_event_match_workspace_bytes(b, t, h, w) == 16 + 2 * ((4 * chunks + 15) // 16 * 16) + 48 * b * t * h * w
    for b, t, h, w in ((-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 1, 46341, 46341), (1, 32768, 256, 256), (1 << 20, 16, 256, 256)):
        assert lib.vad_event_match_workspace_bytes(b, t, h, w) == 0, (b, t, h, w)
    assert lib.vad_event_match_workspace_bytes(1, 32767, 256, 256) > 0                                     # t * h * w = 2^31 - 65536
    out = [hip.C.c_int(0) for _ in range(5)]
    assert lib.vad_event_match_plan(*[hip.C.byref(v) for v in out]) == 0
    label_round, volume_round, scan_round, join_round, threads = (v.value for v in out)
    assert label_round == 4096 * 256 and threads == 256 and join_round % 4096 == 0 and scan_round % 1024 == 0
    # 17 frames of 256 x 256 are more than one grid round of every pass over a volume (tests/test_hip_event_match.py)
    assert max(volume_round, scan_round, join_round) < 17 * 256 * 256 and min(volume_round, scan_round, join_round) >= 256 * 256
    events_plan = [hip.C.c_int(0) for _ in range(5)]
    assert lib.vad_events_plan(*[hip.C.byref(v) for v in events_plan]) == 0
    assert [v.value for v in events_plan[:3]] == [label_round, volume_round, scan_round]                   # the one copy of the volume labelling
    assert lib.vad_event_match_plan(None, None, None, None, None) == -1 and b"NULL" in lib.vad_last_error()


def test_refusals_by_name_without_a_gpu():
    """Every argument check runs on the host, before any device call: the addresses are never read."""
    lib = hip.lib()
    fake = 1 << 20
    need = lib.vad_event_match_workspace_bytes(2, 3, 8, 8)
    #     0     1     2  3  4  5  6  7    8  9  10 11 12   13   14  15    16    17    18    19    20    21
    a = (fake, fake, 0, 2, 3, 8, 8, 0.5, 8, 9, 1, 1, 0.0, 0.0, 64, fake, fake, fake, fake, fake, need, None)
    nan = float("nan")
    for pos, bad, word in ((0, None, b"maps is NULL"), (0, fake + 2, b"maps must be 4-byte"), (1, None, b"masks is NULL"), (2, 2, b"mask_format"),
                           (2, 3, b"mask_format"), (2, -1, b"mask_format"), (3, -1, b"b must"), (4, 0, b"t must"), (4, -3, b"t must"),
                           (5, 0, b"h and w"), (6, 0, b"h and w"), (5, -5, b"h and w"), (7, nan, b"threshold is NaN"),
                           (8, 6, b"connectivity"), (8, 0, b"connectivity"), (9, 0, b"temporal must"), (9, 3, b"temporal must"),
                           (9, 27, b"temporal must"), (10, 0, b"min_duration"), (11, 0, b"min_volume"),
                           (12, nan, b"gt_fraction"), (12, -0.01, b"gt_fraction"), (12, 1.0000001, b"gt_fraction"), (12, float("inf"), b"gt_fraction"),
                           (13, nan, b"pred_fraction"), (13, -1.0, b"pred_fraction"), (13, 2.0, b"pred_fraction"),
                           (14, 0, b"max_events"), (14, 65537, b"max_events"), (14, -1, b"max_events"),
                           (15, None, b"gt_records is NULL"), (15, fake + 8, b"gt_records must be 16-byte"), (16, None, b"pred_records is NULL"),
                           (16, fake + 4, b"pred_records must be 16-byte"), (17, None, b"counts is NULL"), (17, fake + 4, b"counts must be 8-byte"),
                           (18, None, b"frame_counts is NULL"), (18, fake + 2, b"frame_counts must be 4-byte"),
                           (19, None, b"ws is NULL"), (19, fake + 8, b"ws must be 16-byte")):
        args = list(a)
        args[pos] = bad
        assert lib.vad_match_events(*args) == -1 and b"match_events: " in lib.vad_last_error() and word in lib.vad_last_error(), (pos, bad, lib.vad_last_error())
    args = list(a)
    args[1], args[2] = fake + 2, 1
    assert lib.vad_match_events(*args) == -1 and b"float masks must be 4-byte" in lib.vad_last_error()
    args = list(a)
    args[8] = 4                                                               # temporal 9 with connectivity 4
    assert lib.vad_match_events(*args) == -1 and b"temporal 9 needs connectivity 8" in lib.vad_last_error()
    for dims, word in (((1, 1, 65536, 32768), b"2^31 - 1"), ((1, 32768, 256, 256), b"2^31 - 1"), ((1 << 20, 16, 256, 256), b"2^38")):
        args = list(a)
        args[3:7] = dims
        assert lib.vad_match_events(*args) == -1 and word in lib.vad_last_error(), dims
    args = list(a)
    args[20] = need - 1
    assert lib.vad_match_events(*args) == -3 and b"ws_bytes" in lib.vad_last_error()                   # VAD_ERR_WS
    assert b"vad_event_match_workspace_bytes(2, 3, 8, 8)" in lib.vad_last_error()


def test_python_refusals_without_a_gpu():
    maps, masks = torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    VadError = hip.VadError
    with pytest.raises(VadError, match="no CPU fallback"):
        metrics.match_events(maps, masks, 0.5)
    with pytest.raises(VadError, match="torch tensors"):
        metrics.match_events(maps.numpy(), masks, 0.5)
    with pytest.raises(VadError, match="torch tensors"):
        metrics.match_events(maps, masks.numpy(), 0.5)
    for bad_maps, bad_masks, word in ((maps.double(), masks, "float32"), (maps, masks.to(torch.complex64), "masks must be"),
                                      (maps, masks[:1], "do not match"), (maps, torch.zeros(2, 3, 8, 4, dtype=torch.uint8), "do not match"),
                                      (maps, torch.zeros(2, 3, 4, 16, dtype=torch.uint8), "do not match"), (maps, torch.zeros(3, 2, 8, 8), "do not match"),
                                      (maps[0, 0], masks[0, 0], "maps must be"), (maps[:, :, None, None], masks, "maps must be")):
        with pytest.raises(VadError, match=word):
            metrics.match_events(bad_maps, bad_masks, 0.5)
    for kw, word in (({"threshold": float("nan")}, "threshold"), ({"threshold": None}, "threshold"), ({"threshold": True}, "threshold"),
                     ({"threshold": 0.5, "gt_fraction": -0.1}, "gt_fraction"), ({"threshold": 0.5, "gt_fraction": float("nan")}, "gt_fraction"),
                     ({"threshold": 0.5, "pred_fraction": 1.01}, "pred_fraction"), ({"threshold": 0.5, "pred_fraction": "0.5"}, "pred_fraction"),
                     ({"threshold": 0.5, "min_duration": 0}, "min_duration"), ({"threshold": 0.5, "min_volume": 1.5}, "min_volume"),
                     ({"threshold": 0.5, "max_events": 0}, "max_events"), ({"threshold": 0.5, "max_events": 65537}, "max_events"),
                     ({"threshold": 0.5, "connectivity": 6}, "connectivity"), ({"threshold": 0.5, "temporal": 3}, "temporal must be 1 or 9"),
                     ({"threshold": 0.5, "connectivity": 4}, "needs connectivity=8")):
        with pytest.raises(VadError, match=word):
            metrics.match_events(maps, masks, **kw)
    # event_report refuses its arguments before it touches the model or the loader
    for kw, exc, word in (({"map": "psnr"}, VadError, "map"), ({"gt_fraction": 2.0}, VadError, "gt_fraction"), ({"min_duration": 0}, VadError, "min_duration"),
                          ({"connectivity": 5}, VadError, "connectivity"), ({"temporal": 2}, VadError, "temporal"),
                          ({"counts": object()}, VadError, "EventCounts"), ({"counts": metrics.DetectionCounts("cpu")}, VadError, "EventCounts"),
                          ({"morph": [("blur", 3)]}, VadError, "morph"), ({"temporal_filter": ("median", 3)}, VadError, "temporal")):
        with pytest.raises(exc, match=word):
            scoring.event_report(None, None, "cpu", **{"threshold": 0.5, **kw})
    with pytest.raises(VadError, match="threshold"):
        scoring.event_report(None, None, "cpu", float("nan"))
    # clips on another map than the error map, and a temporal filter on an image batch, are refused before the model is touched
    with pytest.raises(VadError, match="error map only"):
        scoring.event_report(None, [{"frames": torch.zeros(1, 2, 3, 16, 16), "mask": torch.zeros(1, 2, 1, 16, 16)}], "cpu", 0.5, map="ssim")
    with pytest.raises(VadError, match="not consecutive"):
        scoring.event_report(None, [{"image": torch.zeros(2, 3, 16, 16), "mask": torch.zeros(2, 1, 16, 16)}], "cpu", 0.5, temporal_filter=("min", 2))


def test_report_arithmetic_and_nan_ratios():
    #       trk det pred match fa drop  tp   fp   fn    tn nan |G| delay imm  fb fp fg fn  cb cp cg cn
    sums = [10, 6, 8, 4, 4, 3, 300, 100, 200, 9400, 7, 500, 9, 2, 5, 2, 3, 10, 3, 1, 2, 4]
    r = metrics.event_report_from_counts(np.array(sums, np.int64))
    assert [r[n] for n in metrics.EVENT_COUNT_NAMES] == sums and r["frames"] == 20 and r["clips"] == 10
    assert r["track_recall"] == 6 / 10 and r["event_precision"] == 4 / 8 and r["event_f1"] == 2 * 0.5 * 0.6 / (0.5 + 0.6)
    assert r["false_alarm_events_per_frame"] == 4 / 20 and r["false_alarm_events_per_clip"] == 4 / 10
    assert r["voxel_precision"] == 300 / 400 and r["voxel_recall"] == 300 / 500 and r["voxel_iou"] == 300 / 600 and r["voxel_dice"] == 600 / 900
    assert r["mean_delay"] == 9 / 6 and r["immediate"] == 2 / 6
    assert r["frame_precision"] == 5 / 7 and r["frame_recall"] == 5 / 8 and r["frame_f1"] == 10 / 15
    assert r["clip_precision"] == 3 / 4 and r["clip_recall"] == 3 / 5 and r["clip_f1"] == 6 / 9
    # a denominator of 0 is nan, never 0 or 1
    empty = metrics.event_report_from_counts(np.zeros(22, np.int64))
    ratios = [k for k in empty if k not in metrics.EVENT_COUNT_NAMES and k not in ("frames", "clips")]
    assert len(ratios) == 17 and all(math.isnan(empty[k]) for k in ratios) and empty["frames"] == 0 and empty["clips"] == 0
    missed = metrics.event_report_from_counts([2, 0, 0, 0, 0, 1, 0, 0, 9, 247, 0, 9, 0, 0, 0, 0, 3, 1, 0, 0, 1, 0])   # two tracks, nothing kept
    assert missed["track_recall"] == 0.0 and math.isnan(missed["event_precision"]) and math.isnan(missed["event_f1"])
    assert math.isnan(missed["mean_delay"]) and math.isnan(missed["immediate"]) and missed["frame_recall"] == 0.0 and math.isnan(missed["frame_precision"])
    assert missed["clip_recall"] == 0.0 and missed["false_alarm_events_per_clip"] == 0.0
    for bad in (np.zeros(21, np.int64), np.zeros(16, np.int64), [-1] + [0] * 21):
        with pytest.raises(hip.VadError, match="counts must be"):
            metrics.event_report_from_counts(bad)


def test_event_counts_on_the_host():
    p = {"threshold": 0.5, "connectivity": 8, "temporal": 9, "min_duration": 2, "min_volume": 1, "gt_fraction": 0.0, "pred_fraction": 0.0}
    assert metrics._event_match_params("x", 0.5, 8, 9, 2, 1, 0.0, 0.0) == p
    a, b = metrics.EventCounts("cpu", p), metrics.EventCounts("cpu", p)
    a.counts += torch.arange(22)
    b.counts += 2
    assert a.merge(b).counts.tolist() == [v + 2 for v in range(22)] and a.all_reduce() == 1
    fresh = metrics.EventCounts("cpu").merge(a)                                  # no operating point yet: it adopts the other's
    assert fresh.params == p and fresh.report()["params"] == p and fresh.report()["gt_tracks"] == 2
    for key, other in (("threshold", 0.25), ("min_duration", 1), ("min_volume", 2), ("connectivity", 4), ("temporal", 1), ("gt_fraction", 0.5),
                       ("pred_fraction", 0.5)):
        with pytest.raises(ValueError, match="gathered with"):
            a.merge(metrics.EventCounts("cpu", {**p, key: other}))
    assert a.counts.tolist() == [v + 2 for v in range(22)]                       # a refused merge adds nothing
    with pytest.raises(hip.VadError, match="EventMatches"):
        a.update(object())
    with pytest.raises(hip.VadError, match="EventCounts"):
        a.merge(metrics.DetectionCounts("cpu"))
    m = metrics.EventMatches(torch.zeros(2, 3, 8, dtype=torch.int32), torch.zeros(2, 3, 8, dtype=torch.int32), torch.ones(2, 22, dtype=torch.int64),
                             torch.zeros(2, 4, 4, dtype=torch.int32), (4, 8, 8), p)
    m.gt_records[0, 0] = torch.tensor([70, 8, 1, 3, 4, 2, 3, 1], dtype=torch.int32)
    m.gt_records[0, 1] = torch.tensor([90, 5, 1, 1, 0, -1, -1, 0], dtype=torch.int32)
    m.counts[0, 0] = 2
    m.frame_counts[1, 2] = torch.tensor([0, 3, 0, 0], dtype=torch.int32)
    a = metrics.EventCounts("cpu")
    assert a.update(m, {"map": "mse"}).counts.tolist() == [3] + [2] * 21 and a.params == {**p, "map": "mse"}
    assert m.gt_volume[0, 0] == 8 and m.gt_hit[0, 0] == 4 and m.detected()[0].tolist() == [True, False, False] and not m.matched().any()
    assert m.delays()[0].tolist() == [1, -1, -1] and m.pred_volume.shape == m.pred_overlap.shape == (2, 3) and m.truncated().tolist() == [False, False]
    assert m.alarms().tolist() == [[False] * 4, [False, False, True, False]]
    rows = m.to_list()
    assert rows[0]["gt"] == [{"root": 70, "volume": 8, "t0": 1, "t1": 3, "hit": 4, "first_hit": 2, "last_hit": 3, "detected": True, "delay": 1},
                             {"root": 90, "volume": 5, "t0": 1, "t1": 1, "hit": 0, "first_hit": None, "last_hit": None, "detected": False, "delay": None}]
    assert rows[1]["counts"]["voxel_tp"] == 1 and len(rows[1]["pred"]) == 1
    with pytest.raises(ValueError, match="gathered with"):
        a.update(metrics.EventMatches(m.gt_records, m.pred_records, m.counts, m.frame_counts, (4, 8, 8), {**p, "min_duration": 3}), {"map": "mse"})


def test_header_and_signatures_agree():
    header = (REPO / "include" / "vad_hip.h").read_text()
    lib = hip.lib()
    for name in ("vad_event_match_workspace_bytes", "vad_event_match_plan", "vad_match_events"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+VAD_EVMATCH_WORDS\s+8\b", header) and re.search(r"#define\s+VAD_EVMATCH_COUNTS\s+22\b", header)
    bare = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("vad_match_events", 22), ("vad_event_match_workspace_bytes", 4), ("vad_event_match_plan", 5)):
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert len(hip.SIGNATURES[name][1]) == len(decl.split(",")) == count, name
    assert hip.SIGNATURES["vad_match_events"][1][12:14] == [hip.C.c_double, hip.C.c_double]
    assert "map_event_match.hip" in hip.SOURCES and (hip.CSRC / "map_event_match.hip").exists()
    # the volume labelling is one copy: both files launch the passes of event_volume.h, neither holds a link or flatten kernel
    shared = (hip.CSRC / "event_volume.h").read_text()
    for kernel in ("events_rebase_kernel", "events_link_kernel", "events_flatten_kernel", "events_count_kernel"):
        assert shared.count("void %s(" % kernel) == 1
    for name in ("map_events.hip", "map_event_match.hip"):
        source = (hip.CSRC / name).read_text()
        assert '#include "event_volume.h"' in source and "events_volume_launch" in source and "vad_label_launch" in source
        assert "label_union" not in source and "label_find" not in source
