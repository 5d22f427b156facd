"""The host half of the per-frame tracks (csrc/map_event_tracks.hip, metrics.event_tracks, EventTracker.update(boxes=True)) on a
machine without a GPU: the numpy restatement (tests/event_tracks_ref.py) against the event records it refines - the defining
equalities of DESIGN.md section 4.24 -, against scipy.ndimage, live mode against clip mode on every prefix, the launch plan, and
every refusal the host makes before it launches anything."""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import event_tracks_ref as ref
import events_ref
import regions_ref
import track_ref

metrics = importlib.import_module("video-anomaly-detection_amd.metrics")
scoring = importlib.import_module("video-anomaly-detection_amd.scoring")
hip = importlib.import_module("video-anomaly-detection_amd.hip")
REPO = Path(__file__).resolve().parent.parent

MODES = ((4, 1), (8, 1), (8, 9))
MODE_IDS = [f"c{c}t{t}" for c, t in MODES]
BIG = 4096


def _volume(rng, shape, density):
    """Distinct values, so that peaks have no ties; foreground = the `density` largest share."""
    n = int(np.prod(shape))
    vol = rng.permutation(np.linspace(-1.0, 1.0, n, dtype=np.float32)).reshape(shape)
    thr = np.sort(vol.reshape(-1))[min(n - 1, int((1.0 - density) * n))]
    return vol, thr


def check_invariants(tracks, records, counts, frame_counts, shape):
    """What ties a clip's tracks to its event records: per kept event inside the table the areas sum to the volume, the boxes unite
    to the box, the largest peak is the peak (at the peak's index), the sums add up, sum f * area = sum_t, and the frames with pixels
    are exactly t0 .. t1; behind the kept events everything is zero; without truncation the areas of a frame sum to its kept pixels."""
    t, h, w = shape
    kept = min(int(counts[0]), len(records))
    assert not tracks[kept:].any()
    sx, sy = ref.sums(tracks)
    ex, ey, et = events_ref.sums(records)
    for e in range(kept):
        r, tr = records[e], tracks[e]
        area = tr[:, ref.AREA].astype(np.int64)
        present = np.flatnonzero(area)
        assert area.sum() == r[events_ref.VOLUME] and present.tolist() == list(range(int(r[events_ref.T0]), int(r[events_ref.T1]) + 1))
        assert not tr[area == 0].any()
        on = tr[present]
        assert (on[:, ref.X0].min(), on[:, ref.Y0].min(), on[:, ref.X1].max(), on[:, ref.Y1].max()) == tuple(r[events_ref.X0:events_ref.Y1 + 1])
        keys = regions_ref.order_key(on[:, ref.PEAK].copy().view(np.float32)).astype(np.int64)
        f = int(present[np.flatnonzero(keys == keys.max())[0]])                 # the earliest frame that holds the largest key
        assert tr[f, ref.PEAK] == r[events_ref.PEAK] and f * h * w + int(tr[f, ref.PEAK_INDEX]) == r[events_ref.PEAK_INDEX]
        assert (sx[e].sum(), sy[e].sum(), int((np.arange(t) * area).sum())) == (ex[e], ey[e], et[e])
        assert int(tr[present[0], ref.ROOT]) + int(present[0]) * h * w == r[events_ref.ROOT]
    if int(counts[0]) <= len(records):
        assert np.array_equal(tracks[:, :, ref.AREA].astype(np.int64).sum(0), frame_counts[:, 1])


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tracks_refine_the_event_records(mode):
    connectivity, temporal = mode
    rng = np.random.default_rng(2500 + connectivity + temporal)
    for shape, density in (((6, 9, 11), 0.15), ((6, 9, 11), 0.4), ((1, 7, 5), 0.5), ((7, 1, 1), 0.6), ((1, 1, 1), 1.0), ((5, 6, 13), 0.7)):
        vol, thr = _volume(rng, shape, density)
        for min_duration, min_volume, max_events in ((1, 1, BIG), (2, 1, BIG), (1, 3, BIG), (1, 1, 2), (2, 2, 1)):
            tracks, records, counts, frames, labels = ref.tracks(vol, thr, connectivity, temporal, min_duration, min_volume, max_events)
            assert tracks.shape == (max_events, shape[0], 12) and tracks.dtype == np.uint32
            check_invariants(tracks, records, counts, frames, shape)
            # pixels of dropped and of truncated events are in no track
            in_table = np.isin(labels, records[:min(int(counts[0]), max_events), events_ref.ROOT].astype(np.int64) + 1) & (labels != 0)
            assert int(tracks[:, :, ref.AREA].astype(np.int64).sum()) == int(in_table.sum())


def test_hand_made_cross_sections():
    t, h, w = 5, 16, 24
    vol = np.zeros((t, h, w), np.float32)
    for f in range(t):                                                           # a 3 x 3 blob that drifts two columns a frame
        vol[f, 4:7, 2 + 2 * f:5 + 2 * f] = 1.0 + f
    vol[1, 12, 20] = vol[3, 12, 20] = 5.0                                        # absent for one frame: two events
    tracks, records, counts, _, _ = ref.tracks(vol, 0.5, 8, 9, 1, 1, 4)
    assert counts[0] == 3
    assert [tuple(r) for r in tracks[0, :, ref.X0:ref.Y1 + 1]] == [(2 + 2 * f, 4, 4 + 2 * f, 6) for f in range(t)]
    assert tuple(records[0, events_ref.X0:events_ref.Y1 + 1]) == (2, 4, 12, 6) and tracks[0, :, ref.AREA].tolist() == [9] * 5
    assert tracks[0, :, ref.ROOT].tolist() == [4 * w + 2 + 2 * f for f in range(t)]
    assert tracks[1, :, ref.AREA].tolist() == [0, 1, 0, 0, 0] and tracks[2, :, ref.AREA].tolist() == [0, 0, 0, 1, 0]
    assert not tracks[1, 0].any() and not tracks[3].any()
    # one event whose cross-section in frame 1 is two pieces (they join in frame 0): ONE record
    vol = np.zeros((2, h, w), np.float32)
    vol[0, 3, 2:9] = 1.0
    vol[1, 3, 2] = 2.0
    vol[1, 3, 8] = 2.0
    tracks, records, counts, _, _ = ref.tracks(vol, 0.5, 8, 1, 1, 1, 4)
    assert counts[0] == 1 and tracks[0, 1, :8].tolist() == [3 * w + 2, 2, 2, 3, 8, 3, np.float32(2.0).view(np.uint32), 3 * w + 2]  # tie: smallest index
    assert ref.sums(tracks)[0][0].tolist() == [sum(range(2, 9)), 10]
    # signed zeros and +Inf through the order key; a NaN is never foreground
    vol = np.full((1, 2, 4), -1.0, np.float32)
    vol[0, 0] = (-0.0, 0.0, -0.0, np.nan)
    vol[0, 1, 3] = np.inf
    tracks, _, counts, _, _ = ref.tracks(vol, -0.0, 4, 1, 1, 1, 4)
    assert counts.tolist() == [2, 0, 4, 1] and tracks[0, 0, :8].tolist() == [0, 3, 0, 0, 2, 0, 0, 1]           # +0.0 at index 1
    assert tracks[1, 0, ref.PEAK] == np.float32(np.inf).view(np.uint32) and tracks[1, 0, ref.PEAK_INDEX] == 7


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_restatement_equals_scipy(mode):
    ndimage = pytest.importorskip("scipy.ndimage")
    connectivity, temporal = mode
    rng = np.random.default_rng(2520 + connectivity + temporal)
    for shape, density in (((6, 9, 11), 0.2), ((5, 12, 7), 0.45), ((4, 8, 8), 0.7)):
        vol, thr = _volume(rng, shape, density)
        t, h, w = shape
        tracks, records, counts, _, _ = ref.tracks(vol, thr, connectivity, temporal, 1, 1, BIG)
        lab, n = ndimage.label(regions_ref.foreground(vol, thr), structure=events_ref.structure(connectivity, temporal))
        assert n == counts[0]                                                    # scipy numbers in ascending order of the first voxel
        sx, sy = ref.sums(tracks)
        for e in range(n):
            for f in range(t):
                mine = lab[f] == e + 1
                got = tracks[e, f]
                objects = ndimage.find_objects(mine.astype(np.int32))
                if not mine.any():
                    assert objects == [] and not got.any()
                    continue
                ys, xs = objects[0]
                assert (xs.start, ys.start, xs.stop - 1, ys.stop - 1) == tuple(got[ref.X0:ref.Y1 + 1])
                assert int(ndimage.sum(mine)) == got[ref.AREA] and np.float32(ndimage.maximum(vol[f], mine)).view(np.uint32) == got[ref.PEAK]
                assert ndimage.maximum_position(vol[f], mine) == divmod(int(got[ref.PEAK_INDEX]), w)      # distinct values: no ties
                cy, cx = ndimage.center_of_mass(mine)
                assert abs(cy - sy[e, f] / got[ref.AREA]) < 1e-9 and abs(cx - sx[e, f] / got[ref.AREA]) < 1e-9
                assert got[ref.ROOT] == np.flatnonzero(mine.reshape(-1))[0]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_live_boxes_are_the_newest_cross_sections_of_the_prefix(mode):
    connectivity, temporal = mode
    rng = np.random.default_rng(2540 + connectivity + temporal)
    for shape, density in (((7, 8, 9), 0.3), ((5, 6, 7), 0.55), ((4, 3, 1), 0.6)):
        t, h, w = shape
        vol, thr = _volume(rng, shape, density)
        tr = track_ref.Tracker(h, w, thr, connectivity, temporal, 1, 1, 64, BIG)
        for f in range(t):
            tr.update(vol[f:f + 1])
            got = ref.boxes(tr, vol[f])
            table = tr.open_table()
            assert np.array_equal(got[:len(tr.table), ref.ROOT], table[:len(tr.table), track_ref.HANDLE]) and not got[len(tr.table):].any()
            clip, records, counts, _, _ = ref.tracks(vol[:f + 1], thr, connectivity, temporal, 1, 1, BIG)
            newest = clip[:int(counts[0]), f]
            newest = newest[newest[:, ref.AREA] > 0]
            assert np.array_equal(newest[np.argsort(newest[:, ref.ROOT])], got[:len(tr.table)])
    # max_open = 2 with three objects: the lost one has no record
    vol = np.zeros((2, 1, 7), np.float32)
    vol[:, 0, 0] = vol[:, 0, 3] = vol[:, 0, 6] = 1.0
    tr = track_ref.Tracker(1, 7, 0.5, 8, 9, 1, 1, 2, 8)
    tr.update(vol[:1])
    assert ref.boxes(tr, vol[0])[:, :2].tolist() == [[0, 1], [3, 1]] and tr.plane[6] == track_ref.NO_RECORD


# ------------------------------------------------------------------------------------------ the library without a GPU
def test_the_plan_without_a_gpu():
    lib = hip.lib()
    out = [hip.C.c_int(0) for _ in range(2)]
    assert lib.vad_event_tracks_plan(*[hip.C.byref(v) for v in out]) == 0
    reduce_round, threads = (v.value for v in out)
    assert threads == 256 and reduce_round % 1024 == 0 and 256 * 256 <= reduce_round < 520 * 520
    assert lib.vad_event_tracks_plan(None, None) == -1 and b"event_tracks_plan" in lib.vad_last_error()
    assert hip.MAX_TRACK_RECORDS == metrics.MAX_TRACK_RECORDS == ref.MAX_RECORDS == 2 ** 26 and hip.REGION_WORDS == ref.WORDS == 12


def test_refusals_by_name_without_a_gpu():
    """Every argument check runs on the host, before any device call: the addresses are never read."""
    lib = hip.lib()
    fake = 1 << 20
    a = (fake, fake, fake, fake, 2, 3, 8, 8, 16, fake, None)            # maps, labels, records, counts, b, t, h, w, max_events, tracks, stream
    for pos, bad, word in ((0, None, b"maps is NULL"), (0, fake + 2, b"maps must be 4-byte"), (1, None, b"labels is NULL"),
                           (1, fake + 1, b"labels must be 4-byte"), (2, None, b"records is NULL"), (2, fake + 8, b"records must be 16-byte"),
                           (3, None, b"counts is NULL"), (3, fake + 2, b"counts must be 4-byte"), (4, -1, b"b must be >= 0"), (5, 0, b"t must be >= 1"),
                           (5, -2, b"t must be >= 1"), (6, 0, b"h and w must be >= 1"), (7, 0, b"h and w must be >= 1"), (7, -3, b"h and w must be >= 1"),
                           (8, 0, b"max_events must be in 1..65536"), (8, 65537, b"max_events must be in 1..65536"), (9, None, b"tracks is NULL"),
                           (9, fake + 8, b"tracks must be 16-byte")):
        args = list(a)
        args[pos] = bad
        assert lib.vad_event_tracks(*args) == -1 and word in lib.vad_last_error() and b"event_tracks:" in lib.vad_last_error(), (pos, bad, lib.vad_last_error())
    for dims, word in (((1, 1, 65536, 32768), b"h * w < 2^31 - 1"), ((1, 1 << 16, 256, 256), b"t * h * w must be below 2^31 - 1"),
                       ((1 << 20, 16, 256, 256), b"b * t * h * w must be at most 2^38")):
        args = list(a)
        args[4:8] = dims
        assert lib.vad_event_tracks(*args) == -1 and word in lib.vad_last_error(), (dims, lib.vad_last_error())
    # the record-count limit: b * max_events * t <= 2^26
    for b, t, max_events, ok in ((64, 16, 65536, True), (65, 16, 65536, False), (1, 1024, 65536, True), (1, 1025, 65536, False), (1 << 16, 1, 1025, False)):
        args = list(a)
        args[4], args[5], args[6], args[7], args[8] = b, t, 2, 2, max_events
        args[0] = None                                                   # the limit is checked in front of the tracks pointer, behind the maps
        assert lib.vad_event_tracks(*args) == -1 and b"maps is NULL" in lib.vad_last_error()
        args[0], args[9] = fake, None
        assert lib.vad_event_tracks(*args) == -1
        assert (b"tracks is NULL" if ok else b"b * max_events * t must be at most 2^26 records") in lib.vad_last_error(), (b, t, max_events)
    args = list(a)
    args[4] = 0                                                          # b == 0 launches nothing, and needs no device
    assert lib.vad_event_tracks(*args) == 0
    x = (fake, 64, 2, 8, 8, 16, fake, fake, None)                        # maps_newest, frame_stride, b, h, w, max_open, state, boxes, stream
    for pos, bad, word in ((0, None, b"maps_newest is NULL"), (0, fake + 2, b"maps_newest must be 4-byte"), (1, 63, b"frame_stride must be"),
                           (1, -64, b"frame_stride must be"), (1, (1 << 38) + 1, b"frame_stride must be"), (2, -1, b"b must be in 0..2^20"),
                           (2, (1 << 20) + 1, b"b must be in 0..2^20"), (3, 0, b"h and w must be >= 1"), (4, 0, b"h and w must be >= 1"),
                           (5, 0, b"max_open must be in 1..65536"), (5, 65537, b"max_open must be in 1..65536"), (6, None, b"state is NULL"),
                           (6, fake + 8, b"state must be 16-byte"), (7, None, b"boxes is NULL"), (7, fake + 4, b"boxes must be 16-byte")):
        args = list(x)
        args[pos] = bad
        assert lib.vad_track_boxes(*args) == -1 and word in lib.vad_last_error() and b"track_boxes:" in lib.vad_last_error(), (pos, bad, lib.vad_last_error())
    args = list(x)
    args[1:5] = (1 << 25, 1, 4097, 4096)
    assert lib.vad_track_boxes(*args) == -1 and b"h * w <= 2^24" in lib.vad_last_error()
    args = list(x)
    args[2] = 0
    assert lib.vad_track_boxes(*args) == 0


def _events(labels=True, t=3, h=4, w=5, max_events=2, lead=(2,), dtype=torch.int32):
    return metrics.Events(torch.zeros((*lead, max_events, 16), dtype=dtype), torch.zeros((*lead, 4), dtype=torch.int32),
                          torch.zeros((*lead, t, 3), dtype=torch.int32), torch.zeros((*lead, t, h, w), dtype=torch.int32) if labels else None,
                          (t, h, w), 0.5, 8, 9, 1, 1)


def test_python_refusals_without_a_gpu():
    maps = torch.zeros(2, 3, 4, 5)
    with pytest.raises(hip.VadError, match="event_tracks: events must be a metrics.Events, got dict"):
        metrics.event_tracks(maps, {})
    with pytest.raises(hip.VadError, match="event_tracks: events carry no labels; detect them with detect_events\\(..., return_labels=True\\)"):
        metrics.event_tracks(maps, _events(labels=False))
    with pytest.raises(hip.VadError, match="event_tracks: maps must be a torch tensor"):
        metrics.event_tracks(np.zeros((2, 3, 4, 5), np.float32), _events())
    for shape in ((2, 3, 4, 6), (3, 3, 4, 5), (3, 4, 5), (2, 3, 2, 4, 5)):
        with pytest.raises(hip.VadError, match="event_tracks: maps .* do not match the events' volumes \\(2, 3, 4, 5\\)"):
            metrics.event_tracks(torch.zeros(shape), _events())
    with pytest.raises(hip.VadError, match="event_tracks: maps .* do not match the events' volumes \\(3, 4, 5\\)"):
        metrics.event_tracks(torch.zeros(1, 3, 4, 5), _events(lead=()))
    bad = _events()
    bad.labels = bad.labels[:, :2]
    with pytest.raises(hip.VadError, match="event_tracks: the events' labels .* do not match their volumes"):
        metrics.event_tracks(maps, bad)
    with pytest.raises(hip.VadError, match="event_tracks: the events' records must be int32, got torch.int64"):
        metrics.event_tracks(maps, _events(dtype=torch.int64))
    with pytest.raises(hip.VadError, match="event_tracks: maps \\(cpu\\) must be on the GPU \\(tracks are reduced on the device; there is no CPU fallback\\)"):
        metrics.event_tracks(maps, _events())
    with pytest.raises(hip.VadError, match="event_tracks: maps \\(cpu\\) must be on the GPU"):
        metrics.event_tracks(maps.view(2, 3, 1, 4, 5), _events())
    assert _events().tracks is None
    up = metrics.TrackUpdate(torch.zeros(1, 2, 20, dtype=torch.int32), torch.zeros(1, 6, dtype=torch.int32), torch.zeros(1, 1, 3, dtype=torch.int32), (4, 5), 2)
    assert up.boxes is None
    with pytest.raises(hip.VadError, match="boxes_alarming: this update carries no boxes; call update\\(maps, boxes=True\\)"):
        up.boxes_alarming()
    with pytest.raises(hip.VadError, match="localize_events: tracks must be a bool"):
        scoring.localize_events(None, torch.zeros(1, 3, 16, 16), 0.5, tracks=1)


def test_views_of_the_records_without_a_gpu():
    vol = np.zeros((1, 3, 6, 7), np.float32)
    vol[0, :, 2:4, 1:3] = 1.0
    vol[0, 1, 3, 2] = 7.0
    vol[0, 1:, 5, 6] = 2.0
    tracks, records, counts, _, _ = ref.tracks_batch(vol, 0.5, 8, 9, 1, 1, 3)
    tr = metrics.EventTracks(torch.from_numpy(tracks.view(np.int32)), torch.from_numpy(counts.view(np.int32)), (3, 6, 7))
    assert tuple(tr.records.shape) == (1, 3, 3, 12) and tr.max_events == 3
    assert tr.present()[0].tolist() == [[True] * 3, [False, True, True], [False] * 3] and tr.area[0, 0].tolist() == [4, 4, 4]
    assert tr.box[0, 1, 1].tolist() == [6, 5, 6, 5] and tr.peak[0, 0].tolist() == [1.0, 7.0, 1.0] and tr.peak_index[0, 0, 1] == 3 * 7 + 2
    assert tr.sum_x[0, 0].tolist() == [6, 6, 6] and tr.sum_y[0, 0].tolist() == [10, 10, 10] and tr.root[0, 1].tolist() == [0, 41, 41]
    c = tr.centroids()
    assert c.dtype == torch.float64 and c[0, 0, 0].tolist() == [2.5, 1.5] and bool(torch.isnan(c[0, 1, 0]).all()) and bool(torch.isnan(c[0, 2]).all())
    assert tr.frame(1).data_ptr() == tr.records[:, :, 1].data_ptr() and tuple(tr.frame(-1).shape) == (1, 3, 12)
    with pytest.raises(hip.VadError, match="EventTracks.frame: t must be an int in -3..2, got 3"):
        tr.frame(3)
    rows = tr.to_list()
    assert len(rows) == 1 and len(rows[0]) == 2 and rows[0][1][0] is None
    assert rows[0][0][1] == {"root": 15, "area": 4, "box": (1, 2, 2, 3), "peak": 7.0, "peak_yx": (3, 2), "centroid_yx": (2.5, 1.5)}
    boxes = metrics.TrackBoxes(tr.frame(2)[:, :2], (6, 7))
    assert boxes.to_list() == [[rows[0][0][2], rows[0][1][2]]] and boxes.present().tolist() == [[True, True]]


def test_header_and_signatures_agree():
    header = (REPO / "include" / "vad_hip.h").read_text()
    lib = hip.lib()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("vad_event_tracks", 11), ("vad_event_tracks_plan", 2), ("vad_track_boxes", 9)):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, plain, flags=re.S).group(1)
        assert len(hip.SIGNATURES[name][1]) == len(decl.split(",")) == count, name
    assert "map_event_tracks.hip" in hip.SOURCES and (hip.CSRC / "map_event_tracks.hip").exists()
    section = header[header.index("Per-frame tracks of anomaly events"):header.index("int vad_event_tracks(")]
    assert "b * max_events * t = 2^26 records" in section                      # the record-count limit is stated where the call is declared
    rows = re.findall(r"\*\s+words? (\d+)(?:-(\d+))?\s+(\w+)", section)
    assert [(int(a), n.rstrip(":")) for a, _, n in rows] == [(0, "the"), (1, "area"), (2, "x0"), (6, "peak"), (7, "peak"), (8, "uint64"), (10, "uint64")]
    assert (ref.ROOT, ref.AREA, ref.X0, ref.PEAK, ref.PEAK_INDEX, ref.SUM_X, ref.SUM_Y) == (0, 1, 2, 6, 7, 8, 10)
