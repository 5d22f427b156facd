"""Per-frame tracks of anomaly events on the GPU (csrc/map_event_tracks.hip, metrics.event_tracks, EventTracker.update(boxes=True)):
every word against the numpy restatement (tests/event_tracks_ref.py) - hand-made volumes, filters and truncation, shapes beyond one
grid round, batching, random volumes under the three structures -, the equalities that tie a track to its event record computed on
the device, one frame against detect_regions, the tracker's boxes for every split of the frames over calls and against the clip
mode on the prefix, captured calls, both seeded models against the host route, and the defaults that launch nothing new."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import event_tracks_ref as ref
import events_ref
import pro_ref
import track_ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
MODES = ((4, 1), (8, 1), (8, 9))
MODE_IDS = [f"c{c}t{t}" for c, t in MODES]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _from_masks(seed, mask):
    return events_ref.map_from_mask(np.random.default_rng(seed), np.asarray(mask, bool), T)


def _run_and_check(vad, maps, t=T, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """maps float32 [b, t, h, w] (numpy) -> (EventTracks, Events, restatement): tracks and event records equal the restatement's."""
    maps = np.ascontiguousarray(maps, np.float32)
    want = ref.tracks_batch(maps, t, connectivity, temporal, min_duration, min_volume, max_events)
    x = torch.from_numpy(maps).cuda()
    ev = vad.metrics.detect_events(x, float(t), connectivity, temporal, min_duration, min_volume, max_events, return_labels=True)
    before = vad.hip.calls.get("event_tracks", 0)
    got = vad.metrics.event_tracks(x, ev)
    assert vad.hip.calls.get("event_tracks", 0) == before + 1
    assert got.records.dtype == torch.int32 and tuple(got.records.shape) == want[0].shape and got.records.is_cuda
    assert torch.equal(ev.records.cpu(), _i32(want[1])) and torch.equal(ev.counts.cpu(), _i32(want[2]))
    assert torch.equal(got.records.cpu(), _i32(want[0])), "tracks differ from the restatement"
    assert got.counts.data_ptr() == ev.counts.data_ptr()
    return got, ev, want


# ------------------------------------------------------------------------------------------ 1. hand-made volumes
def _hand_made():
    t, h, w = 5, 16, 24
    out = {}
    m = np.zeros((t, h, w), bool)
    for f in range(t):
        m[f, 4:7, 2 + 2 * f:5 + 2 * f] = True
    out["drift"] = _from_masks(2601, m)
    m = np.zeros((t, h, w), bool)
    m[0, 3, 2:9] = True
    m[1:, 3, 2] = m[1:, 3, 8] = True                                           # two pieces from frame 1 on: joined through frame 0
    m[1:4, 10:12, 15:18] = True
    out["two_pieces"] = _from_masks(2602, m)
    m = np.zeros((t, h, w), bool)
    m[0:2, 5, 3] = m[0:2, 5, 9] = True                                         # two blobs ...
    m[2, 5, 3:10] = True                                                       # ... merge in frame 2 ...
    m[3:, 5, 4] = m[3:, 5, 8] = True                                           # ... and split again: one event throughout
    out["merge_split"] = _from_masks(2603, m)
    m = np.zeros((t, h, w), bool)
    m[:, 2:4, 2:5] = True
    m[:, 12:15, 18:23] = True
    out["two_events"] = _from_masks(2604, m)
    m = np.zeros((t, h, w), bool)
    m[1:4, 7:9, 11:14] = True
    m[0, 0, 0] = m[4, 15, 23] = True
    out["frames_1_to_3"] = _from_masks(2605, m)
    v = np.zeros((t, h, w), np.float32)
    v[:, 6:9, 6:9] = 1.0
    v[2, 7, 8] = v[2, 8, 6] = v[2, 6, 7] = 3.0                                 # a tie in frame 2: the smallest index wins
    v[3, 8, 8] = v[3, 6, 6] = 3.0
    out["peak_tie"] = v
    v = np.full((t, h, w), -1.0, np.float32)
    v[:, 4, 4:8] = -0.0
    v[1, 4, 5] = v[3, 4, 7] = 0.0                                              # +0.0 above -0.0
    v[:, 10, 10:12] = 0.5
    v[2, 10, 11] = np.inf
    out["zeros_inf"] = v
    v = _from_masks(2606, m)
    v[1:4, 7, 12] = np.nan                                                     # a hole in the blob of frames 1..3
    v[0, 0, 1] = v[4, 15, 22] = np.nan
    out["nan"] = v
    return out


HAND_MADE = _hand_made()


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_volumes(vad, name):
    vol = HAND_MADE[name]
    thr = np.float32(-0.0) if name == "zeros_inf" else T
    for connectivity, temporal in MODES:
        got, ev, want = _run_and_check(vad, vol[None], thr, connectivity, temporal, max_events=8)
    tracks, records, counts = want[0][0], want[1][0], want[2][0]               # (8, 9)
    area = tracks[:, :, ref.AREA]
    if name == "drift":
        assert counts[0] == 1 and [tuple(r) for r in tracks[0, :, ref.X0:ref.Y1 + 1]] == [(2 + 2 * f, 4, 4 + 2 * f, 6) for f in range(5)]
        assert tuple(records[0, events_ref.X0:events_ref.Y1 + 1]) == (2, 4, 12, 6)           # the union: a smear over the path
        assert torch.equal(got.box[0, 0, :, 2].cpu(), torch.tensor([4, 6, 8, 10, 12], dtype=torch.int32)) and bool(got.present()[0, 0].all())
    elif name == "two_pieces":
        assert counts[0] == 2 and area[0].tolist() == [7, 2, 2, 2, 2] and tuple(tracks[0, 3, ref.X0:ref.Y1 + 1]) == (2, 3, 8, 3)
    elif name == "merge_split":
        assert counts[0] == 1 and area[0].tolist() == [2, 2, 7, 2, 2] and tracks[0, :, ref.X0].tolist() == [3, 3, 3, 4, 4]
    elif name == "two_events":
        assert counts[0] == 2 and area[:2].tolist() == [[6] * 5, [15] * 5]
    elif name == "frames_1_to_3":
        assert counts[0] == 3 and area[:3].tolist() == [[1, 0, 0, 0, 0], [0, 6, 6, 6, 0], [0, 0, 0, 0, 1]] and not tracks[1, 0].any()
    elif name == "peak_tie":
        assert tracks[0, :, ref.PEAK_INDEX].tolist() == [6 * 24 + 6, 6 * 24 + 6, 6 * 24 + 7, 6 * 24 + 6, 6 * 24 + 6]
    elif name == "zeros_inf":
        zero, inf = np.float32(0.0).view(np.uint32), np.float32(np.inf).view(np.uint32)
        assert counts[0] == 2 and tracks[0, 1, ref.PEAK:ref.PEAK_INDEX + 1].tolist() == [zero, 4 * 24 + 5]
        assert tracks[0, 0, ref.PEAK:ref.PEAK_INDEX + 1].tolist() == [np.float32(-0.0).view(np.uint32), 4 * 24 + 4]
        assert tracks[1, 2, ref.PEAK:ref.PEAK_INDEX + 1].tolist() == [inf, 10 * 24 + 11] and bool(torch.isinf(got.peak[0, 1, 2]))
    elif name == "nan":
        assert counts.tolist() == [3, 0, 17, 5] and area[1].tolist() == [0, 5, 5, 5, 0]


# ------------------------------------------------------------------------------------------ 2. filters and truncation
def test_filters_and_truncation(vad):
    m = np.zeros((1, 5, 16, 24), bool)
    m[0, :, 1:3, 1:3] = True                                                   # kept
    m[0, 2, 8, 8:12] = True                                                    # one frame: dropped by min_duration 2
    m[0, 1:4, 14, 20] = True                                                   # three pixels: dropped by min_volume 4
    m[0, 1:3, 5:7, 15:17] = True                                               # kept
    m[0, 3:5, 11:13, 3:6] = True                                               # kept
    maps = _from_masks(2610, m)
    got, ev, want = _run_and_check(vad, maps, T, 8, 9, 2, 4, 8)
    assert want[2][0, :2].tolist() == [3, 2] and want[0][0, :, :, ref.AREA].sum(1).tolist() == [20, 8, 12, 0, 0, 0, 0, 0]
    full = want[0][0]
    for max_events in (1, 2):
        got, ev, want = _run_and_check(vad, maps, T, 8, 9, 2, 4, max_events)
        assert bool(ev.truncated()[0]) and int(got.counts[0, 0]) == 3 > max_events           # truncation stays visible
        assert np.array_equal(want[0][0], full[:max_events])                   # the truncated events have no track, the others theirs
        assert len(got.to_list()[0]) == max_events


# ------------------------------------------------------------------------------------------ 3. shapes
def test_odd_shapes(vad):
    _run_and_check(vad, np.ones((1, 1, 1, 1), np.float32))
    _run_and_check(vad, np.zeros((1, 1, 1, 1), np.float32))
    rng = np.random.default_rng(2620)
    for connectivity, temporal in MODES:
        _run_and_check(vad, _from_masks(2621, rng.random((2, 7, 13, 17)) < 0.3), T, connectivity, temporal, 1, 1, 128)


def test_a_frame_one_row_larger_than_a_grid_round(vad):
    out = [ctypes.c_int(0) for _ in range(2)]
    assert vad.hip.lib().vad_event_tracks_plan(*[ctypes.byref(v) for v in out]) == 0
    reduce_round, threads = (v.value for v in out)
    w = 512
    h = reduce_round // w + 1
    assert threads == 256 and reduce_round % w == 0 and (h - 1) * w == reduce_round
    m = np.zeros((1, 2, h, w), bool)
    m[0, :, 0, 0:3] = True                                                     # the first pixels
    m[0, :, h - 1, w - 4:] = True                                              # the last row: behind the round in frame 0, and in frame 1
    m[0, 0, h - 2, 100:110] = m[0, 1, h - 1, 105:130] = True                   # across the end of the round, linked diagonally in time
    m[0, 1, 200:203, 300:310] = True
    m[0, :, 77, :] = True                                                      # a whole row
    got, ev, want = _run_and_check(vad, _from_masks(2630, m), T, 8, 9)
    assert want[2][0, 0] == 5 and want[0][0, 1, :, ref.AREA].tolist() == [w, w] and want[0][0, 2, :, ref.Y1].tolist() == [h - 2, h - 1]


def test_three_clips_in_one_call_equal_each_alone(vad):
    rng = np.random.default_rng(2640)
    mask = np.stack([np.repeat(pro_ref.blobs(rng, 1, 24, 40), 4, axis=0) & (rng.random((4, 24, 40)) < 0.85), rng.random((4, 24, 40)) < 0.1,
                     np.ones((4, 24, 40), bool)])
    maps = _from_masks(2641, mask)
    got, ev, want = _run_and_check(vad, maps, T, 8, 9, 1, 2, 32)
    for c in range(3):
        alone, _, _ = _run_and_check(vad, maps[c:c + 1], T, 8, 9, 1, 2, 32)
        assert torch.equal(alone.records[0], got.records[c])
    assert want[0][2, 0, :, ref.AREA].tolist() == [960] * 4                    # all foreground: one event, one record a frame
    one = vad.metrics.detect_events(torch.from_numpy(maps[0]).cuda(), float(T), 8, 9, 1, 2, 32, return_labels=True)       # [T,H,W]: no leading shape
    single = vad.metrics.event_tracks(torch.from_numpy(maps[0]).cuda(), one)
    assert tuple(single.records.shape) == (32, 4, 12) and torch.equal(single.records, got.records[0])
    five = vad.metrics.event_tracks(torch.from_numpy(maps).cuda()[:, :, None], ev)                                         # [B,T,1,H,W]
    assert torch.equal(five.records, got.records)


# ------------------------------------------------------------------------------------------ 4. random volumes, 5. invariants
def _random_maps():
    rng = np.random.default_rng(2650)
    blobs = np.repeat(pro_ref.blobs(rng, 4, 40, 56)[:, None], 6, axis=1) & (rng.random((4, 6, 40, 56)) < 0.8)
    for c in range(4):
        for f in range(6):
            blobs[c, f] = np.roll(blobs[c, f], (f * (c - 1), f), axis=(0, 1))  # every clip drifts its own way
    return _from_masks(2651, blobs | (rng.random((4, 6, 40, 56)) < 0.01))


RANDOM = _random_maps()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_random_volumes_and_the_invariants_on_the_device(vad, mode):
    connectivity, temporal = mode
    b, t, h, w = RANDOM.shape
    got, ev, want = _run_and_check(vad, RANDOM, T, connectivity, temporal, 1, 1, 256)
    assert not bool(ev.truncated().any()) and int(ev.counts[:, 0].min()) > 5
    used = torch.arange(256, device="cuda")[None, :] < ev.counts[:, :1]                        # [b, E]
    area = got.area.to(torch.int64)
    present = got.present()
    assert torch.equal(area.sum(-1), ev.volume.to(torch.int64)) and not bool(got.records[~used].any())
    big = torch.iinfo(torch.int32).max
    box = got.box
    lo = torch.where(present[..., None], box[..., :2], torch.full_like(box[..., :2], big)).amin(-2)
    hi = torch.where(present[..., None], box[..., 2:], torch.full_like(box[..., 2:], -1)).amax(-2)
    assert torch.equal(torch.cat([lo, hi], -1)[used], ev.box[used])
    bits = got.records[..., 6].to(torch.int64) & 0xFFFFFFFF
    key = torch.where(bits >= 2 ** 31, 0xFFFFFFFF - bits, bits | 2 ** 31)                     # the order key of the peak's bits
    key = torch.where(present, key, torch.full_like(key, -1))
    first = (key == key.amax(-1, keepdim=True)).to(torch.int64).argmax(-1)                     # the earliest frame that holds the peak
    at = first[..., None]
    assert torch.equal(got.records[..., 6].gather(-1, at)[..., 0][used], ev.records[..., 8][used])
    assert torch.equal((first * h * w + got.peak_index.to(torch.int64).gather(-1, at)[..., 0])[used], ev.peak_index.to(torch.int64)[used])
    assert torch.equal(got.sum_x.sum(-1), ev.sum_x) and torch.equal(got.sum_y.sum(-1), ev.sum_y)
    frames = torch.arange(t, device="cuda")
    assert torch.equal((area * frames).sum(-1), ev.sum_t)
    inside = (frames >= ev.t0[..., None]) & (frames <= ev.t1[..., None]) & used[..., None]
    assert torch.equal(present, inside)
    assert torch.equal(area.sum(1), ev.frame_counts[..., 1].to(torch.int64))                   # per frame, over the events
    c = got.centroids()
    assert bool(torch.isnan(c[~present]).all()) and bool((c[present][:, 0] < h).all()) and bool((c[present][:, 1] < w).all())


# ------------------------------------------------------------------------------------------ 6. one frame is the region table
@pytest.mark.parametrize("connectivity", (4, 8))
def test_one_frame_equals_detect_regions(vad, connectivity):
    rng = np.random.default_rng(2660)
    maps = _from_masks(2661, pro_ref.blobs(rng, 3, 37, 53) | (rng.random((3, 37, 53)) < 0.02))
    x = torch.from_numpy(maps).cuda()
    for min_volume, max_events in ((1, 64), (3, 64), (1, 2)):
        ev = vad.metrics.detect_events(x[:, None], float(T), connectivity, 1, 1, min_volume, max_events, return_labels=True)
        tracks = vad.metrics.event_tracks(x[:, None], ev)
        regions = vad.metrics.detect_regions(x, float(T), connectivity, min_area=min_volume, max_regions=max_events)
        assert torch.equal(tracks.records[..., 0, :], regions.records) and torch.equal(tracks.frame(0), regions.records)


# ------------------------------------------------------------------------------------------ 7. the tracker's boxes
def _kw(threshold=T, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_open=16, max_closed=16):
    return dict(threshold=float(threshold), connectivity=connectivity, temporal=temporal, min_duration=min_duration, min_volume=min_volume,
                max_open=max_open, max_closed=max_closed)


def _check_boxes(up, tr, rts, newest, s_list=None):
    """up: the TrackUpdate of the call; rts: the restatement's trackers after the same frames; newest float32 [b, h, w]."""
    assert up.boxes.records.dtype == torch.int32 and tuple(up.boxes.records.shape) == (len(rts), tr.max_open, 12)
    opened = tr.open_events()
    for s in (range(len(rts)) if s_list is None else s_list):
        want = ref.boxes(rts[s], newest[s])
        assert torch.equal(up.boxes.records[s].cpu(), _i32(want)), "boxes differ from the restatement"
        n = int(opened.counts[s])
        assert n == len(rts[s].table) and torch.equal(up.boxes.root[s, :n], opened.handle[s, :n]) and not bool(up.boxes.records[s, n:].any())
        alarming = [rts[s]._passes(e) for e in rts[s].table] + [False] * (tr.max_open - n)
        assert up.boxes_alarming()[s].cpu().tolist() == alarming


def test_boxes_for_every_split_of_seven_frames(vad):
    rng = np.random.default_rng(2670)
    mask = np.repeat(pro_ref.blobs(rng, 2, 12, 20, count=3, radius=3)[:, None], 7, axis=1) & (rng.random((2, 7, 12, 20)) < 0.85)
    for f in range(7):
        mask[0, f] = np.roll(mask[0, f], f, axis=1)                            # stream 0 drifts
    mask[1, 3] = False                                                         # every event of stream 1 closes once
    maps = _from_masks(2671, mask)
    x = torch.from_numpy(maps).cuda()
    kw = _kw(min_duration=2, min_volume=3)
    # the clip mode on every prefix, once: the cross-sections in the prefix's last frame, in raster order of their smallest pixel
    clip_newest = {}
    for f in range(1, 8):
        ev = vad.metrics.detect_events(x[:, :f], kw["threshold"], 8, 9, 1, 1, 64, return_labels=True)
        last = vad.metrics.event_tracks(x[:, :f], ev).frame(f - 1).cpu()
        assert not bool(ev.truncated().any())
        clip_newest[f] = [sorted((r.tolist() for r in last[s] if r[1] > 0), key=lambda r: r[0]) for s in range(2)]
    splits = [c for n in range(1, 8) for c in itertools.product(range(1, 8), repeat=n) if sum(c) == 7]
    assert len(splits) == 64
    for split in splits:
        tr = vad.metrics.EventTracker(2, 12, 20, **kw)
        rts = [track_ref.Tracker(12, 20, **kw) for _ in range(2)]
        at = 0
        for n in split:
            before = vad.hip.calls.get("track_boxes", 0)
            up = tr.update(x[:, at:at + n], boxes=True)
            assert vad.hip.calls.get("track_boxes", 0) == before + 1
            for s in range(2):
                rts[s].update(maps[s, at:at + n])
            at += n
            _check_boxes(up, tr, rts, maps[:, at - 1])
            for s in range(2):                                                 # matched through the handle: both orders are the handles'
                k = len(rts[s].table)
                assert up.boxes.records[s, :k].cpu().tolist() == clip_newest[at][s]


def test_a_lost_event_has_no_box_and_a_reset_leaves_the_other_streams(vad):
    m = np.zeros((3, 4, 6, 20), bool)
    m[:, :, 1:3, 1:3] = m[:, :, 1:4, 8:10] = m[:, :, 4, 15:19] = True          # three objects in every stream
    m[1, :, 0, 5] = True                                                       # a fourth in stream 1
    maps = _from_masks(2680, m)
    x = torch.from_numpy(maps).cuda()
    kw = _kw(max_open=2)
    tr = vad.metrics.EventTracker(3, 6, 20, **kw)
    rts = [track_ref.Tracker(6, 20, **kw) for _ in range(3)]
    for f in range(2):
        up = tr.update(x[:, f], boxes=True)
        for s in range(3):
            rts[s].update(maps[s, f:f + 1])
        _check_boxes(up, tr, rts, maps[:, f])
        assert up.lost().cpu().tolist() == [1, 2, 1] and up.boxes.area.cpu().tolist() == [[4, 6], [1, 4], [4, 6]]           # the third has no record
        assert int((tr.slot_plane[0] == -1).sum()) == 4
    kept = up.boxes.records.clone()
    tr.reset([1])
    rts[1].reset()
    up = tr.update(x[:, 2], boxes=True)
    for s in range(3):
        rts[s].update(maps[s, 2:3])
    _check_boxes(up, tr, rts, maps[:, 2])
    same = _from_masks(2680, m)                                                # the map's values differ by frame; the boxes' geometry does not
    assert torch.equal(up.boxes.records[[0, 2]][..., :6], kept[[0, 2]][..., :6]) and np.array_equal(same, maps)
    # T > 1: the cross-sections of the LAST frame of the call, read in place
    tr2 = vad.metrics.EventTracker(3, 6, 20, **kw)
    up2 = tr2.update(x[:, :3], boxes=True)
    rts2 = [track_ref.Tracker(6, 20, **kw) for _ in range(3)]
    for s in range(3):
        rts2[s].update(maps[s, :3])
    _check_boxes(up2, tr2, rts2, maps[:, 2])
    five = vad.metrics.EventTracker(3, 6, 20, **kw).update(x[:, :3, None], boxes=True)                                      # [B,T,1,H,W]
    assert torch.equal(five.boxes.records, up2.boxes.records)


def test_a_foreign_state_gives_zero_boxes(vad):
    """The header is compared on the device: a blob that is not this geometry's state writes zeros."""
    lib = vad.hip.lib()
    x = torch.from_numpy(_from_masks(2690, np.ones((2, 6, 20), bool))).cuda()
    tr = vad.metrics.EventTracker(2, 6, 20, **_kw(max_open=4))
    tr.update(x)
    boxes = torch.full((2, 4, 12), -7, dtype=torch.int32, device="cuda")

    def call(state, h, w, max_open):
        boxes.fill_(-7)
        vad.hip.check(lib.vad_track_boxes(x.data_ptr(), h * w, 2, h, w, max_open, state.data_ptr(), boxes.data_ptr(), vad.hip.current_stream()), "vad_track_boxes")
        return boxes.cpu()

    assert call(tr.state, 6, 20, 4)[:, 0, :6].tolist() == [[0, 120, 0, 0, 19, 5]] * 2 and not bool(boxes[:, 1:].any())
    assert not bool(call(tr.state, 20, 6, 4).any())                            # another geometry: the header's h, w disagree
    assert not bool(call(torch.zeros_like(tr.state), 6, 20, 4).any())          # no magic
    poisoned = tr.state.clone().view(2, -1)
    poisoned[1, 4] = 0x12345678
    assert call(poisoned, 6, 20, 4)[:, 0, 1].tolist() == [120, 0]              # stream 1 alone is refused


# ------------------------------------------------------------------------------------------ 8. capture
def test_captured_event_tracks_follow_new_contents(vad):
    rng = np.random.default_rng(2700)
    first = _from_masks(2701, np.repeat(pro_ref.blobs(rng, 2, 24, 40)[:, None], 4, axis=1) & (rng.random((2, 4, 24, 40)) < 0.8))
    second = _from_masks(2702, rng.random((2, 4, 24, 40)) < 0.15)
    maps = torch.from_numpy(first).cuda()
    ev = vad.metrics.detect_events(maps, float(T), 8, 9, 2, 1, 16, return_labels=True)
    vad.metrics.event_tracks(maps, ev)                                         # once eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            got = vad.metrics.event_tracks(maps, ev)
    torch.cuda.current_stream().wait_stream(side)
    for contents in (second, first):
        maps.copy_(torch.from_numpy(contents).cuda())
        new = vad.metrics.detect_events(maps, float(T), 8, 9, 2, 1, 16, return_labels=True)
        ev.labels.copy_(new.labels)                                            # the captured call reads the same buffers
        ev.records.copy_(new.records)
        ev.counts.copy_(new.counts)
        got.records.fill_(-7)
        graph.replay()
        want = ref.tracks_batch(contents, T, 8, 9, 2, 1, 16)
        assert torch.equal(got.records.cpu(), _i32(want[0])) and int(want[2][:, 0].sum()) > 0


def test_a_captured_update_with_boxes(vad):
    rng = np.random.default_rng(2710)
    mask = np.repeat(pro_ref.blobs(rng, 2, 24, 40)[:, None], 4, axis=1) & (rng.random((2, 4, 24, 40)) < 0.8)
    maps_np = _from_masks(2711, mask)
    contents = torch.from_numpy(maps_np).cuda()
    kw = _kw(min_duration=2, max_open=64)
    tr = vad.metrics.EventTracker(2, 24, 40, **kw)
    rts = [track_ref.Tracker(24, 40, **kw) for _ in range(2)]
    maps = contents[:, 0].clone()
    tr.update(maps, boxes=True)                                                # frame 0, eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            up = tr.update(maps, boxes=True)
    torch.cuda.current_stream().wait_stream(side)
    for s in range(2):
        rts[s].update(maps_np[s, :1])
    for f in range(1, 4):                                                      # three contents
        maps.copy_(contents[:, f])
        up.boxes.records.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for s in range(2):
            rts[s].update(maps_np[s, f:f + 1])
        _check_boxes(up, tr, rts, maps_np[:, f])
    assert tr.flags() == 0 and tr.frames_seen.cpu().tolist() == [4, 4]


# ------------------------------------------------------------------------------------------ 9. through the models
def _threshold_of(vad, maps, fpr=0.05):
    h, w = maps.shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w]
    lab = torch.from_numpy((((yy // 8) + (xx // 8)) % 2).astype(np.uint8) * 255).cuda().expand(maps.shape).contiguous()
    hist = vad.metrics.ScoreHistogram(11).accumulate(maps, lab)
    t, tpr, reached = vad.metrics.threshold_at_fpr(hist.counts_host(), fpr)
    assert np.isfinite(t) and reached <= fpr
    return t


def _host_tracks(events, maps):
    """The host route: the label volume and the maps copied to the host, the restatement's reduction per (event, frame)."""
    t, h, w = events.volume_shape
    volumes = maps.cpu().numpy().reshape(-1, t, h, w)
    labels = events.labels.cpu().numpy().reshape(-1, t, h, w)
    records = events.records.cpu().numpy().view(np.uint32).reshape(-1, events.max_events, 16)
    kept = events.counts.cpu().numpy().reshape(-1, 4)[:, 0]
    return np.stack([ref.tracks_of(volumes[c], labels[c], records[c], kept[c]) for c in range(len(volumes))])


def _host_boxes(tracker, maps):
    """The same for a tracker: the slot plane and the newest maps [b, h, w] copied to the host."""
    plane = tracker.slot_plane.cpu().numpy().view(np.uint32).reshape(tracker.streams, -1)
    nopen = tracker.open_events().counts.cpu().numpy()
    frames = maps.cpu().numpy().reshape(tracker.streams, tracker.h, tracker.w)
    out = np.zeros((tracker.streams, tracker.max_open, 12), np.uint32)
    for s in range(tracker.streams):
        for r in range(int(nopen[s])):
            out[s, r] = ref.section(frames[s], np.flatnonzero(plane[s] == r + 1))
    return out


def test_localize_events_with_tracks_through_both_models(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = _threshold_of(vad, vad.scoring._anomaly_maps(model, clips, "mse", 1.0, 4.0))
    before = {k: vad.hip.calls.get(k, 0) for k in ("detect_events", "event_tracks", "vid_score")}
    events, maps = vad.scoring.localize_events(model, clips, t, sigma=1.0, temporal=1, min_duration=2, max_events=16, tracks=True)
    assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [1, 1, 1]
    assert tuple(events.tracks.records.shape) == (2, 16, 4, 12) and tuple(events.labels.shape) == (2, 4, 32, 32)
    assert torch.equal(events.tracks.records.cpu(), _i32(_host_tracks(events, maps))) and int(events.tracks.area.sum()) > 0
    image = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, image, 11)
    image = image.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = _threshold_of(vad, vad.scoring._anomaly_maps(image, x, "mse", 1.0, 4.0))
    events, maps = vad.scoring.localize_events(image, x, t, sigma=1.0, connectivity=4, temporal=1, min_volume=2, max_events=8, tracks=True)
    assert tuple(events.tracks.records.shape) == (8, 6, 12) and tuple(maps.shape) == (6, 1, 32, 32)
    assert torch.equal(events.tracks.records.cpu(), _i32(_host_tracks(events, maps))[0]) and int(events.tracks.area.sum()) > 0


def test_localize_stream_with_boxes_through_both_models(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 5, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = _threshold_of(vad, model.score_stateful(clips, None, errmap=True)["errmap"])
    tracker = vad.metrics.EventTracker(2, 32, 32, **_kw(threshold=t, temporal=1, min_duration=2, max_open=256, max_closed=64))
    state, seen = None, 0
    for f in range(5):
        before = {k: vad.hip.calls.get(k, 0) for k in ("track_events", "track_boxes", "vid_score_stateful")}
        up, maps, state = vad.scoring.localize_stream(model, clips[:, f:f + 1], tracker, state, boxes=True)
        assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [1, 1, 1] and int(up.lost().sum()) == 0
        assert torch.equal(up.boxes.records.cpu(), _i32(_host_boxes(tracker, maps)))
        assert torch.equal(up.boxes.root, tracker.open_events().handle) and tuple(up.boxes_alarming().shape) == (2, 256)
        seen += int(up.boxes.area.sum())
    assert seen > 0
    image = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, image, 11)
    image = image.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 8, 3, 32, 32)).cuda().view(2, 4, 3, 32, 32)
    with torch.no_grad():
        t = _threshold_of(vad, vad.scoring._anomaly_maps(image, x.view(8, 3, 32, 32), "mse", 1.0, 4.0))
    tracker = vad.metrics.EventTracker(2, 32, 32, **_kw(threshold=t, connectivity=4, temporal=1, max_open=256, max_closed=64))
    seen = 0
    for f in range(4):
        up, maps, state = vad.scoring.localize_stream(image, x[:, f], tracker, sigma=1.0, boxes=True)
        assert state is None and torch.equal(up.boxes.records.cpu(), _i32(_host_boxes(tracker, maps)))
        seen += int(up.boxes.area.sum())
    assert seen > 0


# ------------------------------------------------------------------------------------------ 10. the defaults launch nothing new
def test_the_defaults_launch_nothing_new(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = _threshold_of(vad, vad.scoring._anomaly_maps(model, clips, "mse", None, 4.0))
    new = ("event_tracks", "track_boxes")
    before = {k: vad.hip.calls.get(k, 0) for k in new}
    plain, maps = vad.scoring.localize_events(model, clips, t, temporal=1, max_events=16)
    explicit, _ = vad.scoring.localize_events(model, clips, t, temporal=1, max_events=16, tracks=False)
    assert plain.tracks is None and plain.labels is None and explicit.tracks is None
    assert all(torch.equal(getattr(plain, k), getattr(explicit, k)) for k in ("records", "counts", "frame_counts"))
    trackers = [vad.metrics.EventTracker(2, 32, 32, **_kw(threshold=t, temporal=1)) for _ in range(3)]
    ups = [vad.scoring.localize_stream(model, clips, trackers[0], None)[0], vad.scoring.localize_stream(model, clips, trackers[1], None, boxes=False)[0],
           trackers[2].update(maps)]
    assert {k: vad.hip.calls.get(k, 0) for k in new} == before
    assert all(up.boxes is None for up in ups) and torch.equal(trackers[0].state, trackers[1].state) and torch.equal(trackers[0].state, trackers[2].state)
    assert all(torch.equal(getattr(ups[0], k), getattr(up, k)) for up in ups[1:] for k in ("records", "counts", "frame_counts"))
    with_tracks, _ = vad.scoring.localize_events(model, clips, t, temporal=1, max_events=16, tracks=True)
    assert all(torch.equal(getattr(plain, k), getattr(with_tracks, k)) for k in ("records", "counts", "frame_counts"))
    with pytest.raises(vad.hip.VadError, match="maps must be float32"):
        vad.metrics.event_tracks(maps.double()[:, :, 0], with_tracks)
