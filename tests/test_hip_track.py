"""Anomaly events across the calls of a live stream on the GPU (csrc/map_track.hip, metrics.EventTracker, scoring.localize_stream):
closed records, counts, causal frame counts, the open table and the slot plane `torch.equal` to the frame-by-frame numpy restatement
(tests/track_ref.py) for every split of the frames over calls, and - converted and sorted - to `metrics.detect_events` on the whole
clip; the links in time a wrong linker gets wrong, ties and non-finite pixels, filters and the causal alarm, lost events, frames
beyond one grid round, any batching and layout, reset, the raw C ABI with poisoned and guarded state and workspace, a captured call
replayed on new contents, and `localize_stream` through both seeded models."""
import numpy as np
import pytest
import torch

import events_ref
import pro_ref
import track_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
MODES = ((4, 1), (8, 1), (8, 9))
MODE_IDS = [f"c{c}t{t}" for c, t in MODES]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _from_masks(seed, mask):
    """mask bool [...] -> a map whose foreground under T is the mask (the value T itself among the foreground)."""
    return events_ref.map_from_mask(np.random.default_rng(seed), np.asarray(mask, bool), T)


def _kw(threshold=T, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_open=256, max_closed=64):
    return dict(threshold=float(threshold), connectivity=connectivity, temporal=temporal, min_duration=min_duration, min_volume=min_volume,
                max_open=max_open, max_closed=max_closed)


def _feed(vad, x, splits, kw, tracker=None):
    """x: float32 GPU maps [b, t, h, w] fed in calls of the given lengths, then flushed -> per stream the dict of track_ref.run, from
    the device.  Every call's closed table is checked to be all-zero behind its records in use."""
    b, t, h, w = x.shape[0], x.shape[1], x.shape[-2], x.shape[-1]            # [b, t, h, w] or [b, t, 1, h, w]
    tr = tracker if tracker is not None else vad.metrics.EventTracker(b, h, w, **kw)
    ups, at = [], 0
    for n in splits:
        ups.append(tr.update(x[:, at:at + n]))                               # raises on a set flag word
        at += n
    assert at == t
    table, plane = tr.open_events().records.cpu().clone(), tr.slot_plane.cpu().clone()
    frames_seen, lost_total = tr.frames_seen.cpu().tolist(), tr.lost_total().cpu().tolist()
    ups.append(tr.flush())
    assert not tr.open_events().records.any() and not tr.slot_plane.any() and not tr.open_events().counts.any()
    assert tr.frames_seen.cpu().tolist() == frames_seen and tr.flags() == 0
    out = []
    for s in range(b):
        closed, truncated = [], False
        for up in ups:
            assert up.records.dtype == torch.int32 and tuple(up.records.shape) == (b, kw["max_closed"], 20) and tuple(up.counts.shape) == (b, 6)
            used = min(int(up.counts[s, 0]), kw["max_closed"])
            assert not up.records[s, used:].any(), "records behind the ones in use are not zero"
            closed.append(up.records[s, :used].cpu())
            truncated |= bool(up.truncated()[s])
        out.append({"closed": torch.cat(closed), "counts": torch.stack([up.counts[s].cpu() for up in ups]),
                    "frame_counts": torch.cat([up.frame_counts[s].cpu() for up in ups]), "table": table[s], "plane": plane[s].reshape(-1),
                    "lost": lost_total[s], "truncated": truncated, "frames": frames_seen[s]})
    return out


def _assert_same(got, want):
    """got: one stream of _feed; want: track_ref.run of the same stream."""
    assert torch.equal(got["closed"], _i32(want["closed"]).reshape(-1, 20)), "closed records differ from the restatement"
    assert torch.equal(got["counts"], _i32(want["counts"])), f"counts differ: {got['counts'].tolist()} != {want['counts'].tolist()}"
    assert torch.equal(got["frame_counts"], _i32(want["frame_counts"])), "frame counts differ from the restatement"
    assert torch.equal(got["table"], _i32(want["table"])), "the open table differs from the restatement"
    assert torch.equal(got["plane"], _i32(want["plane"])), "the slot plane differs from the restatement"
    assert got["lost"] == want["lost"] and got["truncated"] == want["truncated"] and got["frames"] == want["frames"]


def _check(vad, maps, splits_list=None, **kwargs):
    """maps float32 [b, t, h, w] (numpy): the device against the restatement for every split -> the restatement's dicts per stream."""
    kw = _kw(**kwargs)
    maps = np.ascontiguousarray(maps, np.float32)
    t = maps.shape[1]
    x = torch.from_numpy(maps).cuda()
    want = [ref.run(m, (t,), **kw) for m in maps]
    for splits in splits_list or ((t,), (1,) * t):
        got = _feed(vad, x, splits, kw)
        for s, m in enumerate(maps):
            _assert_same(got[s], want[s] if tuple(splits) == (t,) else ref.run(m, splits, **kw))
            # any split: the same concatenated records (a call's table truncates on its own), frame counts and final state as one call
            assert want[s]["truncated"] or np.array_equal(got[s]["closed"].numpy().view(np.uint32), want[s]["closed"])
            assert np.array_equal(got[s]["frame_counts"].numpy().view(np.uint32), want[s]["frame_counts"])
            assert np.array_equal(got[s]["table"].numpy().view(np.uint32), want[s]["table"])
    return want


def _against_detect_events(vad, maps, want, kw):
    """The converted, sorted records of the restatement (= the device's, by _check) equal `metrics.detect_events` on the whole clip."""
    b, t, h, w = maps.shape
    ev = vad.metrics.detect_events(torch.from_numpy(maps).cuda(), kw["threshold"], kw["connectivity"], kw["temporal"], kw["min_duration"],
                                   kw["min_volume"], 4096)
    for s in range(b):
        kept = int(ev.counts[s, 0])
        assert kept <= 4096 and torch.equal(ev.records[s, :kept].cpu(), _i32(ref.convert(want[s]["closed"], h, w)))
        assert int(ev.counts[s, 1]) == int(want[s]["counts"][:, 1].sum())


# ------------------------------------------------------------------------------------------ 1. splits and batching
def _content(kind):
    rng = np.random.default_rng(2400 + len(kind) + int(kind[-2:]))
    if kind == "blobs00":
        mask = np.repeat(pro_ref.blobs(rng, 3, 24, 40)[:, None], 12, axis=1) & (rng.random((3, 12, 24, 40)) < 0.85)
        mask[1, 5] = False                                                    # every event of stream 1 closes once
    else:
        mask = rng.random((3, 12, 24, 40)) < int(kind[-2:]) / 100.0
    return _from_masks(2401, mask)


@pytest.mark.parametrize("kind", ("blobs00", "noise02", "noise05", "noise12"))
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_any_split_of_the_frames_gives_the_events_of_the_clip(vad, mode, kind):
    maps = _content(kind)
    kw = dict(connectivity=mode[0], temporal=mode[1], max_open=256, max_closed=1024)
    for m in maps:                                                            # the inputs are chosen so that nothing is lost or truncated
        r = ref.run(m, (12,), **_kw(**kw))
        assert r["lost"] == 0 and not r["truncated"]
    before = vad.hip.calls.get("track_events", 0)
    want = _check(vad, maps, ((12,), (1,) * 12, (5, 1, 6), (7, 5)), **kw)
    assert vad.hip.calls["track_events"] == before + 1 + 12 + 3 + 2 + 4       # every update and flush
    assert sum(len(wn["closed"]) for wn in want) >= 3
    _against_detect_events(vad, maps, want, _kw(**kw))
    if kind == "noise05":                                                     # the filters, through the same equalities
        kw.update(min_duration=2, min_volume=3)
        _against_detect_events(vad, maps, _check(vad, maps, ((12,), (5, 1, 6)), **kw), _kw(**kw))


# ------------------------------------------------------------------------------------------ 2. links in time
def test_a_pixel_moving_diagonally(vad):
    mask = np.zeros((1, 5, 9, 9), bool)
    for f in range(5):
        mask[0, f, 2 + f, 1 + f] = True
    maps = _from_masks(2410, mask)
    one = _check(vad, maps, temporal=9)[0]
    assert len(one["closed"]) == 1 and (one["closed"][0, ref.T0], one["closed"][0, ref.T1]) == (0, 4) and one["closed"][0, ref.HANDLE] == 6 * 9 + 5
    five = _check(vad, maps, temporal=1)[0]
    assert len(five["closed"]) == 5 and five["closed"][:, ref.T1].tolist() == [0, 1, 2, 3, 4]
    # an L-shaped step: (t, y, x) and (t + 1, y + 1, x + 1) with the corner pixels empty links under the 26-structure only
    step = np.zeros((1, 2, 4, 4), bool)
    step[0, 0, 1, 1] = step[0, 1, 2, 2] = True
    maps = _from_masks(2411, step)
    assert len(_check(vad, maps, temporal=9)[0]["closed"]) == 1 and len(_check(vad, maps, temporal=1)[0]["closed"]) == 2
    assert len(_check(vad, maps, connectivity=4, temporal=1)[0]["closed"]) == 2


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_merge_split_and_gap(vad, mode):
    kw = dict(connectivity=mode[0], temporal=mode[1])
    mask = np.zeros((1, 5, 8, 16), bool)
    mask[0, :, 2:4, 2:4] = True
    mask[0, 1:, 2:4, 10:12] = True
    mask[0, 3, 3, 2:12] = True                                                # a bridge in frame 3
    maps = _from_masks(2412, mask)
    maps[0, 1, 2, 10] = 9.0                                                   # the later blob holds the peak
    one = _check(vad, maps, ((5,), (1,) * 5, (3, 2)), **kw)[0]
    assert len(one["closed"]) == 1
    r = one["closed"][0]
    assert (r[ref.ROOT_PIXEL], r[ref.T0], r[ref.T1]) == (2 * 16 + 2, 0, 4) and ref._u64(r, ref.VOLUME) == 5 * 4 + 4 * 4 + 6
    assert (r[ref.PEAK_FRAME], r[ref.PEAK_PIXEL]) == (1, 2 * 16 + 10) and tuple(r[ref.X0:ref.Y1 + 1]) == (2, 2, 11, 3)
    assert one["counts"][:, 4].tolist() == [1, 0]                             # open after the call, none after the flush
    # one blob that splits: one event, handle = the smaller region's root
    mask = np.zeros((1, 3, 6, 12), bool)
    mask[0, 0, 2, 1:11] = True
    mask[0, 1:, 2, 1:3] = mask[0, 1:, 2, 8:11] = True
    one = _check(vad, _from_masks(2413, mask), **kw)[0]
    assert len(one["closed"]) == 1 and one["closed"][0, ref.HANDLE] == 2 * 12 + 1 and ref._u64(one["closed"][0], ref.VOLUME) == 10 + 2 * 5
    # one blob absent for exactly one frame: two events
    mask = np.zeros((1, 5, 6, 6), bool)
    mask[0, :, 2:4, 2:4] = True
    mask[0, 2] = False
    two = _check(vad, _from_masks(2414, mask), ((5,), (1,) * 5, (2, 1, 2)), **kw)[0]
    assert [(int(r[ref.T0]), int(r[ref.T1])) for r in two["closed"]] == [(0, 1), (3, 4)]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_neighbours_in_memory_that_are_not_neighbours(vad, mode):
    kw = dict(connectivity=mode[0], temporal=mode[1])
    # the last row and pixel of a frame against the first of the next
    mask = np.zeros((1, 2, 5, 7), bool)
    mask[0, 0, 4, :] = True
    mask[0, 1, 0, :] = True
    assert len(_check(vad, _from_masks(2415, mask), **kw)[0]["closed"]) == 2
    # the last frame of stream b against the first of stream b + 1, with identical foreground: streams never link
    mask = np.zeros((3, 2, 5, 7), bool)
    mask[:, :, 1:3, 2:5] = True
    mask[1, 0] = False
    want = _check(vad, _from_masks(2416, mask), **kw)
    assert [len(wn["closed"]) for wn in want] == [1, 1, 1] and [int(wn["closed"][0, ref.T0]) for wn in want] == [0, 1, 0]


# ------------------------------------------------------------------------------------------ 3. values
def test_nan_inf_ties_and_signed_zeros(vad):
    maps = np.zeros((1, 3, 2, 4), np.float32)
    maps[0, 0, 0, :3] = [2.0, np.nan, 2.0]                                    # a NaN cuts in space ...
    maps[0, 1, 0, 0] = np.nan                                                 # ... and in time
    maps[0, 2, 0, 0] = 2.0
    maps[0, 1, 1, 3] = np.inf
    maps[0, 2, 1, 3] = 5.0
    one = _check(vad, maps, threshold=1.0, connectivity=4, temporal=1)[0]
    assert len(one["closed"]) == 4 and int(one["counts"][:, 3].sum()) == 2 and one["frame_counts"][:, 2].tolist() == [1, 1, 0]
    last = one["closed"][-1]
    assert last[ref.PEAK].view(np.float32) == np.inf and (last[ref.PEAK_FRAME], last[ref.PEAK_PIXEL]) == (1, 7)
    # +Inf as the threshold: only +Inf is foreground; a value equal to the threshold is foreground
    assert len(_check(vad, maps, threshold=np.inf, connectivity=4, temporal=1)[0]["closed"]) == 1
    assert int(_check(vad, maps, threshold=5.0)[0]["counts"][:, 2].sum()) == 2
    # a peak tie across frames (the earliest frame) and inside a frame (the smallest pixel)
    tie = np.zeros((1, 3, 1, 4), np.float32)
    tie[0, 0, 0, 2] = 2.0
    tie[0, 1, 0, 1:4] = [3.0, 2.0, 3.0]
    tie[0, 2, 0, 0:3] = [3.0, 3.0, 2.0]
    one = _check(vad, tie, threshold=1.0, connectivity=8, temporal=1)[0]
    assert len(one["closed"]) == 1 and (one["closed"][0, ref.PEAK_FRAME], one["closed"][0, ref.PEAK_PIXEL]) == (1, 1)
    # signed zeros: +0.0 in frame 1 beats -0.0 in frame 0; the other way round the tie is none either
    for first, second, frame in ((-0.0, 0.0, 1), (0.0, -0.0, 0)):
        zeros = np.full((1, 2, 1, 2), -5.0, np.float32)
        zeros[0, 0, 0, 0], zeros[0, 1, 0, 0] = first, second
        one = _check(vad, zeros, threshold=-1.0, temporal=1)[0]
        assert one["closed"][0, ref.PEAK_FRAME] == frame and one["closed"][0, ref.PEAK] == (0 if frame == 1 or first == 0.0 else 0x80000000)


# ------------------------------------------------------------------------------------------ 4. filters and alarms
def test_filters_truncation_and_the_causal_alarm(vad):
    mask = np.zeros((1, 8, 6, 20), bool)
    mask[0, 0:5, 1:3, 1:3] = True                                             # duration 5, volume 20
    mask[0, 2:4, 4, 8] = True                                                 # duration 2, volume 2
    mask[0, 3:6, 1, 12:15] = True                                             # duration 3, volume 9
    mask[0, 6, 3, 17] = True                                                  # duration 1
    maps = _from_masks(2420, mask)
    for min_duration, min_volume, max_closed in ((1, 1, 8), (2, 1, 8), (3, 1, 8), (4, 1, 8), (5, 1, 8), (6, 1, 8), (1, 2, 8), (1, 3, 8), (1, 9, 8),
                                                 (1, 10, 8), (1, 20, 8), (1, 21, 8), (3, 9, 8), (1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 2, 1)):
        one = _check(vad, maps, ((8,), (1,) * 8, (3, 5)), min_duration=min_duration, min_volume=min_volume, max_closed=max_closed)[0]
        full = ref.run(maps[0], (8,), **_kw(min_duration=min_duration, min_volume=min_volume, max_closed=64))
        # the causal word is unchanged by max_closed
        assert np.array_equal(one["frame_counts"], full["frame_counts"]) and int(one["counts"][:, :2].sum()) == 4
    # the alarm begins exactly in the frame in which the duration is reached; an event that closes below it never alarmed
    one = _check(vad, maps, min_duration=3)[0]
    assert one["frame_counts"][:, 1].tolist() == [0, 0, 4, 4, 4, 3, 0, 0]
    # volume so far: the 2 x 2 block passes 9 pixels in its third frame (12), the row of three reaches them in its third (frame 5)
    assert _check(vad, maps, min_volume=9)[0]["frame_counts"][:, 1].tolist() == [0, 0, 4, 4, 4, 3, 0, 0]


# ------------------------------------------------------------------------------------------ 5. lost events
def test_lost_events_are_counted_and_the_tracked_ones_exact(vad):
    mask = np.zeros((2, 5, 6, 12), bool)
    mask[0, :, 1, 1] = mask[0, :, 3, 5:7] = mask[0, :, 4, 10] = True          # three simultaneous events against max_open = 2
    mask[0, 3:, 1, 1] = False                                                 # from frame 3 on the third has a slot: an event with t0 = 3
    mask[1, :, 2, 2] = True                                                   # the neighbour stream is untouched
    maps = _from_masks(2430, mask)
    want = _check(vad, maps, ((5,), (1,) * 5, (2, 3)), max_open=2)
    assert want[0]["lost"] == 3 and want[0]["counts"][:, 5].tolist() == [3, 0] and want[1]["lost"] == 0
    got = ref.convert(want[0]["closed"], 6, 12)
    assert got[:, events_ref.ROOT].tolist() == [13, 3 * 12 + 5, 3 * 72 + 4 * 12 + 10] and got[:, events_ref.VOLUME].tolist() == [3, 10, 2]
    # an old record that continues behind the table goes with it
    mask = np.zeros((1, 2, 1, 5), bool)
    mask[0, 0, 0, 4] = mask[0, 1, 0, 0] = mask[0, 1, 0, 4] = True
    one = _check(vad, _from_masks(2431, mask), max_open=1)[0]
    assert one["lost"] == 1 and int(one["counts"][:, :2].sum()) == 1 and one["closed"][0, ref.T0] == 1


# ------------------------------------------------------------------------------------------ 6. shapes and state
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_dense_stream_is_one_event(vad, mode):
    maps = np.full((1, 8, 64, 64), 1.0, np.float32)
    one = _check(vad, maps, ((8,), (3, 5)), connectivity=mode[0], temporal=mode[1])[0]
    assert len(one["closed"]) == 1 and ref._u64(one["closed"][0], ref.VOLUME) == 8 * 4096 and ref._u64(one["closed"][0], ref.SUM_T) == 28 * 4096


def test_a_sparse_frame_beyond_one_grid_round_of_every_pass(vad):
    lib = vad.hip.lib()
    out = [vad.hip.C.c_int(0) for _ in range(5)]
    assert lib.vad_track_plan(*[vad.hip.C.byref(v) for v in out]) == 0
    h, w = 520, 520
    assert max(out[1].value, out[2].value) < h * w <= out[0].value
    mask = np.zeros((1, 3, h, w), bool)
    mask[0, :, 0, 0] = mask[0, :, h - 1, w - 1] = True                        # the first and the last pixel
    mask[0, 1:, 300:303, 400:460] = True
    mask[0, 0, 517, 3] = mask[0, 1, 518, 4] = mask[0, 2, 519, 5] = True       # a diagonal walk in the last rows
    rng = np.random.default_rng(2440)
    mask[0, 1][rng.random((h, w)) < 0.0005] = True
    want = _check(vad, _from_masks(2441, mask), ((3,), (1, 1, 1)), max_open=1024, max_closed=1024)[0]
    assert want["lost"] == 0 and not want["truncated"] and int(want["table"][0, ref.HANDLE]) == 0 and int(want["plane"][h * w - 1]) != 0


def test_odd_shapes(vad):
    rng = np.random.default_rng(2450)
    for shape in ((1, 6, 1, 131), (2, 6, 77, 1), (2, 4, 1, 1), (1, 5, 3, 67), (1, 4, 37, 53)):
        maps = _from_masks(2451, rng.random(shape) < 0.35)
        for mode in MODES:
            _check(vad, maps, connectivity=mode[0], temporal=mode[1], max_open=2048, max_closed=2048)


def test_three_hundred_calls_of_one_frame(vad):
    """One event that never closes: the frame counter lives on the device; volume and sum_t to the word."""
    mask = np.zeros((1, 300, 16, 16), bool)
    mask[0, :, 4:9, 5:8] = True
    mask[0, ::7, 12, 12] = True                                               # flicker: single-frame events
    maps = _from_masks(2460, mask)
    kw = _kw(min_duration=2)
    got = _feed(vad, torch.from_numpy(maps).cuda(), (1,) * 300, kw)[0]
    _assert_same(got, ref.run(maps[0], (1,) * 300, **kw))
    last = got["closed"][-1].numpy().view(np.uint32)
    assert got["frames"] == 300 and ref._u64(last, ref.VOLUME) == 300 * 15 and ref._u64(last, ref.SUM_T) == 15 * (299 * 300 // 2)
    assert (last[ref.T0], last[ref.T1]) == (0, 299) and int(got["counts"][:, 1].sum()) == 43 and got["frame_counts"][1:, 1].eq(15).all()


# ------------------------------------------------------------------------------------------ 7. layout and reset
def test_any_batching_layout_and_reset(vad):
    rng = np.random.default_rng(2470)
    mask = np.repeat(pro_ref.blobs(rng, 4, 24, 40)[:, None], 6, axis=1) & (rng.random((4, 6, 24, 40)) < 0.8)
    maps = _from_masks(2471, mask)
    kw = _kw(min_duration=2)
    x = torch.from_numpy(maps).cuda()
    whole = _feed(vad, x, (4, 2), kw)
    for s in range(4):                                                        # stream by stream
        _assert_same(whole[s], ref.run(maps[s], (4, 2), **kw))
        alone = _feed(vad, x[s:s + 1], (4, 2), kw)[0]
        assert all(torch.equal(alone[k], whole[s][k]) for k in ("closed", "counts", "frame_counts", "table", "plane"))
    flipped = _feed(vad, x.flip(0), (4, 2), kw)                               # in reverse order (a strided view, made contiguous)
    assert all(torch.equal(flipped[3 - s][k], whole[s][k]) for s in range(4) for k in ("closed", "counts", "frame_counts", "table", "plane"))
    # maps one float off their allocation, 5-D, strided in time, and [B,H,W] for one new map
    arena = torch.zeros(x.numel() + 1, device="cuda")
    off = arena[1:].view_as(x).copy_(x)
    assert off.data_ptr() % 8 == 4
    wide = torch.zeros(4, 12, 24, 40, device="cuda")
    wide[:, ::2] = x
    for other in (_feed(vad, off, (4, 2), kw), _feed(vad, x[:, :, None], (4, 2), kw), _feed(vad, wide[:, ::2], (4, 2), kw)):
        assert all(torch.equal(other[s][k], whole[s][k]) for s in range(4) for k in ("closed", "counts", "frame_counts", "table", "plane"))
    tr = vad.metrics.EventTracker(4, 24, 40, **kw)
    ups = [tr.update(x[:, f]) for f in range(3)]                              # [B,H,W]
    assert tuple(ups[0].frame_counts.shape) == (4, 1, 3) and tuple(ups[0].alarms().shape) == (4, 1)
    # reset of one stream in the middle: that stream starts again at frame 0, the others go on
    tr.reset(streams=[2])
    assert tr.frames_seen.cpu().tolist() == [3, 3, 0, 3] and not tr.slot_plane[2].any() and not tr.open_events().records[2].any()
    rest = _feed(vad, x[:, 3:], (3,), kw, tracker=tr)
    assert torch.equal(rest[2]["closed"], _i32(ref.run(maps[2, 3:], (3,), **kw)["closed"]).reshape(-1, 20))
    assert torch.equal(torch.cat([u.frame_counts[0].cpu() for u in ups] + [rest[0]["frame_counts"]]), whole[0]["frame_counts"])
    assert rest[0]["frames"] == 6 and rest[2]["frames"] == 3
    tr.reset()
    assert not tr.state.view(4, -1)[:, :4].any() and not tr.slot_plane.any()
    # views and the host table
    up = vad.metrics.EventTracker(4, 24, 40, **_kw()).update(x)
    rows = up.to_list()
    assert len(rows) == 4 and len(rows[0]) == min(int(up.counts[0, 0]), 64)
    if rows[0]:
        r = rows[0][0]
        assert r["duration"] == r["t1"] - r["t0"] + 1 == int(up.durations()[0, 0]) and r["volume"] == int(up.volume[0, 0])
        assert r["peak"] == float(up.peak[0, 0]) and abs(r["centroid_tyx"][2] - float(up.centroids()[0, 0, 2])) < 1e-12


def test_refusals(vad):
    tr = vad.metrics.EventTracker(2, 8, 8, 0.5)
    with pytest.raises(vad.hip.VadError, match="no CPU fallback"):
        tr.update(torch.zeros(2, 8, 8))
    with pytest.raises(vad.hip.VadError, match="do not match the tracker's state"):
        tr.update(torch.zeros(2, 8, 9, device="cuda"))
    with pytest.raises(vad.hip.VadError, match="do not match the tracker's state"):
        tr.update(torch.zeros(3, 1, 8, 8, device="cuda"))
    with pytest.raises(vad.hip.VadError, match="float32"):
        tr.update(torch.zeros(2, 8, 8, device="cuda", dtype=torch.float64))
    with pytest.raises(vad.hip.VadError, match=r"\[B,H,W\], \[B,T,H,W\] or \[B,T,1,H,W\]"):
        tr.update(torch.zeros(2, 1, 2, 8, 8, device="cuda"))
    with pytest.raises(vad.hip.VadError, match="at least one new map"):
        tr.update(torch.zeros(2, 0, 8, 8, device="cuda"))
    with pytest.raises(vad.hip.VadError, match="out of range"):
        tr.reset(streams=[2])
    assert tr.frames_seen.cpu().tolist() == [0, 0] and tr.flags() == 0


# ------------------------------------------------------------------------------------------ 8. the C ABI on the device
def test_c_abi_with_poisoned_and_guarded_state_and_workspace(vad):
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    rng = np.random.default_rng(2480)
    mask = np.repeat(pro_ref.blobs(rng, 3, 24, 40)[:, None], 4, axis=1) & (rng.random((3, 4, 24, 40)) < 0.8)
    mask[1] = False
    mask[2, 2] = False
    maps_np = _from_masks(2481, mask)
    b, t, h, w = maps_np.shape
    max_open, max_closed = 32, 8
    kw = _kw(min_duration=2, min_volume=2, max_open=max_open, max_closed=max_closed)
    maps = torch.from_numpy(maps_np).cuda()
    G = 256

    def guarded(nbytes, fill):
        whole = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device="cuda")
        return whole, whole[G:G + nbytes]

    def intact(whole, fill):
        return bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all())

    state_bytes = lib.vad_track_state_bytes(b, h, w, max_open)
    need, need0 = lib.vad_track_workspace_bytes(b, 2, h, w, max_open), lib.vad_track_workspace_bytes(b, 0, h, w, max_open)
    assert state_bytes == b * (64 + 80 * max_open + 4 * h * w) and need0 < need
    bufs = {"state": guarded(state_bytes, 0xAB), "ws": guarded(need, 0xAB), "ws0": guarded(need0, 0xAB), "closed": guarded(b * max_closed * 80, 0xF9),
            "counts": guarded(b * 24, 0xF9), "frames": guarded(b * 2 * 12, 0xF9)}
    ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
    assert all(ptr[k] % 16 == 0 for k in ("state", "ws", "ws0", "closed"))
    assert lib.vad_track_init(ptr["state"], b, h, w, max_open, stream) == 0, lib.vad_last_error()
    words = bufs["state"][1].view(torch.int32).view(b, -1)
    assert words[:, :4].cpu().tolist() == [[0, 0, 0, 0]] * b and words[:, 5:8].cpu().tolist() == [[h, w, max_open]] * b and not words[:, 8:].any()
    want = [ref.Tracker(h, w, **kw) for _ in range(b)]
    for at in (0, 2):
        rc = lib.vad_track_events(maps[:, at:at + 2].contiguous().data_ptr(), b, 2, h, w, float(T), 8, 9, 2, 2, max_open, max_closed, ptr["state"],
                                  ptr["closed"], ptr["counts"], ptr["frames"], ptr["ws"], need, stream)
        assert rc == 0, lib.vad_last_error()
        torch.cuda.synchronize()
        assert int(bufs["ws"][1][:4].view(torch.int32).item()) == 0
        for s in range(b):
            closed, counts, frames = want[s].update(maps_np[s, at:at + 2])
            assert torch.equal(bufs["closed"][1].view(torch.int32).view(b, max_closed, 20)[s].cpu(), _i32(closed))
            assert torch.equal(bufs["counts"][1].view(torch.int32).view(b, 6)[s].cpu(), _i32(counts))
            assert torch.equal(bufs["frames"][1].view(torch.int32).view(b, 2, 3)[s].cpu(), _i32(frames))
            assert torch.equal(words[s, 16:16 + 20 * max_open].cpu().view(max_open, 20), _i32(want[s].open_table()))
            assert torch.equal(words[s, 16 + 20 * max_open:].cpu(), _i32(want[s].plane))
            assert words[s, :4].cpu().tolist() == [at + 2, len(want[s].table), 0, 0]
    before = [bufs[k][1].clone() for k in ("state", "closed", "counts", "frames")]
    common = (maps.data_ptr(), b, 2, h, w, float(T), 8, 9, 2, 2, max_open, max_closed, ptr["state"], ptr["closed"], ptr["counts"], ptr["frames"], ptr["ws"])
    # a short workspace, b == 0 and refused arguments: nothing but the flag word is touched
    assert lib.vad_track_events(*common, need - 1, stream) == -3 and b"ws_bytes" in lib.vad_last_error()
    bufs["ws"][1].fill_(0xAB)
    assert lib.vad_track_events(maps.data_ptr(), 0, 2, h, w, float(T), 8, 9, 2, 2, max_open, max_closed, *common[12:], 16, stream) == 0
    torch.cuda.synchronize()
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == 0 and bool((bufs["ws"][1][16:] == 0xAB).all())
    for pos, bad, word in ((5, float("nan"), b"threshold is NaN"), (6, 4, b"temporal 9 needs connectivity 8"), (2, 0, b"t must"), (10, 0, b"max_open"),
                           (11, 65537, b"max_closed"), (8, 0, b"min_duration"), (9, 0, b"min_volume"), (12, None, b"state is NULL")):
        args = list(common) + [need, stream]
        args[pos] = bad
        assert lib.vad_track_events(*args) == -1 and word in lib.vad_last_error(), (pos, bad)
    torch.cuda.synchronize()
    assert all(torch.equal(a, bufs[k][1]) for a, k in zip(before, ("state", "closed", "counts", "frames")))
    # the flush: its own, smaller workspace
    assert lib.vad_track_flush(b, h, w, 2, 2, max_open, max_closed, ptr["state"], ptr["closed"], ptr["counts"], ptr["ws0"], need0 - 1, stream) == -3
    assert lib.vad_track_flush(b, h, w, 2, 2, max_open, max_closed, ptr["state"], ptr["closed"], ptr["counts"], ptr["ws0"], need0, stream) == 0
    torch.cuda.synchronize()
    for s in range(b):
        closed, counts = want[s].flush()
        assert torch.equal(bufs["closed"][1].view(torch.int32).view(b, max_closed, 20)[s].cpu(), _i32(closed))
        assert torch.equal(bufs["counts"][1].view(torch.int32).view(b, 6)[s].cpu(), _i32(counts))
        assert words[s, :4].cpu().tolist() == [4, 0, 0, 0] and not words[s, 16:].any()
    assert all(intact(v[0], 0xAB if k in ("state", "ws", "ws0") else 0xF9) for k, v in bufs.items()), "a guard was written"
    assert bool((bufs["frames"][1].view(torch.int32).view(b, 2, 3).cpu() == _i32(before[3].cpu().numpy()).view(b, 2, 3)).all())    # a flush leaves frame_counts alone


# ------------------------------------------------------------------------------------------ 9. capture
def test_a_captured_call_counts_its_frames_on_the_device(vad):
    """A T = 1 call captured once and replayed on six new contents equals six eager calls: the host passes no frame number."""
    rng = np.random.default_rng(2490)
    mask = np.repeat(pro_ref.blobs(rng, 2, 24, 40)[:, None], 7, axis=1) & (rng.random((2, 7, 24, 40)) < 0.8)
    mask[0, 4] = False
    maps_np = _from_masks(2491, mask)
    kw = _kw(min_duration=2)
    contents = torch.from_numpy(maps_np).cuda()
    eager = vad.metrics.EventTracker(2, 24, 40, **kw)
    want = [eager.update(contents[:, f]) for f in range(7)]
    tr = vad.metrics.EventTracker(2, 24, 40, **kw)
    maps = contents[:, 0].clone()
    tr.update(maps)                                                           # frame 0, eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            up = tr.update(maps)
    torch.cuda.current_stream().wait_stream(side)
    assert tr.frames_seen.cpu().tolist() == [1, 1]                            # a capture runs nothing
    for f in range(1, 7):
        maps.copy_(contents[:, f])
        graph.replay()
        torch.cuda.synchronize()
        assert tr.frames_seen.cpu().tolist() == [f + 1, f + 1]
        assert torch.equal(up.counts, want[f].counts), (f, up.counts.tolist(), want[f].counts.tolist())
        assert torch.equal(up.frame_counts, want[f].frame_counts), (f, up.frame_counts.tolist(), want[f].frame_counts.tolist())
        assert torch.equal(up.records, want[f].records), f
    assert tr.flags() == 0 and torch.equal(tr.state, eager.state)
    one = ref.run(maps_np[0], (1,) * 7, **kw)
    assert torch.equal(tr.open_events().records[0].cpu(), _i32(one["table"])) and int(sum(int(u.counts[0, 0]) for u in want)) == int(one["counts"][:-1, 0].sum())


# ------------------------------------------------------------------------------------------ 10. through the models
def _threshold_of(vad, maps, fpr=0.05):
    h, w = maps.shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w]
    lab = torch.from_numpy((((yy // 8) + (xx // 8)) % 2).astype(np.uint8) * 255).cuda().expand(maps.shape).contiguous()
    hist = vad.metrics.ScoreHistogram(11).accumulate(maps, lab)
    t, tpr, reached = vad.metrics.threshold_at_fpr(hist.counts_host(), fpr)
    assert np.isfinite(t) and reached <= fpr
    return t


@pytest.mark.parametrize("sigma", (None, 1.0))
def test_localize_stream_through_the_video_model(vad, sigma):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 6, 3, 32, 32)).cuda()
    with torch.no_grad():
        whole = model.score_stateful(clips, None, errmap=True)["errmap"]
        if sigma is not None:
            whole = vad.metrics.smooth_maps(whole, sigma, 4.0)
        t = _threshold_of(vad, whole)
    kw = _kw(threshold=t, temporal=1, min_duration=2, max_open=512, max_closed=256)
    tracker, by_hand = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    state, state2, got, maps_seen = None, None, [], []
    for f in range(6):
        before = {k: vad.hip.calls.get(k, 0) for k in ("track_events", "vid_score_stateful", "smooth_maps")}
        up, maps, state = vad.scoring.localize_stream(model, clips[:, f:f + 1], tracker, state, sigma=sigma)
        assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [1, 1, int(sigma is not None)]
        assert tuple(maps.shape) == (2, 1, 1, 32, 32) and tuple(up.frame_counts.shape) == (2, 1, 3)
        with torch.no_grad():
            out = model.score_stateful(clips[:, f:f + 1], state2, errmap=True)
            state2, m = out["state"], out["errmap"]
            m = vad.metrics.smooth_maps(m, sigma, 4.0) if sigma is not None else m
        want = by_hand.update(m)
        assert torch.equal(maps, m) and torch.equal(up.records, want.records) and torch.equal(up.counts, want.counts)
        assert torch.equal(up.frame_counts, want.frame_counts)
        got.append(up)
        maps_seen.append(maps)
    assert torch.equal(tracker.state, by_hand.state)
    got.append(tracker.flush())
    volume = torch.cat(maps_seen, dim=1)                                      # [2, 6, 1, 32, 32]: the maps the calls returned
    ev = vad.metrics.detect_events(volume, t, 8, 1, 2, 1, 4096)
    total = 0
    for s in range(2):
        closed = np.concatenate([u.records[s, :min(int(u.counts[s, 0]), 256)].cpu().numpy().view(np.uint32) for u in got])
        assert all(int(u.counts[s, 0]) <= 256 and int(u.counts[s, 5]) == 0 for u in got)
        kept = int(ev.counts[s, 0])
        assert torch.equal(ev.records[s, :kept].cpu(), _i32(ref.convert(closed, 32, 32)))
        assert sum(int(u.counts[s, 1]) for u in got) == int(ev.counts[s, 1])
        one = ref.run(volume[s, :, 0].cpu().numpy(), (1,) * 6, **kw)
        assert np.array_equal(closed, one["closed"])
        assert torch.equal(torch.cat([u.frame_counts[s].cpu() for u in got]), _i32(one["frame_counts"]))
        total += int(ev.counts[s, 2])
    print(f"video sigma {sigma}: threshold {t!r} kept {ev.counts[:, 0].tolist()} dropped {ev.counts[:, 1].tolist()}")
    assert total > 0


@pytest.mark.parametrize("calibrated", (False, True))
def test_localize_stream_through_the_image_model(vad, calibrated):
    """The newest frame of two cameras per call: consecutive synthetic frames, one tracker stream per camera."""
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 12, 3, 32, 32)).cuda().view(2, 6, 3, 32, 32)
    stats = vad.scoring.calibrate(model, [{"image": x.view(12, 3, 32, 32)}], "cuda", map="mse", sigma=1.0) if calibrated else None
    min_std = vad.metrics.DEFAULT_MIN_STD if calibrated else None
    with torch.no_grad():
        whole = vad.scoring._anomaly_maps(model, x.view(12, 3, 32, 32), "mse", 1.0, 4.0, stats, min_std).view(2, 6, 32, 32)
    t = 1.0 if calibrated else _threshold_of(vad, whole)
    kw = _kw(threshold=t, connectivity=4, temporal=1, min_volume=2, max_open=512, max_closed=256)
    tracker = vad.metrics.EventTracker(2, 32, 32, **kw)
    got = []
    for f in range(6):
        before = {k: vad.hip.calls.get(k, 0) for k in ("track_events", "img_score", "smooth_maps")}
        up, maps, state = vad.scoring.localize_stream(model, x[:, f], tracker, sigma=1.0, calibration=stats)
        assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [1, 1, 1] and state is None
        assert tuple(maps.shape) == (2, 1, 32, 32) and torch.equal(maps[:, 0], whole[:, f])
        got.append(up)
    got.append(tracker.flush())
    for s in range(2):
        one = ref.run(whole[s].cpu().numpy(), (1,) * 6, **kw)
        assert one["lost"] == 0 and not one["truncated"]
        closed = torch.cat([u.records[s, :int(u.counts[s, 0])].cpu() for u in got])
        assert torch.equal(closed, _i32(one["closed"]).reshape(-1, 20))
        assert torch.equal(torch.cat([u.frame_counts[s].cpu() for u in got]), _i32(one["frame_counts"]))
        assert torch.equal(torch.stack([u.counts[s].cpu() for u in got]), _i32(one["counts"]))
        print(f"image calibrated {calibrated} stream {s}: threshold {t!r} kept {int(one['counts'][:, 0].sum())} alarms {one['frame_counts'][:, 1].tolist()}")
    assert int(sum(int(u.counts[:, 2].sum()) for u in got)) > 0
    with pytest.raises(vad.hip.VadError, match="carries no state"):
        vad.scoring.localize_stream(model, x[:, 0], tracker, state=object())
