"""Anomaly events of a clip on the GPU (csrc/map_events.hip, metrics.detect_events, scoring.localize_events): records, counts, frame
counts and labels `torch.equal` to the numpy restatement (tests/events_ref.py) - on one frame against `detect_regions`, on the links
in time that a wrong linker gets wrong (frame, row and clip boundaries, merges and splits), on ties and non-finite pixels, every
filter and truncation, volumes larger than one grid round of every pass, any batching, the raw C ABI with a poisoned and guarded
workspace, a captured call, and through both seeded models."""
import ctypes

import numpy as np
import pytest
import torch

import events_ref as ref
import pro_ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
MODES = ((4, 1), (8, 1), (8, 9))
MODE_IDS = [f"c{c}t{t}" for c, t in MODES]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _assert_table(got, want, labels=True):
    """got: metrics.Events; want: (records, counts, frame_counts, labels) of the restatement."""
    records, counts, frames, lab = want
    assert got.records.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.frame_counts.dtype == torch.int32
    assert torch.equal(got.records.cpu().reshape(records.shape), _i32(records)), "records differ from the restatement"
    assert torch.equal(got.counts.cpu().reshape(counts.shape), _i32(counts)), "counts differ from the restatement"
    assert torch.equal(got.frame_counts.cpu().reshape(frames.shape), _i32(frames)), "frame counts differ from the restatement"
    if labels:
        assert torch.equal(got.labels.cpu().reshape(lab.shape), torch.from_numpy(lab)), "labels differ from the restatement"


def _run_and_check(vad, maps, t=T, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_events=64):
    """maps: float32 [b, t, h, w]"""
    want = ref.detect_batch(maps, t, connectivity, temporal, min_duration, min_volume, max_events)
    got = vad.metrics.detect_events(torch.from_numpy(maps).cuda(), float(t), connectivity, temporal, min_duration, min_volume, max_events,
                                    return_labels=True)                      # raises on a set flag word
    _assert_table(got, want)
    return got, want


def _from_masks(seed, mask):
    """mask bool [b, t, h, w] -> a map whose foreground under T is the mask (the value T itself among the foreground)."""
    return ref.map_from_mask(np.random.default_rng(seed), np.asarray(mask, bool), T)


def _roots(want, clip=0):
    return want[0][clip, :min(int(want[1][clip, 0]), want[0].shape[1]), ref.ROOT].tolist()


# ------------------------------------------------------------------------------------------ one frame is the region table
@pytest.mark.parametrize("connectivity", (4, 8))
def test_one_frame_equals_detect_regions(vad, connectivity):
    rng = np.random.default_rng(200)
    maps = _from_masks(201, pro_ref.blobs(rng, 3, 48, 80, count=8)[:, None])     # [3, 1, 48, 80]
    x = torch.from_numpy(maps).cuda()
    before = vad.hip.calls.get("detect_events", 0)
    for temporal in ((1,) if connectivity == 4 else (1, 9)):
        ev = vad.metrics.detect_events(x, float(T), connectivity, temporal, 1, 2, 16, return_labels=True)
        rg = vad.metrics.detect_regions(x[:, 0], float(T), connectivity, 2, 16, return_labels=True)
        assert tuple(ev.records.shape) == (3, 16, 16) and tuple(ev.frame_counts.shape) == (3, 1, 3) and tuple(ev.labels.shape) == (3, 1, 48, 80)
        assert int(rg.counts[:, 0].min()) >= 2
        assert torch.equal(ev.root, rg.root) and torch.equal(ev.volume, rg.area) and torch.equal(ev.box, rg.box)
        assert torch.equal(ev.peak.view(torch.int32), rg.peak.view(torch.int32)) and torch.equal(ev.peak_index, rg.peak_index)
        assert torch.equal(ev.sum_x, rg.sum_x) and torch.equal(ev.sum_y, rg.sum_y)
        assert not ev.t0.any() and not ev.t1.any() and not ev.sum_t.any()
        assert torch.equal(ev.counts, rg.counts) and torch.equal(ev.labels[:, 0], rg.labels)
        assert torch.equal(ev.frame_counts[:, 0, 0], rg.counts[:, 2]) and not ev.frame_counts[:, 0, 2].any()
        _assert_table(ev, ref.detect_batch(maps, T, connectivity, temporal, 1, 2, 16))
    assert vad.hip.calls["detect_events"] == before + (1 if connectivity == 4 else 2)


# ------------------------------------------------------------------------------------------ links in time
def test_a_pixel_moving_diagonally(vad):
    mask = np.zeros((1, 5, 9, 9), bool)
    for f in range(5):
        mask[0, f, 2 + f, 1 + f] = True
    maps = _from_masks(202, mask)
    got, want = _run_and_check(vad, maps, T, 8, 9)
    assert want[1][0].tolist() == [1, 0, 5, 0] and want[0][0, 0, :8].tolist() == [2 * 9 + 1, 5, 0, 4, 1, 2, 5, 6]
    assert got.durations()[0, :2].tolist() == [5, 0] and got.alarms().tolist() == [[True] * 5]
    got, want = _run_and_check(vad, maps, T, 8, 1)
    assert want[1][0].tolist() == [5, 0, 5, 0] and _roots(want) == [f * 81 + (2 + f) * 9 + 1 + f for f in range(5)]
    assert got.durations()[0, :5].tolist() == [1] * 5
    # an L-shaped step - one pixel sideways and one frame on - links under the 26-structure only ...
    step = np.zeros((1, 2, 5, 5), bool)
    step[0, 0, 2, 2] = step[0, 1, 2, 3] = True
    for (connectivity, temporal), events in zip(MODES, (2, 2, 1)):
        _, want = _run_and_check(vad, _from_masks(203, step), T, connectivity, temporal)
        assert want[1][0, 0] == events
    # ... unless the corner of the L is set
    step[0, 0, 2, 3] = True
    for connectivity, temporal in MODES:
        _, want = _run_and_check(vad, _from_masks(204, step), T, connectivity, temporal)
        assert want[1][0].tolist() == [1, 0, 3, 0]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_neighbours_in_memory_that_are_not_neighbours(vad, mode):
    connectivity, temporal = mode
    rows = np.zeros((1, 3, 4, 6), bool)
    rows[0, 0, 3, :] = rows[0, 1, 0, :] = True                                # the last row of a frame, the first row of the next
    rows[0, 2, 0, 2:4] = True                                                 # and the same pixels one frame on: these do link
    got, want = _run_and_check(vad, _from_masks(205, rows), T, connectivity, temporal)
    assert want[1][0].tolist() == [2, 0, 14, 0] and _roots(want) == [18, 24]
    assert want[0][0, 1, ref.VOLUME] == 8 and want[0][0, 1, ref.T0:ref.T1 + 1].tolist() == [1, 2]
    ends = np.zeros((1, 3, 4, 6), bool)
    ends[0, 0, 3, 5] = ends[0, 1, 0, 0] = ends[0, 2, 3, 5] = True             # the last pixel of a frame, the first pixel of the next
    got, want = _run_and_check(vad, _from_masks(206, ends), T, connectivity, temporal)
    assert want[1][0].tolist() == [3, 0, 3, 0] and _roots(want) == [23, 24, 71]
    # the last frame of a clip and the first frame of the next clip, with identical foreground
    rng = np.random.default_rng(207)
    clips = np.zeros((3, 2, 12, 20), bool)
    clips[:, 0] = pro_ref.blobs(rng, 3, 12, 20, count=3, radius=3)
    clips[0, 1] = clips[1, 0] = clips[1, 1] = clips[2, 0] = pro_ref.blobs(rng, 1, 12, 20, count=3, radius=3)[0]
    maps = _from_masks(208, clips)
    got, want = _run_and_check(vad, maps, T, connectivity, temporal)
    assert want[1][:, 0].min() >= 1 and (want[0][:, :, ref.T1] <= 1).all()
    for b in range(3):
        alone, _ = _run_and_check(vad, maps[b:b + 1], T, connectivity, temporal)
        assert torch.equal(alone.records[0], got.records[b]) and torch.equal(alone.labels[0], got.labels[b])


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_merge_and_split_in_time(vad, mode):
    connectivity, temporal = mode
    merge = np.zeros((1, 5, 10, 24), bool)
    merge[0, :, 2:5, 2:6] = merge[0, :, 3:6, 15:20] = True                    # two blobs apart ...
    merge[0, 3, 4, 2:20] = True                                               # ... joined by a bar in frame 3
    got, want = _run_and_check(vad, _from_masks(209, merge), T, connectivity, temporal)
    assert want[1][0, :2].tolist() == [1, 0] and want[0][0, 0, :8].tolist() == [2 * 24 + 2, int(merge.sum()), 0, 4, 2, 2, 19, 5]
    split = merge[:, ::-1].copy()                                             # joined in frame 1, apart afterwards: still one event
    split[0, 0] = False
    split[0, 0, 2:5, 2:6] = True
    got, want = _run_and_check(vad, _from_masks(210, split), T, connectivity, temporal)
    assert want[1][0, :2].tolist() == [1, 0] and want[0][0, 0, ref.T0:ref.T1 + 1].tolist() == [0, 4]
    gap = np.zeros((1, 5, 10, 24), bool)
    gap[0, [0, 1, 3, 4], 2:5, 2:6] = True                                     # absent for exactly one frame: two events
    got, want = _run_and_check(vad, _from_masks(211, gap), T, connectivity, temporal)
    assert want[1][0, :2].tolist() == [2, 0] and want[0][0, :2, ref.T0:ref.T1 + 1].tolist() == [[0, 1], [3, 4]]
    assert got.alarms().tolist() == [[True, True, False, True, True]]
    got, want = _run_and_check(vad, _from_masks(211, gap), T, connectivity, temporal, min_duration=3)
    assert want[1][0, :2].tolist() == [0, 2] and not got.alarms().any()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("density", (0.08, 0.3, 0.6))
def test_random_volumes(vad, mode, density):
    """Noise at three densities - isolated voxels, percolating clusters, mostly foreground - on a width that is no multiple of a
    wave, with every filter in use."""
    connectivity, temporal = mode
    rng = np.random.default_rng(212 + int(100 * density))
    maps = _from_masks(213, rng.random((3, 6, 19, 37)) < density)
    _run_and_check(vad, maps, T, connectivity, temporal)
    _, want = _run_and_check(vad, maps, T, connectivity, temporal, 2, 3, 5)
    assert density > 0.5 or want[1][:, 1].min() >= 1                        # the densest volume may be one event


# ------------------------------------------------------------------------------------------ non-finite pixels, ties
def test_nan_inf_ties_and_signed_zeros(vad):
    rng = np.random.default_rng(214)
    vol = ref.map_from_mask(rng, np.zeros((4, 10, 30), bool), T)
    vol[:, 3:7, 4:24] = 1.0 + rng.random((4, 4, 20), dtype=np.float32)         # one bar through all frames ...
    vol[:, 3:7, 13] = np.nan                                                  # ... cut in space by a NaN column
    vol[2, 3:7, 14:24] = np.nan                                               # and its right half cut in time by a NaN plane
    vol[0, 0, 0] = np.nan
    vol[3, 5, 20] = np.inf                                                    # +Inf is a peak
    vol[1, 8, 2:5] = T                                                        # exactly the threshold
    vol[1, 9, 10:14] = np.nextafter(T, np.float32(0))                         # one ulp below: background
    for connectivity, temporal in MODES:
        got, want = _run_and_check(vad, vol[None], T, connectivity, temporal)
        assert want[1][0].tolist() == [4, 0, 4 * 4 * 9 + 3 * 4 * 10 + 3, 4 * 4 + 4 * 10 + 1]
        assert want[0][0, :4, ref.T0:ref.T1 + 1].tolist() == [[0, 3], [0, 1], [1, 1], [3, 3]]
        assert want[0][0, 3, ref.PEAK] == 0x7F800000 and want[0][0, 3, ref.PEAK_INDEX] == 3 * 300 + 5 * 30 + 20
        assert want[0][0, 2, ref.PEAK] == T.view(np.uint32) and want[2][0, :, 2].tolist() == [5, 4, 44, 4]
    got, want = _run_and_check(vad, vol[None], np.inf)                        # +Inf is foreground at every threshold
    assert want[1][0].tolist() == [1, 0, 1, 57]
    _run_and_check(vad, vol[None], -np.inf, 4, 1)                             # every pixel but the NaNs
    tie = np.full((3, 4, 70), -2.0, np.float32)
    tie[:, 1:3, 2:68] = 1.0
    tie[2, 1, 5] = tie[1, 2, 66] = tie[1, 1, 40] = 7.5                        # the maximum in two frames: the smallest volume index
    got, want = _run_and_check(vad, tie[None], 0.5)
    assert want[0][0, 0, ref.PEAK_INDEX] == 280 + 70 + 40 and got.peak[0, 0].item() == 7.5
    zeros = np.full((3, 2, 5), -5.0, np.float32)
    zeros[0, 0, 1:4] = [-0.0, -0.5, -0.0]
    zeros[1, 0, 1:4] = [-0.0, 0.0, 0.0]
    zeros[2, 0, 1] = -0.0
    got, want = _run_and_check(vad, zeros[None], -1.0)
    assert want[0][0, 0, ref.PEAK] == 0 and want[0][0, 0, ref.PEAK_INDEX] == 10 + 2          # the first +0.0, not the first -0.0
    zeros[1, 0, 2:4] = -0.0
    got, want = _run_and_check(vad, zeros[None], -1.0)
    assert want[0][0, 0, ref.PEAK] == 0x80000000 and want[0][0, 0, ref.PEAK_INDEX] == 1 and np.signbit(got.peak[0, 0].item())


# ------------------------------------------------------------------------------------------ the filters and the truncation
def test_filters_truncation_and_the_alarm_signal(vad):
    rng = np.random.default_rng(215)
    mask = np.zeros((2, 6, 24, 40), bool)
    mask[0, 0:4, 2:5, 2:6] = True                                             # duration 4, volume 48
    mask[0, 2:3, 10:12, 10:12] = True                                         # duration 1, volume 4
    mask[0, 1:6, 20, 30:33] = True                                            # duration 5, volume 15
    mask[0, 4:6, 5, 20:22] = True                                             # duration 2, volume 4
    mask[1] = rng.random((6, 24, 40)) < 0.04                                  # speckle: many short events
    maps = _from_masks(216, mask)
    every = ref.detect_batch(maps, T, 8, 9, 1, 1, 4096)
    assert every[1][0].tolist() == [4, 0, 71, 0] and every[1][1, 0] > 64
    for min_duration in (1, 2, 3, 4, 5, 6):
        got, want = _run_and_check(vad, maps, T, 8, 9, min_duration, 1, 64)
        assert want[1][0, :2].tolist() == [sum(d >= min_duration for d in (4, 1, 5, 2)), sum(d < min_duration for d in (4, 1, 5, 2))]
        assert (want[1][:, 0] + want[1][:, 1]).tolist() == every[1][:, 0].tolist()          # kept + dropped = all events
        assert torch.equal(got.labels.cpu(), torch.from_numpy(every[3]))                     # labels keep the dropped events
    got, want = _run_and_check(vad, maps, T, 8, 9, 3, 1, 64)
    assert got.alarms()[0].tolist() == [True, True, True, True, True, True] and want[2][0, :, 1].tolist() == [12, 15, 15, 15, 3, 3]
    got, want = _run_and_check(vad, maps, T, 8, 9, 5, 1, 64)                  # the event of duration 4 leaves its frames un-alarmed
    assert got.alarms()[0].tolist() == [False, True, True, True, True, True]
    for min_volume in (4, 5, 15, 16, 48, 49):
        got, want = _run_and_check(vad, maps, T, 8, 9, 1, min_volume, 64)
        assert want[1][0, 0] == sum(v >= min_volume for v in (48, 4, 15, 4))
    got, want = _run_and_check(vad, maps, T, 8, 9, 2, 5, 64)                  # both at once
    assert want[1][0, :2].tolist() == [2, 2]
    kept = int(every[1][1, 0])
    full = vad.metrics.detect_events(torch.from_numpy(maps).cuda(), float(T), max_events=4096)
    for max_events in (1, 3, 4, 5, kept - 1, kept, kept + 1):
        got, want = _run_and_check(vad, maps, T, 8, 9, 1, 1, max_events)
        assert got.truncated().tolist() == [max_events < 4, max_events < kept] and got.counts[:, 0].tolist() == [4, kept]
        assert torch.equal(got.frame_counts, full.frame_counts)               # the alarm signal does not depend on max_events
    _run_and_check(vad, maps, T, 4, 1, 2, 3, 7)


# ------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_dense_volume_chases_one_root(vad, mode):
    connectivity, temporal = mode
    maps = _from_masks(217, np.ones((1, 8, 64, 64), bool))
    got, want = _run_and_check(vad, maps, T, connectivity, temporal)          # the flag word stays clear: detect_events raises on it
    assert want[1][0].tolist() == [1, 0, 8 * 64 * 64, 0] and want[0][0, 0, :8].tolist() == [0, 8 * 64 * 64, 0, 7, 0, 0, 63, 63]
    assert want[2][0].tolist() == [[4096, 4096, 0]] * 8


def test_a_sparse_volume_beyond_one_grid_round_of_every_pass(vad):
    out = [ctypes.c_int(0) for _ in range(5)]
    assert vad.hip.lib().vad_events_plan(*[ctypes.byref(v) for v in out]) == 0
    label_round, volume_round, scan_round, reduce_round, threads = (v.value for v in out)
    t, h, w = 17, 256, 256
    assert t * h * w > max(volume_round, scan_round, reduce_round) and label_round == 4096 * 256 and threads == 256
    mask = np.zeros((t, h, w), bool)
    mask[0, 0, 0:3] = mask[1, 0, 1:4] = True                                  # the first voxel
    mask[16, 255, 250:] = mask[15, 254, 249:252] = True                       # the last voxel; linked diagonally in time
    mask[3:16, 100:104, 200:204] = True                                       # a long one
    mask[15:17, 10:13, 10:13] = True                                          # one across the end of the first grid round
    assert max(volume_round, scan_round, reduce_round) <= 16 * h * w          # frame 16 lies behind the first round of every pass
    for f in range(4, 12):
        mask[f, 30 + 2 * f, 60 + f:64 + f] = True                             # drifting: two rows per frame - too fast to link
    mask[8, 128, :] = True                                                    # a whole row
    maps = _from_masks(218, mask[None])
    got, want = _run_and_check(vad, maps, T, 8, 9)
    assert want[1][0].tolist() == [13, 0, int(mask.sum()), 0] and 500 < mask.sum() < 1000
    assert _roots(want)[0] == 0 and want[0][0, 12, ref.T1] == 16 and mask.reshape(-1)[-1] and want[3][0, 16, 255, 255] == want[0][0, 12, ref.ROOT] + 1
    got, want = _run_and_check(vad, maps, T, 8, 1, 2, 5, 2)                   # filters and truncation across the rounds
    assert want[1][0, :2].tolist() == [3, 11] and _roots(want) == [0, 3 * h * w + 100 * w + 200]


def test_odd_shapes(vad):
    rng = np.random.default_rng(219)
    dotted = np.arange(301) % 5 != 1
    for shape in ((1, 1, 301), (301, 1, 1), (1, 301, 1)):                     # one row, one pixel over 301 frames, one column
        maps = _from_masks(220, dotted.reshape(1, *shape))
        for connectivity, temporal in MODES:
            got, want = _run_and_check(vad, maps, T, connectivity, temporal, 1, 1, 128)
            assert want[1][0].tolist() == [61, 0, int(dotted.sum()), 0] and want[0][0, 0, ref.VOLUME] == 1 and want[0][0, 1, ref.VOLUME] == 4
            if shape[0] == 301:
                assert want[0][0, 1, ref.T0:ref.T1 + 1].tolist() == [2, 5] and got.centroids()[0, 1].tolist() == [3.5, 0.0, 0.0]
    maps = _from_masks(221, rng.random((2, 5, 3, 67)) < 0.45)                 # rows longer than a wave, frames shorter than a work-group
    for connectivity, temporal in MODES:
        _run_and_check(vad, maps, T, connectivity, temporal)
    _run_and_check(vad, _from_masks(222, np.ones((1, 1, 1, 1), bool)))
    _run_and_check(vad, _from_masks(223, np.zeros((2, 3, 5, 7), bool)))       # nothing at all


def test_views_and_the_host_table(vad):
    rng = np.random.default_rng(224)
    mask = np.repeat(pro_ref.blobs(rng, 2, 40, 56, count=5)[:, None], 4, axis=1)
    mask[:, 2] &= rng.random((2, 40, 56)) < 0.7
    maps = _from_masks(225, mask)
    got, want = _run_and_check(vad, maps, T, 8, 9, 1, 1, 32)
    records, counts = want[0], want[1]
    assert torch.equal(got.root.cpu(), _i32(records[..., 0])) and torch.equal(got.volume.cpu(), _i32(records[..., 1]))
    assert torch.equal(got.t0.cpu(), _i32(records[..., 2])) and torch.equal(got.t1.cpu(), _i32(records[..., 3]))
    assert torch.equal(got.box.cpu(), _i32(records[..., 4:8])) and torch.equal(got.peak_index.cpu(), _i32(records[..., 9]))
    assert got.peak.dtype == torch.float32 and torch.equal(got.peak.cpu().view(torch.int32), _i32(records[..., 8]))
    sx, sy, st = ref.sums(records)
    for view, s in ((got.sum_x, sx), (got.sum_y, sy), (got.sum_t, st)):
        assert view.dtype == torch.int64 and torch.equal(view.cpu(), torch.from_numpy(s))
    cen = got.centroids()
    assert cen.dtype == torch.float64 and cen.is_cuda and tuple(cen.shape) == (2, 32, 3)
    rows = got.to_list()
    assert [len(r) for r in rows] == counts[:, 0].tolist() and min(len(r) for r in rows) >= 2
    for b, clip_rows in enumerate(rows):
        for k, row in enumerate(clip_rows):
            r = records[b, k]
            assert (row["root"], row["volume"], row["t0"], row["t1"], row["box"]) == (int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(v) for v in r[4:8]))
            assert row["duration"] == int(got.durations()[b, k]) == int(r[3]) - int(r[2]) + 1
            assert row["peak"] == float(maps[b].reshape(-1)[r[9]]) and row["peak_tyx"] == tuple(int(v) for v in np.unravel_index(int(r[9]), (4, 40, 56)))
            assert row["centroid_tyx"] == (st[b, k] / r[1], sy[b, k] / r[1], sx[b, k] / r[1]) == tuple(cen[b, k].tolist())
            assert row["t0"] == int(r[0]) // (40 * 56)                         # the root is the event's first voxel
        assert torch.isnan(cen[b, len(clip_rows):]).all() and not got.durations()[b, len(clip_rows):].any()


# ------------------------------------------------------------------------------------------ determinism, input layouts
def test_any_batching_and_any_layout_give_the_same_words(vad):
    rng = np.random.default_rng(226)
    mask = np.concatenate([np.repeat(pro_ref.blobs(rng, 3, 24, 40)[:, None], 4, axis=1) & (rng.random((3, 4, 24, 40)) < 0.8),
                           np.ones((1, 4, 24, 40), bool), rng.random((1, 4, 24, 40)) < 0.4])
    maps_np = _from_masks(227, mask)
    want = ref.detect_batch(maps_np, T, 8, 9, 2, 2, 16)
    maps = torch.from_numpy(maps_np).cuda()
    args = (float(T), 8, 9, 2, 2, 16)
    whole = vad.metrics.detect_events(maps, *args, return_labels=True)
    _assert_table(whole, want)
    assert tuple(whole.records.shape) == (5, 16, 16) and tuple(whole.frame_counts.shape) == (5, 4, 3) and tuple(whole.truncated().shape) == (5,)
    backwards = vad.metrics.detect_events(maps.flip(0), *args, return_labels=True)
    for i in range(5):
        single = vad.metrics.detect_events(maps[i], *args, return_labels=True)            # [T,H,W]: one clip, no leading shape
        assert tuple(single.records.shape) == (16, 16) and tuple(single.counts.shape) == (4,) and tuple(single.frame_counts.shape) == (4, 3)
        assert tuple(single.labels.shape) == (4, 24, 40) and tuple(single.alarms().shape) == (4,) and len(single.to_list()) == 1
        for other in ((single.records, single.counts, single.frame_counts, single.labels),
                      (backwards.records[-1 - i], backwards.counts[-1 - i], backwards.frame_counts[-1 - i], backwards.labels[-1 - i])):
            assert all(torch.equal(a, b) for a, b in zip(other, (whole.records[i], whole.counts[i], whole.frame_counts[i], whole.labels[i])))
    flat = torch.zeros(maps.numel() + 1, device="cuda")
    flat[1:] = maps.reshape(-1)
    sliced = flat[1:].view(*maps.shape)                                       # one float off its allocation
    assert sliced.data_ptr() % 16 == 4 and sliced.is_contiguous()
    _assert_table(vad.metrics.detect_events(sliced, *args, return_labels=True), want)
    five = vad.metrics.detect_events(maps[:, :, None], *args, return_labels=True)          # [B,T,1,H,W]
    assert tuple(five.labels.shape) == (5, 4, 24, 40)
    _assert_table(five, want)
    strided = torch.from_numpy(np.ascontiguousarray(maps_np.transpose(1, 0, 3, 2))).cuda().permute(1, 0, 3, 2)
    assert not strided.is_contiguous() and tuple(strided.shape) == tuple(maps.shape)
    _assert_table(vad.metrics.detect_events(strided, *args, return_labels=True), want)
    without = vad.metrics.detect_events(maps, *args)
    assert without.labels is None
    _assert_table(without, want, labels=False)
    empty = vad.metrics.detect_events(maps[:0], *args, return_labels=True)
    assert tuple(empty.records.shape) == (0, 16, 16) and tuple(empty.frame_counts.shape) == (0, 4, 3) and empty.to_list() == []


def test_refusals(vad):
    t = torch.zeros(2, 3, 8, 8, device="cuda")
    VadError = vad.hip.VadError
    for bad, word in ((t[0, 0], "maps must be"), (t[:, :, None, None], "maps must be"), (t[:, :, None].expand(2, 3, 2, 8, 8), "maps must be"),
                      (t.double(), "float32"), (t.cpu(), "no CPU fallback"), (t[:, :0], "out of range"), (t.numpy(force=True), "torch tensor")):
        with pytest.raises(VadError, match=word):
            vad.metrics.detect_events(bad, 0.5)
    for kw, word in (({"threshold": float("nan")}, "threshold"), ({"threshold": None}, "threshold"), ({"threshold": True}, "threshold"),
                     ({"min_duration": 0}, "min_duration"), ({"min_duration": 1.5}, "min_duration"), ({"min_volume": 0}, "min_volume"),
                     ({"min_volume": 2 ** 32}, "min_volume"), ({"max_events": 0}, "max_events"), ({"max_events": 65537}, "max_events"),
                     ({"connectivity": 6}, "connectivity"), ({"temporal": 27}, "temporal must be 1 or 9"), ({"temporal": True}, "temporal must be"),
                     ({"connectivity": 4, "temporal": 9}, "temporal=9"), ({"connectivity": 4}, "temporal=9")):
        with pytest.raises(VadError, match=word):
            vad.metrics.detect_events(t, **{"threshold": 0.5, **kw})
    assert int(vad.metrics.detect_events(t, 0.5, connectivity=4, temporal=1).counts.sum()) == 0


# ------------------------------------------------------------------------------------------ the C ABI on the device
def test_c_abi_with_a_poisoned_and_guarded_workspace(vad):
    """The workspace contract: exactly vad_events_workspace_bytes are enough, whatever they held before, and not a byte in front of
    or behind them (or behind any output) is written."""
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    rng = np.random.default_rng(228)
    mask = np.repeat(pro_ref.blobs(rng, 3, 24, 40)[:, None], 3, axis=1) & (rng.random((3, 3, 24, 40)) < 0.8)
    mask[1] = False
    maps_np = _from_masks(229, mask)
    want = ref.detect_batch(maps_np, T, 8, 9, 2, 2, 8)
    b, t, h, w = maps_np.shape
    maps = torch.from_numpy(maps_np).cuda()
    need0, need1 = lib.vad_events_workspace_bytes(b, t, h, w, 0), lib.vad_events_workspace_bytes(b, t, h, w, 1)
    assert need0 - need1 == 4 * b * t * h * w and need1 == 16 + 48 + 8 * b * t * h * w      # three chunks per clip: 36 bytes, padded
    G = 256                                                                   # guard bytes in front of and behind every buffer

    def guarded(nbytes, fill):
        whole = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device="cuda")
        return whole, whole[G:G + nbytes]

    def intact(whole, fill):
        return bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all())

    def run(given, need):
        bufs = {"ws": guarded(need, 0xAB), "records": guarded(b * 8 * 16 * 4, 0xF9), "counts": guarded(b * 16, 0xF9),
                "frames": guarded(b * t * 12, 0xF9), "labels": guarded(b * t * h * w * 4, 0xF9)}
        ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
        assert ptr["ws"] % 16 == 0 and ptr["records"] % 16 == 0
        rc = lib.vad_detect_events(maps.data_ptr(), b, t, h, w, float(T), 8, 9, 2, 2, 8, ptr["labels"] if given else None, ptr["records"],
                                   ptr["counts"], ptr["frames"], ptr["ws"], need, stream)
        assert rc == 0, lib.vad_last_error()
        torch.cuda.synchronize()
        assert all(intact(v[0], 0xAB if k == "ws" else 0xF9) for k, v in bufs.items()), "a guard was written"
        assert int(bufs["ws"][1][:4].view(torch.int32).item()) == 0
        assert torch.equal(bufs["records"][1].view(torch.int32).cpu().view(b, 8, 16), _i32(want[0]))
        assert torch.equal(bufs["counts"][1].view(torch.int32).cpu().view(b, 4), _i32(want[1]))
        assert torch.equal(bufs["frames"][1].view(torch.int32).cpu().view(b, t, 3), _i32(want[2]))
        if given:
            assert torch.equal(bufs["labels"][1].view(torch.int32).cpu().view(b, t, h, w), torch.from_numpy(want[3]))
        else:
            assert bool((bufs["labels"][1] == 0xF9).all())
        return bufs

    run(False, need0)                                                         # labels_or_null NULL: the plane lives in ws
    bufs = run(True, need1)                                                   # labels given: the smaller workspace
    ws, records, counts, frames, labels = (bufs[k][1] for k in ("ws", "records", "counts", "frames", "labels"))
    before = [v.clone() for v in (records, counts, frames, labels)]
    common = (maps.data_ptr(), b, t, h, w, float(T), 8, 9, 2, 2, 8)
    outs = (records.data_ptr(), counts.data_ptr(), frames.data_ptr(), ws.data_ptr())
    # a short workspace, b == 0 and a refused argument: nothing but the flag word is touched
    assert lib.vad_detect_events(*common, labels.data_ptr(), *outs, need1 - 1, stream) == -3 and b"ws_bytes" in lib.vad_last_error()
    assert lib.vad_detect_events(*common, None, *outs, need0 - 1, stream) == -3
    ws.fill_(0xAB)
    assert lib.vad_detect_events(maps.data_ptr(), 0, t, h, w, float(T), 8, 9, 2, 2, 8, labels.data_ptr(), *outs, 16, stream) == 0
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[16:] == 0xAB).all())
    assert lib.vad_detect_events(maps.data_ptr(), b, t, h, w, float("nan"), 8, 9, 2, 2, 8, None, *outs, need1, stream) == -1
    assert b"threshold is NaN" in lib.vad_last_error()
    assert lib.vad_detect_events(maps.data_ptr(), b, t, h, w, float(T), 4, 9, 2, 2, 8, None, *outs, need1, stream) == -1
    assert b"temporal 9 needs connectivity 8" in lib.vad_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(before, (records, counts, frames, labels)))


# ------------------------------------------------------------------------------------------ capture
def test_a_captured_call_follows_new_map_contents(vad):
    """Every launch is asynchronous on the caller's stream and nothing is allocated: one call captured on a side stream, replayed
    on new contents of the same buffers, equals the eager result."""
    lib = vad.hip.lib()
    rng = np.random.default_rng(230)
    first = _from_masks(231, np.repeat(pro_ref.blobs(rng, 2, 24, 40)[:, None], 4, axis=1) & (rng.random((2, 4, 24, 40)) < 0.8))
    second = _from_masks(232, rng.random((2, 4, 24, 40)) < 0.2)
    b, t, h, w = first.shape
    maps = torch.from_numpy(first).cuda()
    need = lib.vad_events_workspace_bytes(b, t, h, w, 0)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    records = torch.empty((b, 16, 16), dtype=torch.int32, device="cuda")
    counts = torch.empty((b, 4), dtype=torch.int32, device="cuda")
    frames = torch.empty((b, t, 3), dtype=torch.int32, device="cuda")

    def call():
        vad.hip.check(lib.vad_detect_events(maps.data_ptr(), b, t, h, w, float(T), 8, 9, 2, 1, 16, None, records.data_ptr(), counts.data_ptr(),
                                            frames.data_ptr(), ws.data_ptr(), need, vad.hip.current_stream()), "vad_detect_events")

    call()                                                                                   # once eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for contents in (first, second):
        maps.copy_(torch.from_numpy(contents).cuda())
        records.fill_(-7)
        counts.fill_(-7)
        frames.fill_(-7)
        graph.replay()
        want = ref.detect_batch(contents, T, 8, 9, 2, 1, 16)
        assert torch.equal(records.cpu(), _i32(want[0])) and torch.equal(counts.cpu(), _i32(want[1])) and torch.equal(frames.cpu(), _i32(want[2]))
        assert int(ws[:4].view(torch.int32).item()) == 0
    eager = vad.metrics.detect_events(maps, float(T), 8, 9, 2, 1, 16)
    assert torch.equal(eager.records, records) and torch.equal(eager.counts, counts) and torch.equal(eager.frame_counts, frames)


# ------------------------------------------------------------------------------------------ through the models
def _threshold_of(vad, maps, fpr=0.05):
    """An operating threshold from a histogram of the same maps: the labels are a fixed checkerboard of 8 x 8 blocks, so both
    classes are populated whatever the maps hold."""
    h, w = maps.shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w]
    lab = torch.from_numpy((((yy // 8) + (xx // 8)) % 2).astype(np.uint8) * 255).cuda().expand(maps.shape).contiguous()
    hist = vad.metrics.ScoreHistogram(11).accumulate(maps, lab)
    t, tpr, reached = vad.metrics.threshold_at_fpr(hist.counts_host(), fpr)
    assert np.isfinite(t) and reached <= fpr and float(np.float32(t)) == t
    return t


@pytest.mark.parametrize("sigma", (None, 1.0))
def test_localize_events_through_the_video_model(vad, sigma):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    with torch.no_grad():
        by_hand = vad.scoring._anomaly_maps(model, clips, "mse", sigma, 4.0)
        t = _threshold_of(vad, by_hand)
    before = {k: vad.hip.calls.get(k, 0) for k in ("detect_events", "vid_score", "smooth_maps", "detect_regions")}
    events, maps = vad.scoring.localize_events(model, clips, t, sigma=sigma, temporal=1, min_duration=2, max_events=16)
    after = {k: vad.hip.calls.get(k, 0) for k in before}
    assert [after[k] - before[k] for k in before] == [1, 1, int(sigma is not None), 0]
    assert tuple(maps.shape) == (2, 4, 1, 32, 32) and maps.is_cuda and torch.equal(maps, by_hand)
    assert tuple(events.records.shape) == (2, 16, 16) and tuple(events.frame_counts.shape) == (2, 4, 3) and events.threshold == t
    want = ref.detect_batch(maps.cpu().numpy().reshape(2, 4, 32, 32), t, 8, 1, 2, 1, 16)
    print(f"video sigma {sigma}: threshold {t!r} counts {want[1].tolist()} frames {want[2][..., 1].tolist()}")
    _assert_table(events, want, labels=False)
    assert want[1][:, 2].sum() > 0
    same = vad.metrics.detect_events(by_hand, t, 8, 1, 2, 1, 16)
    assert torch.equal(same.records, events.records) and torch.equal(same.frame_counts, events.frame_counts)
    with pytest.raises(vad.hip.VadError, match="map='mse'"):
        vad.scoring.localize_events(model, clips, t, map="ssim")


@pytest.mark.parametrize("calibrated", (False, True))
def test_localize_events_through_the_image_model(vad, calibrated):
    """A batch of consecutive synthetic frames of one camera is one volume."""
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    stats = vad.scoring.calibrate(model, [{"image": x}], "cuda", map="mse", sigma=1.0) if calibrated else None
    with torch.no_grad():
        by_hand = vad.scoring._anomaly_maps(model, x, "mse", 1.0, 4.0, stats, vad.metrics.DEFAULT_MIN_STD if calibrated else None)
    t = 1.0 if calibrated else _threshold_of(vad, by_hand)                    # a z-score of one standard deviation, or a map value
    before = {k: vad.hip.calls.get(k, 0) for k in ("detect_events", "img_score", "smooth_maps")}
    events, maps = vad.scoring.localize_events(model, x, t, sigma=1.0, calibration=stats, connectivity=4, temporal=1, min_volume=2, max_events=8)
    assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [1, 1, 1]
    assert tuple(maps.shape) == (6, 1, 32, 32) and torch.equal(maps, by_hand)
    assert tuple(events.records.shape) == (8, 16) and tuple(events.counts.shape) == (4,) and tuple(events.frame_counts.shape) == (6, 3)
    want = ref.detect(maps.cpu().numpy()[:, 0], t, 4, 1, 1, 2, 8)
    print(f"image calibrated {calibrated}: threshold {t!r} counts {want[1].tolist()} frames {want[2][:, 1].tolist()}")
    _assert_table(events, want, labels=False)
    assert want[1][2] > 0 and events.volume_shape == (6, 32, 32) and tuple(events.alarms().shape) == (6,)
    with pytest.raises(vad.hip.VadError, match="map must be"):
        vad.scoring.localize_events(model, x, 0.5, map="psnr")
