"""Defect regions of an anomaly map on the GPU (csrc/map_regions.hip, metrics.detect_regions, scoring.localize): records and counts
`torch.equal` to the numpy restatement (tests/regions_ref.py), labels to the reference labeller (tests/pro_ref.py), on the shapes
that defeat a labeller, on ties, non-finite pixels, every filter and truncation, frames larger than one launch's grid, any
batching, the raw C ABI with a poisoned workspace, a captured call, and through both seeded models."""
import numpy as np
import pytest
import torch

import pro_ref
import regions_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
_REFS = {}


def _masks():
    """The shape fixtures of tests/test_hip_pro.py, rebuilt from pro_ref with the same seed."""
    rng = np.random.default_rng(50)
    first, last = np.zeros((9, 13), bool), np.zeros((9, 13), bool)
    first[0, 0] = last[-1, -1] = True
    diag = np.zeros((8, 8), bool)
    diag[1:4, 1:4] = diag[4:7, 4:7] = True
    out = {"empty": np.zeros((1, 19, 23), bool), "full": np.ones((1, 19, 23), bool), "first_pixel": first[None], "last_pixel": last[None],
           "row_1x37": np.ones((1, 1, 37), bool), "column_37x1": np.ones((1, 37, 1), bool),
           "dotted_row": (np.arange(37) % 3 != 1)[None, None], "dotted_column": (np.arange(37) % 3 != 1)[None, :, None],
           "checker_37x53": (np.add.outer(np.arange(37), np.arange(53)) % 2).astype(bool)[None], "diagonal_touch": diag[None],
           "u_64": pro_ref.u_shape(64, 64)[None], "serpentine_64": pro_ref.serpentine(64, 64)[None], "spiral_64": pro_ref.spiral(64)[None],
           "spiral_256": pro_ref.spiral(256)[None], "blobs_48x80": pro_ref.blobs(rng, 2, 48, 80),
           "blobs_130x70": pro_ref.blobs(rng, 2, 130, 70, count=9, radius=9), "noise_33x65": rng.random((2, 33, 65)) < 0.5}
    busy = pro_ref.blobs(rng, 2, 48, 80)
    out["empty_and_busy"] = np.stack([np.zeros((48, 80), bool), busy[0], np.ones((48, 80), bool), busy[1], np.zeros((48, 80), bool)])
    return out


MASKS = _masks()


def _map(name):
    """The fixture as a float map: seeded values >= T on the mask (T itself among them), < T off it."""
    if name not in _REFS:
        _REFS[name] = ref.map_from_mask(np.random.default_rng(80 + list(MASKS).index(name)), MASKS[name], T)
    return _REFS[name]


def _want(name, connectivity):
    if (name, connectivity) not in _REFS:
        _REFS[name, connectivity] = ref.detect_batch(_map(name), T, connectivity, 1, 64)
    return _REFS[name, connectivity]


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _assert_table(got, want, labels=True):
    """got: metrics.Regions; want: (records, counts, labels) of the restatement."""
    records, counts, lab = want
    assert got.records.dtype == torch.int32 and got.counts.dtype == torch.int32
    assert torch.equal(got.records.cpu().reshape(records.shape), _i32(records)), "records differ from the restatement"
    assert torch.equal(got.counts.cpu().reshape(counts.shape), _i32(counts)), "counts differ from the restatement"
    if labels:
        assert torch.equal(got.labels.cpu().reshape(lab.shape), torch.from_numpy(lab)), "labels differ from the reference labeller"


def _run_and_check(vad, maps, t, connectivity=8, min_area=1, max_regions=64):
    want = ref.detect_batch(maps, t, connectivity, min_area, max_regions)
    got = vad.metrics.detect_regions(torch.from_numpy(maps).cuda(), float(t), connectivity, min_area, max_regions, return_labels=True)
    _assert_table(got, want)
    return got, want


# ------------------------------------------------------------------------------------------ the shapes that defeat a labeller
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", list(MASKS))
def test_shape_fixtures_equal_the_restatement(vad, name, connectivity):
    maps = _map(name)
    want = _want(name, connectivity)
    assert np.array_equal(want[2], pro_ref.label_batch(MASKS[name], connectivity)[0])
    before = vad.hip.calls.get("detect_regions", 0)
    got = vad.metrics.detect_regions(torch.from_numpy(maps).cuda(), float(T), connectivity, return_labels=True)   # raises on a set flag
    assert vad.hip.calls["detect_regions"] == before + 1
    assert tuple(got.records.shape) == (len(maps), 64, 12) and tuple(got.counts.shape) == (len(maps), 4) and tuple(got.labels.shape) == maps.shape
    _assert_table(got, want)
    assert got.truncated().tolist() == (want[1][:, 0] > 64).tolist()
    without = vad.metrics.detect_regions(torch.from_numpy(maps).cuda(), float(T), connectivity)
    assert without.labels is None
    _assert_table(without, want, labels=False)


def test_what_the_fixtures_exercise(vad):
    assert _want("checker_37x53", 8)[1][0].tolist() == [1, 0, 980, 0]
    assert _want("checker_37x53", 4)[1][0].tolist() == [980, 0, 980, 0]                    # 980 one-pixel regions: truncated at 64
    got = vad.metrics.detect_regions(torch.from_numpy(_map("checker_37x53")).cuda(), float(T), 4)
    assert got.truncated().tolist() == [True] and int(got.area.sum()) == 64 and int(got.counts[0, 0]) == 980
    assert _want("diagonal_touch", 8)[1][0, 0] == 1 and _want("diagonal_touch", 4)[1][0, 0] == 2
    for name in ("u_64", "serpentine_64", "spiral_64", "spiral_256"):
        assert _want(name, 4)[1][0, 0] == 1 and _want(name, 4)[0][0, 0, ref.AREA] == MASKS[name].sum()
    assert (_map("full") == T).any() and _want("full", 8)[0][0, 0, ref.AREA] == 19 * 23     # a value equal to the threshold is foreground
    assert _want("empty_and_busy", 8)[1][:, 0].tolist()[0::2] == [0, 1, 0]


def test_views_centroids_and_the_host_table(vad):
    maps = _map("blobs_130x70")
    records, counts, _ = _want("blobs_130x70", 8)
    got = vad.metrics.detect_regions(torch.from_numpy(maps).cuda(), float(T))
    assert torch.equal(got.root.cpu(), _i32(records[..., 0])) and torch.equal(got.area.cpu(), _i32(records[..., 1]))
    assert torch.equal(got.box.cpu(), _i32(records[..., 2:6])) and torch.equal(got.peak_index.cpu(), _i32(records[..., 7]))
    assert got.peak.dtype == torch.float32 and torch.equal(got.peak.cpu().view(torch.int32), _i32(records[..., 6]))
    sx, sy = ref.sums(records)
    assert got.sum_x.dtype == torch.int64 and torch.equal(got.sum_x.cpu(), torch.from_numpy(sx)) and torch.equal(got.sum_y.cpu(), torch.from_numpy(sy))
    cen = got.centroids()
    assert cen.dtype == torch.float64 and cen.is_cuda and tuple(cen.shape) == (2, 64, 2)
    rows = got.to_list()
    assert [len(r) for r in rows] == counts[:, 0].tolist() and min(len(r) for r in rows) >= 3
    for f, frame_rows in enumerate(rows):
        for k, row in enumerate(frame_rows):
            r = records[f, k]
            assert (row["root"], row["area"], row["box"]) == (int(r[0]), int(r[1]), tuple(int(v) for v in r[2:6]))
            assert row["peak"] == float(maps[f].reshape(-1)[r[7]]) and row["peak_yx"] == divmod(int(r[7]), 70)
            assert row["centroid_yx"] == (sy[f, k] / r[1], sx[f, k] / r[1]) == tuple(cen[f, k].tolist())
            y0, x0 = divmod(int(r[0]), 70)
            assert r[2] <= x0 <= r[4] and r[3] == y0                                       # the root is the region's first pixel
        assert torch.isnan(cen[f, len(frame_rows):]).all()


# ------------------------------------------------------------------------------------------ ties
def test_ties_signed_zeros_and_the_threshold_itself(vad):
    frame = np.full((12, 70), -2.0, np.float32)
    frame[2:6, 3:68] = 1.0                                                                  # one region over two waves' worth of a row
    frame[3, 66] = frame[5, 4] = frame[4, 30] = 7.5                                         # the maximum three times: the smallest index wins
    frame[8, 5:9] = np.float32(0.5)                                                         # exactly the threshold
    frame[10, 10:14] = np.nextafter(np.float32(0.5), np.float32(0))                         # one ulp below: background
    got, want = _run_and_check(vad, frame[None], 0.5)
    assert want[1][0].tolist() == [2, 0, 4 * 65 + 4, 0]
    assert want[0][0, 0, ref.PEAK_INDEX] == 3 * 70 + 66 and want[0][0, 1].tolist()[:8] == [8 * 70 + 5, 4, 5, 8, 8, 8, 0x3F000000, 8 * 70 + 5]
    zeros = np.full((3, 9), -5.0, np.float32)
    zeros[1, 1:8] = [-0.0, -0.5, -0.0, 0.0, -0.0, 0.0, -0.25]
    got, want = _run_and_check(vad, zeros[None], -1.0)
    assert want[0][0, 0, ref.PEAK] == 0 and want[0][0, 0, ref.PEAK_INDEX] == 9 + 4          # the first +0.0, not the first -0.0
    negz = np.full((3, 9), -5.0, np.float32)
    negz[1, 2:5] = [-0.5, -0.0, -0.0]
    got, want = _run_and_check(vad, negz[None], -1.0)
    assert want[0][0, 0, ref.PEAK] == 0x80000000 and want[0][0, 0, ref.PEAK_INDEX] == 9 + 3
    assert np.signbit(got.peak[0, 0].item())


# ------------------------------------------------------------------------------------------ non-finite pixels
def test_nan_and_inf_pixels(vad):
    rng = np.random.default_rng(81)
    frame = ref.map_from_mask(rng, np.zeros((20, 30), bool), T)
    frame[4:10, 5:25] = 1.0 + rng.random((6, 20), dtype=np.float32)                         # one bar ...
    frame[4:10, 14] = np.nan                                                                # ... cut in two by a NaN column
    frame[12, 3:9] = [0.5, np.nan, 0.5, np.nan, np.nan, 0.5]                                # NaNs between one-pixel regions
    frame[0, 0] = np.nan                                                                    # and one beside everything
    frame[7, 20] = np.inf                                                                   # +Inf is the right bar's peak
    for connectivity in (4, 8):
        got, want = _run_and_check(vad, frame[None], T, connectivity)
        assert want[1][0].tolist() == [5, 0, 6 * 19 + 3, 6 + 3 + 1]
        assert want[0][0, 1, ref.PEAK] == 0x7F800000 and want[0][0, 1, ref.PEAK_INDEX] == 7 * 30 + 20
        assert want[0][0, 0, ref.X1] == 13 and want[0][0, 1, ref.X0] == 15
    # +Inf is foreground at every threshold, +Inf itself included; -Inf as a threshold takes every pixel but the NaNs
    got, want = _run_and_check(vad, frame[None], np.inf)
    assert want[1][0].tolist() == [1, 0, 1, 10] and want[0][0, 0, ref.ROOT] == 7 * 30 + 20
    got, want = _run_and_check(vad, frame[None], -np.inf, 4)
    assert want[1][0, 2] == 20 * 30 - 10 and want[1][0, 3] == 10


def test_a_nan_frame_changes_no_word_of_its_neighbours(vad):
    rng = np.random.default_rng(82)
    maps = ref.map_from_mask(rng, pro_ref.blobs(rng, 3, 40, 56), T)
    clean = vad.metrics.detect_regions(torch.from_numpy(maps).cuda(), float(T), return_labels=True)
    dirty = maps.copy()
    dirty[1] = np.nan
    got, want = _run_and_check(vad, dirty, T)
    assert want[1][1].tolist() == [0, 0, 0, 40 * 56] and not want[0][1].any()
    for f in (0, 2):
        assert torch.equal(got.records[f], clean.records[f]) and torch.equal(got.counts[f], clean.counts[f]) and torch.equal(got.labels[f], clean.labels[f])


# ------------------------------------------------------------------------------------------ the filter and the truncation
def test_min_area_and_max_regions(vad):
    rng = np.random.default_rng(83)
    mask = np.concatenate([pro_ref.blobs(rng, 2, 48, 80, count=10, radius=4), (rng.random((1, 48, 80)) < 0.3)])
    maps = ref.map_from_mask(rng, mask, T)
    records, counts, _ = ref.detect_batch(maps, T, 8, 1, 4096)
    largest = int(records[..., ref.AREA].max())
    kept = int(counts[0, 0])
    assert counts[:, 0].min() >= 4 and counts[2, 0] > 64 and (records[2, :, ref.AREA] == 1).sum() > 8
    for min_area in (1, 2, 5, largest, largest + 1):
        got, want = _run_and_check(vad, maps, T, 8, min_area, 64)
        assert (want[1][:, 0] + want[1][:, 1]).tolist() == counts[:, 0].tolist()            # kept + dropped = all regions
        if min_area == largest + 1:
            assert not want[0].any() and want[1][:, 0].tolist() == [0, 0, 0]
        assert torch.equal(got.labels.cpu(), torch.from_numpy(ref.detect_batch(maps, T, 8, 1, 1)[2]))   # labels keep the dropped regions
    for max_regions in (1, kept - 1, kept, kept + 1, 4096):
        got, want = _run_and_check(vad, maps, T, 8, 1, max_regions)
        assert got.truncated().tolist() == (counts[:, 0] > max_regions).tolist()
        assert got.truncated()[0].item() == (max_regions < kept)
    _run_and_check(vad, maps, T, 4, 2, 7)


# ------------------------------------------------------------------------------------------ layout
def test_a_frame_wider_than_a_work_groups_run(vad):
    """3 x 5000: a row spans several runs of the reduce pass (4096 pixels) and chunks of the scan (1024)."""
    rng = np.random.default_rng(84)
    mask = np.zeros((2, 3, 5000), bool)
    mask[0, 1, 100:4900] = True                                                              # one region across every chunk border
    mask[0, 0, 4990:] = mask[0, 2, :7] = True
    mask[1] = rng.random((3, 5000)) < 0.4
    maps = ref.map_from_mask(rng, mask, T)
    got, want = _run_and_check(vad, maps, T, 4, 1, 64)
    assert want[1][0].tolist() == [3, 0, 4800 + 17, 0] and want[1][1, 0] > 64
    _run_and_check(vad, maps, T, 8, 3, 4096)


def test_one_sparse_frame_beyond_the_launch_grid(vad):
    """1040 x 1040 = 1 081 600 pixels exceed the labeller's 4096 x 256-pixel grid and the scan's 4096 chunks of 1024: the
    grid-stride loops run, and the ranks have to keep raster order across 1057 chunks."""
    rng = np.random.default_rng(85)
    h = w = 1040
    assert h * w > 4096 * 256 and (h * w + 1023) // 1024 == 1057
    mask = np.zeros((h, w), bool)
    mask[0, 0:5] = mask[0, 1030:] = True                                                     # first row, both ends
    mask[h - 1, 3:40] = mask[h - 1, w - 1] = True                                            # last row, the last pixel its own region
    for cy, cx in ((100, 900), (400, 17), (520, 520), (777, 1000), (1030, 600)):
        mask[cy:cy + 6, cx:cx + 7] = True
    mask[300, 200:260] = True
    maps = ref.map_from_mask(rng, mask[None], T)
    got, want = _run_and_check(vad, maps, T)
    assert want[1][0].tolist() == [10, 0, int(mask.sum()), 0] and 300 < mask.sum() < 400
    assert want[0][0, 0, ref.ROOT] == 0 and want[0][0, 9, ref.ROOT] == h * w - 1
    got, want = _run_and_check(vad, maps, T, 8, 11, 3)                                       # filter and truncation across the chunks
    assert want[1][0].tolist() == [7, 3, int(mask.sum()), 0]


def test_maps_off_their_allocation_and_leading_shapes(vad):
    maps = _map("blobs_48x80")
    want = _want("blobs_48x80", 8)
    flat = torch.zeros(maps.size + 1, device="cuda")
    flat[1:] = torch.from_numpy(maps).cuda().reshape(-1)
    sliced = flat[1:].view(*maps.shape)
    assert sliced.data_ptr() % 16 == 4 and sliced.is_contiguous()
    _assert_table(vad.metrics.detect_regions(sliced, float(T), return_labels=True), want)
    t = torch.from_numpy(maps).cuda()
    got = vad.metrics.detect_regions(t[:, None], float(T), return_labels=True)              # [B,1,H,W]
    assert tuple(got.records.shape) == (2, 64, 12) and tuple(got.labels.shape) == (2, 48, 80)
    _assert_table(got, want)
    clips = torch.stack([t, t.flip(0), t])[:, :, None]                                       # [B,T,1,H,W] = [3,2,1,48,80]
    got = vad.metrics.detect_regions(clips, float(T), return_labels=True)
    assert tuple(got.records.shape) == (3, 2, 64, 12) and tuple(got.counts.shape) == (3, 2, 4) and tuple(got.labels.shape) == (3, 2, 48, 80)
    assert tuple(got.truncated().shape) == (3, 2) and tuple(got.sum_x.shape) == (3, 2, 64) and len(got.to_list()) == 6
    for b, order in enumerate(((0, 1), (1, 0), (0, 1))):
        for k, f in enumerate(order):
            assert torch.equal(got.records[b, k].cpu(), _i32(want[0][f])) and torch.equal(got.counts[b, k].cpu(), _i32(want[1][f]))
            assert torch.equal(got.labels[b, k].cpu(), torch.from_numpy(want[2][f]))
    strided = torch.from_numpy(np.ascontiguousarray(maps.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not strided.is_contiguous()
    _assert_table(vad.metrics.detect_regions(strided, float(T), return_labels=True), want)
    empty = vad.metrics.detect_regions(t[:0], float(T), return_labels=True)
    assert tuple(empty.records.shape) == (0, 64, 12) and tuple(empty.labels.shape) == (0, 48, 80) and empty.to_list() == []
    VadError = vad.hip.VadError
    for bad, word in ((t[0, 0], "maps must be"), (t[:, None, None].expand(2, 2, 2, 48, 80), "maps must be"), (t.double(), "float32"), (t.cpu(), "no CPU fallback")):
        with pytest.raises(VadError, match=word):
            vad.metrics.detect_regions(bad, float(T))
    for kw, word in (({"threshold": float("nan")}, "threshold"), ({"threshold": None}, "threshold"), ({"threshold": 0.5, "min_area": 0}, "min_area"),
                     ({"threshold": 0.5, "max_regions": 0}, "max_regions"), ({"threshold": 0.5, "max_regions": 65537}, "max_regions"),
                     ({"threshold": 0.5, "connectivity": 6}, "connectivity")):
        with pytest.raises(VadError, match=word):
            vad.metrics.detect_regions(t, **kw)


# ------------------------------------------------------------------------------------------ determinism
def test_any_batching_gives_the_same_words(vad):
    rng = np.random.default_rng(86)
    mask = np.concatenate([pro_ref.blobs(rng, 4, 40, 56), np.ones((1, 40, 56), bool), rng.random((1, 40, 56)) < 0.5])
    maps = torch.from_numpy(ref.map_from_mask(rng, mask, T)).cuda()
    whole = vad.metrics.detect_regions(maps, float(T), 8, 2, 16, return_labels=True)
    _assert_table(whole, ref.detect_batch(maps.cpu().numpy(), T, 8, 2, 16))
    singles = [vad.metrics.detect_regions(maps[i:i + 1], float(T), 8, 2, 16, return_labels=True) for i in range(len(maps))]
    backwards = vad.metrics.detect_regions(maps.flip(0), float(T), 8, 2, 16, return_labels=True)
    for i in range(len(maps)):
        for other in (singles[i], None):
            rec, cnt, lab = (other.records[0], other.counts[0], other.labels[0]) if other else (backwards.records[-1 - i], backwards.counts[-1 - i], backwards.labels[-1 - i])
            assert torch.equal(rec, whole.records[i]) and torch.equal(cnt, whole.counts[i]) and torch.equal(lab, whole.labels[i])
    again = vad.metrics.detect_regions(maps, float(T), 8, 2, 16, return_labels=True)
    assert torch.equal(again.records, whole.records) and torch.equal(again.counts, whole.counts)


# ------------------------------------------------------------------------------------------ the C ABI on the device
def test_c_abi_with_a_poisoned_workspace(vad):
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    maps_np = _map("empty_and_busy")
    want = ref.detect_batch(maps_np, T, 8, 2, 8)
    n, h, w = maps_np.shape
    maps = torch.from_numpy(maps_np).cuda()
    need0, need1 = lib.vad_regions_workspace_bytes(n, h, w, 0), lib.vad_regions_workspace_bytes(n, h, w, 1)
    assert need0 - need1 == 4 * n * h * w

    def buffers(need):
        return (torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((n, 8, 12), -7, dtype=torch.int32, device="cuda"),
                torch.full((n, 4), -7, dtype=torch.int32, device="cuda"))

    ws, records, counts = buffers(need0)                                                     # labels_or_null NULL: the plane lives in ws
    assert lib.vad_detect_regions(maps.data_ptr(), n, h, w, float(T), 8, 2, 8, None, records.data_ptr(), counts.data_ptr(), ws.data_ptr(), need0, stream) == 0
    assert int(ws[:4].view(torch.int32).item()) == 0
    assert torch.equal(records.cpu(), _i32(want[0])) and torch.equal(counts.cpu(), _i32(want[1]))
    ws1, records1, counts1 = buffers(need1)                                                  # labels given: the smaller workspace
    labels = torch.full((n, h, w), -7, dtype=torch.int32, device="cuda")
    assert lib.vad_detect_regions(maps.data_ptr(), n, h, w, float(T), 8, 2, 8, labels.data_ptr(), records1.data_ptr(), counts1.data_ptr(),
                                  ws1.data_ptr(), need1, stream) == 0
    assert int(ws1[:4].view(torch.int32).item()) == 0
    assert torch.equal(records1, records) and torch.equal(counts1, counts) and torch.equal(labels.cpu(), torch.from_numpy(want[2]))
    # a short workspace, and n == 0: nothing but the flag word is touched
    before = (records.clone(), counts.clone(), labels.clone())
    assert lib.vad_detect_regions(maps.data_ptr(), n, h, w, float(T), 8, 2, 8, None, records.data_ptr(), counts.data_ptr(), ws.data_ptr(), need0 - 1, stream) == -3
    assert b"ws_bytes" in lib.vad_last_error()
    assert lib.vad_detect_regions(maps.data_ptr(), n, h, w, float(T), 8, 2, 8, labels.data_ptr(), records.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                  need1 - 1, stream) == -3
    ws.fill_(0xAB)
    assert lib.vad_detect_regions(maps.data_ptr(), 0, h, w, float(T), 8, 2, 8, labels.data_ptr(), records.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                  16, stream) == 0
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[16:] == 0xAB).all())
    assert torch.equal(records, before[0]) and torch.equal(counts, before[1]) and torch.equal(labels, before[2])
    assert lib.vad_detect_regions(maps.data_ptr(), n, h, w, float("nan"), 8, 2, 8, None, records.data_ptr(), counts.data_ptr(), ws.data_ptr(), need0, stream) == -1
    assert b"threshold is NaN" in lib.vad_last_error()
    torch.cuda.synchronize()
    assert torch.equal(records, before[0]) and torch.equal(counts, before[1])


# ------------------------------------------------------------------------------------------ capture
def test_a_captured_call_follows_new_map_contents(vad):
    """Every launch is asynchronous on the caller's stream and nothing is allocated: one call captured on a side stream, replayed
    on new contents of the same buffers, equals the eager result."""
    lib = vad.hip.lib()
    rng = np.random.default_rng(87)
    first = ref.map_from_mask(rng, pro_ref.blobs(rng, 3, 40, 56), T)
    second = ref.map_from_mask(rng, pro_ref.blobs(rng, 3, 40, 56, count=9), T)
    n, h, w = first.shape
    maps = torch.from_numpy(first).cuda()
    need = lib.vad_regions_workspace_bytes(n, h, w, 0)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    records = torch.empty((n, 16, 12), dtype=torch.int32, device="cuda")
    counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")

    def call():
        vad.hip.check(lib.vad_detect_regions(maps.data_ptr(), n, h, w, float(T), 8, 1, 16, None, records.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                             need, vad.hip.current_stream()), "vad_detect_regions")

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
        graph.replay()
        want = ref.detect_batch(contents, T, 8, 1, 16)
        assert torch.equal(records.cpu(), _i32(want[0])) and torch.equal(counts.cpu(), _i32(want[1]))
        assert int(ws[:4].view(torch.int32).item()) == 0
    eager = vad.metrics.detect_regions(maps, float(T), 8, 1, 16)
    assert torch.equal(eager.records, records) and torch.equal(eager.counts, counts)


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
def test_localize_through_the_image_model(vad, sigma):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    for kind in ("mse", "ssim"):
        with torch.no_grad():
            t = _threshold_of(vad, vad.scoring._anomaly_maps(model, x, kind, sigma, 4.0))
        before = {k: vad.hip.calls.get(k, 0) for k in ("detect_regions", "smooth_maps", "img_score")}
        regions, maps = vad.scoring.localize(model, x, t, map=kind, sigma=sigma, connectivity=4, min_area=2, max_regions=8)
        assert vad.hip.calls["detect_regions"] == before["detect_regions"] + 1
        assert vad.hip.calls.get("smooth_maps", 0) == before["smooth_maps"] + (sigma is not None)
        assert vad.hip.calls["img_score"] == before["img_score"] + 1
        assert tuple(maps.shape) == (6, 1, 32, 32) and maps.is_cuda and tuple(regions.records.shape) == (6, 8, 12)
        want = ref.detect_batch(maps.cpu().numpy()[:, 0], t, 4, 2, 8)
        print(f"image {kind} sigma {sigma}: threshold {t!r} counts {want[1].tolist()}")
        _assert_table(regions, want, labels=False)
        assert want[1][:, 2].sum() > 0 and regions.threshold == t
    with pytest.raises(vad.hip.VadError, match="map"):
        vad.scoring.localize(model, x, 0.5, map="psnr")


@pytest.mark.parametrize("sigma", (None, 1.0))
def test_localize_through_the_video_model(vad, sigma):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    with torch.no_grad():
        t = _threshold_of(vad, vad.scoring._anomaly_maps(model, clips, "mse", sigma, 4.0))
    before = vad.hip.calls.get("detect_regions", 0), vad.hip.calls["vid_score"]
    regions, maps = vad.scoring.localize(model, clips, t, sigma=sigma)
    assert (vad.hip.calls["detect_regions"], vad.hip.calls["vid_score"]) == (before[0] + 1, before[1] + 1)
    assert tuple(maps.shape) == (2, 4, 1, 32, 32) and tuple(regions.records.shape) == (2, 4, 64, 12) and tuple(regions.counts.shape) == (2, 4, 4)
    want = ref.detect_batch(maps.cpu().numpy().reshape(8, 32, 32), t, 8, 1, 64)
    print(f"video sigma {sigma}: threshold {t!r} counts {want[1].tolist()}")
    _assert_table(regions, want, labels=False)
    assert want[1][:, 2].sum() > 0
    with pytest.raises(vad.hip.VadError, match="map='mse'"):
        vad.scoring.localize(model, clips, t, map="ssim")
