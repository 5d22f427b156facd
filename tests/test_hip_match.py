"""Detections against ground-truth masks on the GPU (csrc/map_match.hip, metrics.match_regions, metrics.DetectionCounts,
scoring.detection_report): both tables and the sixteen counters `torch.equal` to the numpy restatement (tests/match_ref.py) on odd
shapes, several chunks, a frame past one grid round of every pass, the region cases a join can get wrong, the fraction boundary,
every mask format, truncation, any batching, a captured call, and through both seeded models."""
import ctypes
import math

import numpy as np
import pytest
import torch

import match_ref as ref
import pro_ref
import regions_ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
SHAPES = ((23, 31), (1, 41), (41, 1), (16, 16), (40, 70))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def _assert_equal(got, want):
    """got: metrics.Matches; want: (gt_records, pred_records, counts) of the restatement."""
    gt, pred, counts = want
    assert got.gt_records.dtype == torch.int32 and got.pred_records.dtype == torch.int32 and got.counts.dtype == torch.int64
    assert torch.equal(got.gt_records.cpu().reshape(gt.shape), _i32(gt)), "gt_records differ from the restatement"
    assert torch.equal(got.pred_records.cpu().reshape(pred.shape), _i32(pred)), "pred_records differ from the restatement"
    assert torch.equal(got.counts.cpu().reshape(counts.shape), _i64(counts)), "counts differ from the restatement"


def _run_and_check(vad, maps, masks, t=T, connectivity=8, min_area=1, gt_fraction=0.0, pred_fraction=0.0, max_regions=64):
    """maps float32 [n, h, w], masks bool [n, h, w] (sent as uint8 0 / 255) -> (Matches, restatement)."""
    want = ref.match_batch(maps, masks, t, connectivity, min_area, gt_fraction, pred_fraction, max_regions)
    got = vad.metrics.match_regions(torch.from_numpy(maps).cuda(), torch.from_numpy(masks.astype(np.uint8) * 255).cuda(), float(t), connectivity,
                                    min_area, gt_fraction, pred_fraction, max_regions)      # raises on a set flag
    _assert_equal(got, want)
    return got, want


def _random_pair(rng, n, h, w, density=0.45):
    masks = rng.random((n, h, w)) < density
    return regions_ref.map_from_mask(rng, rng.random((n, h, w)) < density, T), masks


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes_equal_the_restatement(vad, shape, connectivity):
    """Odd sizes, one row, one column, a power of two, and 40 x 70 = 2800 pixels: three chunks of 1024 of the count / slot scan."""
    h, w = shape
    rng = np.random.default_rng(220 + h + connectivity)
    maps, masks = _random_pair(rng, 3, h, w)
    before = vad.hip.calls.get("match_regions", 0)
    got, want = _run_and_check(vad, maps, masks, T, connectivity, 2, 0.5, 0.25, 64)
    assert vad.hip.calls["match_regions"] == before + 1
    assert tuple(got.gt_records.shape) == (3, 64, 4) and tuple(got.pred_records.shape) == (3, 64, 4) and tuple(got.counts.shape) == (3, 16)
    assert want[2][:, ref.TP].min() > 0 and want[2][:, ref.PRED_DROPPED].max() > 0 and want[2][:, ref.GT_REGIONS].min() > 0
    got, want = _run_and_check(vad, maps, masks, T, connectivity, 1, 0.0, 0.0, 4096)        # the defaults, nothing truncated
    assert not got.truncated().any()
    if shape == (40, 70):
        assert (h * w + 1023) // 1024 == 3
        spread = want[0][0][want[0][0, :, ref.AREA] > 0, ref.ROOT]
        assert spread.min() < 1024 and spread.max() >= 2048                                 # records come from the first and the last chunk


def test_one_frame_past_a_grid_round_of_every_pass(vad):
    """1040 x 1040 pixels exceed what one grid round of the labeller, of the join and of the count / slot scan cover, as
    vad_match_plan reports them: the grid-stride loops run, and the ranks of both tables keep raster order across 1057 chunks."""
    out = [ctypes.c_int(0) for _ in range(4)]
    assert vad.hip.lib().vad_match_plan(*[ctypes.byref(v) for v in out]) == 0
    h = w = 1040
    assert h * w > max(v.value for v in out[:3]) and out[3].value == 256
    rng = np.random.default_rng(221)
    fg, mask = np.zeros((h, w), bool), np.zeros((h, w), bool)
    fg[0, 0:5] = mask[0, 3:9] = True                                                        # the first pixels: a match in chunk 0
    fg[h - 1, w - 1] = mask[h - 1, w - 4:] = True                                           # the last pixel of the frame is a prediction's root
    fg[0, 1030:] = True                                                                     # a false alarm
    mask[h - 1, 3:40] = True                                                                # a miss
    for k, (cy, cx) in enumerate(((100, 900), (400, 17), (520, 520), (777, 1000), (1030, 600), (1024, 0))):
        fg[cy:cy + 6, cx:cx + 7] = True
        mask[cy + 3 - (k % 2) * 6:cy + 9 - (k % 2) * 6, cx + 2:cx + 12] = True              # half the defects overlap their prediction from below, half from above
    fg[300, 200:260] = True
    fg[302, 200:203] = mask[302, 200:203] = True                                            # a prediction dropped at min_area 4 on a mask region
    maps = regions_ref.map_from_mask(rng, fg[None], T)
    got, want = _run_and_check(vad, maps, mask[None], T, 8, 1, 0.0, 0.0, 64)
    c = want[2][0]
    assert c[ref.PRED_REGIONS] == 11 and c[ref.GT_REGIONS] == 10 and c[ref.TP] > 0 and c[ref.TP:ref.TN + 1].sum() == h * w
    assert want[1][0, 0, ref.ROOT] == 0 and want[1][0, 10, ref.ROOT] == h * w - 1 and want[1][0, 10].tolist() == [h * w - 1, 1, 1, 1]
    got, want = _run_and_check(vad, maps, mask[None], T, 8, 4, 0.25, 0.3, 3)                # filter, fractions (15 of 60 is the boundary) and truncation
    assert want[2][0, ref.PRED_DROPPED] == 2 and want[2][0, ref.PRED_REGIONS] == 9 and got.truncated().tolist() == [True]
    assert 0 < want[2][0, ref.GT_DETECTED] < want[2][0, ref.GT_REGIONS] and 0 < want[2][0, ref.PRED_MATCHED] < want[2][0, ref.PRED_REGIONS]


# ------------------------------------------------------------------------------------------ the region cases
def _cases():
    """name -> (map [12, 20], mask bool [12, 20]); background -1, foreground 1 unless a case says otherwise."""
    def blank():
        return np.full((12, 20), -1.0, np.float32), np.zeros((12, 20), bool)
    out = {}
    f, m = blank()
    f[5, 2:18] = 1.0
    m[3:8, 4:6] = m[4:7, 12:15] = True
    out["one_prediction_over_two_gt"] = (f, m)
    f, m = blank()
    m[2:10, 3:17] = True
    f[3:5, 1:6] = f[7:9, 10:19] = 1.0
    out["one_gt_under_two_predictions"] = (f, m)
    f, m = blank()
    f[2:5, 2:5] = 1.0
    m[5:8, 5:8] = True                                                                      # corners (4, 4) and (5, 5) touch diagonally
    out["diagonal_touch"] = (f, m)
    f, m = blank()
    m[4:8, 4:12] = True
    f[5, 6:8] = 1.0                                                                         # two pixels: dropped at min_area 3
    f[1, 15:19] = 1.0
    out["small_prediction_on_gt"] = (f, m)
    f, m = blank()
    f[6, 3:9] = T                                                                           # exactly the threshold
    f[8, 3:9] = np.nextafter(T, np.float32(0))                                              # one ulp below: background
    m[6:9, 5:7] = True
    out["threshold_itself"] = (f, m)
    f, m = blank()
    m[3:7, 5:14] = True
    f[4, 4:12] = 1.0
    f[4, 7] = np.nan                                                                        # cuts the prediction in two, inside the mask region
    f[5, 12] = np.inf                                                                       # inside the mask region, diagonal to the right piece
    f[10, 1] = np.nan                                                                       # a NaN on the background
    out["nan_and_inf_in_gt"] = (f, m)
    f, m = blank()
    f[2:4, 2:9] = 1.0
    out["empty_mask"] = (f, m)
    f, m = blank()
    m[2:4, 2:9] = True
    out["empty_prediction"] = (f, m)
    f, m = blank()
    out["both_empty"] = (f, m)
    out["both_full"] = (np.full((12, 20), 2.0, np.float32), np.ones((12, 20), bool))
    return out


CASES = _cases()


def test_region_cases_in_one_batch(vad):
    names = list(CASES)
    maps = np.stack([CASES[k][0] for k in names])
    masks = np.stack([CASES[k][1] for k in names])
    for connectivity in (4, 8):
        got, want = _run_and_check(vad, maps, masks, T, connectivity, 3, 0.0, 0.0, 8)
        gt, pred, counts = ({k: a[i] for i, k in enumerate(names)} for a in want)
        assert pred["one_prediction_over_two_gt"][0].tolist() == [5 * 20 + 2, 16, 5, 1] and gt["one_prediction_over_two_gt"][:2, 2:].tolist() == [[2, 1], [3, 1]]
        assert gt["one_gt_under_two_predictions"][0].tolist() == [2 * 20 + 3, 8 * 14, 6 + 14, 1]
        assert pred["one_gt_under_two_predictions"][:2, 1:].tolist() == [[10, 6, 1], [18, 14, 1]]
        assert counts["diagonal_touch"][:5].tolist() == [1, 0, 1, 0, 1] and counts["diagonal_touch"][ref.TP] == 0
        c = counts["small_prediction_on_gt"]
        assert c[:6].tolist() == [1, 0, 1, 0, 1, 1] and c[ref.TP] == 0 and c[ref.FN] == 32 and c[ref.FP] == 4 and gt["small_prediction_on_gt"][0].tolist() == [84, 32, 0, 0]
        assert pred["threshold_itself"][0].tolist() == [6 * 20 + 3, 6, 2, 1] and counts["threshold_itself"][ref.PRED_REGIONS] == 1
        c = counts["nan_and_inf_in_gt"]
        assert c[ref.NAN_PIXELS] == 2 and c[ref.GT_PIXELS] == 36 and c[ref.FN] + c[ref.TP] == 36
        assert c[:6].tolist() == ([1, 1, 2, 2, 0, 1] if connectivity == 4 else [1, 1, 2, 2, 0, 0])   # the +Inf pixel: alone under 4, joined under 8
        assert counts["empty_mask"][12:].tolist() == [0, 1, 0, 0] and counts["empty_prediction"][12:].tolist() == [0, 0, 1, 0]
        assert counts["both_empty"][12:].tolist() == [0, 0, 0, 1] and counts["both_empty"][ref.TN] == 240 and not counts["both_empty"][:9].any()
        assert counts["both_full"].tolist() == [1, 1, 1, 1, 0, 0, 240, 0, 0, 0, 0, 240, 1, 0, 0, 0]
        assert gt["both_full"][0].tolist() == pred["both_full"][0].tolist() == [0, 240, 240, 1]
        assert got.counts[:, 12:].sum().item() == len(names)
        rows = got.to_list()
        assert rows[names.index("both_full")]["gt"] == [{"root": 0, "area": 240, "hit": 240, "detected": True}]
        assert rows[names.index("diagonal_touch")]["pred"] == [{"root": 42, "area": 9, "overlap": 0, "matched": False}]
    _run_and_check(vad, maps, masks, T, 8, 1, 0.0, 0.0, 8)                                  # min_area 1: the small prediction now hits


def test_the_fraction_boundary(vad):
    """Area 8: 4 shared pixels pass a fraction of 0.5, 3 do not - on either side, in the same call."""
    maps, masks = np.full((4, 3, 10), -1.0, np.float32), np.zeros((4, 3, 10), bool)
    for k, hit in enumerate((4, 3)):
        masks[k, 1, 1:9] = True                                                             # the mask region has area 8
        maps[k, 1, 1:1 + hit] = 1.0
        maps[2 + k, 1, 1:9] = 1.0                                                           # the prediction has area 8
        masks[2 + k, 1, 1:1 + hit] = True
    got, want = _run_and_check(vad, maps, masks, T, 8, 1, 0.5, 0.5, 2)
    assert want[0][:2, 0].tolist() == [[11, 8, 4, 1], [11, 8, 3, 0]] and want[1][2:, 0].tolist() == [[11, 8, 4, 1], [11, 8, 3, 0]]
    assert got.gt_detected[:2, 0].tolist() == [True, False] and got.pred_matched[2:, 0].tolist() == [True, False]
    assert got.gt_hit[:2, 0].tolist() == [4, 3] and got.pred_overlap[2:, 0].tolist() == [4, 3] and got.gt_area[0, 0].item() == got.pred_area[2, 0].item() == 8
    assert want[2][:, ref.FALSE_ALARMS].tolist() == [0, 0, 0, 1]
    for fractions in ((0.375, 0.375), (1.0, 1.0), (0.3, 0.7), (0.1, 0.1), (1.0 / 3.0, 2.0 / 3.0)):   # products that round, on both sides
        rng = np.random.default_rng(222)
        m, k = _random_pair(rng, 2, 23, 31, 0.5)
        _run_and_check(vad, m, k, T, 4, 1, *fractions, 128)


# ------------------------------------------------------------------------------------------ formats, truncation, leading shapes
def test_every_mask_format(vad):
    rng = np.random.default_rng(223)
    maps, masks = _random_pair(rng, 2, 23, 31)
    want = ref.match_batch(maps, masks, T, 8, 2, 0.25, 0.25, 64)
    dev = torch.from_numpy(maps).cuda()
    f32 = np.where(masks, np.float32(0.50001), np.float32(0.5)).astype(np.float32)          # 0.5 itself is normal
    f32[0, 0, :5] = np.where(masks[0, 0, :5], np.float32(7.0), np.float32(-3.0))
    u8 = np.where(masks, 128, 127).astype(np.uint8)                                         # 127 is normal
    u8[1, 0, :5] = np.where(masks[1, 0, :5], 255, 0)
    ints = np.where(masks, -3, 0)
    half = np.where(masks, np.float16(0.5004883), np.float16(0.5))                          # the next half above 0.5
    for sent in (torch.from_numpy(f32), torch.from_numpy(f32).double(), torch.from_numpy(half), torch.from_numpy(u8), torch.from_numpy(masks),
                 torch.from_numpy(ints.astype(np.int64)), torch.from_numpy(ints.astype(np.int8)), torch.from_numpy(u8)[:, None]):
        if sent.is_floating_point():
            assert np.array_equal(sent.float().numpy() > 0.5, masks)
        _assert_equal(vad.metrics.match_regions(dev, sent.cuda(), float(T), 8, 2, 0.25, 0.25), want)


def test_max_regions_one_keeps_the_counts_full(vad):
    rng = np.random.default_rng(224)
    maps, masks = _random_pair(rng, 3, 23, 31, 0.3)
    got, want = _run_and_check(vad, maps, masks, T, 4, 1, 0.0, 0.0, 1)
    full = ref.match_batch(maps, masks, T, 4, 1, 0.0, 0.0, 4096)
    assert np.array_equal(want[2], full[2]) and want[2][:, ref.GT_REGIONS].min() > 3 and want[2][:, ref.PRED_REGIONS].min() > 3
    assert np.array_equal(want[0][:, 0], full[0][:, 0]) and np.array_equal(want[1][:, 0], full[1][:, 0])
    assert got.truncated().tolist() == [True, True, True] and tuple(got.gt_records.shape) == (3, 1, 4)
    assert all(len(r["gt"]) == 1 and len(r["pred"]) == 1 for r in got.to_list())


def test_clips_and_leading_shapes(vad):
    rng = np.random.default_rng(225)
    maps, masks = _random_pair(rng, 6, 16, 24)
    want = ref.match_batch(maps, masks, T, 8, 2, 0.0, 0.5, 16)
    t, m = torch.from_numpy(maps).cuda(), torch.from_numpy(masks).cuda()
    got = vad.metrics.match_regions(t.view(3, 2, 1, 16, 24), m.view(3, 2, 1, 16, 24), float(T), 8, 2, 0.0, 0.5, 16)   # [B,T,1,H,W]
    assert tuple(got.gt_records.shape) == (3, 2, 16, 4) and tuple(got.counts.shape) == (3, 2, 16) and tuple(got.truncated().shape) == (3, 2)
    assert tuple(got.gt_detected.shape) == (3, 2, 16) and len(got.to_list()) == 6
    _assert_equal(got, want)
    _assert_equal(vad.metrics.match_regions(t[:, None], m[:, None].float(), float(T), 8, 2, 0.0, 0.5, 16), want)       # [B,1,H,W]
    _assert_equal(vad.metrics.match_regions(t[:, None], m, float(T), 8, 2, 0.0, 0.5, 16), want)                        # masks [B,H,W]
    flat = torch.zeros(maps.size + 1, device="cuda")
    flat[1:] = t.reshape(-1)
    sliced = flat[1:].view(*maps.shape)
    assert sliced.data_ptr() % 16 == 4 and sliced.is_contiguous()
    _assert_equal(vad.metrics.match_regions(sliced, m, float(T), 8, 2, 0.0, 0.5, 16), want)
    strided = torch.from_numpy(np.ascontiguousarray(maps.transpose(0, 2, 1))).cuda().transpose(1, 2)
    _assert_equal(vad.metrics.match_regions(strided, m, float(T), 8, 2, 0.0, 0.5, 16), want)
    empty = vad.metrics.match_regions(t[:0], m[:0], float(T))
    assert tuple(empty.gt_records.shape) == (0, 64, 4) and tuple(empty.counts.shape) == (0, 16) and empty.to_list() == []
    VadError = vad.hip.VadError
    for bad_maps, bad_masks, word in ((t, m[:5], "do not match"), (t, m.cpu(), "no CPU fallback"), (t.cpu(), m, "no CPU fallback"), (t.double(), m, "float32"),
                                      (t[:, None, None].expand(6, 2, 2, 16, 24), m[:, None, None].expand(6, 2, 2, 16, 24), "maps must be")):
        with pytest.raises(VadError, match=word):
            vad.metrics.match_regions(bad_maps, bad_masks, float(T))


# ------------------------------------------------------------------------------------------ identities
def test_identities_with_detect_regions_and_label_regions(vad):
    rng = np.random.default_rng(226)
    maps, masks = _random_pair(rng, 4, 40, 70, 0.4)
    t, m = torch.from_numpy(maps).cuda(), torch.from_numpy(masks).cuda()
    for connectivity, min_area in ((8, 1), (4, 3)):
        got = vad.metrics.match_regions(t, m, float(T), connectivity, min_area, 0.5, 0.5, 4096)
        regions = vad.metrics.detect_regions(t, float(T), connectivity, min_area, 4096)
        assert torch.equal(got.pred_records[..., :2], regions.records[..., :2]) and regions.counts[:, 0].min() > 0
        assert torch.equal(got.counts[:, 2], regions.counts[:, 0].long()) and torch.equal(got.counts[:, 5], regions.counts[:, 1].long())
        assert torch.equal(got.counts[:, 10], regions.counts[:, 3].long())
        labels, sizes = vad.metrics.label_regions(m, connectivity)
        for f in range(4):
            roots = torch.nonzero(sizes[f].reshape(-1).view(torch.int32)).reshape(-1)
            k = len(roots)
            assert k == got.counts[f, 0].item() > 0
            assert torch.equal(got.gt_records[f, :k, 0], roots.int()) and torch.equal(got.gt_records[f, :k, 1], sizes[f].reshape(-1).view(torch.int32)[roots])
            assert not got.gt_records[f, k:].any()
        c = got.counts
        assert torch.equal(got.gt_hit.sum(-1).long(), c[:, 6]) and torch.equal(got.pred_overlap.sum(-1).long(), c[:, 6])   # sum hit = sum overlap = TP
        assert (c[:, 6:10].sum(-1) == 40 * 70).all() and torch.equal(c[:, 6] + c[:, 8], c[:, 11]) and torch.equal(c[:, 2] - c[:, 3], c[:, 4])
        assert torch.equal(got.gt_detected.sum(-1), c[:, 1]) and torch.equal(got.pred_matched.sum(-1), c[:, 3]) and (c[:, 12:].sum(-1) == 1).all()


def test_any_batching_gives_the_same_words(vad):
    rng = np.random.default_rng(227)
    masks = np.concatenate([pro_ref.blobs(rng, 4, 40, 56), np.ones((1, 40, 56), bool), np.zeros((1, 40, 56), bool)])
    fg = np.concatenate([pro_ref.blobs(rng, 3, 40, 56, count=8), np.ones((1, 40, 56), bool), rng.random((2, 40, 56)) < 0.5])
    maps = torch.from_numpy(regions_ref.map_from_mask(rng, fg, T)).cuda()
    m = torch.from_numpy(masks).cuda()
    args = (float(T), 8, 2, 0.25, 0.5, 16)
    whole = vad.metrics.match_regions(maps, m, *args)
    _assert_equal(whole, ref.match_batch(maps.cpu().numpy(), masks, T, 8, 2, 0.25, 0.5, 16))
    backwards = vad.metrics.match_regions(maps.flip(0), m.flip(0), *args)
    for i in range(len(maps)):
        single = vad.metrics.match_regions(maps[i:i + 1], m[i:i + 1], *args)
        for other, k in ((single, 0), (backwards, -1 - i)):
            assert torch.equal(other.gt_records[k], whole.gt_records[i]) and torch.equal(other.pred_records[k], whole.pred_records[i])
            assert torch.equal(other.counts[k], whole.counts[i])
    again = vad.metrics.match_regions(maps, m, *args)
    assert torch.equal(again.gt_records, whole.gt_records) and torch.equal(again.pred_records, whole.pred_records) and torch.equal(again.counts, whole.counts)
    sums = vad.metrics.DetectionCounts("cuda").update(whole)
    halves = vad.metrics.DetectionCounts("cuda").update(vad.metrics.match_regions(maps[:2], m[:2], *args)).merge(
        vad.metrics.DetectionCounts("cuda").update(vad.metrics.match_regions(maps[2:], m[2:], *args)))
    assert torch.equal(sums.counts, halves.counts) and torch.equal(sums.counts, whole.counts.sum(0)) and sums.all_reduce() == 1
    assert sums.report()["frames"] == 6 and sums.params == whole.params
    with pytest.raises(ValueError, match="gathered with"):
        sums.update(vad.metrics.match_regions(maps[:1], m[:1], float(T), 8, 3, 0.25, 0.5, 16))


# ------------------------------------------------------------------------------------------ the C ABI: poisoned buffers, capture
def test_a_captured_call_follows_new_contents(vad):
    """Every launch is asynchronous on the caller's stream and nothing is allocated: one call on a poisoned workspace, captured on a
    side stream and replayed on new contents of the same buffers, equals the restatement; n == 0 touches the flag word only."""
    lib = vad.hip.lib()
    rng = np.random.default_rng(228)
    contents = [(regions_ref.map_from_mask(rng, pro_ref.blobs(rng, 3, 40, 56, count=c), T), pro_ref.blobs(rng, 3, 40, 56, count=c)) for c in (6, 9)]
    n, h, w = contents[0][0].shape
    maps = torch.from_numpy(contents[0][0]).cuda()
    masks = torch.from_numpy(contents[0][1].astype(np.float32)).cuda()
    need = lib.vad_match_workspace_bytes(n, h, w)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    gt = torch.full((n, 16, 4), -7, dtype=torch.int32, device="cuda")
    pred = torch.full((n, 16, 4), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((n, 16), -7, dtype=torch.int64, device="cuda")

    def call(frames=n, size=need):
        return lib.vad_match_regions(maps.data_ptr(), masks.data_ptr(), vad.hip.LBL_F32_ELEM, frames, h, w, float(T), 8, 2, 0.25, 0.5, 16, gt.data_ptr(),
                                     pred.data_ptr(), counts.data_ptr(), ws.data_ptr(), size, vad.hip.current_stream())

    def check(k):
        want = ref.match_batch(contents[k][0], contents[k][1], T, 8, 2, 0.25, 0.5, 16)
        assert torch.equal(gt.cpu(), _i32(want[0])) and torch.equal(pred.cpu(), _i32(want[1])) and torch.equal(counts.cpu(), _i64(want[2]))
        assert int(ws[:4].view(torch.int32).item()) == 0

    assert call() == 0                                                                       # once eagerly, on the poisoned workspace
    check(0)
    before = (gt.clone(), pred.clone(), counts.clone())
    assert call(size=need - 1) == -3 and b"ws_bytes" in lib.vad_last_error()
    ws.fill_(0xAB)
    assert call(frames=0, size=16) == 0
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[16:] == 0xAB).all())
    assert torch.equal(gt, before[0]) and torch.equal(pred, before[1]) and torch.equal(counts, before[2])
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            vad.hip.check(call(), "vad_match_regions")
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 0):
        maps.copy_(torch.from_numpy(contents[k][0]).cuda())
        masks.copy_(torch.from_numpy(contents[k][1].astype(np.float32)).cuda())
        for buf in (gt, pred, counts):
            buf.fill_(-7)
        graph.replay()
        check(k)
    eager = vad.metrics.match_regions(maps, masks, float(T), 8, 2, 0.25, 0.5, 16)
    assert torch.equal(eager.gt_records, gt) and torch.equal(eager.pred_records, pred) and torch.equal(eager.counts, counts)


# ------------------------------------------------------------------------------------------ through the models
def _same_report(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k] or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def _check_report(vad, model, key, x, masks, split, lead_hw):
    """detection_report over two ragged batches against the concatenated maps, the restatement, and two merged halves."""
    kw = dict(sigma=1.0, morph=("open", 2), connectivity=4, min_area=2, gt_fraction=0.25, pred_fraction=0.1)
    loader = [{key: x[:split], "mask": masks[:split]}, {key: x[split:], "mask": masks[split:]}]
    with torch.no_grad():
        maps = torch.cat([vad.scoring._anomaly_maps(model, b[key], "mse", 1.0, 4.0, None, None, vad.metrics.morph_steps(("open", 2))) for b in loader])
    t = float(np.float32(np.quantile(maps.cpu().numpy(), 0.85)))
    before = vad.hip.calls.get("match_regions", 0)
    report, counts = vad.scoring.detection_report(model, loader, "cuda", t, **kw)
    assert vad.hip.calls["match_regions"] == before + 2
    whole = vad.metrics.match_regions(maps, masks, t, 4, 2, 0.25, 0.1)
    want = ref.match_batch(maps.cpu().numpy().reshape(-1, *lead_hw), masks.cpu().numpy().reshape(-1, *lead_hw) > 0.5, t, 4, 2, 0.25, 0.1)
    _assert_equal(whole, want)
    sums = want[2].sum(0)
    print(f"{key}: threshold {t!r} sums {sums.tolist()}")
    assert counts.counts.is_cuda and torch.equal(counts.counts.cpu(), _i64(sums)) and sums[ref.TP] > 0 and sums[ref.FP] > 0 and sums[ref.FN] > 0
    assert report["frames"] == len(want[2]) and report["params"]["threshold"] == t and report["params"]["morph"] == (("open", (2, 2)),)
    direct = vad.metrics.DetectionCounts("cuda").update(whole).report()
    direct["params"] = report["params"]                                                     # the report carries the map's description too
    _same_report(report, direct)
    first = vad.scoring.detection_report(model, loader[:1], "cuda", t, **kw)[1]
    second = vad.scoring.detection_report(model, loader[1:], "cuda", t, **kw)[1]
    merged = first.merge(second)
    assert torch.equal(merged.counts, counts.counts)
    _same_report(merged.report(), report)
    continued = vad.scoring.detection_report(model, loader[1:], "cuda", t, counts=vad.scoring.detection_report(model, loader[:1], "cuda", t, **kw)[1], **kw)[1]
    assert torch.equal(continued.counts, counts.counts)
    with pytest.raises(ValueError, match="gathered with"):
        vad.scoring.detection_report(model, loader[:1], "cuda", t, counts=counts, **{**kw, "min_area": 3})
    with pytest.raises(ValueError, match="gathered with"):
        vad.scoring.detection_report(model, loader[:1], "cuda", t, counts=counts, **{**kw, "sigma": 2.0})


def test_detection_report_through_the_image_model(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    masks = torch.from_numpy(pro_ref.blobs(np.random.default_rng(229), 6, 32, 32, count=3, radius=5).astype(np.float32))[:, None].cuda()
    _check_report(vad, model, "image", x, masks, 4, (32, 32))
    with pytest.raises(vad.hip.VadError, match="map"):
        vad.scoring.detection_report(model, [], "cuda", 0.5, map="psnr")


def test_detection_report_through_the_video_model(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 3, 4, 3, 32, 32)).cuda()
    masks = torch.from_numpy(pro_ref.blobs(np.random.default_rng(230), 12, 32, 32, count=3, radius=5).astype(np.float32)).view(3, 4, 1, 32, 32).cuda()
    _check_report(vad, model, "frames", clips, masks, 2, (32, 32))
    with pytest.raises(vad.hip.VadError, match="map='mse'"):
        vad.scoring.detection_report(model, [{"frames": clips, "mask": masks}], "cuda", 0.5, map="ssim")
