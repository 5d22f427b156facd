"""One batch past 2^31 elements: a device tensor of (2050, 1024, 1024) float32 - 2^31 + 2^21 elements,
8.6 GB, the smallest batch of whole frames in which frame 1024 begins at byte 2^32 and frames 2048 and 2049 at or behind element
2^31 (byte 2^33) - through the map entry points whose kernels carry `size_t` / `long long` offsets, and through the three launches
of 2^30 elements of `vad_hist_accumulate`.  Frame i is entry i % 7 of seven seeded frames (tests/frame_pool_ref.py): the
restatements run on the seven, every check of a full-size output runs on the device against the index expansion, ten periods at a
time, and one full-size output exists at a time.  The module's peak of `torch.cuda.max_memory_allocated()` is 58 GiB (the labelling
workspaces of `match_regions` over 2^31 pixels); its fixture skips below 40 GiB of free device memory."""
import numpy as np
import pytest
import torch

import frame_pool_ref as FP
import map_morph_ref
import map_smooth_ref
import map_stats_ref
import map_temporal_ref
import map_topk_ref
import match_ref
import pixel_metrics_ref
import regions_ref
from test_hip_frame_counts import Calls, _same, _up

pytestmark = pytest.mark.gpu

N, H, W, BP, T = FP.BIG_N, FP.BIG_H, FP.BIG_W, FP.BIG_P, FP.T
PERIODS = 10                                # the periods of 7 frames one comparison takes: 280 MB of expected values
NEED_FREE = 40 << 30


class Big:
    def __init__(self):
        self.pool = FP.big_frames()
        self.masks = FP.big_masks(self.pool)
        self.index = torch.arange(N, device="cuda") % BP
        self.x = _up(self.pool)[self.index]                                  # [2050, 1024, 1024]
        assert self.x.numel() == 2 ** 31 + 2 ** 21 and self.x.is_contiguous()

    def expand(self, per_item):
        return _up(per_item)[self.index]

    def same(self, got, per_item, any_nan=False):
        """A full-size output [2050, ...] against the expansion of the seven expected items, PERIODS periods at a time."""
        want = _up(per_item)
        assert got.shape[0] == N and tuple(got.shape[1:]) == tuple(want.shape[1:]), (got.shape, want.shape)
        block = want.repeat(PERIODS, *([1] * (want.dim() - 1)))
        for at in range(0, N, BP * PERIODS):
            part = got[at:at + BP * PERIODS]
            if not _same(part, block[:part.shape[0]], any_nan):
                return False
        return True


@pytest.fixture(scope="module")
def big():
    free, _ = torch.cuda.mem_get_info()
    if free < NEED_FREE:
        pytest.skip(f"{free >> 30} GiB of device memory are free; the 8.6 GB batch and its outputs need {NEED_FREE >> 30}")
    torch.cuda.reset_peak_memory_stats()
    b = Big()
    yield b
    print(f"peak device memory of the module: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    del b.x, b.index
    torch.cuda.empty_cache()


def test_the_boundary_frames(big):
    """Frame 1024 begins at byte 2^32, frame 2048 at element 2^31; both and frame 2049 hold the pool entries their index says."""
    x = big.x
    assert x[1024].data_ptr() - x.data_ptr() == 2 ** 32 and x[2048].data_ptr() - x.data_ptr() == 2 ** 33
    for f in (1023, 1024, 2047, 2048, 2049):
        assert _same(x[f], _up(big.pool[f % BP]))
    assert big.same(x, big.pool)


def test_smooth_maps(vad, big):
    want = map_smooth_ref.smooth(big.pool, 0.5)
    with Calls(vad, smooth_maps=1):
        got, gmax = vad.metrics.smooth_maps(big.x, 0.5, return_max=True)
    assert big.same(got, want, any_nan=True), "smoothed maps differ from the expansion"
    assert _same(gmax, big.expand(map_smooth_ref.frame_max(want)), any_nan=True)


def test_morph_maps(vad, big):
    with Calls(vad, morph_maps=1):
        got = vad.metrics.morph_maps(big.x, "dilate", 3)
    assert big.same(got, map_morph_ref.morph("dilate", big.pool, 3)), "dilated maps differ from the expansion"


def test_map_statistics(vad, big):
    stats = vad.metrics.MapStatistics((H, W))
    with Calls(vad, mapstat_accumulate=1):
        stats.update(big.x)
    assert stats.device_count() == N
    state = FP.weighted_stats(big.pool, N)
    mean, std = stats.mean().cpu().numpy(), stats.std().cpu().numpy()
    mean64 = state.K + state.S1 / N
    std64 = np.sqrt(np.maximum((state.S2 - state.S1 * (state.S1 / N)) / (N - 1.0), 0.0))
    want_mean, want_std = map_stats_ref.finalize(state)
    print(f"mean within {map_stats_ref.ulps32(mean, mean64):.3f} ulp, std within {map_stats_ref.ulps32(std, std64):.3f} ulp")
    assert FP.stats_within_bound(mean, want_mean, mean64) and FP.stats_within_bound(std, want_std, std64)
    z = map_stats_ref.normalize(big.pool, mean, std, 1e-3)
    work = big.x.clone()
    with Calls(vad, map_normalize=1):
        got, gmax = stats.normalize(work, 1e-3, out=work, return_max=True)
    assert got is work and big.same(work, z, any_nan=True), "z-scores differ from the expansion"
    assert _same(gmax, big.expand(map_stats_ref.frame_max(z)), any_nan=True)


@pytest.mark.parametrize("step", [("max", 3), ("ema", 0.5)], ids=["max", "ema"])
def test_temporal_maps_clips_of_one_frame(vad, big, step):
    want = map_temporal_ref.clips([step], big.pool[:, None])
    with Calls(vad, tfilt_maps=1):
        got = vad.metrics.temporal_maps(big.x.view(N, 1, H, W), *step)
    assert big.same(got, want), "filtered one-frame clips differ from the expansion"


def test_temporal_maps_one_clip_of_all_frames(vad, big):
    """One stream of 2050 frames under ("max", 3): the restatement on the first 16 frames; behind them the input has period 7, so
    out[t] == out[t - 7] for t >= 9, checked on the device."""
    head = map_temporal_ref.clips([("max", 3)], big.pool[FP.index(16, BP)][None])
    with Calls(vad, tfilt_maps=1):
        got = vad.metrics.temporal_maps(big.x.view(1, N, H, W), "max", 3)
    assert _same(got[:, :16], _up(head))
    assert _same(got[0, 9:], got[0, 2:N - 7]), "the filtered stream loses its period of seven frames"


def test_map_topk_split_path(vad, big):
    ranks = [1, 1000, 2 ** 20]
    want = map_topk_ref.topk(big.pool, ranks)
    with Calls(vad, map_topk=1):
        got = vad.metrics.map_topk(big.x, ranks)
    assert _same(got["kth"], big.expand(want["kth"])), "kth differs from the expansion"
    index = FP.index(N, BP)
    assert map_topk_ref.mean_within_bound(got["mean"].cpu().numpy(), {"exact": want["exact"][index], "bound": want["bound"][index]})
    assert _same(got["mean"], got["mean"][:BP][big.index])


def test_detect_regions(vad, big):
    records, counts, _ = regions_ref.detect_batch(big.pool, T, 8, 1, 64)
    assert counts[:, 0].min() > 64 // 2
    with Calls(vad, detect_regions=1):
        got = vad.metrics.detect_regions(big.x, float(T), 8, 1, 64)
    assert got.labels is None
    assert _same(got.records, big.expand(records)), "records differ from the expansion"
    assert _same(got.counts, big.expand(counts)), "counts differ from the expansion"


def test_match_regions(vad, big):
    gt, pred, counts = match_ref.match_batch(big.pool, big.masks, T, 8, 1, 0.0, 0.0, 64)
    assert counts[:, match_ref.GT_DETECTED].min() > 0 and counts[:, match_ref.FALSE_ALARMS].min() > 0
    m = big.expand(np.where(big.masks, 200, 100).astype(np.uint8))
    with Calls(vad, match_regions=1):
        got = vad.metrics.match_regions(big.x, m, float(T), 8, 1, 0.0, 0.0, 64)
    assert _same(got.gt_records, big.expand(gt)) and _same(got.pred_records, big.expand(pred)), "records differ from the expansion"
    assert _same(got.counts, big.expand(counts)), "counts differ from the expansion"
    total = vad.metrics.DetectionCounts("cuda").update(got)
    assert total.counts.cpu().tolist() == FP.weighted_counts(counts.view(np.int64), N).tolist()


@pytest.mark.parametrize("labels", ["per_frame", "per_element"])
def test_score_histogram_three_launches(vad, big, labels):
    """2^31 + 2^21 values: launches of 2^30, 2^30 and 2^21 elements; the group of a value is found from `base` + its index."""
    assert 2 * FP.HIST_LAUNCH_ELEMS < big.x.numel() <= 3 * FP.HIST_LAUNCH_ELEMS
    m = 11
    if labels == "per_frame":
        frame_pos = (np.arange(BP) % 3 == 1)                                 # entries 1 and 4 are anomalous frames
        pos = np.broadcast_to(frame_pos[:, None, None], big.pool.shape)
        lab = _up(frame_pos.astype(np.uint8))[big.index]                     # [2050]
        values = big.x.view(N, H * W)
    else:
        pos = big.masks
        lab = big.expand(np.where(big.masks, 255, 0).astype(np.uint8)).view(-1)
        values = big.x.view(-1)
    per_item = [pixel_metrics_ref.ref_counts(big.pool[j], pos[j], m) for j in range(BP)]
    counts = FP.weighted_counts(np.stack([c for c, _ in per_item]), N)
    rejected = FP.weighted_counts(np.stack([r for _, r in per_item]), N)
    hist = vad.metrics.ScoreHistogram(m)
    with Calls(vad, hist_accumulate=1):
        hist.accumulate(values, lab)
    assert torch.equal(hist.counts().cpu(), torch.from_numpy(counts)), "counts differ from the pool's times the multiplicities"
    assert hist.rejected().cpu().tolist() == rejected.tolist() and rejected.min() > 0
    assert int(hist.counts().sum() + hist.rejected().sum()) == N * 2 ** 20
