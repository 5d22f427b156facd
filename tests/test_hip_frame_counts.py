"""More frames than one launch takes: every anomaly-map entry point on N3 = 131075, N2 = 65541 or
NZ = 262145 tiny frames, so that the second and third launch slice of 65535 frames (the host loops `f0 += 65535`) and the second
and third round of the grid-stride loops (`img += gridDim.y`) run under a test.  Batch item i is entry i % 251 of a pool
(tests/frame_pool_ref.py); the restatements of the operations' own test files run on the 251 pool items only, their results are
expanded by the same index on the device, and every output of the big call is compared with the expansion there, bit for bit.
Additive states equal the pool items' integer counts times their multiplicities.  Every case also asserts that the Python layer
made exactly the native calls one batch costs."""
import numpy as np
import pytest
import torch

import event_tracks_ref
import events_ref
import frame_bank_ref
import frame_pool_ref as FP
import hip_helpers as H
import map_morph_ref
import map_smooth_ref
import map_stats_ref
import map_temporal_ref
import map_topk_ref
import match_ref
import pro_ref
import regions_ref
import resize_formats_ref
import resize_ref
import track_ref

pytestmark = pytest.mark.gpu

P, N3, N2, NZ, T = FP.P, FP.N3, FP.N2, FP.NZ, FP.T
GUARD = 64                                  # elements on either side of an output of the caller's (keeps its 256-byte alignment)
FILTERS = (("min", 2), ("max", 3), ("mean", 2), ("ema", 0.5))


# ------------------------------------------------------------------------------------------ device-side helpers
def _idx(n, p=P):
    return torch.arange(n, device="cuda") % p


def _up(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _expand(per_item, n):
    """Per-item expected values [p, ...] (numpy) -> the batch's [n, ...] on the device."""
    t = _up(per_item)
    return t[_idx(n, t.shape[0])]


def _words(t):
    t = t.contiguous()
    if t.dtype == torch.float32 or t.dtype == torch.uint32:
        return t.view(torch.int32)
    if t.dtype == torch.float64 or t.dtype == torch.uint64:
        return t.view(torch.int64)
    return t


def _same(got, want, any_nan=False):
    """Bit identity on the device.  `any_nan`: where the restatement GENERATES a NaN (Inf - Inf, a NaN operand of an addition) its
    sign and payload are the processor's, so a NaN of the restatement matches any NaN; everything else matches on its bits."""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    if not any_nan:
        return torch.equal(_words(got), _words(want))
    nan = torch.isnan(want)
    zero = torch.zeros((), dtype=torch.int32, device=got.device)
    return torch.equal(torch.isnan(got), nan) and torch.equal(torch.where(nan, zero, _words(got)), torch.where(nan, zero, _words(want)))


class Guarded:
    """An output tensor of the caller's between two guards of GUARD elements; `ok()`: the guards kept their bits."""

    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.fill = 0xA5 if dtype == torch.uint8 else -7.0
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.out = self.buf[GUARD:GUARD + n].view(shape)
        self.n = n
        if dtype == torch.float32:
            self.out.fill_(float("nan"))
        assert self.out.is_contiguous() and self.out.data_ptr() % 16 == self.buf.data_ptr() % 16

    def ok(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all())


class Calls:
    """`with Calls(vad, name=k, ...)`: the launch counters rose by exactly k inside the block."""

    def __init__(self, vad, **want):
        self.calls, self.want = vad.hip.calls, want

    def __enter__(self):
        self.before = {k: self.calls.get(k, 0) for k in self.want}

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            got = {k: self.calls.get(k, 0) - self.before[k] for k in self.want}
            assert got == self.want, f"native calls {got}, expected {self.want}"


# ------------------------------------------------------------------------------------------ 1. smooth_maps
def test_smooth_maps_three_slices(vad):
    pool = FP.pool((4, 6), 9101)
    want = map_smooth_ref.smooth(pool, 0.5)
    want_max = map_smooth_ref.frame_max(want)
    x = _expand(pool, N3)
    w, wm = _expand(want, N3), _expand(want_max, N3)
    with Calls(vad, smooth_maps=1):
        got, gmax = vad.metrics.smooth_maps(x, 0.5, return_max=True)
    assert _same(got, w, any_nan=True) and _same(gmax, wm, any_nan=True)
    g = Guarded((N3, 4, 6))
    with Calls(vad, smooth_maps=1):
        assert vad.metrics.smooth_maps(x, 0.5, out=g.out) is g.out
    assert _same(g.out, w, any_nan=True) and g.ok()
    with Calls(vad, smooth_maps=1):
        only = vad.metrics.smooth_maps(x, 0.5, return_max="only")
    assert _same(only, wm, any_nan=True)
    assert _same(x, _expand(pool, N3))                                       # the input is not touched


def test_smooth_maps_two_tiles_per_frame(vad):
    """(N2, 2, 70): the tile-max workspace of the second slice begins at f0 * tiles with tiles = 2."""
    assert vad.hip.SMOOTH_TILE[1] < 70 <= 2 * vad.hip.SMOOTH_TILE[1]
    pool = FP.pool((2, 70), 9102)
    want = map_smooth_ref.smooth(pool, 0.5)
    x = _expand(pool, N2)
    with Calls(vad, smooth_maps=1):
        got, gmax = vad.metrics.smooth_maps(x, 0.5, return_max=True)
    assert _same(got, _expand(want, N2), any_nan=True) and _same(gmax, _expand(map_smooth_ref.frame_max(want), N2), any_nan=True)


# ------------------------------------------------------------------------------------------ 2. morph_maps, apply_morph
def test_morph_maps_three_slices(vad):
    pool = FP.pool((4, 6), 9201)
    x = _expand(pool, N3)
    g = Guarded((N3, 4, 6))
    for size in (3, (2, 3)):
        for op in map_morph_ref.OPS:
            with Calls(vad, morph_maps=1):
                assert vad.metrics.morph_maps(x, op, size, out=g.out) is g.out
            assert _same(g.out, _expand(map_morph_ref.morph(op, pool, size), N3)), (op, size)
            assert g.ok()
    with Calls(vad, morph_maps=1):
        got = vad.metrics.morph_maps(x, "open", 3)                               # the output the call allocates itself
    assert _same(got, _expand(map_morph_ref.morph("open", pool, 3), N3))
    steps = vad.metrics.morph_steps([("open", 2), ("dilate", (3, 2)), ("erode", 3)])   # three steps: both buffers are reused
    want = pool
    for op, size in steps:
        want = map_morph_ref.morph(op, want, size)
    with Calls(vad, morph_maps=3):
        got = vad.metrics.apply_morph(x, steps)
    assert _same(got, _expand(want, N3)) and _same(x, _expand(pool, N3))


def test_morph_maps_two_tiles_per_frame(vad):
    pool = FP.pool((2, 70), 9202)
    x = _expand(pool, N2)
    with Calls(vad, morph_maps=1):
        got = vad.metrics.morph_maps(x, "dilate", 3)
    assert _same(got, _expand(map_morph_ref.morph("dilate", pool, 3), N2))


# ------------------------------------------------------------------------------------------ 3. MapStatistics
def _stats_case(vad, h, w, seed, in_place_only):
    pool = FP.pool((h, w), seed)
    x = _expand(pool, NZ)
    stats = vad.metrics.MapStatistics((h, w))
    with Calls(vad, mapstat_accumulate=1):
        stats.update(x)
    assert stats.device_count() == NZ == stats.count
    state = FP.weighted_stats(pool, NZ)
    mean, std = stats.mean().cpu().numpy(), stats.std().cpu().numpy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mean64 = state.K + state.S1 / NZ
        var64 = np.maximum((state.S2 - state.S1 * (state.S1 / NZ)) / (NZ - 1.0), 0.0)
        std64 = np.sqrt(var64)
    want_mean, want_std = map_stats_ref.finalize(state)
    print(f"{h}x{w}: mean within {map_stats_ref.ulps32(mean[np.isfinite(mean64)], mean64[np.isfinite(mean64)]):.3f} ulp, "
          f"std within {map_stats_ref.ulps32(std[np.isfinite(std64)], std64[np.isfinite(std64)]):.3f} ulp")
    assert FP.stats_within_bound(mean, want_mean, mean64) and FP.stats_within_bound(std, want_std, std64)
    assert np.isnan(std).sum() == 3                                          # the NaN, +Inf and -Inf pixels of the non-finite entry
    # the z-scores: the restatement with the device's own mean and std, so that every bit is specified
    z = map_stats_ref.normalize(pool, mean, std, 1e-3)
    zmax = _expand(map_stats_ref.frame_max(z), NZ)
    if not in_place_only:
        with Calls(vad, map_normalize=1):
            got, gmax = stats.normalize(x, 1e-3, return_max=True)
        assert _same(got, _expand(z, NZ), any_nan=True) and _same(gmax, zmax, any_nan=True)
        del got
        g = Guarded((NZ, h, w))
        with Calls(vad, map_normalize=1):
            assert stats.normalize(x, 1e-3, out=g.out) is g.out
        assert _same(g.out, _expand(z, NZ), any_nan=True) and g.ok()
        del g
    with Calls(vad, map_normalize=1):
        got, gmax = stats.normalize(x, 1e-3, out=x, return_max=True)              # in place
    assert got is x and _same(x, _expand(z, NZ), any_nan=True) and _same(gmax, zmax, any_nan=True)


def test_map_statistics_two_normalize_slices(vad):
    assert NZ > FP.NZ_SLICE and 3 * 5 <= FP.NZ_CHUNK
    _stats_case(vad, 3, 5, 9301, in_place_only=False)


def test_map_statistics_two_chunks_per_frame(vad):
    """(NZ, 5, 205), 1.07 GB: 1025 pixels are two chunks, so the chunk-max workspace of the second slice begins at f0 * 2."""
    lib = vad.hip.lib()
    assert lib.vad_map_normalize_workspace_bytes(1, 1, FP.NZ_CHUNK) == 4 and lib.vad_map_normalize_workspace_bytes(1, 5, 205) == 8
    _stats_case(vad, 5, 205, 9302, in_place_only=True)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ 4. temporal filters
def _nan_rule(op):
    return op in ("mean", "ema")                                             # min / max move bits; mean / ema compute


@pytest.mark.parametrize("n,w", [(N3, 6), (N2, 5)], ids=["f32x4_three_slices", "scalar_two_slices"])
def test_temporal_maps_clip_mode(vad, n, w):
    assert ((2 * w) % 4 == 0) == (w == 6)                                    # 12 pixels: the 16-byte kernel; 10: the scalar one
    pool = FP.pool((3, 2, w), 9400 + w)
    x = _expand(pool, n)
    g = Guarded((n, 3, 2, w))
    for step in FILTERS:
        with Calls(vad, tfilt_maps=1):
            assert vad.metrics.temporal_maps(x, *step, out=g.out) is g.out
        assert _same(g.out, _expand(map_temporal_ref.clips([step], pool), n), any_nan=_nan_rule(step[0])), step
        assert g.ok()
    steps = vad.metrics.temporal_steps([("min", 2), ("max", 3), ("mean", 2)])
    with Calls(vad, tfilt_maps=3):
        got = vad.metrics.apply_temporal(x, steps)
    assert _same(got, _expand(map_temporal_ref.clips(steps, pool), n), any_nan=True)
    assert _same(x, _expand(pool, n))


@pytest.mark.parametrize("step", FILTERS, ids=[s[0] for s in FILTERS])
def test_temporal_filter_streams(vad, step):
    """N3 live streams: the state of slice s0 begins at s0 * stream_words, in the filter and in its initialisation."""
    pool = FP.pool((3, 2, 6), 9410)
    x = _expand(pool, N3)
    f = vad.metrics.TemporalFilter(N3, 2, 6, step)
    for s in f.states:                                                       # a state the initialisation has to overwrite everywhere
        s.fill_(0x5A5A5A5A)
    f.reset()
    clip = map_temporal_ref.clips([step], pool)
    nan = _nan_rule(step[0])
    with Calls(vad, tfilt_maps=2):
        first = f.update(x[:, :2].contiguous())
        g = Guarded((N3, 1, 2, 6))
        assert f.update(x[:, 2:].contiguous(), out=g.out) is g.out
    assert _same(first, _expand(clip[:, :2], N3), any_nan=nan) and _same(g.out, _expand(clip[:, 2:], N3), any_nan=nan) and g.ok()
    assert bool((f.frames_seen() == 3).all())
    # three streams restart - the last of slice 0, the first of slice 1, the first of slice 2 -, every other one goes on
    restart = [FP.SLICE - 1, FP.SLICE, 2 * FP.SLICE]
    f.reset(streams=restart)
    seen = torch.full((N3,), 3, dtype=torch.int64, device="cuda")
    seen[restart] = 0
    assert torch.equal(f.frames_seen(), seen)
    more = np.concatenate([pool, pool[:, :1]], axis=1)                       # frame 0 of every stream once more
    goes_on = _expand(map_temporal_ref.clips([step], more)[:, 3:], N3)
    fresh = _expand(map_temporal_ref.clips([step], pool[:, :1]), N3)
    want = goes_on.clone()
    want[restart] = fresh[restart]
    with Calls(vad, tfilt_maps=1):
        got = f.update(x[:, :1].contiguous())
    assert _same(got, want, any_nan=nan)
    assert torch.equal(f.frames_seen(), seen + 1)


# ------------------------------------------------------------------------------------------ 5. device Resize
def _u8_pool(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, (P, *shape), dtype=np.uint8)


@pytest.mark.parametrize("geometry", [(5, 7, 4, 6), (5, 7, 5, 6), (5, 8, 4, 8)], ids=["both_passes", "horizontal_only", "vertical_only"])
def test_resize_three_byte_frames(vad, geometry):
    ih, iw, oh, ow = geometry
    pool = _u8_pool((ih, iw, 3), 9500 + iw + oh)
    x = _expand(pool, N3)
    for order in ("rgb", "bgr"):
        src = pool if order == "rgb" else np.ascontiguousarray(pool[..., ::-1])
        want = np.stack([resize_ref.resize_ref(f, oh, ow) for f in src])
        g = Guarded((N3, oh, ow, 3), torch.uint8)
        with Calls(vad, resize_u8=1):
            vad.scoring.FrameResizer((oh, ow), channel_order=order)(x, out=g.out)
        assert _same(g.out, _expand(want, N3)) and g.ok(), order
    assert _same(x, _expand(pool, N3))


@pytest.mark.parametrize("fmt", ["l", "rgba", "bgra"])
def test_resize_one_and_four_byte_frames(vad, fmt):
    ih, iw, oh, ow = 5, 7, 4, 6
    pool = _u8_pool((ih, iw) if fmt == "l" else (ih, iw, 4), 9510 + len(fmt))
    if fmt == "l":
        want = np.stack([resize_formats_ref.l_ref(f, oh, ow, 3) for f in pool])
    else:
        want = np.stack([resize_formats_ref.rgba_ref(f, oh, ow, bgra=fmt == "bgra") for f in pool])
    x = _expand(pool, N3)
    g = Guarded((N3, oh, ow, 3), torch.uint8)
    with Calls(vad, resize_u8=1):
        vad.scoring.FrameResizer((oh, ow), pixel_format=fmt)(x, out=g.out)
    assert _same(g.out, _expand(want, N3)) and g.ok()


# ------------------------------------------------------------------------------------------ 6. the layout transposes (C ABI)
@pytest.mark.parametrize("c,cpad", [(3, 4), (5, 8)])
def test_layout_transposes(vad, c, cpad):
    lib, n, h, w = vad.hip.lib(), N3, 2, 3
    pool = FP.signed_lognormal((P, c, h, w), 9600 + c)
    pool[1, 0, 0, 0], pool[1, c - 1, 1, 2], pool[2, 1, 0, 1] = np.nan, np.inf, -0.0
    x = _expand(pool, n)                                                    # NCHW
    want = torch.zeros((n, h, w, cpad), device="cuda")
    want[..., :c] = x.permute(0, 2, 3, 1)
    g = Guarded((n, h, w, cpad))
    vad.hip.check(lib.vad_nchw_to_nhwc_padded(x.data_ptr(), g.out.data_ptr(), n, h, w, c, cpad, H.stream()))
    assert _same(g.out, want) and g.ok()
    back = Guarded((n, c, h, w))
    vad.hip.check(lib.vad_nhwc_padded_to_nchw(g.out.data_ptr(), back.out.data_ptr(), n, h, w, c, cpad, H.stream()))
    assert _same(back.out, x) and back.ok()
    # the padding channels are not read on the way back
    dirty = want.clone()
    dirty[..., c:] = 5.0
    back.out.fill_(float("nan"))
    vad.hip.check(lib.vad_nhwc_padded_to_nchw(dirty.data_ptr(), back.out.data_ptr(), n, h, w, c, cpad, H.stream()))
    assert _same(back.out, want[..., :c].permute(0, 3, 1, 2).contiguous()) and back.ok()


# ------------------------------------------------------------------------------------------ 7. detect_regions
@pytest.mark.parametrize("connectivity", (4, 8))
def test_detect_regions_three_rounds(vad, connectivity):
    pool = FP.pool((5, 7), 9700)
    records, counts, labels = regions_ref.detect_batch(pool, T, connectivity, 2, 2)
    assert (counts[:, 0] > 2).any() and (counts[:, 0] == 0).any() and (counts[:, 1] > 0).any() and (counts[:, 3] > 0).any()
    x = _expand(pool, N3)
    with Calls(vad, detect_regions=1):
        got = vad.metrics.detect_regions(x, float(T), connectivity, min_area=2, max_regions=2, return_labels=True)
    assert _same(got.records, _expand(records, N3)), "records differ from the expansion"
    assert _same(got.counts, _expand(counts, N3)), "counts differ from the expansion"
    assert _same(got.labels, _expand(labels, N3)), "labels differ from the expansion"
    assert torch.equal(got.truncated(), _expand(counts[:, 0] > 2, N3))


# ------------------------------------------------------------------------------------------ 8. match_regions, DetectionCounts
@pytest.mark.parametrize("mask_format", ["u8", "f32"])
def test_match_regions_two_rounds(vad, mask_format):
    pool, masks = FP.pool((5, 7), 9800), FP.masks((5, 7), 9801)
    gt, pred, counts = match_ref.match_batch(pool, masks, T, 8, 1, 0.0, 0.5, 2)
    assert counts[:, match_ref.GT_DETECTED].sum() > 0 and counts[:, match_ref.FALSE_ALARMS].sum() > 0 and (counts[:, match_ref.GT_REGIONS] > 2).any()
    x = _expand(pool, N2)
    if mask_format == "u8":
        m = _expand(np.where(masks, 128, 127).astype(np.uint8), N2)
    else:
        m = _expand(np.where(masks, np.float32(0.50001), np.float32(0.5)).astype(np.float32), N2)
    with Calls(vad, match_regions=1):
        got = vad.metrics.match_regions(x, m, float(T), 8, 1, 0.0, 0.5, 2)
    assert _same(got.gt_records, _expand(gt, N2)), "mask records differ from the expansion"
    assert _same(got.pred_records, _expand(pred, N2)), "prediction records differ from the expansion"
    assert _same(got.counts, _expand(counts, N2)), "counts differ from the expansion"
    total = vad.metrics.DetectionCounts("cuda").update(got)
    want = FP.weighted_counts(counts.view(np.int64), N2)
    assert total.counts.cpu().tolist() == want.tolist() and int(want[match_ref.C_BOTH:match_ref.C_BOTH + 4].sum()) == N2


# ------------------------------------------------------------------------------------------ 9. label_regions, ProHistogram
def _pro_total(pool, masks, labels, n, m):
    """The state words of n batch items: integer counters times multiplicities (uint64 sums wrap as the device's do)."""
    mult = FP.multiplicity(n)
    nb = 255 << m
    wpos, pos, neg = np.zeros(nb, np.uint64), np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    regions, max_region, rejected = 0, 0, np.zeros(2, np.int64)
    for i in range(P):
        st = pro_ref.ref_state(pool[i:i + 1], masks[i:i + 1], labels[i:i + 1], m)
        wpos += st["wpos"] * np.uint64(mult[i])
        pos += st["pos"] * mult[i]
        neg += st["neg"] * mult[i]
        regions += st["regions"] * int(mult[i])
        max_region = max(max_region, st["max_region"])
        rejected += st["rejected"] * mult[i]
    return pro_ref.state_words({"wpos": wpos, "pos": pos, "neg": neg, "regions": regions, "max_region": max_region, "rejected": rejected})


@pytest.mark.parametrize("mask_format", ["u8", "f32"])
def test_label_regions_and_pro_histogram_two_rounds(vad, mask_format):
    pool, masks = FP.pool((5, 7), 9900), FP.masks((5, 7), 9901)
    labels, sizes = pro_ref.label_batch(masks, 8)
    x = _expand(pool, N2)
    if mask_format == "u8":
        m = _expand(np.where(masks, 255, 0).astype(np.uint8), N2)
    else:
        m = _expand(masks.astype(np.float32), N2)
    with Calls(vad, label_regions=1):
        got_labels, got_sizes = vad.metrics.label_regions(m, 8)
    assert _same(got_labels, _expand(labels, N2)), "labels differ from the expansion"
    assert _same(got_sizes.view(torch.int32), _expand(sizes, N2)), "sizes differ from the expansion"
    hist = vad.metrics.ProHistogram(11)
    with Calls(vad, pro_accumulate=1):
        hist.accumulate(x, m)
    want = _pro_total(pool, masks, labels, N2, 11)
    assert hist.flags() == 0 and torch.equal(hist._words().cpu(), torch.from_numpy(want))
    assert hist.regions() == int(FP.weighted_counts((sizes > 0).sum(axis=(1, 2)), N2))


# ------------------------------------------------------------------------------------------ 10. detect_events, event_tracks
@pytest.mark.parametrize("mode", ((4, 1), (8, 1), (8, 9)), ids=["c4t1", "c8t1", "c8t9"])
def test_detect_events_and_event_tracks_two_rounds(vad, mode):
    pool = FP.pool((2, 4, 5), 10000)
    tracks, records, counts, frame_counts, labels = event_tracks_ref.tracks_batch(pool, T, mode[0], mode[1], 1, 1, 4)
    assert (counts[:, 0] >= 2).any() and (counts[:, 0] == 0).any() and (records[:, :, events_ref.T1] > records[:, :, events_ref.T0]).any()
    x = _expand(pool, N2)
    with Calls(vad, detect_events=1):
        ev = vad.metrics.detect_events(x, float(T), mode[0], mode[1], 1, 1, 4, return_labels=True)
    assert _same(ev.records, _expand(records, N2)), "event records differ from the expansion"
    assert _same(ev.counts, _expand(counts, N2)) and _same(ev.frame_counts, _expand(frame_counts, N2))
    assert _same(ev.labels, _expand(labels, N2)), "labels differ from the expansion"
    with Calls(vad, event_tracks=1):
        tr = vad.metrics.event_tracks(x, ev)
    assert _same(tr.records, _expand(tracks, N2)), "tracks differ from the expansion"


# ------------------------------------------------------------------------------------------ 11. EventTracker
def test_event_tracker_two_rounds(vad):
    h, w, kw = 4, 5, dict(threshold=float(T), connectivity=8, temporal=9, min_duration=1, min_volume=1, max_open=4, max_closed=4)
    pool = FP.pool((2, h, w), 10100)
    ref = {k: [] for k in ("c0", "k0", "f0", "c1", "k1", "f1", "boxes", "table", "plane", "cf", "kf")}
    for clip in pool:
        t = track_ref.Tracker(h, w, **kw)
        for step in (0, 1):
            closed, counts, fc = t.update(clip[step:step + 1])
            ref[f"c{step}"].append(closed), ref[f"k{step}"].append(counts), ref[f"f{step}"].append(fc)
        ref["boxes"].append(event_tracks_ref.boxes(t, clip[1]))
        ref["table"].append(t.open_table()), ref["plane"].append(t.plane.reshape(h, w).copy())
        closed, counts = t.flush()
        ref["cf"].append(closed), ref["kf"].append(counts)
    ref = {k: np.stack(v) for k, v in ref.items()}
    assert (ref["k1"][:, 0] > 0).any() and (ref["k1"][:, 4] > 0).any() and (ref["kf"][:, 0] > 0).any()   # closed, open and flushed events
    x = _expand(pool, N2)
    tracker = vad.metrics.EventTracker(N2, h, w, **kw)
    with Calls(vad, track_events=2, track_boxes=1):
        up0 = tracker.update(x[:, 0])
        up1 = tracker.update(x[:, 1], boxes=True)
    for up, s in ((up0, "0"), (up1, "1")):
        assert _same(up.records, _expand(ref["c" + s], N2)), f"closed records of update {s} differ from the expansion"
        assert _same(up.counts, _expand(ref["k" + s], N2)) and _same(up.frame_counts, _expand(ref["f" + s], N2))
    assert _same(up1.boxes.records, _expand(ref["boxes"], N2)), "boxes differ from the expansion"
    table, plane = _expand(ref["table"], N2), _expand(ref["plane"], N2)
    assert _same(tracker.open_events().records, table) and _same(tracker.slot_plane, plane)
    assert bool((tracker.frames_seen == 2).all()) and tracker.flags() == 0
    # three streams restart - the last of round 0, the first and the last of round 1 -, the others keep their open events
    restart = [FP.SLICE - 1, FP.SLICE, N2 - 1]
    tracker.reset(streams=restart)
    table[restart], plane[restart] = 0, 0
    assert _same(tracker.open_events().records, table) and _same(tracker.slot_plane, plane)
    seen = torch.full((N2,), 2, dtype=torch.int64, device="cuda")
    seen[restart] = 0
    assert torch.equal(tracker.frames_seen, seen)
    with Calls(vad, track_events=1):
        end = tracker.flush()
    closed, counts = _expand(ref["cf"], N2), _expand(ref["kf"], N2)
    closed[restart], counts[restart] = 0, 0
    assert _same(end.records, closed) and _same(end.counts, counts)
    assert not tracker.open_events().records.any() and not tracker.slot_plane.any()


# ------------------------------------------------------------------------------------------ 12. FrameBank.gather
@pytest.mark.parametrize("h,w", [(4, 4), (3, 5)], ids=["vector_kernels", "plain_kernels"])
def test_frame_bank_gather_three_rounds(vad, h, w):
    assert ((h * w * 3) % 16 == 0) == ((h, w) == (4, 4))
    frames = frame_bank_ref.video_u8(10200 + w, 300, h, w)
    bank = vad.FrameBank((h, w))
    bank.add_video(torch.from_numpy(frames))
    index = np.random.default_rng(10201).integers(0, 300, N3)
    index[[0, 1, FP.SLICE - 1, FP.SLICE, 2 * FP.SLICE, N3 - 1]] = [0, 299, 299, 0, 299, 0]
    index[5:9] = 17                                                          # repeats side by side
    idx = torch.from_numpy(index).cuda()
    want_u8 = _up(frames)[idx]
    want_f32 = _up(frame_bank_ref.normalised_ref(vad.synth.u8_to_unit, frames))[idx]
    g = Guarded((N3, 3, h, w))
    with Calls(vad, gather_frames=1):
        assert bank.gather(idx, out=g.out) is g.out
    assert _same(g.out, want_f32) and g.ok()
    g = Guarded((N3, h, w, 3), torch.uint8)
    with Calls(vad, gather_frames=1):
        assert bank.gather(idx, dtype=torch.uint8, out=g.out) is g.out
    assert _same(g.out, want_u8) and g.ok()


# ------------------------------------------------------------------------------------------ 13. map_topk
def test_map_topk_one_launch_of_many_frames(vad):
    pool = FP.pool((3, 5), 10300)
    ranks = [1, 2, 15]
    want = map_topk_ref.topk(pool, ranks)
    x = _expand(pool, N3)
    with Calls(vad, map_topk=1):
        got = vad.metrics.map_topk(x, ranks)
    assert _same(got["kth"], _expand(want["kth"], N3)), "kth differs from the expansion"
    mean = got["mean"].cpu().numpy()
    index = FP.index(N3)
    assert map_topk_ref.mean_within_bound(mean, {"exact": want["exact"][index], "bound": want["bound"][index]})
    assert _same(got["mean"], got["mean"][:P][_idx(N3)])                     # a frame's result does not depend on where it stands
