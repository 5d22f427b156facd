"""Temporal filters of anomaly maps on the GPU (csrc/map_temporal.hip, metrics.temporal_maps / TemporalFilter, the `temporal=` and
`temporal_filter=` arguments of the scoring entry points): the kernels against the numpy restatement
(tests/map_temporal_ref.py) on the bits - all four filters are specified to the bit -, on the shapes, window lengths, call lengths
and contents at which a register window over a ring in memory can go wrong, and the chain through the seeded models."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_temporal_ref as ref
from conftest import load_synthetic
from test_map_temporal_plan import compositions

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 16)
ALPHAS = (0.5, 0.1, 0.999)


def _clips(shape, seed):
    """Clips of different content: a few levels (ties, both zeros, negative values) under continuous noise on half the pixels."""
    rng = np.random.default_rng(seed)
    levels = np.float32([-0.0, 0.0, -1.5, 0.25, 2.0, 7.0])
    x = levels[rng.integers(0, 6, shape)]
    noise = rng.standard_normal(shape).astype(np.float32)
    return np.where(rng.random(shape) < 0.5, x, noise).astype(np.float32)


def _all_steps():
    return [(op, k) for op in ("min", "max", "mean") for k in KS] + [("ema", a) for a in ALPHAS]


def _plan(vad):
    threads, lanes = C.c_int(), C.c_int()
    assert vad.hip.lib().vad_tfilt_plan(C.byref(threads), C.byref(lanes)) == 0
    return threads.value, lanes.value


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    return ref.same_bits(got.cpu().numpy(), want)


def _stream(vad, x: np.ndarray, steps, parts, f=None):
    """x [B,T,H,W] through a TemporalFilter in calls of `parts` frames -> (the filtered frames [B,T,H,W] on the device, the filter)."""
    b, t, h, w = x.shape
    f = f or vad.metrics.TemporalFilter(b, h, w, list(steps))
    dev, at, got = torch.from_numpy(x).cuda(), 0, []
    for p in parts:
        got.append(f.update(dev[:, at:at + p].contiguous()).clone())
        at += p
    assert at == t
    return torch.cat(got, dim=1), f


# ------------------------------------------------------------------------------------------ clips: shapes, ops, k, batching
@pytest.mark.parametrize("b", [1, 3])
def test_clip_mode_equals_the_restatement(vad, b):
    """Frames of 1 x 1, 3 x 5 (no multiple of 4: one pixel per work item), 8 x 8, and one of several work-groups per stream on
    either path; T = 11 is above k - 1 for k <= 8 and below it for k = 16."""
    threads, lanes = _plan(vad)
    big = (3 * threads * lanes // 64, 64)                                    # three work-groups of the 16-byte path
    odd = (threads // 8 + 1, 35)                                             # 1155 pixels at 256 threads: five of the scalar path
    for i, (h, w) in enumerate([(1, 1), (3, 5), (8, 8), big, odd]):
        assert (h * w > 2 * threads * lanes) == ((h, w) == big) and ((h * w) % 4 != 0) == ((h, w) in ((1, 1), (3, 5), odd))
        x = _clips((b, 11, h, w), 2300 + i)
        dev = torch.from_numpy(x).cuda()
        for step in _all_steps():
            before = vad.hip.calls.get("tfilt_maps", 0)
            got = vad.metrics.temporal_maps(dev, *step)
            assert vad.hip.calls["tfilt_maps"] == before + 1
            assert _same(got, ref.clips([step], x)), (step, h, w)
        assert torch.equal(dev.cpu(), torch.from_numpy(x))


def test_clip_mode_equals_scipy(vad, golden):
    g = golden("temporal/scipy_temporal.npz")
    x = torch.from_numpy(g["x"][None]).cuda()
    for k in g["ks"]:
        assert np.array_equal(vad.metrics.temporal_maps(x, "min", int(k))[0].cpu().numpy(), g[f"min_{k}"]), k
        assert np.array_equal(vad.metrics.temporal_maps(x, "max", int(k))[0].cpu().numpy(), g[f"max_{k}"]), k


def test_frames_that_break_the_16_byte_alignment(vad):
    """40 x 52 (a multiple of 4) one float behind a 16-byte boundary: maps, out, or both - the scalar path, same bits."""
    x = _clips((2, 9, 40, 52), 2310)
    n = x.size
    for in_off, out_off in ((1, 0), (0, 3), (1, 1), (2, 3), (0, 0)):
        src = torch.zeros(n + 4, device="cuda")
        dst = torch.full((n + 4,), 5.0, device="cuda")
        maps, out = src[in_off:in_off + n].view(x.shape), dst[out_off:out_off + n].view(x.shape)
        maps.copy_(torch.from_numpy(x))
        assert maps.data_ptr() % 16 == 4 * in_off and out.data_ptr() % 16 == 4 * out_off and maps.is_contiguous()
        for step in (("min", 3), ("max", 16), ("mean", 8), ("ema", 0.25)):
            assert vad.metrics.temporal_maps(maps, *step, out=out) is out
            assert _same(out, ref.clips([step], x)), (step, in_off, out_off)
            assert bool((dst[:out_off] == 5.0).all()) and bool((dst[out_off + n:] == 5.0).all())     # nothing outside out
        f = vad.metrics.TemporalFilter(2, 40, 52, ("min", 3))
        got = torch.cat([f.update(maps[:, :4].contiguous()), f.update(maps[:, 4:].contiguous())], dim=1)
        assert _same(got, ref.clips([("min", 3)], x))


def test_layouts_out_and_step_lists(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x5 = _clips((2, 6, 1, 21, 70), 2320)
    dev = torch.from_numpy(x5).cuda()
    got = m.temporal_maps(dev, "max", 3)
    assert got.shape == dev.shape and _same(got[:, :, 0], ref.clips([("max", 3)], x5[:, :, 0]))
    steps = m.temporal_steps([("min", 3), ("max", 3), ("ema", 0.5), ("mean", 2)])
    before = vad.hip.calls.get("tfilt_maps", 0)
    got = m.apply_temporal(dev, steps)
    assert vad.hip.calls["tfilt_maps"] == before + 4
    assert _same(got[:, :, 0], ref.clips(steps, x5[:, :, 0])) and torch.equal(dev.cpu(), torch.from_numpy(x5))
    assert m.apply_temporal(dev, ()) is dev
    # empty calls launch nothing
    before = vad.hip.calls.get("tfilt_maps", 0)
    for shape in ((0, 4, 8, 8), (2, 0, 8, 8)):
        assert tuple(m.temporal_maps(torch.empty(shape, device="cuda"), "min", 2).shape) == shape
    assert vad.hip.calls.get("tfilt_maps", 0) == before
    # overlapping out: refused by the library, and nothing is written
    flat = torch.full((2 * dev.numel(),), 5.0, device="cuda")
    src = flat[:dev.numel()].view_as(dev)
    for off in (0, 1, dev.numel() - 1):
        with pytest.raises(VadError, match="overlaps"):
            m.temporal_maps(src, "min", 1, out=flat[off:off + dev.numel()].view_as(dev))
    torch.cuda.synchronize()
    assert bool((flat == 5.0).all())
    for bad_out in (torch.empty(2, 6, 1, 21, 71, device="cuda"), torch.empty(2, 6, 1, 21, 70, device="cuda", dtype=torch.float64), torch.empty(2, 6, 1, 21, 70)):
        with pytest.raises(VadError, match="out must be"):
            m.temporal_maps(dev, "min", 2, out=bad_out)
    with pytest.raises(VadError, match="float32"):
        m.temporal_maps(dev.double(), "min", 2)
    with pytest.raises(VadError, match="contiguous"):
        m.temporal_maps(dev[:, :, 0].transpose(2, 3), "min", 2)
    for bad in (dev[0, 0, 0], dev[0, 0], torch.empty(2, 6, 3, 8, 8, device="cuda")):
        with pytest.raises(VadError, match=r"\[B,T,H,W\] or \[B,T,1,H,W\]"):
            m.temporal_maps(bad.contiguous(), "min", 2)
    f = m.TemporalFilter(2, 21, 70, ("min", 2))
    mine = torch.full_like(dev, 5.0)                                         # update(out=): the last step's result in a tensor of one's own
    for spec in (("max", 3), [("min", 2), ("ema", 0.5), ("mean", 3)]):
        g = m.TemporalFilter(2, 21, 70, spec)
        assert g.update(dev, out=mine) is mine and _same(mine[:, :, 0], ref.clips(m.temporal_steps(spec), x5[:, :, 0]))
    with pytest.raises(VadError, match="out must be"):
        f.update(dev, out=torch.empty(2, 6, 1, 21, 71, device="cuda"))
    with pytest.raises(VadError, match="overlaps"):
        f.update(dev, out=dev)
    with pytest.raises(VadError, match="do not match the filter's state"):
        f.update(torch.empty(3, 1, 21, 70, device="cuda"))
    with pytest.raises(VadError, match="out of range"):
        f.reset([2])


# ------------------------------------------------------------------------------------------ streams: the ring across calls
@pytest.mark.parametrize("k", [2, 3, 8, 16])
def test_calls_below_at_and_above_the_ring_length(vad, k):
    """A call of t frames writes min(t, k - 1) planes at the ring position, which then advances by t: t = 1, k - 2, k - 1, k, k + 3 in
    one stream, on both paths (8 x 8: 16-byte; 3 x 5: one pixel per work item)."""
    parts = [p for p in (1, k - 2, k - 1, 1, k, k + 3, 1, k - 1, 2) if p > 0]
    for h, w in ((8, 8), (3, 5)):
        x = _clips((3, sum(parts), h, w), 2330 + k)
        for op in ("min", "max", "mean"):
            got, f = _stream(vad, x, [(op, k)], parts)
            assert _same(got, ref.clips([(op, k)], x)), (op, k, h, w)
            assert f.frames_seen().tolist() == [sum(parts)] * 3
            header = f.states[0].view(3, -1)[:, :vad.hip.TFILT_HEADER_WORDS].cpu()
            assert header[:, 1].tolist() == [sum(parts) % (k - 1)] * 3 and header[:, 2].tolist() == [0] * 3      # ring position, ticket


@pytest.mark.parametrize("steps", [[("min", 3)], [("mean", 4)], [("ema", 0.25)], [("min", 3), ("max", 3)], [("max", 16), ("mean", 2)]], ids=str)
def test_every_split_of_seven_frames_gives_the_same_bits(vad, steps):
    x = _clips((3, 7, 8, 8), 2340)
    x[1, 2, 3, 3] = np.nan
    want = ref.clips(steps, x)
    dev = torch.from_numpy(x).cuda()
    clip = vad.metrics.apply_temporal(dev, vad.metrics.temporal_steps(steps))
    assert _same(clip, want)
    f = vad.metrics.TemporalFilter(3, 8, 8, steps)
    n = 0
    for parts in compositions(7):
        f.reset()
        got, _ = _stream(vad, x, steps, parts, f)
        assert torch.equal(_bits(got), _bits(clip)), parts
        n += 1
    assert n == 64 and f.frames_seen().tolist() == [7, 7, 7]
    # an empty call changes nothing
    assert tuple(f.update(dev[:, :0].contiguous()).shape) == (3, 0, 8, 8) and f.frames_seen().tolist() == [7, 7, 7]


def test_reset_of_one_stream_of_three(vad):
    steps = [("min", 3), ("mean", 4), ("ema", 0.5)]
    x = _clips((3, 9, 8, 12), 2350)
    f = vad.metrics.TemporalFilter(3, 8, 12, steps)
    dev = torch.from_numpy(x).cuda()
    first = f.update(dev[:, :4].contiguous())
    f.reset([1])
    assert f.frames_seen().tolist() == [4, 0, 4]
    second = f.update(dev[:, 4:].contiguous())
    assert f.frames_seen().tolist() == [9, 5, 9]
    whole = ref.clips(steps, x)
    assert _same(first, whole[:, :4])
    assert _same(second[0], whole[0, 4:]) and _same(second[2], whole[2, 4:])
    assert _same(second[1], ref.apply(steps, x[1, 4:]))                      # stream 1 began again at its frame 4
    # state_dict: a second filter continues where the first stands; another step list or shape is refused
    state = f.state_dict()
    g = vad.metrics.TemporalFilter(3, 8, 12, steps).load_state_dict(state)
    more = torch.from_numpy(_clips((3, 2, 8, 12), 2351)).cuda()
    assert torch.equal(_bits(g.update(more)), _bits(f.update(more))) and g.frames_seen().tolist() == [11, 7, 11]
    for other in (vad.metrics.TemporalFilter(3, 8, 12, steps[:2]), vad.metrics.TemporalFilter(2, 8, 12, steps),
                  vad.metrics.TemporalFilter(3, 12, 8, steps), vad.metrics.TemporalFilter(3, 8, 12, [("min", 4), ("mean", 4), ("ema", 0.5)])):
        with pytest.raises(vad.hip.VadError, match="load_state_dict"):
            other.load_state_dict(state)


def test_a_state_made_for_another_filter_is_detected_on_the_device(vad):
    lib, m = vad.hip.lib(), vad.metrics
    f = m.TemporalFilter(2, 8, 8, ("min", 3))
    x = torch.from_numpy(_clips((2, 3, 8, 8), 2360)).cuda()
    f.update(x)
    before = f.states[0].clone()
    out = torch.zeros_like(x)
    for op, k, h, w in ((0, 4, 8, 8), (1, 3, 8, 8), (0, 3, 4, 16), (3, 0, 8, 8)):
        assert lib.vad_tfilt_maps(x.data_ptr(), 2, 3, h, w, op, k, 0.5, f.states[0].data_ptr(), out.data_ptr(), vad.hip.current_stream()) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and torch.equal(f.states[0], before), (op, k, h, w)


# ------------------------------------------------------------------------------------------ contents
def test_non_finite_values_zeros_and_denormals(vad):
    x = _clips((2, 14, 6, 10), 2370) * np.float32(1e-3)
    x[0, 3, 1, 1] = np.nan                                                   # enters the windows of frames 3 .. 3 + k - 1, then leaves
    x[0, 0, 2, 2] = np.nan                                                   # in the first frame
    x[1, 13, 0, 0] = np.nan                                                  # in the last
    x[0, 5, 4, 4], x[0, 6, 4, 5], x[1, 2, 3, 3], x[1, 3, 3, 3] = np.inf, -np.inf, np.inf, -np.inf
    x[1, :, 5, :5] = np.float32([0.0, -0.0, 0.0, -0.0, -0.0])[None, :].repeat(14, 0) * np.float32([1, -1] * 7)[:, None]
    x[0, :, 0, 5:] = (np.arange(14 * 5).reshape(14, 5) % 7 - 3).astype(np.float32) * np.float32(1e-45) * 3     # denormals of both signs
    x[1, :, 1, :] = np.float32(3.4e38)                                       # a float64 sum: no overflow on the way to the mean
    assert np.isnan(x).sum() == 3 and (np.abs(x[0, :, 0, 5:]) < 1e-38).all() and np.signbit(x[1, :, 5, :5]).any()
    dev = torch.from_numpy(x).cuda()
    for step in _all_steps():
        want = ref.clips([step], x)
        assert _same(vad.metrics.temporal_maps(dev, *step), want), step
        got, _ = _stream(vad, x, [step], (1, 2, 3, 1, 7))
        assert _same(got, want), step
    y = vad.metrics.temporal_maps(dev, "min", 3).cpu().numpy()
    assert np.isnan(y[0, :, 1, 1]).tolist() == [3 <= t <= 5 for t in range(14)]
    e = vad.metrics.temporal_maps(dev, "ema", 0.5).cpu().numpy()
    assert np.isnan(e[0, :, 1, 1]).tolist() == [t >= 3 for t in range(14)] and np.isnan(e[0, :, 2, 2]).all()
    c = np.full((1, 12, 4, 4), 0.1, np.float32)                              # a constant stream stays constant to the bit: no fused multiply-add
    c[0, :, 0, 0], c[0, :, 0, 1] = 1e-42, -7.3e30
    for alpha in ALPHAS:
        assert _same(vad.metrics.temporal_maps(torch.from_numpy(c).cuda(), "ema", alpha), c), alpha


def test_a_captured_update_replays_on_new_contents(vad):
    """The counters are advanced by the kernel: three replays of one captured `update` are three calls of one stream."""
    steps = [("min", 3), ("mean", 16), ("ema", 0.25)]
    contents = [_clips((2, 2, 24, 48), 2380 + i) for i in range(3)]
    contents[1][1, 0, 5, 6] = np.nan
    x = torch.from_numpy(contents[0]).cuda()
    f = vad.metrics.TemporalFilter(2, 24, 48, steps)
    f.update(x)                                                              # once eagerly: nothing left to set up under capture
    f.reset()
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = f.update(x)
    torch.cuda.current_stream().wait_stream(side)
    f.reset()                                                                # (the capture itself ran nothing)
    want = ref.clips(steps, np.concatenate(contents, axis=1))
    for i, c in enumerate(contents):
        x.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(out, want[:, 2 * i:2 * i + 2]), i
    assert f.frames_seen().tolist() == [6, 6]


# ------------------------------------------------------------------------------------------ through the models
def _video_model(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    return model.cuda().eval()


def _calls(vad):
    return dict(vad.hip.calls)


@pytest.mark.parametrize("split", [(1, 1, 1, 1, 1, 1), (2, 4), (6,)], ids=["one_by_one", "2_4", "whole"])
def test_localize_stream_in_pieces_equals_localize_events_on_the_clip(vad, split):
    model = _video_model(vad)
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 6, 3, 32, 32)).cuda()
    spec = [("min", 2), ("max", 3)]
    with torch.no_grad():
        plain = vad.metrics.smooth_maps(model.score_stateful(clips, None, errmap=True)["errmap"], 1.0)
    want = ref.clips(vad.metrics.temporal_steps(spec), plain.cpu().numpy()[:, :, 0])
    thr = float(np.quantile(want, 0.9))
    events, emaps = vad.scoring.localize_events(model, clips, thr, sigma=1.0, temporal=1, max_events=256, temporal_filter=spec)
    assert tuple(emaps.shape) == (2, 6, 1, 32, 32) and _same(emaps[:, :, 0], want)
    ev = vad.metrics.detect_events(emaps, thr, temporal=1, max_events=256)
    assert torch.equal(events.records, ev.records) and torch.equal(events.counts, ev.counts) and int(events.counts[:, 0].sum()) > 0
    kw = dict(threshold=thr, connectivity=8, temporal=1, min_duration=1, min_volume=1, max_open=512, max_closed=256)
    tracker, by_hand = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    filt = vad.metrics.TemporalFilter(2, 32, 32, spec)
    state, at, seen = None, 0, []
    for p in split:
        before = _calls(vad)
        up, maps, state = vad.scoring.localize_stream(model, clips[:, at:at + p], tracker, state, sigma=1.0, temporal_filter=filt)
        assert vad.hip.calls["tfilt_maps"] == before.get("tfilt_maps", 0) + 2 and vad.hip.calls["vid_score_stateful"] == before["vid_score_stateful"] + 1
        hand = by_hand.update(emaps[:, at:at + p].contiguous())
        assert torch.equal(up.records, hand.records) and torch.equal(up.counts, hand.counts) and torch.equal(up.frame_counts, hand.frame_counts)
        seen.append(maps)
        at += p
    assert torch.equal(_bits(torch.cat(seen, dim=1)), _bits(emaps)) and filt.frames_seen().tolist() == [6, 6]


def test_localize_stream_filters_the_image_models_cameras(vad):
    """[B,1,H,W] of the image model is one new frame of B cameras."""
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    frames = torch.from_numpy(vad.synth.clips(23, 0, 2, 5, 3, 32, 32)).cuda()        # 2 cameras x 5 frames
    with torch.no_grad():
        plain = torch.stack([model.score_all(frames[:, t].contiguous())["errmap"][:, 0] for t in range(5)], dim=1)     # [B,T,H,W]
    spec = ("ema", 0.5)
    want = ref.clips(vad.metrics.temporal_steps(spec), plain.cpu().numpy())
    kw = dict(threshold=float(np.quantile(want, 0.9)), connectivity=8, temporal=9)
    tracker, by_hand = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    filt = vad.metrics.TemporalFilter(2, 32, 32, spec)
    for t in range(5):
        up, maps, state = vad.scoring.localize_stream(model, frames[:, t].contiguous(), tracker, temporal_filter=filt)
        assert state is None and tuple(maps.shape) == (2, 1, 32, 32) and _same(maps[:, 0], want[:, t]), t
        hand = by_hand.update(torch.from_numpy(want[:, t]).cuda())
        assert torch.equal(up.records, hand.records) and torch.equal(up.frame_counts, hand.frame_counts)
    with pytest.raises(vad.hip.VadError, match="are not consecutive"):
        vad.scoring.localize_events(model, frames[:, 0].contiguous(), 0.5, temporal_filter=spec)
    with pytest.raises(vad.hip.VadError, match="are not consecutive"):
        vad.scoring.frame_scores(model, frames[:, 0].contiguous(), "max", temporal=spec)


def test_pixel_metrics_take_the_filtered_maps(vad):
    """pixel_auroc(temporal=) is the histogram of the host-filtered maps; frame_scores, detection_report and pixel_aupro filter the
    same maps; the chain's order is sigma, calibration, morph, temporal."""
    model, m, s = _video_model(vad), vad.metrics, vad.scoring
    clips = torch.from_numpy(vad.synth.clips(24, 0, 2, 5, 3, 32, 32)).cuda()
    masks = torch.zeros(2, 5, 1, 32, 32, device="cuda")
    masks[:, 1:4, :, 8:20, 10:22] = 1.0
    batch = [{"frames": clips, "mask": masks, "frame_labels": np.array([[0, 1, 1, 1, 0]] * 2)}]
    spec = [("mean", 3)]
    with torch.no_grad():
        plain = s._anomaly_maps(model, clips, "mse", 1.0, 4.0, morph=m.morph_steps(("open", 2)))
    want = ref.clips(spec, plain.cpu().numpy()[:, :, 0])[:, :, None]
    before = _calls(vad)
    auroc, _, hist = s.pixel_auroc(model, batch, "cuda", sigma=1.0, morph=("open", 2), temporal=spec)
    delta = {k: v - before.get(k, 0) for k, v in vad.hip.calls.items() if v != before.get(k, 0)}
    assert delta["tfilt_maps"] == 1 and delta["morph_maps"] == 1 and delta["smooth_maps"] == 1
    by_hand = m.ScoreHistogram(11, "cuda").accumulate(torch.from_numpy(want).cuda(), masks)
    assert torch.equal(hist.counts(), by_hand.counts()) and auroc == by_hand.auroc()[0]
    plain_hist = s.pixel_auroc(model, [{"image": clips, "mask": masks}], "cuda", sigma=1.0, morph=("open", 2))[2]
    assert not torch.equal(plain_hist.counts(), hist.counts())
    scores, maps = s.frame_scores(model, clips, "max", sigma=1.0, morph=("open", 2), temporal=spec)
    assert _same(maps, want) and _same(scores, want.reshape(2, 5, -1).max(-1))
    fa = s.frame_auroc(model, batch, "cuda", reduce="max", sigma=1.0, morph=("open", 2), temporal=spec)[2]
    fh = m.ScoreHistogram(11, "cuda").accumulate(scores, torch.from_numpy(batch[0]["frame_labels"]).cuda())
    assert torch.equal(fa.counts(), fh.counts())
    thr = float(np.quantile(want, 0.8))
    report, counts = s.detection_report(model, batch, "cuda", thr, sigma=1.0, morph=("open", 2), temporal=spec)
    hand = m.DetectionCounts("cuda").update(m.match_regions(torch.from_numpy(want).cuda(), masks, thr, max_regions=1))
    assert torch.equal(counts.counts, hand.counts) and counts.params["temporal"] == (("mean", 3),)
    aupro = s.pixel_aupro(model, batch, "cuda", sigma=1.0, morph=("open", 2), temporal=spec)[3]
    ph = m.ProHistogram(11, "cuda").accumulate(torch.from_numpy(want).cuda().flatten(0, 1), masks.flatten(0, 1))      # every frame on its own
    assert torch.equal(aupro.counts(), ph.counts())


def test_none_leaves_every_entry_point_on_its_present_calls(vad):
    """The library calls of every entry point without the argument, and with `None`, are the ones recorded from the commit before
    the temporal filters existed (same models, same batches)."""
    model, s = _video_model(vad), vad.scoring
    img = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, img, 11)
    img = img.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(25, 0, 2, 4, 3, 32, 32)).cuda()
    masks = torch.zeros(2, 4, 1, 32, 32, device="cuda")
    masks[:, 1:3, :, 4:12, 4:12] = 1.0
    batch = [{"frames": clips, "mask": masks, "frame_labels": np.array([[0, 1, 1, 0]] * 2), "image": clips, "label": [0, 1], "defect_type": ["a", "b"]}]
    ibatch = [{"image": clips[:, 0].contiguous(), "mask": masks[:, 1].contiguous(), "label": [0, 1], "defect_type": ["a", "b"]}]
    tracker = lambda: vad.metrics.EventTracker(2, 32, 32, 0.01)

    def delta(call):
        before = _calls(vad)
        call()
        return {k: v - before.get(k, 0) for k, v in vad.hip.calls.items() if v != before.get(k, 0)}

    cases = [
        (lambda **kw: s.localize_events(model, clips, 0.01, **kw), "temporal_filter", {"detect_events": 1, "vid_score": 1}),
        (lambda **kw: s.frame_scores(model, clips, "max", **kw), "temporal", {"map_topk": 1, "vid_score": 1}),
        (lambda **kw: s.frame_auroc(model, batch, "cuda", reduce="max", **kw), "temporal", {"hist_accumulate": 1, "map_topk": 1, "vid_score": 1}),
        (lambda **kw: s.frame_auroc(model, batch, "cuda", **kw), "temporal", {"hist_accumulate": 1, "vid_score": 1}),
        (lambda **kw: s.detection_report(model, batch, "cuda", 0.01, **kw), "temporal", {"match_regions": 1, "vid_score": 1}),
        (lambda **kw: s.pixel_auroc(model, batch, "cuda", **kw), "temporal", {"hist_accumulate": 1, "vid_score": 1}),
        (lambda **kw: s.pixel_aupro(img, ibatch, "cuda", **kw), "temporal", {"img_score": 1, "pro_accumulate": 1}),
        (lambda **kw: s.compute_auroc_maps(img, ibatch, "cuda", **kw), None, {"img_score": 1, "map_topk": 1}),     # image batches only: no argument
        (lambda **kw: s.localize_stream(model, clips, tracker(), **kw), "temporal_filter", {"track_events": 1, "vid_score_stateful": 1}),
    ]
    for call, name, want in cases:
        assert delta(call) == want, name
        if name is not None:
            assert delta(lambda: call(**{name: None})) == want, name
