"""Grey morphology of anomaly maps on the GPU (csrc/map_morph.hip, metrics.morph_maps, the `morph=` argument of the scoring entry
points): the kernel against the numpy restatement (tests/map_morph_ref.py) on the bits - nothing is
rounded, so NaN positions and every other bit are specified -, on the shapes, sizes and contents at which a tiled, fused open /
close can go wrong, and the chain through the seeded models."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_morph_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

OPS = ("erode", "dilate", "open", "close")
SIZES = [1, 2, 3, 4, 5, 15, 16, 31, (1, 5), (5, 1), (2, 31), (31, 2)]


def _pair(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _tile(vad, size, op):
    th, tw = C.c_int(), C.c_int()
    sh, sw = _pair(size)
    assert vad.hip.lib().vad_morph_tile(sh, sw, vad.hip.MORPH_OPS[op], C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def _maps(shape, seed):
    """Frames of different content: a few levels (ties, both zeros, negative values) under continuous noise on half the pixels."""
    rng = np.random.default_rng(seed)
    levels = np.float32([-0.0, 0.0, -1.5, 0.25, 2.0, 7.0])
    x = levels[rng.integers(0, 6, shape)]
    noise = rng.standard_normal(shape).astype(np.float32)
    return np.where(rng.random(shape) < 0.5, x, noise).astype(np.float32)


def _run(vad, x: np.ndarray, op, size) -> np.ndarray:
    return vad.metrics.morph_maps(torch.from_numpy(x).cuda(), op, size).cpu().numpy()


def _check(vad, x: np.ndarray, op, size, what=""):
    got = _run(vad, x, op, size)
    assert ref.same_bits(got, ref.morph(op, x, size)), (what, op, size, x.shape)
    return got


# ------------------------------------------------------------------------------------------ shapes, sizes, ops, batching
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_equals_the_restatement(vad, size):
    """n = 3 frames of different content per shape: a halo that read a neighbouring frame would show."""
    for op in OPS:
        th, tw = _tile(vad, size, op)
        shapes = [(1, 1), (1, 37), (37, 1), (3, 4), (th + 3, 2 * tw + 5), (9, 2 * tw + 2)]      # 37, 2 tw + 5: w no multiple of 4
        for i, (h, w) in enumerate(shapes):
            _check(vad, _maps((3, h, w), 4200 + i), op, size)


@pytest.mark.parametrize("size", [(7, 7), (6, 5)], ids=str)
def test_element_larger_than_the_image_equals_scipy(vad, golden, size):
    g = golden("morph/scipy_grey.npz")
    x = g["x_h3w4"]
    for op in OPS:
        got = _run(vad, x, op, size)
        assert np.array_equal(got, g[f"{op}_h3w4_{size[0]}x{size[1]}"]), (op, size)
        assert ref.same_bits(got, ref.morph(op, x, size))


def test_size_one_is_a_copy_and_empty_calls_launch_nothing(vad):
    x = _maps((2, 1, 19, 23), 4210)
    x[0, 0, 3, 4], x[1, 0, 0, 0] = np.nan, np.inf
    for op in OPS:
        assert ref.same_bits(_run(vad, x, op, 1), x) and ref.same_bits(_run(vad, x, op, (1, 1)), x)
    before = vad.hip.calls.get("morph_maps", 0)
    for shape in ((0, 1, 8, 8), (2, 0, 1, 8, 8)):
        out = vad.metrics.morph_maps(torch.empty(shape, device="cuda"), "open", 3)
        assert tuple(out.shape) == shape
    assert vad.hip.calls.get("morph_maps", 0) == before
    assert vad.hip.lib().vad_morph_maps(0x1000, 0, 8, 8, 2, 3, 3, 0x9000, None) == 0


# ------------------------------------------------------------------------------------------ borders, even sizes, seams
@pytest.mark.parametrize("size", [2, 3, 5, 16, (2, 31), (31, 2)], ids=str)
def test_blobs_on_every_border_and_corner(vad, size):
    """Constant blobs touching each border and each corner, bright on dark and dark on bright.  For open / close this is what
    catches an intermediate image computed outside the frame: the clamped second step must see the blob END at the border."""
    for op in OPS:
        th, tw = _tile(vad, size, op)
        h, w = th + 9, tw + 11
        x = np.zeros((2, h, w), np.float32)
        for f, (lo, hi) in enumerate(((0.0, 1.0), (1.0, 0.0))):
            x[f] = lo
            x[f, :4, :5] = hi
            x[f, :3, -6:] = hi
            x[f, -5:, :4] = hi
            x[f, -4:, -4:] = hi
            x[f, :2, w // 2 - 3:w // 2 + 4] = hi
            x[f, -3:, w // 2 - 2:w // 2 + 5] = hi
            x[f, h // 2 - 3:h // 2 + 3, :3] = hi
            x[f, h // 2 - 2:h // 2 + 4, -2:] = hi
            x[f, th - 2:th + 3, tw - 3:tw + 2] = hi                              # and one across the tile corner
        _check(vad, x, op, size)


@pytest.mark.parametrize("size", [2, 4, 16, (2, 3)], ids=str)
def test_even_sizes_lean_as_scipy_does(vad, size):
    """A single bright and a single dark pixel, at the centre and at (0, 0)."""
    sh, sw = _pair(size)
    for op in OPS:
        th, tw = _tile(vad, size, op)
        h, w = th + 5, tw + 7
        x = np.zeros((4, h, w), np.float32)
        x[0, h // 2, w // 2] = x[1, 0, 0] = 1.0
        x[2:] = 1.0
        x[2, h // 2, w // 2] = x[3, 0, 0] = 0.0
        got = _check(vad, x, op, size)
        if op == "dilate":                                                    # the window [i - (s-1)//2, i + s//2] seen from the pixel
            ys, xs = np.nonzero(got[0])
            assert (ys.min(), ys.max()) == (h // 2 - sh // 2, h // 2 + (sh - 1) // 2)
            assert (xs.min(), xs.max()) == (w // 2 - sw // 2, w // 2 + (sw - 1) // 2)
            assert np.count_nonzero(got[1]) == ((sh - 1) // 2 + 1) * ((sw - 1) // 2 + 1)
        if op == "erode":
            ys, xs = np.nonzero(got[2] == 0)
            assert (ys.min(), ys.max()) == (h // 2 - (sh - 1) // 2, h // 2 + sh // 2)
            assert (xs.min(), xs.max()) == (w // 2 - (sw - 1) // 2, w // 2 + sw // 2)
            assert np.count_nonzero(got[3] == 0) == (sh // 2 + 1) * (sw // 2 + 1)
        if op == "open" and sh * sw > 1:
            assert not got[0].any()                                           # a single pixel does not survive away from the border
        if op == "close" and sh * sw > 1:                                     # (at (0, 0) the clamped windows shrink: the restatement decides)
            assert (got[2] == 1).all()


@pytest.mark.parametrize("size", [2, 3, 5, 15, 31], ids=str)
def test_stripes_across_the_tile_seams(vad, size):
    s = _pair(size)[0]
    for op in OPS:
        th, tw = _tile(vad, size, op)
        h, w = 2 * th + 1, 2 * tw + 1
        yy, xx = np.mgrid[0:h, 0:w]
        frames = []
        for period in (2, s, s + 1, 2 * s - 1, 2 * s + 1):
            for phase in (0, 1):
                on = max(1, period // 2)
                frames.append(((xx + tw - phase) % period < on).astype(np.float32))   # vertical stripes placed against the x seam
                frames.append(((yy + th - phase) % period < on).astype(np.float32))   # horizontal ones against the y seam
        frames.append((((xx - tw) % (s + 1) < 1) | ((yy - th) % (s + 1) < 1)).astype(np.float32) * 3 - 1)
        _check(vad, np.stack(frames), op, size)


# ------------------------------------------------------------------------------------------ non-finite values, zeros
def _window_mask(h, w, points, size, is_max):
    """The pixels whose window of one step holds one of `points` (from the definition, not from the restatement)."""
    (lh, hh), (lw, hw) = ref.reach(size[0], is_max), ref.reach(size[1], is_max)
    m = np.zeros((h, w), bool)
    for i, j in points:
        m[max(0, i - hh):i + lh + 1, max(0, j - hw):j + lw + 1] = True
    return m


@pytest.mark.parametrize("size", [2, 3, (4, 3), 16, (2, 31)], ids=str)
def test_nan_and_inf_follow_the_window(vad, size):
    size = _pair(size)
    for op in OPS:
        th, tw = _tile(vad, size, op)
        h, w = th + 6, tw + 9
        clean = _maps((3, h, w), 4230)
        x = clean.copy()
        nans = [(h // 2 - 3, w // 3), (0, 0), (h - 1, w - 1), (th - 1, tw), (th, tw - 1)]      # interior, corners, both sides of a seam
        for i, j in nans:
            x[1, i, j] = np.nan
        x[1, 5, w - 7], x[1, 0, w - 1], x[1, th, tw + 3] = np.inf, np.inf, np.inf
        x[1, h - 6, 5], x[1, h - 1, 0], x[1, th - 1, tw - 4] = -np.inf, -np.inf, -np.inf
        got = _check(vad, x, op, size)
        first_max = op in ("dilate", "close")
        want = _window_mask(h, w, nans, size, first_max)
        if op in ("open", "close"):                                           # ... and the windows of the second step
            want = _window_mask(h, w, np.argwhere(want), size, not first_max)
        assert np.array_equal(np.isnan(got[1]), want), (op, size)
        assert not np.isnan(got[[0, 2]]).any()
        base = _run(vad, clean, op, size)
        assert ref.same_bits(got[[0, 2]], base[[0, 2]])                       # no bit of another frame changes
        inf_only = x.copy()
        inf_only[np.isnan(inf_only)] = 1.0
        assert not np.isnan(_check(vad, inf_only, op, size)).any()            # infinities are ordinary values: no NaN appears


def test_maps_of_signed_zeros(vad):
    rng = np.random.default_rng(4240)
    for op in OPS:
        for size in (2, 3, (1, 5), 16):
            th, tw = _tile(vad, size, op)
            x = np.where(rng.random((2, th + 2, tw + 3)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            got = _check(vad, x, op, size)
            assert (got == 0).all()                                           # the signs are the restatement's (_check)


# ------------------------------------------------------------------------------------------ the Python surface
def test_layouts_out_and_refusals(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x4, x5 = _maps((3, 1, 21, 70), 4250), _maps((2, 3, 1, 21, 70), 4251)
    for x in (x4, x5):
        for op, size in (("open", 3), ("close", (2, 5)), ("erode", 4)):
            got = _check(vad, x, op, size)
            assert got.shape == x.shape
    one = _run(vad, np.ascontiguousarray(x5[1, 2, 0]), "open", 3)             # a frame alone, [H, W]
    assert ref.same_bits(one, ref.opening(x5, 3)[1, 2, 0])
    x = torch.from_numpy(x4).cuda()
    out = torch.full_like(x, 5.0)
    before = vad.hip.calls.get("morph_maps", 0)
    assert m.morph_maps(x, "close", 3, out=out) is out and vad.hip.calls["morph_maps"] == before + 1
    assert ref.same_bits(out.cpu().numpy(), ref.closing(x4, 3)) and torch.equal(x.cpu(), torch.from_numpy(x4))
    # overlapping out: refused by the library, and nothing is written
    flat = torch.full((2 * x.numel(),), 5.0, device="cuda")
    src = flat[:x.numel()].view_as(x)
    for off in (0, 1, x.numel() - 1):
        with pytest.raises(VadError, match="overlaps"):
            m.morph_maps(src, "open", 3, out=flat[off:off + x.numel()].view_as(x))
    m.morph_maps(src, "open", 3, out=flat[x.numel():].view_as(x))             # adjacent is fine
    torch.cuda.synchronize()
    assert bool((flat[:x.numel()] == 5.0).all()) and bool((flat[x.numel():] == 5.0).all())
    for bad_out in (torch.empty(3, 1, 21, 71, device="cuda"), torch.empty(3, 1, 21, 70, device="cuda", dtype=torch.float64),
                    torch.empty(3, 1, 21, 70), torch.empty(3, 1, 70, 21, device="cuda").transpose(2, 3)):
        with pytest.raises(VadError, match="out must be"):
            m.morph_maps(x, "open", 3, out=bad_out)
    with pytest.raises(VadError, match="float32"):
        m.morph_maps(x.double(), "open", 3)
    with pytest.raises(VadError, match="contiguous"):
        m.morph_maps(x.transpose(2, 3), "open", 3)
    with pytest.raises(VadError, match="at least the two dimensions"):
        m.morph_maps(x.reshape(-1), "open", 3)
    with pytest.raises(VadError, match="op must be one of"):
        m.morph_maps(x, "tophat", 3)
    with pytest.raises(VadError, match="size must be in"):
        m.morph_maps(x, "open", (3, 32))


def test_a_list_of_steps_ping_pongs_two_buffers(vad):
    x_np = _maps((2, 1, 40, 70), 4260)
    x = torch.from_numpy(x_np).cuda()
    steps = vad.metrics.morph_steps([("open", 2), ("close", 5), ("dilate", (1, 3)), ("erode", (3, 1))])
    before = vad.hip.calls.get("morph_maps", 0)
    got = vad.metrics.apply_morph(x, steps)
    assert vad.hip.calls["morph_maps"] == before + 4
    want = x_np
    for op, size in steps:
        want = ref.morph(op, want, size)
    assert ref.same_bits(got.cpu().numpy(), want) and torch.equal(x.cpu(), torch.from_numpy(x_np))
    assert vad.metrics.apply_morph(x, ()) is x


def test_a_captured_call_replays_on_new_contents(vad):
    contents = [_maps((2, 1, 45, 150), 4270 + i) for i in range(3)]
    contents[1][1, 0, 31, 64] = np.nan
    x = torch.from_numpy(contents[0]).cuda()
    outs = {}
    vad.metrics.morph_maps(x, "open", 31)                                     # once eagerly: nothing left to set up under capture
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs["open"] = vad.metrics.morph_maps(x, "open", 31)
            outs["close"] = vad.metrics.morph_maps(x, "close", (2, 5))
            outs["both"] = vad.metrics.morph_maps(outs["open"], "dilate", 3)
    torch.cuda.current_stream().wait_stream(side)
    for c in contents:
        x.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        assert ref.same_bits(outs["open"].cpu().numpy(), ref.opening(c, 31))
        assert ref.same_bits(outs["close"].cpu().numpy(), ref.closing(c, (2, 5)))
        assert ref.same_bits(outs["both"].cpu().numpy(), ref.dilate(ref.opening(c, 31), 3))


# ------------------------------------------------------------------------------------------ through the models
def _image_model(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    return model.cuda().eval()


def _threshold(maps, q=0.9):
    return float(np.quantile(maps.cpu().numpy(), q))


@pytest.mark.parametrize("morph", [("open", 3), [("open", 2), ("close", (3, 5))]], ids=["open3", "open2_close3x5"])
def test_localize_morphs_the_maps_it_labels(vad, morph):
    model = _image_model(vad)
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    steps = vad.metrics.morph_steps(morph)
    for sigma in (None, 1.0):
        with torch.no_grad():
            plain = vad.scoring._anomaly_maps(model, x, "mse", sigma, 4.0)
        by_hand = vad.metrics.apply_morph(plain, steps)
        t = _threshold(by_hand, 0.8)                                          # a fifth of the morphed pixels are foreground
        before = {k: vad.hip.calls.get(k, 0) for k in ("morph_maps", "img_score", "smooth_maps")}
        regions, maps = vad.scoring.localize(model, x, t, sigma=sigma, max_regions=256, morph=morph)
        assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [len(steps), 1, int(sigma is not None)]
        assert torch.equal(maps, by_hand) and not torch.equal(maps, plain)
        want = plain.cpu().numpy()
        for op, size in steps:
            want = ref.morph(op, want, size)
        assert ref.same_bits(maps.cpu().numpy(), want)
        table = vad.metrics.detect_regions(by_hand, t, max_regions=256)
        assert torch.equal(regions.records, table.records) and torch.equal(regions.counts, table.counts)
        assert int(regions.counts[:, 0].sum()) > 0
        # morph=None is the call without the argument
        none_r, none_m = vad.scoring.localize(model, x, t, sigma=sigma, max_regions=256, morph=None)
        plain_r = vad.metrics.detect_regions(plain, t, max_regions=256)
        assert torch.equal(none_m, plain) and torch.equal(none_r.records, plain_r.records)
        # events: the image batch as one volume
        events, emaps = vad.scoring.localize_events(model, x, t, sigma=sigma, max_events=256, morph=morph)
        ev = vad.metrics.detect_events(by_hand[:, 0], t, max_events=256)
        assert torch.equal(emaps, by_hand) and torch.equal(events.records, ev.records) and torch.equal(events.counts, ev.counts)
        assert torch.equal(events.frame_counts, ev.frame_counts)


def test_localize_on_calibrated_clips(vad):
    """The video model's [B,T,1,H,W] maps, morphed after the calibration: in z-score units."""
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    stats = vad.scoring.calibrate(model, [{"frames": clips}], "cuda", sigma=1.0)
    with torch.no_grad():
        z = vad.scoring._anomaly_maps(model, clips, "mse", 1.0, 4.0, stats, vad.metrics.DEFAULT_MIN_STD)
    regions, maps = vad.scoring.localize(model, clips, 0.5, sigma=1.0, calibration=stats, morph=("close", 3))
    assert tuple(maps.shape) == (2, 4, 1, 32, 32) and ref.same_bits(maps.cpu().numpy(), ref.closing(z.cpu().numpy(), 3))
    table = vad.metrics.detect_regions(maps, 0.5)
    assert torch.equal(regions.records, table.records) and torch.equal(regions.counts, table.counts)
    events, emaps = vad.scoring.localize_events(model, clips, 0.5, sigma=1.0, calibration=stats, morph=("close", 3))
    ev = vad.metrics.detect_events(maps, 0.5)
    assert torch.equal(emaps, maps) and torch.equal(events.records, ev.records) and torch.equal(events.counts, ev.counts)
    assert stats.meta == {"map": "mse", "sigma": 1.0, "truncate": 4.0}        # the calibration knows nothing of the morphology


@pytest.mark.parametrize("split", [(1, 1, 1, 1, 1, 1), (2, 4)], ids=["one_by_one", "2_4"])
def test_localize_stream_morphs_every_frame_on_its_own(vad, split):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 6, 3, 32, 32)).cuda()
    with torch.no_grad():
        whole = vad.metrics.smooth_maps(model.score_stateful(clips, None, errmap=True)["errmap"], 1.0)
    morph = ("open", 2)
    t = _threshold(vad.metrics.morph_maps(whole, *morph), 0.9)                # a tenth of the morphed pixels are foreground
    kw = dict(threshold=t, connectivity=8, temporal=1, min_duration=1, min_volume=1, max_open=512, max_closed=256)
    tracker, by_hand = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    plain_tracker = vad.metrics.EventTracker(2, 32, 32, **kw)
    state, plain_state, f, seen, plain_seen = None, None, 0, [], []
    for k in split:
        chunk = clips[:, f:f + k]
        f += k
        _, plain, plain_state = vad.scoring.localize_stream(model, chunk, plain_tracker, plain_state, sigma=1.0)
        before = vad.hip.calls.get("morph_maps", 0)
        up, maps, state = vad.scoring.localize_stream(model, chunk, tracker, state, sigma=1.0, morph=morph)
        assert vad.hip.calls["morph_maps"] == before + 1
        hand = vad.metrics.morph_maps(plain, *morph)
        want = by_hand.update(hand)
        assert torch.equal(maps, hand) and tuple(maps.shape) == (2, k, 1, 32, 32)
        assert torch.equal(up.records, want.records) and torch.equal(up.counts, want.counts) and torch.equal(up.frame_counts, want.frame_counts)
        seen.append(maps)
        plain_seen.append(plain)
    assert torch.equal(tracker.state, by_hand.state)
    volume = torch.cat(seen, dim=1)
    assert ref.same_bits(volume.cpu().numpy(), ref.opening(torch.cat(plain_seen, dim=1).cpu().numpy(), 2))     # frame by frame
    assert int(tracker.flush().counts[:, 0].sum()) + int(volume.ge(t).sum()) > 0


def test_pixel_metrics_accumulate_the_morphed_maps(vad):
    model = _image_model(vad)
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32))
    rng = np.random.default_rng(12)
    raw = np.kron(rng.choice(np.array([0, 255], np.uint8), (6, 4, 4), p=[0.7, 0.3]), np.ones((1, 8, 8), np.uint8))
    masks = torch.from_numpy(raw).cuda()[:, None]
    loader = [{"image": x[:4], "mask": masks[:4]}, {"image": x[4:], "mask": masks[4:]}]
    morph, bits = [("open", 2), ("close", 3)], 11
    steps = vad.metrics.morph_steps(morph)
    before = vad.hip.calls.get("morph_maps", 0)
    _, _, hist = vad.scoring.pixel_auroc(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, morph=morph)
    assert vad.hip.calls["morph_maps"] == before + 2 * len(steps)
    hand, hand_pro, plain = vad.metrics.ScoreHistogram(bits), vad.metrics.ProHistogram(bits), vad.metrics.ScoreHistogram(bits)
    for b in loader:
        with torch.no_grad():
            sm = vad.metrics.smooth_maps(model.score_all(b["image"].cuda())["errmap"], 1.0)
        plain.accumulate(sm, b["mask"])
        morphed = vad.metrics.apply_morph(sm, steps)
        hand.accumulate(morphed, b["mask"])
        hand_pro.accumulate(morphed, b["mask"])
    assert torch.equal(hist.counts(), hand.counts()) and torch.equal(hist.rejected(), hand.rejected())
    assert not torch.equal(hist.counts(), plain.counts()) and int(hist.counts().sum() + hist.rejected().sum()) == 6 * 32 * 32
    _, _, _, pro = vad.scoring.pixel_aupro(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, morph=morph)
    assert torch.equal(pro.weighted(), hand_pro.weighted()) and torch.equal(pro.counts(), hand_pro.counts())
    before = vad.hip.calls["morph_maps"]
    _, _, none = vad.scoring.pixel_auroc(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, morph=None)
    assert torch.equal(none.counts(), plain.counts()) and vad.hip.calls["morph_maps"] == before


def test_an_opening_removes_speckle_and_keeps_the_defect(vad):
    th, tw = _tile(vad, 2, "open")
    h, w, by, bx = 2 * th + 6, 2 * tw + 22, th - 3, tw - 2                   # the defect lies across a tile corner
    rng = np.random.default_rng(4290)
    x = (rng.random((2, h, w)) * 0.2).astype(np.float32)                      # background below the threshold
    planted = 0
    for f in range(2):
        for i in range(1, h - 1, 4):
            for j in range(1 + 2 * (i // 4 % 2), w - 1, 5):                   # isolated single pixels: no two are neighbours
                if not (by - 4 <= i <= by + 9 and bx - 4 <= j <= bx + 10):
                    x[f, i, j] = 1.0 + rng.random()
                    planted += 1
        x[f, by:by + 6, bx + f:bx + 6 + f] = 2.0                              # a 6 x 6 defect
    maps = torch.from_numpy(x).cuda()
    t = 0.5
    raw = vad.metrics.detect_regions(maps, t, max_regions=1024)
    assert int(raw.counts[:, 0].sum()) == planted + 2 and planted > 500
    opened = vad.metrics.morph_maps(maps, "open", 2)
    clean = vad.metrics.detect_regions(opened, t, max_regions=1024)
    assert clean.counts[:, 0].tolist() == [1, 1] and clean.counts[:, 2].tolist() == [36, 36]
    assert clean.area[:, 0].tolist() == [36, 36] and clean.box[:, 0].tolist() == [[bx, by, bx + 5, by + 5], [bx + 1, by, bx + 6, by + 5]]
    assert clean.peak[:, 0].tolist() == [2.0, 2.0]
    assert bool((opened <= maps).all())                                       # anti-extensive: nothing is raised
    # the threshold commutes: the opening of the binary map is the binary map of the opening
    binary = vad.metrics.morph_maps((maps >= t).float(), "open", 2)
    assert torch.equal(binary > 0, opened >= t)
