"""Gaussian map smoothing on the GPU (csrc/map_smooth.hip, metrics.smooth_maps): the smoothed maps and their per-frame maxima equal
the numpy restatement (tests/map_smooth_ref.py) bit for bit on every shape that takes another path of the kernel; batch
independence, non-finite values, refusals, and the drivers through the seeded models."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_smooth_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

TH, TW = 32, 64            # the output tile of one work-group this file assumes (asserted against hip.SMOOTH_TILE and the library)

# name -> (shape, sigma, truncate, radius)
SHAPES = {
    "radius_is_h_and_w": ((1, 16, 16), 4.0, 4.0, 16),                       # both halos are entirely reflection
    "frames_h_ne_w": ((3, 32, 48), 4.0, 4.0, 16),
    "w_not_vector_multiple": ((2, 16, 20), 1.0, 4.0, 4),
    "smallest_frame": ((1, 2, 3), 0.5, 4.0, 2),
    "largest_radius": ((1, 32, 32), 8.0, 4.0, 32),
    "truncate_3": ((2, 24, 40), 2.0, 3.0, 6),
    "three_tiles_each_way": ((1, 3 * TH + 5, 3 * TW + 7), 4.0, 4.0, 16),    # top-left, interior, bottom-right tiles, ragged last tile
    "five_dims": ((2, 3, 1, 16, 16), 2.0, 4.0, 8),
}
_REF = {}


def _maps(shape, seed, signed=True):
    rng = np.random.default_rng(seed)
    x = (np.exp(rng.standard_normal(shape) * 3.0) * 1e-3).astype(np.float32)
    return x * rng.choice(np.array([-1, 1], np.float32), shape) if signed else x


def _case(name):
    """(input, restated smoothing, restated maxima): computed once per module, never modified."""
    if name not in _REF:
        shape, sigma, truncate, _ = SHAPES[name]
        x = _maps(shape, 500 + list(SHAPES).index(name))
        s = ref.smooth(x, sigma, truncate)
        _REF[name] = (x, s, ref.frame_max(s))
    return _REF[name]


def test_tile_constant(vad):
    th, tw = C.c_int(), C.c_int()
    assert vad.hip.lib().vad_smooth_tile(C.byref(th), C.byref(tw)) == 0
    assert (TH, TW) == vad.hip.SMOOTH_TILE == (th.value, tw.value)


@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_restatement(vad, name):
    shape, sigma, truncate, radius = SHAPES[name]
    assert vad.metrics.gaussian_taps(sigma, truncate)[0] == radius
    x, want, want_max = _case(name)
    xt = torch.from_numpy(x).cuda()
    before = vad.hip.calls.get("smooth_maps", 0)
    got, gmax = vad.metrics.smooth_maps(xt, sigma, truncate, return_max=True)
    assert vad.hip.calls["smooth_maps"] == before + 1
    assert got.shape == xt.shape and gmax.shape == xt.shape[:-2] and got.dtype == gmax.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(gmax.cpu(), torch.from_numpy(want_max))
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                       # the input is not touched
    # the map alone, into a buffer of the caller; the maxima alone, with no map
    out = torch.full_like(xt, float("nan"))
    assert vad.metrics.smooth_maps(xt, sigma, truncate, out=out) is out and torch.equal(out.cpu(), torch.from_numpy(want))
    only = vad.metrics.smooth_maps(xt, sigma, truncate, return_max="only")
    assert torch.equal(only.cpu(), torch.from_numpy(want_max))


def test_base_one_float_off_its_allocation(vad):
    """maps and out sliced one float into their allocations: 4-byte aligned bases; the floats around `out` keep their bits."""
    shape, sigma, truncate, _ = SHAPES["w_not_vector_multiple"]
    x, want, want_max = _case("w_not_vector_multiple")
    n = x.size
    buf = torch.zeros(n + 1, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xt = buf[1:].view(shape)
    obuf = torch.full((n + 2,), -7.0, device="cuda")
    out = obuf[1:n + 1].view(shape)
    assert xt.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and xt.is_contiguous()
    got, gmax = vad.metrics.smooth_maps(xt, sigma, truncate, out=out, return_max=True)
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(gmax.cpu(), torch.from_numpy(want_max))
    assert obuf[0].item() == -7.0 and obuf[-1].item() == -7.0


def test_empty_call(vad):
    x = torch.empty(0, 1, 16, 16, device="cuda")
    before = vad.hip.calls.get("smooth_maps", 0)
    got, gmax = vad.metrics.smooth_maps(x, 2.0, return_max=True)
    assert got.shape == (0, 1, 16, 16) and gmax.shape == (0, 1) and vad.hip.calls.get("smooth_maps", 0) == before
    lib = vad.hip.lib()
    taps, some = torch.zeros(9, device="cuda"), torch.full((2, 16, 16), 3.0, device="cuda")
    assert lib.vad_smooth_maps(some[0].data_ptr(), 0, 16, 16, taps.data_ptr(), 4, some[1].data_ptr(), None, None, 0, vad.hip.current_stream()) == 0
    assert bool((some == 3.0).all())


def test_frames_do_not_depend_on_the_batch(vad):
    x, want, want_max = _case("frames_h_ne_w")
    xt = torch.from_numpy(x).cuda()
    whole, wmax = vad.metrics.smooth_maps(xt, 4.0, return_max=True)
    for i in range(x.shape[0]):
        one, omax = vad.metrics.smooth_maps(xt[i:i + 1], 4.0, return_max=True)
        assert torch.equal(one[0], whole[i]) and torch.equal(omax[0], wmax[i])
    tail = vad.metrics.smooth_maps(xt[1:], 4.0)
    assert torch.equal(tail, whole[1:])


def test_nan_and_inf_follow_the_window(vad):
    shape, sigma = (3, 40, 70), 2.0                                         # two tiles along W; radius 8
    r = vad.metrics.gaussian_taps(sigma)[0]
    x = _maps(shape, 77, signed=False)
    clean = torch.from_numpy(x).cuda()
    base, base_max = vad.metrics.smooth_maps(clean, sigma, return_max=True)
    y = x.copy()
    y[1, 2, 66] = np.nan                                                    # near the top-right corner: reflected at both borders
    got, gmax = vad.metrics.smooth_maps(torch.from_numpy(y).cuda(), sigma, return_max=True)
    win = torch.from_numpy(ref.window(40, 70, 2, 66, r))
    assert 0 < int(win.sum()) < 40 * 70
    assert torch.equal(torch.isnan(got[1]).cpu(), win)
    assert torch.equal(got[1].cpu()[~win], base[1].cpu()[~win])
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2])    # the other frames keep every bit
    assert torch.isnan(gmax[1]).item() and torch.equal(gmax[[0, 2]], base_max[[0, 2]])
    want = ref.smooth(y, sigma)                                             # NaN != NaN: compared through the masks
    assert np.array_equal(np.isnan(want), np.isnan(got.cpu().numpy())) and np.array_equal(want[~np.isnan(want)], got.cpu().numpy()[~np.isnan(want)])
    z = x.copy()
    z[0, 39, 0] = np.inf
    got, gmax = vad.metrics.smooth_maps(torch.from_numpy(z).cuda(), sigma, return_max=True)
    win = torch.from_numpy(ref.window(40, 70, 39, 0, r))
    assert not torch.isnan(got).any()
    assert torch.equal(torch.isposinf(got[0]).cpu(), win) and torch.isposinf(gmax[0]).item()
    assert torch.equal(got[0].cpu()[~win], base[0].cpu()[~win]) and torch.equal(got[1:], base[1:])
    assert torch.equal(got.cpu(), torch.from_numpy(ref.smooth(z, sigma)))


def test_refusals(vad):
    VadError = vad.hip.VadError
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    x = torch.from_numpy(_maps((2, 16, 64), 9)).cuda()
    out = torch.full_like(x, 5.0)
    fmax = torch.full((2,), 5.0, device="cuda")
    taps = torch.from_numpy(vad.metrics.gaussian_taps(1.0)[1]).cuda()
    ws = torch.empty(lib.vad_smooth_workspace_bytes(2, 16, 64, 4), dtype=torch.uint8, device="cuda")
    assert ws.numel() == 2 * 4
    call = lambda *a: lib.vad_smooth_maps(*a, stream)
    for r in (0, 33, 17):
        assert call(x.data_ptr(), 2, 16, 64, taps.data_ptr(), r, out.data_ptr(), fmax.data_ptr(), ws.data_ptr(), ws.numel()) == -1, r
        assert b"radius" in lib.vad_last_error()
    assert call(x.data_ptr(), 2, 16, 64, taps.data_ptr(), 4, x.data_ptr(), None, None, 0) == -1 and b"overlaps" in lib.vad_last_error()
    assert call(x.data_ptr(), 1, 16, 64, taps.data_ptr(), 4, x[0, 8:].data_ptr(), None, None, 0) == -1 and b"overlaps" in lib.vad_last_error()
    assert call(x.data_ptr(), 2, 16, 64, taps.data_ptr(), 4, None, None, ws.data_ptr(), ws.numel()) == -1 and b"both NULL" in lib.vad_last_error()
    assert call(x.data_ptr(), 2, 16, 64, taps.data_ptr(), 4, out.data_ptr(), fmax.data_ptr(), ws.data_ptr(), ws.numel() - 1) == -3
    assert b"workspace" in lib.vad_last_error()
    assert call(x.data_ptr() + 2, 2, 16, 64, taps.data_ptr(), 4, out.data_ptr(), None, None, 0) == -1 and b"aligned" in lib.vad_last_error()
    with pytest.raises(VadError, match="contiguous"):
        vad.metrics.smooth_maps(x.transpose(1, 2), 1.0)
    with pytest.raises(VadError, match="contiguous"):
        vad.metrics.smooth_maps(x[:, :, ::2], 1.0)
    with pytest.raises(VadError, match="no CPU fallback"):
        vad.metrics.smooth_maps(x.cpu(), 1.0)
    with pytest.raises(VadError, match="float32"):
        vad.metrics.smooth_maps(x.half(), 1.0)
    with pytest.raises(VadError, match="sigma"):
        vad.metrics.smooth_maps(x, 0.0)
    with pytest.raises(VadError, match="sigma"):
        vad.metrics.smooth_maps(x, -4.0)
    with pytest.raises(VadError, match="sigma"):
        vad.metrics.smooth_maps(x, float("inf"))
    with pytest.raises(VadError, match="radius"):
        vad.metrics.smooth_maps(x, 8.25)                                    # radius 33
    with pytest.raises(VadError, match="one reflection"):
        vad.metrics.smooth_maps(x, 4.25)                                    # radius 17 > H = 16
    with pytest.raises(VadError, match="out must be"):
        vad.metrics.smooth_maps(x, 1.0, out=torch.empty(2, 16, 32, device="cuda"))
    with pytest.raises(VadError, match="overlaps"):
        vad.metrics.smooth_maps(x, 1.0, out=x)
    with pytest.raises(VadError, match="out must be None"):
        vad.metrics.smooth_maps(x, 1.0, out=out, return_max="only")
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((fmax == 5.0).all())           # a refused call writes nothing


# ------------------------------------------------------------------------------------------ through the models
def _image_loader(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32))
    rng = np.random.default_rng(12)
    raw = np.zeros((6, 48, 40), np.uint8)
    for i in range(6):
        raw[i] = np.kron(rng.choice(np.array([0, 127, 128, 255], np.uint8), (6, 5), p=[0.55, 0.1, 0.1, 0.25]), np.ones((8, 8), np.uint8))
    masks = vad.scoring.resize_masks(torch.from_numpy(raw).cuda(), 32)
    labels = np.array([0, 1, 0, 1, 1, 0])
    kinds = ["good", "scratch", "good", "spot", "scratch", "good"]
    loader = [{"image": x[:4], "mask": masks[:4], "label": labels[:4], "defect_type": kinds[:4]},
              {"image": x[4:], "mask": masks[4:], "label": labels[4:], "defect_type": kinds[4:]}]
    return model, loader, labels


def _raw_maps(model, batch, kind):
    with torch.no_grad():
        if kind == "mse":
            return model.score_all(batch["image"].cuda())["errmap"]
        return model.score_criteria(batch["image"].cuda(), ssim_map=True)["ssim_map"]


@pytest.mark.parametrize("kind", ["mse", "ssim"])
def test_drivers_smooth_before_they_accumulate(vad, kind):
    m, sigma = 11, 4.0                                                      # radius 16 on 32 x 32 maps
    model, loader, labels = _image_loader(vad)
    by_hand = [vad.metrics.smooth_maps(_raw_maps(model, b, kind), sigma, return_max=True) for b in loader]
    # the device maps are the restatement of the raw maps
    for b, (sm, mx) in zip(loader, by_hand):
        want = ref.smooth(_raw_maps(model, b, kind).cpu().numpy(), sigma)
        assert torch.equal(sm.cpu(), torch.from_numpy(want)) and torch.equal(mx.cpu(), torch.from_numpy(ref.frame_max(want)))

    before = vad.hip.calls.get("smooth_maps", 0)
    _, _, hist = vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=sigma)
    assert vad.hip.calls["smooth_maps"] == before + 2                       # one smoothing per batch
    hand = vad.metrics.ScoreHistogram(m)
    for b, (sm, _) in zip(loader, by_hand):
        hand.accumulate(sm, b["mask"])
    assert torch.equal(hist.counts(), hand.counts()) and torch.equal(hist.rejected(), hand.rejected())
    assert int(hist.counts().sum() + hist.rejected().sum()) == 6 * 32 * 32

    _, _, _, pro = vad.scoring.pixel_aupro(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=sigma)
    hand_pro = vad.metrics.ProHistogram(m)
    for b, (sm, _) in zip(loader, by_hand):
        hand_pro.accumulate(sm, b["mask"])
    assert torch.equal(pro.weighted(), hand_pro.weighted()) and torch.equal(pro.counts(), hand_pro.counts())
    assert pro.regions() == hand_pro.regions() and torch.equal(pro.counts(), hist.counts())

    # sigma=None is the call without the argument
    before = vad.hip.calls["smooth_maps"]
    _, _, plain = vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, mantissa_bits=m)
    _, _, none = vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=None)
    assert torch.equal(plain.counts(), none.counts()) and torch.equal(plain.rejected(), none.rejected())
    assert not torch.equal(plain.counts(), hist.counts())
    _, _, _, pplain = vad.scoring.pixel_aupro(model, loader, "cuda", map=kind, mantissa_bits=m)
    _, _, _, pnone = vad.scoring.pixel_aupro(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=None)
    assert torch.equal(pplain.weighted(), pnone.weighted()) and torch.equal(pplain.counts(), pnone.counts())
    assert vad.hip.calls["smooth_maps"] == before

    auroc, got_labels, scores, per = vad.scoring.compute_auroc_smoothed(model, loader, "cuda", sigma=sigma, map=kind)
    hand_scores = torch.cat([mx.reshape(-1) for _, mx in by_hand]).cpu().numpy()
    assert scores.dtype == np.float32 and np.array_equal(scores, hand_scores) and got_labels.tolist() == labels.tolist()
    assert auroc == vad.scoring.roc_auc(labels, hand_scores)
    assert set(per) == {"good", "scratch", "spot"} and per["good"]["count"] == 3 and per["spot"]["is_anomaly"] == 1
    with pytest.raises(vad.hip.VadError, match="map"):
        vad.scoring.compute_auroc_smoothed(model, loader, "cuda", map="psnr")


def test_video_maps_are_smoothed_frame_by_frame(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 3, 3, 32, 32)).cuda()
    with torch.no_grad():
        errmap = model.score_all(clips)["errmap"]
    assert errmap.shape == (2, 3, 1, 32, 32)
    got, gmax = vad.metrics.smooth_maps(errmap, 2.0, return_max=True)
    want = ref.smooth(errmap.cpu().numpy(), 2.0)
    assert gmax.shape == (2, 3, 1)
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(gmax.cpu(), torch.from_numpy(ref.frame_max(want)))
    one = vad.metrics.smooth_maps(errmap[1, 2].contiguous(), 2.0)           # a frame alone: nothing crosses time
    assert torch.equal(one, got[1, 2])
