"""Frames above 256 x 256, up to the kernels' frame-size limit.

A. Mid-size frames (camera sizes, odd counts of sixteenths, one-tile-wide strips): the models against the torch oracle at the
   project's bounds - scores 1e-5 relative, reconstruction 5e-5 absolute, layers ATOL of tests/test_hip_layers.py; none of them
   depends on the frame size, a per-pixel sum has the same terms in any frame - and the layers a model call cannot steer.
B. One frame just below VAD_MAX_FRAME_PIXELS = 2^23 - 1 (the persistent kernels multiply pixel indices as 24-bit operands,
   csrc/vad_common.h): 4096 x 2032 = 8,323,072 pixels through the layers whose pixel index is such an operand and through the
   image model; the next size up, 4112 x 2048, is refused.  The CPU half (refusals, size queries) is tests/test_scoring_plan.py.

Every reference is computed once per shape and shared by the cases that need it; oracle times (8 CPU cores) and the errors
measured on MI355X are in the docstrings.  The whole file takes 21 s there, the slowest case 2.3 s."""
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_synthetic, max_abs, rel_err
from oracle import c_oracle, torch_oracle
from ssim_score_ref import ssim_frames
from test_hip_layers import ATOL, _conv_params, _dec4_case, _dec4_run, _precision

pytestmark = pytest.mark.gpu

SCORE_RTOL, RECON_ATOL = 1e-5, 5e-5            # the fuzz's bounds (tests/test_hip_fuzz.py)
# errmap.mean() against the score: every map value is the kernel's own squared error rounded twice more (the division by 3 and
# nothing else: 2 x 2^-24 relative), and the score is the same squared errors through fp32 partial sums that the 1e-5 gate
# against the oracle already holds; 2e-6 is 32 fp32 roundings of headroom for those partial sums, whatever the frame size
MEAN_RTOL = 2e-6


def _state(st):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in st.items()}


def _as_u8(x):
    """float frames [..., 3, H, W] in [-1, 1] -> (uint8 [..., H, W, 3], the float frames those bytes normalise to)"""
    t = torch.from_numpy(np.clip(np.round((x * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8))
    nd = t.dim()
    u8 = t.permute(*range(nd - 3), nd - 2, nd - 1, nd - 3).contiguous()
    return u8, (t.float() / 255.0 - 0.5) / 0.5


def _score64(x, recon):
    """per-frame mean squared error of the oracle's reconstruction, the mean taken in float64"""
    d = x.double() - recon.double()
    return (d * d).flatten(1).mean(dim=1).numpy()


# ------------------------------------------------------------------------------ A1. image model
IMG_LATENT, IMG_WSEED = 32, 41
IMG_SHAPES = [(1088, 1920), (528, 784), (1024, 1024), (16, 4096), (4096, 16)]


def _img_model(vad, precision):
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=IMG_LATENT)
    st = load_synthetic(vad, m, IMG_WSEED)
    m = m.cuda().eval()
    m.precision = precision
    return m, st


@functools.lru_cache(maxsize=None)
def _img_ref(h, w):
    """One synthetic frame of h x w and the oracle's answer for it -> (x, recon, score); the state is the one _img_model loads."""
    import importlib
    vad = importlib.import_module("video-anomaly-detection_amd")
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=IMG_LATENT)
    st = _state(load_synthetic(vad, m, IMG_WSEED))
    x = torch.from_numpy(vad.synth.frames(9000 + h + w, 0, 1, 3, h, w))
    t0 = time.time()
    with torch.no_grad():
        recon = torch_oracle.img_forward(st, x)
    print(f"image oracle {h}x{w}: {time.time() - t0:.2f} s")
    return x, recon, _score64(x, recon)


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
@pytest.mark.parametrize("h,w", IMG_SHAPES, ids=lambda v: str(v))
def test_image_model_mid_size(vad, h, w, precision):
    """One frame of a camera size (1088 x 1920), of 33 x 49 sixteenths (both odd), of 2^20 pixels, and one latent row / column
    wide, in every arithmetic mode: scores, reconstruction, the error map's mean against the score, and uint8 ingest against the
    float path bit for bit.  Oracle (fp32 torch, the fuzz's; its mean in float64): 2.7 s at 1088 x 1920, 1.7 s at 1024 x 1024,
    1.1 s at 528 x 784 on 8 cores, computed once per shape.  Measured on MI355X, max over the 15 cases: score 9.4e-08, recon
    3.6e-07, map mean against score 9.1e-08; the three scoring calls of a case take 0.11 s at most."""
    x, ref_recon, ref_score = _img_ref(h, w)
    m, _ = _img_model(vad, precision)
    u8, as_f32 = _as_u8(x.numpy())
    t0 = time.time()
    with torch.no_grad():
        out = m.score_all(x.cuda())
        from_u8 = m.score_all(u8.cuda())
        from_f32 = m.score_all(as_f32.cuda())
    torch.cuda.synchronize()
    scores = out["scores"].cpu().numpy()
    d_score, d_recon = rel_err(scores, ref_score), max_abs(out["recon"].cpu().numpy(), ref_recon.numpy())
    d_mean = rel_err(out["errmap"].double().mean(dim=(1, 2, 3)).cpu().numpy(), scores)
    print(f"image {h}x{w} {precision}: score rel {d_score:.2e} recon abs {d_recon:.2e} errmap mean vs score {d_mean:.2e}; "
          f"three calls {time.time() - t0:.2f} s")
    assert out["recon"].shape == (1, 3, h, w) and out["errmap"].shape == (1, 1, h, w)
    assert d_score < SCORE_RTOL and d_recon < RECON_ATOL and d_mean < MEAN_RTOL
    for k in ("scores", "recon", "errmap"):
        assert torch.equal(from_u8[k], from_f32[k]), k                       # uint8 ingest == the same frames as fp32


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_image_model_rechunking_at_528x784(vad, precision):
    """Two frames of 528 x 784 in one launch group and in two: the same bits, and frame 0 is the one-frame call's."""
    h, w = 528, 784
    x1, _, _ = _img_ref(h, w)
    x2 = torch.cat([x1, torch.from_numpy(vad.synth.frames(77, 3, 1, 3, h, w))]).cuda()
    m, _ = _img_model(vad, precision)
    with torch.no_grad():
        m.chunk = 2
        both = m.score_all(x2)
        m.chunk = 1
        apart = m.score_all(x2)
        one = m.score_all(x2[:1])
    for k in ("scores", "recon", "errmap"):
        assert torch.equal(both[k], apart[k]) and torch.equal(both[k][:1], one[k]), k
    assert bool(torch.isfinite(both["scores"]).all()) and both["scores"][0] != both["scores"][1]


# ------------------------------------------------------------------------------ A2. video model
VID_WSEED = 43
#: (clips, frames, H, W): a 17 x 33 ConvLSTM map (both odd), and two clips of a 32 x 32 map
VID_CLIPS = [(1, 3, 272, 528), (2, 2, 512, 512)]
#: (latent, hidden, layers, precisions): equal widths in every arithmetic (the split ConvLSTM step needs them equal); and widths
#: that pad differently, with the projection - exact and Winograd (whose layer 0 then stays direct)
VID_MODELS = [(64, 64, 2, ("fp32", "split", "winograd")), (48, 96, 1, ("fp32", "winograd"))]


def _vid_model(vad, latent, hid, layers, precision):
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
    st = load_synthetic(vad, m, VID_WSEED)
    m = m.cuda().eval()
    m.precision = precision
    return m, st


@functools.lru_cache(maxsize=None)
def _vid_ref(b, t, h, w, latent, hid, layers):
    import importlib
    vad = importlib.import_module("video-anomaly-detection_amd")
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid, lstm_num_layers=layers)
    st = _state(load_synthetic(vad, m, VID_WSEED))
    x = torch.from_numpy(vad.synth.clips(9100 + h + w, 0, b, t, 3, h, w))
    t0 = time.time()
    with torch.no_grad():
        recon = torch_oracle.vid_forward(st, x, hid, layers)
    print(f"video oracle {b}x{t} {h}x{w} latent {latent} hid {hid}: {time.time() - t0:.2f} s")
    frame = _score64(x.flatten(0, 1), recon.flatten(0, 1)).reshape(b, t)
    return x, recon, frame


@pytest.mark.parametrize("case", [(c, m[:3], p) for c in VID_CLIPS for m in VID_MODELS for p in m[3]],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[0][2]}x{c[0][3]}-l{c[1][0]}h{c[1][1]}-{c[2]}")
def test_video_model_mid_size(vad, case):
    """Clip and frame scores and the reconstruction against the oracle, and the stateful form of the same frames against the
    clip form bit for bit (tests/test_stateful.py: zero state is the stateless path).  Oracle: 0.3 s per shape at most.  Measured
    on MI355X, max over the cases: frame score 1.2e-07, clip score 5.2e-08, recon 2.4e-07, map mean against score 1.2e-07."""
    (b, t, h, w), (latent, hid, layers), precision = case
    x, ref_recon, ref_frame = _vid_ref(b, t, h, w, latent, hid, layers)
    m, _ = _vid_model(vad, latent, hid, layers, precision)
    t0 = time.time()
    with torch.no_grad():
        out = m.score_all(x.cuda())
        st = m.score_stateful(x.cuda(), None, errmap=True, recon=True)
    torch.cuda.synchronize()
    d_frame = rel_err(out["frame"].cpu().numpy(), ref_frame)
    d_seq = rel_err(out["seq"].cpu().numpy(), ref_frame.mean(axis=1))
    d_recon = max_abs(out["recon"].cpu().numpy(), ref_recon.numpy())
    d_mean = rel_err(out["errmap"].double().mean(dim=(2, 3, 4)).cpu().numpy(), out["frame"].cpu().numpy())
    print(f"video {case}: frame rel {d_frame:.2e} seq rel {d_seq:.2e} recon abs {d_recon:.2e} errmap mean vs score {d_mean:.2e}; "
          f"two calls {time.time() - t0:.2f} s")
    assert d_frame < SCORE_RTOL and d_seq < SCORE_RTOL and d_recon < RECON_ATOL and d_mean < MEAN_RTOL
    assert torch.equal(st["frame"], out["frame"]) and torch.equal(st["errmap"], out["errmap"]) and torch.equal(st["recon"], out["recon"])


# ------------------------------------------------------------------------------ A3. layers a model call cannot steer
def _ref_layer64(x, wt, b, bn, act, pool):
    """Conv2d(3x3, padding 1) + eval BatchNorm + activation (+ MaxPool2d(2)) in float64 torch; x a float tensor [N,C,H,W]."""
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    y = F.conv2d(x.double(), t64(wt), t64(b), padding=1)
    if bn is not None:
        y = F.batch_norm(y, t64(bn[2]), t64(bn[3]), t64(bn[0]), t64(bn[1]), training=False, eps=1e-5)
    y = F.leaky_relu(y, 0.2) if act == 1 else F.relu(y) if act == 2 else y
    return F.max_pool2d(y, 2, 2) if pool else y


def test_dec4_fused_six_strips_ragged_bands():
    """vad_dec4_score on a 33 x 640 input map (66 x 1280 frame): six column strips, and 33 rows leave a ragged last band under
    every band height - against the oracle, the two launches it replaces and itself under other band heights, as
    test_dec4_fused_kernel states them.  Measured on MI355X: recon 5.3e-07, error map 4.9e-07, score 5.7e-08 relative."""
    import hip_helpers as H
    n, h, w = 1, 33, 640
    assert H.hip.lib().vad_dec4_score_partials(2 * h, 2 * w) == 2 * h * 6 * 4
    case = _dec4_case(np.random.default_rng(n * 1000 + h * 10 + w), n, h, w)
    x_in, wt, bt, bn, w3, b3, frames = case
    act = np.maximum(c_oracle.batchnorm_eval(c_oracle.convt2x2(x_in, wt, bt), *bn), 0)
    ref_recon = np.tanh(c_oracle.conv2d(act, w3, b3, 3).astype(np.float64))
    ref_emap = ((frames.astype(np.float64) - ref_recon) ** 2).mean(axis=1)
    ref_scores = ref_emap.mean(axis=(1, 2))
    recon, emap, scores = _dec4_run(H, case, fused=True)
    assert np.isfinite(recon).all() and np.isfinite(emap).all() and np.isfinite(scores).all()
    print(f"dec4 33x640: recon {max_abs(recon, ref_recon):.2e} errmap {max_abs(emap, ref_emap):.2e} score rel {rel_err(scores, ref_scores):.2e}")
    assert max_abs(recon, ref_recon) < ATOL and max_abs(emap, ref_emap) < ATOL
    assert rel_err(scores, ref_scores) < 1e-5
    r2, e2, s2 = _dec4_run(H, case, fused=False)
    assert max_abs(recon, r2) < 2e-6 and rel_err(scores, s2) < 1e-6
    for band in (1, 2, 5, 16, 1000):
        rb, eb, sb = _dec4_run(H, case, fused=True, band=band)
        assert np.array_equal(recon, rb) and np.array_equal(emap, eb) and np.array_equal(scores, sb), band


@pytest.mark.parametrize("form", ["direct", "split", "winograd"])
@pytest.mark.parametrize("cin,cout,pool", [(32, 64, True), (64, 128, False)])
def test_conv3x3_on_a_544x960_frame(cin, cout, pool, form):
    """enc2.0-like (32 -> 64, pooled here) and enc3.0-like (64 -> 128) layers on ONE 544 x 960 frame: 34 x 60 tiles of 16 x 16, a
    grid far past one wave of work-groups per CU.  Reference: float64 torch on the CPU (0.4 s / 1.0 s on 8 cores; most of a
    case's 0.7 s / 2.0 s is the layout changes of 67 M values on the host).  Measured on MI355X, 32 -> 64 | 64 -> 128: direct
    1.1e-05 | 2.1e-05, split 4.4e-06 | 6.7e-06, Winograd 3.9e-06 | 6.8e-06."""
    import hip_helpers as H
    h, w = 544, 960
    rng = np.random.default_rng(cin * 1000 + cout + h)
    x = rng.standard_normal((1, cin, h, w)).astype(np.float32)
    wt, b, bn = _conv_params(rng, cout, cin)
    ref = _ref_layer64(torch.from_numpy(x), wt, b, bn, 1, pool).numpy()
    if form == "winograd":
        got = H.conv3x3_wino(x, wt, b, bn, 1, pool)
    else:
        with _precision(H, 1 if form == "split" else 0):
            got = H.conv3x3(x, wt, b, bn, 1, pool)
    print(f"conv3x3 {cin}->{cout} pool {pool} {form} 544x960: max abs err {max_abs(got, ref):.2e}")
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert max_abs(got, ref) < ATOL


def test_ssim_score_on_a_1088x1920_frame(vad):
    """vad_ssim_score with its map on one 1088 x 1920 plane (34 x 60 tiles of 32 x 32) against the float64 composition, at the
    bounds of tests/test_hip_ssim_score.py: the frame value within GEOM_ATOL, the map within the conditioning rule of its test 5.
    One channel: the float64 composition takes 1.7 s per channel on 8 cores, and the kernel treats every channel alike.
    Measured on MI355X: frame value 3.3e-09, map 4.1e-06 against 5.6e-06 of the fp32 composition."""
    import hip_helpers as H
    from test_hip_ssim_score import GEOM_ATOL, _kernel, _pair
    p, t = _pair(1088 * 1920, 1, 1, 1088, 1920)
    want, want_map = ssim_frames(p, t, 11)
    ref_dev = max_abs(ssim_frames(p, t, 11, torch.float32)[1].numpy(), want_map.numpy())
    out = _kernel(vad, H.dev(p), H.dev(t), 11)
    d, d_map = max_abs(out["ssim"].cpu().numpy(), want.numpy()), max_abs(out["ssim_map"].cpu().numpy(), want_map.numpy())
    print(f"ssim 1088x1920: frame {d:.2e} map {d_map:.2e} (fp32 composition {ref_dev:.2e})")
    assert d < GEOM_ATOL and d_map <= 4 * ref_dev + 2e-6


# ------------------------------------------------------------------------------ B. just below the frame-size limit
BIG_H, BIG_W = 4096, 2032                      # 8,323,072 pixels <= VAD_MAX_FRAME_PIXELS = 8,388,607 < 4112 x 2048
BAND = 24


def _bands(h, w):
    """The first 24 rows, 24 rows around pixel index 2^22 (where bit 22 of the index sets in), and the last 24 rows."""
    mid = (1 << 22) // w - BAND // 2
    return [(0, BAND), (mid, mid + BAND), (h - BAND, h)]


@pytest.fixture(scope="module")
def big_map():
    """A 4096 x 2032 x 32 NHWC map of uniform [0, 1) values (post-ReLU-like) on the host: 1 GiB, made once for section B."""
    assert BIG_H * BIG_W <= 2 ** 23 - 1 < (BIG_H + 16) * (BIG_W + 16)
    rng = np.random.default_rng(4096 * 2032)
    yield torch.from_numpy(rng.random((1, BIG_H, BIG_W, 32), dtype=np.float32))


def _band_ref(x_nhwc, r0, r1, fn, scale=1):
    """fn (float64, zero padding, translation-invariant, +-1 row of support) of rows [r0, r1) of the map: the band is cut with one
    row of halo where the frame goes on, fn pads where it ends, and the halo's output rows are dropped.  scale: output rows per
    input row."""
    h = x_nhwc.shape[1]
    lo, hi = max(r0 - 1, 0), min(r1 + 1, h)
    y = fn(x_nhwc[:, lo:hi].permute(0, 3, 1, 2).double())
    return y[:, :, scale * (r0 - lo):scale * (r1 - lo)]


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("form", ["direct", "winograd"])
def test_conv3x3_32_to_32_just_below_the_pixel_limit(big_map, form):
    """vad_conv3x3 / vad_conv3x3_wino, 32 -> 32 un-pooled, one 4096 x 2032 frame (1 GiB in, 1 GiB out): three row bands against
    float64, and no NaN of the prefilled output left anywhere.  Measured on MI355X: direct 3.3e-06, Winograd 1.1e-06 in every
    band; 0.14 s per case.  (Tried once with the pixel checks compiled out and a 4112 x 2048 frame: the call answers VAD_OK, rows
    4096..4111 - pixel indices from 2^23 - are never written and row 4095 is off by 2.7, having read zeros below it.)"""
    import hip_helpers as H
    l = H.hip.lib()
    rng = np.random.default_rng(32032 + BIG_H)
    wt, b, bn = _conv_params(rng, 32, 32)
    try:
        xin = big_map.cuda()
        out = torch.full((1, BIG_H, BIG_W, 32), float("nan"), device="cuda")
        if form == "winograd":
            keep, bnp = H._bn_ptrs(bn)
            wp = np.empty(l.vad_pack_conv3x3_wino_floats(32, 32), np.float32)
            bo = np.empty(32, np.float32)
            H.hip.check(l.vad_pack_conv3x3_wino(wt.ctypes.data, b.ctypes.data, bnp, 32, 32, wp.ctypes.data, bo.ctypes.data))
            wp, bo = H.dev(wp), H.dev(bo)
            H.hip.check(l.vad_conv3x3_wino(xin.data_ptr(), 0, wp.data_ptr(), bo.data_ptr(), out.data_ptr(), 0, 1, BIG_H, BIG_W, 32, 32, 1, 0, H.stream()))
        else:
            wp, bo = H.pack_conv3x3(wt, b, bn)
            H.hip.check(l.vad_conv3x3(xin.data_ptr(), 0, wp.data_ptr(), bo.data_ptr(), out.data_ptr(), 0, 1, BIG_H, BIG_W, 32, 32, 1, 0, 0, H.stream()))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any())
        for r0, r1 in _bands(BIG_H, BIG_W):
            ref = _band_ref(big_map, r0, r1, lambda v: _ref_layer64(v, wt, b, bn, 1, False)).numpy()
            got = out[:, r0:r1].permute(0, 3, 1, 2).cpu().numpy()
            print(f"conv3x3 {form} 4096x2032 rows {r0}..{r1}: max abs err {max_abs(got, ref):.2e}")
            assert max_abs(got, ref) < ATOL, (r0, r1)
    finally:
        xin = out = None
        _free()


def test_dec4_score_just_below_the_pixel_limit(big_map):
    """vad_dec4_score on a 4096 x 2032 input map (an 8192 x 4064 frame: 17 strips): reconstruction and error map of three bands
    against float64, no NaN left in either, and the score - finite - is the error map's mean.  Measured on MI355X: recon 4.3e-07,
    error map 5.5e-07, score against the map's mean 2.6e-07; 0.8 s."""
    import hip_helpers as H
    l = H.hip.lib()
    h, w, h2, w2 = BIG_H, BIG_W, 2 * BIG_H, 2 * BIG_W
    rng = np.random.default_rng(40962032)
    _, wt, bt, bn, w3, b3, _ = _dec4_case(rng, 1, 1, 8)
    frames = torch.from_numpy(rng.random((1, 3, h2, w2), dtype=np.float32)) * 2 - 1
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()

    def ref_fn(v):
        y = F.conv_transpose2d(v, t64(wt), t64(bt), stride=2)
        y = F.relu(F.batch_norm(y, t64(bn[2]), t64(bn[3]), t64(bn[0]), t64(bn[1]), training=False, eps=1e-5))
        return torch.tanh(F.conv2d(y, t64(w3), t64(b3), padding=1))

    wtp, btp = H.pack_convt(wt, bt, bn)
    w3p = np.empty(l.vad_pack_conv3x3_to3_floats(32), np.float32)
    H.hip.check(l.vad_pack_conv3x3_to3(np.ascontiguousarray(w3).ctypes.data, 32, w3p.ctypes.data))
    w3d, b3d = H.dev(w3p), H.dev(b3)
    try:
        xin, xf = big_map.cuda(), frames.cuda()
        recon = torch.full((1, 3, h2, w2), float("nan"), device="cuda")
        emap = torch.full((1, h2, w2), float("nan"), device="cuda")
        scores = torch.full((1,), float("nan"), device="cuda")
        nparts = l.vad_dec4_score_partials(h2, w2)
        parts = torch.full((1, nparts), float("nan"), device="cuda")
        H.hip.check(l.vad_dec4_score(xin.data_ptr(), wtp.data_ptr(), btp.data_ptr(), w3d.data_ptr() + 4 * 8 * 108, b3d.data_ptr(),
                                     xf.data_ptr(), parts.data_ptr(), recon.data_ptr(), emap.data_ptr(), 1, h, w, H.stream()))
        H.hip.check(l.vad_score_finalize(parts.data_ptr(), nparts, 1, h2, w2, scores.data_ptr(), None, 1, H.stream()))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(recon).any()) and not bool(torch.isnan(emap).any()) and not bool(torch.isnan(parts).any())
        score, mean = float(scores[0]), float(emap.double().mean())
        print(f"dec4 4096x2032: score {score:.7f} errmap mean {mean:.7f} rel {abs(score - mean) / mean:.2e}")
        assert np.isfinite(score) and abs(score - mean) / mean < MEAN_RTOL
        for r0, r1 in _bands(h, w):
            ref = _band_ref(big_map, r0, r1, ref_fn, scale=2)
            ref_e = ((frames[:, :, 2 * r0:2 * r1].double() - ref) ** 2).mean(dim=1).numpy()
            d_r = max_abs(recon[:, :, 2 * r0:2 * r1].cpu().numpy(), ref.numpy())
            d_e = max_abs(emap[:, 2 * r0:2 * r1].cpu().numpy(), ref_e)
            print(f"dec4 4096x2032 input rows {r0}..{r1}: recon {d_r:.2e} errmap {d_e:.2e}")
            assert d_r < ATOL and d_e < ATOL, (r0, r1)
    finally:
        xin = xf = recon = emap = parts = None
        _free()


@pytest.mark.parametrize("u8", [False, True], ids=["fp32", "uint8"])
def test_image_model_just_below_the_pixel_limit(vad, u8):
    """One 4096 x 2032 frame through the image model (exact fp32; float and uint8 input): rows [0, 128) and [H - 128, H) of the
    reconstruction against the oracle run on the 256-row crops at the top and the bottom - the network's receptive field is
    under 64 rows each way and eval-mode BatchNorm is pointwise, so the half of a crop away from its cut is exact -, no NaN
    left anywhere, and the error map's mean against the score.  Measured on MI355X: recon 3.0e-07 in both halves, score against
    the map's mean 8.7e-08 (float) and 1.5e-07 (uint8); 0.7-0.8 s per case."""
    h, w = BIG_H, BIG_W
    m, st = _img_model(vad, "fp32")
    st = _state(st)
    rng = np.random.default_rng(2032 + int(u8))
    x = torch.from_numpy(rng.random((1, 3, h, w), dtype=np.float32)) * 2 - 1
    if u8:
        xu, x = _as_u8(x.numpy())
    try:
        nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
        out = {"scores": nan(1), "errmap": nan(1, 1, h, w), "recon": nan(1, 3, h, w)}       # (score_all's own are torch.empty)
        with torch.no_grad():
            got = m._run_hip((xu if u8 else x).cuda(), scores=True, errmap=True, recon=True, out=out)
        torch.cuda.synchronize()
        assert all(got[k].data_ptr() == v.data_ptr() for k, v in out.items())                 # the call wrote into the prefilled tensors
        assert all(not bool(torch.isnan(v).any()) for v in out.values())
        score, mean = float(out["scores"][0]), float(out["errmap"].double().mean())
        print(f"image 4096x2032 u8 {u8}: score {score:.7f} errmap mean {mean:.7f} rel {abs(score - mean) / mean:.2e}")
        assert abs(score - mean) / mean < MEAN_RTOL
        for name, crop, keep in (("top", slice(0, 256), slice(0, 128)), ("bottom", slice(h - 256, h), slice(128, 256))):
            with torch.no_grad():
                ref = torch_oracle.img_forward(st, x[:, :, crop])[:, :, keep]
            got = out["recon"][:, :, crop][:, :, keep].cpu()
            print(f"image 4096x2032 u8 {u8} {name} 128 rows: recon abs {max_abs(got.numpy(), ref.numpy()):.2e}")
            assert max_abs(got.numpy(), ref.numpy()) < RECON_ATOL, name
    finally:
        out = m = None                          # (the workspace goes with the model)
        _free()


def test_image_model_refuses_the_next_size_up(vad):
    """4112 x 2048 = 8,421,376 pixels: refused through Python (VadError naming the limit) and through the C ABI (VAD_ERR_ARG)
    before anything is launched - the score stays what it was."""
    h, w = BIG_H + 16, BIG_W + 16
    m, _ = _img_model(vad, "fp32")
    l = vad.hip.lib()
    assert l.vad_img_workspace_bytes_c(1, h, w, IMG_LATENT, 3) == 0 and l.vad_img_workspace_bytes_c(1, BIG_H, BIG_W, IMG_LATENT, 3) > 0
    x = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    score = torch.full((1,), float("nan"), device="cuda")
    try:
        with torch.no_grad(), pytest.raises(vad.hip.VadError, match=str(vad.hip.MAX_FRAME_PIXELS)):
            m._run_hip(x, scores=True, out={"scores": score})
        with torch.no_grad(), pytest.raises(vad.hip.VadError, match="multiples of 16 with"):
            m.get_reconstruction_error(x)
        small = torch.zeros(1 << 16, device="cuda")
        rc = l.vad_img_score_c(x.data_ptr(), vad.hip.X_U8_NHWC, 0, 3, 1, h, w, IMG_LATENT, small.data_ptr(), small.data_ptr(), small.numel() * 4, 1,
                               score.data_ptr(), None, None, None, vad.hip.current_stream())
        assert rc == -1 and str(vad.hip.MAX_FRAME_PIXELS).encode() in l.vad_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(score).all())
    finally:
        x = None
        _free()
