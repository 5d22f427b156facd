"""Device Resize of uint8 frames (vad_resize_u8, scoring.FrameResizer) against PIL: every comparison is `torch.equal`, there is
no tolerance anywhere - the resample is integer fixed point, so the device bytes are PIL's bytes and the scores of raw frames
are the scores of the frames PIL resized."""
import threading

import numpy as np
import pytest
import torch

import resize_ref as R
from conftest import GOLDEN, load_synthetic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "resize" / "pil_bilinear.npz", allow_pickle=False)


def _noise(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).cuda()


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixture_cases_equal_pil(vad, fixture, name):
    """Device output == PIL's stored output, RGB order; the BGR flag on the channel-flipped input gives the same bytes."""
    _, _, _, _, _, oh, ow = R.CASES[name]
    x = torch.from_numpy(R.case_input(name)).cuda()
    want = torch.from_numpy(fixture["out_" + name]).cuda()
    before = vad.hip.calls.get("resize_u8", 0)
    got = vad.scoring.FrameResizer((oh, ow))(x)
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want)
    assert vad.hip.calls["resize_u8"] == before + 1
    bgr = x.flip(-1).contiguous()
    assert torch.equal(vad.scoring.FrameResizer((oh, ow), channel_order="bgr")(bgr), want)
    assert torch.equal(vad.scoring.resize_frames(x, (oh, ow)), want)


def test_fresh_geometries_equal_live_pil(vad):
    Image = pytest.importorskip("PIL.Image")
    for i, (ih, iw, oh, ow) in enumerate(R.random_geometries(77, 20)):
        x = np.random.default_rng(500 + i).integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        pil = np.asarray(Image.fromarray(x, "RGB").resize((ow, oh), Image.BILINEAR))
        got = vad.scoring.resize_frames(torch.from_numpy(x).cuda(), (oh, ow))
        assert torch.equal(got.cpu(), torch.from_numpy(pil.copy())), (ih, iw, oh, ow)


def test_fresh_geometries_equal_the_restatement(vad):
    """The same sweep against the numpy restatement (pinned to PIL by tests/test_resize_plan.py): runs where PIL is absent."""
    for i, (ih, iw, oh, ow) in enumerate(R.random_geometries(78, 20)):
        x = np.random.default_rng(600 + i).integers(0, 256, (2, ih, iw, 3), dtype=np.uint8)
        got = vad.scoring.resize_frames(torch.from_numpy(x).cuda(), (oh, ow)).cpu().numpy()
        for f in range(2):
            assert np.array_equal(got[f], R.resize_ref(x[f], oh, ow)), (ih, iw, oh, ow)
        bgr = vad.scoring.resize_frames(torch.from_numpy(x[..., ::-1].copy()).cuda(), (oh, ow), channel_order="bgr").cpu().numpy()
        assert np.array_equal(bgr, got), (ih, iw, oh, ow)


@pytest.mark.parametrize("geo", [(90, 160, 32, 48), (45, 64, 45, 32), (70, 31, 20, 31)])
def test_batch_independence_and_leading_axes(vad, geo):
    ih, iw, oh, ow = geo
    rz = vad.scoring.FrameResizer((oh, ow))
    x = _noise(3, 17, ih, iw, 3)
    alone = torch.stack([rz(x[i:i + 1])[0] for i in range(17)])
    for n in (1, 3, 17):
        assert torch.equal(rz(x[:n]), alone[:n])
    assert torch.equal(rz(x[2:14]), alone[2:14])                       # a slice that does not start at the allocation
    y = x[:12].view(3, 4, ih, iw, 3)
    assert torch.equal(rz(y), alone[:12].view(3, 4, oh, ow, 3))
    assert torch.equal(rz(x[5]), alone[5])                             # no leading axis at all
    assert rz(x[:0]).shape == (0, oh, ow, 3)


def test_identity_copies_and_constant_frames_stay_constant(vad):
    x = _noise(4, 2, 64, 64, 3)
    y = vad.scoring.resize_frames(x, 64)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()
    assert torch.equal(vad.scoring.resize_frames(x, 64, channel_order="bgr"), x.flip(-1))
    for name, (_, _, _, ih, iw, oh, ow) in R.CASES.items():
        for value in (0, 1, 127, 255):
            c = torch.full((1, ih, iw, 3), value, dtype=torch.uint8, device="cuda")
            out = vad.scoring.resize_frames(c, (oh, ow))
            assert out.shape == (1, oh, ow, 3) and bool((out == value).all()), (name, value)


def test_plan_of_another_geometry_never_yields_pixels(vad):
    """The C ABI's guard: the kernels compare the plan header with the call's sizes on the device and write zeros."""
    lib = vad.hip.lib()

    def plan(ih, iw, oh, ow):
        blob = np.empty(lib.vad_resize_plan_bytes(ih, iw, oh, ow) // 4, np.int32)
        vad.hip.check(lib.vad_resize_plan(ih, iw, oh, ow, blob.ctypes.data))
        return torch.from_numpy(blob).cuda()
    x = _noise(5, 2, 96, 128, 3)
    x[:] = x.clamp(min=1)
    ws = torch.empty(lib.vad_resize_workspace_bytes(2, 96, 128, 32, 32), dtype=torch.uint8, device="cuda")
    for p in (plan(96, 128, 32, 32), plan(128, 96, 32, 32), plan(96, 128, 32, 48), torch.zeros(4096, dtype=torch.int32, device="cuda")):
        out = torch.full((2, 32, 32, 3), 9, dtype=torch.uint8, device="cuda")
        vad.hip.check(lib.vad_resize_u8(x.data_ptr(), 2, 96, 128, 0, p.data_ptr(), out.data_ptr(), 32, 32, ws.data_ptr(), ws.numel(),
                                        vad.hip.current_stream()))
        if p[2:6].tolist() == [96, 128, 32, 32]:
            assert torch.equal(out, vad.scoring.resize_frames(x, 32)) and bool((out > 0).all())
        else:
            assert not bool(out.any())


def test_one_resizer_two_geometries_and_two_threads(vad):
    a, b = _noise(6, 3, 120, 200, 3), _noise(7, 2, 77, 50, 3)
    want_a, want_b = vad.scoring.resize_frames(a, (32, 48)), vad.scoring.resize_frames(b, (32, 48))
    rz = vad.scoring.FrameResizer((32, 48))
    for _ in range(2):
        assert torch.equal(rz(a), want_a) and torch.equal(rz(b), want_b)
    assert len(rz._plans) == 2
    torch.cuda.synchronize()
    results, errors = {}, []

    def work(key, x):
        try:
            s = torch.cuda.Stream()
            mine = vad.scoring.FrameResizer((32, 48))
            with torch.cuda.stream(s):
                outs = [mine(x) for _ in range(20)]
            s.synchronize()
            results[key] = outs
        except Exception as e:                                          # noqa: BLE001 - reported by the asserting thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=("a", a)), threading.Thread(target=work, args=("b", b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(torch.equal(o, want_a) for o in results["a"]) and all(torch.equal(o, want_b) for o in results["b"])


# ------------------------------------------------------------------------------ end to end
def _img_model(vad, precision):
    m = vad.ConvAutoencoder()
    load_synthetic(vad, m, 1)
    m.precision = precision
    return m.cuda().eval()


def _vid_model(vad, precision):
    m = vad.VideoAutoencoder()
    load_synthetic(vad, m, 2)
    m.precision = precision
    return m.cuda().eval()


@pytest.mark.parametrize("precision", ["fp32", "winograd"])
def test_raw_frame_scores_equal_pil_resized_scores(vad, fixture, precision):
    raw = torch.from_numpy(R.case_input("240p_64_x6")).cuda()               # six 240x320 frames
    pil = torch.from_numpy(fixture["out_240p_64_x6"]).cuda()                # the same frames, resized to 64x64 by PIL
    img = _img_model(vad, precision)
    with torch.no_grad():
        want = img.get_reconstruction_error(pil)
        want_map = img.get_reconstruction_error(pil, per_pixel=True)
    n0 = vad.hip.calls["img_score"]
    assert torch.equal(vad.scoring.score_raw_images(img, raw, image_size=64), want)
    assert torch.equal(vad.scoring.score_raw_images(img, raw, image_size=64, per_pixel=True), want_map)
    assert torch.equal(vad.scoring.score_raw_images(img, raw.flip(-1).contiguous(), image_size=64, channel_order="bgr"), want)
    assert vad.hip.calls["img_score"] == n0 + 3
    vid = _vid_model(vad, precision)
    clips_raw, clips_pil = raw.view(2, 3, 240, 320, 3), pil.view(2, 3, 64, 64, 3)
    with torch.no_grad():
        want_seq = vid.get_reconstruction_error(clips_pil)
        want_frame = vid.get_reconstruction_error(clips_pil, per_frame=True)
    assert torch.equal(vad.scoring.score_raw_clips(vid, clips_raw, image_size=64), want_seq)
    assert torch.equal(vad.scoring.score_raw_clips(vid, clips_raw, image_size=(64, 64), per_frame=True), want_frame)
    # one live stream, a raw frame at a time, against the PIL-resized frames fed the existing way
    s_raw, st_raw = vad.scoring.score_frames_stateful(vid, (raw[i:i + 1] for i in range(6)), batch=1, image_size=64)
    s_pil, st_pil = vad.scoring.score_frames_stateful(vid, (pil[i:i + 1] for i in range(6)), batch=1)
    assert s_raw.shape == (1, 6) and np.array_equal(s_raw, s_pil) and torch.equal(st_raw.blob, st_pil.blob)
    s_cpu, st_cpu = vad.scoring.score_frames_stateful(vid, (raw[i:i + 1].cpu().numpy() for i in range(6)), batch=1, device="cuda",
                                                      image_size=64)
    assert np.array_equal(s_cpu, s_pil) and torch.equal(st_cpu.blob, st_pil.blob)


def test_full_size_frame_through_the_image_model(vad, fixture):
    raw = torch.from_numpy(R.case_input("1080p_256")).cuda()
    pil = torch.from_numpy(fixture["out_1080p_256"]).cuda()
    img = _img_model(vad, "fp32")
    with torch.no_grad():
        want = img.get_reconstruction_error(pil)
    assert torch.equal(vad.scoring.score_raw_images(img, raw), want)           # image_size defaults to 256


def test_python_refusals(vad):
    S = vad.scoring
    ok = torch.zeros(2, 48, 64, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(vad.hip.VadError, match="GPU tensor"):
        S.resize_frames(ok.cpu(), 32)
    with pytest.raises(vad.hip.VadError, match="uint8"):
        S.resize_frames(ok.float(), 32)
    with pytest.raises(vad.hip.VadError, match="contiguous"):
        S.resize_frames(ok[:, ::2], 32)
    with pytest.raises(vad.hip.VadError, match=r"\[\.\.\., H, W, 3\]"):
        S.resize_frames(torch.zeros(2, 48, 64, 4, dtype=torch.uint8, device="cuda"), 32)
    with pytest.raises(vad.hip.VadError, match="channel_order"):
        S.FrameResizer(32, channel_order="grb")
    with pytest.raises(vad.hip.VadError, match="unsupported geometry"):
        S.resize_frames(torch.zeros(1, 130, 8, 3, dtype=torch.uint8, device="cuda"), (2, 8))       # 65-fold
    with pytest.raises(vad.hip.VadError, match="unsupported geometry"):
        S.resize_frames(ok, 4097)
    with pytest.raises(vad.hip.VadError, match="unsupported geometry"):
        S.resize_frames(ok, 0)
    vid = _vid_model(vad, "fp32")
    with pytest.raises(vad.hip.VadError, match="uint8"):
        S.score_frames_stateful(vid, [ok.float()], batch=2, image_size=32)
