"""Device Resize of one-byte (`l`) and four-byte (`rgba`, `bgra`) frames (vad_resize_u8_f, scoring.FrameResizer(pixel_format=))
against PIL's `convert('RGB')` / `convert('L')` + resize: every comparison is `torch.equal`, there is no tolerance anywhere.
Expected bytes are PIL's stored ones (tests/golden/resize_formats) or tests/resize_formats_ref.py, which
tests/test_resize_formats_plan.py pins to PIL on the CPU.  Shapes are the smallest at which the new kernels can still go wrong."""
import numpy as np
import pytest
import torch

import resize_formats_ref as F
from conftest import GOLDEN, load_synthetic

pytestmark = pytest.mark.gpu

PIX = {"rgb": 0, "bgr": 1, "l": 2, "rgba": 3, "bgra": 4}
FORMS = [("l", 3), ("l", 1), ("rgba", 3), ("bgra", 3)]                       # (pixel_format, out_channels)
FORM_IDS = ["l3", "l1", "rgba", "bgra"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "resize_formats" / "pil_formats.npz", allow_pickle=False)


def _input(fmt, seed, n, ih, iw):
    """Noise in the layout of `fmt` (all four bytes of a 4-byte pixel are noise: an alpha that entered a sum would show)."""
    shape = (n, ih, iw) if fmt == "l" else (n, ih, iw, 4)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _want(fmt, oc, x, oh, ow):
    if fmt == "l":
        return np.stack([F.l_ref(f, oh, ow, oc) for f in x])
    return np.stack([F.rgba_ref(f, oh, ow, bgra=fmt == "bgra") for f in x])


def _check(vad, fmt, oc, x, oh, ow, label=None):
    got = vad.scoring.resize_frames(torch.from_numpy(x).cuda(), (oh, ow), pixel_format=fmt, out_channels=oc)
    want = torch.from_numpy(_want(fmt, oc, x, oh, ow))
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == tuple(want.shape), (label, fmt, oc, got.shape)
    assert torch.equal(got.cpu(), want), (label, fmt, oc, x.shape, oh, ow)
    return got


@pytest.mark.parametrize("name", F.NAMES)
def test_fixture_cases_equal_pil(vad, fixture, name):
    """l -> 3 channels, l -> 1, rgba and (on the B/R-flipped input) bgra against PIL's stored bytes."""
    _, _, _, oh, ow = F.geometry(name)
    plane = torch.from_numpy(fixture["l_" + name]).cuda()
    rgb = torch.from_numpy(fixture["rgba_" + name]).cuda()
    g, a = torch.from_numpy(F.mono_input(name)).cuda(), F.rgba_input(name)
    S = vad.scoring
    before = vad.hip.calls.get("resize_u8", 0)
    got = S.FrameResizer((oh, ow), pixel_format="l")(g)
    assert vad.hip.calls["resize_u8"] == before + 1
    assert got.dtype == torch.uint8 and torch.equal(got, plane[..., None].expand(-1, -1, -1, 3))
    assert torch.equal(S.FrameResizer((oh, ow), pixel_format="l", out_channels=1)(g), plane[..., None])
    assert torch.equal(S.resize_frames(torch.from_numpy(a).cuda(), (oh, ow), pixel_format="rgba"), rgb)
    assert torch.equal(S.resize_frames(torch.from_numpy(F.swap_br(a)).cuda(), (oh, ow), pixel_format="bgra"), rgb)


def test_three_byte_formats_by_name_are_the_existing_path(vad):
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 45, 64, 3), dtype=np.uint8)).cuda()
    S = vad.scoring
    for size in [(32, 48), (45, 48), (32, 64), (45, 64)]:
        assert torch.equal(S.resize_frames(x, size, pixel_format="rgb"), S.resize_frames(x, size))
        assert torch.equal(S.resize_frames(x, size, pixel_format="bgr"), S.resize_frames(x, size, channel_order="bgr"))


def test_phase_and_trimming_of_odd_mono_frames(vad):
    """37 x 53 one-byte frames: odd row and frame byte counts, so every row and every frame base has another phase; the first
    and last staging vectors are trimmed to the tensor - also when the tensor is a slice that starts inside an allocation."""
    x = _input("l", 20, 3, 37, 53)
    for oc in (3, 1):
        whole = _check(vad, "l", oc, x, 32, 48)
        dev = torch.from_numpy(x).cuda()
        rz = vad.scoring.FrameResizer((32, 48), pixel_format="l", out_channels=oc)
        assert torch.equal(rz(dev[1:]), whole[1:])
        assert torch.equal(rz(dev[2]), whole[2])                                     # no leading axis at all
        y = torch.from_numpy(_input("l", 21, 6, 37, 53)).cuda()
        assert torch.equal(rz(y.view(2, 3, 37, 53)), rz(y).view(2, 3, 32, 48, oc))   # [B, T, H, W]
        assert rz(dev[:0]).shape == (0, 32, 48, oc)
    a = _input("rgba", 22, 3, 37, 53)
    whole = _check(vad, "rgba", 3, a, 32, 48)
    assert torch.equal(vad.scoring.resize_frames(torch.from_numpy(a).cuda()[1:], (32, 48), pixel_format="rgba"), whole[1:])
    # a source that is not 4-byte aligned: one byte into an allocation (the staged range and the vertical 4 -> 3 loads carry it)
    for size in [(32, 48), (32, 53)]:
        buf = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(a).cuda().flatten()
        want = torch.from_numpy(_want("rgba", 3, a, *size)).cuda()
        assert torch.equal(vad.scoring.resize_frames(buf[1:].view(3, 37, 53, 4), size, pixel_format="rgba"), want), size


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_narrow_widths(vad, form):
    """Widths 1, 2, 3, 5: fewer input pixels than a tap group, taps clipped at the row end."""
    fmt, oc = form
    for iw in (1, 2, 3, 5):
        _check(vad, fmt, oc, _input(fmt, 30 + iw, 2, 9, iw), 12, 8, "up")
        _check(vad, fmt, oc, _input(fmt, 40 + iw, 2, 9, 37), 6, iw, "down to a narrow row")
    _check(vad, fmt, oc, _input(fmt, 50, 1, 250, 7), 16, 48, "250x7")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_tap_counts(vad, form):
    """At most 4 taps (up-scaling: one tap group), 5 and more (zero-padded groups), and many (a 40-fold reduction)."""
    fmt, oc = form
    _check(vad, fmt, oc, _input(fmt, 60, 2, 20, 30), 64, 96, "up")
    _check(vad, fmt, oc, _input(fmt, 61, 2, 70, 111), 28, 37, "5-6 taps")
    _check(vad, fmt, oc, _input(fmt, 62, 1, 200, 1283), 16, 32, "81 taps, more than one block per frame")


def test_widest_four_byte_row(vad):
    """16384 four-byte pixels: one staged row is 64 KB, above the default dynamic-LDS limit."""
    for fmt in ("rgba", "bgra"):
        _check(vad, fmt, 3, _input(fmt, 63, 1, 2, 16384), 2, 256, "in_w 16384")
    _check(vad, "l", 3, _input("l", 64, 1, 2, 16384), 3, 256, "in_w 16384")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_vertical_forms_and_skipped_passes(vad, form):
    """out_w a multiple of 4 (dword form) and not (byte form), with both passes, horizontal only, vertical only (for the 4-byte
    formats the 4 -> 3 vertical kernel) and the copy (replicated / alpha-stripped / swapped)."""
    fmt, oc = form
    for ow in (48, 50, 4, 1):
        _check(vad, fmt, oc, _input(fmt, 70 + ow, 2, 45, 64), 32, ow, "both")
        _check(vad, fmt, oc, _input(fmt, 80 + ow, 2, 32, 64), 32, ow, "horizontal only")
        _check(vad, fmt, oc, _input(fmt, 90 + ow, 2, 45, ow), 32, ow, "vertical only")
        _check(vad, fmt, oc, _input(fmt, 100 + ow, 2, 70, ow), 90, ow, "vertical only, up")
        _check(vad, fmt, oc, _input(fmt, 110 + ow, 2, 33, ow), 33, ow, "copy")


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_constant_frames_stay_constant(vad, form):
    fmt, oc = form
    for ih, iw, oh, ow in [(37, 53, 32, 48), (100, 180, 128, 128), (64, 777, 64, 128), (1000, 64, 128, 64), (64, 64, 64, 64), (1024, 100, 16, 256)]:
        for value in (0, 1, 127, 255):
            shape = (1, ih, iw) if fmt == "l" else (1, ih, iw, 4)
            c = torch.full(shape, value, dtype=torch.uint8, device="cuda")
            if fmt != "l":
                c[..., 3] = 255 - value                                              # an alpha that must not leak
            out = vad.scoring.resize_frames(c, (oh, ow), pixel_format=fmt, out_channels=oc)
            assert out.shape == (1, oh, ow, oc) and bool((out == value).all()), (ih, iw, oh, ow, value)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("geo", [(90, 160, 32, 48), (45, 64, 45, 31), (70, 31, 20, 31)])
def test_batch_independence(vad, form, geo):
    fmt, oc = form
    ih, iw, oh, ow = geo
    rz = vad.scoring.FrameResizer((oh, ow), pixel_format=fmt, out_channels=oc)
    x = torch.from_numpy(_input(fmt, 3, 9, ih, iw)).cuda()
    alone = torch.stack([rz(x[i:i + 1])[0] for i in range(9)])
    for n in (1, 3, 9):
        assert torch.equal(rz(x[:n]), alone[:n])
    assert torch.equal(rz(x[2:7]), alone[2:7])


def test_one_resizer_serves_several_geometries(vad):
    """One object, two input geometries in turn (one with a workspace, one without): a plan per geometry, the results unchanged."""
    for fmt, oc in FORMS:
        a, b = _input(fmt, 6, 3, 120, 200), _input(fmt, 7, 2, 77, 48)
        want_a, want_b = torch.from_numpy(_want(fmt, oc, a, 32, 48)).cuda(), torch.from_numpy(_want(fmt, oc, b, 32, 48)).cuda()
        rz = vad.scoring.FrameResizer((32, 48), pixel_format=fmt, out_channels=oc)
        a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for _ in range(2):
            assert torch.equal(rz(a), want_a) and torch.equal(rz(b), want_b), (fmt, oc)
        assert len(rz._plans) == 2
        out = torch.empty_like(want_a)
        assert rz(a, out=out) is out and torch.equal(out, want_a)
        with pytest.raises(vad.hip.VadError, match="out must be"):
            rz(a, out=torch.empty(3, 32, 48, oc + 1, dtype=torch.uint8, device="cuda"))


def _plan(vad, ih, iw, oh, ow):
    lib = vad.hip.lib()
    blob = np.empty(lib.vad_resize_plan_bytes(ih, iw, oh, ow) // 4, np.int32)
    vad.hip.check(lib.vad_resize_plan(ih, iw, oh, ow, blob.ctypes.data))
    return torch.from_numpy(blob).cuda()


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("geo", [(96, 128, 32, 32), (96, 32, 32, 32), (32, 128, 32, 32), (32, 32, 32, 32)])      # both, vertical, horizontal, copy
def test_plan_of_another_geometry_never_yields_pixels(vad, form, geo):
    """The C ABI's guard: every new kernel compares the plan header with the call's sizes on the device and writes zeros."""
    fmt, oc = form
    lib = vad.hip.lib()
    ih, iw, oh, ow = geo
    x = torch.from_numpy(_input(fmt, 5, 2, ih, iw)).cuda().clamp(min=1)
    need = lib.vad_resize_workspace_bytes_f(2, ih, iw, oh, ow, PIX[fmt], oc)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    right = vad.scoring.resize_frames(x, (oh, ow), pixel_format=fmt, out_channels=oc)
    plans = [_plan(vad, ih, iw, oh, ow), _plan(vad, iw, ih, oh, ow) if ih != iw else _plan(vad, ih + 1, iw, oh, ow), _plan(vad, ih, iw, oh, ow + 16),
             torch.zeros(4096, dtype=torch.int32, device="cuda")]
    for p in plans:
        out = torch.full((2, oh, ow, oc), 9, dtype=torch.uint8, device="cuda")
        vad.hip.check(lib.vad_resize_u8_f(x.data_ptr(), 2, ih, iw, PIX[fmt], p.data_ptr(), out.data_ptr(), oh, ow, oc, ws.data_ptr(), need,
                                          vad.hip.current_stream()))
        if p[2:6].tolist() == [ih, iw, oh, ow]:
            assert torch.equal(out, right) and bool((out > 0).all())
        else:
            assert not bool(out.any())


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("geo", [(45, 64, 32, 48), (45, 64, 32, 50), (45, 48, 32, 48), (32, 64, 32, 48)])
def test_workspace_contract(vad, form, geo):
    """Exactly the reported size, between guards, whatever it holds on entry (hip_helpers' arenas, as tests/test_hip_workspace.py)."""
    import hip_helpers as H
    fmt, oc = form
    lib = vad.hip.lib()
    ih, iw, oh, ow = geo
    n = 2
    x = torch.from_numpy(_input(fmt, ih + iw, n, ih, iw)).cuda()
    plain = vad.scoring.resize_frames(x, (oh, ow), pixel_format=fmt, out_channels=oc)
    plan = _plan(vad, ih, iw, oh, ow)
    need = lib.vad_resize_workspace_bytes_f(n, ih, iw, oh, ow, PIX[fmt], oc)
    assert (need > 0) == (ih != oh and iw != ow)
    for fill in H.POISONS:
        arena = H.GuardedArena(need, fill)
        dst = H.GuardedArena(plain.numel(), 0xA5)
        vad.hip.check(lib.vad_resize_u8_f(x.data_ptr(), n, ih, iw, PIX[fmt], plan.data_ptr(), dst.ptr(), oh, ow, oc, arena.ptr(), need, H.stream()))
        arena.check("vad_resize_u8_f workspace")
        dst.check("vad_resize_u8_f dst")
        assert torch.equal(dst.body.view(plain.shape), plain), f"resize {fmt} {geo}: the result depends on the workspace (fill 0x{fill:02X})"
    if need:
        arena = H.GuardedArena(need, 0x7F)
        dst = torch.full_like(plain, 0xA5)
        rc = lib.vad_resize_u8_f(x.data_ptr(), n, ih, iw, PIX[fmt], plan.data_ptr(), dst.data_ptr(), oh, ow, oc, arena.ptr(), need - 1, H.stream())
        assert rc == -3 and b"workspace" in lib.vad_last_error()
        assert arena.still_poison() and bool((dst == 0xA5).all())                    # refused: nothing was launched


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
def test_raw_scores_equal_the_rgb_path_on_converted_frames(vad, precision):
    """Grey and RGBA frames score bit for bit as the frames `convert('RGB')` makes of them score on the existing RGB path."""
    S = vad.scoring
    g = torch.from_numpy(F.mono_input("240p_64_x6")).cuda()                          # six 240 x 320 one-byte frames
    g_rgb = g[..., None].expand(-1, -1, -1, 3).contiguous()
    a = torch.from_numpy(F.rgba_input("240p_64_x6")).cuda()
    a_rgb = a[..., :3].contiguous()
    img = _img_model(vad, precision)
    n0 = vad.hip.calls["img_score"]
    assert torch.equal(S.score_raw_images(img, g, image_size=64, pixel_format="l"), S.score_raw_images(img, g_rgb, image_size=64))
    assert torch.equal(S.score_raw_images(img, g, image_size=64, pixel_format="l", per_pixel=True),
                       S.score_raw_images(img, g_rgb, image_size=64, per_pixel=True))
    assert torch.equal(S.score_raw_images(img, a, image_size=64, pixel_format="rgba"), S.score_raw_images(img, a_rgb, image_size=64))
    assert torch.equal(S.score_raw_images(img, a[..., [2, 1, 0, 3]].contiguous(), image_size=64, pixel_format="bgra"),
                       S.score_raw_images(img, a_rgb, image_size=64))
    assert vad.hip.calls["img_score"] == n0 + 8
    vid = _vid_model(vad, precision)
    for raw, rgb, fmt in ((g.view(2, 3, 240, 320), g_rgb.view(2, 3, 240, 320, 3), "l"), (a.view(2, 3, 240, 320, 4), a_rgb.view(2, 3, 240, 320, 3), "rgba")):
        assert torch.equal(S.score_raw_clips(vid, raw, image_size=64, pixel_format=fmt), S.score_raw_clips(vid, rgb, image_size=64))
        assert torch.equal(S.score_raw_clips(vid, raw, image_size=(64, 64), per_frame=True, pixel_format=fmt),
                           S.score_raw_clips(vid, rgb, image_size=(64, 64), per_frame=True))
    # one live stream fed a raw grey frame at a time, against the replicated frames fed the existing way
    s_l, st_l = S.score_frames_stateful(vid, (g[i:i + 1] for i in range(6)), batch=1, image_size=64, pixel_format="l")
    s_rgb, st_rgb = S.score_frames_stateful(vid, (g_rgb[i:i + 1] for i in range(6)), batch=1, image_size=64)
    assert s_l.shape == (1, 6) and np.array_equal(s_l, s_rgb) and torch.equal(st_l.blob, st_rgb.blob)
    s_cpu, st_cpu = S.score_frames_stateful(vid, (g[i:i + 1].cpu().numpy() for i in range(6)), batch=1, device="cuda", image_size=64,
                                            pixel_format="l")
    assert np.array_equal(s_cpu, s_rgb) and torch.equal(st_cpu.blob, st_rgb.blob)


def test_masks_equal_pil_resize_and_totensor(vad, fixture):
    """`resize_masks` = the reference's mask_transform: PIL's L resize, then ToTensor's `/ 255`, as float32 [..., 1, h, w]."""
    for name in ("odd_37x53", "240p_64_x6", "copy_64"):
        _, _, _, oh, ow = F.geometry(name)
        got = vad.scoring.resize_masks(torch.from_numpy(F.mono_input(name)).cuda(), (oh, ow))
        want = torch.from_numpy(fixture["l_" + name]).to(torch.float32).div(255)[:, None]
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got.cpu(), want), name
    # a 0 / 255 mask (a disc) stays within 0 .. 255, i.e. [0, 1], and keeps both values where it is flat
    y, x = np.mgrid[:200, :300]
    mask = (((y - 90) ** 2 + (x - 140) ** 2 < 60 ** 2) * 255).astype(np.uint8)
    got = vad.scoring.resize_masks(torch.from_numpy(mask).cuda(), 64)
    assert got.shape == (1, 64, 64) and float(got.min()) == 0.0 and float(got.max()) == 1.0
    assert torch.equal(got.cpu(), torch.from_numpy(F.plane_ref(mask, 64, 64)).to(torch.float32).div(255)[None])
    assert 0.0 < float(got.mean()) < 1.0 and bool(((got > 0) & (got < 1)).any())     # the antialiased edge is in between


def test_python_refusals(vad):
    S = vad.scoring
    grey = torch.zeros(2, 48, 64, dtype=torch.uint8, device="cuda")
    four = torch.zeros(2, 48, 64, 4, dtype=torch.uint8, device="cuda")
    three = torch.zeros(2, 48, 64, 3, dtype=torch.uint8, device="cuda")
    for fmt in ("rgba", "bgra"):
        with pytest.raises(vad.hip.VadError, match=r"\[\.\.\., H, W, 4\]"):
            S.resize_frames(three, 32, pixel_format=fmt)
        with pytest.raises(vad.hip.VadError, match="out_channels"):
            S.resize_frames(four, 32, pixel_format=fmt, out_channels=1)
    for fmt in ("rgb", "bgr", None):
        with pytest.raises(vad.hip.VadError, match=r"\[\.\.\., H, W, 3\]"):
            S.resize_frames(four, 32, pixel_format=fmt)
        with pytest.raises(vad.hip.VadError, match="out_channels"):
            S.resize_frames(three, 32, pixel_format=fmt, out_channels=1)
    with pytest.raises(vad.hip.VadError, match=r"\[\.\.\., H, W\]"):
        S.resize_frames(grey[0, 0], 32, pixel_format="l")                            # one axis: no H
    with pytest.raises(vad.hip.VadError, match="uint8"):
        S.resize_frames(grey.float(), 32, pixel_format="l")
    with pytest.raises(vad.hip.VadError, match="contiguous"):
        S.resize_frames(grey[:, ::2], 32, pixel_format="l")
    with pytest.raises(vad.hip.VadError, match="GPU tensor"):
        S.resize_masks(grey.cpu(), 32)
    with pytest.raises(vad.hip.VadError, match="not both"):
        S.resize_frames(four, 32, channel_order="bgr", pixel_format="rgba")
    with pytest.raises(vad.hip.VadError, match="unsupported geometry"):
        S.resize_frames(torch.zeros(1, 130, 8, dtype=torch.uint8, device="cuda"), (2, 8), pixel_format="l")       # 65-fold
    # a 3-channel tensor taken as grey frames is [..., H, W] = [.., 64, 3]: legal, so the models refuse what comes out, not this
    assert S.resize_frames(three, (4, 3), pixel_format="l").shape == (2, 48, 4, 3, 3)
    vid = _vid_model(vad, "fp32")
    with pytest.raises(vad.hip.VadError, match="uint8"):
        S.score_frames_stateful(vid, [grey.float()], batch=2, image_size=32, pixel_format="l")
