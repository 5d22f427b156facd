"""CPU checks of the device Resize's other pixel formats (vad_resize_u8_f: one-byte `l`, four-byte `rgba` / `bgra`): what the
device is held to (tests/resize_formats_ref.py, built on the restatement tests/resize_ref.py) against PIL's stored and live
output of `convert('RGB')` / `convert('L')` followed by the resize, and the new entry point's host-side refusals and workspace
sizes.  No GPU needed: the library loads without one."""
import numpy as np
import pytest

import resize_formats_ref as F
import resize_ref as R
from conftest import GOLDEN

FIXTURE = GOLDEN / "resize_formats" / "pil_formats.npz"
PIX = {"rgb": 0, "bgr": 1, "l": 2, "rgba": 3, "bgra": 4}     # include/vad_hip.h VAD_PIX_*


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE, allow_pickle=False)


def test_fixture_lists_the_cases(fixture):
    assert list(fixture["names"]) == list(F.NAMES) and str(fixture["pil_version"])
    assert fixture["table"].tolist() == [list(F.geometry(name)) for name in F.NAMES]
    for name in F.NAMES:
        n, _, _, oh, ow = F.geometry(name)
        assert fixture["l_" + name].shape == (n, oh, ow) and fixture["l_" + name].dtype == np.uint8
        assert fixture["rgba_" + name].shape == (n, oh, ow, 3) and fixture["rgba_" + name].dtype == np.uint8
    assert FIXTURE.stat().st_size < 1 << 20
    assert (GOLDEN / "resize_formats" / "make_golden_resize_formats.py").exists()


@pytest.mark.parametrize("name", F.NAMES)
def test_restatement_reproduces_stored_pil_output(fixture, name):
    """Pins what the device is compared with to PIL's `convert` + `resize`, byte for byte."""
    n, _, _, oh, ow = F.geometry(name)
    g, a = F.mono_input(name), F.rgba_input(name)
    for i in range(n):
        assert np.array_equal(F.plane_ref(g[i], oh, ow), fixture["l_" + name][i]), (name, i)
        assert np.array_equal(F.rgba_ref(a[i], oh, ow), fixture["rgba_" + name][i]), (name, i)
        assert np.array_equal(F.rgba_ref(F.swap_br(a[i]), oh, ow, bgra=True), fixture["rgba_" + name][i]), (name, i)


def _live_pil_case(Image, rng, ih, iw, oh, ow):
    g = rng.integers(0, 256, (ih, iw), dtype=np.uint8)
    a = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    plane = np.asarray(Image.fromarray(g, "L").resize((ow, oh), Image.BILINEAR))
    as_rgb = np.asarray(Image.fromarray(g, "L").convert("RGB").resize((ow, oh), Image.BILINEAR))
    stripped = np.asarray(Image.fromarray(a, "RGBA").convert("RGB").resize((ow, oh), Image.BILINEAR))
    geo = (ih, iw, oh, ow)
    assert np.array_equal(F.l_ref(g, oh, ow, 1)[..., 0], plane), geo
    assert np.array_equal(F.l_ref(g, oh, ow, 3), as_rgb), geo
    assert np.array_equal(F.rgba_ref(a, oh, ow), stripped), geo
    assert np.array_equal(F.rgba_ref(F.swap_br(a), oh, ow, bgra=True), stripped), geo


def test_restatement_matches_live_pil_on_fixture_geometries():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(31)
    for name in F.NAMES:
        _live_pil_case(Image, rng, *F.geometry(name)[1:])


def test_restatement_matches_live_pil_on_random_geometries():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2025)
    for geo in R.random_geometries(12, 100):
        _live_pil_case(Image, rng, *geo)


def test_workspace_sizes(vad):
    lib = vad.hip.lib()
    both, rows = (2, 1080, 1920, 256, 256), 1080
    assert lib.vad_resize_workspace_bytes(*both) == 2 * rows * 256 * 3
    for fmt in ("rgb", "bgr", "rgba", "bgra"):                    # the intermediate is 3-byte pixels in output order
        assert lib.vad_resize_workspace_bytes_f(*both, PIX[fmt], 3) == 2 * rows * 256 * 3, fmt
    for oc in (1, 3):                                             # one byte per pixel: the value is replicated on the last store
        assert lib.vad_resize_workspace_bytes_f(*both, PIX["l"], oc) == 2 * rows * 256
    lo, count, _ = R.plan_axis(100, 128)                          # up-scaling: exactly the rows the vertical pass reads
    need = int((lo + count).max()) - int(lo.min())
    assert lib.vad_resize_workspace_bytes_f(3, 100, 180, 128, 128, PIX["l"], 1) == 3 * need * 128
    assert lib.vad_resize_workspace_bytes_f(3, 100, 180, 128, 128, PIX["rgba"], 3) == 3 * need * 128 * 3
    for fmt in PIX.values():                                      # at most one pass, and the copy: it writes dst directly
        for geo in [(64, 777, 64, 128), (1000, 64, 128, 64), (64, 64, 64, 64)]:
            assert lib.vad_resize_workspace_bytes_f(2, *geo, fmt, 3) == 0
    # what the launcher refuses has no size
    assert lib.vad_resize_workspace_bytes_f(-1, 64, 64, 32, 32, PIX["l"], 3) == 0
    assert lib.vad_resize_workspace_bytes_f(1, 64 * 32 + 1, 64, 32, 32, PIX["l"], 3) == 0
    for fmt, oc in [(5, 3), (-1, 3), (PIX["l"], 0), (PIX["l"], 2), (PIX["l"], 4), (PIX["rgb"], 1), (PIX["bgr"], 1), (PIX["rgba"], 1),
                    (PIX["bgra"], 1), (PIX["rgba"], 4)]:
        assert lib.vad_resize_workspace_bytes_f(2, 1080, 1920, 256, 256, fmt, oc) == 0, (fmt, oc)


def test_refusals_before_any_launch(vad):
    """Argument errors of the launcher are raised before anything touches a device (this runs without one)."""
    lib = vad.hip.lib()
    keep = np.zeros(16, np.int32)
    one = keep.ctypes.data

    def call(fmt, oc, src=one, n=1, ih=64, iw=64, plan=one, dst=one, ws=None, ws_bytes=0):
        return lib.vad_resize_u8_f(src, n, ih, iw, fmt, plan, dst, 32, 32, oc, ws, ws_bytes, None)
    for fmt in (5, -1, 255):
        assert call(fmt, 3) == -1 and b"pixel_format" in lib.vad_last_error(), fmt
    for fmt, oc in [(PIX["l"], 0), (PIX["l"], 2), (PIX["l"], 4), (PIX["rgb"], 1), (PIX["bgr"], 1), (PIX["rgba"], 1), (PIX["bgra"], 1),
                    (PIX["rgba"], 4)]:
        assert call(fmt, oc) == -1 and b"out_channels" in lib.vad_last_error(), (fmt, oc)
    for fmt in PIX.values():
        assert call(fmt, 3, src=None, plan=None, dst=None) == -1 and b"null" in lib.vad_last_error(), fmt
        assert call(fmt, 3, n=-1) == -1 and b"negative" in lib.vad_last_error(), fmt
        assert call(fmt, 3, ih=64 * 32 + 1) == -1 and b"unsupported geometry" in lib.vad_last_error(), fmt
        assert call(fmt, 3, plan=one + 4) == -1 and b"16-B aligned" in lib.vad_last_error(), fmt
        assert call(fmt, 3) == -3 and b"workspace" in lib.vad_last_error(), fmt          # both passes and no workspace at all
        need = lib.vad_resize_workspace_bytes_f(1, 64, 64, 32, 32, fmt, 3)
        assert need > 1
        assert call(fmt, 3, ws=one, ws_bytes=need - 1) == -3 and b"workspace" in lib.vad_last_error(), fmt     # one byte short
    assert call(PIX["l"], 1, ws=one, ws_bytes=lib.vad_resize_workspace_bytes_f(1, 64, 64, 32, 32, PIX["l"], 1) - 1) == -3
    # the old entry point keeps its own refusal: a format code is not a channel order
    assert lib.vad_resize_u8(one, 1, 64, 64, 2, one, one, 32, 32, None, 0, None) == -1 and b"channel_order" in lib.vad_last_error()


def test_python_arguments_without_a_device(vad):
    S = vad.scoring
    with pytest.raises(vad.hip.VadError, match="pixel_format"):
        S.FrameResizer(32, pixel_format="yuv")
    with pytest.raises(vad.hip.VadError, match="not both"):
        S.FrameResizer(32, channel_order="bgr", pixel_format="rgba")
    for fmt in (None, "rgb", "bgr", "rgba", "bgra"):
        with pytest.raises(vad.hip.VadError, match="out_channels"):
            S.FrameResizer(32, pixel_format=fmt, out_channels=1)
    with pytest.raises(vad.hip.VadError, match="out_channels"):
        S.FrameResizer(32, pixel_format="l", out_channels=2)
    with pytest.raises(vad.hip.VadError, match="channel_order"):
        S.FrameResizer(32, channel_order="grb")
    rz = S.FrameResizer((32, 48), pixel_format="l", out_channels=1)
    assert (rz.out_h, rz.out_w, rz.pixel_format, rz.out_channels) == (32, 48, "l", 1)
    assert S.FrameResizer(32, channel_order="rgb", pixel_format="bgra").pixel_format == "bgra"      # the default order is no conflict
    assert {k: v[0] for k, v in S.PIXEL_FORMATS.items()} == PIX
