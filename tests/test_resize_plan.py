"""CPU checks of the device Resize: the numpy restatement (tests/resize_ref.py) against PIL's stored and live output, and the
host planner `vad_resize_plan` (csrc/pack.cpp) against the restatement, integer for integer.  No GPU needed: the library
loads without one."""
import numpy as np
import pytest

import resize_ref as R
from conftest import GOLDEN

PLAN_HEADER_WORDS = 16
MAGIC = 0x52444156      # "VADR"


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN / "resize" / "pil_bilinear.npz", allow_pickle=False)


def test_fixture_lists_the_cases_of_the_restatement(fixture):
    assert list(fixture["names"]) == list(R.CASES)
    table = [[seed, n, ih, iw, oh, ow] for _, seed, n, ih, iw, oh, ow in R.CASES.values()]
    assert fixture["table"].tolist() == table and str(fixture["pil_version"])
    for name, (_, _, n, _, _, oh, ow) in R.CASES.items():
        assert fixture["out_" + name].shape == (n, oh, ow, 3) and fixture["out_" + name].dtype == np.uint8
    assert (GOLDEN / "resize" / "pil_bilinear.npz").stat().st_size < 1 << 20
    assert (GOLDEN / "resize" / "make_golden_resize.py").exists()


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_stored_pil_output(fixture, name):
    """Pins the restatement - and with it everything tested against it - to PIL, byte for byte."""
    x = R.case_input(name)
    _, _, n, _, _, oh, ow = R.CASES[name]
    for i in range(n):
        assert np.array_equal(R.resize_ref(x[i], oh, ow), fixture["out_" + name][i]), (name, i)


def test_restatement_matches_live_pil_on_random_geometries():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(2024)
    for ih, iw, oh, ow in R.random_geometries(11, 100):
        x = rng.integers(0, 256, (ih, iw, 3), dtype=np.uint8)
        pil = np.asarray(Image.fromarray(x, "RGB").resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(R.resize_ref(x, oh, ow), pil), (ih, iw, oh, ow)


def _plan(vad, ih, iw, oh, ow) -> np.ndarray:
    lib = vad.hip.lib()
    nbytes = lib.vad_resize_plan_bytes(ih, iw, oh, ow)
    assert nbytes >= PLAN_HEADER_WORDS * 4 and nbytes % 4 == 0
    blob = np.full(nbytes // 4, -7, np.int32)
    vad.hip.check(lib.vad_resize_plan(ih, iw, oh, ow, blob.ctypes.data), "vad_resize_plan")
    return blob


def _check_axis(blob, off, kpad, n_in, n_out):
    if n_in == n_out:
        assert off == 0 and kpad == 0
        return
    lo, count, weights = R.plan_axis(n_in, n_out)
    assert kpad == (int(count.max()) + 3) // 4 * 4 and off >= PLAN_HEADER_WORDS
    assert np.array_equal(blob[off:off + n_out], lo) and np.array_equal(blob[off + n_out:off + 2 * n_out], count)
    w0 = off + (2 * n_out + 3) // 4 * 4
    table = blob[w0:w0 + kpad * n_out].reshape(kpad // 4, n_out, 4).transpose(1, 0, 2).reshape(n_out, kpad)     # [o][tap]
    for o in range(n_out):
        assert np.array_equal(table[o, :count[o]], weights[o]), (n_in, n_out, o)
        assert not table[o, count[o]:].any()


def test_planner_matches_restatement_on_fixture_geometries(vad):
    for name, (_, _, _, ih, iw, oh, ow) in R.CASES.items():
        blob = _plan(vad, ih, iw, oh, ow)
        hdr = blob[:PLAN_HEADER_WORDS]
        assert int(hdr[0]) == MAGIC and int(hdr[1]) >> 16 == vad.hip.ABI_VERSION and hdr[2:6].tolist() == [ih, iw, oh, ow]
        assert int(hdr[12]) == blob.size and not (blob == -7).any()
        _check_axis(blob, int(hdr[8]), int(hdr[6]), iw, ow)
        _check_axis(blob, int(hdr[9]), int(hdr[7]), ih, oh)
        if ih != oh:                                      # rows the vertical pass reads = rows the horizontal pass produces
            lo, count, _ = R.plan_axis(ih, oh)
            assert int(hdr[10]) == int(lo.min()) and int(hdr[10]) + int(hdr[11]) == int((lo + count).max())
        else:
            assert hdr[10:12].tolist() == [0, ih]


def test_planner_matches_restatement_on_random_axes(vad):
    rng = np.random.default_rng(7)
    pairs = [(16384, 256), (4096, 4096 - 1), (1, 4096), (4096, 64), (1, 1 + 1)]
    while len(pairs) < 200:
        n_in = int(rng.integers(1, R.MAX_IN + 1)) if rng.random() < 0.3 else int(rng.integers(1, 2000))
        n_out = int(rng.integers(max(1, -(-n_in // R.MAX_RATIO)), min(R.MAX_OUT, 4 * n_in + 64) + 1))
        if n_in != n_out:
            pairs.append((n_in, n_out))
    for i, (n_in, n_out) in enumerate(pairs):
        if i % 2:                                          # the axis under test alternates between horizontal and vertical
            blob = _plan(vad, 8, n_in, 8, n_out)
            _check_axis(blob, int(blob[8]), int(blob[6]), n_in, n_out)
        else:
            blob = _plan(vad, n_in, 8, n_out, 8)
            _check_axis(blob, int(blob[9]), int(blob[7]), n_in, n_out)


def test_unsupported_geometries_are_refused(vad):
    lib = vad.hip.lib()
    buf = np.zeros(1 << 16, np.int32)
    bad = [(0, 64, 64, 64), (64, 0, 64, 64), (64, 64, 0, 64), (64, 64, 64, 0), (-1, 64, 64, 64), (16385, 64, 256, 64), (64, 16385, 64, 256),
           (64, 64, 4097, 64), (64, 64, 64, 4097), (64 * 100 + 1, 64, 100, 64), (64, 64 * 7 + 1, 64, 7), (16384, 64, 255, 64)]
    for geo in bad:
        assert lib.vad_resize_plan_bytes(*geo) == 0, geo
        assert lib.vad_resize_plan(*geo, buf.ctypes.data) == -1, geo
        assert b"unsupported geometry" in lib.vad_last_error(), geo
        assert lib.vad_resize_workspace_bytes(1, *geo) == 0
        assert not R.supported(*geo)
    for geo in [(16384, 16384, 256, 256), (6400, 64, 100, 64), (1, 1, 4096, 4096), (64, 64, 64, 64)]:
        assert R.supported(*geo) and lib.vad_resize_plan_bytes(*geo) >= PLAN_HEADER_WORDS * 4, geo
    blob = _plan(vad, 16384, 4, 256, 4)                    # the size corner is accepted
    assert blob[2:6].tolist() == [16384, 4, 256, 4] and int(blob[7]) == (int(R.plan_axis(16384, 256)[1].max()) + 3) // 4 * 4 >= 128 and int(blob[6]) == 0
    assert lib.vad_resize_plan(64, 64, 32, 32, None) == -1 and b"null" in lib.vad_last_error()
    # workspace: the horizontal pass's rows, nothing when at most one axis changes
    assert lib.vad_resize_workspace_bytes(2, 1080, 1920, 256, 256) == 2 * 1080 * 256 * 3
    assert lib.vad_resize_workspace_bytes(2, 64, 777, 64, 128) == 0 and lib.vad_resize_workspace_bytes(-1, 64, 64, 32, 32) == 0
    # argument errors of the launcher are raised before anything touches a device
    assert lib.vad_resize_u8(None, 1, 64, 64, 0, None, None, 32, 32, None, 0, None) == -1 and b"null" in lib.vad_last_error()
    keep = np.zeros(16, np.int32)
    one = keep.ctypes.data
    assert lib.vad_resize_u8(one, -1, 64, 64, 0, one, one, 32, 32, None, 0, None) == -1 and b"negative" in lib.vad_last_error()
    assert lib.vad_resize_u8(one, 1, 64, 64, 2, one, one, 32, 32, None, 0, None) == -1 and b"channel_order" in lib.vad_last_error()
    assert lib.vad_resize_u8(one, 1, 64 * 32 + 1, 64, 0, one, one, 32, 32, None, 0, None) == -1 and b"unsupported geometry" in lib.vad_last_error()
    assert lib.vad_resize_u8(one, 1, 64, 64, 0, one, one, 32, 32, None, 0, None) == -3 and b"workspace" in lib.vad_last_error()
