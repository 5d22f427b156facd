"""CPU checks of the Gaussian map smoothing: the host taps against scipy's impulse response, the numpy
restatement (tests/map_smooth_ref.py - what the GPU tests compare the kernel with, bit for bit) against scipy's float64 results
within the derived rounding bound, and every refusal that needs no device.  scipy's numbers come from
tests/golden/smooth/scipy_gaussian.npz (make_golden_smooth.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_smooth_ref as ref

GOLDEN = "smooth/scipy_gaussian.npz"


@pytest.mark.parametrize("sigma,truncate", [(0.5, 4.0), (1.0, 4.0), (2.0, 4.0), (4.0, 4.0), (8.0, 4.0), (2.0, 3.0), (4.0, 3.0)])
def test_taps_are_scipys(vad, golden, sigma, truncate):
    want = golden(GOLDEN)[f"taps_{sigma}_{truncate}"]
    r, w = vad.metrics.gaussian_taps(sigma, truncate)
    assert r == int(truncate * sigma + 0.5) and w.dtype == np.float32 and w.shape == want.shape == (2 * r + 1,)
    w64 = vad.metrics._gaussian_taps64(sigma, r)
    assert np.abs(w64 - want).max() <= 1e-15
    assert np.array_equal(w, want.astype(np.float32))                       # rounded once: the float32 of scipy's float64 taps
    assert (w > 0).all() and np.array_equal(w, w[::-1])
    r2, w2 = ref.taps(sigma, truncate)
    assert r2 == r and np.array_equal(w2, w)


def test_restatement_is_within_the_derived_bound_of_scipy(vad, golden):
    """Each pass is a sequential sum of n = 2r + 1 rounded products of once-rounded taps: relative error (n + 2) u per pass to
    first order, u = 2^-24, against the same sum of absolute values; two passes: |got - exact| <= 2 (n + 2) u G(|x|), G(|x|) =
    scipy's float64 smoothing of |x|.  The bound is the tolerance: every pixel, no slack factor."""
    g = golden(GOLDEN)
    for name in g["names"]:
        sigma, truncate = g[f"p_{name}"]
        x, s = g[f"x_{name}"], g[f"s_{name}"]
        r, w = vad.metrics.gaussian_taps(float(sigma), float(truncate))
        assert np.array_equal(w, ref.taps(sigma, truncate)[1])               # the restatement runs on the library's taps
        n = 2 * r + 1
        bound = 2 * (n + 2) * 2.0 ** -24 * g[f"g_{name}"]
        for maps, exact in ((x, g[f"g_{name}"]), (x * s.astype(np.float32), g[f"gs_{name}"])):
            got = ref.smooth(maps, sigma, truncate)
            assert got.dtype == np.float32 and got.shape == maps.shape
            ratio = float((np.abs(got.astype(np.float64) - exact) / bound).max())
            print(f"{name}: largest error {ratio:.3f} of the bound")
            assert ratio <= 1.0, (name, ratio)


def test_restatement_details(vad):
    """Reflection indices are scipy's (d c b a | a b c d | d c b a); frames are smoothed one by one; NaN / Inf follow the window."""
    assert ref.reflect_index(4, 3).tolist() == [2, 1, 0, 0, 1, 2, 3, 3, 2, 1]
    assert ref.reflect_index(2, 2).tolist() == [1, 0, 0, 1, 1, 0]
    with pytest.raises(ValueError, match="one reflection"):
        ref.reflect_index(2, 3)
    with pytest.raises(ValueError, match="one reflection"):                 # r = 2 > min(H, W) = 1: refused, not supported
        ref.smooth(np.ones((1, 3), np.float32), 0.5)
    rng = np.random.default_rng(3)
    x = rng.random((3, 2, 1, 9, 11), dtype=np.float32)
    whole = ref.smooth(x, 1.0)
    assert np.array_equal(whole[1, 0, 0], ref.smooth(x[1, 0, 0], 1.0))
    y = x[0, 0, 0].copy()
    y[0, 10] = np.nan
    y[8, 3] = np.inf
    got = ref.smooth(y, 1.0)
    r = vad.metrics.gaussian_taps(1.0)[0]
    assert r == 4
    nan_win, inf_win = ref.window(9, 11, 0, 10, r), ref.window(9, 11, 8, 3, r)
    assert np.array_equal(np.isnan(got), nan_win)
    assert np.array_equal(np.isposinf(got), inf_win & ~nan_win)
    assert np.array_equal(got[~nan_win & ~inf_win], ref.smooth(x[0, 0, 0], 1.0)[~nan_win & ~inf_win])
    assert np.isnan(ref.frame_max(got)) and ref.frame_max(whole).shape == (3, 2, 1)


def test_host_refusals(vad):
    VadError = vad.hip.VadError
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "4", True):
        with pytest.raises(VadError, match="sigma"):
            vad.metrics.gaussian_taps(bad)
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(VadError, match="truncate"):
            vad.metrics.gaussian_taps(4.0, bad)
    with pytest.raises(VadError, match="radius"):
        vad.metrics.gaussian_taps(0.1)                                      # radius 0
    with pytest.raises(VadError, match="radius"):
        vad.metrics.gaussian_taps(8.2)                                      # radius 33
    with pytest.raises(VadError, match="underflow"):
        vad.metrics.gaussian_taps(2.0, 16.0)                                # radius 32, outer taps e^-128
    assert vad.metrics.gaussian_taps(8.0)[0] == 32 == vad.metrics.SMOOTH_MAX_RADIUS
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(VadError, match="sigma"):
        vad.metrics.smooth_maps(x, sigma=0.0)
    with pytest.raises(VadError, match="sigma"):
        vad.metrics.smooth_maps(x, sigma=float("inf"))
    with pytest.raises(VadError, match="no CPU fallback"):
        vad.metrics.smooth_maps(x)
    with pytest.raises(VadError, match="torch tensor"):
        vad.metrics.smooth_maps(np.zeros((16, 16), np.float32))
    with pytest.raises(VadError, match="return_max"):
        vad.metrics.smooth_maps(x, return_max="yes")


def test_c_abi_refusals_need_no_device(vad):
    """Every argument check of vad_smooth_maps comes before anything is launched: with pointers that are never followed."""
    lib = vad.hip.lib()
    th, tw = C.c_int(), C.c_int()
    assert lib.vad_smooth_tile(C.byref(th), C.byref(tw)) == 0 and (th.value, tw.value) == vad.hip.SMOOTH_TILE
    tiles = lambda h, w: -(-h // th.value) * -(-w // tw.value)
    assert lib.vad_smooth_workspace_bytes(512, 256, 256, 16) == 512 * tiles(256, 256) * 4
    assert lib.vad_smooth_workspace_bytes(3, 33, 65, 1) == 3 * 2 * 2 * 4
    assert lib.vad_smooth_workspace_bytes(0, 16, 16, 4) == 0
    for n, h, w, r in ((1, 16, 16, 0), (1, 64, 64, 33), (1, 8, 64, 9), (1, 64, 8, 9), (-1, 16, 16, 4), (1, 0, 16, 1), (1, 4096, 4096, 4)):
        assert lib.vad_smooth_workspace_bytes(n, h, w, r) == 0, (n, h, w, r)
    maps, out, taps, fmax, ws = 0x10000, 0x90000, 0x8000, 0x4000, 0x2000     # 32 KiB of maps at most below
    call = lambda *a: lib.vad_smooth_maps(*a, None)
    ERR_ARG, ERR_WS = -1, -3
    for r, text in ((0, b"radius must be in 1..32"), (33, b"radius must be in 1..32"), (17, b"exceeds min(h, w)")):
        assert call(maps, 2, 16, 64, taps, r, out, None, None, 0) == ERR_ARG and text in lib.vad_last_error(), r
    assert call(maps, 2, 64, 16, taps, 17, out, None, None, 0) == ERR_ARG and b"exceeds min(h, w)" in lib.vad_last_error()
    assert call(maps, -1, 16, 16, taps, 4, out, None, None, 0) == ERR_ARG and b"negative" in lib.vad_last_error()
    assert call(maps, 2, 4096, 4096, taps, 4, out, None, None, 0) == ERR_ARG and b"pixels per frame" in lib.vad_last_error()
    assert call(maps, 2, 16, 16, taps, 4, None, None, ws, 64) == ERR_ARG and b"both NULL" in lib.vad_last_error()
    assert call(None, 2, 16, 16, taps, 4, out, None, None, 0) == ERR_ARG and b"NULL" in lib.vad_last_error()
    assert call(maps, 2, 16, 16, None, 4, out, None, None, 0) == ERR_ARG and b"NULL" in lib.vad_last_error()
    for a, b in ((maps, maps), (maps, maps + 4), (maps, maps + 2 * 256 * 4 - 4), (maps + 2 * 256 * 4 - 4, maps)):
        assert call(a, 2, 16, 16, taps, 4, b, None, None, 0) == ERR_ARG and b"overlaps" in lib.vad_last_error(), (a, b)
    for ptrs in ((maps + 2, out, taps, fmax, ws), (maps, out + 1, taps, fmax, ws), (maps, out, taps + 2, fmax, ws), (maps, out, taps, fmax + 2, ws),
                 (maps, out, taps, fmax, ws + 1)):
        m, o, t, f, w_ = ptrs
        assert call(m, 2, 16, 16, t, 4, o, f, w_, 64) == ERR_ARG and b"aligned" in lib.vad_last_error(), ptrs
    assert call(maps, 2, 16, 16, taps, 4, out, fmax, ws, 7) == ERR_WS and b"workspace of 8 bytes needed, 7 given" in lib.vad_last_error()
    assert call(maps, 2, 16, 16, taps, 4, out, fmax, None, 0) == ERR_WS
    assert call(maps, 0, 16, 16, taps, 4, out, fmax, None, 0) == 0           # n == 0: VAD_OK, nothing launched, no workspace needed
    assert call(maps, 0, 16, 16, taps, 4, out, None, None, 0) == 0
