"""GPU tests of the fused enc1 launch (`vad_conv3x3_c3_fused`) at every kind of tile position.

The persistent kernel writes the first convolution's activations into its LDS tile in one straight line and then, at positions
that touch or hang over the image's edge, overwrites the out-of-image pixels with +0.0 (the zero padding of the second
convolution).  Which lanes do that is fixed per position, so the cases here are chosen by position kind:

  16 x 16   one tile: all four borders at once
  48 x 48   3 x 3 tiles: four corners, four edges and ONE INTERIOR tile (the other fused tests stop at 38 x 22: none)
  34 x 50   3 x 4 tiles whose last row holds 2 image rows and whose last column holds 2 image columns (ragged)

Each shape runs n = 5 frames under the one-CU plan of tests/test_hip_persistent.py (a work-group walks several frames) and again
under the default plan.  Exact fp32 is held to bit identity with the one-tile kernel (conv variant 0), with frame-by-frame calls
and with the default plan, and to the C oracle at the layer tests' bound; split-fp16 to frame-by-frame identity and the bound of
tests/test_hip_layers.py::test_conv3x3_c3_fused (the same 3e-5).  Non-finite inputs are compared bit pattern by bit pattern;
uint8 frames reach the kernel through the image model, as in test_image_model_scores_do_not_depend_on_the_plan."""
import functools

import numpy as np
import pytest
import torch

import test_hip_layers as L
from test_hip_persistent import C3FUSED, POOL, _default_plan, _variant, assert_tiling, last_plan, one_cu   # noqa: F401  (one_cu: autouse, module scope)
from conftest import load_synthetic, max_abs

pytestmark = pytest.mark.gpu

ATOL = L.ATOL            # 3e-5: the bound of test_conv3x3_c3_fused and of tests/test_hip_persistent.py
N = 5
SHAPES = [(16, 16), (48, 48), (34, 50)]


@functools.lru_cache(maxsize=None)
def _case(h, w):
    """Inputs, parameters and the oracle's output on frames 0, 2 and 4 of one shape: computed once, shared by both precisions,
    read-only."""
    rng = L._rng(h * 100 + w + N)
    x = rng.uniform(-1, 1, (N, 3, h, w)).astype(np.float32)
    p0, p1 = L._conv_params(rng, 32, 3), L._conv_params(rng, 32, 32)
    idx = [0, N // 2, N - 1]
    ref = L._ref_conv(L._ref_conv(x[idx], *p0, 1, False), *p1, 1, True)
    ref.setflags(write=False)
    return x, p0, p1, idx, ref


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("precision", [0, 1])
def test_enc1_every_position_kind(one_cu, h, w, precision):   # noqa: F811
    import hip_helpers as H
    l = one_cu
    x, p0, p1, idx, ref = _case(h, w)
    tiles = ((h + 15) // 16) * ((w + 15) // 16)
    with L._precision(H, precision):
        got = H.conv3x3_c3_fused(x, *p0, *p1)
        plan = last_plan(l)
        print(f"conv3x3_c3_fused {h}x{w} precision {precision}: {plan}")
        assert plan["grid"] > 0, "the launch was not persistent"
        assert_tiling(plan, C3FUSED, (2, 1, 4, 1), POOL)
        assert plan["items"] == N * tiles
        assert plan["grid"] < plan["items"], f"no work-group walks more than one frame: {plan}"
        err = max_abs(got[idx], ref)
        print(f"  max abs err against the oracle {err:.3e}")
        assert got.shape == (N, 32, h // 2, w // 2) and np.isfinite(got).all()
        assert err < ATOL
        for i in range(N):                                           # the hand-over between frames
            assert np.array_equal(got[i:i + 1], H.conv3x3_c3_fused(x[i:i + 1], *p0, *p1)), i
        with _default_plan(l):                                       # every work-group one frame (or few)
            dflt = H.conv3x3_c3_fused(x, *p0, *p1)
            assert last_plan(l)["grid"] > 0
        assert np.array_equal(got, dflt)
        if precision == 0:
            with _variant(l, 0):                                     # the one-tile kernel
                one_tile = H.conv3x3_c3_fused(x, *p0, *p1)
                assert last_plan(l)["grid"] == 0
            assert np.array_equal(got, one_tile)


def _reach(bad, h, w):
    """Pooled outputs [h/2, w/2] that an input pixel of the boolean map `bad` [h, w] can reach: two 3x3 convolutions (2 pixels
    each way), then the 2x2 pool."""
    m = np.zeros((h + 4, w + 4), bool)
    for dy in range(5):
        for dx in range(5):
            m[dy:dy + h, dx:dx + w] |= bad
    m = m[2:2 + h, 2:2 + w]
    return m.reshape(h // 2, 2, w // 2, 2).any(axis=(1, 3))


def test_enc1_non_finite_inputs(one_cu):   # noqa: F811
    """48 x 48, exact fp32: +Inf at a corner pixel of frame 1 (the first stage then computes Inf / NaN at out-of-image halo
    positions, which the zero padding must replace by 0.0 exactly as `inside ? v : 0` does) and a NaN in row 1 of frame 3.  Bit
    patterns equal those of the one-tile kernel under both plans; what only padding and finite pixels reach stays finite - the
    frames in between included, which the same work-groups compute from the same LDS right behind the poisoned ones."""
    import hip_helpers as H
    l, h, w = one_cu, 48, 48
    x0, p0, p1, _, _ = _case(h, w)
    x = x0.copy()
    x[1, 0, 0, 0] = np.inf
    x[3, 2, 1, 20] = np.nan
    got = H.conv3x3_c3_fused(x, *p0, *p1)
    assert last_plan(l)["grid"] > 0
    with _default_plan(l):
        dflt = H.conv3x3_c3_fused(x, *p0, *p1)
    with _variant(l, 0):
        one_tile = H.conv3x3_c3_fused(x, *p0, *p1)
        assert last_plan(l)["grid"] == 0
    assert np.array_equal(got.view(np.uint32), one_tile.view(np.uint32))
    assert np.array_equal(dflt.view(np.uint32), one_tile.view(np.uint32))
    bad = ~np.isfinite(x).all(axis=1)                                # [N, h, w]
    for i in range(N):
        reach = _reach(bad[i], h, w)
        assert np.isfinite(got[i][:, ~reach]).all(), i
        if not bad[i].any():
            assert np.array_equal(got[i], H.conv3x3_c3_fused(x0[i:i + 1], *p0, *p1)[0]), i
    assert not np.isfinite(got[1, :, 0, 0]).all() and not np.isfinite(got[3, :, 0, 10]).all()   # (the poison did arrive)


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_enc1_uint8_ingest_48x48(vad, one_cu, precision):   # noqa: F811
    """uint8 NHWC frames are normalised where the halo is written to LDS; padding must be 0.0 AFTER normalisation.  The image
    model's outputs on uint8 frames equal those on the normalised float frames, under the walk and under the default plan."""
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=64)
    load_synthetic(vad, m, 95)
    m = m.cuda().eval()
    m.precision = precision
    u8 = vad.synth.frames_u8(96, 0, N, 3, 48, 48, anomalies=True)
    xf = torch.from_numpy(vad.synth.u8_to_unit(u8)).cuda()
    xu = torch.from_numpy(np.ascontiguousarray(np.moveaxis(u8, -3, -1))).cuda()
    with torch.no_grad():
        a, b = m.score_all(xf), m.score_all(xu)
        with _default_plan(one_cu):
            c = m.score_all(xu)
    for k in ("scores", "errmap", "recon"):
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]) and torch.equal(b[k], c[k]), k
