"""CPU checks of the video training step's workspace plan with a criterion (`vad_vid_train_workspace_bytes_l`, csrc/train_step.hip):
host arithmetic through ctypes, no GPU.  Kind 0 (MSE) must be the legacy size to the byte; the SSIM / combined kinds add, behind
everything else, the reconstruction, its gradient, the larger of the two SSIM scratch sizes and two 64-float slots of device
scalars (`out3`, `ones`).  Every slot of the carve is rounded up to 64 floats, so the five new slots cost at most
5 * 63 floats of rounding + 128 floats of scalars = 1772 bytes on top of the arrays: inside the 4096 allowed here."""
import itertools

import pytest

SHAPES = [(1, 1, 16, 16), (2, 3, 32, 32), (2, 2, 48, 80)]          # (b, t, h, w)
MODELS = [(32, 32, 1), (32, 64, 2)]                                # (latent, hid, layers)
CASES = list(itertools.product(SHAPES, MODELS))


@pytest.fixture(scope="module")
def lib(vad):
    return vad.hip.lib()


@pytest.mark.parametrize("shape,model", CASES)
def test_mse_kind_is_the_legacy_size(lib, shape, model):
    legacy = lib.vad_vid_train_workspace_bytes(*shape, *model)
    assert legacy > 0
    assert lib.vad_vid_train_workspace_bytes_l(*shape, *model, 0) == legacy


@pytest.mark.parametrize("shape,model", CASES)
def test_criterion_kinds_add_their_buffers_behind_the_legacy_carve(lib, shape, model):
    b, t, h, w = shape
    planes = b * t * 3
    k0, k1, k2 = (lib.vad_vid_train_workspace_bytes_l(*shape, *model, kind) for kind in (0, 1, 2))
    assert k1 == k2
    f = 2 * planes * h * w + max(lib.vad_ssim_workspace_floats(planes, h, w), lib.vad_ssim_grad_workspace_floats(planes, h, w))
    assert 4 * f <= k1 - k0 <= 4 * f + 4096, (k1 - k0, 4 * f)


@pytest.mark.parametrize("model", MODELS)
def test_unsupported_shapes_and_kinds_have_no_size(lib, model):
    assert lib.vad_vid_train_workspace_bytes_l(2, 3, 32, 32, *model, 2) > 0
    for kind in (0, 1, 2):
        assert lib.vad_vid_train_workspace_bytes_l(2, 3, 24, 32, *model, kind) == 0
    assert lib.vad_vid_train_workspace_bytes_l(2, 3, 32, 32, *model, 3) == 0
    assert lib.vad_vid_train_workspace_bytes_l(2, 3, 32, 32, *model, -1) == 0
