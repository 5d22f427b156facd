"""Torch composition of per-frame SSIM (the formula of the reference's utils/losses.py:51-93 kept per frame and per pixel), in
a chosen dtype, on the CPU: what tests/test_hip_ssim_score.py compares vad_ssim_score with.  float64 is the yardstick; the
float32 run is the reference's own arithmetic (five F.conv2d with the 2-D window), whose distance from float64 on the same
inputs is the measure of how ill-conditioned those inputs are."""
import torch
import torch.nn.functional as F

C1, C2, SIGMA = 0.01 ** 2, 0.03 ** 2, 1.5


def window_2d(size: int, channels: int, dtype) -> torch.Tensor:
    """utils/losses.py:34-49: the 1-D Gaussian is built and normalised in float32, then widened."""
    offs = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-offs ** 2 / (2 * SIGMA ** 2))
    g = (g / g.sum()).to(dtype)
    return torch.outer(g, g).expand(channels, 1, size, size).contiguous()


def ssim_frames(pred, target, window_size: int, dtype=torch.float64):
    """pred, target: [N,C,H,W] (numpy or tensors) -> (ssim [N] = 1 - mean S per frame, map [N,1,H,W] = channel mean of 1 - S)."""
    p = torch.as_tensor(pred).to("cpu", dtype)
    t = torch.as_tensor(target).to("cpu", dtype)
    c, pad = p.shape[1], window_size // 2
    win = window_2d(window_size, c, dtype)

    def blur(v):
        return F.conv2d(v, win, padding=pad, groups=c)

    mu_p, mu_t = blur(p), blur(t)
    mpp, mtt, mpt = mu_p ** 2, mu_t ** 2, mu_p * mu_t
    var_p, var_t, cov = blur(p ** 2) - mpp, blur(t ** 2) - mtt, blur(p * t) - mpt
    s = ((2 * mpt + C1) * (2 * cov + C2)) / ((mpp + mtt + C1) * (var_p + var_t + C2))
    return 1 - s.mean(dim=[1, 2, 3]), (1 - s).mean(dim=1, keepdim=True)
