"""Generate tests/golden/ssim_score/*.npz by running the REFERENCE's own models and criteria (build container only): the
fixtures of per-frame SSIM / combined scoring (tests/test_hip_ssim_score.py).  Same conventions as tests/golden/make_golden.py,
whose loader of the reference's modules and synthetic-weight generator this script reuses, so no weights are stored.

Per-sample values are the reference's criterion objects on a batch of one: `SSIMLoss(window)(recon[i:i+1], x[i:i+1])`,
`CombinedLoss(alpha, window)(...)` (utils/losses.py:14-121), next to `model.get_reconstruction_error`.

The `validate_*` fixtures hold the tuple `validate(model, loader, criterion, device)` returns (train.py:54-91,
train_video.py:68-98).  Those two scripts do not import here (their `utils` package needs torchvision), so `_validate`
makes the same calls on the reference's model and criterion objects, per batch and in that loop's order - the forward, the
criterion on its result, `.item()`, `get_reconstruction_error` - and reduces what they returned itself: batch losses averaged
over the batches, errors averaged per label.  For clips the SSIM criteria take the frames of the batch as one `[B*T,C,H,W]` batch: a frame is the only
sample shape SSIMLoss accepts (train_video.py itself offers MSELoss only).

    python tests/golden/ssim_score/make_golden_ssim_score.py                      # rewrites every fixture
    python tests/golden/ssim_score/make_golden_ssim_score.py img_c3_48x80.npz     # rewrites the named ones
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ALPHA = 0.3          # per-sample fixtures (not the default, so a dropped argument shows); validate uses train.py's default 0.5


def _base():
    """tests/golden/make_golden.py as a module (it loads the reference's modules under private names)."""
    spec = importlib.util.spec_from_file_location("_make_golden", HERE.parent / "make_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _save(name, **arrays):
    path = HERE / name
    np.savez_compressed(path, **arrays)
    print(f"{name}: {path.stat().st_size / 1024:.0f} KiB")


def _per_sample(base, recon, x, window, alpha):
    """The reference's criteria on every sample as a batch of one -> (ssim [N], combined [N]) float32."""
    ssim_l, comb_l = base.ref_losses.SSIMLoss(window_size=window, channels=x.shape[1]), base.ref_losses.CombinedLoss(alpha=alpha, window_size=window)
    comb_l.ssim = base.ref_losses.SSIMLoss(window_size=window, channels=x.shape[1])      # (CombinedLoss builds a 3-channel window)
    ssim = [ssim_l(recon[i:i + 1], x[i:i + 1]) for i in range(len(x))]
    comb = [comb_l(recon[i:i + 1], x[i:i + 1]) for i in range(len(x))]
    return torch.stack(ssim).numpy(), torch.stack(comb).numpy()


def image_fixture(name, in_ch, h, w, n, windows, wseed, xseed, latent=32, lowcontrast=False):
    """`lowcontrast`: the frames are `0.8 + 0.01 * noise` instead of the synthetic stream - the target's variance terms then
    cancel in fp32 over the C2 floor.  (The reconstruction of such a frame by a synthetic-weight model is NOT low-contrast; on
    a pair where both sides are, the reference's own fp32 per-frame value is 5e-6 from float64 at window 11 and 1e-5 at
    window 15, which no 2e-6 comparison with it can survive: that pair is generated inside the map test, whose bound is
    relative to exactly this error.  On every fixture written here the reference is within 9e-7 of float64.)"""
    base = _base()
    torch.manual_seed(0)
    model = base._load_synth(base.ref_ae.ConvAutoencoder(in_channels=in_ch, latent_dim=latent), wseed)
    if lowcontrast:
        x = torch.from_numpy((0.8 + 0.01 * np.random.default_rng(xseed).standard_normal((n, in_ch, h, w))).astype(np.float32))
    else:
        x = torch.from_numpy(base.synth.frames(xseed, 0, n, in_ch, h, w))
    arrays = {}
    with torch.no_grad():
        recon = model(x)
        mse = model.get_reconstruction_error(x, per_pixel=False)
        for win in windows:
            arrays[f"ssim_w{win}"], arrays[f"combined_w{win}"] = _per_sample(base, recon, x, win, ALPHA)
    _save(name, latent_dim=np.array(latent), in_channels=np.array(in_ch), wseed=np.array(wseed), xseed=np.array(xseed),
          windows=np.array(windows), alpha=np.array(ALPHA), x=x.numpy(), recon=recon.numpy(), mse=mse.numpy(), **arrays)


def video_fixture(name, b=2, t=3, hw=32, latent=32, hid=32, layers=2, wseed=91, xseed=291, window=11):
    base = _base()
    torch.manual_seed(0)
    model = base._load_synth(base.ref_vae.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid,
                                                           lstm_num_layers=layers), wseed)
    x = torch.from_numpy(base.synth.clips(xseed, 0, b, t, 3, hw, hw))
    with torch.no_grad():
        recon = model(x)
        frame = model.get_reconstruction_error(x, per_frame=True)
        seq = model.get_reconstruction_error(x, per_frame=False)
        ssim, comb = _per_sample(base, recon.reshape(b * t, 3, hw, hw), x.reshape(b * t, 3, hw, hw), window, ALPHA)
    ssim, comb = ssim.reshape(b, t), comb.reshape(b, t)
    _save(name, latent_dim=np.array(latent), hid=np.array(hid), layers=np.array(layers), wseed=np.array(wseed), xseed=np.array(xseed),
          b=np.array(b), t=np.array(t), hw=np.array(hw), window=np.array(window), alpha=np.array(ALPHA), recon=recon.numpy(),
          mse=frame.numpy(), ssim=ssim, combined=comb, seq_mse=seq.numpy(), seq_ssim=ssim.mean(axis=1), seq_combined=comb.mean(axis=1))


def _criteria(base):
    return {"mse": torch.nn.MSELoss(), "ssim": base.ref_losses.SSIMLoss(), "combined": base.ref_losses.CombinedLoss(alpha=0.5)}


def _validate(model, loader, criterion, key, frames_as_batch):
    """What the reference's validation loop returns (see the module docstring), from per-batch and per-sample arrays: the
    batch criteria averaged over the batches, and the reconstruction errors averaged per label (0 where a label has no sample).
    The per-label means add the float32 errors one after the other in loader order, as a running float32 sum does."""
    model.eval()
    losses, errors, labels = [], [], []
    with torch.no_grad():
        for batch in loader:
            x = batch[key]
            recon = model(x)
            if frames_as_batch:                       # clips under an SSIM criterion: [B,T,C,H,W] -> [B*T,C,H,W]
                losses.append(criterion(recon.flatten(0, 1), x.flatten(0, 1)).item())
            else:
                losses.append(criterion(recon, x).item())
            errors.append(model.get_reconstruction_error(x).numpy())
            labels.append(batch["label"].numpy())
    errors, labels = np.concatenate(errors), np.concatenate(labels)

    def label_mean(mask):
        e = errors[mask]
        return e.cumsum(dtype=np.float32)[-1] / np.float32(len(e)) if len(e) else 0

    return float(np.sum(losses)) / len(losses), label_mean(labels == 0), label_mean(labels != 0)


BATCHES = (4, 4, 2)      # a ragged loader


def validate_image_fixture(name, hw=32, latent=32, wseed=92, xseed=292):
    base = _base()
    torch.manual_seed(0)
    model = base._load_synth(base.ref_ae.ConvAutoencoder(in_channels=3, latent_dim=latent), wseed)
    n = sum(BATCHES)
    labels = base.synth.frame_label(xseed, np.arange(n))
    assert 0 < labels.sum() < n, "the loader must carry both labels"
    loader, s = [], 0
    for k in BATCHES:
        loader.append({"image": torch.from_numpy(base.synth.frames(xseed, s, k, 3, hw, hw)), "label": torch.from_numpy(labels[s:s + k])})
        s += k
    res = {tag: np.array(_validate(model, loader, crit, "image", False), dtype=np.float64) for tag, crit in _criteria(base).items()}
    _save(name, latent_dim=np.array(latent), hw=np.array(hw), wseed=np.array(wseed), xseed=np.array(xseed), batches=np.array(BATCHES),
          labels=labels, **res)


def validate_video_fixture(name, t=3, hw=32, latent=32, hid=32, layers=2, wseed=93, xseed=293):
    base = _base()
    torch.manual_seed(0)
    model = base._load_synth(base.ref_vae.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=hid,
                                                           lstm_num_layers=layers), wseed)
    n = sum(BATCHES)
    labels = base.synth.frame_label(xseed, np.arange(n))
    assert 0 < labels.sum() < n, "the loader must carry both labels"
    loader, s = [], 0
    for k in BATCHES:
        loader.append({"frames": torch.from_numpy(base.synth.clips(xseed, s, k, t, 3, hw, hw)), "label": torch.from_numpy(labels[s:s + k])})
        s += k
    res = {tag: np.array(_validate(model, loader, crit, "frames", tag != "mse"), dtype=np.float64) for tag, crit in _criteria(base).items()}
    _save(name, latent_dim=np.array(latent), hid=np.array(hid), layers=np.array(layers), t=np.array(t), hw=np.array(hw),
          wseed=np.array(wseed), xseed=np.array(xseed), batches=np.array(BATCHES), labels=labels, **res)


FIXTURES = {
    "img_c3_48x80.npz": lambda n: image_fixture(n, in_ch=3, h=48, w=80, n=5, windows=(11, 3), wseed=94, xseed=294),
    "img_c1_32.npz": lambda n: image_fixture(n, in_ch=1, h=32, w=32, n=2, windows=(15,), wseed=95, xseed=295),
    "img_c5_16.npz": lambda n: image_fixture(n, in_ch=5, h=16, w=16, n=2, windows=(11,), wseed=96, xseed=296),
    "img_lowcontrast_32x48.npz": lambda n: image_fixture(n, in_ch=3, h=32, w=48, n=3, windows=(11, 3), wseed=97, xseed=311, lowcontrast=True),
    "vid_l32_32.npz": video_fixture,
    "validate_img.npz": validate_image_fixture,
    "validate_vid.npz": validate_video_fixture,
}

if __name__ == "__main__":
    torch.set_num_threads(8)
    for fixture in (sys.argv[1:] or list(FIXTURES)):
        FIXTURES[fixture](fixture)
