"""Oracles for `VideoTrainer(loss=...)`: the float64 / fp32 CPU restatements of one training step of the video autoencoder with
the criterion as an argument (tests/test_hip_train_step.py states them for nn.MSELoss only).  A helper module, not a test file.

The criterion of a clip batch is that of its frames as one batch: `criterion(recon.view(B*T,3,H,W), x.view(B*T,3,H,W))`, the one
shape SSIMLoss takes.  Decision recording is tests/test_hip_train_step.py's, the float64 Gaussian window substitution
tests/test_hip_train_img.py's (a float64 module keeps its window as a plain attribute, which `.double()` does not convert)."""
import numpy as np
import torch
import torch.nn as nn

from conftest import load_synthetic

WD = 1e-5


def dims(latent):
    """(latent_dim, lstm_hidden_dim); a plain int means both are equal (proj = Identity)."""
    return latent if isinstance(latent, tuple) else (latent, latent)


def make(vad, latent, layers, wseed):
    lat, hid = dims(latent)
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=lat, lstm_hidden_dim=hid, lstm_num_layers=layers)
    load_synthetic(vad, m, wseed)
    return m


def criterion(vad, loss, alpha=0.5, window=11, double=False):
    """nn.MSELoss | SSIMLoss(window) | CombinedLoss(alpha, window) of this package (CPU: the stock torch composition)."""
    if loss == "mse":
        return nn.MSELoss()
    crit = vad.SSIMLoss(window_size=window) if loss == "ssim" else vad.CombinedLoss(alpha=alpha, window_size=window)
    if double:
        ssim = crit if loss == "ssim" else crit.ssim
        ssim.window = vad.losses._gaussian_window(window, 3).double()
    return crit


def frames(t):
    """[B,T,3,H,W] -> [B*T,3,H,W]"""
    return t.reshape(-1, *t.shape[2:])


def bn_fed_biases(model):
    """names of conv / convT biases directly followed by BatchNorm (true gradient zero in train mode)"""
    names = []
    for prefix, seq in (("encoder.encoder", model.encoder.encoder), ("decoder.decoder", model.decoder.decoder)):
        mods = list(seq)
        for i, m in enumerate(mods[:-1]):
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and isinstance(mods[i + 1], nn.BatchNorm2d):
                names.append(f"{prefix}.{i}.bias")
    return set(names)


def record_decisions(vad, tr, x):
    """One native forward_backward with the branch decisions of every BatchNorm backward recorded, in the order
    csrc/train_step.hip issues them -> (loss, {(kind, stage): uint8 [N,C,h,w]})."""
    l = vad.hip.lib()
    b, t, _, h, w = x.shape
    n, lat = b * t, tr.cfg[0]
    dec_c, enc_c = [128, 64, 32], [32, 64, 128, lat]
    sizes = [("dec", j, (n, (h // 16) << (j + 1), (w // 16) << (j + 1), dec_c[j])) for j in (2, 1, 0)]
    sizes += [("enc", k, (n, (h >> k) // 2, (w >> k) // 2, enc_c[k])) for k in (3, 2, 1, 0)]
    total = sum(int(np.prod(s)) for _, _, s in sizes)
    buf = torch.zeros(total, dtype=torch.uint8, device="cuda")
    vad.hip.check(l.vad_debug_set_train_decisions(buf.data_ptr(), total))
    try:
        loss, _ = tr.forward_backward(x)
        torch.cuda.synchronize()
        assert l.vad_debug_train_decisions_used() == total
    finally:
        l.vad_debug_set_train_decisions(None, 0)
    out, off, host = {}, 0, buf.cpu()
    for kind, i, shape in sizes:
        k = int(np.prod(shape))
        out[(kind, i)] = host[off:off + k].view(*shape).permute(0, 3, 1, 2).contiguous()
        off += k
    return float(loss), out


def conditioned_float64(vad, latent, layers, wseed, x, decisions, loss="mse", alpha=0.5, window=11):
    """float64 loss + gradients of the train-mode composition with the given branch decisions imposed and `loss` as the
    criterion; also, per stage, (name, decisions differing from the float64 model's own, largest margin among those, total)."""
    m = make(vad, latent, layers, wseed).double().train()
    b, t, _, h, w = x.shape
    n = b * t
    cur = x.double().view(n, 3, h, w)
    enc, report = list(m.encoder.encoder), []
    for k in range(4):
        v = enc[4 * k + 1](enc[4 * k](cur))
        nn_, c, hh, ww = v.shape
        win = v.view(nn_, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(nn_, c, hh // 2, ww // 2, 4)   # scan order
        d = decisions[("enc", k)]
        am, pos = (d & 3).long(), (d & 4) > 0
        chosen = win.gather(-1, am.unsqueeze(-1)).squeeze(-1)
        cur = chosen * torch.where(pos, 1.0, 0.2).double()
        with torch.no_grad():
            best, am64 = win.max(-1)
            diff_am = am64 != am
            gap = (best - chosen)[diff_am]
            diff_sign = (~diff_am) & ((chosen > 0) != pos)
            margins = torch.cat([gap.abs().reshape(-1), chosen[diff_sign].abs().reshape(-1)])
            report.append((f"enc{k}", int(diff_am.sum() + diff_sign.sum()), float(margins.max()) if margins.numel() else 0.0, d.numel()))
    h16, w16 = h // 16, w // 16
    lat, hid = dims(latent)
    hs, _ = m.convlstm(cur.view(b, t, lat, h16, w16))
    cur = m.proj(hs.reshape(n, hid, h16, w16))
    dec = list(m.decoder.decoder)
    for j in range(3):
        v = dec[3 * j + 1](dec[3 * j](cur))
        mask = (decisions[("dec", j)] & 4) > 0
        cur = v * mask.double()
        with torch.no_grad():
            diff = (v > 0) != mask
            report.append((f"dec{j}", int(diff.sum()), float(v[diff].abs().max()) if diff.any() else 0.0, mask.numel()))
    crit = criterion(vad, loss, alpha, window, double=True)
    out = crit(torch.tanh(dec[9](cur)), x.double().view(n, 3, h, w))
    out.backward()
    return float(out.detach()), {k: p.grad.detach().numpy() for k, p in m.named_parameters()}, report


def cpu_trajectory(vad, latent, layers, wseed, x, loss, steps, lr, alpha=0.5, window=11, double=False):
    """Losses of `steps` Adam(lr, weight_decay 1e-5) steps of stock autograd on the CPU (train_video.py:44-65 with `loss` as
    the criterion), fp32 or float64."""
    m = make(vad, latent, layers, wseed)
    crit = criterion(vad, loss, alpha, window, double=double)
    if double:
        m, x = m.double(), x.double()
    m.train()
    opt, out = torch.optim.Adam(m.parameters(), lr=lr, weight_decay=WD), []
    for _ in range(steps):
        val = crit(frames(m(x)), frames(x))
        opt.zero_grad()
        val.backward()
        opt.step()
        out.append(float(val.detach()))
    return out
