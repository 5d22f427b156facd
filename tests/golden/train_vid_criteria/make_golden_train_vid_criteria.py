"""Generate tests/golden/train_vid_criteria/*.npz by running the REFERENCE's own model, criteria and optimiser (build container
only): the fixtures of `VideoTrainer(loss="ssim" | "combined")` (tests/test_hip_train_vid_criteria.py).  Same conventions as
tests/golden/make_golden.py, whose loader of the reference's modules (by file path: `import utils` would pull in torchvision) and
synthetic-weight generator this script reuses, so no weights are stored.

One fixture per criterion: the reference's `VideoAutoencoder.train()`, its `SSIMLoss()` / `CombinedLoss(alpha=0.5)`
(utils/losses.py:14-121) on the frames of the batch as one `[B*T,3,H,W]` batch - a frame is the only sample shape SSIMLoss accepts -
and `torch.optim.Adam(lr 1e-4, weight_decay 1e-5)`, three steps on one seeded batch.  Shapes, seeds and the strided storage are
those of `train_fixture` in tests/golden/make_golden.py (the MSE fixture train_vid_l32.npz), entry for entry.

    python tests/golden/train_vid_criteria/make_golden_train_vid_criteria.py                # rewrites every fixture
    python tests/golden/train_vid_criteria/make_golden_train_vid_criteria.py ssim.npz       # rewrites the named ones
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent


def _base():
    """tests/golden/make_golden.py as a module (it loads the reference's modules under private names)."""
    spec = importlib.util.spec_from_file_location("_make_golden", HERE.parent / "make_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _criterion(base, tag):
    return {"ssim": lambda: base.ref_losses.SSIMLoss(), "combined": lambda: base.ref_losses.CombinedLoss(alpha=0.5)}[tag]()


def train_fixture(name, tag, latent=32, layers=2, b=2, t=3, hw=32, wseed=61, xseed=161, steps=3, stride=7):
    base = _base()
    m = base.ref_vae.VideoAutoencoder(in_channels=3, latent_dim=latent, lstm_hidden_dim=latent, lstm_num_layers=layers)
    base._load_synth(m, wseed)
    m.train()
    x = torch.from_numpy(base.synth.clips(xseed, 0, b, t, 3, hw, hw))
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=1e-5)
    crit = _criterion(base, tag)
    arrays, losses = {}, []
    for s in range(steps):
        loss = crit(m(x).view(b * t, 3, hw, hw), x.view(b * t, 3, hw, hw))
        opt.zero_grad()
        loss.backward()
        if s == 0:
            arrays["param_keys"] = np.array([k for k, _ in m.named_parameters()])
            arrays["grad_norms"] = np.array([float(p.grad.double().norm()) for _, p in m.named_parameters()])
            for i, (_, p) in enumerate(m.named_parameters()):
                arrays[f"grad_{i}"] = p.grad.detach().reshape(-1)[::stride].numpy().copy()
        opt.step()
        losses.append(float(loss.detach()))
    st = m.state_dict()
    arrays["state_keys"] = np.array(list(st.keys()))
    for i, (k, v) in enumerate(st.items()):
        arrays[f"state_{i}"] = (v.detach().reshape(-1)[::stride] if v.dim() else v.detach().reshape(1)).numpy().copy()
    path = HERE / name
    np.savez_compressed(path, criterion=np.array(tag), alpha=np.array(0.5), window=np.array(11), losses=np.array(losses),
                        latent=np.array(latent), layers=np.array(layers), b=np.array(b), t=np.array(t), hw=np.array(hw),
                        wseed=np.array(wseed), xseed=np.array(xseed), steps=np.array(steps), stride=np.array(stride), **arrays)
    print(f"{name}: {path.stat().st_size / 1024:.0f} KiB, losses {losses}")


FIXTURES = {"ssim.npz": lambda n: train_fixture(n, "ssim"), "combined.npz": lambda n: train_fixture(n, "combined")}

if __name__ == "__main__":
    torch.set_num_threads(8)
    for fixture in (sys.argv[1:] or list(FIXTURES)):
        FIXTURES[fixture](fixture)
