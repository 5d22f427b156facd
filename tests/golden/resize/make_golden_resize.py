"""Generate tests/golden/resize/pil_bilinear.npz: PIL's own `Image.resize(..., Image.BILINEAR)` on regenerated inputs, the
fixtures of the device resize (tests/test_resize_plan.py, tests/test_hip_resize.py).  Needs numpy + PIL only.

torchvision's `transforms.Resize((h, w))` on a PIL image is `img.resize((w, h), Image.BILINEAR)`.

Inputs are NOT stored: tests/resize_ref.py rebuilds them (hash noise from synth.frames_u8 transposed to HWC, and one smooth
ramp).  Stored: the case table (names, seeds, geometries), PIL's version and PIL's output of every case.

    python tests/golden/resize/make_golden_resize.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
import resize_ref  # noqa: E402  (tests/resize_ref.py)


def main() -> None:
    arrays = {"pil_version": np.array(PIL.__version__), "names": np.array(list(resize_ref.CASES)),
              "table": np.array([[seed, n, ih, iw, oh, ow] for _, seed, n, ih, iw, oh, ow in resize_ref.CASES.values()], np.int64),
              "kinds": np.array([c[0] for c in resize_ref.CASES.values()])}
    for name, (_, _, _, _, _, oh, ow) in resize_ref.CASES.items():
        frames = resize_ref.case_input(name)
        arrays["out_" + name] = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((ow, oh), Image.BILINEAR)) for f in frames])
    path = HERE / "pil_bilinear.npz"
    np.savez_compressed(path, **arrays)
    print(f"{path.name}: {path.stat().st_size / 1024:.0f} KiB (PIL {PIL.__version__})")


if __name__ == "__main__":
    main()
