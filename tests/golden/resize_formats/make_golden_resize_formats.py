"""Generate tests/golden/resize_formats/pil_formats.npz: PIL's own output for one-byte (mode L) and RGBA inputs, the fixtures
of the device Resize's other pixel formats (tests/test_resize_formats_plan.py, tests/test_hip_resize_formats.py).  Needs numpy
+ PIL only.

The reference opens every file with `Image.open(path).convert('RGB')` and the ground-truth masks with `convert('L')`; then
torchvision's `transforms.Resize((h, w))` is `img.resize((w, h), Image.BILINEAR)`.

Inputs are NOT stored: tests/resize_formats_ref.py rebuilds them (hash noise from synth.frames_u8).  Stored: the case names and
geometries, PIL's version, and per case
    l_<name>     [n, oh, ow]      fromarray(g, 'L').resize(...)                  (the mask path)
    rgba_<name>  [n, oh, ow, 3]   fromarray(a, 'RGBA').convert('RGB').resize(...)
`fromarray(g, 'L').convert('RGB').resize(...)` is checked HERE to be l_<name> in all three channels and is not stored a second
time.

    python tests/golden/resize_formats/make_golden_resize_formats.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
import resize_formats_ref as F  # noqa: E402  (tests/resize_formats_ref.py)


def main() -> None:
    arrays = {"pil_version": np.array(PIL.__version__), "names": np.array(list(F.NAMES)),
              "table": np.array([list(F.geometry(name)) for name in F.NAMES], np.int64)}
    for name in F.NAMES:
        _, _, _, oh, ow = F.geometry(name)
        planes = np.stack([np.asarray(Image.fromarray(g, "L").resize((ow, oh), Image.BILINEAR)) for g in F.mono_input(name)])
        as_rgb = np.stack([np.asarray(Image.fromarray(g, "L").convert("RGB").resize((ow, oh), Image.BILINEAR)) for g in F.mono_input(name)])
        assert np.array_equal(as_rgb, np.repeat(planes[..., None], 3, axis=-1)), name
        arrays["l_" + name] = planes
        arrays["rgba_" + name] = np.stack([np.asarray(Image.fromarray(a, "RGBA").convert("RGB").resize((ow, oh), Image.BILINEAR))
                                           for a in F.rgba_input(name)])
    path = HERE / "pil_formats.npz"
    np.savez_compressed(path, **arrays)
    print(f"{path.name}: {path.stat().st_size / 1024:.0f} KiB (PIL {PIL.__version__})")


if __name__ == "__main__":
    main()
