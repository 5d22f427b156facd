"""Writes scipy_grey.npz: small finite float32 maps and the results of scipy.ndimage.grey_erosion / grey_dilation / grey_opening /
grey_closing for them (flat `size=`, mode="reflect"; recorded with scipy 1.15.3), so that the suite needs no scipy.  Run from the
repository root:  python tests/golden/morph/make_golden_morph.py

maps: names [M]; x_<map> float32 [H, W].  Per map, size and op: <op>_<map>_<size_h>x<size_w> float32 [H, W].  `cases` int32 [K, 3]:
(index into names, size_h, size_w) of every recorded result.  Values repeat within a map (drawn from 12 levels, signed), so windows
hold ties; all finite - scipy leaves NaN unspecified."""
from pathlib import Path

import numpy as np
from scipy import ndimage

MAPS = {"h13w17": (13, 17), "h8w9": (8, 9), "h3w4": (3, 4), "h1w6": (1, 6)}
SIZES = [(2, 2), (3, 3), (4, 3), (1, 5), (7, 7), (6, 5)]
FUNCS = {"erode": ndimage.grey_erosion, "dilate": ndimage.grey_dilation, "open": ndimage.grey_opening, "close": ndimage.grey_closing}


def main():
    out = {"names": np.array(list(MAPS))}
    cases = []
    for i, (name, (h, w)) in enumerate(MAPS.items()):
        rng = np.random.default_rng(4200 + i)
        levels = (rng.standard_normal(12) * 2.0).astype(np.float32)
        x = levels[rng.integers(0, 12, (h, w))]
        out[f"x_{name}"] = x
        for sh, sw in SIZES:
            cases.append((i, sh, sw))
            for op, fn in FUNCS.items():
                got = fn(x, size=(sh, sw), mode="reflect")
                assert got.dtype == np.float32 and got.shape == x.shape
                out[f"{op}_{name}_{sh}x{sw}"] = got
    out["cases"] = np.array(cases, np.int32)
    path = Path(__file__).resolve().parent / "scipy_grey.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
