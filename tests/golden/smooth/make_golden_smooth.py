"""Writes scipy_gaussian.npz: small float32 maps and scipy.ndimage.gaussian_filter's float64 results for them (mode="reflect"), so
that the suite needs no scipy.  Run from the repository root:  python tests/golden/smooth/make_golden_smooth.py

Per case `name` (CASES below): x_<name> float32 [H, W] >= 0, log-normal over many exponents; s_<name> int8 [H, W] of +-1;
g_<name> float64 = gaussian_filter(float64(x)) - also G(|x|) of both variants; gs_<name> float64 = gaussian_filter(float64(x * s)).
taps_<sigma>_<truncate> float64: scipy's impulse response (the filter applied to a unit impulse, cut to 2r + 1 samples)."""
from pathlib import Path

import numpy as np
from scipy.ndimage import gaussian_filter

# name -> (H, W, sigma, truncate)
CASES = {
    "h16w16_s4": (16, 16, 4.0, 4.0),
    "h32w48_s4": (32, 48, 4.0, 4.0),
    "h64w64_s4": (64, 64, 4.0, 4.0),
    "h16w20_s1": (16, 20, 1.0, 4.0),
    "h32w32_s8": (32, 32, 8.0, 4.0),
    "h2w3_s05": (2, 3, 0.5, 4.0),
    "h24w40_s2_t3": (24, 40, 2.0, 3.0),
}
TAPS = [(0.5, 4.0), (1.0, 4.0), (2.0, 4.0), (4.0, 4.0), (8.0, 4.0), (2.0, 3.0), (4.0, 3.0)]


def main():
    out = {"names": np.array(list(CASES))}
    for i, (name, (h, w, sigma, truncate)) in enumerate(CASES.items()):
        rng = np.random.default_rng(4140 + i)
        x = (np.exp(rng.standard_normal((h, w)) * 3.0) * 1e-3).astype(np.float32)
        s = rng.choice(np.array([-1, 1], np.int8), (h, w))
        out[f"x_{name}"] = x
        out[f"s_{name}"] = s
        out[f"g_{name}"] = gaussian_filter(x.astype(np.float64), sigma, truncate=truncate, mode="reflect")
        out[f"gs_{name}"] = gaussian_filter(x.astype(np.float64) * s, sigma, truncate=truncate, mode="reflect")
        out[f"p_{name}"] = np.array([sigma, truncate], np.float64)
    for sigma, truncate in TAPS:
        r = int(truncate * sigma + 0.5)
        impulse = np.zeros(4 * r + 1)
        impulse[2 * r] = 1.0
        out[f"taps_{sigma}_{truncate}"] = gaussian_filter(impulse, sigma, truncate=truncate, mode="constant")[r:3 * r + 1]
    path = Path(__file__).resolve().parent / "scipy_gaussian.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
