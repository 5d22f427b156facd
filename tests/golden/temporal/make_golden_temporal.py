"""Writes scipy_temporal.npz: a small finite float32 clip and, along its time axis, the results of scipy.ndimage.minimum_filter1d /
maximum_filter1d with `origin=(k - 1) // 2, mode="nearest"` - the causal window x[max(0, t - k + 1) .. t] - and of a float64
scipy.signal.lfilter exponential average (recorded with scipy 1.15.3), so that the suite needs no scipy.  Run from the repository
root:  python tests/golden/temporal/make_golden_temporal.py

x float32 [11, 3, 4]: values repeat (12 levels, signed, both zeros among them), so windows hold ties; all finite - scipy leaves NaN
unspecified.  ks int32: 1, 2, 3, 4, 7, 8, 16 (16 is longer than the clip).  min_<k>, max_<k> float32 [11, 3, 4].  alphas float64 [A]:
the float32 values a kernel would multiply with, exactly; ema_<i> float64 [11, 3, 4] = y[0] = x[0], y[t] = (1 - a) y[t-1] + a x[t]."""
from pathlib import Path

import numpy as np
from scipy import ndimage, signal

KS = [1, 2, 3, 4, 7, 8, 16]
ALPHAS = [0.5, 0.25, 0.1, 0.9]


def main():
    rng = np.random.default_rng(2300)
    levels = np.concatenate([np.float32([-0.0, 0.0]), (rng.standard_normal(10) * 2.0).astype(np.float32)])
    x = levels[rng.integers(0, 12, (11, 3, 4))]
    out = {"x": x, "ks": np.array(KS, np.int32)}
    for k in KS:
        for name, fn in (("min", ndimage.minimum_filter1d), ("max", ndimage.maximum_filter1d)):
            got = fn(x, size=k, axis=0, mode="nearest", origin=(k - 1) // 2)
            assert got.dtype == np.float32 and got.shape == x.shape
            out[f"{name}_{k}"] = got
    alphas = np.array([float(np.float32(a)) for a in ALPHAS], np.float64)
    out["alphas"] = alphas
    x64 = x.astype(np.float64)
    for i, a in enumerate(alphas):
        y, _ = signal.lfilter([a], [1.0, a - 1.0], x64, axis=0, zi=(1.0 - a) * x64[:1])
        assert y.dtype == np.float64 and np.array_equal(y[0], x64[0])
        out[f"ema_{i}"] = y
    path = Path(__file__).resolve().parent / "scipy_temporal.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
