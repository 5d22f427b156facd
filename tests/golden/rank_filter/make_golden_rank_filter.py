"""Writes scipy_rank.npz: small finite float32 maps and the results of scipy.ndimage.rank_filter / median_filter /
percentile_filter for them (`size=`, mode="reflect"; recorded with scipy 1.15.3), so that the suite needs no scipy.  Run from the
repository root:  python tests/golden/rank_filter/make_golden_rank_filter.py

maps: names [M]; x_<map> float32 [H, W].  Values repeat within a map (drawn from 12 levels, signed, both zeros among them), so
windows hold ties; all finite - scipy leaves NaN unspecified.  Per map:
  rank_cases_<map> int32 [K, 3] = (size_h, size_w, rank), rank_<map> float32 [K, H, W]: rank_filter at ranks 0, n // 2, 9 n // 10
      and n - 1 of every size of SIZES;
  median_cases_<map> int32 [S, 2] = (size_h, size_w), median_<map> float32 [S, H, W]: median_filter of every size.
For the maps of PCT_MAPS also
  pct_cases_<map> float64 [P, 4] = (size_h, size_w, percentile, the rank scipy's formula gives), pct_<map> float32 [P, H, W]:
      percentile_filter at the percentiles of PERCENTILES for the sizes of PCT_SIZES."""
from pathlib import Path

import numpy as np
from scipy import ndimage

MAPS = {"h1w1": (1, 1), "h1w7": (1, 7), "h7w1": (7, 1), "h2w3": (2, 3), "h5w9": (5, 9), "h17w33": (17, 33), "h3w40": (3, 40),
        "h1w9": (1, 9), "h9w1": (9, 1), "h3w2": (3, 2)}
SIZES = [(1, 1), (3, 3), (5, 5), (2, 2), (4, 3), (1, 7), (7, 1), (15, 15), (6, 15), (9, 2), (8, 8), (9, 9), (2, 15), (15, 2)]
PCT_MAPS = ("h2w3", "h5w9", "h3w40")
PCT_SIZES = [(3, 3), (2, 2), (4, 3), (5, 5), (1, 7)]
PERCENTILES = [0, 10, 25, 50, 75, 90, 99.9, 100, -25]


def ranks_of(n):
    return sorted({0, n // 2, 9 * n // 10, n - 1})


def main():
    out = {"names": np.array(list(MAPS))}
    for i, (name, (h, w)) in enumerate(MAPS.items()):
        rng = np.random.default_rng(4600 + i)
        levels = np.concatenate([np.float32([-0.0, 0.0]), (rng.standard_normal(10) * 2.0).astype(np.float32)])
        x = levels[rng.integers(0, 12, (h, w))]
        out[f"x_{name}"] = x
        cases, res, med = [], [], []
        for sh, sw in SIZES:
            for r in ranks_of(sh * sw):
                got = ndimage.rank_filter(x, rank=r, size=(sh, sw), mode="reflect")
                assert got.dtype == np.float32 and got.shape == x.shape
                cases.append((sh, sw, r))
                res.append(got)
            med.append(ndimage.median_filter(x, size=(sh, sw), mode="reflect"))
        out[f"rank_cases_{name}"] = np.array(cases, np.int32)
        out[f"rank_{name}"] = np.stack(res)
        out[f"median_cases_{name}"] = np.array(SIZES, np.int32)
        out[f"median_{name}"] = np.stack(med)
        if name in PCT_MAPS:
            cases, res = [], []
            for sh, sw in PCT_SIZES:
                n = sh * sw
                for p in PERCENTILES:
                    q = p + 100 if p < 0 else p
                    r = n - 1 if q == 100 else int(float(n) * q / 100.0)
                    got = ndimage.percentile_filter(x, p, size=(sh, sw), mode="reflect")
                    assert np.array_equal(got, ndimage.rank_filter(x, rank=r, size=(sh, sw), mode="reflect")), (name, sh, sw, p, r)
                    cases.append((sh, sw, p, r))
                    res.append(got)
            out[f"pct_cases_{name}"] = np.array(cases, np.float64)
            out[f"pct_{name}"] = np.stack(res)
    path = Path(__file__).resolve().parent / "scipy_rank.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
