"""numpy restatement of the order statistics and top-k means of anomaly maps (`vad_map_topk`,
csrc/map_topk.hip): what the GPU tests compare the kernel with - `kth` bit for bit, `mean` within `mean_bound`.

Pixels are ordered by the monotone key of their bits, a STABLE sort by key decides every tie (-0.0 below +0.0).  Rank k is the k-th
largest.  The top-k mean is exact: `math.fsum` over the k largest pixels as doubles, one division, rounded once to float32.  A frame
with a NaN pixel is the canonical quiet NaN in every output."""
import math
from fractions import Fraction

import numpy as np

QNAN_BITS = 0x7FC00000
MAX_RANKS = 8


def key(x):
    """uint32 keys of float32 values: bits ^ (sign ? 0xFFFFFFFF : 0x80000000); unsigned order = -inf < .. < -0 < +0 < .. < +inf."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def descending(frame):
    """The frame's pixels from the largest key to the smallest (float32 [P], bits unchanged)."""
    flat = np.ascontiguousarray(frame, np.float32).reshape(-1)
    return flat[np.argsort(key(flat), kind="stable")[::-1]]


def spacing32(v):
    """The gap between float32 neighbours at |v| (v a float64 scalar that float32 can hold; the smallest denormal below that)."""
    f = np.float32(v)
    return float(np.spacing(np.abs(f))) if np.isfinite(f) else float("inf")


def frame_topk(frame, ranks):
    """One frame -> (kth float32 [nk], mean float32 [nk], exact float64 [nk], bound float64 [nk]).  `exact` is the top-k mean before
    its rounding to float32 (fsum / k, itself rounded once to double); `bound` is how far a float64 sum in any order, divided and
    rounded to float32, may lie from it: 0.5 * spacing32(exact) + P * 2^-52 * mean(|top k|)."""
    flat = np.ascontiguousarray(frame, np.float32).reshape(-1)
    nk = len(ranks)
    if np.isnan(flat).any():
        nan = np.full(nk, QNAN_BITS, np.uint32).view(np.float32)
        return nan, nan.copy(), np.full(nk, np.nan), np.zeros(nk)
    d = descending(flat)
    kth = np.array([d[k - 1] for k in ranks], np.float32)
    exact, bound = np.empty(nk), np.empty(nk)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, k in enumerate(ranks):
            top = d[:k].astype(np.float64)
            if np.isinf(top).any():
                exact[j] = float(top.sum()) / k                               # IEEE decides: +inf, -inf, or NaN for both signs
                bound[j] = 0.0
            else:
                exact[j] = math.fsum(top.tolist()) / k
                bound[j] = 0.5 * spacing32(exact[j]) + flat.size * 2.0 ** -52 * (math.fsum(np.abs(top).tolist()) / k)
        mean = exact.astype(np.float32)
    return kth, mean, exact, bound


def topk(maps, ranks):
    """maps [..., H, W], ranks a list of nk ints -> dict of 'kth', 'mean' float32 [..., nk] and 'exact', 'bound' float64 [..., nk]."""
    maps = np.ascontiguousarray(maps, np.float32)
    lead = maps.shape[:-2]
    frames = maps.reshape((-1,) + maps.shape[-2:])
    rows = [frame_topk(f, list(ranks)) for f in frames]
    return {name: np.stack([r[i] for r in rows]).reshape(lead + (len(ranks),)) if rows else np.zeros(lead + (len(ranks),), np.float32)
            for i, name in enumerate(("kth", "mean", "exact", "bound"))}


def mean_within_bound(got, want):
    """Is a float32 `mean` within the bound of the restatement `want` = topk(...)?  Non-finite exact values must match as such."""
    got = np.asarray(got, np.float64)
    exact, bound = want["exact"], want["bound"]
    finite = np.isfinite(exact)
    ok = np.where(finite, np.abs(got - np.where(finite, exact, 0.0)) <= bound, (got == exact) | (np.isnan(got) & np.isnan(exact)))
    return bool(ok.all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rank_of_fraction(fraction, pixels):
    """min(P, max(1, ceil(fraction * P))), exact rational arithmetic on the float as given."""
    return min(pixels, max(1, math.ceil(Fraction(float(fraction)) * pixels)))


def rank_of_quantile(q, pixels):
    """P - ceil(q * (P - 1)), the product in float64: `kth` at that rank is np.quantile(x, q, method="higher")."""
    return pixels - int(math.ceil(float(np.float64(q) * np.float64(pixels - 1))))
