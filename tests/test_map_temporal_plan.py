"""CPU checks of the temporal filters of anomaly maps: the numpy restatement (tests/map_temporal_ref.py -
what the GPU tests compare the kernel with, bit for bit) against scipy's recorded results (tests/golden/temporal/scipy_temporal.npz,
make_golden_temporal.py), its stateful form against the whole-clip form, the properties that let one float kernel serve the whole
detection chain, the derived error bounds of the mean and the exponential average, the `temporal=` spec, and every refusal of the
C ABI that needs no device."""
import ctypes as C
import itertools
import math
from fractions import Fraction
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import map_temporal_ref as ref

REPO = Path(__file__).resolve().parent.parent
GOLDEN = "temporal/scipy_temporal.npz"
OPS = {"min": 0, "max": 1, "mean": 2, "ema": 3}
KS = [1, 2, 3, 4, 7, 8, 16]
U32 = 2.0 ** -24                                  # unit roundoff of float32


def levels_clip(seed, t=11, h=3, w=4, levels=7):
    """A finite clip with many ties: `levels` distinct values, negative ones and both zeros among them."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.float32([-0.0, 0.0]), (rng.standard_normal(levels - 2) * 2).astype(np.float32)])
    return vals[rng.integers(0, levels, (t, h, w))]


def compositions(n):
    """Every way to write n as an ordered sum of positive integers: 2^(n-1) of them."""
    for cuts in itertools.product((False, True), repeat=n - 1):
        parts, run = [], 1
        for c in cuts:
            if c:
                parts.append(run)
                run = 1
            else:
                run += 1
        yield parts + [run]


def test_restatement_equals_scipy(golden):
    g = golden(GOLDEN)
    x = g["x"]
    assert x.dtype == np.float32 and x.shape == (11, 3, 4) and np.isfinite(x).all() and len(np.unique(x)) <= 12
    assert g["ks"].tolist() == KS and KS[-1] > x.shape[0]
    for k in KS:
        assert np.array_equal(ref.temporal("min", x, k), g[f"min_{k}"]), k          # values: scipy leaves the sign of a zero tie open
        assert np.array_equal(ref.temporal("max", x, k), g[f"max_{k}"]), k
    assert ref.same_bits(ref.temporal("min", x, 1), x) and ref.same_bits(ref.temporal("mean", x, 1), x)
    big = float(np.abs(x).max())
    for i, a in enumerate(g["alphas"]):
        assert float(np.float32(a)) == a and 0 < a < 1
        got, want = ref.temporal("ema", x, a).astype(np.float64), g[f"ema_{i}"]
        for t in range(x.shape[0]):
            assert np.abs(got[t] - want[t]).max() <= ema_bound(t, a, big), (a, t)


def ema_bound(t, a, big):
    """|float32 recursion - float64 recursion| after t steps for |x| <= big: a step adds at most
    (4 a + 1) u big - the rounded difference and product, relative 2 u of a * |x - y| <= 2 a big, and the rounded sum, u big - and the
    recursion damps what is there by 1 - a: a geometric sum, at most min(t, 1 / a) steps' worth.  The factor 1 + 2^-19: the average
    stays within big (1 + 4 u), so the second-order terms of a step are at most 15 u of it (2^-20), and the float64 side's own error
    obeys the same bound with 2^-53 for u, 2^-29 of this one (scipy's form (1 - a) y + a x: three times that).  3 * 2^-150 per step:
    the three roundings where a result is subnormal."""
    return min(t, 1.0 / a) * (4 * a + 1) * U32 * big * (1 + 2.0 ** -19) + 3 * t * 2.0 ** -150


@pytest.mark.parametrize("steps", [(("min", 3),), (("max", 2),), (("mean", 4),), (("ema", 0.25),), (("mean", 16),), (("min", 1),),
                                   (("min", 3), ("max", 3)), (("ema", 0.5), ("min", 2), ("mean", 3))])
def test_stateful_equals_whole_clip_for_every_split(steps):
    x = levels_clip(5, t=7)
    x[2, 1, 1] = np.nan
    whole = ref.apply(steps, x)
    n = 0
    for parts in compositions(7):
        s, at, got = ref.Stream(steps), 0, []
        for p in parts:
            got.append(s.update(x[at:at + p]))
            at += p
        assert s.seen == 7 and ref.same_bits(np.concatenate(got), whole), parts
        n += 1
    assert n == 64
    assert ref.same_bits(ref.clips(steps, np.stack([x, x[::-1]]))[1], ref.apply(steps, x[::-1]))


@pytest.mark.parametrize("k", KS)
def test_commutes_with_the_threshold(k):
    """op(x) >= thr is the binary op of x >= thr - what lets the filtered map feed the ranking metrics, the labeller and the tracker.
    Thresholds: below, a TIE value of the map, between two values, the largest value, above."""
    x = levels_clip(11)
    ties = np.unique(x)
    for op in ("min", "max"):
        y = ref.temporal(op, x, k)
        for thr in (ties[0] - 1, ties[2], (ties[2] + ties[3]) / 2, ties[-1], ties[-1] + 1):
            assert np.array_equal(y >= thr, ref.temporal(op, (x >= thr).astype(np.float32), k) > 0), (op, k, thr)


@pytest.mark.parametrize("k", KS)
def test_order_and_the_delayed_opening(k):
    """Min is anti-extensive, max extensive.  The temporal opening [("min", k), ("max", k)] is the morphological opening DELAYED by
    k - 1 frames (both windows look back; the opening's dilation would look ahead), so applying it twice is not the identity on its
    range but one more delay: open(open(x))[t] = open(x)[t - (k - 1)] wherever no window reaches before the stream's first frame."""
    for seed in (21, 22):
        x = levels_clip(seed, t=40)
        lo, hi = ref.temporal("min", x, k), ref.temporal("max", x, k)
        assert (lo <= x).all() and (hi >= x).all() and (ref.temporal("mean", x, k) <= hi).all() and (ref.temporal("mean", x, k) >= lo).all()
        opening = [("min", k), ("max", k)]
        o = ref.apply(opening, x)
        assert (o <= hi).all() and (o[k - 1:] <= x[:len(x) - (k - 1)]).all()                     # anti-extensive, up to the delay
        oo = ref.apply(opening, o)
        first = 4 * (k - 1)
        if first < len(x):
            assert ref.same_bits(oo[first:], o[first - (k - 1):len(x) - (k - 1)]), k
    x = np.float32([0, 1, 1, 0, 0, 0]).reshape(6, 1)                                             # the counter-example to idempotence
    assert ref.apply([("min", 2), ("max", 2)], x).ravel().tolist() == [0, 0, 1, 1, 0, 0]
    assert ref.apply([("min", 2), ("max", 2)] * 2, x).ravel().tolist() == [0, 0, 0, 1, 1, 0]


def test_nan_zeros_and_infinities_are_specified():
    x = np.full((12, 2), 0.5, np.float32)
    x[4, 0] = np.nan
    for op in ("min", "max", "mean"):
        y = ref.temporal(op, x, 3)
        assert np.isnan(y[:, 0]).tolist() == [4 <= t <= 6 for t in range(12)] and not np.isnan(y[:, 1]).any(), op
    assert np.isnan(ref.temporal("ema", x, 0.5)[:, 0]).tolist() == [t >= 4 for t in range(12)]   # stays until the stream is reset
    z = np.float32([0.0, -0.0, 0.0, 0.0, 0.0]).reshape(5, 1)
    assert np.signbit(ref.temporal("min", z, 3)).ravel().tolist() == [False, True, True, True, False]
    assert np.signbit(ref.temporal("max", -z, 3)).ravel().tolist() == [True, False, False, False, True]
    assert np.signbit(ref.temporal("mean", -z, 2)).ravel().tolist() == [True, False, False, True, True]   # -0 + -0 = -0, -0 + +0 = +0
    inf = np.float32([1, np.inf, 2, -np.inf, 3, 4]).reshape(6, 1)
    assert ref.temporal("min", inf, 2).ravel().tolist() == [1, 1, 2, -np.inf, -np.inf, 3]
    assert ref.temporal("max", inf, 2).ravel().tolist() == [1, np.inf, np.inf, 2, 3, 4]
    m = ref.temporal("mean", inf, 3).ravel()
    assert m[1] == np.inf and m[2] == np.inf and np.isnan(m[3]) and m[4] == -np.inf and m[5] == -np.inf


@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e30, 1e-42])
def test_mean_is_within_its_derived_bound(scale):
    """S is c - 1 float64 additions and one division, each within 2^-53 relative: |S / c - m| <= (c + 1) 2^-53 sum|x| / c of the exact
    mean m; the one rounding to float32 adds 2^-24 |m| (2^-150 where the result is subnormal).  Held against the exact mean in
    rational arithmetic, and against math.fsum / c, which is m within one rounding of the sum and one of the division: two more
    units."""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((20, 6)) * scale).astype(np.float32)
    for k in (1, 2, 3, 5, 8, 16):
        y = ref.temporal("mean", x, k)
        for t in range(x.shape[0]):
            for p in range(x.shape[1]):
                win = [float(v) for v in x[max(0, t - k + 1):t + 1, p]]
                c = len(win)
                exact = sum(Fraction(v) for v in win) / c
                mag = sum(Fraction(abs(v)) for v in win) / c
                assert abs(Fraction(float(y[t, p])) - exact) <= Fraction(2) ** -24 * abs(exact) + Fraction(2) ** -150 + (c + 1) * Fraction(2) ** -53 * mag, (k, t, p)
                m = math.fsum(win) / c
                bound = U32 * abs(m) + 2.0 ** -150 + (c + 3) * 2.0 ** -53 * math.fsum(abs(v) for v in win) / c
                assert abs(float(y[t, p]) - m) <= bound, (k, t, p)


def test_ema_is_within_its_derived_bound_and_keeps_a_constant():
    rng = np.random.default_rng(8)
    for scale in (1.0, 1e-20, 1e20):
        x = (rng.standard_normal((60, 5)) * scale).astype(np.float32)
        big = float(np.abs(x).max())
        for alpha in (0.5, 0.1, 0.9, 1e-3, 0.999):
            a = float(np.float32(alpha))
            y = ref.temporal("ema", x, alpha).astype(np.float64)
            want = x[0].astype(np.float64)
            for t in range(1, len(x)):
                want = want + a * (x[t].astype(np.float64) - want)
                assert np.abs(y[t] - want).max() <= ema_bound(t, a, big), (scale, alpha, t)
    for v in (0.1, -3.7e-5, 1e30, -3.4e38, 1e-42, 0.0):                      # x - y = +0, a * 0 = +0, y + 0 = y: every finite constant
        c = np.full((30, 3), v, np.float32)
        for alpha in (0.1, 0.5, 0.999):
            assert ref.same_bits(ref.temporal("ema", c, alpha), c), (v, alpha)
    # the two constants the arithmetic does not keep: -0 - -0 = +0 and -0 + +0 = +0; Inf - Inf = NaN (it follows the arithmetic)
    z = ref.temporal("ema", np.full((4, 1), -0.0, np.float32), 0.5).ravel()
    assert (z == 0).all() and np.signbit(z).tolist() == [True, False, False, False]
    i = ref.temporal("ema", np.full((4, 1), np.inf, np.float32), 0.5).ravel()
    assert i[0] == np.inf and np.isnan(i[1:]).all()


def test_temporal_steps_normalises_and_refuses(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    assert m.temporal_steps(None) == ()
    assert m.temporal_steps(("min", 3)) == (("min", 3),)
    assert m.temporal_steps([("min", 3), ["max", np.int64(3)]]) == (("min", 3), ("max", 3))
    assert m.temporal_steps(("ema", 0.1)) == (("ema", float(np.float32(0.1))),)
    assert m.temporal_steps([("mean", 16)] * 4) == (("mean", 16),) * 4
    assert m.TEMPORAL_MAX_K == vad.hip.TFILT_MAX_K == 16 and m.TEMPORAL_OPS == ("min", "max", "mean", "ema")
    for bad in ([], [("min", 2)] * 5, "min", ("min",), ("min", 3, 3), 3, (None, 3), [("min", 2), "max"], [("min",)]):
        with pytest.raises(VadError, match="step"):
            m.temporal_steps(bad)
    for bad in (("median", 3), ("MIN", 3), [(None, 3)], [(3, "min")]):
        with pytest.raises(VadError, match="op must be one of"):
            m.temporal_steps(bad)
    for bad in (0, 17, -1, 2.0, True, (3,), "3", None):
        with pytest.raises(VadError, match="k must be an int in 1..16"):
            m.temporal_steps(("mean", bad))
    for bad in (0, 0.0, 1, 1.0, -0.5, float("nan"), 1 - 1e-12, 1e-50, "0.5", None, True):           # float32(1 - 1e-12) is 1, float32(1e-50) is 0
        with pytest.raises(VadError, match="alpha must be"):
            m.temporal_steps(("ema", bad))


def test_host_refusals(vad):
    m, s, VadError = vad.metrics, vad.scoring, vad.hip.VadError
    x = torch.zeros(2, 5, 16, 16)
    with pytest.raises(VadError, match="no CPU fallback"):
        m.temporal_maps(x, "min", 3)
    with pytest.raises(VadError, match="torch tensor"):
        m.temporal_maps(np.zeros((2, 5, 16, 16), np.float32), "min", 3)
    with pytest.raises(VadError, match="op must be one of"):
        m.temporal_maps(x, "median", 3)
    with pytest.raises(VadError, match="k must be an int in 1..16"):
        m.temporal_maps(x, "max", 17)
    with pytest.raises(VadError, match="alpha must be"):
        m.temporal_maps(x, "ema", 1.0)
    with pytest.raises(VadError, match="no CPU fallback"):
        m.apply_temporal(x, m.temporal_steps(("mean", 2)))
    assert m.apply_temporal(x, ()) is x
    for bad, text in ((dict(steps=None), "at least one step"), (dict(steps=("min", 0)), "k must be"), (dict(streams=-1), "streams must be"),
                      (dict(h=0), "h must be"), (dict(h=4096, w=4096), "out of range"), (dict(device="cpu"), "must be a GPU")):
        args = dict(streams=2, h=16, w=16, steps=("min", 2))
        args.update(bad)
        with pytest.raises(VadError, match=text):
            m.TemporalFilter(**args)
    # the scoring entry points refuse a bad spec, or a filter that is none, before they score anything (no model, no device needed)
    img = torch.zeros(1, 3, 16, 16)
    for call in (lambda: s.pixel_auroc(None, [], "cpu", temporal=("min", 0)), lambda: s.pixel_aupro(None, [], "cpu", temporal=("blur", 3)),
                 lambda: s.detection_report(None, [], "cpu", 0.5, temporal=[]), lambda: s.frame_scores(None, img, "max", temporal=("ema", 1.0)),
                 lambda: s.frame_auroc(None, [], "cpu", reduce="max", temporal="min"),
                 lambda: s.localize_events(None, img, 0.5, temporal_filter=("max", 2.5))):
        with pytest.raises(VadError, match="temporal_steps"):
            call()
    with pytest.raises(VadError, match="needs a reduce|pass a reduce"):
        s.frame_auroc(None, [], "cpu", temporal=("min", 2))
    with pytest.raises(VadError, match="temporal_filter must be a metrics.TemporalFilter"):
        s.localize_stream(None, img, None, temporal_filter=("min", 2))


def test_image_batches_are_refused_with_a_temporal_filter(vad):
    """[B,C,H,W] is not a sequence: refused before the model is asked for anything."""
    s, VadError = vad.scoring, vad.hip.VadError
    img = torch.zeros(2, 3, 16, 16)
    batch = [{"image": img, "mask": torch.zeros(2, 1, 16, 16), "label": [0, 0], "defect_type": ["a", "a"]}]
    for call in (lambda: s.frame_scores(None, img, "max", temporal=("min", 2)), lambda: s.localize_events(None, img, 0.5, temporal_filter=("min", 2)),
                 lambda: s.pixel_auroc(None, batch, "cpu", hist=SimpleNamespace(accumulate=None), temporal=("min", 2)),
                 lambda: s.pixel_aupro(None, batch, "cpu", hist=SimpleNamespace(accumulate=None), temporal=("min", 2)),
                 lambda: s.detection_report(None, batch, "cpu", 0.5, counts=vad.metrics.DetectionCounts("cpu"), temporal=("min", 2))):
        with pytest.raises(VadError, match="are not consecutive"):
            call()


def test_c_abi_refusals_need_no_device(vad):
    """Every argument check of vad_tfilt_maps / vad_tfilt_init comes before anything is launched.  The pointers are made up, so no
    call here may get as far as a launch - with or without a device: every call either has a bad argument or has b == 0 or t == 0."""
    lib = vad.hip.lib()
    maps, out, state = 0x10000, 0x90000, 0x200000                             # 2 x 3 x 16 x 16 floats = 6 KiB of maps below
    call = lambda m=maps, b=2, t=3, h=16, w=16, op=0, k=3, alpha=0.5, st=state, o=out: lib.vad_tfilt_maps(m, b, t, h, w, op, k, alpha, st, o, None)
    init = lambda st=state, b=2, h=16, w=16, op=0, k=3: lib.vad_tfilt_init(st, b, h, w, op, k, None)
    ERR_ARG = -1
    err = lambda: lib.vad_last_error()
    for op in (-1, 4, 99):
        assert call(op=op) == ERR_ARG and b"unknown op" in err(), op
        assert init(op=op) == ERR_ARG and b"unknown op" in err(), op
        assert lib.vad_tfilt_state_bytes(2, 16, 16, op, 3) == 0
    for op in (0, 1, 2):
        for k in (0, 17, -1):
            assert call(op=op, k=k) == ERR_ARG and b"k must be in 1..16" in err(), (op, k)
            assert init(op=op, k=k) == ERR_ARG and b"k must be in 1..16" in err(), (op, k)
            assert lib.vad_tfilt_state_bytes(2, 16, 16, op, k) == 0
    for alpha in (float("nan"), 0.0, 1.0, -0.5, 1.5, float("inf")):
        assert call(op=3, alpha=alpha) == ERR_ARG and b"alpha must be" in err(), alpha
    for op in (0, 1, 2):                                                     # alpha belongs to the ema alone (t = 0: every check runs, no launch)
        assert call(op=op, alpha=float("nan"), t=0) == 0 and call(op=op, alpha=7.0, b=0) == 0
    assert call(op=3, k=0, t=0) == 0 and call(op=3, k=99, b=0) == 0           # and k to the others
    for b in (-1, 2 ** 20 + 1):
        assert call(b=b) == ERR_ARG and b"b must be in 0..2^20" in err()
        assert init(b=b) == ERR_ARG and b"b must be in 0..2^20" in err()
        assert lib.vad_tfilt_state_bytes(b, 16, 16, 0, 3) == 0
    assert call(t=-1) == ERR_ARG and b"negative" in err()
    for h, w in ((0, 16), (16, 0), (-4, 16)):
        assert call(h=h, w=w) == ERR_ARG and b"must be positive" in err(), (h, w)
        assert init(h=h, w=w) == ERR_ARG and b"must be positive" in err(), (h, w)
        assert lib.vad_tfilt_state_bytes(2, h, w, 0, 3) == 0
    assert call(h=4096, w=4096) == ERR_ARG and b"pixels per frame" in err()
    assert init(h=4096, w=4096) == ERR_ARG and b"pixels per frame" in err()
    assert lib.vad_tfilt_state_bytes(2, 4096, 4096, 0, 3) == 0
    assert call(b=2 ** 20, t=2 ** 30, h=2048, w=2048) == ERR_ARG and b"not representable" in err()
    assert call(m=None) == ERR_ARG and b"NULL" in err()
    assert call(o=None) == ERR_ARG and b"NULL" in err()
    assert init(st=None) == ERR_ARG and b"NULL" in err()
    for kw in (dict(m=maps + 2), dict(o=out + 1), dict(st=state + 8), dict(st=state + 4)):
        assert call(**kw) == ERR_ARG and b"aligned" in err(), kw
    assert init(st=state + 8) == ERR_ARG and b"aligned" in err()
    total = 2 * 3 * 256 * 4
    for a, b in ((maps, maps), (maps, maps + 4), (maps, maps + total - 4), (maps + total - 4, maps)):
        for op in range(4):                                                  # k = 1 included: a copy, but never in place
            assert call(m=a, o=b, op=op, k=1) == ERR_ARG and b"overlaps" in err(), (a, b)
    for op in range(4):                                                      # b == 0 or t == 0: VAD_OK, nothing launched
        assert call(b=0, op=op) == 0 and call(t=0, op=op) == 0 and call(t=0, op=op, st=None) == 0
    assert init(b=0) == 0
    assert call(t=0, o=maps + total) == 0                                    # adjacent, not overlapping


def test_state_sizes_and_plan(vad):
    lib = vad.hip.lib()
    size = lib.vad_tfilt_state_bytes
    hdr = 4 * vad.hip.TFILT_HEADER_WORDS
    assert hdr == 64
    for b in (0, 1, 3):
        for h, w in ((1, 1), (3, 5), (8, 8), (40, 52)):
            plane = 4 * ((h * w + 3) // 4 * 4)                               # planes are padded to 16 bytes
            for op in (0, 1, 2):
                for k in range(1, 17):
                    assert size(b, h, w, op, k) == b * (hdr + (k - 1) * plane), (b, h, w, op, k)
            for k in (0, 1, 99, -5):                                         # the ema has one plane; k is not its argument
                assert size(b, h, w, 3, k) == b * (hdr + plane)
    assert size(1, 2896, 2896, 0, 16) > 0 and size(2 ** 20, 16, 16, 0, 2) == 2 ** 20 * (hdr + 1024)
    threads, lanes = C.c_int(), C.c_int()
    assert lib.vad_tfilt_plan(C.byref(threads), C.byref(lanes)) == 0 and threads.value in (64, 128, 256, 512, 1024) and lanes.value == 4
    assert lib.vad_tfilt_plan(None, C.byref(lanes)) == -1 and b"NULL" in lib.vad_last_error()


def test_header_and_signatures_agree(vad):
    hip = vad.hip
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "vad_hip.h").read_text(), flags=re.S)
    lib = hip.lib()
    for name, nargs in {"vad_tfilt_state_bytes": 5, "vad_tfilt_init": 7, "vad_tfilt_maps": 11, "vad_tfilt_plan": 2}.items():
        decl = re.search(r"\b(?:int|size_t)\s+%s\s*\((.*?)\);" % name, header, flags=re.S)
        assert decl, f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+VAD_TFILT_MAX_K\s+16\b", header)
    assert re.search(r"enum\s*\{\s*VAD_TFILT_MIN\s*=\s*0,\s*VAD_TFILT_MAX\s*=\s*1,\s*VAD_TFILT_MEAN\s*=\s*2,\s*VAD_TFILT_EMA\s*=\s*3\s*\}", header)
    assert hip.TFILT_OPS == OPS and re.search(r"#define\s+VAD_ABI_VERSION\s+3\b", header) and hip.ABI_VERSION == 3
    assert "map_temporal.hip" in hip.SOURCES and (hip.CSRC / "map_temporal.hip").exists()
    build = (hip.PKG_DIR / "hip.py").read_text()
    assert re.search(r'"map_temporal\.hip":\s*\["-ffp-contract=off"\]', build)         # the ema's product and sum round on their own
