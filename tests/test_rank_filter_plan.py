"""CPU checks of the rank filters of anomaly maps: the numpy restatement (tests/rank_filter_ref.py - what
the GPU tests compare the kernel with, bit for bit) against scipy's recorded results (tests/golden/rank_filter/scipy_rank.npz,
make_golden_rank_filter.py), its NaN and zero rules, the relations to the grey morphology, the `rank_filter=` spec, and every
refusal of the C ABI that needs no device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import map_morph_ref as morph_ref
import rank_filter_ref as ref

REPO = Path(__file__).resolve().parent.parent
GOLDEN = "rank_filter/scipy_rank.npz"
FRAMES = {"h1w1", "h1w7", "h7w1", "h2w3", "h5w9", "h17w33", "h3w40", "h1w9", "h9w1", "h3w2"}
SIZES = {(1, 1), (3, 3), (5, 5), (2, 2), (4, 3), (1, 7), (7, 1), (15, 15), (6, 15), (9, 2), (8, 8), (9, 9), (2, 15), (15, 2)}
PERCENTILES = [0, 10, 25, 50, 75, 90, 99.9, 100, -25]


def levels_map(seed, h=13, w=17, levels=7):
    """A finite map with many ties: `levels` distinct values, negative ones and both zeros among them."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.float32([-0.0, 0.0]), (rng.standard_normal(levels - 2) * 2).astype(np.float32)])
    return vals[rng.integers(0, levels, (h, w))]


# ------------------------------------------------------------------------------------------ the restatement against scipy
def test_restatement_equals_scipy(golden):
    g = golden(GOLDEN)
    names = [str(n) for n in g["names"]]
    assert set(names) == FRAMES
    checked = 0
    for name in names:
        x = g[f"x_{name}"]
        assert x.dtype == np.float32 and np.isfinite(x).all() and x.shape == tuple(int(v) for v in re.findall(r"\d+", name))
        cases = g[f"rank_cases_{name}"]
        assert {(int(sh), int(sw)) for sh, sw, _ in cases} == SIZES
        for (sh, sw, r), want in zip(cases, g[f"rank_{name}"]):
            n = int(sh) * int(sw)
            assert int(r) in (0, n // 2, 9 * n // 10, n - 1)
            assert np.array_equal(ref.rank_filter(x, (sh, sw), r), want), (name, sh, sw, r)
            if x.size <= 45 and n <= 64:                                     # the per-pixel loop: an independent second form
                assert np.array_equal(ref.loop(x, (sh, sw), int(r)), want), (name, sh, sw, r)
            checked += 1
        for (sh, sw), want in zip(g[f"median_cases_{name}"], g[f"median_{name}"]):
            assert np.array_equal(ref.rank_filter(x, (sh, sw), "median"), want), (name, sh, sw)
            assert np.array_equal(ref.rank_filter(x, (sh, sw), (int(sh) * int(sw)) // 2), want)
            checked += 1
    assert checked >= 10 * 14 * 3


def test_rank_of_percentile_is_scipys(vad, golden):
    g = golden(GOLDEN)
    seen = set()
    for name in ("h2w3", "h5w9", "h3w40"):
        x = g[f"x_{name}"]
        for (sh, sw, p, r), want in zip(g[f"pct_cases_{name}"], g[f"pct_{name}"]):
            sh, sw, r = int(sh), int(sw), int(r)
            assert vad.metrics.rank_of_percentile(sh * sw, float(p)) == r == ref.rank_of_percentile(sh * sw, float(p)), (sh, sw, p)
            assert np.array_equal(ref.rank_filter(x, (sh, sw), r), want), (name, sh, sw, p)
            assert vad.metrics.rank_filter_steps(("percentile", (sh, sw), float(p))) == (((sh, sw), r),)
            seen.add(float(p))
    assert seen == {float(p) for p in PERCENTILES}
    rp = vad.metrics.rank_of_percentile
    assert [rp(9, p) for p in (0, 50, 100, -100, -50, 99.9)] == [0, 4, 8, 0, 4, 8] and rp(4, 50) == 2 and rp(1, 37.5) == 0
    assert rp(225, 90) == 202 and rp(25, np.float32(90.0)) == 22 and rp(np.int64(25), 10) == 2
    for bad in (100.5, -100.5, 101, float("nan"), "50", None, True):
        with pytest.raises(vad.hip.VadError, match="p must be a number in -100..100"):
            rp(9, bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(vad.hip.VadError, match="n must be an int >= 1"):
            rp(bad, 50)


def test_nan_and_signed_zeros_are_specified():
    x = np.full((9, 11), 0.5, np.float32)
    x[0, 10] = x[6, 3] = np.nan
    for size, rank in (((3, 2), 0), ((3, 2), 3), ((3, 2), 5), (5, 12), ((4, 15), 30)):
        got = ref.rank_filter(x, size, rank)
        want = ref.nan_footprint(9, 11, [(0, 10), (6, 3)], size)
        assert np.array_equal(np.isnan(got), want) and (got[~want] == 0.5).all(), (size, rank)
    # the corner NaN at (0, 10): size 5 sees it from rows 0..2 and columns 8..10; size 2 (windows [i - 1, i]) from rows 0..1 of column 10
    assert ref.nan_footprint(9, 11, [(0, 10)], 5).sum() == 9 and ref.nan_footprint(9, 11, [(0, 10)], 2).sum() == 2
    z = np.float32([[0.0, -0.0, 0.0, 0.0, 0.0]])
    assert np.signbit(ref.rank_filter(z, (1, 3), 0)).tolist() == [[True, True, True, False, False]]
    assert np.signbit(ref.rank_filter(z, (1, 3), 1)).tolist() == [[False, False, False, False, False]]
    assert np.signbit(ref.rank_filter(-z, (1, 3), 1)).tolist() == [[True, True, True, True, True]]
    assert np.signbit(ref.rank_filter(-z, (1, 3), 2)).tolist() == [[False, False, False, True, True]]
    assert ref.same_bits(z, z) and not ref.same_bits(z, -z)
    inf = np.float32([[1, np.inf, 2, -np.inf, 3]])
    assert ref.rank_filter(inf, (1, 3), 1).tolist() == [[1, 2, 2, 2, 3]]
    assert ref.rank_filter(inf, (1, 3), 0).tolist() == [[1, 1, -np.inf, -np.inf, -np.inf]]
    den = np.float32([[1e-45, -1e-45, 0.0, 3e-45, -0.0]])
    assert ref.same_bits(ref.rank_filter(den, (1, 5), 2)[:, 2], np.float32([0.0]))
    assert ref.same_bits(ref.rank_filter(den, (1, 5), 1)[:, 2], np.float32([-0.0]))
    assert ref.same_bits(ref.rank_filter(x, 1, 0), x)                        # size 1 is a copy, NaN included


@pytest.mark.parametrize("size", [1, 2, 3, 5, (4, 3), (1, 7), (7, 1), 8, 9, 15, (2, 15), (15, 2)], ids=str)
def test_end_ranks_are_erosion_and_dilation(size):
    """Rank 0 is grey_erosion at every size; rank n - 1 is grey_dilation at odd sizes only (scipy's dilation mirrors the origin of
    an even element).  On a frame smaller than the window too: the reflected duplicates change no minimum and no maximum."""
    sh, sw = ref.pair(size)
    for x in (levels_map(41), levels_map(42, 3, 4)):
        assert ref.same_bits(ref.rank_filter(x, size, 0), morph_ref.erode(x, size))
        top = ref.rank_filter(x, size, sh * sw - 1)
        if sh % 2 and sw % 2:
            assert ref.same_bits(top, morph_ref.dilate(x, size))
    one = np.zeros((13, 17), np.float32)
    one[6, 8] = 1.0                                                          # a single bright pixel shows which way an even window leans
    assert ref.same_bits(ref.rank_filter(one, size, sh * sw - 1), morph_ref.dilate(one, size)) == bool(sh % 2 and sw % 2)
    ys, xs = np.nonzero(ref.rank_filter(one, size, sh * sw - 1))
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (max(0, 6 - (sh - 1) // 2), min(12, 6 + sh // 2), 8 - (sw - 1) // 2, 8 + sw // 2)


def test_commutes_with_the_threshold_and_batches():
    x = levels_map(11)
    ties = np.unique(x)
    for size, rank in ((3, 4), ((4, 3), 6), (5, 22), ((1, 7), 0), (2, 2)):
        y = ref.rank_filter(x, size, rank)
        for t in (ties[0] - 1, ties[2], (ties[2] + ties[3]) / 2, ties[-1], ties[-1] + 1):
            assert np.array_equal(y >= t, ref.rank_filter((x >= t).astype(np.float32), size, rank) > 0), (size, rank, t)
    whole = np.stack([levels_map(31), levels_map(32)])[:, None]              # leading axes are batch axes
    assert ref.same_bits(ref.rank_filter(whole, 3, "median")[1, 0], ref.rank_filter(levels_map(32), 3, 4))
    steps = (((3, 3), 4), ((1, 5), 0))
    assert ref.same_bits(ref.apply(x, steps), ref.rank_filter(ref.rank_filter(x, 3, 4), (1, 5), 0))


def test_a_median_removes_impulses_and_keeps_edges():
    x = np.zeros((12, 12), np.float32)
    x[:, 6:] = 1.0                                                           # a step edge
    x[3, 2], x[8, 9] = 5.0, -5.0                                             # two impulses
    y = ref.rank_filter(x, 3, "median")
    want = np.zeros((12, 12), np.float32)
    want[:, 6:] = 1.0
    assert np.array_equal(y, want)


# ------------------------------------------------------------------------------------------ the spec
def test_rank_filter_steps_normalises_and_refuses(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    assert m.RANKFILT_MAX_SIZE == vad.hip.RANKFILT_MAX_SIZE == 15 and m.RANKFILT_MAX_STEPS == 4
    assert m.rank_filter_steps(None) == ()
    assert m.rank_filter_steps(("median", 3)) == (((3, 3), 4),)
    assert m.rank_filter_steps(("median", (2, 2))) == (((2, 2), 2),)         # the upper median of an even window
    assert m.rank_filter_steps(("median", (3, 5))) == (((3, 5), 7),)
    assert m.rank_filter_steps(("percentile", 5, 90)) == (((5, 5), 22),)
    assert m.rank_filter_steps(("percentile", (4, 3), -25)) == (((4, 3), 9),)
    assert m.rank_filter_steps(("rank", 3, 0)) == (((3, 3), 0),)
    assert m.rank_filter_steps([("median", 3), ["rank", [15, 1], np.int64(14)]]) == (((3, 3), 4), ((15, 1), 14))
    assert m.rank_filter_steps([("median", np.int64(15))] * 4) == (((15, 15), 112),) * 4
    for bad in ([], [("median", 3)] * 5, "median", ("median",), ("median", 3, 3), ("rank", 3), ("percentile", 3), 3, (None, 3),
                [("median", 3), "median"], [("median",)], ("rank", 3, 1, 1)):
        with pytest.raises(VadError, match="step"):
            m.rank_filter_steps(bad)
    for bad in (("mean", 3), ("MEDIAN", 3), [(None, 3)], [(3, "median")], ("open", 3)):
        with pytest.raises(VadError, match="kind must be one of"):
            m.rank_filter_steps(bad)
    for bad in (0, 16, -1, (3, 0), (16, 3), 2.0, True, (3,), (3, 3, 3), "3", None):
        with pytest.raises(VadError, match="size"):
            m.rank_filter_steps(("median", bad))
    for bad in (-1, 9, 2.0, True, None, "median"):
        with pytest.raises(VadError, match=r"rank must be an int in 0\.\.8"):
            m.rank_filter_steps(("rank", 3, bad))
    for bad in (100.5, -101, float("nan"), "50", None, True):
        with pytest.raises(VadError, match="a percentile must be a number in -100..100"):
            m.rank_filter_steps(("percentile", 3, bad))
    # the morphology and temporal specs do not learn the word
    with pytest.raises(VadError, match="op must be one of"):
        m.morph_steps(("median", 3))
    with pytest.raises(VadError, match="op must be one of"):
        m.temporal_steps(("median", 3))


def test_host_refusals(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(VadError, match="no CPU fallback"):
        m.rank_filter_maps(x, 3)
    with pytest.raises(VadError, match=r"maps \(cpu\) must be on the GPU"):
        m.apply_rank_filter(x, m.rank_filter_steps(("median", 3)))
    with pytest.raises(VadError, match="torch tensor"):
        m.rank_filter_maps(np.zeros((16, 16), np.float32), 3)
    with pytest.raises(VadError, match="size must be in 1..15"):
        m.rank_filter_maps(x, 16)
    with pytest.raises(VadError, match="size must be an int or"):
        m.rank_filter_maps(x, 2.5)
    with pytest.raises(VadError, match="rank must be 'median' or an int"):
        m.rank_filter_maps(x, 3, "mean")
    for bad in (9, -1, 2.0, True):
        with pytest.raises(VadError, match=r"rank must be an int in 0\.\.8"):
            m.rank_filter_maps(x, 3, bad)
    assert m.apply_rank_filter(x, ()) is x
    # the scoring entry points refuse a bad spec before they score anything (no model, no device needed)
    s = vad.scoring
    img, clip = torch.zeros(1, 3, 16, 16), torch.zeros(1, 2, 3, 16, 16)
    tracker = object()
    for call in (lambda: s.pixel_auroc(None, [], "cpu", rank_filter=("median", 0)),
                 lambda: s.pixel_aupro(None, [], "cpu", rank_filter=("blur", 3)),
                 lambda: s.detection_report(None, [], "cpu", 0.5, rank_filter=("rank", 3, 9)),
                 lambda: s.frame_scores(None, img, "max", rank_filter=[]),
                 lambda: s.frame_auroc(None, [], "cpu", reduce="max", rank_filter=("percentile", 3, 101)),
                 lambda: s.frame_auroc(None, [], "cpu", rank_filter=("median", 16)),
                 lambda: s.compute_auroc_maps(None, [], "cpu", rank_filter=("median", 16)),
                 lambda: s.localize(None, img, 0.5, rank_filter=[]),
                 lambda: s.localize_events(None, clip, 0.5, rank_filter=("median", 16)),
                 lambda: s.localize_stream(None, clip, tracker, rank_filter=("median", (3, 3, 3)))):
        with pytest.raises(VadError, match="rank_filter_steps"):
            call()
    with pytest.raises(VadError, match="rank_filter= filters the error maps before they are reduced"):
        s.frame_auroc(None, [], "cpu", rank_filter=("median", 3))


def test_the_keyword_is_trailing_and_keyword_only(vad):
    s = vad.scoring
    for name in ("_anomaly_maps", "pixel_auroc", "pixel_aupro", "detection_report", "frame_scores", "frame_auroc", "compute_auroc_maps",
                 "localize", "localize_events", "localize_stream"):
        params = list(inspect.signature(getattr(s, name)).parameters.values())
        assert params[-1].name == "rank_filter" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default is None, name
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:-1]), name     # positional call sites keep working
    assert "rank_filter" not in inspect.signature(s.calibrate).parameters


class _CpuModel:
    """Stands where a model stands: its maps are CPU tensors, so the filter's own device check is what answers."""
    def score_all(self, images):
        return {"errmap": torch.zeros(images.shape[0], 1, 16, 16)}


def test_the_keyword_is_refused_on_cpu_tensors(vad):
    s, VadError = vad.scoring, vad.hip.VadError
    img = torch.zeros(2, 3, 16, 16)
    with pytest.raises(VadError, match=r"rank_filter_maps: maps \(cpu\) must be on the GPU \(the rank filter runs on the device; there is no CPU fallback\)"):
        s.localize(_CpuModel(), img, 0.5, rank_filter=("median", 3))
    with pytest.raises(VadError, match=r"rank_filter_maps: maps \(cpu\) must be on the GPU"):
        s.frame_scores(_CpuModel(), img, "max", rank_filter=[("rank", (1, 3), 2), ("median", 3)])
    with pytest.raises(VadError, match=r"morph_maps: maps \(cpu\) must be on the GPU"):     # the wording it mirrors
        s.localize(_CpuModel(), img, 0.5, morph=("open", 3))


# ------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_c_abi_refusals_need_no_device(vad):
    """Every argument check of vad_rankfilt_maps comes before anything is launched: with pointers that are never followed."""
    lib = vad.hip.lib()
    maps, out = 0x10000, 0x90000                                             # 2 KiB of maps at most below
    call = lambda *a: lib.vad_rankfilt_maps(*a, None)
    ERR_ARG = -1
    for sh, sw in ((0, 3), (3, 0), (16, 3), (3, 16), (-1, 3)):
        assert call(maps, 2, 16, 16, sh, sw, 0, out) == ERR_ARG and b"rankfilt_maps: size must be in 1..15" in lib.vad_last_error(), (sh, sw)
    for sh, sw, r in ((3, 3, -1), (3, 3, 9), (1, 1, 1), (15, 15, 225), (2, 3, 6)):
        assert call(maps, 2, 16, 16, sh, sw, r, out) == ERR_ARG and b"rank must be in 0.." in lib.vad_last_error(), (sh, sw, r)
    assert b"rank must be in 0..5 (a window of 2x3), got 6" in lib.vad_last_error()
    assert call(maps, -1, 16, 16, 3, 3, 4, out) == ERR_ARG and b"negative" in lib.vad_last_error()
    for h, w in ((0, 16), (16, 0), (-4, 16)):
        assert call(maps, 2, h, w, 3, 3, 4, out) == ERR_ARG and b"must be positive" in lib.vad_last_error(), (h, w)
    assert call(maps, 2, 4096, 4096, 3, 3, 4, out) == ERR_ARG and b"pixels per frame" in lib.vad_last_error()
    assert call(maps, 1 << 50, 2048, 2048, 3, 3, 4, out) == ERR_ARG and b"not representable" in lib.vad_last_error()
    assert call(None, 2, 16, 16, 3, 3, 4, out) == ERR_ARG and b"NULL" in lib.vad_last_error()
    assert call(maps, 2, 16, 16, 3, 3, 4, None) == ERR_ARG and b"NULL" in lib.vad_last_error()
    for a, b in ((maps + 2, out), (maps, out + 1)):
        assert call(a, 2, 16, 16, 3, 3, 4, b) == ERR_ARG and b"aligned" in lib.vad_last_error(), (a, b)
    for a, b in ((maps, maps), (maps, maps + 4), (maps, maps + 2 * 256 * 4 - 4), (maps + 2 * 256 * 4 - 4, maps)):
        for sh, sw, r in ((1, 1, 0), (3, 3, 4)):                             # size 1 x 1 included: a copy, but never in place
            assert call(a, 2, 16, 16, sh, sw, r, b) == ERR_ARG and b"overlaps" in lib.vad_last_error(), (a, b)
    assert b"rankfilt_maps" in lib.vad_last_error()
    for sh, sw, r in ((1, 1, 0), (3, 3, 4), (15, 15, 224), (2, 15, 0)):
        assert call(maps, 0, 16, 16, sh, sw, r, out) == 0                    # n == 0: VAD_OK, nothing launched
    assert call(maps, 0, 16, 16, 3, 3, 4, maps + 2 * 256 * 4) == 0           # adjacent, not overlapping


def test_tile_answers_for_every_size(vad):
    lib = vad.hip.lib()
    th, tw = C.c_int(), C.c_int()
    for sh in range(1, 16):
        for sw in range(1, 16):
            th.value = tw.value = 0
            assert lib.vad_rankfilt_tile(sh, sw, C.byref(th), C.byref(tw)) == 0
            assert 8 <= th.value <= 256 and 8 <= tw.value <= 256, (sh, sw, th.value, tw.value)
    assert lib.vad_rankfilt_tile(3, 3, None, None) == 0
    for sh, sw in ((0, 3), (3, 16), (16, 16), (3, -1)):
        assert lib.vad_rankfilt_tile(sh, sw, C.byref(th), C.byref(tw)) == -1 and b"rankfilt_tile: size must be in 1..15" in lib.vad_last_error()


def test_header_and_signatures_agree(vad):
    hip = vad.hip
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "vad_hip.h").read_text(), flags=re.S)
    lib = hip.lib()
    for name, nargs in {"vad_rankfilt_maps": 9, "vad_rankfilt_tile": 4}.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, header, flags=re.S)
        assert decl, f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+VAD_RANKFILT_MAX_SIZE\s+15\b", header)
    assert "map_rankfilt.hip" in hip.SOURCES and (hip.CSRC / "map_rankfilt.hip").exists()
    text = (hip.CSRC / "map_rankfilt.hip").read_text()
    assert "vad_req_map_dims" in text and "vad_disjoint" in text and "vad_aligned" in text      # the shared checks, no copies
    assert "map_rankfilt.hip" not in inspect.getsource(hip.build).split("extra = ")[1].split("}")[0]   # selects only: no -ffp-contract=off
