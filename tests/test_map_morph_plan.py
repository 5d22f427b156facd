"""CPU checks of the grey morphology of anomaly maps: the numpy restatement (tests/map_morph_ref.py - what
the GPU tests compare the kernel with, bit for bit) against scipy's recorded results (tests/golden/morph/scipy_grey.npz,
make_golden_morph.py), the properties that make one float kernel serve the whole detection chain (it commutes with the threshold),
the `morph=` spec, and every refusal of the C ABI that needs no device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import map_morph_ref as ref

REPO = Path(__file__).resolve().parent.parent
GOLDEN = "morph/scipy_grey.npz"
OPS = {"erode": 0, "dilate": 1, "open": 2, "close": 3}
SIZES = [1, 2, 3, 4, 5, (1, 5), (5, 1), (4, 3), (6, 5), (7, 7)]


def levels_map(seed, h=13, w=17, levels=7):
    """A finite map with many ties: `levels` distinct values, negative ones and both zeros among them."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.float32([-0.0, 0.0]), (rng.standard_normal(levels - 2) * 2).astype(np.float32)])
    return vals[rng.integers(0, levels, (h, w))]


def test_restatement_equals_scipy(golden):
    g = golden(GOLDEN)
    names = [str(n) for n in g["names"]]
    assert {(int(sh), int(sw)) for _, sh, sw in g["cases"]} == {(2, 2), (3, 3), (4, 3), (1, 5), (7, 7), (6, 5)}
    assert "h3w4" in names and g["x_h3w4"].shape == (3, 4)                   # 7 x 7 and 6 x 5 on it: an element larger than the image
    checked = 0
    for i, sh, sw in g["cases"]:
        x = g[f"x_{names[i]}"]
        assert x.dtype == np.float32 and np.isfinite(x).all()
        for op in ref.OPS:
            want = g[f"{op}_{names[i]}_{sh}x{sw}"]
            assert np.array_equal(ref.morph(op, x, (int(sh), int(sw))), want), (names[i], sh, sw, op)
            assert np.array_equal(ref.loop(op, x, (int(sh), int(sw))), want), (names[i], sh, sw, op)
            checked += 1
    assert checked == 4 * 6 * len(names)


def test_even_sizes_lean_as_scipy_does():
    """Size 2: erode's window is [i - 1, i], dilate's [i, i + 1]; a single bright / dark pixel shows it."""
    x = np.zeros((5, 5), np.float32)
    x[2, 2] = 1
    d = ref.dilate(x, 2)
    assert np.argwhere(d == 1).tolist() == [[1, 1], [1, 2], [2, 1], [2, 2]]
    e = ref.erode(-x, 2)
    assert np.argwhere(e == -1).tolist() == [[2, 2], [2, 3], [3, 2], [3, 3]]
    assert ref.opening(x, 2).max() == 0 and ref.closing(-x, 2).min() == 0    # a single pixel does not survive
    assert np.array_equal(ref.morph("erode", x, 1), x) and np.array_equal(ref.morph("close", x, (1, 1)), x)


def test_nan_and_signed_zeros_are_specified():
    x = np.full((9, 11), 0.5, np.float32)
    x[0, 10] = np.nan
    x[6, 3] = np.nan
    for op in ("erode", "dilate"):
        got = ref.morph(op, x, (3, 2))
        want = np.zeros_like(x, bool)
        for (i, j) in ((0, 10), (6, 3)):                                     # pixel p is NaN iff its window holds the NaN
            (lh, hh), (lw, hw) = ref.reach(3, op == "dilate"), ref.reach(2, op == "dilate")
            want[max(0, i - hh):i + lh + 1, max(0, j - hw):j + lw + 1] = True
        assert np.array_equal(np.isnan(got), want) and (got[~want] == 0.5).all(), op
    both = ref.dilate(np.isnan(ref.erode(x, (3, 2))).astype(np.float32), (3, 2)) > 0     # open: the windows of both steps
    assert np.array_equal(np.isnan(ref.opening(x, (3, 2))), both) and both.sum() > np.isnan(ref.erode(x, (3, 2))).sum()
    z = np.float32([[0.0, -0.0, 0.0, 0.0, 0.0]])
    assert np.signbit(ref.erode(z, (1, 3))).tolist() == [[True, True, True, False, False]]
    assert np.signbit(ref.dilate(z, (1, 3))).tolist() == [[False, False, False, False, False]]
    assert np.signbit(ref.dilate(-z, (1, 3))).tolist() == [[False, False, False, True, True]]
    assert ref.same_bits(z, z) and not ref.same_bits(z, -z)
    inf = np.float32([[1, np.inf, 2, -np.inf, 3]])
    assert ref.erode(inf, (1, 3)).tolist() == [[1, 1, -np.inf, -np.inf, -np.inf]]
    assert ref.dilate(inf, (1, 3)).tolist() == [[np.inf, np.inf, np.inf, 3, 3]]


@pytest.mark.parametrize("size", SIZES)
def test_commutes_with_the_threshold(size):
    """op(x) >= t is the binary op of x >= t - what lets one float kernel serve the ranking metrics, the labeller and the tracker.
    Thresholds: below, between, a TIE value of the map, above."""
    x = levels_map(11)
    ties = np.unique(x)
    for op in ref.OPS:
        y = ref.morph(op, x, size)
        for t in (ties[0] - 1, ties[2], (ties[2] + ties[3]) / 2, ties[-1], ties[-1] + 1):
            assert np.array_equal(y >= t, ref.morph(op, (x >= t).astype(np.float32), size) > 0), (op, size, t)


@pytest.mark.parametrize("size", SIZES)
def test_order_and_idempotence(size):
    for seed in (21, 22):
        x = levels_map(seed)
        o, c = ref.opening(x, size), ref.closing(x, size)
        assert (o <= x).all() and (c >= x).all()                             # open is anti-extensive, close extensive
        assert (ref.erode(x, size) <= o).all() and (c <= ref.dilate(x, size)).all()
        assert ref.same_bits(ref.opening(o, size), o) and ref.same_bits(ref.closing(c, size), c)
    whole = np.stack([levels_map(31), levels_map(32)])[:, None]              # leading axes are batch axes
    assert ref.same_bits(ref.opening(whole, size)[1, 0], ref.opening(levels_map(32), size))


def test_morph_steps_normalises_and_refuses(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    assert m.morph_steps(None) == ()
    assert m.morph_steps(("open", 3)) == (("open", (3, 3)),)
    assert m.morph_steps(("close", (3, 5))) == (("close", (3, 5)),)
    assert m.morph_steps([("open", 2), ["close", [5, 1]]]) == (("open", (2, 2)), ("close", (5, 1)))
    assert m.morph_steps([("erode", np.int64(31))] * 4) == (("erode", (31, 31)),) * 4
    assert m.MORPH_MAX_SIZE == vad.hip.MORPH_MAX_SIZE == 31 and m.MORPH_OPS == ("erode", "dilate", "open", "close")
    for bad in ([], [("open", 2)] * 5, "open", ("open",), ("open", 3, 3), 3, (None, 3), [("open", 2), "close"], [("open",)]):
        with pytest.raises(VadError, match="step"):
            m.morph_steps(bad)
    for bad in (("opening", 3), ("OPEN", 3), [(None, 3)], [(3, "open")]):
        with pytest.raises(VadError, match="op must be one of"):
            m.morph_steps(bad)
    for bad in (0, 32, -1, (3, 0), (32, 3), 2.0, True, (3,), (3, 3, 3), "3", None):
        with pytest.raises(VadError, match="size"):
            m.morph_steps(("open", bad))


def test_host_refusals(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(VadError, match="no CPU fallback"):
        m.morph_maps(x, "open", 3)
    with pytest.raises(VadError, match="torch tensor"):
        m.morph_maps(np.zeros((16, 16), np.float32), "open", 3)
    with pytest.raises(VadError, match="op must be one of"):
        m.morph_maps(x, "opening", 3)
    with pytest.raises(VadError, match="size must be in 1..31"):
        m.morph_maps(x, "open", 32)
    with pytest.raises(VadError, match="size must be an int or"):
        m.morph_maps(x, "open", 2.5)
    # the scoring entry points refuse a bad spec before they score anything (no model, no device needed)
    s = vad.scoring
    for call in (lambda: s.pixel_auroc(None, [], "cpu", morph=("open", 0)), lambda: s.pixel_aupro(None, [], "cpu", morph=("blur", 3)),
                 lambda: s.localize(None, torch.zeros(1, 3, 16, 16), 0.5, morph=[]),
                 lambda: s.localize_events(None, torch.zeros(1, 3, 16, 16), 0.5, morph=("open", 32))):
        with pytest.raises(VadError, match="morph_steps"):
            call()


def test_c_abi_refusals_need_no_device(vad):
    """Every argument check of vad_morph_maps comes before anything is launched: with pointers that are never followed."""
    lib = vad.hip.lib()
    maps, out = 0x10000, 0x90000                                             # 2 KiB of maps at most below
    call = lambda *a: lib.vad_morph_maps(*a, None)
    ERR_ARG = -1
    for op in (-1, 4, 99):
        assert call(maps, 2, 16, 16, op, 3, 3, out) == ERR_ARG and b"unknown op" in lib.vad_last_error(), op
    for sh, sw in ((0, 3), (3, 0), (32, 3), (3, 32), (-1, 3)):
        assert call(maps, 2, 16, 16, 2, sh, sw, out) == ERR_ARG and b"size must be in 1..31" in lib.vad_last_error(), (sh, sw)
    assert call(maps, -1, 16, 16, 2, 3, 3, out) == ERR_ARG and b"negative" in lib.vad_last_error()
    for h, w in ((0, 16), (16, 0), (-4, 16)):
        assert call(maps, 2, h, w, 2, 3, 3, out) == ERR_ARG and b"must be positive" in lib.vad_last_error(), (h, w)
    assert call(maps, 2, 4096, 4096, 2, 3, 3, out) == ERR_ARG and b"pixels per frame" in lib.vad_last_error()
    assert call(maps, 1 << 50, 2048, 2048, 2, 3, 3, out) == ERR_ARG and b"not representable" in lib.vad_last_error()
    assert call(None, 2, 16, 16, 2, 3, 3, out) == ERR_ARG and b"NULL" in lib.vad_last_error()
    assert call(maps, 2, 16, 16, 2, 3, 3, None) == ERR_ARG and b"NULL" in lib.vad_last_error()
    for a, b in ((maps + 2, out), (maps, out + 1)):
        assert call(a, 2, 16, 16, 2, 3, 3, b) == ERR_ARG and b"aligned" in lib.vad_last_error(), (a, b)
    for a, b in ((maps, maps), (maps, maps + 4), (maps, maps + 2 * 256 * 4 - 4), (maps + 2 * 256 * 4 - 4, maps)):
        for op in range(4):                                                  # size 1 x 1 included: a copy, but never in place
            assert call(a, 2, 16, 16, op, 1, 1, b) == ERR_ARG and b"overlaps" in lib.vad_last_error(), (a, b)
    for op in range(4):
        assert call(maps, 0, 16, 16, op, 31, 31, out) == 0                   # n == 0: VAD_OK, nothing launched
    assert call(maps, 0, 16, 16, 2, 3, 3, maps + 2 * 256 * 4) == 0           # adjacent, not overlapping


def test_tile_answers_for_every_size_class(vad):
    lib = vad.hip.lib()
    th, tw = C.c_int(), C.c_int()
    for op in range(4):
        for sh in range(1, 32):
            for sw in (1, 2, 7, 8, 16, 31, sh):
                th.value = tw.value = 0
                assert lib.vad_morph_tile(sh, sw, op, C.byref(th), C.byref(tw)) == 0
                assert 8 <= th.value <= 256 and 8 <= tw.value <= 256, (op, sh, sw, th.value, tw.value)
    assert lib.vad_morph_tile(3, 3, 2, None, None) == 0
    for sh, sw, op, text in ((0, 3, 0, b"size must be in 1..31"), (3, 32, 0, b"size must be in 1..31"), (3, 3, 4, b"unknown op"),
                             (3, 3, -1, b"unknown op")):
        assert lib.vad_morph_tile(sh, sw, op, C.byref(th), C.byref(tw)) == -1 and text in lib.vad_last_error()


def test_header_and_signatures_agree(vad):
    hip = vad.hip
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "vad_hip.h").read_text(), flags=re.S)
    lib = hip.lib()
    for name, nargs in {"vad_morph_maps": 9, "vad_morph_tile": 5}.items():
        decl = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, header, flags=re.S)
        assert decl, f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+VAD_MORPH_MAX_SIZE\s+31\b", header)
    enum = re.search(r"enum\s*\{\s*VAD_MORPH_ERODE\s*=\s*0,\s*VAD_MORPH_DILATE\s*=\s*1,\s*VAD_MORPH_OPEN\s*=\s*2,\s*VAD_MORPH_CLOSE\s*=\s*3\s*\}", header)
    assert enum and hip.MORPH_OPS == OPS
    assert "map_morph.hip" in hip.SOURCES and (hip.CSRC / "map_morph.hip").exists()
    assert "vad_vmin" in (hip.CSRC / "vad_common.h").read_text()
