"""Rank filters of anomaly maps on the GPU (csrc/map_rankfilt.hip, metrics.rank_filter_maps, the `rank_filter=` keyword of the
scoring entry points): the kernel against the numpy restatement (tests/rank_filter_ref.py) on the bits -
nothing is computed, only selected, so NaN positions and every other bit are specified - and against scipy's recorded results, on
the shapes, sizes, ranks and contents at which a tiled selection can go wrong, and the chain through the seeded models.

The kernel has ONE selection route - a bitwise binary search over the 32-bit key, instantiated per window width, the height a loop
- so every size below runs the same code; the data classes run at a small, an even, a rectangular and the largest window, and
exercise every bit of the search (values that differ in the low 10 bits only, in the exponent only, in the sign only)."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import map_morph_ref as morph_ref
import rank_filter_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, (4, 3), (1, 7), (7, 1), 8, 9, 15, (2, 15), (15, 2)]
CLASS_SIZES = [3, (4, 3), 8, 15, (2, 15)]
CALLS_FILE = Path(__file__).resolve().parent / "golden" / "rank_filter" / "entry_point_calls.json"


def _pair(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _ranks(size):
    """0, the median, the last, and one other."""
    sh, sw = _pair(size)
    n = sh * sw
    return sorted({0, n // 2, n - 1, (9 * n) // 10, n // 3})


def _tile(vad, size):
    th, tw = C.c_int(), C.c_int()
    sh, sw = _pair(size)
    assert vad.hip.lib().vad_rankfilt_tile(sh, sw, C.byref(th), C.byref(tw)) == 0
    return th.value, tw.value


def _maps(shape, seed):
    """Frames of different content: a few levels (ties, both zeros, negative values) under continuous noise on half the pixels."""
    rng = np.random.default_rng(seed)
    levels = np.float32([-0.0, 0.0, -1.5, 0.25, 2.0, 7.0])
    x = levels[rng.integers(0, 6, shape)]
    noise = rng.standard_normal(shape).astype(np.float32)
    return np.where(rng.random(shape) < 0.5, x, noise).astype(np.float32)


def _run(vad, x: np.ndarray, size, rank="median") -> np.ndarray:
    return vad.metrics.rank_filter_maps(torch.from_numpy(x).cuda(), size, rank).cpu().numpy()


def _check(vad, x: np.ndarray, size, ranks=None, what=""):
    """Every rank of `ranks` (default: `_ranks(size)`) against the restatement; returns {rank: device result}."""
    want = ref.rank_filters(x, size, _ranks(size) if ranks is None else ranks)
    got = {}
    for r, w in want.items():
        got[r] = _run(vad, x, size, r)
        assert ref.same_bits(got[r], w), (what, size, r, x.shape)
    return got


def _bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on NaN positions plus every other bit."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


# ------------------------------------------------------------------------------------------ shapes, sizes, ranks
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_equals_the_restatement(vad, size):
    """n = 3 frames of different content per shape: a halo that read a neighbouring frame would show.  1 x 1 to 3 x 2: windows up
    to 15 x 15 reflect several times; tile + 1 rows and 2 tiles + 3 columns: seams and ragged tiles; one 1040-wide frame."""
    th, tw = _tile(vad, size)
    shapes = [(1, 1), (1, 9), (9, 1), (3, 2), (th + 1, 2 * tw + 3), (5, 1040)]
    for i, (h, w) in enumerate(shapes):
        _check(vad, _maps((3, h, w), 4600 + i), size)
    x = _maps((2, 7, 9), 4610)
    assert ref.same_bits(_run(vad, x, size), ref.rank_filter(x, size, "median"))     # the default rank


def test_equals_the_scipy_goldens(vad, golden):
    g = golden("rank_filter/scipy_rank.npz")
    checked = 0
    for name in (str(n) for n in g["names"]):
        x = g[f"x_{name}"]
        for (sh, sw, r), want in zip(g[f"rank_cases_{name}"], g[f"rank_{name}"]):
            got = _run(vad, x, (int(sh), int(sw)), int(r))
            assert np.array_equal(got, want), (name, sh, sw, r)
            checked += 1
        for (sh, sw), want in zip(g[f"median_cases_{name}"], g[f"median_{name}"]):
            assert np.array_equal(_run(vad, x, (int(sh), int(sw)), "median"), want), (name, sh, sw)
        if f"pct_{name}" in g.files:
            for (sh, sw, p, _), want in zip(g[f"pct_cases_{name}"], g[f"pct_{name}"]):
                r = vad.metrics.rank_of_percentile(int(sh) * int(sw), float(p))
                assert np.array_equal(_run(vad, x, (int(sh), int(sw)), r), want), (name, sh, sw, p)
    assert checked >= 10 * 14 * 3


# ------------------------------------------------------------------------------------------ data classes
def _data_classes(h, w, seed):
    """name -> one frame [h, w].  Every class exercises other bits of the key the search walks."""
    rng = np.random.default_rng(seed)
    u = rng.random((h, w)).astype(np.float32)
    out = {"continuous": (u * 4 - 1).astype(np.float32)}
    out["three_levels"] = np.float32([0.125, 0.5, 3.0])[rng.integers(0, 3, (h, w))]
    out["all_equal"] = np.full((h, w), 0.75, np.float32)
    base = np.float32(1.5).view(np.int32)
    out["low_10_bits"] = (base + rng.integers(0, 1024, (h, w)).astype(np.int32)).astype(np.int32).view(np.float32)
    out["exponent_only"] = np.ldexp(np.float32(1.0), rng.integers(-126, 128, (h, w))).astype(np.float32)
    out["mixed_signs"] = (rng.standard_normal((h, w)) * 1e3).astype(np.float32)
    out["signed_zeros"] = np.where(rng.random((h, w)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    z = out["continuous"].copy() * np.float32(1e-3)
    z[rng.random((h, w)) < 0.3] = 0.0
    z[rng.random((h, w)) < 0.3] = -0.0
    out["zeros_in_a_window"] = z
    den = rng.integers(-40, 41, (h, w)).astype(np.int32)                     # +-k * 2^-149, k up to 40, and +0
    out["denormals"] = np.where(den < 0, (-den) | np.int32(-2 ** 31), den).astype(np.int32).view(np.float32)
    inf = out["mixed_signs"].copy()
    inf[rng.random((h, w)) < 0.2] = np.inf
    inf[rng.random((h, w)) < 0.2] = -np.inf
    out["infinities"] = inf
    return out


@pytest.mark.parametrize("size", CLASS_SIZES, ids=str)
def test_every_data_class(vad, size):
    th, tw = _tile(vad, size)
    classes = _data_classes(th + 3, tw + 5, 4620)
    assert np.signbit(classes["denormals"]).any() and (np.abs(classes["denormals"]) < 1e-40).all()
    assert np.isinf(classes["infinities"]).sum() > 50
    x = np.stack(list(classes.values()))                                     # one batch, one frame per class
    got = _check(vad, x, size, what="classes")
    for r, y in got.items():
        assert not np.isnan(y).any()                                         # infinities and zeros are ordinary values
        for k, name in enumerate(classes):                                   # a rank SELECTS: every result is a value of its frame
            assert np.isin(y[k].view(np.int32), x[k].view(np.int32)).all(), (name, size, r)
    sh, sw = _pair(size)
    assert ref.same_bits(got[0][2], classes["all_equal"]) and ref.same_bits(got[sh * sw - 1][2], classes["all_equal"])


@pytest.mark.parametrize("size", CLASS_SIZES, ids=str)
def test_nan_at_a_corner_a_border_and_inside(vad, size):
    """A reflected NaN counts in every window that sees it - at every rank; the restatement's footprint, built pixel by pixel from
    the index formula, is the expectation.  No bit of another frame changes."""
    th, tw = _tile(vad, size)
    h, w = th + 4, tw + 6
    clean = _maps((3, h, w), 4630)
    x = clean.copy()
    nans = [(0, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, 7), (5, w - 1), (h // 2 - 2, w // 3), (th - 1, tw), (th, tw - 1)]
    for i, j in nans:
        x[1, i, j] = np.nan
    x[1, 3, 3] = -np.nan                                                     # a NaN with the sign bit set is a NaN, not a small key
    nans.append((3, 3))
    want = ref.nan_footprint(h, w, nans, size)
    got = _check(vad, x, size)
    base = _check(vad, clean, size)
    for r in got:
        assert np.array_equal(np.isnan(got[r][1]), want), (size, r)
        assert not np.isnan(got[r][[0, 2]]).any() and ref.same_bits(got[r][[0, 2]], base[r][[0, 2]])
    tiny = np.float32([[np.nan, 1.0], [2.0, 3.0], [4.0, 5.0]])               # 3 x 2 under a 15-wide window: every pixel sees it
    assert np.isnan(_run(vad, tiny, 15, 7)).all() and np.isnan(_run(vad, tiny, size, 0)).any()


# ------------------------------------------------------------------------------------------ borders, seams
@pytest.mark.parametrize("size", [2, 3, 5, 9, 15, (2, 15), (15, 2)], ids=str)
def test_stripes_and_hot_pixels_across_the_tile_seams(vad, size):
    sh, sw = _pair(size)
    th, tw = _tile(vad, size)
    h, w = 2 * th + 1, 2 * tw + 1
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for period in sorted({2, sw, sw + 1, 2 * sw - 1, 2 * sh + 1}):
        for phase in (0, 1):
            on = max(1, period // 2)
            frames.append(((xx + tw - phase) % period < on).astype(np.float32))      # vertical stripes placed against the x seam
            frames.append(((yy + th - phase) % period < on).astype(np.float32))      # horizontal ones against the y seam
    if sh * sw > 49:
        frames = frames[::3]                                                 # (the restatement sorts every window: keep large ones few)
    frames.append((((xx - tw) % (sw + 1) < 1) | ((yy - th) % (sh + 1) < 1)).astype(np.float32) * 3 - 1)
    hot = np.zeros((2, h, w), np.float32)                                    # single hot pixels: corners, borders, both sides of each seam
    for i, j in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1),
                 (th - 1, tw - 1), (th, tw), (th - 1, tw + 7), (th + 5, tw - 1), (2 * th, 2 * tw), (2 * th - 1, 5)):
        hot[0, i, j] = 1.0 + i + j
        hot[1, i, j] = -1.0
    hot[1] += 1.0                                                            # ... and single cold pixels on a bright frame
    _check(vad, np.concatenate([np.stack(frames), hot]), size)


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_end_ranks_are_erosion_and_dilation_on_the_device(vad, size):
    sh, sw = _pair(size)
    th, tw = _tile(vad, size)
    x_np = _maps((2, th + 2, tw + 7), 4640)
    x_np[1, 4, 5] = np.nan
    m = vad.metrics
    for x in (torch.from_numpy(x_np).cuda(), torch.from_numpy(_maps((3, 3, 2), 4641)).cuda()):
        assert _bits(m.rank_filter_maps(x, size, 0), m.morph_maps(x, "erode", size))
        if sh % 2 and sw % 2:
            assert _bits(m.rank_filter_maps(x, size, sh * sw - 1), m.morph_maps(x, "dilate", size))


# ------------------------------------------------------------------------------------------ batching, buffers
def test_a_frames_bits_do_not_depend_on_its_batch(vad):
    m = vad.metrics
    for size, rank in ((3, "median"), ((4, 3), 9), (15, 100)):
        th, tw = _tile(vad, size)
        x_np = _maps((5, th + 1, tw + 2), 4650)
        x_np[3, 2, 2] = np.nan
        x = torch.from_numpy(x_np).cuda()
        whole = m.rank_filter_maps(x, size, rank)
        for f in range(5):
            assert _bits(m.rank_filter_maps(x[f].contiguous(), size, rank), whole[f]), (size, f)
        assert _bits(m.rank_filter_maps(x[1:4], size, rank), whole[1:4])
        # maps and out one float off the 16-byte alignment of the allocator
        flat_in = torch.empty(x.numel() + 3, device="cuda")
        flat_out = torch.full((x.numel() + 3,), 9.0, device="cuda")
        for off in (1, 3):
            src = flat_in[off:off + x.numel()].view_as(x).copy_(x)
            dst = flat_out[off:off + x.numel()].view_as(x)
            assert src.data_ptr() % 16 != 0 and m.rank_filter_maps(src, size, rank, out=dst) is dst
            assert _bits(dst, whole), (size, off)


def test_layouts_out_refusals_and_empty_calls(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x4, x5 = _maps((3, 1, 21, 70), 4660), _maps((2, 3, 1, 21, 70), 4661)
    for x in (x4, x5):
        for size, rank in ((3, "median"), ((2, 5), 7), (4, 0)):
            got = _run(vad, x, size, rank)
            assert got.shape == x.shape and ref.same_bits(got, ref.rank_filter(x, size, rank))
    one = _run(vad, np.ascontiguousarray(x5[1, 2, 0]), 3)                     # a frame alone, [H, W]
    assert ref.same_bits(one, ref.rank_filter(x5, 3, "median")[1, 2, 0])
    x = torch.from_numpy(x4).cuda()
    out = torch.full_like(x, 5.0)
    before = vad.hip.calls.get("rank_filter_maps", 0)
    assert m.rank_filter_maps(x, 3, 4, out=out) is out and vad.hip.calls["rank_filter_maps"] == before + 1
    assert ref.same_bits(out.cpu().numpy(), ref.rank_filter(x4, 3, 4)) and torch.equal(x.cpu(), torch.from_numpy(x4))
    # overlapping out: refused by the library, and nothing is written
    flat = torch.full((2 * x.numel(),), 5.0, device="cuda")
    src = flat[:x.numel()].view_as(x)
    for off in (0, 1, x.numel() - 1):
        with pytest.raises(VadError, match="overlaps"):
            m.rank_filter_maps(src, 3, out=flat[off:off + x.numel()].view_as(x))
    m.rank_filter_maps(src, 3, out=flat[x.numel():].view_as(x))               # adjacent is fine
    torch.cuda.synchronize()
    assert bool((flat[:x.numel()] == 5.0).all()) and bool((flat[x.numel():] == 5.0).all())
    for bad_out in (torch.empty(3, 1, 21, 71, device="cuda"), torch.empty(3, 1, 21, 70, device="cuda", dtype=torch.float64),
                    torch.empty(3, 1, 21, 70), torch.empty(3, 1, 70, 21, device="cuda").transpose(2, 3)):
        with pytest.raises(VadError, match="out must be"):
            m.rank_filter_maps(x, 3, out=bad_out)
    with pytest.raises(VadError, match="float32"):
        m.rank_filter_maps(x.double(), 3)
    with pytest.raises(VadError, match="contiguous"):
        m.rank_filter_maps(x.transpose(2, 3), 3)
    with pytest.raises(VadError, match="at least the two dimensions"):
        m.rank_filter_maps(x.reshape(-1), 3)
    with pytest.raises(VadError, match="size must be in"):
        m.rank_filter_maps(x, (3, 16))
    with pytest.raises(VadError, match="rank must be an int in 0..8"):
        m.rank_filter_maps(x, 3, 9)
    # size 1 is a copy; an empty call launches nothing
    c = _maps((2, 1, 19, 23), 4662)
    c[0, 0, 3, 4], c[1, 0, 0, 0] = np.nan, np.inf
    assert ref.same_bits(_run(vad, c, 1, 0), c) and ref.same_bits(_run(vad, c, (1, 1)), c)
    before = vad.hip.calls.get("rank_filter_maps", 0)
    for shape in ((0, 1, 8, 8), (2, 0, 1, 8, 8)):
        out = m.rank_filter_maps(torch.empty(shape, device="cuda"), 3)
        assert tuple(out.shape) == shape
    assert vad.hip.calls.get("rank_filter_maps", 0) == before
    assert vad.hip.lib().vad_rankfilt_maps(0x1000, 0, 8, 8, 3, 3, 4, 0x9000, None) == 0


def test_a_list_of_steps_ping_pongs_two_buffers(vad):
    x_np = _maps((2, 1, 40, 70), 4670)
    x = torch.from_numpy(x_np).cuda()
    steps = vad.metrics.rank_filter_steps([("median", 3), ("percentile", (1, 5), 90), ("rank", (4, 3), 0)])
    assert steps == (((3, 3), 4), ((1, 5), 4), ((4, 3), 0))
    before = vad.hip.calls.get("rank_filter_maps", 0)
    ptrs = set()
    real = vad.metrics.rank_filter_maps

    def spy(maps, size, rank="median", out=None):
        got = real(maps, size, rank, out)
        ptrs.add(got.data_ptr())
        return got

    vad.metrics.rank_filter_maps = spy
    try:
        got = vad.metrics.apply_rank_filter(x, steps)
    finally:
        vad.metrics.rank_filter_maps = real
    assert vad.hip.calls["rank_filter_maps"] == before + 3
    assert len(ptrs) == 2 and x.data_ptr() not in ptrs                        # two buffers of its own
    assert ref.same_bits(got.cpu().numpy(), ref.apply(x_np, steps)) and torch.equal(x.cpu(), torch.from_numpy(x_np))
    assert vad.metrics.apply_rank_filter(x, ()) is x


# ------------------------------------------------------------------------------------------ scale
def test_more_frames_than_one_grid_dimension(vad):
    """65,537 frames of 2 x 3: frame 65,535 is the first of the second slice of gridDim.y.  Frame i is entry i % 251 of a pool; the
    restatement runs on the pool, the comparison with the expansion on the device."""
    n, pool = 65537, _maps((251, 2, 3), 4680)
    index = torch.arange(n, device="cuda") % 251
    x = torch.from_numpy(pool).cuda()[index].contiguous()
    for size, rank in ((3, "median"), ((2, 15), 29)):
        before = vad.hip.calls.get("rank_filter_maps", 0)
        got = vad.metrics.rank_filter_maps(x, size, rank)
        assert vad.hip.calls["rank_filter_maps"] == before + 1
        want = torch.from_numpy(ref.rank_filter(pool, size, rank)).cuda()[index]
        assert _bits(got, want), size
        assert _bits(got[65534:], want[65534:])                               # the last frame of one slice, the first of the next


def test_an_offset_past_two_to_the_31_elements(vad):
    """2050 frames of 1024 x 1024 = 2^31 + 2^21 elements, as the morphology case of tests/test_hip_large_offsets.py; the first and the
    last frame are checked (the last one begins past element 2^31), the frames between are whatever the allocation holds."""
    n, h, w = 2050, 1024, 1024
    free, _ = torch.cuda.mem_get_info()
    if free < 20 << 30:
        pytest.skip(f"{free >> 30} GiB of device memory are free; the 8.6 GB batch and its output need 20")
    first, last = _maps((h, w), 4690), _maps((h, w), 4691)
    x = torch.empty((n, h, w), device="cuda")
    x[1:n - 1].zero_()
    x[0].copy_(torch.from_numpy(first))
    x[n - 1].copy_(torch.from_numpy(last))
    assert x[n - 1].data_ptr() - x.data_ptr() > 4 * 2 ** 31
    got = vad.metrics.rank_filter_maps(x, 3)
    g0, g1, mid = got[0].cpu().numpy(), got[n - 1].cpu().numpy(), bool((got[1:n - 1:97] == 0).all())
    del x, got
    torch.cuda.empty_cache()
    assert ref.same_bits(g0, ref.rank_filter(first, 3, "median")) and ref.same_bits(g1, ref.rank_filter(last, 3, "median")) and mid


def test_a_captured_call_replays_on_new_contents(vad):
    contents = [_maps((2, 1, 45, 150), 4700 + i) for i in range(3)]
    contents[1][1, 0, 15, 64] = np.nan
    x = torch.from_numpy(contents[0]).cuda()
    outs = {}
    vad.metrics.rank_filter_maps(x, 15)                                       # once eagerly: nothing left to set up under capture
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            outs["m15"] = vad.metrics.rank_filter_maps(x, 15)
            outs["p"] = vad.metrics.rank_filter_maps(x, (2, 5), 8)
            outs["both"] = vad.metrics.rank_filter_maps(outs["m15"], 3, 0)
    torch.cuda.current_stream().wait_stream(side)
    for c in contents:
        x.copy_(torch.from_numpy(c))
        graph.replay()
        torch.cuda.synchronize()
        m15 = ref.rank_filter(c, 15, "median")
        assert ref.same_bits(outs["m15"].cpu().numpy(), m15)
        assert ref.same_bits(outs["p"].cpu().numpy(), ref.rank_filter(c, (2, 5), 8))
        assert ref.same_bits(outs["both"].cpu().numpy(), ref.rank_filter(m15, 3, 0))


# ------------------------------------------------------------------------------------------ through the models
def _image_model(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    return model.cuda().eval()


def _video_model(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    return model.cuda().eval()


def _threshold(maps, q=0.9):
    return float(np.quantile(maps.cpu().numpy(), q))


@pytest.mark.parametrize("spec", [("median", 3), [("median", 3), ("percentile", (3, 5), 75)]], ids=["median3", "median3_p75"])
def test_localize_filters_the_maps_it_labels(vad, spec):
    model = _image_model(vad)
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32)).cuda()
    steps = vad.metrics.rank_filter_steps(spec)
    for sigma in (None, 1.0):
        with torch.no_grad():
            plain = vad.scoring._anomaly_maps(model, x, "mse", sigma, 4.0)
        by_hand = vad.metrics.apply_rank_filter(plain, steps)
        t = _threshold(by_hand, 0.8)
        before = {k: vad.hip.calls.get(k, 0) for k in ("rank_filter_maps", "img_score", "smooth_maps", "morph_maps")}
        regions, maps = vad.scoring.localize(model, x, t, sigma=sigma, max_regions=256, rank_filter=spec)
        assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [len(steps), 1, int(sigma is not None), 0]
        assert torch.equal(maps, by_hand) and not torch.equal(maps, plain)
        assert ref.same_bits(maps.cpu().numpy(), ref.apply(plain.cpu().numpy(), steps))
        table = vad.metrics.detect_regions(by_hand, t, max_regions=256)
        assert torch.equal(regions.records, table.records) and torch.equal(regions.counts, table.counts)
        assert int(regions.counts[:, 0].sum()) > 0
        events, emaps = vad.scoring.localize_events(model, x, t, sigma=sigma, max_events=256, rank_filter=spec)
        ev = vad.metrics.detect_events(by_hand[:, 0], t, max_events=256)
        assert torch.equal(emaps, by_hand) and torch.equal(events.records, ev.records) and torch.equal(events.counts, ev.counts)


def test_the_order_is_calibration_rank_filter_morph(vad):
    """sigma, calibration, rank filter, morph: in z-score units, the median before the opening (the two do not commute)."""
    model = _video_model(vad)
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 4, 3, 32, 32)).cuda()
    stats = vad.scoring.calibrate(model, [{"frames": clips}], "cuda", sigma=1.0)
    with torch.no_grad():
        z = vad.scoring._anomaly_maps(model, clips, "mse", 1.0, 4.0, stats, vad.metrics.DEFAULT_MIN_STD).cpu().numpy()
    want = morph_ref.opening(ref.rank_filter(z, (3, 5), "median"), 2)
    other = ref.rank_filter(morph_ref.opening(z, 2), (3, 5), "median")
    assert not ref.same_bits(want, other)
    regions, maps = vad.scoring.localize(model, clips, 0.5, sigma=1.0, calibration=stats, morph=("open", 2), rank_filter=("median", (3, 5)))
    assert tuple(maps.shape) == (2, 4, 1, 32, 32) and ref.same_bits(maps.cpu().numpy(), want)
    table = vad.metrics.detect_regions(maps, 0.5)
    assert torch.equal(regions.records, table.records) and torch.equal(regions.counts, table.counts)
    scores, smaps = vad.scoring.frame_scores(model, clips, "max", sigma=1.0, calibration=stats, morph=("open", 2), temporal=("max", 2),
                                             rank_filter=("median", (3, 5)))
    import map_temporal_ref
    last = map_temporal_ref.clips([("max", 2)], want[:, :, 0])[:, :, None]    # ... and the temporal filter last
    assert ref.same_bits(smaps.cpu().numpy(), last) and ref.same_bits(scores.cpu().numpy(), last.reshape(2, 4, -1).max(-1))
    assert stats.meta == {"map": "mse", "sigma": 1.0, "truncate": 4.0}        # the calibration knows nothing of the filter


@pytest.mark.parametrize("split", [(6,), (1, 1, 1, 1, 1, 1), (2, 4)], ids=["whole", "one_by_one", "2_4"])
def test_localize_stream_filters_every_frame_on_its_own(vad, split):
    model = _video_model(vad)
    clips = torch.from_numpy(vad.synth.clips(22, 0, 2, 6, 3, 32, 32)).cuda()
    with torch.no_grad():
        whole = vad.metrics.smooth_maps(model.score_stateful(clips, None, errmap=True)["errmap"], 1.0)
    spec = ("median", 3)
    filtered = vad.metrics.rank_filter_maps(whole, 3)
    t = _threshold(filtered, 0.9)
    kw = dict(threshold=t, connectivity=8, temporal=1, min_duration=1, min_volume=1, max_open=512, max_closed=256)
    tracker, by_hand = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    plain_tracker, one_tracker = vad.metrics.EventTracker(2, 32, 32, **kw), vad.metrics.EventTracker(2, 32, 32, **kw)
    state, plain_state, f, seen, plain_seen = None, None, 0, [], []
    for k in split:
        chunk = clips[:, f:f + k]
        f += k
        _, plain, plain_state = vad.scoring.localize_stream(model, chunk, plain_tracker, plain_state, sigma=1.0)
        before = vad.hip.calls.get("rank_filter_maps", 0)
        up, maps, state = vad.scoring.localize_stream(model, chunk, tracker, state, sigma=1.0, rank_filter=spec)
        assert vad.hip.calls["rank_filter_maps"] == before + 1
        hand = vad.metrics.rank_filter_maps(plain, 3)
        want = by_hand.update(hand)
        assert torch.equal(maps, hand) and tuple(maps.shape) == (2, k, 1, 32, 32)
        assert torch.equal(up.records, want.records) and torch.equal(up.counts, want.counts) and torch.equal(up.frame_counts, want.frame_counts)
        seen.append(maps)
        plain_seen.append(plain)
    assert torch.equal(tracker.state, by_hand.state)
    volume = torch.cat(seen, dim=1)
    assert ref.same_bits(volume.cpu().numpy(), ref.rank_filter(torch.cat(plain_seen, dim=1).cpu().numpy(), 3, "median"))     # frame by frame
    _, one_call, _ = vad.scoring.localize_stream(model, clips, one_tracker, None, sigma=1.0, rank_filter=spec)
    assert torch.equal(one_call, volume) and torch.equal(one_tracker.state, tracker.state)      # however the frames are split over calls
    assert int(tracker.flush().counts[:, 0].sum()) + int(volume.ge(t).sum()) > 0


def test_pixel_metrics_accumulate_the_filtered_maps(vad):
    model = _image_model(vad)
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32))
    rng = np.random.default_rng(12)
    raw = np.kron(rng.choice(np.array([0, 255], np.uint8), (6, 4, 4), p=[0.7, 0.3]), np.ones((1, 8, 8), np.uint8))
    masks = torch.from_numpy(raw).cuda()[:, None]
    loader = [{"image": x[:4], "mask": masks[:4], "label": [0, 1, 0, 1], "defect_type": list("abab")},
              {"image": x[4:], "mask": masks[4:], "label": [0, 1], "defect_type": list("ab")}]
    spec, bits = [("median", 3), ("rank", (2, 2), 3)], 11
    steps = vad.metrics.rank_filter_steps(spec)
    before = vad.hip.calls.get("rank_filter_maps", 0)
    _, _, hist = vad.scoring.pixel_auroc(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, rank_filter=spec)
    assert vad.hip.calls["rank_filter_maps"] == before + 2 * len(steps)
    hand, hand_pro, plain = vad.metrics.ScoreHistogram(bits), vad.metrics.ProHistogram(bits), vad.metrics.ScoreHistogram(bits)
    counts, scores = vad.metrics.DetectionCounts("cuda"), []
    for b in loader:
        with torch.no_grad():
            sm = vad.metrics.smooth_maps(model.score_all(b["image"].cuda())["errmap"], 1.0)
        plain.accumulate(sm, b["mask"])
        filtered = vad.metrics.apply_rank_filter(sm, steps)
        hand.accumulate(filtered, b["mask"])
        hand_pro.accumulate(filtered, b["mask"])
        counts.update(vad.metrics.match_regions(filtered, b["mask"], 0.01, max_regions=1))
        scores.append(filtered.flatten(1).max(dim=1).values)
    assert torch.equal(hist.counts(), hand.counts()) and torch.equal(hist.rejected(), hand.rejected())
    assert not torch.equal(hist.counts(), plain.counts()) and int(hist.counts().sum() + hist.rejected().sum()) == 6 * 32 * 32
    _, _, _, pro = vad.scoring.pixel_aupro(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, rank_filter=spec)
    assert torch.equal(pro.weighted(), hand_pro.weighted()) and torch.equal(pro.counts(), hand_pro.counts())
    _, got = vad.scoring.detection_report(model, loader, "cuda", 0.01, sigma=1.0, rank_filter=spec)
    assert torch.equal(got.counts, counts.counts) and got.params["rank_filter"] == steps
    _, _, got_scores, _ = vad.scoring.compute_auroc_maps(model, loader, "cuda", reduce="max", sigma=1.0, rank_filter=spec)
    assert np.array_equal(got_scores, torch.cat(scores).cpu().numpy())
    before = vad.hip.calls["rank_filter_maps"]
    _, _, none = vad.scoring.pixel_auroc(model, loader, "cuda", mantissa_bits=bits, sigma=1.0, rank_filter=None)
    assert torch.equal(none.counts(), plain.counts()) and vad.hip.calls["rank_filter_maps"] == before


def test_none_leaves_every_entry_point_on_its_present_calls(vad):
    """The library calls of every touched entry point without the keyword, and with `rank_filter=None`, are the ones recorded before
    the rank filters existed (tests/golden/rank_filter/entry_point_calls.json; same models, same batches as the temporal filters'
    test of the same name)."""
    recorded = json.loads(CALLS_FILE.read_text())
    model, img, s = _video_model(vad), _image_model(vad), vad.scoring
    clips = torch.from_numpy(vad.synth.clips(25, 0, 2, 4, 3, 32, 32)).cuda()
    masks = torch.zeros(2, 4, 1, 32, 32, device="cuda")
    masks[:, 1:3, :, 4:12, 4:12] = 1.0
    batch = [{"frames": clips, "mask": masks, "frame_labels": np.array([[0, 1, 1, 0]] * 2), "image": clips, "label": [0, 1], "defect_type": ["a", "b"]}]
    ibatch = [{"image": clips[:, 0].contiguous(), "mask": masks[:, 1].contiguous(), "label": [0, 1], "defect_type": ["a", "b"]}]
    tracker = lambda: vad.metrics.EventTracker(2, 32, 32, 0.01)

    def delta(call):
        before = dict(vad.hip.calls)
        with torch.no_grad():
            call()
        return {k: v - before.get(k, 0) for k, v in vad.hip.calls.items() if v != before.get(k, 0)}

    cases = {
        "_anomaly_maps": lambda **kw: s._anomaly_maps(img, clips[:, 0].contiguous(), "mse", None, 4.0, **kw),
        "pixel_auroc": lambda **kw: s.pixel_auroc(model, batch, "cuda", **kw),
        "pixel_aupro": lambda **kw: s.pixel_aupro(img, ibatch, "cuda", **kw),
        "detection_report": lambda **kw: s.detection_report(model, batch, "cuda", 0.01, **kw),
        "frame_scores": lambda **kw: s.frame_scores(model, clips, "max", **kw),
        "frame_auroc_reduced": lambda **kw: s.frame_auroc(model, batch, "cuda", reduce="max", **kw),
        "frame_auroc": lambda **kw: s.frame_auroc(model, batch, "cuda", **kw),
        "compute_auroc_maps": lambda **kw: s.compute_auroc_maps(img, ibatch, "cuda", **kw),
        "localize": lambda **kw: s.localize(img, clips[:, 0].contiguous(), 0.01, **kw),
        "localize_events": lambda **kw: s.localize_events(model, clips, 0.01, **kw),
        "localize_stream": lambda **kw: s.localize_stream(model, clips, tracker(), **kw),
    }
    assert set(cases) == set(recorded)
    for name, call in cases.items():
        assert delta(call) == recorded[name], name
        assert delta(lambda: call(rank_filter=None)) == recorded[name], name
        assert "rank_filter_maps" not in recorded[name]


# ------------------------------------------------------------------------------------------ what the filter is for
def _regions(mask: np.ndarray) -> int:
    """8-connected regions of a small boolean frame (a flood fill: the CPU side of the count)."""
    seen, n = np.zeros_like(mask), 0
    for i, j in np.argwhere(mask):
        if seen[i, j]:
            continue
        n += 1
        stack = [(i, j)]
        seen[i, j] = True
        while stack:
            y, x = stack.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < mask.shape[0] and 0 <= xx < mask.shape[1] and mask[yy, xx] and not seen[yy, xx]:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
    return n


def test_a_median_removes_hot_pixels_and_keeps_the_defect(vad):
    """Flat noise below the threshold, isolated hot pixels above it, one 6 x 6 defect across a tile corner; threshold between noise
    and defect.  Every count is taken from the restatements on the CPU first; the device must equal them.
    Frame 0, the defect an axis-aligned 6 x 6 square: ("median", 3) leaves exactly one region, 32 of the defect's 36 pixels (the four
    corners see 4 defect pixels of 9).  A 3 x 3 opening of an axis-aligned square is lossless - erosion leaves 4 x 4, dilation
    restores 6 x 6 -, so ("open", 3) leaves 36 there, not fewer: that relation cannot hold on a square, for scipy's filters as for
    these, and the counts are asserted as they are.
    Frame 1, the same 6 x 6 extent with its corners cut (an octagon of 24 pixels, rows of 2 4 6 6 4 2 - a defect that HAS corners and
    thin parts for an opening to eat): ("open", 3) leaves 16 pixels, ("median", 3) more of it."""
    th, tw = _tile(vad, 3)
    h, w, by, bx = 2 * th + 6, 2 * tw + 22, th - 3, tw - 2
    rng = np.random.default_rng(4710)
    x = (rng.random((2, h, w)) * 0.2).astype(np.float32)
    planted = 0
    octagon = np.zeros((6, 6), bool)
    for i, (a, b) in enumerate(((2, 4), (1, 5), (0, 6), (0, 6), (1, 5), (2, 4))):
        octagon[i, a:b] = True
    defect = [np.ones((6, 6), bool), octagon]
    for f in range(2):
        for i in range(1, h - 1, 4):
            for j in range(1 + 2 * (i // 4 % 2), w - 1, 5):                   # isolated single pixels: no 3 x 3 window holds two
                if not (by - 4 <= i <= by + 9 and bx - 4 <= j <= bx + 10):
                    x[f, i, j] = 1.0 + rng.random()
                    planted += 1
        x[f, by:by + 6, bx:bx + 6][defect[f]] = 2.0
    t = 0.5
    box = np.zeros((2, h, w), bool)
    box[:, by:by + 6, bx:bx + 6] = True
    med_ref, open_ref = ref.rank_filter(x, 3, "median") >= t, morph_ref.opening(x, 3) >= t
    assert [_regions(med_ref[f]) for f in range(2)] == [1, 1] and not (med_ref & ~box).any() and not (open_ref & ~box).any()
    med_area, open_area = med_ref.sum(axis=(1, 2)).tolist(), open_ref.sum(axis=(1, 2)).tolist()
    assert med_area[0] == 32 <= 36 and open_area[0] == 36                     # the square: see the docstring
    assert open_area[1] == 16 < med_area[1] <= 24                             # the defect with corners: the opening leaves fewer pixels
    maps = torch.from_numpy(x).cuda()
    raw = vad.metrics.detect_regions(maps, t, max_regions=1024)
    assert int(raw.counts[:, 0].sum()) == planted + 2 and planted > 300
    med = vad.metrics.rank_filter_maps(maps, 3)
    clean = vad.metrics.detect_regions(med, t, max_regions=1024)
    assert clean.counts[:, 0].tolist() == [1, 1] and clean.area[:, 0].tolist() == med_area
    assert torch.equal((med >= t).cpu(), torch.from_numpy(med_ref))
    opened = vad.metrics.detect_regions(vad.metrics.morph_maps(maps, "open", 3), t, max_regions=1024)
    assert opened.counts[:, 0].tolist() == [1, 1] and opened.area[:, 0].tolist() == open_area
    flat = ~box & (x < t)                                                     # ... and the level of flat areas is left alone: a median of
    assert bool((med.cpu().numpy()[flat] > 0.0).all()) and float(med.cpu().numpy()[flat].max()) < 0.2      # noise is noise
