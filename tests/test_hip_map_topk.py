"""Order statistics and top-k means of anomaly maps on the GPU (`vad_map_topk`, csrc/map_topk.hip) against the
numpy restatement tests/map_topk_ref.py: `kth` to the bit, `mean` within the derived bound
    0.5 * spacing32(exact) + P * 2^-52 * mean(|top k|)
(a float64 sum of at most P exactly representable terms errs by less than P * 2^-53 * sum|x| in any order; divided by k; the rounding
to float32 adds half a spacing).  Up to `vad_topk_plan`'s boundary a frame is one work-group of 1024 threads, pixels dealt to
threads in rounds of 1024, four rounds per loop trip - so the small shapes are those at which that walk changes: fewer pixels than
threads, a ragged last round, more than one unrolled trip (80 x 96 = 7.5 rounds) -; above it a frame is split into slices over
several launches, and one frame sits on each side of the boundary, the upper one with a last slice of a single pixel."""
import ctypes as C

import numpy as np
import pytest
import torch

import map_topk_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

SHAPES = {
    "one_pixel": (3, 1, 1),
    "smallest_frame": (3, 2, 3),
    "fewer_pixels_than_threads": (3, 7, 9),
    "w_not_vector_multiple": (3, 16, 20),
    "several_pixels_per_thread": (3, 80, 96),
    "five_dims": (2, 3, 1, 16, 16),
}
_REF = {}


def _maps(shape, seed, signed=True):
    rng = np.random.default_rng(seed)
    x = (np.exp(rng.standard_normal(shape) * 3.0) * 1e-3).astype(np.float32)
    return x * rng.choice(np.array([-1, 1], np.float32), shape) if signed else x


def _ranks(p):
    """1, 2, P - 1, P and the helpers' ranks for 0.1 % / 1 % / 10 %, clipped into 1 .. P (duplicates are allowed)."""
    return [1, min(2, p), max(1, p - 1), p, ref.rank_of_fraction(0.001, p), ref.rank_of_fraction(0.01, p), ref.rank_of_fraction(0.1, p)]


def _case(name):
    """(input, ranks, restatement): computed once per module, never modified."""
    if name not in _REF:
        shape = SHAPES[name]
        x = _maps(shape, 900 + list(SHAPES).index(name))
        ranks = _ranks(shape[-2] * shape[-1])
        _REF[name] = (x, ranks, ref.topk(x, ranks))
    return _REF[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(got, want, what=""):
    """A result dict of metrics.map_topk against the restatement's: kth as floats and as bits, mean within the bound."""
    if "kth" in got:
        kth = got["kth"].cpu()
        assert kth.dtype == torch.float32 and tuple(kth.shape) == want["kth"].shape, what
        finite = torch.from_numpy(~np.isnan(want["kth"]))
        assert torch.equal(kth[finite], torch.from_numpy(want["kth"])[finite]), what
        assert torch.equal(_bits(kth), _bits(torch.from_numpy(want["kth"]))), what
    if "mean" in got:
        mean = got["mean"].cpu().numpy()
        assert mean.dtype == np.float32 and mean.shape == want["mean"].shape, what
        with np.errstate(invalid="ignore"):                                 # inf - inf where both are infinite
            err = np.abs(mean.astype(np.float64) - want["exact"])
        print(f"{what}: max |mean - exact| / bound = {np.nanmax(np.where(want['bound'] > 0, err / np.maximum(want['bound'], 1e-300), 0.0)):.3f}")
        assert ref.mean_within_bound(mean, want), what
        nan = np.isnan(want["kth"])
        assert (mean.view(np.uint32)[nan] == ref.QNAN_BITS).all(), what      # a NaN frame: the canonical quiet NaN


@pytest.mark.parametrize("name", list(SHAPES))
def test_equals_the_restatement(vad, name):
    x, ranks, want = _case(name)
    xt = torch.from_numpy(x).cuda()
    before = vad.hip.calls.get("map_topk", 0)
    got = vad.metrics.map_topk(xt, ranks)
    assert vad.hip.calls["map_topk"] == before + 1 and set(got) == {"kth", "mean"}
    assert got["kth"].shape == got["mean"].shape == xt.shape[:-2] + (len(ranks),) and got["kth"].is_cuda
    _check(got, want, name)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                        # the input is not touched
    only_k, only_m = vad.metrics.map_topk(xt, ranks, mean=False), vad.metrics.map_topk(xt, ranks, kth=False)
    assert set(only_k) == {"kth"} and set(only_m) == {"mean"}
    assert torch.equal(_bits(only_k["kth"]), _bits(got["kth"])) and torch.equal(_bits(only_m["mean"]), _bits(got["mean"]))
    one = vad.metrics.map_topk(xt, ranks[-1])                                # an int: no rank axis
    assert one["kth"].shape == xt.shape[:-2] and torch.equal(_bits(one["kth"]), _bits(got["kth"][..., -1]))
    assert torch.equal(_bits(one["mean"]), _bits(got["mean"][..., -1]))


def test_eight_ranks_equal_eight_calls_in_any_order_with_duplicates(vad):
    x, _, _ = _case("several_pixels_per_thread")
    p = 80 * 96
    xt = torch.from_numpy(x).cuda()
    ranks = [p, 5000, 768, 768, 77, 8, 1, 1]                                 # descending, duplicates
    want = ref.topk(x, ranks)
    got = vad.metrics.map_topk(xt, ranks)
    _check(got, want, "eight ranks")
    for j, k in enumerate(ranks):
        single = vad.metrics.map_topk(xt, [k])
        assert torch.equal(_bits(single["kth"][:, 0]), _bits(got["kth"][:, j])), k
        assert torch.equal(_bits(single["mean"][:, 0]), _bits(got["mean"][:, j])), k
    assert torch.equal(_bits(got["kth"][:, 2]), _bits(got["kth"][:, 3])) and torch.equal(_bits(got["mean"][:, 6]), _bits(got["mean"][:, 7]))
    shuffled = vad.metrics.map_topk(xt, ranks[::-1])
    assert torch.equal(_bits(shuffled["kth"].flip(-1)), _bits(got["kth"])) and torch.equal(_bits(shuffled["mean"].flip(-1)), _bits(got["mean"]))


def _contents():
    """name -> one 16 x 20 frame that exercises a digit pass, a tie or a class of values (P = 320)."""
    rng = np.random.default_rng(77)
    h, w, p = 16, 20, 320
    u32 = lambda a: np.asarray(a, np.uint32).view(np.float32).reshape(h, w)
    base = np.float32(1.5).view(np.uint32)
    out = {}
    out["all_equal"] = np.full((h, w), 0.37, np.float32)
    step = np.full(p, 2.0, np.float32)
    step[rng.permutation(p)[:100]] = 3.0                                     # 100 pixels of 3.0: ranks 100 | 101 straddle the step
    out["two_values"] = step.reshape(h, w)
    out["last_10_bits"] = u32(base + rng.integers(0, 1 << 10, p).astype(np.uint32))
    out["middle_11_bits"] = u32(base + (rng.integers(0, 1 << 11, p).astype(np.uint32) << np.uint32(10)))
    out["sign_only"] = (np.float32(0.75) * rng.choice(np.float32([-1, 1]), p)).reshape(h, w)
    out["zeros_of_both_signs"] = rng.choice(np.float32([0.0, -0.0]), p).reshape(h, w)
    out["denormals"] = u32(rng.integers(1, 1 << 23, p).astype(np.uint32) | (rng.integers(0, 2, p).astype(np.uint32) << np.uint32(31)))
    inf = _maps((p,), 78)
    inf[rng.permutation(p)[:5]] = np.float32([np.inf, np.inf, -np.inf, -np.inf, np.inf])
    out["infinities"] = inf.reshape(h, w)
    return out


CONTENT_RANKS = [1, 2, 3, 100, 101, 160, 319, 320]                          # 1 .. 3: the +inf pixels; 319, 320: -inf inside the top k


def test_contents_that_exercise_every_digit_pass(vad):
    frames = _contents()
    x = np.stack(list(frames.values()))
    want = ref.topk(x, CONTENT_RANKS)
    got = vad.metrics.map_topk(torch.from_numpy(x).cuda(), CONTENT_RANKS)
    kth, mean = got["kth"].cpu(), got["mean"].cpu()
    for i, name in enumerate(frames):
        row = {k: v[i] for k, v in want.items()}
        _check({"kth": kth[i], "mean": mean[i]}, row, name)
    names = list(frames)
    two = kth[names.index("two_values")].tolist()
    assert two[3] == 3.0 and two[4] == 2.0                                   # the rank on either side of the step
    z = kth[names.index("zeros_of_both_signs")]
    plus = int((~np.signbit(frames["zeros_of_both_signs"])).sum())
    assert [bool(np.signbit(v)) for v in z.numpy()] == [k > plus for k in CONTENT_RANKS]      # +0.0 ranks above -0.0
    i = names.index("infinities")
    assert kth[i, :3].tolist() == [np.inf] * 3 and kth[i, -2:].tolist() == [-np.inf] * 2
    assert mean[i, :6].tolist() == [np.inf] * 6 and bool(torch.isnan(mean[i, -2:]).all())    # both signs inside the top k: NaN


@pytest.mark.parametrize("where", ["first_pixel", "last_pixel", "one_frame_of_three"])
def test_nan_makes_its_frame_nan_and_no_other(vad, where):
    x = _case("several_pixels_per_thread")[0].copy()
    ranks = [1, 77, 80 * 96]
    if where == "first_pixel":
        x[0, 0, 0] = np.nan
    elif where == "last_pixel":
        x[0, -1, -1] = np.float32(np.uint32(0xFFC00001).view(np.float32))    # a negative NaN with a payload
    else:
        x[1, 40, 3] = np.nan
    bad = 1 if where == "one_frame_of_three" else 0
    xt = torch.from_numpy(x).cuda()
    got = vad.metrics.map_topk(xt, ranks)
    _check(got, ref.topk(x, ranks), where)
    assert bool((_bits(got["kth"][bad]) == ref.QNAN_BITS).all()) and bool((_bits(got["mean"][bad]) == ref.QNAN_BITS).all())
    for i in range(3):
        if i != bad:
            solo = vad.metrics.map_topk(xt[i].contiguous(), ranks)
            assert torch.equal(_bits(solo["kth"]), _bits(got["kth"][i])) and torch.equal(_bits(solo["mean"]), _bits(got["mean"][i]))


def test_frames_do_not_depend_on_the_batch(vad):
    x, ranks, want = _case("w_not_vector_multiple")                          # 320 pixels: frames of a batch start at every alignment
    xt = torch.from_numpy(x).cuda()
    solo = [vad.metrics.map_topk(xt[i].contiguous(), ranks) for i in range(3)]
    other = torch.from_numpy(_maps((16, 20), 5)).cuda()
    for i in range(3):
        _check(solo[i], {k: v[i] for k, v in want.items()}, f"solo {i}")
        for pos in range(3):
            batch = torch.stack([xt[i] if j == pos else other * (j + 1) for j in range(3)])
            got = vad.metrics.map_topk(batch, ranks)
            assert torch.equal(_bits(got["kth"][pos]), _bits(solo[i]["kth"])) and torch.equal(_bits(got["mean"][pos]), _bits(solo[i]["mean"])), (i, pos)


def test_bases_one_float_off_their_allocations(vad):
    """maps and both outputs sliced one float into their allocations; outputs pre-filled with NaN and fully overwritten; the floats
    on either side of them keep their bits; the record in the workspace holds c and S of the formula."""
    x, ranks, want = _case("w_not_vector_multiple")
    n, p, nk = 3, 320, len(ranks)
    buf = torch.zeros(x.size + 1, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xt = buf[1:]
    outs = []
    for _ in range(2):
        o = torch.full((n * nk + 2,), float("nan"), device="cuda")
        o[0] = o[-1] = -7.0
        outs.append(o)
    kth, mean = outs[0][1:-1], outs[1][1:-1]
    assert xt.data_ptr() % 16 == 4 and kth.data_ptr() % 16 == 4 and mean.data_ptr() % 16 == 4
    lib = vad.hip.lib()
    need = lib.vad_topk_workspace_bytes(n, 16, 20, nk)
    assert need == n * nk * 16
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    vad.hip.check(lib.vad_map_topk(xt.data_ptr(), n, 16, 20, (C.c_uint * nk)(*ranks), nk, kth.data_ptr(), mean.data_ptr(), ws.data_ptr(), need,
                                   vad.hip.current_stream()), "vad_map_topk")
    _check({"kth": kth.view(n, nk), "mean": mean.view(n, nk)}, want, "off by one float")
    for o in outs:
        assert o[0].item() == -7.0 and o[-1].item() == -7.0
    assert torch.equal(buf[1:].cpu(), torch.from_numpy(x).reshape(-1)) and buf[0].item() == 0.0
    rec = ws.cpu().numpy().view(np.uint32).reshape(n, nk, 4)
    keys = ref.key(x.reshape(n, -1))
    for i in range(n):
        for j, k in enumerate(ranks):
            assert rec[i, j, 0] == want["kth"][i, j].view(np.uint32)
            above = keys[i] > ref.key(want["kth"][i, j:j + 1])[0]
            assert rec[i, j, 1] == int(above.sum()) < k
            s = rec[i, j, 2:].copy().view(np.float64)[0]
            top = x[i].reshape(-1)[above].astype(np.float64)
            assert abs(s - ref.math.fsum(top.tolist())) <= p * 2.0 ** -53 * float(np.abs(top).sum())
    short = lib.vad_map_topk(xt.data_ptr(), n, 16, 20, (C.c_uint * nk)(*ranks), nk, kth.data_ptr(), None, ws.data_ptr(), need - 1, vad.hip.current_stream())
    assert short == -3 and b"ws_bytes" in lib.vad_last_error()


SPLIT_ABOVE, SLICE = 262144, 32768                                           # asserted against the library
BOUNDARY = {"at_the_boundary": (2, 512, 512), "one_pixel_above": (2, 65, 4033)}   # 262,144 and 262,145 pixels: 9 slices, the last of one pixel


def _boundary_case(side):
    if side not in _REF:
        shape = BOUNDARY[side]
        p = shape[1] * shape[2]
        x = _maps(shape, 950 + list(BOUNDARY).index(side))
        ranks = _ranks(p) + [100000]                                         # eight ranks
        _REF[side] = (x, ranks, ref.topk(x, ranks))
    return _REF[side]


@pytest.mark.parametrize("side", list(BOUNDARY))
def test_a_frame_on_each_side_of_the_split(vad, side):
    split, piece = C.c_int(), C.c_int()
    assert vad.hip.lib().vad_topk_plan(C.byref(split), C.byref(piece)) == 0 and (split.value, piece.value) == (SPLIT_ABOVE, SLICE)
    x, ranks, want = _boundary_case(side)
    n, h, w = x.shape
    assert (h * w > SPLIT_ABOVE) == (side == "one_pixel_above") and h * w - SPLIT_ABOVE in (0, 1) and len(ranks) == 8
    xt = torch.from_numpy(x).cuda()
    got = vad.metrics.map_topk(xt, ranks)
    _check(got, want, side)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))
    few = vad.metrics.map_topk(xt, [ranks[5], ranks[0], ranks[3]])           # another number of ranks, another order
    for j, col in enumerate((5, 0, 3)):
        assert torch.equal(_bits(few["kth"][:, j]), _bits(got["kth"][:, col])) and torch.equal(_bits(few["mean"][:, j]), _bits(got["mean"][:, col]))
    solo = vad.metrics.map_topk(xt[1].contiguous(), ranks)                   # a frame alone: the same words
    assert torch.equal(_bits(solo["kth"]), _bits(got["kth"][1])) and torch.equal(_bits(solo["mean"]), _bits(got["mean"][1]))
    y = xt.clone()
    y[0, -1, -1] = float("nan")                                              # the last pixel: the slice of one pixel
    bad = vad.metrics.map_topk(y, ranks)
    assert bool((_bits(bad["kth"][0]) == ref.QNAN_BITS).all()) and bool((_bits(bad["mean"][0]) == ref.QNAN_BITS).all())
    assert torch.equal(_bits(bad["kth"][1]), _bits(got["kth"][1])) and torch.equal(_bits(bad["mean"][1]), _bits(got["mean"][1]))
    # the call captured (above the boundary: a memset and six launches) and replayed on the frames in the other order
    lib, nk = vad.hip.lib(), len(ranks)
    maps, kth, mean = xt.clone(), torch.empty(n, nk, device="cuda"), torch.empty(n, nk, device="cuda")
    need = lib.vad_topk_workspace_bytes(n, h, w, nk)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    c_ranks = (C.c_uint * nk)(*ranks)

    def call():
        vad.hip.check(lib.vad_map_topk(maps.data_ptr(), n, h, w, c_ranks, nk, kth.data_ptr(), mean.data_ptr(), ws.data_ptr(), need,
                                       vad.hip.current_stream()), "vad_map_topk")

    call()                                                                   # once eagerly, on a poisoned workspace
    assert torch.equal(_bits(kth), _bits(got["kth"])) and torch.equal(_bits(mean), _bits(got["mean"]))
    torch.cuda.synchronize()
    graph, side_stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side_stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side_stream):
        with torch.cuda.graph(graph, stream=side_stream):
            call()
    torch.cuda.current_stream().wait_stream(side_stream)
    maps.copy_(xt.flip(0))
    kth.fill_(float("nan"))
    mean.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(kth), _bits(got["kth"].flip(0))) and torch.equal(_bits(mean), _bits(got["mean"].flip(0)))


def test_empty_call(vad):
    x = torch.empty(0, 1, 16, 16, device="cuda")
    before = vad.hip.calls.get("map_topk", 0)
    got = vad.metrics.map_topk(x, [1, 2])
    assert got["kth"].shape == got["mean"].shape == (0, 1, 2) and vad.hip.calls.get("map_topk", 0) == before
    assert vad.metrics.map_topk(x, 3)["kth"].shape == (0, 1)


def test_captured_call_replays_on_new_contents(vad):
    n, h, w = 3, 16, 20
    ranks = [1, 4, 33, 320]
    nk = len(ranks)
    contents = [_maps((n, h, w), 60 + i) for i in range(4)]
    maps = torch.from_numpy(contents[0]).cuda()
    kth = torch.empty(n, nk, device="cuda")
    mean = torch.empty(n, nk, device="cuda")
    lib = vad.hip.lib()
    need = lib.vad_topk_workspace_bytes(n, h, w, nk)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    c_ranks = (C.c_uint * nk)(*ranks)

    def call():
        vad.hip.check(lib.vad_map_topk(maps.data_ptr(), n, h, w, c_ranks, nk, kth.data_ptr(), mean.data_ptr(), ws.data_ptr(), need,
                                       vad.hip.current_stream()), "vad_map_topk")

    call()                                                                   # once eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for k in range(nk):
        c_ranks[k] = 1                                                       # the ranks travelled with the captured launch
    for x in contents[1:]:
        maps.copy_(torch.from_numpy(x).cuda())
        kth.fill_(float("nan"))
        mean.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = vad.metrics.map_topk(maps, ranks)
        assert torch.equal(_bits(kth), _bits(eager["kth"])) and torch.equal(_bits(mean), _bits(eager["mean"]))
        _check({"kth": kth, "mean": mean}, ref.topk(x, ranks), "replayed")


# ------------------------------------------------------------------------------------------ with what exists
def _image_model(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32))
    labels = np.array([0, 1, 0, 1, 1, 0])
    kinds = ["good", "scratch", "good", "spot", "scratch", "good"]
    loader = [{"image": x[:4], "label": labels[:4], "defect_type": kinds[:4]}, {"image": x[4:], "label": labels[4:], "defect_type": kinds[4:]}]
    return model, loader, labels


def _video_model(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 4, 3, 3, 32, 32))
    frame_labels = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 1], [0, 0, 0]])
    loader = [{"frames": clips[:2], "frame_labels": frame_labels[:2]}, {"frames": clips[2:], "frame_labels": frame_labels[2:]}]
    return model, loader


def _host_scores(vad, maps, reduce):
    """The host route: `.cpu()` maps [..., 1, H, W] through the restatement -> (scores float32 [...], restatement dict)."""
    x = maps.cpu().numpy()
    p = x.shape[-2] * x.shape[-1]
    if reduce == "max":
        kind, rank = "kth", 1
    elif reduce[0] == "topk":
        kind, rank = "mean", ref.rank_of_fraction(reduce[1], p)
    elif reduce[0] == "quantile":
        kind, rank = "kth", ref.rank_of_quantile(reduce[1], p)
    else:
        kind, rank = "kth", reduce[1]
    want = ref.topk(x, [rank])
    want = {k: v[..., 0, 0] for k, v in want.items()}                        # drop the channel axis and the rank axis
    return kind, want


def _check_scores(scores, kind, want, what):
    got = scores.cpu()
    assert tuple(got.shape) == want[kind].shape and scores.is_cuda, what
    if kind == "kth":
        assert torch.equal(_bits(got), _bits(torch.from_numpy(want["kth"]))), what
    else:
        assert ref.mean_within_bound(got.numpy(), want), what


def test_max_of_a_smoothed_map_and_mean_of_an_error_map(vad):
    model, loader, _ = _image_model(vad)
    with torch.no_grad():
        errmap = model.score_all(loader[0]["image"].cuda())["errmap"]
    sm, mx = vad.metrics.smooth_maps(errmap, 2.0, return_max=True)
    assert torch.equal(vad.metrics.reduce_maps(sm, "max"), mx)
    assert torch.equal(vad.metrics.reduce_maps(sm, ("rank", 1)), vad.metrics.smooth_maps(errmap, 2.0, return_max="only"))
    p = 32 * 32
    top_p = vad.metrics.map_topk(errmap, p, kth=False)["mean"].cpu().numpy()
    host = errmap.cpu().numpy().reshape(4, 1, p).astype(np.float64)
    mean64 = host.mean(-1)
    bound = 0.5 * np.vectorize(ref.spacing32)(mean64) + p * 2.0 ** -52 * np.abs(host).mean(-1)
    assert top_p.shape == (4, 1) and (np.abs(top_p - mean64) <= bound + p * 2.0 ** -53 * np.abs(host).mean(-1)).all()   # numpy's own sum errs too
    assert torch.equal(vad.metrics.reduce_maps(errmap, ("topk", 1.0)), torch.from_numpy(top_p).cuda())
    assert torch.equal(vad.metrics.reduce_maps(errmap, ("quantile", 0.0)), errmap.amin((-2, -1)))


@pytest.mark.parametrize("reduce,extra", [(("topk", 0.01), {}), ("max", {"sigma": 2.0}), (("quantile", 0.99), {"morph": ("open", 3)}),
                                          (("topk", 0.1), {"calibrated": True}), (("rank", 5), {})])
def test_image_drivers_equal_the_host_route(vad, reduce, extra):
    model, loader, labels = _image_model(vad)
    kw = dict(extra)
    if kw.pop("calibrated", False):
        kw["calibration"] = vad.scoring.calibrate(model, loader, "cuda")
    host = []
    before = vad.hip.calls.get("map_topk", 0)
    for b in loader:
        scores, maps = vad.scoring.frame_scores(model, b["image"].cuda(), reduce, **kw)
        _, chain = vad.scoring.localize(model, b["image"].cuda(), 0.5, **kw)  # the maps `localize` thresholds
        assert torch.equal(maps, chain) and maps.shape == (len(b["label"]), 1, 32, 32) and scores.shape == (len(b["label"]),)
        kind, want = _host_scores(vad, maps, reduce)
        _check_scores(scores, kind, want, (reduce, extra))
        host.append(want[kind] if kind == "kth" else scores.cpu().numpy())
    assert vad.hip.calls["map_topk"] == before + 2                           # one reduction per batch
    host = np.concatenate(host)
    auroc, got_labels, scores, per = vad.scoring.compute_auroc_maps(model, loader, "cuda", reduce=reduce, **kw)
    assert scores.dtype == np.float32 and np.array_equal(scores, host) and got_labels.tolist() == labels.tolist()
    assert auroc == vad.scoring.roc_auc(labels, host)
    assert set(per) == {"good", "scratch", "spot"} and per["good"]["count"] == 3 and per["spot"]["is_anomaly"] == 1
    if not extra:
        default = vad.scoring.compute_auroc_maps(model, loader, "cuda")      # the default is the top 1 %
        assert (reduce != ("topk", 0.01)) or np.array_equal(default[2], scores)


def test_video_drivers_equal_the_host_route(vad):
    model, loader = _video_model(vad)
    m = 11
    # reduce=None is the call without the argument: the histogram of score_seq_and_frames, as before
    hand = vad.metrics.ScoreHistogram(m)
    with torch.no_grad():
        for b in loader:
            hand.accumulate(model.score_seq_and_frames(b["frames"].cuda())["frame"], torch.from_numpy(b["frame_labels"]).cuda())
    before = vad.hip.calls.get("map_topk", 0)
    auroc, tie, hist = vad.scoring.frame_auroc(model, loader, "cuda", mantissa_bits=m)
    auroc2, tie2, hist2 = vad.scoring.frame_auroc(model, loader, "cuda", mantissa_bits=m, reduce=None, sigma=2.0, morph=("open", 3))
    assert vad.hip.calls.get("map_topk", 0) == before
    assert torch.equal(hist.counts(), hand.counts()) and torch.equal(hist2.counts(), hand.counts()) and (auroc, tie) == (auroc2, tie2) == hand.auroc()

    for reduce, kw in ((("quantile", 0.99), {}), ("max", {"sigma": 2.0}), (("rank", 3), {"morph": ("close", 2)})):
        by_hand = vad.metrics.ScoreHistogram(m)
        for b in loader:
            scores, maps = vad.scoring.frame_scores(model, b["frames"].cuda(), reduce, **kw)
            assert maps.shape == (2, 3, 1, 32, 32) and scores.shape == (2, 3)
            kind, want = _host_scores(vad, maps, reduce)
            _check_scores(scores, kind, want, (reduce, kw))
            by_hand.accumulate(torch.from_numpy(want["kth"]).cuda(), torch.from_numpy(b["frame_labels"]).cuda())
        a, t, h = vad.scoring.frame_auroc(model, loader, "cuda", mantissa_bits=m, reduce=reduce, **kw)
        assert torch.equal(h.counts(), by_hand.counts()) and torch.equal(h.rejected(), by_hand.rejected()) and (a, t) == by_hand.auroc()
        assert int(h.counts().sum()) == 12 and not torch.equal(h.counts(), hand.counts())
    scores, maps = vad.scoring.frame_scores(model, loader[0]["frames"].cuda(), ("topk", 0.05))
    _check_scores(scores, *_host_scores(vad, maps, ("topk", 0.05)), "video top-k")
    with pytest.raises(vad.hip.VadError, match="error map only"):
        vad.scoring.frame_scores(model, loader[0]["frames"].cuda(), "max", map="ssim")
