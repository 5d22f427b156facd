"""Per-region overlap on the GPU (csrc/region_overlap.hip, metrics.ProHistogram): labels and region sizes `torch.equal` to the
numpy restatement (tests/pro_ref.py) on the masks that defeat a too-small iteration bound and cross every block border, the
weighted histogram's state bit for bit for every m and mask format, refusals, a captured call, and `scoring.pixel_aupro` through
the seeded image model."""
import numpy as np
import pytest
import torch

import pixel_metrics_ref as hist_ref
import pro_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

MS = (4, 11, 15)
FMTS = ("u8", "f32")
_HISTS = {}
_REFS = {}


def _hist(vad, m, which=0):
    """Two histograms per m for the whole module (the m = 15 state is 200 MB), cleared on every request."""
    if (m, which) not in _HISTS:
        _HISTS[m, which] = vad.metrics.ProHistogram(m)
    return _HISTS[m, which].reset()


def _masks():
    rng = np.random.default_rng(50)
    first, last = np.zeros((9, 13), bool), np.zeros((9, 13), bool)
    first[0, 0] = last[-1, -1] = True
    diag = np.zeros((8, 8), bool)
    diag[1:4, 1:4] = diag[4:7, 4:7] = True
    out = {"empty": np.zeros((1, 19, 23), bool), "full": np.ones((1, 19, 23), bool), "first_pixel": first[None], "last_pixel": last[None],
           "row_1x37": np.ones((1, 1, 37), bool), "column_37x1": np.ones((1, 37, 1), bool),
           "dotted_row": (np.arange(37) % 3 != 1)[None, None], "dotted_column": (np.arange(37) % 3 != 1)[None, :, None],
           "checker_37x53": (np.add.outer(np.arange(37), np.arange(53)) % 2).astype(bool)[None], "diagonal_touch": diag[None],
           "u_64": ref.u_shape(64, 64)[None], "serpentine_64": ref.serpentine(64, 64)[None], "spiral_64": ref.spiral(64)[None],
           "spiral_256": ref.spiral(256)[None], "blobs_48x80": ref.blobs(rng, 2, 48, 80), "blobs_130x70": ref.blobs(rng, 2, 130, 70, count=9, radius=9),
           "noise_33x65": rng.random((2, 33, 65)) < 0.5}
    busy = ref.blobs(rng, 2, 48, 80)
    out["empty_and_busy"] = np.stack([np.zeros((48, 80), bool), busy[0], np.ones((48, 80), bool), busy[1], np.zeros((48, 80), bool)])
    return out


MASKS = _masks()


def _want(name, connectivity):
    if (name, connectivity) not in _REFS:
        _REFS[name, connectivity] = ref.label_batch(MASKS[name], connectivity)
    return _REFS[name, connectivity]


def _encode(rng, pos, fmt):
    """bool -> mask bytes drawn from {128, 200, 255} / {0, 1, 127}, or those bytes / 255 as float32 (what ToTensor makes of them)."""
    b = np.where(pos, rng.choice(np.array([128, 200, 255], np.uint8), pos.shape), rng.choice(np.array([0, 1, 127], np.uint8), pos.shape))
    b = b.astype(np.uint8)
    assert np.array_equal(ref.positive(b, "u8"), pos)
    if fmt == "u8":
        return b
    f = b.astype(np.float32) / np.float32(255)
    assert np.array_equal(ref.positive(f, "f32"), pos)
    return f


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("connectivity", (4, 8))
@pytest.mark.parametrize("name", list(MASKS))
def test_labels_and_sizes_equal_the_reference(vad, name, connectivity, fmt):
    rng = np.random.default_rng(51 + list(MASKS).index(name))
    pos = MASKS[name]
    before = vad.hip.calls.get("label_regions", 0)
    labels, sizes = vad.metrics.label_regions(torch.from_numpy(_encode(rng, pos, fmt)).cuda(), connectivity)   # raises on a set flag
    assert vad.hip.calls["label_regions"] == before + 1
    want_labels, want_sizes = _want(name, connectivity)
    assert labels.dtype == torch.int32 and sizes.dtype == torch.uint32 and tuple(labels.shape) == pos.shape == tuple(sizes.shape)
    assert torch.equal(labels.cpu(), torch.from_numpy(want_labels))
    assert torch.equal(sizes.cpu().view(torch.int32), torch.from_numpy(want_sizes.view(np.int32)))


def test_what_the_fixtures_exercise():
    checker = MASKS["checker_37x53"]
    assert int((_want("checker_37x53", 8)[1] > 0).sum()) == 1 and int((_want("checker_37x53", 4)[1] > 0).sum()) == int(checker.sum())
    assert int((_want("diagonal_touch", 8)[1] > 0).sum()) == 1 and int((_want("diagonal_touch", 4)[1] > 0).sum()) == 2
    for name in ("u_64", "serpentine_64", "spiral_64", "spiral_256"):                     # one long 4-connected path each
        assert int((_want(name, 4)[1] > 0).sum()) == 1 and int(_want(name, 4)[1].max()) == int(MASKS[name].sum())
    assert int(MASKS["spiral_256"].sum()) > 256 * 256 // 2 - 256 and int(_want("spiral_256", 8)[0].max()) == 1


@pytest.mark.parametrize("fmt", FMTS)
def test_masks_one_element_off_their_allocation_and_other_dtypes(vad, fmt):
    rng = np.random.default_rng(52)
    pos = MASKS["blobs_48x80"]
    enc = _encode(rng, pos, fmt)
    flat = torch.zeros(enc.size + 1, dtype=torch.from_numpy(enc).dtype, device="cuda")
    flat[1:] = torch.from_numpy(enc).cuda().reshape(-1)
    sliced = flat[1:].view(*enc.shape)
    assert sliced.data_ptr() % 16 == flat.element_size() and sliced.is_contiguous()
    want_labels, want_sizes = _want("blobs_48x80", 8)
    labels, sizes = vad.metrics.label_regions(sliced)
    assert torch.equal(labels.cpu(), torch.from_numpy(want_labels)) and torch.equal(sizes.cpu().view(torch.int32), torch.from_numpy(want_sizes.view(np.int32)))
    for other in (torch.from_numpy(pos), torch.from_numpy(pos.astype(np.int64) * 3), torch.from_numpy(pos.astype(np.float64)),
                  torch.from_numpy(enc)[:, None]):                              # bool, int64, float64, [B,1,H,W]
        assert torch.equal(vad.metrics.label_regions(other.cuda())[0].cpu(), torch.from_numpy(want_labels)), other.dtype


def test_label_regions_c_abi(vad):
    """Sizes are optional; the workspace size is checked; every argument the host can see is refused by name."""
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    pos = MASKS["blobs_48x80"]
    n, h, w = pos.shape
    mask = torch.from_numpy(pos.astype(np.uint8) * 255).cuda()
    need = lib.vad_pro_workspace_bytes(n, h, w)
    assert need == 16 + 8 * n * h * w and lib.vad_pro_workspace_bytes(2, 3, 4) == 16 + 8 * 24
    assert lib.vad_pro_workspace_bytes(1, 0, 5) == 0 and lib.vad_pro_workspace_bytes(-1, 4, 4) == 0 and lib.vad_pro_workspace_bytes(1, 65536, 32768) == 0
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    labels = torch.full((n, h, w), -7, dtype=torch.int32, device="cuda")
    assert lib.vad_label_regions(mask.data_ptr(), 0, n, h, w, 8, labels.data_ptr(), None, ws.data_ptr(), need, stream) == 0
    assert torch.equal(labels.cpu(), torch.from_numpy(_want("blobs_48x80", 8)[0])) and int(ws[:4].view(torch.int32).item()) == 0
    before = labels.clone()
    a = (mask.data_ptr(), 0, n, h, w, 8, labels.data_ptr(), None, ws.data_ptr(), need, stream)
    for pos_, bad, word in ((0, None, b"masks"), (1, 2, b"label_format"), (2, -1, b"n must"), (3, 0, b"h and w"), (4, -3, b"h and w"),
                            (5, 6, b"connectivity"), (6, None, b"labels is NULL"), (8, None, b"ws is NULL"), (8, ws.data_ptr() + 4, b"16-byte"),
                            (9, need - 1, b"ws_bytes")):
        args = list(a)
        args[pos_] = bad
        assert lib.vad_label_regions(*args) == -1 and word in lib.vad_last_error(), (pos_, lib.vad_last_error())
    assert lib.vad_label_regions(mask.data_ptr(), 0, 1, 65536, 32768, 8, labels.data_ptr(), None, ws.data_ptr(), need, stream) == -1
    assert b"2^31 - 1" in lib.vad_last_error()
    assert lib.vad_label_regions(mask.data_ptr(), 0, 0, h, w, 8, labels.data_ptr(), None, ws.data_ptr(), need, stream) == 0   # nothing to label
    torch.cuda.synchronize()
    assert torch.equal(labels, before)
    VadError = vad.hip.VadError
    with pytest.raises(VadError, match="connectivity"):
        vad.metrics.label_regions(mask, 6)
    with pytest.raises(VadError, match="masks must be"):
        vad.metrics.label_regions(mask[0, 0])
    with pytest.raises(VadError, match="no CPU fallback"):
        vad.metrics.label_regions(mask.cpu())


# ------------------------------------------------------------------------------------------ the weighted histogram
def _values(rng, shape, pos):
    """Scores over many exponents, higher inside the regions, with exact repeats, zeros and - in both classes - negatives, NaNs
    and infinities."""
    n = int(np.prod(shape))
    v = (np.exp(rng.standard_normal(n) * 3.0) * 1e-3).astype(np.float32) * np.where(pos.reshape(-1), np.float32(4), np.float32(1))
    v[rng.random(n) < 0.2] = np.float32(0.015625)
    v[rng.random(n) < 0.05] = 0.0
    v[rng.random(n) < 0.03] = -1.0
    v[rng.random(n) < 0.01] = np.nan
    v[rng.random(n) < 0.01] = np.inf
    v[rng.random(n) < 0.005] = -0.0
    return v.astype(np.float32).reshape(shape)


def _batch(seed):
    rng = np.random.default_rng(seed)
    pos = np.concatenate([ref.blobs(rng, 3, 40, 56), np.zeros((1, 40, 56), bool)])       # the last image is a good one
    pos[2, 5:30, 10:50] = True                                                            # one large region among the small ones
    return rng, pos, _values(rng, pos.shape, pos)


def _assert_state(h, st):
    assert torch.equal(h._words().cpu(), torch.from_numpy(ref.state_words(st)))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("m", MS)
def test_state_equals_the_reference(vad, m, fmt):
    rng, pos, v = _batch(60 + FMTS.index(fmt))
    labels, _ = ref.label_batch(pos, 8)
    st = ref.ref_state(v, pos, labels, m)
    assert st["rejected"].min() > 0 and st["regions"] > 3 and st["max_region"] >= 1000
    vt, mt = torch.from_numpy(v).cuda(), torch.from_numpy(_encode(rng, pos, fmt)).cuda()
    before = vad.hip.calls.get("pro_accumulate", 0)
    h = _hist(vad, m).accumulate(vt[:, None], mt)                                         # [B,1,H,W] values with [B,H,W] masks
    assert vad.hip.calls["pro_accumulate"] == before + 1
    _assert_state(h, st)
    assert h.flags() == 0 and h.regions() == st["regions"] and h.max_region() == st["max_region"]
    assert h.rejected().tolist() == st["rejected"].tolist()
    counts = hist_ref.ref_counts(v, pos, m)[0]
    assert torch.equal(h.counts().cpu(), torch.from_numpy(counts))                        # what ScoreHistogram would hold
    assert torch.equal(h.weighted().cpu(), torch.from_numpy(ref.wpos_bits(st["wpos"])))
    # per-image calls, in reverse order: the same bits
    h = _hist(vad, m)
    for i in reversed(range(len(v))):
        h.accumulate(vt[i:i + 1], mt[i:i + 1, None])
    _assert_state(h, st)
    # two states merged: the same bits; the source is unchanged
    a, b = _hist(vad, m).accumulate(vt[:1], mt[:1]), _hist(vad, m, 1).accumulate(vt[1:], mt[1:])
    part = ref.ref_state(v[1:], pos[1:], labels[1:], m)
    a.merge(b)
    _assert_state(a, st)
    _assert_state(b, part)
    assert st["max_region"] == part["max_region"] > ref.ref_state(v[:1], pos[:1], labels[:1], m)["max_region"]
    if m == 11:
        want = vad.metrics.aupro_from_counts(ref.wpos_bits(st["wpos"]), st["neg"], st["regions"], st["max_region"], 0.3)
        assert a.aupro() == want and a.auroc() == vad.metrics.auroc_from_counts(counts)
        fpr, pro, thr = a.pro_curve()
        assert fpr[-1] == 1.0 and 0.0 < pro[-1] <= 1.0 and len(fpr) == len(pro) == len(thr)
        sd = a.state_dict()
        assert sd["regions"] == st["regions"] and sd["connectivity"] == 8
        again = _hist(vad, m, 1).load_state_dict(sd)
        assert torch.equal(again._state, a._state)


def test_connectivity_4_counts_other_regions(vad):
    m = 4
    pos = np.stack([MASKS["checker_37x53"][0], MASKS["diagonal_touch"][0].repeat(5, 0).repeat(7, 1)[:37, :53]])
    rng = np.random.default_rng(61)
    v = _values(rng, pos.shape, pos)
    vt, mt = torch.from_numpy(v).cuda(), torch.from_numpy(pos).cuda()
    for connectivity in (4, 8):
        labels, _ = ref.label_batch(pos, connectivity)
        st = ref.ref_state(v, pos, labels, m)
        h = vad.metrics.ProHistogram(m, connectivity=connectivity).accumulate(vt, mt)
        _assert_state(h, st)
    assert st["regions"] == 2


def test_one_region_per_pixel_and_one_bin(vad):
    """Full contention on the weighted path: a constant map over a full mask (one (key, region) pair for every wave) and over a
    4-connected checkerboard (every anomalous pixel its own region of weight 2^44)."""
    m = 11
    key = 0x3E800000 >> (23 - m)
    const = torch.full((2, 37, 53), 0.25, device="cuda")
    full = torch.ones(2, 37, 53, dtype=torch.uint8, device="cuda") * 255
    full[1, 36, 52] = 0                                                                   # one normal pixel
    h = _hist(vad, m).accumulate(const, full)
    sizes = (37 * 53, 37 * 53 - 1)
    assert h.regions() == 2 and h.max_region() == sizes[0] and h.flags() == 0
    assert int(h.weighted()[key]) == sum(s * ref.weight(s) for s in sizes) and int(h.weighted().ne(0).sum()) == 1
    assert h.counts()[:, key].tolist() == [1, sum(sizes)]
    checker = torch.from_numpy(MASKS["checker_37x53"]).cuda()
    h = vad.metrics.ProHistogram(m, connectivity=4).accumulate(const[:1], checker)
    k = int(MASKS["checker_37x53"].sum())
    assert h.regions() == k and h.max_region() == 1 and int(h.weighted()[key]) == k << 44
    aupro, quant_bound, weight_bound = h.aupro(1.0)
    assert aupro == 0.5 and quant_bound == 0.5 and weight_bound == 2.0 ** -45             # one shared bin: the diagonal, and its bound


def test_refusals_leave_the_state_unchanged(vad):
    VadError = vad.hip.VadError
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    rng, pos, v = _batch(62)
    n, hh, w = pos.shape
    vt, mt = torch.from_numpy(v).cuda(), torch.from_numpy(pos.astype(np.uint8) * 255).cuda()
    h = vad.metrics.ProHistogram(4).accumulate(vt, mt)
    other = vad.metrics.ProHistogram(11)
    before, other_before = h._state.clone(), other._state.clone()
    need = lib.vad_pro_workspace_bytes(n, hh, w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a = (vt.data_ptr(), mt.data_ptr(), 0, n, hh, w, 8, h._state.data_ptr(), 4, ws.data_ptr(), need, stream)
    for pos_, bad, word in ((0, None, b"values"), (1, None, b"masks"), (2, 2, b"label_format"), (3, -1, b"n must"), (4, 0, b"h and w"),
                            (6, 5, b"connectivity"), (7, None, b"state is NULL"), (7, h._state.data_ptr() + 8, b"state must be 16-byte"),
                            (8, 3, b"m (mantissa_bits)"), (8, 16, b"m (mantissa_bits)"), (9, None, b"ws is NULL"), (10, need - 1, b"ws_bytes")):
        args = list(a)
        args[pos_] = bad
        assert lib.vad_pro_accumulate(*args) == -1 and word in lib.vad_last_error(), (pos_, lib.vad_last_error())
    for bad in (3, 16):
        assert lib.vad_pro_state_bytes(bad) == 0
        assert lib.vad_pro_reset(h._state.data_ptr(), bad, stream) == -1 and b"m (mantissa_bits)" in lib.vad_last_error()
        assert lib.vad_pro_merge(h._state.data_ptr(), other._state.data_ptr(), bad, stream) == -1
        with pytest.raises(VadError, match="mantissa_bits"):
            vad.metrics.ProHistogram(bad)
    assert lib.vad_pro_merge(h._state.data_ptr(), h._state.data_ptr(), 4, stream) == -1 and b"same state" in lib.vad_last_error()
    assert lib.vad_pro_state_bytes(4) == 16 + 8 * (3 * (255 << 4) + 5) == h._state.numel()
    # a state built for another m: the kernels compare the header on the device - the call changes nothing and follows no offset
    # of the smaller blob - and the Python layer, which knows both widths, refuses by name
    args = list(a)
    args[8] = 11
    assert lib.vad_pro_accumulate(*args) == 0
    assert lib.vad_pro_merge(h._state.data_ptr(), other._state.data_ptr(), 11, stream) == 0
    assert lib.vad_pro_merge(other._state.data_ptr(), h._state.data_ptr(), 11, stream) == 0
    score_hist = vad.metrics.ScoreHistogram(4)                                            # the other kind of blob of the same m
    args = list(a)
    args[7] = score_hist._state.data_ptr()
    sh_before = score_hist._state.clone()
    assert lib.vad_pro_accumulate(*args) == 0
    with pytest.raises(VadError, match="mantissa_bits"):
        h.merge(other)
    with pytest.raises(VadError, match="connectivity"):
        h.merge(vad.metrics.ProHistogram(4, connectivity=4))
    with pytest.raises(VadError, match="mantissa_bits"):
        h.load_state_dict(other.state_dict())
    with pytest.raises(VadError, match="connectivity"):
        h.load_state_dict({**h.state_dict(), "connectivity": 4})
    with pytest.raises(VadError, match="ProHistogram"):
        h.merge(score_hist)
    with pytest.raises(VadError, match="masks"):
        h.accumulate(vt, mt[:2])
    with pytest.raises(VadError, match="masks"):
        h.accumulate(vt, mt[:, :, :-1])
    with pytest.raises(VadError, match="values must be float32"):
        h.accumulate(vt.double(), mt)
    with pytest.raises(VadError, match=r"values must be \[B,1,H,W\]"):
        h.accumulate(vt.reshape(-1), mt)
    with pytest.raises(VadError, match="no CPU fallback"):
        h.accumulate(vt.cpu(), mt.cpu())
    with pytest.raises(VadError, match="no CPU fallback"):
        h.accumulate(vt, mt.cpu())
    with pytest.raises(ValueError, match="fpr_limit"):
        h.aupro(0.0)
    with pytest.raises(ValueError, match="no region"):
        other.aupro()
    h.accumulate(vt[:0], mt[:0])                                                          # nothing to add
    torch.cuda.synchronize()
    assert torch.equal(h._state, before) and torch.equal(other._state, other_before) and torch.equal(score_hist._state, sh_before)
    # a set flag word is an error wherever the counters are read
    flagged = vad.metrics.ProHistogram(4).load_state_dict({**h.state_dict(), "flags": 1})
    for read in (flagged.aupro, flagged.regions, flagged.pro_curve):
        with pytest.raises(VadError, match="flags"):
            read()


def test_accumulate_in_a_captured_graph(vad):
    """`accumulate` keeps its workspace, allocates nothing once it has it and never synchronises: captured by hip.CapturedCall on a
    single stream, one replay adds the batch once."""
    m = 11
    rng, pos, v = _batch(63)
    labels, _ = ref.label_batch(pos, 8)
    st = ref.ref_state(v, pos, labels, m)
    vt, mt = torch.from_numpy(v).cuda(), torch.from_numpy(_encode(rng, pos, "f32")).cuda()
    h = vad.metrics.ProHistogram(m).accumulate(vt, mt)                                     # the eager call that sizes the workspace
    h.reset()
    torch.cuda.synchronize()
    g = vad.hip.CapturedCall(lambda: h.accumulate(vt, mt), vt, h, keep=(vt, mt, h))
    torch.cuda.synchronize()
    assert int(h._words().ne(0).sum()) == 0                                               # capturing records, it does not run
    g.replay()
    _assert_state(h, st)


# ------------------------------------------------------------------------------------------ through the image model
def test_pixel_aupro_through_the_image_model(vad):
    m = 11
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 6, 3, 32, 32))
    rng = np.random.default_rng(12)
    raw = np.zeros((6, 48, 40), np.uint8)
    for i in range(6):                                                      # blocks of 0 / 127 / 128 / 255 at camera resolution
        raw[i] = np.kron(rng.choice(np.array([0, 127, 128, 255], np.uint8), (6, 5), p=[0.55, 0.1, 0.1, 0.25]), np.ones((8, 8), np.uint8))
    masks = vad.scoring.resize_masks(torch.from_numpy(raw).cuda(), 32)
    assert masks.shape == (6, 1, 32, 32) and masks.dtype == torch.float32
    loader = [{"image": x[:4], "mask": masks[:4]}, {"image": x[4:], "mask": masks[4:]}]
    pos = masks.cpu().numpy()[:, 0] > np.float32(0.5)
    labels, _ = ref.label_batch(pos, 8)
    with torch.no_grad():
        maps = {"mse": torch.cat([model.score_all(b["image"].cuda())["errmap"] for b in loader]).cpu().numpy()[:, 0],
                "ssim": torch.cat([model.score_criteria(b["image"].cuda(), ssim_map=True)["ssim_map"] for b in loader]).cpu().numpy()[:, 0]}
    for kind in ("mse", "ssim"):
        before = vad.hip.calls.get("pro_accumulate", 0)
        aupro, quant_bound, weight_bound, hist = vad.scoring.pixel_aupro(model, loader, "cuda", map=kind, mantissa_bits=m)
        assert vad.hip.calls["pro_accumulate"] == before + 2               # one accumulate per batch
        st = ref.ref_state(maps[kind], pos, labels, m)
        print(f"{kind}: aupro {aupro!r} quant_bound {quant_bound!r} weight_bound {weight_bound!r} regions {st['regions']} "
              f"max_region {st['max_region']} rejected {st['rejected'].tolist()}")
        _assert_state(hist, st)
        assert (aupro, quant_bound, weight_bound) == vad.metrics.aupro_from_counts(ref.wpos_bits(st["wpos"]), st["neg"], st["regions"],
                                                                                   st["max_region"], 0.3)
        assert st["rejected"].sum() == 0 and st["regions"] >= 6 and weight_bound == st["max_region"] / 2.0 ** 45
        exact = ref.aupro_oracle(maps[kind], labels, pos, 0.3)
        assert abs(aupro - exact) <= quant_bound + weight_bound + 1e-12, (aupro, exact, quant_bound, weight_bound)
        assert hist.auroc() == vad.metrics.auroc_from_counts(hist_ref.ref_counts(maps[kind], pos, m)[0])
    # uint8 masks mean the same pixels; a histogram handed in is continued; another limit and connectivity
    u8 = masks.mul(255).round().to(torch.uint8)
    a2, _, _, h2 = vad.scoring.pixel_aupro(model, [{"image": x, "mask": u8}], "cuda", mantissa_bits=m, fpr_limit=1.0)
    st = ref.ref_state(maps["mse"], pos, labels, m)
    assert torch.equal(h2.weighted().cpu(), torch.from_numpy(ref.wpos_bits(st["wpos"]))) and h2.regions() == st["regions"]
    assert abs(a2 - ref.aupro_oracle(maps["mse"], labels, pos, 1.0)) <= h2.aupro(1.0)[1] + h2.aupro(1.0)[2] + 1e-12
    _, _, _, h3 = vad.scoring.pixel_aupro(model, loader, "cuda", hist=h2)
    assert h3 is h2 and h3.regions() == 2 * st["regions"] and int(h3.counts().sum()) == 2 * 6 * 32 * 32
    _, _, _, h4 = vad.scoring.pixel_aupro(model, loader, "cuda", mantissa_bits=m, connectivity=4)
    assert h4.connectivity == 4 and h4.regions() == int((ref.label_batch(pos, 4)[1] > 0).sum())
    with pytest.raises(vad.hip.VadError, match="map"):
        vad.scoring.pixel_aupro(model, loader, "cuda", map="psnr")
