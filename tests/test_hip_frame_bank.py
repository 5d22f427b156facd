"""The frame bank on the device: `vad_gather_frames_u8` (csrc/frame_gather.hip), `FrameBank` end to end, its loaders feeding
`scoring.score_clips` and both trainers' `train_epoch`.  Every comparison is `torch.equal`: the gather is a copy plus a
normalisation whose 256 results are defined bit for bit (`synth.u8_to_unit` = `vad_norm_u8`), and the steps downstream of equal
inputs are deterministic.  The oracle is tests/frame_bank_ref.py.  Shapes are the smallest at which the kernels can go wrong:
(16,16), (16,48), (32,32), (64,64) take the 16-byte paths ((64,64) with more than one block per frame), (1,1), (3,5), (17,23)
the plain ones."""
import numpy as np
import pytest
import torch

import frame_bank_ref as B
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (16, 16), (16, 48), (17, 23), (32, 32), (64, 64)]
FRAMES = 9
# lengths 1..12; repeats, descending runs, frame 0 and frame F-1
BASE = [8, 0, 3, 3, 7, 6, 5, 0, 8, 8, 1, 4]
INDEX_LISTS = [BASE[:k] for k in range(1, 13)] + [[0], [8, 7, 6, 5, 4, 3, 2, 1, 0], [4, 4, 4, 4]]
POISON_F32, POISON_U8 = -12345.5, 0xA5
GUARD = 256


def _want(vad, bank_np, index, fmt):
    u8 = bank_np[np.asarray(index, np.int64)]
    if fmt == "u8":
        return torch.from_numpy(np.ascontiguousarray(u8))
    return torch.from_numpy(B.normalised_ref(vad.synth.u8_to_unit, u8))


def _guarded_out(n, h, w, fmt):
    """`out` carved from a larger buffer with GUARD poisoned bytes on each side; returns (whole buffer, the out view)."""
    nbytes = n * h * w * 3 * (4 if fmt == "f32" else 1)
    raw = torch.full((GUARD + nbytes + GUARD,), POISON_U8, dtype=torch.uint8, device="cuda")
    body = raw[GUARD:GUARD + nbytes]
    if fmt == "f32":
        out = body.view(torch.float32).view(n, 3, h, w)
        out.fill_(POISON_F32)
    else:
        out = body.view(n, h, w, 3)
    return raw, out


def _guards_intact(raw):
    return bool((raw[:GUARD] == POISON_U8).all()) and bool((raw[-GUARD:] == POISON_U8).all())


def _raw_gather(vad, bank_dev, bank_frames, index, h, w, fmt, out):
    idx = torch.tensor(index, dtype=torch.int64, device="cuda")
    rc = vad.hip.lib().vad_gather_frames_u8(bank_dev.data_ptr(), bank_frames, idx.data_ptr(), len(index), h, w,
                                            vad.hip.X_F32_NCHW if fmt == "f32" else vad.hip.X_U8_NHWC, out.data_ptr(),
                                            vad.hip.current_stream())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ 1. kernel exactness
@pytest.mark.parametrize("fmt", ["f32", "u8"])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_gather_is_exact(vad, hw, fmt):
    h, w = hw
    rounds = B.all_bytes_rounds(FRAMES, h, w)                 # 1 unless the whole bank has fewer than 256 pixels
    seen = np.zeros((3, 256), bool)
    for r in range(rounds):
        bank_np = B.all_bytes_bank(FRAMES, h, w, offset=r * FRAMES * h * w)
        for c in range(3):
            seen[c, bank_np[..., c].reshape(-1)] = True
        bank_dev = torch.from_numpy(bank_np).cuda()
        for index in (INDEX_LISTS if r == 0 else [list(range(FRAMES))]):
            raw, out = _guarded_out(len(index), h, w, fmt)
            assert _raw_gather(vad, bank_dev, FRAMES, index, h, w, fmt, out) == 0
            assert torch.equal(out.cpu(), _want(vad, bank_np, index, fmt)), (hw, fmt, index)
            assert _guards_intact(raw), (hw, fmt, index)
    assert seen.all()                                         # every byte value went through every channel


@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_bank_pointer_inside_an_allocation(vad, fmt):
    """The bank is a view starting at frame 1 of a (17, 23) bank: 1173 bytes in, an odd address."""
    h, w = 17, 23
    bank_np = B.all_bytes_bank(FRAMES, h, w)
    whole = torch.from_numpy(bank_np).cuda()
    view = whole[1:]
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 2 == 1
    index = [7, 0, 0, 3, 2, 1]
    raw, out = _guarded_out(len(index), h, w, fmt)
    assert _raw_gather(vad, view, FRAMES - 1, index, h, w, fmt, out) == 0
    assert torch.equal(out.cpu(), _want(vad, bank_np[1:], index, fmt))
    assert _guards_intact(raw)


@pytest.mark.parametrize("fmt", ["f32", "u8"])
def test_misaligned_addresses_with_a_vector_shape(vad, fmt):
    """A shape whose frames are multiples of 16 bytes, at addresses that are not: bank 1 byte (f32 out 4 bytes, u8 out 1 byte)
    into an allocation.  The launcher must take the plain path from the addresses, not from the shape."""
    h, w = 16, 16
    bank_np = B.all_bytes_bank(FRAMES, h, w)
    buf = torch.zeros(bank_np.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(bank_np).cuda().flatten()
    index = [8, 0, 5, 5]
    want = _want(vad, bank_np, index, fmt)
    for shift_bank, shift_out in ((1, 0), (0, 1), (1, 1)):
        bank_dev = buf[1:] if shift_bank else torch.from_numpy(bank_np).cuda()
        elem = 4 if fmt == "f32" else 1
        raw = torch.full((GUARD + want.numel() * elem + 16 + GUARD,), POISON_U8, dtype=torch.uint8, device="cuda")
        start = GUARD + (elem if shift_out else 0)               # 256 is 16-aligned within a fresh allocation
        body = raw[start:start + want.numel() * elem]
        out = body.view(torch.float32).view(want.shape) if fmt == "f32" else body.view(want.shape)
        assert (out.data_ptr() % 16 != 0) == bool(shift_out)
        assert _raw_gather(vad, bank_dev, FRAMES, index, h, w, fmt, out) == 0
        assert torch.equal(out.cpu(), want), (shift_bank, shift_out)
        assert bool((raw[:start] == POISON_U8).all()) and bool((raw[start + want.numel() * elem:] == POISON_U8).all())


# ------------------------------------------------------------------------------------------------ 2. guards
@pytest.mark.parametrize("fmt", ["f32", "u8"])
@pytest.mark.parametrize("hw", [(16, 16), (17, 23)], ids=["vector", "plain"])
def test_out_of_range_indices_skip_their_frames(vad, hw, fmt):
    h, w = hw
    bank_np = B.all_bytes_bank(FRAMES, h, w)
    bank_dev = torch.from_numpy(bank_np).cuda()
    index = [2, FRAMES, 0, -1, FRAMES - 1]
    raw, out = _guarded_out(len(index), h, w, fmt)
    assert _raw_gather(vad, bank_dev, FRAMES, index, h, w, fmt, out) == 0          # the host cannot see device indices: success
    got = out.cpu()
    for i, f in enumerate(index):
        if 0 <= f < FRAMES:
            assert torch.equal(got[i], _want(vad, bank_np, [f], fmt)[0]), (i, f)
        elif fmt == "f32":
            assert bool((got[i] == POISON_F32).all()), (i, f)
        else:
            assert bool((got[i] == POISON_U8).all()), (i, f)
    assert _guards_intact(raw)


# ------------------------------------------------------------------------------------------------ 3. ABI refusals
def test_abi_refusals(vad):
    l, h, w = vad.hip.lib(), 16, 16
    bank = torch.from_numpy(B.all_bytes_bank(FRAMES, h, w)).cuda()
    idx = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    raw, out = _guarded_out(2, h, w, "f32")
    F32, U8, s = vad.hip.X_F32_NCHW, vad.hip.X_U8_NHWC, vad.hip.current_stream()
    cases = [
        ((None, FRAMES, idx.data_ptr(), 2, h, w, F32, out.data_ptr(), s), "bank is NULL"),
        ((bank.data_ptr(), FRAMES, None, 2, h, w, F32, out.data_ptr(), s), "index is NULL"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, h, w, F32, None, s), "out is NULL"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, 0, w, F32, out.data_ptr(), s), "h and w must be positive"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, h, -3, U8, out.data_ptr(), s), "h and w must be positive"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), -1, h, w, F32, out.data_ptr(), s), "n must be >= 0"),
        ((bank.data_ptr(), 0, idx.data_ptr(), 2, h, w, F32, out.data_ptr(), s), "bank_frames must be positive"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, h, w, 2, out.data_ptr(), s), "out_format must be"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, h, w, -1, out.data_ptr(), s), "out_format must be"),
        ((bank.data_ptr(), FRAMES, idx.data_ptr(), 2, h, w, F32, out.data_ptr() + 2, s), "4-byte aligned"),
    ]
    for args, text in cases:
        assert l.vad_gather_frames_u8(*args) == -1, text                          # VAD_ERR_ARG
        assert text in l.vad_last_error().decode(), (text, l.vad_last_error())
    # a uint8 out has no alignment rule; n == 0 is not an error and launches nothing
    assert l.vad_gather_frames_u8(bank.data_ptr(), FRAMES, idx.data_ptr(), 0, h, w, F32, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert bool((out == POISON_F32).all()) and _guards_intact(raw)                # nothing above wrote anything
    raw8, out8 = _guarded_out(2, h, w, "u8")
    assert l.vad_gather_frames_u8(bank.data_ptr(), FRAMES, idx.data_ptr(), 1, h, w, U8, out8.data_ptr() + 1, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw8[GUARD + 1:GUARD + 1 + h * w * 3], bank[0].flatten()) and _guards_intact(raw8)


# ------------------------------------------------------------------------------------------------ 4. FrameBank end to end
SIZE, T = 32, 3


def _camera_videos():
    """Three videos at their own resolutions: 37x53 RGB, 64x48 mode L (one byte per pixel), and one already 32x32."""
    return [B.video_u8(21, 7, 37, 53), B.video_u8(22, 5, 64, 48, channels=1), B.video_u8(23, 6, SIZE, SIZE)]


@pytest.fixture(scope="module")
def resized():
    """The oracle's bank contents per video (PIL's resize, restated), computed once."""
    return [B.resized_ref(v, SIZE) for v in _camera_videos()]


def _fill(vad, on_gpu, capacity=None):
    bank = vad.FrameBank(SIZE, capacity_frames=capacity)
    vids = _camera_videos()
    meta = []
    for i, v in enumerate(vids):
        t = torch.from_numpy(v)
        fl = (np.arange(len(v)) == 2).astype(np.int64)
        bank.add_video(t.cuda() if on_gpu else t, video_id=f"v{i}", frame_labels=fl, pixel_format="l" if v.ndim == 3 else None)
        meta.append({"n": len(v), "video_id": f"v{i}", "label": 0, "frame_labels": fl})
    return bank, meta


@pytest.mark.parametrize("on_gpu", [False, True], ids=["cpu_frames", "gpu_frames"])
def test_bank_end_to_end(vad, resized, on_gpu):
    bank, meta = _fill(vad, on_gpu, capacity=2)                      # reallocates twice: 7 -> 14 -> 28 frames
    assert bank.num_frames == 18 and bank.capacity_frames >= 18
    assert torch.equal(bank.frames.cpu(), torch.from_numpy(np.concatenate(resized)))      # earlier frames survived the growth
    seqs = B.sequences_ref(meta, T, 2)
    ids = [len(seqs) - 1, 0, 3, 3, 1]
    want_f, want_u = B.clips_ref(vad.synth.u8_to_unit, resized, seqs, ids, T)
    before = vad.hip.calls.get("gather_frames", 0)
    got_f = bank.batch(ids, T, stride=2)
    got_u = bank.batch(torch.tensor(ids), T, dtype=torch.uint8, stride=2)
    assert vad.hip.calls["gather_frames"] == before + 2              # one launch per batch
    assert got_f.dtype == torch.float32 and tuple(got_f.shape) == (5, T, 3, SIZE, SIZE) and got_f.is_contiguous()
    assert got_u.dtype == torch.uint8 and tuple(got_u.shape) == (5, T, SIZE, SIZE, 3)
    assert torch.equal(got_f.cpu(), torch.from_numpy(want_f)) and torch.equal(got_u.cpu(), torch.from_numpy(want_u))
    with pytest.raises(vad.hip.VadError, match="seq_ids"):
        bank.batch([len(seqs)], T, stride=2)
    # the loader: collated like default_collate, in sequence order
    batches = list(bank.loader(T, 2, 4))
    assert [len(b["label"]) for b in batches] == [4] * (len(seqs) // 4) + ([len(seqs) % 4] if len(seqs) % 4 else [])
    at = 0
    for b in batches:
        k = len(b["label"])
        part = seqs[at:at + k]
        wf, _ = B.clips_ref(vad.synth.u8_to_unit, resized, seqs, range(at, at + k), T)
        assert torch.equal(b["frames"].cpu(), torch.from_numpy(wf))
        assert b["label"].dtype == torch.int64 and not b["label"].is_cuda and b["label"].tolist() == [s["label"] for s in part]
        assert b["start_frame"].tolist() == [s["start_frame"] for s in part] and b["video_id"] == [s["video_id"] for s in part]
        assert b["frame_labels"].tolist() == [s["frame_labels"].tolist() for s in part]
        at += k
    assert at == len(seqs) and {0, 1} == {s["label"] for s in seqs}


def test_image_loader_batches(vad, resized):
    bank = vad.FrameBank(SIZE)
    cam = B.video_u8(21, 7, 37, 53)
    labels = [0, 1, 0, 0, 1, 0, 1]
    bank.add_images(torch.from_numpy(cam), labels, defect_types=[f"d{l}" for l in labels])
    g = torch.Generator().manual_seed(9)
    order = list(torch.utils.data.RandomSampler(range(7), generator=torch.Generator().manual_seed(9)))
    batches = list(bank.image_loader(3, shuffle=True, generator=g))
    assert [len(b["label"]) for b in batches] == [3, 3, 1]
    want = torch.from_numpy(B.normalised_ref(vad.synth.u8_to_unit, resized[0][order]))
    assert torch.equal(torch.cat([b["image"] for b in batches]).cpu(), want)
    assert torch.cat([b["label"] for b in batches]).tolist() == [labels[i] for i in order]
    assert sum((b["defect_type"] for b in batches), []) == [f"d{labels[i]}" for i in order]
    u8 = list(bank.image_loader(7, dtype=torch.uint8))[0]["image"]
    assert torch.equal(u8.cpu(), torch.from_numpy(resized[0]))


# ------------------------------------------------------------------------------------------------ 5. scoring
def test_scoring_from_uint8_and_float_loaders(vad, resized):
    bank, meta = _fill(vad, on_gpu=True)
    model = vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 31)
    model = model.cuda().eval()
    S = vad.scoring
    from_u8 = S.score_clips(model, bank.loader(T, 1, 4, dtype=torch.uint8), "cuda", per_frame=True)
    from_f32 = S.score_clips(model, bank.loader(T, 1, 4), "cuda", per_frame=True)
    seqs = B.sequences_ref(meta, T, 1)
    oracle = []
    for at in range(0, len(seqs), 4):
        ids = range(at, min(at + 4, len(seqs)))
        wf, _ = B.clips_ref(vad.synth.u8_to_unit, resized, seqs, ids, T)
        oracle.append({"frames": torch.from_numpy(wf), "label": torch.tensor([seqs[i]["label"] for i in ids])})
    from_oracle = S.score_clips(model, oracle, "cuda", per_frame=True)
    assert len(from_u8[0]) == len(seqs) and from_u8[2].shape == (len(seqs), T)
    for a, b, c in zip(from_u8, from_f32, from_oracle):
        assert a.dtype == b.dtype == c.dtype and np.array_equal(a, b) and np.array_equal(b, c)
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))


# ------------------------------------------------------------------------------------------------ 6. training
def _state(tr):
    bufs = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    return bufs, tr.exp_avg.clone(), tr.exp_avg_sq.clone()


def _same_state(a, b):
    sa, sb = _state(a), _state(b)
    assert sa[0].keys() == sb[0].keys()
    for k in sa[0]:
        assert torch.equal(sa[0][k], sb[0][k]), k                      # parameters, BatchNorm buffers, num_batches_tracked
    assert torch.equal(sa[1], sb[1]) and torch.equal(sa[2], sb[2])      # Adam moments
    assert a.steps == b.steps


def test_video_train_epoch_from_the_bank(vad, resized):
    bank, meta = _fill(vad, on_gpu=False)
    seqs = B.sequences_ref(meta, T, 2)
    assert len(seqs) == 7                                             # drop_last: 3 batches of 2 clips x 3 frames at 32x32

    def trainer():
        m = vad.VideoAutoencoder(in_channels=3, latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
        load_synthetic(vad, m, 41)
        return vad.VideoTrainer(m.cuda())

    a, b = trainer(), trainer()
    before = vad.hip.calls.get("gather_frames", 0)
    got = a.train_epoch(bank.loader(T, 2, 2, drop_last=True))
    assert vad.hip.calls["gather_frames"] == before + 3
    total = 0.0
    for at in range(0, 6, 2):
        wf, _ = B.clips_ref(vad.synth.u8_to_unit, resized, seqs, range(at, at + 2), T)
        total += b.step(torch.from_numpy(wf).cuda()).item()
    assert isinstance(got, float) and got == total / 3
    _same_state(a, b)
    with pytest.raises(ValueError):
        a.train_epoch([])


def test_image_train_epoch_from_the_bank(vad, resized):
    bank = vad.FrameBank(SIZE)
    bank.add_images(torch.from_numpy(B.video_u8(21, 7, 37, 53))[:6], [0] * 6)

    def trainer():
        m = vad.ConvAutoencoder(in_channels=3, latent_dim=32)
        load_synthetic(vad, m, 42)
        return vad.ImageTrainer(m.cuda())

    a, b = trainer(), trainer()
    before = vad.hip.calls.get("gather_frames", 0)
    got = a.train_epoch(bank.image_loader(2))
    assert vad.hip.calls["gather_frames"] == before + 3
    total = 0.0
    for at in range(0, 6, 2):
        total += b.step(torch.from_numpy(B.normalised_ref(vad.synth.u8_to_unit, resized[0][at:at + 2])).cuda()).item()
    assert got == total / 3
    _same_state(a, b)


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_gather_captured_in_a_graph_follows_the_bank(vad):
    h = w = 16
    first, second = B.all_bytes_bank(FRAMES, h, w), B.all_bytes_bank(FRAMES, h, w, offset=101)
    bank = vad.FrameBank(h, capacity_frames=FRAMES)
    bank.add_video(torch.from_numpy(first))
    index = [8, 0, 3, 3]
    idx = torch.tensor(index, dtype=torch.int64, device="cuda")
    out = torch.empty(len(index), 3, h, w, device="cuda")
    bank.gather(idx, out=out)                                        # once eagerly
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            bank.gather(idx, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.fill_(POISON_F32)
    graph.replay()
    assert torch.equal(out.cpu(), _want(vad, first, index, "f32"))
    bank.frames.copy_(torch.from_numpy(second).cuda())               # new content, same storage
    out.fill_(POISON_F32)
    graph.replay()
    assert torch.equal(out.cpu(), _want(vad, second, index, "f32"))
