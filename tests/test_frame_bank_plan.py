"""Host side of the frame bank (FrameBank: sequence index, labels, epoch order, argument checks): no GPU needed.  The bank here
lives on the CPU and takes frames that are already at its size (a copy); resizing and gathering are device-only and are
tested in tests/test_hip_frame_bank.py.  The oracle is tests/frame_bank_ref.py, the restated rules of the reference's datasets."""
import numpy as np
import pytest
import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
from torch.utils.data.distributed import DistributedSampler

import frame_bank_ref as B

T = 5
LENGTHS = (0, T - 1, T, T + 1, 3 * T + 2)
STRIDES = (1, 4, T, T + 3)
S = 4                                                     # bank resolution: frames of 4 x 4 need no resize


def _videos(with_labels: str):
    """`with_labels`: 'none', 'all' or 'some' of the videos carry frame labels.  The longest video's only anomalous frame is
    frame T - 1: the LAST frame of the window starting at 0 (and inside no window starting after it at strides >= T)."""
    vids = []
    for v, n in enumerate(LENGTHS):
        fl = None
        if with_labels == "all" or (with_labels == "some" and v % 2 == 0):
            fl = np.zeros(n, np.int64)
            if n == 3 * T + 2:
                fl[T - 1] = 1
            elif n == T + 1:
                fl[0] = 1                                  # in the window at 0, not in the one at 1
        vids.append({"n": n, "video_id": f"{v + 1:02d}", "label": v % 2, "frame_labels": fl})
    return vids


def _bank(vad, vids):
    bank = vad.FrameBank(S, device="cpu")
    rng = np.random.default_rng(3)
    for vid in vids:
        frames = rng.integers(0, 256, (vid["n"], S, S, 3), dtype=np.uint8)
        bank.add_video(frames, video_id=vid["video_id"], label=vid["label"], frame_labels=vid["frame_labels"])
    return bank


@pytest.mark.parametrize("with_labels", ["none", "all", "some"])
@pytest.mark.parametrize("stride", STRIDES)
def test_sequences_equal_the_restated_rules(vad, with_labels, stride):
    vids = _videos(with_labels)
    bank = _bank(vad, vids)
    want = B.sequences_ref(vids, T, stride)
    got = bank.sequences(T, stride)
    assert len(got) == len(want) and len(want) > 0
    assert got.video.tolist() == [s["video"] for s in want]
    assert got.start_frame.tolist() == [s["start_frame"] for s in want]
    assert got.label.tolist() == [s["label"] for s in want]
    assert got.video_id == [s["video_id"] for s in want]
    firsts = np.cumsum([0] + [v["n"] for v in vids])
    assert got.first.tolist() == [int(firsts[s["video"]]) + s["start_frame"] for s in want]
    if with_labels == "all":
        assert got.frame_labels.tolist() == [s["frame_labels"].tolist() for s in want]
        long = [s for s in want if vids[s["video"]]["n"] == 3 * T + 2]
        assert long[0]["label"] == 1 and long[0]["frame_labels"][-1] == 1          # anomalous through its last frame only
        assert [s["label"] for s in long if s["start_frame"] >= T] == [0] * sum(s["start_frame"] >= T for s in long)
    else:
        assert got.frame_labels is None
    # the videos shorter than T contribute nothing, the one of exactly T frames one sequence
    assert set(got.video.tolist()) == {2, 3, 4} and got.video.tolist().count(2) == 1


def test_frames_at_the_bank_size_are_copied_and_growth_keeps_them(vad):
    bank = vad.FrameBank(S, device="cpu", capacity_frames=2)
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 256, (3, S, S, 3), dtype=np.uint8), rng.integers(0, 256, (40, S, S, 3), dtype=np.uint8)
    bank.add_video(a)
    bank.add_video(torch.from_numpy(b))
    assert bank.num_frames == 43 and bank.capacity_frames >= 43
    assert torch.equal(bank.frames, torch.from_numpy(np.concatenate([a, b])))
    assert [v["video_id"] for v in bank.videos] == ["0", "1"]


def _reference_batches(n, batch_size, shuffle, drop_last, gen_seed, rank, world, seed, epoch):
    if world > 1:
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
        sampler.set_epoch(epoch)
    elif shuffle:
        sampler = RandomSampler(range(n), generator=torch.Generator().manual_seed(gen_seed))
    else:
        sampler = SequentialSampler(range(n))
    return [list(b) for b in BatchSampler(sampler, batch_size, drop_last)]


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_loader_order_is_the_samplers(vad, world, shuffle, drop_last):
    bank = vad.FrameBank(S, device="cpu")
    bank.add_video(np.zeros((23 + 2, S, S, 3), np.uint8))
    n, bs = 23, 4                                              # 23 sequences of 3 frames: not a multiple of 4, 8 or 12
    assert len(bank.sequences(3, 1)) == n
    counts = []
    for rank in range(world):
        for epoch in (0, 3):
            ld = bank.loader(3, 1, bs, shuffle=shuffle, generator=torch.Generator().manual_seed(11), drop_last=drop_last,
                             rank=rank, world=world, seed=5, epoch=epoch)
            got = [b.tolist() for b in ld.batch_ids()]
            assert got == _reference_batches(n, bs, shuffle, drop_last, 11, rank, world, 5, epoch), (rank, epoch)
            assert len(ld) == len(got)
            counts.append(len(got))
    assert len(set(counts)) == 1                               # every rank takes the same number of steps
    if world == 1 and shuffle:                                 # a second iteration draws the generator's next permutation
        g = torch.Generator().manual_seed(11)
        ld = bank.loader(3, 1, bs, shuffle=True, generator=g)
        first, second = ld.batch_ids(), ld.batch_ids()
        g2 = torch.Generator().manual_seed(11)
        rs = RandomSampler(range(n), generator=g2)
        assert np.concatenate(first).tolist() == list(rs) and np.concatenate(second).tolist() == list(rs)


def test_image_loader_order(vad):
    bank = vad.FrameBank(S, device="cpu")
    bank.add_images(np.zeros((7, S, S, 3), np.uint8), labels=[0, 1, 0, 0, 1, 1, 0], defect_types=list("abcdefg"))
    ld = bank.image_loader(3, shuffle=True, generator=torch.Generator().manual_seed(2))
    want = _reference_batches(7, 3, True, False, 2, 0, 1, 0, 0)
    assert [b.tolist() for b in ld.batch_ids()] == want and len(ld) == 3
    assert [im["defect_type"] for im in bank.images] == list("abcdefg") and [im["frame"] for im in bank.images] == list(range(7))


def test_argument_errors_name_the_argument(vad):
    E = vad.hip.VadError
    bank = vad.FrameBank(S, device="cpu")
    bank.add_video(np.zeros((6, S, S, 3), np.uint8))
    with pytest.raises(E, match="frames_u8.*uint8"):
        bank.add_video(np.zeros((2, S, S, 3), np.float32))                       # wrong dtype
    with pytest.raises(E, match="frames_u8.*shape"):
        bank.add_video(np.zeros((2, S, S), np.uint8))                            # wrong layout: no channel axis without pixel_format="l"
    with pytest.raises(E, match="frames_u8.*shape"):
        bank.add_video(np.zeros((2, S, S, 4), np.uint8))                         # four bytes per pixel need pixel_format="rgba"
    with pytest.raises(E, match="frames_u8.*shape"):
        bank.add_images(np.zeros((S, S, 3), np.uint8), labels=[0])               # no leading axis
    with pytest.raises(E, match="pixel_format"):
        bank.add_video(np.zeros((2, S, S, 3), np.uint8), pixel_format="yuv")
    with pytest.raises(E, match="frame_labels"):
        bank.add_video(np.zeros((2, S, S, 3), np.uint8), frame_labels=[0, 1, 0])
    with pytest.raises(E, match="labels"):
        bank.add_images(np.zeros((2, S, S, 3), np.uint8), labels=[0])
    assert bank.num_frames == 6 and len(bank.videos) == 1                        # nothing was added by a refused call
    with pytest.raises(E, match="stride"):
        bank.sequences(3, 0)
    with pytest.raises(E, match="stride"):
        bank.loader(3, 0, 2)
    with pytest.raises(E, match="batch_size"):
        bank.loader(3, 1, 0)
    with pytest.raises(E, match="batch_size"):
        bank.image_loader(-1)
    with pytest.raises(E, match="dtype"):
        bank.loader(3, 1, 2, dtype=torch.float16)
    with pytest.raises(E, match="rank"):
        bank.loader(3, 1, 2, rank=2, world=2)
    n = len(bank.sequences(3, 1))
    for bad in ([n], [-1], [0, n + 5]):
        with pytest.raises(E, match="seq_ids"):
            bank.batch(bad, 3)
    with pytest.raises(E, match="seq_ids"):
        bank.batch([0.5], 3)
    with pytest.raises(E, match="no CPU fallback"):                             # valid ids: the gather itself is device-only
        bank.batch([0], 3)
    with pytest.raises(E, match="no CPU fallback"):                             # so is the resize
        bank.add_video(np.zeros((2, S + 1, S, 3), np.uint8))
    with pytest.raises(E, match="size"):
        vad.FrameBank((4, 4, 4))


def test_train_epoch_is_part_of_both_trainers(vad):
    assert callable(vad.VideoTrainer.train_epoch) and vad.VideoTrainer.train_epoch is vad.ImageTrainer.train_epoch
