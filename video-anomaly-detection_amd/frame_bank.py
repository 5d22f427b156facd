"""Frame bank: the decoded frames of a dataset, resized ONCE on the device and kept resident in HBM as uint8, and epochs of
clip / image batches gathered from them by one HIP launch per batch (csrc/frame_gather.hip).

This is the build's counterpart of the reference's dataset classes and their `DataLoader`: `IPADDataset` / `VideoDataset`
(utils/video_dataset.py:113-152, 240-329) decode, resize and normalise every frame `sequence_length / stride` times per
epoch on the host, then `default_collate` stacks the samples.  Here a frame is uploaded once, resized once by `FrameResizer`
(PIL-exact) straight into the bank, and a batch is `out[n] = normalise(bank[index[n]])`: overlapping sequences are index
entries, not copies.  At 256x256x3 a frame is 196 KB, so 100 k frames take 19.6 GB.

    bank = FrameBank(256)
    for frames, labels in videos:                       # uint8 [n, H, W, 3], CPU or GPU, any resolution per video
        bank.add_video(frames, frame_labels=labels)
    for epoch in range(epochs):
        loader = bank.loader(16, 4, batch_size=4, shuffle=True, generator=g)
        loss = trainer.train_epoch(loader)              # batches {'frames': fp32 [B,T,3,h,w], 'label', 'start_frame', 'video_id'}

The sequence index and the epoch order are host-side and need no GPU (`sequence_table`, `epoch_order`); the frames and the
gather are device-only: there is no CPU fallback.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hip
from .scoring import PIXEL_FORMATS, FrameResizer

UPLOAD_CHUNK_BYTES = 64 << 20           # CPU frames go to the device in chunks of about this size


# ------------------------------------------------------------------------------------------------ host-side plans
def sequence_table(lengths: Sequence[int], sequence_length: int, stride: int):
    """The sliding windows the reference's datasets build (utils/video_dataset.py:99-100, 114, 236-240, 257-264): per video,
    in order, `start in range(0, n - T + 1, stride)`; a video shorter than T contributes none.  Returns (video int64[N],
    start int64[N])."""
    t, s = int(sequence_length), int(stride)
    if t < 1:
        raise hip.VadError(f"sequence_length must be >= 1, got {sequence_length!r}")
    if s < 1:
        raise hip.VadError(f"stride must be >= 1, got {stride!r}")
    video, start = [], []
    for v, n in enumerate(lengths):
        if n < t:
            continue
        st = np.arange(0, n - t + 1, s, dtype=np.int64)
        start.append(st)
        video.append(np.full(len(st), v, np.int64))
    if not start:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(video), np.concatenate(start)


def epoch_order(n: int, shuffle: bool = False, generator=None, rank: int = 0, world: int = 1, seed: int = 0, epoch: int = 0) -> np.ndarray:
    """The sample order of one epoch on one rank, int64: `range(n)`; with `shuffle` and one rank what
    `RandomSampler(range(n), generator=generator)` yields (the sampler `DataLoader(shuffle=True, generator=generator)` builds);
    with `world > 1` the order, padding and split of `DistributedSampler(num_replicas=world, rank=rank, shuffle=shuffle,
    seed=seed)` after `set_epoch(epoch)` - every rank gets the same number of samples.  The samplers themselves are run, so
    the order is theirs by construction."""
    if world < 1 or not 0 <= rank < world:
        raise hip.VadError(f"rank must be in [0, world), got rank={rank!r} world={world!r}")
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=bool(shuffle), seed=int(seed))
        sampler.set_epoch(int(epoch))
        return np.array(list(sampler), np.int64)
    if shuffle and n > 0:
        from torch.utils.data import RandomSampler
        return np.array(list(RandomSampler(range(n), generator=generator)), np.int64)     # run to its end: it draws once more there
    return np.arange(n, dtype=np.int64)


def split_batches(order: np.ndarray, batch_size: int, drop_last: bool = False) -> List[np.ndarray]:
    """`BatchSampler(order, batch_size, drop_last)`: consecutive runs of `batch_size`, the short last one kept unless `drop_last`."""
    b = int(batch_size)
    if b < 1:
        raise hip.VadError(f"batch_size must be >= 1, got {batch_size!r}")
    out = [order[i:i + b] for i in range(0, len(order), b)]
    if drop_last and out and len(out[-1]) < b:
        out.pop()
    return out


class SequenceIndex:
    """What `FrameBank.sequences` returns: one row per sequence, in the reference's order.  `video` (index into the bank's videos),
    `start_frame`, `label` are int64 arrays, `first` the bank frame of the sequence's first frame, `video_id` a list, and
    `frame_labels` int64 [N, T] when every video of the bank has frame labels (None otherwise)."""

    def __init__(self, sequence_length, stride, video, start_frame, first, label, video_id, frame_labels):
        self.sequence_length, self.stride = sequence_length, stride
        self.video, self.start_frame, self.first, self.label = video, start_frame, first, label
        self.video_id, self.frame_labels = video_id, frame_labels

    def __len__(self) -> int:
        return len(self.start_frame)


def _as_u8_frames(frames_u8, pixel_format, channel_order, what):
    """Validate decoded frames `[n, H, W, 3]` (or the `pixel_format` layouts); returns (tensor, pixel-format key, bytes per pixel)."""
    if isinstance(frames_u8, np.ndarray):
        frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8))
    if not isinstance(frames_u8, torch.Tensor):
        raise hip.VadError(f"{what}: frames_u8 must be a torch tensor or a numpy array, got {type(frames_u8).__name__}")
    if pixel_format is not None and pixel_format not in PIXEL_FORMATS:
        raise hip.VadError(f"{what}: pixel_format must be one of {sorted(PIXEL_FORMATS)} or None, got {pixel_format!r}")
    if channel_order not in ("rgb", "bgr"):
        raise hip.VadError(f"{what}: channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    if pixel_format is not None and channel_order != "rgb":
        raise hip.VadError(f"{what}: give channel_order={channel_order!r} or pixel_format={pixel_format!r}, not both")
    key = pixel_format or channel_order
    _, bpp, layout = PIXEL_FORMATS[key]
    layout = layout.replace("...", "n")
    if frames_u8.dtype != torch.uint8:
        raise hip.VadError(f"{what}: frames_u8 must be uint8 {layout}, got dtype {frames_u8.dtype}")
    dims = 3 if bpp == 1 else 4
    if frames_u8.dim() != dims or (bpp != 1 and frames_u8.shape[-1] != bpp) or frames_u8.shape[1] < 1 or frames_u8.shape[2] < 1:
        raise hip.VadError(f"{what}: frames_u8 must be uint8 {layout}, got shape {tuple(frames_u8.shape)}")
    return frames_u8, key, bpp


class FrameBank:
    """uint8 frames `[F, h, w, 3]` (RGB, the model's resolution) resident on `device`, with the videos / images they belong to.

    `size`: int or (h, w).  `capacity_frames` pre-allocates; without it the bank grows by doubling, and a reallocation copies
    the frames it holds, so an earlier frame always reads the same.  Use one bank per thread / stream (it owns `FrameResizer`s)."""

    def __init__(self, size=256, device="cuda", capacity_frames: Optional[int] = None):
        if isinstance(size, (tuple, list)):
            if len(size) != 2:
                raise hip.VadError(f"FrameBank: size must be an int or (h, w), got {size!r}")
            self.h, self.w = int(size[0]), int(size[1])
        else:
            self.h = self.w = int(size)
        if self.h < 1 or self.w < 1:
            raise hip.VadError(f"FrameBank: size must be positive, got {size!r}")
        if capacity_frames is not None and int(capacity_frames) < 0:
            raise hip.VadError(f"FrameBank: capacity_frames must be >= 0, got {capacity_frames!r}")
        self.device = torch.device(device)
        self._capacity0 = int(capacity_frames or 0)
        self._bank: Optional[torch.Tensor] = None
        self.num_frames = 0
        self.videos: List[dict] = []          # {'first', 'n', 'video_id', 'label', 'frame_labels'}
        self.images: List[dict] = []          # {'frame', 'label', 'defect_type'}
        self._resizers = {}
        self._seq_cache = {}

    # ------------------------------------------------------------------------------------------------ storage
    @property
    def frames(self) -> torch.Tensor:
        """The frames held so far, uint8 `[F, h, w, 3]` (a view of the bank)."""
        if self._bank is None:
            return torch.empty(0, self.h, self.w, 3, dtype=torch.uint8, device=self.device)
        return self._bank[:self.num_frames]

    @property
    def capacity_frames(self) -> int:
        return 0 if self._bank is None else int(self._bank.shape[0])

    def _reserve(self, extra: int) -> None:
        need = self.num_frames + extra
        if self._bank is not None and need <= self._bank.shape[0]:
            return
        cap = max(need, 2 * self.capacity_frames, self._capacity0, 1)
        new = torch.empty(cap, self.h, self.w, 3, dtype=torch.uint8, device=self.device)
        if self.num_frames:
            new[:self.num_frames].copy_(self._bank[:self.num_frames])
        self._bank = new

    def _resizer(self, key: str) -> FrameResizer:
        if key not in self._resizers:
            self._resizers[key] = (FrameResizer((self.h, self.w), channel_order=key) if key in ("rgb", "bgr")
                                   else FrameResizer((self.h, self.w), pixel_format=key))
        return self._resizers[key]

    def _append(self, frames: torch.Tensor, key: str, bpp: int, what: str) -> int:
        """Resize (or copy) `frames` into the bank behind the frames it holds; returns the bank index of the first."""
        n, in_h, in_w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        first = self.num_frames
        if n == 0:
            return first
        self._reserve(n)
        same = key == "rgb" and (in_h, in_w) == (self.h, self.w)          # already the bank's layout: a copy
        if not same and self.device.type != "cuda":
            raise hip.VadError(f"{what}: frames_u8 {tuple(frames.shape)} need the device Resize to become {self.h}x{self.w} RGB, and this "
                               f"bank is on {self.device} (there is no CPU fallback)")
        on_host = not frames.is_cuda
        per = max(1, UPLOAD_CHUNK_BYTES // max(1, in_h * in_w * bpp)) if on_host else n
        for s in range(0, n, per):
            chunk = frames[s:s + per].contiguous()
            dst = self._bank[first + s:first + s + chunk.shape[0]]
            if on_host and self.device.type == "cuda":
                try:
                    chunk = chunk.pin_memory()
                except RuntimeError:                                       # no pinned memory to be had: a pageable copy
                    pass
                if same:
                    dst.copy_(chunk, non_blocking=True)
                    continue
                chunk = chunk.to(self.device, non_blocking=True)
            if same:
                dst.copy_(chunk)
            else:
                self._resizer(key)(chunk.to(self.device), out=dst)
        self.num_frames += n
        self._seq_cache.clear()
        return first

    # ------------------------------------------------------------------------------------------------ filling
    def add_video(self, frames_u8, video_id=None, label: int = 0, frame_labels=None, pixel_format: Optional[str] = None,
                  channel_order: str = "rgb") -> int:
        """Add the decoded frames of one video: uint8 `[n, H, W, 3]` in `channel_order`, or the `pixel_format` layouts of
        `FrameResizer` ("l": `[n, H, W]`, "rgba" / "bgra": `[n, H, W, 4]`), on the CPU or the GPU, at the video's own resolution.
        `label` is the video's label (`VideoDataset`: its folder); `frame_labels` (n values, 1 = anomalous) the per-frame labels
        of `IPADDataset`, from which a sequence's label then follows.  `video_id` defaults to the video's number.  Returns the
        video's index."""
        frames, key, bpp = _as_u8_frames(frames_u8, pixel_format, channel_order, "FrameBank.add_video")
        n = int(frames.shape[0])
        if frame_labels is not None:
            frame_labels = np.asarray(frame_labels).astype(np.int64).reshape(-1)
            if len(frame_labels) != n:
                raise hip.VadError(f"FrameBank.add_video: frame_labels must have one entry per frame ({n}), got {len(frame_labels)}")
        first = self._append(frames, key, bpp, "FrameBank.add_video")
        self.videos.append({"first": first, "n": n, "video_id": str(len(self.videos)) if video_id is None else video_id,
                            "label": int(label), "frame_labels": frame_labels})
        return len(self.videos) - 1

    def add_images(self, frames_u8, labels, defect_types=None, pixel_format: Optional[str] = None, channel_order: str = "rgb") -> int:
        """Add single images (the image model's samples, utils/dataset.py:136-160): uint8 `[n, H, W, 3]` (or a `pixel_format`
        layout) of one resolution, `labels` one int per image, `defect_types` one name per image ('good' / 'defect' by label when
        omitted).  Returns the index of the first image added."""
        frames, key, bpp = _as_u8_frames(frames_u8, pixel_format, channel_order, "FrameBank.add_images")
        n = int(frames.shape[0])
        labels = np.asarray(labels).astype(np.int64).reshape(-1)
        if len(labels) != n:
            raise hip.VadError(f"FrameBank.add_images: labels must have one entry per image ({n}), got {len(labels)}")
        if defect_types is None:
            defect_types = ["good" if l == 0 else "defect" for l in labels]
        if len(defect_types) != n:
            raise hip.VadError(f"FrameBank.add_images: defect_types must have one entry per image ({n}), got {len(defect_types)}")
        first = self._append(frames, key, bpp, "FrameBank.add_images")
        at = len(self.images)
        self.images.extend({"frame": first + i, "label": int(labels[i]), "defect_type": defect_types[i]} for i in range(n))
        return at

    # ------------------------------------------------------------------------------------------------ index
    def sequences(self, sequence_length: int, stride: int = 1) -> SequenceIndex:
        """The sequence list the reference's datasets build over the videos added so far (`sequence_table`).  A sequence of a
        video with `frame_labels` is anomalous when any of its frames is labelled 1 (utils/video_dataset.py:117-123); otherwise
        it takes the video's `label` (:240-247, 264-271)."""
        key = (int(sequence_length), int(stride))
        if key in self._seq_cache:
            return self._seq_cache[key]
        t = key[0]
        video, start = sequence_table([v["n"] for v in self.videos], *key)
        first = np.array([self.videos[v]["first"] for v in video], np.int64).reshape(-1) + start
        all_labelled = bool(self.videos) and all(v["frame_labels"] is not None for v in self.videos)
        label = np.zeros(len(start), np.int64)
        fl = np.zeros((len(start), t), np.int64) if all_labelled else None
        for i, (v, s) in enumerate(zip(video, start)):
            vid = self.videos[v]
            if vid["frame_labels"] is not None:
                window = vid["frame_labels"][s:s + t]
                label[i] = 1 if np.any(window == 1) else 0
                if fl is not None:
                    fl[i] = window
            else:
                label[i] = vid["label"]
        idx = SequenceIndex(t, key[1], video, start, first, label, [self.videos[v]["video_id"] for v in video], fl)
        self._seq_cache[key] = idx
        return idx

    # ------------------------------------------------------------------------------------------------ gather
    def gather(self, index_dev: torch.Tensor, dtype=torch.float32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ONE launch of `vad_gather_frames_u8` on the current stream: `index_dev` is an int64 device tensor `[n]` of bank frame
        numbers that the caller has validated (a view into a larger table is fine); returns fp32 `[n, 3, h, w]` normalised frames
        or uint8 `[n, h, w, 3]`.  No allocation when `out` is given, no host synchronisation: capturable in a graph."""
        if dtype not in (torch.float32, torch.uint8):
            raise hip.VadError(f"FrameBank: dtype must be torch.float32 or torch.uint8, got {dtype!r}")
        if self.device.type != "cuda" or self._bank is None:
            raise hip.VadError("FrameBank: batches are gathered on the device; this bank is " +
                               ("empty" if self.device.type == "cuda" else f"on {self.device} (there is no CPU fallback)"))
        if index_dev.dtype != torch.int64 or index_dev.dim() != 1 or index_dev.device != self._bank.device or not index_dev.is_contiguous():
            raise hip.VadError(f"FrameBank.gather: index_dev must be a contiguous int64 vector on {self._bank.device}")
        n = int(index_dev.shape[0])
        f32 = dtype == torch.float32
        shape = (n, 3, self.h, self.w) if f32 else (n, self.h, self.w, 3)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self._bank.device)
        elif tuple(out.shape) != shape or out.dtype != dtype or out.device != self._bank.device or not out.is_contiguous():
            raise hip.VadError(f"FrameBank.gather: out must be a contiguous {dtype} tensor {shape} on {self._bank.device}")
        if n == 0:
            return out
        with torch.cuda.device(self._bank.device):
            hip.check(hip.lib().vad_gather_frames_u8(self._bank.data_ptr(), self.num_frames, index_dev.data_ptr(), n, self.h, self.w,
                                                     hip.X_F32_NCHW if f32 else hip.X_U8_NHWC, out.data_ptr(), hip.current_stream()),
                      "vad_gather_frames_u8")
        hip.calls["gather_frames"] = hip.calls.get("gather_frames", 0) + 1
        return out

    def _frame_table(self, first: np.ndarray, t: int) -> np.ndarray:
        """Bank frame numbers `[len(first) * t]` of sequences starting at `first`, validated against the bank on the host."""
        table = (first[:, None] + np.arange(t, dtype=np.int64)[None, :]).reshape(-1)
        if len(table) and (table.min() < 0 or table.max() >= self.num_frames):
            raise hip.VadError(f"FrameBank: a frame index is outside the bank's {self.num_frames} frames")
        return table

    def _upload(self, table: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(table)).to(self.device)

    def _shape_clips(self, flat: torch.Tensor, b: int, t: int) -> torch.Tensor:
        return flat.view((b, t) + tuple(flat.shape[1:]))

    def batch(self, seq_ids, sequence_length: int, dtype=torch.float32, stride: int = 1) -> torch.Tensor:
        """The clips of sequences `seq_ids` (ids into `sequences(sequence_length, stride)`): fp32 `[B, T, 3, h, w]` normalised, or
        with `dtype=torch.uint8` the raw `[B, T, h, w, 3]` the scoring entry points ingest.  One gather launch; the index is
        built and validated on the host."""
        idx = self.sequences(sequence_length, stride)
        ids = np.asarray(seq_ids.cpu() if isinstance(seq_ids, torch.Tensor) else seq_ids)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise hip.VadError(f"FrameBank.batch: seq_ids must be a vector of integers, got {ids.dtype} {ids.shape}")
        ids = ids.astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= len(idx)):
            raise hip.VadError(f"FrameBank.batch: seq_ids must be in [0, {len(idx)}) for sequence_length={sequence_length} "
                               f"stride={stride}, got {int(ids.min())}..{int(ids.max())}")
        if dtype not in (torch.float32, torch.uint8):
            raise hip.VadError(f"FrameBank: dtype must be torch.float32 or torch.uint8, got {dtype!r}")
        table = self._frame_table(idx.first[ids], idx.sequence_length)
        if self.device.type != "cuda":
            raise hip.VadError(f"FrameBank.batch: batches are gathered on the device; this bank is on {self.device} (there is no CPU fallback)")
        return self._shape_clips(self.gather(self._upload(table), dtype), len(ids), idx.sequence_length)

    # ------------------------------------------------------------------------------------------------ loaders
    def loader(self, sequence_length: int, stride: int, batch_size: int, shuffle: bool = False, generator=None, drop_last: bool = False,
               dtype=torch.float32, rank: int = 0, world: int = 1, seed: int = 0, epoch: int = 0) -> "BankLoader":
        """A re-iterable over the clip batches of one rank, in place of `DataLoader(IPADDataset(...), batch_size, shuffle)`:
        dict batches {'frames' (device), 'label' int64 [B], 'start_frame' int64 [B], 'video_id' list, 'frame_labels' int64 [B, T]
        when every video has them} collated like `default_collate`.  Order: `epoch_order`."""
        return BankLoader(self, "clips", sequence_length, stride, batch_size, shuffle, generator, drop_last, dtype, rank, world, seed, epoch)

    def image_loader(self, batch_size: int, shuffle: bool = False, generator=None, drop_last: bool = False, dtype=torch.float32,
                     rank: int = 0, world: int = 1, seed: int = 0, epoch: int = 0) -> "BankLoader":
        """The same over the images: {'image' fp32 [B, 3, h, w] (uint8 [B, h, w, 3]), 'label' int64 [B], 'defect_type' list}."""
        return BankLoader(self, "images", 1, 1, batch_size, shuffle, generator, drop_last, dtype, rank, world, seed, epoch)


class BankLoader:
    """Iterating yields one epoch's batches of one rank.  The epoch's whole frame-index table is uploaded once; every batch is
    one gather launch reading its slice of that table.  `set_epoch` as on `DistributedSampler`; with `shuffle` and one rank
    every iteration draws a new permutation from `generator`, as a `DataLoader` does."""

    def __init__(self, bank: FrameBank, kind: str, sequence_length, stride, batch_size, shuffle, generator, drop_last, dtype, rank, world,
                 seed, epoch):
        if int(batch_size) < 1:
            raise hip.VadError(f"FrameBank.loader: batch_size must be >= 1, got {batch_size!r}")
        if int(stride) < 1:
            raise hip.VadError(f"FrameBank.loader: stride must be >= 1, got {stride!r}")
        if dtype not in (torch.float32, torch.uint8):
            raise hip.VadError(f"FrameBank.loader: dtype must be torch.float32 or torch.uint8, got {dtype!r}")
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise hip.VadError(f"FrameBank.loader: rank must be in [0, world), got rank={rank!r} world={world!r}")
        self.bank, self.kind, self.dtype = bank, kind, dtype
        self.sequence_length, self.stride, self.batch_size = int(sequence_length), int(stride), int(batch_size)
        self.shuffle, self.generator, self.drop_last = bool(shuffle), generator, bool(drop_last)
        self.rank, self.world, self.seed, self.epoch = int(rank), int(world), int(seed), int(epoch)
        if kind == "clips":
            bank.sequences(self.sequence_length, self.stride)              # argument errors surface here, not in the first epoch

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def num_samples(self) -> int:
        return len(self.bank.sequences(self.sequence_length, self.stride)) if self.kind == "clips" else len(self.bank.images)

    def __len__(self) -> int:
        n = self.num_samples()
        per_rank = -(-n // self.world) if self.world > 1 else n
        return per_rank // self.batch_size if self.drop_last else -(-per_rank // self.batch_size)

    def batch_ids(self) -> List[np.ndarray]:
        """The sample ids of every batch of this epoch on this rank (consumes `generator` like an iteration does)."""
        order = epoch_order(self.num_samples(), self.shuffle, self.generator, self.rank, self.world, self.seed, self.epoch)
        return split_batches(order, self.batch_size, self.drop_last)

    def __iter__(self):
        bank, t = self.bank, self.sequence_length
        batches = self.batch_ids()
        if not batches:
            return
        ids = np.concatenate(batches)
        if self.kind == "clips":
            idx = bank.sequences(t, self.stride)
            first = idx.first[ids]
        else:
            first = np.array([bank.images[i]["frame"] for i in ids], np.int64)
        table = bank._upload(bank._frame_table(first, t))                  # the epoch's whole index, uploaded once
        at = 0
        for b_ids in batches:
            b = len(b_ids)
            flat = bank.gather(table[at * t:(at + b) * t], self.dtype)
            at += b
            if self.kind == "clips":
                out = {"frames": bank._shape_clips(flat, b, t), "label": torch.from_numpy(idx.label[b_ids].copy()),
                       "start_frame": torch.from_numpy(idx.start_frame[b_ids].copy()), "video_id": [idx.video_id[i] for i in b_ids]}
                if idx.frame_labels is not None:
                    out["frame_labels"] = torch.from_numpy(idx.frame_labels[b_ids].copy())
            else:
                out = {"image": flat, "label": torch.tensor([bank.images[i]["label"] for i in b_ids], dtype=torch.int64),
                       "defect_type": [bank.images[i]["defect_type"] for i in b_ids]}
            yield out
