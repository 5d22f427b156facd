"""Oracle of the frame bank (FrameBank, vad_gather_frames_u8): a restatement of what the reference's datasets do, numpy only.
Shared by tests/test_frame_bank_plan.py (CPU) and tests/test_hip_frame_bank.py (GPU).  The reference's dataset module itself
cannot be imported by the tests (it needs torchvision and cv2), so its rules are restated here next to the lines they come from:

  sequences   utils/video_dataset.py:99-100   `if len(frame_files) < self.sequence_length: continue`
              utils/video_dataset.py:114      `for start_idx in range(0, len(frame_files) - self.sequence_length + 1, self.stride)`
              utils/video_dataset.py:118-123  `is_anomaly = 1 if np.any(seq_labels == 1) else 0` over `frame_labels[start:end]`,
                                              0 without labels; VideoDataset (:240-247, 264-271) takes the folder's label
              utils/video_dataset.py:125-131  each entry keeps `label`, `video_id`, `start_frame`, `frame_labels[start:end]`
  frames      utils/video_dataset.py:62-66    Resize((S, S)) -> ToTensor -> Normalize(0.5, 0.5), stacked to [T, C, H, W] (:144)
              Resize on a PIL image is `Image.resize(BILINEAR)`: tests/resize_ref.py, which tests/test_resize_plan.py pins to PIL;
              ToTensor + Normalize is `synth.u8_to_unit`, (u8/255 - 0.5)/0.5 step by step in fp32.
"""
from __future__ import annotations

import numpy as np

import resize_formats_ref as F
import resize_ref as R


def sequences_ref(videos, sequence_length: int, stride: int):
    """`videos`: list of dicts {'n', 'video_id', 'label', 'frame_labels' (array or None)} in insertion order.  Returns the
    reference's `self.sequences` as a list of dicts {'video', 'video_id', 'start_frame', 'label', 'frame_labels'}."""
    out = []
    for v, vid in enumerate(videos):
        if vid["n"] < sequence_length:
            continue
        for start_idx in range(0, vid["n"] - sequence_length + 1, stride):
            end_idx = start_idx + sequence_length
            fl = vid.get("frame_labels")
            if fl is not None:
                seq_labels = np.asarray(fl)[start_idx:end_idx]
                label = 1 if np.any(seq_labels == 1) else 0
            else:
                seq_labels = None
                label = vid["label"]
            out.append({"video": v, "video_id": vid["video_id"], "start_frame": start_idx, "label": label, "frame_labels": seq_labels})
    return out


def video_u8(seed: int, n: int, h: int, w: int, channels: int = 3) -> np.ndarray:
    """Decoded frames of one synthetic video: uint8 [n, h, w, 3] noise ([n, h, w] with channels == 1, a mode-L video)."""
    shape = (n, h, w) if channels == 1 else (n, h, w, channels)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def resized_ref(frames: np.ndarray, size: int) -> np.ndarray:
    """What the bank must hold for one video: uint8 [n, size, size, 3] RGB; `frames` [n, H, W, 3] RGB or [n, H, W] mode L
    (`convert('RGB')` replicates the plane)."""
    if frames.ndim == 3:
        return np.stack([F.l_ref(f, size, size, 3) for f in frames]) if len(frames) else np.zeros((0, size, size, 3), np.uint8)
    return np.stack([R.resize_ref(np.ascontiguousarray(f), size, size) for f in frames]) if len(frames) else np.zeros((0, size, size, 3), np.uint8)


def normalised_ref(u8_to_unit, frames_u8: np.ndarray) -> np.ndarray:
    """ToTensor + Normalize of uint8 [..., h, w, 3] -> float32 [..., 3, h, w]; `u8_to_unit` is `synth.u8_to_unit`."""
    return np.ascontiguousarray(np.moveaxis(u8_to_unit(frames_u8), -1, -3))


def clips_ref(u8_to_unit, videos_resized, seqs, ids, sequence_length: int):
    """The collated batch of sequences `ids`: (float32 [B, T, 3, h, w], uint8 [B, T, h, w, 3]); `videos_resized[v]` is
    `resized_ref` of video v, `seqs` is `sequences_ref`'s list."""
    u8 = np.stack([videos_resized[seqs[i]["video"]][seqs[i]["start_frame"]:seqs[i]["start_frame"] + sequence_length] for i in ids])
    return normalised_ref(u8_to_unit, u8), u8


def all_bytes_bank(frames: int, h: int, w: int, offset: int = 0, seed: int = 7) -> np.ndarray:
    """uint8 [frames, h, w, 3]: channel c of pixel k of the bank holds perm_c[(k + offset) % 256], a different permutation of
    0..255 per channel, so every byte value occurs in every channel once the bank has 256 pixels, and a kernel that mixed up
    channels, pixels or frames would show.  A smaller bank covers all values over `all_bytes_rounds` banks whose `offset`s
    are consecutive multiples of its pixel count."""
    rng = np.random.default_rng(seed)
    k = np.arange(frames * h * w) + offset
    return np.ascontiguousarray(np.stack([rng.permutation(256).astype(np.uint8)[(k + 37 * c) % 256] for c in range(3)], axis=-1)
                                .reshape(frames, h, w, 3))


def all_bytes_rounds(frames: int, h: int, w: int) -> int:
    return -(-256 // (frames * h * w))
