"""Scoring loops around the models: the build's counterpart of the reference's evaluate drivers.

* `compute_auroc` mirrors `evaluate.compute_auroc(model, test_loader, device)` (reference
  evaluate.py:46-91): same arguments, same 4-tuple result.
* `score_clips` mirrors the clip loop of `evaluate_video.evaluate` (reference evaluate_video.py:138-154).
* `sharded_scores` is new (the reference is single-process): contiguous block partition of the
  frame / clip stream over ranks, no data-path collective, ONE all_gather of the score vector
  (RCCL over xGMI when the backend is "nccl"; gloo in the CPU tests).
"""
from __future__ import annotations

from typing import Callable, Iterable, Optional, Tuple

import numpy as np
import torch

from . import hip
from . import metrics


def roc_auc(labels, scores) -> float:
    """Area under the ROC curve (Mann-Whitney U with average ranks for ties): the statistic
    sklearn.metrics.roc_auc_score returns for binary labels (reference evaluate.py:74)."""
    labels = np.asarray(labels).astype(bool)
    scores = np.asarray(scores, dtype=np.float64)
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc_auc needs both classes")
    order = np.argsort(scores, kind="mergesort")
    s = scores[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty_like(ranks)
    r[order] = ranks
    return float((r[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def compute_auroc(model, test_loader: Iterable[dict], device):
    """Same contract as the reference's evaluate.compute_auroc (evaluate.py:46-91): iterate batches
    {'image', 'label', 'defect_type'}, score with get_reconstruction_error(per_pixel=False), return
    (auroc, labels, scores, per-defect {count, mean_score, is_anomaly})."""
    all_labels, all_scores, all_types = [], [], []
    with torch.no_grad():
        for batch in test_loader:
            images = batch["image"].to(device)
            scores = model.get_reconstruction_error(images, per_pixel=False)
            all_scores.extend(scores.cpu().numpy())
            all_labels.extend(np.asarray(batch["label"]))
            all_types.extend(batch["defect_type"])
    labels = np.array(all_labels)
    scores = np.array(all_scores)
    auroc = roc_auc(labels, scores)
    per_defect = {}
    for name in set(all_types):
        m = np.array([d == name for d in all_types])
        per_defect[name] = {"count": int(m.sum()), "mean_score": scores[m].mean(),
                            "is_anomaly": labels[m][0] if m.any() else 0}
    return auroc, labels, scores, per_defect


def compute_auroc_smoothed(model, test_loader: Iterable[dict], device, sigma: float = 4.0, truncate: float = 4.0, map: str = "mse",
                           calibration=None, min_std: Optional[float] = None):
    """`compute_auroc` with the image score of the published MVTec evaluations: the maximum of the Gaussian-smoothed anomaly map
    (`metrics.smooth_maps(..., return_max="only")`) instead of the mean squared error - a small defect on a large frame barely
    moves the mean.  Same batches, same 4-tuple; `map` as in `pixel_auroc`.  The maps stay on the device: a batch's scores are read
    back once, as `compute_auroc` does.  `calibration`, `min_std` as in `pixel_auroc`: the score is the maximum of the z-score of the
    smoothed map (the smoothed map is normalised, its maximum taken by the same call)."""
    _check_map_name(map, "compute_auroc_smoothed")
    min_std = _check_calibration(calibration, "compute_auroc_smoothed", map, sigma, truncate, min_std)
    all_labels, all_scores, all_types = [], [], []
    with torch.no_grad():
        for batch in test_loader:
            images = batch["image"].to(device)
            values = _anomaly_maps(model, images, map, None, truncate)
            if calibration is None:
                scores = metrics.smooth_maps(values, sigma, truncate, return_max="only").reshape(images.shape[0])
            else:
                values = metrics.smooth_maps(values, sigma, truncate)
                scores = calibration.normalize(values, min_std, return_max="only").reshape(images.shape[0])
            all_scores.extend(scores.cpu().numpy())
            all_labels.extend(np.asarray(batch["label"]))
            all_types.extend(batch["defect_type"])
    labels = np.array(all_labels)
    scores = np.array(all_scores)
    auroc = roc_auc(labels, scores)
    per_defect = {}
    for name in set(all_types):
        m = np.array([d == name for d in all_types])
        per_defect[name] = {"count": int(m.sum()), "mean_score": scores[m].mean(),
                            "is_anomaly": labels[m][0] if m.any() else 0}
    return auroc, labels, scores, per_defect


def frame_scores(model, images, reduce, map: str = "mse", sigma=None, truncate: float = 4.0, calibration=None,
                 min_std: Optional[float] = None, morph=None, temporal=None, *, rank_filter=None):
    """Robust frame scores of one batch: the model's anomaly maps - the chain of `localize`: `map`, `sigma`,
    `truncate`, `calibration`, `min_std`, `morph` as there - reduced per frame by `metrics.reduce_maps(maps, reduce)`: `reduce` =
    "max", ("topk", fraction) - the mean of the top fraction of the pixels -, ("quantile", q) or ("rank", k).  `images`: `[B,C,H,W]`
    for the image model, `[B,T,C,H,W]` clips for the video model (map "mse" only).  Per batch ONE scoring call, the optional
    smoothing / calibration / morphology calls and ONE `metrics.map_topk` call; nothing is read by the host.  Returns (scores, maps):
    `[B]` / `[B,T]` float32 on the device, and the maps they were reduced from (`[B,1,H,W]` / `[B,T,1,H,W]`), so that a stream which
    also localises does not score twice.  `temporal` as in `pixel_auroc` (clips only; last in the chain, before the reduction);
    `rank_filter` as there (after the calibration, before `morph`)."""
    what = "frame_scores"
    _check_map_name(map, what)
    metrics.reduce_spec(reduce, what)
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal = metrics.temporal_steps(temporal)
    if images.dim() == 5 and map != "mse":
        _refuse_clips_on(map, what, "scored")
    min_std = _check_calibration(calibration, what, map, sigma, truncate, min_std)
    with torch.no_grad():
        maps = _anomaly_maps(model, images, map, sigma, truncate, calibration, min_std, morph, temporal, what, rank_filter=rank_filter)
        return metrics.reduce_maps(maps, reduce).reshape(maps.shape[:-3]), maps


def compute_auroc_maps(model, test_loader: Iterable[dict], device, reduce=("topk", 0.01), map: str = "mse", sigma=None,
                       truncate: float = 4.0, calibration=None, min_std: Optional[float] = None, morph=None, *, rank_filter=None):
    """`compute_auroc` with a robust image score: `frame_scores(model, images, reduce, ...)` - by default the mean of the top 1 % of
    the error map's pixels - instead of the mean squared error, which a small defect on a large frame barely moves, or the maximum
    (`compute_auroc_smoothed`), which is one pixel.  Same batches, same 4-tuple; the map arguments as in `pixel_auroc`.  The maps stay
    on the device: a batch's scores are read back once, as `compute_auroc` does."""
    what = "compute_auroc_maps"
    _check_map_name(map, what)
    metrics.reduce_spec(reduce, what)
    metrics.morph_steps(morph)
    metrics.rank_filter_steps(rank_filter)
    _check_calibration(calibration, what, map, sigma, truncate, min_std)
    all_labels, all_scores, all_types = [], [], []
    for batch in test_loader:
        scores, _ = frame_scores(model, batch["image"].to(device), reduce, map, sigma, truncate, calibration, min_std, morph,
                                 rank_filter=rank_filter)
        all_scores.extend(scores.cpu().numpy())
        all_labels.extend(np.asarray(batch["label"]))
        all_types.extend(batch["defect_type"])
    labels = np.array(all_labels)
    scores = np.array(all_scores)
    auroc = roc_auc(labels, scores)
    per_defect = {}
    for name in set(all_types):
        m = np.array([d == name for d in all_types])
        per_defect[name] = {"count": int(m.sum()), "mean_score": scores[m].mean(),
                            "is_anomaly": labels[m][0] if m.any() else 0}
    return auroc, labels, scores, per_defect


def score_clips(model, loader: Iterable[dict], device, per_frame: bool = False):
    """Clip loop of the reference's evaluate_video.evaluate (evaluate_video.py:137-154): returns
    (clip scores float32[N], labels) and, when per_frame, also float32[N,T] frame scores computed in
    the SAME pass (the reference runs a second forward, evaluate_video.py:147-149).  Only the two score
    vectors are produced: no reconstruction or error map is written."""
    seq, frm, labels = [], [], []
    with torch.no_grad():
        for batch in loader:
            frames = batch["frames"].to(device)
            if per_frame:
                out = model.score_seq_and_frames(frames)
                seq.extend(out["seq"].cpu().numpy())
                frm.extend(out["frame"].cpu().numpy())
            else:
                seq.extend(model.get_reconstruction_error(frames, per_frame=False).cpu().numpy())
            labels.extend(np.asarray(batch["label"]))
    if per_frame:
        return np.array(seq), np.array(labels), np.array(frm)
    return np.array(seq), np.array(labels)


def score_frames_stateful(model, frame_iter: Iterable, batch: int = 1, state=None, device=None, image_size=None,
                          channel_order: str = "rgb", pixel_format: Optional[str] = None):
    """Drive live streams through `VideoAutoencoder.score_stateful`: `frame_iter` yields the newest frames, one item per
    time step - `[B,C,H,W]` float (`[B,H,W,3]` uint8) for `batch` = B parallel streams, or `[B,T,...]` to hand over a few
    frames per stream at once.  Every frame goes through the encoder, ONE ConvLSTM step and the decoder once; the
    recurrent state is carried between calls (the reference's video-file mode re-scores a 16-frame window per new frame,
    evaluate_video.py:322-352).  Returns (float32[B, frames] scores, final VideoState); `state` continues earlier streams.
    With `image_size` (int or (h, w)) the items are decoded uint8 frames `[B,H,W,3]` / `[B,T,H,W,3]` at any one resolution, in
    `channel_order` "rgb" or "bgr": they are resized on the device (`FrameResizer`, PIL-exact) before they are scored.
    `pixel_format` names another layout of the items instead (`FrameResizer`: "l" = `[B,H,W]` / `[B,T,H,W]` grey frames, "rgba" /
    "bgra" = four bytes per pixel)."""
    scores = []
    resizer = FrameResizer(image_size, channel_order, pixel_format) if image_size is not None else None
    with torch.no_grad():
        for frames in frame_iter:
            frames = torch.as_tensor(frames)
            if device is not None:
                frames = frames.to(device)
            if resizer is not None:
                frames = resizer(frames)
            if frames.dim() == 4:
                frames = frames.unsqueeze(1)
            if frames.shape[0] != batch:
                raise hip.VadError(f"expected {batch} streams per step, got {tuple(frames.shape)}")
            out = model.score_stateful(frames, state)
            state = out["state"]
            scores.append(out["frame"])
    if not scores:
        return np.zeros((batch, 0), np.float32), state
    return torch.cat(scores, dim=1).cpu().numpy(), state


CRITERIA = ("mse", "ssim", "combined")     # train.py --loss


def validate(model, loader: Iterable[dict], device, criterion: str = "mse", ssim_weight: float = 0.5, window_size: int = 11):
    """The validation loop of the reference's train.py:54-91 / train_video.py:68-98 with ONE forward per batch (the reference
    runs `model(images)`, the criterion and `get_reconstruction_error`): batches {'image' | 'frames', 'label'}; `criterion` is
    train.py's --loss choice ('mse', 'ssim', 'combined' with `ssim_weight` = its alpha).  Returns (avg_loss, avg_normal,
    avg_anomaly): the batch losses averaged over batches, and the mean reconstruction error of the samples labelled 0 and of
    the others (0 when there are none).  A batch's loss is the mean of its samples' criterion (`score_criteria`); the samples
    of a batch are equally large, so that is the criterion of the batch (for clips: of its frames as one batch, the one way
    SSIMLoss takes them)."""
    if criterion not in CRITERIA:
        raise hip.VadError(f"validate: criterion must be one of {CRITERIA}, got {criterion!r}")
    model.eval()
    total, batches, normal, anomaly = 0.0, 0, [], []
    with torch.no_grad():
        for batch in loader:
            video = "frames" in batch
            x = batch["frames" if video else "image"].to(device)
            out = model.score_criteria(x, window_size=window_size, alpha=ssim_weight)
            errors = out["seq_mse" if video else "mse"]
            total += float(out[("seq_" if video else "") + criterion].mean())
            batches += 1
            for err, label in zip(errors.cpu().numpy(), np.asarray(batch["label"])):
                (normal if label == 0 else anomaly).append(err)
    if batches == 0:
        raise ValueError("validate needs at least one batch")
    return (total / batches, sum(normal) / len(normal) if normal else 0, sum(anomaly) / len(anomaly) if anomaly else 0)


# ------------------------------------------------------------------------------ Resize on the device
CHANNEL_ORDERS = {"rgb": 0, "bgr": 1}
# include/vad_hip.h VAD_PIX_*: name -> (code, bytes per pixel, the layout as the messages spell it)
PIXEL_FORMATS = {"rgb": (0, 3, "[..., H, W, 3]"), "bgr": (1, 3, "[..., H, W, 3]"), "l": (2, 1, "[..., H, W]"),
                 "rgba": (3, 4, "[..., H, W, 4]"), "bgra": (4, 4, "[..., H, W, 4]")}


class FrameResizer:
    """`transforms.Resize(size)` of the reference's input pipelines (utils/dataset.py:65-70, utils/video_dataset.py:62-66) for
    decoded uint8 frames that are already on the GPU: `resizer(frames)` takes uint8 `[..., H, W, 3]` (contiguous, any number of
    leading axes) and returns uint8 `[..., h, w, 3]` RGB, byte for byte what PIL's `Image.resize((w, h), BILINEAR)` gives - the
    form the models take as uint8 input.  `channel_order="bgr"` for frames as `cv2.VideoCapture` delivers them.

    `pixel_format` ("rgb" | "bgr" | "l" | "rgba" | "bgra"; None = the 3-byte layout in `channel_order`) takes the frames as the
    decoder left them, where the reference runs `Image.open(path).convert('RGB')` first: "l" is `[..., H, W]` with no channel
    axis (`np.asarray` of a mode-L image) and comes out as the resized plane in all three channels, or with `out_channels=1` as
    `[..., h, w, 1]` (the ground-truth masks: `resize_masks`); "rgba" / "bgra" are `[..., H, W, 4]` with the fourth byte ignored,
    "bgra" with B and R exchanged as "bgr" does.  Each is byte for byte `convert('RGB')` (`convert('L')`) followed by the resize.

    The object owns the device plan blob of every input geometry it has seen (computed once on the host, like packed weights)
    and the workspace of the horizontal pass; use one per thread / stream."""

    def __init__(self, size=256, channel_order: str = "rgb", pixel_format: Optional[str] = None, out_channels: int = 3):
        if isinstance(size, (tuple, list)):
            if len(size) != 2:
                raise hip.VadError(f"FrameResizer: size must be an int or (h, w), got {size!r}")
            self.out_h, self.out_w = int(size[0]), int(size[1])
        else:
            self.out_h = self.out_w = int(size)
        if channel_order not in CHANNEL_ORDERS:
            raise hip.VadError(f"FrameResizer: channel_order must be one of {sorted(CHANNEL_ORDERS)}, got {channel_order!r}")
        self.channel_order = channel_order
        if pixel_format is not None:
            if pixel_format not in PIXEL_FORMATS:
                raise hip.VadError(f"FrameResizer: pixel_format must be one of {sorted(PIXEL_FORMATS)} or None, got {pixel_format!r}")
            if channel_order != "rgb":
                raise hip.VadError(f"FrameResizer: give channel_order={channel_order!r} or pixel_format={pixel_format!r}, not both")
        if out_channels != 3 and not (out_channels == 1 and pixel_format == "l"):
            raise hip.VadError(f"FrameResizer: out_channels must be 3, or 1 with pixel_format='l', got {out_channels!r} "
                               f"with pixel_format={pixel_format!r}")
        self.pixel_format, self.out_channels = pixel_format, int(out_channels)
        self._plans = {}
        self._ws = None

    def _plan(self, in_h: int, in_w: int, device) -> torch.Tensor:
        key = (str(device), in_h, in_w)
        if key not in self._plans:
            l = hip.lib()
            nbytes = l.vad_resize_plan_bytes(in_h, in_w, self.out_h, self.out_w)
            blob = np.empty(max(nbytes // 4, 1), np.int32)
            hip.check(l.vad_resize_plan(in_h, in_w, self.out_h, self.out_w, blob.ctypes.data), "vad_resize_plan")
            self._plans[key] = torch.from_numpy(blob).to(device)
        return self._plans[key]

    def __call__(self, frames: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise hip.VadError("FrameResizer: frames must be a GPU tensor (the resize runs on the device; there is no CPU fallback)")
        code, bpp, layout = PIXEL_FORMATS[self.pixel_format or self.channel_order]
        if frames.dtype != torch.uint8:
            raise hip.VadError(f"FrameResizer: expected uint8 frames {layout}, got dtype {frames.dtype}")
        axes = 2 if bpp == 1 else 3                               # H, W and, unless a pixel is one byte, the channel axis
        if frames.dim() < axes or (bpp != 1 and frames.shape[-1] != bpp):
            raise hip.VadError(f"FrameResizer: expected uint8 frames {layout}, got {tuple(frames.shape)}")
        if not frames.is_contiguous():
            raise hip.VadError("FrameResizer: frames must be contiguous")
        lead, in_h, in_w = tuple(frames.shape[:-axes]), int(frames.shape[-axes]), int(frames.shape[1 - axes])
        n = int(np.prod(lead, dtype=np.int64)) if lead else 1
        shape = lead + (self.out_h, self.out_w, self.out_channels)
        with torch.cuda.device(frames.device):
            plan = self._plan(in_h, in_w, frames.device)
            if out is None:
                out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
            elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous():
                raise hip.VadError(f"FrameResizer: out must be a contiguous uint8 tensor {shape} on {frames.device}")
            if n == 0:
                return out
            l = hip.lib()
            if self.pixel_format is None:
                need = l.vad_resize_workspace_bytes(n, in_h, in_w, self.out_h, self.out_w)
            else:
                need = l.vad_resize_workspace_bytes_f(n, in_h, in_w, self.out_h, self.out_w, code, self.out_channels)
            if need and (self._ws is None or self._ws.numel() < need or self._ws.device != frames.device):
                self._ws = torch.empty(need, dtype=torch.uint8, device=frames.device)
            ws = self._ws.data_ptr() if need else None
            if self.pixel_format is None:
                hip.check(l.vad_resize_u8(frames.data_ptr(), n, in_h, in_w, CHANNEL_ORDERS[self.channel_order], plan.data_ptr(), out.data_ptr(),
                                          self.out_h, self.out_w, ws, need, hip.current_stream()), "vad_resize_u8")
            else:
                hip.check(l.vad_resize_u8_f(frames.data_ptr(), n, in_h, in_w, code, plan.data_ptr(), out.data_ptr(), self.out_h, self.out_w,
                                            self.out_channels, ws, need, hip.current_stream()), "vad_resize_u8_f")
        hip.calls["resize_u8"] = hip.calls.get("resize_u8", 0) + 1
        return out


def resize_frames(frames: torch.Tensor, size=256, channel_order: str = "rgb", pixel_format: Optional[str] = None,
                  out_channels: int = 3) -> torch.Tensor:
    """One-shot form of `FrameResizer` (plans the geometry on every call: keep a FrameResizer in a loop)."""
    return FrameResizer(size, channel_order, pixel_format, out_channels)(frames)


def resize_masks(masks_u8: torch.Tensor, size=256) -> torch.Tensor:
    """The reference's `mask_transform` (`Resize` + `ToTensor` on a `convert('L')` image, utils/dataset.py:74-77, 147-148) for
    uint8 masks `[..., H, W]` on the GPU: float32 `[..., 1, h, w]`, PIL's L resize divided by 255 - what `errmap` / `ssim_map` are
    compared with at the model's resolution.  The 256 quotients are computed once on the host, so they are ToTensor's floats."""
    small = FrameResizer(size, pixel_format="l", out_channels=1)(masks_u8)
    quotients = (torch.arange(256, dtype=torch.float32) / 255).to(small.device)
    return quotients[small.movedim(-1, -3).long()]


def score_raw_images(model, frames_u8: torch.Tensor, image_size=256, channel_order: str = "rgb", per_pixel: bool = False,
                     resizer: Optional[FrameResizer] = None, pixel_format: Optional[str] = None):
    """Decoded uint8 images `[B, H, W, 3]` at camera resolution -> Resize on the device -> `ConvAutoencoder.
    get_reconstruction_error(per_pixel=...)`: bit for bit the scores of the frames PIL resized.  Pass a `resizer` to reuse its
    plans and workspace across calls (its size, channel order and pixel format then apply).  `pixel_format`: `FrameResizer`'s
    ("l": `[B, H, W]` grey images, "rgba" / "bgra": `[B, H, W, 4]`) - the scores of `convert('RGB')` + Resize."""
    resizer = resizer or FrameResizer(image_size, channel_order, pixel_format)
    with torch.no_grad():
        return model.get_reconstruction_error(resizer(frames_u8), per_pixel=per_pixel)


def score_raw_clips(model, clips_u8: torch.Tensor, image_size=256, channel_order: str = "rgb", per_frame: bool = False,
                    resizer: Optional[FrameResizer] = None, pixel_format: Optional[str] = None):
    """Decoded uint8 clips `[B, T, H, W, 3]` (`pixel_format` "l": `[B, T, H, W]`, "rgba" / "bgra": `[B, T, H, W, 4]`) -> Resize on
    the device -> `VideoAutoencoder.get_reconstruction_error(per_frame=...)`."""
    resizer = resizer or FrameResizer(image_size, channel_order, pixel_format)
    with torch.no_grad():
        return model.get_reconstruction_error(resizer(clips_u8), per_frame=per_frame)


# ------------------------------------------------------------------------------ device synth
def synth_frames_device(seed: int, first_frame: int, n: int, h: int = 256, w: int = 256, c: int = 3,
                        device="cuda", anomalies: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NCHW fp32 frames generated on the GPU, bit-identical to `synth.frames` (numpy)."""
    if out is None:
        out = torch.empty(n, c, h, w, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        hip.check(hip.lib().vad_synth_frames(out.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, first_frame, n, c, h, w,
                                             int(anomalies), hip.current_stream()), "vad_synth_frames")
    return out


# ------------------------------------------------------------------------------ multi-GPU
def block_partition(n_items: int, world: int, rank: int) -> Tuple[int, int, int]:
    """Contiguous block partition: rank r owns [r*per, min((r+1)*per, n)); returns (start, count, per).
    Clips are items, so a clip is never split across ranks (the ConvLSTM recurrence is sequential in t)."""
    per = -(-n_items // world)
    start = min(rank * per, n_items)
    return start, max(0, min(per, n_items - start)), per


def sharded_scores(score_block: Callable[[int, int], torch.Tensor], n_items: int, width: int = 1,
                   rank: int = 0, world: int = 1, device="cpu", group=None, force_collective: bool = False) -> torch.Tensor:
    """Score items [0, n_items) across `world` ranks and return float32[n_items, width] (squeezed to
    [n_items] when width == 1) in the original order on EVERY rank.

    `score_block(first, count)` returns this rank's scores for items [first, first+count) as a float32
    tensor [count] or [count, width] on `device`.  The only communication is one all_gather of
    `per * width` floats per rank; the tail of the last block is zero padding that is cut off after the
    gather, so rank-major order == original order.  `force_collective` runs the all_gather for world == 1 too (a
    one-rank process group: how the RCCL branch is exercised on a one-GPU box).
    """
    start, count, per = block_partition(n_items, world, rank)
    local = torch.zeros(per, width, dtype=torch.float32, device=device)
    if count:
        local[:count] = score_block(start, count).reshape(count, width).to(torch.float32)
    if world > 1 or force_collective:
        import torch.distributed as dist
        gathered = torch.empty(world * per, width, dtype=torch.float32, device=device)
        dist.all_gather_into_tensor(gathered, local, group=group)
    else:
        gathered = local
    out = gathered[:n_items]
    return out[:, 0] if width == 1 else out


def score_stream(model, seed: int, n_frames: int, chunk: int = 512, h: int = 256, w: int = 256, rank: int = 0,
                 world: int = 1, device="cuda", anomalies: bool = False, group=None, force_collective: bool = False) -> torch.Tensor:
    """BASELINE configs[3]: score a long synthetic frame stream without ever materialising it.  The stream is
    block-partitioned over ranks; each rank regenerates its frames on the device `chunk` at a time (the counter-based
    generator makes any sub-range reproducible, on any rank and on the CPU), scores them with
    `model.get_reconstruction_error`, and ONE all_gather returns float32[n_frames] in stream order on every rank."""
    dev = torch.device(device)
    buf = torch.empty(min(chunk, max(n_frames, 1)), 3, h, w, dtype=torch.float32, device=dev)

    def score_block(first: int, count: int) -> torch.Tensor:
        out = torch.empty(count, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for s in range(0, count, buf.shape[0]):
                k = min(buf.shape[0], count - s)
                synth_frames_device(seed, first + s, k, h, w, 3, dev, anomalies, out=buf[:k])
                out[s:s + k] = model.get_reconstruction_error(buf[:k])
        return out

    return sharded_scores(score_block, n_frames, 1, rank, world, dev, group, force_collective)


# ------------------------------------------------------------------------------ ranking metrics on the device
def _anomaly_maps(model, images, map: str, sigma, truncate, calibration=None, min_std=None, morph=(), temporal=(), what: str = "scoring",
                  *, rank_filter=None):
    """The batch's anomaly map [B,1,H,W] of the pixel metrics: the error map or the SSIM map, through `metrics.smooth_maps` when a
    sigma is given, then - with a `calibration` - turned into its z-score in place (the map is this call's own), then through the
    steps of `rank_filter` (`metrics.rank_filter_steps`) and of `morph` (`metrics.morph_steps`), in z-score units when calibrated,
    then - clips [B,T,C,H,W] only, every clip a fresh stream - through the steps of `temporal` (`metrics.temporal_steps`): the order
    is sigma, calibration, rank filter, morph, temporal."""
    if temporal and images.dim() != 5:
        raise hip.VadError(f"{what}: temporal= filters the consecutive frames of clips [B,T,C,H,W]; the frames of an image batch "
                           f"{tuple(images.shape)} are not consecutive (a live camera: localize_stream(temporal_filter=))")
    if map == "mse":
        values = model.score_all(images)["errmap"]
    else:
        values = model.score_criteria(images, ssim_map=True)["ssim_map"]
    if sigma is not None:
        values = metrics.smooth_maps(values, sigma, truncate)
    if calibration is not None:
        values = calibration.normalize(values, min_std, out=values)
    if rank_filter:
        values = metrics.apply_rank_filter(values, rank_filter)
    if morph:
        values = metrics.apply_morph(values, morph)
    if temporal:
        values = metrics.apply_temporal(values, temporal)
    return values


def _check_map_name(map, what: str) -> None:
    if map not in ("mse", "ssim"):
        raise hip.VadError(f"{what}: map must be 'mse' or 'ssim', got {map!r}")


def _refuse_clips_on(map, what: str, verb: str) -> None:
    """The video model has an error map only; `verb`: what `what` does with clips."""
    raise hip.VadError(f"{what}: clips [B,T,C,H,W] are {verb} on the error map only (map='mse'), got {map!r}")


def _masked_maps(model, batch: dict, device, map: str, sigma, truncate, calibration, min_std, morph, key: str = "image", temporal=(),
                 what: str = "scoring", rank_filter=()):
    """One batch of the mask metrics: (`_anomaly_maps` of batch[key], batch['mask']), both on the device."""
    images = batch[key].to(device)
    masks = torch.as_tensor(batch["mask"]).to(device)
    return _anomaly_maps(model, images, map, sigma, truncate, calibration, min_std, morph, temporal, what, rank_filter=rank_filter), masks


def _clip_key(batch: dict, temporal, map, what: str) -> str:
    """The key of a mask metric's frames: 'image', or - with `temporal=` - the 'frames' [B,T,C,H,W] of a video batch (map "mse")."""
    if temporal and "frames" in batch and "image" not in batch:
        if map != "mse":
            _refuse_clips_on(map, what, "filtered")
        return "frames"
    return "image"


def _map_meta(map: str, sigma, truncate) -> dict:
    """What kind of map a calibration holds the statistics of: `MapStatistics.meta`."""
    return {"map": map, "sigma": None if sigma is None else float(sigma), "truncate": float(truncate)}


def _check_calibration(calibration, what: str, map: str, sigma, truncate, min_std) -> float:
    """A calibration applies to the maps it was gathered on: `ValueError` for another map, sigma or truncate - thresholds on such
    z-scores would be meaningless.  -> the min_std to use (without a calibration: as given, it is not used)."""
    if calibration is None:
        return min_std
    if not isinstance(calibration, metrics.MapStatistics):
        raise hip.VadError(f"{what}: calibration must be a metrics.MapStatistics, got {type(calibration).__name__}")
    want = _map_meta(map, sigma, truncate)
    if calibration.meta != want:
        raise ValueError(f"{what}: the calibration was gathered on {calibration.meta}, this call makes {want}")
    return metrics.DEFAULT_MIN_STD if min_std is None else min_std


def calibrate(model, loader: Iterable[dict], device, map: str = "mse", sigma=None, truncate: float = 4.0, stats=None):
    """Per-pixel statistics of a model's anomaly map over NORMAL data - the train split; the reference trains on normal frames only
    (utils/dataset.py, utils/video_dataset.py) -: the loop of `pixel_auroc` without masks.  Batches {'image' [B,C,H,W]} for the image
    model, {'frames' [B,T,C,H,W]} for the video model (map "mse" only), where every frame of every clip goes into the same per-pixel
    statistics.  `map`, `sigma`, `truncate` as in `pixel_auroc`.  Each batch is ONE scoring call, an optional smoothing call and ONE
    `MapStatistics.update`; no map is copied to the host.  Returns the `metrics.MapStatistics` with `meta` = {map, sigma, truncate};
    pass `stats` to continue one (its meta must be that of this call).  Hand the result to `pixel_auroc` / `pixel_aupro` /
    `compute_auroc_smoothed` / `localize` as `calibration=`."""
    _check_map_name(map, "calibrate")
    meta = _map_meta(map, sigma, truncate)
    if stats is not None:
        if not isinstance(stats, metrics.MapStatistics):
            raise hip.VadError(f"calibrate: stats must be a metrics.MapStatistics, got {type(stats).__name__}")
        if stats.meta and stats.meta != meta:
            raise ValueError(f"calibrate: stats was gathered on {stats.meta}, this call makes {meta}")
    with torch.no_grad():
        for batch in loader:
            video = "frames" in batch
            if video and map != "mse":
                _refuse_clips_on(map, "calibrate", "calibrated")
            values = _anomaly_maps(model, batch["frames" if video else "image"].to(device), map, sigma, truncate)
            if stats is None:
                stats = metrics.MapStatistics(tuple(int(v) for v in values.shape[-2:]), values.device)
            stats.update(values)
    if stats is None:
        raise ValueError("calibrate needs at least one batch")
    stats.meta = meta
    return stats


def pixel_auroc(model, loader: Iterable[dict], device, map: str = "mse", mantissa_bits: int = 11, hist=None, sigma=None,
                truncate: float = 4.0, calibration=None, min_std: Optional[float] = None, morph=None, temporal=None, *, rank_filter=None):
    """Pixel-level AUROC of an image model's anomaly map against the ground-truth masks - the localisation metric of MVTec-style
    datasets; the reference loads `sample['mask']` and only plots it beside the map (evaluate.py:142-171).  Batches are
    {'image', 'mask', ...} as `MVTecDataset` yields them (utils/dataset.py:150-156): mask float `[B,1,H,W]` (ToTensor: a pixel is
    anomalous iff > 0.5; `resize_masks` makes these on the device) or uint8 (iff >= 128 - the same pixels).
    `map`: "mse" = the channel-mean squared error map of `score_all`; "ssim" = `score_criteria(ssim_map=True)['ssim_map']`, which
    already holds 1 - SSIM per pixel (channel mean, `losses.ssim_per_frame`), so it is scored as it stands: higher = more
    anomalous, like the error map.  It can be slightly negative where SSIM exceeds 1 by rounding; such pixels are counted in
    `hist.rejected()`, not binned.
    `sigma` (None = the raw map, as before): smooth every map with `metrics.smooth_maps(sigma, truncate)` first - scipy's
    `gaussian_filter`, sigma = 4 in the published MVTec evaluations - still on the device.
    Each batch is ONE scoring call and ONE `accumulate`; no map is copied to the host - the only host read is the counters, once,
    at the end.  Returns (auroc, tie_bound, hist) (`metrics.auroc_from_counts`); pass `hist` to continue an earlier evaluation or
    to all-reduce before reading (`hist.all_reduce()`), in which case its own mantissa_bits applies.
    `calibration` (None = the map as it stands, as before): a `metrics.MapStatistics` from `calibrate` with the same `map`, `sigma`
    and `truncate` (`ValueError` otherwise, or for another frame shape) - the map is turned into its per-pixel z-score
    (`MapStatistics.normalize`, floor `min_std`, default `metrics.DEFAULT_MIN_STD`) after the smoothing and before the histogram, in
    place, still on the device.  The histogram bins values >= 0: z-scores below 0 - pixels less anomalous than on the normal frames'
    average - are counted in `hist.rejected()`, so the curve and its thresholds are those of the z-scores above 0.
    `morph` (None = no morphology, as before): a `metrics.morph_steps` spec - one step `("open", 3)` / `("close", (3, 5))` or a list of
    at most four, e.g. `[("open", 2), ("close", 5)]` - applied with `metrics.morph_maps` after the smoothing and the calibration (in
    z-score units when calibrated) and before the histogram.  `calibrate` takes none: statistics are those of the un-morphed map.
    Grey morphology commutes with a threshold, so a threshold read from this histogram is the one `localize(morph=...)` takes.
    `temporal` (None = no temporal filter, as before): a `metrics.temporal_steps` spec - one step `("min", k)` / `("max", k)` /
    `("mean", k)` / `("ema", alpha)` or a list of at most four - for batches of CLIPS: {'frames' [B,T,C,H,W], 'mask' [B,T,1,H,W]} of the
    video model (map "mse"; or 'image' holding such clips).  Every clip is a fresh stream; every pixel is filtered over the last k
    frames of its clip with `metrics.temporal_maps`, LAST in the chain - sigma, calibration, morph, temporal - and before the
    histogram.  An image batch [B,C,H,W] with it is refused with `VadError`: its frames are not consecutive.  `calibrate` takes
    none: a calibration is gathered on unfiltered maps.
    `rank_filter` (None = no rank filter, as before; keyword only): a `metrics.rank_filter_steps` spec - one step `("median", 3)` /
    `("percentile", (3, 5), 90)` / `("rank", 3, 2)` or a list of at most four - applied with `metrics.rank_filter_maps` after the
    calibration (in z-score units when calibrated) and immediately before `morph`: the chain is sigma, calibration, rank filter,
    morph, temporal.  A median removes isolated hot pixels before anything ranks, thresholds or labels them, keeps step edges where
    they are and leaves flat areas at their level.  Like the morphology it only selects values, so it commutes with a threshold.
    `calibrate` takes none."""
    _check_map_name(map, "pixel_auroc")
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal = metrics.temporal_steps(temporal)
    min_std = _check_calibration(calibration, "pixel_auroc", map, sigma, truncate, min_std)
    if hist is None:
        hist = metrics.ScoreHistogram(mantissa_bits, device)
    with torch.no_grad():
        for batch in loader:
            key = _clip_key(batch, temporal, map, "pixel_auroc")
            hist.accumulate(*_masked_maps(model, batch, device, map, sigma, truncate, calibration, min_std, morph, key, temporal, "pixel_auroc",
                                          rank_filter))
    auroc, tie_bound = hist.auroc()
    return auroc, tie_bound, hist


def pixel_aupro(model, loader: Iterable[dict], device, map: str = "mse", fpr_limit: float = 0.3, mantissa_bits: int = 11, hist=None,
                connectivity: int = 8, sigma=None, truncate: float = 4.0, calibration=None, min_std: Optional[float] = None, morph=None,
                temporal=None, *, rank_filter=None):
    """Per-region overlap (AUPRO) of an image model's anomaly map against the ground-truth masks: every connected anomalous region
    of the masks weighs the same, and the curve is integrated up to a false-positive rate of `fpr_limit` - the localisation metric
    of the MVTec evaluation, where pixel AUROC is dominated by the large defects.  The loop of `pixel_auroc` (same batches, same
    `map`, same `sigma` / `truncate` - AUPRO is the metric speckle hurts most, its curve ends at FPR 0.3): each batch is ONE scoring
    call and ONE `ProHistogram.accumulate`, which labels the masks' regions and adds the counters
    on the device; the only host read is the counters, once, at the end.  Returns (aupro, quant_bound, weight_bound, hist)
    (`metrics.aupro_from_counts`); pass `hist` to continue an earlier evaluation or to all-reduce before reading, in which case
    its own mantissa_bits and connectivity apply.  `hist.auroc()` is the pixel AUROC of the same evaluation.  `calibration`,
    `min_std`, `morph`, `temporal`, `rank_filter` as in `pixel_auroc`."""
    _check_map_name(map, "pixel_aupro")
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal = metrics.temporal_steps(temporal)
    min_std = _check_calibration(calibration, "pixel_aupro", map, sigma, truncate, min_std)
    if hist is None:
        hist = metrics.ProHistogram(mantissa_bits, device, connectivity)
    with torch.no_grad():
        for batch in loader:
            key = _clip_key(batch, temporal, map, "pixel_aupro")
            maps, masks = _masked_maps(model, batch, device, map, sigma, truncate, calibration, min_std, morph, key, temporal, "pixel_aupro",
                                       rank_filter)
            if temporal:                                                      # clips: every frame's regions on their own, [B*T,1,H,W]
                maps, masks = maps.flatten(0, 1), masks.reshape(maps.shape[0] * maps.shape[1], *masks.shape[-3:])
            hist.accumulate(maps, masks)
    aupro, quant_bound, weight_bound = hist.aupro(fpr_limit)
    return aupro, quant_bound, weight_bound, hist


def detection_report(model, loader: Iterable[dict], device, threshold: float, map: str = "mse", sigma=None, truncate: float = 4.0,
                     calibration=None, min_std: Optional[float] = None, morph=(), connectivity: int = 8, min_area: int = 1,
                     gt_fraction: float = 0.0, pred_fraction: float = 0.0, counts=None, temporal=None, *, rank_filter=None):
    """What an operating point does against the ground-truth masks: how many of the labelled defects it finds, how many false
    alarms per frame it raises, which pixel IoU it reaches - the questions AUROC and AUPRO, which rank pixels over all thresholds and
    know nothing of `min_area` or of regions as units, do not answer.  The loop of `pixel_aupro`, over the same batches: {'image'
    [B,C,H,W], 'mask' [B,1,H,W]} for the image model, {'frames' [B,T,C,H,W], 'mask' [B,T,1,H,W]} for the video model (map "mse" only;
    every frame is matched on its own; `event_report` matches the events of a clip).  The maps come from the chain `localize` thresholds (`map`, `sigma`, `truncate`,
    `calibration`, `min_std`, `morph` as there), so the report is of exactly the detections `localize(threshold, connectivity,
    min_area)` returns.  Each batch is ONE scoring call, the optional smoothing / calibration / morphology calls and ONE
    `metrics.match_regions`, whose 16 counters per frame are summed on the device; no map or mask is copied to the host.
    `gt_fraction`, `pred_fraction` as in `metrics.match_regions`.  Returns (report dict of `metrics.report_from_counts`, the
    `metrics.DetectionCounts`); pass `counts` to continue an earlier evaluation or to all-reduce before reading
    (`counts.all_reduce()`, then `counts.report()`) - counters gathered at another operating point are refused with `ValueError`.
    `temporal` as in `pixel_auroc`: video batches only, every clip a fresh stream, after `morph` and before the threshold; it is part
    of the operating point the counters are gathered at.  `rank_filter` as in `pixel_auroc` (after the calibration, before `morph`),
    and part of the operating point likewise."""
    what = "detection_report"
    _check_map_name(map, what)
    morph = metrics.morph_steps(None if morph == () else morph)          # () = no morphology, like None elsewhere
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal = metrics.temporal_steps(temporal)
    min_std = _check_calibration(calibration, what, map, sigma, truncate, min_std)
    params = metrics._match_params(what, threshold, connectivity, min_area, gt_fraction, pred_fraction)
    meta = dict(_map_meta(map, sigma, truncate), morph=tuple(morph), calibrated=calibration is not None,
                min_std=None if calibration is None else float(min_std))
    if temporal:
        meta["temporal"] = tuple(temporal)
    if rank_filter:
        meta["rank_filter"] = tuple(rank_filter)
    if counts is None:
        counts = metrics.DetectionCounts(device)
    elif not isinstance(counts, metrics.DetectionCounts):
        raise hip.VadError(f"{what}: counts must be a metrics.DetectionCounts, got {type(counts).__name__}")
    counts._adopt({**params, **meta}, what)
    with torch.no_grad():
        for batch in loader:
            video = "frames" in batch
            if video and map != "mse":
                _refuse_clips_on(map, what, "reported")
            maps, masks = _masked_maps(model, batch, device, map, sigma, truncate, calibration, min_std, morph, "frames" if video else "image",
                                       temporal, what, rank_filter)
            counts.update(metrics.match_regions(maps, masks, threshold, connectivity, min_area, gt_fraction, pred_fraction, max_regions=1), meta)
    return counts.report(), counts


def frame_auroc(model, loader: Iterable[dict], device, hist=None, mantissa_bits: int = 11, reduce=None, sigma=None, truncate: float = 4.0,
                calibration=None, min_std: Optional[float] = None, morph=None, temporal=None, *, rank_filter=None):
    """Frame-level AUROC of a video model (evaluate_video.py:171-176) without gathering the scores: the clip loop of
    `score_clips(per_frame=True)` - batches {'frames' [B,T,C,H,W], 'frame_labels' [B,T], ...} -, each batch's frame scores and
    labels going into a histogram on the device.  Returns (auroc, tie_bound, hist); ranks of a sharded evaluation call
    `hist.all_reduce()` on a histogram they pass in instead of gathering score vectors.
    `reduce` (None = the mean squared error per frame of `score_seq_and_frames`, as before; the other arguments are then not used):
    a `frame_scores` spec - "max", ("topk", fraction), ("quantile", q), ("rank", k) -; the frame scores are then those of
    `frame_scores(model, frames, reduce, "mse", sigma, truncate, calibration, min_std, morph)`, reduced from the error maps on the
    device, and go into the same histogram (which bins scores >= 0: a calibrated score below 0 is counted in `hist.rejected()`).
    `temporal` and `rank_filter` as in `frame_scores` (they filter maps, so they need a `reduce`: `VadError` without one)."""
    if metrics.temporal_steps(temporal) and reduce is None:
        raise hip.VadError("frame_auroc: temporal= filters the error maps before they are reduced; pass a reduce (\"max\", (\"topk\", f), ...)")
    if metrics.rank_filter_steps(rank_filter) and reduce is None:
        raise hip.VadError("frame_auroc: rank_filter= filters the error maps before they are reduced; pass a reduce (\"max\", (\"topk\", f), ...)")
    if reduce is not None:
        metrics.reduce_spec(reduce, "frame_auroc")
        metrics.morph_steps(morph)
        _check_calibration(calibration, "frame_auroc", "mse", sigma, truncate, min_std)
    if hist is None:
        hist = metrics.ScoreHistogram(mantissa_bits, device)
    with torch.no_grad():
        for batch in loader:
            frames = batch["frames"].to(device)
            labels = torch.as_tensor(np.asarray(batch["frame_labels"])).to(device)
            if reduce is None:
                scores = model.score_seq_and_frames(frames)["frame"]
            else:
                scores, _ = frame_scores(model, frames, reduce, "mse", sigma, truncate, calibration, min_std, morph, temporal,
                                         rank_filter=rank_filter)
            hist.accumulate(scores, labels)
    auroc, tie_bound = hist.auroc()
    return auroc, tie_bound, hist


def localize(model, images, threshold: float, map: str = "mse", sigma=None, truncate: float = 4.0, connectivity: int = 8,
             min_area: int = 1, max_regions: int = 64, calibration=None, min_std: Optional[float] = None, morph=None, *, rank_filter=None):
    """Detections of one batch: the model's anomaly maps and the connected regions of `map >= threshold` in them - where the
    reference paints the map (evaluate.py:142-171, main.py:231-250) and compares one scalar with a constant (main.py:282-283).
    `images`: `[B,C,H,W]` frames for the image model, `[B,T,C,H,W]` clips for the video model (map "mse" only; every frame of a
    clip is labelled on its own).  `map`, `sigma`, `truncate` as in `pixel_auroc`, so a threshold taken from its histogram
    (`metrics.threshold_at_fpr`, `best_f1_threshold`) applies as it stands.  Per batch ONE scoring call, an optional smoothing call
    and ONE `metrics.detect_regions` call; nothing but the flag word is read by the host.  Returns (`metrics.Regions`, maps): the
    table with the leading shape `[B]` / `[B,T]`, and the maps it was made from, `[B,1,H,W]` / `[B,T,1,H,W]`, still on the device.
    `calibration`, `min_std` as in `pixel_auroc`: `threshold` is then a z-score (3.0 = three standard deviations of that pixel over
    the normal frames), the regions are those of `z >= threshold`, and the maps returned are the z-score maps.
    `morph` as in `pixel_auroc` (one `metrics.morph_maps` launch per step, last in the chain): the regions are those of the morphed
    maps - `("open", 2)` drops single-pixel speckle before it is labelled, where `min_area` drops it after and cannot cut a
    one-pixel bridge between two defects - and the maps returned are the morphed maps.
    `rank_filter` as in `pixel_auroc` (one `metrics.rank_filter_maps` launch per step, after the calibration and immediately before
    `morph`): `("median", 3)` removes isolated hot pixels like an opening, but leaves the corners and thin parts of a real defect and
    the level of flat areas alone; the maps returned are the filtered maps."""
    _check_map_name(map, "localize")
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    if images.dim() == 5 and map != "mse":
        _refuse_clips_on(map, "localize", "localised")
    min_std = _check_calibration(calibration, "localize", map, sigma, truncate, min_std)
    with torch.no_grad():
        maps = _anomaly_maps(model, images, map, sigma, truncate, calibration, min_std, morph, rank_filter=rank_filter)
        return metrics.detect_regions(maps, threshold, connectivity, min_area, max_regions), maps


def localize_events(model, images, threshold: float, map: str = "mse", sigma=None, truncate: float = 4.0, calibration=None,
                    min_std: Optional[float] = None, connectivity: int = 8, temporal: int = 9, min_duration: int = 1, min_volume: int = 1,
                    max_events: int = 64, morph=None, temporal_filter=None, tracks: bool = False, *, rank_filter=None):
    """`localize` with the event table: the model's anomaly maps and the events of `map >= threshold` in them - regions linked
    across consecutive frames (`metrics.detect_events`), so that a line alarms on what persists (`min_duration`) and not on one
    noisy map.  `images`: `[B,T,C,H,W]` clips for the video model (map "mse" only), every clip its own volume; `[N,C,H,W]` frames
    for the image model, the batch in order being N consecutive frames of one camera: one volume.  `map`, `sigma`, `truncate`,
    `calibration`, `min_std`, `morph` as in `localize`.  Per batch ONE scoring call, the optional smoothing and calibration calls and ONE
    `detect_events` call; nothing but the flag word is read by the host.  Returns (`metrics.Events`, maps): the table with the
    leading shape `[B]` (video) or `()` (image), and the maps it was made from, `[B,T,1,H,W]` / `[N,1,H,W]`, still on the device.
    `temporal_filter`: the `temporal=` spec of `pixel_auroc` under another name - `temporal` is this entry point's link structure -:
    clips only (an image batch is refused, although this entry point reads it as one volume: use `localize_stream(temporal_filter=)`
    for a camera), every clip a fresh stream, after `morph` and before the threshold; the maps returned are the filtered maps.
    `("min", 2)` in front of the labeller removes what differs from frame to frame.
    `tracks=True`: the labels are requested from `detect_events` and ONE `metrics.event_tracks` call follows; `events.tracks` is then
    a `metrics.EventTracks` - a box, a peak and a centroid per kept event and frame - and `events.labels` the label volume.  The
    default leaves launches and outputs as they are (`events.tracks` is None).
    `rank_filter` as in `localize`: every frame filtered on its own, after the calibration and immediately before `morph`."""
    _check_map_name(map, "localize_events")
    if not isinstance(tracks, bool):
        raise hip.VadError(f"localize_events: tracks must be a bool, got {tracks!r}")
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal_filter = metrics.temporal_steps(temporal_filter)
    if images.dim() == 5 and map != "mse":
        _refuse_clips_on(map, "localize_events", "localised")
    min_std = _check_calibration(calibration, "localize_events", map, sigma, truncate, min_std)
    with torch.no_grad():
        maps = _anomaly_maps(model, images, map, sigma, truncate, calibration, min_std, morph, temporal_filter, "localize_events",
                             rank_filter=rank_filter)
        volumes = maps if maps.dim() == 5 else maps[:, 0]                 # [B,T,1,H,W], or the image batch as one clip [N,H,W]
        events = metrics.detect_events(volumes, threshold, connectivity, temporal, min_duration, min_volume, max_events, return_labels=tracks)
        if tracks:
            events.tracks = metrics.event_tracks(volumes, events)
        return events, maps


def event_report(model, loader: Iterable[dict], device, threshold: float, map: str = "mse", sigma=None, truncate: float = 4.0,
                 calibration=None, min_std: Optional[float] = None, morph=(), connectivity: int = 8, temporal: int = 9, min_duration: int = 1,
                 min_volume: int = 1, gt_fraction: float = 0.0, pred_fraction: float = 0.0, counts=None, temporal_filter=None, *,
                 rank_filter=None):
    """What a debounced alarm does against the ground-truth masks: how many of the labelled anomalies the kept events still find,
    how many false-alarm events they raise, how many frames after a defect appears the alarm fires, and the frame-level precision and
    recall of `events.alarms()` - what `detection_report`, which matches every frame on its own, cannot see of `min_duration`,
    `min_volume` and the links in time.  The chain and the conventions of `localize_events` (`map`, `sigma`, `truncate`,
    `calibration`, `min_std`, `morph`, `rank_filter`, `temporal_filter`, `connectivity`, `temporal`, `min_duration`, `min_volume` as
    there), so the report is of exactly the events `localize_events` returns.  Video batches are {'frames' [B,T,C,H,W], 'mask'
    [B,T,1,H,W]} for the video model (map "mse" only), every clip its own volume; image batches {'image' [N,C,H,W], 'mask'
    [N,1,H,W]} are read as one volume of N consecutive frames (no `temporal_filter`, as in `localize_events`).  Each batch is ONE
    scoring call, the optional filter calls and ONE `metrics.match_events`, whose 22 counters per clip are summed on the device; no
    map or mask is copied to the host.  `gt_fraction`, `pred_fraction` as in `metrics.match_events`.  Returns (report dict of
    `metrics.event_report_from_counts`, the `metrics.EventCounts`); pass `counts` to continue an earlier evaluation or to all-reduce
    before reading (`counts.all_reduce()`, then `counts.report()`) - counters gathered at another operating point are refused with
    `ValueError`."""
    what = "event_report"
    _check_map_name(map, what)
    morph = metrics.morph_steps(None if morph == () else morph)          # () = no morphology, like None elsewhere
    rank_filter = metrics.rank_filter_steps(rank_filter)
    temporal_filter = metrics.temporal_steps(temporal_filter)
    min_std = _check_calibration(calibration, what, map, sigma, truncate, min_std)
    params = metrics._event_match_params(what, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction)
    meta = dict(_map_meta(map, sigma, truncate), morph=tuple(morph), calibrated=calibration is not None,
                min_std=None if calibration is None else float(min_std))
    if temporal_filter:
        meta["temporal_filter"] = tuple(temporal_filter)
    if rank_filter:
        meta["rank_filter"] = tuple(rank_filter)
    if counts is None:
        counts = metrics.EventCounts(device)
    elif not isinstance(counts, metrics.EventCounts):
        raise hip.VadError(f"{what}: counts must be a metrics.EventCounts, got {type(counts).__name__}")
    counts._adopt({**params, **meta}, what)
    with torch.no_grad():
        for batch in loader:
            video = "frames" in batch
            if video and map != "mse":
                _refuse_clips_on(map, what, "reported")
            maps, masks = _masked_maps(model, batch, device, map, sigma, truncate, calibration, min_std, morph, "frames" if video else "image",
                                       temporal_filter, what, rank_filter)
            if not video:                                                 # the image batch as one clip [N,H,W]
                maps, masks = maps[:, 0], masks.reshape(maps.shape[0], *maps.shape[-2:])
            counts.update(metrics.match_events(maps, masks, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction,
                                               pred_fraction, max_events=1), meta)
    return counts.report(), counts


def localize_stream(model, frames, tracker, state=None, sigma=None, truncate: float = 4.0, calibration=None, min_std: Optional[float] = None,
                    morph=None, temporal_filter=None, boxes: bool = False, *, rank_filter=None):
    """One step of a live stream with events carried between calls (`metrics.EventTracker`): the newest
    frames are scored, their error maps smoothed and calibrated as in `localize_events`, and handed to `tracker.update`.
    Video model: `frames` `[B,T,C,H,W]` (or the uint8 layouts `score_stateful` takes) are the next T frames of B streams; ONE
    `score_stateful(errmap=True)` call continues the ConvLSTM `state` (None = fresh streams).  Image model: `frames` `[B,C,H,W]`
    is the newest frame of B cameras; ONE `score_all`; `state` must be None and None is returned.  The error map only ("mse").
    Returns (`metrics.TrackUpdate`, maps, state): the events that closed in this step and the causal alarms of its frames, the maps
    they were made from (`[B,T,1,H,W]` / `[B,1,H,W]`, on the device), and the scoring state for the next call.  The tracker's
    threshold applies to the maps as made here: with a `calibration` it is a z-score.  `morph` as in `localize`: every frame is
    morphed on its own, so the result does not depend on how the frames are split over calls.
    `temporal_filter` (None = none, as before): a `metrics.TemporalFilter` for B streams of these maps, which carries the last frames
    between calls - the maps go through `temporal_filter.update` after the morphology and before the tracker, so tracker and filter
    see what `localize_events(temporal=)` sees on the whole stream, however its frames are split over calls.  Both models: the image
    model's `[B,1,H,W]` is one new frame of B cameras.  The maps returned are the filtered maps.  Reset it with the tracker.
    `boxes` is handed to `tracker.update`: with True, `update.boxes` holds the cross-section of every open event in the newest frame
    (`metrics.TrackBoxes`), and `update.boxes_alarming()` which of them alarm now.
    `rank_filter` as in `localize` (after the calibration, immediately before `morph`): every frame is filtered on its own, so the
    result does not depend on how the frames are split over calls."""
    morph = metrics.morph_steps(morph)
    rank_filter = metrics.rank_filter_steps(rank_filter)
    if temporal_filter is not None and not isinstance(temporal_filter, metrics.TemporalFilter):
        raise hip.VadError(f"localize_stream: temporal_filter must be a metrics.TemporalFilter, got {type(temporal_filter).__name__}")
    if not isinstance(tracker, metrics.EventTracker):
        raise hip.VadError(f"localize_stream: tracker must be a metrics.EventTracker, got {type(tracker).__name__}")
    min_std = _check_calibration(calibration, "localize_stream", "mse", sigma, truncate, min_std)
    video = hasattr(model, "score_stateful")
    if not video and state is not None:
        raise hip.VadError("localize_stream: the image model carries no state between calls; pass state=None")
    with torch.no_grad():
        if video:
            out = model.score_stateful(frames, state, errmap=True)
            maps, state = out["errmap"], out["state"]
        else:
            maps = model.score_all(frames)["errmap"]
        if sigma is not None:
            maps = metrics.smooth_maps(maps, sigma, truncate)
        if calibration is not None:
            maps = calibration.normalize(maps, min_std, out=maps)
        if rank_filter:
            maps = metrics.apply_rank_filter(maps, rank_filter)
        if morph:
            maps = metrics.apply_morph(maps, morph)
        if temporal_filter is not None:                                   # [B,T,1,H,W] as it stands; [B,1,H,W] = B streams x 1 frame
            maps = temporal_filter.update(maps.contiguous())
        update = tracker.update(maps if video else maps[:, 0], boxes=boxes)
    return update, maps, state
