"""Ranking metrics from a score histogram: pixel-level and frame-level AUROC without the scores ever leaving the device.

A ranking metric needs only the joint distribution of (score, label).  `ScoreHistogram` is the device half: integer counters over
the scores' float bit patterns, one row per class, accumulated batch by batch by `vad_hist_accumulate` (csrc/score_hist.hip) from
error maps / SSIM maps and their ground-truth masks, or from frame scores and frame labels.  The counters are integers, so the
result does not depend on batching, launch order or sharding, and ranks combine with ONE all-reduce of the counters.

The `*_from_counts` functions are the host half: pure numpy on an int64 `[2, nbins]` array (row 0 = normal, row 1 = anomalous),
usable on a machine without a GPU.  The reference computes these with `sklearn.metrics.roc_auc_score` on host vectors
(evaluate.py:74, evaluate_video.py:171-176) and only plots the masks (evaluate.py:142-171).

Quantiser: `mantissa_bits` = m in 4..15.  A finite v >= 0 falls into bin `float_bits(v) >> (23 - m)` (sign-less exponent and the
top m mantissa bits; -0.0 counts as 0), of `255 << m` bins; the bin's lower edge is the score with the low mantissa bits cleared.
The map is monotone, so quantising can only create ties, never swap a pair: `auroc_from_counts` returns the AUROC of the quantised
scores together with a rigorous bound on its distance from the AUROC of the unquantised ones.  Negative values, NaNs and
infinities are not binned; they are counted per class in `rejected`.

The second half of the file is the per-region overlap (AUPRO): `label_regions`, `ProHistogram` (csrc/region_overlap.hip) and
`aupro_from_counts` / `pro_curve_from_counts`, built on the same quantiser.

The third part is what goes in front of both: `gaussian_taps` / `smooth_maps` (csrc/map_smooth.hip) smooth the anomaly maps with
scipy's Gaussian on the device and give the per-frame maximum of the smoothed map, the image score of the MVTec evaluation.

The last part is what comes behind them on a deployed line: `detect_regions` (csrc/map_regions.hip) turns a map and an operating
threshold into a table of connected regions per frame - box, area, peak, centroid sums - without a map leaving the device; `detect_events` (csrc/map_events.hip) links those regions across the frames of a
clip into events - first and last frame, union box, peak, volume - and counts per frame the pixels of the events that persist.
`match_regions` (csrc/map_match.hip) joins the detections of `detect_regions` with the masks' regions of `label_regions` - which
labelled defects an operating point finds, which detections are false alarms, the pixel classes - and `DetectionCounts` sums its
sixteen counters per frame into the report a line is accepted on.

Across all of them sits the calibration: `MapStatistics` (csrc/map_stats.hip) holds the per-pixel mean and standard deviation of the
map over normal frames and turns a map into its z-score, which is then smoothed-and-ranked, thresholded and labelled like a raw map.

Between the frames of a clip or a live stream sit `temporal_maps` / `TemporalFilter` (csrc/map_temporal.hip): every pixel filtered
over the last k frames - causal minimum, maximum, mean, exponential average - before the threshold.

Between the calibration and the morphology sit `rank_filter_maps` / `apply_rank_filter` (csrc/map_rankfilt.hip): the sliding-window
median, percentile or rank of every map - the denoiser of single hot pixels that keeps edges and flat levels where they are.

At the end of the chain, where a map becomes ONE number per frame, sit `map_topk` and `reduce_maps` (csrc/map_topk.hip): the k-th
largest pixel and the mean of the k largest, the robust frame scores between the mean of the map and its maximum.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import hip

MIN_MANTISSA_BITS, MAX_MANTISSA_BITS = hip.HIST_MIN_M, hip.HIST_MAX_M
_HIST_MAGIC = 0x48444156      # "VADH", csrc/score_hist.hip
_HEADER_BYTES = 16


# ---------------------------------------------------------------------- argument checks, each written once
# Every entry point below refuses a bad argument with `VadError` before it launches anything, and says which argument of which
# call it was (`what`).  The wording is part of the interface (tests/test_metrics_messages_plan.py holds every message in full).
def _is_int(v) -> bool:
    """A plain integer: True and False are no sizes, counts or choices."""
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_int(v, name: str, what: str, lo: int, hi: int) -> int:
    if not _is_int(v) or not lo <= int(v) <= hi:
        raise hip.VadError(f"{what}: {name} must be an int in {lo}..{hi}, got {v!r}")
    return int(v)


def _check_choice(v, name: str, what: str, a: int, b: int) -> int:
    if not _is_int(v) or int(v) not in (a, b):
        raise hip.VadError(f"{what}: {name} must be {a} or {b}, got {v!r}")
    return int(v)


def _check_number(v, name: str, what: str, ok, rule: str, error=hip.VadError) -> float:
    """A real number - no bool, no string - that `ok` accepts; `rule` is what the message says it must be."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not ok(v):
        raise error(f"{what}: {name} must be {rule}, got {v!r}")
    return float(v)


def _check_m(m, what: str) -> int:
    return _check_int(m, "mantissa_bits", what, MIN_MANTISSA_BITS, MAX_MANTISSA_BITS)


def _check_connectivity(c, what: str) -> int:
    return _check_choice(c, "connectivity", what, 4, 8)


def _check_structure(connectivity, temporal, what: str) -> Tuple[int, int]:
    """(connectivity, temporal) of the event volumes: (4, 1), (8, 1) or (8, 9)."""
    connectivity = _check_connectivity(connectivity, what)
    temporal = _check_choice(temporal, "temporal", what, 1, 9)
    if temporal == 9 and connectivity != 8:
        raise hip.VadError(f"{what}: temporal=9 (the 3 x 3 of the frame before) needs connectivity=8, got connectivity={connectivity}")
    return connectivity, temporal


def _check_threshold(threshold, what: str) -> float:
    """-> the threshold as the float32 value the kernels compare with."""
    _check_number(threshold, "threshold", what, lambda v: not np.isnan(v), "a number that is not NaN")
    return float(np.float32(threshold))


def _check_fraction(v, name: str, what: str) -> float:
    return _check_number(v, name, what, lambda v: 0.0 <= float(v) <= 1.0, "a number in [0, 1]")   # false for NaN


# The check of a map batch that `detect_regions`, `detect_events`, `EventTracker.update` and `MapStatistics` share, in the order they
# keep; each goes on with a layout step of its own.  `smooth_maps` and `morph_maps` spell their checks out, and `gaussian_taps` its
# two: on a small frame they are calls of 13 us that the host paces, and the helpers' own calls showed in them, beyond what a second
# copy of the parent shows against the parent (profiles/metrics_args_ab.json); `MapStatistics.normalize` is written like them.
def _check_maps(maps, what: str, where: str, device=None) -> None:
    """A map batch is a tensor, on the GPU (`where`: what the message says runs there; "" = nothing) - on `device`, for the
    statistics, which have one -, and float32."""
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    if not maps.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the GPU ({where}{'; ' if where else ''}there is no CPU fallback)")
    if device is not None and maps.device != device:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the statistics' device {device}")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")


# ---------------------------------------------------------------------- the launch epilogue
def _count(name: str) -> None:
    """One more call of a native entry point: `hip.calls` is how tests see that the device path really ran."""
    hip.calls[name] = hip.calls.get(name, 0) + 1


def _workspace(nbytes: int, device, what: str, out_of_range: str) -> torch.Tensor:
    """A workspace of the size the library asked for; a size of 0 is its answer to shapes it does not take."""
    if nbytes == 0:
        raise hip.VadError(f"{what}: {out_of_range}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _flag_word(ws: torch.Tensor) -> int:
    """The labelling kernels' flag word, the first four bytes of their workspace: one 4-byte copy, which waits for the call."""
    return int(ws[:4].view(torch.int32).item())


def _raise_on_flags(flags: int, what: str) -> None:
    if flags:
        raise hip.VadError(f"{what}: flags {flags:#x} are set - a walk of the labelling kernels ran out of its step bound (bit 0) or a "
                           "region has no size (bit 1); the labels and counters of this evaluation are not to be trusted")


def _launched(ws: torch.Tensor, what: str) -> None:
    """After a labelling launch of the entry point `what`: count it, read its flag word, raise if a bit is set."""
    _count(what)
    _raise_on_flags(_flag_word(ws), what)


def num_bins(mantissa_bits: int) -> int:
    return 255 << _check_m(mantissa_bits, "num_bins")


def state_bytes(mantissa_bits: int) -> int:
    """Size of the device blob: 16-byte header, uint64 counts[2][nbins], uint64 rejected[2] (vad_hist_state_bytes)."""
    return _HEADER_BYTES + 8 * (2 * num_bins(mantissa_bits) + 2)


def allreduce_counters_(counters: torch.Tensor, group=None, force_collective: bool = False) -> int:
    """Sum an int64 counter tensor over the ranks of `group`, in place: ONE all_reduce(SUM), as `training.allreduce_sum_` does for
    the flat gradient buffer.  Returns the world size (1 when no process group is initialised).  With gloo a GPU tensor goes
    through a host copy; with "nccl" (RCCL) the collective runs on the device."""
    import torch.distributed as dist
    if counters.dtype != torch.int64:
        raise hip.VadError(f"allreduce_counters_: counters must be int64, got {counters.dtype}")
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    world = dist.get_world_size(group)
    if world == 1 and not force_collective:
        return 1
    if counters.is_cuda and dist.get_backend(group) == "gloo":
        host = counters.detach().cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        counters.copy_(host)
    else:
        dist.all_reduce(counters, op=dist.ReduceOp.SUM, group=group)
    return world


class _CounterBlob:
    """What `ScoreHistogram` and `ProHistogram` share: one blob - a 16-byte header (magic, ABI version and mantissa_bits), then
    uint64 counters - on a GPU, where the library writes it, or on the host as a container.  A subclass sets `mantissa_bits`, names
    its magic, the library's functions (`_LIB`_state_bytes / _reset) and its kind for the messages, and lays out the words."""
    _MAGIC, _LIB, _NAME, _KIND = 0, "", "", ""

    def _allocate(self, device, nbytes: int) -> None:
        self.nbins = 255 << self.mantissa_bits
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.device.type == "cuda":
            assert getattr(hip.lib(), f"{self._LIB}_state_bytes")(self.mantissa_bits) == self._state.numel()
        self.reset()

    def _words(self) -> torch.Tensor:
        """Everything behind the header as one int64 view of the blob (the uint64 counters stay below 2^63)."""
        return self._state[_HEADER_BYTES:].view(torch.int64)

    def _header(self) -> np.ndarray:
        m = self.mantissa_bits
        return np.array([self._MAGIC, (hip.ABI_VERSION << 16) | m, m, 0], np.uint32)

    def reset(self):
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                hip.check(getattr(hip.lib(), f"{self._LIB}_reset")(self._state.data_ptr(), self.mantissa_bits, hip.current_stream()),
                          f"{self._LIB}_reset")
        else:
            self._state.zero_()
            self._state[:_HEADER_BYTES] = torch.from_numpy(self._header().view(np.uint8).copy())
        return self

    def _host_words(self) -> np.ndarray:
        """The words behind the header as numpy int64: the one device -> host read.  The header travels with them and is checked."""
        blob = self._state.cpu().numpy()
        if not np.array_equal(blob[:_HEADER_BYTES].view(np.uint32), self._header()):
            raise hip.VadError(f"{self._NAME}: the state's header is not that of {self._KIND} with mantissa_bits "
                               f"{self.mantissa_bits} (the blob was overwritten)")
        return blob[_HEADER_BYTES:].view(np.int64)

    def _check_saved_m(self, state: dict) -> None:
        if state.get("mantissa_bits") != self.mantissa_bits:
            raise hip.VadError(f"{self._NAME}.load_state_dict: mantissa_bits {state.get('mantissa_bits')!r} of the saved state differs "
                               f"from this histogram's {self.mantissa_bits}")

    def _check_merge(self, other, cls) -> None:
        name = self._NAME
        if not isinstance(other, cls):
            raise hip.VadError(f"{name}.merge: other must be a {name}, got {type(other).__name__}")
        if other.mantissa_bits != self.mantissa_bits:
            raise hip.VadError(f"{name}.merge: mantissa_bits differ ({self.mantissa_bits} and {other.mantissa_bits}); bins of "
                               "different widths cannot be added")
        if other is self:
            raise hip.VadError(f"{name}.merge: other is this histogram")


class ScoreHistogram(_CounterBlob):
    """Counters of (score bin, class) in one device blob (include/vad_hip.h `vad_hist_*`): counts[2][nbins], then rejected[2].

    `accumulate(values, labels)` adds a batch on the GPU; `counts()` / `rejected()` are int64 device tensors, `counts_host()` is the
    one host read (16 * (255 << m) bytes: 8 MB at the default m = 11); `merge`, `all_reduce`, `state_dict` / `load_state_dict`
    combine and carry states.  With `device="cpu"` the object is a container for counters (load, merge, all-reduce, read):
    accumulating runs on the GPU only and there is no CPU fallback."""
    _MAGIC, _LIB, _NAME, _KIND = _HIST_MAGIC, "vad_hist", "ScoreHistogram", "a histogram"

    def __init__(self, mantissa_bits: int = 11, device="cuda"):
        self.mantissa_bits = _check_m(mantissa_bits, "ScoreHistogram")
        self._allocate(device, state_bytes(self.mantissa_bits))

    # ------------------------------------------------------------------ state
    def counts(self) -> torch.Tensor:
        """int64 [2, nbins] on the histogram's device (a copy): row 0 = normal, row 1 = anomalous."""
        return self._words()[:2 * self.nbins].view(2, self.nbins).clone()

    def rejected(self) -> torch.Tensor:
        """int64 [2]: negative, NaN and infinite values seen per class (they are in no bin)."""
        return self._words()[2 * self.nbins:].clone()

    def counts_host(self) -> np.ndarray:
        """The counters as numpy int64 [2, nbins]: the one device -> host read of an evaluation.  The blob's header travels with
        them and is checked."""
        return self._host_words()[:2 * self.nbins].reshape(2, self.nbins).copy()

    def state_dict(self) -> dict:
        """{'mantissa_bits', 'counts' int64 [2, nbins], 'rejected' int64 [2]} on the host: resume a long evaluation later."""
        return {"mantissa_bits": self.mantissa_bits, "counts": self.counts().cpu(), "rejected": self.rejected().cpu()}

    def load_state_dict(self, state: dict) -> "ScoreHistogram":
        self._check_saved_m(state)
        counts = torch.as_tensor(np.asarray(state["counts"]))
        rejected = torch.as_tensor(np.asarray(state["rejected"]))
        if tuple(counts.shape) != (2, self.nbins) or tuple(rejected.shape) != (2,) or counts.dtype != torch.int64 or rejected.dtype != torch.int64:
            raise hip.VadError(f"ScoreHistogram.load_state_dict: counts must be int64 [2, {self.nbins}] and rejected int64 [2], got "
                               f"{counts.dtype} {tuple(counts.shape)} and {rejected.dtype} {tuple(rejected.shape)}")
        words = self._words()
        words[:2 * self.nbins].copy_(counts.reshape(-1))
        words[2 * self.nbins:].copy_(rejected)
        return self

    # ------------------------------------------------------------------ accumulate
    def _accumulate_raw(self, values: torch.Tensor, labels: torch.Tensor, label_format: int, n_groups: int, group_elems: int) -> None:
        """One vad_hist_accumulate call; tensors on this histogram's GPU, kept alive by the caller's references until it ran."""
        with torch.cuda.device(self.device):
            hip.check(hip.lib().vad_hist_accumulate(values.data_ptr(), n_groups, group_elems, labels.data_ptr(), label_format,
                                                    self._state.data_ptr(), self.mantissa_bits, hip.current_stream()),
                      "vad_hist_accumulate")
        _count("hist_accumulate")

    def accumulate(self, values: torch.Tensor, labels: torch.Tensor) -> "ScoreHistogram":
        """Add a batch.  `values`: float32 GPU tensor of any shape (an error map [B,1,H,W], frame scores [B,T], ...).  `labels`:
          * as many elements as `values` - one label per element: float32 (a mask as `resize_masks` / ToTensor give it, positive
            iff > 0.5), uint8 (mask bytes, positive iff >= 128 - the same pixels), bool / other integers (positive iff non-zero);
          * or the shape of the leading axes of `values` - one label per group, applied to all its elements (a frame's label for
            its pixels): positive iff non-zero (floats: iff > 0.5).
        Anything else raises VadError.  Asynchronous on the current stream."""
        if not isinstance(values, torch.Tensor) or not isinstance(labels, torch.Tensor):
            raise hip.VadError("ScoreHistogram.accumulate: values and labels must be torch tensors")
        if self.device.type != "cuda" or not values.is_cuda or not labels.is_cuda:
            raise hip.VadError(f"ScoreHistogram.accumulate: values ({values.device}), labels ({labels.device}) and the histogram "
                               f"({self.device}) must be on the GPU (the histogram is built on the device; there is no CPU fallback)")
        if values.device != self.device or labels.device != self.device:
            raise hip.VadError(f"ScoreHistogram.accumulate: values ({values.device}) and labels ({labels.device}) must be on the "
                               f"histogram's device {self.device}")
        if values.dtype != torch.float32:
            raise hip.VadError(f"ScoreHistogram.accumulate: values must be float32, got {values.dtype}")
        n = values.numel()
        if labels.numel() == n:
            per_group = False
        elif 1 <= labels.dim() < values.dim() and tuple(labels.shape) == tuple(values.shape[:labels.dim()]):
            per_group = True
        else:
            raise hip.VadError(f"ScoreHistogram.accumulate: labels {tuple(labels.shape)} must have as many elements as values "
                               f"{tuple(values.shape)} or the shape of its leading axes")
        if n == 0:
            return self
        values = values.contiguous()
        if per_group:
            lab = (labels > 0.5) if labels.is_floating_point() else (labels != 0)
            lab = lab.to(torch.uint8).contiguous()
            self._accumulate_raw(values, lab, hip.LBL_U8_GROUP, lab.numel(), n // lab.numel())
        elif labels.is_floating_point():
            lab = labels.contiguous() if labels.dtype == torch.float32 else labels.float().contiguous()
            self._accumulate_raw(values, lab, hip.LBL_F32_ELEM, 1, n)
        else:
            lab = labels.contiguous() if labels.dtype == torch.uint8 else ((labels != 0).to(torch.uint8) * 255).contiguous()
            self._accumulate_raw(values, lab, hip.LBL_U8_ELEM, 1, n)
        return self

    # ------------------------------------------------------------------ combine
    def merge(self, other: "ScoreHistogram") -> "ScoreHistogram":
        """self += other (counts and rejected): two streams, or states gathered from elsewhere."""
        self._check_merge(other, ScoreHistogram)
        if self.device.type == "cuda" and other.device == self.device:
            with torch.cuda.device(self.device):
                hip.check(hip.lib().vad_hist_merge(self._state.data_ptr(), other._state.data_ptr(), self.mantissa_bits,
                                                   hip.current_stream()), "vad_hist_merge")
        else:
            self._words().add_(other._words().to(self.device))
        return self

    def all_reduce(self, group=None, force_collective: bool = False) -> int:
        """Sum the counters over the ranks of `group`: ONE all_reduce(SUM) of (2 * nbins + 2) int64 words, after which every rank
        holds the histogram of the whole stream.  Returns the world size."""
        return allreduce_counters_(self._words(), group, force_collective)

    # ------------------------------------------------------------------ metrics (one host read)
    def auroc(self) -> Tuple[float, float]:
        return auroc_from_counts(self.counts_host())


# ====================================================================== host half: numpy, float64 from integer counts
def _mantissa_bits_of(nbins: int) -> Optional[int]:
    """The m with 255 << m == nbins, or None."""
    return next((k for k in range(MIN_MANTISSA_BITS, MAX_MANTISSA_BITS + 1) if 255 << k == nbins), None)


def _as_counts(counts) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (neg int64 [nbins], pos int64 [nbins], mantissa_bits)."""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"counts must be an integer array [2, nbins], got {c.dtype} {c.shape}")
    m = _mantissa_bits_of(c.shape[1])
    if m is None:
        raise ValueError(f"counts has {c.shape[1]} bins: not 255 << m for a mantissa_bits m in {MIN_MANTISSA_BITS}..{MAX_MANTISSA_BITS}")
    c = c.astype(np.int64, copy=False)
    if (c < 0).any():
        raise ValueError("counts must be non-negative")
    return c[0], c[1], m


def bin_lower_edges(keys, mantissa_bits: int) -> np.ndarray:
    """The float32 whose bits are key << (23 - m): the smallest score of bin `key`, and the value every score of the bin is
    quantised to."""
    return (np.asarray(keys, dtype=np.uint32) << np.uint32(23 - mantissa_bits)).view(np.float32)


def _total(c: np.ndarray) -> int:
    """Sum of int64 counters as a Python int (exact beyond 2^63)."""
    if len(c) == 0:
        return 0
    return int(c.sum()) if float(c.max()) * len(c) < 2.0 ** 62 else sum(c.tolist())


def _exact_cumsum(c: np.ndarray) -> np.ndarray:
    """Running sums of non-negative int64 / uint64 counters as float64, each rounded once: in int64 while the total stays below
    2^62, in Python integers near 2^63."""
    if len(c) and float(c.max()) * len(c) < 2.0 ** 62:
        return np.cumsum(c.astype(np.int64)).astype(np.float64)
    sums, run = [], 0
    for v in c.tolist():
        run += v
        sums.append(float(run))
    return np.array(sums, np.float64)


def _populated(counts, what: str):
    """-> (keys ascending, neg, pos, P, N, m) over the populated bins; P, N as Python ints."""
    neg, pos, m = _as_counts(counts)
    keys = np.flatnonzero((neg != 0) | (pos != 0))
    neg, pos = neg[keys], pos[keys]
    n_pos, n_neg = _total(pos), _total(neg)
    if n_pos == 0 or n_neg == 0:
        raise ValueError(f"{what} needs both classes")
    return keys, neg, pos, n_pos, n_neg, m


def auroc_from_counts(counts) -> Tuple[float, float]:
    """(auroc, tie_bound).  auroc: the Mann-Whitney statistic of the quantised scores with half credit inside a bin -
    `scoring.roc_auc(labels, q(scores))`, q = keep the top m mantissa bits.  tie_bound = 0.5 * sum_b pos[b] * neg[b] / (P * N):
    quantising is monotone, so the only pairs it can change are the (anomalous, normal) pairs that share a bin, each by at most
    half a credit - |auroc - AUROC of the unquantised scores| <= tie_bound, from the same counts.  The sums are exact integers
    (int64 while 2 P N < 2^63, Python integers above) and each quotient is rounded once."""
    keys, neg, pos, n_pos, n_neg, _ = _populated(counts, "auroc_from_counts")
    denom = 2 * n_pos * n_neg
    if denom < 2 ** 63:
        below = np.cumsum(neg) - neg                                   # normal scores in lower bins
        two_u = int((pos * (2 * below + neg)).sum())
        ties = int((pos * neg).sum())
    else:
        two_u = ties = below = 0
        for p, q in zip(pos.tolist(), neg.tolist()):
            two_u += p * (2 * below + q)
            ties += p * q
            below += q
    return two_u / denom, ties / denom


def roc_curve_from_counts(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(fpr, tpr, thresholds) at the populated bins: point k >= 1 classifies `score >= thresholds[k]` as anomalous, thresholds are
    the bins' lower edges (float32) in descending order - a raw score is >= a bin's lower edge exactly when its bin is that one
    or a higher one, so the thresholds apply to unquantised scores as they stand.  Point 0 is (0, 0) with threshold +inf."""
    keys, neg, pos, n_pos, n_neg, m = _populated(counts, "roc_curve_from_counts")
    tp = np.concatenate([[0], np.cumsum(pos[::-1])])
    fp = np.concatenate([[0], np.cumsum(neg[::-1])])
    thr = np.concatenate([np.array([np.inf], np.float32), bin_lower_edges(keys[::-1], m)])
    return fp / float(n_neg), tp / float(n_pos), thr


def average_precision_from_counts(counts) -> float:
    """sum_k (recall_k - recall_{k-1}) * precision_k over the thresholds of `roc_curve_from_counts`:
    sklearn.metrics.average_precision_score of the quantised scores."""
    keys, neg, pos, n_pos, n_neg, _ = _populated(counts, "average_precision_from_counts")
    tp = np.cumsum(pos[::-1]).astype(np.float64)
    fp = np.cumsum(neg[::-1]).astype(np.float64)
    return float(np.sum(pos[::-1] / float(n_pos) * (tp / (tp + fp))))


def threshold_at_fpr(counts, fpr: float) -> Tuple[float, float, float]:
    """(threshold, tpr, fpr reached): the lowest threshold of the curve whose false-positive rate is <= `fpr` (the highest
    detection rate at that budget).  +inf (nothing flagged) when even the top bin exceeds it."""
    if not 0.0 <= fpr <= 1.0:
        raise ValueError(f"threshold_at_fpr: fpr must be in [0, 1], got {fpr!r}")
    f, t, thr = roc_curve_from_counts(counts)
    k = int(np.flatnonzero(f <= fpr)[-1])
    return float(thr[k]), float(t[k]), float(f[k])


def best_f1_threshold(counts) -> Tuple[float, float]:
    """(threshold, f1): the curve threshold with the largest F1 = 2 TP / (2 TP + FP + FN); the highest such threshold on a tie."""
    keys, neg, pos, n_pos, n_neg, m = _populated(counts, "best_f1_threshold")
    tp = np.cumsum(pos[::-1]).astype(np.float64)
    fp = np.cumsum(neg[::-1]).astype(np.float64)
    f1 = 2.0 * tp / (tp + fp + float(n_pos))
    k = int(np.argmax(f1))
    return float(bin_lower_edges(keys[::-1], m)[k]), float(f1[k])


def class_stats_from_counts(counts) -> dict:
    """{'normal' | 'anomaly': {'count', 'mean', 'std'}} of the quantised scores (population std, as numpy's `.std()`): the "Score
    Statistics" of evaluate_video.py:178-187.  A class without scores has count 0 and NaN statistics."""
    neg, pos, m = _as_counts(counts)
    out = {}
    for name, c in (("normal", neg), ("anomaly", pos)):
        keys = np.flatnonzero(c)
        n = _total(c[keys])
        if n == 0:
            out[name] = {"count": 0, "mean": float("nan"), "std": float("nan")}
            continue
        w = c[keys].astype(np.float64) / float(n)
        e = bin_lower_edges(keys, m).astype(np.float64)
        mean = float(np.sum(w * e))
        out[name] = {"count": n, "mean": mean, "std": float(np.sqrt(np.sum(w * (e - mean) ** 2)))}
    return out


# ====================================================================== per-region overlap (AUPRO)
# Per-region overlap, the localisation metric of MVTec-style data.  Thresholds are the bins' lower edges;
# FPR(t) = the share of all normal pixels with v >= t; PRO(t) = the mean over all connected anomalous regions r of the evaluation
# of |{p in r : v_p >= t}| / |r|.  PRO(t) = sum over anomalous pixels of [v_p >= t] / (R |r(p)|) is a histogram in which a pixel
# adds a weight; the device adds the integer W(r) = (2^44 + |r| / 2) // |r| (`vad_pro_accumulate`, csrc/region_overlap.hip), so
# the counters stay exact integer sums.
PRO_WEIGHT_BITS = hip.PRO_WEIGHT_BITS
PRO_MAX_REGIONS = 1 << 19      # a region adds at most 2^44 + |r| / 2 to a bin: beyond 2^19 regions a uint64 bin could wrap
_PRO_MAGIC = 0x50444156        # "VADP", csrc/region_overlap.hip
_PRO_TAIL = 5                  # regions, max_region, rejected[2], flags


def pro_state_bytes(mantissa_bits: int) -> int:
    """Size of the device blob: 16-byte header, uint64 wpos / pos / neg [nbins], uint64 regions, max_region, rejected[2], flags."""
    return _HEADER_BYTES + 8 * (3 * num_bins(mantissa_bits) + _PRO_TAIL)


def region_weight(size: int) -> int:
    """W(r) for a region of `size` pixels: 2^44 / size rounded to the nearest integer."""
    return ((1 << PRO_WEIGHT_BITS) + size // 2) // size


def _pro_points(wpos, neg, regions, what: str):
    """-> (keys descending, fpr float64 [K + 1], pro float64 [K + 1], m): the curve's vertices after (0, 0), one per populated bin
    from the highest key down."""
    w = np.asarray(wpos.detach().cpu().numpy() if isinstance(wpos, torch.Tensor) else wpos)
    q = np.asarray(neg.detach().cpu().numpy() if isinstance(neg, torch.Tensor) else neg)
    if w.ndim != 1 or q.shape != w.shape or not np.issubdtype(w.dtype, np.integer) or not np.issubdtype(q.dtype, np.integer):
        raise ValueError(f"{what}: wpos and neg must be integer arrays [nbins] of one length, got {w.dtype} {w.shape} and {q.dtype} {q.shape}")
    m = _mantissa_bits_of(w.shape[0])
    if m is None:
        raise ValueError(f"{what}: {w.shape[0]} bins are not 255 << m for a mantissa_bits m in {MIN_MANTISSA_BITS}..{MAX_MANTISSA_BITS}")
    if w.dtype == np.int64:
        w = w.view(np.uint64)                                          # the device's uint64 sums, read through an int64 view
    if (q < 0).any() or (w.dtype != np.uint64 and (w < 0).any()):
        raise ValueError(f"{what}: counters must be non-negative")
    regions = int(regions)
    if regions <= 0:
        raise ValueError(f"{what}: no region (the masks hold no anomalous pixel)")
    if regions > PRO_MAX_REGIONS:
        raise ValueError(f"{what}: {regions} regions are more than 2^19 = {PRO_MAX_REGIONS}: a weighted bin may have wrapped")
    keys = np.flatnonzero((w != 0) | (q != 0))[::-1]
    w, q = w[keys], q[keys].astype(np.int64)
    n_neg = _total(q)
    if n_neg == 0:
        raise ValueError(f"{what}: no normal pixel")
    fpr = np.concatenate([[0.0], _exact_cumsum(q) / float(n_neg)])
    pro = np.concatenate([[0.0], _exact_cumsum(w) / float(regions << PRO_WEIGHT_BITS)])
    return keys, fpr, pro, m


def pro_curve_from_counts(wpos, neg, regions) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(fpr, pro, thresholds) at the populated bins, as `roc_curve_from_counts`: point k >= 1 flags `score >= thresholds[k]`
    (bin lower edges, float32, descending - they apply to unquantised scores as they stand); point 0 is (0, 0) at +inf."""
    keys, fpr, pro, m = _pro_points(wpos, neg, regions, "pro_curve_from_counts")
    return fpr, pro, np.concatenate([np.array([np.inf], np.float32), bin_lower_edges(keys, m)])


def aupro_from_counts(wpos, neg, regions, max_region, fpr_limit: float = 0.3) -> Tuple[float, float, float]:
    """(aupro, quant_bound, weight_bound) from the weighted histogram `wpos` [nbins], the normal pixels' histogram `neg` [nbins],
    the number of regions and the largest region's size.

    aupro: the curve (fpr, pro) of `pro_curve_from_counts`, joined by straight lines, integrated up to `fpr_limit` (in (0, 1]) with
    one linear interpolation on the segment the limit cuts, divided by `fpr_limit` - the integration of the MVTec evaluation.
    weight_bound = max_region / 2^45: a weight is 2^44 / |r| rounded to an integer, so the overlap of one region is off by at most
    |r| / 2^45 at every threshold, and so are their mean and the normalised area: |aupro - AUPRO of the quantised scores| <= it.
    quant_bound: a threshold at a bin edge selects the same pixels on raw and on quantised scores, so every vertex of this curve is
    a vertex of the exact curve, which is monotone between two of them: the areas differ by at most 0.5 * dFPR * dPRO per whole
    segment and (fpr_limit - FPR_0) * dPRO on the cut one, all divided by `fpr_limit`.
    |aupro - AUPRO of the unquantised scores| <= quant_bound + weight_bound."""
    limit = _check_number(fpr_limit, "fpr_limit", "aupro_from_counts", lambda v: 0.0 < float(v) <= 1.0, "in (0, 1]", ValueError)
    _, fpr, pro, _ = _pro_points(wpos, neg, regions, "aupro_from_counts")
    max_region = int(max_region)
    if max_region <= 0:
        raise ValueError(f"aupro_from_counts: max_region must be positive with {int(regions)} regions, got {max_region}")
    whole = int(np.flatnonzero(fpr <= limit)[-1])                      # vertices 0..whole lie inside the limit
    df, dp = np.diff(fpr[:whole + 1]), np.diff(pro[:whole + 1])
    area = float(np.sum(df * (pro[1:whole + 1] + pro[:whole]) * 0.5))
    bound = float(np.sum(0.5 * df * dp))
    if fpr[whole] < limit:                                             # the limit cuts segment whole -> whole + 1 (fpr ends at 1)
        f0, f1, p0, p1 = fpr[whole], fpr[whole + 1], pro[whole], pro[whole + 1]
        p_cut = p0 + (p1 - p0) * (limit - f0) / (f1 - f0)
        area += float((limit - f0) * (p0 + p_cut) * 0.5)
        bound += float((limit - f0) * (p1 - p0))
    return area / limit, bound / limit, max_region / float(1 << (PRO_WEIGHT_BITS + 1))


def _mask_planes(masks: torch.Tensor, what: str):
    """-> (contiguous mask tensor, label format, B, H, W) for a mask batch [B,H,W] or [B,1,H,W]: float masks (anomalous iff > 0.5)
    as float32, uint8 bytes (iff >= 128) as they are, bool / other integers (iff non-zero) as bytes 0 / 255."""
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise hip.VadError(f"{what}: masks must be [B,H,W] or [B,1,H,W], got {tuple(masks.shape)}")
    if masks.is_floating_point():
        m, fmt = (masks if masks.dtype == torch.float32 else masks.float()).contiguous(), hip.LBL_F32_ELEM
    else:
        m, fmt = (masks if masks.dtype == torch.uint8 else (masks != 0).to(torch.uint8) * 255).contiguous(), hip.LBL_U8_ELEM
    return m, fmt, m.shape[0], m.shape[1], m.shape[2]


def _pro_workspace(n: int, h: int, w: int, device, what: str) -> torch.Tensor:
    return _workspace(hip.lib().vad_pro_workspace_bytes(n, h, w), device, what,
                      f"{n} masks of {h} x {w} are out of range (h * w < 2^31 - 1, n * h * w <= 2^38)")


def label_regions(masks: torch.Tensor, connectivity: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """Connected anomalous regions of a batch of masks on the GPU (`vad_label_regions`): -> (labels int32 [B,H,W], sizes uint32
    [B,H,W]).  labels: 0 = normal, otherwise 1 + (the smallest y * W + x of the pixel's region); every image is labelled on its own.
    sizes: the region's pixel count at its root pixel (label == own index + 1), 0 elsewhere.  connectivity 8 is
    `scipy.ndimage.label(mask, structure=ones((3, 3)))`, 4 its default structure.  Reads the kernels' flag word (one 4-byte copy,
    which waits for the labelling) and raises VadError if it is set."""
    connectivity = _check_connectivity(connectivity, "label_regions")
    if not isinstance(masks, torch.Tensor):
        raise hip.VadError("label_regions: masks must be a torch tensor")
    if not masks.is_cuda:
        raise hip.VadError(f"label_regions: masks ({masks.device}) must be on the GPU (regions are labelled on the device; there is no CPU fallback)")
    m, fmt, b, h, w = _mask_planes(masks, "label_regions")
    labels = torch.empty((b, h, w), dtype=torch.int32, device=m.device)
    sizes = torch.empty((b, h, w), dtype=torch.uint32, device=m.device)
    with torch.cuda.device(m.device):
        ws = _pro_workspace(b, h, w, m.device, "label_regions")
        hip.check(hip.lib().vad_label_regions(m.data_ptr(), fmt, b, h, w, connectivity, labels.data_ptr(), sizes.data_ptr(),
                                              ws.data_ptr(), ws.numel(), hip.current_stream()), "vad_label_regions")
    _launched(ws, "label_regions")
    return labels, sizes


class ProHistogram(_CounterBlob):
    """The counters of the per-region overlap in one device blob (include/vad_hip.h `vad_pro_*`): the weighted histogram `wpos`
    of the anomalous pixels, their plain histogram `pos` and the normal pixels' `neg` - `counts()` is what a `ScoreHistogram` of
    the same batches would hold, so `auroc()` comes with it -, the number of regions, the largest region, rejected values per
    class and the labelling kernels' flag word.

    `accumulate(values, masks)` labels the masks and adds the batch on the GPU, asynchronously; `aupro()` is the one host read
    (24 * (255 << m) bytes: 12 MB at the default m = 11).  With `device="cpu"` the object is a container for counters (load,
    merge, all-reduce, read): accumulating runs on the GPU only and there is no CPU fallback.  The words behind the header: wpos,
    pos, neg [nbins] each, then regions, max_region, rejected[2], flags."""
    _MAGIC, _LIB, _NAME, _KIND = _PRO_MAGIC, "vad_pro", "ProHistogram", "a per-region histogram"

    def __init__(self, mantissa_bits: int = 11, device="cuda", connectivity: int = 8):
        self.mantissa_bits = _check_m(mantissa_bits, "ProHistogram")
        self.connectivity = _check_connectivity(connectivity, "ProHistogram")
        self._ws = None
        self._allocate(device, pro_state_bytes(self.mantissa_bits))

    # ------------------------------------------------------------------ state
    def weighted(self) -> torch.Tensor:
        """int64 [nbins] on the histogram's device (a copy): the bits of the uint64 sums of W(r) per bin."""
        return self._words()[:self.nbins].clone()

    def counts(self) -> torch.Tensor:
        """int64 [2, nbins] (a copy): row 0 = normal, row 1 = anomalous - the counts of `ScoreHistogram`."""
        w = self._words()
        return torch.stack([w[2 * self.nbins:3 * self.nbins], w[self.nbins:2 * self.nbins]])

    def _tail(self) -> list:
        """[regions, max_region, rejected normal, rejected anomalous, flags] on the host; raises on a set flag word."""
        tail = self._words()[3 * self.nbins:].tolist()
        _raise_on_flags(tail[4], "ProHistogram")
        return tail

    def regions(self) -> int:
        return self._tail()[0]

    def max_region(self) -> int:
        return self._tail()[1]

    def rejected(self) -> torch.Tensor:
        """int64 [2]: negative, NaN and infinite values seen per class (in no bin; an anomalous one still counts towards |r|)."""
        return self._words()[3 * self.nbins + 2:3 * self.nbins + 4].clone()

    def flags(self) -> int:
        return int(self._words()[3 * self.nbins + 4].item())

    def _host(self):
        """(wpos uint64 [nbins], pos, neg int64 [nbins], tail): the one device -> host read; header and flags are checked."""
        words = self._host_words()
        tail = words[3 * self.nbins:].tolist()
        _raise_on_flags(tail[4], "ProHistogram")
        nb = self.nbins
        return words[:nb].view(np.uint64).copy(), words[nb:2 * nb].copy(), words[2 * nb:3 * nb].copy(), tail

    def state_dict(self) -> dict:
        """Host copies of every counter, with mantissa_bits and connectivity: resume a long evaluation later."""
        w = self._words().cpu()
        nb = self.nbins
        return {"mantissa_bits": self.mantissa_bits, "connectivity": self.connectivity, "weighted": w[:nb].clone(),
                "counts": torch.stack([w[2 * nb:3 * nb], w[nb:2 * nb]]), "regions": int(w[3 * nb]), "max_region": int(w[3 * nb + 1]),
                "rejected": w[3 * nb + 2:3 * nb + 4].clone(), "flags": int(w[3 * nb + 4])}

    def load_state_dict(self, state: dict) -> "ProHistogram":
        self._check_saved_m(state)
        if state.get("connectivity") != self.connectivity:
            raise hip.VadError(f"ProHistogram.load_state_dict: connectivity {state.get('connectivity')!r} of the saved state differs "
                               f"from this histogram's {self.connectivity}")
        weighted = torch.as_tensor(np.asarray(state["weighted"]))
        counts = torch.as_tensor(np.asarray(state["counts"]))
        rejected = torch.as_tensor(np.asarray(state["rejected"]))
        nb = self.nbins
        if (tuple(weighted.shape) != (nb,) or tuple(counts.shape) != (2, nb) or tuple(rejected.shape) != (2,)
                or any(t.dtype != torch.int64 for t in (weighted, counts, rejected))):
            raise hip.VadError(f"ProHistogram.load_state_dict: weighted must be int64 [{nb}], counts int64 [2, {nb}] and rejected int64 "
                               f"[2], got {weighted.dtype} {tuple(weighted.shape)}, {counts.dtype} {tuple(counts.shape)} and "
                               f"{rejected.dtype} {tuple(rejected.shape)}")
        words = self._words()
        words[:nb].copy_(weighted)
        words[nb:2 * nb].copy_(counts[1])
        words[2 * nb:3 * nb].copy_(counts[0])
        words[3 * nb:].copy_(torch.tensor([int(state["regions"]), int(state["max_region"]), int(rejected[0]), int(rejected[1]),
                                           int(state.get("flags", 0))], dtype=torch.int64))
        return self

    # ------------------------------------------------------------------ accumulate
    def accumulate(self, values: torch.Tensor, masks: torch.Tensor) -> "ProHistogram":
        """Add a batch.  `values`: float32 GPU tensor [B,1,H,W] or [B,H,W] (an error map, an SSIM map).  `masks`: the ground truth
        at the same resolution, [B,1,H,W] or [B,H,W]: float (anomalous iff > 0.5), uint8 (iff >= 128 - the same pixels), bool /
        other integers (iff non-zero).  Labels the masks and adds the counters in one `vad_pro_accumulate` call, asynchronous on
        the current stream; the workspace is kept and grown as needed."""
        what = "ProHistogram.accumulate"
        if not isinstance(values, torch.Tensor) or not isinstance(masks, torch.Tensor):
            raise hip.VadError(f"{what}: values and masks must be torch tensors")
        if self.device.type != "cuda" or not values.is_cuda or not masks.is_cuda:
            raise hip.VadError(f"{what}: values ({values.device}), masks ({masks.device}) and the histogram ({self.device}) must be "
                               "on the GPU (regions are labelled on the device; there is no CPU fallback)")
        if values.device != self.device or masks.device != self.device:
            raise hip.VadError(f"{what}: values ({values.device}) and masks ({masks.device}) must be on the histogram's device {self.device}")
        if values.dtype != torch.float32:
            raise hip.VadError(f"{what}: values must be float32, got {values.dtype}")
        if values.dim() == 4 and values.shape[1] == 1:
            values = values[:, 0]
        if values.dim() != 3:
            raise hip.VadError(f"{what}: values must be [B,1,H,W] or [B,H,W], got {tuple(values.shape)}")
        m, fmt, b, h, w = _mask_planes(masks, what)
        if tuple(values.shape) != (b, h, w):
            raise hip.VadError(f"{what}: masks {tuple(masks.shape)} must have the batch and resolution of values {tuple(values.shape)}")
        if b == 0:
            return self
        values = values.contiguous()
        with torch.cuda.device(self.device):
            need = hip.lib().vad_pro_workspace_bytes(b, h, w)
            if self._ws is None or self._ws.numel() < need:
                self._ws = _pro_workspace(b, h, w, self.device, what)
            hip.check(hip.lib().vad_pro_accumulate(values.data_ptr(), m.data_ptr(), fmt, b, h, w, self.connectivity,
                                                   self._state.data_ptr(), self.mantissa_bits, self._ws.data_ptr(), self._ws.numel(),
                                                   hip.current_stream()), "vad_pro_accumulate")
        _count("pro_accumulate")
        return self

    # ------------------------------------------------------------------ combine
    def merge(self, other: "ProHistogram") -> "ProHistogram":
        """self += other: sums of the counters, the larger max_region, the union of the flags."""
        self._check_merge(other, ProHistogram)
        if other.connectivity != self.connectivity:
            raise hip.VadError(f"ProHistogram.merge: connectivity differs ({self.connectivity} and {other.connectivity}); regions "
                               "of different definitions cannot be averaged")
        if self.device.type == "cuda" and other.device == self.device:
            with torch.cuda.device(self.device):
                hip.check(hip.lib().vad_pro_merge(self._state.data_ptr(), other._state.data_ptr(), self.mantissa_bits,
                                                  hip.current_stream()), "vad_pro_merge")
        else:
            mine, theirs = self._words(), other._words().to(self.device)
            k = 3 * self.nbins
            biggest, flags = torch.maximum(mine[k + 1], theirs[k + 1]), mine[k + 4] | theirs[k + 4]
            mine.add_(theirs)
            mine[k + 1], mine[k + 4] = biggest, flags
        return self

    def all_reduce(self, group=None, force_collective: bool = False) -> int:
        """Combine the ranks of `group`: ONE all_reduce(SUM) of the counters (a summed flag word is non-zero exactly when a rank's
        is) and ONE all_reduce(MAX) of the max_region word.  Returns the world size."""
        import torch.distributed as dist
        words = self._words()
        k = 3 * self.nbins + 1
        biggest = words[k:k + 1].clone()
        words[k] = 0
        world = allreduce_counters_(words, group, force_collective)
        if world > 1 or (force_collective and dist.is_available() and dist.is_initialized()):
            if biggest.is_cuda and dist.get_backend(group) == "gloo":
                host = biggest.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.MAX, group=group)
                biggest.copy_(host)
            else:
                dist.all_reduce(biggest, op=dist.ReduceOp.MAX, group=group)
        words[k] = biggest[0]
        return world

    # ------------------------------------------------------------------ metrics (one host read)
    def aupro(self, fpr_limit: float = 0.3) -> Tuple[float, float, float]:
        wpos, _, neg, tail = self._host()
        return aupro_from_counts(wpos, neg, tail[0], tail[1], fpr_limit)

    def pro_curve(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        wpos, _, neg, tail = self._host()
        return pro_curve_from_counts(wpos, neg, tail[0])

    def auroc(self) -> Tuple[float, float]:
        _, pos, neg, _ = self._host()
        return auroc_from_counts(np.stack([neg, pos]))


# ====================================================================== smoothed anomaly maps
# The two steps an MVTec-style evaluation takes before it ranks pixels and images: the map is smoothed with
# a Gaussian - `scipy.ndimage.gaussian_filter(map, sigma=4)`; a raw squared-error map is speckle, and isolated hot pixels on normal
# texture use up the false-positive budget AUPRO integrates over - and the image is scored by the maximum of the smoothed map.
SMOOTH_MAX_RADIUS = hip.SMOOTH_MAX_RADIUS
_TAPS = {}                     # (sigma, truncate, device) -> device taps: uploaded once, never written again


def _gaussian_taps64(sigma: float, r: int) -> np.ndarray:
    """scipy's `_gaussian_kernel1d(sigma, 0, r)`: float64 [2r + 1], normalised."""
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def gaussian_taps(sigma: float, truncate: float = 4.0) -> Tuple[int, np.ndarray]:
    """(r, float32 [2r + 1]): the taps of `scipy.ndimage.gaussian_filter(sigma=sigma, truncate=truncate)` - r = int(truncate * sigma
    + 0.5), w[k] = exp(-0.5 / sigma^2 * (k - r)^2) in float64, divided by their float64 sum, rounded once to float32.  Host only.
    VadError for a sigma / truncate that is not a positive finite number, for a radius outside 1..32, and for taps that underflow
    float32 (every tap must be > 0: a zero tap would turn an infinite pixel into NaN)."""
    for name, v in (("sigma", sigma), ("truncate", truncate)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
            raise hip.VadError(f"gaussian_taps: {name} must be a positive finite number, got {v!r}")
    sigma, truncate = float(sigma), float(truncate)
    r = int(truncate * sigma + 0.5)
    if not 1 <= r <= SMOOTH_MAX_RADIUS:
        raise hip.VadError(f"gaussian_taps: radius int(truncate * sigma + 0.5) = {r} (sigma {sigma}, truncate {truncate}) must be in "
                           f"1..{SMOOTH_MAX_RADIUS}")
    w = _gaussian_taps64(sigma, r).astype(np.float32)
    if not (w > 0).all():
        raise hip.VadError(f"gaussian_taps: the outer taps of sigma {sigma}, truncate {truncate} underflow float32; use a smaller truncate")
    return r, w


def _device_taps(sigma: float, truncate: float, device, host_taps: np.ndarray) -> torch.Tensor:
    """The taps of (sigma, truncate) on `device`: uploaded on first use, then read only."""
    key = (float(sigma), float(truncate), str(device))
    with hip._lock:
        hit = _TAPS.get(key)
    if hit is None:
        hit = torch.from_numpy(host_taps).to(device)
        with hip._lock:
            hit = _TAPS.setdefault(key, hit)
    return hit


def smooth_maps(maps: torch.Tensor, sigma: float = 4.0, truncate: float = 4.0, out: Optional[torch.Tensor] = None, return_max=False):
    """`scipy.ndimage.gaussian_filter(frame, sigma, truncate=truncate)` (mode="reflect") of every H x W frame of `maps` on the GPU
    (`vad_smooth_maps`, csrc/map_smooth.hip).  `maps`: float32 GPU tensor, contiguous, the last two dimensions H, W and any leading
    ones - `[B,1,H,W]` error / SSIM maps, the `[B,T,1,H,W]` maps of the video model's `score_all`, `[N,H,W]`; frames are smoothed one
    by one, never across time.  The arithmetic is float32 and fully specified (first along H, then along W, ascending taps, every
    product and sum rounded on its own): tests/map_smooth_ref.py restates it bit for bit; it is within 2 (2r + 3) 2^-24 G(|x|) of
    scipy's float64 result.  The radius r = int(truncate * sigma + 0.5) must be in 1..32 and <= min(H, W) (one reflection).
    Returns the smoothed tensor (written to `out` if given: same shape, float32, contiguous, not overlapping `maps`); with
    `return_max=True` also the per-frame maxima of the smoothed maps in the leading shape (`torch.amax` semantics: NaN if any
    pixel of the frame is NaN) - the image score of the MVTec evaluation; with `return_max="only"` just the maxima, and no map is
    written.  Taps are uploaded once per (sigma, truncate, device).  Asynchronous on the current stream."""
    what = "smooth_maps"
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    if not isinstance(return_max, bool) and return_max != "only":
        raise hip.VadError(f"{what}: return_max must be False, True or 'only', got {return_max!r}")
    r, host_taps = gaussian_taps(sigma, truncate)                 # refuses a bad sigma / truncate before anything else
    if not maps.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the GPU (the smoothing runs on the device; there is no CPU fallback)")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if maps.dim() < 2:
        raise hip.VadError(f"{what}: maps must have at least the two dimensions H, W, got {tuple(maps.shape)}")
    if not maps.is_contiguous():
        raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
    lead, h, w = tuple(maps.shape[:-2]), int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
    if r > min(h, w):
        raise hip.VadError(f"{what}: radius {r} (sigma {sigma}, truncate {truncate}) exceeds min(H, W) of {h} x {w} frames: only one "
                           "reflection at the border is supported")
    only = return_max == "only"
    if only and out is not None:
        raise hip.VadError(f"{what}: return_max='only' writes no map; out must be None")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(maps.shape) or out.dtype != torch.float32
                            or out.device != maps.device or not out.is_contiguous()):
        raise hip.VadError(f"{what}: out must be a contiguous float32 tensor {tuple(maps.shape)} on {maps.device}")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    with torch.cuda.device(maps.device):
        if out is None and not only:
            out = torch.empty_like(maps)
        fmax = torch.empty(lead, dtype=torch.float32, device=maps.device) if return_max else None
        if n > 0:
            l = hip.lib()
            taps = _device_taps(sigma, truncate, maps.device, host_taps)
            need = l.vad_smooth_workspace_bytes(n, h, w, r) if return_max else 0
            ws = torch.empty(need, dtype=torch.uint8, device=maps.device) if need else None
            hip.check(l.vad_smooth_maps(maps.data_ptr(), n, h, w, taps.data_ptr(), r, hip.ptr(out), hip.ptr(fmax), hip.ptr(ws), need,
                                        hip.current_stream()), "vad_smooth_maps")
            _count("smooth_maps")
    if only:
        return fmax
    return (out, fmax) if return_max else out


# ====================================================================== grey morphology of anomaly maps
# The clean-up a deployed line applies between the map and its threshold: an opening removes speckle that no
# Gaussian removes without blurring real defects, a closing fills pinholes and joins the fragments of one cracked defect.  Flat
# rectangular structuring element; scipy.ndimage.grey_erosion / grey_dilation / grey_opening / grey_closing to the bit.
MORPH_MAX_SIZE = hip.MORPH_MAX_SIZE
MORPH_OPS = tuple(hip.MORPH_OPS)
MORPH_MAX_STEPS = 4


def _morph_size(size, what: str) -> Tuple[int, int]:
    """An int or (size_h, size_w), each in 1..31 -> (size_h, size_w)."""
    if _is_int(size):
        size = (size, size)
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size):
        raise hip.VadError(f"{what}: size must be an int or (size_h, size_w), got {size!r}")
    sh, sw = int(size[0]), int(size[1])
    if not (1 <= sh <= MORPH_MAX_SIZE and 1 <= sw <= MORPH_MAX_SIZE):
        raise hip.VadError(f"{what}: size must be in 1..{MORPH_MAX_SIZE} per side, got {sh} x {sw}")
    return sh, sw


def _morph_op(op, what: str) -> str:
    if not isinstance(op, str) or op not in hip.MORPH_OPS:
        raise hip.VadError(f"{what}: op must be one of {MORPH_OPS}, got {op!r}")
    return op


def morph_steps(spec) -> Tuple[Tuple[str, Tuple[int, int]], ...]:
    """What the `morph=` arguments of the scoring entry points take, normalised to a tuple of (op, (size_h, size_w)) steps: None ->
    (), one step `("open", 3)` / `("open", (3, 5))`, or a list of at most four steps such as `[("open", 2), ("close", 5)]` (despeckle,
    then join fragments).  `VadError` for anything else: an unknown op, a size outside 1..31, an empty list, more than four steps."""
    what = "morph_steps"
    if spec is None:
        return ()
    if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str):
        spec = [spec]
    if not isinstance(spec, list):
        raise hip.VadError(f"{what}: a spec is None, one step (op, size) or a list of steps, got {spec!r}")
    if not 1 <= len(spec) <= MORPH_MAX_STEPS:
        raise hip.VadError(f"{what}: a list holds 1..{MORPH_MAX_STEPS} steps, got {len(spec)}")
    steps = []
    for step in spec:
        if not isinstance(step, (tuple, list)) or len(step) != 2:
            raise hip.VadError(f"{what}: a step is (op, size), got {step!r}")
        steps.append((_morph_op(step[0], what), _morph_size(step[1], what)))
    return tuple(steps)


def morph_maps(maps: torch.Tensor, op: str, size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`scipy.ndimage.grey_erosion` / `grey_dilation` / `grey_opening` / `grey_closing` (`op` = "erode" | "dilate" | "open" | "close")
    with `size=(size_h, size_w)` (an int = a square) and mode="reflect" of every H x W frame of `maps` on the GPU (`vad_morph_maps`,
    csrc/map_morph.hip): for a flat rectangle, the minimum / maximum over a window clamped to the frame, even sizes by scipy's
    convention (erode reaches size // 2 towards index 0, dilate (size - 1) // 2); sides in 1..31, larger than the frame allowed.
    `maps` as `smooth_maps` takes them: float32 GPU tensor, contiguous, the last two dimensions H, W and any leading ones; frames
    are processed one by one.  Nothing is rounded, so the result is specified to the bit (tests/map_morph_ref.py): a NaN makes
    exactly the pixels whose window holds it NaN (open / close: the windows of both steps), -0 orders below +0.  The operations
    commute with a threshold: `morph_maps(x, op, s) >= t` is the binary `op` of `x >= t`.  Returns a new tensor, or `out` (same
    shape, float32, contiguous, not overlapping `maps`).  One launch, no workspace; asynchronous on the current stream."""
    what = "morph_maps"
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    code = hip.MORPH_OPS[_morph_op(op, what)]
    sh, sw = _morph_size(size, what)
    if not maps.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the GPU (the morphology runs on the device; there is no CPU fallback)")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if maps.dim() < 2:
        raise hip.VadError(f"{what}: maps must have at least the two dimensions H, W, got {tuple(maps.shape)}")
    if not maps.is_contiguous():
        raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
    lead, h, w = tuple(maps.shape[:-2]), int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(maps.shape) or out.dtype != torch.float32
                            or out.device != maps.device or not out.is_contiguous()):
        raise hip.VadError(f"{what}: out must be a contiguous float32 tensor {tuple(maps.shape)} on {maps.device}")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    with torch.cuda.device(maps.device):
        if out is None:
            out = torch.empty_like(maps)
        if n > 0:
            hip.check(hip.lib().vad_morph_maps(maps.data_ptr(), n, h, w, code, sh, sw, out.data_ptr(), hip.current_stream()), "vad_morph_maps")
            _count("morph_maps")
    return out


def apply_morph(maps: torch.Tensor, steps) -> torch.Tensor:
    """`maps` through the steps of `morph_steps(...)`, one launch per step.  One step returns a new tensor; a list ping-pongs two
    buffers of its own, so `maps` is never written.  No steps: `maps` itself."""
    bufs = []
    for op, size in steps:
        if len(bufs) < 2:
            bufs.append(morph_maps(maps, op, size))
        else:
            bufs.append(morph_maps(maps, op, size, out=bufs[-2]))
        maps = bufs[-1]
    return maps


# ====================================================================== rank filters of anomaly maps
# The sliding-window median and its generalisation, the r-th smallest value of a rectangular window: the
# denoiser of impulsive noise - single hot pixels on edges, gloss and sensor noise - that keeps step edges where they are and leaves
# the level of flat areas alone.  Erosion and dilation are its two end ranks.  scipy.ndimage.rank_filter / median_filter /
# percentile_filter with mode="reflect" to the bit on NaN-free maps; a NaN makes its windows NaN.
RANKFILT_MAX_SIZE = hip.RANKFILT_MAX_SIZE
RANKFILT_KINDS = ("median", "percentile", "rank")
RANKFILT_MAX_STEPS = 4


def _rankfilt_size(size, what: str) -> Tuple[int, int]:
    """An int or (size_h, size_w), each in 1..15 -> (size_h, size_w)."""
    if _is_int(size):
        size = (size, size)
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) for v in size):
        raise hip.VadError(f"{what}: size must be an int or (size_h, size_w), got {size!r}")
    sh, sw = int(size[0]), int(size[1])
    if not (1 <= sh <= RANKFILT_MAX_SIZE and 1 <= sw <= RANKFILT_MAX_SIZE):
        raise hip.VadError(f"{what}: size must be in 1..{RANKFILT_MAX_SIZE} per side, got {sh} x {sw}")
    return sh, sw


def _rankfilt_rank(rank, n: int, what: str) -> int:
    """A 0-based ascending rank of a window of n values."""
    if not _is_int(rank) or not 0 <= int(rank) < n:
        raise hip.VadError(f"{what}: rank must be an int in 0..{n - 1} (a window of {n} values), got {rank!r}")
    return int(rank)


def rank_of_percentile(n: int, p) -> int:
    """The 0-based ascending rank `scipy.ndimage.percentile_filter(x, p, ...)` selects from a window of n values: p += 100 if p < 0,
    then n - 1 for p == 100, else int(float(n) * p / 100.0).  -100 <= p <= 100."""
    what = "rank_of_percentile"
    if not _is_int(n) or int(n) < 1:
        raise hip.VadError(f"{what}: n must be an int >= 1, got {n!r}")
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not -100.0 <= float(p) <= 100.0:
        raise hip.VadError(f"{what}: p must be a number in -100..100, got {p!r}")
    p = float(p)
    if p < 0.0:
        p += 100.0
    return int(n) - 1 if p == 100.0 else int(float(int(n)) * p / 100.0)


def rank_filter_steps(spec) -> Tuple[Tuple[Tuple[int, int], int], ...]:
    """What the `rank_filter=` arguments of the scoring entry points take, normalised to a tuple of ((size_h, size_w), rank) steps:
    None -> (), one step or a list of at most four.  A step is `("median", size)` (rank n // 2: the upper median of an even
    window), `("percentile", size, p)` (`rank_of_percentile`) or `("rank", size, r)` (0-based, ascending); `size` an int or
    `(size_h, size_w)`, sides in 1..15.  `VadError` for anything else."""
    what = "rank_filter_steps"
    if spec is None:
        return ()
    if isinstance(spec, tuple) and len(spec) in (2, 3) and isinstance(spec[0], str):
        spec = [spec]
    if not isinstance(spec, list):
        raise hip.VadError(f"{what}: a spec is None, one step (kind, size[, p or rank]) or a list of steps, got {spec!r}")
    if not 1 <= len(spec) <= RANKFILT_MAX_STEPS:
        raise hip.VadError(f"{what}: a list holds 1..{RANKFILT_MAX_STEPS} steps, got {len(spec)}")
    steps = []
    for step in spec:
        if not isinstance(step, (tuple, list)) or len(step) not in (2, 3):
            raise hip.VadError(f"{what}: a step is ('median', size), ('percentile', size, p) or ('rank', size, r), got {step!r}")
        kind = step[0]
        if not isinstance(kind, str) or kind not in RANKFILT_KINDS:
            raise hip.VadError(f"{what}: kind must be one of {RANKFILT_KINDS}, got {kind!r}")
        if len(step) != (2 if kind == "median" else 3):
            raise hip.VadError(f"{what}: a step is ('median', size), ('percentile', size, p) or ('rank', size, r), got {step!r}")
        sh, sw = _rankfilt_size(step[1], what)
        n = sh * sw
        if kind == "median":
            rank = n // 2
        elif kind == "percentile":
            p = step[2]
            if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not -100.0 <= float(p) <= 100.0:
                raise hip.VadError(f"{what}: a percentile must be a number in -100..100, got {p!r}")
            rank = rank_of_percentile(n, p)
        else:
            rank = _rankfilt_rank(step[2], n, what)
        steps.append(((sh, sw), rank))
    return tuple(steps)


def rank_filter_maps(maps: torch.Tensor, size, rank="median", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`scipy.ndimage.rank_filter(x, rank, size=(size_h, size_w), mode="reflect")` of every H x W frame of `maps` on the GPU
    (`vad_rankfilt_maps`, csrc/map_rankfilt.hip): the `rank`-th smallest value (0-based) of the window around each pixel, even sizes
    leaning towards index 0, reflected pixels counted as often as they appear; `size` an int (a square) or (size_h, size_w), sides in
    1..15, larger than the frame allowed.  `rank` = "median" is n // 2 of the n = size_h * size_w values (`median_filter`; the upper
    median of an even n); `rank_of_percentile(n, p)` gives `percentile_filter`'s.  Rank 0 is `morph_maps(x, "erode", size)`; rank
    n - 1 is `"dilate"` at odd sizes only.  `maps` as `morph_maps` takes them: float32 GPU tensor, contiguous, the last two
    dimensions H, W and any leading ones; frames are processed one by one.  Nothing is computed, only selected, so the result is
    specified to the bit (tests/rank_filter_ref.py): one of the window's values, -0 ordered below +0; a NaN makes exactly the pixels
    whose window holds it NaN, at every rank.  Returns a new tensor, or `out` (same shape, float32, contiguous, not overlapping
    `maps`).  One launch, no workspace; asynchronous on the current stream."""
    what = "rank_filter_maps"
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    sh, sw = _rankfilt_size(size, what)
    if isinstance(rank, str):
        if rank != "median":
            raise hip.VadError(f"{what}: rank must be 'median' or an int in 0..{sh * sw - 1}, got {rank!r}")
        r = (sh * sw) // 2
    else:
        r = _rankfilt_rank(rank, sh * sw, what)
    if not maps.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the GPU (the rank filter runs on the device; there is no CPU fallback)")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if maps.dim() < 2:
        raise hip.VadError(f"{what}: maps must have at least the two dimensions H, W, got {tuple(maps.shape)}")
    if not maps.is_contiguous():
        raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
    lead, h, w = tuple(maps.shape[:-2]), int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(maps.shape) or out.dtype != torch.float32
                            or out.device != maps.device or not out.is_contiguous()):
        raise hip.VadError(f"{what}: out must be a contiguous float32 tensor {tuple(maps.shape)} on {maps.device}")
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    with torch.cuda.device(maps.device):
        if out is None:
            out = torch.empty_like(maps)
        if n > 0:
            hip.check(hip.lib().vad_rankfilt_maps(maps.data_ptr(), n, h, w, sh, sw, r, out.data_ptr(), hip.current_stream()), "vad_rankfilt_maps")
            _count("rank_filter_maps")
    return out


def apply_rank_filter(maps: torch.Tensor, steps) -> torch.Tensor:
    """`maps` through the steps of `rank_filter_steps(...)`, one launch per step.  One step returns a new tensor; a list ping-pongs
    two buffers of its own, so `maps` is never written.  No steps: `maps` itself."""
    bufs = []
    for size, rank in steps:
        if len(bufs) < 2:
            bufs.append(rank_filter_maps(maps, size, rank))
        else:
            bufs.append(rank_filter_maps(maps, size, rank, out=bufs[-2]))
        maps = bufs[-1]
    return maps


# ====================================================================== temporal filters of anomaly maps
# Every pixel filtered over the last k frames of its stream, between the calibration / morphology and the
# threshold: the minimum is a temporal erosion - "high in each of the last k frames", which removes noise that differs from frame
# to frame without any spatial blur -, the maximum holds a detection across a dropped frame, the mean and the exponential average
# lower the noise floor of a fixed camera.  Causal, windowed over the frames that exist; `vad_tfilt_maps`, csrc/map_temporal.hip.
TEMPORAL_MAX_K = hip.TFILT_MAX_K
TEMPORAL_OPS = tuple(hip.TFILT_OPS)
TEMPORAL_MAX_STEPS = 4


def _temporal_op(op, what: str) -> str:
    if not isinstance(op, str) or op not in hip.TFILT_OPS:
        raise hip.VadError(f"{what}: op must be one of {TEMPORAL_OPS}, got {op!r}")
    return op


def _temporal_param(op: str, v, what: str):
    """k in 1..16 for "min" / "max" / "mean" -> int; alpha for "ema" -> the float32 value the kernel multiplies with, 0 < alpha < 1."""
    if op == "ema":
        _check_number(v, "alpha", what, lambda a: 0.0 < float(np.float32(a)) < 1.0, "a number with 0 < float32(alpha) < 1")   # false for NaN
        return float(np.float32(v))
    return _check_int(v, "k", what, 1, TEMPORAL_MAX_K)


def temporal_steps(spec) -> Tuple[Tuple[str, object], ...]:
    """What the `temporal=` arguments of the scoring entry points and `TemporalFilter` take, normalised to a tuple of steps: None ->
    (), one step `("min", 3)` / `("max", k)` / `("mean", k)` (k in 1..16) / `("ema", alpha)` (0 < float32(alpha) < 1), or a list of at
    most four steps that run in order: `[("min", 3), ("max", 3)]` is a temporal opening.  `VadError` for anything else."""
    what = "temporal_steps"
    if spec is None:
        return ()
    if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], str):
        spec = [spec]
    if not isinstance(spec, list):
        raise hip.VadError(f"{what}: a spec is None, one step (op, k) / ('ema', alpha) or a list of steps, got {spec!r}")
    if not 1 <= len(spec) <= TEMPORAL_MAX_STEPS:
        raise hip.VadError(f"{what}: a list holds 1..{TEMPORAL_MAX_STEPS} steps, got {len(spec)}")
    steps = []
    for step in spec:
        if not isinstance(step, (tuple, list)) or len(step) != 2:
            raise hip.VadError(f"{what}: a step is (op, k) or ('ema', alpha), got {step!r}")
        op = _temporal_op(step[0], what)
        steps.append((op, _temporal_param(op, step[1], what)))
    return tuple(steps)


def _temporal_frames(maps, what: str) -> Tuple[int, int, int, int]:
    """maps [B,T,H,W] or [B,T,1,H,W], float32, on the GPU, contiguous -> (B, T, H, W)."""
    _check_maps(maps, what, "the filter runs on the device")
    if not (maps.dim() == 4 or (maps.dim() == 5 and maps.shape[2] == 1)):
        raise hip.VadError(f"{what}: maps must be [B,T,H,W] or [B,T,1,H,W] - T consecutive frames of B streams -, got {tuple(maps.shape)}")
    if not maps.is_contiguous():
        raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
    b, t, h, w = int(maps.shape[0]), int(maps.shape[1]), int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
    if b > 2 ** 20:
        raise hip.VadError(f"{what}: {b} streams are out of range (B <= 2^20)")
    return b, t, h, w


def _temporal_out(maps, out, what: str):
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(maps.shape) or out.dtype != torch.float32
                            or out.device != maps.device or not out.is_contiguous()):
        raise hip.VadError(f"{what}: out must be a contiguous float32 tensor {tuple(maps.shape)} on {maps.device}")
    return torch.empty_like(maps) if out is None else out


def _tfilt(maps, b, t, h, w, op: str, param, state_ptr, out) -> None:
    k, alpha = (0, param) if op == "ema" else (param, 0.0)
    if b > 0 and t > 0:
        hip.check(hip.lib().vad_tfilt_maps(maps.data_ptr(), b, t, h, w, hip.TFILT_OPS[op], k, alpha, state_ptr, out.data_ptr(), hip.current_stream()),
                  "vad_tfilt_maps")
        _count("tfilt_maps")


def temporal_maps(maps: torch.Tensor, op: str, k_or_alpha, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One temporal filter over the T frames of every clip of `maps` (`[B,T,H,W]` or `[B,T,1,H,W]`, float32 GPU tensor, contiguous),
    every clip a fresh stream (`vad_tfilt_maps` without a state, csrc/map_temporal.hip).  Per pixel, causal, over the frames that exist:
    `op` "min" / "max": `y[t]` = minimum / maximum of `x[max(0, t - k + 1) .. t]` - `scipy.ndimage.minimum_filter1d` /
    `maximum_filter1d(x, size=k, axis=1, mode="nearest", origin=(k - 1) // 2)` -, nothing rounded, NaN in exactly the k outputs whose
    window holds one, -0 below +0; they commute with a threshold.  "mean": the float64 sum of the window added oldest to newest,
    divided by the frames in it, rounded once.  "ema": `y[0] = x[0]`, `y[t] = y[t-1] + a * (x[t] - y[t-1])` in float32 without a fused
    multiply-add, `a = float32(alpha)`, so a finite constant stream stays constant to the bit; a NaN stays in the average to the end of
    the clip.  tests/map_temporal_ref.py restates all
    four to the bit.  k in 1..16 (1 is a copy), 0 < alpha < 1.  Returns a new tensor, or `out` (same shape, not overlapping
    `maps`).  One launch; asynchronous on the current stream."""
    what = "temporal_maps"
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    op = _temporal_op(op, what)
    param = _temporal_param(op, k_or_alpha, what)
    b, t, h, w = _temporal_frames(maps, what)
    with torch.cuda.device(maps.device):
        out = _temporal_out(maps, out, what)
        _tfilt(maps, b, t, h, w, op, param, None, out)
    return out


def apply_temporal(maps: torch.Tensor, steps) -> torch.Tensor:
    """`maps` (clips, as `temporal_maps` takes them) through the steps of `temporal_steps(...)`, one launch per step.  One step returns
    a new tensor; a list ping-pongs two buffers of its own, so `maps` is never written.  No steps: `maps` itself."""
    bufs = []
    for op, param in steps:
        if len(bufs) < 2:
            bufs.append(temporal_maps(maps, op, param))
        else:
            bufs.append(temporal_maps(maps, op, param, out=bufs[-2]))
        maps = bufs[-1]
    return maps


class TemporalFilter:
    """The temporal filters of `temporal_steps(steps)` over B live streams, carried across calls on the device (DESIGN.md section
    4.23): `update(maps)` takes the next T >= 0 maps of every stream and returns them filtered - the bits `apply_temporal` gives on the
    whole stream, for any split of its frames over calls.  One state blob per step (a ring of the k - 1 newest planes of its input;
    one plane for "ema") and one launch per step; the frame counters live in the blobs and are advanced by the kernel, so a captured
    `update` can be replayed.  An "ema" step keeps a NaN it has met until the stream is reset.  No CPU fallback."""

    def __init__(self, streams: int, h: int, w: int, steps, device=None):
        what = "TemporalFilter"
        self.steps = temporal_steps(steps)
        if not self.steps:
            raise hip.VadError(f"{what}: steps must hold at least one step, got {steps!r}")
        self.streams = _check_int(streams, "streams", what, 0, 2 ** 20)
        self.h, self.w = _check_int(h, "h", what, 1, hip.MAX_FRAME_PIXELS), _check_int(w, "w", what, 1, hip.MAX_FRAME_PIXELS)
        if self.h * self.w > hip.MAX_FRAME_PIXELS:
            raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (h * w <= {hip.MAX_FRAME_PIXELS})")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise hip.VadError(f"{what}: device ({dev}) must be a GPU (the filter runs on the device; there is no CPU fallback)")
        self.device = dev
        l = hip.lib()
        self.states = []
        for op, param in self.steps:
            size = l.vad_tfilt_state_bytes(self.streams, self.h, self.w, hip.TFILT_OPS[op], self._k(op, param))
            self.states.append(torch.empty(size // 4, dtype=torch.int32, device=dev))
        self.reset()

    @staticmethod
    def _k(op: str, param) -> int:
        return 0 if op == "ema" else param

    def _stream_words(self, i: int) -> int:
        return self.states[i].numel() // max(self.streams, 1)

    def reset(self, streams=None) -> None:
        """Fresh state (asynchronous): of every stream, or of the streams in `streams` (indices) - their next frame is frame 0."""
        l = hip.lib()
        which = [None] if streams is None else [int(s) for s in streams]
        for s in which:
            if s is not None and not 0 <= s < self.streams:
                raise hip.VadError(f"TemporalFilter.reset: stream {s} is out of range (0..{self.streams - 1})")
        if not self.streams:
            return
        with torch.cuda.device(self.device):
            for i, (op, param) in enumerate(self.steps):
                for s in which:
                    at, n = (0, self.streams) if s is None else (4 * s * self._stream_words(i), 1)
                    hip.check(l.vad_tfilt_init(self.states[i].data_ptr() + at, n, self.h, self.w, hip.TFILT_OPS[op], self._k(op, param),
                                               hip.current_stream()), "vad_tfilt_init")

    def frames_seen(self) -> torch.Tensor:
        """int64 [B] on the device: the frames every stream has taken in since its last reset (it stops at 2^32 - 1)."""
        if not self.streams:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        return self.states[0].view(self.streams, -1)[:, 0].to(torch.int64) & 0xFFFFFFFF

    def state_dict(self) -> dict:
        return {"steps": [list(s) for s in self.steps], "streams": self.streams, "h": self.h, "w": self.w,
                "states": [s.cpu().numpy().copy() for s in self.states]}

    def load_state_dict(self, state: dict) -> "TemporalFilter":
        what = "TemporalFilter.load_state_dict"
        got = (tuple(tuple(s) for s in state["steps"]), int(state["streams"]), int(state["h"]), int(state["w"]))
        if got != (self.steps, self.streams, self.h, self.w):
            raise hip.VadError(f"{what}: the state is of steps {got[0]} on {got[1]} streams of {got[2]} x {got[3]}, this filter of "
                               f"{self.steps} on {self.streams} streams of {self.h} x {self.w}")
        blobs = [np.asarray(b, dtype=np.int32) for b in state["states"]]
        if [b.shape for b in blobs] != [tuple(s.shape) for s in self.states]:
            raise hip.VadError(f"{what}: the state's blobs do not have the sizes of this filter's")
        for mine, b in zip(self.states, blobs):
            mine.copy_(torch.from_numpy(b))
        return self

    def update(self, maps: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """maps: float32 GPU tensor `[B,T,H,W]` or `[B,T,1,H,W]`, the next T frames of the B streams -> the filtered maps, same shape.
        The library call allocates nothing; this method makes one output tensor per step for the first two steps of a list
        (`torch.empty_like`: the caching allocator, or the graph's pool under capture).  Pass `out` (same shape, float32,
        contiguous, not overlapping `maps`) to receive the last step's result in a tensor of one's own - a one-step filter then
        allocates nothing."""
        what = "TemporalFilter.update"
        b, t, h, w = _temporal_frames(maps, what)
        if out is not None:
            _temporal_out(maps, out, what)
        if (b, h, w) != (self.streams, self.h, self.w):
            raise hip.VadError(f"{what}: maps {tuple(maps.shape)} do not match the filter's state: {self.streams} streams of {self.h} x {self.w}")
        if maps.device != self.states[0].device:
            raise hip.VadError(f"{what}: maps ({maps.device}) and the filter's state ({self.states[0].device}) are on different devices")
        with torch.cuda.device(maps.device):
            bufs = []
            for i, (op, param) in enumerate(self.steps):
                step_out = out if out is not None and i == len(self.steps) - 1 else torch.empty_like(maps) if len(bufs) < 2 else bufs[-2]
                _tfilt(maps, b, t, h, w, op, param, self.states[i].data_ptr(), step_out)
                bufs.append(step_out)
                maps = step_out
        return maps


# ====================================================================== robust frame scores: top-k means and quantiles of maps
# The reduction from a map to a frame score.  The reference's score is the mean of the error map, which a
# 20 x 20 scratch on a 256 x 256 frame barely moves; the maximum (`smooth_maps(return_max=)`) is one pixel.  Between the two sit
# the mean of the k largest pixels (top-k pooling, k = 0.1 % .. 10 % of the frame) and a high quantile of the map: a radix select
# on the device (`vad_map_topk`, csrc/map_topk.hip), no sort, no `torch.topk` / `torch.quantile` over `[N, H * W]`.
TOPK_MAX_RANKS = hip.TOPK_MAX_RANKS
REDUCE_KINDS = ("topk", "quantile", "rank")


def _check_pixels(pixels, what: str) -> int:
    return _check_int(pixels, "pixels", what, 1, hip.MAX_FRAME_PIXELS)


def rank_of_fraction(fraction, pixels: int) -> int:
    """The rank k of "the top `fraction` of a frame of `pixels` pixels": min(P, max(1, ceil(fraction * P))), in exact rational
    arithmetic on the Python float as given - 0.01 of 65,536 pixels is 656 (the double nearest 0.01 lies above it).  `fraction` in
    (0, 1]; `VadError` for anything else."""
    from fractions import Fraction
    what = "rank_of_fraction"
    p = _check_pixels(pixels, what)
    _check_number(fraction, "fraction", what, lambda v: 0.0 < float(v) <= 1.0, "a number in (0, 1]")   # false for NaN
    k = Fraction(float(fraction)) * p
    return min(p, max(1, -((-k.numerator) // k.denominator)))


def rank_of_quantile(q, pixels: int) -> int:
    """The rank k at which `kth` is `np.quantile(frame, q, method="higher")`: P - ceil(q * (P - 1)), the product in float64 as numpy
    forms it.  `q` in [0, 1] (1 = the maximum, rank 1; 0 = the minimum, rank P); `VadError` for anything else."""
    import math
    what = "rank_of_quantile"
    p = _check_pixels(pixels, what)
    q = _check_fraction(q, "q", what)
    return p - int(math.ceil(float(np.float64(q) * np.float64(p - 1))))


def _check_ranks(ranks, pixels: int, what: str) -> Tuple[list, bool]:
    """An int or a sequence of 1 .. 8 ints, each in 1 .. pixels -> (list, was it a single int)."""
    single = _is_int(ranks)
    if single:
        ranks = [ranks]
    if not isinstance(ranks, (list, tuple)) or not 1 <= len(ranks) <= TOPK_MAX_RANKS or not all(_is_int(k) for k in ranks):
        raise hip.VadError(f"{what}: ranks must be an int or a sequence of 1..{TOPK_MAX_RANKS} ints, got {ranks!r}")
    for k in ranks:
        if not 1 <= int(k) <= pixels:
            raise hip.VadError(f"{what}: a rank must be in 1..{pixels} (H * W; rank k = the k-th largest pixel), got {k!r}")
    return [int(k) for k in ranks], single


def map_topk(maps: torch.Tensor, ranks, kth: bool = True, mean: bool = True) -> dict:
    """Order statistics and top-k means of every H x W frame of `maps` on the GPU (`vad_map_topk`, csrc/map_topk.hip).  `maps` as
    `smooth_maps` takes them: float32 GPU tensor, contiguous, the last two dimensions H, W and any leading ones (`[B,1,H,W]`, the
    `[B,T,1,H,W]` maps of the video model, `[N,H,W]`); every frame on its own.  `ranks`: an int or a sequence of 1 .. 8 ints, each in
    1 .. H * W; rank k is the k-th largest pixel; any order, duplicates allowed (`rank_of_fraction`, `rank_of_quantile` make them).
    Returns a dict with 'kth' (if `kth`) and 'mean' (if `mean`), each float32 `[..., nk]` - `[...]` for an int - on the device:
      kth   the k-th largest pixel in the order -inf < ... < -0.0 < +0.0 < ... < +inf, its bits unchanged;
      mean  the mean of the k largest pixels, summed in float64 and rounded once to float32: within half a float32 spacing plus
            P * 2^-52 * mean(|top k|) of the exact mean (tests/map_topk_ref.py).
    A frame with a NaN pixel is NaN in both (`torch.amax`'s rule).  A frame's results do not depend on the batch around it.  One
    launch (frames above `vad_topk_plan`'s 262,144 pixels: split over work-groups, six launches), no sort, no host synchronisation;
    the ranks travel with the launches.  Asynchronous on the current stream."""
    what = "map_topk"
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    if not (isinstance(kth, bool) and isinstance(mean, bool)) or not (kth or mean):
        raise hip.VadError(f"{what}: kth and mean must be bools, at least one of them True, got {kth!r} and {mean!r}")
    if not maps.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) must be on the GPU (the selection runs on the device; there is no CPU fallback)")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if maps.dim() < 2:
        raise hip.VadError(f"{what}: maps must have at least the two dimensions H, W, got {tuple(maps.shape)}")
    if not maps.is_contiguous():
        raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
    lead, h, w = tuple(maps.shape[:-2]), int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
    ranks, single = _check_ranks(ranks, h * w, what)
    nk = len(ranks)
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    shape = lead if single else lead + (nk,)
    with torch.cuda.device(maps.device):
        out = {name: torch.empty(shape, dtype=torch.float32, device=maps.device) for name, on in (("kth", kth), ("mean", mean)) if on}
        if n > 0:
            l = hip.lib()
            ws = _workspace(l.vad_topk_workspace_bytes(n, h, w, nk), maps.device, what, f"{n} maps of {h} x {w} with {nk} ranks are out of range")
            hip.check(l.vad_map_topk(maps.data_ptr(), n, h, w, (hip.C.c_uint * nk)(*ranks), nk, hip.ptr(out.get("kth")), hip.ptr(out.get("mean")),
                                     ws.data_ptr(), ws.numel(), hip.current_stream()), "vad_map_topk")
            _count("map_topk")
    return out


def reduce_spec(reduce, what: str) -> Tuple[str, object]:
    """What the `reduce=` arguments of the scoring entry points take, checked and normalised to (kind, argument): "max" -> ("rank",
    1); ("topk", fraction in (0, 1]); ("quantile", q in [0, 1]); ("rank", k >= 1).  `VadError`, naming the spec, for anything else -
    "mean" among them: the scoring tails already produce the mean with their own arithmetic."""
    if reduce == "max":
        return "rank", 1
    if not isinstance(reduce, (tuple, list)) or len(reduce) != 2 or reduce[0] not in REDUCE_KINDS:
        raise hip.VadError(f"{what}: reduce must be 'max', ('topk', fraction), ('quantile', q) or ('rank', k), got {reduce!r}")
    kind, arg = reduce
    if kind == "topk":
        _check_number(arg, "the fraction of reduce=('topk', fraction)", what, lambda v: 0.0 < float(v) <= 1.0, "a number in (0, 1]")
    elif kind == "quantile":
        _check_fraction(arg, "the q of reduce=('quantile', q)", what)
    else:
        arg = _check_int(arg, "the k of reduce=('rank', k)", what, 1, hip.MAX_FRAME_PIXELS)
    return kind, arg


def reduce_maps(maps: torch.Tensor, reduce) -> torch.Tensor:
    """The one place that turns maps `[..., H, W]` into frame scores `[...]`, on the device, with ONE `map_topk` call: `reduce` =
    "max" (rank 1), ("topk", fraction) - the mean of the `rank_of_fraction(fraction, H * W)` largest pixels -, ("quantile", q) - the
    pixel at `rank_of_quantile(q, H * W)`, numpy's `quantile(method="higher")` -, or ("rank", k) - the k-th largest pixel."""
    what = "reduce_maps"
    kind, arg = reduce_spec(reduce, what)
    if not isinstance(maps, torch.Tensor) or maps.dim() < 2:
        raise hip.VadError(f"{what}: maps must be a torch tensor with at least the two dimensions H, W")
    pixels = int(maps.shape[-2]) * int(maps.shape[-1])
    if kind == "topk":
        return map_topk(maps, rank_of_fraction(arg, pixels), kth=False)["mean"]
    rank = rank_of_quantile(arg, pixels) if kind == "quantile" else arg
    return map_topk(maps, rank, mean=False)["kth"]


# ====================================================================== defect regions of an anomaly map
# What a deployed line needs after the thresholds above: which connected regions of a frame's map are at or
# above the operating threshold, where they are, how large and how strong - as a compact table per frame, not as a picture.  The
# host route is a copy of every map (256 KB per 256 x 256 frame) and scipy.ndimage label / find_objects / maximum_position /
# center_of_mass per frame; here the maps stay on the device and the table is what a renderer, an alarm or a logger reads.
REGION_WORDS = hip.REGION_WORDS
MAX_REGIONS = hip.MAX_REGIONS


class Regions:
    """The table `detect_regions` returns, as device tensors with the leading shape of the maps (`[B]`, or `[B,T]` for clips):

      records  int32 [..., R, 12]: the words of `vad_detect_regions` (include/vad_hip.h), R = max_regions; the kept regions of a
               frame in raster order of their first pixel, all-zero records behind them
      counts   int32 [..., 4]: kept regions (the full number: above R the table is truncated), regions dropped for their area,
               foreground pixels, NaN pixels (a NaN is never foreground; it does not vanish silently)
      labels   int32 [..., H, W] or None: 0, or 1 + root, for ALL foreground regions (with `return_labels=True`)

    Views of `records` (no copies): `root`, `area`, `peak_index` int32 [..., R]; `box` int32 [..., R, 4] = x0, y0, x1, y1 inclusive;
    `peak` float32 [..., R]; `sum_x`, `sum_y` int64 [..., R]."""

    def __init__(self, records: torch.Tensor, counts: torch.Tensor, labels: Optional[torch.Tensor], frame_shape: Tuple[int, int],
                 threshold: float, connectivity: int, min_area: int):
        self.records, self.counts, self.labels = records, counts, labels
        self.frame_shape, self.threshold, self.connectivity, self.min_area = frame_shape, threshold, connectivity, min_area
        self.max_regions = int(records.shape[-2])

    root = property(lambda self: self.records[..., 0])
    area = property(lambda self: self.records[..., 1])
    box = property(lambda self: self.records[..., 2:6])
    peak = property(lambda self: self.records[..., 6].view(torch.float32))
    peak_index = property(lambda self: self.records[..., 7])
    sum_x = property(lambda self: self.records[..., 8:10].view(torch.int64)[..., 0])
    sum_y = property(lambda self: self.records[..., 10:12].view(torch.int64)[..., 0])

    def centroids(self) -> torch.Tensor:
        """float64 [..., R, 2] on the device: (y, x) = (sum_y / area, sum_x / area), each quotient rounded once; NaN for the
        all-zero records behind a frame's last region."""
        area = self.area.to(torch.float64)
        return torch.stack([self.sum_y.to(torch.float64) / area, self.sum_x.to(torch.float64) / area], dim=-1)

    def truncated(self) -> torch.Tensor:
        """bool [...]: the frame has more kept regions than the table has records."""
        return self.counts[..., 0] > self.max_regions

    def to_list(self) -> list:
        """A host copy of the table - 48 bytes per record, never a map -: one list per frame (frames in row-major order of the
        leading shape) of {'root', 'area', 'box': (x0, y0, x1, y1), 'peak', 'peak_yx', 'centroid_yx'} in table order."""
        w = self.frame_shape[1]
        rec = self.records.reshape(-1, self.max_regions, REGION_WORDS).cpu().numpy()
        kept = self.counts.reshape(-1, 4)[:, 0].cpu().numpy()
        out = []
        for f in range(rec.shape[0]):
            rows = []
            for r in rec[f, :min(int(kept[f]), self.max_regions)]:
                area = int(r[1])
                sx, sy = (int(v) for v in r[8:12].copy().view(np.int64))
                rows.append({"root": int(r[0]), "area": area, "box": tuple(int(v) for v in r[2:6]), "peak": float(r[6:7].copy().view(np.float32)[0]),
                             "peak_yx": divmod(int(r[7]), w), "centroid_yx": (sy / area, sx / area)})
            out.append(rows)
        return out


def _region_frames(maps: torch.Tensor, what: str):
    """-> (contiguous [N,H,W] view / copy, leading shape) of maps [B,H,W], [B,1,H,W] or [B,T,1,H,W]."""
    if maps.dim() == 3:
        lead = (maps.shape[0],)
    elif maps.dim() == 4 and maps.shape[1] == 1:
        lead = (maps.shape[0],)
    elif maps.dim() == 5 and maps.shape[2] == 1:
        lead = (maps.shape[0], maps.shape[1])
    else:
        raise hip.VadError(f"{what}: maps must be [B,H,W], [B,1,H,W] or [B,T,1,H,W], got {tuple(maps.shape)}")
    h, w = int(maps.shape[-2]), int(maps.shape[-1])
    if h < 1 or w < 1:
        raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (H, W >= 1)")
    return maps.reshape(-1, h, w).contiguous(), tuple(int(v) for v in lead)


def detect_regions(maps: torch.Tensor, threshold: float, connectivity: int = 8, min_area: int = 1, max_regions: int = 64,
                   return_labels: bool = False) -> Regions:
    """The connected regions of `maps >= threshold` of every frame, on the GPU (`vad_detect_regions`, csrc/map_regions.hip).
    `maps`: float32 GPU tensor `[B,H,W]`, `[B,1,H,W]` (error / SSIM / smoothed maps) or `[B,T,1,H,W]` (the video model's maps); every
    frame is labelled on its own, never across time.  `threshold`: a float32 value (NaN is refused) - the predicate is the one of
    `roc_curve_from_counts`, so `threshold_at_fpr` / `best_f1_threshold` results apply as they stand.  Regions are those of
    `label_regions` (connectivity 8 or 4); the ones with at least `min_area` pixels are kept, in raster order of their first pixel
    (scipy.ndimage.label's numbering), the first `max_regions` (1..65536) written.  Returns a `Regions`; like `label_regions` it
    reads the kernels' flag word (one 4-byte copy, which waits for the call) and raises VadError if it is set.  No CPU fallback."""
    what = "detect_regions"
    connectivity = _check_connectivity(connectivity, what)
    _check_maps(maps, what, "regions are detected on the device")
    threshold = _check_threshold(threshold, what)
    min_area = _check_int(min_area, "min_area", what, 1, 2 ** 32 - 1)
    max_regions = _check_int(max_regions, "max_regions", what, 1, MAX_REGIONS)
    frames, lead = _region_frames(maps, what)
    n, h, w = frames.shape
    if n == 0:                                                            # nothing to detect, nothing to launch
        return Regions(torch.zeros((*lead, max_regions, REGION_WORDS), dtype=torch.int32, device=frames.device),
                       torch.zeros((*lead, 4), dtype=torch.int32, device=frames.device),
                       torch.zeros((*lead, h, w), dtype=torch.int32, device=frames.device) if return_labels else None, (h, w),
                       threshold, connectivity, min_area)
    with torch.cuda.device(frames.device):
        l = hip.lib()
        ws = _workspace(l.vad_regions_workspace_bytes(n, h, w, 1 if return_labels else 0), frames.device, what,
                        f"{n} frames of {h} x {w} are out of range (h * w < 2^31 - 1, n * h * w <= 2^38)")
        records = torch.empty((n, max_regions, REGION_WORDS), dtype=torch.int32, device=frames.device)
        counts = torch.empty((n, 4), dtype=torch.int32, device=frames.device)
        labels = torch.empty((n, h, w), dtype=torch.int32, device=frames.device) if return_labels else None
        hip.check(l.vad_detect_regions(frames.data_ptr(), n, h, w, threshold, connectivity, min_area, max_regions,
                                       hip.ptr(labels), records.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                       hip.current_stream()), "vad_detect_regions")
    _launched(ws, what)
    return Regions(records.view(*lead, max_regions, REGION_WORDS), counts.view(*lead, 4),
                   labels.view(*lead, h, w) if return_labels else None, (h, w), threshold, connectivity, min_area)


# ====================================================================== detections against ground-truth masks
# The link between the operating point and the ranking metrics: with a threshold, a min_area, a morph list
# and a calibration chosen, how many of the labelled defects are found, how many false alarms are raised per frame, which pixel IoU
# is reached.  AUROC and AUPRO rank pixels over all thresholds and know nothing of min_area or of regions as units; the host route
# copies every map and mask and runs scipy.ndimage label / sum_labels of one labelling under the other.
MATCH_WORDS = hip.MATCH_WORDS
MATCH_COUNTS = hip.MATCH_COUNTS
COUNT_NAMES = ("gt_regions", "gt_detected", "pred_regions", "pred_matched", "false_alarms", "pred_dropped", "pixel_tp", "pixel_fp",
               "pixel_fn", "pixel_tn", "nan_pixels", "gt_pixels", "frames_gt_pred", "frames_pred_only", "frames_gt_only", "frames_neither")


class Matches:
    """What `match_regions` returns, as device tensors with the leading shape of the maps (`[B]`, or `[B,T]` for clips):

      gt_records    int32 [..., R, 4]: the mask's regions of a frame - root, area, hit = pixels shared with kept predictions, flags
                    (bit 0: detected) - in raster order of their first pixel, R = max_regions, all-zero records behind them
      pred_records  int32 [..., R, 4]: the kept predicted regions - root, area, overlap = pixels shared with the mask, flags (bit 0:
                    matched; a kept prediction that is not matched is a false alarm) - in the same order
      counts        int64 [..., 16]: the words of `vad_match_regions` (include/vad_hip.h), named by `COUNT_NAMES`; the region
                    counters are the full numbers, so a truncated table is visible

    Views of the records (no copies): `gt_area`, `gt_hit`, `pred_area`, `pred_overlap` int32 [..., R]; `gt_detected`, `pred_matched`
    bool [..., R]."""

    def __init__(self, gt_records: torch.Tensor, pred_records: torch.Tensor, counts: torch.Tensor, frame_shape: Tuple[int, int], params: dict):
        self.gt_records, self.pred_records, self.counts = gt_records, pred_records, counts
        self.frame_shape, self.params = frame_shape, dict(params)
        self.max_regions = int(gt_records.shape[-2])

    gt_area = property(lambda self: self.gt_records[..., 1])
    gt_hit = property(lambda self: self.gt_records[..., 2])
    gt_detected = property(lambda self: (self.gt_records[..., 3] & 1) != 0)
    pred_area = property(lambda self: self.pred_records[..., 1])
    pred_overlap = property(lambda self: self.pred_records[..., 2])
    pred_matched = property(lambda self: (self.pred_records[..., 3] & 1) != 0)

    def truncated(self) -> torch.Tensor:
        """bool [...]: the frame has more mask regions or more kept predictions than a table has records."""
        return (self.counts[..., 0] > self.max_regions) | (self.counts[..., 2] > self.max_regions)

    def to_list(self) -> list:
        """A host copy of the tables - 16 bytes per record, never a map -: one dict per frame (frames in row-major order of the
        leading shape) {'gt': [{'root', 'area', 'hit', 'detected'}], 'pred': [{'root', 'area', 'overlap', 'matched'}], 'counts':
        {name: int}} in table order."""
        gt = self.gt_records.reshape(-1, self.max_regions, MATCH_WORDS).cpu().numpy()
        pred = self.pred_records.reshape(-1, self.max_regions, MATCH_WORDS).cpu().numpy()
        counts = self.counts.reshape(-1, MATCH_COUNTS).cpu().numpy()
        out = []
        for f in range(counts.shape[0]):
            out.append({"gt": [{"root": int(r[0]), "area": int(r[1]), "hit": int(r[2]), "detected": bool(r[3] & 1)}
                               for r in gt[f, :min(int(counts[f, 0]), self.max_regions)]],
                        "pred": [{"root": int(r[0]), "area": int(r[1]), "overlap": int(r[2]), "matched": bool(r[3] & 1)}
                                 for r in pred[f, :min(int(counts[f, 2]), self.max_regions)]],
                        "counts": {name: int(v) for name, v in zip(COUNT_NAMES, counts[f])}})
        return out


def _match_params(what: str, threshold, connectivity, min_area, gt_fraction, pred_fraction) -> dict:
    """The checked operating point of `match_regions` / `DetectionCounts`: what two sets of counters must share to be added."""
    connectivity = _check_connectivity(connectivity, what)
    return {"threshold": _check_threshold(threshold, what), "connectivity": connectivity,
            "min_area": _check_int(min_area, "min_area", what, 1, 2 ** 32 - 1),
            "gt_fraction": _check_fraction(gt_fraction, "gt_fraction", what), "pred_fraction": _check_fraction(pred_fraction, "pred_fraction", what)}


def match_regions(maps: torch.Tensor, masks: torch.Tensor, threshold: float, connectivity: int = 8, min_area: int = 1,
                  gt_fraction: float = 0.0, pred_fraction: float = 0.0, max_regions: int = 64) -> Matches:
    """The detections of `maps >= threshold` held against the ground-truth `masks`, on the GPU (`vad_match_regions`,
    csrc/map_match.hip).  `maps`: float32 GPU tensor `[B,H,W]`, `[B,1,H,W]` or `[B,T,1,H,W]` as in `detect_regions`; `masks`: a GPU
    tensor of a matching shape in the formats of `label_regions` (float: anomalous iff > 0.5; uint8: iff >= 128; bool and other
    integers: iff non-zero).  The predicted regions are those of `detect_regions` with the same `threshold`, `connectivity` and
    `min_area`; a region dropped for its area counts as background.  A mask region is DETECTED iff it shares at least one pixel, and
    at least `gt_fraction` of its area, with the kept predictions; a kept prediction is MATCHED iff it shares at least one pixel, and
    at least `pred_fraction` of its area, with the mask - otherwise it is a false alarm.  Both fractions lie in [0, 1]; 0 = any
    shared pixel.  Touching, diagonally too, is no overlap.  Returns a `Matches`; like `detect_regions` it reads the kernels' flag
    word (one 4-byte copy, which waits for the call) and raises VadError if it is set.  No CPU fallback."""
    what = "match_regions"
    params = _match_params(what, threshold, connectivity, min_area, gt_fraction, pred_fraction)
    # maps and masks are refused together, in words of their own, and the device comes after the shapes: of `_check_maps` only the
    # float32 line has a counterpart here, and it is written out
    if not isinstance(maps, torch.Tensor) or not isinstance(masks, torch.Tensor):
        raise hip.VadError(f"{what}: maps and masks must be torch tensors")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if masks.is_complex():
        raise hip.VadError(f"{what}: masks must be float, uint8, bool or integer, got {masks.dtype}")
    max_regions = _check_int(max_regions, "max_regions", what, 1, MAX_REGIONS)
    if maps.dim() not in (3, 4, 5) or masks.dim() not in (3, 4, 5) or masks.numel() != maps.numel() or masks.shape[-2:] != maps.shape[-2:] \
            or masks.shape[0] != maps.shape[0]:
        raise hip.VadError(f"{what}: masks {tuple(masks.shape)} do not match maps {tuple(maps.shape)}")
    if not maps.is_cuda or not masks.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) and masks ({masks.device}) must be on the GPU (regions are matched on the "
                           "device; there is no CPU fallback)")
    if maps.device != masks.device:
        raise hip.VadError(f"{what}: maps ({maps.device}) and masks ({masks.device}) must be on the same device")
    frames, lead = _region_frames(maps, what)
    n, h, w = frames.shape
    m, fmt, _, _, _ = _mask_planes(masks.reshape(-1, h, w), what)
    dev = frames.device
    if n == 0:                                                            # nothing to match, nothing to launch
        return Matches(torch.zeros((*lead, max_regions, MATCH_WORDS), dtype=torch.int32, device=dev),
                       torch.zeros((*lead, max_regions, MATCH_WORDS), dtype=torch.int32, device=dev),
                       torch.zeros((*lead, MATCH_COUNTS), dtype=torch.int64, device=dev), (h, w), params)
    with torch.cuda.device(dev):
        l = hip.lib()
        ws = _workspace(l.vad_match_workspace_bytes(n, h, w), dev, what,
                        f"{n} frames of {h} x {w} are out of range (h * w < 2^31 - 1, n * h * w <= 2^38)")
        gt_records = torch.empty((n, max_regions, MATCH_WORDS), dtype=torch.int32, device=dev)
        pred_records = torch.empty((n, max_regions, MATCH_WORDS), dtype=torch.int32, device=dev)
        counts = torch.empty((n, MATCH_COUNTS), dtype=torch.int64, device=dev)
        hip.check(l.vad_match_regions(frames.data_ptr(), m.data_ptr(), fmt, n, h, w, params["threshold"], params["connectivity"],
                                      params["min_area"], params["gt_fraction"], params["pred_fraction"], max_regions,
                                      gt_records.data_ptr(), pred_records.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                      hip.current_stream()), "vad_match_regions")
    _launched(ws, what)
    return Matches(gt_records.view(*lead, max_regions, MATCH_WORDS), pred_records.view(*lead, max_regions, MATCH_WORDS),
                   counts.view(*lead, MATCH_COUNTS), (h, w), params)


def _ratio(num: int, den: int) -> float:
    """num / den in float64; nan - never 0 or 1 - when there is nothing to divide by."""
    return float(num) / float(den) if den else float("nan")


def report_from_counts(counts) -> dict:
    """The operating-point report from the 16 sums of `vad_match_regions`' counters (`COUNT_NAMES`), on the host - usable on a
    machine without a GPU.  Region level: recall = detected / mask regions, precision = matched / kept predictions, F1 their
    harmonic mean, false alarms per frame.  Pixel level: precision, recall, IoU = TP / (TP + FP + FN), Dice.  Image level (a frame is
    positive with a mask region, alarmed with a kept prediction): precision, recall, F1.  A ratio whose denominator is 0 is nan."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != MATCH_COUNTS or min(c) < 0:
        raise hip.VadError(f"report_from_counts: counts must be {MATCH_COUNTS} non-negative integers, got {counts!r}")
    gt, det, pred, matched, fa, _, tp, fp, fn, _, _, _, both, pred_only, gt_only, neither = c
    frames = both + pred_only + gt_only + neither
    recall, precision = _ratio(det, gt), _ratio(matched, pred)
    out = {name: v for name, v in zip(COUNT_NAMES, c)}
    out.update({"frames": frames, "region_recall": recall, "region_precision": precision,
                "region_f1": 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else float("nan"),
                "false_alarms_per_frame": _ratio(fa, frames),
                "pixel_precision": _ratio(tp, tp + fp), "pixel_recall": _ratio(tp, tp + fn), "pixel_iou": _ratio(tp, tp + fp + fn),
                "pixel_dice": _ratio(2 * tp, 2 * tp + fp + fn),
                "image_precision": _ratio(both, both + pred_only), "image_recall": _ratio(both, both + gt_only),
                "image_f1": _ratio(2 * both, 2 * both + pred_only + gt_only)})
    return out


class DetectionCounts:
    """The 16 counters of `match_regions` summed over frames: an int64 `[16]` device tensor (`COUNT_NAMES`) and the operating point
    they were gathered at - `params` = {threshold, connectivity, min_area, gt_fraction, pred_fraction} plus whatever `meta` the
    caller adds (`scoring.detection_report`: map, sigma, truncate, morph, calibrated).  Counters gathered at another operating point
    are refused with `ValueError`, as a calibration gathered on other maps is: their sum would describe no setting at all.  Integer
    sums: the result does not depend on batching or sharding, and ranks combine with ONE all-reduce."""

    def __init__(self, device="cuda", params: Optional[dict] = None):
        self.counts = torch.zeros(MATCH_COUNTS, dtype=torch.int64, device=device)
        self.params = dict(params) if params else None

    def _adopt(self, params, what: str) -> None:
        if params is None:
            return
        if self.params is None:
            self.params = dict(params)
        elif self.params != dict(params):
            raise ValueError(f"{what}: these counters were gathered with {self.params}, the others with {dict(params)}")

    def update(self, matches: Matches, meta: Optional[dict] = None) -> "DetectionCounts":
        """Add the frames of one `match_regions` result (one reduction on the device; nothing is read by the host)."""
        if not isinstance(matches, Matches):
            raise hip.VadError(f"DetectionCounts.update: matches must be a metrics.Matches, got {type(matches).__name__}")
        if matches.counts.device != self.counts.device:
            raise hip.VadError(f"DetectionCounts.update: the matches are on {matches.counts.device}, the counters on {self.counts.device}")
        self._adopt({**matches.params, **(meta or {})}, "DetectionCounts.update")
        self.counts += matches.counts.reshape(-1, MATCH_COUNTS).sum(dim=0)
        return self

    def merge(self, other: "DetectionCounts") -> "DetectionCounts":
        """self += other (two streams, two halves of a dataset, or the states of several ranks after a gather)."""
        if not isinstance(other, DetectionCounts):
            raise hip.VadError(f"DetectionCounts.merge: other must be a DetectionCounts, got {type(other).__name__}")
        self._adopt(other.params, "DetectionCounts.merge")
        self.counts += other.counts.to(self.counts.device)
        return self

    def all_reduce(self, group=None, force_collective: bool = False) -> int:
        """Sum the counters over the ranks of `group` (`allreduce_counters_`: one all_reduce).  Every rank must hold counters of the
        same operating point: this call does NOT check it - the collective carries the 16 words only, and `params` stay this
        rank's -, so ranks compare their `params` themselves (e.g. `all_gather_object`) where they may differ.  Returns the world
        size."""
        return allreduce_counters_(self.counts, group, force_collective)

    def state_dict(self) -> dict:
        return {"counts": self.counts.cpu().clone(), "params": None if self.params is None else dict(self.params)}

    def load_state_dict(self, state: dict) -> "DetectionCounts":
        """Replace the counters by a saved state.  An object that already has an operating point takes only a state of the same
        one (`ValueError` otherwise, nothing changed), like `merge` and `update`; a fresh one adopts the state's."""
        counts = torch.as_tensor(state["counts"])
        if counts.dtype != torch.int64 or tuple(counts.shape) != (MATCH_COUNTS,) or bool((counts < 0).any()):
            raise hip.VadError(f"DetectionCounts.load_state_dict: counts must be {MATCH_COUNTS} non-negative int64 words, got "
                               f"{counts.dtype} {tuple(counts.shape)}")
        self._adopt(state.get("params"), "DetectionCounts.load_state_dict")
        self.counts.copy_(counts)
        return self

    def report(self) -> dict:
        """`report_from_counts` of the sums (one 128-byte copy to the host) with the operating point under 'params'."""
        out = report_from_counts(self.counts.cpu().numpy())
        out["params"] = None if self.params is None else dict(self.params)
        return out


# ====================================================================== anomaly events of a clip
# Nobody alarms on a single-frame blob: regions that overlap from frame to frame are one event, and a line
# alarms on the events that last.  An event is a connected component of `map >= threshold` in the volume [T,H,W] of one clip; the
# host route is a copy of every map of the clip and scipy.ndimage.label with a 3-D structure, find_objects and maximum_position.
EVENT_WORDS = hip.EVENT_WORDS
MAX_EVENTS = hip.MAX_EVENTS


class Events:
    """The table `detect_events` returns, as device tensors with the leading shape of the clips (`[B]`, or `()` for one clip):

      records       int32 [..., E, 16]: the words of `vad_detect_events` (include/vad_hip.h), E = max_events; the kept events of a
                    clip in ascending order of their first voxel, all-zero records behind them
      counts        int32 [..., 4]: kept events (the full number: above E the table is truncated), events dropped by a filter,
                    foreground pixels, NaN pixels
      frame_counts  int32 [..., T, 3]: foreground pixels of the frame, pixels of the frame that belong to kept events (whether or
                    not the event has a record: independent of max_events), NaN pixels of the frame
      labels        int32 [..., T, H, W] or None: 0, or 1 + root, for ALL foreground pixels (with `return_labels=True`)
      tracks        None, or the `EventTracks` that `scoring.localize_events(tracks=True)` attached: a box per event and frame

    Views of `records` (no copies): `root`, `volume`, `t0`, `t1`, `peak_index` int32 [..., E]; `box` int32 [..., E, 4] = x0, y0, x1,
    y1 inclusive, the union over the event's frames; `peak` float32 [..., E]; `sum_x`, `sum_y`, `sum_t` int64 [..., E].  A root or a
    peak index is a volume index t * H * W + y * W + x."""

    def __init__(self, records: torch.Tensor, counts: torch.Tensor, frame_counts: torch.Tensor, labels: Optional[torch.Tensor],
                 volume_shape: Tuple[int, int, int], threshold: float, connectivity: int, temporal: int, min_duration: int, min_volume: int):
        self.records, self.counts, self.frame_counts, self.labels = records, counts, frame_counts, labels
        self.volume_shape, self.threshold, self.connectivity, self.temporal = volume_shape, threshold, connectivity, temporal
        self.min_duration, self.min_volume = min_duration, min_volume
        self.max_events = int(records.shape[-2])
        self.tracks = None                                                    # an `EventTracks`, where a caller attached one

    root = property(lambda self: self.records[..., 0])
    volume = property(lambda self: self.records[..., 1])
    t0 = property(lambda self: self.records[..., 2])
    t1 = property(lambda self: self.records[..., 3])
    box = property(lambda self: self.records[..., 4:8])
    peak = property(lambda self: self.records[..., 8].view(torch.float32))
    peak_index = property(lambda self: self.records[..., 9])
    sum_x = property(lambda self: self.records[..., 10:12].view(torch.int64)[..., 0])
    sum_y = property(lambda self: self.records[..., 12:14].view(torch.int64)[..., 0])
    sum_t = property(lambda self: self.records[..., 14:16].view(torch.int64)[..., 0])

    def durations(self) -> torch.Tensor:
        """int32 [..., E]: t1 - t0 + 1 of the records in use, 0 for the all-zero records behind them."""
        return torch.where(self.volume > 0, self.t1 - self.t0 + 1, torch.zeros_like(self.t1))

    def centroids(self) -> torch.Tensor:
        """float64 [..., E, 3] on the device: (t, y, x) = sums / volume, each quotient rounded once; NaN for the all-zero records."""
        volume = self.volume.to(torch.float64)
        return torch.stack([s.to(torch.float64) / volume for s in (self.sum_t, self.sum_y, self.sum_x)], dim=-1)

    def alarms(self) -> torch.Tensor:
        """bool [..., T]: the frame holds a pixel of a kept event - the debounced alarm signal; it does not depend on max_events."""
        return self.frame_counts[..., 1] > 0

    def truncated(self) -> torch.Tensor:
        """bool [...]: the clip has more kept events than the table has records."""
        return self.counts[..., 0] > self.max_events

    def to_list(self) -> list:
        """A host copy of the table - 64 bytes per record, never a map -: one list per clip (clips in order) of {'root', 'volume',
        't0', 't1', 'duration', 'box': (x0, y0, x1, y1), 'peak', 'peak_tyx', 'centroid_tyx'} in table order."""
        _, h, w = self.volume_shape
        rec = self.records.reshape(-1, self.max_events, EVENT_WORDS).cpu().numpy()
        kept = self.counts.reshape(-1, 4)[:, 0].cpu().numpy()
        out = []
        for c in range(rec.shape[0]):
            rows = []
            for r in rec[c, :min(int(kept[c]), self.max_events)]:
                volume = int(r[1])
                sx, sy, st = (int(v) for v in r[10:16].copy().view(np.int64))
                pt, pp = divmod(int(r[9]), h * w)
                rows.append({"root": int(r[0]), "volume": volume, "t0": int(r[2]), "t1": int(r[3]), "duration": int(r[3]) - int(r[2]) + 1,
                             "box": tuple(int(v) for v in r[4:8]), "peak": float(r[8:9].copy().view(np.float32)[0]),
                             "peak_tyx": (pt, *divmod(pp, w)), "centroid_tyx": (st / volume, sy / volume, sx / volume)})
            out.append(rows)
        return out


def detect_events(maps: torch.Tensor, threshold: float, connectivity: int = 8, temporal: int = 9, min_duration: int = 1,
                  min_volume: int = 1, max_events: int = 64, return_labels: bool = False) -> Events:
    """The events of every clip, on the GPU (`vad_detect_events`, csrc/map_events.hip): the connected components of `maps >=
    threshold` in the volume `[T,H,W]` - the regions of `detect_regions` linked across consecutive frames.  `maps`: float32 GPU
    tensor `[T,H,W]` (one clip), `[B,T,H,W]` or `[B,T,1,H,W]` (the video model's maps); clips never link.  Inside a frame pixels
    connect as in `label_regions` (connectivity 8 or 4); `temporal` 1 links (t, y, x) to (t-1, y, x), `temporal` 9 to the set pixels
    of the 3 x 3 around it in frame t-1 (connectivity 8 only): (4, 1), (8, 1), (8, 9) are scipy.ndimage.label's 3-D structures
    `generate_binary_structure(3, 1)`, the full centre plane with single-pixel outer planes, and `generate_binary_structure(3, 3)`.
    Events that last at least `min_duration` frames and have at least `min_volume` pixels are kept, in ascending order of their
    first voxel (scipy's numbering), the first `max_events` (1..65536) written.  Returns an `Events`; like `detect_regions` it reads
    the kernels' flag word (one 4-byte copy, which waits for the call) and raises VadError if it is set.  No CPU fallback."""
    what = "detect_events"
    connectivity, temporal = _check_structure(connectivity, temporal, what)
    _check_maps(maps, what, "events are detected on the device")
    thr = _check_threshold(threshold, what)
    min_duration = _check_int(min_duration, "min_duration", what, 1, 2 ** 32 - 1)
    min_volume = _check_int(min_volume, "min_volume", what, 1, 2 ** 32 - 1)
    max_events = _check_int(max_events, "max_events", what, 1, MAX_EVENTS)
    if maps.dim() == 3:
        lead = ()
    elif maps.dim() == 4 or (maps.dim() == 5 and maps.shape[2] == 1):
        lead = (int(maps.shape[0]),)
    else:
        raise hip.VadError(f"{what}: maps must be [T,H,W], [B,T,H,W] or [B,T,1,H,W], got {tuple(maps.shape)}")
    t, h, w = int(maps.shape[-4] if maps.dim() == 5 else maps.shape[-3]), int(maps.shape[-2]), int(maps.shape[-1])
    if t < 1 or h < 1 or w < 1:
        raise hip.VadError(f"{what}: clips of {t} x {h} x {w} are out of range (T, H, W >= 1)")
    clips = maps.reshape(-1, t, h, w).contiguous()
    b = int(clips.shape[0])
    dev = clips.device

    def result(records, counts, frame_counts, labels):
        return Events(records.view(*lead, max_events, EVENT_WORDS), counts.view(*lead, 4), frame_counts.view(*lead, t, 3),
                      labels.view(*lead, t, h, w) if labels is not None else None, (t, h, w), thr, connectivity, temporal, min_duration,
                      min_volume)

    if b == 0:                                                            # nothing to detect, nothing to launch
        return result(torch.zeros((0, max_events, EVENT_WORDS), dtype=torch.int32, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev),
                      torch.zeros((0, t, 3), dtype=torch.int32, device=dev),
                      torch.zeros((0, t, h, w), dtype=torch.int32, device=dev) if return_labels else None)
    with torch.cuda.device(dev):
        l = hip.lib()
        ws = _workspace(l.vad_events_workspace_bytes(b, t, h, w, 1 if return_labels else 0), dev, what,
                        f"{b} clips of {t} x {h} x {w} are out of range (t * h * w < 2^31 - 1, b * t * h * w <= 2^38)")
        records = torch.empty((b, max_events, EVENT_WORDS), dtype=torch.int32, device=dev)
        counts = torch.empty((b, 4), dtype=torch.int32, device=dev)
        frame_counts = torch.empty((b, t, 3), dtype=torch.int32, device=dev)
        labels = torch.empty((b, t, h, w), dtype=torch.int32, device=dev) if return_labels else None
        hip.check(l.vad_detect_events(clips.data_ptr(), b, t, h, w, thr, connectivity, temporal, min_duration, min_volume, max_events,
                                      hip.ptr(labels), records.data_ptr(), counts.data_ptr(), frame_counts.data_ptr(), ws.data_ptr(),
                                      ws.numel(), hip.current_stream()), "vad_detect_events")
    _launched(ws, what)
    return result(records, counts, frame_counts, labels)


# ====================================================================== events against ground-truth masks
# `match_regions` in three dimensions: the per-frame report cannot see `min_duration`, `min_volume` or the
# links in time at all.  The kept events of `detect_events` are joined with the connected tracks of the clip's mask volume: how many
# labelled anomalies the debounced alarm still finds, how many false-alarm events it raises, how many frames after a defect appears
# it fires.  The host route copies every map and mask volume and runs a 3-D scipy.ndimage.label of both, sum_labels and minimum.
EVMATCH_WORDS = hip.EVMATCH_WORDS
EVMATCH_COUNTS = hip.EVMATCH_COUNTS
EVENT_COUNT_NAMES = ("gt_tracks", "gt_detected", "pred_events", "pred_matched", "false_alarm_events", "pred_dropped", "voxel_tp", "voxel_fp",
                     "voxel_fn", "voxel_tn", "nan_voxels", "gt_voxels", "delay_sum", "immediate_tracks", "frames_gt_pred", "frames_pred_only",
                     "frames_gt_only", "frames_neither", "clips_gt_pred", "clips_pred_only", "clips_gt_only", "clips_neither")
_NO_FRAME = -1                 # words 5-6 of a record without a shared voxel: 0xffffffff as int32


class EventMatches:
    """What `match_events` returns, as device tensors with the leading shape of the clips (`[B]`, or `()` for one volume):

      gt_records    int32 [..., E, 8]: the mask volume's tracks - root, volume, t0, t1, hit = voxels shared with kept events, first and
                    last frame of a shared voxel (-1 without one), flags (bit 0: detected) - in ascending order of their first voxel,
                    E = max_events, all-zero records behind them
      pred_records  int32 [..., E, 8]: the kept events - root, volume, t0, t1, overlap = voxels shared with the masks, first and last
                    frame of a shared voxel, flags (bit 0: matched; a kept event that is not matched is a false alarm)
      counts        int64 [..., 22]: the words of `vad_match_events` (include/vad_hip.h), named by `EVENT_COUNT_NAMES`; the track and
                    event counters are the full numbers, so a truncated table is visible
      frame_counts  int32 [..., T, 4]: voxels of P & G, P \\ G, G \\ P and NaN voxels of the frame

    Views of the records (no copies): `gt_volume`, `gt_hit`, `pred_volume`, `pred_overlap` int32 [..., E]."""

    def __init__(self, gt_records: torch.Tensor, pred_records: torch.Tensor, counts: torch.Tensor, frame_counts: torch.Tensor,
                 volume_shape: Tuple[int, int, int], params: dict):
        self.gt_records, self.pred_records, self.counts, self.frame_counts = gt_records, pred_records, counts, frame_counts
        self.volume_shape, self.params = volume_shape, dict(params)
        self.max_events = int(gt_records.shape[-2])

    gt_volume = property(lambda self: self.gt_records[..., 1])
    gt_hit = property(lambda self: self.gt_records[..., 4])
    pred_volume = property(lambda self: self.pred_records[..., 1])
    pred_overlap = property(lambda self: self.pred_records[..., 4])

    def detected(self) -> torch.Tensor:
        """bool [..., E]: the track of the record is detected (False for the all-zero records)."""
        return (self.gt_records[..., 7] & 1) != 0

    def matched(self) -> torch.Tensor:
        """bool [..., E]: the kept event of the record is matched; a record in use that is not is a false alarm."""
        return (self.pred_records[..., 7] & 1) != 0

    def delays(self) -> torch.Tensor:
        """int32 [..., E]: first shared frame - t0 of the detected tracks, -1 for every other record."""
        return torch.where(self.detected(), self.gt_records[..., 5] - self.gt_records[..., 2], torch.full_like(self.gt_records[..., 5], -1))

    def alarms(self) -> torch.Tensor:
        """bool [..., T]: the frame holds a voxel of a kept event - `Events.alarms()` of the same operating point."""
        return (self.frame_counts[..., 0] + self.frame_counts[..., 1]) > 0

    def truncated(self) -> torch.Tensor:
        """bool [...]: the clip has more tracks or more kept events than a table has records."""
        return (self.counts[..., 0] > self.max_events) | (self.counts[..., 2] > self.max_events)

    def to_list(self) -> list:
        """A host copy of the tables - 32 bytes per record, never a map -: one dict per clip {'gt': [{'root', 'volume', 't0', 't1',
        'hit', 'first_hit', 'last_hit', 'detected', 'delay'}], 'pred': [{'root', 'volume', 't0', 't1', 'overlap', 'first_overlap',
        'last_overlap', 'matched'}], 'counts': {name: int}} in table order; a frame that does not exist is None."""
        gt = self.gt_records.reshape(-1, self.max_events, EVMATCH_WORDS).cpu().numpy()
        pred = self.pred_records.reshape(-1, self.max_events, EVMATCH_WORDS).cpu().numpy()
        counts = self.counts.reshape(-1, EVMATCH_COUNTS).cpu().numpy()

        def frame(v):
            return None if int(v) == _NO_FRAME else int(v)

        out = []
        for c in range(counts.shape[0]):
            out.append({"gt": [{"root": int(r[0]), "volume": int(r[1]), "t0": int(r[2]), "t1": int(r[3]), "hit": int(r[4]), "first_hit": frame(r[5]),
                                "last_hit": frame(r[6]), "detected": bool(r[7] & 1), "delay": int(r[5]) - int(r[2]) if r[7] & 1 else None}
                               for r in gt[c, :min(int(counts[c, 0]), self.max_events)]],
                        "pred": [{"root": int(r[0]), "volume": int(r[1]), "t0": int(r[2]), "t1": int(r[3]), "overlap": int(r[4]),
                                  "first_overlap": frame(r[5]), "last_overlap": frame(r[6]), "matched": bool(r[7] & 1)}
                                 for r in pred[c, :min(int(counts[c, 2]), self.max_events)]],
                        "counts": {name: int(v) for name, v in zip(EVENT_COUNT_NAMES, counts[c])}})
        return out


def _event_match_params(what: str, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction) -> dict:
    """The checked operating point of `match_events` / `EventCounts`: what two sets of counters must share to be added."""
    connectivity, temporal = _check_structure(connectivity, temporal, what)
    return {"threshold": _check_threshold(threshold, what), "connectivity": connectivity, "temporal": temporal,
            "min_duration": _check_int(min_duration, "min_duration", what, 1, 2 ** 32 - 1),
            "min_volume": _check_int(min_volume, "min_volume", what, 1, 2 ** 32 - 1),
            "gt_fraction": _check_fraction(gt_fraction, "gt_fraction", what), "pred_fraction": _check_fraction(pred_fraction, "pred_fraction", what)}


def match_events(maps: torch.Tensor, masks: torch.Tensor, threshold: float, connectivity: int = 8, temporal: int = 9, min_duration: int = 1,
                 min_volume: int = 1, gt_fraction: float = 0.0, pred_fraction: float = 0.0, max_events: int = 64) -> EventMatches:
    """The events of `maps >= threshold` held against the ground-truth `masks`, on the GPU (`vad_match_events`,
    csrc/map_event_match.hip).  `maps`: float32 GPU tensor `[B,T,H,W]`, `[B,T,1,H,W]` or one volume `[T,H,W]` as in `detect_events`;
    `masks`: a GPU tensor with as many elements and the same `B` (`T` for one volume), `H`, `W`, in the formats of `match_regions`
    (float: anomalous iff > 0.5; uint8: iff >= 128; bool and other integers: iff non-zero).  The predictions are the events of
    `detect_events` with the same `threshold`, `connectivity`, `temporal`, `min_duration` and `min_volume`; a dropped event counts as
    background.  The connected components of the mask volume under the same structure are the ground-truth tracks; all of them
    count.  A track is DETECTED iff it shares at least one voxel, and at least `gt_fraction` of its volume, with the kept events; a
    kept event is MATCHED iff it shares at least one voxel, and at least `pred_fraction` of its volume, with the masks - otherwise
    it is a false alarm.  The delay of a detected track is the first frame of a shared voxel minus its first frame.  Touching, in
    space or in time, is no overlap; clips never link.  Returns an `EventMatches`; like `detect_events` it reads the kernels' flag
    word (one 4-byte copy, which waits for the call) and raises VadError if it is set.  No CPU fallback."""
    what = "match_events"
    params = _event_match_params(what, threshold, connectivity, temporal, min_duration, min_volume, gt_fraction, pred_fraction)
    if not isinstance(maps, torch.Tensor) or not isinstance(masks, torch.Tensor):
        raise hip.VadError(f"{what}: maps and masks must be torch tensors")
    if maps.dtype != torch.float32:
        raise hip.VadError(f"{what}: maps must be float32, got {maps.dtype}")
    if masks.is_complex():
        raise hip.VadError(f"{what}: masks must be float, uint8, bool or integer, got {masks.dtype}")
    max_events = _check_int(max_events, "max_events", what, 1, MAX_EVENTS)
    if maps.dim() == 3:
        lead = ()
    elif maps.dim() == 4 or (maps.dim() == 5 and maps.shape[2] == 1):
        lead = (int(maps.shape[0]),)
    else:
        raise hip.VadError(f"{what}: maps must be [T,H,W], [B,T,H,W] or [B,T,1,H,W], got {tuple(maps.shape)}")
    if masks.dim() not in (3, 4, 5) or masks.numel() != maps.numel() or masks.shape[-2:] != maps.shape[-2:] or masks.shape[0] != maps.shape[0]:
        raise hip.VadError(f"{what}: masks {tuple(masks.shape)} do not match maps {tuple(maps.shape)}")
    if not maps.is_cuda or not masks.is_cuda:
        raise hip.VadError(f"{what}: maps ({maps.device}) and masks ({masks.device}) must be on the GPU (events are matched on the "
                           "device; there is no CPU fallback)")
    if maps.device != masks.device:
        raise hip.VadError(f"{what}: maps ({maps.device}) and masks ({masks.device}) must be on the same device")
    t, h, w = int(maps.shape[-4] if maps.dim() == 5 else maps.shape[-3]), int(maps.shape[-2]), int(maps.shape[-1])
    if t < 1 or h < 1 or w < 1:
        raise hip.VadError(f"{what}: clips of {t} x {h} x {w} are out of range (T, H, W >= 1)")
    clips = maps.reshape(-1, t, h, w).contiguous()
    b = int(clips.shape[0])
    m, fmt, _, _, _ = _mask_planes(masks.reshape(-1, h, w), what)
    dev = clips.device

    def result(gt_records, pred_records, counts, frame_counts):
        return EventMatches(gt_records.view(*lead, max_events, EVMATCH_WORDS), pred_records.view(*lead, max_events, EVMATCH_WORDS),
                            counts.view(*lead, EVMATCH_COUNTS), frame_counts.view(*lead, t, 4), (t, h, w), params)

    if b == 0:                                                            # nothing to match, nothing to launch
        return result(torch.zeros((0, max_events, EVMATCH_WORDS), dtype=torch.int32, device=dev),
                      torch.zeros((0, max_events, EVMATCH_WORDS), dtype=torch.int32, device=dev),
                      torch.zeros((0, EVMATCH_COUNTS), dtype=torch.int64, device=dev), torch.zeros((0, t, 4), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        l = hip.lib()
        ws = _workspace(l.vad_event_match_workspace_bytes(b, t, h, w), dev, what,
                        f"{b} clips of {t} x {h} x {w} are out of range (t * h * w < 2^31 - 1, b * t * h * w <= 2^38)")
        gt_records = torch.empty((b, max_events, EVMATCH_WORDS), dtype=torch.int32, device=dev)
        pred_records = torch.empty((b, max_events, EVMATCH_WORDS), dtype=torch.int32, device=dev)
        counts = torch.empty((b, EVMATCH_COUNTS), dtype=torch.int64, device=dev)
        frame_counts = torch.empty((b, t, 4), dtype=torch.int32, device=dev)
        hip.check(l.vad_match_events(clips.data_ptr(), m.data_ptr(), fmt, b, t, h, w, params["threshold"], params["connectivity"],
                                     params["temporal"], params["min_duration"], params["min_volume"], params["gt_fraction"],
                                     params["pred_fraction"], max_events, gt_records.data_ptr(), pred_records.data_ptr(), counts.data_ptr(),
                                     frame_counts.data_ptr(), ws.data_ptr(), ws.numel(), hip.current_stream()), "vad_match_events")
    _launched(ws, what)
    return result(gt_records, pred_records, counts, frame_counts)


def event_report_from_counts(counts) -> dict:
    """The operating-point report of a debounced alarm from the 22 sums of `vad_match_events`' counters (`EVENT_COUNT_NAMES`), on the
    host - usable on a machine without a GPU.  Event level: track_recall = detected / tracks, event_precision = matched / kept
    events, event_f1 their harmonic mean, false-alarm events per frame and per clip.  Voxel level: precision, recall, IoU, Dice.
    Delay: mean_delay = the sum of the delays / detected tracks, in frames; immediate = the share of the detected tracks found in
    their first frame.  Frame level (a frame is positive with a mask voxel, alarmed with a voxel of a kept event - `alarms()`):
    precision, recall, F1.  Clip level (positive with a track, alarmed with a kept event) likewise.  A ratio whose denominator is 0
    is nan."""
    c = [int(v) for v in np.asarray(counts).reshape(-1)]
    if len(c) != EVMATCH_COUNTS or min(c) < 0:
        raise hip.VadError(f"event_report_from_counts: counts must be {EVMATCH_COUNTS} non-negative integers, got {counts!r}")
    gt, det, pred, matched, fa, _, tp, fp, fn, _, _, _, delay_sum, immediate, f_both, f_pred, f_gt, f_none, c_both, c_pred, c_gt, c_none = c
    frames, clips = f_both + f_pred + f_gt + f_none, c_both + c_pred + c_gt + c_none
    recall, precision = _ratio(det, gt), _ratio(matched, pred)
    out = {name: v for name, v in zip(EVENT_COUNT_NAMES, c)}
    out.update({"frames": frames, "clips": clips, "track_recall": recall, "event_precision": precision,
                "event_f1": 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else float("nan"),
                "false_alarm_events_per_frame": _ratio(fa, frames), "false_alarm_events_per_clip": _ratio(fa, clips),
                "voxel_precision": _ratio(tp, tp + fp), "voxel_recall": _ratio(tp, tp + fn), "voxel_iou": _ratio(tp, tp + fp + fn),
                "voxel_dice": _ratio(2 * tp, 2 * tp + fp + fn),
                "mean_delay": _ratio(delay_sum, det), "immediate": _ratio(immediate, det),
                "frame_precision": _ratio(f_both, f_both + f_pred), "frame_recall": _ratio(f_both, f_both + f_gt),
                "frame_f1": _ratio(2 * f_both, 2 * f_both + f_pred + f_gt),
                "clip_precision": _ratio(c_both, c_both + c_pred), "clip_recall": _ratio(c_both, c_both + c_gt),
                "clip_f1": _ratio(2 * c_both, 2 * c_both + c_pred + c_gt)})
    return out


class EventCounts:
    """The 22 counters of `match_events` summed over clips: an int64 `[22]` device tensor (`EVENT_COUNT_NAMES`) and the operating
    point they were gathered at - `params` = {threshold, connectivity, temporal, min_duration, min_volume, gt_fraction,
    pred_fraction} plus whatever `meta` the caller adds (`scoring.event_report`: map, sigma, truncate, morph, calibrated, the
    filters).  Counters gathered at another operating point are refused with `ValueError`, as in `DetectionCounts`.  Integer sums:
    the result does not depend on batching or sharding, and ranks combine with ONE all-reduce."""

    def __init__(self, device="cuda", params: Optional[dict] = None):
        self.counts = torch.zeros(EVMATCH_COUNTS, dtype=torch.int64, device=device)
        self.params = dict(params) if params else None

    def _adopt(self, params, what: str) -> None:
        if params is None:
            return
        if self.params is None:
            self.params = dict(params)
        elif self.params != dict(params):
            raise ValueError(f"{what}: these counters were gathered with {self.params}, the others with {dict(params)}")

    def update(self, matches: EventMatches, meta: Optional[dict] = None) -> "EventCounts":
        """Add the clips of one `match_events` result (one reduction on the device; nothing is read by the host)."""
        if not isinstance(matches, EventMatches):
            raise hip.VadError(f"EventCounts.update: matches must be a metrics.EventMatches, got {type(matches).__name__}")
        if matches.counts.device != self.counts.device:
            raise hip.VadError(f"EventCounts.update: the matches are on {matches.counts.device}, the counters on {self.counts.device}")
        self._adopt({**matches.params, **(meta or {})}, "EventCounts.update")
        self.counts += matches.counts.reshape(-1, EVMATCH_COUNTS).sum(dim=0)
        return self

    def merge(self, other: "EventCounts") -> "EventCounts":
        """self += other (two halves of a dataset, or the states of several ranks after a gather)."""
        if not isinstance(other, EventCounts):
            raise hip.VadError(f"EventCounts.merge: other must be an EventCounts, got {type(other).__name__}")
        self._adopt(other.params, "EventCounts.merge")
        self.counts += other.counts.to(self.counts.device)
        return self

    def all_reduce(self, group=None, force_collective: bool = False) -> int:
        """Sum the counters over the ranks of `group` (`allreduce_counters_`: one all_reduce).  Like `DetectionCounts.all_reduce` it
        carries the 22 words only: ranks compare their `params` themselves where they may differ.  Returns the world size."""
        return allreduce_counters_(self.counts, group, force_collective)

    def report(self) -> dict:
        """`event_report_from_counts` of the sums (one 176-byte copy to the host) with the operating point under 'params'."""
        out = event_report_from_counts(self.counts.cpu().numpy())
        out["params"] = None if self.params is None else dict(self.params)
        return out


# ====================================================================== per-frame tracks of anomaly events
# An event record holds the union box over the event's whole life; for anything that moves that is a smear over its path (DESIGN.md
# section 4.24).  A cross-section is the set of one event's pixels in one frame, as a record in the layout of `Regions`: a box that
# follows the object, where it is now, a trajectory.  The host route copies the label volume and runs scipy.ndimage find_objects /
# sum / maximum_position per frame and label; here the reduction per (event, frame) runs behind the labeller, on the device.
MAX_TRACK_RECORDS = hip.MAX_TRACK_RECORDS


class _CrossSections:
    """Views of cross-section records int32 [..., 12] (include/vad_hip.h: the words of a region record), no copies."""
    records: torch.Tensor

    root = property(lambda self: self.records[..., 0])
    area = property(lambda self: self.records[..., 1])
    box = property(lambda self: self.records[..., 2:6])
    peak = property(lambda self: self.records[..., 6].view(torch.float32))
    peak_index = property(lambda self: self.records[..., 7])
    sum_x = property(lambda self: self.records[..., 8:10].view(torch.int64)[..., 0])
    sum_y = property(lambda self: self.records[..., 10:12].view(torch.int64)[..., 0])

    def present(self) -> torch.Tensor:
        """bool [...]: the event has a pixel there (`area > 0`)."""
        return self.area > 0

    def centroids(self) -> torch.Tensor:
        """float64 [..., 2] on the device: (y, x) = (sum_y / area, sum_x / area), each quotient rounded once; NaN where absent."""
        area = self.area.to(torch.float64)
        return torch.stack([self.sum_y.to(torch.float64) / area, self.sum_x.to(torch.float64) / area], dim=-1)

    @staticmethod
    def _row(r: np.ndarray, w: int) -> dict:
        area = int(r[1])
        sx, sy = (int(v) for v in r[8:12].copy().view(np.int64))
        return {"root": int(r[0]), "area": area, "box": tuple(int(v) for v in r[2:6]), "peak": float(r[6:7].copy().view(np.float32)[0]),
                "peak_yx": divmod(int(r[7]), w), "centroid_yx": (sy / area, sx / area)}


class EventTracks(_CrossSections):
    """What `event_tracks` returns, with the leading shape of the events it was made from (`[B]`, or `()` for one clip):

      records  int32 [..., E, T, 12]: record (e, f) is the cross-section of kept event e - record e of the `Events` - in frame f:
               the smallest pixel y * W + x, the area, the box, the peak and its pixel, the coordinate sums of the event's pixels IN
               THAT FRAME; all-zero where the event has no pixel in the frame and for the slots behind the kept events
      counts   int32 [..., 4]: the counts of the `Events` (a view: `counts[..., 0]` kept events, which may exceed E)

    Views of `records` (no copies): `root`, `area`, `peak_index` int32 [..., E, T]; `box` int32 [..., E, T, 4] = x0, y0, x1, y1
    inclusive; `peak` float32 [..., E, T]; `sum_x`, `sum_y` int64 [..., E, T].  A cross-section may be disconnected inside its frame
    (its pieces join through other frames): it is one record."""

    def __init__(self, records: torch.Tensor, counts: torch.Tensor, volume_shape: Tuple[int, int, int]):
        self.records, self.counts, self.volume_shape = records, counts, volume_shape
        self.max_events = int(records.shape[-3])

    def frame(self, t: int) -> torch.Tensor:
        """int32 [..., E, 12] view: the cross-sections of every event in frame t - a region table of that frame, by event."""
        frames = int(self.records.shape[-2])
        if not _is_int(t) or not -frames <= t < frames:
            raise hip.VadError(f"EventTracks.frame: t must be an int in {-frames}..{frames - 1}, got {t!r}")
        return self.records[..., t, :]

    def to_list(self) -> list:
        """A host copy of the kept events' tracks only - 48 bytes per event and frame, never a map -: one list per clip of one list
        per kept event of one entry per frame, None where the event is absent, else {'root', 'area', 'box': (x0, y0, x1, y1), 'peak',
        'peak_yx', 'centroid_yx'}."""
        frames, w = int(self.records.shape[-2]), self.volume_shape[2]
        kept = torch.clamp(self.counts.reshape(-1, 4)[:, 0], max=self.max_events).cpu().numpy()
        flat = self.records.reshape(-1, self.max_events, frames, REGION_WORDS)
        out = []
        for c in range(flat.shape[0]):
            rec = flat[c, :int(kept[c])].cpu().numpy()
            out.append([[self._row(r, w) if r[1] else None for r in track] for track in rec])
        return out


def event_tracks(maps: torch.Tensor, events: "Events") -> EventTracks:
    """The cross-sections of every kept event of `events` in every frame, on the GPU (`vad_event_tracks`,
    csrc/map_event_tracks.hip).  `maps`: the float32 GPU tensor `events` was detected on (`[T,H,W]`, `[B,T,H,W]` or `[B,T,1,H,W]`);
    `events`: what `detect_events(maps, ..., return_labels=True)` returned - its label volume says which event a pixel belongs to,
    its records which events are kept and inside the table.  Events dropped by `min_duration` / `min_volume` and events without a
    record (`events.truncated()`) have no track.  Returns an `EventTracks`; at most 2^26 records `B * max_events * T` per call.
    Three launches behind the labeller, no workspace, nothing read by the host: the call can be captured.  No CPU fallback."""
    what = "event_tracks"
    if not isinstance(events, Events):
        raise hip.VadError(f"{what}: events must be a metrics.Events, got {type(events).__name__}")
    if events.labels is None:
        raise hip.VadError(f"{what}: events carry no labels; detect them with detect_events(..., return_labels=True)")
    if not isinstance(maps, torch.Tensor):
        raise hip.VadError(f"{what}: maps must be a torch tensor")
    t, h, w = events.volume_shape
    lead = tuple(int(v) for v in events.counts.shape[:-1])
    max_events = events.max_events
    shapes = [(*lead, t, h, w)] + ([(*lead, t, 1, h, w)] if lead else [])
    if tuple(maps.shape) not in shapes:
        raise hip.VadError(f"{what}: maps {tuple(maps.shape)} do not match the events' volumes {shapes[0]}")
    for name, v, shape in (("labels", events.labels, (*lead, t, h, w)), ("records", events.records, (*lead, max_events, EVENT_WORDS))):
        if tuple(v.shape) != shape:
            raise hip.VadError(f"{what}: the events' {name} {tuple(v.shape)} do not match their volumes: expected {shape}")
    for name, v in (("labels", events.labels), ("records", events.records), ("counts", events.counts)):
        if v.dtype != torch.int32:
            raise hip.VadError(f"{what}: the events' {name} must be int32, got {v.dtype}")
    _check_maps(maps, what, "tracks are reduced on the device")
    for name, v in (("labels", events.labels), ("records", events.records), ("counts", events.counts)):
        if v.device != maps.device:
            raise hip.VadError(f"{what}: maps ({maps.device}) and the events' {name} ({v.device}) are on different devices")
    b = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if b * max_events * t > MAX_TRACK_RECORDS:
        raise hip.VadError(f"{what}: {b} clips x {max_events} events x {t} frames are more than 2^26 records; call it on fewer clips")
    dev = maps.device
    clips, labels = maps.reshape(b, t, h, w).contiguous(), events.labels.reshape(b, t, h, w).contiguous()
    records, counts = events.records.reshape(b, max_events, EVENT_WORDS).contiguous(), events.counts.reshape(b, 4).contiguous()
    tracks = torch.empty((b, max_events, t, REGION_WORDS), dtype=torch.int32, device=dev)
    if b:
        with torch.cuda.device(dev):
            hip.check(hip.lib().vad_event_tracks(clips.data_ptr(), labels.data_ptr(), records.data_ptr(), counts.data_ptr(), b, t, h, w,
                                                 max_events, tracks.data_ptr(), hip.current_stream()), "vad_event_tracks")
        _count(what)
    return EventTracks(tracks.view(*lead, max_events, t, REGION_WORDS), events.counts, (t, h, w))


# ====================================================================== anomaly events across the calls of a live stream
# `detect_events` closes every event at the end of its clip.  A camera that hands over its newest frame (`score_stateful`) needs the
# events continued between calls: the open events and the newest frame's slot plane are state on the
# device, a call takes the new maps in and returns the events that closed and the causal alarm of every new frame.
TRACK_WORDS = hip.TRACK_WORDS
TRACK_MAX_OPEN = hip.TRACK_MAX_OPEN


class _TrackRecords:
    """Views of tracker records int32 [..., E, 20] (include/vad_hip.h, VAD_TRACK_WORDS), no copies."""
    records: torch.Tensor

    root_pixel = property(lambda self: self.records[..., 0])
    t0 = property(lambda self: self.records[..., 1])
    t1 = property(lambda self: self.records[..., 2])
    handle = property(lambda self: self.records[..., 3])
    box = property(lambda self: self.records[..., 4:8])
    peak = property(lambda self: self.records[..., 8].view(torch.float32))
    peak_pixel = property(lambda self: self.records[..., 9])
    peak_frame = property(lambda self: self.records[..., 10])
    volume = property(lambda self: self.records[..., 12:14].view(torch.int64)[..., 0])
    sum_x = property(lambda self: self.records[..., 14:16].view(torch.int64)[..., 0])
    sum_y = property(lambda self: self.records[..., 16:18].view(torch.int64)[..., 0])
    sum_t = property(lambda self: self.records[..., 18:20].view(torch.int64)[..., 0])

    def durations(self) -> torch.Tensor:
        """int64 [..., E]: t1 - t0 + 1 of the records in use (frame numbers are unsigned 32-bit words), 0 for the all-zero ones."""
        span = (self.t1.to(torch.int64) & 0xFFFFFFFF) - (self.t0.to(torch.int64) & 0xFFFFFFFF) + 1
        return torch.where(self.volume != 0, span, torch.zeros_like(span))

    def centroids(self) -> torch.Tensor:
        """float64 [..., E, 3] on the device: (t, y, x) = sums / volume; NaN for the all-zero records."""
        volume = self.volume.to(torch.float64)
        return torch.stack([s.to(torch.float64) / volume for s in (self.sum_t, self.sum_y, self.sum_x)], dim=-1)

    def _rows(self, used) -> list:
        rec = self.records.reshape(-1, self.records.shape[-2], TRACK_WORDS).cpu().numpy()
        w = self.frame_shape[1]
        out = []
        for c in range(rec.shape[0]):
            rows = []
            for r in rec[c, :int(used[c])]:
                u = r.view(np.uint32)
                volume, sx, sy, st = (int(v) for v in u[12:20].copy().view(np.uint64))
                rows.append({"root_pixel": int(u[0]), "t0": int(u[1]), "t1": int(u[2]), "duration": int(u[2]) - int(u[1]) + 1, "handle": int(u[3]),
                             "volume": volume, "box": tuple(int(v) for v in u[4:8]), "peak": float(u[8:9].copy().view(np.float32)[0]),
                             "peak_tyx": (int(u[10]), *divmod(int(u[9]), w)), "centroid_tyx": (st / volume, sy / volume, sx / volume)})
            out.append(rows)
        return out


class TrackBoxes(_CrossSections):
    """`TrackUpdate.boxes`: `records` int32 [B, max_open, 12] - record r is the cross-section, in the newest frame of the call, of
    the open event in slot r (`vad_track_boxes`): its smallest pixel (the event's `handle`), area, box, peak and peak pixel,
    coordinate sums IN THAT FRAME; all-zero behind the open events.  A lost event has no record.  The views of `EventTracks`
    without the frame axis: `root`, `area`, `box`, `peak`, `peak_index`, `sum_x`, `sum_y`, `present()`, `centroids()`."""

    def __init__(self, records, frame_shape):
        self.records, self.frame_shape = records, frame_shape

    def to_list(self) -> list:
        """A host copy - 48 bytes per slot, never a map -: one list per stream of the open slots' cross-sections, in slot order."""
        w = self.frame_shape[1]
        rec = self.records.cpu().numpy()
        return [[self._row(r, w) for r in stream if r[1]] for stream in rec]


class TrackUpdate(_TrackRecords):
    """What one `EventTracker.update` / `flush` returns, as device tensors with the leading shape `[B]` of the streams:

      records       int32 [B, E, 20]: the events that CLOSED in this call and pass the filters, in ascending (t1, handle) order, E =
                    max_closed; all-zero records behind them
      counts        int32 [B, 6]: closed and kept (the full number: above E the table is truncated), closed and dropped by a filter,
                    foreground pixels, NaN pixels, events open after the call, events lost in this call
      frame_counts  int32 [B, T, 3]: foreground pixels of the frame, pixels of the frame that belong to events which alarm NOW
                    (duration so far >= min_duration, volume so far >= min_volume), NaN pixels of the frame; T = 0 for a flush

    Views of `records` as in `Events`, with `root_pixel` / `t0` in place of `root`, `peak_pixel` / `peak_frame` in place of
    `peak_index`, `handle`, and `volume` as int64.

      boxes         a `TrackBoxes` after `update(maps, boxes=True)`, else None: the cross-sections of the open events in the newest
                    frame of the call"""

    def __init__(self, records, counts, frame_counts, frame_shape, max_closed, boxes=None, tracker=None):
        self.records, self.counts, self.frame_counts, self.frame_shape, self.max_closed = records, counts, frame_counts, frame_shape, max_closed
        self.boxes, self._tracker = boxes, tracker

    def boxes_alarming(self) -> torch.Tensor:
        """bool [B, max_open]: the open event in that slot alarms now - it has lasted `min_duration` frames and gathered
        `min_volume` pixels -, false behind the open events.  Torch operations on the tracker's open table AS IT STANDS: ask before
        the next `update` / `flush` / `reset` of the tracker.  Needs `update(maps, boxes=True)`."""
        if self.boxes is None:
            raise hip.VadError("TrackUpdate.boxes_alarming: this update carries no boxes; call update(maps, boxes=True)")
        tr = self._tracker
        opened = tr.open_events()
        in_use = torch.arange(tr.max_open, device=opened.records.device)[None, :] < opened.counts[:, None]
        return in_use & (opened.durations() >= tr.min_duration) & (opened.volume >= tr.min_volume)

    def alarms(self) -> torch.Tensor:
        """bool [B, T]: the frame holds a pixel of an event that has lasted min_duration frames and gathered min_volume pixels."""
        return self.frame_counts[..., 1] > 0

    def truncated(self) -> torch.Tensor:
        """bool [B]: more events closed and passed the filters in this call than the table has records."""
        return self.counts[..., 0] > self.max_closed

    def lost(self) -> torch.Tensor:
        """int32 [B]: open events that found no slot in the open table in this call (max_open): they have no record, never alarm."""
        return self.counts[..., 5]

    def to_list(self) -> list:
        """A host copy of the closed table - 80 bytes per record, never a map -: one list per stream of dicts in table order."""
        return self._rows(torch.clamp(self.counts[:, 0], max=self.max_closed).cpu().numpy())


class OpenEvents(_TrackRecords):
    """The live table of an `EventTracker`: `records` int32 [B, max_open, 20] - a view of the state, slot r = the open event whose
    handle has rank r in raster order -, `counts` int32 [B] = the open events with a record."""

    def __init__(self, records, counts, frame_shape):
        self.records, self.counts, self.frame_shape = records, counts, frame_shape

    def to_list(self) -> list:
        return self._rows(self.counts.cpu().numpy())


class EventTracker:
    """Events of B live streams, carried across calls on the device (`vad_track_events`, csrc/map_track.hip).
    The specification is `detect_events` applied to prefixes of a stream: the same predicate (`v >= threshold`, NaN never, `+Inf`
    always), the same structures (`connectivity`, `temporal`) = (4, 1), (8, 1), (8, 9).  `update(maps)` continues every stream by
    T >= 1 maps and returns a `TrackUpdate`: the events that closed (no pixel of the next frame links to them) and pass
    `min_duration` / `min_volume`, and per new frame the pixels of the events that alarm now.  Closed + flushed events are exactly
    the events `detect_events` finds in the whole stream, for any split of the frames over calls - while nothing is lost: at most
    `max_open` (1..65536) events are open at a time, one behind that has no record and is counted in `TrackUpdate.lost()`.
    The frame number is counted on the device, so a captured `update` can be replayed.  Like `detect_events`, every call reads the
    kernels' 4-byte flag word (which waits for the call) and raises VadError if it is set - unless the call is being captured into
    a graph: then read `flags()` after the replays.  No CPU fallback."""

    def __init__(self, streams: int, h: int, w: int, threshold: float, connectivity: int = 8, temporal: int = 9, min_duration: int = 1,
                 min_volume: int = 1, max_open: int = 1024, max_closed: int = 64, device=None):
        what = "EventTracker"
        self.connectivity, self.temporal = _check_structure(connectivity, temporal, what)
        self.threshold = _check_threshold(threshold, what)
        self.streams = _check_int(streams, "streams", what, 0, 2 ** 20)
        self.h, self.w = _check_int(h, "h", what, 1, 2 ** 24), _check_int(w, "w", what, 1, 2 ** 24)
        self.min_duration = _check_int(min_duration, "min_duration", what, 1, 2 ** 32 - 1)
        self.min_volume = _check_int(min_volume, "min_volume", what, 1, 2 ** 32 - 1)
        self.max_open = _check_int(max_open, "max_open", what, 1, TRACK_MAX_OPEN)
        self.max_closed = _check_int(max_closed, "max_closed", what, 1, TRACK_MAX_OPEN)
        if self.h * self.w > 2 ** 24:
            raise hip.VadError(f"{what}: frames of {h} x {w} are out of range (h * w <= 2^24)")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise hip.VadError(f"{what}: device ({dev}) must be a GPU (events are tracked on the device; there is no CPU fallback)")
        self.device = dev
        l = hip.lib()
        size = l.vad_track_state_bytes(self.streams, self.h, self.w, self.max_open)
        if self.streams and size == 0:
            raise hip.VadError(f"{what}: {streams} streams of {h} x {w} with max_open {max_open} are out of range")
        self._stream_words = size // 4 // max(self.streams, 1)
        self.state = torch.empty(size // 4, dtype=torch.int32, device=dev)
        self._ws = None
        self.reset()

    def _blob(self) -> torch.Tensor:
        return self.state.view(self.streams, self._stream_words) if self.streams else self.state.view(0, hip.TRACK_HEADER_WORDS)

    def reset(self, streams=None) -> None:
        """A fresh header, table and plane (asynchronous): of every stream, or of the streams in `streams` (indices)."""
        l = hip.lib()
        with torch.cuda.device(self.device):
            if streams is None:
                if self.streams:
                    hip.check(l.vad_track_init(self.state.data_ptr(), self.streams, self.h, self.w, self.max_open, hip.current_stream()), "vad_track_init")
                return
            for s in streams:
                s = int(s)
                if not 0 <= s < self.streams:
                    raise hip.VadError(f"EventTracker.reset: stream {s} is out of range (0..{self.streams - 1})")
                hip.check(l.vad_track_init(self.state.data_ptr() + 4 * s * self._stream_words, 1, self.h, self.w, self.max_open,
                                           hip.current_stream()), "vad_track_init")

    @property
    def header(self) -> torch.Tensor:
        """int32 [B, 16] view: frames seen, open events, lost in total, flags, magic, h, w, max_open, zeros."""
        return self._blob()[:, :hip.TRACK_HEADER_WORDS]

    @property
    def frames_seen(self) -> torch.Tensor:
        """int64 [B] on the device: the frames every stream has taken in since its last reset."""
        return self.header[:, 0].to(torch.int64) & 0xFFFFFFFF

    @property
    def slot_plane(self) -> torch.Tensor:
        """int32 [B, H, W] view of the state: 0, slot + 1 of the pixel's open event in the newest frame, or -1 (no record)."""
        at = hip.TRACK_HEADER_WORDS + self.max_open * TRACK_WORDS
        return self._blob()[:, at:at + self.h * self.w].view(self.streams, self.h, self.w)

    def open_events(self) -> OpenEvents:
        at = hip.TRACK_HEADER_WORDS
        table = self._blob()[:, at:at + self.max_open * TRACK_WORDS].view(self.streams, self.max_open, TRACK_WORDS)
        return OpenEvents(table, self.header[:, 1], (self.h, self.w))

    def lost_total(self) -> torch.Tensor:
        return self.header[:, 2]

    def flags(self) -> int:
        """The sticky flag words of every stream, OR-ed (a host read): 0, or what `update` would have raised on."""
        return int(np.bitwise_or.reduce(self.header[:, 3].cpu().numpy(), initial=0)) if self.streams else 0

    def _workspace(self, t: int) -> torch.Tensor:
        size = hip.lib().vad_track_workspace_bytes(self.streams, t, self.h, self.w, self.max_open)
        if size == 0 or self._ws is None or self._ws.numel() < size:      # kept and grown as needed
            self._ws = _workspace(size, self.device, "EventTracker",
                                  f"{self.streams} streams of {t} x {self.h} x {self.w} are out of range (b * t * h * w <= 2^38)")
        return self._ws

    def _done(self, ws, what):
        _count("track_events")
        if torch.cuda.is_current_stream_capturing():                      # no host read inside a capture: see `flags()`
            return
        flags = _flag_word(ws)
        if flags & ~3:
            raise hip.VadError(f"{what}: flags {flags:#x} are set - a stream's frame counter stands at 2^32 - 1; reset the tracker")
        _raise_on_flags(flags, what)

    def update(self, maps: torch.Tensor, boxes: bool = False) -> TrackUpdate:
        """maps: float32 GPU tensor `[B,H,W]` (one new map per stream), `[B,T,H,W]` or `[B,T,1,H,W]`.
        `boxes=True`: `vad_track_boxes` is launched behind the tracker's launches and `TrackUpdate.boxes` holds, per open slot, the
        cross-section of its event in the LAST frame of the call (a `TrackBoxes`; its `root` is `open_events().handle`) - the box
        that follows the object, where the open record has the union box of the event's life.  With T > 1 only the last frame has
        cross-sections: a live stream calls with T = 1.  `boxes=False` (the default): nothing more is launched, `boxes` is None."""
        what = "EventTracker.update"
        if not isinstance(boxes, bool):
            raise hip.VadError(f"{what}: boxes must be a bool, got {boxes!r}")
        _check_maps(maps, what, "events are tracked on the device")
        if maps.dim() == 3:
            maps = maps[:, None]
        elif maps.dim() == 5 and maps.shape[2] == 1:
            maps = maps[:, :, 0]
        elif maps.dim() != 4:
            raise hip.VadError(f"{what}: maps must be [B,H,W], [B,T,H,W] or [B,T,1,H,W], got {tuple(maps.shape)}")
        b, t = int(maps.shape[0]), int(maps.shape[1])
        if (b, int(maps.shape[2]), int(maps.shape[3])) != (self.streams, self.h, self.w):
            raise hip.VadError(f"{what}: maps {tuple(maps.shape)} do not match the tracker's state: {self.streams} streams of {self.h} x {self.w}")
        if t < 1:
            raise hip.VadError(f"{what}: every stream needs at least one new map, got T = {t}")
        if maps.device != self.state.device:
            raise hip.VadError(f"{what}: maps ({maps.device}) and the tracker's state ({self.state.device}) are on different devices")
        maps = maps.contiguous()
        dev = self.state.device
        records = torch.empty((b, self.max_closed, TRACK_WORDS), dtype=torch.int32, device=dev)
        counts = torch.empty((b, 6), dtype=torch.int32, device=dev)
        frame_counts = torch.empty((b, t, 3), dtype=torch.int32, device=dev)
        table = torch.empty((b, self.max_open, REGION_WORDS), dtype=torch.int32, device=dev) if boxes else None
        if b == 0:
            return TrackUpdate(records, counts, frame_counts, (self.h, self.w), self.max_closed,
                               TrackBoxes(table, (self.h, self.w)) if boxes else None, self)
        with torch.cuda.device(dev):
            ws = self._workspace(t)
            hip.check(hip.lib().vad_track_events(maps.data_ptr(), b, t, self.h, self.w, self.threshold, self.connectivity, self.temporal,
                                                 self.min_duration, self.min_volume, self.max_open, self.max_closed, self.state.data_ptr(),
                                                 records.data_ptr(), counts.data_ptr(), frame_counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 hip.current_stream()), "vad_track_events")
            if boxes:                                                         # the last frame of the call, in place
                npix = self.h * self.w
                hip.check(hip.lib().vad_track_boxes(maps.data_ptr() + 4 * (t - 1) * npix, t * npix, b, self.h, self.w, self.max_open,
                                                    self.state.data_ptr(), table.data_ptr(), hip.current_stream()), "vad_track_boxes")
                _count("track_boxes")
            self._done(ws, what)
        return TrackUpdate(records, counts, frame_counts, (self.h, self.w), self.max_closed,
                           TrackBoxes(table, (self.h, self.w)) if boxes else None, self)

    def flush(self) -> TrackUpdate:
        """Closes every open event as if an empty frame had arrived - in slot order, through the same filters -, without advancing
        the frame counter: the end of a recording.  The table and the plane are empty afterwards."""
        b, dev = self.streams, self.state.device
        records = torch.empty((b, self.max_closed, TRACK_WORDS), dtype=torch.int32, device=dev)
        counts = torch.empty((b, 6), dtype=torch.int32, device=dev)
        frame_counts = torch.zeros((b, 0, 3), dtype=torch.int32, device=dev)
        if b:
            with torch.cuda.device(dev):
                ws = self._workspace(0)
                hip.check(hip.lib().vad_track_flush(b, self.h, self.w, self.min_duration, self.min_volume, self.max_open, self.max_closed,
                                                    self.state.data_ptr(), records.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    hip.current_stream()), "vad_track_flush")
                self._done(ws, "EventTracker.flush")
        return TrackUpdate(records, counts, frame_counts, (self.h, self.w), self.max_closed)


# ====================================================================== per-pixel calibration of anomaly maps
# An autoencoder's error is not the same everywhere: on a fixed camera, edges, glossy patches and fine
# texture reconstruct worse than flat background in every normal frame, so one global threshold either fires there all day or is
# set so high that a defect on the background is missed.  Calibration on normal data: the per-pixel mean and standard deviation of
# the map over the training frames, and z = (map - mean) / std in place of the map.  The host route is a copy of every training
# map and numpy `mean` / `std` over N x H x W; here the maps never leave the device.
_MS_MAGIC = 0x4d444156         # "VADM", csrc/map_stats.hip
_MS_HEADER_BYTES = 32
# The floor of the standard deviation: 2^-14 = 6.10e-5, the squared error of ONE grey level of an 8-bit input on the models' [-1, 1]
# scale ((2 / 255)^2 = 6.15e-5) rounded to a power of two (the division by it is exact).  A pixel whose error varied by less than
# that over the normal frames - a masked border, a saturated patch: std 0 - is treated as varying by one grey level, so rounding
# noise there stays far below z = 1 and a real deviation still stands out.
DEFAULT_MIN_STD = 2.0 ** -14


def _check_min_std(min_std, what: str) -> float:
    ok = not isinstance(min_std, bool) and isinstance(min_std, (int, float, np.integer, np.floating))
    with np.errstate(over="ignore"):
        v = np.float32(min_std) if ok else np.float32("nan")
    if not (np.isfinite(v) and v > 0):                           # as float32: what the kernel divides by
        raise hip.VadError(f"{what}: min_std must be a finite float32 greater than 0, got {min_std!r}")
    return float(v)


class MapStatistics:
    """Per-pixel mean and standard deviation of anomaly maps over a stream of frames, in one device blob (include/vad_hip.h
    `vad_mapstat_*`): a header with the geometry and the frame count, and three float64 planes K (the pixel's first value), S1 =
    sum(x - K), S2 = sum((x - K)^2).  The arithmetic is fully specified (tests/map_stats_ref.py restates it bit for bit): every
    frame is added in order, so the state does not depend on how the frames were batched.

    `update(maps)` adds a batch on the GPU, asynchronously; `mean()` / `std(ddof)` are float32 `[H, W]` device tensors;
    `normalize(maps)` is the z-score map (and its per-frame maxima); `merge`, `state_dict` / `load_state_dict` combine and carry
    states.  `count` is the number of frames, tracked on the host as well so that a call that needs more frames than were seen is
    refused with `ValueError`; `meta` records what kind of map was accumulated (`scoring.calibrate` fills it, the scoring drivers
    compare it with their own arguments).  GPU only: there is no CPU fallback."""

    def __init__(self, frame_shape, device="cuda"):
        if not isinstance(frame_shape, (tuple, list)) or len(frame_shape) != 2 or not all(_is_int(v) for v in frame_shape):
            raise hip.VadError(f"MapStatistics: frame_shape must be (H, W), got {frame_shape!r}")
        h, w = int(frame_shape[0]), int(frame_shape[1])
        if h < 1 or w < 1 or h * w > hip.MAX_FRAME_PIXELS:
            raise hip.VadError(f"MapStatistics: frames of {h} x {w} are out of range (H, W >= 1 and H * W <= {hip.MAX_FRAME_PIXELS})")
        self.frame_shape = (h, w)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip.VadError(f"MapStatistics: device {self.device} is not a GPU (the statistics are gathered on the device; there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        nbytes = hip.lib().vad_mapstat_state_bytes(h, w)
        assert nbytes == _MS_HEADER_BYTES + 24 * h * w
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.meta = {}
        self.reset()

    # ------------------------------------------------------------------ state
    def _planes(self) -> torch.Tensor:
        """K, S1, S2 as one float64 view [3, H, W] of the blob."""
        return self._state[_MS_HEADER_BYTES:].view(torch.float64).view(3, *self.frame_shape)

    def reset(self) -> "MapStatistics":
        h, w = self.frame_shape
        with torch.cuda.device(self.device):
            hip.check(hip.lib().vad_mapstat_reset(self._state.data_ptr(), h, w, hip.current_stream()), "vad_mapstat_reset")
        self.count = 0
        self._final = {}
        return self

    def device_count(self) -> int:
        """The frame count of the device header (one 8-byte copy, which waits for the stream): what a replayed graph advanced."""
        return int(self._state[16:24].view(torch.int64).item())

    def state_dict(self) -> dict:
        """{'frame_shape', 'count', 'K', 'S1', 'S2' float64 [H, W] on the host, 'meta'}: carry a calibration to another process."""
        planes = self._planes().cpu()
        return {"frame_shape": self.frame_shape, "count": self.device_count(), "K": planes[0].clone(), "S1": planes[1].clone(),
                "S2": planes[2].clone(), "meta": dict(self.meta)}

    def load_state_dict(self, state: dict) -> "MapStatistics":
        if tuple(state.get("frame_shape", ())) != self.frame_shape:
            raise hip.VadError(f"MapStatistics.load_state_dict: frame_shape {state.get('frame_shape')!r} of the saved state differs from "
                               f"this object's {self.frame_shape}")
        planes = [torch.as_tensor(np.asarray(state[k])) for k in ("K", "S1", "S2")]
        if any(tuple(t.shape) != self.frame_shape or t.dtype != torch.float64 for t in planes):
            raise hip.VadError(f"MapStatistics.load_state_dict: K, S1 and S2 must be float64 {self.frame_shape}")
        count = int(state["count"])
        if count < 0:
            raise hip.VadError(f"MapStatistics.load_state_dict: count must not be negative, got {count}")
        self.reset()
        self._planes().copy_(torch.stack(planes))
        self._state[16:24].view(torch.int64).fill_(count)
        self.count = count
        self.meta = dict(state.get("meta", {}))
        return self

    # ------------------------------------------------------------------ accumulate / combine
    def _frames(self, maps: torch.Tensor, what: str) -> int:
        """Checks a map batch [..., H, W]; -> the number of frames.  Between the two common parts, `ValueError` for another frame
        shape: statistics of other maps, as in `merge`."""
        _check_maps(maps, what, "", self.device)
        if maps.dim() < 2 or tuple(maps.shape[-2:]) != self.frame_shape:
            raise ValueError(f"{what}: maps {tuple(maps.shape)} do not end in the frame shape {self.frame_shape} of the statistics")
        if not maps.is_contiguous():
            raise hip.VadError(f"{what}: maps must be contiguous (got strides {tuple(maps.stride())} for {tuple(maps.shape)}); it is not copied silently")
        lead = tuple(maps.shape[:-2])
        return int(np.prod(lead, dtype=np.int64)) if lead else 1

    def update(self, maps: torch.Tensor) -> "MapStatistics":
        """Add every H x W frame of `maps` (float32 GPU tensor, contiguous, any leading dimensions - `[B,1,H,W]` error / SSIM maps, the
        `[B,T,1,H,W]` maps of the video model) in row-major order of the leading dimensions.  Asynchronous on the current stream."""
        n = self._frames(maps, "MapStatistics.update")
        if n == 0:
            return self
        h, w = self.frame_shape
        with torch.cuda.device(self.device):
            hip.check(hip.lib().vad_mapstat_accumulate(maps.data_ptr(), n, h, w, self._state.data_ptr(), hip.current_stream()),
                      "vad_mapstat_accumulate")
        _count("mapstat_accumulate")
        self.count += n
        self._final = {}
        return self

    def merge(self, other: "MapStatistics") -> "MapStatistics":
        """self += other, for statistics gathered separately (two streams, two loaders): as if other's frames had followed."""
        if not isinstance(other, MapStatistics):
            raise hip.VadError(f"MapStatistics.merge: other must be a MapStatistics, got {type(other).__name__}")
        if other is self:
            raise hip.VadError("MapStatistics.merge: other is this object")
        if other.frame_shape != self.frame_shape:
            raise ValueError(f"MapStatistics.merge: frame shapes differ ({self.frame_shape} and {other.frame_shape})")
        if self.meta and other.meta and self.meta != other.meta:
            raise ValueError(f"MapStatistics.merge: the statistics are of different maps ({self.meta} and {other.meta})")
        if other.device != self.device:
            raise hip.VadError(f"MapStatistics.merge: other ({other.device}) must be on this object's device {self.device}")
        h, w = self.frame_shape
        with torch.cuda.device(self.device):
            hip.check(hip.lib().vad_mapstat_merge(self._state.data_ptr(), other._state.data_ptr(), h, w, hip.current_stream()),
                      "vad_mapstat_merge")
        self.count += other.count
        self.meta = dict(self.meta or other.meta)
        self._final = {}
        return self

    # ------------------------------------------------------------------ results
    def _finalize(self, ddof: int):
        """(mean, std) float32 [H, W] for `ddof`, computed once per state."""
        if ddof not in self._final:
            h, w = self.frame_shape
            mean = torch.empty(self.frame_shape, dtype=torch.float32, device=self.device)
            std = torch.empty(self.frame_shape, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                hip.check(hip.lib().vad_mapstat_finalize(self._state.data_ptr(), h, w, ddof, mean.data_ptr(), std.data_ptr(),
                                                         hip.current_stream()), "vad_mapstat_finalize")
            self._final[ddof] = (mean, std)
        return self._final[ddof]

    def _check_ddof(self, ddof, what: str) -> int:
        ddof = _check_choice(ddof, "ddof", what, 0, 1)
        if self.count - ddof <= 0:
            raise ValueError(f"{what}: {self.count} frames are not enough for a standard deviation with ddof={ddof}")
        return ddof

    def mean(self) -> torch.Tensor:
        """float32 [H, W]: fl32(K + S1 / n); NaN everywhere before the first frame.  Do not write to it (it is kept)."""
        return self._finalize(0 if self.count < 2 else 1)[0]

    def std(self, ddof: int = 1) -> torch.Tensor:
        """float32 [H, W]: sqrtf(fl32(max((S2 - S1^2 / n) / (n - ddof), 0))); `ValueError` when count - ddof <= 0.  Kept: do not write."""
        return self._finalize(self._check_ddof(ddof, "MapStatistics.std"))[1]

    def normalize(self, maps: torch.Tensor, min_std: float = DEFAULT_MIN_STD, out: Optional[torch.Tensor] = None, return_max=False,
                  ddof: int = 1):
        """z = (maps - mean) / max(std, min_std) of every frame on the GPU (`vad_map_normalize`), float32, each operation rounded on
        its own; a pixel whose std is NaN (it saw a NaN or an Inf) gives NaN.  `maps` as in `update`.  Returns the z-score tensor
        (written to `out` if given: same shape, float32, contiguous; `out=maps` normalises in place, a partly overlapping `out` is
        refused); with `return_max=True` also the per-frame maxima in the leading shape (`torch.amax` semantics), with
        `return_max="only"` just the maxima, and no map is written - the arguments of `smooth_maps`.  `ValueError` when
        count - ddof <= 0.  Asynchronous on the current stream."""
        what = "MapStatistics.normalize"
        if not isinstance(return_max, bool) and return_max != "only":
            raise hip.VadError(f"{what}: return_max must be False, True or 'only', got {return_max!r}")
        min_std = _check_min_std(min_std, what)
        n = self._frames(maps, what)
        ddof = self._check_ddof(ddof, what)
        only = return_max == "only"
        if only and out is not None:
            raise hip.VadError(f"{what}: return_max='only' writes no map; out must be None")
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(maps.shape) or out.dtype != torch.float32
                                or out.device != maps.device or not out.is_contiguous()):
            raise hip.VadError(f"{what}: out must be a contiguous float32 tensor {tuple(maps.shape)} on {maps.device}")
        lead, (h, w) = tuple(maps.shape[:-2]), self.frame_shape
        mean, std = self._finalize(ddof)
        with torch.cuda.device(self.device):
            if out is None and not only:
                out = torch.empty_like(maps)
            fmax = torch.empty(lead, dtype=torch.float32, device=self.device) if return_max else None
            if n > 0:
                l = hip.lib()
                need = l.vad_map_normalize_workspace_bytes(n, h, w) if return_max else 0
                ws = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
                hip.check(l.vad_map_normalize(maps.data_ptr(), n, h, w, mean.data_ptr(), std.data_ptr(), min_std, hip.ptr(out), hip.ptr(fmax),
                                              hip.ptr(ws), need, hip.current_stream()), "vad_map_normalize")
                _count("map_normalize")
        if only:
            return fmax
        return (out, fmax) if return_max else out
