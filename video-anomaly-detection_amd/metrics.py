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
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import hip

MIN_MANTISSA_BITS, MAX_MANTISSA_BITS = hip.HIST_MIN_M, hip.HIST_MAX_M
_MAGIC = 0x48444156           # "VADH", csrc/score_hist.hip
_HEADER_BYTES = 16


def _check_m(m, what: str) -> int:
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not MIN_MANTISSA_BITS <= int(m) <= MAX_MANTISSA_BITS:
        raise hip.VadError(f"{what}: mantissa_bits must be an int in {MIN_MANTISSA_BITS}..{MAX_MANTISSA_BITS}, got {m!r}")
    return int(m)


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


class ScoreHistogram:
    """Counters of (score bin, class) in one device blob (include/vad_hip.h `vad_hist_*`).

    `accumulate(values, labels)` adds a batch on the GPU; `counts()` / `rejected()` are int64 device tensors, `counts_host()` is the
    one host read (16 * (255 << m) bytes: 8 MB at the default m = 11); `merge`, `all_reduce`, `state_dict` / `load_state_dict`
    combine and carry states.  With `device="cpu"` the object is a container for counters (load, merge, all-reduce, read):
    accumulating runs on the GPU only and there is no CPU fallback."""

    def __init__(self, mantissa_bits: int = 11, device="cuda"):
        self.mantissa_bits = _check_m(mantissa_bits, "ScoreHistogram")
        self.nbins = 255 << self.mantissa_bits
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._state = torch.empty(state_bytes(self.mantissa_bits), dtype=torch.uint8, device=self.device)
        if self.device.type == "cuda":
            assert hip.lib().vad_hist_state_bytes(self.mantissa_bits) == self._state.numel()
        self.reset()

    # ------------------------------------------------------------------ state
    def _words(self) -> torch.Tensor:
        """counts[2][nbins] then rejected[2] as one int64 view of the blob (the uint64 counters stay below 2^63)."""
        return self._state[_HEADER_BYTES:].view(torch.int64)

    def _header(self) -> np.ndarray:
        m = self.mantissa_bits
        return np.array([_MAGIC, (hip.ABI_VERSION << 16) | m, m, 0], np.uint32)

    def reset(self) -> "ScoreHistogram":
        if self.device.type == "cuda":
            with torch.cuda.device(self.device):
                hip.check(hip.lib().vad_hist_reset(self._state.data_ptr(), self.mantissa_bits, hip.current_stream()), "vad_hist_reset")
        else:
            self._state.zero_()
            self._state[:_HEADER_BYTES] = torch.from_numpy(self._header().view(np.uint8).copy())
        return self

    def counts(self) -> torch.Tensor:
        """int64 [2, nbins] on the histogram's device (a copy): row 0 = normal, row 1 = anomalous."""
        return self._words()[:2 * self.nbins].view(2, self.nbins).clone()

    def rejected(self) -> torch.Tensor:
        """int64 [2]: negative, NaN and infinite values seen per class (they are in no bin)."""
        return self._words()[2 * self.nbins:].clone()

    def counts_host(self) -> np.ndarray:
        """The counters as numpy int64 [2, nbins]: the one device -> host read of an evaluation.  The blob's header travels with
        them and is checked."""
        blob = self._state.cpu().numpy()
        if not np.array_equal(blob[:_HEADER_BYTES].view(np.uint32), self._header()):
            raise hip.VadError("ScoreHistogram: the state's header is not that of a histogram with mantissa_bits "
                               f"{self.mantissa_bits} (the blob was overwritten)")
        return blob[_HEADER_BYTES:_HEADER_BYTES + 16 * self.nbins].view(np.int64).reshape(2, self.nbins).copy()

    def state_dict(self) -> dict:
        """{'mantissa_bits', 'counts' int64 [2, nbins], 'rejected' int64 [2]} on the host: resume a long evaluation later."""
        return {"mantissa_bits": self.mantissa_bits, "counts": self.counts().cpu(), "rejected": self.rejected().cpu()}

    def load_state_dict(self, state: dict) -> "ScoreHistogram":
        m = state.get("mantissa_bits")
        if m != self.mantissa_bits:
            raise hip.VadError(f"ScoreHistogram.load_state_dict: mantissa_bits {m!r} of the saved state differs from this histogram's "
                               f"{self.mantissa_bits}")
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
        hip.calls["hist_accumulate"] = hip.calls.get("hist_accumulate", 0) + 1

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
        if not isinstance(other, ScoreHistogram):
            raise hip.VadError(f"ScoreHistogram.merge: other must be a ScoreHistogram, got {type(other).__name__}")
        if other.mantissa_bits != self.mantissa_bits:
            raise hip.VadError(f"ScoreHistogram.merge: mantissa_bits differ ({self.mantissa_bits} and {other.mantissa_bits}); bins of "
                               "different widths cannot be added")
        if other is self:
            raise hip.VadError("ScoreHistogram.merge: other is this histogram")
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
def _as_counts(counts) -> Tuple[np.ndarray, np.ndarray, int]:
    """-> (neg int64 [nbins], pos int64 [nbins], mantissa_bits)."""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"counts must be an integer array [2, nbins], got {c.dtype} {c.shape}")
    m = next((k for k in range(MIN_MANTISSA_BITS, MAX_MANTISSA_BITS + 1) if 255 << k == c.shape[1]), None)
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
