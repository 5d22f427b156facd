"""Cost of the score histogram (developer tool; not part of the product path).  `ScoreHistogram.accumulate` on a
`--frames` x 1 x S x S map (default 512 x 256 x 256) with float32 masks, for three kinds of values, alternated in one run:

  real      the error maps `score_all` of the seeded ConvAutoencoder writes for `synth` frames with anomalies (masks = the
            saturated patches): the concentrated distribution the kernel's combining is for;
  uniform   uniform random values in [0, 4): ~20 k populated (bin, class) pairs, more than a work-group's table holds;
  constant  one value: every element into one counter.

Each time stands beside (1) the HBM floor of reading 8 bytes per element at --hbm-tbps (6.29), (2) the time
of `score_all` on the same batch, measured in the same run, and (3) the host route the histogram replaces - map and mask
`.cpu()`, then the `np.argsort`-based `scoring.roc_auc` - on `--host-frames` frames, scaled per frame.  Device-event timing
around back-to-back calls after warm-up; the variants alternate `--repeats` times, best and worst are reported.  The counts of the
real case are checked against numpy first.  Prints one JSON line and writes it to --out.

    python tools/pixel_metrics_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/pixel_metrics_bench.json]
"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
vad = importlib.import_module("video-anomaly-detection_amd")


def timed(fn, iters: int, warmup: int) -> float:
    """ms per call: device events around `iters` calls on the current stream."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(fns: dict, repeats: int, run) -> dict:
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(run(fn))
    return {k: (min(v), max(v)) for k, v in ms.items()}


def numpy_counts(values: np.ndarray, pos: np.ndarray, m: int) -> np.ndarray:
    bits = values.reshape(-1).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    ok = bits < 0x7F800000
    key, pos = bits >> np.uint32(23 - m), pos.reshape(-1)
    return np.stack([np.bincount(key[ok & (pos == c)], minlength=255 << m) for c in (False, True)]).astype(np.int64)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--mantissa-bits", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--host-frames", type=int, default=8, help="frames of the host route (its rank loop is Python: ~1 us per pixel)")
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "pixel_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_metrics_bench needs a GPU: a time is measured on the device or not at all")
    n, S, m = args.frames, args.size, args.mantissa_bits

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)
    mask = (x == 1.0).all(dim=1, keepdim=True).float()                     # the saturated patches of the labelled frames
    gen = torch.Generator(device="cuda").manual_seed(2)
    with torch.no_grad():
        maps = {"real": model.score_all(x)["errmap"].clone(),
                "uniform": torch.rand(n, 1, S, S, device="cuda", generator=gen) * 4.0,
                "constant": torch.full((n, 1, S, S), 0.25, device="cuda")}
    elems = n * S * S
    out = {"tool": "pixel_metrics_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "mantissa_bits": m,
           "elements": elems, "anomalous_pixels": int(mask.sum()), "iters": args.iters, "repeats": args.repeats,
           "hbm_tbps": args.hbm_tbps, "hbm_floor_us": round(8 * elems / (args.hbm_tbps * 1e12) * 1e6, 2), "accumulate": {}}

    # the counts are those of numpy (real case, whole batch), and the metric is within its own bound of the exact one on a slice
    hist = vad.metrics.ScoreHistogram(m)
    hist.accumulate(maps["real"], mask)
    want = numpy_counts(maps["real"].cpu().numpy(), mask.cpu().numpy() > 0.5, m)
    got = hist.counts_host()
    assert np.array_equal(got, want), "the histogram's counts differ from numpy's"
    auroc, tie_bound = vad.metrics.auroc_from_counts(got)
    out["real_auroc"], out["real_tie_bound"] = auroc, tie_bound
    out["real_populated_bins"] = int(np.count_nonzero(got))
    out["uniform_populated_bins"] = int(np.count_nonzero(numpy_counts(maps["uniform"].cpu().numpy(), mask.cpu().numpy() > 0.5, m)))

    with torch.no_grad():
        fns = {k: (lambda v=v: hist.accumulate(v, mask)) for k, v in maps.items()}
        fns["score_all"] = lambda: model.score_all(x)
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    score_ms = r.pop("score_all")
    out["score_all_ms"], out["score_all_ms_max"] = round(score_ms[0], 4), round(score_ms[1], 4)
    for k, (lo, hi) in r.items():
        out["accumulate"][k] = {"ms": round(lo, 4), "ms_max": round(hi, 4), "G_elements_per_s": round(elems / lo / 1e6, 2),
                                "hbm_floor_fraction": round(out["hbm_floor_us"] / (lo * 1e3), 4),
                                "of_score_all": round(lo / score_ms[0], 4)}

    # the one host read of an evaluation: the counters
    t0 = time.perf_counter()
    hist.counts_host()
    out["counters_read_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["counters_bytes"] = 16 * (255 << m)

    # the host route: copy map and mask, sort
    k = max(1, min(args.host_frames, n))
    host = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv, hm = maps["real"][:k].cpu().numpy().reshape(-1), mask[:k].cpu().numpy().reshape(-1) > 0.5
        t1 = time.perf_counter()
        exact = vad.scoring.roc_auc(hm, hv)
        host.append((time.perf_counter() - t0, t1 - t0))
    best = min(host)
    sub = vad.metrics.ScoreHistogram(m).accumulate(maps["real"][:k], mask[:k]).auroc()
    assert abs(sub[0] - exact) <= sub[1] + 1e-12, "the quantised AUROC is outside its own bound"
    out["host_route"] = {"frames": k, "ms_per_frame": round(best[0] * 1e3 / k, 3), "copy_ms_per_frame": round(best[1] * 1e3 / k, 3),
                         "ms_for_the_batch_scaled": round(best[0] * 1e3 / k * n, 1), "auroc_exact": exact, "auroc_hist": sub[0],
                         "tie_bound": sub[1]}
    out["accumulate_real_us_per_frame"] = round(out["accumulate"]["real"]["ms"] * 1e3 / n, 4)
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
