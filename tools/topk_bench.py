"""Cost of the robust frame scores (developer tool; not part of the product path).  `metrics.map_topk` on the error maps `score_all`
of the seeded ConvAutoencoder writes for `--frames` x S x S `synth` frames (default 512 x 256 x 256), at the ranks 1, 0.1 %, 1 %,
10 % of the frame and P (all of it) - each rank in a call of its own ("cells") and all five in one call -, and eight ranks in one
call beside eight calls of one.

Each cell stands beside (1) the HBM floor of 4 bytes per element (one read of the maps) at --hbm-tbps (6.29),
(2) `score_all` on the same batch, (3) the torch compositions on the device - `torch.topk(maps.flatten(1), k).values.mean(1)` for
the top-k mean and `torch.kthvalue` for the order statistic -, all alternated in one run, and (4) the host route the kernel
replaces - `.cpu()` + `np.partition` - on `--host-frames` frames, scaled.  Device-event timing around back-to-back calls after
warm-up; the candidates alternate `--repeats` times, best and worst are reported.  The kernel's results are checked first: `kth`
equal to `torch.kthvalue`'s, `mean` against a float64 mean of the sorted frame on the host frames.  A last section times one
3840 x 2160 frame (above `vad_topk_plan`'s boundary: split into slices over six launches).  Prints one JSON line and writes it to --out.

    python tools/topk_bench.py [--frames 512] [--size 256] [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/topk_bench.json]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "topk_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a GPU: a time is measured on the device or not at all")
    if args.repeats < 3:
        raise SystemExit("topk_bench: --repeats must be at least 3 (the candidates are alternated; min .. max are reported)")
    n, S = args.frames, args.size
    P = S * S
    m = vad.metrics
    ranks = {"rank_1": 1, "top_0.1%": m.rank_of_fraction(0.001, P), "top_1%": m.rank_of_fraction(0.01, P),
             "top_10%": m.rank_of_fraction(0.1, P), "all_P": P}

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)
    with torch.no_grad():
        maps = model.score_all(x)["errmap"].clone()
    flat = maps.flatten(1)
    elems = n * P
    out = {"tool": "topk_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "ranks": ranks, "elements": elems,
           "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps,
           "hbm_floor_us": round(4 * elems / (args.hbm_tbps * 1e12) * 1e6, 2), "cells": {}}

    # checks first: kth against torch.kthvalue on every frame, mean against a float64 mean of the sorted host frames
    all_ranks = list(ranks.values())
    got = m.map_topk(maps, all_ranks)
    kth, mean = got["kth"].reshape(n, -1), got["mean"].reshape(n, -1)
    for j, k in enumerate(all_ranks):
        assert torch.equal(kth[:, j], torch.kthvalue(flat, P - k + 1, dim=1).values), f"kth differs from torch.kthvalue at rank {k}"
    hk = max(1, min(args.host_frames, n))
    host = np.sort(flat[:hk].cpu().numpy().astype(np.float64), axis=1)
    worst = 0.0
    for j, k in enumerate(all_ranks):
        exact = host[:, P - k:].mean(1)
        err = np.abs(mean[:hk, j].cpu().numpy().astype(np.float64) - exact)
        bound = 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64) + P * 2.0 ** -51 * np.abs(exact)   # numpy's sum errs too
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"the top-{k} mean is outside its bound"
    out["largest_mean_error_of_bound"] = round(worst, 4)

    with torch.no_grad():
        fns = {"score_all": lambda: model.score_all(x), "map_topk/all_five": lambda: m.map_topk(maps, all_ranks)}
        for name, k in ranks.items():
            fns[f"map_topk/{name}"] = lambda k=k: m.map_topk(maps, k)
            fns[f"torch_topk_mean/{name}"] = lambda k=k: torch.topk(flat, k, dim=1).values.mean(1)
            fns[f"torch_kthvalue/{name}"] = lambda k=k: torch.kthvalue(flat, P - k + 1, dim=1).values
        eight = [ranks["top_1%"] + 7 * j for j in range(8)]
        fns["map_topk/eight_in_one_call"] = lambda: m.map_topk(maps, eight)
        fns["map_topk/eight_calls"] = lambda: [m.map_topk(maps, k) for k in eight]
        res = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    score_ms = res.pop("score_all")
    out["score_all_ms"], out["score_all_ms_max"] = round(score_ms[0], 4), round(score_ms[1], 4)
    pair = lambda v: {"ms": round(v[0], 4), "ms_max": round(v[1], 4)}
    beats = True
    for name in list(ranks) + ["all_five"]:
        ours = res[f"map_topk/{name}"]
        cell = dict(pair(ours), hbm_floor_fraction=round(out["hbm_floor_us"] / (ours[0] * 1e3), 4), of_score_all=round(ours[0] / score_ms[0], 4))
        if name in ranks:
            for other in ("torch_topk_mean", "torch_kthvalue"):
                t = res[f"{other}/{name}"]
                cell[other] = dict(pair(t), over_kernel=round(t[0] / ours[0], 2), kernel_wins_beyond_spread=bool(ours[1] < t[0]))
                beats = beats and ours[1] < t[0]
        out["cells"][name] = cell
    out["kernel_beats_torch_in_every_cell"] = bool(beats)
    one, calls = res["map_topk/eight_in_one_call"], res["map_topk/eight_calls"]
    out["eight_ranks"] = {"one_call": pair(one), "eight_calls": pair(calls), "calls_over_one": round(calls[0] / one[0], 2)}

    # the host route: copy the maps, np.partition
    host_t = []
    k1 = ranks["top_1%"]
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv = flat[:hk].cpu().numpy()
        t1 = time.perf_counter()
        scores = [float(np.partition(f, P - k1)[P - k1:].astype(np.float64).mean()) for f in hv]
        host_t.append((time.perf_counter() - t0, t1 - t0))
    best = min(host_t)
    out["host_route"] = {"frames": hk, "ms_per_frame": round(best[0] * 1e3 / hk, 3), "copy_ms_per_frame": round(best[1] * 1e3 / hk, 3),
                         "ms_for_the_batch_scaled": round(best[0] * 1e3 / hk * n, 1), "first_score": scores[0]}
    out["topk_us_per_frame"] = round(out["cells"]["top_1%"]["ms"] * 1e3 / n, 4)

    # one 4K frame: above the split boundary, 254 slices
    h4, w4 = 2160, 3840
    big = torch.rand(1, h4, w4, device="cuda").square_()
    k4 = [1, m.rank_of_fraction(0.01, h4 * w4), h4 * w4]
    g4 = m.map_topk(big, k4)
    assert torch.equal(g4["kth"][0, 0], big.max()) and torch.equal(g4["kth"][0, 2], big.min())
    r4 = alternate({"one": lambda: m.map_topk(big, k4[1]), "three": lambda: m.map_topk(big, k4),
                    "torch_topk_mean": lambda: torch.topk(big.flatten(1), k4[1], dim=1).values.mean(1)},
                   args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    out["frame_4k"] = {"h": h4, "w": w4, "rank": k4[1], "one_rank": pair(r4["one"]), "three_ranks": pair(r4["three"]),
                       "torch_topk_mean": pair(r4["torch_topk_mean"])}
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
