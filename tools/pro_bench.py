"""Cost of the per-region overlap (developer tool; not part of the product path).  On the error maps `score_all` of the seeded
ConvAutoencoder writes for `--frames` x S x S `synth` frames with anomalies (default 512 x 256 x 256; masks = the saturated
patches, float32), alternated in one run:

  pro         `ProHistogram.accumulate`: labelling + the region-weighted histogram (one `vad_pro_accumulate` call)
  label       `vad_label_regions` alone into the same workspace (init, merge, flatten); the histogram's share is pro - label
  hist        `ScoreHistogram.accumulate` on the same maps and masks
  score_all   the scoring call that wrote the maps

beside two floors at --hbm-tbps (6.29): the compulsory 8 bytes per element (map and mask read once), and the
bytes the three labelling passes and the histogram pass move as built (28 per element: mask 4, label plane written 4 and read 3 x 4,
size plane written 4, map 4; the writes and reads at anomalous pixels on top).  The host route it replaces - map and mask
`.cpu()`, `scipy.ndimage.label` per frame, a sort - runs on `--host-frames` frames and is scaled per frame (skipped, with a
note, where scipy is missing).  The state of the whole batch is checked against numpy + the host labelling first.  Device-event
timing around back-to-back calls after warm-up; variants alternate `--repeats` times, best and worst are reported.  Prints one
JSON line and writes it to --out.

    python tools/pro_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/pro_bench.json]
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
sys.path.insert(0, str(REPO / "tools"))
vad = importlib.import_module("video-anomaly-detection_amd")
from pixel_metrics_bench import alternate, numpy_counts, timed  # noqa: E402


def host_aupro(values: np.ndarray, pos: np.ndarray, limit: float):
    """AUPRO on the host from the definition: scipy labels per frame, one sort.  -> (aupro, regions) or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    weights, regions = np.zeros(values.shape, np.float64), 0
    for i in range(len(values)):
        lab, count = ndimage.label(pos[i], structure=np.ones((3, 3), int))
        sizes = np.bincount(lab.reshape(-1), minlength=count + 1)
        weights[i] = np.where(lab > 0, 1.0 / np.maximum(sizes[lab], 1), 0.0)
        regions += count
    v, p, w = values.reshape(-1), pos.reshape(-1), weights.reshape(-1)
    order = np.argsort(-v, kind="stable")
    v, p, w = v[order], p[order], w[order]
    last = np.flatnonzero(np.append(v[1:] != v[:-1], True))               # the last element of every run of equal scores
    fpr = np.concatenate([[0.0], np.cumsum(~p)[last] / float((~p).sum())])
    pro = np.concatenate([[0.0], np.cumsum(w)[last] / regions])
    k = int(np.flatnonzero(fpr <= limit)[-1])
    area = float(np.sum(np.diff(fpr[:k + 1]) * (pro[1:k + 1] + pro[:k]) * 0.5))
    if fpr[k] < limit:
        cut = pro[k] + (pro[k + 1] - pro[k]) * (limit - fpr[k]) / (fpr[k + 1] - fpr[k])
        area += (limit - fpr[k]) * (pro[k] + cut) * 0.5
    return area / limit, regions


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--mantissa-bits", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--fpr-limit", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "pro_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pro_bench needs a GPU: a time is measured on the device or not at all")
    n, S, m = args.frames, args.size, args.mantissa_bits

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)
    mask = (x == 1.0).all(dim=1, keepdim=True).float()                     # the saturated patches of the labelled frames
    with torch.no_grad():
        errmap = model.score_all(x)["errmap"].clone()
    elems = n * S * S
    out = {"tool": "pro_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "mantissa_bits": m, "elements": elems,
           "anomalous_pixels": int(mask.sum()), "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps,
           "floor_compulsory_us": round(8 * elems / (args.hbm_tbps * 1e12) * 1e6, 2),
           "floor_as_built_us": round(28 * elems / (args.hbm_tbps * 1e12) * 1e6, 2)}

    # the state of the whole batch against numpy: the plain counters, the region count and the largest region
    pro = vad.metrics.ProHistogram(m)
    pro.accumulate(errmap, mask)
    labels, sizes = vad.metrics.label_regions(mask)
    sizes = sizes.view(torch.int32)                                        # region sizes are far below 2^31
    pos = mask.cpu().numpy()[:, 0] > 0.5
    assert np.array_equal(pro.counts().cpu().numpy(), numpy_counts(errmap.cpu().numpy(), pos, m)), "the plain counters differ from numpy's"
    assert pro.regions() == int((sizes != 0).sum()) and pro.max_region() == int(sizes.max()) and pro.flags() == 0
    assert torch.equal(labels != 0, mask[:, 0] > 0.5) and int(sizes.sum()) == int(pos.sum())
    aupro, quant_bound, weight_bound = pro.aupro(args.fpr_limit)
    out.update(regions=pro.regions(), max_region=pro.max_region(), fpr_limit=args.fpr_limit, aupro=aupro, quant_bound=quant_bound,
               weight_bound=weight_bound, auroc=pro.auroc()[0])

    hist = vad.metrics.ScoreHistogram(m)
    lib, ws, planes = vad.hip.lib(), pro._ws, mask[:, 0].contiguous()
    label_out = torch.empty((n, S, S), dtype=torch.int32, device="cuda")
    size_out = torch.empty((n, S, S), dtype=torch.int32, device="cuda")

    def label_only():
        vad.hip.check(lib.vad_label_regions(planes.data_ptr(), vad.hip.LBL_F32_ELEM, n, S, S, 8, label_out.data_ptr(), size_out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), vad.hip.current_stream()), "vad_label_regions")

    with torch.no_grad():
        fns = {"pro": lambda: pro.accumulate(errmap, mask), "label": label_only, "hist": lambda: hist.accumulate(errmap, mask),
               "score_all": lambda: model.score_all(x)}
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    assert pro.flags() == 0
    for k, (lo, hi) in r.items():
        out[f"{k}_ms"], out[f"{k}_ms_max"] = round(lo, 4), round(hi, 4)
    out["weighted_hist_ms_by_difference"] = round(r["pro"][0] - r["label"][0], 4)
    out["pro_of_score_all"] = round(r["pro"][0] / r["score_all"][0], 4)
    out["pro_of_hist"] = round(r["pro"][0] / r["hist"][0], 2)
    out["pro_floor_compulsory_fraction"] = round(out["floor_compulsory_us"] / (r["pro"][0] * 1e3), 4)
    out["pro_floor_as_built_fraction"] = round(out["floor_as_built_us"] / (r["pro"][0] * 1e3), 4)
    out["pro_us_per_frame"] = round(r["pro"][0] * 1e3 / n, 4)

    t0 = time.perf_counter()
    pro._host()
    out["counters_read_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["counters_bytes"] = pro._state.numel()

    # the host route: copy map and mask, label every frame, sort
    k = max(1, min(args.host_frames, n))
    host, exact = [], None
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv, hm = errmap[:k].cpu().numpy()[:, 0], mask[:k].cpu().numpy()[:, 0] > 0.5
        t1 = time.perf_counter()
        exact = host_aupro(hv, hm, args.fpr_limit)
        host.append((time.perf_counter() - t0, t1 - t0))
    if exact is None:
        out["host_route"] = "skipped: scipy is not installed"
    else:
        best = min(host)
        sub = vad.metrics.ProHistogram(m).accumulate(errmap[:k], mask[:k]).aupro(args.fpr_limit)
        assert abs(sub[0] - exact[0]) <= sub[1] + sub[2] + 1e-12, "the AUPRO from counts is outside its own bounds"
        out["host_route"] = {"frames": k, "regions": exact[1], "ms_per_frame": round(best[0] * 1e3 / k, 3),
                             "copy_ms_per_frame": round(best[1] * 1e3 / k, 3), "ms_for_the_batch_scaled": round(best[0] * 1e3 / k * n, 1),
                             "aupro_exact": exact[0], "aupro_counts": sub[0], "quant_bound": sub[1], "weight_bound": sub[2]}
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
