"""Cost of the defect-region table (developer tool; not part of the product path).  `vad_detect_regions` on `--frames` x S x S maps
(default 512 x 256 x 256) of three kinds, alternated in one run:

  sparse    low noise with four discs above the threshold per frame: a few regions, the deployed case
  speckle   uniform noise with 15 % of the pixels above the threshold: thousands of regions per frame, most below min_area = 16
  full      every pixel above the threshold: one region per frame - every pixel of a frame meets in one record (atomic contention)

beside, in the same alternation,

  pro        `ProHistogram.accumulate` on the sparse maps with their own foreground as masks
  score_all  the scoring call of the seeded ConvAutoencoder on as many `synth` frames
  api        `metrics.detect_regions` on the sparse maps: the call above plus its allocations and the read of the flag word
  label_*    `vad_label_regions` alone on the foreground of each kind (init, merge, flatten: the passes the call shares with the
             per-region overlap); the table's own passes - count, slot, reduce, finish - are detect - label by difference

and the floor of reading the maps once at --hbm-tbps (6.29).  The host route it replaces - `.cpu()`,
`scipy.ndimage.label`, `find_objects`, `maximum_position` per frame - runs on `--host-frames` frames of every kind and is scaled
per frame (skipped, with a note, where scipy is missing); the device's table of those frames is checked against it first.
Device-event timing around back-to-back calls after warm-up; variants alternate `--repeats` times, best and worst are reported.
Prints one JSON line and writes it to --out.

    python tools/regions_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/regions_bench.json]
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
from pixel_metrics_bench import alternate, timed  # noqa: E402

THRESHOLD = 0.5
KINDS = {"sparse": 1, "speckle": 16, "full": 1}                            # kind -> min_area


def make_maps(kind: str, n: int, s: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "full":
        return 0.5 + torch.rand((n, s, s), generator=g, device="cuda")
    if kind == "speckle":
        return torch.rand((n, s, s), generator=g, device="cuda") * (THRESHOLD / 0.85)     # 15 % of the pixels reach the threshold
    maps = torch.rand((n, s, s), generator=g, device="cuda") * 0.2
    yy, xx = torch.meshgrid(torch.arange(s, device="cuda"), torch.arange(s, device="cuda"), indexing="ij")
    for _ in range(4):
        cy = torch.randint(0, s, (n, 1, 1), generator=g, device="cuda")
        cx = torch.randint(0, s, (n, 1, 1), generator=g, device="cuda")
        r = torch.randint(3, max(4, s // 20), (n, 1, 1), generator=g, device="cuda")
        disc = (yy[None] - cy) ** 2 + (xx[None] - cx) ** 2 <= r * r
        maps = torch.where(disc, 1.0 + torch.rand((n, s, s), generator=g, device="cuda"), maps)
    return maps


def host_table(maps: np.ndarray, min_area: int):
    """scipy per frame -> list of [(root, area, (x0, y0, x1, y1), peak index)] in label order, or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    out = []
    w = maps.shape[2]
    for frame in maps:
        lab, count = ndimage.label(frame >= np.float32(THRESHOLD), structure=np.ones((3, 3), int))
        index = np.arange(1, count + 1)
        boxes = ndimage.find_objects(lab)
        area = np.bincount(lab.reshape(-1), minlength=count + 1)[1:]
        peaks = ndimage.maximum_position(frame, lab, index) if count else []
        first = ndimage.minimum_position(np.arange(frame.size).reshape(frame.shape), lab, index) if count else []
        out.append([(fy * w + fx, int(area[k]), (boxes[k][1].start, boxes[k][0].start, boxes[k][1].stop - 1, boxes[k][0].stop - 1), py * w + px)
                    for k, ((py, px), (fy, fx)) in enumerate(zip(peaks, first)) if area[k] >= min_area])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-regions", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "regions_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regions_bench needs a GPU: a time is measured on the device or not at all")
    n, S, R = args.frames, args.size, args.max_regions
    elems = n * S * S
    lib = vad.hip.lib()

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)

    maps = {k: make_maps(k, n, S, args.seed + i) for i, k in enumerate(KINDS)}
    need = lib.vad_regions_workspace_bytes(n, S, S, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    records = torch.empty((n, R, vad.hip.REGION_WORDS), dtype=torch.int32, device="cuda")
    counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    out = {"tool": "regions_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "elements": elems, "threshold": THRESHOLD,
           "connectivity": 8, "max_regions": R, "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps,
           "workspace_bytes": need, "floor_read_maps_once_us": round(4 * elems / (args.hbm_tbps * 1e12) * 1e6, 2)}

    def detect(kind):
        vad.hip.check(lib.vad_detect_regions(maps[kind].data_ptr(), n, S, S, THRESHOLD, 8, KINDS[kind], R, None, records.data_ptr(), counts.data_ptr(),
                                             ws.data_ptr(), need, vad.hip.current_stream()), "vad_detect_regions")

    # what the maps hold, and the table of the first frames against scipy
    k = max(1, min(args.host_frames, n))
    host = {}
    for kind, min_area in KINDS.items():
        detect(kind)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the labelling kernels set their flag word"
        c = counts.cpu().numpy().astype(np.int64)
        out[kind] = {"min_area": min_area, "kept_per_frame": round(float(c[:, 0].mean()), 2), "dropped_per_frame": round(float(c[:, 1].mean()), 2),
                     "foreground_share": round(float(c[:, 2].sum()) / elems, 4), "truncated_frames": int((c[:, 0] > R).sum())}
        rec = records[:k].cpu().numpy()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv = maps[kind][:k].cpu().numpy()
            t1 = time.perf_counter()
            table = host_table(hv, min_area)
            times.append((time.perf_counter() - t0, t1 - t0))
        if table is None:
            host[kind] = "skipped: scipy is not installed"
            continue
        for f in range(k):
            assert len(table[f]) == c[f, 0], "the kept regions differ from scipy's"
            for j, (root, area, box, peak) in enumerate(table[f][:R]):
                assert (root, area, box, peak) == (int(rec[f, j, 0]), int(rec[f, j, 1]), tuple(int(v) for v in rec[f, j, 2:6]), int(rec[f, j, 7])), \
                    "a record differs from scipy's"
        best = min(times)
        host[kind] = {"frames": k, "ms_per_frame": round(best[0] * 1e3 / k, 3), "copy_ms_per_frame": round(best[1] * 1e3 / k, 3),
                      "ms_for_the_batch_scaled": round(best[0] * 1e3 / k * n, 1)}
    out["host_route"] = host

    sparse_mask = (maps["sparse"] >= THRESHOLD).float()
    label_ws = torch.empty(lib.vad_pro_workspace_bytes(n, S, S), dtype=torch.uint8, device="cuda")
    label_out = torch.empty((2, n, S, S), dtype=torch.int32, device="cuda")

    def label_only(kind):
        vad.hip.check(lib.vad_label_regions(masks[kind].data_ptr(), vad.hip.LBL_F32_ELEM, n, S, S, 8, label_out[0].data_ptr(), label_out[1].data_ptr(),
                                            label_ws.data_ptr(), label_ws.numel(), vad.hip.current_stream()), "vad_label_regions")

    masks = {"sparse": sparse_mask, "speckle": (maps["speckle"] >= THRESHOLD).float(), "full": (maps["full"] >= THRESHOLD).float()}
    pro = vad.metrics.ProHistogram(11)
    with torch.no_grad():
        fns = {kind: (lambda kind=kind: detect(kind)) for kind in KINDS}
        fns["pro"] = lambda: pro.accumulate(maps["sparse"], sparse_mask)
        fns["score_all"] = lambda: model.score_all(x)
        fns["api"] = lambda: vad.metrics.detect_regions(maps["sparse"], THRESHOLD, 8, 1, R)
        fns.update({f"label_{kind}": (lambda kind=kind: label_only(kind)) for kind in KINDS})
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    for key, (lo, hi) in r.items():
        out[f"{key}_ms"], out[f"{key}_ms_max"] = round(lo, 4), round(hi, 4)
    for kind in KINDS:
        out[f"{kind}_of_score_all"] = round(r[kind][0] / r["score_all"][0], 4)
        out[f"{kind}_floor_fraction"] = round(out["floor_read_maps_once_us"] / (r[kind][0] * 1e3), 4)
        out[f"{kind}_us_per_frame"] = round(r[kind][0] * 1e3 / n, 4)
        out[f"{kind}_table_ms_by_difference"] = round(r[kind][0] - r[f"label_{kind}"][0], 4)
        if isinstance(host[kind], dict):
            out[f"{kind}_host_over_device"] = round(host[kind]["ms_for_the_batch_scaled"] / r[kind][0], 1)
    out["sparse_of_pro"] = round(r["sparse"][0] / r["pro"][0], 3)
    out["full_of_sparse"] = round(r["full"][0] / r["sparse"][0], 3)
    out["speckle_of_sparse"] = round(r["speckle"][0] / r["sparse"][0], 3)
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
