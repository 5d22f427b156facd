"""Cost of the event table (developer tool; not part of the product path).  `vad_detect_events` on `--clips` clips of `--frames`
frames of S x S maps (default 32 x 16 x 256 x 256: the 512 maps of tools/regions_bench.py) of three kinds, alternated in one run:

  sparse    low noise with four discs above the threshold per clip, each drifting one pixel per frame: a few long events
  speckle   uniform noise with 5 % of the pixels above the threshold (15 %, the speckle of regions_bench, percolates under the
            26-structure: one event), min_duration = 3: tens of thousands of events per clip, nearly all shorter than the filter
  full      every pixel above the threshold: one event per clip - every pixel of a clip chases one root and meets in one record

beside, in the same alternation,

  regions_*  `vad_detect_regions` on the same 512 maps, every frame on its own
  label_*    `vad_label_regions` alone on the foreground of each kind: the labelling inside the frames that all three share; the
             passes this table adds - rebase, link, flatten, count, slot, reduce, finish - are events - label by difference
  score_all  the scoring call of the seeded ConvAutoencoder on as many `synth` frames
  api        `metrics.detect_events` on the sparse maps: the call above plus its allocations and the read of the flag word

and the floor of reading the maps once at --hbm-tbps (6.29).  The host route it replaces - `.cpu()` of a clip,
3-D `scipy.ndimage.label` with the 26-structure, `find_objects`, `maximum_position` - runs on the first clip of every kind and is
scaled per clip (skipped, with a note, where scipy is missing); the device's table of that clip is checked against it first.
Device-event timing around back-to-back calls after warm-up; variants alternate `--repeats` times, best and worst are reported.
Prints one JSON line and writes it to --out.

    python tools/events_bench.py [--clips 32] [--frames 16] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/events_bench.json]
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
KINDS = {"sparse": 1, "speckle": 3, "full": 1}                             # kind -> min_duration


def make_maps(kind: str, b: int, t: int, s: int, seed: int) -> torch.Tensor:
    g = torch.Generator(device="cuda").manual_seed(seed)
    if kind == "full":
        return 0.5 + torch.rand((b, t, s, s), generator=g, device="cuda")
    if kind == "speckle":
        return torch.rand((b, t, s, s), generator=g, device="cuda") * (THRESHOLD / 0.95)   # 5 % of the pixels reach the threshold
    maps = torch.rand((b, t, s, s), generator=g, device="cuda") * 0.2
    yy, xx = torch.meshgrid(torch.arange(s, device="cuda"), torch.arange(s, device="cuda"), indexing="ij")
    drift = torch.arange(t, device="cuda").view(1, t, 1, 1)
    for _ in range(4):
        cy = torch.randint(0, s, (b, 1, 1, 1), generator=g, device="cuda") + drift
        cx = torch.randint(0, s, (b, 1, 1, 1), generator=g, device="cuda") + drift
        r = torch.randint(3, max(4, s // 20), (b, 1, 1, 1), generator=g, device="cuda")
        disc = (yy[None, None] - cy) ** 2 + (xx[None, None] - cx) ** 2 <= r * r
        maps = torch.where(disc, 1.0 + torch.rand((b, t, s, s), generator=g, device="cuda"), maps)
    return maps


def host_table(clip: np.ndarray, min_duration: int):
    """scipy on one clip -> [(root, volume, t0, t1, (x0, y0, x1, y1), peak index)] in label order, or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    lab, count = ndimage.label(clip >= np.float32(THRESHOLD), structure=np.ones((3, 3, 3), int))
    index = np.arange(1, count + 1)
    boxes = ndimage.find_objects(lab)
    volume = np.bincount(lab.reshape(-1), minlength=count + 1)[1:]
    peaks = ndimage.maximum_position(clip, lab, index) if count else []
    first = np.full(count + 1, clip.size, np.int64)
    np.minimum.at(first, lab.reshape(-1), np.arange(clip.size))
    _, h, w = clip.shape
    return [(int(first[k + 1]), int(volume[k]), bx[0].start, bx[0].stop - 1, (bx[2].start, bx[1].start, bx[2].stop - 1, bx[1].stop - 1),
             (pk[0] * h + pk[1]) * w + pk[2]) for k, (bx, pk) in enumerate(zip(boxes, peaks)) if bx[0].stop - bx[0].start >= min_duration]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-events", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "events_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("events_bench needs a GPU: a time is measured on the device or not at all")
    b, t, S, E = args.clips, args.frames, args.size, args.max_events
    n = b * t
    elems = n * S * S
    lib = vad.hip.lib()

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)

    maps = {k: make_maps(k, b, t, S, args.seed + i) for i, k in enumerate(KINDS)}
    need = lib.vad_events_workspace_bytes(b, t, S, S, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    records = torch.empty((b, E, vad.hip.EVENT_WORDS), dtype=torch.int32, device="cuda")
    counts = torch.empty((b, 4), dtype=torch.int32, device="cuda")
    frame_counts = torch.empty((b, t, 3), dtype=torch.int32, device="cuda")
    out = {"tool": "events_bench", "device": torch.cuda.get_device_name(0), "clips": b, "frames_per_clip": t, "size": S, "elements": elems,
           "threshold": THRESHOLD, "connectivity": 8, "temporal": 9, "max_events": E, "iters": args.iters, "repeats": args.repeats,
           "hbm_tbps": args.hbm_tbps, "workspace_bytes": need, "floor_read_maps_once_us": round(4 * elems / (args.hbm_tbps * 1e12) * 1e6, 2)}

    def detect(kind):
        vad.hip.check(lib.vad_detect_events(maps[kind].data_ptr(), b, t, S, S, THRESHOLD, 8, 9, KINDS[kind], 1, E, None, records.data_ptr(),
                                            counts.data_ptr(), frame_counts.data_ptr(), ws.data_ptr(), need, vad.hip.current_stream()),
                      "vad_detect_events")

    # what the maps hold, and the table of the first clip against scipy
    host = {}
    for kind, min_duration in KINDS.items():
        detect(kind)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the labelling kernels set their flag word"
        c = counts.cpu().numpy().astype(np.int64)
        fc = frame_counts.cpu().numpy().astype(np.int64)
        out[kind] = {"min_duration": min_duration, "kept_per_clip": round(float(c[:, 0].mean()), 2), "dropped_per_clip": round(float(c[:, 1].mean()), 2),
                     "foreground_share": round(float(c[:, 2].sum()) / elems, 4), "truncated_clips": int((c[:, 0] > E).sum()),
                     "alarmed_frames_share": round(float((fc[..., 1] > 0).mean()), 4)}
        rec = records[0].cpu().numpy()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv = maps[kind][0].cpu().numpy()
            t1 = time.perf_counter()
            table = host_table(hv, min_duration)
            times.append((time.perf_counter() - t0, t1 - t0))
        if table is None:
            host[kind] = "skipped: scipy is not installed"
            continue
        assert len(table) == c[0, 0], "the kept events differ from scipy's"
        for j, (root, volume, f0, f1, box, peak) in enumerate(table[:E]):
            assert (root, volume, f0, f1, box, peak) == (int(rec[j, 0]), int(rec[j, 1]), int(rec[j, 2]), int(rec[j, 3]),
                                                         tuple(int(v) for v in rec[j, 4:8]), int(rec[j, 9])), "a record differs from scipy's"
        best = min(times)
        host[kind] = {"clips": 1, "ms_per_clip": round(best[0] * 1e3, 3), "copy_ms_per_clip": round(best[1] * 1e3, 3),
                      "ms_for_the_batch_scaled": round(best[0] * 1e3 * b, 1)}
    out["host_route"] = host

    flat = {k: v.view(n, S, S) for k, v in maps.items()}
    masks = {k: (v >= THRESHOLD).float() for k, v in flat.items()}
    label_ws = torch.empty(lib.vad_pro_workspace_bytes(n, S, S), dtype=torch.uint8, device="cuda")
    label_out = torch.empty((2, n, S, S), dtype=torch.int32, device="cuda")
    reg_need = lib.vad_regions_workspace_bytes(n, S, S, 0)
    reg_ws = torch.empty(reg_need, dtype=torch.uint8, device="cuda")
    reg_records = torch.empty((n, E, vad.hip.REGION_WORDS), dtype=torch.int32, device="cuda")
    reg_counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")

    def label_only(kind):
        vad.hip.check(lib.vad_label_regions(masks[kind].data_ptr(), vad.hip.LBL_F32_ELEM, n, S, S, 8, label_out[0].data_ptr(), label_out[1].data_ptr(),
                                            label_ws.data_ptr(), label_ws.numel(), vad.hip.current_stream()), "vad_label_regions")

    def regions(kind):
        vad.hip.check(lib.vad_detect_regions(flat[kind].data_ptr(), n, S, S, THRESHOLD, 8, 1, E, None, reg_records.data_ptr(), reg_counts.data_ptr(),
                                             reg_ws.data_ptr(), reg_need, vad.hip.current_stream()), "vad_detect_regions")

    with torch.no_grad():
        fns = {kind: (lambda kind=kind: detect(kind)) for kind in KINDS}
        fns.update({f"regions_{kind}": (lambda kind=kind: regions(kind)) for kind in KINDS})
        fns.update({f"label_{kind}": (lambda kind=kind: label_only(kind)) for kind in KINDS})
        fns["score_all"] = lambda: model.score_all(x)
        fns["api"] = lambda: vad.metrics.detect_events(maps["sparse"], THRESHOLD, 8, 9, 1, 1, E)
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    for key, (lo, hi) in r.items():
        out[f"{key}_ms"], out[f"{key}_ms_max"] = round(lo, 4), round(hi, 4)
    for kind in KINDS:
        out[f"{kind}_of_score_all"] = round(r[kind][0] / r["score_all"][0], 4)
        out[f"{kind}_of_detect_regions"] = round(r[kind][0] / r[f"regions_{kind}"][0], 3)
        out[f"{kind}_floor_fraction"] = round(out["floor_read_maps_once_us"] / (r[kind][0] * 1e3), 4)
        out[f"{kind}_us_per_clip"] = round(r[kind][0] * 1e3 / b, 4)
        out[f"{kind}_new_passes_ms_by_difference"] = round(r[kind][0] - r[f"label_{kind}"][0], 4)
        if isinstance(host[kind], dict):
            out[f"{kind}_host_over_device"] = round(host[kind]["ms_for_the_batch_scaled"] / r[kind][1], 1)   # fastest host, slowest device
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
