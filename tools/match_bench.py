"""Cost of matching detections against ground-truth masks (developer tool; not part of the product path).  `vad_match_regions` on
`--frames` x S x S maps (default 512 x 256 x 256) of the three kinds of tools/regions_bench.py - sparse, speckle, full -, each with
masks of a few discs per frame, alternated in one run beside

  labels_*    the two labellings the call contains, alone: `vad_label_regions` on the uint8 masks and on the maps' foreground as an
              fp32 plane (init, merge, flatten each; the same bytes per pixel as the call's own labellings read); the join's own
              passes - zeroing the hit / overlap planes, join, count, slot, finish - are match - labels by difference, set against the floor of the bytes those passes must move (36 per pixel: 8 zeroed, 12 read by the join,
              8 each by the count and the slot scan) at --hbm-tbps
  detect_*    `vad_detect_regions` with labels plus `vad_label_regions` on the masks: what a caller had to run before to hold both
              labellings on the device - and still had no join
  score_all   the scoring call of the seeded ConvAutoencoder on as many `synth` frames
  api         `metrics.match_regions` on the sparse maps: the call plus its allocations and the read of the flag word

The host route it replaces - `.cpu()` of maps and masks, `scipy.ndimage.label` of both, `sum_labels` of one labelling under the other -
runs on `--host-frames` frames of every kind and is scaled per frame (skipped, with a note, where scipy is missing); the device's
tables of those frames are checked against it first.  Device-event timing around back-to-back calls after warm-up; variants alternate
`--repeats` times, best and worst are reported.  Prints one JSON line and writes it to --out.

    python tools/match_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/match_bench.json]
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
from regions_bench import KINDS, THRESHOLD, make_maps  # noqa: E402

JOIN_BYTES_PER_PIXEL = 36


def make_masks(n: int, s: int, seed: int) -> torch.Tensor:
    """uint8 [n, s, s], 0 / 255: three discs per frame."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(s, device="cuda"), torch.arange(s, device="cuda"), indexing="ij")
    mask = torch.zeros((n, s, s), dtype=torch.bool, device="cuda")
    for _ in range(3):
        cy = torch.randint(0, s, (n, 1, 1), generator=g, device="cuda")
        cx = torch.randint(0, s, (n, 1, 1), generator=g, device="cuda")
        r = torch.randint(3, max(4, s // 12), (n, 1, 1), generator=g, device="cuda")
        mask |= (yy[None] - cy) ** 2 + (xx[None] - cx) ** 2 <= r * r
    return mask.to(torch.uint8) * 255


def host_tables(maps: np.ndarray, masks: np.ndarray, min_area: int):
    """scipy per frame -> [(gt [(area, hit)], pred [(area, overlap)])] in label order, or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    out = []
    ones = np.ones((3, 3), int)
    for frame, mask in zip(maps, masks):
        G = mask >= 128
        plab, pcount = ndimage.label(frame >= np.float32(THRESHOLD), structure=ones)
        glab, gcount = ndimage.label(G, structure=ones)
        area = np.bincount(plab.reshape(-1), minlength=pcount + 1)
        kept = np.flatnonzero(area[1:] >= min_area) + 1
        P = np.isin(plab, kept)
        overlap = ndimage.sum_labels(G, plab, kept).astype(np.int64) if len(kept) else np.zeros(0, np.int64)
        gindex = np.arange(1, gcount + 1)
        garea = np.bincount(glab.reshape(-1), minlength=gcount + 1)[1:]
        hit = ndimage.sum_labels(P, glab, gindex).astype(np.int64) if gcount else np.zeros(0, np.int64)
        out.append((list(zip(garea.tolist(), hit.tolist())), list(zip(area[kept].tolist(), overlap.tolist()))))
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
    ap.add_argument("--out", default=str(REPO / "profiles" / "match_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_bench needs a GPU: a time is measured on the device or not at all")
    n, S, R = args.frames, args.size, args.max_regions
    elems = n * S * S
    lib = vad.hip.lib()

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)

    maps = {k: make_maps(k, n, S, args.seed + i) for i, k in enumerate(KINDS)}
    masks = make_masks(n, S, args.seed + 17)
    need = lib.vad_match_workspace_bytes(n, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gt = torch.empty((n, R, vad.hip.MATCH_WORDS), dtype=torch.int32, device="cuda")
    pred = torch.empty((n, R, vad.hip.MATCH_WORDS), dtype=torch.int32, device="cuda")
    counts = torch.empty((n, vad.hip.MATCH_COUNTS), dtype=torch.int64, device="cuda")
    out = {"tool": "match_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "elements": elems, "threshold": THRESHOLD,
           "connectivity": 8, "max_regions": R, "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps, "workspace_bytes": need,
           "mask_share": round(float((masks != 0).float().mean()), 4), "join_bytes_per_pixel": JOIN_BYTES_PER_PIXEL,
           "floor_join_passes_us": round(JOIN_BYTES_PER_PIXEL * elems / (args.hbm_tbps * 1e12) * 1e6, 2)}

    def match(kind):
        vad.hip.check(lib.vad_match_regions(maps[kind].data_ptr(), masks.data_ptr(), vad.hip.LBL_U8_ELEM, n, S, S, THRESHOLD, 8, KINDS[kind], 0.0, 0.0,
                                            R, gt.data_ptr(), pred.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, vad.hip.current_stream()),
                      "vad_match_regions")

    # what the batch holds, and the tables of the first frames against scipy
    k = max(1, min(args.host_frames, n))
    host = {}
    for kind, min_area in KINDS.items():
        match(kind)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the labelling kernels set their flag word"
        c = counts.cpu().numpy()
        sums = c.sum(0)
        out[kind] = {"min_area": min_area, "report": {key: (None if isinstance(v, float) and v != v else v)
                                                      for key, v in vad.metrics.report_from_counts(sums).items()},
                     "truncated_frames": int(((c[:, 0] > R) | (c[:, 2] > R)).sum())}
        g_rec, p_rec = gt[:k].cpu().numpy(), pred[:k].cpu().numpy()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hm = maps[kind][:k].cpu().numpy(), masks[:k].cpu().numpy()
            t1 = time.perf_counter()
            tables = host_tables(hv, hm, min_area)
            times.append((time.perf_counter() - t0, t1 - t0))
        if tables is None:
            host[kind] = "skipped: scipy is not installed"
            continue
        for f in range(k):
            assert (len(tables[f][0]), len(tables[f][1])) == (int(c[f, 0]), int(c[f, 2])), "the region counts differ from scipy's"
            assert tables[f][0][:R] == [(int(r[1]), int(r[2])) for r in g_rec[f, :min(int(c[f, 0]), R)]], "a mask region differs from scipy's"
            assert tables[f][1][:R] == [(int(r[1]), int(r[2])) for r in p_rec[f, :min(int(c[f, 2]), R)]], "a prediction differs from scipy's"
        best = min(times)
        host[kind] = {"frames": k, "ms_per_frame": round(best[0] * 1e3 / k, 3), "copy_ms_per_frame": round(best[1] * 1e3 / k, 3),
                      "ms_for_the_batch_scaled": round(best[0] * 1e3 / k * n, 1)}
    out["host_route"] = host

    # the foreground as fp32 planes: their labelling reads 4 bytes per pixel, as the call's own labelling of the fp32 maps does
    fg = {kind: (maps[kind] >= THRESHOLD).float() for kind in KINDS}
    label_ws = torch.empty(lib.vad_pro_workspace_bytes(n, S, S), dtype=torch.uint8, device="cuda")
    label_out = torch.empty((4, n, S, S), dtype=torch.int32, device="cuda")
    det_ws = torch.empty(lib.vad_regions_workspace_bytes(n, S, S, 1), dtype=torch.uint8, device="cuda")
    det_records = torch.empty((n, R, vad.hip.REGION_WORDS), dtype=torch.int32, device="cuda")
    det_counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")

    def label(src, fmt, slot):
        vad.hip.check(lib.vad_label_regions(src.data_ptr(), fmt, n, S, S, 8, label_out[slot].data_ptr(), label_out[slot + 1].data_ptr(),
                                            label_ws.data_ptr(), label_ws.numel(), vad.hip.current_stream()), "vad_label_regions")

    def labels_only(kind):
        label(masks, vad.hip.LBL_U8_ELEM, 0)
        label(fg[kind], vad.hip.LBL_F32_ELEM, 2)

    def detect_and_label(kind):
        vad.hip.check(lib.vad_detect_regions(maps[kind].data_ptr(), n, S, S, THRESHOLD, 8, KINDS[kind], R, label_out[2].data_ptr(), det_records.data_ptr(),
                                             det_counts.data_ptr(), det_ws.data_ptr(), det_ws.numel(), vad.hip.current_stream()), "vad_detect_regions")
        label(masks, vad.hip.LBL_U8_ELEM, 0)

    with torch.no_grad():
        fns = {kind: (lambda kind=kind: match(kind)) for kind in KINDS}
        fns.update({f"labels_{kind}": (lambda kind=kind: labels_only(kind)) for kind in KINDS})
        fns.update({f"detect_{kind}": (lambda kind=kind: detect_and_label(kind)) for kind in KINDS})
        fns["score_all"] = lambda: model.score_all(x)
        fns["api"] = lambda: vad.metrics.match_regions(maps["sparse"], masks, THRESHOLD, 8, 1, 0.0, 0.0, R)
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    for key, (lo, hi) in r.items():
        out[f"{key}_ms"], out[f"{key}_ms_max"] = round(lo, 4), round(hi, 4)
    for kind in KINDS:
        join = r[kind][0] - r[f"labels_{kind}"][0]
        out[f"{kind}_of_score_all"] = round(r[kind][0] / r["score_all"][0], 4)
        out[f"{kind}_us_per_frame"] = round(r[kind][0] * 1e3 / n, 4)
        out[f"{kind}_join_ms_by_difference"] = round(join, 4)
        out[f"{kind}_join_floor_fraction"] = round(out["floor_join_passes_us"] / (join * 1e3), 4) if join > 0 else None
        out[f"{kind}_of_detect_plus_label"] = round(r[kind][0] / r[f"detect_{kind}"][0], 4)
        if isinstance(host[kind], dict):
            out[f"{kind}_host_over_device"] = round(host[kind]["ms_for_the_batch_scaled"] / r[kind][0], 1)
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
