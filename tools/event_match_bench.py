"""Cost of the matched-event tables (developer tool; not part of the product path).  `vad_match_events` on `--clips` clips of
`--frames` frames of S x S maps (default 32 x 16 x 256 x 256: the clips of tools/events_bench.py, whose three kinds of maps it
reuses - sparse drifting blobs, speckle, all-foreground) against masks of three drifting discs per clip, alternated in one run with

  composition_*  what the commit before this table could do with the same inputs: `vad_detect_events` on the maps plus
                 `vad_detect_events` on the masks as floats - two labellings of the volumes, two event tables, and NO join
  score_all      the scoring call of the seeded ConvAutoencoder on as many `synth` frames
  api            `metrics.match_events` on the sparse maps: the call above plus its allocations and the read of the flag word

and, from one profiled call per kind (torch.profiler; "unavailable" where the profiler is), the device time of every kernel of the
call: the join's own share of it, and the bytes the join has to move - maps and both label planes once, 12 bytes per voxel - against
the floor of moving them at --hbm-tbps (6.29).  The host route it replaces - `.cpu()` of a clip's maps and
masks, 3-D `scipy.ndimage.label` of both with the 26-structure, `sum_labels` both ways, `minimum` of the frame index - runs on the
first clip of every kind and is scaled per clip (skipped, with a note, where scipy is missing); the device's tables of that clip
are checked against it first.  Device-event timing around back-to-back calls after warm-up; variants alternate `--repeats` times,
best and worst are reported.  Prints one JSON line and writes it to --out.

    python tools/event_match_bench.py [--clips 32] [--frames 16] [--size 256] [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/event_match_bench.json]
"""
import argparse
import importlib
import json
import re
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))
vad = importlib.import_module("video-anomaly-detection_amd")
from events_bench import KINDS, THRESHOLD, make_maps  # noqa: E402
from pixel_metrics_bench import alternate, timed  # noqa: E402


def make_masks(b: int, t: int, s: int, seed: int) -> torch.Tensor:
    """uint8 [b, t, s, s], 0 or 255: three discs per clip, each drifting one pixel per frame."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(s, device="cuda"), torch.arange(s, device="cuda"), indexing="ij")
    drift = torch.arange(t, device="cuda").view(1, t, 1, 1)
    masks = torch.zeros((b, t, s, s), dtype=torch.bool, device="cuda")
    for _ in range(3):
        cy = torch.randint(0, s, (b, 1, 1, 1), generator=g, device="cuda") + drift
        cx = torch.randint(0, s, (b, 1, 1, 1), generator=g, device="cuda") - drift
        r = torch.randint(4, max(5, s // 12), (b, 1, 1, 1), generator=g, device="cuda")
        masks |= (yy[None, None] - cy) ** 2 + (xx[None, None] - cx) ** 2 <= r * r
    return masks.to(torch.uint8) * 255


def host_tables(clip: np.ndarray, mask: np.ndarray, min_duration: int):
    """scipy on one clip -> ([(first voxel, volume, hit, first shared frame)] of the tracks, the same of the kept events with
    overlap), or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    structure = np.ones((3, 3, 3), int)
    plab, pcount = ndimage.label(clip >= np.float32(THRESHOLD), structure=structure)
    glab, gcount = ndimage.label(mask, structure=structure)
    frames = np.broadcast_to(np.arange(clip.shape[0])[:, None, None], clip.shape)
    durations = np.array([bx[0].stop - bx[0].start for bx in ndimage.find_objects(plab)], np.int64)
    kept = np.flatnonzero(durations >= min_duration) + 1
    P = np.isin(plab, kept)

    def table(lab, index, other):
        if not len(index):
            return []
        first = np.full(int(lab.max()) + 1, lab.size, np.int64)
        np.minimum.at(first, lab.reshape(-1), np.arange(lab.size))
        volume = np.bincount(lab.reshape(-1), minlength=len(first))
        shared = ndimage.sum_labels(other, lab, index).astype(np.int64)
        since = ndimage.minimum(frames, np.where(other, lab, 0), index).astype(np.int64)
        return [(int(first[k]), int(volume[k]), int(s), int(f) if s else 0xFFFFFFFF) for k, s, f in zip(index, shared, since)]

    return table(glab, np.arange(1, gcount + 1), P), table(plab, kept, mask)


def kernel_times(fn) -> dict:
    """name -> device microseconds of every kernel of one call of fn, by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0))
        if us > 0.0:
            found = re.search(r"(\w+_kernel)\b", e.key)                       # "void (anonymous namespace)::evmatch_join_kernel(...)"
            name = found.group(1) if found else e.key[:48]
            out[name] = out.get(name, 0.0) + us
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-events", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "event_match_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("event_match_bench needs a GPU: a time is measured on the device or not at all")
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
    masks = make_masks(b, t, S, args.seed + 7)
    masks_f = (masks != 0).float()
    need = lib.vad_event_match_workspace_bytes(b, t, S, S)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gt = torch.empty((b, E, vad.hip.EVMATCH_WORDS), dtype=torch.int32, device="cuda")
    pred = torch.empty((b, E, vad.hip.EVMATCH_WORDS), dtype=torch.int32, device="cuda")
    counts = torch.empty((b, vad.hip.EVMATCH_COUNTS), dtype=torch.int64, device="cuda")
    frame_counts = torch.empty((b, t, 4), dtype=torch.int32, device="cuda")
    ev_need = lib.vad_events_workspace_bytes(b, t, S, S, 0)
    ev_ws = torch.empty(ev_need, dtype=torch.uint8, device="cuda")
    ev_records = torch.empty((b, E, vad.hip.EVENT_WORDS), dtype=torch.int32, device="cuda")
    ev_counts = torch.empty((b, 4), dtype=torch.int32, device="cuda")
    ev_frames = torch.empty((b, t, 3), dtype=torch.int32, device="cuda")
    out = {"tool": "event_match_bench", "device": torch.cuda.get_device_name(0), "clips": b, "frames_per_clip": t, "size": S, "elements": elems,
           "threshold": THRESHOLD, "connectivity": 8, "temporal": 9, "max_events": E, "iters": args.iters, "repeats": args.repeats,
           "hbm_tbps": args.hbm_tbps, "workspace_bytes": need, "events_workspace_bytes": ev_need,
           "join_bytes": 12 * elems, "join_floor_us": round(12 * elems / (args.hbm_tbps * 1e12) * 1e6, 2),
           "mask_share": round(float((masks != 0).float().mean()), 4)}

    def match(kind):
        vad.hip.check(lib.vad_match_events(maps[kind].data_ptr(), masks.data_ptr(), vad.hip.LBL_U8_ELEM, b, t, S, S, THRESHOLD, 8, 9, KINDS[kind], 1,
                                           0.0, 0.0, E, gt.data_ptr(), pred.data_ptr(), counts.data_ptr(), frame_counts.data_ptr(), ws.data_ptr(),
                                           need, vad.hip.current_stream()), "vad_match_events")

    def detect(values, min_duration):
        vad.hip.check(lib.vad_detect_events(values.data_ptr(), b, t, S, S, THRESHOLD, 8, 9, min_duration, 1, E, None, ev_records.data_ptr(),
                                            ev_counts.data_ptr(), ev_frames.data_ptr(), ev_ws.data_ptr(), ev_need, vad.hip.current_stream()),
                      "vad_detect_events")

    def composition(kind):
        detect(maps[kind], KINDS[kind])
        detect(masks_f, 1)

    # what the inputs hold, and the tables of the first clip against scipy
    host = {}
    for kind, min_duration in KINDS.items():
        match(kind)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the labelling kernels set their flag word"
        c = counts.cpu().numpy()
        named = dict(zip(vad.metrics.EVENT_COUNT_NAMES, c.sum(0).tolist()))
        out[kind] = {"min_duration": min_duration, "counts": named, "report": {k: v for k, v in vad.metrics.event_report_from_counts(c.sum(0)).items()
                                                                             if k not in named},
                     "truncated_clips": int(((c[:, 0] > E) | (c[:, 2] > E)).sum())}
        g0, p0 = gt[0].cpu().numpy().view(np.uint32), pred[0].cpu().numpy().view(np.uint32)
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hm = maps[kind][0].cpu().numpy(), masks[0].cpu().numpy() >= 128
            t1 = time.perf_counter()
            tables = host_tables(hv, hm, min_duration)
            times.append((time.perf_counter() - t0, t1 - t0))
        if tables is None:
            host[kind] = "skipped: scipy is not installed"
            continue
        for rec, table, full in ((g0, tables[0], int(c[0, 0])), (p0, tables[1], int(c[0, 2]))):
            assert len(table) == full, "the tracks or kept events differ from scipy's"
            for j, row in enumerate(table[:E]):
                assert row == (int(rec[j, 0]), int(rec[j, 1]), int(rec[j, 4]), int(rec[j, 5])), "a record differs from scipy's"
        best = min(times)
        host[kind] = {"clips": 1, "ms_per_clip": round(best[0] * 1e3, 3), "copy_ms_per_clip": round(best[1] * 1e3, 3),
                      "ms_for_the_batch_scaled": round(best[0] * 1e3 * b, 1)}
    out["host_route"] = host

    with torch.no_grad():
        fns = {kind: (lambda kind=kind: match(kind)) for kind in KINDS}
        fns.update({f"composition_{kind}": (lambda kind=kind: composition(kind)) for kind in KINDS})
        fns["score_all"] = lambda: model.score_all(x)
        fns["api"] = lambda: vad.metrics.match_events(maps["sparse"], masks, THRESHOLD, 8, 9, 1, 1, 0.0, 0.0, E)
        r = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    for key, (lo, hi) in r.items():
        out[f"{key}_ms"], out[f"{key}_ms_max"] = round(lo, 4), round(hi, 4)
    for kind in KINDS:
        out[f"{kind}_of_score_all"] = round(r[kind][0] / r["score_all"][0], 4)
        out[f"{kind}_of_composition"] = round(r[kind][0] / r[f"composition_{kind}"][0], 3)
        out[f"{kind}_us_per_clip"] = round(r[kind][0] * 1e3 / b, 4)
        if isinstance(host[kind], dict):
            out[f"{kind}_host_over_device"] = round(host[kind]["ms_for_the_batch_scaled"] / r[kind][1], 1)   # fastest host, slowest device
        try:
            kernels = kernel_times(lambda kind=kind: match(kind))
            total = sum(kernels.values())
            join = sum(us for name, us in kernels.items() if "evmatch_join" in name)
            out[f"{kind}_kernels_us"] = {name: round(us, 1) for name, us in sorted(kernels.items(), key=lambda kv: -kv[1])}
            out[f"{kind}_join_us"], out[f"{kind}_join_share"] = round(join, 1), round(join / total, 4) if total else None
            out[f"{kind}_join_floor_fraction"] = round(out["join_floor_us"] / join, 4) if join else None
        except Exception as e:                                                # noqa: BLE001 - a profiler that does not load is a note, not a failure
            out[f"{kind}_kernels_us"] = f"unavailable: {type(e).__name__}: {e}"
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
