"""Cost of the event tracker (developer tool; not part of the product path).  `--streams` live streams (default 1, 4, 16, 64) hand
over one new S x S map per call (default 256 x 256), of the three kinds of tools/events_bench.py (sparse: four drifting discs on low
noise; speckle: 5 % foreground, min_duration 3; full: every pixel foreground).  Three variants, alternated `--repeats` times in one
run, device events around back-to-back calls after warm-up:

  track    `vad_track_events` with t = 1: the new map into the tracker's state
  window   `vad_detect_events` on every stream's trailing 16-frame window - the only way to a persistence alarm for the newest frame
           without the tracker; it also cuts every event at the window's edge
  stateful `score_stateful` of the seeded VideoAutoencoder on one new frame per stream: the scoring call the tracker stands behind

The maps of a stream are a ring of 16 frames, so the window variant's input is the ring itself.  First, per kind, one stream's 16
frames go through `metrics.EventTracker` (one call, then one frame per call) and the closed + flushed records - converted and
sorted - are compared with `metrics.detect_events` on the same frames.  The bar: at every stream count and kind the slowest track
repeat beats the fastest window repeat of the same run; a cell that misses it is listed in `bar_missed`, not dropped.  Also: the
tracker's share of the stateful scoring call and its distance from the floor of reading the new maps once at --hbm-tbps.
Prints one JSON line and writes it to --out.

    python tools/track_bench.py [--streams 1 4 16 64] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/track_bench.json]
"""
import argparse
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))
vad = importlib.import_module("video-anomaly-detection_amd")
from events_bench import KINDS, THRESHOLD, make_maps  # noqa: E402
from pixel_metrics_bench import alternate, timed  # noqa: E402

WINDOW = 16


def converted(records: np.ndarray, h: int, w: int) -> np.ndarray:
    """Tracker records uint32 [k, 20] -> the 16 words of vad_detect_events, sorted by root."""
    r = records.astype(np.uint32)
    out = np.zeros((len(r), 16), np.uint32)
    out[:, 0] = r[:, 1] * np.uint32(h * w) + r[:, 0]
    out[:, 1], out[:, 2], out[:, 3], out[:, 4:8], out[:, 8] = r[:, 12], r[:, 1], r[:, 2], r[:, 4:8], r[:, 8]
    out[:, 9] = r[:, 10] * np.uint32(h * w) + r[:, 9]
    out[:, 10:16] = r[:, 14:20]
    assert not r[:, 13].any(), "a volume beyond 32 bits in a 16-frame check"
    return out[np.argsort(out[:, 0], kind="stable")]


def check_against_detect_events(kind: str, maps: torch.Tensor, max_open: int) -> dict:
    """maps [1, 16, S, S]: tracker (whole clip in one call, and frame by frame) == detect_events on the clip."""
    _, t, h, w = maps.shape
    ev = vad.metrics.detect_events(maps, THRESHOLD, 8, 9, KINDS[kind], 1, 65536)
    kept = int(ev.counts[0, 0])
    want = ev.records[0, :kept].cpu().numpy().view(np.uint32)
    for splits in ((t,), (1,) * t):
        tr = vad.metrics.EventTracker(1, h, w, THRESHOLD, 8, 9, KINDS[kind], 1, max_open, 65536)
        ups, at = [], 0
        for n in splits:
            ups.append(tr.update(maps[:, at:at + n]))
            at += n
        ups.append(tr.flush())
        assert all(int(u.counts[0, 5]) == 0 and int(u.counts[0, 0]) <= 65536 for u in ups), "an event was lost or the closed table truncated"
        closed = np.concatenate([u.records[0, :int(u.counts[0, 0])].cpu().numpy().view(np.uint32) for u in ups])
        assert np.array_equal(converted(closed, h, w), want), f"{kind}: the tracker's events differ from detect_events'"
        assert sum(int(u.counts[0, 1]) for u in ups) == int(ev.counts[0, 1]), f"{kind}: the dropped events differ"
    return {"kept": kept, "dropped": int(ev.counts[0, 1]), "open_at_most": int(max(int(u.counts[0, 4]) for u in ups))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--max-open", type=int, default=4096)
    ap.add_argument("--max-closed", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "track_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench needs a GPU: a time is measured on the device or not at all")
    S, O, E = args.size, args.max_open, args.max_closed
    lib = vad.hip.lib()
    out = {"tool": "track_bench", "device": torch.cuda.get_device_name(0), "size": S, "window": WINDOW, "threshold": THRESHOLD, "connectivity": 8,
           "temporal": 9, "max_open": O, "max_closed": E, "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps, "checked": {},
           "cells": {}, "bar_missed": []}
    for i, kind in enumerate(KINDS):
        out["checked"][kind] = check_against_detect_events(kind, make_maps(kind, 1, WINDOW, S, args.seed + i), O)

    model = vad.VideoAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 2).items()})
    model = model.cuda().eval()

    for b in args.streams:
        state = torch.empty(lib.vad_track_state_bytes(b, S, S, O), dtype=torch.uint8, device="cuda")
        need = lib.vad_track_workspace_bytes(b, 1, S, S, O)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        closed = torch.empty((b, E, vad.hip.TRACK_WORDS), dtype=torch.int32, device="cuda")
        counts = torch.empty((b, 6), dtype=torch.int32, device="cuda")
        frame_counts = torch.empty((b, 1, 3), dtype=torch.int32, device="cuda")
        wneed = lib.vad_events_workspace_bytes(b, WINDOW, S, S, 0)
        wws = torch.empty(wneed, dtype=torch.uint8, device="cuda")
        wrecords = torch.empty((b, E, vad.hip.EVENT_WORDS), dtype=torch.int32, device="cuda")
        wcounts = torch.empty((b, 4), dtype=torch.int32, device="cuda")
        wframes = torch.empty((b, WINDOW, 3), dtype=torch.int32, device="cuda")
        newest = vad.scoring.synth_frames_device(3, 0, b, S, S).view(b, 1, 3, S, S)
        with torch.no_grad():
            vstate = model.score_stateful(newest)["state"]
        floor_us = 4 * b * S * S / (args.hbm_tbps * 1e12) * 1e6
        for i, kind in enumerate(KINDS):
            ring = make_maps(kind, b, WINDOW, S, args.seed + i)
            frames = [ring[:, f].contiguous() for f in range(WINDOW)]
            at = [0]

            def track():
                vad.hip.check(lib.vad_track_events(frames[at[0] % WINDOW].data_ptr(), b, 1, S, S, THRESHOLD, 8, 9, KINDS[kind], 1, O, E, state.data_ptr(),
                                                   closed.data_ptr(), counts.data_ptr(), frame_counts.data_ptr(), ws.data_ptr(), need,
                                                   vad.hip.current_stream()), "vad_track_events")
                at[0] += 1

            def window():
                vad.hip.check(lib.vad_detect_events(ring.data_ptr(), b, WINDOW, S, S, THRESHOLD, 8, 9, KINDS[kind], 1, E, None, wrecords.data_ptr(),
                                                    wcounts.data_ptr(), wframes.data_ptr(), wws.data_ptr(), wneed, vad.hip.current_stream()),
                              "vad_detect_events")

            vad.hip.check(lib.vad_track_init(state.data_ptr(), b, S, S, O, vad.hip.current_stream()), "vad_track_init")
            with torch.no_grad():
                r = alternate({"track": track, "window": window, "stateful": lambda: model.score_stateful(newest, vstate)}, args.repeats,
                              lambda fn: timed(fn, args.iters, args.warmup))
            torch.cuda.synchronize()
            assert int(ws[:4].view(torch.int32).item()) == 0 and int(wws[:4].view(torch.int32).item()) == 0, "a flag word is set"
            header = state.view(torch.int32).view(b, -1)[:, :4].cpu().numpy()
            assert not header[:, 3].any() and int(header[0, 0]) == at[0], "the state's flags or frame counter"
            cell = {"track_ms": round(r["track"][0], 4), "track_ms_max": round(r["track"][1], 4), "window_ms": round(r["window"][0], 4),
                    "window_ms_max": round(r["window"][1], 4), "stateful_ms": round(r["stateful"][0], 4), "stateful_ms_max": round(r["stateful"][1], 4),
                    "window_over_track": round(r["window"][0] / r["track"][1], 2), "track_of_stateful": round(r["track"][0] / r["stateful"][0], 4),
                    "floor_read_new_maps_once_us": round(floor_us, 3), "floor_fraction": round(floor_us / (r["track"][0] * 1e3), 5),
                    "open_after": int(header[:, 1].max()), "lost_in_total": int(header[:, 2].sum()), "bar_met": bool(r["track"][1] < r["window"][0])}
            out["cells"][f"{b}_{kind}"] = cell
            if not cell["bar_met"]:
                out["bar_missed"].append(f"{b}_{kind}")
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
