"""Cost of the per-frame tracks (developer tool; not part of the product path).  Clip mode: `vad_event_tracks` on `--clips` clips of
`--frames` frames of S x S maps (default 32 x 16 x 256 x 256) of the three kinds of tools/events_bench.py - sparse (four drifting
discs per clip), speckle (5 % foreground, min_duration 3), full (every pixel foreground: one event per clip, where every pixel of a
frame meets in ONE record) - behind the `vad_detect_events` call that feeds it, alternated in one run with

  events_labels_*   `vad_detect_events` with the label volume written (what the tracks need)
  events_*          the same without it: the difference is the added cost of `return_labels=True`
  score_all         the scoring call of the seeded ConvAutoencoder on as many `synth` frames

and beside the HBM figure of one read of the label volume, one read of the maps at the foreground pixels and the table's write at
--hbm-tbps (6.29).  The host route it replaces - `.cpu()` of labels and maps, scipy `find_objects` per frame and
label, `sum`, `maximum_position` - runs on the first clip of every kind and is scaled per clip (skipped, with a note, where scipy is
missing); the device's boxes, areas and peaks of that clip are checked against it first.
Live mode: `vad_track_boxes` behind `vad_track_events` with one new map per stream at `--streams` (default 1, 4, 16, 64) streams,
against the tracker call alone and against the one-frame `score_stateful` call of the seeded VideoAutoencoder.
Device-event timing around back-to-back calls after warm-up; variants alternate `--repeats` times; median, min and max are reported.
The expectation the run confirms or refutes per kind: the clip call costs less than the `detect_events` call that feeds it
(`*_below_detect_events`; a cell that misses it is listed in `bar_missed`, not dropped).  Prints one JSON line and writes it to --out.

    python tools/tracks_bench.py [--clips 32] [--frames 16] [--size 256] [--streams 1 4 16 64] [--iters 20] [--warmup 5] [--repeats 3]
                                 [--out profiles/event_tracks_bench.json]
"""
import argparse
import importlib
import json
import statistics
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
from pixel_metrics_bench import timed  # noqa: E402


def alternate(fns: dict, repeats: int, iters: int, warmup: int) -> dict:
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters, warmup))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}


def host_tracks(clip: np.ndarray, labels: np.ndarray, roots) -> list:
    """scipy on one clip -> per kept event and frame None or (area, (x0, y0, x1, y1), peak index), or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    t, h, w = clip.shape
    out = []
    for root in roots:
        track = []
        for f in range(t):
            mine = labels[f] == root + 1
            objects = ndimage.find_objects(mine.astype(np.int32))
            if not objects:
                track.append(None)
                continue
            ys, xs = objects[0]
            py, px = ndimage.maximum_position(clip[f], mine)
            track.append((int(ndimage.sum(mine)), (xs.start, ys.start, xs.stop - 1, ys.stop - 1), py * w + px))
        out.append(track)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--max-events", type=int, default=64)
    ap.add_argument("--max-open", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "event_tracks_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tracks_bench needs a GPU: a time is measured on the device or not at all")
    b, t, S, E, O = args.clips, args.frames, args.size, args.max_events, args.max_open
    n = b * t
    elems = n * S * S
    lib = vad.hip.lib()
    out = {"tool": "tracks_bench", "device": torch.cuda.get_device_name(0), "clips": b, "frames_per_clip": t, "size": S, "elements": elems,
           "threshold": THRESHOLD, "connectivity": 8, "temporal": 9, "max_events": E, "max_open": O, "iters": args.iters, "repeats": args.repeats,
           "hbm_tbps": args.hbm_tbps, "clip": {}, "live": {}, "bar_missed": []}

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)

    maps = {k: make_maps(k, b, t, S, args.seed + i) for i, k in enumerate(KINDS)}
    need = {given: lib.vad_events_workspace_bytes(b, t, S, S, given) for given in (0, 1)}
    ws = torch.empty(max(need.values()), dtype=torch.uint8, device="cuda")
    labels = {k: torch.empty((b, t, S, S), dtype=torch.int32, device="cuda") for k in KINDS}
    records = {k: torch.empty((b, E, vad.hip.EVENT_WORDS), dtype=torch.int32, device="cuda") for k in KINDS}
    counts = {k: torch.empty((b, 4), dtype=torch.int32, device="cuda") for k in KINDS}
    frame_counts = torch.empty((b, t, 3), dtype=torch.int32, device="cuda")
    tracks = torch.empty((b, E, t, vad.hip.REGION_WORDS), dtype=torch.int32, device="cuda")
    scratch_records = torch.empty((b, E, vad.hip.EVENT_WORDS), dtype=torch.int32, device="cuda")
    scratch_counts = torch.empty((b, 4), dtype=torch.int32, device="cuda")

    def detect(kind, with_labels, rec=None, cnt=None):
        rec, cnt = (records[kind], counts[kind]) if rec is None else (rec, cnt)
        vad.hip.check(lib.vad_detect_events(maps[kind].data_ptr(), b, t, S, S, THRESHOLD, 8, 9, KINDS[kind], 1, E,
                                            labels[kind].data_ptr() if with_labels else None, rec.data_ptr(), cnt.data_ptr(), frame_counts.data_ptr(),
                                            ws.data_ptr(), need[1 if with_labels else 0], vad.hip.current_stream()), "vad_detect_events")

    def reduce(kind):
        vad.hip.check(lib.vad_event_tracks(maps[kind].data_ptr(), labels[kind].data_ptr(), records[kind].data_ptr(), counts[kind].data_ptr(), b, t, S, S,
                                           E, tracks.data_ptr(), vad.hip.current_stream()), "vad_event_tracks")

    # what the tables hold, and the tracks of the first clip against scipy
    host = {}
    for kind in KINDS:
        detect(kind, True)
        reduce(kind)
        torch.cuda.synchronize()
        assert int(ws[:4].view(torch.int32).item()) == 0, "the labelling kernels set their flag word"
        c = counts[kind].cpu().numpy().astype(np.int64)
        area = tracks[..., 1].to(torch.int64)
        in_table = int(area.sum())
        assert torch.equal(area.sum(-1), records[kind][..., 1].to(torch.int64)), "the areas of a track do not sum to the event's volume"
        out["clip"][kind] = {"min_duration": KINDS[kind], "kept_per_clip": round(float(c[:, 0].mean()), 2), "truncated_clips": int((c[:, 0] > E).sum()),
                             "foreground_share": round(float(c[:, 2].sum()) / elems, 4), "pixels_in_tracks_share": round(in_table / elems, 4),
                             "cross_sections_per_clip": round(float((area > 0).sum()) / b, 2),
                             "hbm_us": round((4 * elems + 4 * int(c[:, 2].sum()) + 48 * b * E * t) / (args.hbm_tbps * 1e12) * 1e6, 2)}
        kept = min(int(c[0, 0]), E)
        roots = records[kind][0, :kept, 0].cpu().numpy().astype(np.int64)
        got = tracks[0, :kept].cpu().numpy()
        times = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hv, hl = maps[kind][0].cpu().numpy(), labels[kind][0].cpu().numpy()
            t1 = time.perf_counter()
            table = host_tracks(hv, hl, roots)
            times.append((time.perf_counter() - t0, t1 - t0))
        if table is None:
            host[kind] = "skipped: scipy is not installed"
            continue
        for e, track in enumerate(table):
            for f, want in enumerate(track):
                r = got[e, f]
                assert (want is None and not r.any()) or want == (int(r[1]), tuple(int(v) for v in r[2:6]), int(r[7])), "a cross-section differs from scipy's"
        best = min(times)
        host[kind] = {"clips": 1, "events": kept, "ms_per_clip": round(best[0] * 1e3, 3), "copy_ms_per_clip": round(best[1] * 1e3, 3),
                      "ms_for_the_batch_scaled": round(best[0] * 1e3 * b, 1)}
    out["host_route"] = host

    with torch.no_grad():
        fns = {f"tracks_{kind}": (lambda kind=kind: reduce(kind)) for kind in KINDS}
        fns.update({f"events_labels_{kind}": (lambda kind=kind: detect(kind, True, scratch_records, scratch_counts)) for kind in KINDS})
        fns.update({f"events_{kind}": (lambda kind=kind: detect(kind, False, scratch_records, scratch_counts)) for kind in KINDS})
        fns["score_all"] = lambda: model.score_all(x)
        fns["api"] = lambda: vad.metrics.event_tracks(maps["sparse"], api_events)
        api_events = vad.metrics.detect_events(maps["sparse"], THRESHOLD, 8, 9, 1, 1, E, return_labels=True)
        r = alternate(fns, args.repeats, args.iters, args.warmup)
    out["timings"] = r
    for kind in KINDS:
        cell = out["clip"][kind]
        tr, ev, evl = r[f"tracks_{kind}"], r[f"events_{kind}"], r[f"events_labels_{kind}"]
        cell["tracks_of_detect_events"] = round(tr["median_ms"] / evl["median_ms"], 4)
        cell["tracks_of_score_all"] = round(tr["median_ms"] / r["score_all"]["median_ms"], 4)
        cell["labels_added_ms"] = round(evl["median_ms"] - ev["median_ms"], 4)
        cell["hbm_fraction"] = round(cell["hbm_us"] / (tr["median_ms"] * 1e3), 4)
        cell["below_detect_events"] = tr["max_ms"] < evl["min_ms"]             # the slowest tracks repeat against the fastest feeding call
        if not cell["below_detect_events"]:
            out["bar_missed"].append({"kind": kind, "tracks": tr, "detect_events": evl})
        if isinstance(host[kind], dict):
            cell["host_over_device"] = round(host[kind]["ms_for_the_batch_scaled"] / tr["max_ms"], 1)

    video = vad.VideoAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in video.state_dict().items()}
    video.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 2).items()})
    video = video.cuda().eval()
    for s in args.streams:
        state = torch.empty(lib.vad_track_state_bytes(s, S, S, O), dtype=torch.uint8, device="cuda")
        tneed = lib.vad_track_workspace_bytes(s, 1, S, S, O)
        tws = torch.empty(tneed, dtype=torch.uint8, device="cuda")
        closed = torch.empty((s, E, vad.hip.TRACK_WORDS), dtype=torch.int32, device="cuda")
        tcounts = torch.empty((s, 6), dtype=torch.int32, device="cuda")
        tframes = torch.empty((s, 1, 3), dtype=torch.int32, device="cuda")
        boxes = torch.empty((s, O, vad.hip.REGION_WORDS), dtype=torch.int32, device="cuda")
        newest = vad.scoring.synth_frames_device(3, 0, s, S, S).view(s, 1, 3, S, S)
        with torch.no_grad():
            vstate = video.score_stateful(newest)["state"]
        out["live"][str(s)] = {}
        for i, kind in enumerate(KINDS):
            ring = make_maps(kind, s, 16, S, args.seed + i)
            frames = [ring[:, f].contiguous() for f in range(16)]
            at = [0]

            def track(with_boxes):
                m = frames[at[0] % 16]
                vad.hip.check(lib.vad_track_events(m.data_ptr(), s, 1, S, S, THRESHOLD, 8, 9, KINDS[kind], 1, O, E, state.data_ptr(), closed.data_ptr(),
                                                   tcounts.data_ptr(), tframes.data_ptr(), tws.data_ptr(), tneed, vad.hip.current_stream()), "vad_track_events")
                if with_boxes:
                    vad.hip.check(lib.vad_track_boxes(m.data_ptr(), S * S, s, S, S, O, state.data_ptr(), boxes.data_ptr(), vad.hip.current_stream()),
                                  "vad_track_boxes")
                at[0] += 1

            vad.hip.check(lib.vad_track_init(state.data_ptr(), s, S, S, O, vad.hip.current_stream()), "vad_track_init")
            with torch.no_grad():
                r = alternate({"update_boxes": lambda: track(True), "update": lambda: track(False), "stateful": lambda: video.score_stateful(newest, vstate)},
                              args.repeats, args.iters, args.warmup)
            track(True)
            torch.cuda.synchronize()
            header = state.view(torch.int32).view(s, -1)[:, :4].cpu().numpy()
            assert int(tws[:4].view(torch.int32).item()) == 0 and not header[:, 3].any(), "a flag word is set"
            nopen = int(header[0, 1])
            table = state.view(torch.int32).view(s, -1)[0, 16:16 + 20 * O].view(O, 20)
            assert torch.equal(boxes[0, :nopen, 0], table[:nopen, 3]) and not bool(boxes[0, nopen:].any()), "a box's smallest pixel is not its event's handle"
            r["boxes_added_ms"] = round(r["update_boxes"]["median_ms"] - r["update"]["median_ms"], 4)
            r["boxes_added_of_update"] = round(r["boxes_added_ms"] / r["update"]["median_ms"], 4)
            r["boxes_added_of_stateful"] = round(r["boxes_added_ms"] / r["stateful"]["median_ms"], 4)
            r["open_events_stream_0"] = nopen
            out["live"][str(s)][kind] = r
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
