"""Latency of ONE new frame per stream on the stateful video path (developer tool; not part of the product path).

For B = 1, 4, 16, 64 streams of 256x256 frames, in one run:
  * `score_stateful` with T = 1: the newest frame of every stream through the encoder, one ConvLSTM step per layer and
    the decoder, the recurrent state carried in place;
  * the only way to get the newest frame's score without a carried state: re-score the trailing 16-frame window
    (`get_reconstruction_error(per_frame=True)` on [B,16,...], whose last column is that score; for one stream this is
    the one-window `score_windows` call of the reference's video-file mode, evaluate_video.py:322-352).
Device-event timing around `--iters` back-to-back calls after `--warmup` calls of the same shape; the two forms alternate
`--repeats` times so that drift shows as spread.  Prints one JSON line.

    python tools/stream_bench.py [--streams 1 4 16 64] [--hw 256] [--iters 50] [--warmup 10] [--repeats 3]
"""
import argparse
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a GPU: a latency is measured on the device or not at all")
    model = vad.VideoAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 2).items()})
    model.precision = args.precision
    model = model.cuda().eval()
    rows = []
    with torch.no_grad():
        for b in args.streams:
            t = args.window
            clip = vad.scoring.synth_frames_device(3, 0, b * t, args.hw, args.hw).view(b, t, 3, args.hw, args.hw)
            newest = clip[:, t - 1:t].contiguous()
            # the two forms agree on what they compute: the stateful roll-out of the window ends on the window's last score
            state = model.score_stateful(clip[:, :t - 1])["state"]
            one = model.score_stateful(newest, state.clone())["frame"][:, 0]
            win = model.get_reconstruction_error(clip, per_frame=True)[:, t - 1]
            assert torch.equal(one, win), "one-frame call and window re-score disagree"
            launches = {}
            for name, fn in (("one_frame", lambda: model.score_stateful(newest, state)),
                             ("window", lambda: model.get_reconstruction_error(clip, per_frame=True))):
                vad.hip.lib().vad_prof_reset(); vad.hip.lib().vad_prof_enable(1)
                fn()
                ms, n = np.zeros(vad.hip.PROF_SLOTS, np.float32), np.zeros(vad.hip.PROF_SLOTS, np.int32)
                vad.hip.check(vad.hip.lib().vad_prof_read(ms.ctypes.data, n.ctypes.data))
                vad.hip.lib().vad_prof_enable(0)
                launches[name] = int(n.sum())                   # profiled launch scopes of one call
            one_ms, win_ms = [], []
            for _ in range(args.repeats):                       # alternate the two forms
                one_ms.append(timed(lambda: model.score_stateful(newest, state), args.iters, args.warmup))
                win_ms.append(timed(lambda: model.get_reconstruction_error(clip, per_frame=True), max(5, args.iters // 5), max(2, args.warmup // 5)))
            rows.append({"streams": b, "one_frame_ms": round(min(one_ms), 4), "one_frame_ms_max": round(max(one_ms), 4),
                         "window_ms": round(min(win_ms), 4), "window_ms_max": round(max(win_ms), 4),
                         "speedup": round(min(win_ms) / min(one_ms), 2), "scopes_one_frame": launches["one_frame"],
                         "scopes_window": launches["window"],
                         "frames_per_s_one_frame": round(b / min(one_ms) * 1e3, 1)})
    print(json.dumps({"tool": "stream_bench", "hw": args.hw, "window": args.window, "precision": args.precision, "iters": args.iters,
                      "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
