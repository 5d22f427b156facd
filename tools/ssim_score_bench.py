"""Cost of per-frame SSIM scoring (developer tool; not part of the product path).  In one run, on 256x256x3 frames in device memory:

  1. `vad_ssim_score` with and without the per-pixel map, fp32 and uint8 originals, beside `vad_ssim_mse` (the whole-batch
     criterion) on the same planes: us per frame at N = 1 / 16 / 512, bytes moved / time (8 B per element read, + 4 B per pixel
     of map);
  2. `ConvAutoencoder.score_criteria` against `score_all`-style scoring (`scores + recon`) and against `get_reconstruction_error`
     at batch 512: the difference is what the criteria add to a scoring call.
Only N = 512 (805 MB per call) is HBM traffic: at N = 1 / 16 the back-to-back calls re-read 1.6 / 25 MB from L2 / Infinity
Cache, so those columns are launch and latency figures.  Device-event timing around back-to-back calls after warm-up; the
alternatives alternate `--repeats` times, best and worst are reported.  Prints one JSON line.

    python tools/ssim_score_bench.py [--iters 20] [--warmup 5] [--repeats 3] [--frames 1 16 512] [--batch 512]
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
H = W = 256


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
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 512])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=int, default=11)
    args = ap.parse_args()
    l, hip = vad.hip.lib(), vad.hip
    st = hip.current_stream()
    res = {"window": args.window, "kernel": {}, "model": {}}

    def run(fn):
        return timed(fn, args.iters, args.warmup)

    for n in args.frames:
        x = vad.scoring.synth_frames_device(3, 0, n, H, W)
        recon = (x + 0.1 * torch.randn_like(x)).clamp(-1, 1)
        xu8 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda")
        mse = ((recon - x) ** 2).mean(dim=(1, 2, 3))
        ws = torch.empty(l.vad_ssim_score_workspace_floats(n, H, W), device="cuda")
        ws_b = torch.empty(l.vad_ssim_workspace_floats(3 * n, H, W), device="cuda")
        ssim, comb, smap, out3 = (torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 1, H, W, device="cuda"),
                                  torch.empty(3, device="cuda"))

        def score(xt, fmt, want_map):
            return lambda: hip.check(l.vad_ssim_score(recon.data_ptr(), xt.data_ptr(), fmt, n, 3, H, W, args.window, 0.5, mse.data_ptr(),
                                                      ws.data_ptr(), ssim.data_ptr(), comb.data_ptr(), smap.data_ptr() if want_map else None, st))

        fns = {"ssim_mse_batch": lambda: hip.check(l.vad_ssim_mse(recon.data_ptr(), x.data_ptr(), 3 * n, H, W, args.window, 0.5, ws_b.data_ptr(),
                                                                  out3.data_ptr(), st)),
               "ssim_score": score(x, hip.X_F32_NCHW, False), "ssim_score_map": score(x, hip.X_F32_NCHW, True),
               "ssim_score_u8": score(xu8, hip.X_U8_NHWC, False), "ssim_score_u8_map": score(xu8, hip.X_U8_NHWC, True)}
        read = {"ssim_mse_batch": 8, "ssim_score": 8, "ssim_score_map": 8, "ssim_score_u8": 5, "ssim_score_u8_map": 5}
        row = {}
        for k, (lo, hi) in alternate(fns, args.repeats, run).items():
            nbytes = n * H * W * (3 * read[k] + (4 if k.endswith("map") else 0))
            row[k] = {"us_per_frame": round(lo * 1e3 / n, 3), "us_per_frame_worst": round(hi * 1e3 / n, 3),
                      "GBps_algorithmic": round(nbytes / (lo * 1e-3) / 1e9, 1)}
        res["kernel"][f"n{n}"] = row

    b = args.batch
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=256)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    m = m.cuda().eval()
    x = vad.scoring.synth_frames_device(5, 0, b, H, W)
    with torch.no_grad():
        fns = {"scores": lambda: m.get_reconstruction_error(x), "scores_recon": lambda: m._run_hip(x, scores=True, recon=True),
               "score_all": lambda: m.score_all(x), "score_criteria": lambda: m.score_criteria(x),
               "score_criteria_map": lambda: m.score_criteria(x, ssim_map=True)}
        for k, (lo, hi) in alternate(fns, args.repeats, run).items():
            res["model"][k] = {"ms": round(lo, 3), "ms_worst": round(hi, 3), "us_per_frame": round(lo * 1e3 / b, 3)}
    res["model"]["batch"] = b
    res["model"]["criteria_over_scores_recon"] = round(res["model"]["score_criteria"]["ms"] / res["model"]["scores_recon"]["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
