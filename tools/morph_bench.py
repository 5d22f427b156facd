"""Cost of the grey morphology of anomaly maps (developer tool; not part of the product path).  `metrics.morph_maps` on the error
maps `score_all` of the seeded ConvAutoencoder writes for `--frames` x S x S `synth` frames (default 512 x 256 x 256): the four
ops at the sizes 2, 3, 5, 15 and 31, one cell each.  Every cell stands beside

  (1) the HBM floor of 8 bytes per element (one read, one write) at --hbm-tbps (6.29),
  (2) `metrics.smooth_maps` at sigma 4 on the same maps, timed in the same alternated run,
  (3) the same op composed from torch ops on the device: `+-max_pool2d(+-x, size, stride=1)` on a map padded with -+inf by the
      window's reach on each side (open / close: two of them).  Clamping a window is padding with the identity, so the
      composition computes the same values; it is asserted `torch.equal` to the kernel for the odd sizes and reported for the
      even ones.

Device-event timing around back-to-back calls after warm-up; kernel, composition and smoothing alternate `--repeats` times within a
cell; median, min and max are reported.  Prints one JSON line and writes it to --out.

    python tools/morph_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 5] [--out profiles/morph_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
vad = importlib.import_module("video-anomaly-detection_amd")

OPS = ("erode", "dilate", "open", "close")
SIZES = (2, 3, 5, 15, 31)


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


def torch_step(x: torch.Tensor, s: int, is_max: bool) -> torch.Tensor:
    """One erosion / dilation of [N,1,H,W] with a flat s x s element as a max-pool over an identity-padded map."""
    lo, hi = ((s - 1) // 2, s // 2) if is_max else (s // 2, (s - 1) // 2)
    if is_max:
        return F.max_pool2d(F.pad(x, (lo, hi, lo, hi), value=float("-inf")), s, stride=1)
    return -F.max_pool2d(F.pad(-x, (lo, hi, lo, hi), value=float("-inf")), s, stride=1)


def torch_morph(x: torch.Tensor, op: str, s: int) -> torch.Tensor:
    seq = {"erode": (False,), "dilate": (True,), "open": (False, True), "close": (True, False)}[op]
    for is_max in seq:
        x = torch_step(x, s, is_max)
    return x


def summary(ms: list) -> dict:
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--composition-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "morph_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("morph_bench needs a GPU: a time is measured on the device or not at all")
    if args.repeats < 3:
        raise SystemExit("morph_bench: --repeats must be at least 3 (the variants are alternated; median, min and max are reported)")
    n, S = args.frames, args.size

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)
    with torch.no_grad():
        maps = model.score_all(x)["errmap"].clone()
    del x, model
    elems = n * S * S
    floor_us = 8 * elems / (args.hbm_tbps * 1e12) * 1e6
    out = {"tool": "morph_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "elements": elems, "iters": args.iters,
           "composition_iters": args.composition_iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps, "hbm_floor_us": round(floor_us, 2),
           "smooth_sigma": 4.0, "cells": {}}
    buf = torch.empty_like(maps)
    smooth_ms = []
    all_beat = True
    with torch.no_grad():
        for op in OPS:
            for s in SIZES:
                got = vad.metrics.morph_maps(maps, op, s, out=buf)
                comp = torch_morph(maps, op, s)
                same = bool(torch.equal(comp, got))
                if s % 2:
                    assert same, f"{op} {s}: the torch composition and the kernel differ"
                del comp
                kernel, composed = [], []
                for _ in range(args.repeats):
                    kernel.append(timed(lambda: vad.metrics.morph_maps(maps, op, s, out=buf), args.iters, args.warmup))
                    composed.append(timed(lambda: torch_morph(maps, op, s), args.composition_iters, 1))
                    smooth_ms.append(timed(lambda: vad.metrics.smooth_maps(maps, 4.0, out=buf), args.iters, args.warmup))
                tile_h, tile_w = C.c_int(), C.c_int()
                vad.hip.check(vad.hip.lib().vad_morph_tile(s, s, vad.hip.MORPH_OPS[op], C.byref(tile_h), C.byref(tile_w)), "vad_morph_tile")
                cell = summary(kernel)
                comp_cell = summary(composed)
                beats = cell["ms_max"] < comp_cell["ms_min"]                  # by more than the run-to-run spread of the two
                all_beat &= beats
                cell.update({"tile": [tile_h.value, tile_w.value], "hbm_floor_fraction": round(floor_us / (cell["ms"] * 1e3), 4),
                             "G_elements_per_s": round(elems / cell["ms"] / 1e6, 2), "torch_composition": comp_cell,
                             "composition_equals_kernel": same, "composition_over_kernel": round(comp_cell["ms"] / cell["ms"], 2),
                             "slowest_kernel_run_beats_fastest_composition": beats})
                out["cells"][f"{op}_{s}"] = cell
    sm = summary(smooth_ms)
    sm["hbm_floor_fraction"] = round(floor_us / (sm["ms"] * 1e3), 4)
    out["smooth_maps_sigma4"] = sm
    for cell in out["cells"].values():
        cell["of_smooth_maps"] = round(cell["ms"] / sm["ms"], 4)
    out["every_cell_beats_the_composition"] = bool(all_beat)
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)
    assert all_beat, "a cell does not beat the torch composition by more than the spread of the two"


if __name__ == "__main__":
    main()
