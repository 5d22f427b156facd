"""Cost of the per-pixel map statistics and the z-score map (developer tool; not part of the product path).  `metrics.MapStatistics`
on the error maps `score_all` of the seeded ConvAutoencoder writes for `--frames` x S x S `synth` frames (default 512 x 256 x 256),
alternated in one run:

  accumulate        one `update` of all the maps (HBM floor: 4 bytes per element, one read);
  normalize         the z-score map (floor: 8 bytes per element, one read and one write);
  normalize_max     the z-score map and the per-frame maxima;
  max_only          the maxima only (no map is written);
  *_rotating        accumulate / max_only over a ring of `--ring` copies of the maps, more bytes than the Infinity Cache holds:
                    the same maps again and again (128 MiB at the default size) are served on-die, which a long calibration never is;
  torch_var_mean    what accumulate + finalize replace: `torch.var_mean(maps.double(), 0)` and the root, on the device;
  torch_normalize   what normalize replaces: `(maps - mean) / std.clamp_min(min_std)`, and `.amax` for the maxima;
  score_all         the scoring call that produced the maps;
  one_frame_*       `update` / `normalize(return_max=True)` of ONE frame per call: the live-stream case.

Each time stands beside its HBM floor at --hbm-tbps (6.29) and beside the host route the kernels replace -
`.cpu()` + numpy float64 `mean` / `std` - on `--host-frames` frames, scaled.  Device-event timing around back-to-back calls after
warm-up; the variants alternate `--repeats` times, best and worst are reported.  The statistics are checked against torch's float64
`var_mean` (one float32 unit) and the z-scores against the composition first.  Prints one JSON line and writes it to --out.

    python tools/map_stats_bench.py [--frames 512] [--size 256] [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/map_stats_bench.json]
"""
import argparse
import ctypes
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
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


def alternate(fns: dict, repeats: int, run) -> dict:
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(run(fn))
    return {k: (min(v), max(v)) for k, v in ms.items()}


def ulps32(got: torch.Tensor, want64: torch.Tensor) -> float:
    """Largest distance of float32 `got` from float64 `want64` in float32 units in the last place at `want64`."""
    w = want64.cpu().numpy()
    unit = np.spacing(np.abs(w).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - w) / unit))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--min-std", type=float, default=vad.metrics.DEFAULT_MIN_STD)
    ap.add_argument("--ring", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--host-frames", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--out", default=str(REPO / "profiles" / "map_stats_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_stats_bench needs a GPU: a time is measured on the device or not at all")
    if args.repeats < 3:
        raise SystemExit("map_stats_bench: --repeats must be at least 3 (the variants are alternated; min .. max are reported)")
    n, S, min_std = args.frames, args.size, float(np.float32(args.min_std))

    model = vad.ConvAutoencoder()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 1).items()})
    model = model.cuda().eval()
    x = vad.scoring.synth_frames_device(args.seed, 0, n, S, S, anomalies=True)
    with torch.no_grad():
        maps = model.score_all(x)["errmap"].clone()
    elems = n * S * S
    floor4, floor8 = 4 * elems / (args.hbm_tbps * 1e12) * 1e6, 8 * elems / (args.hbm_tbps * 1e12) * 1e6
    plan = [ctypes.c_int() for _ in range(3)]
    vad.hip.check(vad.hip.lib().vad_mapstat_plan(*(ctypes.byref(p) for p in plan)), "vad_mapstat_plan")
    out = {"tool": "map_stats_bench", "device": torch.cuda.get_device_name(0), "frames": n, "size": S, "elements": elems, "min_std": min_std,
           "plan": {"pixels_per_thread": plan[0].value, "frames_in_flight": plan[1].value, "threads": plan[2].value},
           "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps, "maps_MiB": round(4 * elems / 2 ** 20, 1),
           "ring_MiB": round(args.ring * 4 * elems / 2 ** 20, 1), "accumulate_floor_us": round(floor4, 2), "normalize_floor_us": round(floor8, 2)}

    # checks first: the statistics against torch's float64, the z-scores against the composition
    stats = vad.metrics.MapStatistics((S, S)).update(maps)
    var64, mean64 = torch.var_mean(maps.double().reshape(n, S, S), 0)
    out["mean_ulps_of_float64"] = round(ulps32(stats.mean(), mean64), 3)
    out["std_ulps_of_float64"] = round(ulps32(stats.std(), var64.sqrt()), 3)
    assert out["mean_ulps_of_float64"] <= 1.0 and out["std_ulps_of_float64"] <= 1.0, "the statistics are not within one float32 unit of float64's"
    mean, std = stats.mean(), stats.std()

    def torch_var_mean():
        v, m = torch.var_mean(maps.double(), 0)
        return m.float(), v.float().sqrt()

    def torch_normalize():
        return (maps - mean) / std.clamp_min(min_std)

    z, zmax = stats.normalize(maps, min_std, return_max=True)
    comp = torch_normalize()
    out["composition_equal_bits"] = bool(torch.equal(z, comp))
    out["composition_max_abs_diff_over_1_plus_abs"] = float(((comp - z).abs() / (1 + z.abs())).max())
    assert out["composition_max_abs_diff_over_1_plus_abs"] < 1e-5, "the torch composition does not compute the same z-scores"
    del comp
    assert torch.equal(zmax.reshape(-1), z.amax(dim=(-2, -1)).reshape(-1)), "the per-frame maxima differ from torch.amax of the maps"
    assert torch.equal(stats.normalize(maps, min_std, return_max="only"), zmax)
    del z, var64, mean64

    ring = [maps] + [maps.clone() for _ in range(args.ring - 1)]
    turn = {"a": 0, "n": 0}

    def next_of(key):
        turn[key] = (turn[key] + 1) % len(ring)
        return ring[turn[key]]

    scratch = vad.metrics.MapStatistics((S, S))
    live = vad.metrics.MapStatistics((S, S)).update(maps[:2])
    buf = torch.empty_like(maps)
    one = maps[:1].contiguous()
    one_buf = torch.empty_like(one)
    with torch.no_grad():
        fns = {"accumulate": lambda: scratch.update(maps),
               "accumulate_rotating": lambda: scratch.update(next_of("a")),
               "normalize": lambda: stats.normalize(maps, min_std, out=buf),
               "normalize_max": lambda: stats.normalize(maps, min_std, out=buf, return_max=True),
               "max_only": lambda: stats.normalize(maps, min_std, return_max="only"),
               "max_only_rotating": lambda: stats.normalize(next_of("n"), min_std, return_max="only"),
               "torch_var_mean": torch_var_mean,
               "torch_normalize": torch_normalize,
               "torch_normalize_max": lambda: torch_normalize().amax(dim=(-2, -1)),
               "score_all": lambda: model.score_all(x),
               "one_frame_update": lambda: live.update(one),
               "one_frame_normalize_max": lambda: stats.normalize(one, min_std, out=one_buf, return_max=True)}
        res = alternate(fns, args.repeats, lambda fn: timed(fn, args.iters, args.warmup))
    score_ms = res["score_all"]
    floors = {"accumulate": floor4, "accumulate_rotating": floor4, "max_only": floor4, "max_only_rotating": floor4, "normalize": floor8,
              "normalize_max": floor8}
    against = {"accumulate": "torch_var_mean", "accumulate_rotating": "torch_var_mean", "normalize": "torch_normalize",
               "normalize_max": "torch_normalize_max", "max_only": "torch_normalize_max", "max_only_rotating": "torch_normalize_max"}
    out["times"] = {}
    for name, (lo, hi) in res.items():
        row = {"ms": round(lo, 4), "ms_max": round(hi, 4)}
        if name in floors:
            row.update(G_elements_per_s=round(elems / lo / 1e6, 2), hbm_floor_fraction=round(floors[name] / (lo * 1e3), 4),
                       of_score_all=round(lo / score_ms[0], 4), composition_over_kernel=round(res[against[name]][0] / lo, 2),
                       slowest_run_beats_fastest_composition=bool(hi <= res[against[name]][0]))
        out["times"][name] = row
    out["one_frame_update_us"] = round(res["one_frame_update"][0] * 1e3, 2)
    out["one_frame_normalize_max_us"] = round(res["one_frame_normalize_max"][0] * 1e3, 2)

    # the host route: copy the maps, numpy float64
    k = max(2, min(args.host_frames, n))
    host = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hv = maps[:k, 0].cpu().numpy()
        t1 = time.perf_counter()
        h64 = hv.astype(np.float64)
        hm, hs = h64.mean(0), h64.std(0, ddof=1)
        host.append((time.perf_counter() - t0, t1 - t0))
    best = min(host)
    out["host_route"] = {"frames": k, "ms_per_frame": round(best[0] * 1e3 / k, 3), "copy_ms_per_frame": round(best[1] * 1e3 / k, 3),
                         "ms_for_the_batch_scaled": round(best[0] * 1e3 / k * n, 1), "first_mean": float(hm[0, 0]), "first_std": float(hs[0, 0])}
    line = json.dumps(out)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
