"""Cost of the frame bank's gather (developer tool; not part of the product path).  In one run, alternated `--repeats` times,
device events after warm-up, best and worst reported:

  a. `vad_gather_frames_u8` alone: the training batch (32 clips x 10 frames of 256x256, fp32 NCHW out) and a scoring batch
     (512 frames, uint8 out), each against the HBM floor of its own bytes at --hbm-tbps (6.29);
  b. the same batches made by the torch composition a user has without the kernel,
     `bank[idx].permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5).contiguous()` (uint8: `bank[idx]`): the baseline;
  c. a bf16 `VideoTrainer.train_epoch` of --steps steps fed by `FrameBank.loader`, against the same number of steps on float
     batches made beforehand: the difference per step is what feeding from the bank costs inside an epoch.
The bank holds --bank-frames frames (default 4096 = 805 MB, more than the 256 MiB Infinity Cache), the clips start at random
frames.  Prints one JSON line; `--out FILE` also writes it there.

    python tools/frame_bank_bench.py [--size 256] [--bank-frames 4096] [--iters 20] [--warmup 5] [--repeats 3] [--steps 20] [--no-train]
"""
import argparse
import importlib
import itertools
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


def alternate(fns: dict, repeats: int, run) -> dict:
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(run(fn))
    return {k: (min(v), max(v)) for k, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--bank-frames", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--clip-len", type=int, default=10)
    ap.add_argument("--score-frames", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--hbm-tbps", type=float, default=6.29)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_bank_bench needs a GPU: a time is measured on the device or not at all")
    S, F, B, T = args.size, args.bank_frames, args.clips, args.clip_len
    gen = torch.Generator(device="cuda").manual_seed(1)
    bank = vad.FrameBank(S, capacity_frames=F)
    bank.add_video(torch.randint(0, 256, (F, S, S, 3), dtype=torch.uint8, device="cuda", generator=gen))      # one long video
    frames = bank.frames
    rng = np.random.default_rng(2)
    out = {"tool": "frame_bank_bench", "device": torch.cuda.get_device_name(0), "size": S, "bank_frames": F, "bank_MB": round(frames.numel() / 1e6, 1),
           "iters": args.iters, "repeats": args.repeats, "hbm_tbps": args.hbm_tbps, "gather": [], "epoch": None}

    # ---- a / b: the gather alone against the torch composition
    def clip_index(n_clips):
        starts = rng.integers(0, F - T + 1, n_clips)
        return torch.from_numpy((starts[:, None] + np.arange(T)[None, :]).reshape(-1).astype(np.int64)).cuda()

    cases = [("train_batch_f32", clip_index(B), torch.float32),
             ("score_batch_u8", torch.from_numpy(rng.integers(0, F, args.score_frames).astype(np.int64)).cuda(), torch.uint8)]
    for name, idx, dtype in cases:
        n = int(idx.numel())
        f32 = dtype == torch.float32
        dst = torch.empty((n, 3, S, S) if f32 else (n, S, S, 3), dtype=dtype, device="cuda")
        if f32:
            def torch_way(idx=idx):
                return frames[idx].permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5).contiguous()
        else:
            def torch_way(idx=idx):
                return frames[idx]
        kernel = bank.gather(idx, dtype, out=dst)
        diff = float((kernel.float() - torch_way().float()).abs().max())
        r = alternate({"kernel": lambda idx=idx, dst=dst, dtype=dtype: bank.gather(idx, dtype, out=dst), "torch": torch_way}, args.repeats,
                      lambda fn: timed(fn, args.iters, args.warmup))
        moved = n * S * S * 3 * (5 if f32 else 2)
        floor_us = moved / (args.hbm_tbps * 1e12) * 1e6
        out["gather"].append({"case": name, "frames": n, "bytes": moved, "hbm_floor_us": round(floor_us, 2),
                              "kernel_us": round(r["kernel"][0] * 1e3, 2), "kernel_us_max": round(r["kernel"][1] * 1e3, 2),
                              "kernel_floor_fraction": round(floor_us / (r["kernel"][0] * 1e3), 4),
                              "kernel_GBps": round(moved / r["kernel"][0] / 1e6, 1),
                              "torch_us": round(r["torch"][0] * 1e3, 2), "torch_us_max": round(r["torch"][1] * 1e3, 2),
                              "torch_over_kernel": round(r["torch"][0] / r["kernel"][0], 3), "max_abs_diff_to_torch": diff})
        del dst
        print(f"frame_bank_bench: {name} done", file=sys.stderr, flush=True)

    # ---- c: an epoch fed from the bank against the same steps on float batches made beforehand
    if not args.no_train:
        model = vad.VideoAutoencoder()
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vad.synth.synthetic_state(shapes, 3).items()})
        trainer = vad.VideoTrainer(model.cuda(), precision="bf16")
        stride = max(1, (F - T + 1) // (args.steps * B + B))
        loader = bank.loader(T, stride, B, shuffle=True, generator=torch.Generator().manual_seed(4), drop_last=True)
        assert len(loader) >= args.steps, (len(loader), args.steps)
        premade = [{"frames": b["frames"].clone()} for b in itertools.islice(loader, args.steps)]

        def epoch(batches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            trainer.train_epoch(batches)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / args.steps

        fns = {"bank": lambda: itertools.islice(loader, args.steps), "premade": lambda: premade}
        epoch(premade[:3])                                       # warm-up: workspace, first-call set-up
        r = alternate(fns, args.repeats, lambda make: epoch(make()))
        out["epoch"] = {"steps": args.steps, "clips": B, "clip_len": T, "precision": "bf16",
                        "bank_ms_per_step": round(r["bank"][0], 4), "bank_ms_per_step_max": round(r["bank"][1], 4),
                        "premade_ms_per_step": round(r["premade"][0], 4), "premade_ms_per_step_max": round(r["premade"][1], 4),
                        "extra_us_per_step": round((r["bank"][0] - r["premade"][0]) * 1e3, 2),
                        "frames_per_s_bank": round(B * T / r["bank"][0] * 1e3, 1), "frames_per_s_premade": round(B * T / r["premade"][0] * 1e3, 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
