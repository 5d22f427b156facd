"""The N > 1 form of bench.py, exactly as the driver launches it (`python -m torch.distributed.run --nproc-per-node N
bench.py --gpus N ...`), rehearsed on the one GPU of the test box: two ranks share device 0 over gloo (RCCL needs one device
per rank; the code path - block partition, no data-path collective, ONE all_gather of the score vector per step, max-over-
ranks timing - is the same).  The JSON line must verify itself: both ranks' devices listed, the collective timed, and rank
0's comparison of the GATHERED vector with the CPU oracle on one frame from every rank's block within 1e-4."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# world 4 = the largest rehearsal a GPU box allows from inside the test session (at most 6 processes may hold the card: the
# session itself + 4 ranks); image: 8 frames per rank per step and a ragged 1,030-frame stream (blocks of 258, the last 256),
# video: ONE clip per rank.  The 8-rank form of the same host logic runs on CPU ranks in tests/test_sharding.py.
@pytest.mark.parametrize("world,workload,extra", [(2, "image", ["--batch", "24", "--size", "64"]),       # with the split / winograd objects
                                                  (2, "video", ["--batch", "3", "--clip-len", "4", "--size", "64", "--no-split"]),
                                                  (4, "image", ["--batch", "8", "--size", "64", "--stream-frames", "1030", "--no-split"]),
                                                  (4, "video", ["--batch", "1", "--clip-len", "10", "--size", "64", "--no-split"])])
def test_multi_rank_bench_line_verifies_itself(world, workload, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(REPO / "bench.py"), "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--share-gpu", "--workload", workload, "--full", "--no-train", *extra]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                    # rank 0 prints ONE JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["scaling"] == "weak" and d["value"] > 0 and d["steps"] == 2
    mg = d["multi_gpu"]
    assert mg["world_size"] == world and mg["backend"] == "gloo" and [r["rank"] for r in mg["ranks"]] == list(range(world))
    assert mg["allgather_ms"] > 0 and len(mg["parity"]["checked_items"]) == world      # one item out of EVERY rank's block
    per = d["config"]["frames_per_gpu_per_step"] // (10 if (workload == "video" and world == 4) else 4 if workload == "video" else 1)
    assert [i // per for i in mg["parity"]["checked_items"]] == list(range(world))
    assert mg["parity"]["within_1e-4"] and mg["parity"]["max_rel_score_err_vs_cpu"] < 1e-5
    assert "cpu_baseline" not in d                                 # the CPU baseline is an N = 1 measurement
    if "--no-split" not in extra:                                  # the opt-in modes ride in the N > 1 line too, never as `value`
        assert d["dtype"] == "f32"
        for mode in ("split_precision", "winograd_precision"):
            assert d[mode]["value"] > 0 and d[mode]["max_rel_score_diff_vs_exact_fp32"] < 1e-5, mode
    if "--stream-frames" in extra:                                 # configs[3] on `world` ranks with a ragged tail
        st = d["stream"]
        assert st["frames"] == 1030 and st["frames_per_rank"] == 258 and st["scaling"] == "strong" and st["value"] > 0
        pr = st["parity"]                                          # one frame of every rank's block + the very last frame
        assert [f // 258 for f in pr["checked_frames"]] == [0, 1, 2, 3, 3] and pr["checked_frames"][-1] == 1029
        assert pr["within_1e-4"] and pr["max_rel_score_err_vs_cpu"] < 1e-5


def test_default_bench_line_carries_every_single_gpu_object():
    """`python bench.py --gpus 1 --steps K --warmup W --full`: ONE JSON line with the contract's fields, the
    roofline and cpu_baseline objects of configs[1], and - as secondary objects that never enter `value` - configs[2] with its
    own roofline / cpu_baseline, the configs[3] stream on one rank, the training step and the reference's own call sizes."""
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"]
    out = subprocess.run(cmd, cwd=REPO, env=dict(os.environ), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["vs_baseline"] is None and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("port", "reference") and c["sample"]
    assert d["value"] > 100 * c["value"]                                     # frames/s on the GPU vs the CPU restatement
    # the line's own parity statement: the scores of the timed steps against the CPU restatement on the baseline's sample
    # (north_star's bar is 1e-4; the exact-fp32 path is held to 1e-5 - it measured 1.7e-7)
    assert c["gpu_vs_cpu_max_rel_score_err"] < 1e-5
    # `traffic` is a number only when the committed counter file was measured on these very kernel sources
    assert (r["traffic"] is None) == r["traffic_source"].startswith("null:"), r["traffic_source"]
    v = d["video"]
    assert v["value"] > 0 and 0 < v["roofline"]["frac"] < 1 and v["cpu_baseline"]["value"] > 0
    assert v["cpu_baseline"]["gpu_vs_cpu_max_rel_score_err"] < 1e-5
    assert d["stream"]["frames"] == 100000 and d["stream"]["value"] > 0 and d["stream"]["parity"]["max_rel_score_err_vs_cpu"] < 1e-5
    assert d["training_step"]["bf16_precision"]["value"] > 0 and d["split_precision"]["value"] > 0
    rc = d["reference_call_sizes"]
    assert set(rc) == {"image_batch_1", "image_batch_16", "video_4x16", "video_1x16"} and all(x["ms"] > 0 for x in rc.values())


@pytest.mark.parametrize("workload,extra", [("image", ["--batch", "16", "--size", "64"]), ("video", ["--batch", "4", "--clip-len", "5", "--size", "64"])])
def test_bench_line_with_an_opt_in_mode_as_the_timed_path_says_so(workload, extra):
    """`bench.py --precision winograd`: the opt-in arithmetic as the timed path must be visible in the line itself - `dtype` names
    it, no secondary-mode objects ride along, and the CPU baseline's parity figure is that of the mode (still inside 1e-5)."""
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--precision", "winograd",
           "--workload", workload, "--full", "--no-train", "--no-small", *extra]
    out = subprocess.run(cmd, cwd=REPO, env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert "Winograd" in d["dtype"] and d["value"] > 0 and d["vs_baseline"] is None
    assert 0 < d["roofline"]["frac"] < 1 and "executed" in d["roofline"]["flops"]       # executed matrix FLOPs, not algorithmic ones
    assert "split_precision" not in d and "winograd_precision" not in d
    assert d["cpu_baseline"]["gpu_vs_cpu_max_rel_score_err"] < 1e-5


# A plain line (no --full): the headline steps only.  `--dump-outputs` must hand back what the timed path returned in its last
# step, on inputs fixed by the arguments alone: the dumped scores are checked against the CPU oracle on a few items of the same
# seeded frames and weights bench.py builds (image: state seed 7, frame seed 0xC0FFEE + 1; video: state seed 8, seed 0xC0FFEE + 2).
@pytest.mark.parametrize("workload,extra,shape", [("image", [], (512,)),
                                                  ("video", ["--batch", "3", "--clip-len", "4", "--size", "64"], (3, 4))])
def test_plain_bench_line_is_lean_and_dumps_the_timed_scores(vad, tmp_path, workload, extra, shape):
    import numpy as np
    import torch
    from conftest import synthetic_state_for
    from oracle import torch_oracle
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", workload,
           "--dump-outputs", str(tmp_path / "out"), *extra]
    out = subprocess.run(cmd, cwd=REPO, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    fps = d["config"]["frames_per_gpu_per_step"] / (d["ms_per_step"] * 1e-3)
    assert abs(d["value"] - fps) <= 0.01 * fps
    for k in ("layers", "cpu_baseline", "split_precision", "winograd_precision", "stream", "video", "training_step",
              "reference_call_sizes", "multi_gpu"):
        assert k not in d, k
    assert d["roofline"] is None
    got = np.load(tmp_path / "out" / "scores.npy")
    assert got.dtype == np.float32 and got.shape == shape and np.all(np.isfinite(got))
    hw = 64 if "--size" in extra else 256
    items = [0, shape[0] // 2, shape[0] - 1]
    if workload == "image":
        m = vad.ConvAutoencoder(in_channels=3, latent_dim=256)
        st = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_for(vad, m, 7).items()}
        xs = torch.from_numpy(np.concatenate([vad.synth.frames(0xC0FFEE + 1, i, 1, 3, hw, hw) for i in items]))
        with torch.no_grad():
            ref = torch_oracle.img_scores(st, xs)["scores"].numpy()
    else:
        m = vad.VideoAutoencoder(in_channels=3, latent_dim=128, lstm_hidden_dim=128, lstm_num_layers=2)
        st = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_for(vad, m, 8).items()}
        xs = torch.from_numpy(np.concatenate([vad.synth.clips(0xC0FFEE + 2, i, 1, shape[1], 3, hw, hw) for i in items]))
        with torch.no_grad():
            ref = torch_oracle.vid_scores(st, xs, 128, 2)["frame"].numpy()
    rel = float(np.max(np.abs(got[items] - ref) / np.abs(ref)))
    assert rel < 1e-5, rel
