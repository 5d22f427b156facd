"""CPU checks of the scoring entry points' host code (csrc/vad_api.hip): workspace sizes, what a call launches and where in the
workspace each launch points, and what a call with one bad argument answers - all against fixtures recorded from the library as
it was when every workspace layout was written twice (a size formula and a pointer walk) and every entry point spelled out its
own argument checks.  No GPU needed: the library loads without one, and tests/score_launch_trace.cpp stands in for HIP.

`VAD_LIB=<libvad_hip.so of the commit to record from> python tests/test_scoring_plan.py <that commit>` rewrites the fixtures;
with `add-refusals` behind the commit it only ADDS the refusal cases that scoring_refusals.json does not hold yet: every recorded
entry must come out as recorded, and the file's source line gains the commit the new ones were recorded from."""
import itertools
import json
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

from conftest import GOLDEN

PREC = {"fp32": 0, "split": 1, "winograd": 4}


@pytest.fixture(scope="module")
def lib(vad):
    return vad.hip.lib()


# ------------------------------------------------------------------------------ A. sizes
def size_grids(vad):
    """name -> (size function, axes in call order); vid / windows: `cfg` is (latent, hid), `stride` 0 / 1 / 2 stands for 1 / t / t + 1."""
    hip = vad.hip
    chunks, ts, layers = [1, 2, 7, 127, 128], [1, 3, 16], [1, 2, 3, 8]        # 16x16, hid 128: chunk 127 | 128 is the 256-work-group threshold
    vhw, cfg = [(16, 16), (16, 32), (48, 32), (256, 256)], [(32, 32), (32, 64), (100, 100), (64, 128), (256, 256)]
    return {
        "vad_img_workspace_bytes_c": ([1, 2, 16], [(16, 16), (16, 48), (32, 16), (256, 256), (250, 256)], [1, 32, 100, 256, 2049, hip.MAX_WIDTH + 1],
                                      [2, 3, 5, hip.MAX_IN_CHANNELS + 1]),
        "vad_vid_workspace_bytes_c": (chunks, ts, vhw, cfg, layers, [3, 5]),
        "vad_vid_windows_workspace_bytes_c": (chunks, ts, [0, 1, 2], vhw, cfg, layers, [3, 5]),
        "vad_convlstm_seq_workspace_bytes": ([1, 2, 127, 128], [1, 3], [(1, 1), (3, 5), (16, 16)], [32, 64], [64, 128], [1, 2, 8], [0, 1]),
    }


def sizes(l, name, axes):
    fn, res = getattr(l, name), []
    for point in itertools.product(*axes):
        args = [v for a in point for v in (a if isinstance(a, tuple) else (a,))]
        if name == "vad_vid_windows_workspace_bytes_c":
            args[2] = (1, args[1], args[1] + 1)[args[2]]
        res.append(fn(*args))
    return res


def test_workspace_sizes_are_the_recorded_ones(vad, lib):
    table = json.loads((GOLDEN / "scoring_ws_bytes.json").read_text())
    for name, axes in size_grids(vad).items():
        assert table[name]["axes"] == json.loads(json.dumps(axes)), name
        got = sizes(lib, name, axes)
        assert len(got) > 300 and got == table[name]["bytes"], name
    assert lib.vad_vid_workspace_bytes(2, 3, 16, 32, 32, 64, 2) == lib.vad_vid_workspace_bytes_c(2, 3, 16, 32, 32, 64, 2, 3) > 0
    assert lib.vad_vid_windows_workspace_bytes(2, 3, 1, 16, 32, 32, 64, 2) == lib.vad_vid_windows_workspace_bytes_c(2, 3, 1, 16, 32, 32, 64, 2, 3) > 0
    assert lib.vad_img_workspace_bytes(2, 16, 48, 100) == lib.vad_img_workspace_bytes_c(2, 16, 48, 100, 5) > 0


# ------------------------------------------------------------------------------ B. launches, streams, events, workspace offsets
def launch_script():
    """The scoring cases of tests/test_hip_workspace.py as lines for tests/score_launch_trace.cpp, each under every switch setting
    and output selection, in groups of one digest each."""
    import test_hip_workspace as W
    ch = lambda cin: max(cin, 3)                 # (fewer than 3 planes are zero-widened by the Python layer)
    img = [f"img {int(u8)} {PREC[p]} {ch(cin)} {b} {h} {w} {latent} {chunk}" for cin, latent, h, w, b, chunk, p, _, u8 in W.IMG_CASES if ch(cin) == 3 or not u8]
    img.append("img 0 0 3 3 16 16 2049 2")       # test_image_scoring_workspace_wide_latent
    vid = [f"vid {int(u8)} {PREC[p]} {ch(cin)} {b} {t} {h} {w} {latent} {hid} {layers} {chunk}"
           for cin, latent, hid, layers, h, w, b, t, chunk, p, u8 in W.VID_CASES]
    win = [f"win 0 {PREC[p]} 3 11 4 {stride} 16 32 32 64 {layers} 2" for stride in (1, 3) for layers, p in ((1, "fp32"), (2, "winograd"))]
    stateful = [f"vid 0 {PREC[p]} 3 3 1 16 32 {latent} {hid} {layers} 2" for latent, hid, layers, p in ((32, 32, 1, "fp32"), (32, 64, 2, "winograd"), (100, 100, 2, "split"))]
    # the ConvLSTM module's cases (b 2, t 3, a 3 x 5 grid; hidden 32 | 40 pad to 64), equal widths in every arithmetic, and both sides
    # of the 256-work-group threshold
    seq = [f"seq 0 2 3 3 5 32 64 {layers} {al}" for layers in (1, 2) for al in (0, 1)]
    seq += [f"seq {p} 2 3 3 5 64 64 {layers} {al}" for p in (0, 1, 4) for layers in (1, 3) for al in (0, 1)]
    seq += [f"seq 0 {b} 2 1 1 64 128 2 0" for b in (127, 128)]
    with_outputs = lambda lines, masks: [f"{line} {m}" for line in lines for m in masks]
    families = {"img": with_outputs(img, (15, 1, 8)),                        # everything; scores only; latent only
                "vid": with_outputs(vid, (15, 3, 32)),                       # everything; scores only; state only
                "win": with_outputs(win, (15, 3)),
                "stateful": with_outputs(stateful, (15 + 48, 3 + 16, 32, 48)),
                "seq": with_outputs(seq, (0, 1, 2, 3))}
    out = []
    for wf, cv in itertools.product((0, 1, 2), (1, 33, 65)):
        out += [f"set vad_debug_set_lstm_wavefront {wf}", f"set vad_debug_set_conv_variant {cv}"]
        for name, lines in families.items():
            out += [f"group {name}-wf{wf}-cv{cv}"] + lines
    out.append("set vad_debug_set_lstm_wavefront 1")
    for cv, fused, tg in itertools.product((1, 33, 65), (0, 1), (0, 1)):
        out += [f"set vad_debug_set_conv_variant {cv}", f"set vad_debug_set_dec4_fused {fused}", f"set vad_debug_set_tail_group {tg}",
                f"group img-cv{cv}-fused{fused}-tg{tg}"] + families["img"]
    return "\n".join(out) + "\n"


def build_tracer(lib_path, workdir):
    """tests/score_launch_trace.cpp compiled, and the library's kernel symbols in the file it reads -> (program, symbol file)"""
    exe, syms = (Path(workdir) / n for n in ("score_launch_trace", "kernels.txt"))
    src = Path(__file__).with_name("score_launch_trace.cpp")
    subprocess.run([shutil.which("g++") or shutil.which("c++"), "-O1", "-std=c++17", "-rdynamic", "-o", str(exe), str(src), "-ldl"], check=True)
    table = [line.split() for line in subprocess.run(["nm", str(lib_path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    syms.write_text("".join(f"{t[0]} {t[2]}\n" for t in table if len(t) == 3 and "kernel" in t[2]))
    return exe, syms


def launch_digests(lib_path, workdir):
    exe, syms = build_tracer(lib_path, workdir)
    script = Path(workdir) / "script.txt"
    script.write_text(launch_script())
    out = subprocess.run([str(exe), str(lib_path), str(syms), str(script)], check=True, capture_output=True, text=True).stdout.split()
    return dict(zip(out[0::3], out[2::3])), sum(map(int, out[1::3]))


def test_launches_are_the_recorded_ones(vad, tmp_path):
    """Kernel, grid, block, LDS, stream and workspace offsets of every launch, and every event record / wait, of the scoring cases
    under the wavefront, hoisting, gate-split and tail switches (tests/golden/scoring_launches.json)."""
    want = json.loads((GOLDEN / "scoring_launches.json").read_text())
    got, calls = launch_digests(vad.hip.LIB_PATH, tmp_path)
    assert calls == want["calls"] > 3000
    assert len(got) == 9 * 5 + 12 and got == want["fnv1a64"]


# ------------------------------------------------------------------------------ B2. the planning override
PLAN_CALLS = ("img 0 0 3 1 64 64 256 1 15", "vid 0 0 3 1 4 64 64 128 128 2 1 15")      # one 64 x 64 frame; one clip of four


def traced_launches(exe, lib_path, syms, workdir, plan_cus):
    """The tracer's `dump` text of PLAN_CALLS under vad_debug_set_plan_cus(plan_cus) -> per call a list of (kernel name, its
    integer template arguments, grid.x), and the group's digest."""
    script = Path(workdir) / f"plan{plan_cus}.txt"
    script.write_text(f"set vad_debug_set_plan_cus {plan_cus}\ngroup plan\n" + "\n".join(PLAN_CALLS) + "\n")
    run = subprocess.run([str(exe), str(lib_path), str(syms), str(script), "dump"], check=True, capture_output=True, text=True)
    calls = []
    for line in run.stderr.splitlines():
        if line in PLAN_CALLS:
            calls.append([])
        elif line.startswith(" L "):
            _, sym, grid = line.split()[:3]
            name = re.match(r"_Z(?:N\d+_GLOBAL__N_1)?(\d+)", sym)         # (the fused tail's kernel lives in an unnamed namespace)
            start = name.end()
            calls[-1].append((sym[start:start + int(name.group(1))], tuple(int(v) for v in re.findall(r"Li(\d+)E", sym)), int(grid.split(",")[0])))
        elif line.startswith(" ws "):
            assert " rc 0" in line, line
    assert len(calls) == len(PLAN_CALLS)
    return calls, run.stdout.split()[2]


def is_persistent(name):
    return "pkernel" in name or name == "dec4_score_kernel"


def test_plan_cus_override_reaches_every_planner(vad, tmp_path):
    """vad_debug_set_plan_cus(1) under the tracer (256 CUs assumed, occupancy 2): a one-frame image call and a one-clip video call
    take the throughput tilings of every convolution - conv3x3 (2,2,2,2), (1,2,2,2), (2,2,4,1), convt2x2 (2,4) - instead of the
    latency tilings and the gate-split kernel, and every persistent grid shrinks; with the switch at 0 the launches are the ones
    recorded without it."""
    exe, syms = build_tracer(vad.hip.LIB_PATH, tmp_path)
    (img0, vid0), digest0 = traced_launches(exe, vad.hip.LIB_PATH, syms, tmp_path, 0)
    (img1, vid1), digest1 = traced_launches(exe, vad.hip.LIB_PATH, syms, tmp_path, 1)
    assert digest0 != digest1
    tiling = lambda launch: launch[1][1:5]                                   # conv3x3_mfma_pkernel<CK, MT, NT, WM, WN, ...>
    conv = lambda call: {tiling(k) for k in call if k[0] == "conv3x3_mfma_pkernel"}
    convt = lambda call: {k[1][:2] for k in call if k[0] == "convt2x2_pkernel"}
    latency = {(1, 1, 2, 2)}
    for dflt, one in ((img0, img1), (vid0, vid1)):
        assert conv(dflt) & latency and not conv(one) & latency
        assert any(k[0] == "convlstm_gate_kernel" for k in dflt) and not any(k[0] == "convlstm_gate_kernel" for k in one)
        assert {(2, 2, 2, 2), (1, 2, 2, 2), (2, 2, 4, 1)} <= conv(one)
        assert convt(dflt) == {(1, 1)} and convt(one) == {(2, 4)}
    # the image call launches one kernel per layer either way: launch by launch, a persistent grid under the one-CU plan is
    # smaller - or, where both plans launch the same frame-walking instantiation on the call's one frame, the same: that grid is
    # the work-group positions of one frame whatever the cap (the fused first layer and the cout-32 convolution of dec4)
    assert len(img0) == len(img1) and sum(is_persistent(k[0]) for k in img1) >= 14
    same = 0
    for k0, k1 in zip(img0, img1):
        if not is_persistent(k1[0]):
            assert k0 == k1
        elif k0[:2] == k1[:2] and k1[0] == "conv3x3_mfma_pkernel":
            assert k1[2] == k0[2]
            same += 1
        else:
            assert k1[2] < k0[2], (k0, k1)
    assert same == 2
    # the video call launches another sequence (x halves per step); per kernel family every grid is smaller than any of the default's
    for family in ("conv3x3_c3_pkernel", "conv3x3_mfma_pkernel", "convt2x2_pkernel"):
        g0, g1 = [k[2] for k in vid0 if k[0] == family], [k[2] for k in vid1 if k[0] == family]
        assert g0 and g1 and max(g1) < min(g0), family
    # occupancy 2 x one CU: item walkers launch two work-groups, frame walkers the positions of one frame
    assert all(k[2] <= 2 for call in (img1, vid1) for k in call if k[0] in ("conv3x3_c3_pkernel", "convt2x2_pkernel", "dec4_score_kernel"))
    # and back at 0 the recorded digests hold (test_launches_are_the_recorded_ones runs the whole script; here: the same two calls)
    assert traced_launches(exe, vad.hip.LIB_PATH, syms, tmp_path, 0)[1] == digest0


# ------------------------------------------------------------------------------ C. refusals
X, PACKED, WS, OUT, STATE, STREAM = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000    # never dereferenced: every check comes first


def refusal_cases(vad):
    """entry point -> (argument names, valid values, the size function's arguments, [(label, {name: bad value})])."""
    hip = vad.hip
    outs = lambda *names: {n: OUT + 0x100000 * i for i, n in enumerate(names)}
    common = [("bad precision", dict(precision=2)), ("bad format", dict(x_format=2)), ("in_ch 2", dict(in_ch=2)),
              ("in_ch max+1", dict(in_ch=hip.MAX_IN_CHANNELS + 1)), ("uint8 with in_ch 5", dict(x_format=1, in_ch=5)), ("h 250", dict(h=250)),
              ("latent 0", dict(latent=0)), ("latent max+1", dict(latent=hip.MAX_WIDTH + 1)), ("chunk 0", dict(chunk=0)), ("workspace one byte short", dict(ws_bytes=-1)),
              ("misaligned workspace", dict(ws=WS + 16)), ("misaligned weights", dict(packed=PACKED + 4))]
    nulls = lambda *names: [(f"null {n}", {n: None}) for n in names]
    none_of = lambda *names: [("no output requested", {n: None for n in names})]
    img = dict(x=X, x_format=0, precision=0, in_ch=3, b=3, h=16, w=48, latent=32, packed=PACKED, ws=WS, ws_bytes=0, chunk=2,
               **outs("scores", "errmap", "recon", "latent_out"), stream=STREAM)
    vid = dict(x=X, x_format=0, precision=0, in_ch=3, b=3, t=2, h=16, w=32, latent=32, hid=64, layers=2, packed=PACKED, ws=WS, ws_bytes=0, chunk=2,
               **outs("seq_scores", "frame_scores", "errmap", "recon"), state_in=STATE, state_out=STATE + 0x100000, stream=STREAM)
    win = dict(x=X, x_format=0, precision=0, in_ch=3, nframes=9, t=4, stride=3, h=16, w=32, latent=32, hid=64, layers=2, packed=PACKED, ws=WS, ws_bytes=0,
               chunk=2, **outs("seq_scores", "frame_scores", "errmap", "recon"), stream=STREAM)
    seq = dict(x=X, precision=0, b=2, t=3, gh=3, gw=5, cin_p=32, hid_p=64, layers=2, packed=PACKED, ws=WS, ws_bytes=0, hseq_out=OUT, all_layers=0,
               state_in=STATE, state_out=STATE + 0x100000, stream=STREAM)
    misaligned_state = [("misaligned state_in", dict(state_in=STATE + 4)), ("misaligned state_out", dict(state_out=STATE + 4))]
    # one pixel more than the kernels' 24-bit pixel indices hold (VAD_MAX_FRAME_PIXELS = 2^23 - 1); recorded behind the older cases
    too_large = [("frame of 2^23 pixels", dict(h=4096, w=2048))]
    return {
        "vad_img_score_c": (img, "vad_img_workspace_bytes_c", ("chunk", "h", "w", "latent", "in_ch"),
                            nulls("x", "packed", "ws") + common + none_of("scores", "errmap", "recon", "latent_out") + too_large),
        "vad_vid_score_s": (vid, "vad_vid_workspace_bytes_c", ("chunk", "t", "h", "w", "latent", "hid", "layers", "in_ch"),
                            nulls("x", "packed", "ws") + common + none_of("seq_scores", "frame_scores", "errmap", "recon", "state_out") + misaligned_state + too_large),
        "vad_vid_score_windows_c": (win, "vad_vid_windows_workspace_bytes_c", ("chunk", "t", "stride", "h", "w", "latent", "hid", "layers", "in_ch"),
                                    nulls("x", "packed", "ws") + common + none_of("seq_scores", "frame_scores", "errmap", "recon")
                                    + [("stride > T", dict(stride=5)), ("frames < T", dict(nframes=3))] + too_large),
        "vad_convlstm_seq": (seq, "vad_convlstm_seq_workspace_bytes", ("b", "t", "gh", "gw", "cin_p", "hid_p", "layers", "all_layers"),
                             nulls("x", "packed", "ws", "hseq_out") + [c for c in common if c[0] in ("bad precision", "workspace one byte short", "misaligned workspace", "misaligned weights")]
                             + misaligned_state + [("misaligned x", dict(x=X + 4)), ("cin_p != hid_p in split mode", dict(precision=1)),
                                                   ("grid of 2^23 positions", dict(gh=4096, gw=2048))]),
    }


def refusals(vad, l):
    res = {}
    for entry, (valid, size_fn, size_args, faults) in refusal_cases(vad).items():
        need = getattr(l, size_fn)(*[valid[k] for k in size_args])
        assert need > 1, entry
        for label, bad in faults:
            args = dict(valid, ws_bytes=need)
            args.update({k: need - 1 if k == "ws_bytes" else v for k, v in bad.items()})
            rc = getattr(l, entry)(*args.values())
            res[f"{entry}: {label}"] = [rc, l.vad_last_error().decode()]
    return res


def test_refusals_are_the_recorded_ones(vad, lib):
    """Return code and vad_last_error() text of calls with ONE bad argument.  Every check runs before the first HIP call."""
    want = json.loads((GOLDEN / "scoring_refusals.json").read_text())["refusals"]
    got = refusals(vad, lib)
    assert len(got) == 17 + 19 + 19 + 13 and all(rc < 0 and text for rc, text in got.values())
    assert got == want
    over = {k: v for k, v in got.items() if "2^23" in k}
    assert len(over) == 4 and all(rc == -1 and str(PIXEL_LIMIT) in text for rc, text in over.values()), over


PIXEL_LIMIT = 2 ** 23 - 1                      # VAD_MAX_FRAME_PIXELS: the largest frame whose pixel indices fit a 24-bit multiply operand
OVER = [(4096, 2048), (2048, 4096), (16, 2 ** 19), (4112, 2048)]          # 2^23 pixels three ways, and the next multiple of 16 rows
UNDER = (4096, 2032)                           # 8,323,072 pixels: the largest 4096-row frame of 16-pixel steps below the limit


def test_size_queries_refuse_frames_over_the_pixel_limit(vad, lib):
    """Every workspace query answers 0 for a frame of 2^23 pixels or more - the scoring ones, the ConvLSTM roll-out's and the
    trainers' - and a size for the largest frame below."""
    queries = {
        "vad_img_workspace_bytes": lambda h, w: (1, h, w, 32),
        "vad_img_workspace_bytes_c": lambda h, w: (1, h, w, 32, 3),
        "vad_vid_workspace_bytes": lambda h, w: (1, 1, h, w, 32, 32, 1),
        "vad_vid_workspace_bytes_c": lambda h, w: (1, 1, h, w, 32, 32, 1, 3),
        "vad_vid_windows_workspace_bytes": lambda h, w: (1, 2, 1, h, w, 32, 32, 1),
        "vad_vid_windows_workspace_bytes_c": lambda h, w: (1, 2, 1, h, w, 32, 32, 1, 3),
        "vad_convlstm_seq_workspace_bytes": lambda h, w: (1, 1, h, w, 32, 64, 1, 0),
        "vad_img_train_workspace_bytes": lambda h, w: (1, h, w, 32),
        "vad_vid_train_workspace_bytes": lambda h, w: (1, 1, h, w, 32, 32, 1),
        "vad_vid_train_workspace_bytes_l": lambda h, w: (1, 1, h, w, 32, 32, 1, 2),
    }
    for name, args in queries.items():
        fn = getattr(lib, name)
        assert fn(*args(*UNDER)) > 0, name
        for h, w in OVER:
            assert fn(*args(h, w)) == 0, (name, h, w)


def layer_refusal_cases(l):
    """Layer entry point -> a call of it on one h x w frame with dummy, never-dereferenced pointers."""
    P = X                                      # any non-null, 16-B aligned address
    return {
        "conv3x3": lambda h, w: l.vad_conv3x3(P, 0, P, P, P, 0, 1, h, w, 32, 32, 1, 0, 0, None),
        "conv3x3 pooled, split": lambda h, w: l.vad_conv3x3(P, 0, P, P, P, 0, 1, h, w, 32, 32, 1, 1, 1, None),
        "conv3x3_wino": lambda h, w: l.vad_conv3x3_wino(P, 0, P, P, P, 0, 1, h, w, 32, 32, 1, 0, None),
        "convlstm_step": lambda h, w: l.vad_convlstm_step(P, 0, None, 0, None, P, P, P, 0, P, 1, h, w, 32, 64, 0, None),
        "convlstm_step_wino": lambda h, w: l.vad_convlstm_step_wino(P, 0, None, 0, None, P, P, P, 0, P, P, 1, h, w, 32, 32, None),
        "conv3x3_c3": lambda h, w: l.vad_conv3x3_c3(P, P, P, P, 1, h, w, 32, 1, 0, None),
        "conv3x3_c3 pooled": lambda h, w: l.vad_conv3x3_c3(P, P, P, P, 1, h, w, 32, 1, 1, None),
        "conv3x3_c3_fused": lambda h, w: l.vad_conv3x3_c3_fused(P, P, P, P, P, P, 1, h, w, 0, None),
        "conv3x3_c3_fused split": lambda h, w: l.vad_conv3x3_c3_fused(P, P, P, P, P, P, 1, h, w, 1, None),
        "convt2x2": lambda h, w: l.vad_convt2x2(P, 0, P, P, P, 0, 1, h, w, 32, 32, 2, 0, None),
        "dec4_score": lambda h, w: l.vad_dec4_score(P, P, P, P, P, P, P, P, P, 1, h, w, None),
    }


def test_layer_entry_points_refuse_frames_over_the_pixel_limit(lib):
    """One bad argument - a frame of 2^23 pixels or more - at every layer entry point whose kernel multiplies a pixel index as a
    24-bit operand (and at vad_conv3x3_c3, the first layer in front of them): VAD_ERR_ARG before the first HIP call, and the
    message names the limit.  The un-pooled first layer also counts its output in BYTES: 128 channels of a 4096 x 1024 frame are
    2^29 elements but 2^31 bytes, the limit of every other layer's offsets inside one frame."""
    for name, call in layer_refusal_cases(lib).items():
        for h, w in OVER:
            assert call(h, w) == -1, (name, h, w)
            text = lib.vad_last_error().decode()
            assert name.split()[0] + ":" in text and str(PIXEL_LIMIT) in text and f"{h}x{w}" in text, (name, text)
    assert lib.vad_conv3x3_c3(X, X, X, X, 1, 4096, 1024, 128, 0, 0, None) == -1
    assert "2^31 bytes" in lib.vad_last_error().decode()
    # the bf16 1x1 convolution runs a pixel count that is no multiple of 16 as ONE ragged frame of 16-pixel rows: the same limit
    # (VAD_PREC_BF16S = 3)
    assert lib.vad_conv1x1_p(X, X, X, X, 2 ** 23 + 1, 32, 32, 3, None) == -1
    text = lib.vad_last_error().decode()
    assert "conv1x1 (bf16):" in text and str(PIXEL_LIMIT) in text, text
    # the trainers refuse the same frames before anything is launched (their plans; dummy pointers, a workspace of any size)
    for h, w in OVER:
        assert lib.vad_img_train_fwd_bwd(X, 1, h, w, 32, X, X, X, X, 1 << 40, 0, 0.0, 11, 0, X, None, None) == -1
        assert str(PIXEL_LIMIT) in lib.vad_last_error().decode()
        assert lib.vad_vid_train_fwd_bwd(X, 1, 1, h, w, 32, 32, 1, X, X, X, X, 1 << 40, 0, X, None, None) == -1
        assert str(PIXEL_LIMIT) in lib.vad_last_error().decode()


if __name__ == "__main__":                     # record the fixtures from the library VAD_LIB names
    import importlib
    import tempfile
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    pkg = importlib.import_module("video-anomaly-detection_amd")
    source, l = f"recorded from commit {sys.argv[1]}", pkg.hip.lib()
    dump = lambda name, obj: (GOLDEN / name).write_text(json.dumps(dict(source=source, **obj), separators=(",", ":")) + "\n")
    if sys.argv[2:] == ["add-refusals"]:
        old, now = json.loads((GOLDEN / "scoring_refusals.json").read_text()), refusals(pkg, l)
        changed = [k for k, v in old["refusals"].items() if now.get(k) != v]
        assert not changed, f"recorded refusals came out differently: {changed}"
        added = [k for k in now if k not in old["refusals"]]
        source = f"{old['source']}; new cases recorded from commit {sys.argv[1]}"
        dump("scoring_refusals.json", dict(refusals=now))
        print(source, pkg.hip.LIB_PATH, "added", added)
        sys.exit(0)
    dump("scoring_ws_bytes.json", {name: dict(axes=axes, bytes=sizes(l, name, axes)) for name, axes in size_grids(pkg).items()})
    dump("scoring_refusals.json", dict(refusals=refusals(pkg, l)))
    with tempfile.TemporaryDirectory() as tmp:
        digests, calls = launch_digests(pkg.hip.LIB_PATH, tmp)
    dump("scoring_launches.json", dict(stubs="device properties query fails (256 CUs assumed), occupancy query answers 2", calls=calls, fnv1a64=digests))
    print(source, pkg.hip.LIB_PATH, calls, "traced calls")
