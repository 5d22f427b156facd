"""The host half of the event tracker (csrc/map_track.hip, metrics.EventTracker) on a machine without a GPU: the frame-by-frame
numpy restatement (tests/track_ref.py) against tests/events_ref.py on whole volumes and on every prefix - the defining equalities
of DESIGN.md section 4.19 -, the lost rule, the state and workspace sizes, the launch plan, and every refusal the host makes before
it launches anything."""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import events_ref
import track_ref as ref

metrics = importlib.import_module("video-anomaly-detection_amd.metrics")
scoring = importlib.import_module("video-anomaly-detection_amd.scoring")
hip = importlib.import_module("video-anomaly-detection_amd.hip")
REPO = Path(__file__).resolve().parent.parent

MODES = ((4, 1), (8, 1), (8, 9))
SHAPES = ((6, 9, 11), (1, 7, 5), (7, 1, 1), (1, 1, 1), (3, 1, 13), (4, 12, 1), (9, 5, 5))
FILTERS = ((1, 1), (2, 1), (1, 3), (3, 4))
BIG = 4096


def _volume(rng, shape, density):
    """Distinct values, so that peaks have no ties; foreground = the `density` largest share."""
    n = int(np.prod(shape))
    vol = rng.permutation(np.linspace(-1.0, 1.0, n, dtype=np.float32)).reshape(shape)
    thr = np.sort(vol.reshape(-1))[min(n - 1, int((1.0 - density) * n))]
    return vol, thr


def _splits(rng, t):
    out = [(t,), (1,) * t]
    if t >= 3:
        a = int(rng.integers(1, t - 1))
        out.append((a, 1, t - a - 1) if t - a - 1 >= 1 else (a, t - a))
    return out


@pytest.mark.parametrize("mode", MODES, ids=[f"c{c}t{t}" for c, t in MODES])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_closed_and_flushed_events_are_the_events_of_the_whole_volume(shape, mode):
    connectivity, temporal = mode
    rng = np.random.default_rng(1900 + sum(shape) + connectivity + temporal)
    t, h, w = shape
    for density in (0.15, 0.4, 0.7):
        vol, thr = _volume(rng, shape, density)
        for min_duration, min_volume in FILTERS:
            want, counts, _, _ = events_ref.detect(vol, thr, connectivity, temporal, min_duration, min_volume, BIG)
            got = [ref.run(vol, s, threshold=thr, connectivity=connectivity, temporal=temporal, min_duration=min_duration, min_volume=min_volume,
                           max_open=BIG, max_closed=BIG) for s in _splits(rng, t)]
            for g in got:
                assert g["lost"] == 0 and not g["truncated"] and g["frames"] == t
                assert np.array_equal(ref.convert(g["closed"], h, w), want[:int(counts[0])])
                assert int(g["counts"][:, 0].sum()) == int(counts[0]) and int(g["counts"][:, 1].sum()) == int(counts[1])
                assert int(g["counts"][:, 2].sum()) == int(counts[2]) and int(g["counts"][-1, 4]) == 0
                # any split: the same concatenated outputs, in the same order, and the same final state
                assert np.array_equal(g["closed"], got[0]["closed"]) and np.array_equal(g["frame_counts"], got[0]["frame_counts"])
                assert np.array_equal(g["table"], got[0]["table"]) and np.array_equal(g["plane"], got[0]["plane"])
            # closed records leave in ascending (t1, handle) order
            order = [(int(r[ref.T1]), int(r[ref.HANDLE])) for r in got[0]["closed"]]
            assert order == sorted(order)


@pytest.mark.parametrize("mode", MODES, ids=[f"c{c}t{t}" for c, t in MODES])
def test_every_prefix_gives_the_causal_word_and_the_open_events(mode):
    connectivity, temporal = mode
    rng = np.random.default_rng(1950 + connectivity + temporal)
    for shape, density in (((7, 8, 9), 0.3), ((5, 6, 7), 0.55), ((6, 1, 9), 0.5), ((4, 3, 1), 0.6)):
        t, h, w = shape
        vol, thr = _volume(rng, shape, density)
        for min_duration, min_volume in FILTERS:
            tr = ref.Tracker(h, w, thr, connectivity, temporal, min_duration, min_volume, BIG, BIG)
            for f in range(t):
                _, counts, frames = tr.update(vol[f:f + 1])
                _, _, want_frames, _ = events_ref.detect(vol[:f + 1], thr, connectivity, temporal, min_duration, min_volume, BIG)
                assert frames.tolist() == [want_frames[-1].tolist()], (shape, f)
                every, _, _, _ = events_ref.detect(vol[:f + 1], thr, connectivity, temporal, 1, 1, BIG)
                every = every[every[:, events_ref.VOLUME] > 0]
                still = every[every[:, events_ref.T1] == f]
                table = tr.open_table()
                assert int(counts[4]) == len(still) == len(tr.table)
                assert np.array_equal(ref.convert(table[:len(still)], h, w), still) and not table[len(still):].any()
                # slot r = rank r of the handles in raster order; the plane holds slot + 1 on the frame's foreground only
                handles = table[:len(still), ref.HANDLE].astype(np.int64)
                assert np.array_equal(handles, np.sort(handles)) and np.array_equal(tr.plane[handles], np.arange(1, len(still) + 1))
                assert np.array_equal(tr.plane != 0, events_ref.foreground(vol[f], thr).reshape(-1))


def test_merge_split_gap_and_ties_in_the_restatement():
    # two blobs that join in frame 3: one event, the smaller root, sums added
    vol = np.zeros((5, 3, 9), np.float32)
    vol[:, 1, 1] = 2.0
    vol[1:, 1, 7] = 3.0
    vol[3, 1, 1:8] = 1.0
    vol[3, 1, 1], vol[3, 1, 7] = 2.0, 3.0
    g = ref.run(vol, (2, 3), threshold=0.5, max_open=8, max_closed=8)
    assert len(g["closed"]) == 1 and g["counts"][:, 0].tolist() == [0, 0, 1]
    r = g["closed"][0]
    assert (r[ref.ROOT_PIXEL], r[ref.T0], r[ref.T1], r[ref.HANDLE]) == (10, 0, 4, 10) and ref._u64(r, ref.VOLUME) == 5 + 4 + 5
    assert (r[ref.PEAK].view(np.float32), r[ref.PEAK_FRAME], r[ref.PEAK_PIXEL]) == (3.0, 1, 16)       # the earliest frame that holds 3.0
    assert g["frame_counts"][:, 0].tolist() == [1, 2, 2, 7, 2]
    # a blob that splits stays one event; its handle is the smaller region's root
    vol = np.zeros((3, 1, 7), np.float32)
    vol[0, 0, 1:6] = 1.0
    vol[1:, 0, 1] = vol[1:, 0, 5] = 1.0
    g = ref.run(vol, (1, 1, 1), threshold=0.5, connectivity=4, temporal=1, max_open=8, max_closed=8)
    assert len(g["closed"]) == 1 and g["closed"][0, ref.HANDLE] == 1 and ref._u64(g["closed"][0], ref.VOLUME) == 9
    assert g["counts"][:3, 4].tolist() == [1, 1, 1]
    # absent for exactly one frame: two events
    vol = np.zeros((3, 2, 2), np.float32)
    vol[0, 0, 0] = vol[2, 0, 0] = 1.0
    g = ref.run(vol, (3,), threshold=0.5, max_open=8, max_closed=8)
    assert [(int(r[ref.T0]), int(r[ref.T1])) for r in g["closed"]] == [(0, 0), (2, 2)]
    # min_duration 2: neither is kept, no frame alarms
    g = ref.run(vol, (3,), threshold=0.5, min_duration=2, max_open=8, max_closed=8)
    assert len(g["closed"]) == 0 and int(g["counts"][:, 1].sum()) == 2 and not g["frame_counts"][:, 1].any()
    # the alarm begins exactly in the frame in which the duration is reached
    vol = np.zeros((4, 1, 3), np.float32)
    vol[:, 0, 1] = 1.0
    g = ref.run(vol, (4,), threshold=0.5, min_duration=3, max_open=8, max_closed=1)
    assert g["frame_counts"][:, 1].tolist() == [0, 0, 1, 1]
    # truncation: the full number is counted, the first max_closed written, the causal word unchanged
    vol = np.zeros((2, 1, 5), np.float32)
    vol[0, 0, ::2] = 1.0
    a = ref.run(vol, (2,), threshold=0.5, max_open=8, max_closed=2)
    b = ref.run(vol, (2,), threshold=0.5, max_open=8, max_closed=8)
    assert a["truncated"] and a["counts"][0, 0] == 3 and len(a["closed"]) == 2 and np.array_equal(a["closed"], b["closed"][:2])
    assert np.array_equal(a["frame_counts"], b["frame_counts"])


def test_lost_events_in_the_restatement():
    """max_open = 2 with three simultaneous events: the one of rank 2 has no record, is lost once per frame it begins anew in (its
    pixels are background for the links of the next frame), never alarms; the tracked two are exact."""
    vol = np.zeros((4, 1, 7), np.float32)
    vol[:, 0, 0] = vol[:, 0, 3] = vol[:, 0, 6] = 1.0
    vol[2:, 0, 0] = 0.0                                                      # from frame 2 on the last one has rank 1: a record, t0 = 2
    tr = ref.Tracker(1, 7, 0.5, 8, 9, 1, 1, 2, 8)
    lost, planes, alarms = [], [], []
    for f in range(4):
        _, counts, frames = tr.update(vol[f:f + 1])
        lost.append(int(counts[5]))
        planes.append(tr.plane.tolist())
        alarms.append(int(frames[0, 1]))
        assert int(counts[4]) == 2
    assert lost == [1, 1, 0, 0] and tr.lost_total == 2 and alarms == [2, 2, 2, 2]
    assert planes[1] == [1, 0, 0, 2, 0, 0, ref.NO_RECORD] and planes[2] == [0, 0, 0, 1, 0, 0, 2]
    closed, counts = tr.flush()
    got = ref.convert(closed[:2], 1, 7)
    assert counts.tolist()[:2] == [2, 0] and got[:, events_ref.ROOT].tolist() == [3, 2 * 7 + 6] and got[:, events_ref.VOLUME].tolist() == [4, 2]
    # without the lost one the volume's events are the tracked ones
    seen = vol.copy()
    seen[:2, 0, 6] = 0.0
    want, _, _, _ = events_ref.detect(seen, 0.5, 8, 9, 1, 1, 8)
    assert np.array_equal(got, want[1:3]) and want[0, events_ref.ROOT] == 0
    # an old record that continues behind the table is dropped with it: lost, neither kept nor dropped
    vol = np.zeros((2, 1, 5), np.float32)
    vol[0, 0, 4] = 1.0
    vol[1, 0, 0] = vol[1, 0, 4] = 1.0
    g = ref.run(vol, (1, 1), threshold=0.5, max_open=1, max_closed=8)
    assert g["lost"] == 1 and g["counts"][:, :2].sum() == 1 and g["closed"][0, ref.HANDLE] == 0 and g["closed"][0, ref.T0] == 1


def test_state_and_workspace_bytes_and_the_plan_without_a_gpu():
    lib = hip.lib()
    assert hip.TRACK_WORDS == 20 and metrics.TRACK_WORDS == 20 and hip.TRACK_MAX_OPEN == 65536 and ref.WORDS == 20 and ref.HEADER_WORDS == 16

    def pad(n):
        return (n + 15) // 16 * 16

    # per stream: 64 bytes of header, 80 per slot, 4 per pixel, padded to 16
    assert lib.vad_track_state_bytes(64, 256, 256, 1024) == 64 * (64 + 80 * 1024 + 4 * 65536)
    assert lib.vad_track_state_bytes(3, 5, 7, 3) == 3 * pad(64 + 240 + 140)
    assert lib.vad_track_state_bytes(0, 5, 7, 3) == 0 and lib.vad_track_state_bytes(1, 1, 1, 1) == pad(64 + 80 + 4)
    for b, h, w, m in ((-1, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0), (1, 4, 4, 65537), (1, 4097, 4096, 4), ((1 << 20) + 1, 4, 4, 4)):
        assert lib.vad_track_state_bytes(b, h, w, m) == 0 and lib.vad_track_workspace_bytes(b, 1, h, w, m) == 0, (b, h, w, m)
    assert lib.vad_track_state_bytes(1, 4096, 4096, 65536) == 64 + 80 * 65536 + 4 * (1 << 24)

    def ws(b, t, h, w, m):
        return 16 + pad(4 * b * t * h * w) + pad(4 * b * m) + pad(4 * b * ((h * w + 1023) // 1024)) + pad(4 * b * h * w) + 96 * b * m + pad(4 * b)

    for args in ((64, 1, 256, 256, 1024), (3, 12, 24, 40, 256), (1, 3, 37, 53, 5), (2, 0, 9, 9, 7), (1, 1, 1, 1, 1)):
        assert lib.vad_track_workspace_bytes(*args) == ws(*args), args
    assert lib.vad_track_workspace_bytes(0, 4, 4, 4, 4) == 16
    assert lib.vad_track_workspace_bytes(1, -1, 4, 4, 4) == 0 and lib.vad_track_workspace_bytes(1 << 20, 16, 256, 256, 4) == 0
    out = [hip.C.c_int(0) for _ in range(5)]
    assert lib.vad_track_plan(*[hip.C.byref(v) for v in out]) == 0
    label_round, pixel_round, scan_round, table_round, threads = (v.value for v in out)
    assert label_round == 4096 * 256 and threads == 256 and table_round >= 1024
    # a frame of 520 x 520 is more than one grid round of every per-frame pass over pixels
    assert 256 * 256 <= min(pixel_round, scan_round) and max(pixel_round, scan_round) < 520 * 520
    assert lib.vad_track_plan(None, None, None, None, None) == -1


def test_refusals_by_name_without_a_gpu():
    """Every argument check runs on the host, before any device call: the addresses are never read."""
    lib = hip.lib()
    fake = 1 << 20
    need = lib.vad_track_workspace_bytes(2, 3, 8, 8, 16)
    a = (fake, 2, 3, 8, 8, 0.5, 8, 9, 1, 1, 16, 4, fake, fake, fake, fake, fake, need, None)
    for pos, bad, word in ((0, None, b"maps is NULL"), (0, fake + 2, b"maps must be 4-byte"), (1, -1, b"b must"), (1, (1 << 20) + 1, b"b must"),
                           (2, 0, b"t must"), (2, -3, b"t must"), (3, 0, b"h and w"), (4, 0, b"h and w"), (3, -5, b"h and w"),
                           (5, float("nan"), b"threshold is NaN"), (6, 6, b"connectivity"), (6, 0, b"connectivity"), (7, 0, b"temporal must"),
                           (7, 3, b"temporal must"), (7, 27, b"temporal must"), (8, 0, b"min_duration"), (9, 0, b"min_volume"),
                           (10, 0, b"max_open"), (10, 65537, b"max_open"), (11, 0, b"max_closed"), (11, 65537, b"max_closed"),
                           (12, None, b"state is NULL"), (12, fake + 8, b"state must be 16-byte"), (13, None, b"closed is NULL"),
                           (13, fake + 8, b"closed must be 16-byte"), (14, None, b"counts is NULL"), (14, fake + 1, b"counts must be 4-byte"),
                           (15, None, b"frame_counts is NULL"), (15, fake + 2, b"frame_counts must be 4-byte"), (16, None, b"ws is NULL"),
                           (16, fake + 8, b"ws must be 16-byte")):
        args = list(a)
        args[pos] = bad
        assert lib.vad_track_events(*args) == -1 and word in lib.vad_last_error() and b"track_events" in lib.vad_last_error(), (pos, bad, lib.vad_last_error())
    args = list(a)
    args[6] = 4                                                               # temporal 9 with connectivity 4
    assert lib.vad_track_events(*args) == -1 and b"temporal 9 needs connectivity 8" in lib.vad_last_error()
    for dims, word in (((1, 1, 4097, 4096), b"2^24"), ((1 << 20, 16, 256, 256), b"2^38")):
        args = list(a)
        args[1:5] = dims
        assert lib.vad_track_events(*args) == -1 and word in lib.vad_last_error(), dims
    args = list(a)
    args[17] = need - 1
    assert lib.vad_track_events(*args) == -3 and b"ws_bytes" in lib.vad_last_error()                    # VAD_ERR_WS
    need0 = lib.vad_track_workspace_bytes(2, 0, 8, 8, 16)
    f = (2, 8, 8, 1, 1, 16, 4, fake, fake, fake, fake, need0, None)
    for pos, bad, word in ((0, -1, b"b must"), (1, 0, b"h and w"), (3, 0, b"min_duration"), (4, 0, b"min_volume"), (5, 0, b"max_open"), (6, 0, b"max_closed"),
                           (7, None, b"state is NULL"), (7, fake + 4, b"state must be 16-byte"), (8, None, b"closed is NULL"),
                           (9, None, b"counts is NULL"), (10, None, b"ws is NULL"), (10, fake + 4, b"ws must be 16-byte")):
        args = list(f)
        args[pos] = bad
        assert lib.vad_track_flush(*args) == -1 and word in lib.vad_last_error() and b"track_flush" in lib.vad_last_error(), (pos, bad)
    args = list(f)
    args[11] = need0 - 1
    assert lib.vad_track_flush(*args) == -3 and b"ws_bytes" in lib.vad_last_error()
    i = (fake, 2, 8, 8, 16, None)
    for pos, bad, word in ((0, None, b"state is NULL"), (0, fake + 8, b"state must be 16-byte"), (1, -1, b"b must"), (2, 0, b"h and w"),
                           (3, 5000000, b"h and w"), (4, 0, b"max_open"), (4, 65537, b"max_open")):
        args = list(i)
        args[pos] = bad
        assert lib.vad_track_init(*args) == -1 and word in lib.vad_last_error() and b"track_init" in lib.vad_last_error(), (pos, bad)


def test_python_refusals_without_a_gpu():
    kw = dict(streams=2, h=8, w=8, threshold=0.5)
    with pytest.raises(hip.VadError, match="no CPU fallback"):
        metrics.EventTracker(**kw, device="cpu")
    with pytest.raises(hip.VadError, match="connectivity"):
        metrics.EventTracker(**kw, connectivity=6)
    with pytest.raises(hip.VadError, match="temporal must be 1 or 9"):
        metrics.EventTracker(**kw, temporal=3)
    with pytest.raises(hip.VadError, match="temporal=9 .* needs connectivity=8"):
        metrics.EventTracker(**kw, connectivity=4)
    with pytest.raises(hip.VadError, match="threshold must be a number that is not NaN"):
        metrics.EventTracker(2, 8, 8, float("nan"))
    for name, bad in (("min_duration", 0), ("min_volume", 0), ("max_open", 0), ("max_open", 65537), ("max_closed", 0), ("max_closed", 65537),
                      ("min_duration", True), ("h", 0), ("w", -1), ("streams", -1)):
        with pytest.raises(hip.VadError, match=f"{name} must be an int"):
            metrics.EventTracker(**{**kw, name: bad})
    with pytest.raises(hip.VadError, match="h \\* w <= 2\\^24"):
        metrics.EventTracker(1, 4097, 4096, 0.5)
    with pytest.raises(hip.VadError, match="tracker must be a metrics.EventTracker"):
        scoring.localize_stream(None, torch.zeros(1, 3, 16, 16), tracker=None)


def test_header_and_signatures_agree():
    header = (REPO / "include" / "vad_hip.h").read_text()
    lib = hip.lib()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count in (("vad_track_state_bytes", 4), ("vad_track_workspace_bytes", 5), ("vad_track_init", 6), ("vad_track_events", 19),
                        ("vad_track_flush", 13), ("vad_track_plan", 5)):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, plain, flags=re.S).group(1)
        assert len(hip.SIGNATURES[name][1]) == len(decl.split(",")) == count, name
    assert re.search(r"#define\s+VAD_TRACK_WORDS\s+20\b", header)
    assert "map_track.hip" in hip.SOURCES and (hip.CSRC / "map_track.hip").exists()
    # the word order of the record: the header's table, hip.py's users and the restatement alike
    rows = re.findall(r"\*\s+words? (\d+)(?:-(\d+))?\s+(\w+)", header[header.index("VAD_TRACK_WORDS = 20"):header.index("#define VAD_TRACK_WORDS")])
    names = {int(a): n.rstrip(":") for a, _, n in rows}
    assert names == {0: "root_pixel", 1: "t0", 3: "handle", 4: "x0", 8: "peak", 9: "peak_pixel", 11: "reserved", 12: "uint64", 14: "uint64", 16: "uint64",
                     18: "uint64"}
    assert (ref.ROOT_PIXEL, ref.T0, ref.T1, ref.HANDLE, ref.X0, ref.PEAK, ref.PEAK_PIXEL, ref.PEAK_FRAME, ref.RESERVED, ref.VOLUME, ref.SUM_X, ref.SUM_Y,
            ref.SUM_T) == (0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 14, 16, 18)
