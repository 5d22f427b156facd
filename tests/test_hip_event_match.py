"""Events against ground-truth masks on the GPU (csrc/map_event_match.hip, metrics.match_events, metrics.EventCounts,
scoring.event_report): both tables, the 22 counters and the frame counts `torch.equal` to the numpy restatement
(tests/event_match_ref.py) on odd shapes under the three structures, a volume past one grid round of every pass, the cases by hand,
both mask formats and unaligned views, the equalities with `detect_events` and `match_regions` computed on the device, any batching,
a captured call, the raw C ABI with a poisoned and guarded workspace, and through both seeded models."""
import ctypes
import math

import numpy as np
import pytest
import torch

import event_match_ref as ref
import events_ref
import pro_ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

T = np.float32(0.25)
MODES = ((4, 1), (8, 1), (8, 9))
MODE_IDS = [f"c{c}t{t}" for c, t in MODES]
SHAPES = ((1, 1, 1), (3, 1, 41), (3, 41, 1), (4, 23, 31), (2, 40, 70))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64))


def _assert_equal(got, want):
    """got: metrics.EventMatches; want: (gt_records, pred_records, counts, frame_counts) of the restatement."""
    g, p, c, f = want
    assert got.gt_records.dtype == torch.int32 and got.pred_records.dtype == torch.int32
    assert got.counts.dtype == torch.int64 and got.frame_counts.dtype == torch.int32
    assert torch.equal(got.gt_records.cpu().reshape(g.shape), _i32(g)), "gt records differ from the restatement"
    assert torch.equal(got.pred_records.cpu().reshape(p.shape), _i32(p)), "pred records differ from the restatement"
    assert torch.equal(got.counts.cpu().reshape(c.shape), _i64(c)), "counts differ from the restatement"
    assert torch.equal(got.frame_counts.cpu().reshape(f.shape), _i32(f)), "frame counts differ from the restatement"


def _run_and_check(vad, maps, masks, t=T, *args):
    """maps float32 [b, t, h, w], masks bool [b, t, h, w]; args: connectivity, temporal, min_duration, min_volume, gt_fraction,
    pred_fraction, max_events"""
    want = ref.match_batch(maps, masks, t, *args)
    got = vad.metrics.match_events(torch.from_numpy(maps).cuda(), torch.from_numpy(masks).cuda(), float(t), *args)   # raises on a set flag word
    _assert_equal(got, want)
    return got, want


def _from_masks(seed, mask):
    return events_ref.map_from_mask(np.random.default_rng(seed), np.asarray(mask, bool), T)


# ------------------------------------------------------------------------------------------ shapes and structures
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_shapes_equal_the_restatement(vad, mode):
    connectivity, temporal = mode
    rng = np.random.default_rng(300 + connectivity + temporal)
    for shape in SHAPES:                                                      # (2, 40, 70): six chunks of 1024
        for density, filters in ((0.3, (1, 1, 0.0, 0.0, 64)), (0.55, (2, 3, 0.5, 0.25, 8))):
            fg, masks = rng.random((2,) + shape) < density, rng.random((2,) + shape) < density
            if shape[1] * shape[2] > 100:                                     # blobs, so that tracks and events have volumes to share
                masks = np.repeat(pro_ref.blobs(rng, 2, shape[1], shape[2], count=4, radius=5)[:, None], shape[0], axis=1) & (rng.random((2,) + shape) < 0.9)
            got, want = _run_and_check(vad, _from_masks(301, fg), masks, T, connectivity, temporal, *filters)
            assert want[2][:, ref.TP:ref.TN + 1].sum(1).tolist() == [int(np.prod(shape))] * 2
    assert -(-2 * 40 * 70 // 1024) == 6


def test_a_sparse_volume_beyond_one_grid_round_of_every_pass(vad):
    out = [ctypes.c_int(0) for _ in range(5)]
    assert vad.hip.lib().vad_event_match_plan(*[ctypes.byref(v) for v in out]) == 0
    label_round, volume_round, scan_round, join_round, threads = (v.value for v in out)
    t, h, w = 17, 256, 256
    assert t * h * w > max(volume_round, scan_round, join_round) and label_round == 4096 * 256 and threads == 256
    assert max(volume_round, scan_round, join_round) <= 16 * h * w            # frame 16 lies behind the first round of every pass
    fg, gt = np.zeros((t, h, w), bool), np.zeros((t, h, w), bool)
    fg[0, 0, 0:3] = fg[1, 0, 1:4] = True                                      # the first voxel, in the first chunk
    gt[0, 0, 0:2] = True
    fg[16, 255, 250:] = fg[15, 254, 249:252] = True                           # the last voxel, in the last chunk; linked diagonally in time
    gt[16, 255, 253:] = gt[14:17, 250:253, 252:255] = True
    fg[3:16, 100:104, 200:204] = True                                         # a long event under a track that starts before it
    gt[1:10, 101:106, 201:206] = True
    fg[15:17, 10:13, 10:13] = True                                            # an event across the end of the first grid round, no track
    gt[15:17, 40:43, 40:43] = True                                            # a track across it, no event
    for f in range(4, 12):
        fg[f, 30 + 2 * f, 60 + f:64 + f] = True                               # drifting two rows per frame: eight events of one frame each
    gt[4:12, 36:54, 62:70] = True
    fg[8, 128, :] = True                                                      # a whole row
    maps = _from_masks(302, fg[None])
    got, want = _run_and_check(vad, maps, gt[None], T, 8, 9, 1, 1, 0.0, 0.0, 64)
    g, p, c, f = (v[0] for v in want)
    assert c[ref.GT_TRACKS] == 6 and c[ref.PRED_EVENTS] == 13 and c[ref.GT_DETECTED] == 4 and c[ref.PRED_MATCHED] == 9
    assert g[0, ref.ROOT] == 0 and p[0, ref.ROOT] == 0 and p[12, ref.T1] == 16 and fg.reshape(-1)[-1] and gt.reshape(-1)[-1]
    assert g[5, ref.ROOT] == t * h * w - 3 and g[5, ref.SHARED] == 3 and p[12, ref.LAST] == 16     # records from the last chunk, joined in the last run
    assert c[ref.DELAY_SUM] == 2 and c[ref.IMMEDIATE] == 3 and c[ref.F_NEITHER] == 0
    got, want = _run_and_check(vad, maps, gt[None], T, 8, 1, 2, 5, 0.5, 0.5, 2)       # filters, fractions and truncation across the rounds
    assert want[2][0, ref.PRED_EVENTS] == 3 and want[2][0, ref.PRED_DROPPED] == 11 and got.truncated().tolist() == [True]


# ------------------------------------------------------------------------------------------ the cases by hand
@pytest.mark.parametrize("name", ref.CASES)
def test_the_cases_by_hand(vad, name):
    maps, masks, kw = ref.case(name)
    kw = {"connectivity": 8, "temporal": 9, "min_duration": 1, "min_volume": 1, "gt_fraction": 0.0, "pred_fraction": 0.0, "max_events": 4, **kw}
    got, want = _run_and_check(vad, maps, masks, ref.T, *kw.values())
    g, p, c, f = want
    if name == "hit_in_the_last_frame":
        assert c[0, ref.DELAY_SUM] == 3 and got.delays()[0, 0].item() == 3 and got.delays()[0, 1].item() == -1
    if name == "hit_by_a_dropped_event":
        assert c[0, ref.PRED_DROPPED] == 1 and c[0, ref.GT_DETECTED] == 0 and c[0, ref.FN] == c[0, ref.GT_VOXELS] and not got.alarms().any()
    if name == "clips_never_link":
        assert c[:, ref.TP].tolist() == [0, 0] and c[:, ref.C_PRED_ONLY].tolist() == [1, 0] and c[:, ref.C_GT_ONLY].tolist() == [0, 1]
    if name == "nan_inside_a_track":
        assert c[0, ref.NAN_VOXELS] == 1 and c[0, ref.FN] == 1
    if name.startswith("fraction_boundary"):
        passes = name.endswith("passes")
        assert g[0, 0, ref.VOLUME] == p[0, 0, ref.VOLUME] == 60 and g[0, 0, ref.SHARED] == (15 if passes else 14)
        assert got.detected()[0, 0].item() == got.matched()[0, 0].item() == passes
    if name == "truncation":
        assert got.truncated().tolist() == [True] and c[0, :3].tolist() == [5, 4, 4] and tuple(got.gt_records.shape) == (1, 3, 8)
    rows = got.to_list()
    assert [len(r["gt"]) for r in rows] == np.minimum(c[:, 0], kw["max_events"]).tolist()
    assert [r["counts"]["voxel_tp"] for r in rows] == c[:, ref.TP].tolist()


# ------------------------------------------------------------------------------------------ mask formats, views
def test_every_mask_format_and_unaligned_views(vad):
    rng = np.random.default_rng(310)
    shape = (2, 3, 24, 40)
    gt = np.repeat(pro_ref.blobs(rng, 2, 24, 40, count=4)[:, None], 3, axis=1) & (rng.random(shape) < 0.9)
    maps_np = _from_masks(311, np.repeat(pro_ref.blobs(rng, 2, 24, 40, count=4)[:, None], 3, axis=1) & (rng.random(shape) < 0.9))
    args = (float(T), 8, 9, 2, 2, 0.25, 0.25, 16)
    want = ref.match_batch(maps_np, gt, *args)
    maps = torch.from_numpy(maps_np).cuda()
    u8 = np.where(gt, rng.choice(np.array([128, 200, 255], np.uint8), shape), rng.choice(np.array([0, 1, 127], np.uint8), shape)).astype(np.uint8)
    f32 = np.where(gt, rng.choice(np.array([0.50001, 1.0, 7.0, np.inf], np.float32), shape),
                   rng.choice(np.array([0.5, 0.0, -1.0, np.nan], np.float32), shape)).astype(np.float32)
    for masks in (torch.from_numpy(u8), torch.from_numpy(f32), torch.from_numpy(gt), torch.from_numpy(gt.astype(np.int64) * 3),
                  torch.from_numpy(f32.astype(np.float64)), torch.from_numpy(u8)[:, :, None]):
        _assert_equal(vad.metrics.match_events(maps, masks.cuda(), *args), want)
    # one element off their allocations: the maps 4 bytes, the byte masks 1, the float masks 4
    flat = torch.zeros(maps.numel() + 1, device="cuda")
    flat[1:] = maps.reshape(-1)
    off_maps = flat[1:].view(shape)
    bytes_ = torch.zeros(maps.numel() + 1, dtype=torch.uint8, device="cuda")
    bytes_[1:] = torch.from_numpy(u8).cuda().reshape(-1)
    floats = torch.zeros(maps.numel() + 1, device="cuda")
    floats[1:] = torch.from_numpy(f32).cuda().reshape(-1)
    assert off_maps.data_ptr() % 16 == 4 and bytes_[1:].data_ptr() % 4 == 1 and floats[1:].data_ptr() % 16 == 4
    _assert_equal(vad.metrics.match_events(off_maps, bytes_[1:].view(shape), *args), want)
    _assert_equal(vad.metrics.match_events(off_maps, floats[1:].view(shape), *args), want)
    strided = torch.from_numpy(np.ascontiguousarray(maps_np.transpose(1, 0, 3, 2))).cuda().permute(1, 0, 3, 2)
    assert not strided.is_contiguous()
    _assert_equal(vad.metrics.match_events(strided, torch.from_numpy(u8).cuda(), *args), want)
    one = vad.metrics.match_events(maps[1], torch.from_numpy(gt[1]).cuda(), *args)         # [T,H,W]: one volume, no leading shape
    assert tuple(one.gt_records.shape) == (16, 8) and tuple(one.counts.shape) == (22,) and tuple(one.frame_counts.shape) == (3, 4)
    _assert_equal(one, tuple(v[1] for v in want))
    empty = vad.metrics.match_events(maps[:0], torch.from_numpy(gt[:0]).cuda(), *args)
    assert tuple(empty.pred_records.shape) == (0, 16, 8) and tuple(empty.frame_counts.shape) == (0, 3, 4) and empty.to_list() == []


# ------------------------------------------------------------------------------------------ equalities computed on the device
def test_identities_with_detect_events_and_match_regions(vad):
    rng = np.random.default_rng(320)
    shape = (3, 4, 24, 40)
    gt = torch.from_numpy(np.repeat(pro_ref.blobs(rng, 3, 24, 40, count=4)[:, None], 4, axis=1) & (rng.random(shape) < 0.9)).cuda()
    maps_np = _from_masks(321, np.repeat(pro_ref.blobs(rng, 3, 24, 40, count=5)[:, None], 4, axis=1) & (rng.random(shape) < 0.8))
    maps_np[0, 1, 3, 3] = maps_np[2, 0, 0, 0] = np.nan
    maps = torch.from_numpy(maps_np).cuda()
    for connectivity, temporal in MODES:
        for min_duration, min_volume, max_events in ((1, 1, 32), (2, 3, 4)):
            m = vad.metrics.match_events(maps, gt, float(T), connectivity, temporal, min_duration, min_volume, 0.25, 0.5, max_events)
            e = vad.metrics.detect_events(maps, float(T), connectivity, temporal, min_duration, min_volume, max_events)
            assert torch.equal(m.pred_records[..., :4], e.records[..., :4])
            assert torch.equal(m.frame_counts[..., 0] + m.frame_counts[..., 1], e.frame_counts[..., 1]) and torch.equal(m.alarms(), e.alarms())
            assert torch.equal(m.frame_counts[..., 3], e.frame_counts[..., 2])
            assert torch.equal(m.counts[:, 2], e.counts[:, 0].long()) and torch.equal(m.counts[:, 5], e.counts[:, 1].long())
            assert m.counts[:, 6:10].sum(1).tolist() == [4 * 24 * 40] * 3
            assert torch.equal(m.counts[:, 6:9], m.frame_counts[..., :3].sum(1).long()) and torch.equal(m.counts[:, 10], m.frame_counts[..., 3].sum(1).long())
            assert torch.equal(m.counts[:, 11], gt.reshape(3, -1).sum(1)) and m.counts[:, 10].tolist() == [1, 0, 1]
            assert m.counts[:, 14:18].sum(1).tolist() == [4] * 3 and m.counts[:, 18:].sum(1).tolist() == [1] * 3
            assert torch.equal(m.gt_records[..., 4].sum(1).long(), m.counts[:, 6]) or bool(m.truncated().any())
    # T = 1: the region match of the same frames
    frames, fmask = maps.reshape(12, 1, 24, 40), gt.reshape(12, 1, 24, 40)
    for connectivity, temporal in MODES:
        m = vad.metrics.match_events(frames, fmask, float(T), connectivity, temporal, 1, 2, 0.25, 0.5, 8)
        r = vad.metrics.match_regions(frames[:, 0], fmask[:, 0], float(T), connectivity, 2, 0.25, 0.5, 8)
        assert torch.equal(m.gt_records[..., [0, 1, 4, 7]], r.gt_records) and torch.equal(m.pred_records[..., [0, 1, 4, 7]], r.pred_records)
        assert torch.equal(m.counts[:, :12], r.counts[:, :12]) and torch.equal(m.counts[:, 18:], r.counts[:, 12:]) and torch.equal(m.counts[:, 14:18], r.counts[:, 12:])
        assert not m.gt_records[..., 2:4].any() and int(m.counts[:, 12].sum()) == 0 and torch.equal(m.counts[:, 13], m.counts[:, 1])


# ------------------------------------------------------------------------------------------ determinism
def test_any_batching_gives_the_same_words(vad):
    rng = np.random.default_rng(330)
    shape = (5, 4, 24, 40)
    gt_np = np.repeat(pro_ref.blobs(rng, 5, 24, 40, count=4)[:, None], 4, axis=1) & (rng.random(shape) < 0.9)
    fg = np.repeat(pro_ref.blobs(rng, 5, 24, 40, count=4)[:, None], 4, axis=1) & (rng.random(shape) < 0.8)
    fg[3], gt_np[4] = True, False                                             # an all-foreground clip, a clip without a track
    maps_np = _from_masks(331, fg)
    args = (float(T), 8, 9, 2, 2, 0.25, 0.1, 16)
    want = ref.match_batch(maps_np, gt_np, *args)
    maps, gt = torch.from_numpy(maps_np).cuda(), torch.from_numpy(gt_np).cuda()
    whole = vad.metrics.match_events(maps, gt, *args)
    _assert_equal(whole, want)
    parts = lambda m: (m.gt_records, m.pred_records, m.counts, m.frame_counts)
    halves = [vad.metrics.match_events(maps[a:b], gt[a:b], *args) for a, b in ((0, 2), (2, 5))]
    singles = [vad.metrics.match_events(maps[i:i + 1], gt[i:i + 1], *args) for i in range(5)]
    for split in (halves, singles):
        for k, tensor in enumerate(parts(whole)):
            assert torch.equal(torch.cat([parts(m)[k] for m in split]), tensor)
    backwards = vad.metrics.match_events(maps.flip(0), gt.flip(0), *args)
    assert all(torch.equal(a.flip(0), b) for a, b in zip(parts(backwards), parts(whole)))
    sums = vad.metrics.EventCounts("cuda")
    for m in singles:
        sums.update(m)
    assert torch.equal(sums.counts, whole.counts.sum(0)) and sums.all_reduce() == 1 and torch.equal(sums.counts, _i64(want[2].sum(0)).cuda())
    report = sums.report()
    assert report["clips"] == 5 and report["frames"] == 20 and report["params"] == whole.params
    with pytest.raises(ValueError, match="gathered with"):
        sums.update(vad.metrics.match_events(maps[:1], gt[:1], float(T), 8, 9, 3, 2, 0.25, 0.1, 16))


# ------------------------------------------------------------------------------------------ the C ABI on the device
def _buffers(b, t, max_events):
    return (torch.empty((b, max_events, 8), dtype=torch.int32, device="cuda"), torch.empty((b, max_events, 8), dtype=torch.int32, device="cuda"),
            torch.empty((b, 22), dtype=torch.int64, device="cuda"), torch.empty((b, t, 4), dtype=torch.int32, device="cuda"))


def test_a_captured_call_follows_new_contents(vad):
    """Every launch is asynchronous on the caller's stream and nothing is allocated: one call captured on a side stream, replayed
    on three contents of the same buffers, equals the restatement and the eager result."""
    lib = vad.hip.lib()
    rng = np.random.default_rng(340)
    shape = (2, 4, 24, 40)
    contents = []
    for k, density in enumerate((0.8, 0.2, 0.5)):
        fg = np.repeat(pro_ref.blobs(rng, 2, 24, 40)[:, None], 4, axis=1) & (rng.random(shape) < density) if k != 1 else rng.random(shape) < density
        contents.append((_from_masks(341 + k, fg), np.repeat(pro_ref.blobs(rng, 2, 24, 40, count=3)[:, None], 4, axis=1) & (rng.random(shape) < 0.9)))
    b, t, h, w = shape
    maps = torch.from_numpy(contents[0][0]).cuda()
    masks = torch.from_numpy(contents[0][1].astype(np.float32)).cuda()
    need = lib.vad_event_match_workspace_bytes(b, t, h, w)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device="cuda")
    gt, pred, counts, frames = _buffers(b, t, 16)

    def call():
        return lib.vad_match_events(maps.data_ptr(), masks.data_ptr(), vad.hip.LBL_F32_ELEM, b, t, h, w, float(T), 8, 9, 2, 1, 0.25, 0.5, 16,
                                    gt.data_ptr(), pred.data_ptr(), counts.data_ptr(), frames.data_ptr(), ws.data_ptr(), need, vad.hip.current_stream())

    def check(k):
        want = ref.match_batch(contents[k][0], contents[k][1], T, 8, 9, 2, 1, 0.25, 0.5, 16)
        assert torch.equal(gt.cpu(), _i32(want[0])) and torch.equal(pred.cpu(), _i32(want[1]))
        assert torch.equal(counts.cpu(), _i64(want[2])) and torch.equal(frames.cpu(), _i32(want[3]))
        assert int(ws[:4].view(torch.int32).item()) == 0

    vad.hip.check(call(), "vad_match_events")                                                # once eagerly
    torch.cuda.synchronize()
    check(0)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            vad.hip.check(call(), "vad_match_events")
    torch.cuda.current_stream().wait_stream(side)
    for k in (1, 2, 0):
        maps.copy_(torch.from_numpy(contents[k][0]).cuda())
        masks.copy_(torch.from_numpy(contents[k][1].astype(np.float32)).cuda())
        for buf in (gt, pred, counts, frames):
            buf.fill_(-7)
        graph.replay()
        check(k)
    eager = vad.metrics.match_events(maps, masks, float(T), 8, 9, 2, 1, 0.25, 0.5, 16)
    assert torch.equal(eager.gt_records, gt) and torch.equal(eager.pred_records, pred) and torch.equal(eager.counts, counts)
    assert torch.equal(eager.frame_counts, frames)


def test_c_abi_with_a_poisoned_and_guarded_workspace(vad):
    """The workspace contract: exactly vad_event_match_workspace_bytes are enough, whatever they held before, and not a byte in front
    of or behind them (or behind any output) is written."""
    lib = vad.hip.lib()
    stream = vad.hip.current_stream()
    rng = np.random.default_rng(350)
    shape = (3, 3, 24, 40)
    gt_np = np.repeat(pro_ref.blobs(rng, 3, 24, 40, count=4)[:, None], 3, axis=1) & (rng.random(shape) < 0.9)
    fg = np.repeat(pro_ref.blobs(rng, 3, 24, 40)[:, None], 3, axis=1) & (rng.random(shape) < 0.8)
    fg[1] = False
    maps_np = _from_masks(351, fg)
    want = ref.match_batch(maps_np, gt_np, T, 8, 9, 2, 2, 0.25, 0.5, 8)
    b, t, h, w = shape
    maps = torch.from_numpy(maps_np).cuda()
    masks = torch.from_numpy(gt_np.astype(np.uint8) * 255).cuda()
    need = lib.vad_event_match_workspace_bytes(b, t, h, w)
    assert need == 16 + 2 * 48 + 48 * b * t * h * w                           # three chunks per clip: 36 bytes, padded to 48, twice
    G = 256                                                                   # guard bytes in front of and behind every buffer

    def guarded(nbytes, fill):
        whole = torch.full((nbytes + 2 * G,), fill, dtype=torch.uint8, device="cuda")
        return whole, whole[G:G + nbytes]

    def intact(whole, fill):
        return bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all())

    bufs = {"ws": guarded(need, 0xAB), "gt": guarded(b * 8 * 8 * 4, 0xF9), "pred": guarded(b * 8 * 8 * 4, 0xF9), "counts": guarded(b * 22 * 8, 0xF9),
            "frames": guarded(b * t * 16, 0xF9)}
    ptr = {k: v[1].data_ptr() for k, v in bufs.items()}
    assert ptr["ws"] % 16 == 0 and ptr["gt"] % 16 == 0 and ptr["pred"] % 16 == 0 and ptr["counts"] % 8 == 0
    common = (maps.data_ptr(), masks.data_ptr(), vad.hip.LBL_U8_ELEM, b, t, h, w, float(T), 8, 9, 2, 2, 0.25, 0.5, 8)
    outs = (ptr["gt"], ptr["pred"], ptr["counts"], ptr["frames"], ptr["ws"])
    assert lib.vad_match_events(*common, *outs, need, stream) == 0, lib.vad_last_error()
    torch.cuda.synchronize()
    assert all(intact(v[0], 0xAB if k == "ws" else 0xF9) for k, v in bufs.items()), "a guard was written"
    assert int(bufs["ws"][1][:4].view(torch.int32).item()) == 0
    assert torch.equal(bufs["gt"][1].view(torch.int32).cpu().view(b, 8, 8), _i32(want[0]))
    assert torch.equal(bufs["pred"][1].view(torch.int32).cpu().view(b, 8, 8), _i32(want[1]))
    assert torch.equal(bufs["counts"][1].view(torch.int64).cpu().view(b, 22), _i64(want[2]))
    assert torch.equal(bufs["frames"][1].view(torch.int32).cpu().view(b, t, 4), _i32(want[3]))
    ws = bufs["ws"][1]
    before = [bufs[k][1].clone() for k in ("gt", "pred", "counts", "frames")]
    # a short workspace, b == 0 and a refused argument: nothing but the flag word is touched
    assert lib.vad_match_events(*common, *outs, need - 1, stream) == -3 and b"ws_bytes" in lib.vad_last_error()
    ws.fill_(0xAB)
    assert lib.vad_match_events(maps.data_ptr(), masks.data_ptr(), vad.hip.LBL_U8_ELEM, 0, t, h, w, float(T), 8, 9, 2, 2, 0.25, 0.5, 8, *outs, 16, stream) == 0
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32).item()) == 0 and bool((ws[16:] == 0xAB).all())
    bad = list(common)
    bad[7] = float("nan")
    assert lib.vad_match_events(*bad, *outs, need, stream) == -1 and b"threshold is NaN" in lib.vad_last_error()
    bad = list(common)
    bad[12] = 1.5
    assert lib.vad_match_events(*bad, *outs, need, stream) == -1 and b"gt_fraction" in lib.vad_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, bufs[k][1]) for a, k in zip(before, ("gt", "pred", "counts", "frames")))


def test_refusals(vad):
    t = torch.zeros(2, 3, 8, 8, device="cuda")
    m = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda")
    VadError = vad.hip.VadError
    for bad, bad_m, word in ((t[0, 0], m[0, 0], "maps must be"), (t.double(), m, "float32"), (t.cpu(), m, "no CPU fallback"), (t, m.cpu(), "no CPU fallback"),
                             (t, m[:1], "do not match"), (t[:, :0], m[:, :0], "out of range"), (t, m.to(torch.complex64), "masks must be")):
        with pytest.raises(VadError, match=word):
            vad.metrics.match_events(bad, bad_m, 0.5)
    for kw, word in (({"threshold": float("nan")}, "threshold"), ({"min_duration": 0}, "min_duration"), ({"min_volume": 2 ** 32}, "min_volume"),
                     ({"max_events": 65537}, "max_events"), ({"temporal": 27}, "temporal must be 1 or 9"), ({"connectivity": 4}, "temporal=9"),
                     ({"gt_fraction": 1.5}, "gt_fraction"), ({"pred_fraction": float("nan")}, "pred_fraction")):
        with pytest.raises(VadError, match=word):
            vad.metrics.match_events(t, m, **{"threshold": 0.5, **kw})
    before = vad.hip.calls.get("match_events", 0)
    assert int(vad.metrics.match_events(t, m, 0.5, connectivity=4, temporal=1).counts[:, :9].sum()) == 0
    assert vad.hip.calls["match_events"] == before + 1


# ------------------------------------------------------------------------------------------ through the models
def _same_report(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k] or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


def _check_report(vad, model, key, loader, volumes, kw, score_call):
    """event_report over the batches of `loader` against the host route on the maps `localize_events` returns for the same batches
    (`volumes`: how a batch's maps and masks are cut into clips), two merged halves, a continued evaluation."""
    with torch.no_grad():
        first = vad.scoring._anomaly_maps(model, loader[0][key], "mse", kw.get("sigma"), 4.0)
    t = float(np.float32(np.quantile(first.cpu().numpy(), 0.85)))
    localize_kw = {k: v for k, v in kw.items() if k not in ("gt_fraction", "pred_fraction")}
    sums = np.zeros(22, np.uint64)
    for batch in loader:
        events, maps = vad.scoring.localize_events(model, batch[key], t, max_events=16, **localize_kw)
        maps_np, masks_np = volumes(maps.cpu().numpy()), volumes(batch["mask"].cpu().numpy()) > 0.5
        want = ref.match_batch(maps_np, masks_np, t, kw.get("connectivity", 8), kw.get("temporal", 9), kw.get("min_duration", 1), kw.get("min_volume", 1),
                               kw["gt_fraction"], kw["pred_fraction"], 16)
        sums += want[2].sum(0)
        # the report is of exactly the events localize_events returns
        assert torch.equal(events.records.reshape(-1, 16, 16)[..., :4].cpu(), _i32(want[1][..., :4]))
        assert torch.equal(events.frame_counts.reshape(len(maps_np), -1, 3)[..., 1].cpu(), _i32(want[3][..., 0] + want[3][..., 1]))
    before = {k: vad.hip.calls.get(k, 0) for k in ("match_events", score_call, "detect_events")}
    report, counts = vad.scoring.event_report(model, loader, "cuda", t, **kw)
    assert [vad.hip.calls.get(k, 0) - before[k] for k in before] == [len(loader), len(loader), 0]
    print(f"{key}: threshold {t!r} sums {sums.tolist()}")
    assert counts.counts.is_cuda and torch.equal(counts.counts.cpu(), _i64(sums))
    assert sums[ref.TP] > 0 and sums[ref.FP] > 0 and sums[ref.FN] > 0 and sums[ref.PRED_EVENTS] > 0 and sums[ref.GT_TRACKS] > 0
    assert report["clips"] == int(sums[ref.C_BOTH:].sum()) and report["params"]["threshold"] == t and report["params"]["map"] == "mse"
    _same_report({k: v for k, v in report.items() if k != "params"}, vad.metrics.event_report_from_counts(sums))
    assert counts.all_reduce() == 1 and torch.equal(counts.counts.cpu(), _i64(sums))                 # world size 1: the sums stand
    a = vad.scoring.event_report(model, loader[:1], "cuda", t, **kw)[1]
    b = vad.scoring.event_report(model, loader[1:], "cuda", t, **kw)[1]
    assert torch.equal(a.merge(b).counts, counts.counts)
    _same_report(a.report(), report)
    continued = vad.scoring.event_report(model, loader[1:], "cuda", t, counts=vad.scoring.event_report(model, loader[:1], "cuda", t, **kw)[1], **kw)[1]
    assert torch.equal(continued.counts, counts.counts)
    with pytest.raises(ValueError, match="gathered with"):
        vad.scoring.event_report(model, loader[:1], "cuda", t, counts=counts, **{**kw, "min_duration": kw.get("min_duration", 1) + 1})
    with pytest.raises(ValueError, match="gathered with"):
        vad.scoring.event_report(model, loader[:1], "cuda", t, counts=counts, **{**kw, "sigma": 2.0})
    return report


def test_event_report_through_the_video_model(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 13)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(22, 0, 3, 4, 3, 32, 32)).cuda()
    masks = np.repeat(pro_ref.blobs(np.random.default_rng(360), 3, 32, 32, count=3, radius=6)[:, None], 4, axis=1)
    masks[:, 0] = False                                                       # the tracks start in frame 1
    masks = torch.from_numpy(masks.astype(np.float32)).view(3, 4, 1, 32, 32).cuda()
    loader = [{"frames": clips[:2], "mask": masks[:2]}, {"frames": clips[2:], "mask": masks[2:]}]
    kw = dict(sigma=1.0, connectivity=8, temporal=9, min_duration=2, min_volume=1, gt_fraction=0.1, pred_fraction=0.05, temporal_filter=("min", 2))
    report = _check_report(vad, model, "frames", loader, lambda a: a.reshape(-1, 4, 32, 32), kw, "vid_score")
    assert report["params"]["temporal_filter"] == (("min", 2),) and report["frames"] == 12
    with pytest.raises(vad.hip.VadError, match="map='mse'"):
        vad.scoring.event_report(model, loader, "cuda", 0.5, map="ssim")


def test_event_report_through_the_image_model(vad):
    """A batch of consecutive synthetic frames of one camera is one volume."""
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 11)
    model = model.cuda().eval()
    x = torch.from_numpy(vad.synth.frames(21, 0, 10, 3, 32, 32)).cuda()
    masks = np.repeat(pro_ref.blobs(np.random.default_rng(361), 2, 32, 32, count=3, radius=6), [6, 4], axis=0)
    masks = torch.from_numpy(masks.astype(np.float32))[:, None].cuda()
    loader = [{"image": x[:6], "mask": masks[:6]}, {"image": x[6:], "mask": masks[6:]}]
    kw = dict(sigma=1.0, morph=("open", 2), connectivity=4, temporal=1, min_duration=2, min_volume=3, gt_fraction=0.1, pred_fraction=0.05)
    report = _check_report(vad, model, "image", loader, lambda a: a.reshape(1, -1, 32, 32), kw, "img_score")
    assert report["clips"] == 2 and report["frames"] == 10 and report["params"]["morph"] == (("open", (2, 2)),)
    with pytest.raises(vad.hip.VadError, match="not consecutive"):
        vad.scoring.event_report(model, loader, "cuda", 0.5, temporal_filter=("min", 2))
