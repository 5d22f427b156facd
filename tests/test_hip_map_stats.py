"""Per-pixel map statistics and the z-score map on the GPU (csrc/map_stats.hip, metrics.MapStatistics): the state planes, the
finalized mean / std and the normalised maps equal the numpy restatement (tests/map_stats_ref.py) bit for bit on every shape that
takes another path of the kernels - the shapes are built from `vad_mapstat_plan`, not from the workload -; independence of the
batching, graph replay, merge, non-finite values, exact scaling, the workspace contract, refusals, and the drivers through the
seeded models."""
import ctypes as C

import numpy as np
import pytest
import torch

import hip_helpers as H
import map_stats_ref as ref
from conftest import load_synthetic

pytestmark = pytest.mark.gpu

_PLAN = {}


def _plan(vad):
    """(pixels per thread, frames in flight, threads per work-group) of the accumulate kernel; pixels per work-group of normalize."""
    if not _PLAN:
        lib = vad.hip.lib()
        ppt, fif, threads = C.c_int(), C.c_int(), C.c_int()
        assert lib.vad_mapstat_plan(C.byref(ppt), C.byref(fif), C.byref(threads)) == 0
        chunk = next(p - 1 for p in range(2, 1 << 16) if lib.vad_map_normalize_workspace_bytes(1, 1, p) == 8)
        _PLAN.update(ppt=ppt.value, fif=fif.value, threads=threads.value, chunk=chunk)
    return _PLAN


def _lognormal(shape, seed):
    rng = np.random.default_rng(seed)
    return (np.exp(rng.standard_normal(shape) * 3.0) * 1e-3).astype(np.float32)


def _same(got, want):
    """Bit identity, -0.0 against +0.0 included; a NaN matches any NaN (the sign and payload of a generated NaN are the
    processor's)."""
    g = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.ascontiguousarray(want)
    assert g.shape == want.shape and g.dtype == want.dtype, (g.shape, g.dtype, want.shape, want.dtype)
    nan = np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    return np.array_equal(np.isnan(g), nan) and np.array_equal(np.ascontiguousarray(g).view(bits)[~nan], want.view(bits)[~nan])


def _restated(x):
    return ref.accumulate(ref.State(*x.shape[-2:]), x)


def _state_is(stats, want):
    return stats.device_count() == want.n == stats.count and _same(stats._planes(), want.planes())


def _shapes(vad):
    p = _plan(vad)
    group = p["ppt"] * p["threads"]
    return {"one_pixel": (3, 1, 1),
            "w_not_vector_multiple": (5, 16, 20),
            "three_groups_ragged": (4, 3, group - 5),                        # 3 * group - 15 pixels: the last work-group is ragged
            "frames_cross_the_pipeline": (2 * p["fif"] + 3, 6, 7),           # two full groups of loads and a short one
            "exactly_one_group_of_frames": (p["fif"], 5, 3),
            "five_leading_dims": (2, 1, 3, 1, 2, 6, 7)}


SHAPE_NAMES = ("one_pixel", "w_not_vector_multiple", "three_groups_ragged", "frames_cross_the_pipeline", "exactly_one_group_of_frames",
               "five_leading_dims")


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_equals_the_restatement(vad, name):
    shape = _shapes(vad)[name]
    x = _lognormal(shape, 700 + SHAPE_NAMES.index(name))
    want = _restated(x)
    xt = torch.from_numpy(x).cuda()
    stats = vad.metrics.MapStatistics(shape[-2:])
    before = vad.hip.calls.get("mapstat_accumulate", 0)
    assert stats.update(xt) is stats and vad.hip.calls["mapstat_accumulate"] == before + 1
    assert _state_is(stats, want)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))                        # the input is not touched
    for ddof in (1, 0):
        mean, std = ref.finalize(want, ddof)
        assert _same(stats.mean(), mean) and _same(stats.std(ddof), std)
    assert stats.mean().shape == shape[-2:] and stats.std().dtype == torch.float32
    # the z-scores of the same maps, and of the maps alone / the maxima alone
    mean, std = ref.finalize(want)
    z = ref.normalize(x, mean, std, 1e-3)
    got, gmax = stats.normalize(xt, 1e-3, return_max=True)
    assert got.shape == xt.shape and gmax.shape == xt.shape[:-2]
    assert _same(got, z) and _same(gmax, ref.frame_max(z))
    assert _same(stats.normalize(xt, 1e-3, return_max="only"), ref.frame_max(z))
    out = torch.full_like(xt, 7.0)
    assert stats.normalize(xt, 1e-3, out=out) is out and _same(out, z)
    assert torch.equal(xt.cpu(), torch.from_numpy(x))
    assert stats.normalize(xt, 1e-3, out=xt) is xt and _same(xt, z)          # in place


def test_base_one_float_off_its_allocation(vad):
    """maps, mean, std and out sliced one float into their allocations: 4-byte aligned bases; the neighbours keep their bits."""
    lib, stream = vad.hip.lib(), vad.hip.current_stream()
    shape = _shapes(vad)["w_not_vector_multiple"]
    n, h, w = shape
    x = _lognormal(shape, 720)
    want = _restated(x)
    buf = torch.zeros(x.size + 1, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().reshape(-1)
    xt = buf[1:].view(shape)
    assert xt.data_ptr() % 16 == 4 and xt.is_contiguous()
    stats = vad.metrics.MapStatistics((h, w)).update(xt)
    assert _state_is(stats, want)
    mbuf, sbuf = torch.full((h * w + 2,), -7.0, device="cuda"), torch.full((h * w + 2,), -7.0, device="cuda")
    assert lib.vad_mapstat_finalize(stats._state.data_ptr(), h, w, 1, mbuf[1:].data_ptr(), sbuf[1:].data_ptr(), stream) == 0
    mean, std = ref.finalize(want)
    assert _same(mbuf[1:-1].view(h, w), mean) and _same(sbuf[1:-1].view(h, w), std)
    assert all(b[0].item() == -7.0 and b[-1].item() == -7.0 for b in (mbuf, sbuf))
    # one output alone: the other pointer is NULL
    only = torch.full((h * w,), -7.0, device="cuda")
    assert lib.vad_mapstat_finalize(stats._state.data_ptr(), h, w, 1, None, only.data_ptr(), stream) == 0 and _same(only.view(h, w), std)
    obuf = torch.full((x.size + 2,), -7.0, device="cuda")
    fbuf = torch.full((n + 2,), -7.0, device="cuda")
    need = lib.vad_map_normalize_workspace_bytes(n, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.vad_map_normalize(xt.data_ptr(), n, h, w, mbuf[1:].data_ptr(), sbuf[1:].data_ptr(), 1e-3, obuf[1:].data_ptr(), fbuf[1:].data_ptr(),
                                 ws.data_ptr(), need, stream) == 0
    z = ref.normalize(x, mean, std, 1e-3)
    assert _same(obuf[1:-1].view(shape), z) and _same(fbuf[1:-1], ref.frame_max(z))
    assert all(b[0].item() == -7.0 and b[-1].item() == -7.0 for b in (obuf, fbuf))


def test_state_does_not_depend_on_the_batching(vad):
    shape = _shapes(vad)["frames_cross_the_pipeline"]
    x = _lognormal(shape, 730)
    xt = torch.from_numpy(x).cuda()
    want = _restated(x)
    whole = vad.metrics.MapStatistics(shape[-2:]).update(xt)
    split = vad.metrics.MapStatistics(shape[-2:])
    for part in (xt[:1], xt[1:7], xt[7:7], xt[7:]):
        split.update(part)
    single = vad.metrics.MapStatistics(shape[-2:])
    for i in range(shape[0]):
        single.update(xt[i:i + 1])
    torch.cuda.synchronize()
    for stats in (whole, split, single):
        assert _state_is(stats, want)
        assert H.same_bits(stats._state, whole._state)                       # the whole blob, header included: byte-equal


def test_captured_accumulate_replays(vad):
    """The count lives on the device: a captured call, replayed twice behind one eager call, is three eager calls."""
    lib = vad.hip.lib()
    shape = (_plan(vad)["fif"] + 2, 6, 7)
    n, h, w = shape
    x = _lognormal(shape, 740)
    xt = torch.from_numpy(x).cuda()
    stats = vad.metrics.MapStatistics((h, w)).update(xt)

    def run():
        vad.hip.check(lib.vad_mapstat_accumulate(xt.data_ptr(), n, h, w, stats._state.data_ptr(), vad.hip.current_stream()), "vad_mapstat_accumulate")

    call = vad.hip.CapturedCall(run, None, None, (xt, stats))
    call.replay()
    call.replay()
    torch.cuda.synchronize()
    eager = vad.metrics.MapStatistics((h, w))
    want = ref.State(h, w)
    for _ in range(3):
        eager.update(xt)
        ref.accumulate(want, x)
    assert stats.device_count() == 3 * n and stats.count == n                # the host's count saw the eager call only
    assert H.same_bits(stats._state, eager._state) and _same(stats._planes(), want.planes())


def test_merge(vad):
    shape = (37, 9, 11)
    x = _lognormal(shape, 750) + np.float32(0.25)
    xt = torch.from_numpy(x).cuda()
    a = vad.metrics.MapStatistics(shape[-2:]).update(xt[:13])
    b = vad.metrics.MapStatistics(shape[-2:]).update(xt[13:])
    b_before = b._state.clone()
    assert a.merge(b) is a
    want = ref.merge(_restated(x[:13]), _restated(x[13:]))
    assert _state_is(a, want) and H.same_bits(b._state, b_before)
    one = _restated(x)
    for ddof in (0, 1):
        for got, single in zip((a.mean(), a.std(ddof)), ref.finalize(one, ddof)):
            assert ref.ulps32(got.cpu().numpy(), single.astype(np.float64)) <= 1.0
    # an empty side gives the other side, bit for bit
    full = vad.metrics.MapStatistics(shape[-2:]).update(xt)
    into_empty = vad.metrics.MapStatistics(shape[-2:]).merge(full)
    assert _state_is(into_empty, one) and H.same_bits(into_empty._state, full._state)
    assert _state_is(full.merge(vad.metrics.MapStatistics(shape[-2:])), one)
    with pytest.raises(vad.hip.VadError, match="this object"):
        a.merge(a)
    with pytest.raises(ValueError, match="frame shapes"):
        a.merge(vad.metrics.MapStatistics((9, 12)))


def test_finalize_with_one_frame(vad):
    lib, stream = vad.hip.lib(), vad.hip.current_stream()
    x = _lognormal((1, 6, 7), 760)
    stats = vad.metrics.MapStatistics((6, 7))
    assert stats.count == 0 and torch.isnan(stats.mean()).all()
    with pytest.raises(ValueError, match="0 frames"):
        stats.std(0)
    stats.update(torch.from_numpy(x).cuda())
    mean, std = torch.empty(6, 7, device="cuda"), torch.empty(6, 7, device="cuda")
    assert lib.vad_mapstat_finalize(stats._state.data_ptr(), 6, 7, 1, mean.data_ptr(), std.data_ptr(), stream) == 0
    assert torch.isnan(std).all() and _same(mean, x[0])                      # ddof = 1 at n = 1: no std, a finite mean
    with pytest.raises(ValueError, match="1 frames"):
        stats.std()
    with pytest.raises(ValueError, match="1 frames"):
        stats.normalize(torch.from_numpy(x).cuda())
    assert _same(stats.mean(), x[0]) and not stats.std(ddof=0).any()
    z = stats.normalize(torch.from_numpy(x).cuda(), 0.5, ddof=0)
    assert not z.any()
    with pytest.raises(vad.hip.VadError, match="ddof"):
        stats.std(ddof=2)


def test_state_dict_round_trip(vad):
    x = _lognormal((9, 6, 7), 765)
    stats = vad.metrics.MapStatistics((6, 7)).update(torch.from_numpy(x).cuda())
    stats.meta = {"map": "mse", "sigma": None, "truncate": 4.0}
    saved = stats.state_dict()
    assert saved["count"] == 9 and saved["K"].dtype == torch.float64 and not saved["K"].is_cuda
    other = vad.metrics.MapStatistics((6, 7)).load_state_dict(saved)
    assert H.same_bits(other._state, stats._state) and other.count == 9 and other.meta == stats.meta
    assert _same(other.std(), ref.finalize(_restated(x))[1])
    assert stats.reset() is stats and stats.count == 0 and stats.device_count() == 0 and not stats._planes().any()
    with pytest.raises(vad.hip.VadError, match="frame_shape"):
        vad.metrics.MapStatistics((6, 8)).load_state_dict(saved)


def test_non_finite_values_stay_in_their_pixel(vad):
    shape = (2 * _plan(vad)["fif"] + 3, 6, 7)
    x = _lognormal(shape, 770)
    clean = vad.metrics.MapStatistics(shape[-2:]).update(torch.from_numpy(x).cuda())
    hit = np.zeros(shape[-2:], bool)
    hit[2, 3] = True
    for frame, value in ((5, np.nan), (0, np.inf), (shape[0] - 2, np.inf), (7, -np.inf)):
        y = x.copy()
        y[frame, 2, 3] = value
        stats = vad.metrics.MapStatistics(shape[-2:]).update(torch.from_numpy(y).cuda())
        assert _state_is(stats, _restated(y))
        mean, std = stats.mean().cpu().numpy(), stats.std().cpu().numpy()
        # the variance is NaN; the mean is NaN, or - an Inf behind the first frame - the infinity numpy's mean gives
        assert np.isnan(std[2, 3]) and not np.isfinite(mean[2, 3]) and (np.isnan(mean[2, 3]) or frame > 0)
        assert _same(mean[~hit], clean.mean().cpu().numpy()[~hit]) and _same(std[~hit], clean.std().cpu().numpy()[~hit])
        z = stats.normalize(torch.from_numpy(x).cuda())                     # a NaN std gives NaN, there alone
        assert torch.equal(torch.isnan(z).cpu(), torch.from_numpy(np.broadcast_to(hit, shape).copy()))
        assert torch.isnan(stats.normalize(torch.from_numpy(x).cuda(), return_max="only")).all()


@pytest.mark.parametrize("power", (20, -20))
def test_scaling_by_a_power_of_two_is_exact(vad, power):
    x = _lognormal((11, 6, 7), 780)
    base = vad.metrics.MapStatistics((6, 7)).update(torch.from_numpy(x).cuda())
    scale = np.float32(2.0 ** power)
    scaled = vad.metrics.MapStatistics((6, 7)).update(torch.from_numpy(x * scale).cuda())
    assert _same(scaled.mean(), base.mean().cpu().numpy() * scale) and _same(scaled.std(), base.std().cpu().numpy() * scale)
    assert _same(scaled.std(0), base.std(0).cpu().numpy() * scale)


def _normalize_case(vad):
    """Maps of three work-groups of pixels with a ragged last one, more frames than one work-group takes; std 0 and NaN pixels."""
    chunk = _plan(vad)["chunk"]
    shape = (7, 3, chunk - 5)
    x = _lognormal(shape, 791)
    mean = _lognormal(shape[1:], 792)
    std = _lognormal(shape[1:], 793)
    std[0, :5] = 0.0
    std[1, 7] = np.nan
    std[2, -1] = np.float32(1e-3)                                            # equal to the floor: not below it
    x[3, 0, 2] = mean[0, 2]                                                  # 0 / floor
    return x, mean, std, np.float32(1e-3)


def test_normalize_floor_nan_and_maxima(vad):
    x, mean, std, floor = _normalize_case(vad)
    lib, stream = vad.hip.lib(), vad.hip.current_stream()
    n, h, w = x.shape
    z = ref.normalize(x, mean, std, floor)
    assert np.array_equal(z[:, 0, :5], (x[:, 0, :5] - mean[0, :5]) / floor) and z[3, 0, 2] == 0 and np.isnan(z[:, 1, 7]).all()
    xt, mt, st = (torch.from_numpy(a).cuda() for a in (x, mean, std))
    need = lib.vad_map_normalize_workspace_bytes(n, h, w)
    assert need == 4 * n * 3

    def call(out, fmax, ws, ws_bytes, src=xt):
        return lib.vad_map_normalize(src.data_ptr(), n, h, w, mt.data_ptr(), st.data_ptr(), float(floor), vad.hip.ptr(out), vad.hip.ptr(fmax), ws, ws_bytes, stream)

    out, fmax = torch.full_like(xt, 5.0), torch.full((n,), 5.0, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert call(out, fmax, ws.data_ptr(), need) == 0
    assert _same(out, z) and _same(fmax, ref.frame_max(z)) and torch.isnan(fmax).all()     # the NaN pixel is in every frame
    st2 = st.clone()
    st2[1, 7] = 2.0
    std2 = std.copy()
    std2[1, 7] = 2.0
    z2 = ref.normalize(x, mean, std2, floor)
    fmax2 = torch.full((n,), 5.0, device="cuda")
    assert lib.vad_map_normalize(xt.data_ptr(), n, h, w, mt.data_ptr(), st2.data_ptr(), float(floor), None, fmax2.data_ptr(), ws.data_ptr(), need, stream) == 0
    assert _same(fmax2, ref.frame_max(z2)) and torch.isfinite(fmax2).all()               # frame_max alone
    # in place, without a workspace
    inplace = xt.clone()
    assert call(inplace, None, None, 0, src=inplace) == 0 and _same(inplace, z)
    # frames do not depend on the batch
    one = torch.empty(1, h, w, device="cuda")
    for i in (0, 3, 6):
        assert lib.vad_map_normalize(xt[i].data_ptr(), 1, h, w, mt.data_ptr(), st.data_ptr(), float(floor), one.data_ptr(), None, None, 0, stream) == 0
        assert _same(one[0], z[i])


def test_normalize_workspace_contract(vad):
    """Exact size, poisoned contents, guarded ends (tests/test_hip_workspace.py): the same bits for every fill, clean guards."""
    x, mean, std, floor = _normalize_case(vad)
    std[1, 7] = 2.0
    lib, stream = vad.hip.lib(), vad.hip.current_stream()
    n, h, w = x.shape
    z = ref.normalize(x, mean, std, floor)
    xt, mt, st = (torch.from_numpy(a).cuda() for a in (x, mean, std))
    need = lib.vad_map_normalize_workspace_bytes(n, h, w)
    for fill in H.POISONS:
        arena = H.GuardedArena(need, fill)
        out, fmax = torch.full_like(xt, 5.0), torch.full((n,), 5.0, device="cuda")
        assert lib.vad_map_normalize(xt.data_ptr(), n, h, w, mt.data_ptr(), st.data_ptr(), float(floor), out.data_ptr(), fmax.data_ptr(), arena.ptr(),
                                     need, stream) == 0
        arena.check(f"normalize workspace, fill 0x{fill:02X}")
        assert _same(out, z) and _same(fmax, ref.frame_max(z)), hex(fill)
    fresh = H.GuardedArena(need, 0x7F)
    out, fmax = torch.full_like(xt, 5.0), torch.full((n,), 5.0, device="cuda")
    assert lib.vad_map_normalize(xt.data_ptr(), n, h, w, mt.data_ptr(), st.data_ptr(), float(floor), out.data_ptr(), fmax.data_ptr(), fresh.ptr(),
                                 need - 1, stream) == -3                     # one byte short: refused, nothing written
    assert fresh.still_poison() and bool((out == 5.0).all()) and bool((fmax == 5.0).all())
    assert lib.vad_map_normalize(xt.data_ptr(), n, h, w, mt.data_ptr(), st.data_ptr(), float(floor), out.data_ptr(), None, fresh.ptr(), need, stream) == 0
    assert fresh.still_poison() and _same(out, z)                            # without frame_max the workspace is not used
    fresh.check("normalize workspace, unused")


def test_refusals(vad):
    VadError = vad.hip.VadError
    lib, stream = vad.hip.lib(), vad.hip.current_stream()
    x = torch.from_numpy(_lognormal((4, 8, 8), 800)).cuda()
    stats = vad.metrics.MapStatistics((8, 8)).update(x)
    before = stats._state.clone()
    # a state made for another geometry: the header is compared on the device, the call changes nothing
    assert lib.vad_mapstat_accumulate(x.data_ptr(), 4, 4, 16, stats._state.data_ptr(), stream) == 0
    other = vad.metrics.MapStatistics((4, 16)).update(x.view(4, 4, 16))
    other_before = other._state.clone()
    assert lib.vad_mapstat_merge(other._state.data_ptr(), stats._state.data_ptr(), 4, 16, stream) == 0
    mean, std = torch.zeros(4, 16, device="cuda"), torch.zeros(4, 16, device="cuda")
    assert lib.vad_mapstat_finalize(stats._state.data_ptr(), 4, 16, 1, mean.data_ptr(), std.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert H.same_bits(stats._state, before) and H.same_bits(other._state, other_before)
    assert torch.isnan(mean).all() and torch.isnan(std).all()
    out = torch.full_like(x, 5.0)
    m, s = stats.mean(), stats.std()
    for args, code, word in (((x.data_ptr(), 4, 8, 8, m.data_ptr(), s.data_ptr(), 0.0, out.data_ptr(), None, None, 0), -1, b"min_std"),
                             ((x.data_ptr(), 4, 8, 8, m.data_ptr(), s.data_ptr(), float("nan"), out.data_ptr(), None, None, 0), -1, b"min_std"),
                             ((x.data_ptr(), 4, 8, 8, m.data_ptr(), s.data_ptr(), 1e-3, None, None, None, 0), -1, b"both NULL"),
                             ((x.data_ptr(), 4, 8, 8, m.data_ptr(), s.data_ptr(), 1e-3, x[1].data_ptr(), None, None, 0), -1, b"partly overlaps"),
                             ((x.data_ptr() + 2, 4, 8, 8, m.data_ptr(), s.data_ptr(), 1e-3, out.data_ptr(), None, None, 0), -1, b"4-byte"),
                             ((x.data_ptr(), -1, 8, 8, m.data_ptr(), s.data_ptr(), 1e-3, out.data_ptr(), None, None, 0), -1, b"negative"),
                             ((x.data_ptr(), 4, 8, 8, m.data_ptr(), s.data_ptr(), 1e-3, out.data_ptr(), out.data_ptr(), None, 0), -3, b"workspace")):
        assert lib.vad_map_normalize(*args, stream) == code and word in lib.vad_last_error(), (args, lib.vad_last_error())
    assert lib.vad_mapstat_finalize(stats._state.data_ptr(), 8, 8, 2, m.data_ptr(), s.data_ptr(), stream) == -1 and b"ddof" in lib.vad_last_error()
    assert lib.vad_mapstat_accumulate(x.data_ptr() + 2, 4, 8, 8, stats._state.data_ptr(), stream) == -1 and b"4-byte" in lib.vad_last_error()
    assert lib.vad_mapstat_accumulate(x.data_ptr(), 4, 8, 8, stats._state.data_ptr() + 8, stream) == -1 and b"16-byte" in lib.vad_last_error()
    assert lib.vad_mapstat_accumulate(x.data_ptr(), -2, 8, 8, stats._state.data_ptr(), stream) == -1 and b"negative" in lib.vad_last_error()
    assert lib.vad_mapstat_merge(stats._state.data_ptr(), stats._state.data_ptr(), 8, 8, stream) == -1 and b"overlaps" in lib.vad_last_error()
    assert lib.vad_mapstat_accumulate(x.data_ptr(), 0, 8, 8, stats._state.data_ptr(), stream) == 0                  # n == 0: nothing launched
    with pytest.raises(ValueError, match="frame shape"):
        stats.update(x.view(4, 4, 16))
    with pytest.raises(ValueError, match="frame shape"):
        stats.normalize(x.view(4, 4, 16))
    with pytest.raises(VadError, match="contiguous"):
        stats.update(x.transpose(1, 2))
    with pytest.raises(VadError, match="float32"):
        stats.update(x.double())
    with pytest.raises(VadError, match="GPU"):
        stats.update(x.cpu())
    with pytest.raises(VadError, match="min_std"):
        stats.normalize(x, 0.0)
    with pytest.raises(VadError, match="out must be"):
        stats.normalize(x, out=torch.empty(4, 8, 4, device="cuda"))
    with pytest.raises(VadError, match="partly overlaps"):
        stats.normalize(x[:3], out=x[1:])
    with pytest.raises(VadError, match="out must be None"):
        stats.normalize(x, out=out, return_max="only")
    with pytest.raises(VadError, match="return_max"):
        stats.normalize(x, return_max="both")
    torch.cuda.synchronize()
    assert H.same_bits(stats._state, before) and bool((out == 5.0).all())    # a refused call writes nothing


# ------------------------------------------------------------------------------------------ through the models
def _image_setup(vad):
    model = vad.ConvAutoencoder(latent_dim=32)
    load_synthetic(vad, model, 31)
    model = model.cuda().eval()
    train = torch.from_numpy(vad.synth.frames(41, 0, 10, 3, 32, 32))
    x = torch.from_numpy(vad.synth.frames(42, 0, 6, 3, 32, 32))
    rng = np.random.default_rng(43)
    raw = np.zeros((6, 48, 40), np.uint8)
    for i in range(6):
        raw[i] = np.kron(rng.choice(np.array([0, 127, 128, 255], np.uint8), (6, 5), p=[0.55, 0.1, 0.1, 0.25]), np.ones((8, 8), np.uint8))
    masks = vad.scoring.resize_masks(torch.from_numpy(raw).cuda(), 32)
    labels = np.array([0, 1, 0, 1, 1, 0])
    kinds = ["good", "scratch", "good", "spot", "scratch", "good"]
    train_loader = [{"image": train[:4]}, {"image": train[4:7]}, {"image": train[7:]}]
    loader = [{"image": x[:4], "mask": masks[:4], "label": labels[:4], "defect_type": kinds[:4]},
              {"image": x[4:], "mask": masks[4:], "label": labels[4:], "defect_type": kinds[4:]}]
    return model, train_loader, loader, labels


def _raw_maps(vad, model, images, kind, sigma):
    with torch.no_grad():
        if kind == "mse":
            values = model.score_all(images.cuda())["errmap"]
        else:
            values = model.score_criteria(images.cuda(), ssim_map=True)["ssim_map"]
    return values if sigma is None else vad.metrics.smooth_maps(values, sigma)


@pytest.mark.parametrize("kind,sigma", [("mse", None), ("mse", 2.0), ("ssim", None)])
def test_drivers_calibrate_and_normalise(vad, kind, sigma):
    model, train_loader, loader, labels = _image_setup(vad)
    before = vad.hip.calls.get("mapstat_accumulate", 0)
    cal = vad.scoring.calibrate(model, train_loader, "cuda", map=kind, sigma=sigma)
    assert vad.hip.calls["mapstat_accumulate"] == before + 3                 # one update per batch
    assert cal.meta == {"map": kind, "sigma": sigma, "truncate": 4.0} and cal.count == 10 and cal.frame_shape == (32, 32)
    hand = vad.metrics.MapStatistics((32, 32))
    for b in train_loader:
        hand.update(_raw_maps(vad, model, b["image"], kind, sigma))
    assert H.same_bits(cal._state, hand._state)
    train_maps = torch.cat([_raw_maps(vad, model, b["image"], kind, sigma) for b in train_loader]).cpu().numpy()
    assert _same(cal._planes(), _restated(train_maps).planes())
    # continuing a calibration, and one whose maps are of another kind
    again = vad.scoring.calibrate(model, train_loader[:1], "cuda", map=kind, sigma=sigma, stats=vad.scoring.calibrate(
        model, train_loader[1:], "cuda", map=kind, sigma=sigma))
    assert again.count == 10 and again.meta == cal.meta
    with pytest.raises(ValueError, match="gathered on"):
        vad.scoring.calibrate(model, train_loader, "cuda", map=kind, sigma=3.0, stats=cal)

    m, min_std = 11, 1e-4
    z_hand = [cal.normalize(_raw_maps(vad, model, b["image"], kind, sigma), min_std) for b in loader]
    want = ref.normalize(torch.cat([_raw_maps(vad, model, b["image"], kind, sigma) for b in loader]).cpu().numpy(),
                         *ref.finalize(_restated(train_maps)), min_std)
    assert _same(torch.cat(z_hand), want)

    _, _, hist = vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=sigma, calibration=cal, min_std=min_std)
    by_hand = vad.metrics.ScoreHistogram(m)
    for b, z in zip(loader, z_hand):
        by_hand.accumulate(z, b["mask"])
    assert torch.equal(hist.counts(), by_hand.counts()) and torch.equal(hist.rejected(), by_hand.rejected())
    assert int(hist.counts().sum() + hist.rejected().sum()) == 6 * 32 * 32
    _, _, plain = vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=sigma)
    assert not torch.equal(plain.counts(), hist.counts())

    _, _, _, pro = vad.scoring.pixel_aupro(model, loader, "cuda", map=kind, mantissa_bits=m, sigma=sigma, calibration=cal, min_std=min_std)
    pro_hand = vad.metrics.ProHistogram(m)
    for b, z in zip(loader, z_hand):
        pro_hand.accumulate(z, b["mask"])
    assert torch.equal(pro.weighted(), pro_hand.weighted()) and torch.equal(pro.counts(), hist.counts())

    regions, maps = vad.scoring.localize(model, loader[0]["image"].cuda(), 2.0, map=kind, sigma=sigma, calibration=cal, min_std=min_std)
    assert _same(maps, z_hand[0].cpu().numpy())
    direct = vad.metrics.detect_regions(z_hand[0], 2.0)
    assert torch.equal(regions.records, direct.records) and torch.equal(regions.counts, direct.counts)
    assert int(regions.counts[:, 2].sum()) == int((z_hand[0] >= 2.0).sum())

    if sigma is not None:
        auroc, got_labels, scores, _ = vad.scoring.compute_auroc_smoothed(model, loader, "cuda", sigma=sigma, map=kind, calibration=cal, min_std=min_std)
        hand_scores = torch.cat([cal.normalize(_raw_maps(vad, model, b["image"], kind, sigma), min_std, return_max="only").reshape(-1)
                                 for b in loader]).cpu().numpy()
        assert np.array_equal(scores, hand_scores) and np.array_equal(hand_scores, ref.frame_max(want).reshape(-1))
        assert auroc == vad.scoring.roc_auc(labels, hand_scores) and got_labels.tolist() == labels.tolist()

    # a calibration applies to the maps it was gathered on
    other_sigma = 3.0 if sigma is None else None
    for call in (lambda **k: vad.scoring.pixel_auroc(model, loader, "cuda", **k), lambda **k: vad.scoring.pixel_aupro(model, loader, "cuda", **k),
                 lambda **k: vad.scoring.localize(model, loader[0]["image"].cuda(), 2.0, **k)):
        with pytest.raises(ValueError, match="gathered on"):
            call(map=kind, sigma=other_sigma, calibration=cal)
        with pytest.raises(ValueError, match="gathered on"):
            call(map="ssim" if kind == "mse" else "mse", sigma=sigma, calibration=cal)
        with pytest.raises(ValueError, match="gathered on"):
            call(map=kind, sigma=sigma, truncate=3.0, calibration=cal)
    with pytest.raises(ValueError, match="gathered on"):
        vad.scoring.compute_auroc_smoothed(model, loader, "cuda", sigma=4.0 if sigma != 4.0 else 2.0, map=kind, calibration=cal)
    small = vad.metrics.MapStatistics((16, 16))
    small.update(torch.rand(3, 16, 16, device="cuda"))
    small.meta = dict(cal.meta)
    with pytest.raises(ValueError, match="frame shape"):
        vad.scoring.pixel_auroc(model, loader, "cuda", map=kind, sigma=sigma, calibration=small)


def test_video_model_pools_clips_and_frames(vad):
    model = vad.VideoAutoencoder(latent_dim=32, lstm_hidden_dim=32, lstm_num_layers=1)
    load_synthetic(vad, model, 33)
    model = model.cuda().eval()
    clips = torch.from_numpy(vad.synth.clips(44, 0, 4, 3, 3, 32, 32))
    train_loader = [{"frames": clips[:3]}, {"frames": clips[3:]}]
    cal = vad.scoring.calibrate(model, train_loader, "cuda")
    assert cal.count == 4 * 3 and cal.frame_shape == (32, 32) and cal.meta["map"] == "mse"
    with torch.no_grad():
        errmap = torch.cat([model.score_all(b["frames"].cuda())["errmap"] for b in train_loader])
        first_two = model.score_all(clips[:2].cuda())["errmap"].cpu().numpy()
    assert errmap.shape == (4, 3, 1, 32, 32)
    want = _restated(errmap.cpu().numpy())                                   # every frame of every clip, clip by clip
    assert _state_is(cal, want)
    regions, maps = vad.scoring.localize(model, clips[:2].cuda(), 1.5, calibration=cal, min_std=1e-4)
    z = ref.normalize(first_two, *ref.finalize(want), 1e-4)
    assert maps.shape == (2, 3, 1, 32, 32) and _same(maps, z) and regions.counts.shape == (2, 3, 4)
    assert int(regions.counts[..., 2].sum()) == int((z >= 1.5).sum())
    with pytest.raises(vad.hip.VadError, match="error map only"):
        vad.scoring.calibrate(model, train_loader, "cuda", map="ssim")
