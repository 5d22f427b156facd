"""CPU checks of the robust frame scores: the numpy restatement (tests/map_topk_ref.py - what the GPU tests
compare the kernel with) against np.partition, np.sort, np.quantile(method="higher"), np.max / np.min / a float64 mean; the rank
helpers and the `reduce=` spec; and every refusal of `vad_map_topk` and `metrics.map_topk` that needs no device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import map_topk_ref as ref

REPO = Path(__file__).resolve().parent.parent
ERR_ARG, ERR_WS = -1, -3
MAX_PIXELS = 2 ** 23 - 1


def _maps(shape, seed, signed=True):
    """Seeded signed log-normal maps, as test_hip_map_smooth._maps makes them."""
    rng = np.random.default_rng(seed)
    x = (np.exp(rng.standard_normal(shape) * 3.0) * 1e-3).astype(np.float32)
    return x * rng.choice(np.array([-1, 1], np.float32), shape) if signed else x


def _ranks(p):
    return sorted({1, min(2, p), max(1, p - 1), p, ref.rank_of_fraction(0.001, p), ref.rank_of_fraction(0.01, p), ref.rank_of_fraction(0.1, p)})


# ------------------------------------------------------------------------------------------ the restatement
def test_key_orders_every_class_of_value():
    vals = np.float32([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 2.0, np.inf])
    k = ref.key(vals)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()
    assert k[3] == 0x7FFFFFFF and k[4] == 0x80000000                        # -0.0 directly below +0.0: the tie is decided
    rng = np.random.default_rng(1)
    x = rng.standard_normal(4096).astype(np.float32)
    assert np.array_equal(np.argsort(ref.key(x), kind="stable"), np.argsort(x, kind="stable"))   # distinct finite values: the usual order
    z = np.float32([0.0, -0.0, 0.0, -0.0])
    assert np.signbit(ref.descending(z)).tolist() == [False, False, True, True]


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (7, 9), (16, 20), (80, 96)])
def test_kth_equals_partition_and_sort(shape):
    x = _maps((3,) + shape, 40 + shape[0])
    p = shape[0] * shape[1]
    ranks = _ranks(p)
    for group in (ranks[:ref.MAX_RANKS], ranks[-1:]):
        got = ref.topk(x, group)
        for i, frame in enumerate(x):
            flat, srt = frame.reshape(-1), np.sort(frame.reshape(-1))
            for j, k in enumerate(group):
                assert got["kth"][i, j] == srt[p - k] == np.partition(flat, p - k)[p - k], (shape, k)
                top = srt[p - k:].astype(np.float64)
                assert abs(got["exact"][i, j] - top.sum() / k) <= p * 2.0 ** -53 * np.abs(top).sum() / k + 1e-300
                assert got["mean"][i, j] == np.float32(got["exact"][i, j]) and got["bound"][i, j] > 0
    one = ref.topk(x[1], ranks[:3])                                          # leading axes are batch axes
    assert ref.same_bits(one["kth"], ref.topk(x, ranks[:3])["kth"][1])


def test_rank_1_rank_p_and_the_top_p_mean_are_max_min_mean():
    x = _maps((4, 31, 29), 7)
    p = 31 * 29
    got = ref.topk(x, [1, p])
    flat = x.reshape(4, -1)
    assert np.array_equal(got["kth"][:, 0], flat.max(1)) and np.array_equal(got["kth"][:, 1], flat.min(1))
    mean64 = flat.astype(np.float64).mean(1)
    assert (np.abs(got["exact"][:, 1] - mean64) <= got["bound"][:, 1]).all()
    assert ref.mean_within_bound(mean64.astype(np.float32)[:, None], {"exact": got["exact"][:, 1:], "bound": got["bound"][:, 1:]})
    assert np.array_equal(got["mean"][:, 0], got["kth"][:, 0])               # the top-1 mean is the maximum, exactly
    # the bound is tight enough to mean something: half a float32 spacing dominates it on a 65,536-pixel frame
    big = _maps((256, 256), 8)
    k = ref.rank_of_fraction(0.01, big.size)
    r = ref.topk(big, [k])
    naive = float(np.sort(big.reshape(-1))[-k:].astype(np.float64).sum() / k)
    assert abs(naive - r["exact"][0]) <= big.size * 2.0 ** -52 * abs(r["exact"][0]) and r["bound"][0] < 0.51 * ref.spacing32(r["exact"][0])


@pytest.mark.parametrize("p", [1, 2, 15, 63, 65536])
def test_quantile_identity_on_distinct_values(p):
    rng = np.random.default_rng(p)
    x = rng.permutation(p).astype(np.float32) - np.float32(p // 2)           # distinct, both signs
    for q in (0, 0.5, 0.9, 0.99, 0.999, 1):
        k = ref.rank_of_quantile(q, p)
        assert 1 <= k <= p
        assert ref.topk(x.reshape(1, p), [k])["kth"][0] == np.quantile(x, q, method="higher"), (p, q)
    assert ref.rank_of_quantile(1, p) == 1 and ref.rank_of_quantile(0, p) == p


def test_nan_rule_and_infinities():
    x = _maps((3, 5, 7), 3)
    x[1, 4, 6] = np.nan
    got = ref.topk(x, [1, 35])
    assert (got["kth"][1].view(np.uint32) == ref.QNAN_BITS).all() and (got["mean"][1].view(np.uint32) == ref.QNAN_BITS).all()
    clean = ref.topk(np.delete(x, 1, 0), [1, 35])
    assert ref.same_bits(got["kth"][[0, 2]], clean["kth"]) and ref.same_bits(got["mean"][[0, 2]], clean["mean"])
    y = np.float32([[np.inf, 1.0, -np.inf, 2.0]])
    r = ref.topk(y, [1, 3, 4])
    assert r["kth"].tolist() == [np.inf, 1.0, -np.inf]
    assert r["mean"][0] == np.inf and r["mean"][1] == np.inf and np.isnan(r["mean"][2])
    assert ref.mean_within_bound(np.float32([np.inf, np.inf, np.nan]), r) and not ref.mean_within_bound(np.float32([np.inf, 1.0, np.nan]), r)


# ------------------------------------------------------------------------------------------ the rank helpers and the reduce spec
def test_rank_helpers(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    assert m.rank_of_fraction(0.01, 65536) == 656 == ref.rank_of_fraction(0.01, 65536)   # the double nearest 0.01 lies above it
    assert m.rank_of_fraction(0.001, 65536) == 66 and m.rank_of_fraction(0.1, 65536) == 6554 and m.rank_of_fraction(0.5, 65536) == 32768
    assert m.rank_of_fraction(1, 63) == 63 and m.rank_of_fraction(1e-9, 63) == 1 and m.rank_of_fraction(1.0, 1) == 1
    for p in (1, 2, 15, 63, 1024, 65536, MAX_PIXELS):
        for f in (1e-6, 0.001, 0.01, 0.1, 0.25, 1 / 3, 0.999, 1.0):
            assert m.rank_of_fraction(f, p) == ref.rank_of_fraction(f, p) and 1 <= m.rank_of_fraction(f, p) <= p
        for q in (0, 0.5, 0.9, 0.99, 0.999, 1, 1 / 3):
            assert m.rank_of_quantile(q, p) == ref.rank_of_quantile(q, p) and 1 <= m.rank_of_quantile(q, p) <= p
    for bad in (0, 0.0, -0.1, 1.0000001, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(VadError, match="rank_of_fraction: fraction"):
            m.rank_of_fraction(bad, 100)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, False):
        with pytest.raises(VadError, match="rank_of_quantile: q"):
            m.rank_of_quantile(bad, 100)
    for bad in (0, -1, 2.0, MAX_PIXELS + 1, None, True):
        with pytest.raises(VadError, match="pixels"):
            m.rank_of_fraction(0.5, bad)
        with pytest.raises(VadError, match="pixels"):
            m.rank_of_quantile(0.5, bad)


def test_reduce_spec(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    assert m.reduce_spec("max", "t") == ("rank", 1)
    assert m.reduce_spec(("topk", 0.01), "t") == ("topk", 0.01) and m.reduce_spec(["quantile", 1], "t") == ("quantile", 1)
    assert m.reduce_spec(("rank", np.int64(7)), "t") == ("rank", 7)
    for bad in ("mean", "min", None, ("topk",), ("topk", 0.1, 2), ("top", 0.1), 3, ("mean", 1)):
        with pytest.raises(VadError, match="who: reduce must be 'max'"):
            m.reduce_spec(bad, "who")
    for bad, text in ((("topk", 0), "fraction"), (("topk", 1.5), "fraction"), (("topk", "x"), "fraction"), (("quantile", -0.1), "q of"),
                      (("quantile", float("nan")), "q of"), (("rank", 0), "k of"), (("rank", 1.0), "k of"), (("rank", True), "k of")):
        with pytest.raises(VadError, match=text):
            m.reduce_spec(bad, "who")
    # the scoring entry points refuse a bad spec before they score anything (no model, no device needed)
    s = vad.scoring
    for call in (lambda: s.frame_scores(None, torch.zeros(1, 3, 16, 16), "mean"), lambda: s.compute_auroc_maps(None, [], "cpu", reduce=("topk", 0)),
                 lambda: s.frame_auroc(None, [], "cpu", reduce=("median", 1))):
        with pytest.raises(VadError, match="reduce"):
            call()
    with pytest.raises(VadError, match="map must be"):
        s.frame_scores(None, torch.zeros(1, 3, 16, 16), "max", map="psnr")
    with pytest.raises(VadError, match="error map only"):
        s.frame_scores(None, torch.zeros(1, 2, 3, 16, 16), "max", map="ssim")
    with pytest.raises(VadError, match="morph_steps"):
        s.frame_scores(None, torch.zeros(1, 3, 16, 16), "max", morph=("open", 0))


def test_host_refusals(vad):
    m, VadError = vad.metrics, vad.hip.VadError
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(VadError, match="map_topk: maps .* no CPU fallback"):
        m.map_topk(x, 1)
    with pytest.raises(VadError, match="map_topk: maps must be a torch tensor"):
        m.map_topk(np.zeros((16, 16), np.float32), 1)
    with pytest.raises(VadError, match="map_topk: kth and mean"):
        m.map_topk(x, 1, kth=False, mean=False)
    with pytest.raises(VadError, match="map_topk: kth and mean"):
        m.map_topk(x, 1, kth=1)
    with pytest.raises(VadError, match="reduce_maps: reduce must be"):
        m.reduce_maps(x, "mean")
    with pytest.raises(VadError, match="no CPU fallback"):
        m.reduce_maps(x, ("topk", 0.01))
    for bad in ([], [1] * 9, "1", None, 1.0, [1, 2.0], (True,)):
        with pytest.raises(VadError, match="ranks must be an int or a sequence of 1..8 ints"):
            m._check_ranks(bad, 256, "map_topk")
    for bad in (0, 257, [1, 0], [256, 257], -3):
        with pytest.raises(VadError, match="a rank must be in 1..256"):
            m._check_ranks(bad, 256, "map_topk")
    assert m._check_ranks(np.int64(5), 256, "t") == ([5], True) and m._check_ranks((256, 1, 1), 256, "t") == ([256, 1, 1], False)
    assert m.TOPK_MAX_RANKS == vad.hip.TOPK_MAX_RANKS == ref.MAX_RANKS == 8


# ------------------------------------------------------------------------------------------ the C ABI without a device
def _u(*ranks):
    return (C.c_uint * len(ranks))(*ranks)


def test_c_abi_refusals_need_no_device(vad):
    """Every argument check of vad_map_topk comes before anything is launched: with device pointers that are never followed."""
    lib = vad.hip.lib()
    maps, kth, mean, ws = 0x10000, 0x90000, 0xA0000, 0xB0000                 # 2 frames of 16 x 16: 2 KiB of maps
    big = 1 << 20

    def call(m=maps, n=2, h=16, w=16, ranks=(1, 256), nk=None, k=kth, t=mean, s=ws, sb=big):
        return lib.vad_map_topk(m, n, h, w, _u(*ranks) if ranks is not None else None, len(ranks) if nk is None else nk, k, t, s, sb, None)

    def refused(rc, *texts):
        msg = lib.vad_last_error()
        return rc == ERR_ARG and msg.startswith(b"map_topk: ") and all(t in msg for t in texts)

    assert refused(call(k=None, t=None), b"kth and topk_mean are both NULL")
    for nk in (0, -1, 9):
        assert refused(call(ranks=(1,) * 9, nk=nk), b"nk must be in 1..8"), nk
    assert refused(call(ranks=None, nk=1), b"ranks is NULL")
    for ranks, j in (((0,), 0), ((257,), 0), ((1, 256, 0), 2), ((1, 0xFFFFFFFF), 1)):
        assert refused(call(ranks=ranks), b"ranks[%d] must be in 1..256" % j), ranks
    assert refused(call(h=2, w=3, ranks=(7,)), b"ranks[0] must be in 1..6")
    assert refused(call(n=-1), b"negative")
    for h, w in ((0, 16), (16, 0), (-4, 16)):
        assert refused(call(h=h, w=w), b"must be positive"), (h, w)
    assert refused(call(h=4096, w=4096), b"pixels per frame")
    assert refused(call(n=1 << 50, h=2048, w=2048), b"not representable")
    assert refused(call(n=(1 << 56) + 1, h=1, w=1, ranks=(1,)), b"out of range")
    assert refused(call(m=None), b"maps is NULL")
    assert refused(call(s=None), b"ws is NULL")
    for kw, name in (({"m": maps + 2}, b"maps"), ({"k": kth + 1}, b"kth"), ({"t": mean + 2}, b"topk_mean"), ({"s": ws + 4}, b"ws")):
        assert refused(call(**kw), name + b" must be", b"aligned"), kw
    for out in (maps, maps + 4, maps + 2 * 256 * 4 - 4, maps - 2 * 2 * 4 + 4):
        assert refused(call(k=out), b"kth overlaps maps"), out
        assert refused(call(t=out), b"topk_mean overlaps maps"), out
    need = lib.vad_topk_workspace_bytes(2, 16, 16, 2)
    assert need == 2 * 2 * 16
    rc = call(sb=need - 1)
    assert rc == ERR_WS and lib.vad_last_error() == b"map_topk: ws_bytes 63 is less than vad_topk_workspace_bytes(2, 16, 16, 2) = 64"
    # n == 0: VAD_OK, nothing launched, no workspace needed; adjacent buffers do not overlap
    assert call(n=0, s=None, sb=0) == 0 and call(n=0, k=None) == 0 and call(n=0, t=None, ranks=(256,) * 8) == 0
    assert call(n=0, k=maps + 2 * 256 * 4) == 0 and call(n=0, k=maps - 2 * 2 * 4) == 0


def test_size_query_answers_zero_where_the_call_refuses_dims(vad):
    lib = vad.hip.lib()
    q = lib.vad_topk_workspace_bytes
    split, piece = C.c_int(), C.c_int()
    assert lib.vad_topk_plan(C.byref(split), C.byref(piece)) == 0 and lib.vad_topk_plan(None, None) == 0
    split, piece = split.value, piece.value
    assert 256 * 256 <= split < MAX_PIXELS and 1024 <= piece <= split         # the project's own maps stay on one work-group
    for n, h, w, nk in ((1, 1, 1, 1), (3, 7, 9, 8), (512, 256, 256, 5), (2, 1, split, 3), (1 << 56, 1, 1, 8),
                        (1, 1, split + 1, 1), (3, 2047, 4097, 8), (1 << 37, 2048, 4095, 1)):
        slices = -(-(h * w) // piece) if h * w > split else 0                # records; split path: + state, tables, slice sums
        assert q(n, h, w, nk) == n * nk * 16 + (n * (80 + nk * 8192 + slices * nk * 8) if slices else 0), (n, h, w, nk)
    assert q(0, 16, 16, 1) == 0                                              # nothing to hold
    ranks = _u(1)
    for n, h, w, nk in ((-1, 16, 16, 1), (1, 0, 16, 1), (1, 16, 0, 1), (1, -1, -1, 1), (1, 4096, 2048, 1), (1, 2896, 2897, 1),
                        (1 << 50, 2048, 2048, 1), ((1 << 56) + 1, 1, 1, 1), (1, 16, 16, 0), (1, 16, 16, 9), (1, 16, 16, -1)):
        assert q(n, h, w, nk) == 0, (n, h, w, nk)
        assert lib.vad_map_topk(0x10000, n, h, w, ranks if 1 <= nk <= 8 else _u(*([1] * 9)), nk, 0x90000, None, 0xB0000, 1 << 62, None) == ERR_ARG, (n, h, w, nk)


def test_header_and_signatures_agree(vad):
    hip = vad.hip
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "vad_hip.h").read_text(), flags=re.S)
    lib = hip.lib()
    for name, ret, nargs in (("vad_map_topk", "int", 11), ("vad_topk_workspace_bytes", "size_t", 4), ("vad_topk_plan", "int", 2)):
        decl = re.search(r"\b%s\s+%s\s*\((.*?)\);" % (ret, name), header, flags=re.S)
        assert decl, f"{name} is not declared in include/vad_hip.h"
        assert name in hip.SIGNATURES and hasattr(lib, name)
        assert len(hip.SIGNATURES[name][1]) == len(decl.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+VAD_TOPK_MAX_RANKS\s+8\b", header)
    assert "map_topk.hip" in hip.SOURCES and (hip.CSRC / "map_topk.hip").exists()
    assert hip.ABI_VERSION == 3 and lib.vad_abi_version() == 3               # additive: the version stays
    src = (hip.CSRC / "map_topk.hip").read_text()
    assert "atomicAdd(&hist" in src and not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", src)   # integer counters only
