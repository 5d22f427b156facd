"""CPU checks of the weight-gradient launch plan (csrc/wgrad.hip): `vad_conv_wgrad_plan` reports the kernel form, the partial
slots and the work items `vad_conv_wgrad` would use, `vad_conv_wgrad_ws_floats` sizes the workspace those slots are written to.
Both are host arithmetic over the same per-form helpers.  No GPU needed: the library loads without one."""
import ctypes as C
import itertools
import json
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import GOLDEN

WAVE_F32, WAVE_BF16, WAVE_SPLIT, SPLIT_LDS, RING, PAIRS, BF16_LDS = range(7)     # include/vad_hip.h VAD_WGRAD_*
FP32, SPLIT, BF16, BF16S = range(4)                                              # VAD_PREC_*
DEFAULTS = (3, 3, 1)                                                             # pairs, split, ring_f32

TAPS = [1, 9]
CIN = [32, 64, 96, 128, 256, 512]
NCOLS = [32, 64, 96, 128, 256, 1024]
N = [1, 2, 7, 32]
H = [1, 5, 16, 64]
W = [1, 3, 16, 17, 33, 64, 256]


@pytest.fixture(scope="module")
def lib(vad):
    l = vad.hip.lib()
    yield l
    _set(l, DEFAULTS)


def _set(l, switches):
    l.vad_debug_set_wgrad_pairs(switches[0])
    l.vad_debug_set_wgrad_split(switches[1])
    l.vad_debug_set_wgrad_ring_f32(switches[2])


def _plan(l, precision, n, h, w, cin, ncols, taps):
    form, slots, items = C.c_int(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = l.vad_conv_wgrad_plan(precision, n, h, w, cin, ncols, taps, C.byref(form), C.byref(slots), C.byref(items))
    assert rc == 0, (rc, precision, n, h, w, cin, ncols, taps)
    return form.value, slots.value, items.value


def test_slots_fit_the_workspace_and_items_fit_32_bits_over_the_whole_domain(lib):
    """The one property that ties the plan to the workspace size: for every precision, shape and switch setting the partial
    slots the chosen form writes fit what vad_conv_wgrad_ws_floats reports (which knows neither the map width, the precision
    nor the switches), and the work items fit a 32-bit grid."""
    ws = {k: lib.vad_conv_wgrad_ws_floats(*k) for k in itertools.product(N, H, TAPS, CIN, NCOLS)}
    form, slots, items = C.c_int(), C.c_longlong(), C.c_longlong()
    out = (C.byref(form), C.byref(slots), C.byref(items))
    plan = lib.vad_conv_wgrad_plan
    bad, seen = [], set()
    try:
        for switches in itertools.product(range(4), range(4), range(2)):
            _set(lib, switches)
            for precision, taps, cin, ncols, n, h, w in itertools.product(range(4), TAPS, CIN, NCOLS, N, H, W):
                assert plan(precision, n, h, w, cin, ncols, taps, *out) == 0
                seen.add(form.value)
                if not (0 < slots.value * taps * cin * ncols <= ws[n, h, taps, cin, ncols] and 0 < items.value < 2 ** 31):
                    bad.append((switches, precision, taps, cin, ncols, n, h, w, form.value, slots.value, items.value))
    finally:
        _set(lib, DEFAULTS)
    assert not bad, (len(bad), bad[:10])
    assert seen == set(range(7))                  # the grid reaches every form


# (precision, taps, cin, ncols, w, switches) -> form; None = every value of that axis.  Derived by hand from the selection
# order: ring, LDS-staged, pairs, per-wave - the first that the precision, the switches and the shape admit.
CASES = [
    (BF16S, 9, 64, 64, 40, DEFAULTS, RING),
    (BF16S, 9, 64, 64, 40, (2, 3, 1), PAIRS),            # ncols is not a multiple of 128: no LDS-staged tile
    (BF16S, 9, 64, 64, 40, (1, 3, 1), PAIRS),
    (BF16S, 9, 64, 64, 40, (0, 3, 1), WAVE_BF16),
    (BF16S, 9, 64, 128, 40, (2, 3, 1), BF16_LDS),        # 64-channel tiles: only on maps wider than 16
    (BF16S, 9, 64, 128, 16, (2, 3, 1), PAIRS),
    (BF16S, 9, 128, 128, 16, (2, 3, 1), BF16_LDS),
    (BF16S, 1, 128, 256, None, DEFAULTS, BF16_LDS),      # the ring takes 3x3 layers only
    (BF16S, 1, 64, 256, None, DEFAULTS, PAIRS),          # 1x1 / transposed layers: LDS-staged with 128-channel tiles only
    (BF16S, 1, 32, 128, None, DEFAULTS, WAVE_BF16),
    (SPLIT, 9, 32, 64, 33, (3, 3, 1), RING),
    (SPLIT, 9, 32, 64, 33, (3, 2, 1), SPLIT_LDS),
    (SPLIT, 9, 32, 64, 16, (3, 2, 1), WAVE_SPLIT),       # the 32-channel pixel-halves tiling needs w > 16
    (SPLIT, 9, 64, 64, 16, (3, 2, 1), SPLIT_LDS),
    (SPLIT, 9, 32, 64, 33, (3, 1, 1), WAVE_SPLIT),
    (SPLIT, 1, 64, 256, None, DEFAULTS, WAVE_SPLIT),
    (SPLIT, 9, None, None, None, (3, 0, 1), WAVE_F32),
    (SPLIT, 1, None, None, None, (3, 0, 0), WAVE_F32),
    (FP32, 9, 128, 256, None, (3, 3, 1), RING),
    (FP32, 9, 128, 256, None, (3, 3, 0), WAVE_F32),
    (FP32, 1, None, None, None, DEFAULTS, WAVE_F32),
    (FP32, 9, 64, 32, None, DEFAULTS, WAVE_F32),         # the ring needs ncols % 64 == 0
    (FP32, 9, 96, 64, None, None, WAVE_F32),             # no tiled form takes cin 96
    (SPLIT, 9, 96, 64, None, DEFAULTS, WAVE_SPLIT),
    (BF16S, 9, 96, 64, None, None, WAVE_BF16),
    (BF16, None, None, None, None, None, WAVE_BF16),     # bf16 operands from fp32 tensors: always per-wave
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join("x" if v is None else "".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c))
def test_form_matches_the_selection_order(lib, case):
    precision, taps, cin, ncols, w, switches, want = case
    axis = lambda v, every: every if v is None else [v]
    all_switches = [DEFAULTS, (0, 0, 0), (1, 1, 0), (2, 2, 1), (0, 3, 1), (3, 0, 0)]
    try:
        for sw in axis(switches, all_switches):
            _set(lib, sw)
            for t, ci, nc, w_ in itertools.product(axis(taps, TAPS), axis(cin, CIN), axis(ncols, NCOLS), axis(w, W)):
                for n, h in ((2, 8), (7, 5)):
                    assert _plan(lib, precision, n, h, w_, ci, nc, t)[0] == want, (sw, t, ci, nc, w_, n, h)
    finally:
        _set(lib, DEFAULTS)


def test_plan_counts_for_a_hand_computed_layer(lib):
    """64 -> 128 channels, 3x3, 4 frames of 12 x 40, bf16 tensors."""
    # per-wave: 2 x 4 tiles of 32 x 32, ceil(2048 / 8) = 256 splits capped by the 48 image rows -> 48 slots, 384 wave items
    _set(lib, (0, 3, 1))
    try:
        assert _plan(lib, BF16S, 4, 12, 40, 64, 128, 9) == (WAVE_BF16, 48, 8 * 48)
        # pairs: 1 x 2 tiles of 64 x 64 x 3 kernel rows -> ceil(2048 / 6) = 342 -> 48 splits, 288 items
        _set(lib, (1, 3, 1))
        assert _plan(lib, BF16S, 4, 12, 40, 64, 128, 9) == (PAIRS, 48, 6 * 48)
        # LDS-staged: 64-channel tiles in pixel halves (ps 2): 1 x 1 x 3 tiles, target 4096 / 4 = 1024 work-groups -> 342 -> 48
        # splits, two slots each
        _set(lib, (2, 3, 1))
        assert _plan(lib, BF16S, 4, 12, 40, 64, 128, 9) == (BF16_LDS, 96, 3 * 48)
        # ring: 2 strips of 32 pixels, 1 x 1 tiles of 64 x 128; one frame per item costs the fewest rounds -> 4 x 2 slots
        _set(lib, DEFAULTS)
        assert _plan(lib, BF16S, 4, 12, 40, 64, 128, 9) == (RING, 8, 8)
        # 16 x 32 tiles of 32 x 128 -> ceil(2048 / 512) = 4 splits of ceil(9 / 4) = 3 rows: the fourth would be empty and is dropped
        assert _plan(lib, FP32, 1, 9, 8, 512, 4096, 1) == (WAVE_F32, 3, 512 * 3)
    finally:
        _set(lib, DEFAULTS)


def test_plan_rejects_what_conv_wgrad_rejects(lib):
    form, slots, items = C.c_int(), C.c_longlong(), C.c_longlong()
    out = (C.byref(form), C.byref(slots), C.byref(items))
    ok = (0, 2, 8, 8, 64, 64, 9)
    assert lib.vad_conv_wgrad_plan(*ok, *out) == 0
    for i, v in [(0, 4), (0, -1), (1, 0), (2, 0), (3, 0), (4, 48), (4, 0), (5, 16), (6, 3), (3, 1 << 20)]:
        args = list(ok)
        args[i] = v
        assert lib.vad_conv_wgrad_plan(*args, *out) == -1, args
    assert lib.vad_conv_wgrad_plan(*ok, None, C.byref(slots), C.byref(items)) == -1


def test_workspace_size_is_the_recorded_one(lib):
    """vad_conv_wgrad_ws_floats sizes the workspaces of both training steps: the table was written by the library before the
    plan existed (hand-written formulas per kernel form) and must not move."""
    table = json.loads((GOLDEN / "wgrad_ws_floats.json").read_text())
    assert table["order"] == ["n", "h", "taps", "cin", "ncols"]
    assert [table[k] for k in table["order"]] == [N, H, TAPS, CIN, NCOLS]
    got = [lib.vad_conv_wgrad_ws_floats(*k) for k in itertools.product(N, H, TAPS, CIN, NCOLS)]
    assert got == table["floats"]
    assert lib.vad_conv_wgrad_ws_floats(2, 8, 4, 64, 64) == 0 and lib.vad_conv_wgrad_ws_floats(2, 8, 9, 48, 64) == 0


def launch_digests(lib_path, workdir):
    """Per switch setting, a digest of what vad_conv_wgrad launches for every point of the grid: kernel symbol, grid, block, dynamic
    LDS, the integer kernel parameters and the reduce launch, recorded without a GPU by tests/wgrad_launch_trace.cpp (which
    takes the grid from here and the kernel handles' names from the library's symbol table)."""
    exe, syms = Path(workdir) / "wgrad_launch_trace", Path(workdir) / "kernels.txt"
    src = Path(__file__).with_name("wgrad_launch_trace.cpp")
    subprocess.run([shutil.which("g++") or shutil.which("c++"), "-O1", "-std=c++17", "-rdynamic", "-o", str(exe), str(src), "-ldl"], check=True)
    table = [line.split() for line in subprocess.run(["nm", str(lib_path)], check=True, capture_output=True, text=True).stdout.splitlines()]
    syms.write_text("".join(f"{t[0]} {t[2]}\n" for t in table if len(t) == 3 and "kernel" in t[2]))
    grid = [",".join(map(str, axis)) for axis in (CIN, NCOLS, N, H, W)]
    out = subprocess.run([str(exe), str(lib_path), str(syms), *grid], check=True, capture_output=True, text=True).stdout.split()
    return dict(zip(out[0::3], out[2::3])), sum(map(int, out[1::3]))


def test_launches_are_the_recorded_ones(vad, lib, tmp_path):
    """Kernel, grid, block and kernel parameters of every vad_conv_wgrad call over the grid and the 32 switch settings, against
    digests recorded from the library as it was when each kernel form had its own hand-written launch block
    (tests/golden/wgrad_launches.json): the launch plan chooses and sizes exactly what those blocks did."""
    want = json.loads((GOLDEN / "wgrad_launches.json").read_text())
    got, calls = launch_digests(vad.hip.LIB_PATH, tmp_path)
    assert calls == 32 * 4 * len(TAPS) * len(CIN) * len(NCOLS) * len(N) * len(H) * len(W) == want["calls"]
    assert len(got) == 32 and got == want["fnv1a64"]
