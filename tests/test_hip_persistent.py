"""GPU layer tests of the THROUGHPUT tilings and of the persistent kernels' multi-iteration walks.

The other layer tests run 2 or 3 small frames: every launch then takes a latency tiling or the gate-split kernel, and every
work-group of a persistent kernel runs one frame (or item) and exits.  Here `vad_debug_set_plan_cus(1)` makes every planning
decision see ONE compute unit, so a few dozen small frames run the tilings the benchmark runs, on a grid of `occupancy`
work-groups that each walk many frames.  After every walked launch `vad_debug_last_plan` is read back and the WALK CONDITION is
asserted (a gate: it fails, never skips):

  * `items >= 3 * walks + 1`: some walk runs a first, two middle and a last iteration (walks = the grid; 4 x the grid for the
    wave-persistent transposed-convolution kernel, whose items are walked by waves);
  * unequal trip counts, `items % walks != 0` - for item walkers and for SINGLE-TILE frames (n = 29 frames, a prime, of exactly
    one tile of the tiling under test: 16x16 where the tile is 16 rows, 8x16 / 4x16 for the 8- and 4-row tiles, so that
    per_frame = 1 and the grid is `min(29, occupancy)` frame groups);
  * for RAGGED MULTI-TILE frames (37x21, 38x22 where pooling needs even sizes, n = 5; per_frame > cap) the frame groups collapse
    to one: `items == n * grid`, every work-group walks all n frames behind each other.  Trip counts are equal there by
    construction (items is a multiple of the grid whenever fgroups == 1), so the second condition is replaced by that identity.

Every walked launch is then held to (a) the oracle on frames 0, middle and last at the layer tests' tolerances (ATOL = 3e-5;
2e-5 for the ConvLSTM step), (b) bit identity of EVERY frame with the same frame launched alone (n = 1), and - exact fp32 -
(c) bit identity with the one-tile-per-work-group kernel (`vad_debug_set_conv_variant(0)`) and with the default-planned
launch (`plan_cus` 0) of the same data.  bf16 forms are checked by the helpers lifted from tests/test_hip_train_bf16.py.
Nothing is timed.

Persistent instantiation families and the case that walks each:

  conv3x3_mfma_pkernel, exact fp32     (2,2,2,2) PLAIN / POOL, (1,2,2,2) PLAIN, (2,2,4,1) PLAIN / POOL, (2,1,4,1) PLAIN / POOL:
                                       test_conv3x3_fp32_tilings  ((1,2,2,2) has no POOL instantiation: pooled cout % 128
                                       launches always take (2,2,2,2)); FS_PAD / FS_TIME among its cases
  conv3x3_mfma_pkernel, split          (4,1,1,4), (2,1,2,2), (2,1,4,1): test_conv3x3_split_tilings
  conv3x3_mfma_pkernel, bf16 / IO16    the same tilings on bf16 operands and bf16 tensors, forward and data gradient:
                                       test_conv3x3_bf16_walks
  conv3x3_mfma_pkernel, fused enc1     fp32 and split, both geometries: test_conv3x3_c3_fused_walks (uint8 frames reach the
                                       kernel through the models only: test_image_model_scores_do_not_depend_on_the_plan)
  conv3x3_mfma_pkernel, MODE_LSTM      (1,4,2,2), variant 1|8, zero / non-zero state, fp32 and split: test_convlstm_step_walks
                                       (cx != hid in fp32 always runs the one-tile kernel: asserted as NOT persistent)
  conv3x3_mfma_pkernel, kpart          the x halves of vad_convlstm_seq, (1,2,2,2): test_convlstm_seq_x_halves_walk (read from
                                       the record of the latest PERSISTENT launch: a sequence ends with a step)
  conv3x3_c3_pkernel                   pooled / un-pooled: test_conv3x3_c3_walks; bf16 output and bf16 operands:
                                       test_conv3x3_c3_bf16_output_walks
  convt2x2_pkernel                     fp32 (2,4), split (2,2), small_ct (1,1), FS_TIME: test_convt2x2_walks; bf16 operands
                                       and tensors (2,2): test_convt2x2_and_conv1x1_bf16_walks
  convt2x2_pkernel as vad_conv1x1_p    narrow (2,1) and wide (2,2), ragged npix: test_conv1x1_p_walks
  dec4_score_kernel                    float targets, band chosen by the overridden plan: test_dec4_score_walks (uint8 targets:
                                       through the image model)
  conv3x3_wino_pkernel                 NT 2 and the fused-cell form, two shapes of tests/test_hip_layers.py each:
                                       test_conv3x3_winograd_walks, test_convlstm_step_winograd_walks
  statistics (ST = 1) instantiations   conv3x3 / convt2x2 in fp32, split, bf16 operands and bf16 tensors, partial rows against
                                       float64 sums: test_statistics_launches_walk; first layer: test_first_layer_statistics_walk
  the training steps                   re-run with their own bounds under the plan; the smallest cases are one or two frames and do
                                       not walk: test_training_steps_hold_their_bounds_under_the_plan,
                                       test_bf16_training_holds_its_bounds_under_the_plan (16 frames of 64 x 64)

`vad_convt2x2_to3_score` and `vad_conv3x3_to3_score` (csrc/tail.hip) launch one work-group per tile / per four items: their grids
are not planned from the CU count and they have no item loop, so there is nothing for the switch to change."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_hip_layers as L
import test_hip_train_bf16 as B
from test_hip_train_step import _fixed_cpu_threads      # noqa: F401  (autouse: the CPU references of the training cases)
from conftest import load_synthetic, max_abs
from oracle import c_oracle

pytestmark = pytest.mark.gpu

ATOL = L.ATOL            # 3e-5, the layer tests' bound
LSTM_ATOL = 2e-5         # the ConvLSTM step's
FIELDS = ("grid", "items", "walks", "family", "mt", "nt", "wm", "wn", "mode")
CONV3, C3FUSED, C3, CONVT, CONV1X1, DEC4, WINO = 1, 2, 3, 4, 5, 6, 7
PLAIN, POOL, LSTM = 0, 1, 2


@pytest.fixture(scope="module", autouse=True)
def one_cu(vad):
    """Every launch of this module is planned for one CU; the default comes back whatever happens."""
    l = vad.hip.lib()
    vad.hip.check(l.vad_debug_set_plan_cus(1))
    try:
        yield l
    finally:
        l.vad_debug_set_plan_cus(0)


class _default_plan:
    """`with _default_plan(l):` - the device's own CU count inside, one CU again after."""

    def __init__(self, l):
        self.l = l

    def __enter__(self):
        self.l.vad_debug_set_plan_cus(0)

    def __exit__(self, *exc):
        self.l.vad_debug_set_plan_cus(1)


class _variant:
    def __init__(self, l, bits):
        self.l, self.bits = l, bits

    def __enter__(self):
        self.l.vad_debug_set_conv_variant(self.bits)

    def __exit__(self, *exc):
        self.l.vad_debug_set_conv_variant(1)


def last_plan(l, persistent=False):
    """The read-back of the thread's latest layer launch, or (persistent) of its latest persistent one."""
    buf = (C.c_int * (2 * len(FIELDS)))()
    assert l.vad_debug_last_plan(buf, len(buf)) == len(buf)
    return dict(zip(FIELDS, buf[len(FIELDS):] if persistent else buf[:len(FIELDS)]))


def assert_walk(plan, what, n=None, multi=False):
    """The walk condition of the module docstring on a read-back."""
    print(f"{what}: {plan}")
    grid, items, walks = plan["grid"], plan["items"], plan["walks"]
    assert grid > 0, f"{what}: the launch was not persistent"
    assert items >= 3 * walks + 1 and items >= 3 * grid + 1, f"{what}: no walk runs a first, two middle and a last iteration: {plan}"
    if multi:
        assert items == n * grid, f"{what}: more than one frame group on ragged multi-tile frames: {plan}"
    else:
        assert items % walks != 0, f"{what}: equal trip counts: {plan}"


def assert_tiling(plan, family, tiling=None, mode=None):
    assert plan["family"] == family, plan
    if tiling is not None:
        assert (plan["mt"], plan["nt"], plan["wm"], plan["wn"])[:len(tiling)] == tuple(tiling), plan
    if mode is not None:
        assert plan["mode"] == mode, plan


def _three(n):
    return [0, n // 2, n - 1]


# ------------------------------------------------------------------------------------------------ vad_conv3x3
def _conv3x3_case(l, H, cin, cout, h, w, n, act, pool, fs, multi, tiling, precision):
    rng = L._rng(cin * 1000 + cout + h + n)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt, b, bn = L._conv_params(rng, cout, cin)
    layout = getattr(H, fs) if fs else None
    with L._precision(H, precision):
        got = H.conv3x3(x, wt, b, bn, act, pool, fs=layout)
        plan = last_plan(l)
        assert_walk(plan, f"conv3x3 {tiling} precision {precision}", n, multi)
        assert_tiling(plan, CONV3, tiling, POOL if pool else PLAIN)
        assert np.isfinite(got).all()
        idx = _three(n)                                                                    # (a)
        assert max_abs(got[idx], L._ref_conv(x[idx], wt, b, bn, act, pool)) < ATOL
        for i in range(n):                                                                 # (b)
            assert np.array_equal(got[i:i + 1], H.conv3x3(x[i:i + 1], wt, b, bn, act, pool, fs=layout)), i
        if precision == 0:                                                                 # (c)
            with _variant(l, 0):
                assert np.array_equal(got, H.conv3x3(x, wt, b, bn, act, pool, fs=layout))
                assert last_plan(l)["grid"] == 0
            with _default_plan(l):
                assert np.array_equal(got, H.conv3x3(x, wt, b, bn, act, pool, fs=layout))


@pytest.mark.parametrize("cin,cout,h,w,n,act,pool,fs,multi,tiling", [
    (32, 128, 8, 16, 29, 1, True, None, False, (2, 2, 2, 2)),
    (64, 128, 38, 22, 5, 2, True, None, True, (2, 2, 2, 2)),
    (32, 128, 70, 45, 29, 0, False, None, True, (2, 2, 2, 2)),       # un-pooled: 29 x 27 = 783 >= 768 tiles of 8 x 16 pixels
    (32, 128, 4, 16, 29, 2, False, "FS_TIME", False, (1, 2, 2, 2)),
    (128, 256, 37, 21, 5, 1, False, None, True, (1, 2, 2, 2)),
    (64, 64, 16, 16, 29, 1, False, "FS_PAD", False, (2, 2, 4, 1)),
    (32, 64, 16, 16, 29, 0, True, None, False, (2, 2, 4, 1)),
    (32, 192, 38, 22, 5, 2, True, None, True, (2, 2, 4, 1)),
    (32, 96, 37, 21, 5, 0, False, None, True, (2, 1, 4, 1)),
    (32, 32, 16, 16, 29, 1, True, None, False, (2, 1, 4, 1)),
    (64, 32, 16, 16, 29, 2, False, None, False, (2, 1, 4, 1)),
])
def test_conv3x3_fp32_tilings(one_cu, cin, cout, h, w, n, act, pool, fs, multi, tiling):
    import hip_helpers as H
    _conv3x3_case(one_cu, H, cin, cout, h, w, n, act, pool, fs, multi, tiling, 0)


@pytest.mark.parametrize("cin,cout,h,w,n,act,pool,multi,tiling", [
    (32, 128, 8, 16, 29, 1, False, False, (4, 1, 1, 4)),
    (64, 128, 38, 22, 5, 2, True, True, (4, 1, 1, 4)),
    (32, 64, 8, 16, 29, 0, True, False, (2, 1, 2, 2)),
    (32, 96, 37, 21, 5, 2, False, True, (2, 1, 4, 1)),
])
def test_conv3x3_split_tilings(one_cu, cin, cout, h, w, n, act, pool, multi, tiling):
    import hip_helpers as H
    _conv3x3_case(one_cu, H, cin, cout, h, w, n, act, pool, None, multi, tiling, 1)


@pytest.fixture
def scratch():
    """`scratch(n)`: n floats of NaN between guards that must be untouched when the test ends - what the helpers of
    tests/test_hip_train_bf16.py take their scratch from."""
    import hip_helpers as H
    pool = H.ArenaPool(0xFF)
    yield pool.floats
    pool.check()


def _tiling_of(cout):
    return (4, 1, 1, 4) if cout % 128 == 0 else (2, 1, 2, 2) if cout % 64 == 0 else (2, 1, 4, 1)


@pytest.mark.parametrize("n,h,w,cin,cout,multi", [(29, 8, 16, 32, 128, False), (29, 8, 16, 64, 64, False), (5, 37, 21, 64, 128, True)])
def test_conv3x3_bf16_walks(vad, one_cu, scratch, n, h, w, cin, cout, multi):
    """bf16 operands (VAD_PREC_BF16) and bf16 tensors (VAD_PREC_BF16S), forward and data gradient, checked the way
    tests/test_hip_train_bf16.py checks them, with the walk condition and the tiling asserted behind each of the four launches."""
    seen = []

    def launched(what):
        plan = last_plan(one_cu)
        assert_walk(plan, what, n, multi)
        assert_tiling(plan, CONV3, _tiling_of(cin if "gradient" in what else cout), PLAIN)
        seen.append(what)

    B.check_conv3x3_on_bf16_tensors(vad, n, h, w, cin, cout, launched, ws=scratch)
    assert len(seen) == 4


# ------------------------------------------------------------------------------------------------ first layer
@pytest.mark.parametrize("h,w,n,multi", [(16, 16, 29, False), (38, 22, 5, True)])
@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_c3_fused_walks(one_cu, h, w, n, multi, precision):
    """The fused first block: a frame's first stage is staged right behind the barrier that ends the previous frame's, so the
    hand-over between frames is what (b) pins."""
    import hip_helpers as H
    l = one_cu
    rng = L._rng(h * 100 + w + n)
    x = rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32)
    p0, p1 = L._conv_params(rng, 32, 3), L._conv_params(rng, 32, 32)
    with L._precision(H, precision):
        got = H.conv3x3_c3_fused(x, *p0, *p1)
        plan = last_plan(l)
        assert_walk(plan, f"conv3x3_c3_fused precision {precision}", n, multi)
        assert_tiling(plan, C3FUSED, (2, 1, 4, 1), POOL)
        idx = _three(n)
        ref = L._ref_conv(L._ref_conv(x[idx], *p0, 1, False), *p1, 1, True)
        assert np.isfinite(got).all() and max_abs(got[idx], ref) < ATOL
        for i in range(n):
            assert np.array_equal(got[i:i + 1], H.conv3x3_c3_fused(x[i:i + 1], *p0, *p1)), i
        if precision == 0:
            with _variant(l, 0):
                assert np.array_equal(got, H.conv3x3_c3_fused(x, *p0, *p1))
                assert last_plan(l)["grid"] == 0
            with _default_plan(l):
                assert np.array_equal(got, H.conv3x3_c3_fused(x, *p0, *p1))


@pytest.mark.parametrize("cout,h,w,n,act,pool", [(32, 16, 16, 29, 1, False), (32, 16, 16, 29, 2, True), (64, 70, 14, 9, 0, True)])
def test_conv3x3_c3_walks(one_cu, cout, h, w, n, act, pool):
    """vad_conv3x3_c3 walks tiles of 32 rows x 16 columns across the whole batch (an item walker): 29 / 29 / 27 items."""
    import hip_helpers as H
    l = one_cu
    rng = L._rng(cout + h + n)
    x = rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float32)
    wt, b, bn = L._conv_params(rng, cout, 3)
    got = H.conv3x3(x, wt, b, bn, act, pool)
    plan = last_plan(l)
    assert_walk(plan, "conv3x3_c3")
    assert_tiling(plan, C3, mode=POOL if pool else PLAIN)
    idx = _three(n)
    assert np.isfinite(got).all() and max_abs(got[idx], L._ref_conv(x[idx], wt, b, bn, act, pool)) < ATOL
    for i in range(n):
        assert np.array_equal(got[i:i + 1], H.conv3x3(x[i:i + 1], wt, b, bn, act, pool)), i
    with _variant(l, 0):
        assert np.array_equal(got, H.conv3x3(x, wt, b, bn, act, pool))
        assert last_plan(l)["grid"] == 0
    with _default_plan(l):
        assert np.array_equal(got, H.conv3x3(x, wt, b, bn, act, pool))


def test_conv3x3_c3_bf16_output_walks(vad, one_cu):
    """The bf16-output forms of the first layer (training forward of the bf16-tensor mode), held to what
    test_first_and_last_layer_on_bf16_tensors holds them to, on 29 single-tile frames."""
    import hip_helpers as H
    l, rng, n, h, w = one_cu, L._rng(29), 29, 16, 16
    x = H.dev(rng.uniform(-1, 1, (n, 3, h, w)))
    w0 = rng.standard_normal((32, 3, 3, 3)).astype(np.float32) * 0.2
    wp, bo = H.pack_conv3x3(w0, rng.standard_normal(32).astype(np.float32) * 0.1)
    nan = lambda dt: torch.full((n, h, w, 32), float("nan"), dtype=dt, device="cuda")
    o32, o16 = nan(torch.float32), nan(torch.bfloat16)
    vad.hip.check(l.vad_conv3x3_c3(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), o32.data_ptr(), n, h, w, 32, 0, 0, H.stream()))
    assert_walk(last_plan(l), "conv3x3_c3, un-activated")
    vad.hip.check(l.vad_conv3x3_c3_bf16(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), o16.data_ptr(), n, h, w, 32, H.stream()))
    assert_walk(last_plan(l), "conv3x3_c3_bf16")
    assert torch.equal(o16, o32.to(torch.bfloat16))
    xr, wr = x.to(torch.bfloat16).float(), torch.from_numpy(w0).to(torch.bfloat16).float().numpy()
    wpr, _ = H.pack_conv3x3(wr, np.zeros(32, np.float32))
    o32r, o16op, o16op_any = nan(torch.float32), nan(torch.bfloat16), nan(torch.bfloat16)
    vad.hip.check(l.vad_conv3x3_c3(xr.data_ptr(), wpr.data_ptr(), bo.data_ptr(), o32r.data_ptr(), n, h, w, 32, 0, 0, H.stream()))
    vad.hip.check(l.vad_conv3x3_c3_bf16op(xr.data_ptr(), wpr.data_ptr(), bo.data_ptr(), o16op.data_ptr(), n, h, w, 32, H.stream()))
    assert_walk(last_plan(l), "conv3x3_c3_bf16op")
    vad.hip.check(l.vad_conv3x3_c3_bf16op(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), o16op_any.data_ptr(), n, h, w, 32, H.stream()))
    want = o32r.to(torch.bfloat16)
    same = (o16op == want).float().mean().item()
    ulp = (o16op.float() - want.float()).abs() / (want.float().abs() * 2.0 ** -7 + 1e-30)
    assert same > 0.995 and float(ulp.max()) <= 1.0 + 1e-6, (same, float(ulp.max()))
    assert torch.equal(o16op_any, o16op)
    with _default_plan(l):                                    # the grouping of the walk changes no output bit
        d16 = nan(torch.bfloat16)
        vad.hip.check(l.vad_conv3x3_c3_bf16op(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), d16.data_ptr(), n, h, w, 32, H.stream()))
    assert torch.equal(d16, o16op_any)


# ------------------------------------------------------------------------------------------------ ConvLSTM step
def _lstm_inputs(rng, n, cx, hid, h, w, zero_state):
    x = rng.standard_normal((n, cx, h, w)).astype(np.float32)
    wt = (rng.standard_normal((4 * hid, cx + hid, 3, 3)) * np.sqrt(1.0 / ((cx + hid) * 9))).astype(np.float32)
    b = (rng.standard_normal(4 * hid) * 0.1).astype(np.float32)
    hp = None if zero_state else (rng.standard_normal((n, hid, h, w)) * 0.5).astype(np.float32)
    cp = None if zero_state else rng.standard_normal((n, hid, h, w)).astype(np.float32)
    return x, hp, cp, wt, b


@pytest.mark.parametrize("cx,hid,h,w,n,zero_state,precision,multi", [
    (64, 64, 4, 16, 29, True, 0, False), (64, 64, 4, 16, 29, False, 0, False), (64, 64, 37, 21, 5, False, 0, True),
    (64, 64, 4, 16, 29, False, 1, False), (64, 64, 37, 21, 5, True, 1, True), (32, 64, 4, 16, 29, False, 0, None)])
def test_convlstm_step_walks(one_cu, cx, hid, h, w, n, zero_state, precision, multi):
    """The LSTM-mode persistent kernel (variant 1|8: never the small-grid kernels).  multi None: cx != hid, which the exact step
    always runs as one tile per work-group - asserted as not persistent, and held to (a), (b), (c) like the others."""
    import hip_helpers as H
    l = one_cu
    x, hp, cp, wt, b = _lstm_inputs(L._rng(cx + hid + h + n), n, cx, hid, h, w, zero_state)
    sl = lambda a, i: None if a is None else a[i]
    zeros = np.zeros((n, hid, h, w), np.float32)
    with L._precision(H, precision), _variant(l, 1 | 8):
        gh, gc = H.convlstm_step(x, hp, cp, wt, b)
        plan = last_plan(l)
        if multi is None:
            assert plan["grid"] == 0, plan
        else:
            assert_walk(plan, f"convlstm_step precision {precision}", n, multi)
            assert_tiling(plan, CONV3, (1, 4, 2, 2), LSTM)
        idx = _three(n)
        rh, rc = c_oracle.convlstm_cell(x[idx], (zeros if hp is None else hp)[idx], (zeros if cp is None else cp)[idx], wt, b)
        assert np.isfinite(gh).all() and max_abs(gh[idx], rh) < LSTM_ATOL and max_abs(gc[idx], rc) < LSTM_ATOL
        for i in range(n):
            ah, ac = H.convlstm_step(x[i:i + 1], sl(hp, slice(i, i + 1)), sl(cp, slice(i, i + 1)), wt, b)
            assert np.array_equal(gh[i:i + 1], ah) and np.array_equal(gc[i:i + 1], ac), i
    if precision == 0:
        with _variant(l, 0):
            th, tc = H.convlstm_step(x, hp, cp, wt, b)
        with _default_plan(l):
            dh, dc = H.convlstm_step(x, hp, cp, wt, b)
        for oh, oc in ((th, tc), (dh, dc)):
            assert np.array_equal(gh, oh) and np.array_equal(gc, oc)


@pytest.mark.parametrize("layers,b,t,h,w", [(1, 29, 3, 4, 16), (2, 5, 3, 5, 9)])
def test_convlstm_seq_x_halves_walk(vad, one_cu, layers, b, t, h, w):
    """vad_convlstm_seq on a small grid computes bias + x half of the steps ahead of the recurrence with vad_conv3x3_kpart (a
    channel sub-range of the cell's weights).  Under the one-CU plan that launch takes the (1,2,2,2) throughput tiling (the
    default plan: the gate-split kernel) and walks its frames: all 87 source frames of the one-layer case in one launch, the 5
    clips of a step in the upper layer of the two-layer case (a wavefront on helper streams).  The steps that follow are not
    persistent, so the walk is read from the record of the latest persistent launch.  A cell has 4 * hid >= 256 output columns =
    at least two column blocks per tile, more than half the occupancy: one frame group, `items == n * grid`.  Sequences and
    states are the same bits under both plans, and the torch composition of the module agrees at the step's tolerance."""
    m = vad.ConvLSTM(input_dim=64, hidden_dims=[64] * layers, kernel_size=3, num_layers=layers, return_all_layers=True)
    load_synthetic(vad, m, 77)
    m = m.cuda().eval()
    x = torch.from_numpy(L._rng(78 + layers).standard_normal((b, t, 64, h, w)).astype(np.float32)).cuda()
    before = vad.hip.calls["convlstm_seq"]
    with torch.no_grad():
        outs, states = m(x)
        assert last_plan(one_cu)["grid"] == 0                          # the last launch is a step: the small-grid kernel
        plan = last_plan(one_cu, persistent=True)
        with _default_plan(one_cu):
            outs0, states0 = m(x)
    assert vad.hip.calls["convlstm_seq"] == before + 2
    n = b * t if layers == 1 else b
    assert_walk(plan, f"conv3x3_kpart, {layers} layer(s)", n, multi=True)
    assert_tiling(plan, CONV3, (1, 2, 2, 2), PLAIN)
    for a, a0 in zip(outs, outs0):
        assert torch.isfinite(a).all() and torch.equal(a, a0)
    for (h1, c1), (h0, c0) in zip(states, states0):
        assert torch.equal(h1, h0) and torch.equal(c1, c0)
    with torch.enable_grad():                                  # autograd on: the torch composition
        ref, _ = m(x)
    for a, r in zip(outs, ref):
        assert max_abs(a.cpu().numpy(), r.detach().cpu().numpy()) < LSTM_ATOL


# ------------------------------------------------------------------------------------------------ transposed convolution, 1x1
def _convt_ref(x, wt, b, bn, act):
    ref = c_oracle.batchnorm_eval(c_oracle.convt2x2(x, wt, b), *bn)
    return np.where(ref > 0, ref, np.float32(0.2) * ref) if act == 1 else (np.maximum(ref, 0) if act == 2 else ref)


@pytest.mark.parametrize("cin,cout,h,w,n,act,precision,fs,tiling", [
    (64, 32, 20, 16, 29, 2, 0, None, (2, 4)), (32, 32, 35, 21, 7, 1, 0, "FS_TIME", (2, 4)), (64, 32, 20, 16, 29, 0, 1, None, (2, 2)),
    (128, 32, 35, 13, 7, 2, 1, None, (2, 2)), (64, 32, 4, 16, 3, 2, 0, None, (1, 1))])
def test_convt2x2_walks(one_cu, cin, cout, h, w, n, act, precision, fs, tiling):
    """Items (a frame's 4-row x 16-column tile x one column group) are walked by WAVES, four per work-group: 145, 126, 290 and
    126 items here, none a multiple of 4 x occupancy for any occupancy up to 8.  The small_ct form
    (1,1) is chosen only below 4 x CUs items of the (2,4) tiling, i.e. for at most 24 items of its own under the one-CU plan:
    against at least 8 waves that cannot meet the walk condition, so its case asserts the tiling and (a), (b), (c) only."""
    import hip_helpers as H
    l = one_cu
    rng = L._rng(cin + cout * 7 + h + n)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cin, cout, 2, 2)) * np.sqrt(1.0 / cin)).astype(np.float32)
    b, bn = L._conv_params(rng, cout, cin)[1:]
    layout = getattr(H, fs) if fs else None
    with L._precision(H, precision):
        got = H.convt2x2(x, wt, b, bn, act, fs=layout)
        plan = last_plan(l)
        if tiling == (1, 1):
            print(plan)
            assert plan["grid"] > 0 and plan["items"] == 24
        else:
            assert_walk(plan, f"convt2x2 {tiling} precision {precision}")
        assert_tiling(plan, CONVT, tiling, precision)
        idx = _three(n)
        assert np.isfinite(got).all() and max_abs(got[idx], _convt_ref(x[idx], wt, b, bn, act)) < ATOL
        for i in range(n):
            assert np.array_equal(got[i:i + 1], H.convt2x2(x[i:i + 1], wt, b, bn, act, fs=layout)), i
        if precision == 0:
            with _variant(l, 0):
                assert np.array_equal(got, H.convt2x2(x, wt, b, bn, act, fs=layout))
                assert last_plan(l)["grid"] == 0
            with _default_plan(l):
                assert np.array_equal(got, H.convt2x2(x, wt, b, bn, act, fs=layout))


@pytest.mark.parametrize("n,h,w,cin,cout", [(29, 20, 16, 64, 32), (7, 35, 13, 128, 32)])
def test_convt2x2_and_conv1x1_bf16_walks(vad, one_cu, scratch, n, h, w, cin, cout):
    """convt2x2 on bf16 operands and bf16 tensors (2,2), and its data gradient = vad_conv1x1_p (K = 4 * cout -> cin: wide for
    cin 64 / 128), checked by the helper of tests/test_hip_train_bf16.py.  The pixel list of that data gradient is whatever the
    transposed convolution's shape leaves (580 and 100 items): its walk length is asserted here, unequal trip counts in
    test_conv1x1_p_walks."""
    seen = []

    def launched(what):
        plan = last_plan(one_cu)
        if what.startswith("convt2x2"):
            assert_walk(plan, what)
            assert_tiling(plan, CONVT, (2, 2), 3 if "tensors" in what else 2)
        else:
            print(f"{what}: {plan}")
            assert plan["grid"] > 0 and plan["items"] >= 3 * plan["walks"] + 1, plan
            assert_tiling(plan, CONV1X1, (2, 2))
        seen.append(what)

    B.check_convt2x2_on_bf16_tensors(vad, n, h, w, cin, cout, launched, ws=scratch)
    assert len(seen) == 3


@pytest.mark.parametrize("npix,cin,cout", [(29 * 80, 64, 32), (29 * 80, 64, 128), (6443, 32, 96), (6443, 32, 64)])
def test_conv1x1_p_walks(vad, one_cu, scratch, npix, cin, cout):
    """vad_conv1x1_p, narrow (32 / 96 columns: one N-tile per item) and wide, on pixel counts that are and are not a multiple of
    16 (6443 pixels: one ragged frame of 403 rows, 101 row tiles).  Each launch's tiling is read back: (2,2) where its
    output width is a multiple of 64 (forward: cout, data gradient: cin), else (2,1)."""
    seen = []

    def launched(what):
        plan = last_plan(one_cu)
        assert_walk(plan, what)
        width = cin if "gradient" in what else cout
        assert_tiling(plan, CONV1X1, (2, 2) if width % 64 == 0 else (2, 1))
        seen.append(what)

    B.check_conv1x1_on_bf16_tensors(vad, npix, cin, cout, launched, ws=scratch)
    assert len(seen) == 2


# ------------------------------------------------------------------------------------------------ scoring tail
@pytest.mark.parametrize("n,h,w", [(29, 16, 16), (29, 5, 72), (7, 33, 136)])
def test_dec4_score_walks(one_cu, n, h, w):
    """vad_dec4_score with vad_debug_set_dec4_band left at 0: the band height comes from the overridden plan.  Items are (frame,
    band, strip); the grid is the occupancy.  Oracle on three frames, every frame alone, the default plan and two forced band
    heights bit for bit."""
    import hip_helpers as H
    l = one_cu
    case = L._dec4_case(L._rng(n * 1000 + h * 10 + w), n, h, w)
    x_in, wt, bt, bn, w3, b3, frames = case
    recon, emap, scores = L._dec4_run(H, case, fused=True)
    plan = last_plan(l)
    print(plan)
    assert plan["family"] == DEC4 and plan["grid"] > 0
    assert plan["items"] >= 3 * plan["walks"] + 1, plan
    if n == 29:                 # (the third case has two strips per frame and one band: 14 items, a walk of equal lengths on an even grid)
        assert plan["items"] % plan["walks"] != 0, plan
    idx = _three(n)
    act = np.maximum(c_oracle.batchnorm_eval(c_oracle.convt2x2(x_in[idx], wt, bt), *bn), 0)
    ref_recon = np.tanh(c_oracle.conv2d(act, w3, b3, 3).astype(np.float64))
    ref_emap = ((frames[idx].astype(np.float64) - ref_recon) ** 2).mean(axis=1)
    ref_scores = ref_emap.mean(axis=(1, 2))
    assert np.isfinite(recon).all() and np.isfinite(emap).all() and np.isfinite(scores).all()
    assert max_abs(recon[idx], ref_recon) < ATOL and max_abs(emap[idx], ref_emap) < ATOL
    assert np.max(np.abs(scores[idx] - ref_scores) / ref_scores) < 1e-5
    for i in range(n):
        one = (x_in[i:i + 1], wt, bt, bn, w3, b3, frames[i:i + 1])
        r1, e1, s1 = L._dec4_run(H, one, fused=True)
        assert np.array_equal(recon[i:i + 1], r1) and np.array_equal(emap[i:i + 1], e1) and np.array_equal(scores[i:i + 1], s1), i
    with _default_plan(l):
        r0, e0, s0 = L._dec4_run(H, case, fused=True)
    assert np.array_equal(recon, r0) and np.array_equal(emap, e0) and np.array_equal(scores, s0)
    for band in (1, 3):
        rb, eb, sb = L._dec4_run(H, case, fused=True, band=band)
        assert np.array_equal(recon, rb) and np.array_equal(emap, eb) and np.array_equal(scores, sb), band


# ------------------------------------------------------------------------------------------------ Winograd
@pytest.mark.parametrize("cin,cout,h,w,act,pool,n", [(128, 128, 32, 32, 2, False, 9), (128, 256, 4, 4, 1, False, 7)])
def test_conv3x3_winograd_walks(one_cu, cin, cout, h, w, act, pool, n):
    """Two shapes of test_conv3x3_winograd: under the one-CU plan both take two N-tiles per wave and walk their frames."""
    import hip_helpers as H
    l = one_cu
    rng = L._rng(cin * 1000 + cout + h + 77)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt, b, bn = L._conv_params(rng, cout, cin)
    got = H.conv3x3_wino(x, wt, b, bn, act, pool)
    plan = last_plan(l)
    assert_walk(plan, "conv3x3_wino", n, multi=True)               # 16 / 4 positions per frame, more than the one CU holds
    assert plan["family"] == WINO and plan["nt"] == 2
    idx = _three(n)
    assert np.isfinite(got).all() and max_abs(got[idx], L._ref_conv(x[idx], wt, b, bn, act, pool)) < ATOL
    for i in range(n):
        assert np.array_equal(got[i:i + 1], H.conv3x3_wino(x[i:i + 1], wt, b, bn, act, pool)), i
    with _default_plan(l):
        assert np.array_equal(got, H.conv3x3_wino(x, wt, b, bn, act, pool))


@pytest.mark.parametrize("n,hid,h,w,zero_state", [(40, 128, 16, 16, False), (70, 64, 5, 7, False)])
def test_convlstm_step_winograd_walks(one_cu, n, hid, h, w, zero_state):
    """Two shapes of test_convlstm_step_winograd: the fused-cell form (mode 2), walked."""
    import hip_helpers as H
    l = one_cu
    x, hp, cp, wt, b = _lstm_inputs(L._rng(n + hid + h + 5), n, hid, hid, h, w, zero_state)
    gh, gc = H.convlstm_step_wino(x, hp, cp, wt, b)
    plan = last_plan(l)
    assert_walk(plan, "convlstm_step_wino", n, multi=True)         # 16 / 4 positions per frame: one frame group
    assert plan["family"] == WINO and plan["mode"] == 2
    idx = _three(n)
    rh, rc = c_oracle.convlstm_cell(x[idx], hp[idx], cp[idx], wt, b)
    assert np.isfinite(gh).all() and max_abs(gh[idx], rh) < LSTM_ATOL and max_abs(gc[idx], rc) < LSTM_ATOL
    for i in (0, 1, n // 2, n - 1):
        ah, ac = H.convlstm_step_wino(x[i:i + 1], hp[i:i + 1], cp[i:i + 1], wt, b)
        assert np.array_equal(gh[i:i + 1], ah) and np.array_equal(gc[i:i + 1], ac), i
    with _default_plan(l):
        dh, dc = H.convlstm_step_wino(x, hp, cp, wt, b)
    assert np.array_equal(gh, dh) and np.array_equal(gc, dc)


# ------------------------------------------------------------------------------------------------ statistics launches
# The un-activated, un-pooled launches of the training forward also write BatchNorm partial sums, one row per work-group (or
# wave), accumulated ACROSS the frames / items a work-group walks.  Each row holds, per channel, sum(y - bias) and sum((y - bias)^2).
BF16, BF16S = 2, 3


def _assert_partial_sums(H, st, nfloats, rows, y, bias, yerr=0.0):
    """The float64 sum of the `rows` partial rows against the float64 sums over the launch's own outputs y [.., cout] (fp32 values).
    Bound, from the number format alone: a sum of T fp32 terms in ANY order is within gamma(T) = T u / (1 - T u), u = 2^-24, of
    the exact sum relative to the sum of magnitudes; forming y - bias and its square adds 4 roundings (gamma(T + 4)).  yerr:
    relative error of y itself where only a rounded copy (bf16: 2^-9) of the values the kernel summed exists.  A frame summed
    twice or not at all moves the sums by 1 / n of the magnitudes: 3 % at n = 29, 14 % at n = 7."""
    cout = bias.numel()
    assert rows > 0 and rows * 2 * cout <= nfloats and H._guard_ok(st, nfloats)
    part = st[:rows * 2 * cout].view(rows, 2, cout)
    assert bool(torch.isfinite(part).all()), "a partial row was not written"
    assert bool(torch.isnan(st[rows * 2 * cout:nfloats]).all()), "rows behind the reported count were written"
    got = part.double().sum(0)
    yd = y.double().reshape(-1, cout)
    d = yd - bias.double()
    t = d.shape[0] + 4
    gamma = t * 2.0 ** -24 / (1 - t * 2.0 ** -24)
    tol1 = gamma * d.abs().sum(0) + yerr * yd.abs().sum(0)
    tol2 = gamma * (d * d).sum(0) + yerr * (2 * d.abs() * yd.abs() + yerr * yd * yd).sum(0)
    e1, e2 = (got[0] - d.sum(0)).abs(), (got[1] - (d * d).sum(0)).abs()
    print(f"partial sums: {rows} rows, worst error / bound {float((e1 / tol1).max()):.3f} (sums) {float((e2 / tol2).max()):.3f} (squares)")
    assert bool((e1 <= tol1).all()) and bool((e2 <= tol2).all())


def _stats_launch(l, H, kind, xin, wp, bo, out, n, h, w, cin, cout, precision):
    """One statistics launch (kind 0 conv3x3, 1 convt2x2) -> (guarded stats buffer, its size, rows, plan)."""
    nfloats = l.vad_debug_stats_floats(kind, cout, n, h, w)
    st, rows = H._guarded(nfloats, 256), C.c_int(-1)
    fn = l.vad_debug_convt2x2_stats if kind else l.vad_debug_conv3x3_stats
    H.hip.check(fn(xin.data_ptr(), 0, wp.data_ptr(), bo.data_ptr(), out.data_ptr(), 0, n, h, w, cin, cout, precision, st.data_ptr(), C.byref(rows),
                   H.stream()))
    plan = last_plan(l)
    torch.cuda.synchronize()
    return st, nfloats, rows.value, plan


def _packed(vad, l, H, kind, wt, b, precision, scratch):
    """Forward weights of a 3x3 (kind 0, wt OIHW) or transposed 2x2 (kind 1, wt IOHW) convolution for `precision`."""
    if precision < BF16:
        with L._precision(H, precision):
            return H.pack_convt(wt, b) if kind else H.pack_conv3x3(wt, b)
    wd = H.dev(wt)
    if kind:
        cin, cout = wt.shape[:2]
        fwd, dgr = scratch(l.vad_pack_convt2x2_floats(cin, cout)), scratch(l.vad_pack_conv1x1_floats(cin, 4 * cout))
        vad.hip.check(l.vad_train_pack_convt2x2(wd.data_ptr(), cin, cout, fwd.data_ptr(), dgr.data_ptr(), precision, H.stream()))
    else:
        cout, cin = wt.shape[:2]
        fwd, dgr = scratch(l.vad_pack_conv3x3_floats(cout, cin)), scratch(l.vad_pack_conv3x3_floats(cin, cout))
        vad.hip.check(l.vad_train_pack_conv3x3(wd.data_ptr(), cout, cin, fwd.data_ptr(), dgr.data_ptr(), precision, H.stream()))
    return fwd, H.dev(b)


@pytest.mark.parametrize("kind,cin,cout,h,w,n,precision,multi,tiling", [
    (0, 32, 128, 4, 16, 29, 0, False, (1, 2, 2, 2)), (0, 32, 64, 37, 21, 5, 0, True, (2, 2, 4, 1)), (0, 32, 32, 16, 16, 29, 0, False, (2, 1, 4, 1)),
    (0, 32, 128, 8, 16, 29, 1, False, (4, 1, 1, 4)), (0, 64, 64, 37, 21, 5, BF16, True, (2, 1, 2, 2)), (0, 32, 128, 8, 16, 29, BF16S, False, (4, 1, 1, 4)),
    (1, 64, 32, 20, 16, 29, 0, False, (2, 4)), (1, 64, 32, 20, 16, 29, 1, False, (2, 2)), (1, 128, 32, 35, 13, 7, BF16, False, (2, 2)),
    (1, 64, 32, 20, 16, 29, BF16S, False, (2, 2))])
def test_statistics_launches_walk(vad, one_cu, scratch, kind, cin, cout, h, w, n, precision, multi, tiling):
    """The statistics (ST = 1) instantiations of conv3x3_mfma_pkernel and convt2x2_pkernel, in every arithmetic the trainers use:
    the walk and the tiling from the read-back; the outputs bit-identical to the plain launch of the same data (fp32 and split:
    three frames against the oracle as well); the partial rows summed in float64 against the sums over the outputs (bf16 tensors:
    over the fp32 outputs of the bf16-operand launch, whose accumulators are the same); and the same sums under the default plan."""
    import hip_helpers as H
    l, rng = one_cu, L._rng(kind * 7 + cin + cout + h + n + precision)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    if kind:
        wt = (rng.standard_normal((cin, cout, 2, 2)) * np.sqrt(1.0 / cin)).astype(np.float32)
    else:
        wt = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    wp, bo = _packed(vad, l, H, kind, wt, b, precision, scratch)
    x32 = H.nhwc(x)
    if precision >= BF16:
        x32 = x32.to(torch.bfloat16).float()                           # bf16-representable inputs
    xin = x32.to(torch.bfloat16) if precision == BF16S else x32
    oshape = (n, 2 * h, 2 * w, cout) if kind else (n, h, w, cout)
    nan = lambda dt: torch.full(oshape, float("nan"), dtype=dt, device="cuda")
    out = nan(torch.bfloat16 if precision == BF16S else torch.float32)
    st, nfloats, rows, plan = _stats_launch(l, H, kind, xin, wp, bo, out, n, h, w, cin, cout, precision)
    assert_walk(plan, f"statistics launch, kind {kind}, precision {precision}", n, multi)
    assert_tiling(plan, CONVT if kind else CONV3, tiling, precision if kind else PLAIN)
    plain = torch.full_like(out, float("nan"))
    if kind:
        H.hip.check(l.vad_convt2x2(xin.data_ptr(), 0, wp.data_ptr(), bo.data_ptr(), plain.data_ptr(), 0, n, h, w, cin, cout, 0, precision, H.stream()))
    else:
        H.hip.check(l.vad_conv3x3(xin.data_ptr(), 0, wp.data_ptr(), bo.data_ptr(), plain.data_ptr(), 0, n, h, w, cin, cout, 0, 0, precision, H.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, plain)
    if precision < BF16:
        idx = _three(n)
        ref = c_oracle.convt2x2(x[idx], wt, b) if kind else L._ref_conv(x[idx], wt, b, None, 0, False)
        assert max_abs(H.to_nchw(out[idx]), ref) < ATOL
    y = out
    if precision == BF16S:                                             # the fp32 values behind the bf16 outputs
        y = nan(torch.float32)
        _stats_launch(l, H, kind, x32, wp, bo, y, n, h, w, cin, cout, BF16)
        assert torch.equal(out, y.to(torch.bfloat16))
    _assert_partial_sums(H, st, nfloats, rows, y, bo)
    with _default_plan(l):
        out0 = torch.full_like(out, float("nan"))
        st0, _, rows0, _ = _stats_launch(l, H, kind, xin, wp, bo, out0, n, h, w, cin, cout, precision)
    assert torch.equal(out0, out)
    _assert_partial_sums(H, st0, nfloats, rows0, y, bo)


@pytest.mark.parametrize("h,w,n,out16", [(16, 16, 29, 0), (70, 14, 9, 0), (16, 16, 29, 1), (16, 16, 29, 2)])
def test_first_layer_statistics_walk(vad, one_cu, h, w, n, out16):
    """conv3x3_c3_pkernel with the statistics epilogue (cout 32, un-pooled, un-activated): fp32 output, bf16 output (the sums are
    those of the fp32 launch's outputs) and bf16 operands as well (only the bf16-rounded outputs exist: yerr = 2^-9)."""
    import hip_helpers as H
    l, rng = one_cu, L._rng(h + n + out16)
    x = H.dev(rng.uniform(-1, 1, (n, 3, h, w)))
    if out16 == 2:
        x = x.to(torch.bfloat16).float()
    wp, bo = H.pack_conv3x3(rng.standard_normal((32, 3, 3, 3)).astype(np.float32) * 0.2, rng.standard_normal(32).astype(np.float32) * 0.1)
    nan = lambda dt: torch.full((n, h, w, 32), float("nan"), dtype=dt, device="cuda")
    out = nan(torch.bfloat16 if out16 else torch.float32)
    nfloats = l.vad_debug_stats_floats(2, 32, n, h, w)
    st, rows = H._guarded(nfloats, 256), C.c_int(-1)
    H.hip.check(l.vad_debug_conv3x3_c3_stats(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), out.data_ptr(), out16, n, h, w, st.data_ptr(), C.byref(rows),
                                             H.stream()))
    plan = last_plan(l)
    assert_walk(plan, f"first-layer statistics launch, out16 {out16}")
    assert_tiling(plan, C3, mode=PLAIN)
    assert rows.value == plan["grid"]
    plain = torch.full_like(out, float("nan"))
    if out16 == 0:
        H.hip.check(l.vad_conv3x3_c3(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), plain.data_ptr(), n, h, w, 32, 0, 0, H.stream()))
    else:
        fn = l.vad_conv3x3_c3_bf16 if out16 == 1 else l.vad_conv3x3_c3_bf16op
        H.hip.check(fn(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), plain.data_ptr(), n, h, w, 32, H.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and torch.equal(out, plain)
    y, yerr = out, 0.0
    if out16 == 1:
        y = nan(torch.float32)
        H.hip.check(l.vad_conv3x3_c3(x.data_ptr(), wp.data_ptr(), bo.data_ptr(), y.data_ptr(), n, h, w, 32, 0, 0, H.stream()))
        torch.cuda.synchronize()
        assert torch.equal(out, y.to(torch.bfloat16))
    elif out16 == 2:
        y, yerr = out.float(), 2.0 ** -9
    _assert_partial_sums(H, st, nfloats, rows.value, y, bo, yerr)


# ------------------------------------------------------------------------------------------------ training steps
@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_training_steps_hold_their_bounds_under_the_plan(vad, one_cu, precision):
    """The smallest cases of the decision-conditioned float64 gradient tests of the video and the image trainer, re-run under
    the one-CU plan with their own bounds (the grouping of the BatchNorm partial sums changes with the grid, so no bit equality
    with the default plan is asked).  One and two 16 x 16 frames: the plan changes the tilings and the grids here, but nothing
    walks - the walks of the statistics launches are the layer tests above."""
    import test_hip_train_img as TI
    import test_hip_train_step as TS
    TS.test_train_step_gradients_match_decision_conditioned_float64(vad, latent=32, layers=1, b=1, t=1, hw=16, wseed=50, precision=precision)
    TI.test_image_train_step_gradients_match_decision_conditioned_float64(vad, latent=32, n=2, hw=16, loss="mse", alpha=0.5, window=11, wseed=84,
                                                                          precision=precision)


@pytest.mark.parametrize("mode", ["bf16", "bf16_operands"])
def test_bf16_training_holds_its_bounds_under_the_plan(vad, one_cu, mode):
    """16 frames of 64 x 64 at the default model size: every layer of this step has more work than the one CU's slots."""
    import test_hip_train_step as TS
    TS.test_bf16_training_gradients_stay_close_to_fp32(vad, mode=mode)


# ------------------------------------------------------------------------------------------------ models end to end
def _u8_nhwc(vad, u8):
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(u8, -3, -1))).cuda()


@pytest.mark.parametrize("precision", ["fp32", "split", "winograd"])
def test_image_model_scores_do_not_depend_on_the_plan(vad, one_cu, precision):
    """ConvAutoencoder, b = 7 frames of 32 x 48, float and uint8: score_all under the one-CU plan == under the default plan, bit
    for bit (the fused first layer and the fused tail take their uint8 forms here)."""
    m = vad.ConvAutoencoder(in_channels=3, latent_dim=64)
    load_synthetic(vad, m, 91)
    m = m.cuda().eval()
    m.precision = precision
    u8 = vad.synth.frames_u8(92, 0, 7, 3, 32, 48, anomalies=True)
    xs = (torch.from_numpy(vad.synth.u8_to_unit(u8)).cuda(), _u8_nhwc(vad, u8))
    with torch.no_grad():
        one = []
        for fmt, x in enumerate(xs):                                   # 0 = float NCHW, 1 = uint8 NHWC
            one.append(m.score_all(x))
            plan = last_plan(one_cu, persistent=True)                  # a call's last persistent launch: the fused tail
            print(f"dec4 tail, format {fmt}: {plan}")
            assert plan["family"] == DEC4 and plan["mode"] == fmt and plan["grid"] > 0, plan
            assert plan["items"] >= 3 * plan["walks"] + 1, plan
        with _default_plan(one_cu):
            dflt = [m.score_all(x) for x in xs]
    for a, b in zip(one, dflt):
        for k in ("scores", "errmap", "recon"):
            assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k
    for k in ("scores", "errmap", "recon"):
        assert torch.equal(one[0][k], one[1][k]), k                # uint8 ingest == normalised float frames, under the walk too


@pytest.mark.parametrize("precision,hid", [("fp32", 128), ("split", 64), ("winograd", 128)])
def test_video_model_scores_do_not_depend_on_the_plan(vad, one_cu, precision, hid):
    """VideoAutoencoder with lstm_hidden_dim != latent_dim (layer 0's two sources differ in width and the projection runs), 2
    layers, b = 3, t = 4.  The split-fp16 ConvLSTM step refuses unequal widths under any plan (test_convlstm_step_oracle pins
    the refusal), so the split model has lstm_hidden_dim == latent_dim."""
    m = vad.VideoAutoencoder(in_channels=3, latent_dim=64, lstm_hidden_dim=hid, lstm_num_layers=2)
    load_synthetic(vad, m, 93)
    m = m.cuda().eval()
    m.precision = precision
    x = torch.from_numpy(vad.synth.clips(94, 0, 3, 4, 3, 32, 48)).cuda()
    with torch.no_grad():
        one = m.score_all(x)
        with _default_plan(one_cu):
            dflt = m.score_all(x)
    for k in ("seq", "frame", "errmap", "recon"):
        assert torch.isfinite(one[k]).all() and torch.equal(one[k], dflt[k]), k
